"""Kernel-level tests of the small operators between the convolution families and the model: every entry point of
include/vlfb.h that the model tests reach only through vlfb.engine at one shape, and every dispatch branch of
csrc/vlfb_ops.hip / csrc/vlfb_pool.hip / csrc/vlfb_head.hip that only other shapes select.

Calls go through libvlfb_hip.so (ctypes).  Inputs are rounded through the storage type first; every reference is plain
torch-CPU in fp64 or a bit-exact restatement, none calls the library.  Bit-identity checks between two entry points of the
library come on top of an independent reference.

Bars: where tests/gpu_util.py / tests/test_kernels_gpu.py hold one for the operator and output type it is used unchanged;
results that are determined bit for bit are compared with torch.equal; everything else (softmax_ce, the sigmoid_ce edges, the
softmax row sums) gets its bar at run time from the reference side alone -- derived_bar(): the same formula in plain fp32
torch-CPU against fp64 on that very input, times 8 (the kernel's other summation order, __expf / expf at a few ulp where
torch's exp is below one), floor 1e-6.  Every such case prints its measured error beside the bar.
"""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_util import DTYPES, TOL, dev, q, rel_err, to_ncthw, to_nthwc

pytestmark = pytest.mark.gpu

hip = None


def setup_module(module):
    from vlfb import hip as h
    module.hip = h
    h.lib()


_KEEP = []


def gpu(t, dtype=None):
    t = t.to(dev())
    return t.to(dtype) if dtype is not None else t


def gp(t, dtype=None):
    """device copy of `t` kept alive until the end of the test; returns its device pointer"""
    g = gpu(t, dtype)
    _KEEP.append(g)
    return g.data_ptr()


@pytest.fixture(autouse=True)
def _release_kept_tensors():
    yield
    torch.cuda.synchronize()
    del _KEEP[:]


def derived_bar(ref32, ref64):
    """8 x the error of the plain-fp32 evaluation of the reference formula against its fp64 evaluation, floor 1e-6"""
    return max(8.0 * rel_err(ref32, ref64), 1e-6)


def scalar_err(got, ref):
    got, ref = float(got), float(ref)
    return abs(got - ref) / (abs(ref) if ref != 0 else 1.0)


def report(what, err, bar):
    print("\n[%s] err %.3e  bar %.3e" % (what, err, bar))


def rejected(name, *args, match=None):
    """the call must come back with an error code and a message"""
    with pytest.raises(hip.VlfbError, match=match) as e:
        hip.call(name, *args)
    assert str(e.value).split(":", 1)[1].strip(), "no message behind the error code"


def sentinel(shape, dtype, value=-77.0):
    return torch.full(shape, value, device=dev(), dtype=dtype)


# ------------------------------------------------------------------------------------------------
# softmax: rowreg<4> (cols % 4 == 0, cols <= 1024), rowreg<8> (cols <= 2048), the generic strided kernel
# ------------------------------------------------------------------------------------------------
SOFTMAX_COLS = [4, 252, 784, 1024, 1028, 1568, 2048, 2052, 3136, 1023, 37]
SOFTMAX_ROWS = [1, 5, 37]            # (4 waves per block: 1 and 5 and 37 leave waves of the last block without a row)
SOFTMAX_SCALE = 512 ** -0.5


def softmax_scores(rows, cols, gen):
    s = torch.randn(rows, cols, generator=gen) * 8
    r = rows // 2
    s[r, (7 * cols) // 11] = 60.0 / SOFTMAX_SCALE          # one row with a single dominant entry
    return s


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols", SOFTMAX_COLS)
def test_softmax_fwd_bwd_every_dispatch_branch(cols, dtype):
    code = hip.dtype_code(dtype)
    scale = SOFTMAX_SCALE
    for rows in SOFTMAX_ROWS:
        gen = torch.Generator().manual_seed(1000 * rows + cols)
        s = softmax_scores(rows, cols, gen)
        P = sentinel((rows + 1, cols), dtype)
        hip.call("vlfb_softmax_fwd", gp(s), hip.ptr(P), code, rows, cols, scale)
        p_ref = torch.softmax(s.double() * scale, dim=1)
        got = P[:rows].float().cpu()
        assert torch.isfinite(got).all()
        assert float(P[rows].float().min()) == -77.0 and float(P[rows].float().max()) == -77.0, "wrote past the last row"
        assert rel_err(got, p_ref) < (1e-5 if dtype == torch.float32 else 4e-3), (rows, cols)
        if dtype == torch.float32:
            p32 = torch.softmax(s * torch.tensor(scale), dim=1)
            bar = max(8.0 * float((p32.double().sum(1) - 1).abs().max()), 1e-6)
            err = float((got.double().sum(1) - 1).abs().max())
            report("softmax row sums rows=%d cols=%d" % (rows, cols), err, bar)
            assert err < bar
        # backward on the stored (rounded) probabilities, as the engine runs it
        dp = torch.randn(rows, cols, generator=gen)
        pq = got.double()
        ds_ref = scale * pq * (dp.double() - (dp.double() * pq).sum(1, keepdim=True))
        DS = sentinel((rows + 1, cols), dtype)
        hip.call("vlfb_softmax_bwd", gp(dp), hip.ptr(P), hip.ptr(DS), code, rows, cols, scale)
        assert float(DS[rows].float().min()) == -77.0 and float(DS[rows].float().max()) == -77.0
        assert rel_err(DS[:rows].float(), ds_ref) < TOL[dtype], (rows, cols)


P32_COLS = [c for c in SOFTMAX_COLS if c % 4 == 0 and c <= 2048]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cols", P32_COLS)
def test_softmax_bwd_p32(cols, dtype):
    """fp32 probabilities in, 16-bit ds out.  Against fp64; and against vlfb_softmax_bwd on the ROUNDED probabilities, which
    must be no more accurate.  That comparison is one between two error norms that differ by an independent rounding of P
    (a statement in expectation), so it is asserted over the 43 rows of the three row counts together."""
    code = hip.dtype_code(dtype)
    scale = SOFTMAX_SCALE
    got_p32, got_rnd, refs = [], [], []
    for rows in SOFTMAX_ROWS:
        gen = torch.Generator().manual_seed(2000 * rows + cols)
        s = softmax_scores(rows, cols, gen)
        p = torch.softmax(s.double() * scale, dim=1).float()
        dp = torch.randn(rows, cols, generator=gen)
        ds_ref = scale * p.double() * (dp.double() - (dp.double() * p.double()).sum(1, keepdim=True))
        DS = sentinel((rows + 1, cols), dtype)
        hip.call("vlfb_softmax_bwd_p32", gp(dp), gp(p), hip.ptr(DS), code, rows, cols, scale)
        assert float(DS[rows].float().min()) == -77.0 and float(DS[rows].float().max()) == -77.0
        assert torch.isfinite(DS[:rows].float()).all()
        # (the row with the dominant entry is all but one-hot: its ds ~ 1e-28 lies below the fp16 format, whose subnormal
        # quantum 2^-24 bounds the rounding of an element by 2^-25 absolutely -- the bar is TOL relative plus that)
        diff = (DS[:rows].double().cpu() - ds_ref).norm().item()
        floor = math.sqrt(rows * cols) * 2.0 ** -25 if dtype == torch.float16 else 0.0
        assert diff <= TOL[dtype] * ds_ref.norm().item() + floor, (rows, cols)
        D2 = torch.empty(rows, cols, device=dev(), dtype=dtype)
        hip.call("vlfb_softmax_bwd", gp(dp), gp(p, dtype), hip.ptr(D2), code, rows, cols, scale)
        got_p32.append(DS[:rows].float().cpu())
        got_rnd.append(D2.float().cpu())
        refs.append(ds_ref)
    e32, ernd = rel_err(torch.cat(got_p32), torch.cat(refs)), rel_err(torch.cat(got_rnd), torch.cat(refs))
    print("\n[softmax_bwd_p32 %s cols=%d] p32 %.3e  rounded-P %.3e" % (dtype, cols, e32, ernd))
    assert e32 <= ernd


def test_softmax_bwd_p32_rejections_launch_nothing():
    rows = 3
    for cols, code in ((1023, hip.F16), (37, hip.BF16), (2052, hip.F16), (3136, hip.BF16), (784, hip.F32)):
        dp = torch.randn(rows, cols)
        p = torch.softmax(torch.randn(rows, cols), dim=1)
        DS = sentinel((rows, cols), torch.float32)       # (large enough for any ds type)
        rejected("vlfb_softmax_bwd_p32", gp(dp), gp(p), hip.ptr(DS), code, rows, cols, 1.0, match="softmax_bwd_p32")
        torch.cuda.synchronize()
        assert float(DS.min()) == -77.0 and float(DS.max()) == -77.0


# ------------------------------------------------------------------------------------------------
# vlfb_softmax_ce: prob = softmax, loss = scale * mean_r -log prob[r][label_r], dlogits = scale * (prob - onehot) / rows
# ------------------------------------------------------------------------------------------------
def softmax_ce_ref(x, labels, scale, dt):
    x = x.to(dt)
    prob = torch.softmax(x, dim=1)
    loss = torch.tensor(scale, dtype=dt) * F.nll_loss(F.log_softmax(x, dim=1), labels.long(), reduction="mean")
    onehot = F.one_hot(labels.long(), x.shape[1]).to(dt)
    dl = torch.tensor(scale, dtype=dt) * (prob - onehot) / x.shape[0]
    return prob, loss, dl


def run_softmax_ce(x, labels, scale):
    rows, cols = x.shape
    prob, dl = sentinel((rows + 1, cols), torch.float32), sentinel((rows + 1, cols), torch.float32)
    loss = sentinel((2,), torch.float32)
    hip.call("vlfb_softmax_ce", gp(x), gp(labels), hip.ptr(prob), hip.ptr(loss), hip.ptr(dl), rows, cols, scale)
    torch.cuda.synchronize()
    for t in (prob[rows], dl[rows], loss[1:]):
        assert float(t.min()) == -77.0 and float(t.max()) == -77.0, "wrote outside its output"
    return prob[:rows].cpu(), loss[0].cpu(), dl[:rows].cpu()


SOFTMAX_CE_SHAPES = [(1, 125), (5, 352), (8, 125), (3, 64), (4, 1), (6, 1000)]


@pytest.mark.parametrize("rows,cols", SOFTMAX_CE_SHAPES)
def test_softmax_ce_against_fp64(rows, cols):
    gen = torch.Generator().manual_seed(100 * rows + cols)
    x = torch.randn(rows, cols, generator=gen) * 4
    labels = torch.randint(0, cols, (rows,), generator=gen, dtype=torch.int32)
    scale = 0.5
    prob, loss, dl = run_softmax_ce(x, labels, scale)
    p64, l64, d64 = softmax_ce_ref(x, labels, scale, torch.float64)
    p32, l32, d32 = softmax_ce_ref(x, labels, scale, torch.float32)
    assert torch.isfinite(prob).all() and torch.isfinite(dl).all() and math.isfinite(float(loss))
    for what, got, r32, r64 in (("prob", prob, p32, p64), ("dlogits", dl, d32, d64)):
        err, bar = rel_err(got, r64), derived_bar(r32, r64)
        report("softmax_ce %s %dx%d" % (what, rows, cols), err, bar)
        assert err < bar, what
    err, bar = scalar_err(loss, l64), max(8.0 * scalar_err(l32, l64), 1e-6)
    report("softmax_ce loss %dx%d" % (rows, cols), err, bar)
    assert err < bar


def test_softmax_ce_is_shift_invariant():
    """a row offset by +80 gives the row without the offset.  The logits are multiples of 2^-12 below 32 in magnitude, so
    x + 80 is exact in fp32 and every x[c] - max of the two rows is the same number: the results must be IDENTICAL."""
    rows, cols, scale = 5, 352, 1.0
    gen = torch.Generator().manual_seed(7)
    x = torch.round(torch.clamp(torch.randn(rows, cols, generator=gen) * 4, -31, 31) * 4096) / 4096
    labels = torch.randint(0, cols, (rows,), generator=gen, dtype=torch.int32)
    xo = x.clone()
    xo[2] += 80.0
    assert torch.equal(xo[2] - 80.0, x[2])
    p0, l0, d0 = run_softmax_ce(x, labels, scale)
    p1, l1, d1 = run_softmax_ce(xo, labels, scale)
    assert torch.equal(p0, p1) and torch.equal(d0, d1) and torch.equal(l0, l1)
    p64, l64, d64 = softmax_ce_ref(xo, labels, scale, torch.float64)
    p32, l32, d32 = softmax_ce_ref(xo, labels, scale, torch.float32)
    for what, got, r32, r64 in (("prob", p1, p32, p64), ("dlogits", d1, d32, d64)):
        err, bar = rel_err(got, r64), derived_bar(r32, r64)
        report("softmax_ce +80 %s" % what, err, bar)
        assert err < bar
    err, bar = scalar_err(l1, l64), max(8.0 * scalar_err(l32, l64), 1e-6)
    report("softmax_ce +80 loss", err, bar)
    assert err < bar


@pytest.mark.parametrize("bad", ["cols", "minus_one"])
def test_softmax_ce_poisons_the_loss_on_a_label_out_of_range(bad):
    rows, cols = 5, 125
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(rows, cols, generator=gen) * 4
    labels = torch.randint(0, cols, (rows,), generator=gen, dtype=torch.int32)
    labels[3] = cols if bad == "cols" else -1
    prob, loss, dl = run_softmax_ce(x, labels, 1.0)
    assert math.isnan(float(loss))
    p64, p32 = torch.softmax(x.double(), dim=1), torch.softmax(x, dim=1)
    err, bar = rel_err(prob, p64), derived_bar(p32, p64)
    report("softmax_ce prob beside a bad label (%s)" % bad, err, bar)
    assert err < bar


def test_softmax_ce_test_mode_and_its_rejection():
    rows, cols = 6, 352
    gen = torch.Generator().manual_seed(13)
    x = torch.randn(rows, cols, generator=gen) * 4
    prob = sentinel((rows + 1, cols), torch.float32)
    hip.call("vlfb_softmax_ce", gp(x), None, hip.ptr(prob), None, None, rows, cols, 1.0)
    p64, p32 = torch.softmax(x.double(), dim=1), torch.softmax(x, dim=1)
    err, bar = rel_err(prob[:rows], p64), derived_bar(p32, p64)
    report("softmax_ce probabilities only", err, bar)
    assert err < bar and float(prob[rows].min()) == -77.0 and float(prob[rows].max()) == -77.0
    loss = sentinel((1,), torch.float32)
    prob2 = sentinel((rows, cols), torch.float32)
    rejected("vlfb_softmax_ce", gp(x), None, hip.ptr(prob2), hip.ptr(loss), None, rows, cols, 1.0, match="need labels")
    torch.cuda.synchronize()
    assert float(loss) == -77.0 and float(prob2.max()) == -77.0 and float(prob2.min()) == -77.0


# ------------------------------------------------------------------------------------------------
# vlfb_sigmoid_ce edges
# ------------------------------------------------------------------------------------------------
def sigmoid_ce_ref(x, labels, scale, dt):
    """the formula of test_fc_and_sigmoid_ce (vlfb.h), evaluated in `dt`"""
    x = x.to(dt)
    t = labels.to(dt)
    valid = (labels >= 0).to(dt)
    pos = (x >= 0).to(dt)
    l = -x * (t - pos) + torch.log(1 + torch.exp(x - 2 * x * pos))
    norm = torch.clamp(valid.sum(), min=1e-5)
    sc = torch.tensor(scale, dtype=dt)
    loss = sc * (l * valid).sum() / norm
    prob = torch.sigmoid(x)
    dl = sc * (prob - t) / norm * valid
    return prob, loss, dl


def test_sigmoid_ce_with_every_label_ignored_is_exactly_zero():
    rows, cols = 6, 157
    gen = torch.Generator().manual_seed(17)
    x = torch.randn(rows, cols, generator=gen) * 3
    labels = torch.full((rows, cols), -1, dtype=torch.int32)
    prob, dl = sentinel((rows, cols), torch.float32), sentinel((rows, cols), torch.float32)
    loss = sentinel((1,), torch.float32)
    hip.call("vlfb_sigmoid_ce", gp(x), gp(labels), hip.ptr(prob), hip.ptr(loss), hip.ptr(dl), rows, cols, 0.125)
    assert float(loss) == 0.0
    assert torch.equal(dl.cpu(), torch.zeros(rows, cols))
    p64, _, _ = sigmoid_ce_ref(x, labels, 0.125, torch.float64)
    p32, _, _ = sigmoid_ce_ref(x, labels, 0.125, torch.float32)
    err, bar = rel_err(prob, p64), derived_bar(p32, p64)
    report("sigmoid_ce prob, all ignored", err, bar)
    assert err < bar


def test_sigmoid_ce_probabilities_only():
    rows, cols = 5, 157
    gen = torch.Generator().manual_seed(19)
    x = torch.randn(rows, cols, generator=gen) * 3
    prob = sentinel((rows + 1, cols), torch.float32)
    hip.call("vlfb_sigmoid_ce", gp(x), None, hip.ptr(prob), None, None, rows, cols, 1.0)
    p64, p32 = torch.sigmoid(x.double()), torch.sigmoid(x)
    err, bar = rel_err(prob[:rows], p64), derived_bar(p32, p64)
    report("sigmoid_ce probabilities only", err, bar)
    assert err < bar and float(prob[rows].min()) == -77.0 and float(prob[rows].max()) == -77.0
    loss = sentinel((1,), torch.float32)
    rejected("vlfb_sigmoid_ce", gp(x), None, hip.ptr(prob), hip.ptr(loss), None, rows, cols, 1.0, match="need labels")
    torch.cuda.synchronize()
    assert float(loss) == -77.0


def test_sigmoid_ce_logits_of_large_magnitude():
    rows, cols = 6, 157
    gen = torch.Generator().manual_seed(23)
    x = torch.randn(rows, cols, generator=gen) * 2
    labels = (torch.rand(rows, cols, generator=gen) < 0.3).to(torch.int32)
    # every extreme value once with label 0, once with label 1, once ignored
    for j, v in enumerate((-100.0, -20.0, 0.0, 20.0, 100.0)):
        for i, t in enumerate((0, 1, -1)):
            x[i, 10 * j + 3] = v
            labels[i, 10 * j + 3] = t
    scale = 0.25
    prob, dl = sentinel((rows, cols), torch.float32), sentinel((rows, cols), torch.float32)
    loss = sentinel((1,), torch.float32)
    hip.call("vlfb_sigmoid_ce", gp(x), gp(labels), hip.ptr(prob), hip.ptr(loss), hip.ptr(dl), rows, cols, scale)
    prob, dl, loss = prob.cpu(), dl.cpu(), loss.cpu()
    assert torch.isfinite(prob).all() and torch.isfinite(dl).all() and torch.isfinite(loss).all()
    p64, l64, d64 = sigmoid_ce_ref(x, labels, scale, torch.float64)
    p32, l32, d32 = sigmoid_ce_ref(x, labels, scale, torch.float32)
    for what, got, r32, r64 in (("prob", prob, p32, p64), ("dlogits", dl, d32, d64)):
        err, bar = rel_err(got, r64), derived_bar(r32, r64)
        report("sigmoid_ce extremes %s" % what, err, bar)
        assert err < bar
    err, bar = scalar_err(loss, l64), max(8.0 * scalar_err(l32, l64), 1e-6)
    report("sigmoid_ce extremes loss", err, bar)
    assert err < bar
    assert torch.equal(dl[labels < 0], torch.zeros(int((labels < 0).sum())))


# ------------------------------------------------------------------------------------------------
# vlfb_relu_fwd / vlfb_relu_bwd / vlfb_add with b == NULL: vector body + scalar tail of the 4- and the 8-wide vector
# ------------------------------------------------------------------------------------------------
RELU_N = [1, 7, 8, 9, 8003, 65536 + 5]


def relu_input(n, gen, dtype):
    x = q(torch.randn(n, generator=gen), dtype)
    x[::5] = 0.0
    x[2::7] = -0.0
    return x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", RELU_N)
def test_relu_fwd_bwd_and_add_without_second_operand(n, dtype):
    """exact against torch.relu / torch.where on the rounded inputs (equality of VALUES: the sign of a zero result is not
    pinned, IEEE maxNum leaves max(-0, +0) open)"""
    code = hip.dtype_code(dtype)
    gen = torch.Generator().manual_seed(n)
    x = relu_input(n, gen, dtype)
    dy = relu_input(n, gen, dtype)
    X = gpu(x, dtype)
    Y = sentinel((n + 8,), dtype)
    hip.call("vlfb_relu_fwd", hip.ptr(X), hip.ptr(Y), code, n)
    assert torch.equal(Y[:n].float().cpu(), torch.relu(x))
    assert float(Y[n:].float().min()) == -77.0 and float(Y[n:].float().max()) == -77.0
    DX = sentinel((n + 8,), dtype)
    hip.call("vlfb_relu_bwd", gp(dy, dtype), hip.ptr(Y), hip.ptr(DX), code, n)
    y = torch.relu(x)
    assert torch.equal(DX[:n].float().cpu(), torch.where(y > 0, dy, torch.zeros_like(dy)))
    assert float(DX[n:].float().min()) == -77.0 and float(DX[n:].float().max()) == -77.0
    # in place, as the engine runs both
    XI = torch.cat([gpu(x, dtype), sentinel((8,), dtype)])
    hip.call("vlfb_relu_fwd", hip.ptr(XI), hip.ptr(XI), code, n)
    assert torch.equal(XI.cpu(), Y.cpu())
    G = torch.cat([gpu(dy, dtype), sentinel((8,), dtype)])
    hip.call("vlfb_relu_bwd", hip.ptr(G), hip.ptr(XI), hip.ptr(G), code, n)
    assert torch.equal(G.cpu(), DX.cpu())
    # vlfb_add itself with b == NULL: copy / ReLU / mask
    m = relu_input(n, gen, dtype)
    for relu, mask in ((0, None), (1, None), (0, m), (1, m)):
        O = sentinel((n + 8,), dtype)
        hip.call("vlfb_add", hip.ptr(X), None, hip.ptr(O), None if mask is None else gp(mask, dtype), code, n, relu)
        ref = torch.relu(x) if relu else x
        if mask is not None:
            ref = torch.where(mask > 0, ref, torch.zeros_like(ref))
        assert torch.equal(O[:n].float().cpu(), ref), (relu, mask is not None)
        assert float(O[n:].float().min()) == -77.0 and float(O[n:].float().max()) == -77.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_add_and_relu_of_nothing_are_no_ops(dtype):
    """n == 0 is accepted by vlfb_add / vlfb_relu_* (vlfb.h) and writes nothing"""
    code = hip.dtype_code(dtype)
    X, Y = sentinel((8,), dtype, 3.0), sentinel((8,), dtype)
    hip.call("vlfb_add", hip.ptr(X), hip.ptr(X), hip.ptr(Y), None, code, 0, 1)
    hip.call("vlfb_relu_fwd", hip.ptr(X), hip.ptr(Y), code, 0)
    hip.call("vlfb_relu_bwd", hip.ptr(X), hip.ptr(X), hip.ptr(Y), code, 0)
    assert float(Y.float().min()) == -77.0 and float(Y.float().max()) == -77.0


# ------------------------------------------------------------------------------------------------
# vlfb_copy2d: the head's Concat and its backward
# ------------------------------------------------------------------------------------------------
COPY2D = [  # rows, cols, lds, ldd, destination column offset
    (6, 512, 512, 2560, 2048),      # Concat of the FBO output behind the RoI feature
    (5, 37, 64, 101, 3),            # odd cols, both strides wider, offset not 16-byte aligned for any type
    (1, 9, 9, 9, 0),                # one dense row
    (1, 5, 16, 32, 7),
    (33, 64, 200, 64, 0),           # the backward: a slice of a wide gradient into a dense tensor
    (7, 1, 3, 5, 1),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", COPY2D)
def test_copy2d(case, dtype):
    rows, cols, lds, ldd, off = case
    code = hip.dtype_code(dtype)
    es = torch.empty(0, dtype=dtype).element_size()
    gen = torch.Generator().manual_seed(rows * 1000 + cols)
    src = q(torch.randn(rows, lds, generator=gen), dtype)
    ldd_full = ldd + off
    dst = sentinel((rows + 1, ldd_full), dtype)
    hip.call("vlfb_copy2d", gp(src, dtype), lds, dst.data_ptr() + off * es, ldd_full, code, rows, cols)
    want = torch.full((rows + 1, ldd_full), -77.0)
    want[:rows, off:off + cols] = src[:, :cols]
    assert torch.equal(dst.float().cpu(), want)


# ------------------------------------------------------------------------------------------------
# vlfb_zero_f32, vlfb_scale_inplace, vlfb_store_scalars
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 7, 1001, 65536 + 3])
def test_zero_f32(n):
    x = sentinel((n + 5,), torch.float32)
    hip.call("vlfb_zero_f32", hip.ptr(x), n)
    want = torch.full((n + 5,), -77.0)
    want[:n] = 0.0
    assert torch.equal(x.cpu(), want)


@pytest.mark.parametrize("n", [1, 7, 1001, 65536 + 3])
def test_scale_inplace(n):
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=gen)
    s = float(torch.tensor(1.0 / 1024 * 3.3))          # (an fp32 value, as the C float argument carries it)
    X = torch.cat([gpu(x), sentinel((5,), torch.float32)])
    hip.call("vlfb_scale_inplace", hip.ptr(X), n, s)
    assert torch.equal(X[:n].cpu(), x * torch.tensor(s)) and float(X[n:].min()) == -77.0 and float(X[n:].max()) == -77.0
    rejected("vlfb_scale_inplace", hip.ptr(X), 0, s, match="scale_inplace")


def test_store_scalars():
    vals = [0xFEDCBA9876543210, 0x8000000000000001, 0xFFFFFFFFFFFFFFFF, 1, 0x3F80000000000000, 0x123456789ABCDEF0,
            0xDEADBEEFCAFEF00D, 0x00000000FFFFFFFF]
    for n in (1, 3, 8):
        arr = (C.c_uint64 * 8)(*vals)
        dst = torch.full((10,), -5, device=dev(), dtype=torch.int64)
        hip.call("vlfb_store_scalars", hip.ptr(dst), n, C.cast(arr, C.c_void_p))
        for i in range(8):
            arr[i] = 0                      # (the values travel in the launch packet: the host copy is free at once)
        got = dst.cpu().numpy().view(np.uint64)
        assert got[:n].tolist() == vals[:n]
        assert dst.cpu()[n:].tolist() == [-5] * (10 - n)
    arr = (C.c_uint64 * 9)(*([7] * 9))
    dst = torch.full((10,), -5, device=dev(), dtype=torch.int64)
    for n in (0, 9):
        rejected("vlfb_store_scalars", hip.ptr(dst), n, C.cast(arr, C.c_void_p), match="store_scalars")
    torch.cuda.synchronize()
    assert dst.cpu().tolist() == [-5] * 10


# ------------------------------------------------------------------------------------------------
# the device-scalar twins of the captured step
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 10007])
@pytest.mark.parametrize("nesterov", [0, 1])
@pytest.mark.parametrize("wd", [1e-4, 0.0])
def test_sgd_update_dev_and_sgd_update(wd, nesterov, n):
    gen = torch.Generator().manual_seed(37 + n)
    p, g, m = (torch.randn(n, generator=gen) for _ in range(3))
    lr, mu = 0.02, 0.9
    lr32, wd32, mu32 = (float(torch.tensor(v)) for v in (lr, wd, mu))      # what the float arguments carry
    g2 = g.double() + wd32 * p.double()
    m2 = mu32 * m.double() + lr32 * g2
    step = (1 + mu32) * m2 - mu32 * m.double() if nesterov else m2
    outs = []
    for devscalar in (False, True):
        P, G, M = gpu(p.clone()), gpu(g.clone()), gpu(m.clone())
        if devscalar:
            hip.call("vlfb_sgd_update_dev", hip.ptr(P), hip.ptr(G), hip.ptr(M), n, gp(torch.tensor([lr])), wd, mu, nesterov)
        else:
            hip.call("vlfb_sgd_update", hip.ptr(P), hip.ptr(G), hip.ptr(M), n, lr, wd, mu, nesterov)
        assert rel_err(P, p.double() - step) < 1e-6 and rel_err(M, m2) < 1e-6 and rel_err(G, step) < 1e-6, devscalar
        outs.append((P.cpu(), G.cpu(), M.cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b), "the scalar and the device-scalar entry point share one kernel"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ratio", [0.0, 0.2, 0.5])
def test_dropout_fwd_dev_and_dropout_fwd(ratio, dtype):
    from oracle import rng as orng
    code = hip.dtype_code(dtype)
    R, K, Cc = 3, 5, 17                                       # 255 elements: the last block is partial
    gen = torch.Generator().manual_seed(43)
    xs = q(torch.randn(R, K, Cc, generator=gen), dtype)       # stored [(r*K + k)*C + c]
    for seed in (0x1234567890ABCDEF, 0xF00DFACE00000001):     # (the second one has its top bit set)
        seed_dev = torch.from_numpy(np.array([seed], dtype=np.uint64).view(np.int64)).to(dev())
        res = []
        for devseed in (False, True):
            Y = sentinel((R * K * Cc + 3,), dtype)
            Mk = torch.full((R * K * Cc + 3,), 9, device=dev(), dtype=torch.uint8)
            if devseed:
                hip.call("vlfb_dropout_fwd_dev", gp(xs, dtype), hip.ptr(Y), hip.ptr(Mk), code, R, K, Cc, ratio, hip.ptr(seed_dev))
            else:
                hip.call("vlfb_dropout_fwd", gp(xs, dtype), hip.ptr(Y), hip.ptr(Mk), code, R, K, Cc, ratio, seed)
            res.append((Y.cpu(), Mk.cpu()))
        (y0, m0), (y1, m1) = res
        assert torch.equal(y0, y1) and torch.equal(m0, m1)
        n = R * K * Cc
        assert m0[n:].tolist() == [9, 9, 9] and float(y0[n:].float().min()) == -77.0 and float(y0[n:].float().max()) == -77.0
        keep = torch.from_numpy(orng.dropout_keep_mask(seed, (R, Cc, K), ratio)).permute(0, 2, 1)    # reference layout (R, C, K)
        assert torch.equal(m0[:n].view(R, K, Cc).bool(), keep)
        got = y0[:n].view(R, K, Cc).float()
        if ratio == 0.0:
            assert keep.all() and torch.equal(got, xs)
        else:
            assert not keep.all() and keep.any()
            # y = x * (1 / (1 - ratio)) in fp32, rounded once to the storage type
            ref = torch.where(keep, xs * (torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(ratio))), torch.zeros_like(xs))
            assert torch.equal(got, q(ref, dtype))


# ------------------------------------------------------------------------------------------------
# vlfb_weight_prep_batched
# ------------------------------------------------------------------------------------------------
WPREP_ITEMS = [  # cout, taps, cin, with scale, with the DGRAD copy
    (40, 3, 72, True, True),
    (157, 1, 2560, False, True),        # the classifier-like wide row, no frozen scale
    (64, 9, 4, True, True),             # 4 input channels: one ragged cin tile
    (33, 1, 31, True, False),           # no DGRAD copy; one element past a tile in both directions
    (96, 9, 40, True, True),
    (128, 3, 64, True, True),           # whole tiles only
]


def wprep_tiles(cout, taps, cin):
    return taps * ((cout + 31) // 32) * ((cin + 31) // 32)


def items_to_device(items):
    arr = (hip.WPrepItem * len(items))(*items)
    t = torch.frombuffer(bytearray(bytes(memoryview(arr))), dtype=torch.uint8).to(dev())
    _KEEP.append(t)
    return t


@pytest.mark.parametrize("dtype", DTYPES)
def test_weight_prep_batched(dtype):
    code = hip.dtype_code(dtype)
    es = torch.empty(0, dtype=dtype).element_size()
    gen = torch.Generator().manual_seed(47)
    GAP = 24                                                  # sentinel elements between and behind the outputs
    total = sum((c * t * i + GAP) * (2 if d else 1) for c, t, i, _, d in WPREP_ITEMS)
    out = sentinel((total,), dtype)
    items, where, tile, off = [], [], 0, 0
    for cout, taps, cin, has_s, has_d in WPREP_ITEMS:
        w = torch.randn(cout, taps, cin, generator=gen)
        s = torch.rand(cout, generator=gen) + 0.5 if has_s else None
        W, S = gpu(w), (gpu(s) if has_s else None)
        _KEEP.extend([W, S])
        n = cout * taps * cin
        it = hip.WPrepItem()
        it.w, it.scale = W.data_ptr(), (S.data_ptr() if has_s else None)
        it.w_fprop = out.data_ptr() + off * es
        f_off = off
        off += n + GAP
        d_off = None
        if has_d:
            it.w_dgrad = out.data_ptr() + off * es
            d_off = off
            off += n + GAP
        else:
            it.w_dgrad = None
        it.cout, it.taps, it.cin, it.tile_begin = cout, taps, cin, tile
        tile += wprep_tiles(cout, taps, cin)
        items.append(it)
        where.append((w, s, W, S, f_off, d_off))
    assert off == total
    hip.call("vlfb_weight_prep_batched", hip.ptr(items_to_device(items)), len(items), tile, code)
    got = out.cpu()
    covered = torch.zeros(total, dtype=torch.bool)
    for (cout, taps, cin, has_s, has_d), (w, s, W, S, f_off, d_off) in zip(WPREP_ITEMS, where):
        n = cout * taps * cin
        ref = ((w * s.view(-1, 1, 1)) if has_s else w).to(dtype)
        assert torch.equal(got[f_off:f_off + n].view(cout, taps, cin), ref), (cout, taps, cin)
        covered[f_off:f_off + n] = True
        wf1 = sentinel((n,), dtype)
        wd1 = sentinel((n,), dtype) if has_d else None
        hip.call("vlfb_weight_prep", hip.ptr(W), hip.ptr(S), hip.ptr(wf1), hip.ptr(wd1), code, cout, taps, cin)
        assert torch.equal(wf1.cpu(), got[f_off:f_off + n])
        if has_d:
            assert torch.equal(got[d_off:d_off + n].view(cin, taps, cout), ref.permute(2, 1, 0).contiguous()), (cout, taps, cin)
            assert torch.equal(wd1.cpu(), got[d_off:d_off + n])
            covered[d_off:d_off + n] = True
    rest = got[~covered].float()
    assert rest.numel() == GAP * (len(WPREP_ITEMS) + sum(1 for it in WPREP_ITEMS if it[4]))
    assert float(rest.min()) == -77.0 and float(rest.max()) == -77.0, "memory between / behind the outputs was written"


class _StubConvStep:
    """what Engine._wprep_table_of reads of a ConvStep (one group)"""
    group, sname_fmt = 1, "s%d"

    def __init__(self, i, cout, taps, cin, wcode, w_f, w_d, has_s):
        self.Cog, self.Cin_k, self._taps, self.wcode = cout, cin, taps, wcode
        self.wname, self.sname = "w%d" % i, ("s%d" % i if has_s else None)
        self.wblk, self.w_f, self.w_d = cout * taps * cin, w_f, w_d

    def taps(self):
        return self._taps

    def wf_ptr(self, g):
        return self.w_f.data_ptr()

    def wd_ptr(self, g):
        return self.w_d.data_ptr()


@pytest.mark.parametrize("fmt", ["MIX_W2", "MIXH_W2"])
def test_weight_prep_batched_two_term_formats_through_the_engine_table_builder(fmt):
    """The "mix" weight formats, with the device table built by the engine's own Engine._wprep_table_of (reachable without a
    model: it reads a handful of attributes of its conv steps, stubbed here).  Bit-identical to vlfb_weight_prep per item;
    the terms reconstruct the fp32 master w * s within the bar tests/test_pair_gpu.py holds for weight planes
    (|v' - v| <= max(|v| 2^-21, 2^-24) on the stored value v)."""
    from vlfb.engine import Engine
    wcode = getattr(hip, fmt)
    gen = torch.Generator().manual_seed(53)
    params, steps, host = {}, [], []
    for i, (cout, taps, cin, has_s, has_d) in enumerate(WPREP_ITEMS):
        w = torch.randn(cout, taps, cin, generator=gen) * 0.07
        s = torch.rand(cout, generator=gen) + 0.5 if has_s else None
        params["w%d" % i] = gpu(w)
        if has_s:
            params["s%d" % i] = gpu(s)
        n = cout * taps * cin
        # FPROP copy: three bf16 planes (MIX_W2) / two fp16 planes (MIXH_W2); DGRAD copy: two fp16 terms [cin][2][taps][cout]
        w_f = sentinel((3 if fmt == "MIX_W2" else 2, cout, taps, cin), torch.bfloat16 if fmt == "MIX_W2" else torch.float16)
        w_d = sentinel((cin, 2, taps, cout), torch.float16) if has_d else None
        steps.append(_StubConvStep(i, cout, taps, cin, wcode, w_f, w_d, has_s))
        host.append((w, s))
    eng = types.SimpleNamespace(param_tensor=lambda name: params[name], device=dev())
    tab, n_items, tiles, code = Engine._wprep_table_of(eng, steps, wcode)
    assert n_items == len(steps) and code == wcode and tiles == sum(wprep_tiles(c, t, i) for c, t, i, _, _ in WPREP_ITEMS)
    hip.call("vlfb_weight_prep_batched", hip.ptr(tab), n_items, tiles, wcode)
    for st, (w, s), (cout, taps, cin, has_s, has_d) in zip(steps, host, WPREP_ITEMS):
        wf1 = torch.empty_like(st.w_f)
        wd1 = torch.empty_like(st.w_d) if has_d else None
        hip.call("vlfb_weight_prep", hip.ptr(params[st.wname]), hip.ptr(params[st.sname]) if has_s else None, hip.ptr(wf1),
                 hip.ptr(wd1), wcode, cout, taps, cin)
        assert torch.equal(wf1, st.w_f) and (not has_d or torch.equal(wd1, st.w_d))
        ws = ((w * s.view(-1, 1, 1)) if has_s else w)          # the fp32 master the kernel expands (rounded product)
        if fmt == "MIX_W2":
            v, back = ws.double(), st.w_f.double().sum(0).cpu()
        else:
            v, back = ws.double() * hip.MIX_W2_SCALE, st.w_f.double().sum(0).cpu()
        assert ((back - v).abs() <= torch.clamp(v.abs() * 2.0 ** -21, min=2.0 ** -24)).all(), "FPROP terms"
        if has_d:
            v = ws.double().permute(2, 1, 0) * hip.MIX_W2_SCALE
            back = st.w_d.double().sum(1).cpu()
            assert ((back - v).abs() <= torch.clamp(v.abs() * 2.0 ** -21, min=2.0 ** -24)).all(), "DGRAD terms"


# every weight code is a pair (FPROP copy, DGRAD copy), include/vlfb.h: "elem" = elements of the code's own type, "bf16x3" /
# "bf16x2" = bf16 term planes, "h2" = two fp16 planes of v * 2^10, "f16" = fp16 elements, "w2" / "w2i" = two fp16 terms of
# v * 2^10 as [Cin][term][taps][Cout] / interleaved [Cin][taps][Cout / 64][term][64]
WFORMATS = {"F32": ("elem", "elem"), "F16": ("elem", "elem"), "BF16": ("elem", "elem"), "SPLIT": ("bf16x3", "bf16x2"),
            "MIX": ("bf16x3", "f16"), "MIX_W2": ("bf16x3", "w2"), "MIX_W2I": ("bf16x3", "w2i"),
            "MIXH": ("h2", "f16"), "MIXH_W2": ("h2", "w2"), "MIXH_W2I": ("h2", "w2i")}
WFORMAT_ITEMS = [(64, 9, 4, True, True), (128, 3, 64, True, True), (192, 1, 40, False, True)]      # Cout % 64 == 0
WFORMAT_ITEMS_ANY_COUT = [(33, 1, 31, True, False), (40, 3, 72, True, True)]


def wformat_bytes(kind, v, elem):
    """the bytes of one weight operand copy of the fp32 values v (already in the copy's [a][taps][b] order), by definition"""
    from conv_desc_ref import bf16_terms, f16_pair, w2i_rows
    if kind == "elem":
        t = v.to(elem)
    elif kind == "f16":
        t = v.half()
    elif kind in ("bf16x3", "bf16x2"):
        t = torch.stack(bf16_terms(v, int(kind[-1])))
    elif kind == "h2":
        t = torch.stack(f16_pair(v * hip.MIX_W2_SCALE))
    elif kind == "w2":
        t = torch.stack(f16_pair(v * hip.MIX_W2_SCALE), 1)                     # [Cin][term][taps][Cout]
    else:
        t = w2i_rows((v * hip.MIX_W2_SCALE).reshape(-1, v.shape[-1]))[0]       # rows (Cin, tap) of [Cout / 64][term][64]
    return t.contiguous().view(-1).view(torch.uint8)


@pytest.mark.parametrize("fmt", sorted(WFORMATS))
def test_weight_prep_formats_batched_and_per_item(fmt):
    """All ten weight codes: the batched launch writes, per item and copy, exactly the bytes vlfb_weight_prep writes, those
    are the format's definition applied to the fp32-rounded w * s (tests/conv_desc_ref.py: bf16_terms, f16_pair, w2i_rows),
    and the bytes between and behind the outputs keep their sentinel."""
    wcode = getattr(hip, fmt)
    f_kind, d_kind = WFORMATS[fmt]
    elem = hip.TORCH_DTYPE.get(wcode)
    size = lambda kind: {"elem": elem.itemsize if elem else 0, "f16": 2, "bf16x3": 6, "bf16x2": 4, "h2": 4, "w2": 4, "w2i": 4}[kind]
    cases = WFORMAT_ITEMS + ([] if d_kind == "w2i" else WFORMAT_ITEMS_ANY_COUT)
    gen = torch.Generator().manual_seed(61)
    GAP, FILL = 48, 0xA5                                       # sentinel bytes between and behind the outputs (16-byte steps)
    total = sum(c * t * i * (size(f_kind) + (size(d_kind) if d else 0)) + GAP * (2 if d else 1) for c, t, i, _, d in cases)
    out = torch.full((total,), FILL, device=dev(), dtype=torch.uint8)
    items, where, tile, off = [], [], 0, 0
    for cout, taps, cin, has_s, has_d in cases:
        w = torch.randn(cout, taps, cin, generator=gen) * 0.07
        s = torch.rand(cout, generator=gen) + 0.5 if has_s else None
        W, S = gpu(w), (gpu(s) if has_s else None)
        _KEEP.extend([W, S])
        n = cout * taps * cin
        it = hip.WPrepItem()
        it.w, it.scale = W.data_ptr(), (S.data_ptr() if has_s else None)
        it.w_fprop, f_off = out.data_ptr() + off, off
        off += n * size(f_kind) + GAP
        it.w_dgrad, d_off = (out.data_ptr() + off, off) if has_d else (None, None)
        off += (n * size(d_kind) + GAP) if has_d else 0
        it.cout, it.taps, it.cin, it.tile_begin = cout, taps, cin, tile
        tile += wprep_tiles(cout, taps, cin)
        items.append(it)
        where.append((w, s, W, S, f_off, d_off))
    assert off == total
    hip.call("vlfb_weight_prep_batched", hip.ptr(items_to_device(items)), len(items), tile, wcode)
    got = out.cpu()
    covered = torch.zeros(total, dtype=torch.bool)
    for (cout, taps, cin, has_s, has_d), (w, s, W, S, f_off, d_off) in zip(cases, where):
        n = cout * taps * cin
        nf, nd = n * size(f_kind), n * size(d_kind)
        wf1 = torch.full((nf + GAP,), FILL, device=dev(), dtype=torch.uint8)
        wd1 = torch.full((nd + GAP,), FILL, device=dev(), dtype=torch.uint8) if has_d else None
        hip.call("vlfb_weight_prep", hip.ptr(W), hip.ptr(S), hip.ptr(wf1), hip.ptr(wd1), wcode, cout, taps, cin)
        ws = (w * s.view(-1, 1, 1)) if has_s else w              # the fp32-rounded product the formats are defined on
        for kind, v, o, nb, one in ((f_kind, ws, f_off, nf, wf1),) + (((d_kind, ws.permute(2, 1, 0).contiguous(), d_off, nd, wd1),) if has_d else ()):
            one = one.cpu()
            assert torch.equal(one[:nb], got[o:o + nb]), (cout, taps, cin, kind, "batched != per item")
            assert bool((one[nb:] == FILL).all()), (cout, taps, cin, kind, "vlfb_weight_prep wrote behind its output")
            assert torch.equal(one[:nb], wformat_bytes(kind, v, elem)), (cout, taps, cin, kind, "not the format's definition")
            covered[o:o + nb] = True
    rest = got[~covered]
    assert rest.numel() == GAP * (len(cases) + sum(1 for c in cases if c[4]))
    assert bool((rest == FILL).all()), "memory between / behind the outputs was written"


def test_weight_prep_rejects_what_is_not_a_weight_code():
    """VLFB_F16PAIR (8) names two-plane tensors, not a weight format; 11 is past the last code"""
    W = gpu(torch.ones(64, 1, 64))
    out = sentinel((2 * 3 * 64 * 64,), torch.float32)
    it = hip.WPrepItem()
    it.w, it.scale, it.w_fprop, it.w_dgrad = W.data_ptr(), None, out.data_ptr(), None
    it.cout, it.taps, it.cin, it.tile_begin = 64, 1, 64, 0
    tab = items_to_device([it])
    for code in (hip.F16PAIR, 11, -1):
        rejected("vlfb_weight_prep", hip.ptr(W), None, hip.ptr(out), None, code, 64, 1, 64, match="weight_prep: bad dtype")
        rejected("vlfb_weight_prep_batched", hip.ptr(tab), 1, wprep_tiles(64, 1, 64), code, match="weight_prep_batched: bad dtype")
    assert float(out.min()) == -77.0 and float(out.max()) == -77.0


# ------------------------------------------------------------------------------------------------
# vlfb_ncthw_to_nthwc / vlfb_nthwc_to_ncthw
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("thw", [1, 49, 1000])
@pytest.mark.parametrize("c", [3, 64, 65])
def test_layout_movers(c, thw, dtype):
    code = hip.dtype_code(dtype)
    n = 2
    gen = torch.Generator().manual_seed(c * 10000 + thw)
    x = torch.randn(n, c, thw, generator=gen)                      # fp32 NCTHW (T*H*W flattened)
    X = gpu(x)
    for c_pad in (c, (c + 8) // 8 * 8):
        D = sentinel((n * thw * c_pad + 4,), dtype)
        hip.call("vlfb_ncthw_to_nthwc", hip.ptr(X), hip.ptr(D), code, n, c, thw, c_pad)
        got = D[:n * thw * c_pad].view(n, thw, c_pad).cpu()
        assert torch.equal(got[:, :, :c], x.permute(0, 2, 1).to(dtype))
        assert torch.equal(got[:, :, c:].float(), torch.zeros(n, thw, c_pad - c)), "padded channels"
        assert float(D[n * thw * c_pad:].float().min()) == -77.0 and float(D[n * thw * c_pad:].float().max()) == -77.0
    # back: NTHWC `dtype` -> fp32 NCTHW
    src = q(torch.randn(n, thw, c, generator=gen), dtype)
    B = sentinel((n * c * thw + 4,), torch.float32)
    hip.call("vlfb_nthwc_to_ncthw", gp(src, dtype), hip.ptr(B), code, n, c, thw)
    assert torch.equal(B[:n * c * thw].view(n, c, thw).cpu(), src.permute(0, 2, 1).contiguous())
    assert float(B[n * c * thw:].min()) == -77.0 and float(B[n * c * thw:].max()) == -77.0
    if dtype == torch.float32:
        D = torch.empty(n, thw, c, device=dev())
        hip.call("vlfb_ncthw_to_nthwc", hip.ptr(X), hip.ptr(D), code, n, c, thw, c)
        R = torch.empty(n, c, thw, device=dev())
        hip.call("vlfb_nthwc_to_ncthw", hip.ptr(D), hip.ptr(R), code, n, c, thw)
        assert torch.equal(R.cpu(), x), "round trip"


# ------------------------------------------------------------------------------------------------
# max pooling with more than 255 taps: the 16-bit arg-max
# ------------------------------------------------------------------------------------------------
WIDE_POOLS = {
    # name: (k, s, p, (N, T, H, W))
    "k488_global": ((4, 8, 8), (4, 8, 8), (0, 0, 0), (2, 4, 8, 8)),
    "k488_strided": ((4, 8, 8), (2, 4, 4), (1, 2, 2), (2, 8, 16, 16)),
    "k2x16x16_global": ((2, 16, 16), (2, 16, 16), (0, 0, 0), (2, 2, 16, 16)),
    "k2x16x16_strided": ((2, 16, 16), (1, 8, 8), (0, 4, 4), (1, 4, 24, 24)),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(WIDE_POOLS))
def test_maxpool_with_a_16_bit_argmax(name, dtype):
    k, s, p, (N, T, H, W) = WIDE_POOLS[name]
    Cc = 16
    code = hip.dtype_code(dtype)
    d = hip.pool_desc(code, N, T, H, W, Cc, 1, 1, 1, k, s, p)
    assert hip.lib().vlfb_pool_argmax_bytes(C.byref(d)) == 2
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    x = q(torch.randn(N, Cc, T, H, W, generator=gen), dtype)
    xd = x.double().requires_grad_(True)
    y_ref, idx = F.max_pool3d(xd, k, s, p, return_indices=True)
    To, Ho, Wo = y_ref.shape[2:]
    d = hip.pool_desc(code, N, T, H, W, Cc, To, Ho, Wo, k, s, p)
    assert hip.query_workspace(hip.WS_MAXPOOL_ARGMAX, d) == N * To * Ho * Wo * Cc * 2
    X = gpu(to_nthwc(x), dtype)
    Y = torch.empty(N, To, Ho, Wo, Cc, device=dev(), dtype=dtype)
    AM = torch.full((N * To * Ho * Wo * Cc + 8,), -3, device=dev(), dtype=torch.int16)
    hip.call("vlfb_maxpool_fwd", C.byref(d), hip.ptr(X), hip.ptr(Y), hip.ptr(AM))
    assert torch.equal(to_ncthw(Y.float()).cpu(), y_ref.float())
    assert AM[-8:].tolist() == [-3] * 8
    # the tap index inside the window, from torch's flat input index (both take the first maximum in t, h, w order)
    ti, hi, wi = idx // (H * W), (idx // W) % H, idx % W
    to = torch.arange(To).view(1, 1, To, 1, 1)
    ho = torch.arange(Ho).view(1, 1, 1, Ho, 1)
    wo = torch.arange(Wo).view(1, 1, 1, 1, Wo)
    tap = ((ti - (to * s[0] - p[0])) * k[1] + (hi - (ho * s[1] - p[1]))) * k[2] + (wi - (wo * s[2] - p[2]))
    am = AM[:-8].view(N, To, Ho, Wo, Cc).cpu().to(torch.int32) & 0xFFFF
    assert torch.equal(to_ncthw(am).long(), tap)
    if k[0] * k[1] * k[2] > 256:      # (256 taps: indices end at 255, the value the one-byte kernels keep for "no window")
        assert int(am.max()) > 255, "no arg-max beyond one byte: the case does not tell the two widths apart"
    # backward
    dy = q(torch.randn(N, Cc, To, Ho, Wo, generator=gen), dtype)
    (gx,) = torch.autograd.grad(y_ref, (xd,), dy.double())
    add = q(torch.randn(N, Cc, T, H, W, generator=gen), dtype)
    DX = torch.empty(N, T, H, W, Cc, device=dev(), dtype=dtype)
    DY = gp(to_nthwc(dy), dtype)
    hip.call("vlfb_maxpool_bwd", C.byref(d), DY, hip.ptr(AM), hip.ptr(DX), None, None)
    assert rel_err(to_ncthw(DX.float()), gx) < TOL[dtype]
    hip.call("vlfb_maxpool_bwd", C.byref(d), DY, hip.ptr(AM), hip.ptr(DX), gp(to_nthwc(add), dtype), hip.ptr(X))
    ref = torch.where(x.double() > 0, gx + add.double(), torch.zeros_like(gx))
    assert rel_err(to_ncthw(DX.float()), ref) < TOL[dtype]
    # pool of a ReLU output: mask from the pooled tensor == mask from the input, bit for bit
    XR = torch.relu(X)
    hip.call("vlfb_maxpool_fwd", C.byref(d), hip.ptr(XR), hip.ptr(Y), hip.ptr(AM))
    D1, D2 = torch.empty_like(DX), torch.empty_like(DX)
    hip.call("vlfb_maxpool_bwd", C.byref(d), DY, hip.ptr(AM), hip.ptr(D1), None, hip.ptr(XR))
    hip.call("vlfb_maxpool_relu_bwd", C.byref(d), DY, hip.ptr(AM), hip.ptr(Y), hip.ptr(D2))
    assert torch.equal(D1, D2) and float(D1.float().abs().sum()) > 0
    xr = torch.relu(x).double().requires_grad_(True)
    yr = F.max_pool3d(xr, k, s, p)
    (gr,) = torch.autograd.grad(yr, (xr,), dy.double())
    assert rel_err(to_ncthw(D1.float()), torch.where(xr > 0, gr, torch.zeros_like(gr))) < TOL[dtype]


# ------------------------------------------------------------------------------------------------
# vlfb_colsum
# ------------------------------------------------------------------------------------------------
COLSUM = [  # rows, cols, ld, accumulate
    (1, 8, 8, 0),
    (1025, 104, 128, 0),            # two slabs, the second of ONE row; ld > cols; the last column block mostly out of range
    (5000, 2048, 2048, 0),          # many column blocks x five slabs
    (300000, 64, 64, 0),            # 293 slabs of one or two column blocks
    (2500, 200, 264, 1),            # onto a random base
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", COLSUM)
def test_colsum(case, dtype):
    rows, cols, ld, accumulate = case
    code = hip.dtype_code(dtype)
    gen = torch.Generator().manual_seed(rows + cols)
    g = q(torch.randn(rows, ld, generator=gen), dtype)
    base = torch.randn(cols, generator=gen)
    out = torch.cat([gpu(base.clone()) if accumulate else sentinel((cols,), torch.float32), sentinel((8,), torch.float32)])
    hip.call("vlfb_colsum", gp(g, dtype), code, rows, cols, ld, hip.ptr(out), accumulate)
    ref = g[:, :cols].double().sum(0) + (base.double() if accumulate else 0.0)
    err = rel_err(out[:cols], ref)
    print("\n[colsum %s %dx%d ld %d acc %d] rel err %.2e" % (dtype, rows, cols, ld, accumulate, err))
    assert err < 1e-5
    assert float(out[cols:].min()) == -77.0 and float(out[cols:].max()) == -77.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_colsum_rejects_before_it_launches(dtype):
    """cols / ld that are not whole 16-byte vectors: an error code, and `out` as it was (accumulate = 0 zeroes it otherwise)"""
    code = hip.dtype_code(dtype)
    v = 4 if dtype == torch.float32 else 8
    g = gpu(torch.zeros(16, 4 * v), dtype)
    for cols, ld in ((v + v // 2, 4 * v), (v, 2 * v + 1)):
        out = sentinel((4 * v,), torch.float32)
        rejected("vlfb_colsum", hip.ptr(g), code, 16, cols, ld, hip.ptr(out), 0, match="multiples of")
        torch.cuda.synchronize()
        assert float(out.min()) == -77.0 and float(out.max()) == -77.0


# ------------------------------------------------------------------------------------------------
# vlfb_layernorm_*: fewer columns than lanes, a partial last lane group, a row without variance
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 9])
@pytest.mark.parametrize("cols", [8, 40, 100, 512, 1000])
def test_layernorm_widths_and_a_constant_row(cols, rows, dtype):
    """The constant row holds -2.5: with so few mantissa bits every fp32 partial sum of up to 1000 of them is exact in any
    order, so mean == -2.5 and var == 0 exactly and anything but y == 0, rstd == fp32(1 / sqrt(eps)) is an error."""
    code = hip.dtype_code(dtype)
    eps = 1e-5
    gen = torch.Generator().manual_seed(cols * 10 + rows)
    x = q(torch.randn(rows, cols, generator=gen) * 3 + 1, dtype)
    const = rows // 2 if rows > 1 else None
    if const is not None:
        x[const] = -2.5
    xd = x.double().requires_grad_(True)
    y_ref = F.layer_norm(xd, (cols,), eps=eps)
    Y = sentinel((rows + 1, cols), dtype)
    rstd = sentinel((rows + 1,), torch.float32)
    hip.call("vlfb_layernorm_fwd", gp(x, dtype), hip.ptr(Y), hip.ptr(rstd), code, rows, cols, eps)
    assert rel_err(Y[:rows].float(), y_ref) < TOL[dtype]
    assert float(Y[rows].float().min()) == -77.0 and float(Y[rows].float().max()) == -77.0 and float(rstd[rows]) == -77.0
    rstd_ref = 1.0 / torch.sqrt(x.double().var(1, unbiased=False) + float(torch.tensor(eps)))
    assert rel_err(rstd[:rows], rstd_ref) < 1e-5
    if const is not None:
        assert torch.equal(Y[const].float().cpu(), torch.zeros(cols))
        want = 1.0 / math.sqrt(float(torch.tensor(eps)))
        assert abs(float(rstd[const]) - want) <= 2.0 ** -23 * want
    dy = q(torch.randn(rows, cols, generator=gen), dtype)
    (gx,) = torch.autograd.grad(y_ref, (xd,), dy.double())
    DX = sentinel((rows + 1, cols), dtype)
    hip.call("vlfb_layernorm_bwd", gp(dy, dtype), hip.ptr(Y), hip.ptr(rstd), hip.ptr(DX), code, rows, cols)
    assert torch.isfinite(DX[:rows].float()).all()
    assert rel_err(DX[:rows].float(), gx) < (1e-4 if dtype == torch.float32 else 2e-2)
    assert float(DX[rows].float().min()) == -77.0 and float(DX[rows].float().max()) == -77.0


# ------------------------------------------------------------------------------------------------
# vlfb_fc_*: no bias, accumulate, one row, one class
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cin,cout", [(6, 2560, 157), (1, 2560, 157), (6, 200, 1), (1, 72, 1), (5, 37, 3)])
def test_fc_without_bias_and_with_accumulate(rows, cin, cout, dtype):
    code = hip.dtype_code(dtype)
    gen = torch.Generator().manual_seed(rows * 7 + cin + cout)
    x = q(torch.randn(rows, cin, generator=gen), dtype)
    w = torch.randn(cout, cin, generator=gen) * 0.05
    b = torch.randn(cout, generator=gen) * 0.1
    X = gpu(x, dtype)
    lin = x.double() @ w.double().t()
    for bias in (None, b):
        L = sentinel((rows * cout + 4,), torch.float32)
        hip.call("vlfb_fc_fwd", hip.ptr(X), code, gp(w), None if bias is None else gp(bias), hip.ptr(L), rows, cin, cout)
        assert rel_err(L[:rows * cout].view(rows, cout), lin + (0 if bias is None else bias.double())) < 1e-5
        assert float(L[rows * cout:].min()) == -77.0 and float(L[rows * cout:].max()) == -77.0
    dl = torch.randn(rows, cout, generator=gen)
    gx, gw, gb = dl.double() @ w.double(), dl.double().t() @ x.double(), dl.double().sum(0)
    for accumulate in (0, 1):
        dw0, db0 = torch.randn(cout, cin, generator=gen), torch.randn(cout, generator=gen)
        DX = sentinel((rows * cin + 8,), dtype)
        DW = torch.cat([gpu(dw0.clone()).view(-1), sentinel((4,), torch.float32)])
        DB = torch.cat([gpu(db0.clone()), sentinel((4,), torch.float32)])
        hip.call("vlfb_fc_bwd", hip.ptr(X), code, gp(w), gp(dl), hip.ptr(DX), hip.ptr(DW), hip.ptr(DB), rows, cin, cout, accumulate)
        assert rel_err(DX[:rows * cin].view(rows, cin).float(), gx) < TOL[dtype]
        assert rel_err(DW[:cout * cin].view(cout, cin), gw + (dw0.double() if accumulate else 0)) < 1e-4
        assert rel_err(DB[:cout], gb + (db0.double() if accumulate else 0)) < 1e-4
        for t in (DX[rows * cin:].float(), DW[cout * cin:], DB[cout:]):
            assert float(t.min()) == -77.0 and float(t.max()) == -77.0
    # parameter gradients only (dx == NULL), bias gradient not wanted (db == NULL)
    DW = torch.empty(cout, cin, device=dev())
    hip.call("vlfb_fc_bwd", hip.ptr(X), code, gp(w), gp(dl), None, hip.ptr(DW), None, rows, cin, cout, 0)
    assert rel_err(DW, gw) < 1e-4


# ------------------------------------------------------------------------------------------------
# vlfb_fbo_attn_fwd_shared: one projected bank per clip, rows pick theirs through the batch-index column of the RoIs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [512, 40])
def test_fbo_attention_with_shared_banks(dtype, D):
    """against fp64 on the bank each row owns (bars of test_fbo_attention_core), and bit-identical to vlfb_fbo_attn_fwd on the
    duplicated banks, as vlfb.h promises.  D = 512: chip-wide kernels; D = 40: per-row kernel."""
    gen = torch.Generator().manual_seed(59)
    code = hip.dtype_code(dtype)
    R, K, NB = 7, 300, 3
    rois = torch.zeros(R, 5)
    rois[:, 0] = torch.tensor([0, 0, 2, 1, 2, 2, 0], dtype=torch.float32)     # not sorted, a bank with one reader
    rois[:, 1:] = torch.rand(R, 4, generator=gen) * 200
    owner = rois[:, 0].long()
    theta = q(torch.randn(R, D, generator=gen), dtype)
    phi = q(torch.randn(NB, K, D, generator=gen), dtype)
    g = q(torch.randn(NB, K, D, generator=gen), dtype)
    scale = D ** -0.5
    p_ref = torch.softmax(torch.einsum("rd,rkd->rk", theta.double(), phi.double()[owner]) * scale, dim=1)
    t_ref = torch.einsum("rk,rkd->rd", p_ref, g.double()[owner])
    TH, PH, G, RO = gpu(theta, dtype), gpu(phi, dtype), gpu(g, dtype), gpu(rois)
    P = sentinel((R + 1, K), torch.float32)
    T = sentinel((R + 1, D), dtype)
    hip.call("vlfb_fbo_attn_fwd_shared", hip.ptr(TH), hip.ptr(PH), hip.ptr(G), hip.ptr(P), hip.ptr(T), code, R, K, D, D, scale,
             hip.ptr(RO), 5)
    assert rel_err(P[:R], p_ref) < 1e-5
    assert rel_err(T[:R].float(), t_ref) < TOL[dtype]
    assert float(P[R].min()) == -77.0 and float(P[R].max()) == -77.0
    assert float(T[R].float().min()) == -77.0 and float(T[R].float().max()) == -77.0
    P2 = torch.empty(R, K, device=dev())
    T2 = torch.empty(R, D, device=dev(), dtype=dtype)
    hip.call("vlfb_fbo_attn_fwd", hip.ptr(TH), gp(phi[owner].contiguous(), dtype), gp(g[owner].contiguous(), dtype), hip.ptr(P2),
             hip.ptr(T2), code, R, K, D, D, scale)
    assert torch.equal(P[:R], P2) and torch.equal(T[:R], T2)
    rejected("vlfb_fbo_attn_fwd_shared", hip.ptr(TH), hip.ptr(PH), hip.ptr(G), hip.ptr(P), hip.ptr(T), code, R, K, D, D, scale,
             None, 5, match="owner")
