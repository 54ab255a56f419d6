"""The pooling kernels of csrc/vlfb_pool.hip against the references of tests/pool_cases.py, on the case table that
tests/test_pool_cases_host.py holds to its routes and tie conditions.

Max pools are compared bit for bit -- forward values and arg-max taps, and the backward against the fp32-ordered emulation on
every route (band R=3 / R=2, the three compiled windows with and without the pooled-value mask, the generic kernel with a one-
and a two-byte arg-max), generator and operand combination.  Average pools are compared per element with the fp64 reference
under the bound derived in pool_cases; where every input position lies in one window the backward is one product and is
compared bit for bit, the two-term form included; the average forward pools are also compared bit for bit with the fp32-ordered
emulation of pool_cases."""
import ctypes as C

import pytest
import torch

import pool_cases as pc
from gpu_util import dev

pytestmark = pytest.mark.gpu

hip = None
GUARD = 16                                          # bytes behind the arg-max buffer that no launch may touch


def setup_module(module):
    from vlfb import hip as h
    module.hip = h
    h.lib()


def gpu(t):
    return t.contiguous().to(dev())


def code_of(dtype_name):
    return hip.dtype_code(pc.DTYPES[dtype_name])


def max_desc(case, code):
    N, T, H, W = case.shape
    return hip.pool_desc(code, N, T, H, W, case.C, *pc.out_dims(case), case.k, case.s, case.p)


def argmax_buffer(d, numel):
    nbytes = hip.lib().vlfb_pool_argmax_bytes(C.byref(d))
    return torch.full((numel * nbytes + GUARD,), 0xA5, device=dev(), dtype=torch.uint8), nbytes


def taps_of(am, nbytes, shape):
    body = am[:-GUARD].cpu()
    if nbytes == 2:
        body = body.view(torch.int16).to(torch.int64) & 0xFFFF
    return body.to(torch.int64).view(shape)


def same_bits(got, ref):
    return torch.equal(pc.bits(got.cpu()), pc.bits(ref))


# ------------------------------------------------------------------------------------------------
# max pool, forward
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.MAX_CASES, ids=lambda c: c.name)
def test_maxpool_forward_values_and_taps(case):
    for dtype_name in case.dtypes:
        d = max_desc(case, code_of(dtype_name))
        for gen in pc.GENERATORS:
            ref = pc.max_data(case.name, dtype_name, gen)
            X = gpu(ref.x)
            Y = torch.full(ref.y.shape, float("nan"), device=dev(), dtype=ref.y.dtype)
            AM, nbytes = argmax_buffer(d, ref.y.numel())
            hip.call("vlfb_maxpool_fwd", C.byref(d), hip.ptr(X), hip.ptr(Y), hip.ptr(AM))
            assert same_bits(Y, ref.y), (dtype_name, gen)
            assert torch.equal(taps_of(AM, nbytes, ref.tap.shape), ref.tap), (dtype_name, gen)
            assert AM[-GUARD:].tolist() == [0xA5] * GUARD
            # inference: no arg-max
            Y.fill_(float("nan"))
            hip.call("vlfb_maxpool_fwd", C.byref(d), hip.ptr(X), hip.ptr(Y), None)
            assert same_bits(Y, ref.y)


def pair_inputs(case, gen):
    """canonical two-plane input made by vlfb_pair_split on the device: (device pair tensor, hi, lo on the CPU)"""
    v = pc.values(gen, tuple(case.shape) + (case.C,), None, pc._gen(case.name, gen))
    V = gpu(v)
    P = torch.empty(2 * v.numel(), device=dev(), dtype=torch.float16)
    hip.call("vlfb_pair_split", hip.ptr(V), hip.ptr(P), v.numel())
    planes = P.cpu().view((2,) + tuple(v.shape))
    hi, lo = pc.pair_split(v)
    assert same_bits(planes[0], hi) and same_bits(planes[1], lo)
    return P, planes[0], planes[1]


@pytest.mark.parametrize("case", pc.MAX_CASES + pc.MIX_CASES, ids=lambda c: c.name)
def test_pair_maxpool_forward_values_and_taps(case):
    d = max_desc(case, hip.F16PAIR)
    gens = pc.GENERATORS if case in pc.MAX_CASES else pc.MIX_GENERATORS
    for gen in gens:
        P, hi, lo = pair_inputs(case, gen)
        (yh, yl), tap = pc.max_fwd(hi, case, lo=lo)
        Y = torch.full((2,) + tuple(yh.shape), float("nan"), device=dev(), dtype=torch.float16)
        AM, nbytes = argmax_buffer(d, yh.numel())
        hip.call("vlfb_maxpool_fwd", C.byref(d), hip.ptr(P), hip.ptr(Y), hip.ptr(AM))
        assert same_bits(Y[0], yh) and same_bits(Y[1], yl), gen
        assert torch.equal(taps_of(AM, nbytes, tap.shape), tap), gen
        assert AM[-GUARD:].tolist() == [0xA5] * GUARD


# ------------------------------------------------------------------------------------------------
# max pool, backward
# ------------------------------------------------------------------------------------------------
def run_max_bwd(d, combo, DY, AM, Y, ADD, MASK, shape, dtype):
    """one backward launch into a NaN-filled buffer (alias: into a copy of `add`); returns dx"""
    if combo == "alias":
        DX = ADD.clone()
        hip.call("vlfb_maxpool_bwd", C.byref(d), hip.ptr(DY), hip.ptr(AM), hip.ptr(DX), hip.ptr(DX), None)
        return DX
    DX = torch.full(shape, float("nan"), device=dev(), dtype=dtype)
    if combo == "relu":
        hip.call("vlfb_maxpool_relu_bwd", C.byref(d), hip.ptr(DY), hip.ptr(AM), hip.ptr(Y), hip.ptr(DX))
    else:
        hip.call("vlfb_maxpool_bwd", C.byref(d), hip.ptr(DY), hip.ptr(AM), hip.ptr(DX),
                 hip.ptr(ADD) if "add" in combo else None, hip.ptr(MASK) if "mask" in combo else None)
    return DX


@pytest.mark.parametrize("case", pc.MAX_CASES, ids=lambda c: c.name)
def test_maxpool_backward_is_the_fp32_ordered_sum_bit_for_bit(case):
    cov = pc.covered(case)
    for dtype_name in case.dtypes:
        dtype = pc.DTYPES[dtype_name]
        d = max_desc(case, code_of(dtype_name))
        for gen in pc.GENERATORS:
            ref = pc.max_data(case.name, dtype_name, gen)
            X, DY, ADD, MASK = gpu(ref.x), gpu(ref.dy), gpu(ref.add), gpu(ref.mask)
            Y = torch.empty(ref.y.shape, device=dev(), dtype=dtype)
            AM, nbytes = argmax_buffer(d, ref.y.numel())
            hip.call("vlfb_maxpool_fwd", C.byref(d), hip.ptr(X), hip.ptr(Y), hip.ptr(AM))
            assert torch.equal(taps_of(AM, nbytes, ref.tap.shape), ref.tap)
            got = {}
            for combo in case.combos:
                what = (case.name, dtype_name, gen, combo, hip.maxpool_bwd_route(d, add="add" in combo or combo == "alias",
                                                                                   mask="mask" in combo, y=combo == "relu"))
                assert what[-1] == pc.expected_route(case, dtype_name, combo)
                DX = run_max_bwd(d, combo, DY, AM, Y, ADD, MASK, ref.x.shape, dtype)
                want = pc.max_bwd_combo(case, ref, combo)
                assert same_bits(DX, want), what
                again = run_max_bwd(d, combo, DY, AM, Y, ADD, MASK, ref.x.shape, dtype)
                assert torch.equal(pc.bits(again.cpu()), pc.bits(DX.cpu())), what       # the same launch twice
                got[combo] = DX.cpu()
                if combo in ("none", "relu", "mask"):
                    assert (pc.bits(got[combo])[:, ~cov] == 0).all(), what               # no covering window: exactly +0
            if "alias" in got:
                assert torch.equal(pc.bits(got["alias"]), pc.bits(got["add"]))
            if gen == "relu_levels" and "relu" in got:
                # the pooled values as the ReLU mask == the input as the mask, bit for bit
                D1 = torch.full(ref.x.shape, float("nan"), device=dev(), dtype=dtype)
                hip.call("vlfb_maxpool_bwd", C.byref(d), hip.ptr(DY), hip.ptr(AM), hip.ptr(D1), None, hip.ptr(X))
                assert torch.equal(pc.bits(D1.cpu()), pc.bits(got["relu"])) and float(D1.float().abs().sum()) > 0
                assert same_bits(D1, pc.max_bwd(case, ref.tap, ref.dy, mask=ref.x))
    if case.name == "temporal_odd":
        assert not cov[4].any()
    if case.name == "nl_odd":
        assert not cov[:, -1].any() and not cov[:, :, -1].any()


@pytest.mark.parametrize("case", pc.MIX_CASES, ids=lambda c: c.name)
def test_mix_route_pair_forward_then_fp16_backward_on_the_hi_plane(case):
    """as the engine does on `mix`: the forward on two fp16 planes, the backward in fp16 through the arg-max of that forward
    with y = the hi plane of the pooled pair"""
    dp, db = max_desc(case, hip.F16PAIR), max_desc(case, hip.F16)
    assert hip.maxpool_bwd_route(db, y=True) == pc.expected_route(case, "fp16", "relu")
    for gen in pc.MIX_GENERATORS:
        P, hi, lo = pair_inputs(case, gen)
        (yh, yl), tap = pc.max_fwd(hi, case, lo=lo)
        Y = torch.full((2,) + tuple(yh.shape), float("nan"), device=dev(), dtype=torch.float16)
        AM, nbytes = argmax_buffer(dp, yh.numel())
        hip.call("vlfb_maxpool_fwd", C.byref(dp), hip.ptr(P), hip.ptr(Y), hip.ptr(AM))
        assert same_bits(Y[0], yh) and torch.equal(taps_of(AM, nbytes, tap.shape), tap)
        dy = pc.operands(tap.shape, torch.float16, pc._gen(case.name, gen, "dy"))
        DY = gpu(dy)
        DX = torch.full(hi.shape, float("nan"), device=dev(), dtype=torch.float16)
        hip.call("vlfb_maxpool_relu_bwd", C.byref(db), hip.ptr(DY), hip.ptr(AM), hip.ptr(Y), hip.ptr(DX))   # (Y: the hi plane first)
        assert same_bits(DX, pc.max_bwd(case, tap, dy, y=yh)), gen
        assert float(DX.float().abs().sum()) > 0


# ------------------------------------------------------------------------------------------------
# average pools
# ------------------------------------------------------------------------------------------------
def avg_desc(case, code):
    N, T, H, W = case.shape
    geo = pc.MaxCase(case.name, case.k, case.s, (0, 0, 0), case.shape, case.C, None, None)
    return hip.pool_desc(code, N, T, H, W, case.C, *pc.out_dims(geo), case.k, case.s, (0, 0, 0)), pc.out_dims(geo)


def worst_ratio(got, ref, bound):
    err = (got.double().cpu() - ref).abs()
    assert (err <= bound).all(), "worst %.3f of the bound" % (err / bound.clamp_min(1e-300)).max().item()
    nz = bound > 0
    return (err[nz] / bound[nz]).max().item() if nz.any() else 0.0


@pytest.mark.parametrize("dtype_name", list(pc.DTYPES) + ["f16pair"])
@pytest.mark.parametrize("case", pc.AVG_CASES, ids=lambda c: c.name)
def test_avgpool_forward_within_the_derived_bound(case, dtype_name):
    g = pc._gen(case.name, dtype_name, "x")
    shape = tuple(case.shape) + (case.C,)
    if dtype_name == "f16pair":
        d, od = avg_desc(case, hip.F16PAIR)
        V = gpu(torch.randn(shape, generator=g))
        P = torch.empty(2 * V.numel(), device=dev(), dtype=torch.float16)
        hip.call("vlfb_pair_split", hip.ptr(V), hip.ptr(P), V.numel())
        planes = P.cpu().view((2,) + shape)
        ref, bound = pc.avg_fwd(planes[0], case, lo=planes[1])
        emu = pc.avg_fwd_emulated(planes[0], case, lo=planes[1])
        Y = torch.full(ref.shape, float("nan"), device=dev(), dtype=torch.float32)
        hip.call("vlfb_avgpool_fwd", C.byref(d), hip.ptr(P), hip.ptr(Y))
    else:
        dtype = pc.DTYPES[dtype_name]
        d, od = avg_desc(case, code_of(dtype_name))
        x = torch.randn(shape, generator=g).to(dtype)
        ref, bound = pc.avg_fwd(x, case)
        emu = pc.avg_fwd_emulated(x, case)
        if dtype_name != "fp32":
            bound = bound + 0.5 * pc.ulp(ref, dtype_name)
        X = gpu(x)
        Y = torch.full(ref.shape, float("nan"), device=dev(), dtype=dtype)
        hip.call("vlfb_avgpool_fwd", C.byref(d), hip.ptr(X), hip.ptr(Y))
    assert tuple(ref.shape[1:4]) == od
    print("avgpool_fwd %s %s (%s): worst %.3f of the bound" % (case.name, dtype_name, "global" if case.is_global else "window",
                                                              worst_ratio(Y, ref, bound)))
    assert same_bits(Y, emu), "%d elements differ from the fp32-ordered emulation" % int((pc.bits(Y.cpu()) != pc.bits(emu)).sum())


@pytest.mark.parametrize("dtype_name", list(pc.DTYPES))
@pytest.mark.parametrize("case", pc.AVG_CASES, ids=lambda c: c.name)
def test_avgpool_backward_within_the_derived_bound(case, dtype_name):
    dtype = pc.DTYPES[dtype_name]
    d, od = avg_desc(case, code_of(dtype_name))
    g = pc._gen(case.name, dtype_name, "dy")
    shape = tuple(case.shape) + (case.C,)
    dy = pc.operands((case.shape[0],) + od + (case.C,), dtype, g)
    add, mask = pc.operands(shape, dtype, g), pc.mask_operand(shape, dtype, g)
    DY, ADD, MASK = gpu(dy), gpu(add), gpu(mask)
    for combo in pc.AVG_COMBOS:
        a, m = (add if "add" in combo else None), (mask if "mask" in combo else None)
        ref, bound = pc.avg_bwd(case, dy, add=a, mask=m)
        if dtype_name != "fp32":
            bound = bound + 0.5 * pc.ulp(ref, dtype_name)
        DX = torch.full(shape, float("nan"), device=dev(), dtype=dtype)
        hip.call("vlfb_avgpool_bwd", C.byref(d), hip.ptr(DY), hip.ptr(DX), hip.ptr(ADD) if a is not None else None,
                 hip.ptr(MASK) if m is not None else None)
        print("avgpool_bwd %s %s %s: worst %.3f of the bound" % (case.name, dtype_name, combo, worst_ratio(DX, ref, bound)))
        if case.one_window and a is None:
            # one window per position: one product, one rounding -- exact
            _, hi, _ = pc.avg_bwd_one_window(case, dy.float(), dtype, mask=m)
            assert same_bits(DX, hi), combo


@pytest.mark.parametrize("dtype_name", ["fp16", "bf16"])
@pytest.mark.parametrize("case", pc.AVG_CASES, ids=lambda c: c.name)
def test_avgpool_backward_two_term(case, dtype_name):
    dtype = pc.DTYPES[dtype_name]
    d, od = avg_desc(case, code_of(dtype_name))
    g = pc._gen(case.name, dtype_name, "dy32")
    shape = tuple(case.shape) + (case.C,)
    dy = torch.randn((case.shape[0],) + od + (case.C,), generator=g) * 64.0     # (gradients carry the loss scale)
    mask = pc.mask_operand(shape, dtype, g)
    DY, MASK = gpu(dy), gpu(mask)
    for m in (None, mask):
        ref, b32 = pc.avg_bwd(case, dy, mask=m)
        HI, LO = (torch.full(shape, float("nan"), device=dev(), dtype=dtype) for _ in range(2))
        hip.call("vlfb_avgpool_bwd_two_term", C.byref(d), hip.ptr(DY), hip.ptr(HI), hip.ptr(LO), hip.ptr(MASK) if m is not None else None)
        r_hi = worst_ratio(HI, ref, b32 + 0.5 * pc.ulp(ref, dtype_name))
        # lo = round_T(v - hi) with |v - hi| <= |ref - hi| + the fp32 bound: one more rounding, of that magnitude
        resid = (ref - HI.double().cpu()).abs() + b32
        r_two = worst_ratio(HI.double() + LO.double(), ref, b32 + 0.5 * pc.ulp(resid, dtype_name))
        print("avgpool_bwd_two_term %s %s mask=%s: hi worst %.3f, hi + lo worst %.3f of the bound" % (case.name, dtype_name, m is not None,
                                                                                                     r_hi, r_two))
        if case.one_window:
            _, hi, lo = pc.avg_bwd_one_window(case, dy, dtype, mask=m)
            assert same_bits(HI, hi) and same_bits(LO, lo)


# ------------------------------------------------------------------------------------------------
# descriptors that contradict themselves launch nothing
# ------------------------------------------------------------------------------------------------
def test_inconsistent_descriptors_raise_and_leave_the_output_untouched():
    N, T, H, W, Cc = 1, 2, 9, 11, 8
    X = torch.randn(N, T, H, W, Cc, device=dev()).to(torch.float16)
    big = N * T * H * W * Cc

    def untouched(buf):
        return bool(torch.isnan(buf).all())
    # max pool: one output column more than the input carries (Wo = 7: window start 11 > 10)
    d = hip.pool_desc(hip.F16, N, T, H, W, Cc, T, 5, 7, (1, 3, 3), (1, 2, 2), (0, 1, 1))
    Y = torch.full((big,), float("nan"), device=dev(), dtype=torch.float16)
    AM = torch.zeros(big, device=dev(), dtype=torch.uint8)
    with pytest.raises(hip.VlfbError, match="dimension w"):
        hip.call("vlfb_maxpool_fwd", C.byref(d), hip.ptr(X), hip.ptr(Y), hip.ptr(AM))
    assert untouched(Y)
    with pytest.raises(hip.VlfbError, match="dimension w"):
        hip.call("vlfb_maxpool_bwd", C.byref(d), hip.ptr(X), hip.ptr(AM), hip.ptr(Y), None, None)
    with pytest.raises(hip.VlfbError, match="dimension w"):
        hip.call("vlfb_maxpool_relu_bwd", C.byref(d), hip.ptr(X), hip.ptr(AM), hip.ptr(X), hip.ptr(Y))
    assert untouched(Y)
    # average pool: the last window row leaves the input (Ho = 5: 4 * 2 + 3 > 9), a pad as large as the kernel
    d = hip.pool_desc(hip.F16, N, T, H, W, Cc, T, 5, 5, (1, 3, 3), (1, 2, 2), (0, 0, 0))
    with pytest.raises(hip.VlfbError, match="dimension h"):
        hip.call("vlfb_avgpool_fwd", C.byref(d), hip.ptr(X), hip.ptr(Y))
    with pytest.raises(hip.VlfbError, match="dimension h"):
        hip.call("vlfb_avgpool_bwd", C.byref(d), hip.ptr(X), hip.ptr(Y), None, None)
    G = torch.zeros(big, device=dev(), dtype=torch.float32)
    with pytest.raises(hip.VlfbError, match="dimension h"):
        hip.call("vlfb_avgpool_bwd_two_term", C.byref(d), hip.ptr(G), hip.ptr(Y), hip.ptr(Y), None)
    d = hip.pool_desc(hip.F16, N, T, H, W, Cc, T, 4, 5, (1, 3, 3), (1, 2, 2), (1, 0, 0))
    with pytest.raises(hip.VlfbError, match="dimension t: pad 1"):
        hip.call("vlfb_maxpool_fwd", C.byref(d), hip.ptr(X), hip.ptr(Y), hip.ptr(AM))
    torch.cuda.synchronize()
    assert untouched(Y)
