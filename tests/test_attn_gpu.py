"""The fused non-local attention kernels (csrc/vlfb_attn.hip): scores + row softmax, and the backward
dS = scale * P o (dP - rowsum(dP o P)) with dP = dY g^T computed on the fly, against fp64 torch -- on the key
counts of the model (784: 32 x 224^2 clips, 1024: test crop 256), ragged query tiles and both 16-bit types."""
import numpy as np
import pytest
import torch

import attn_cases as ac
from gpu_util import dev, q, rel_err

pytestmark = pytest.mark.gpu

CASES = [(2, 200, 784, 256), (1, 128, 1024, 512), (3, 64, 520, 64), (1, 3136, 784, 256)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,L1,L2,Ci", CASES)
def test_fused_scores_softmax_forward_and_backward(B, L1, L2, Ci, dtype):
    from vlfb import hip
    hip.lib()
    code = hip.dtype_code(dtype)
    assert hip.lib().vlfb_attn_scores_supported(code, L1, L2, Ci) & hip.ATTN_CAN_RUN
    gen = torch.Generator().manual_seed(L1 * 7 + L2)
    theta = q(torch.randn(B, L1, Ci, generator=gen), dtype)
    phi = q(torch.randn(B, L2, Ci, generator=gen), dtype)
    scale = Ci ** -0.5
    th, ph = theta.to(dev(), dtype), phi.to(dev(), dtype)
    P = torch.full((B, L1, L2), float("nan"), device=dev(), dtype=dtype)
    hip.call("vlfb_attn_scores_fwd", hip.ptr(th), hip.ptr(ph), hip.ptr(P), code, B, L1, L2, Ci, scale)
    torch.cuda.synchronize()
    ref = torch.softmax(scale * torch.bmm(theta.double(), phi.double().transpose(1, 2)), dim=2)
    tol = 6e-3 if dtype == torch.bfloat16 else 8e-4
    assert rel_err(P.float(), ref) < tol
    assert float((P.float().sum(dim=2) - 1).abs().max()) < (2e-2 if dtype == torch.bfloat16 else 3e-3)
    # the composed path (GEMM -> fp32 scores -> softmax kernel) gives the same probabilities up to the last bit or two
    S = torch.empty(B, L1, L2, device=dev(), dtype=torch.float32)
    d = hip.conv_desc(mode=hip.FPROP, dtype=code, out_dtype=hip.F32, N=1, Tr=1, Hr=1, Wr=L1, Ts=1, Hs=1, Ws=L1, batch=B,
                      Cs=Ci, Cn=L2, a_bstride=L1 * Ci, b_bstride=L2 * Ci, o_bstride=L1 * L2)
    hip.conv_run(d, th, ph, None, S)
    P2 = torch.empty_like(P)
    hip.call("vlfb_softmax_fwd", hip.ptr(S), hip.ptr(P2), code, B * L1, L2, scale)
    torch.cuda.synchronize()
    assert rel_err(P.float(), P2.float()) < (2e-3 if dtype == torch.bfloat16 else 3e-4)
    # ---- backward ---------------------------------------------------------------------------------------------
    dY = q(torch.randn(B, L1, Ci, generator=gen), dtype)
    g = q(torch.randn(B, L2, Ci, generator=gen), dtype)
    dS = torch.full((B, L1, L2), float("nan"), device=dev(), dtype=dtype)
    dYd, gd = dY.to(dev(), dtype), g.to(dev(), dtype)       # named: a temporary would be freed before the launch runs
    hip.call("vlfb_attn_scores_bwd", hip.ptr(dYd), hip.ptr(gd), hip.ptr(P), hip.ptr(dS), code, B, L1, L2, Ci, scale)
    torch.cuda.synchronize()
    Pd = P.double().cpu()                                   # the probabilities the kernel saw
    dP = torch.bmm(dY.double(), g.double().transpose(1, 2))
    want = scale * Pd * (dP - (dP * Pd).sum(dim=2, keepdim=True))
    assert rel_err(dS.float(), want) < (6e-3 if dtype == torch.bfloat16 else 8e-4)


def test_unsupported_shapes_are_refused():
    from vlfb import hip
    hip.lib()
    assert hip.lib().vlfb_attn_scores_supported(hip.F32, 3136, 784, 256) == 0        # parity path keeps fp32 scores
    assert hip.lib().vlfb_attn_scores_supported(hip.BF16, 6272, 1568, 512) == 0      # 64-frame clips: 1568 keys
    assert hip.lib().vlfb_attn_scores_supported(hip.BF16, 784, 196, 256) == 0
    t = torch.zeros(64 * 1568, device=dev(), dtype=torch.bfloat16)
    with pytest.raises(hip.VlfbError):
        hip.call("vlfb_attn_scores_fwd", hip.ptr(t), hip.ptr(t), hip.ptr(t), hip.BF16, 1, 64, 1568, 64, 1.0)


# ----------------------------------------------------------------------------------------------------------------------
# Per-element tests over every tiling and edge: tests/attn_cases.py holds the cases, the fp64 references and the bounds
# (derived from operation counts; tests/test_attn_cases_host.py proves the conditions on them on the CPU).
# ----------------------------------------------------------------------------------------------------------------------
GUARD_ROWS = 64
NAN_BITS = 0x7FC1            # a NaN in bf16 and in fp16


def _sentinel(rows, cols, dtype):
    return torch.full((rows, cols), NAN_BITS, device=dev(), dtype=torch.int16).view(dtype)


def _guard_intact(t, rows):
    return bool((t.view(torch.int16)[rows:] == NAN_BITS).all())


def _check(what, kernel, shape, got, want, bound):
    """got within bound of want, elementwise; a failure names the element, its owner in the kernel and the ratio"""
    B, L1, L2, Ci = shape
    got = got.double().cpu().reshape(B, L1, L2)
    assert torch.isfinite(got).all(), "%s: %d non-finite elements" % (what, int((~torch.isfinite(got)).sum()))
    err = (got - want).abs()
    ratio, i = ac.worst(err, bound)
    b, qrow, key = i // (L1 * L2), (i // L2) % L1, i % L2
    print("%s %s %s: worst element at %.3f of its bound" % (what, kernel, ac.case_id(shape), ratio))
    assert ratio <= 1, "%s: element (b %d, q %d, k %d) = %r, want %r: %.2f of its bound %.3g; %d elements over; owner: %s" % (
        what, b, qrow, key, float(got[b, qrow, key]), float(want[b, qrow, key]), ratio, float(bound[b, qrow, key]),
        int((err > bound).sum()), ac.ownership(kernel, qrow, key))
    return ratio


def _forward(shape, gen, name):
    from vlfb import hip
    B, L1, L2, Ci = shape
    dtype = ac.DTYPES[name]
    code = hip.dtype_code(dtype)
    assert hip.lib().vlfb_attn_scores_supported(code, L1, L2, Ci) & hip.ATTN_CAN_RUN
    theta, phi, dY, g = (t.to(dev(), dtype) for t in ac.fused_inputs(shape, gen, name))
    P = _sentinel(B * L1 + GUARD_ROWS, L2, dtype)
    hip.call("vlfb_attn_scores_fwd", hip.ptr(theta), hip.ptr(phi), hip.ptr(P), code, B, L1, L2, Ci, Ci ** -0.5)
    torch.cuda.synchronize()
    return P, dY, g, code


def _backward(shape, P, dY, g, code, scale):
    from vlfb import hip
    B, L1, L2, Ci = shape
    dS = _sentinel(B * L1 + GUARD_ROWS, L2, P.dtype)
    hip.call("vlfb_attn_scores_bwd", hip.ptr(dY), hip.ptr(g), hip.ptr(P), hip.ptr(dS), code, B, L1, L2, Ci, scale)
    torch.cuda.synchronize()
    return dS


@pytest.mark.parametrize("name", ac.FUSED_DTYPES)
@pytest.mark.parametrize("gen", ac.FUSED_GENERATORS)
@pytest.mark.parametrize("case", ac.FUSED_CASES, ids=lambda c: c[0] + "-" + ac.case_id(c[1:]))
def test_fused_scores_per_element(case, gen, name):
    kernel, shape = case[0], case[1:]
    B, L1, L2, Ci = shape
    P, dY, g, code = _forward(shape, gen, name)
    pref, pbound = ac.fused_forward_ref(shape, gen, name)
    assert _guard_intact(P, B * L1), "the forward wrote behind row B * L1"
    _check("P %s %s" % (gen, name), kernel, shape, P[:B * L1], pref, pbound)
    rows = P[:B * L1].double().cpu().sum(dim=1)
    row_tol = L2 * (ac.U_OUT[name] * pref.reshape(B * L1, L2).max(dim=1).values + 2.0 ** -25)
    over = (rows - 1).abs() / row_tol
    assert float(over.max()) <= 1, "row %d sums to %r: %.2f of the allowed %g" % (
        int(over.argmax()), float(rows[over.argmax()]), float(over.max()), float(row_tol[over.argmax()]))
    if gen == "flat":       # every logit of a row is the same number in any summation order: one value everywhere
        assert bool((P[:B * L1] == P[0, 0]).all())
    # ---- backward on the probabilities just written
    scale = Ci ** -0.5
    dS = _backward(shape, P, dY, g, code, scale)
    assert _guard_intact(dS, B * L1), "the backward wrote behind row B * L1"
    assert _guard_intact(P, B * L1)
    want, dbound = ac.fused_backward_ref(shape, gen, name, P[:B * L1].float().cpu().reshape(B, L1, L2), scale)
    _check("dS %s %s" % (gen, name), kernel, shape, dS[:B * L1], want, dbound)


@pytest.mark.parametrize("gen", ["randn", "hot"])
@pytest.mark.parametrize("shape", ac.ENGINE_SCALE_SHAPES, ids=ac.case_id)
def test_fused_backward_at_the_engine_scale(shape, gen):
    """fp16: the engine stores dS times 16 << bit_length(L2 - 1) (16384 at 784 and at 1024 keys)"""
    B, L1, L2, Ci = shape
    kernel = ac.fused_kernel(L2, Ci)
    factor = ac.engine_ds_scale(L2)
    assert factor == float(16 << max(L2 - 1, 1).bit_length()) == 16384.0          # vlfb/engine.py, restated
    scale = Ci ** -0.5 * factor
    P, dY, g, code = _forward(shape, gen, "fp16")
    dS = _backward(shape, P, dY, g, code, scale)
    assert _guard_intact(dS, B * L1)
    want, bound = ac.fused_backward_ref(shape, gen, "fp16", P[:B * L1].float().cpu().reshape(B, L1, L2), scale)
    _check("dS x %g %s fp16" % (factor, gen), kernel, shape, dS[:B * L1], want, bound)


@pytest.mark.parametrize("name", ac.FUSED_DTYPES)
@pytest.mark.parametrize("gen", ["randn", "hot"])
@pytest.mark.parametrize("shape", ac.COMPOSED_SHAPES, ids=ac.case_id)
def test_fused_matches_composed_per_element(shape, gen, name):
    """the fused forward against vlfb_conv_run (fp32 scores) + vlfb_softmax_fwd: two independent roundings of nearly equal
    fp32 values, so at most twice the output term apart -- for each of the three kernels"""
    from vlfb import hip
    B, L1, L2, Ci = shape
    dtype = ac.DTYPES[name]
    P, _, _, code = _forward(shape, gen, name)
    theta, phi = (t.to(dev(), dtype) for t in ac.fused_inputs(shape, gen, name)[:2])
    S = torch.empty(B, L1, L2, device=dev(), dtype=torch.float32)
    d = hip.conv_desc(mode=hip.FPROP, dtype=code, out_dtype=hip.F32, N=1, Tr=1, Hr=1, Wr=L1, Ts=1, Hs=1, Ws=L1, batch=B,
                      Cs=Ci, Cn=L2, a_bstride=L1 * Ci, b_bstride=L2 * Ci, o_bstride=L1 * L2)
    hip.conv_run(d, theta, phi, None, S)
    P2 = torch.empty(B * L1, L2, device=dev(), dtype=dtype)
    hip.call("vlfb_softmax_fwd", hip.ptr(S), hip.ptr(P2), code, B * L1, L2, Ci ** -0.5)
    torch.cuda.synchronize()
    pref, _ = ac.fused_forward_ref(shape, gen, name)
    _check("fused - composed %s %s" % (gen, name), ac.fused_kernel(L2, Ci), shape, P[:B * L1].double().cpu() - P2.double().cpu().reshape(-1, L2),
           torch.zeros_like(pref), 2 * ac.out_term(pref, name))


def test_refusals_launch_nothing():
    from vlfb import hip
    B, L1, L2 = 1, 64, 784
    dtype, code = torch.bfloat16, hip.BF16
    ops = torch.ones(max(L2, L1) * 1088, device=dev(), dtype=dtype)       # large enough for every shape below
    prob = torch.full((B * L1, L2), 1.0 / L2, device=dev(), dtype=dtype)
    out = _sentinel(B * L1 + GUARD_ROWS, L2, dtype)
    for l1, ci, scale in ((64, 256, 0.0), (64, 256, -0.0625), (63, 256, 0.0625), (64, 1088, 0.0625), (64, 256, float("nan"))):
        with pytest.raises(hip.VlfbError):
            hip.call("vlfb_attn_scores_fwd", hip.ptr(ops), hip.ptr(ops), hip.ptr(out), code, B, l1, L2, ci, scale)
        with pytest.raises(hip.VlfbError):
            hip.call("vlfb_attn_scores_bwd", hip.ptr(ops), hip.ptr(ops), hip.ptr(prob), hip.ptr(out), code, B, l1, L2, ci, scale)
        torch.cuda.synchronize()
        assert _guard_intact(out, 0), "a refused call wrote to its output (l1 %d, ci %d, scale %r)" % (l1, ci, scale)
