"""The FBO attention core (vlfb_fbo_attn_fwd / _fwd_shared / _bwd, csrc/vlfb_head.hip) per element against fp64, on both
kernel paths, with a row stride ld > D, short banks (K < 32, K = 1, K % 8 != 0) and a single row.  Cases, references and
bounds: tests/attn_cases.py (conditions on them: tests/test_attn_cases_host.py).  The padding columns of the inputs hold a
finite sentinel -- a kernel that read them would give a wrong dot product, not a NaN something might mask -- and everything
behind and between the outputs holds another, which must survive bit for bit."""
import pytest
import torch

import attn_cases as ac
from gpu_util import dev
from vlfb import hip

pytestmark = pytest.mark.gpu

GUARD = -77.0
GUARD_ROWS = 2


def strided(x, ld, dtype):
    """(R, K, D) CPU values -> (R, K, ld) device tensor of the type, padding columns = ac.PAD"""
    R, K, D = x.shape
    out = torch.full((R, K, ld), ac.PAD, dtype=torch.float32)
    out[:, :, :D] = x
    return out.to(dev(), dtype)


def guarded(rows, cols, dtype):
    return torch.full((rows + GUARD_ROWS, cols), GUARD, device=dev(), dtype=dtype)


def untouched(t):
    return bool((t == GUARD).all())


def check(what, got, want, bound):
    got = got.double().cpu()
    assert torch.isfinite(got).all(), "%s: non-finite elements" % what
    err = (got - want).abs()
    ratio, i = ac.worst(err, bound)
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), want.shape))
    assert ratio <= 1, "%s%r = %r, want %r: %.2f of its bound %.3g; %d elements over" % (
        what, idx, float(got[idx]), float(want[idx]), ratio, float(bound[idx]), int((err > bound).sum()))
    return ratio


@pytest.mark.parametrize("gen", ac.FBO_GENERATORS)
@pytest.mark.parametrize("case", ac.FBO_CASES, ids=lambda c: "%s-%s-%s" % (c[0], c[1], ac.case_id(c[2:])))
def test_fbo_forward_backward_per_element(case, gen):
    path, name, shape = case[0], case[1], case[2:]
    R, K, D, ld = shape
    dtype = ac.DTYPES[name]
    code = hip.dtype_code(dtype)
    theta, phi, g, dt = ac.fbo_inputs(shape, gen, name)
    scale = D ** -0.5
    TH, DT = theta.to(dev(), dtype), dt.to(dev(), dtype)
    PH, G = strided(phi, ld, dtype), strided(g, ld, dtype)
    P, T = guarded(R, K, torch.float32), guarded(R, D, dtype)
    hip.call("vlfb_fbo_attn_fwd", hip.ptr(TH), hip.ptr(PH), hip.ptr(G), hip.ptr(P), hip.ptr(T), code, R, K, D, ld, scale)
    torch.cuda.synchronize()
    p, pb, t, tb = ac.fbo_forward_ref(shape, gen, name)
    assert untouched(P[R:]) and untouched(T[R:]), "the forward wrote behind its outputs"
    ratios = {"p": check("p", P[:R], p, pb), "t": check("t", T[:R], t, tb)}
    # ---- backward on the probabilities just written
    DTH, DSW = guarded(R, D, dtype), guarded(R, K, torch.float32)
    DPH = torch.full((R * K + GUARD_ROWS, ld), GUARD, device=dev(), dtype=dtype)
    DG = torch.full((R * K + GUARD_ROWS, ld), GUARD, device=dev(), dtype=dtype)
    hip.call("vlfb_fbo_attn_bwd", hip.ptr(DT), hip.ptr(TH), hip.ptr(PH), hip.ptr(G), hip.ptr(P), hip.ptr(DTH), hip.ptr(DPH),
             hip.ptr(DG), hip.ptr(DSW), code, R, K, D, ld, scale)
    torch.cuda.synchronize()
    assert untouched(P[R:]) and untouched(DTH[R:]) and untouched(DSW[R:]) and untouched(DPH[R * K:]) and untouched(DG[R * K:]), \
        "the backward wrote behind its outputs"
    assert untouched(DPH[:, D:]) and untouched(DG[:, D:]), "the backward wrote into the padding columns of dphi / dg"
    assert torch.equal(PH[:, :, D:], torch.full_like(PH[:, :, D:], ac.PAD)) and torch.equal(G[:, :, D:], torch.full_like(G[:, :, D:], ac.PAD))
    refs = ac.fbo_backward_ref(shape, gen, name, P[:R].cpu())
    got = {"ds_ws": DSW[:R], "dtheta": DTH[:R], "dphi": DPH[:R * K, :D].reshape(R, K, D), "dg": DG[:R * K, :D].reshape(R, K, D)}
    for key, (want, bound) in refs.items():
        ratios[key] = check(key, got[key], want, bound)
    print("%s %s %s %s: worst elements at %s of their bounds" % (
        path, name, ac.case_id(shape), gen, " ".join("%s %.3f" % kv for kv in ratios.items())))


@pytest.mark.parametrize("name", list(ac.DTYPES))
@pytest.mark.parametrize("shape", ac.SHARED_SHAPES, ids=ac.case_id)
def test_fbo_shared_banks_with_row_stride(shape, name):
    """NB = 3 banks with ld > D read through an unsorted owner column (stride 5, as in a RoI table): per element against fp64
    on the bank each row owns, and bit-identical to vlfb_fbo_attn_fwd on the duplicated banks"""
    R, K, D, ld = shape
    dtype = ac.DTYPES[name]
    code = hip.dtype_code(dtype)
    theta, phi, g, _ = ac.fbo_inputs(shape, "randn", name, ac.SHARED_NB)
    own = torch.tensor(ac.SHARED_OWNER)
    rois = torch.full((R, 5), 3.0)
    rois[:, 0] = own.float()
    scale = D ** -0.5
    TH, RO = theta.to(dev(), dtype), rois.to(dev())
    PH, G = strided(phi, ld, dtype), strided(g, ld, dtype)
    P, T = guarded(R, K, torch.float32), guarded(R, D, dtype)
    hip.call("vlfb_fbo_attn_fwd_shared", hip.ptr(TH), hip.ptr(PH), hip.ptr(G), hip.ptr(P), hip.ptr(T), code, R, K, D, ld, scale,
             hip.ptr(RO), 5)
    torch.cuda.synchronize()
    p, pb, t, tb = ac.fbo_shared_ref(shape, "randn", name)
    assert untouched(P[R:]) and untouched(T[R:])
    check("p", P[:R], p, pb)
    check("t", T[:R], t, tb)
    PH2, G2 = strided(phi[own], ld, dtype), strided(g[own], ld, dtype)
    P2, T2 = guarded(R, K, torch.float32), guarded(R, D, dtype)
    hip.call("vlfb_fbo_attn_fwd", hip.ptr(TH), hip.ptr(PH2), hip.ptr(G2), hip.ptr(P2), hip.ptr(T2), code, R, K, D, ld, scale)
    torch.cuda.synchronize()
    assert torch.equal(P, P2) and torch.equal(T, T2)
