"""Per-element tests of the RoI head kernels (vlfb_roi_align_max_fwd / _bwd / _decisions, csrc/vlfb_roi.hip) on the case
table of tests/roi_cases.py: a non-square map, boxes outside / across / beyond the image, exact ties for the maximum, every
row-group count the host code can derive, and bounds derived from the kernel's operation count (roi_cases.py docstring).

Every comparison is per (RoI, channel) or per pixel; each test prints its largest |error| / bound before it asserts."""
import functools

import numpy as np
import pytest
import torch

import roi_cases as rc
from gpu_util import dev

pytestmark = pytest.mark.gpu

hip = None


def setup_module(module):
    from vlfb import hip as h
    module.hip = h
    h.lib()


def _ids(case):
    return "-".join(str(v) for v in case)


def _launch_fwd(feat, name, rois, pooled, with_dbg=False):
    """feat (N,C,H,W) fp32 numpy (already rounded through the dtype) -> O (R,C) fp64 numpy, AB (R,C) int64 numpy, dbg"""
    dtype = rc.DTYPES[name]
    n, c, h, w = feat.shape
    r = rois.shape[0]
    fg = torch.from_numpy(feat).permute(0, 2, 3, 1).contiguous().to(dev()).to(dtype)          # [N,H,W,C]
    rg = torch.from_numpy(rois).to(dev())
    out = torch.full((r, c), float("nan"), device=dev(), dtype=dtype)
    ab = torch.full((r, c), 255, device=dev(), dtype=torch.uint8)
    dbg = torch.full((r, pooled, pooled, 8), -7, device=dev(), dtype=torch.int32) if with_dbg else None
    hip.call("vlfb_roi_align_max_fwd", hip.ptr(fg), hip.dtype_code(dtype), hip.ptr(rg), hip.ptr(out), hip.ptr(ab),
             hip.ptr(dbg), n, h, w, c, r, pooled, rc.SCALE)
    torch.cuda.synchronize()
    return out.cpu(), ab.cpu(), (dbg.cpu().numpy() if with_dbg else None)


@functools.lru_cache(maxsize=None)
def _fwd(name, c, gen):
    out, ab, dbg = _launch_fwd(rc.ref(name, gen, c).feat, name, rc.ROIS, rc.POOLED, with_dbg=True)
    return out.double().numpy(), ab.long().numpy(), dbg


def _launch_bwd(do, name, rois, arg, c, pooled):
    """do (R,C) fp32 torch (rounded through the dtype), arg (R,C) ints -> dfeat (N,C,H,W) fp32 torch on the CPU"""
    dtype = rc.DTYPES[name]
    r = rois.shape[0]
    dg = do.to(dev()).to(dtype)
    rg = torch.from_numpy(rois).to(dev())
    ag = torch.from_numpy(arg.astype(np.uint8)).to(dev())
    df = torch.zeros(rc.N, rc.H, rc.W, c, device=dev(), dtype=torch.float32)
    hip.call("vlfb_roi_align_max_bwd", hip.ptr(dg), hip.dtype_code(dtype), hip.ptr(rg), hip.ptr(ag), hip.ptr(df),
             rc.N, rc.H, rc.W, c, r, pooled, rc.SCALE)
    torch.cuda.synchronize()
    return df.cpu().permute(0, 3, 1, 2).contiguous()


def _check_forward(name, rf, out, ab):
    """the assertions of tests 2 and 3 on one forward result; returns the largest |error| / bound"""
    r, c = ab.shape
    assert np.isfinite(out).all() and ab.min() >= 0 and ab.max() < rf.pooled ** 2
    # first maximal bin of the fp32 oracle, exactly: ties, every group count
    want = rf.arg
    bad = np.argwhere(ab != want)
    assert bad.size == 0, "argbin differs from the first fp32 argmax at %d of %d (RoI, channel) pairs, first %s: got %d want %d" % (
        len(bad), r * c, bad[0], ab[tuple(bad[0])], want[tuple(bad[0])])
    # values, per element
    err = np.abs(out - rf.ref64_at_arg)
    bound = rf.out_bound(name)
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert (err <= bound).all(), "O off by %.3e > bound %.3e at (RoI, channel) %s" % (err[worst], bound[worst], worst)
    return ratio


# ------------------------------------------------------------------------------------------------------------ 1. decisions
def test_decisions_of_every_sample_match_the_oracle():
    from oracle.roi_align import roi_decisions
    rg = torch.from_numpy(rc.ROIS).to(dev())
    got = torch.full((rc.R, 7, 7, 4, 4, 8), -7, device=dev(), dtype=torch.int32)
    hip.call("vlfb_roi_align_decisions", hip.ptr(rg), hip.ptr(got), rc.H, rc.W, rc.R, 7, rc.SCALE, 4)
    torch.cuda.synchronize()
    want = roi_decisions(rc.ROIS, rc.H, rc.W, 7, rc.SCALE, max_grid=4)
    assert want[..., 1].max() == 3 and want[..., 2].max() == 4
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("name", list(rc.DTYPES))
def test_forward_dbg_matches_the_oracle(name):
    _, _, dbg = _fwd(name, 32, "randn")
    assert np.array_equal(dbg, rc.ref(name, "randn", 32).dbg)


# --------------------------------------------------------------------------------------------------- 2. forward values
@pytest.mark.parametrize("case", rc.FWD_CASES, ids=_ids)
def test_forward_values_per_element(case):
    name, c, gen = case
    rf = rc.ref(name, gen, c)
    out, ab, _ = _fwd(name, c, gen)
    sel = np.take_along_axis(rf.ref64, rf.arg[:, :, None], 2)[:, :, 0]
    err = np.abs(out - sel)
    bound = rf.out_bound(name)
    nz = bound > 0
    print("forward %s C=%d gr=%d %s: max |error| / bound = %.4f" % (name, c, rc.row_groups(name, c), gen,
                                                                     (err[nz] / bound[nz]).max()))
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert (err <= bound).all(), "O off by %.3e > bound %.3e at (RoI, channel) %s" % (err[worst], bound[worst], worst)
    # the wholly-outside RoI: every sample skipped -> exactly 0, bin 0
    assert (out[rc.WHOLLY_OUTSIDE] == 0).all() and (ab[rc.WHOLLY_OUTSIDE] == 0).all()


# ------------------------------------------------------------------------------------------------------------ 3. argbin
@pytest.mark.parametrize("case", rc.FWD_CASES, ids=_ids)
def test_argbin_is_the_first_maximal_bin(case):
    """The kernel accumulates in fp32 in the operation order of roi_align_loop (the file is built with -ffp-contract=off),
    so argbin equals the first argmax of the fp32 oracle exactly -- every tie, every group count, every dtype."""
    name, c, gen = case
    rf = rc.ref(name, gen, c)
    _, ab, _ = _fwd(name, c, gen)
    assert ab.min() >= 0 and ab.max() < 49
    # the weaker rule no rounding can excuse: the chosen bin is maximal in fp64 up to twice the forward bound
    at = np.take_along_axis(rf.ref64, ab[:, :, None], 2)[:, :, 0]
    assert (at >= rf.ref64.max(axis=2) - 2 * rf.fwd_bound_max).all()
    want = rf.arg
    bad = np.argwhere(ab != want)
    print("argbin %s C=%d gr=%d %s: %d of %d differ" % (name, c, rc.row_groups(name, c), gen, len(bad), ab.size))
    assert bad.size == 0, "argbin differs from the first fp32 argmax at %d of %d pairs, first (RoI, channel) %s: got %d want %d" % (
        len(bad), ab.size, bad[0], ab[tuple(bad[0])], want[tuple(bad[0])])


# ----------------------------------------------------------------------------------------------------------- 4. backward
@pytest.mark.parametrize("c", [32, 2048])
@pytest.mark.parametrize("name", list(rc.DTYPES))
def test_backward_per_pixel(name, c):
    """dfeat against fp64 autograd through roi_align_torch, per pixel.  argbin is the oracle's (what test 3 establishes
    the forward writes); clip 0 has five overlapping RoIs and the table is not sorted by clip."""
    rf = rc.ref(name, "neg_relu", c)
    do = rc.dout(name, c)
    gf, s, bound = rc.backward_ref(rf.feat, rc.ROIS, rf.arg, do)
    df = _launch_bwd(do, name, rc.ROIS, rf.arg, c, rc.POOLED).double().numpy()
    err = np.abs(df - gf)
    print("backward %s C=%d: max |error| / bound = %.4f, %d of %d pixels untouched" % (
        name, c, (err[s > 0] / bound[s > 0]).max(), (s == 0).sum(), s.size))
    assert (s == 0).any() and (s > 0).any()
    assert (df[s == 0] == 0).all(), "a pixel no sample reaches must stay exactly 0"
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert (err <= bound).all(), "dfeat off by %.3e > bound %.3e at (n, c, y, x) %s" % (err[worst], bound[worst], worst)


# -------------------------------------------------------------------------------------------------------- 5. determinism
@pytest.mark.parametrize("name,c", [("fp32", 800), ("bf16", 2048), ("fp16", 1600)])
def test_two_launches_are_bit_identical(name, c):
    rf = rc.ref(name, "neg_relu", c)
    o1, a1, _ = _launch_fwd(rf.feat, name, rc.ROIS, rc.POOLED)
    o2, a2, _ = _launch_fwd(rf.feat, name, rc.ROIS, rc.POOLED)
    assert torch.equal(o1, o2) and torch.equal(a1, a2)
    do = rc.dout(name, c)
    d1 = _launch_bwd(do, name, rc.ROIS, rf.arg, c, rc.POOLED)
    d2 = _launch_bwd(do, name, rc.ROIS, rf.arg, c, rc.POOLED)
    assert torch.equal(d1, d2) and d1.abs().sum() > 0


# ------------------------------------------------------------------------------------------------- 6. other pooled values
@pytest.mark.parametrize("pooled", [3, 2])
@pytest.mark.parametrize("name", list(rc.DTYPES))
def test_other_pooled_resolutions(name, pooled):
    """gr clamped to pooled (3 and 2 groups of one row); the boxes sample on grids up to 9 x 14"""
    c = 32
    rf = rc.ref_pooled(name, "neg_relu", c, pooled)
    assert rc.row_groups(name, c, pooled) == pooled
    out, ab, dbg = _launch_fwd(rf.feat, name, rc.ROIS, pooled, with_dbg=True)
    assert np.array_equal(dbg, rf.dbg)
    ratio = _check_forward(name, rf, out.double().numpy(), ab.long().numpy())
    do = rc.dout(name, c)
    gf, s, bound = rc.backward_ref(rf.feat, rc.ROIS, rf.arg, do, pooled)
    df = _launch_bwd(do, name, rc.ROIS, rf.arg, c, pooled).double().numpy()
    err = np.abs(df - gf)
    print("pooled %d %s: forward %.4f, backward %.4f of the bound" % (pooled, name, ratio, (err[s > 0] / bound[s > 0]).max()))
    assert (df[s == 0] == 0).all() and (err <= bound).all()


# ----------------------------------------------------------------------------------------------------------- 7. rejections
@pytest.mark.parametrize("what,name,code,c,r,pooled", [
    ("C % V != 0 (fp32)", "fp32", None, 30, 4, 7),
    ("C % V != 0 (16-bit)", "bf16", None, 36, 4, 7),
    ("pooled = 16: 256 bins", "fp32", None, 32, 4, 16),
    ("more than 1024 channel chunks (fp32)", "fp32", None, 4100, 4, 7),
    ("more than 1024 channel chunks (16-bit)", "fp16", None, 8200, 4, 7),
    ("r = 0", "fp32", None, 32, 0, 7),
    ("bad dtype code", "fp32", 99, 32, 4, 7),
], ids=lambda v: v if isinstance(v, str) and " " in v else None)
def test_rejected_calls_launch_nothing(what, name, code, c, r, pooled):
    """every buffer is large enough for the call as stated, so that a launch that should not have happened shows as
    overwritten sentinels, never as an access outside a buffer"""
    dtype = rc.DTYPES[name]
    rows = 4
    fg = torch.zeros(rc.N, rc.H, rc.W, c, device=dev(), dtype=dtype)
    rg = torch.from_numpy(rc.ROIS[:rows].copy()).to(dev())
    out = torch.full((rows, c), 12345.0, device=dev(), dtype=dtype)
    ab = torch.full((rows, c), 201, device=dev(), dtype=torch.uint8)
    out0, ab0 = out.clone(), ab.clone()
    with pytest.raises(hip.VlfbError):
        hip.call("vlfb_roi_align_max_fwd", hip.ptr(fg), hip.dtype_code(dtype) if code is None else code, hip.ptr(rg),
                 hip.ptr(out), hip.ptr(ab), None, rc.N, rc.H, rc.W, c, r, pooled, rc.SCALE)
    torch.cuda.synchronize()
    assert torch.equal(out, out0) and torch.equal(ab, ab0), what
