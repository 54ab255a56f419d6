"""Conditions on the RoI case table of tests/roi_cases.py, checked on the CPU: the two oracle restatements agree on these
boxes, the table reaches every branch it claims to, the forward bound holds for the fp32 oracle itself, and the feature
generators produce the ties (and no near ties) the GPU tests rely on."""
import numpy as np
import pytest

import roi_cases as rc
from oracle.roi_align import roi_align_loop, roi_align_vec, roi_decisions


def test_loop_and_vectorised_oracles_agree_on_the_table():
    feat = rc.features("fp32", "randn", 8)
    for pooled in (7, 3, 2):
        a, da = roi_align_loop(feat, rc.ROIS, pooled, rc.SCALE)
        b, db = roi_align_vec(feat, rc.ROIS, pooled, rc.SCALE)
        assert np.array_equal(da, db)
        assert np.abs(a - b).max() <= 1e-6


def test_table_reaches_what_it_claims():
    gh, gw = rc.grids(rc.ROIS, rc.POOLED)
    assert list(zip(gh.tolist(), gw.tolist())) == rc.GRIDS
    assert sorted(set(rc.ROIS[:, 0].astype(int).tolist())) == list(range(rc.N))      # every clip has a RoI, none invalid
    assert (np.diff(rc.ROIS[:, 0]) < 0).any()                                         # ... and they are not sorted by clip
    d = roi_decisions(rc.ROIS, rc.H, rc.W, rc.POOLED, rc.SCALE, max_grid=4)           # (R,7,7,4,4,8)
    inside = d[..., 7].reshape(rc.R, -1)
    n_in, n_out = (inside == 1).sum(axis=1), (inside == 0).sum(axis=1)
    assert ((n_in > 0) & (n_out > 0)).any(), "a RoI with samples on both sides of the inside predicate"
    assert n_in[rc.WHOLLY_OUTSIDE] == 0 and n_out[rc.WHOLLY_OUTSIDE] > 0, "a RoI with no inside sample at all"
    assert ((n_in == 0) & (n_out > 0)).sum() == 1
    assert 3 in d[..., 1] and 4 in d[..., 2], "a grid of 3 and a grid of 4"
    ok = d[..., 7] == 1
    yl, xl, yh, xh = d[..., 3], d[..., 4], d[..., 5], d[..., 6]
    assert (ok & (yl == rc.H - 1) & (yh == yl)).any(), "clamp at H-1"
    assert (ok & (xl == rc.W - 1) & (xh == xl)).any(), "clamp at W-1"
    assert (ok & (yl == 0)).any() and (ok & (xl == 0)).any()
    # three overlapping RoIs in one clip (the backward adds them into the same pixels)
    assert (rc.ROIS[:, 0] == 0).sum() >= 3


def test_channel_table_gives_the_row_groups_it_claims():
    for name, table in rc.CHANNELS.items():
        for c, gr in table.items():
            assert c % rc.VEC[name] == 0 and c // rc.VEC[name] <= 1024
            assert rc.row_groups(name, c) == gr
    # trailing groups that scan nothing: rows_per = ceil(7 / gr) = 2 leaves groups 4 (and 5) empty
    assert {gr for t in rc.CHANNELS.values() for gr in t.values()} >= {1, 2, 3, 4, 5, 6, 7}
    assert rc.row_groups("fp32", 32, 3) == 3 and rc.row_groups("fp32", 32, 2) == 2


@pytest.mark.parametrize("gen", rc.GENERATORS)
@pytest.mark.parametrize("name", list(rc.DTYPES))
def test_fp32_oracle_is_within_the_forward_bound(name, gen):
    rf = rc.ref(name, gen, rc.CMAX[name])
    err = np.abs(rf.ref32.astype(np.float64) - rf.ref64)
    assert (err <= rf.fwd_bound).all()
    nz = rf.fwd_bound > 0
    print("%s %s: fp32 oracle at %.3f of fwd_bound" % (name, gen, (err[nz] / rf.fwd_bound[nz]).max()))
    assert (rf.ref32[rc.WHOLLY_OUTSIDE] == 0).all() and (rf.arg[rc.WHOLLY_OUTSIDE] == 0).all()


@pytest.mark.parametrize("name", list(rc.DTYPES))
def test_tie_conditions(name):
    s = rc.tie_stats(rc.ref(name, "randn", rc.CMAX[name]))
    print("%s randn: %s" % (name, s))
    assert s["near"] <= 0.01
    s = rc.tie_stats(rc.ref(name, "neg_relu", rc.CMAX[name]))
    print("%s neg_relu: %s" % (name, s))
    assert s["exact_not_bin0"] >= 0.30
    assert s["exact_row1"] >= 0.10


def test_backward_bound_holds_for_fp32_autograd():
    import torch
    from oracle.roi_align import roi_align_torch
    rf = rc.ref("fp32", "randn", 32)
    do = rc.dout("fp32", 32)
    gf, s, bound = rc.backward_ref(rf.feat, rc.ROIS, rf.arg, do)
    f32 = torch.from_numpy(rf.feat).requires_grad_(True)
    bins = roi_align_torch(f32, rc.ROIS, rc.POOLED, rc.SCALE).reshape(rc.R, 32, 49)
    sel = bins.gather(2, torch.from_numpy(rf.arg).unsqueeze(2)).squeeze(2)
    (g32,) = torch.autograd.grad(sel, (f32,), do)
    err = np.abs(g32.numpy().astype(np.float64) - gf)
    assert (err <= bound).all()
    assert (s == 0).any() and (g32.numpy()[s == 0] == 0).all()
    print("fp32 autograd at %.4f of bwd_bound, M = %d" % ((err[s > 0] / bound[s > 0]).max(), rc.bwd_ops(rc.ROIS, 7)))
