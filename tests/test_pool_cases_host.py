"""Conditions on the pool case table of tests/pool_cases.py, checked on the CPU: the reference agrees with torch's own
pooling in fp64 (values, first-maximum indices, gradients), every case reports the backward route the table names
(vlfb_maxpool_bwd_describe: a host function, no GPU), the generators produce the exact ties the GPU tests rely on, and the
descriptor checks of the pool entry points reject what they should and nothing the model builds."""
import ctypes as C
import itertools

import pytest
import torch
import torch.nn.functional as F

import pool_cases as pc

ALL_MAX = pc.MAX_CASES + pc.MIX_CASES


def hip_lib():
    import os
    from vlfb import hip
    if not os.path.exists(hip.LIB_PATH):
        pytest.skip("libvlfb_hip.so not built (run __graft_entry__.build())")
    return hip, hip.lib()


def ncthw(t):
    return t.permute(0, 4, 1, 2, 3).contiguous()


def nthwc(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def case_inputs(case, dtype_name, gen):
    if case in pc.MIX_CASES:
        g = pc._gen(case.name, gen)
        hi, _ = pc.pair_split(pc.values(gen, tuple(case.shape) + (case.C,), None, g))
        return hi
    return pc.max_data(case.name, dtype_name, gen).x


# ------------------------------------------------------------------------------------------------
# the reference against torch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.MAX_CASES, ids=lambda c: c.name)
def test_max_reference_equals_torch_in_fp64(case):
    """values and indices on every generator (torch's CPU kernel keeps the first maximum too); the backward emulation
    against autograd in fp64 on `randn`, to one output rounding plus the fp32 roundings of the (at most 8) additions"""
    (kt, kh, kw), s, p = case.k, case.s, case.p
    N, T, H, W = case.shape
    To, Ho, Wo = pc.out_dims(case)
    to = torch.arange(To).view(1, 1, To, 1, 1)
    ho = torch.arange(Ho).view(1, 1, 1, Ho, 1)
    wo = torch.arange(Wo).view(1, 1, 1, 1, Wo)
    for dtype_name, gen in itertools.product(case.dtypes, pc.GENERATORS):
        d = pc.max_data(case.name, dtype_name, gen)
        xd = ncthw(d.x.double()).requires_grad_(True)
        y_ref, idx = F.max_pool3d(xd, case.k, s, p, return_indices=True)
        assert tuple(y_ref.shape[2:]) == (To, Ho, Wo)
        assert torch.equal(ncthw(d.y.double()), y_ref.detach()), (dtype_name, gen)
        ti, hi, wi = idx // (H * W), (idx // W) % H, idx % W
        tap = ((ti - (to * s[0] - p[0])) * kh + (hi - (ho * s[1] - p[1]))) * kw + (wi - (wo * s[2] - p[2]))
        assert torch.equal(ncthw(d.tap), tap), (dtype_name, gen)
        if gen != "randn":
            continue
        dy = ncthw(d.dy.double())
        (gx,) = torch.autograd.grad(y_ref, (xd,), dy, retain_graph=True)
        (sabs,) = torch.autograd.grad(y_ref, (xd,), dy.abs())
        gx, sabs = nthwc(gx), nthwc(sabs)
        m = -(-kt // s[0]) * -(-kh // s[1]) * -(-kw // s[2])                # covering windows of one position, at most
        for combo in ("none", "add", "mask", "add_mask"):
            ref, mag = gx, sabs
            if "add" in combo:
                ref, mag = ref + d.add.double(), mag + d.add.double().abs()
            if "mask" in combo:
                ref = torch.where(d.mask.double() > 0, ref, torch.zeros_like(ref))
            got = pc.max_bwd_combo(case, d, combo).double()
            bound = (m + 1) * pc.U32 * mag + (0.5 * pc.ulp(ref, dtype_name) if dtype_name != "fp32" else 0.5 * pc.ulp(ref, "fp32"))
            assert ((got - ref).abs() <= bound).all(), (dtype_name, combo)


@pytest.mark.parametrize("case", pc.MIX_CASES, ids=lambda c: c.name)
def test_pair_reference_equals_torch_on_hi_plus_lo(case):
    for gen in pc.MIX_GENERATORS:
        g = pc._gen(case.name, gen)
        hi, lo = pc.pair_split(pc.values(gen, tuple(case.shape) + (case.C,), None, g))
        (yh, yl), tap = pc.max_fwd(hi, case, lo=lo)
        v = hi.float() + lo.float()
        y_ref = F.max_pool3d(ncthw(v.double()), case.k, case.s, case.p)
        assert torch.equal(ncthw(yh.double() + yl.double()), y_ref)
        y1, tap1 = pc.max_fwd(v, case)
        assert torch.equal(tap, tap1) and torch.equal(yh.float() + yl.float(), y1)


def test_avg_reference_equals_torch_in_fp64():
    for case in pc.AVG_CASES:
        g = pc._gen(case.name)
        x = torch.randn(tuple(case.shape) + (case.C,), generator=g, dtype=torch.float64)
        xd = ncthw(x).requires_grad_(True)
        y_ref = F.avg_pool3d(xd, case.k, case.s)
        mean, bound = pc.avg_fwd(x, case)
        assert (nthwc(y_ref.detach()) - mean).abs().max() < 1e-14 and (bound > 0).all()
        # the fp32-ordered emulation the GPU test compares bit for bit lies inside the bound, plain and on hi + lo planes
        hi, lo = pc.pair_split(x.float())
        for emu, (ref, bound) in ((pc.avg_fwd_emulated(x.float(), case), pc.avg_fwd(x.float(), case)),
                                  (pc.avg_fwd_emulated(hi, case, lo=lo), pc.avg_fwd(hi, case, lo=lo))):
            assert emu.dtype == torch.float32 and ((emu.double() - ref).abs() <= bound).all(), case.name
        dy = torch.randn(mean.shape, generator=g, dtype=torch.float64)
        (gx,) = torch.autograd.grad(y_ref, (xd,), ncthw(dy))
        dx, _ = pc.avg_bwd(case, dy)
        assert (nthwc(gx) - dx).abs().max() < 1e-14
        if case.one_window:
            v, hi, lo = pc.avg_bwd_one_window(case, dy.float(), torch.float16)
            ref, bound = pc.avg_bwd(case, dy.float())
            assert ((v.double() - ref).abs() <= bound).all()
            assert ((hi.double() - ref).abs() <= bound + 0.5 * pc.ulp(ref, "fp16")).all()


# ------------------------------------------------------------------------------------------------
# routes
# ------------------------------------------------------------------------------------------------
def describe(hip, lib, case, dtype_name, combo):
    N, T, H, W = case.shape
    To, Ho, Wo = pc.out_dims(case)
    d = hip.pool_desc(hip.dtype_code(pc.DTYPES[dtype_name]), N, T, H, W, case.C, To, Ho, Wo, case.k, case.s, case.p)
    buf = C.create_string_buffer(64)
    rc = lib.vlfb_maxpool_bwd_describe(C.byref(d), int("add" in combo or combo == "alias"), int("mask" in combo),
                                       int(combo == "relu"), buf, 64)
    assert rc == 0, lib.vlfb_last_error().decode()
    return buf.value.decode()


def test_every_case_reports_the_route_the_table_names():
    hip, lib = hip_lib()
    reached = set()
    for case in ALL_MAX:
        for dtype_name, combo in itertools.product(case.dtypes, case.combos):
            route = describe(hip, lib, case, dtype_name, combo)
            assert route == pc.expected_route(case, dtype_name, combo), (case.name, dtype_name, combo)
            words = [w for w in route.split() if w not in pc.ROUTE_DT.values() and not w.startswith("bands=")]
            reached.add(" ".join(words))
    print("routes reached: %s" % sorted(reached))
    assert reached >= set(pc.ALL_ROUTES), sorted(set(pc.ALL_ROUTES) - reached)
    assert len(pc.ALL_ROUTES) == 8
    # the wrapper of the binding says the same
    case = pc.MAX_BY_NAME["band_r3"]
    N, T, H, W = case.shape
    d = hip.pool_desc(hip.F16, N, T, H, W, case.C, *pc.out_dims(case), case.k, case.s, case.p)
    assert hip.maxpool_bwd_route(d) == "band f16 R=3 bands=3" and hip.maxpool_bwd_route(d, add=True) == "fixed 1x3x3/1x2x2 f16"
    assert hip.maxpool_bwd_route(d, y=True) == "band f16 R=3 bands=3 ymask"


def test_table_loops_take_more_than_one_trip():
    """what the shapes are for: the loops of the row and band kernels iterate more than once, on chunk counts that are no
    power of two"""
    c = pc.MAX_BY_NAME["band_r3"]
    Wo = pc.out_dims(c)[2]
    assert [(3 + 2) * Wo * (c.C // v) for v in (8, 4)] == [540, 1080] and c.C // 8 == 9
    assert -(-c.shape[2] // 6) == 3 and c.shape[2] - 2 * 6 == 1                      # three bands, one row in the last
    assert pc.MAX_BY_NAME["row_133_addmask"].shape[3] * (c.C // 8) > 128
    c = pc.MAX_BY_NAME["temporal_odd"]
    assert [c.shape[3] * (c.C // v) for v in (8, 4)] == [144, 288] and c.shape[1] % 2 == 1
    c = pc.MAX_BY_NAME["nl_odd"]
    assert [c.shape[3] * (c.C // v) for v in (8, 4)] == [153, 306] and c.shape[2] % 2 == 1 and c.shape[3] % 2 == 1
    cov = pc.covered(c)
    assert not cov[:, -1, :].any() and not cov[:, :, -1].any() and cov[:, :-1, :-1].all()
    cov = pc.covered(pc.MAX_BY_NAME["temporal_odd"])
    assert not cov[4].any() and cov[:4].all()


# ------------------------------------------------------------------------------------------------
# ties: conditions on the inputs, not measurements
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_MAX, ids=lambda c: c.name)
def test_tie_conditions(case):
    taps = case.k[0] * case.k[1] * case.k[2]
    gens = ("levels", "relu_levels") if case in pc.MAX_CASES else ("relu_levels",)
    for dtype_name, gen in itertools.product(case.dtypes, gens):
        x = case_inputs(case, dtype_name, gen)
        st = pc.tie_stats(case, x)
        print("%s %s %s: %s" % (case.name, dtype_name, gen, st))
        assert st["tied_pos"] >= 0.05
        if taps > 2:
            assert st["not_tap0"] >= 0.05
        # a kernel that kept the LAST maximum would give another dx
        g = pc._gen(case.name, dtype_name, gen, "dy")
        _, tap = pc.max_fwd(x, case)
        _, tap_last = pc.max_fwd(x, case, last=True)
        dy = pc.operands(tap.shape, x.dtype, g)
        assert not torch.equal(pc.max_bwd(case, tap, dy), pc.max_bwd(case, tap_last, dy))


# ------------------------------------------------------------------------------------------------
# descriptor checks
# ------------------------------------------------------------------------------------------------
def max_status(hip, lib, d):
    buf = C.create_string_buffer(64)
    rc = lib.vlfb_maxpool_bwd_describe(C.byref(d), 0, 0, 0, buf, 64)
    return rc, lib.vlfb_last_error().decode()


def avg_status(hip, lib, d):
    """the descriptor check comes before the pointer check: "null pointer" means the descriptor was accepted"""
    rc = lib.vlfb_avgpool_fwd(C.byref(d), None, None, None)
    assert rc != 0
    return lib.vlfb_last_error().decode()


def test_inconsistent_descriptors_are_rejected_with_the_dimension_named():
    hip, lib = hip_lib()
    good = dict(dtype=hip.BF16, N=1, Ti=4, Hi=9, Wi=11, C=8, To=4, Ho=5, Wo=6, kt=1, kh=3, kw=3, st=1, sh=2, sw=2, pt=0, ph=1, pw=1)

    def desc(**kw):
        d = hip.PoolDesc()
        for k, v in dict(good, **kw).items():
            setattr(d, k, v)
        return d
    assert max_status(hip, lib, desc())[0] == 0
    bad = [(dict(Ti=0), "dimension t"), (dict(Ho=0), "dimension h"), (dict(kw=0), "dimension w"), (dict(sh=0), "dimension h"),
           (dict(st=-1), "dimension t"), (dict(N=0), "N=0"),
           (dict(pt=1), "dimension t: pad 1"), (dict(ph=3), "dimension h: pad 3"), (dict(pw=4), "dimension w: pad 4"),
           (dict(pw=-1), "dimension w: pad -1"),
           (dict(To=5), "dimension t: the last of 5 windows"), (dict(Ho=7), "dimension h: the last of 7 windows"),
           (dict(Wo=8), "dimension w: the last of 8 windows")]
    for kw, msg in bad:
        rc, err = max_status(hip, lib, desc(**kw))
        assert rc != 0 and msg in err, (kw, err)
    # the largest outputs whose last window still has a tap inside: (Ho-1)*2 - 1 <= 8, (Wo-1)*2 - 1 <= 10
    assert max_status(hip, lib, desc(Wo=6))[0] == 0 and max_status(hip, lib, desc(Wo=7))[0] != 0
    # average pools: the window must lie inside
    avg = dict(pt=0, ph=0, pw=0, To=4, Ho=4, Wo=5)
    assert "null pointer" in avg_status(hip, lib, desc(**avg))
    for kw, msg in [(dict(To=5), "dimension t: the last of 5 windows"), (dict(Ho=5), "dimension h: the last of 5 windows"),
                    (dict(Wo=6), "dimension w: the last of 6 windows"), (dict(kt=5), "dimension t"), (dict(sw=3), "dimension w"),
                    (dict(kh=0), "dimension h"), (dict(Wi=0), "dimension w")]:
        err = avg_status(hip, lib, desc(**dict(avg, **kw)))
        assert msg in err and ("leaves the input" in err or "must be positive" in err), (kw, err)
    # the same check guards every entry point, before any pointer is looked at
    d, da = desc(Wo=8), desc(**dict(avg, Wo=8))
    for call in (lambda: lib.vlfb_maxpool_fwd(C.byref(d), None, None, None, None),
                 lambda: lib.vlfb_maxpool_bwd(C.byref(d), None, None, None, None, None, None),
                 lambda: lib.vlfb_maxpool_relu_bwd(C.byref(d), None, None, None, None, None),
                 lambda: lib.vlfb_avgpool_bwd(C.byref(da), None, None, None, None, None),
                 lambda: lib.vlfb_avgpool_bwd_two_term(C.byref(da), None, None, None, None, None)):
        assert call() != 0 and "dimension w" in lib.vlfb_last_error().decode()


def test_every_descriptor_of_the_table_is_accepted():
    hip, lib = hip_lib()
    for case in ALL_MAX:
        N, T, H, W = case.shape
        d = hip.pool_desc(hip.F16, N, T, H, W, case.C, *pc.out_dims(case), case.k, case.s, case.p)
        assert max_status(hip, lib, d)[0] == 0, case.name
    for case in pc.AVG_CASES:
        N, T, H, W = case.shape
        geo = pc.MaxCase(case.name, case.k, case.s, (0, 0, 0), case.shape, case.C, None, None)
        d = hip.pool_desc(hip.F16, N, T, H, W, case.C, *pc.out_dims(geo), case.k, case.s, (0, 0, 0))
        assert "null pointer" in avg_status(hip, lib, d), case.name


def test_every_pool_the_shipped_configs_build_is_accepted():
    """(k, s, p) and extents of every MaxPool / AveragePool the model builders emit, train and test graph of all presets"""
    hip, lib = hip_lib()
    from test_lowering import plan
    from vlfb.presets import PRESETS
    small = ("NUM_GPUS", 1, "TRAIN.BATCH_SIZE", 2, "TEST.BATCH_SIZE", 2, "TRAIN.VIDEO_LENGTH", 8, "TEST.VIDEO_LENGTH", 8,
             "TRAIN.CROP_SIZE", 64, "TEST.CROP_SIZE", 64)
    seen = set()
    for name in sorted(PRESETS):
        for split in ("train", "test"):
            cfg, m, eng = plan(name, small, split=split)
            for st in eng.steps:
                if type(st).__name__ != "PoolStep":
                    continue
                N, Cc, T, H, W = st.x.shape
                To, Ho, Wo = st.out.shape[2:]
                key = (st.is_max, T, H, W, Cc, To, Ho, Wo, tuple(st.k), tuple(st.s), tuple(st.p))
                if key in seen:
                    continue
                seen.add(key)
                d = hip.pool_desc(hip.F16, N, T, H, W, Cc, To, Ho, Wo, st.k, st.s, st.p)
                if st.is_max:
                    rc, err = max_status(hip, lib, d)
                    assert rc == 0, (name, split, key, err)
                else:
                    assert "null pointer" in avg_status(hip, lib, d), (name, split, key)
    kinds = {(k[0], k[8], k[9]) for k in seen}
    assert (True, (1, 3, 3), (1, 2, 2)) in kinds and (True, (2, 1, 1), (2, 1, 1)) in kinds and (True, (1, 2, 2), (1, 2, 2)) in kinds
    assert any(not k[0] for k in kinds)
