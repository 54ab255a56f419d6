"""The conditions on the WGRAD edge table (tests/wgrad_cases.py), with the built library and no GPU: the planner is a pure
host function of the descriptor, so what an entry records -- plan string, split count, size of the last split -- is checked
here exactly, the fp64 model must accept every entry, the table must cover what its docstring lists, and the model's bound
must have teeth on every split entry (one dropped position is past it)."""
import pytest
import torch

import conv_desc_ref as cr
import wgrad_cases as wc

IDS = wc.case_ids()


def lib_plan(d):
    from vlfb import hip
    return hip.conv_plan(hip.conv_desc(**d))


def planned():
    """{(name, type): plan string} of the whole table"""
    return {(n, t): lib_plan(wc.full(wc.CASES[n].fields, t)) for n, t in IDS}


def test_defaults_are_the_library_defaults():
    from vlfb import hip
    assert cr.desc_dict(hip.conv_desc()) == wc.DEFAULTS
    assert (wc.F32, wc.BF16, wc.F16, wc.WGRAD, wc.MATH_BF16X3, wc.ALGO_PIPE256) == (
        cr.F32, cr.BF16, cr.F16, cr.WGRAD, cr.MATH_BF16X3, hip.ALGO_PIPE256)


@pytest.mark.parametrize("name,tname", IDS, ids=["%s-%s" % i for i in IDS])
def test_entry_plans_what_it_records(name, tname):
    from vlfb import hip
    e = wc.CASES[name]
    d = wc.full(e.fields, tname)
    plan = lib_plan(d)
    assert plan == wc.plan_of(e, tname)
    sp = wc.splits_of(plan)
    if sp == 1:
        assert e.last is None
    else:
        n, per, last, width = wc.split_layout(d, wc.family_of(plan), sp)
        assert (n, last) == (sp, e.last), (n, per, last)
        assert 1 <= last <= per and (sp - 1) * per + last == (d["N"] * d["Tr"] * d["Hr"] * d["Wr"]) // width
    # the workspace the planner states: the slabs, and the bias-gradient rows of the route the plan takes
    g = cr.Geometry(d)
    ws = d["Cn"] * g.K * sp if sp > 1 else 0
    if d["wgrad_bias"]:
        fused = wc.family_of(plan) == "tn_tr" and d["batch"] == 1 and not d["accumulate"]
        slabs = -(-g.M // 1024)   # column-sum slabs of 1024 rows (far below the cap of 2048 workgroups)
        ws += d["Cn"] * (sp if sp > 1 else 0) if fused else d["Cn"] * slabs
    assert hip.conv_workspace_bytes(hip.conv_desc(**d)) == 4 * ws


@pytest.mark.parametrize("name,tname", IDS, ids=["%s-%s" % i for i in IDS])
def test_model_accepts_the_entry(name, tname):
    e = wc.CASES[name]
    d = wc.full(e.fields, tname)
    g = cr.Geometry(d)
    c = cr.Case(d, e.ops, seed=wc.seed_of(name, tname))
    assert c.ref.shape == (g.batch, d["Cn"], g.K) and bool(torch.isfinite(c.bound()).all())
    assert ("dbias" in e.ops) == bool(d["wgrad_bias"])
    if not g.ident and d["Ts"] > d["kt"] - 1 - d["pt"]:
        # every tap reads data for some row (where the clip has fewer frames than the window reaches past its padding -- the
        # one- and two-frame shapes of the whole-row kernels -- the outermost taps cannot)
        assert g.live_taps() == g.taps, (g.live_taps(), g.taps)


def test_refusals_are_refused_with_their_message():
    from vlfb import hip
    for name, (fields, text) in wc.REFUSALS.items():
        for tname in wc.T16:
            with pytest.raises(hip.VlfbError) as ex:
                lib_plan(wc.full(fields, tname))
            assert text in str(ex.value), (name, str(ex.value))


def test_table_covers_families_tiles_grids_and_reduce_instances():
    plans = planned()
    fams = {wc.family_of(p) for p in plans.values()}
    assert fams == set(wc.FAMILIES), sorted(fams)
    tiles = lambda fam, ts: {p.split()[2] for (n, t), p in plans.items() if wc.family_of(p) == fam and t in ts}
    # launch_tn: the 64x256 tile exists for 16-bit operands only
    assert tiles("tn", ("f32",)) == {"128x128", "64x128", "128x64", "64x64"}
    for t in wc.T16:
        assert tiles("tn", (t,)) == {"64x256", "64x64"}
        assert tiles("tn_tr", (t,)) == {"128x128", "64x128", "128x64", "64x64"}      # launch_tn_tr_as
    assert tiles("tn_tr_planes", ("f32x3",)) == {"128x128", "64x128", "64x64"}
    assert tiles("tn_split", ("f32x3",)) == {"128x128", "64x128", "64x64"}
    tiled = [(k, wc.splits_of(p)) for k, p in plans.items() if wc.family_of(p) not in wc.WHOLE_ROW]
    for t in wc.T16:
        sp = sorted({s for (n, tt), s in tiled if tt == t and plans[(n, tt)].startswith("tn_tr ") and s > 1})
        assert {wc.grid_form(s) for s in sp} == {"1d", "2d"}
        # the three reduce instances, each with a split count below 4 G (its tail loop only) and one past 4 G that is no
        # multiple of it (unrolled loop, then the tail); G = 4 also with 16 = 4 G exactly (no tail)
        for G, below, past in ((1, 3, 7), (4, 9, 31), (16, 40, 72)):
            assert below in sp and wc.reduce_group(below) == G and below < 4 * G
            assert past in sp and wc.reduce_group(past) == G and past > 4 * G and past % (4 * G)
        assert 16 in sp and wc.reduce_group(16) == 4
        assert 2 in sp and 9 in sp and 33 in sp        # fewer splits than lane groups: G = 4 at 9 > 4, G = 16 at 33 > 16
        assert 8 in sp and 32 in sp                    # the thresholds themselves
        # a last split of a single position, in both grid forms
        ones = {wc.grid_form(wc.splits_of(plans[(n, t)])) for n, e in wc.CASES.items() if e.last == 1 and t in e.types and
                plans[(n, t)].startswith("tn_tr ")}
        assert ones == {"1d", "2d"}


def test_table_covers_rows_per_workgroup_and_both_bias_routes():
    plans = planned()
    for fam in wc.WHOLE_ROW:
        for t in wc.T16:
            tpw, ragged = set(), False
            for (n, tt), p in plans.items():
                if wc.family_of(p) == fam and tt == t:
                    _, per, last, _ = wc.split_layout(wc.full(wc.CASES[n].fields, t), fam)
                    tpw.add(per)
                    ragged |= last < per
            assert tpw == {1, 2, 3} and ragged, (fam, t, tpw)
    fused, unfused = set(), set()
    for (n, t), p in plans.items():
        d = wc.full(wc.CASES[n].fields, t)
        if d["wgrad_bias"]:
            f = wc.family_of(p) == "tn_tr" and d["batch"] == 1 and not d["accumulate"]
            (fused if f else unfused).add((wc.family_of(p), wc.splits_of(p) > 1, bool(d["accumulate"]), d["batch"] > 1))
    assert fused == {("tn_tr", False, False, False), ("tn_tr", True, False, False)}
    assert unfused >= {("tn_tr", False, True, False), ("tn_tr", False, False, True), ("tn", False, False, False),
                       ("tn", True, False, False), ("tn_split", False, False, False), ("tn8", False, False, False),
                       ("wgrad_rows", True, False, False)}


SPLIT_IDS = [(n, t) for n, t in IDS if wc.CASES[n].last is not None]


@pytest.mark.parametrize("name,tname", SPLIT_IDS, ids=["%s-%s" % i for i in SPLIT_IDS])
def test_one_dropped_position_is_past_the_bound(name, tname):
    """see "Teeth" in wgrad_cases: the reference minus one position's contribution must fail the comparison"""
    e = wc.CASES[name]
    d = wc.full(e.fields, tname)
    c = cr.Case(d, e.ops, seed=wc.seed_of(name, tname))
    g = c.g
    assert g.batch == 1
    sp, per, last, width = wc.split_layout(d, wc.family_of(e.plan), wc.splits_of(e.plan))
    idx = None if g.ident else g.gather_index()
    a = c.a_val[:g.S * g.lda].view(g.S, g.lda)[:, :d["Cs"]]
    a0 = torch.cat([a, torch.zeros(1, d["Cs"], dtype=a.dtype)])
    p = c.p_val[:g.M * g.ldp].view(g.M, g.ldp)[:, :d["Cn"]]
    rs = c.rowscale.double().view(-1, 1) if c.rowscale is not None else 1.0
    alpha = float(torch.tensor(d["alpha"], dtype=torch.float32))
    bound = c.bound()
    n = d["Wr"] if name in wc.ROW_TEETH else 1           # positions dropped: one (ROW_TEETH: one output row)
    for m0 in (g.M - n, per * width):
        contrib = torch.zeros(1, d["Cn"], g.K, dtype=torch.float64)
        reads = torch.zeros(g.K, dtype=torch.bool)
        for m in range(m0, m0 + n):
            row = a[m] if idx is None else a0[torch.where(idx[m] < 0, g.S, idx[m])].reshape(-1)
            contrib += (alpha * rs * torch.outer(p[m], row)).view(1, d["Cn"], g.K)
            # columns whose tap reads data at m (all of them on plain rows)
            reads |= torch.ones(g.K, dtype=torch.bool) if idx is None else (idx[m] >= 0).repeat_interleave(g.cpt)
        with pytest.raises(AssertionError):
            c._compare("O", c.ref - contrib, c.ref, bound, c.l2_bar())
        assert bool(reads.any())
        share = float((contrib.abs() > bound)[:, :, reads].double().mean())
        assert share >= 0.5, "position %d: %.3f of the outputs past the bound" % (m0, share)
