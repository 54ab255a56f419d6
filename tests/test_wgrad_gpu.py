"""Every WGRAD kernel family against the fp64 descriptor model, element by element, over the edge table of
tests/wgrad_cases.py (what the table pins, and why its bound has teeth: there and in tests/test_wgrad_cases_host.py).

Per entry and element type: the plan string is asserted (family, tile, split count), the launch runs through
conv_desc_ref.Case -- NaN-filled outputs, sentinel guard bands around O, dbias and an exactly-sized NaN-filled workspace --
and is held to Case.bound(), the elementwise bound from operation counts; a second launch must reproduce O and dbias bit
for bit (ordered, atomic-free reductions).  The largest error / bound per family is printed when the module ends."""
import collections

import pytest
import torch

import conv_desc_ref as cr
import wgrad_cases as wc

pytestmark = pytest.mark.gpu

hip = None
WORST = collections.defaultdict(float)      # (family, type, output) -> largest error / bound


def setup_module(module):
    from vlfb import hip as h
    module.hip = h
    h.lib()


def teardown_module(module):
    print("\nlargest error / bound per family:")
    for (fam, t, what), r in sorted(WORST.items()):
        print("  %-14s %-5s %-5s %.3f" % (fam, t, what, r))


def outputs(c):
    """raw device bytes of O and dbias (guard bands included), and the live values of both"""
    raw = [t.cpu().view(torch.uint8) for t in (c.O, c.dbias) if t is not None]
    got = c._live_values(c.O.cpu().double(), c.o_live)
    db = None if c.dbias is None else c.dbias.cpu().double()[cr.GUARD:cr.GUARD + c.d["Cn"]]
    return raw, got, db


IDS = wc.case_ids()


@pytest.mark.parametrize("name,tname", IDS, ids=["%s-%s" % i for i in IDS])
def test_wgrad_entry_matches_the_model(name, tname):
    e = wc.CASES[name]
    d = wc.full(e.fields, tname)
    desc = hip.conv_desc(**d)
    plan = hip.conv_plan(desc)
    assert plan == wc.plan_of(e, tname)
    c = cr.Case(d, e.ops, seed=wc.seed_of(name, tname))
    c.run(hip)
    raw, got, db = outputs(c)
    fam = wc.family_of(plan)
    # the figures first, so that a failing entry still shows them
    ratio = float(((got - c.ref).abs() / c.bound()).max()) if bool(torch.isfinite(got).all()) else float("nan")
    print("%s %s: O error / bound %.3f" % (name, tname, ratio))
    c.check()
    what = "O" if d["out_dtype"] == cr.F32 else "O16"          # (a 16-bit output reaches 1: that is its rounding)
    WORST[(fam, tname, what)] = max(WORST[(fam, tname, what)], ratio)
    if db is not None:
        u = c.u_prod() + 2.0 ** -24 * (c.g.M // 16 + 64)
        r = float(((db - c.dbias_ref).abs() / (2 * u * c.dbias_mag + 1e-37)).max())
        WORST[(fam, tname, "dbias")] = max(WORST[(fam, tname, "dbias")], r)
    c.run(hip)
    again, _, _ = outputs(c)
    assert len(raw) == len(again) and all(torch.equal(a, b) for a, b in zip(raw, again)), "a second launch differs"


@pytest.mark.parametrize("name", list(wc.REFUSALS))
@pytest.mark.parametrize("tname", wc.T16)
def test_refused_descriptors_launch_nothing(name, tname):
    fields, text = wc.REFUSALS[name]
    d = wc.full(fields, tname)
    c = cr.Case(d, ("rowscale",), seed=1)
    buf, _, _ = c._out_buffer(torch.float32)
    want = torch.full_like(buf, cr.SENTINEL)
    O = want.cuda()
    ws = torch.full((1 << 20,), cr.SENTINEL, dtype=torch.float32, device="cuda")
    with pytest.raises(hip.VlfbError) as ex:
        hip.conv_run(hip.conv_desc(**d), c.A_dev.cuda(), None, c.P_dev.cuda(), O[cr.GUARD:], rowscale=c.rowscale.cuda(),
                     workspace=ws)
    torch.cuda.synchronize()
    assert text in str(ex.value), str(ex.value)
    assert torch.equal(O.cpu(), want) and bool((ws == cr.SENTINEL).all()), "a refused launch wrote"
