"""Coverage check of the launch replay (tests/test_conv_launches_gpu.py), with the built library and no GPU: every
descriptor the engine stores in the dry-run plans of the benchmarked presets shrinks (N, T, then H / W) to a descriptor
with the same plan, small enough for the fp64 model, on which every tap still reads data, and the model accepts it.  The planner is a pure function of the
descriptor, so the replay of the shrunk descriptor runs the kernel instance the product launches."""
import collections

import pytest

import conv_desc_ref as cr
from test_lowering import plan

PRESETS = ("ava_r50_lfb_nl", "charades_r50_baseline")
DTYPES = ("mix", "fp16", "bf16", "split", "fp32")
FULL = ("NUM_GPUS", 1, "TRAIN.BATCH_SIZE", 2, "TRAIN.VIDEO_LENGTH", 32, "TRAIN.CROP_SIZE", 224)
# the 256-row kernels and the split-K WGRADs are chosen for launches with enough row tiles to fill the chip: those cannot
# shrink below a GFLOP or so without leaving their plan; the rest reaches the ~0.5 GFLOP of a quick fp64 check
SMALL_FLOPS, MAX_FLOPS = 0.5e9, 32e9


def stored_descs(eng):
    from vlfb import hip
    for s in eng.steps:
        for k, v in vars(s).items():
            if isinstance(v, hip.ConvDesc):
                yield "%s.%s" % (getattr(s.out, "name", type(s).__name__), k), v


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("preset", PRESETS)
def test_every_stored_descriptor_shrinks_to_its_plan(preset, dtype):
    from vlfb import hip
    _, _, eng = plan(preset, overrides=FULL, dtype=dtype)
    pf = lambda e: hip.conv_plan(hip.conv_desc(**e))
    seen, big = collections.Counter(), []
    n = 0
    for name, d in stored_descs(eng):
        dd = cr.desc_dict(d)
        e = cr.shrink(dd, pf, 0.0)
        assert cr.plan_key(pf(e)) == cr.plan_key(pf(dd)), name
        f = cr.flops(e)
        assert f <= MAX_FLOPS, (name, pf(dd), f)
        if f > SMALL_FLOPS:
            big.append((name, pf(dd)))
            assert pf(dd).startswith(("nt8", "tn8")) or "splits=1" not in pf(dd), (name, pf(dd), f)
        g, ge = cr.Geometry(dd), cr.Geometry(e)   # (the model's geometry accepts both: Unmodelled otherwise)
        # every tap of the launch reads data for some row of the shrunk descriptor -- none falls wholly into the padding, so
        # the replay exercises the tap cursor over all of K -- and each row axis keeps more than one position where it had it
        assert g.live_taps() == g.taps and ge.live_taps() == ge.taps, (name, pf(dd), ge.live_taps(), ge.taps)
        assert all(e[ax + "r"] >= min(dd[ax + "r"], 2) for ax in "THW"), (name, pf(dd))
        seen[cr.plan_key(pf(dd))] += 1
        n += 1
    assert n > 0 and len(seen) >= 5
