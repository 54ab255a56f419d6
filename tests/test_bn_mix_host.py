"""SpatialBN on the `mix` dtype, host side: the plan of a batch-norm graph (the ReLU and the residual Sum behind a SpatialBN
run in its apply pass, the trunk stays on the two-plane kernels, the residual stream keeps its two-term gradient) and the
argument checks of vlfb_bn_fwd_mix / vlfb_bn_bwd_mix / vlfb_bn_mix_workspace_bytes (no launch, no GPU)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (the override list of tests/test_bn_gpu.py)
BN = ["MODEL.USE_AFFINE", False, "NONLOCAL.USE_BN", True, "NONLOCAL.USE_AFFINE", False, "MODEL.DILATIONS_AFTER_CONV5", False]


def _dry(dtype, split, overrides=BN):
    p = os.path.join(ROOT, "tools")
    if p not in sys.path:
        sys.path.insert(0, p)
    import make_conv_plan_golden as plans
    return plans.dry_engine("ava_r50_lfb_nl", dtype, 2, 16, 64, split, overrides=overrides)


def _kind(st):
    return type(st).__name__


def _by_bn(eng, b):
    return _kind(b.root.producer) == "BNStep"


def _trunk(name):
    return name.startswith(("res_conv1", "res2_", "res3_", "res4_", "res5_", "pool", "nonlocal_conv"))


@pytest.mark.parametrize("split", ["train", "test"])
def test_mix_plan_of_a_bn_graph_folds_relu_and_sum_and_stays_two_plane(split):
    eng = _dry("mix", split)
    steps = eng.steps
    bns = [st for st in steps if _kind(st) == "BNStep"]
    assert len(bns) == 1 + 16 * 3 + 4 + 5
    # no separate ReLU / Sum pass reads a SpatialBN output
    for st in steps:
        if _kind(st) in ("ReluStep", "AddStep"):
            assert not any(_by_bn(eng, b) for b in st.inputs), st.name()
    fused_relu = [st for st in bns if st.relu]
    fused_sum = [st for st in bns if st.residual is not None]
    assert len(fused_relu) == 1 + 16 * 3 and len(fused_sum) == 16 + 5
    # a projection block: the first operand's BN takes the Sum, the shortcut's BN stays as it is and is the residual
    for st in fused_sum:
        assert st.residual.root is not st.x.root and st.x.root.dead is False and st.out.root.pair == st.residual.root.pair
    proj = [st for st in bns if "branch1" in st.out.name]
    assert len(proj) == 4 and all(not st.relu and st.residual is None for st in proj)
    # every ungrouped trunk conv behind conv1 reads and writes two planes; so does every BN of the trunk
    convs = [st for st in steps if _kind(st) == "ConvStep" and _trunk(st.out.name)]
    assert len(convs) >= 1 + 16 * 3 + 4
    for st in convs:
        if st.stem:
            assert st.o_pair, st.name()
        elif st.group == 1 and _kind(st.x.root.producer) in ("BNStep", "PoolStep") and not st.out.root.grad_f32:
            assert st.x_pair and st.o_pair, st.name()
    for st in bns:
        if _trunk(st.out.name):
            assert st.out.root.name in eng.pair_blobs and st.xf == 8, st.name()         # (VLFB_F16PAIR)
            assert st.gt == 2 or split == "test"                                         # (VLFB_F16 gradients)
    if split == "train":
        # the residual stream keeps the two-term gradient of the affine plan
        aff = _dry("mix", "train", overrides=[])
        want = {b.name for b in aff.all_blobs if b.root is b and b.slot is not None and b.slot.two_term}
        have = {b.name: b for b in eng.all_blobs if b.root is b and not b.dead}
        common = sorted(n for n in want if n in have)
        assert len(common) >= 16, common
        lost = [n for n in common if not have[n].slot.two_term]
        assert not lost, lost
        # the ReLU masks of the fused outputs are among the blobs discrete_decisions() walks
        assert all(st.out.root.relu and not st.out.root.dead for st in fused_relu)


@pytest.mark.parametrize("preset", ["charades_r50_baseline", "charades_r50_lfb_nl", "epic_verb_r50_lfb_nl", "epic_noun_r50_baseline",
                                    "ava_r50_lfb_max"])
def test_bn_variants_of_the_other_presets_plan_on_mix(preset):
    """BNStep.setup raises at plan time for a (format, gradient) combination it has no launch for: none occurs"""
    p = os.path.join(ROOT, "tools")
    if p not in sys.path:
        sys.path.insert(0, p)
    import make_conv_plan_golden as plans
    for split in ("train", "test"):
        eng = plans.dry_engine(preset, "mix", 2, 16, 64, split, overrides=BN)
        bns = [st for st in eng.steps if _kind(st) == "BNStep"]
        assert len(bns) == 58 and all(st.xf in (0, 8) and st.gt in (0, 2) for st in bns)
        assert all(st.xf == 8 for st in bns if _trunk(st.out.name))
        assert not [st.name() for st in eng.steps if _kind(st) in ("ReluStep", "AddStep") and any(_by_bn(eng, b) for b in st.inputs)]


def test_the_fold_does_not_leak_to_split():
    eng = _dry("split", "train")
    kinds = [_kind(st) for st in eng.steps]
    # (the ReLU behind a block's Sum is part of its AddStep there: 1 + 2 per block separate ReLU passes)
    assert kinds.count("ReluStep") >= 1 + 16 * 2 and kinds.count("AddStep") >= 16 + 5
    reads_bn = [st for st in eng.steps if _kind(st) in ("ReluStep", "AddStep") and any(_by_bn(eng, b) for b in st.inputs)]
    assert len(reads_bn) >= 1 + 16 * 2 + 16 + 5
    assert all(not st.relu and st.residual is None for st in eng.steps if _kind(st) == "BNStep")
    assert not eng.pair_blobs


def test_mix_falls_back_to_the_fp32_value_form(monkeypatch):
    from vlfb.engine import Engine
    monkeypatch.setattr(Engine, "MIX_PAIR", False)
    eng = _dry("mix", "train")
    bns = [st for st in eng.steps if _kind(st) == "BNStep"]
    assert bns and all(st.xf == 0 for st in bns) and not eng.pair_blobs
    # the fp32 outputs the backward reads get their fp16 copy from a copy pass behind the step
    assert any(st._half_post for st in bns)


def test_argument_checks_of_the_mix_bn_entry_points():
    from vlfb import hip
    if not os.path.exists(hip.LIB_PATH):
        pytest.skip("libvlfb_hip.so not built")
    lib = hip.lib()
    PAIR, F32, F16, BF16 = hip.F16PAIR, hip.F32, hip.F16, hip.BF16
    for xf, rows, ch in ((PAIR, 25088, 64), (F32, 33, 512)):
        n = lib.vlfb_bn_mix_workspace_bytes(xf, rows, ch)
        assert n > 0 and n % 4 == 0
    assert lib.vlfb_bn_mix_workspace_bytes(F16, 64, 64) == -1 and lib.vlfb_bn_mix_workspace_bytes(PAIR, 0, 64) == -1
    p = 0x10000            # a non-null address: every check below fails before anything is launched or read
    big = 1 << 30

    def fwd(x=p, y=p, res=None, xf=PAIR, rows=64, ch=64, ws=p, ws_bytes=big, is_test=0, save=p):
        # (called on the library itself with a null stream: hip.call would ask torch for the current stream of a GPU)
        hip._check(lib.vlfb_bn_fwd_mix(x, y, res, p, p, p, p, save, save, ws, ws_bytes, xf, rows, ch, 1e-5, 0.9, is_test, 1, None),
                   "vlfb_bn_fwd_mix")

    def bwd(dy=p, dy_lo=None, x=p, dx=p, xf=PAIR, gt=F16, rows=64, ch=64, ws=p, ws_bytes=big):
        hip._check(lib.vlfb_bn_bwd_mix(dy, dy_lo, x, p, p, p, dx, p, p, ws, ws_bytes, xf, gt, rows, ch, 1.0, None), "vlfb_bn_bwd_mix")

    with pytest.raises(hip.VlfbError, match="null x"):
        fwd(x=None)
    with pytest.raises(hip.VlfbError, match="null x"):
        bwd(x=None)
    with pytest.raises(hip.VlfbError, match="multiple of 8"):
        fwd(ch=68)
    with pytest.raises(hip.VlfbError, match="multiple of 8"):
        bwd(ch=12)
    with pytest.raises(hip.VlfbError, match="multiple of 4"):
        fwd(xf=F32, ch=6)
    for bad in (F16, BF16, 5):
        with pytest.raises(hip.VlfbError, match="value format"):
            fwd(xf=bad)
        with pytest.raises(hip.VlfbError, match="value format"):
            bwd(xf=bad)
    for bad in (BF16, PAIR, 7):
        with pytest.raises(hip.VlfbError, match="gradient type"):
            bwd(gt=bad)
    with pytest.raises(hip.VlfbError, match="dy_lo"):
        bwd(dy_lo=p, gt=F32)
    with pytest.raises(hip.VlfbError, match="residual without an output"):
        fwd(y=None, res=p)
    with pytest.raises(hip.VlfbError, match="save_mean"):
        fwd(save=None)
    with pytest.raises(hip.VlfbError, match="nothing to compute"):
        hip._check(lib.vlfb_bn_bwd_mix(p, None, p, p, p, p, None, None, None, p, big, PAIR, F16, 64, 64, 1.0, None), "vlfb_bn_bwd_mix")
    need = lib.vlfb_bn_mix_workspace_bytes(PAIR, 64, 64)
    for kw in (dict(ws_bytes=need - 4), dict(ws=None)):
        with pytest.raises(hip.VlfbError, match="workspace"):
            fwd(**kw)
        with pytest.raises(hip.VlfbError, match="workspace"):
            bwd(**kw)
