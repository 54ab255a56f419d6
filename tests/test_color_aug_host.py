"""Colour augmentation of the device clip loader, host side: plan_color draws what the reference draws
(tests/golden/ref_color_aug.npz: the reference's own images_and_boxes_preprocessing, tools/make_ref_color_aug_golden.py),
the fp32 restatement the kernels are held to (tests/color_aug_ref.py) reproduces the reference's clips, and the new entry
points reject bad descriptors before any launch."""
import ctypes as C

import numpy as np
import pytest

import color_aug_cases as cases
import color_aug_ref as R

META, CASES = cases.load()
IDS = ["seed%d" % c["seed"] for c in CASES]


def _plans(case, cfg):
    """plan_clip then plan_color on RandomState(seed) -> (geometry, boxes, colour, the generator afterwards)"""
    from datasets import data_input_helper as dh
    h, w = case["frames"].shape[1:3]
    rng = np.random.RandomState(case["seed"])
    plan, boxes = dh.plan_clip(h, w, META["split"], META["crop"], META["shift"], case["boxes_in"].copy(), rng)
    return plan, boxes, dh.plan_color(rng), rng


def _pca_switch(case):
    return True if case["pca_only"] else None          # None: the key stays undefined and must read as False


def test_fixture_covers_the_cases():
    jit = [c for c in CASES if not c["pca_only"]]
    assert {tuple(c["order"]) for c in jit} == {(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)}
    assert {c["flip"] for c in jit} == {True, False} and {c["shape"] for c in jit} == {"wide", "tall"}
    assert any(c["pca_only"] for c in CASES) and any(c["use_bgr"] for c in CASES)
    assert META["generator"] == "tools/make_ref_color_aug_golden.py" and META["numpy"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_random_stream_and_boxes(case):
    with cases.case_cfg(META, case["use_bgr"], _pca_switch(case)) as cfg:
        plan, boxes, color, rng = _plans(case, cfg)
    assert float(rng.uniform()) == case["next_uniform"]             # same number and kind of draws as the reference
    assert np.array_equal(boxes, case["boxes_out"])
    assert bool(plan["flip"]) == case["flip"] and color["ops"] == case["order"]
    assert len(color["alphas"]) == len(color["ops"]) and all(0.6 <= a <= 1.4 for a in color["alphas"])
    assert len(color["light"]) == 3


def test_flag_off_draws_nothing_and_pca_only_draws_the_normal():
    from datasets import data_input_helper as dh
    with cases.case_cfg(META, color=False):
        rng = np.random.RandomState(5)
        assert dh.plan_color(rng) is None
        assert float(rng.uniform()) == float(np.random.RandomState(5).uniform())
    with cases.case_cfg(META, pca_only=True) as cfg:
        rng, twin = np.random.RandomState(5), np.random.RandomState(5)
        color = dh.plan_color(rng)
        alpha = twin.normal(0, 0.1, size=(1, 3))
        assert color["ops"] == [] and color["alphas"] == []
        assert float(rng.uniform()) == float(twin.uniform())
        eigval = np.array(cfg.TRAIN.PCA_EIGVAL).astype(np.float32)
        eigvec = np.array(cfg.TRAIN.PCA_EIGVEC).astype(np.float32)
        rgb = [sum(eigvec[i][j] * alpha[0][j] * eigval[j] for j in range(3)) for i in range(3)]
        assert np.allclose(color["light"], [rgb[2], rgb[1], rgb[0]], rtol=1e-12, atol=0)
    with cases.case_cfg(META, pca_only=False):                       # the key is honoured when present
        rng, twin = np.random.RandomState(5), np.random.RandomState(5)
        color = dh.plan_color(rng)
        assert color["ops"] == [int(v) for v in twin.permutation(np.arange(3))]


def test_restatement_matches_the_reference():
    """every element of every case within cases.GATE = 4 x the maximum measured here (printed; cited in DESIGN.md
    section 7).  The reference runs the chain in float64 from the first blend on, the restatement rounds every step
    to float32; nothing else differs, so the figure is a few float32 ulps of the outputs (|x| < 5, ulp 4.8e-7)."""
    worst = 0.0
    for case in CASES:
        with cases.case_cfg(META, case["use_bgr"], _pca_switch(case)) as cfg:
            plan, _, color, _ = _plans(case, cfg)
            mean, std = [np.float32(v) for v in cfg.DATA_MEAN], [np.float32(v) for v in cfg.DATA_STD]
        win = R.window_u8(case["frames"], plan, META["crop"], META["crop"])
        got = R.color_clip(win, color, mean, std, to_rgb=not case["use_bgr"]).transpose(3, 0, 1, 2)
        assert got.shape == case["clip"].shape and got.dtype == np.float32
        diff = float(np.abs(got.astype(np.float64) - case["clip"].astype(np.float64)).max())
        print("case seed %d order %s: max abs diff %.3e, max |clip| %.3f" % (case["seed"], case["order"], diff,
                                                                           float(np.abs(case["clip"]).max())))
        worst = max(worst, diff)
        assert diff <= cases.GATE, (case["seed"], diff)
    print("max abs diff over all cases %.3e (gate %.3e)" % (worst, cases.GATE))
    assert worst >= cases.MEASURED_MAX_ABS_DIFF * 0.999, "the recorded measurement is stale: %.3e" % worst


def test_frames_differ_in_brightness_so_a_clip_wide_mean_would_show():
    """swapping the per-frame grey mean for the clip's would move a contrast case far outside the gate"""
    case = next(c for c in CASES if 1 in c["order"])
    with cases.case_cfg(META, case["use_bgr"], _pca_switch(case)) as cfg:
        plan, _, _, _ = _plans(case, cfg)
    win = R.window_u8(case["frames"], plan, META["crop"], META["crop"])
    means = [float(R.grey_mean(s, META["crop"], META["crop"])) for s in R.band_sums(win)]
    assert max(means) - min(means) > 0.1


def _valid_call_args():
    from vlfb import hip
    d = hip.ClipDesc()
    d.frames, d.src_h, d.src_w, d.resized_h, d.resized_w = 2, 16, 16, 16, 16
    d.crop_h = d.crop_w = 8
    d.y0, d.x0, d.flip, d.to_rgb = 1, 2, 0, 1
    d.w_left, d.w_total, d.c_pad = 0, 8, 3
    for c in range(3):
        d.mean[c], d.std[c] = 0.45, 0.225
    q = hip.ClipColorDesc()
    q.n_ops = 3
    q.op[0], q.op[1], q.op[2] = 0, 1, 2
    q.alpha[0] = q.alpha[1] = q.alpha[2] = 1.0
    # host memory that no check dereferences: every call below is rejected before a launch
    bufs = [C.create_string_buffer(2 * 16 * 16 * 3), C.create_string_buffer(2 * 8 * 3 * 8), C.create_string_buffer(2 * 8 * 8 * 3 * 4)]
    return hip, d, q, bufs


def test_argument_checks_need_no_gpu():
    import os
    hip, d, q, (frames, sums, dst) = _valid_call_args()
    if not os.path.exists(hip.LIB_PATH):
        pytest.skip("libvlfb_hip.so not built")
    lib = hip.lib()
    fp, sp, dp = C.addressof(frames), C.addressof(sums), C.addressof(dst)

    def color(n_ops=3, ops=(0, 1, 2), sums=sp):
        q.n_ops = n_ops
        for i, o in enumerate(ops):
            q.op[i] = o
        rc = lib.vlfb_clip_preprocess_color(C.byref(d), C.byref(q), fp, None, None, None, None, sums, dp, hip.F32, None)
        if rc != 0:
            raise hip.VlfbError(lib.vlfb_last_error().decode())

    with pytest.raises(hip.VlfbError, match="n_ops 4"):
        color(n_ops=4)
    with pytest.raises(hip.VlfbError, match="op code 3"):
        color(ops=[0, 3, 2])
    with pytest.raises(hip.VlfbError, match="appears twice"):
        color(ops=[2, 1, 2])
    with pytest.raises(hip.VlfbError, match="contrast op needs the channel sums"):
        color(sums=None)
    with pytest.raises(hip.VlfbError, match="NULL sums"):
        hip._check(lib.vlfb_clip_channel_sums(C.byref(d), fp, None, None, None, None, None, None), "vlfb_clip_channel_sums")
    d.x0 = 9
    with pytest.raises(hip.VlfbError, match="crop window leaves the resized frame"):
        hip._check(lib.vlfb_clip_channel_sums(C.byref(d), fp, None, None, None, None, sp, None), "vlfb_clip_channel_sums")
    with pytest.raises(hip.VlfbError, match="crop window leaves the resized frame"):
        color()
