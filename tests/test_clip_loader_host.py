"""Host side of the minibatch clip loader (datasets.clip_loader): plan_minibatch draws what N successive per-clip calls
draw, the batched entry points reject bad items without a GPU, the item structure has the documented size, and the RoI rows
of a ragged minibatch are the per-clip rows under Engine.feed's padding rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import clip_loader_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBOX = [2, 0, 3]


def _same_plan(a, b):
    assert a == b and all(type(a[k]) is type(b[k]) for k in a)


def _check_planning(split, shift):
    from datasets import data_input_helper as dh
    bx = cases.boxes(3, NBOX)
    for seed in range(6):
        rng = np.random.RandomState(seed)
        plans, colors, out = dh.plan_minibatch(cases.SIZES, split, cases.CROP, shift, [b.copy() for b in bx], rng)
        ref = np.random.RandomState(seed)
        for n, (h, w) in enumerate(cases.SIZES):
            plan, b = dh.plan_clip(h, w, split, cases.CROP, shift, bx[n].copy(), ref)
            color = dh.plan_color(ref) if split == 1 else None
            _same_plan(plans[n], plan)
            assert colors[n] == color
            assert out[n].shape == b.shape and np.array_equal(out[n], b)
        assert rng.uniform() == ref.uniform()              # the same number of draws
    return plans, colors


@pytest.mark.parametrize("mode", list(cases.COLOR_MODES))
def test_plan_minibatch_is_n_per_clip_plans_train(mode):
    with cases.loader_cfg(**cases.COLOR_MODES[mode]):
        plans, colors = _check_planning(1, 1)
        assert all((c is None) == (mode == "off") for c in colors)
        if mode == "all":
            assert all(sorted(c["ops"]) == [0, 1, 2] for c in colors)
        if mode == "light":
            assert all(c["ops"] == [] and any(c["light"]) for c in colors)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("shift", [0, 1, 2])
def test_plan_minibatch_is_n_per_clip_plans_test(shift, flip):
    with cases.loader_cfg(extra=["AVA.FORCE_TEST_FLIP", flip]):
        plans, colors = _check_planning(0, shift)
        assert colors == [None] * 3 and all(p["flip"] == int(flip) for p in plans)


def test_plan_minibatch_takes_one_shift_per_clip():
    from datasets import data_input_helper as dh
    with cases.loader_cfg():
        plans, _, _ = dh.plan_minibatch(cases.SIZES, 0, cases.CROP, [0, 1, 2], None, np.random.RandomState(0))
        for n, (h, w) in enumerate(cases.SIZES):
            _same_plan(plans[n], dh.plan_clip(h, w, 0, cases.CROP, n)[0])


def test_item_structure_has_the_documented_size():
    from vlfb import hip
    text = open(os.path.join(ROOT, "include", "vlfb.h")).read()
    documented = int(re.search(r"#define VLFB_CLIP_ITEM_BYTES (\d+)", text).group(1))
    assert C.sizeof(hip.ClipItem) == documented == hip.CLIP_ITEM_BYTES == 176
    assert "sizeof = VLFB_CLIP_ITEM_BYTES = 176" in text
    assert [getattr(hip.ClipItem, f).offset for f in ("frames", "xofs", "xcoef", "yofs", "ycoef", "dst", "sums", "geo", "color")] == \
        [0, 8, 16, 24, 32, 40, 48, 56, 136]
    assert C.sizeof(hip.ClipDesc) == 80 and C.sizeof(hip.ClipColorDesc) == 40


def _items(n=2):
    """valid items over made-up addresses (a rejected call reads none of them): a resized, flipped clip and a plain one"""
    from datasets import data_input_helper as dh
    from vlfb import hip
    items = (hip.ClipItem * n)()
    for i in range(n):
        it = items[i]
        it.geo = dh.clip_desc(dict(resized_h=70, resized_w=93, y0=3, x0=70, flip=1), 3, 72, 96, cases.CROP, 4, 4)
        it.frames, it.xofs, it.xcoef, it.yofs, it.ycoef, it.dst, it.sums = [0x1000 * (k + 1) for k in range(7)]
        it.color = dh.color_desc(dict(ops=[0, 1, 2], alphas=[1.1, 0.9, 1.2], light=[0.01, -0.02, 0.03]))
    return items


def _rejects(items, n, pattern):
    from vlfb import hip
    lib = hip.lib()
    host, dev = C.cast(items, C.c_void_p), C.c_void_p(0x100000)
    for rc in (lib.vlfb_clip_batch_channel_sums(host, dev, n, None), lib.vlfb_clip_batch_preprocess(host, dev, n, hip.F32, None)):
        assert rc != 0
        msg = lib.vlfb_last_error().decode()
        assert re.search(pattern, msg) and msg.startswith("clip_batch_"), msg


def test_batched_entry_points_reject_bad_items_without_a_gpu():
    from vlfb import hip
    if not os.path.exists(hip.LIB_PATH):
        pytest.skip("libvlfb_hip.so not built")
    _rejects(_items(), 0, "n_items 0 is not in 1..65535")
    _rejects(_items(), 65536, "n_items 65536")
    bad = _items()
    bad[1].geo.x0 = 62                                      # flipped: the window would start left of column 0
    _rejects(bad, 2, "crop window leaves the resized frame")
    bad = _items()
    bad[1].geo.y0 = 7                                       # 7 + 64 > 70
    _rejects(bad, 2, "crop window leaves the resized frame")
    bad = _items()
    bad[0].ycoef = 0
    _rejects(bad, 2, "resize tables are required")
    bad = _items()
    bad[1].geo.c_pad = 2
    _rejects(bad, 2, "bad destination row")
    bad = _items()
    bad[1].color.op[2] = 0
    _rejects(bad, 2, "op code 0 appears twice")
    bad = _items()
    bad[0].sums = 0
    _rejects(bad, 2, "a contrast op needs the channel sums")
    lib = hip.lib()
    assert lib.vlfb_clip_batch_preprocess(C.cast(_items(), C.c_void_p), None, 2, hip.F32, None) != 0
    assert "NULL item array" in lib.vlfb_last_error().decode()


def test_rows_of_a_ragged_minibatch_are_the_per_clip_rows_padded_as_feed_pads():
    """2 + 0 + 3 boxes on a 6-row plan"""
    from datasets import data_input_helper as dh
    rows, classes = 6, 7
    rng = np.random.default_rng(5)
    bx = [b * 60.0 for b in cases.boxes(4, NBOX)]                       # transformed boxes, as plan_clip returns them
    bx[1] = None
    labels = [(rng.uniform(size=(k, classes)) < 0.3).astype(np.int32) for k in NBOX]
    props, lab, used = dh.minibatch_rows(bx, labels, rows, classes)
    # the per-clip path (tests/test_train_loop_gpu.py clip_inputs) ...
    want_p = np.concatenate([np.concatenate([np.full((len(b), 1), n), b], axis=1) for n, b in enumerate(bx) if b is not None])
    want_p = want_p.astype(np.float32)
    want_l = np.concatenate(labels).astype(np.int32)
    assert used == 5 and want_p.shape == (5, 5)
    # ... and Engine.feed's rule for a RoI batch smaller than the plan: labels -1, box 0 of clip 0
    want_p = np.concatenate([want_p, np.zeros((1, 5), np.float32)])
    want_l = np.concatenate([want_l, np.full((1, classes), -1, np.int32)])
    assert props.dtype == np.float32 and lab.dtype == np.int32
    assert np.array_equal(props, want_p) and np.array_equal(lab, want_l)
    assert list(props[:, 0]) == [0, 0, 2, 2, 2, 0]
    with pytest.raises(AssertionError):
        dh.minibatch_rows(bx, labels, 4, classes)
