"""What of the device-resident AVA multi-crop pass needs no GPU: the argument checks of vlfb_multicrop_merge (every one
returns VLFB_ERR_ARG with a message before anything is launched), the order of the pass's 18 views, and what the kernel's
fixture test relies on in tests/golden/ref_aux.npz."""
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_aux.npz")


def _lib():
    from vlfb import hip
    if not os.path.exists(hip.LIB_PATH):
        pytest.skip("libvlfb_hip.so not built (run __graft_entry__.build())")
    return hip


# (logits, dtype, shift_stride, ld, boxes, frame_hw, rows, cols, scale, max_crop, flip, first, acc, out32, valid); the
# addresses are never read: every case is refused, or has no rows
GOOD = dict(logits=64, dtype=0, shift_stride=800, ld=88, boxes=64, frame_hw=64, rows=9, cols=80, scale=224, max_crop=256,
            flip=0, first=1, acc=64, out32=None, valid=None)
ORDER = ["logits", "dtype", "shift_stride", "ld", "boxes", "frame_hw", "rows", "cols", "scale", "max_crop", "flip", "first",
         "acc", "out32", "valid"]


def _call(hip, **change):
    a = dict(GOOD, **change)
    return hip.lib().vlfb_multicrop_merge(*([a[k] for k in ORDER] + [None]))


@pytest.mark.parametrize("change, message", [
    (dict(logits=None), "logits"), (dict(boxes=None), "boxes"), (dict(frame_hw=None), "frame_hw"), (dict(acc=None), "acc"),
    (dict(cols=0), "cols"), (dict(rows=-1), "rows"), (dict(ld=79), "ld"), (dict(scale=0), "scale"), (dict(max_crop=0), "max_crop"),
    (dict(dtype=3), "dtype"), (dict(dtype=-1), "dtype"), (dict(dtype=12), "dtype"),
], ids=lambda v: "-".join("%s=%r" % kv for kv in v.items()) if isinstance(v, dict) else None)
def test_every_bad_argument_is_refused_with_a_message(change, message):
    hip = _lib()
    assert _call(hip, **change) == -1                                     # VLFB_ERR_ARG
    text = hip.lib().vlfb_last_error().decode()
    assert text.startswith("multicrop_merge:") and message in text, text
    with pytest.raises(hip.VlfbError, match="multicrop_merge: .*%s" % message):
        hip._check(_call(hip, **change), "vlfb_multicrop_merge")


def test_no_rows_succeeds_without_a_device():
    hip = _lib()
    assert _call(hip, rows=0) == 0
    for code in (hip.F32, hip.BF16, hip.F16, hip.F64):
        assert _call(hip, rows=0, dtype=code) == 0
    assert "vlfb_multicrop_merge" in hip.EXPORTED_SYMBOLS


def test_the_views_of_a_keyframe_come_in_merge_order():
    from vlfb import multicrop as mc
    views = mc.multi_crop_views([224, 256, 320], max_crop=256)
    assert len(views) == 18
    want = [(s, f, k, min(256, s)) for s in (224, 256, 320) for f in (False, True) for k in (0, 1, 2)]
    assert [tuple(v) for v in views] == want
    assert [v.crop for v in views[::6]] == [224, 256, 256]
    assert [tuple(v) for v in mc.multi_crop_views([56, 64, 80], max_crop=64)[::3]] == [
        (56, False, 0, 56), (56, True, 0, 56), (64, False, 0, 64), (64, True, 0, 64), (80, False, 0, 64), (80, True, 0, 64)]


def test_the_fixture_holds_no_nan_and_every_number_of_valid_shifts():
    from vlfb import multicrop as mc
    z = np.load(GOLDEN)
    cases = json.loads(bytes(z["meta"]).decode())["multicrop"]
    seen = set()
    for k, case in enumerate(cases):
        assert not np.isnan(z["mc_%d_combined" % k]).any() and not np.isnan(z["mc_%d_final" % k]).any()
        assert z["mc_%d_logits" % k].shape[2:] == (3, 9, 3) and z["mc_%d_logits" % k].dtype == np.float64
        for scale in case["scales"]:
            for flip in (False, True):
                seen |= set(mc.shift_validity(z["mc_%d_boxes" % k], flip, scale, case["height"], case["width"]).sum(axis=0).tolist())
    assert len(cases) == 3 and seen == {1, 2, 3}


def test_the_merged_score_file_has_the_reference_s_lines(tmp_path):
    """write_merged_scores: one line per (detection, whitelisted class), `key,x1,y1,x2,y2,class,score` with the box as
    write_results prints it and the score as '%f' (merge_ava_score_files, metrics.py:703-710)"""
    from vlfb import multicrop as mc
    scores = np.array([[0.1234564, 2.5, 3.0000004], [5.9999996, 1e-7, 0.25]])
    result = dict(scores=scores, boxes=np.array([[0.1, 0.2, 0.3, 0.4], [0.002, 0.5, 1.0, 0.75]]),
                  metadata=np.array([[1, 902], [0, 1000]]))
    path = mc.write_merged_scores(str(tmp_path / "final.csv"), result, {0: "vidA", 1: "vidB"}, class_whitelist={1, 3})
    lines = open(path).read().splitlines()
    assert lines == ["vidB,0902,0.100,0.200,0.300,0.400,1,0.123456", "vidB,0902,0.100,0.200,0.300,0.400,3,3.000000",
                     "vidA,1000,0.002,0.500,1.000,0.750,1,6.000000", "vidA,1000,0.002,0.500,1.000,0.750,3,0.250000"]
    assert [float(l.split(",")[-1]) for l in lines] == [float("%f" % scores[r, c]) for r in (0, 1) for c in (0, 2)]
