"""vlfb_ava_match_tp and vlfb_class_ap_voc against the fp64 restatement of the protocol (tests/ava_eval_ref.py).

Bars: tp and n_gt are EXACTLY the restatement's; ap is within (n + 8) * 2^-52 of it (one division per term and one
fixed-order fp64 sum on either side, the bound tests/test_metrics_gpu.py holds vlfb_class_ap_auc to).  Every output buffer
carries 64 sentinel bytes behind it that must survive.
"""
import numpy as np
import pytest
import torch

import ava_eval_ref as R
import test_ava_eval_host as H

pytestmark = pytest.mark.gpu

GUARD = 64
_cache = {}


def shared(name, make):
    """a case and its restated results, computed once and left unchanged"""
    if name not in _cache:
        case = make()
        _cache[name] = (case, H.reference(case))
    return _cache[name]


def guarded(nbytes):
    buf = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[:nbytes]


def run(case, flags=0):
    """both entry points, by name -> (tp, n_gt, ap) as numpy, sentinels checked"""
    from vlfb import hip
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda() if a.size else None
    scores = up(case["scores"])
    n_rows, cols = case["scores"].shape
    n_img = len(case["img_det_ptr"]) - 1
    dev = [up(case[k]) for k in ("det_box", "img_det_ptr", "det_rows", "img_gt_ptr", "gt_box", "gt_class", "mask")]
    tp_buf, tp = guarded(n_rows * cols)
    gt_buf, n_gt = guarded(4 * cols)
    ap_buf, ap = guarded(8 * cols)
    dptr, gptr = np.ascontiguousarray(case["img_det_ptr"], np.int32), np.ascontiguousarray(case["img_gt_ptr"], np.int32)
    hip.call("vlfb_ava_match_tp", hip.ptr(scores), hip.ptr(dev[0]), n_rows, cols, hip.ptr(dev[1]), hip.ptr(dev[2]), hip.ptr(dev[3]),
             hip.ptr(dev[4]), hip.ptr(dev[5]), n_img, dptr.ctypes.data, gptr.ctypes.data, hip.ptr(dev[6]), hip.ptr(tp), hip.ptr(n_gt))
    ws_bytes = hip.query_workspace(hip.WS_CLASS_AP_VOC, (n_rows, cols)) \
        if (n_rows > hip.CLASS_AP_VOC_LDS_MAX or flags & hip.CLASS_AP_FORCE_GLOBAL) else 0
    ws_buf, ws = guarded(ws_bytes)
    hip.call("vlfb_class_ap_voc", hip.ptr(scores), hip.ptr(tp), hip.ptr(n_gt), n_rows, cols, hip.ptr(ap),
             hip.ptr(ws) if ws_bytes else None, ws_bytes, flags)
    torch.cuda.synchronize()
    for name, buf in (("tp", tp_buf), ("n_gt", gt_buf), ("ap", ap_buf), ("workspace", ws_buf)):
        assert bool((buf[-GUARD:] == 0xA5).all()), "bytes behind %s were written" % name
    return (tp.cpu().numpy().reshape(n_rows, cols), n_gt.cpu().numpy().view(np.int32).copy(),
            ap.cpu().numpy().view(np.float64).copy())


def check(case, want, got):
    tp_w, n_gt_w, ap_w, _ = want
    tp, n_gt, ap = got
    assert np.array_equal(tp, tp_w), "tp differs in %d cells" % int(np.sum(tp != tp_w))
    assert np.array_equal(n_gt, n_gt_w)
    assert np.array_equal(np.isnan(ap), np.isnan(ap_w))
    err = float(np.nanmax(np.abs(ap - ap_w))) if not np.all(np.isnan(ap_w)) else 0.0
    print("ap error %.3e (bound %.3e)" % (err, R.bound(case["scores"].shape[0])))
    assert err <= R.bound(case["scores"].shape[0])


@pytest.mark.parametrize("name", sorted(H.hand_cases()))
def test_hand_worked_cases(name):
    case, want_tp, want_ap = H.hand_cases()[name]
    tp, n_gt, ap = run(case)
    assert [int(v) for v in tp[case["det_rows"], 0]] == want_tp
    for got, want in zip(ap, want_ap):
        assert (np.isnan(got) and np.isnan(want)) or abs(got - want) <= R.bound(len(want_tp)), (got, want)
    check(case, H.reference(case), (tp, n_gt, ap))


def test_seeded_random_case_and_repeat_call():
    case, want = shared("random", H.random_case)
    assert case["distinct_checked"] is True
    first = run(case)
    check(case, want, first)
    again = run(case)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()                        # bit-identical on a second call
    mask = case["mask"]
    assert np.all(first[0][:, mask == 0] == 255) and np.all(first[1][mask == 0] == 0) and np.all(np.isnan(first[2][mask == 0]))
    named = np.zeros(case["scores"].shape[0], bool)
    named[case["det_rows"]] = True
    assert np.all(first[0][~named] == 255)                       # padding rows keep their 255 and leave the sort
    assert abs(R.mean_ap(first[2], first[1], mask) - want[3]) <= R.bound(case["scores"].shape[0])


def test_ties_follow_score_then_row():
    case, want = shared("ties", lambda: H.random_case(seed=11, quantize=4))
    col = case["scores"][case["det_rows"]]
    assert len(np.unique(col)) <= 5                              # equal scores inside every image and across images
    check(case, want, run(case))
    # and a constructed one: two equal-score detections on one box -- the lower ROW wins, whatever the CSR order says
    c = H.build_case([{"dets": [(H.A, [0.5]), (H.A, [0.5]), (H.FAR, [0.5])], "gts": [(H.A, 1)]},
                      {"dets": [(H.FAR, [0.5]), (H.B, [0.5])], "gts": [(H.B, 1)]}], pad_before=1)
    c["det_rows"][:3] = c["det_rows"][:3][::-1]
    tp, n_gt, ap = run(c)
    check(c, H.reference(c), (tp, n_gt, ap))
    assert tp[:, 0].tolist() == [255, 1, 0, 0, 255, 0, 1]
    assert abs(ap[0] - 0.7) <= R.bound(7)                        # TP FP FP FP TP of two: 0.5 * 1 + 0.5 * 2/5


def tiled(n_rows):
    """the seeded case repeated (images, rows and all) until the table holds n_rows, the remainder as padding rows"""
    base = H.random_case(seed=5)
    rows0, C = base["scores"].shape
    reps = n_rows // rows0
    rng = np.random.RandomState(n_rows)
    scores = np.stack([(rng.permutation(n_rows) + 0.5) / n_rows for _ in range(C)], axis=1).astype(np.float32)
    box = np.zeros((n_rows, 4), np.float64)
    box[:reps * rows0] = np.tile(base["det_box"], (reps, 1))
    nd, ng = len(base["det_rows"]), len(base["gt_class"])
    return {"scores": scores, "det_box": box, "mask": base["mask"],
            "det_rows": np.concatenate([base["det_rows"] + r * rows0 for r in range(reps)]).astype(np.int32),
            "img_det_ptr": np.concatenate([[0]] + [base["img_det_ptr"][1:] + r * nd for r in range(reps)]).astype(np.int32),
            "img_gt_ptr": np.concatenate([[0]] + [base["img_gt_ptr"][1:] + r * ng for r in range(reps)]).astype(np.int32),
            "gt_box": np.tile(base["gt_box"], (reps, 1)), "gt_class": np.tile(base["gt_class"], reps)}


def test_two_sort_paths_are_bit_identical():
    from vlfb import hip
    n = hip.CLASS_AP_VOC_LDS_MAX + 1                             # one above the LDS limit: the workspace path by itself
    case, want = shared("above", lambda: tiled(n))
    above = run(case)
    check(case, want, above)
    below, want_below = shared("below", lambda: tiled(hip.CLASS_AP_VOC_LDS_MAX - 1))
    lds = run(below)
    forced = run(below, hip.CLASS_AP_FORCE_GLOBAL)
    check(below, want_below, lds)
    for a, b in zip(lds, forced):
        assert a.tobytes() == b.tobytes()


def test_limits_of_one_image_and_more_classes_than_lanes():
    """128 detections on 128 ground-truth rows in one image (four chunks of IoU rows, both halves of the taken mask), and
    130 classes (a second round of lanes)"""
    rng = np.random.RandomState(2)
    C, n = 130, 128
    gts, dets = [], []
    for i in range(n):
        x, y = 40.0 * (i % 16), 40.0 * (i // 16)
        gts.append(((x, y, x + 30, y + 30), int(rng.choice([1, 2, 129, 130]))))
        j = rng.uniform(-4, 4, 4)
        dets.append(((x + j[0], y + j[1], x + 30 + j[2], y + 30 + j[3]), None))
    scores = np.stack([(rng.permutation(n) + 0.5) / n for _ in range(C)], axis=1)
    case = H.build_case([{"dets": [(b, scores[i]) for i, (b, _) in enumerate(dets)], "gts": gts}], C=C)
    check(case, H.reference(case), run(case))


def test_frame_ap_drops_invalid_boxes_and_leaves_masked_classes():
    """the two degenerate inputs through vlfb.metrics.ava_frame_ap: a class outside the whitelist stays at 255 / NaN, a
    detection with x2 < x1 is dropped on the host and never reaches the kernels"""
    from vlfb.metrics import ava_frame_ap
    gt = ({"v,0001": [[0, 0, 1, 1], [0, 0, 1, 1]]}, {"v,0001": [1, 2]})
    table = torch.tensor([[0.9, 0.9], [0.8, 0.8], [0.7, 0.7]], dtype=torch.float32, device="cuda")
    keys, boxes = ["v,0001"] * 3, [[1, 0, 0, 1], [0, 0, 1, 1], [10, 10, 11, 11]]             # row 0: x2 < x1
    r = ava_frame_ap(table, [0, 1, 2], keys, boxes, gt, class_whitelist={1}, return_tp=True)
    assert r["tp"].tolist() == [[255, 255], [1, 255], [0, 255]] and r["detections"] == 2
    assert r["n_gt"].tolist() == [1, 0] and r["ap"][0] == 1.0 and np.isnan(r["ap"][1]) and r["mean_ap"] == 1.0
    r = ava_frame_ap(table, [0, 1, 2], keys, boxes, gt, excluded_keys={"v,0001"})
    assert r["images"] == 0 and np.isnan(r["mean_ap"]) and r["n_gt"].tolist() == [0, 0]
    from vlfb import hip
    many = ["v,0001"] * (hip.AVA_MAX_DET + 1)
    big = torch.zeros((len(many), 2), dtype=torch.float32, device="cuda")
    with pytest.raises(hip.VlfbError, match="image 'v,0001' has 129 detections"):
        ava_frame_ap(big, np.arange(len(many)), many, [[0, 0, 1, 1]] * len(many), gt)
