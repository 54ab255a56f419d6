"""AVA frame-mAP on the CPU: what is pinned to what.

  * The file-format layer of lib/utils/ava_eval_helper.py (and get_ava_mini_groundtruth of utils/metrics.py) is pinned to the
    REFERENCE's executed functions: tests/golden/ref_ava_eval.json.gz (tools/make_ref_ava_eval_golden.py) holds the text of
    seeded synthetic files and what the reference's own functions returned for them; the product must return the same, value
    for value, and write the result file byte for byte.
  * The evaluator cannot be pinned to reference code -- the reference ships none.  It is the public PASCAL-VOC protocol at
    IoU 0.5; tests/ava_eval_ref.py restates it, and the hand-worked cases below pin the restatement.  The GPU tests
    (tests/test_ava_eval_gpu.py) then hold the two kernels to the restatement on these cases and on the seeded ones built here.
"""
import ctypes
import gzip
import json
import os

import numpy as np
import pytest

import ava_eval_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_ava_eval.json.gz")


# ---- cases ---------------------------------------------------------------------------------------------------------------
def build_case(images, C=1, mask=None, pad_before=0):
    """images: [{"dets": [(box xyxy, [score per class])], "gts": [(box xyxy, class id)]}].  Detections take table rows in
    order; `pad_before` padding rows (scores 0.99, never named) precede every image's rows."""
    scores, boxes, det_rows, dptr, gptr, gbox, gcls = [], [], [], [0], [0], [], []
    for im in images:
        for _ in range(pad_before):
            scores.append([0.99] * C)
            boxes.append([0.0, 0.0, 0.0, 0.0])
        for box, s in im.get("dets", []):
            det_rows.append(len(scores))
            scores.append(list(s))
            boxes.append(list(box))
        dptr.append(len(det_rows))
        for box, cid in im.get("gts", []):
            gbox.append(list(box))
            gcls.append(cid)
        gptr.append(len(gcls))
    if not scores:
        scores, boxes = [[0.0] * C], [[0.0] * 4]
    return {"scores": np.asarray(scores, np.float32).reshape(-1, C), "det_box": np.asarray(boxes, np.float64).reshape(-1, 4),
            "img_det_ptr": np.asarray(dptr, np.int32), "det_rows": np.asarray(det_rows, np.int32),
            "img_gt_ptr": np.asarray(gptr, np.int32), "gt_box": np.asarray(gbox, np.float64).reshape(-1, 4),
            "gt_class": np.asarray(gcls, np.int32), "mask": np.ones(C, np.uint8) if mask is None else np.asarray(mask, np.uint8)}


def reference(case):
    return R.evaluate(case["scores"], case["det_box"], case["img_det_ptr"], case["det_rows"], case["img_gt_ptr"],
                      case["gt_box"], case["gt_class"], case["mask"])


A, B, FAR = (0, 0, 1, 1), (5, 5, 6, 6), (10, 10, 11, 11)
G0, G1 = (0, 0, 10, 10), (0, 0, 10, 4.2)


def hand_cases():
    """name -> (case, tp of the detection rows of class column 0 in row order, [AP per class])"""
    nan = float("nan")
    return {
        "a_two_on_one": (build_case([{"dets": [(A, [0.9]), (A, [0.8])], "gts": [(A, 1)]}]), [1, 0], [1.0]),
        "b_fp_then_tp": (build_case([{"dets": [(FAR, [0.9]), (A, [0.8])], "gts": [(A, 1)]}]), [0, 1], [0.5]),
        # d1 = (0,0,10,7): IoU 0.7 with g0, 0.6 with g1; g0 went to d0, and d1 does NOT fall back to g1
        "c_no_fallback": (build_case([{"dets": [(G0, [0.9]), ((0, 0, 10, 7), [0.8])], "gts": [(G0, 1), (G1, 1)]}]), [1, 0], [0.5]),
        "d_tp_fp_tp": (build_case([{"dets": [(A, [0.9]), (FAR, [0.8]), (B, [0.7])], "gts": [(A, 1), (B, 1)]}]), [1, 0, 1], [5.0 / 6.0]),
        "e_envelope": (build_case([{"dets": [(FAR, [0.9]), (A, [0.8]), (B, [0.7])], "gts": [(A, 1), (B, 1)]}]), [0, 1, 1], [2.0 / 3.0]),
        "f_iou_exactly_half": (build_case([{"dets": [((0, 0, 2, 1), [0.9])], "gts": [(A, 1)]}]), [1], [1.0]),
        "g_class_without_gt": (build_case([{"dets": [(A, [0.9, 0.3]), (FAR, [0.2, 0.8])], "gts": [(A, 1)]}], C=2), [1, 0], [1.0, nan]),
        "h_image_without_gt": (build_case([{"dets": [(A, [0.9]), (B, [0.7])], "gts": []},
                                           {"dets": [(A, [0.8])], "gts": [(A, 1)]}]), [0, 0, 1], [0.5]),
    }


def random_case(seed=7, quantize=None):
    """37 images, 80 classes of which 60 are whitelisted, 0-9 detections per image, 0-6 ground-truth boxes with 1-3 labels
    each; detection boxes are jittered copies of ground-truth boxes plus random ones; three pairs sit at IoU exactly 0.5 and
    one ulp of a coordinate either side; images 3 and 11 have only detections, 5 and 17 only ground truth; 0-2 padding rows
    precede every image's rows.  Scores: a permutation per class column, so fp32 scores are distinct within every column
    (asserted; recorded as case["distinct_checked"]) -- unless `quantize` levels are asked for, which makes ties inside
    images and across them."""
    rng = np.random.RandomState(seed)
    C, n_img = 80, 37
    mask = np.zeros(C, np.uint8)
    mask[rng.permutation(C)[:60]] = 1
    boxes, det_rows, dptr, gptr, gbox, gcls = [], [], [0], [0], [], []
    edge = {8: np.inf, 9: None, 10: -np.inf}        # x2 of the detection one ulp up / exact / one ulp down: IoU below / at / above 0.5
    for img in range(n_img):
        for _ in range(rng.randint(0, 3)):
            boxes.append([0.0, 0.0, 1.0, 1.0])                   # a padding row
        n_box = 0 if img in (3, 11) else rng.randint(1 if img in (5, 17) else 0, 7)
        mine = []
        for _ in range(n_box):
            x1, y1 = rng.uniform(0, 200, 2)
            w, h = rng.uniform(20, 120, 2)
            mine.append([x1, y1, x1 + w, y1 + h])
        if img in edge:
            off = float(300 + img)
            mine.append([off, off, off + 1.0, off + 1.0])
        for b in mine:
            for cid in rng.choice(np.flatnonzero(mask) + 1, rng.randint(1, 4), replace=False):
                gbox.append(b)
                gcls.append(int(cid))
        gptr.append(len(gcls))
        dets = []
        if img not in (5, 17):
            for b in mine[:n_box]:
                if rng.rand() < 0.8:
                    j = rng.uniform(-0.12, 0.12, 4) * np.array([b[2] - b[0], b[3] - b[1]] * 2)
                    dets.append([b[0] + j[0], b[1] + j[1], b[2] + j[2], b[3] + j[3]])
            for _ in range(rng.randint(0, 3) if img not in (3, 11) else 4):
                x1, y1 = rng.uniform(0, 200, 2)
                w, h = rng.uniform(20, 120, 2)
                dets.append([x1, y1, x1 + w, y1 + h])
            dets = dets[:8]
            if img in edge:
                off = float(300 + img)
                dets.append([off, off, off + 2.0 if edge[img] is None else np.nextafter(off + 2.0, edge[img]), off + 1.0])
        assert len(dets) <= 9
        for b in dets:
            det_rows.append(len(boxes))
            boxes.append(b)
        dptr.append(len(det_rows))
    n_rows = len(boxes)
    scores = np.stack([(rng.permutation(n_rows) + 0.5) / n_rows for _ in range(C)], axis=1).astype(np.float32)
    distinct = all(len(np.unique(scores[:, c])) == n_rows for c in range(C))
    if quantize:
        scores = (np.floor(scores * quantize) / quantize).astype(np.float32)
    else:
        assert distinct, "fp32 scores collide inside a class column"
    case = {"scores": scores, "det_box": np.asarray(boxes, np.float64), "img_det_ptr": np.asarray(dptr, np.int32),
            "det_rows": np.asarray(det_rows, np.int32), "img_gt_ptr": np.asarray(gptr, np.int32),
            "gt_box": np.asarray(gbox, np.float64).reshape(-1, 4), "gt_class": np.asarray(gcls, np.int32), "mask": mask,
            "distinct_checked": bool(distinct and not quantize)}
    for img, want in ((8, -1), (9, 0), (10, 1)):                # the constructed pairs land where they were aimed
        d = case["det_box"][det_rows[dptr[img + 1] - 1]]
        v = R.iou(d, gbox[gptr[img + 1] - 1])
        assert (v < 0.5, v == 0.5, v > 0.5)[want + 1] and abs(v - 0.5) < 1e-13, (img, v)
    return case


# ---- the restatement against the hand-worked cases -------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_restatement_reproduces_the_hand_worked_case(name):
    case, want_tp, want_ap = hand_cases()[name]
    tp, n_gt, ap, mean = reference(case)
    assert [int(v) for v in tp[case["det_rows"], 0]] == want_tp
    for got, want in zip(ap, want_ap):
        assert (np.isnan(got) and np.isnan(want)) or abs(got - want) <= R.bound(len(want_tp)), (got, want)
    kept = [w for w in want_ap if not np.isnan(w)]
    assert abs(mean - np.mean(kept)) <= R.bound(len(want_tp))                # (g): the class without ground truth leaves the mean
    if name == "c_no_fallback":
        assert abs(R.iou((0, 0, 10, 7), G0) - 0.7) < 1e-15 and abs(R.iou((0, 0, 10, 7), G1) - 0.6) < 1e-15
    if name == "e_envelope":
        assert abs(ap[0] - 7.0 / 12.0) > 0.05                                # not the un-enveloped sum
    if name == "f_iou_exactly_half":
        assert R.iou((0, 0, 2, 1), A) == 0.5
    if name == "h_image_without_gt":
        assert list(n_gt) == [1]


def test_seeded_cases_are_what_the_issue_asks_for():
    case = random_case()
    assert case["distinct_checked"] is True
    per_det, per_gt = np.diff(case["img_det_ptr"]), np.diff(case["img_gt_ptr"])
    assert len(per_det) == 37 and case["scores"].shape[1] == 80 and int(case["mask"].sum()) == 60
    assert per_det.max() <= 9 and per_det[[5, 17]].tolist() == [0, 0] and per_gt[[3, 11]].tolist() == [0, 0]
    assert per_det[[3, 11]].min() > 0 and per_gt[[5, 17]].min() > 0
    assert case["scores"].shape[0] > len(case["det_rows"])                   # padding rows are interleaved
    assert np.all(case["mask"][case["gt_class"] - 1] == 1)
    tp, n_gt, ap, mean = reference(case)
    named = np.zeros(case["scores"].shape[0], bool)
    named[case["det_rows"]] = True
    assert np.all(tp[~named] == 255) and np.all(tp[:, case["mask"] == 0] == 255)
    assert set(np.unique(tp[named][:, case["mask"] == 1])) == {0, 1}
    assert 0.0 < mean < 1.0 and int(n_gt.sum()) == len(case["gt_class"])
    assert int(np.sum(tp == 1)) >= 100                                       # (random scores: most cells are false positives)
    ties = random_case(quantize=4)
    assert ties["distinct_checked"] is False and len(np.unique(ties["scores"])) <= 5


# ---- the helper layer against the reference's executed functions -------------------------------------------------------------
def load():
    with gzip.open(GOLDEN, "rb") as f:
        return json.loads(f.read().decode())


def plain(triple):
    return [[[k, list(v)] for k, v in d.items()] for d in triple]


@pytest.fixture()
def files(tmp_path):
    g = load()
    paths = {}
    for name, text in g["files"].items():
        p = tmp_path / name
        p.write_text(text)
        paths[name] = str(p)
    return g, paths, tmp_path


def test_fixture_is_data_only():
    g = load()
    assert g["evaluator_run"] is False and os.path.getsize(GOLDEN) < 32768
    assert set(g["files"]) == {"labelmap", "gt", "det", "excl"}


def test_helper_functions_equal_the_reference(files):
    import utils.ava_eval_helper as A_
    import utils.metrics as M
    g, paths, tmp = files
    for v, t, want in g["image_keys"]:
        assert A_.make_image_key(v, t) == want
    categories, whitelist = A_.read_labelmap(paths["labelmap"])
    assert categories == g["labelmap"]["categories"] and sorted(whitelist) == g["labelmap"]["class_ids"]
    assert isinstance(whitelist, set)
    assert sorted(A_.read_exclusions(paths["excl"])) == g["exclusions"] and A_.read_exclusions(None) == set()
    want = g["read_csv"]
    assert plain(A_.read_csv(paths["gt"])) == want["gt_plain"]
    assert plain(A_.read_csv(paths["gt"], whitelist)) == want["gt_whitelist"]
    assert plain(A_.read_csv(paths["gt"], whitelist, load_score=False)) == want["gt_whitelist_flag"]
    assert plain(A_.read_csv(paths["det"], None, load_score=True)) == want["det_scores"]
    assert plain(A_.read_csv(paths["det"], whitelist, load_score=True)) == want["det_scores_whitelist"]
    assert plain(A_.read_csv(paths["det"], whitelist)) == want["det_no_scores"]
    assert plain(M.get_ava_mini_groundtruth(A_.read_csv(paths["gt"], whitelist))) == g["mini_groundtruth"]
    e = g["eval_data"]
    det = A_.get_ava_eval_data(np.asarray(e["scores"], np.float32), np.asarray(e["boxes"], np.float32),
                               np.asarray(e["metadata"], np.float32), whitelist,
                               video_idx_to_name={i: v for i, v in enumerate(e["videos"])})
    assert plain(det) == e["detections"]
    out = str(tmp / "results.csv")
    A_.write_results(det, out)
    assert open(out, "rb").read() == e["written"].encode()
    A_.write_results(A_.read_csv(paths["det"], whitelist, load_score=True), out)
    assert open(out, "rb").read() == g["written_from_csv"].encode()
    for name in ("run_evaluation", "evaluate_ava", "evaluate_ava_from_files"):
        assert callable(getattr(A_, name))


def test_image_index_drops_invalid_boxes_and_excluded_keys():
    from vlfb.metrics import ava_image_index
    gt = ({"v,0001": [[0, 0, 1, 1], [0, 0, 1, 1]], "v,0002": [[0, 0, 1, 1]], "w,0001": [[2, 3, 4, 5]]},
          {"v,0001": [3, 5], "v,0002": [1], "w,0001": [2]})
    keys = ["x,0009", "v,0001", "v,0002", "v,0001", "w,0001"]
    boxes = [[0, 0, 1, 1], [0, 0, 1, 1], [0, 0, 1, 1], [3, 0, 1, 1], [0, 0, 1, 1]]            # the fourth has x2 < x1
    ix = ava_image_index([4, 0, 2, 6, 9], keys, boxes, gt, excluded_keys={"v,0002"})
    assert ix["keys"] == ["v,0001", "w,0001", "x,0009"]
    assert ix["img_det_ptr"].tolist() == [0, 1, 2, 3] and ix["det_rows"].tolist() == [0, 9, 4]
    assert ix["img_gt_ptr"].tolist() == [0, 2, 3, 3] and ix["gt_class"].tolist() == [3, 5, 2]
    assert ix["gt_box"].tolist()[2] == [3.0, 2.0, 5.0, 4.0]                                    # [y1, x1, y2, x2] -> (x1, y1, x2, y2)


# ---- refusals on the host: nothing is launched, no pointer is dereferenced ------------------------------------------------
def test_host_side_refusals_need_no_gpu():
    from vlfb import hip
    if not os.path.exists(hip.LIB_PATH):
        pytest.skip("libvlfb_hip.so not built")
    L = hip.lib()
    p = 4096
    arr = lambda v: (ctypes.c_int32 * len(v))(*v)
    ok, big_det, big_gt = arr([0, 3, 5]), arr([0, 2, 2 + hip.AVA_MAX_DET + 1]), arr([0, hip.AVA_MAX_GT + 1, hip.AVA_MAX_GT + 1])
    addr = lambda a: ctypes.cast(a, ctypes.c_void_p)
    call = lambda dptr, gptr, n_rows=400: L.vlfb_ava_match_tp(p, p, n_rows, 80, p, p, p, p, p, 2, addr(dptr), addr(gptr), p, p, p, None)
    with pytest.raises(hip.VlfbError, match=r"image 1 has 129 detection rows"):
        hip._check(call(big_det, ok), "vlfb_ava_match_tp")
    with pytest.raises(hip.VlfbError, match=r"image 0 has 129 ground-truth rows"):
        hip._check(call(ok, big_gt), "vlfb_ava_match_tp")
    with pytest.raises(hip.VlfbError, match="decreases at image 1"):
        hip._check(call(arr([0, 3, 2]), ok), "vlfb_ava_match_tp")
    with pytest.raises(hip.VlfbError, match="host copy"):
        hip._check(L.vlfb_ava_match_tp(p, p, 400, 80, p, p, p, p, p, 2, None, addr(ok), p, p, p, None), "vlfb_ava_match_tp")
    with pytest.raises(hip.VlfbError, match="5 detections named for a table of 4 rows"):
        hip._check(call(ok, ok, n_rows=4), "vlfb_ava_match_tp")
    with pytest.raises(hip.VlfbError, match="short workspace"):
        hip._check(L.vlfb_class_ap_voc(p, p, p, hip.CLASS_AP_VOC_LDS_MAX + 1, 4, p, p, 16, 0, None), "vlfb_class_ap_voc")
    with pytest.raises(hip.VlfbError, match="short workspace"):
        hip._check(L.vlfb_class_ap_voc(p, p, p, 100, 4, p, None, 0, hip.CLASS_AP_FORCE_GLOBAL, None), "vlfb_class_ap_voc")
    with pytest.raises(hip.VlfbError, match="unknown flags"):
        hip._check(L.vlfb_class_ap_voc(p, p, p, 100, 4, p, None, 0, 2, None), "vlfb_class_ap_voc")
    with pytest.raises(hip.VlfbError, match=r"n = 0"):
        hip._check(L.vlfb_class_ap_voc(p, p, p, 0, 4, p, None, 0, 0, None), "vlfb_class_ap_voc")
    assert hip.WS_CLASS_AP_VOC not in (17, hip.WS_CLASS_AP)
    assert hip.query_workspace(hip.WS_CLASS_AP_VOC, (4097, 80)) == 8192 * 80 * 8
    assert hip.query_workspace(hip.WS_CLASS_AP_VOC, (1 << 17, 80)) == (1 << 17) * 80 * 8
    with pytest.raises(hip.VlfbError, match="class_ap_voc"):
        hip.query_workspace(hip.WS_CLASS_AP_VOC, (hip.CLASS_AP_MAX_N + 1, 3))


def test_metrics_calculator_keeps_the_reference_names():
    import inspect
    import utils.metrics as M
    args = inspect.signature(M.MetricsCalculator.__init__).parameters
    for name in ("ava_groundtruth", "excluded_keys", "class_whitelist", "categories"):
        assert name in args and args[name].default is None
    assert callable(M.MetricsCalculator.add_ava_batch) and callable(M.get_ava_mini_groundtruth)
    for name in ("evaluate_ava", "read_csv", "read_exclusions", "read_labelmap", "evaluate_ava_from_files"):
        assert hasattr(M, name), name
