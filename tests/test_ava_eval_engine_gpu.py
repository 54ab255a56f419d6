"""AVA frame-mAP through the engine: utils.metrics.MetricsCalculator(eng, "test", ava_groundtruth=...) attaches the "ava"
meter behind the head of ava_r50_lfb_nl; three test iterations with different real RoI counts (full, ragged, a single box)
are appended to the device table inside the step; finalize_metrics scores the table with the two kernels.  Held to the fp64
restatement (tests/ava_eval_ref.py) applied to the fetched `prob` rows, within (n + 8) * 2^-52."""
import numpy as np
import pytest

import ava_eval_ref as R
from test_metrics_engine_gpu import TEST_SMALL
from test_model_gpu import build

pytestmark = pytest.mark.gpu

VIDEOS = {0: "vidA", 1: "vidB"}


def forward_names(eng):
    from vlfb import hip
    rec = hip.trace_begin()
    try:
        eng.forward()
    finally:
        hip.trace_end()
    return [name for _, _, name in rec]


def test_three_ragged_test_iterations_end_in_the_restated_map(capsys, tmp_path, monkeypatch):
    import utils.ava_eval_helper as A
    import utils.metrics as M
    monkeypatch.chdir(tmp_path)                                   # (evaluate_ava writes detections_<name>.csv where it runs)
    cfg, model, eng, inputs, params, _ = build("ava_r50_lfb_nl", "bf16", overrides=TEST_SMALL, train=False)
    C = cfg.MODEL.NUM_CLASSES
    planned = inputs["proposals"].shape[0]
    assert planned == 5
    whitelist = set(range(1, C + 1)) - {2, 16, 40}
    categories = [{"id": i, "name": "action %d" % i} for i in range(1, C + 1)]
    takes = [[0, 1, 2, 3, 4], [0, 1, 2], [3]]                      # full, ragged (clip 0: two boxes, clip 1: one), a single box
    rng = np.random.RandomState(4)
    # original boxes: what the annotation files speak of; ground truth = some of them (IoU 1), some shifted (IoU < 0.5)
    metadata, original, gt_boxes, gt_labels = [], [], {}, {}
    for it, take in enumerate(takes):
        md, ob = [], []
        for r in take:
            clip = int(inputs["proposals"][r, 0])
            x1, y1 = rng.uniform(0, 0.5, 2)
            box = [x1, y1, x1 + rng.uniform(0.1, 0.4), y1 + rng.uniform(0.1, 0.4)]
            md.append([clip + rng.uniform(-0.1, 0.1), 902 + it])
            ob.append([clip] + box)
            key = "%s,%04d" % (VIDEOS[clip], 902 + it)
            g = box if rng.rand() < 0.7 else [box[0] + 0.5, box[1], box[2] + 0.5, box[3]]
            for cid in rng.choice(np.arange(1, C + 1), 3, replace=False):
                gt_boxes.setdefault(key, []).append([g[1], g[0], g[3], g[2]])
                gt_labels.setdefault(key, []).append(int(cid))
        metadata.append(np.asarray(md, np.float32))
        original.append(np.asarray(ob, np.float32))
    gt_boxes["vidB,0950"], gt_labels["vidB,0950"] = [[0.1, 0.1, 0.5, 0.5]], [7]          # ground truth only: adds to n_gt
    gt_boxes["vidA,0903"] = gt_boxes.pop("vidA,0903")                                     # (reorders the keys)
    gt_labels["vidA,0903"] = gt_labels.pop("vidA,0903")
    groundtruth = (gt_boxes, gt_labels, {k: [1.0] * len(v) for k, v in gt_labels.items()})
    excluded = {"vidA,0902"}

    mc = M.MetricsCalculator(eng, "test", video_idx_to_name=VIDEOS, ava_groundtruth=groundtruth, excluded_keys=excluded,
                             class_whitelist=whitelist, categories=categories, ava_table_rows=3 * planned)
    assert mc.meter is not None and mc.meter.kind == "ava" and mc.meter.n_items == 15 and mc.batch_rows == planned
    names = None
    fetched = []
    timer = type("T", (), {"diff": 0.0, "average_time": 0.0})()
    for it, take in enumerate(takes):
        for k in ("proposals", "lfb", "labels"):
            if (k + "_test") in model.input_blob_names:
                eng.feed(k + "_test", inputs[k][take])
        names = forward_names(eng)
        fetched.append(eng.fetch("prob").reshape(planned, C).astype(np.float32))
        mc.add_ava_batch(metadata[it], original[it])
        mc.calculate_and_log_all_metrics_test(it, timer, 3)
    assert names.count("vlfb_scores_merge_max") == 1
    mc.finalize_metrics()
    table = np.concatenate(fetched)
    assert mc.meter.table.cpu().numpy().tobytes() == table.tobytes()                      # the padding rows are in the table ...
    assert mc.results["rows_seen"] == 15 and mc.results["detections"] == 7                # ... and are never named (9 real - 2 excluded)

    # the restatement on the fetched rows: an index built here, by hand
    keys = [k for k in gt_boxes if k not in excluded]
    det = []                                                                              # (table row, key, box)
    for it, take in enumerate(takes):
        for r in range(len(take)):
            key = "%s,%04d" % (VIDEOS[int(np.round(metadata[it][r][0]))], int(np.round(metadata[it][r][1])))
            if key not in excluded:
                det.append((it * planned + r, key, original[it][r][1:5].astype(np.float64)))
                if key not in keys:
                    keys.append(key)
    det_box = np.zeros((15, 4))
    det_rows, dptr, gptr, gbox, gcls = [], [0], [0], [], []
    for key in keys:
        for row, k, box in det:
            if k == key:
                det_rows.append(row)
                det_box[row] = box
        dptr.append(len(det_rows))
        for b, l in zip(gt_boxes.get(key, []), gt_labels.get(key, [])):
            gbox.append([b[1], b[0], b[3], b[2]])
            gcls.append(l)
        gptr.append(len(gcls))
    mask = np.array([1 if c + 1 in whitelist else 0 for c in range(C)], np.uint8)
    tp, n_gt, ap, want = R.evaluate(table, det_box, dptr, det_rows, gptr, np.asarray(gbox, np.float64), gcls, mask)
    print("full_map %.17g restated %.17g  classes with ground truth %d  true positives %d" % (
        mc.full_map, want, int(np.sum(n_gt > 0)), int(np.sum(tp == 1))))
    assert int(np.sum(tp == 1)) > 0 and int(np.sum(n_gt > 0)) > 5
    assert np.array_equal(mc.results["n_gt"], n_gt)
    assert abs(mc.full_map - want) <= R.bound(15)
    assert np.nanmax(np.abs(mc.results["ap"] - ap)) <= R.bound(15) and np.array_equal(np.isnan(mc.results["ap"]), np.isnan(ap))
    assert mc.get_computed_metrics()["test_full_map"] == mc.full_map
    capsys.readouterr()
    mc.log_final_metrics(2, 3)
    line = capsys.readouterr().out
    assert "testing finished #iters [3|3]: mAP: %.3f" % mc.full_map in line

    # the array path: the same rows, compacted as the reference's meter would hold them
    preds = np.concatenate([fetched[it][:len(take)] for it, take in enumerate(takes)])
    got = A.evaluate_ava(preds, np.concatenate(original), np.concatenate(metadata), excluded, whitelist, categories,
                         groundtruth=groundtruth, video_idx_to_name=VIDEOS, name="t")
    assert abs(got - mc.full_map) <= R.bound(15)
    assert (tmp_path / "detections_t.csv").read_text().count("\n") == 9 * len(whitelist)
    scored = [c for c in categories if c["id"] in whitelist]
    res = A.run_evaluation(scored, groundtruth, A.read_csv(str(tmp_path / "detections_t.csv"), whitelist, load_score=True),
                           excluded, verbose=False)
    assert set(res) == {A.MAP_KEY} | {A.CATEGORY_KEY + c["name"] for c in scored}
    assert 0.0 <= res[A.MAP_KEY] <= 1.0                           # (scores and boxes rounded to the file's 4 / 3 decimals)


def test_without_groundtruth_nothing_changes():
    """no ava_groundtruth: no meter, the forward pass issues what it issued before, finalize_metrics refuses as before"""
    import utils.metrics as M
    cfg, model, eng, inputs, params, _ = build("ava_r50_lfb_nl", "bf16", overrides=TEST_SMALL, train=False)
    plain = forward_names(eng)
    mc = M.MetricsCalculator(eng, "test")
    assert mc.meter is None and eng.meter is None
    assert forward_names(eng) == plain and not any("merge" in n or "ava" in n for n in plain)
    with pytest.raises(NotImplementedError, match="ava_evaluation"):
        mc.finalize_metrics()
    with_gt = M.MetricsCalculator(eng, "test", video_idx_to_name=VIDEOS, ava_groundtruth=({}, {}, {}), ava_table_rows=5)
    metered = forward_names(eng)
    assert [n for n in metered if n != "vlfb_scores_merge_max"] == plain and len(metered) == len(plain) + 1
    eng.attach_meter(None)
    assert forward_names(eng) == plain
    assert with_gt.meter.counters()[2] == 5
