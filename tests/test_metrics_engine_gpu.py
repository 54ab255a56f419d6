"""A DeviceMeter attached to the engine (Engine.attach_meter): its kernels sit behind the loss head inside the step --
walked, re-issued from the recorded call list, or replayed as a captured graph -- and only READ the step's blobs.

The engine's probability blob is named `prob` (the reference names it `pred`, which is the logits blob here)."""
import numpy as np
import pytest
import torch

import test_metrics_host as H
from test_model_gpu import SMALL, build

pytestmark = pytest.mark.gpu

TEST_SMALL = SMALL + ["TEST.BATCH_SIZE", 2, "TEST.VIDEO_LENGTH", 16, "TEST.CROP_SIZE", 64]
MODES = {"eager": dict(STEP_TRACE=False, STEP_GRAPH=False), "trace": dict(STEP_TRACE=True, STEP_GRAPH=False),
         "graph": dict(STEP_TRACE=False, STEP_GRAPH=True)}


def engine(preset, mode, meter_kind=None):
    from vlfb.metrics import DeviceMeter
    cfg, model, eng, inputs, params, _ = build(preset, "bf16", overrides=SMALL)
    for k, v in MODES[mode].items():
        setattr(eng, k, v)
    meter = None
    if meter_kind == "topk":
        meter = DeviceMeter("topk", cfg.MODEL.NUM_CLASSES, ks=(1, 5), device=eng.device)
    elif meter_kind == "map":
        meter = DeviceMeter("map", cfg.MODEL.NUM_CLASSES, n_items=3, device=eng.device)
    if meter is not None:
        eng.attach_meter(meter)
    return eng, meter, inputs


@pytest.mark.parametrize("mode", ["eager", "trace", "graph"])
@pytest.mark.parametrize("preset,kind", [("epic_verb_r50_baseline", "topk"), ("charades_r50_baseline", "map")])
def test_six_metered_training_steps(preset, kind, mode):
    """(a) the counters equal the restatement applied to the twin's fetched probabilities after each step; (b) losses and
    every parameter are bit-identical with and without a meter; (d) under STEP_GRAPH the meter's calls are captured: a
    synchronising call inside update() would fail the capture"""
    eng, meter, inputs = engine(preset, mode, kind)
    twin, _, _ = engine(preset, "eager")
    labels = inputs["labels"]
    hits, rows, batches = [0, 0], 0, []
    for it in range(6):
        lr = 0.01 * (it + 1)
        eng.train_step(lr)
        twin.train_step(lr)
        prob = twin.fetch("prob")
        if kind == "topk":
            h, r = H.topk_hits(prob, labels, (1, 5))
            hits, rows = [hits[0] + h[0], hits[1] + h[1]], rows + r
        else:
            batches.append((prob, labels))
    if mode == "trace":
        assert eng._trace is not None and any(name in ("vlfb_topk_hits", "vlfb_scores_merge_max") for _, _, name in eng._trace)
    if mode == "graph":
        assert eng._graph is not None
    if kind == "topk":
        r = meter.read()
        print(preset, mode, r, hits, rows)
        assert [r["hits"][1], r["hits"][5]] == hits and r["rows"] == rows == 12
    else:
        _, _, cursor, _ = meter.counters()
        want = H.merge_max(batches, 3, prob.shape[1])
        assert cursor == 12 and meter.table.cpu().numpy().tobytes() == want[0].tobytes()
        assert np.array_equal(meter.labels.cpu().numpy(), want[1])
    la, lb = eng.recent_losses(), twin.recent_losses()
    assert la == lb and len(la) == 6
    torch.cuda.synchronize()
    assert torch.equal(eng.flat_param, twin.flat_param) and torch.equal(eng.flat_mom, twin.flat_mom)
    assert float(eng.flat_param.abs().sum()) > 0


def test_detaching_restores_the_launch_list():
    eng, meter, _ = engine("epic_verb_r50_baseline", "trace", "topk")
    for _ in range(3):
        eng.train_step(0.01)
    with_meter = [name for _, _, name in eng._trace]
    eng.attach_meter(None)
    for _ in range(2):
        eng.train_step(0.01)
    without = [name for _, _, name in eng._trace]
    assert [n for n in with_meter if n != "vlfb_topk_hits"] == without and len(with_meter) == len(without) + 1
    assert meter.read()["rows"] == 6


def test_charades_test_run_ends_in_the_restated_map(capsys):
    """(c) a test-mode run over 3 clips x 4 videos (+ the padding of the last batch, which the meter drops) through
    utils.metrics.MetricsCalculator"""
    import utils.metrics as M
    cfg, model, eng, inputs, params, _ = build("charades_r50_baseline", "bf16", overrides=TEST_SMALL, train=False)
    cfg.CHARADES.NUM_TEST_CLIPS, cfg.TEST.DATASET_SIZE, cfg.LOG_PERIOD = 3, 4, 2
    try:
        mc = M.MetricsCalculator(eng, "test")
        assert mc.num_test_clips == 3 and mc.meter.n_items == 4 and mc.meter.total_rows == 12
        rng = np.random.RandomState(3)
        video_labels = (rng.rand(4, 157) < 0.3).astype(np.int32)
        video_labels[:, 5] = 0
        timer = type("T", (), {"diff": 0.0, "average_time": 0.0})()
        seen = []
        for it in range(7):                                # 14 rows: 12 + 2 of padding
            pos = np.arange(2 * it, 2 * it + 2)
            lab = video_labels[pos % 4]
            eng.feed("data_test", rng.randn(*inputs["data"].shape).astype(np.float32))
            eng.feed("labels_test", lab)
            eng.forward()
            seen.append((eng.fetch("prob"), lab))
            mc.calculate_and_log_all_metrics_test(it, timer, 7)
        mc.finalize_metrics()
        out = capsys.readouterr().out
        assert out.count("| Test: [") == 4                 # iterations 2, 4, 6 and the last
        table, labels, pos, mismatches = H.merge_max(seen, 4, 157, total=12)
        assert mismatches == 0 and np.array_equal(labels, video_labels)
        want = H.mean_ap(table, labels)
        r = mc.results
        print(r["mean_ap"], want[1], r["rows_seen"])
        assert r["rows"] == 4 and r["rows_seen"] == 14 and r["label_mismatches"] == 0
        tol = H.bound(4)
        assert abs(r["mean_ap"] - want[1]) <= tol and abs(r["mean_wap"] - want[2]) <= tol and H.same(r["mean_auc"], want[0], tol)
        assert mc.full_map == r["mean_ap"] and mc.get_computed_metrics()["test_full_map"] == r["mean_ap"]
        mc.log_final_metrics(6, 7)
        assert "mAP:" in capsys.readouterr().out
    finally:
        del cfg.CHARADES["NUM_TEST_CLIPS"]


def test_training_loop_logs_the_reference_line(capsys):
    import utils.metrics as M
    cfg, model, eng, inputs, params, _ = build("epic_verb_r50_baseline", "bf16", overrides=SMALL)
    cfg.LOG_PERIOD = 3
    mc = M.MetricsCalculator(eng, "train")
    timer = type("T", (), {"diff": 0.0, "average_time": 0.0})()
    for it in range(6):
        eng.train_step(0.01)
        mc.calculate_and_log_all_metrics_train(it, timer)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("| Train ETA:")]
    assert len(lines) == 2 and all(" top1 " in l and " top5 " in l and " Loss " in l for l in lines)
    mc.finalize_metrics(is_train=True)
    assert mc.aggr_batch_size == 12 and 0.0 <= mc.get_computed_metrics()["train_err5"] <= mc.get_computed_metrics()["train_err"] <= 100.0


def test_ava_map_is_not_implemented():
    import utils.metrics as M
    cfg, model, eng, inputs, params, _ = build("ava_r50_lfb_nl", "bf16", overrides=SMALL)
    mc = M.MetricsCalculator(eng, "test")
    with pytest.raises(NotImplementedError, match="ava_evaluation"):
        mc.finalize_metrics()
