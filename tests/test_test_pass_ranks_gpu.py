"""The test pass and the in-training evaluation shared by two ranks (vlfb.passes.run_pass_ranks, the per-rank meters of
utils.metrics.MetricsCalculator, vlfb_rows_interleave): with NUM_GPUS 2 and BATCH_SIZE 2n the two ranks issue exactly the
slices of one process with NUM_GPUS 1 and BATCH_SIZE n, a test-mode row does not depend on its batch-mates, and so score
tables, kept predictions, counters and final figures are equal in bits.

Set-up as tests/test_lfb_pass_ranks_gpu.py: two spawned processes share cuda:0 over gloo, every case in one spawn, errors
come back through the queue, each process exits after destroy_process_group.  The parent runs the single-process passes.
Sizes give an odd number P of slices (rank 1 has one slice fewer), one Charades case has P = 1 (none for rank 1), and
LOG_PERIOD is 1: a collective that sat in a per-slice callback would leave rank 0 waiting in the last global iteration."""
import contextlib
import os
import pickle
import socket

import numpy as np
import pytest
import torch

import clip_loader_cases as cases
import frame_pass_cases as fc
import test_ava_pass_gpu as avap
from test_lfb_pass_ranks_gpu import _collect, _setup_paths

pytestmark = pytest.mark.gpu

WORLD = 2
SFX = "_final_test"
# name -> (preset, clips per GPU, clips of the walk)
CASES = {
    "charades": ("charades_r50_baseline", 2, 9),       # 3 videos x 3 clips: P = 5, the last slice padded
    "tiny": ("charades_r50_baseline", 4, 3),           # 1 video x 3 clips in one padded slice: P = 1
    "epic": ("epic_verb_r50_baseline", 2, 5),          # 5 annotated segments: P = 3, the last slice padded
    "ava": ("ava_r50_baseline", 2, 5),                 # 5 keyframes: P = 3, the last slice padded
}
CHARADES_LENGTHS = {"charades": [40, 23, 31], "tiny": [40]}
EPIC_NAMES, EPIC_LENGTHS = ["P26_01", "P27_02"], [40, 30]
EPIC_ROWS = [("P26", "P26_01", 0.10, 0.50, 3, 17), ("P26", "P26_01", 0.40, 1.10, 120, 5), ("P27", "P27_02", 0.00, 0.30, 7, 351),
             ("P27", "P27_02", 0.50, 0.90, 0, 0), ("P26", "P26_01", 0.90, 1.30, 64, 200)]
EXCLUDED = {"V0,0902"}


def slices(name):
    _, n, clips = CASES[name]
    return -(-clips // n)


@contextlib.contextmanager
def _cfg(name, root, num_gpus):
    preset, n, _ = CASES[name]
    frames = avap.T if name == "ava" else fc.T
    extra = ["NUM_GPUS", num_gpus, "TEST.BATCH_SIZE", n * num_gpus]
    if name != "ava":
        extra = fc.EXTRA + extra + ["CHARADES.NUM_TEST_CLIPS_FINAL_EVAL", 3]
    with cases.loader_cfg(preset, clips=n, frames=frames, extra=extra) as cfg:
        d = os.path.join(root, name)
        if name == "ava":
            avap._point_cfg_at(cfg, d)
            cfg.AVA.FULL_EVAL = True
            cfg.AVA.DETECTION_SCORE_THRESH = 0.8
            cfg.TEST.DATASET_SIZE = 5
        else:
            fc.point_cfg_at(cfg, d)
            cfg.TEST.DATASET_SIZE = 5 if name == "epic" else len(CHARADES_LENGTHS[name])
        cfg.LOG_PERIOD = 1
        assert cfg.TEST.BATCH_SIZE == n * num_gpus and cfg.NUM_GPUS == num_gpus
        yield cfg


def _videos(name, ava_videos):
    if name == "ava":
        return ava_videos
    if name == "epic":
        vids = fc.videos(EPIC_LENGTHS, seed=8)
        return {n: v for n, v in zip(EPIC_NAMES, vids)}
    return fc.videos(CHARADES_LENGTHS[name], seed=4)


def _params_file(root, name):
    return os.path.join(root, name, "model.pkl")


def _ava_groundtruth(index, C):
    """read_csv's triple over the index's own boxes, two labels a box, every third box moved away (a false positive)"""
    rng = np.random.RandomState(4)
    gt_boxes, gt_labels = {}, {}
    for v, sec, _ in index.keyframe_indices:
        key = "%s,%04d" % (index.video_idx_to_name[v], sec)
        for n, (box, _) in enumerate(index.boxes_and_labels[v][sec]):
            g = box if (n + sec) % 3 else [box[0] * 0.2, box[1], box[2] * 0.2, box[3]]
            for cid in rng.choice(np.arange(1, C + 1), 2, replace=False):
                gt_boxes.setdefault(key, []).append([g[1], g[0], g[3], g[2]])
                gt_labels.setdefault(key, []).append(int(cid))
    return gt_boxes, gt_labels, {k: [1.0] * len(v) for k, v in gt_labels.items()}


def _run_case(name, root, ava_videos, out_dir):
    """the pass of case `name` under the loaded cfg -> a dict of plain numpy / Python values"""
    from vlfb import test_pass, train_pass
    vids = _videos(name, ava_videos)
    make_store = fc.store_factory(lambda v, f: vids[v][f])
    kw = dict(max_src_hw=(fc.H, fc.W))
    if name == "ava":
        from core.config import config as cfg
        from datasets import ava
        from vlfb import synth
        C = cfg.MODEL.NUM_CLASSES
        gt = _ava_groundtruth(ava.AvaIndex.from_cfg(cfg.TEST.DATA_TYPE, False), C)
        w = train_pass.create_wrapper(False, make_store, None, dtype="bf16", ava_groundtruth=gt, excluded_keys=EXCLUDED,
                                      class_whitelist=set(range(1, C + 1)) - {2, 16}, **kw)
        w.engine.feed_params({k: v for k, v in synth.params(w.model, seed=2).items() if k in w.engine.param_views})
        ran = train_pass.eval_pass(w)
        r = w.meter.results
        return dict(ran=ran, ap=r["ap"].copy(), n_gt=r["n_gt"].copy(), full_map=w.meter.full_map, rows_seen=r["rows_seen"],
                    detections=r["detections"], best_map=w.meter.best_map)
    if name == "epic":
        mc = test_pass.test_one_crop(_params_file(root, name), make_store, out_dir=out_dir, **kw)
        with open(os.path.join(out_dir, "epic_predictions_final.pkl"), "rb") as f:
            data = f.read()
        return dict(file=data, err=mc.avg_err, err5=mc.avg_err5, rows=mc.aggr_batch_size, pred=mc.predictions[0].copy(),
                    labels=mc.predictions[1].copy())
    mc = test_pass.test_net(_params_file(root, name), make_store, **kw)
    meter = mc.merged if getattr(mc, "merged", None) is not None else mc.meter
    return dict(table=fc.bits(meter.table), labels=meter.labels.cpu().numpy().copy(), full_map=mc.full_map,
                rows_seen=mc.results["rows_seen"], rows=mc.results["rows"], all_aps=mc.results["all_aps"].copy(),
                mismatches=mc.results["label_mismatches"])


def _worker(rank, world, port, q, root, ava_videos):
    try:
        _worker_body(rank, world, port, q, root, ava_videos)
    except BaseException:
        import traceback
        q.put((rank, {"_error": traceback.format_exc()}))
        raise


def _worker_body(rank, world, port, q, root, ava_videos):
    _setup_paths()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), VLFB_FORCE_DEVICE="0", VLFB_DIST_BACKEND="gloo")
    from vlfb import dist
    from vlfb.engine import Engine
    dist.init_from_env()
    calls, dumps = [0], [0]
    forward, dump = Engine.forward, pickle.dump

    def counted(self):
        calls[0] += 1
        return forward(self)

    def counted_dump(obj, f, *a, **k):
        if getattr(f, "name", "").endswith("epic_predictions_final.pkl"):
            dumps[0] += 1
        return dump(obj, f, *a, **k)
    Engine.forward = counted
    pickle.dump = counted_dump
    out = {}
    for name in CASES:
        with _cfg(name, root, WORLD):
            calls[0] = 0
            out[name] = dict(_run_case(name, root, ava_videos, os.path.join(root, name, "out")), forwards=calls[0])
    out["dumps"] = dumps[0]
    q.put((rank, out))
    dist.barrier()
    torch.distributed.destroy_process_group()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    import torch.multiprocessing as mp
    from utils import checkpoints as ck
    _setup_paths()
    root = str(tmp_path_factory.mktemp("pass_ranks"))
    ava_videos = None
    for name in CASES:
        d = os.path.join(root, name)
        os.makedirs(os.path.join(d, "out"))
        os.makedirs(os.path.join(d, "single"))
        with _cfg(name, root, 1):
            if name == "ava":
                ava_videos = avap._write_inputs(d)
                continue
            if name == "epic":
                fc.write_epic_lists(d, EPIC_NAMES, EPIC_LENGTHS)
                fc.write_epic_annotations(d, EPIC_ROWS)
            else:
                lengths = CHARADES_LENGTHS[name]
                rng = np.random.default_rng(11)
                labels = [[[int(x) for x in rng.choice(157, int(rng.integers(0, 3)), replace=False)] for _ in range(n)] for n in lengths]
                fc.write_charades_lists(d, lengths, labels)
            _, eng, params = fc.engine(SFX)
            ck.write_blobs(_params_file(root, name), dict(params, lr=np.array([0.1], dtype=np.float32)))
            del eng
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, WORLD, port, q, root, ava_videos)) for r in range(WORLD)]
    for p in procs:
        p.start()
    ranks = dict(_collect(q, procs, WORLD))
    single = {}
    for name in CASES:
        with _cfg(name, root, 1):
            single[name] = _run_case(name, root, ava_videos, os.path.join(root, name, "single"))
    return ranks, single, root


def _forwards(runs, name):
    from vlfb.lfb_pass import rank_iterations
    ranks = runs[0]
    got = [ranks[r][name]["forwards"] for r in range(WORLD)]
    assert got == [len(rank_iterations(slices(name), r, WORLD)) for r in range(WORLD)], (name, got)
    return got


@pytest.mark.parametrize("name", ["charades", "tiny"])
def test_charades_test_net_on_two_ranks_equals_the_single_process(runs, name):
    ranks, single, _ = runs
    want = single[name]
    videos = len(CHARADES_LENGTHS[name])
    assert want["rows"] == videos and want["rows_seen"] == slices(name) * CASES[name][1] and want["mismatches"] == 0
    assert float(np.abs(want["table"]).max()) > 0
    for rank in range(WORLD):
        got = ranks[rank][name]
        assert np.array_equal(got["table"], want["table"]), rank
        assert np.array_equal(got["labels"], want["labels"]), rank
        assert got["full_map"] == want["full_map"] and got["all_aps"].tobytes() == want["all_aps"].tobytes(), rank
        assert got["rows_seen"] == want["rows_seen"] and got["rows"] == want["rows"] and got["mismatches"] == 0, rank
    assert _forwards(runs, name) == ([3, 2] if name == "charades" else [1, 0])


def test_epic_predictions_are_the_single_process_file_written_once(runs):
    ranks, single, root = runs
    want = single["epic"]
    assert len(want["file"]) > 0 and want["pred"].shape == (5, 125) and want["rows"] == 6
    assert want["labels"].tolist() == [r[4] for r in EPIC_ROWS]
    with open(os.path.join(root, "epic", "out", "epic_predictions_final.pkl"), "rb") as f:
        assert f.read() == want["file"]
    for rank in range(WORLD):
        got = ranks[rank]["epic"]
        assert got["file"] == want["file"], rank
        assert got["pred"].tobytes() == want["pred"].tobytes() and np.array_equal(got["labels"], want["labels"]), rank
        assert (got["err"], got["err5"], got["rows"]) == (want["err"], want["err5"], want["rows"]), rank
    assert [ranks[r]["dumps"] for r in range(WORLD)] == [1, 0]
    assert _forwards(runs, "epic") == [2, 1]


def test_ava_eval_pass_on_two_ranks_equals_the_single_process(runs):
    ranks, single, _ = runs
    want = single["ava"]
    assert want["ran"] == 3 and want["detections"] > 0 and 0.0 < want["full_map"] <= 1.0
    for rank in range(WORLD):
        got = ranks[rank]["ava"]
        assert got["ap"].tobytes() == want["ap"].tobytes() and np.array_equal(got["n_gt"], want["n_gt"]), rank
        assert got["full_map"] == want["full_map"] == got["best_map"], rank
        assert got["rows_seen"] == want["rows_seen"] and got["detections"] == want["detections"], rank
        assert got["ran"] == 2                                          # global iterations: ceil(3 / 2)
    assert _forwards(runs, "ava") == [2, 1]


def test_num_gpus_without_a_group_of_that_size_is_refused(tmp_path, monkeypatch):
    """today's silent pass over 1 / NUM_GPUS of the split"""
    from utils import checkpoints as ck
    from vlfb import hip, test_pass
    from vlfb.engine import Engine
    d = os.path.join(str(tmp_path), "charades")
    os.makedirs(d)
    forwards = []
    monkeypatch.setattr(Engine, "forward", lambda self: forwards.append(1))
    with _cfg("charades", str(tmp_path), 2):
        fc.write_charades_lists(d, CHARADES_LENGTHS["charades"])
        _, eng, params = fc.engine(SFX)
        ck.write_blobs(_params_file(str(tmp_path), "charades"), dict(params, lr=np.array([0.1], dtype=np.float32)))
        del eng
        with pytest.raises(hip.VlfbError, match="process group of 2 ranks"):
            test_pass.test_one_crop(_params_file(str(tmp_path), "charades"), fc.store_factory(lambda v, f: None),
                                    max_src_hw=(fc.H, fc.W))
    assert not forwards                                                  # refused before the first slice
