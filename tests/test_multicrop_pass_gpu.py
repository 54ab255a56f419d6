"""The device-resident AVA multi-crop pass (vlfb.multicrop.AvaMultiCropPass, run_ava_multi_crop) on the small AVA set-up of
tests/test_ava_pass_gpu.py: generated frame and box lists, 3 videos, 5 keyframes with RoI counts 1, 3, 2, 3, 1, batches of 2
(the last one padded), T = 8, fp32, scales 56 / 64 / 80 with crops of at most 64, frames of 40 x 100 out of a
FrameStore.fetch.

The checker is AvaMultiCropTester.run on the SAME engines (the pass builds them through its tester), fed the same clips as
stacked arrays minibatch by minibatch with the same number of RoI rows: both feeds use the same preprocessing arithmetic
(include/vlfb.h: "with index[t] = t the output is theirs bit for bit"), so the 18 logit sets must be bit-identical and the
merged scores agree at rtol = 1e-12 (the device's fp64 exp against the host's: a few ulp)."""
import os

import numpy as np
import pytest
import torch

import ava_eval_ref as R
import clip_loader_cases as cases

pytestmark = pytest.mark.gpu

T, N = 8, 2
H, W, FRAMES = 40, 100, 130
SCALES, MAX_CROP = [56, 64, 80], 64
ROWS = [("V0", 902, 1), ("V0", 903, 3), ("V1", 903, 2), ("V2", 902, 3), ("V2", 904, 1)]
# (x1, y1, x2, y2): at scale 80 (nc = 0.32) the first is seen by the left crop only, the second by left and centre, the
# third by all three, the fourth by the centre only
POOL = [(0.05, 0.10, 0.30, 0.80), (0.10, 0.20, 0.50, 0.90), (0.20, 0.05, 0.80, 0.60), (0.40, 0.30, 0.60, 0.95),
        (0.55, 0.10, 0.97, 0.70), (0.02, 0.40, 0.45, 0.85)]
UNSEEN = (0.325, 0.2, 0.335, 0.8)            # at scale 80: right of the left crop, left of the centre crop, flipped or not
DUMMY = [0.3, 0.3, 0.6, 0.6]
RTOL = 1e-12


def _write_inputs(tmp_path, rows=ROWS, unseen_in=None):
    rng = np.random.default_rng(7)
    lines, k = [], 0
    for i, (name, sec, n) in enumerate(rows):
        for j in range(n):
            b = UNSEEN if (unseen_in == i and j == 0) else POOL[k % len(POOL)]
            k += 1
            lines.append("%s,%d,%.3f,%.3f,%.3f,%.3f,,%.2f" % ((name, sec) + tuple(b) + (rng.uniform(0.9, 1.0),)))
    lines.append("V1,902,0.1,0.1,0.5,0.5,,0.50")                                   # below the threshold: no keyframe
    with open(os.path.join(str(tmp_path), "boxes.csv"), "w") as f:
        f.write("\n".join(lines) + "\n")
    frames = ["original_vido_id video_id frame_id path labels"]
    for vi in range(len({name for name, _, _ in rows})):                           # (the index wants boxes for every listed video)
        frames += ['V%d %d %d V%d/%06d.jpg ""' % (vi, vi, k, vi, k + 1) for k in range(FRAMES)]
    with open(os.path.join(str(tmp_path), "frames.csv"), "w") as f:
        f.write("\n".join(frames) + "\n")
    return [rng.integers(0, 256, (FRAMES, H, W, 3)).astype(np.uint8) for _ in range(3)]


def _cfg(preset, extra=()):
    return cases.loader_cfg(preset, clips=N, frames=T, extra=["AVA.TEST_MULTI_CROP", True, "AVA.TEST_MULTI_CROP_SCALES",
                                                               list(SCALES)] + list(extra))


def _point_cfg_at(cfg, tmp_path):
    a = cfg.AVA
    a.FRAME_LIST_DIR = a.ANNOTATION_DIR = str(tmp_path)
    a.TRAIN_LISTS = a.TEST_LISTS = ["frames.csv"]
    a.TRAIN_BOX_LISTS = a.TEST_BOX_LISTS = a.TRAIN_LFB_BOX_LISTS = a.TEST_LFB_BOX_LISTS = ["boxes.csv"]
    cfg.CHECKPOINT.DIR = cfg.LFB.LOAD_LFB_PATH = str(tmp_path)
    a.FULL_EVAL = True                                                             # what the driver sets (test_net.py:59, :101)
    a.DETECTION_SCORE_THRESH = a.DETECTION_SCORE_THRESH_EVAL[0]


def _store_maker(videos):
    from datasets.frame_store import FrameStore

    def make_store(device, stream):
        st = FrameStore(H, W, 4 * N * T, device, stream)
        st.fetch = lambda v, f: videos[v][f]
        return st
    return make_store


def _groundtruth(index, C):
    """read_csv's triple: most keyframes' boxes with two labels each (one box moved away: a false positive), and a key with
    ground truth only"""
    rng = np.random.RandomState(4)
    gt_boxes, gt_labels = {}, {}
    for v, sec, _ in index.keyframe_indices:
        key = "%s,%04d" % (index.video_idx_to_name[v], sec)
        for n, (box, _) in enumerate(index.boxes_and_labels[v][sec]):
            g = box if (n + sec) % 3 else [box[0] * 0.2, box[1], box[2] * 0.2, box[3]]
            for cid in rng.choice(np.arange(1, C + 1), 2, replace=False):
                gt_boxes.setdefault(key, []).append([g[1], g[0], g[3], g[2]])
                gt_labels.setdefault(key, []).append(int(cid))
    gt_boxes["V1,0950"], gt_labels["V1,0950"] = [[0.1, 0.1, 0.5, 0.5]], [7]
    return gt_boxes, gt_labels, {k: [1.0] * len(v) for k, v in gt_labels.items()}


def _tester_scores(p, index, videos, lfb=None):
    """AvaMultiCropTester.run over the pass's engines, minibatch by minibatch, with dummy boxes behind the last clip's so
    that every minibatch has the planned number of rows.  -> (scores of the real rows, per minibatch (used rows, per_pass))"""
    size = index.get_db_size()
    scores, passes = [], []
    for lo in range(0, size, N):
        infos = index.get_minibatch_info(list(range(lo, min(lo + N, size))))
        clips = [videos[c.video][np.array(c.seq)] for c in infos]
        boxes = [np.asarray(c.boxes, dtype=np.float64).reshape(-1, 4) for c in infos]
        used = sum(len(b) for b in boxes)
        fed = list(boxes)
        fed[-1] = np.concatenate([boxes[-1], np.tile(DUMMY, (p.rows - used, 1))])
        got, per_pass = p.tester.run(clips, fed, lfb)
        assert got.shape == (p.rows, p.cols)
        passes.append((used, per_pass))
        r = 0
        for n, b in enumerate(boxes):
            if lo + n < size:                                                      # not a clip that only pads the batch
                scores.append(got[r:r + len(b)])
            r += len(b)
    return np.concatenate(scores), passes


def _first_differing_view(trace, passes, rows):
    """the pass's 18 `pred` sets per minibatch against the tester's, bit for bit on the real rows"""
    for pos, view, pred in trace:
        used, per_pass = passes[pos // rows]
        mine = pred.float().cpu().numpy().reshape(rows, -1).astype(np.float64)[:used]
        theirs = per_pass[(view.scale, view.flip, view.shift)][:used]
        if not np.array_equal(mine, theirs):
            return "minibatch %d %r: max |diff| %.3e" % (pos // rows, tuple(view), float(np.abs(mine - theirs).max()))
    return None


def test_the_whole_pass_against_the_tester_and_the_driver_from_a_parameter_file(tmp_path, monkeypatch):
    import utils.ava_eval_helper as A
    from datasets import ava
    from oracle import model as om
    from utils import checkpoints as ck
    from vlfb import multicrop as mc
    monkeypatch.chdir(tmp_path)                                   # (evaluate_ava writes detections_<name>.csv where it runs)
    videos = _write_inputs(tmp_path)
    with _cfg("ava_r50_baseline") as cfg:
        _point_cfg_at(cfg, tmp_path)
        C = cfg.MODEL.NUM_CLASSES
        index = ava.AvaIndex.from_cfg("test", False)
        size = index.get_db_size()
        assert size == 5 and size % N and [len(index.boxes_and_labels[v][s]) for v, s, _ in index.keyframe_indices] == [1, 3, 2, 3, 1]
        all_boxes = np.array([b for v, s, _ in index.keyframe_indices for b, _ in index.boxes_and_labels[v][s]])
        counts = set()
        for scale in SCALES:
            for flip in (False, True):
                n_valid = mc.shift_validity(all_boxes, flip, scale, H, W, MAX_CROP).sum(axis=0)
                assert n_valid.min() >= 1                                          # every box is seen by some crop of every pass
                counts |= {(scale, flip, int(n)) for n in n_valid}
        assert any({(s, f, 1), (s, f, 2), (s, f, 3)} <= counts for s in SCALES for f in (False, True))

        groundtruth = _groundtruth(index, C)
        excluded = {"V0,0902"}
        whitelist = set(range(1, C + 1)) - {2, 16, 40}
        categories = [{"id": i, "name": "action %d" % i} for i in range(1, C + 1)]
        params = om.synth_params(cfg, seed=3)
        before = (cfg.TEST.SCALE, cfg.TEST.CROP_SIZE, cfg.AVA.FORCE_TEST_FLIP)

        p = mc.AvaMultiCropPass(index, _store_maker(videos), params, dtype="fp32", max_crop=MAX_CROP)
        assert len(p.views) == 18 and len(p.engines) == 2 and p.rows == N * 3
        p.trace = []
        res = p.run(groundtruth, excluded, whitelist)
        assert (cfg.TEST.SCALE, cfg.TEST.CROP_SIZE, cfg.AVA.FORCE_TEST_FLIP) == before

        # rows: the padded clip's rows and the rows behind the last box are absent, every issued row is accounted for
        n_batches = -(-size // N)
        assert res["rows_seen"] == n_batches * p.rows
        assert res["rows"].tolist() == [0, 1, 2, 3, 6, 7, 8, 9, 10, 12]
        assert res["keys"] == ["V0,0902"] + ["V0,0903"] * 3 + ["V1,0903"] * 2 + ["V2,0902"] * 3 + ["V2,0904"]
        assert np.array_equal(res["boxes"], all_boxes) and res["scores"].shape == (10, C) and res["scores"].dtype == np.float64
        assert res["detections"] == 9                                              # 10 real rows, one of an excluded key
        # decode once, not 18 times
        need = {(c.video, int(f)) for i in range(size) for c in index.get_minibatch_info([i])[:1] for f in c.seq}
        assert p.store.fetched == len(need) and p.store.requested == n_batches * N * T

        # the tester on the same engines
        want, passes = _tester_scores(p, index, videos)
        assert len(p.trace) == 18 * n_batches
        differing = _first_differing_view(p.trace, passes, p.rows)
        assert differing is None, "the pass and the tester feed different logits: " + differing
        rel = np.abs(res["scores"] - want) / np.abs(want)
        print("merged scores: max rel diff to the tester %.3e" % float(rel.max()))
        assert np.allclose(res["scores"], want, rtol=RTOL, atol=0)
        assert np.isfinite(want).all() and want.min() > 0 and want.max() < 2 * len(SCALES)

        # the meter: float32 of the merged scores, scored as evaluate_ava scores them
        table = p.meter.table.cpu().numpy()
        assert np.array_equal(table[res["rows"]], res["scores"].astype(np.float32))
        boxes5 = np.concatenate([np.zeros((10, 1)), res["boxes"]], axis=1)
        wanted = [c for c in categories if c["id"] in whitelist]
        ev = A.run_evaluation(wanted, groundtruth, A.AvaDetections(res["scores"].astype(np.float32), res["boxes"], res["keys"]),
                              excluded, verbose=False)
        n_scored = 0
        for c in wanted:
            a, b = res["ap"][c["id"] - 1], ev[A.CATEGORY_KEY + c["name"]]
            assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= R.bound(n_batches * p.rows), c
            n_scored += not np.isnan(a)
        assert n_scored > 5
        got_map = A.evaluate_ava(res["scores"].astype(np.float32), boxes5, res["metadata"], excluded, whitelist, categories,
                                 groundtruth=groundtruth, video_idx_to_name=index.video_idx_to_name, name="mc")
        assert abs(got_map - res["mean_ap"]) <= R.bound(n_batches * p.rows) and 0.0 < res["mean_ap"] <= 1.0

        # the driver: the same pass from a parameter file, and the merged score file
        path = os.path.join(str(tmp_path), "model.pkl")
        ck.write_blobs(path, dict(params, lr=np.array([0.1], dtype=np.float32)))
        del p
        out = mc.run_ava_multi_crop(path, _store_maker(videos), groundtruth, excluded, whitelist, dtype="fp32", max_crop=MAX_CROP,
                                    out_csv=os.path.join(str(tmp_path), "final_multi_crop_testing_results.csv"))
        assert list(out) == [cfg.AVA.DETECTION_SCORE_THRESH_EVAL[0]]
        drv = out[cfg.AVA.DETECTION_SCORE_THRESH_EVAL[0]]
        assert drv["mean_ap"] == res["mean_ap"] and np.array_equal(drv["scores"], res["scores"])
        lines = open(drv["csv"]).read().splitlines()
        assert len(lines) == 10 * len(whitelist)
        k = 0
        for r in range(10):
            for cid in sorted(whitelist):
                f = lines[k].split(",")
                assert ",".join(f[:2]) == res["keys"][r] and int(f[6]) == cid
                assert [float(x) for x in f[2:6]] == [float("%.03f" % x) for x in res["boxes"][r]]
                assert f[7] == "%f" % res["scores"][r, cid - 1] and float(f[7]) == float("%f" % res["scores"][r, cid - 1])
                k += 1


def test_with_a_bank_every_view_reads_one_draw_of_the_window(tmp_path):
    """ava_r50_lfb_nl, one minibatch: the window of every RoI is sampled once into both engines' `lfb` blobs, and the scores
    are the tester's when it is given that sampled bank"""
    from datasets import ava
    from oracle import model as om
    from vlfb import multicrop as mc
    from vlfb.lfb_bank import DeviceBank
    videos = _write_inputs(tmp_path, rows=ROWS[:2])
    with _cfg("ava_r50_lfb_nl", extra=["LFB.WINDOW_SIZE", 4]) as cfg:
        _point_cfg_at(cfg, tmp_path)
        index = ava.AvaIndex.from_cfg("test", False)
        assert index.get_db_size() == 2
        bank = DeviceBank(3, 3, 4, cfg.LFB.LFB_DIM, "fp32", step_base=902)
        rng = np.random.default_rng(3)
        feats = torch.as_tensor(np.maximum(rng.standard_normal((10, cfg.LFB.LFB_DIM)), 0).astype(np.float32) * 0.5).cuda()
        bank.append(feats, [0, 0, 0, 0, 1, 1, 2, 2, 2, 2], [902, 903, 903, 903, 903, 903, 902, 902, 902, 904])
        params = om.synth_params(cfg, seed=3)
        p = mc.AvaMultiCropPass(index, _store_maker(videos), params, dtype="fp32", max_crop=MAX_CROP, bank=bank)
        assert len(p.engines) == 2
        p.trace = []
        res = p.run(({}, {}, {}))
        assert res["rows"].tolist() == [0, 1, 2, 3] and res["rows_seen"] == p.rows
        blobs = []
        for model, eng in p.engines:
            name = [n for n in model.input_blob_names if n.startswith("lfb")][0]
            blobs.append(eng.fetch(name))
        k = cfg.LFB.WINDOW_SIZE * cfg.AVA.LFB_MAX_NUM_FEAT_PER_STEP
        assert blobs[0].shape == (p.rows, k, cfg.LFB.LFB_DIM)
        assert np.array_equal(blobs[0], blobs[1]) and np.abs(blobs[0][:4]).max() > 0 and not blobs[0][4:].any()
        assert np.array_equal(blobs[0][1], blobs[0][2])                            # RoIs of one clip share the clip's draw
        want, passes = _tester_scores(p, index, videos, lfb=blobs[0])
        differing = _first_differing_view(p.trace, passes, p.rows)
        assert differing is None, "the pass and the tester feed different logits: " + differing
        assert np.allclose(res["scores"], want, rtol=RTOL, atol=0)


def test_a_box_outside_every_crop_of_a_pass_is_reported_by_its_image_key(tmp_path):
    from datasets import ava
    from oracle import model as om
    from vlfb import hip
    from vlfb import multicrop as mc
    videos = _write_inputs(tmp_path, rows=ROWS[:2], unseen_in=1)
    with _cfg("ava_r50_baseline") as cfg:
        _point_cfg_at(cfg, tmp_path)
        index = ava.AvaIndex.from_cfg("test", False)
        boxes = np.array([b for v, s, _ in index.keyframe_indices for b, _ in index.boxes_and_labels[v][s]])
        seen = np.stack([mc.shift_validity(boxes, f, s, H, W, MAX_CROP).any(axis=0) for s in SCALES for f in (False, True)])
        assert seen[:4].all() and seen[4:, [0, 2, 3]].all() and not seen[4:, 1].any()   # unseen at scale 80 only, flipped or not
        p = mc.AvaMultiCropPass(index, _store_maker(videos), om.synth_params(cfg, seed=3), dtype="fp32", max_crop=MAX_CROP)
        for args in ava.minibatch_source(index, p.store, np.random):
            p.run_minibatch(*args)
        with pytest.raises(hip.VlfbError, match=r"1 box\(es\) lie outside every crop.*V0,0903") as e:
            p.finish(({}, {}, {}))
        assert "V0,0902" not in str(e.value)
        acc = p.acc.view(p.n_items, p.cols).cpu().numpy()
        assert np.isnan(acc[1]).all() and np.isfinite(acc[[0, 2, 3]]).all()
        assert p.valid.view(6, p.n_items)[:, :4].cpu().numpy().tolist() == [
            mc.shift_validity(boxes, f, s, H, W, MAX_CROP).astype(np.uint8).T.dot([1, 2, 4]).tolist()
            for s in SCALES for f in (False, True)]
