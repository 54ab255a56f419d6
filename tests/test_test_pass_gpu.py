"""The test driver (vlfb.test_pass) on the small engines of tests/frame_pass_cases.py, against the same chain wired by hand
from product calls: the clips of the index preprocessed one by one, Engine.feed, forward, the probabilities fetched after
every iteration.  Same kernels on the same bytes: tables and files are compared bit for bit, hit counts exactly."""
import os
import pickle

import numpy as np
import pytest
import torch

import clip_loader_cases as cases
import frame_pass_cases as fc
from test_topk_keep_gpu import rank_rule_hits

pytestmark = pytest.mark.gpu
N, T = fc.N, fc.T
SFX = "_final_test"
TIMER = type("T", (), {"diff": 0.0, "average_time": 0.0})()


def _write_params(tmp_path, params):
    from utils import checkpoints as ck
    path = os.path.join(str(tmp_path), "model.pkl")
    ck.write_blobs(path, dict(params, lr=np.array([0.1], dtype=np.float32)))
    return path


def test_charades_test_net_equals_the_hand_wired_chain(tmp_path):
    """2 videos x 6 clips (3 shifts x 2 segments): mAP and merged table; CHARADES.NUM_TEST_CLIPS is put back"""
    import utils.metrics as M
    from datasets import charades
    from vlfb import test_pass
    lengths = [40, 23]
    rng = np.random.default_rng(11)
    labels = [[[int(x) for x in rng.choice(157, int(rng.integers(0, 3)), replace=False)] for _ in range(n)] for n in lengths]
    vids = fc.videos(lengths, seed=4)
    with cases.loader_cfg("charades_r50_baseline", clips=N, frames=T, extra=fc.EXTRA + ["CHARADES.NUM_TEST_CLIPS_FINAL_EVAL", 6]) as cfg:
        fc.point_cfg_at(cfg, tmp_path)
        fc.write_charades_lists(tmp_path, lengths, labels)
        cfg.TEST.DATASET_SIZE = 2
        assert "NUM_TEST_CLIPS" not in cfg.CHARADES
        cfg.CHARADES.NUM_TEST_CLIPS = 6
        try:
            index = charades.CharadesIndex.from_cfg("test", False)
            assert index.get_db_size() == 12
            m, eng, params = fc.engine(SFX)
            mc = M.MetricsCalculator(eng, "test")
            for it, lo in enumerate(range(0, 12, N)):
                infos = index.get_minibatch_info(list(range(lo, lo + N)))
                fc.feed_clips(eng, SFX, infos, lambda v: vids[v])
                eng.feed("labels" + SFX, np.stack([charades.construct_label_array(c.labels) for c in infos]))
                eng.forward()
                mc.calculate_and_log_all_metrics_test(it, TIMER, 6)
            mc.finalize_metrics()
            want_table, want_labels, want = mc.meter.table.cpu().numpy().copy(), mc.meter.labels.cpu().numpy().copy(), dict(mc.results)
        finally:
            del cfg.CHARADES["NUM_TEST_CLIPS"]
        assert want["rows"] == 2 and want["rows_seen"] == 12 and float(np.abs(want_table).max()) > 0
        path = _write_params(tmp_path, params)
        del mc, eng
        make_store = fc.store_factory(lambda v, f: vids[v][f])
        got = test_pass.test_net(path, make_store, max_src_hw=(fc.H, fc.W))
        assert "NUM_TEST_CLIPS" not in cfg.CHARADES
        assert got.num_test_clips == 6 and got.meter.total_rows == 12
        assert got.meter.table.cpu().numpy().tobytes() == want_table.tobytes()
        assert np.array_equal(got.meter.labels.cpu().numpy(), want_labels)
        assert got.results["mean_ap"] == want["mean_ap"] == got.full_map and got.results["rows_seen"] == 12
        assert got.results["label_mismatches"] == 0
        # a value that was set before the call comes back as it was
        cfg.CHARADES.NUM_TEST_CLIPS = 3
        try:
            with pytest.raises(AssertionError, match="No params files"):
                test_pass.test_net("", make_store)
            assert cfg.CHARADES.NUM_TEST_CLIPS == 3
        finally:
            del cfg.CHARADES["NUM_TEST_CLIPS"]


# five test annotations (participants beyond P25) at batch 2: the last batch is padded with its first clip; the rows of
# the training participants are what the action prior is counted from
NAMES, LENGTHS = ["P26_01", "P27_02"], [40, 30]
TEST_ROWS = [("P26", "P26_01", 0.10, 0.50, 3, 17), ("P26", "P26_01", 0.40, 1.10, 120, 5), ("P27", "P27_02", 0.00, 0.30, 7, 351),
             ("P27", "P27_02", 0.50, 0.90, 0, 0), ("P26", "P26_01", 0.90, 1.30, 64, 200)]


def _train_rows():
    rng = np.random.default_rng(6)
    pairs = [(3, 17), (120, 5), (7, 351), (0, 0), (64, 200), (3, 5), (7, 17), (64, 0)]
    return [("P%02d" % rng.integers(1, 26), "P01_01", 0.0, 1.0) + pairs[int(rng.integers(0, len(pairs)))] for _ in range(40)]


def _epic_pass(tmp_path, class_type, vids):
    """-> (the predictions file of test_one_crop, the labels in annotation order); asserts the file against the hand chain"""
    import utils.metrics as M
    from datasets import epic
    from vlfb import test_pass
    out_dir = os.path.join(str(tmp_path), class_type)
    os.makedirs(out_dir)
    with cases.loader_cfg("epic_%s_r50_baseline" % class_type, clips=N, frames=T, extra=fc.EXTRA) as cfg:
        fc.point_cfg_at(cfg, tmp_path)
        cfg.TEST.DATASET_SIZE = 5
        cols = cfg.MODEL.NUM_CLASSES
        index = epic.EpicIndex.from_cfg("test", False, shift=cfg.TEST.CROP_SHIFT)
        assert index.get_db_size() == 5 and [a[0] for a in index.annotations] == [r[0] for r in TEST_ROWS]
        want_labels = np.array([r[4 if class_type == "verb" else 5] for r in TEST_ROWS], dtype=np.int32)
        m, eng, params = fc.engine(SFX)
        fetched, fed = [], []
        for lo in range(0, 5, N):
            infos = index.get_minibatch_info(list(range(lo, min(lo + N, 5))))
            assert len(infos) == N
            fc.feed_clips(eng, SFX, infos, lambda v: vids[NAMES.index(v)])
            eng.feed("labels" + SFX, np.array([c.labels for c in infos], dtype=np.int32))
            eng.forward()
            torch.cuda.synchronize()
            fetched.append(eng.fetch("prob").reshape(N, cols).astype(np.float32))
            fed += [c.labels for c in infos]
        fetched = np.concatenate(fetched)
        assert fetched.shape == (6, cols) and fed[:5] == want_labels.tolist() and fed[5] == fed[4]
        path = _write_params(tmp_path, params)
        del eng
        make_store = fc.store_factory(lambda v, f: vids[NAMES.index(v)][f])
        mc = test_pass.test_one_crop(path, make_store, max_src_hw=(fc.H, fc.W), out_dir=out_dir)
        out = os.path.join(out_dir, "epic_predictions_final.pkl")
        assert mc.predictions_file == out and mc.meter.keep_rows == 5
        with open(out, "rb") as f:
            pred, lab = pickle.load(f)
        assert pred.dtype == np.float32 and lab.dtype == np.int32 and pred.shape == (5, cols) and lab.shape == (5,)
        assert pred.tobytes() == fetched[:5].tobytes() and np.array_equal(lab, want_labels)
        # the running error counts the padded clip too, as the reference's does
        h1, h5, rows = rank_rule_hits(fetched, fed, (1, 5))
        assert rows == 6 and mc.avg_err == (1.0 - h1 / 6.0) * 100 and mc.avg_err5 == (1.0 - h5 / 6.0) * 100
        os.remove(out)
        plain = test_pass.test_one_crop(path, make_store, max_src_hw=(fc.H, fc.W), out_dir=out_dir, keep_predictions=False)
        assert plain.meter.keep_rows == 0 and not os.path.exists(out)
        assert (plain.avg_err, plain.avg_err5) == (mc.avg_err, mc.avg_err5)
        with open(out, "wb") as f:
            pickle.dump((pred, lab), f, 2)
        return out


def test_epic_kept_predictions_and_action_accuracy(tmp_path):
    from vlfb import epic_eval
    import test_metrics_host as H
    vids = fc.videos(LENGTHS, seed=8)
    fc.write_epic_lists(tmp_path, NAMES, LENGTHS)
    fc.write_epic_annotations(tmp_path, _train_rows()[:20] + TEST_ROWS[:2] + _train_rows()[20:] + TEST_ROWS[2:])
    verb_file = _epic_pass(tmp_path, "verb", vids)
    noun_file = _epic_pass(tmp_path, "noun", vids)
    got = epic_eval.evaluate_actions(verb_file, noun_file, str(tmp_path))
    # the header's rank rule in numpy on the device's own softmaxed tables (hits are integers: no tolerance)
    (vp, vl), (np_, nl) = epic_eval.load_predictions(verb_file), epic_eval.load_predictions(noun_file)
    verb, noun = epic_eval.softmax_rows(vp).cpu().numpy(), epic_eval.softmax_rows(np_).cpu().numpy()
    assert verb.shape == (5, 125) and noun.shape == (5, 352) and not np.array_equal(verb, vp)
    counts = epic_eval.training_action_counts(125, 352, str(tmp_path))
    assert counts.sum() == 40 and counts[3, 17] > 0                # (the test participants' rows are not counted)
    prior = epic_eval.verb_given_noun(epic_eval.get_training_action_freq(125, 352, str(tmp_path))).astype(np.float32)
    want = {}
    for k_at, k in enumerate((1, 5)):
        want["verb_top%d" % k] = 100.0 * rank_rule_hits(verb, vl, (1, 5))[k_at] / 5
        want["noun_top%d" % k] = 100.0 * rank_rule_hits(noun, nl, (1, 5))[k_at] / 5
        want["action_top%d" % k] = 100.0 * rank_rule_hits(H.action_scores(verb, noun, prior), vl * 352 + nl, (1, 5))[k_at] / 5
    print(got, want)
    assert got == want
    with open(noun_file, "wb") as f:
        pickle.dump((np_[:4], nl[:4]), f, 2)
    with pytest.raises(AssertionError, match="5 rows, the noun file 4"):
        epic_eval.evaluate_actions(verb_file, noun_file, str(tmp_path))


def test_epic_verb_test_pass_with_an_inferred_bank(tmp_path):
    """epic_verb_r50_lfb_nl: test_one_crop infers the bank itself (lfb_pass.get_lfb over the files whose number is a multiple
    of 10: 4 + 3 clips) and samples it per clip on the loader's stream, by video NAME; the kept predictions equal the hand
    chain's, fed from the synchronous sampler of a bank inferred the same way"""
    from datasets import epic
    from vlfb import lfb_pass, test_pass
    vids = fc.videos(LENGTHS, seed=9)
    fc.write_epic_lists(tmp_path, NAMES, LENGTHS)
    fc.write_epic_annotations(tmp_path, TEST_ROWS)
    extra = fc.EXTRA + ["EPIC.VERB_LFB_CLIPS_PER_SECOND", 3, "LFB.WINDOW_SIZE", 4]
    with cases.loader_cfg("epic_verb_r50_lfb_nl", clips=N, frames=T, extra=extra) as cfg:
        fc.point_cfg_at(cfg, tmp_path)
        cfg.TEST.DATASET_SIZE = 5
        make_store = fc.store_factory(lambda v, f: vids[NAMES.index(v)][f])
        _, infer, infer_params = fc.engine("_infer_test", infer_only=True)
        del infer
        from utils import checkpoints as ck
        cfg.LFB.MODEL_PARAMS_FILE = os.path.join(str(tmp_path), "baseline.pkl")
        ck.write_blobs(cfg.LFB.MODEL_PARAMS_FILE, dict(infer_params, lr=np.array([0.1], dtype=np.float32)))
        bank = lfb_pass.get_lfb(cfg.LFB.MODEL_PARAMS_FILE, False, make_store, max_src_hw=(fc.H, fc.W))
        assert bank.video_ids == NAMES and bank.counts().tolist() == [[0, 1, 1, 1, 1], [0, 1, 1, 1, 0]]
        index = epic.EpicIndex.from_cfg("test", False, shift=cfg.TEST.CROP_SHIFT)
        m, eng, params = fc.engine(SFX, lfb=bank)
        lfb = eng.input_tensor("lfb" + SFX)
        fetched, seen_bank = [], 0.0
        for lo in range(0, 5, N):
            infos = index.get_minibatch_info(list(range(lo, min(lo + N, 5))))
            fc.feed_clips(eng, SFX, infos, lambda v: vids[NAMES.index(v)])
            eng.feed("labels" + SFX, np.array([c.labels for c in infos], dtype=np.int32))
            bank.sample_epic_verb([c.video for c in infos], [c.center for c in infos], cfg.LFB.WINDOW_SIZE,
                                  cfg.EPIC.VERB_LFB_CLIPS_PER_SECOND, out=lfb)
            seen_bank = max(seen_bank, float(lfb.float().abs().max()))
            eng.forward()
            torch.cuda.synchronize()
            fetched.append(eng.fetch("prob").reshape(N, 125).astype(np.float32))
        assert seen_bank > 0                                       # the windows held bank features
        path = _write_params(tmp_path, params)
        del eng, bank
        mc = test_pass.test_one_crop(path, make_store, max_src_hw=(fc.H, fc.W), out_dir=str(tmp_path))
        with open(mc.predictions_file, "rb") as f:
            pred, lab = pickle.load(f)
        assert pred.tobytes() == np.concatenate(fetched)[:5].tobytes() and lab.tolist() == [r[4] for r in TEST_ROWS]
