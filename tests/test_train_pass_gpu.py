"""The training driver (vlfb.train_pass) on the small data sets of tests/frame_pass_cases.py: T = 8, crop 64, 2 clips,
SOLVER.MAX_ITER 4, checkpoints and evaluations every 2 iterations.  What train() leaves -- parameters, momenta, checkpoints --
is compared bit for bit with the same chain written out by hand from the loader, source and engine calls."""
import collections
import os
import random
import threading

import numpy as np
import pytest
import torch

import clip_loader_cases as cases
import frame_pass_cases as fc

pytestmark = pytest.mark.gpu

N, T, RATE = 2, 8, 4
LENGTHS = [40, 45, 52]
LOOP = ["SOLVER.MAX_ITER", 4, "CHECKPOINT.CHECKPOINT_PERIOD", 2, "TRAIN.EVAL_PERIOD", 2, "SOLVER.STEP_SIZES", [3, 1],
        "SOLVER.LRS", [1, 0.1], "SOLVER.BASE_LR", 0.02, "SOLVER.WARMUP.WARMUP_ON", False, "TRAIN.SAMPLE_RATE", RATE,
        "TEST.SAMPLE_RATE", RATE, "NONLOCAL.CONV3_NONLOCAL", False, "TRAIN.PARAMS_FILE", "", "CHECKPOINT.RESUME", False,
        "CHECKPOINT.CONVERT_MODEL", False, "TRAIN.TEST_AFTER_TRAIN", False, "CHARADES.NUM_TEST_CLIPS_DURING_TRAINING", 3]
BN = ["MODEL.USE_AFFINE", False, "NONLOCAL.USE_BN", True, "NONLOCAL.USE_AFFINE", False, "MODEL.DILATIONS_AFTER_CONV5", False]
JSON_KEYS = ["eval_period", "batchSize", "dataset", "num_classes", "momentum", "weightDecay", "nGPU", "LR", "bn_momentum",
             "current_learning_rate", "train_loss", "train_full_map", "test_full_map", "test_best_map", "used_gpu_memory",
             "currentIter", "epoch"]


def ckpt(tmp_path, it):
    return os.path.join(str(tmp_path), "checkpoints", "c2_model_iter%d.pkl" % it)


def loader_threads():
    return [t for t in threading.enumerate() if t.name == "vlfb-clip-loader" and t.is_alive()]


def charades_cfg(tmp_path, extra=()):
    """context: the Charades baseline at the loop's sizes, three videos with frame labels under tmp_path"""
    rng = np.random.default_rng(5)
    labels = [[[int(x) for x in rng.choice(157, int(rng.integers(0, 3)), replace=False)] for _ in range(n)] for n in LENGTHS]
    ctx = cases.loader_cfg("charades_r50_baseline", clips=N, frames=T, extra=LOOP + list(extra))

    class Ctx(object):
        def __enter__(self):
            cfg = ctx.__enter__()
            fc.point_cfg_at(cfg, tmp_path)
            fc.write_charades_lists(tmp_path, LENGTHS, labels)
            cfg.LOG_PERIOD = 1
            cfg.TRAIN.DATASET_SIZE = cfg.TEST.DATASET_SIZE = len(LENGTHS)
            return cfg

        def __exit__(self, *exc):
            return ctx.__exit__(*exc)
    return Ctx()


def synthetic_init(seed=2):
    from vlfb import synth

    def init(engine):
        engine.feed_params({k: v for k, v in synth.params(engine.model, seed=seed).items() if k in engine.param_views})
    return init


def test_charades_train_equals_the_hand_chain_and_resumes(tmp_path, monkeypatch, capsys):
    from datasets import charades
    from datasets.clip_loader import FrameLoader
    from models.model_builder_video import ModelBuilder
    from utils import checkpoints as ck
    from utils import misc
    from vlfb import lfb_pass, train_pass
    from vlfb.engine import Engine
    vids = fc.videos(LENGTHS, seed=3)
    make_store = fc.store_factory(lambda v, f: vids[v][f])
    kw = dict(dtype="bf16", max_src_hw=(fc.H, fc.W), init_params=synthetic_init())
    with charades_cfg(tmp_path) as cfg:
        # ---- by hand: seed, index, engine, loader on frame_train_source, four steps ------------------------------------
        misc.generate_random_seed()
        rng = random.Random(cfg.RNG_SEED)
        m = ModelBuilder(train=True, split="train", name="train")
        m.build_model(suffix="_train")
        eng = Engine(m, "bf16", device="cuda:0", base_seed=cfg.RNG_SEED)
        shapes = {"data_train": (N, 3, T, cases.CROP, cases.CROP), "labels_train": (N, cfg.MODEL.NUM_CLASSES)}
        eng.plan(collections.OrderedDict((b, shapes[b]) for b in m.input_blob_names))
        synthetic_init()(eng)
        index = charades.CharadesIndex.from_cfg("train", False)
        assert index.get_db_size() == 3
        loader = FrameLoader(eng, "_train", 1, n_slots=2, max_src_hw=(fc.H, fc.W), device="cuda:0")
        store = make_store(loader.device, loader.stream)
        loader.start(lfb_pass.frame_train_source(index, store, rng, None, aug_rng=np.random))
        lrs, snaps = [], {}
        try:
            for it in range(4):
                m.UpdateWorkspaceLr(it)
                loader.deliver(loader.next())
                eng.train_step(float(m.current_lr))
                lrs.append(float(m.current_lr))
                if it in (1, 3):
                    snaps[it + 1] = (eng.flat_param.clone(), eng.flat_mom.clone())
        finally:
            loader.stop()
        torch.cuda.synchronize()
        assert lrs == pytest.approx([0.02, 0.02, 0.02, 0.002])
        assert not torch.equal(snaps[2][0], snaps[4][0])
        mom_name = "pred_w"
        mom2 = None
        del eng, loader, m
        assert not loader_threads()

        # ---- train() ----------------------------------------------------------------------------------------------------
        capsys.readouterr()
        out = train_pass.train(make_store, **kw)
        assert not loader_threads()
        assert "NUM_TEST_CLIPS" not in cfg.CHARADES
        tr = out["train"]
        assert torch.equal(tr.engine.flat_param, snaps[4][0]) and torch.equal(tr.engine.flat_mom, snaps[4][1])
        # checkpoints, with model_iter and lr as the reference stores them
        for it, lr in ((2, 0.02), (4, 0.002)):
            path = ckpt(tmp_path, it)
            assert os.path.exists(path)
            blobs = ck.read_blobs(path)
            assert int(blobs["model_iter"]) == it and float(blobs["lr"]) == pytest.approx(lr)
        assert out["last_checkpoint"].endswith("c2_model_iter4.pkl")
        mom2 = ck.read_blobs(ckpt(tmp_path, 2))[mom_name + "_momentum"]
        # two evaluations of get_total_test_iters iterations each: 3 videos x 3 clips at batch 2
        assert misc.get_total_test_iters(out["test"].index) == 5 and out["eval_iters"] == [5, 5]
        assert "res4_1_branch2a_w" in out["test"].engine.shared_params
        text = capsys.readouterr().out
        assert text.count("testing finished") == 2 and text.count("| Train ETA") == 4
        # the JSON stats lines
        assert [list(s) for s in out["json_stats"]] == [JSON_KEYS, JSON_KEYS]
        assert [s["currentIter"] for s in out["json_stats"]] == [2, 4]
        assert out["json_stats"][1]["current_learning_rate"] == pytest.approx(0.002)
        assert out["json_stats"][1]["test_full_map"] == out["test"].meter.full_map
        assert np.isfinite(out["json_stats"][0]["train_loss"])
        del out, tr

        # ---- resume: the latest checkpoint wins; its iteration and momentum are in place before the first step ----------
        os.remove(ckpt(tmp_path, 4))
        cfg.CHECKPOINT.RESUME = True
        seen = []
        real = Engine.train_step

        def spy(self, lr=None):
            if not seen:
                seen.append((self.iteration, self.fetch_momentum(mom_name).copy(), lr))
            return real(self, lr)
        monkeypatch.setattr(Engine, "train_step", spy)
        again = train_pass.train(make_store, dtype="bf16", max_src_hw=(fc.H, fc.W))
        assert again["start_model_iter"] == 2 and seen[0][0] == 2 and seen[0][2] == pytest.approx(0.02)
        assert np.array_equal(seen[0][1], mom2) and float(np.abs(mom2).max()) > 0
        assert again["eval_iters"] == [5] and os.path.exists(ckpt(tmp_path, 4))
        assert not loader_threads()


def test_a_step_that_raises_leaves_no_loader_thread(tmp_path, monkeypatch):
    from vlfb import train_pass
    from vlfb.engine import Engine
    vids = fc.videos(LENGTHS, seed=3)
    make_store = fc.store_factory(lambda v, f: vids[v][f])

    def boom(self, lr=None):
        raise RuntimeError("step failed")
    with charades_cfg(tmp_path) as cfg:
        monkeypatch.setattr(Engine, "train_step", boom)
        with pytest.raises(RuntimeError, match="step failed"):
            train_pass.train(make_store, dtype="bf16", max_src_hw=(fc.H, fc.W), init_params=synthetic_init())
        assert not loader_threads()
        assert "NUM_TEST_CLIPS" not in cfg.CHARADES


def test_precise_bn_goes_into_the_checkpoint(tmp_path, monkeypatch):
    """a SpatialBN graph on bf16 with TRAIN.COMPUTE_PRECISE_BN: the checkpoint holds the precise statistics, not the momentum
    average; the evaluation of the same iteration writes the same rows again without a forward"""
    from utils import checkpoints as ck
    from vlfb import precise_bn, train_pass
    vids = fc.videos(LENGTHS, seed=3)
    make_store = fc.store_factory(lambda v, f: vids[v][f])
    extra = BN + ["TRAIN.COMPUTE_PRECISE_BN", True, "TRAIN.ITER_COMPUTE_PRECISE_BN", 2, "SOLVER.MAX_ITER", 2, "SOLVER.STEP_SIZES", [1, 1]]
    layer = "res_conv1"                                       # (bn_helper.py:139-142: the blob name less "_bn_s")
    before, calls = [], []
    real = precise_bn.PreciseBN.compute_and_update_bn_stats

    def spy(self, curr_iter=None):
        before.append(self.train_engine.param_tensor(layer + "_bn_rm").clone())
        calls.append((curr_iter, self.forwards))
        return real(self, curr_iter)
    monkeypatch.setattr(precise_bn.PreciseBN, "compute_and_update_bn_stats", spy)
    with charades_cfg(tmp_path, extra):
        out = train_pass.train(make_store, dtype="bf16", max_src_hw=(fc.H, fc.W), init_params=synthetic_init())
        assert not loader_threads()
        pbn = out["bn_aux"]
        assert calls == [(1, 0), (1, 2)] and pbn.forwards == 2          # checkpoint computes, the evaluation only updates
        at = pbn.layer_names().index(layer)
        off = sum(st.C for st in pbn.steps[:at])
        want = pbn.sum_mean[off:off + pbn.steps[at].C].cpu().numpy()
        saved = ck.read_blobs(ckpt(tmp_path, 2))[layer + "_bn_rm"]
        assert saved.dtype == np.float32 and np.array_equal(saved, want)
        assert not np.array_equal(saved, before[0].cpu().numpy())        # the momentum average it replaced
        assert np.array_equal(out["train"].engine.fetch_param(layer + "_bn_rm"), want)
        riv = ck.read_blobs(ckpt(tmp_path, 2))[layer + "_bn_riv"]
        assert np.array_equal(riv, pbn.sum_mean2[off:off + pbn.steps[at].C].cpu().numpy()) and (riv > 0).all()
        assert np.isfinite(out["json_stats"][0]["test_full_map"])


def test_precise_bn_on_an_affine_graph_is_refused(tmp_path):
    from vlfb import train_pass
    vids = fc.videos(LENGTHS, seed=3)
    make_store = fc.store_factory(lambda v, f: vids[v][f])
    with charades_cfg(tmp_path, ["TRAIN.COMPUTE_PRECISE_BN", True]):
        with pytest.raises(ValueError, match="SpatialBN"):
            train_pass.train(make_store, dtype="bf16", max_src_hw=(fc.H, fc.W), init_params=synthetic_init())
        assert not loader_threads()


def test_ava_lfb_train_equals_the_hand_chain_and_scores_single_crop(tmp_path, monkeypatch):
    """ava_r50_lfb_nl on the small AVA set-up of tests/test_multicrop_pass_gpu.py (3 videos, 5 keyframes, RoI counts 1, 3, 2,
    3, 1) with a device bank: parameters and momenta against the hand chain; the in-training single-crop evaluation against
    evaluate_ava on the arrays of a pass made by hand with the trained parameters"""
    import ava_eval_ref as R
    import test_multicrop_pass_gpu as mp
    import utils.ava_eval_helper as A
    from datasets import ava
    from datasets.clip_loader import MinibatchLoader
    from models.model_builder_video import ModelBuilder
    from utils import checkpoints as ck
    from utils import misc
    from vlfb import test_pass, train_pass
    from vlfb.engine import Engine
    from vlfb.lfb_bank import DeviceBank
    monkeypatch.chdir(tmp_path)                                   # (evaluate_ava writes detections_<name>.csv where it runs)
    videos = mp._write_inputs(tmp_path)
    make_store = mp._store_maker(videos)
    extra = LOOP + ["LFB.WINDOW_SIZE", 4, "AVA.DETECTION_SCORE_THRESH_TRAIN", 0.8, "AVA.FULL_EVAL_DURING_TRAINING", True]
    with cases.loader_cfg("ava_r50_lfb_nl", clips=N, frames=T, extra=extra) as cfg:
        mp._point_cfg_at(cfg, tmp_path)
        cfg.LOG_PERIOD = 1
        cfg.TRAIN.DATASET_SIZE = cfg.TEST.DATASET_SIZE = 5
        C = cfg.MODEL.NUM_CLASSES
        bank = DeviceBank(3, 3, 4, cfg.LFB.LFB_DIM, "bf16", step_base=902)
        rng = np.random.default_rng(3)
        feats = torch.as_tensor(np.maximum(rng.standard_normal((10, cfg.LFB.LFB_DIM)), 0).astype(np.float32) * 0.5).cuda()
        bank.append(feats, [0, 0, 0, 0, 1, 1, 2, 2, 2, 2], [902, 903, 903, 903, 903, 903, 902, 902, 902, 904])

        # ---- by hand ----------------------------------------------------------------------------------------------------
        misc.generate_random_seed()
        cfg.AVA.FULL_EVAL, cfg.AVA.DETECTION_SCORE_THRESH = cfg.AVA.FULL_EVAL_DURING_TRAINING, cfg.AVA.DETECTION_SCORE_THRESH_TRAIN
        index = ava.AvaIndex.from_cfg("train", False)
        assert index.get_db_size() == 5
        rows = N * 3
        m = ModelBuilder(train=True, split="train", name="train")
        m.build_model(suffix="_train", lfb=bank)
        eng = Engine(m, "bf16", device="cuda:0", base_seed=cfg.RNG_SEED)
        k = cfg.LFB.WINDOW_SIZE * cfg.AVA.LFB_MAX_NUM_FEAT_PER_STEP
        shapes = {"data_train": (N, 3, T, cases.CROP, cases.CROP), "labels_train": (rows, C), "proposals_train": (rows, 5),
                  "lfb_train": (rows, k, cfg.LFB.LFB_DIM)}
        eng.plan(collections.OrderedDict((b, shapes[b]) for b in m.input_blob_names))
        synthetic_init()(eng)
        loader = MinibatchLoader(eng, "_train", 1, n_slots=2, max_src_hw=(mp.H, mp.W), bank=bank, device="cuda:0")
        store = make_store(loader.device, loader.stream)
        loader.start(ava.minibatch_source(index, store, np.random, bank=bank))
        try:
            for it in range(4):
                m.UpdateWorkspaceLr(it)
                loader.deliver(loader.next())
                eng.train_step(float(m.current_lr))
        finally:
            loader.stop()
        torch.cuda.synchronize()
        assert float(eng.blob_tensor("lfb_train")[0].float().abs().max()) > 0           # the head saw bank features
        want = (eng.flat_param.clone(), eng.flat_mom.clone())
        test_index = ava.AvaIndex.from_cfg("test", False)
        groundtruth = mp._groundtruth(test_index, C)
        excluded = {"V0,0902"}
        whitelist = set(range(1, C + 1)) - {2, 16, 40}
        categories = [{"id": i, "name": "action %d" % i} for i in range(1, C + 1)]
        del eng, loader, m

        # ---- train() ----------------------------------------------------------------------------------------------------
        out = train_pass.train(make_store, dtype="bf16", max_src_hw=(mp.H, mp.W), init_params=synthetic_init(), train_lfb=bank,
                               test_lfb=bank, ava_groundtruth=groundtruth, excluded_keys=excluded, class_whitelist=whitelist,
                               categories=categories)
        assert not loader_threads()
        tr, te = out["train"], out["test"]
        assert torch.equal(tr.engine.flat_param, want[0]) and torch.equal(tr.engine.flat_mom, want[1])
        assert out["eval_iters"] == [3, 3] and misc.get_total_test_iters(te.index) == 3
        assert [list(s) for s in out["json_stats"]] == [JSON_KEYS, JSON_KEYS]
        assert int(ck.read_blobs(ckpt(tmp_path, 2))["model_iter"]) == 2 and os.path.exists(ckpt(tmp_path, 4))
        full_map = te.meter.full_map
        assert out["json_stats"][1]["test_full_map"] == full_map and 0.0 < full_map <= 1.0
        assert out["json_stats"][1]["test_best_map"] == max(s["test_full_map"] for s in out["json_stats"])

        # ---- the single-crop pass by hand, on the trained parameters the test engine aliases ------------------------------
        cfg.AVA.FULL_EVAL, cfg.AVA.DETECTION_SCORE_THRESH = cfg.AVA.FULL_EVAL_DURING_TRAINING, cfg.AVA.DETECTION_SCORE_THRESH_TRAIN
        te.loader.start(ava.minibatch_source(te.index, te.store, np.random.RandomState(cfg.RNG_SEED), bank=bank))
        preds, boxes, metadata = [], [], []
        try:
            for it in range(3):
                mb = te.loader.next()
                te.loader.deliver(mb)
                te.engine.forward()
                torch.cuda.synchronize()
                preds.append(te.engine.fetch("prob").reshape(rows, C)[:mb.used].astype(np.float32))
                boxes.append(mb.original_boxes)
                metadata.append(mb.metadata[:, :2])
        finally:
            te.loader.stop()
        got = A.evaluate_ava(np.concatenate(preds), np.concatenate(boxes), np.concatenate(metadata), excluded, whitelist,
                             categories, groundtruth=groundtruth, video_idx_to_name=te.index.video_idx_to_name, name="hand")
        assert abs(got - full_map) <= R.bound(3 * rows)

        # test_net keeps refusing the single-crop AVA pass: it is reached through train_pass only
        cfg.AVA.TEST_MULTI_CROP = False
        with pytest.raises(NotImplementedError, match="single-crop"):
            test_pass.test_net(out["last_checkpoint"], make_store)


def test_the_default_mix_dtype_trains_and_evaluates_on_bf16(tmp_path):
    """dtype "mix" is a training path: the forward-only test engine of the evaluation runs on bf16 and still aliases the
    parameters (fp32 storage either way)"""
    from vlfb import train_pass
    vids = fc.videos(LENGTHS, seed=3)
    make_store = fc.store_factory(lambda v, f: vids[v][f])
    with charades_cfg(tmp_path, ["SOLVER.MAX_ITER", 2, "SOLVER.STEP_SIZES", [1, 1]]):
        out = train_pass.train(make_store, max_src_hw=(fc.H, fc.W), init_params=synthetic_init())
        assert out["train"].engine.mix and out["test"].engine.tdtype == torch.bfloat16
        assert "res4_1_branch2a_w" in out["test"].engine.shared_params
        assert out["eval_iters"] == [5] and np.isfinite(out["json_stats"][0]["train_loss"])
        assert 0.0 <= out["json_stats"][0]["test_full_map"] and os.path.exists(ckpt(tmp_path, 2))
        assert not loader_threads()
