"""train() on two ranks (vlfb.train_pass under a process group): each rank trains on its slices of ONE index walk with its own
augmentation generator, the gradients are reduced, rank 0 writes, and what train() leaves equals -- in bits, on each rank --
the same chain written out by hand from Engine.enable_data_parallel, lfb_pass.rank_source and the loader and engine calls.

Set-up as tests/test_lfb_pass_ranks_gpu.py: two spawned processes share cuda:0 over gloo, errors come back through the
queue, each process exits after destroy_process_group.  Charades at the sizes of tests/test_train_pass_gpu.py with 5 videos,
NUM_GPUS 2, TRAIN.BATCH_SIZE 4 (2 clips per rank), MAX_ITER 4, checkpoint and evaluation every 2 iterations; one AVA case
of 2 steps on the inputs of tests/test_ava_pass_gpu.py."""
import collections
import hashlib
import itertools
import os
import random
import socket

import numpy as np
import pytest
import torch

import clip_loader_cases as cases
import frame_pass_cases as fc
import test_ava_pass_gpu as avap
import test_train_pass_gpu as tp
from test_lfb_pass_ranks_gpu import _collect, _setup_paths

pytestmark = pytest.mark.gpu

WORLD, N, T = 2, tp.N, tp.T
LENGTHS = [40, 45, 52, 47, 43]
GROUP = ["NUM_GPUS", WORLD, "TRAIN.BATCH_SIZE", N * WORLD, "TEST.BATCH_SIZE", N * WORLD]
TEST_SLICES = -(-len(LENGTHS) * 3 // N)                  # 5 videos x 3 clips in slices of 2: P = 8


def charades_cfg(root):
    rng = np.random.default_rng(5)
    labels = [[[int(x) for x in rng.choice(157, int(rng.integers(0, 3)), replace=False)] for _ in range(n)] for n in LENGTHS]
    ctx = cases.loader_cfg("charades_r50_baseline", clips=N, frames=T, extra=tp.LOOP + GROUP)

    class Ctx(object):
        def __enter__(self):
            cfg = ctx.__enter__()
            fc.point_cfg_at(cfg, root)
            if not os.path.exists(os.path.join(root, "frames.csv")):
                fc.write_charades_lists(root, LENGTHS, labels)
            cfg.LOG_PERIOD = 1
            cfg.TRAIN.DATASET_SIZE = cfg.TEST.DATASET_SIZE = len(LENGTHS)
            return cfg

        def __exit__(self, *exc):
            return ctx.__exit__(*exc)
    return Ctx()


def digest(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _spy_on_loaders(seen):
    """every minibatch a loader hands out is noted as (loader, meta)"""
    from datasets.clip_loader import ClipSlots
    real = ClipSlots.next

    def spy(self):
        mb = real(self)
        seen.append((self, dict(mb.meta)))
        return mb
    ClipSlots.next = spy


def _charades(rank, root, out, seen):
    from datasets import charades
    from datasets.clip_loader import FrameLoader
    from models.model_builder_video import ModelBuilder
    from utils import checkpoints as ck
    from utils import misc
    from vlfb import lfb_pass, train_pass
    from vlfb.engine import Engine
    vids = fc.videos(LENGTHS, seed=3)
    make_store = fc.store_factory(lambda v, f: vids[v][f])
    init = tp.synthetic_init(seed=2 + rank)                                  # rank 1 starts elsewhere: rank 0's must win
    saves = []
    real_save = ck.save_model_params

    def counted_save(*a, **k):
        saves.append(k.get("params_file"))
        return real_save(*a, **k)
    ck.save_model_params = counted_save
    with charades_cfg(root) as cfg:
        assert cfg.NUM_GPUS == WORLD and cfg.TRAIN.BATCH_SIZE == N * WORLD
        # ---- by hand ------------------------------------------------------------------------------------------------------
        misc.generate_random_seed()
        m = ModelBuilder(train=True, split="train", name="train")
        m.build_model(suffix="_train")
        eng = Engine(m, "bf16", device="cuda:0", base_seed=cfg.RNG_SEED)
        shapes = {"data_train": (N, 3, T, cases.CROP, cases.CROP), "labels_train": (N, cfg.MODEL.NUM_CLASSES)}
        eng.plan(collections.OrderedDict((b, shapes[b]) for b in m.input_blob_names))
        init(eng)
        own = digest(eng.flat_param)
        eng.enable_data_parallel()
        out["start"] = (own, digest(eng.flat_param))
        index = charades.CharadesIndex.from_cfg("train", False)
        assert index.get_db_size() == len(LENGTHS)
        loader = FrameLoader(eng, "_train", 1, n_slots=2, max_src_hw=(fc.H, fc.W), device="cuda:0")
        store = make_store(loader.device, loader.stream)
        walk = lfb_pass.frame_train_source(index, store, random.Random(cfg.RNG_SEED), None,
                                           aug_rng=np.random.RandomState(cfg.RNG_SEED + 1 + rank))
        loader.start(lfb_pass.rank_source(walk, None))
        try:
            for it in range(4):
                m.UpdateWorkspaceLr(it)
                loader.deliver(loader.next())
                eng.train_step(float(m.current_lr))
        finally:
            loader.stop()
        torch.cuda.synchronize()
        want = (eng.flat_param.clone(), eng.flat_mom.clone())
        out["hand_iterations"] = [meta["iteration"] for _, meta in seen]
        out["hand_videos"] = [meta["videos"] for _, meta in seen]
        del seen[:]
        del eng, loader, m
        assert not tp.loader_threads()

        # ---- train() ------------------------------------------------------------------------------------------------------
        res = train_pass.train(make_store, dtype="bf16", max_src_hw=(fc.H, fc.W), init_params=init)
        assert not tp.loader_threads()
        tr, te = res["train"], res["test"]
        out["equals_hand"] = bool(torch.equal(tr.engine.flat_param, want[0]) and torch.equal(tr.engine.flat_mom, want[1]))
        out["moved"] = digest(want[0]) != out["start"][1]
        out["param"], out["mom"] = digest(tr.engine.flat_param), digest(tr.engine.flat_mom)
        out["train_iterations"] = [meta["iteration"] for ld, meta in seen if ld is tr.loader]
        out["train_videos"] = [meta["videos"] for ld, meta in seen if ld is tr.loader]
        out["saves"] = [os.path.basename(p) for p in saves]
        out["files"] = sorted(os.listdir(os.path.join(root, "checkpoints")))
        out["last_checkpoint"] = res["last_checkpoint"]
        blobs = ck.read_blobs(res["last_checkpoint"])
        names = [k for k in tr.engine.param_views if k in blobs]
        out["checkpoint_params"] = len(names)
        out["checkpoint_equals_final"] = all(
            np.array_equal(np.asarray(blobs[k]).reshape(-1), np.asarray(tr.engine.fetch_param(k)).reshape(-1)) for k in names)
        out["model_iter"] = int(blobs["model_iter"])
        out["json_stats"], out["eval_iters"] = res["json_stats"], res["eval_iters"]
        out["total_test_iters"] = misc.get_total_test_iters(te.index)
        again = train_pass.eval_pass(te)
        out["eval_again"] = (again, te.meter.full_map)
        assert not tp.loader_threads()
        # the refusals come before anything is built
        cfg.TRAIN.COMPUTE_PRECISE_BN = True
        try:
            train_pass.train(make_store, dtype="bf16", max_src_hw=(fc.H, fc.W), init_params=init)
            out["refused_COMPUTE_PRECISE_BN"] = False
        except NotImplementedError as e:
            out["refused_COMPUTE_PRECISE_BN"] = "PRECISE_BN" in str(e)
        cfg.TRAIN.COMPUTE_PRECISE_BN = False
    ck.save_model_params = real_save
    del seen[:]


def _ava(rank, root, out, seen):
    from datasets import ava
    from vlfb import train_pass
    extra = tp.LOOP + GROUP + ["SOLVER.MAX_ITER", 2, "SOLVER.STEP_SIZES", [1, 1], "TRAIN.EVAL_PERIOD", 100,
                               "AVA.DETECTION_SCORE_THRESH_TRAIN", 0.8, "AVA.FULL_EVAL_DURING_TRAINING", True]
    with cases.loader_cfg("ava_r50_baseline", clips=N, frames=T, extra=extra) as cfg:
        avap._point_cfg_at(cfg, root)
        cfg.LOG_PERIOD = 1
        cfg.TRAIN.DATASET_SIZE = cfg.TEST.DATASET_SIZE = 5
        videos = out.pop("_ava_videos")
        make_store = fc.store_factory(lambda v, f: videos[v][f])
        res = train_pass.train(make_store, dtype="bf16", max_src_hw=(avap.H, avap.W), init_params=tp.synthetic_init(seed=2 + rank))
        assert not tp.loader_threads()
        tr = res["train"]
        mine = [meta for ld, meta in seen if ld is tr.loader]
        out["ava_iterations"] = [meta["iteration"] for meta in mine]
        out["ava_keyframes"] = [list(zip(meta["videos"], meta["secs"])) for meta in mine]
        out["ava_param"], out["ava_mom"] = digest(tr.engine.flat_param), digest(tr.engine.flat_mom)
        out["ava_files"] = sorted(os.listdir(os.path.join(root, "checkpoints")))
        # the one walk, on the host: the generator train() seeds alike on both ranks
        cfg.AVA.FULL_EVAL, cfg.AVA.DETECTION_SCORE_THRESH = True, 0.8
        index = ava.AvaIndex.from_cfg("train", False)
        walk = ava.minibatch_source(index, None, np.random.RandomState(cfg.RNG_SEED), aug_rng=np.random.RandomState(0))
        out["ava_walk"] = [list(zip(item[3]["videos"], item[3]["secs"])) for item in itertools.islice(walk, 2 * WORLD)]


def _worker(rank, world, port, q, root, ava_videos):
    try:
        _setup_paths()
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank), VLFB_FORCE_DEVICE="0", VLFB_DIST_BACKEND="gloo")
        from vlfb import dist
        dist.init_from_env()
        out, seen = {"_ava_videos": ava_videos}, []
        _spy_on_loaders(seen)
        _charades(rank, os.path.join(root, "charades"), out, seen)
        _ava(rank, os.path.join(root, "ava"), out, seen)
        q.put((rank, out))
        dist.barrier()
        torch.distributed.destroy_process_group()
    except BaseException:
        import traceback
        q.put((rank, {"_error": traceback.format_exc()}))
        raise


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    import torch.multiprocessing as mp
    _setup_paths()
    root = str(tmp_path_factory.mktemp("train_ranks"))
    for name in ("charades", "ava"):
        os.makedirs(os.path.join(root, name))
    with charades_cfg(os.path.join(root, "charades")):
        pass                                                               # (writes the frame lists once, before the spawn)
    ava_videos = avap._write_inputs(os.path.join(root, "ava"))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, WORLD, port, q, root, ava_videos)) for r in range(WORLD)]
    for p in procs:
        p.start()
    return dict(_collect(q, procs, WORLD))


def test_train_on_two_ranks_equals_the_hand_chain_on_each_rank(ranks):
    for r in range(WORLD):
        got = ranks[r]
        assert got["equals_hand"] and got["moved"], r
        # rank 0's parameters on both ranks before the first step, although rank 1 initialised others
        assert got["start"][1] == ranks[0]["start"][0], r
        # slice s * 2 + r of the one walk at step s, in the hand chain and in train()
        assert got["hand_iterations"] == got["train_iterations"] == [s * WORLD + r for s in range(4)], r
        assert got["hand_videos"] == got["train_videos"], r
    assert ranks[1]["start"][0] != ranks[0]["start"][0]
    assert (ranks[0]["param"], ranks[0]["mom"]) == (ranks[1]["param"], ranks[1]["mom"])
    assert ranks[0]["train_videos"] != ranks[1]["train_videos"]


def test_rank_0_writes_the_checkpoints_and_every_rank_returns_the_same(ranks):
    files = ["c2_model_iter2.pkl", "c2_model_iter4.pkl"]
    assert ranks[0]["saves"] == files and ranks[1]["saves"] == []
    for r in range(WORLD):
        got = ranks[r]
        assert got["files"] == files and got["last_checkpoint"].endswith(files[1]), r
        assert got["checkpoint_equals_final"] and got["checkpoint_params"] > 50 and got["model_iter"] == 4, r
        assert got["eval_iters"] == [-(-TEST_SLICES // WORLD)] * 2 == [got["total_test_iters"]] * 2, r
        assert [list(s) for s in got["json_stats"]] == [tp.JSON_KEYS, tp.JSON_KEYS], r
        assert got["json_stats"][1]["nGPU"] == WORLD and np.isfinite(got["json_stats"][0]["train_loss"]), r
        # a further evaluation on both ranks reproduces the last one
        assert got["eval_again"] == (got["total_test_iters"], got["json_stats"][1]["test_full_map"]), r
        assert got["refused_COMPUTE_PRECISE_BN"], r
    assert ranks[0]["json_stats"] == ranks[1]["json_stats"] and ranks[0]["last_checkpoint"] == ranks[1]["last_checkpoint"]


def test_ava_ranks_train_on_the_two_halves_of_one_walk(ranks):
    """with one generator for walk and augmentation, consumed by each rank's loader thread, the ranks' walks drift apart (and
    each rank would walk every slice); here rank r trains on slices 2s + r of the walk both seed alike"""
    walk = ranks[0]["ava_walk"]
    assert walk == ranks[1]["ava_walk"] and len(walk) == 2 * WORLD
    for r in range(WORLD):
        got = ranks[r]
        assert got["ava_iterations"] == [s * WORLD + r for s in range(2)], r
        assert got["ava_keyframes"] == [walk[s * WORLD + r] for s in range(2)], r
        assert got["ava_files"] == ["c2_model_iter2.pkl"], r
    assert not set(ranks[0]["ava_iterations"]) & set(ranks[1]["ava_iterations"])
    assert ranks[0]["ava_keyframes"] != ranks[1]["ava_keyframes"]
    assert (ranks[0]["ava_param"], ranks[0]["ava_mom"]) == (ranks[1]["ava_param"], ranks[1]["ava_mom"])
