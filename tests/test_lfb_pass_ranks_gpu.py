"""The bank-construction pass shared by two ranks (vlfb.lfb_pass: rank_iterations, DeviceBank.all_gather_ranks): each rank
runs only its iterations of the single-process walk, and both end with the bank of the single-process pass, bit for bit.

Set-up as tests/test_dp_gpu.py: two spawned processes share cuda:0 over gloo, errors come back through the queue, and each
process exits after destroy_process_group.  Data: the small Charades lists of tests/frame_pass_cases.py and the small AVA
inputs of tests/test_ava_pass_gpu.py, with lengths that give an odd number of iterations (3, the last one padded), so the
ranks get unequal shares; and a Charades split of one iteration, so that rank 1 runs none.  The workers run every case in
one spawn (process start-up is most of the cost), the parent runs the single-process passes on the same files."""
import contextlib
import os
import pickle
import socket
import sys

import numpy as np
import pytest
import torch

import clip_loader_cases as cases
import frame_pass_cases as fc
import test_ava_pass_gpu as avap

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD = 2
N = fc.N
assert N == avap.N
# name -> (dataset, Charades frames per video, LFB.WRITE_LFB in the workers)
CASES = {
    "charades": ("charades", [48, 23], True),      # 4 + 1 bank clips: 3 iterations, the last padded
    "tiny": ("charades", [23, 23], False),         # 1 + 1: one iteration, none for rank 1
    "ava": ("ava", None, True),                    # 5 keyframes: 3 iterations, the last padded
}
CLIPS = {"charades": 5, "tiny": 2, "ava": 5}       # clips of the walk: bank cells of a Charades bank, keyframes of AVA
# the synthetic banks of the shared-cell merge (3 videos x 5 steps, capacity 4): the ranks share cells (0,0) (0,4) (1,1)
# (1,3) (2,4), two of them filled to the capacity
SYN = {0: [[1, 0, 2, 0, 1], [0, 2, 0, 1, 0], [1, 0, 0, 0, 3]],
       1: [[2, 1, 0, 0, 1], [0, 1, 0, 3, 0], [0, 2, 0, 1, 1]]}


def _setup_paths():
    for p in (os.path.join(ROOT, "video-long-term-feature-banks_amd", "lib"), ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)


@contextlib.contextmanager
def _cfg(name, root, num_gpus=WORLD):
    """the product cfg of case `name`, pointed at its directory under `root`: TEST.BATCH_SIZE = N clips per GPU"""
    kind = CASES[name][0]
    preset = "charades_r50_baseline" if kind == "charades" else "ava_r50_baseline"
    frames = fc.T if kind == "charades" else avap.T
    extra = (fc.EXTRA if kind == "charades" else []) + ["NUM_GPUS", num_gpus, "TEST.BATCH_SIZE", N * num_gpus]
    with cases.loader_cfg(preset, clips=N, frames=frames, extra=extra) as cfg:
        d = os.path.join(root, name)
        if kind == "charades":
            fc.point_cfg_at(cfg, d)
            cfg.TRAIN.DATASET_SIZE = cfg.TEST.DATASET_SIZE = len(CASES[name][1])
        else:
            avap._point_cfg_at(cfg, d)
        cfg.CHECKPOINT.DIR = os.path.join(d, "out")
        yield cfg


def _make_store(name, ava_videos):
    if CASES[name][0] == "charades":
        vids = fc.videos(CASES[name][1], seed=5)
        return fc.store_factory(lambda v, f: vids[v][f])
    return fc.store_factory(lambda v, f: ava_videos[v][f])


def _params_file(root, name):
    return os.path.join(root, name, "baseline.pkl")


def _run_pass(name, root, ava_videos):
    """get_lfb (the train bank) of case `name` from its parameter file; cfg already loaded"""
    from vlfb import lfb_pass
    return lfb_pass.get_lfb(_params_file(root, name), True, _make_store(name, ava_videos), max_src_hw=(fc.H, fc.W))


def _state(bank):
    """count and the bits of the occupied slots, cell order then slot order"""
    cnt = bank.counts()
    mask = (np.arange(bank.capacity)[None, :] < np.minimum(cnt.reshape(-1), bank.capacity)[:, None]).reshape(-1)
    return dict(count=cnt, rows=fc.bits(bank.bank).reshape(-1, bank.dim)[mask])


def _same_state(a, b):
    return np.array_equal(a["count"], b["count"]) and np.array_equal(a["rows"], b["rows"])


def _synthetic_bank(rank):
    from vlfb.lfb_bank import DeviceBank
    bank = DeviceBank(3, 5, 4, 20, "bf16", step_base=902)
    cnt = np.asarray(SYN[rank]).reshape(-1)
    cells = np.repeat(np.arange(cnt.size), cnt)
    rng = np.random.default_rng(60 + rank)
    rng.shuffle(cells)
    bank.append(rng.standard_normal((cells.size, 20)).astype(np.float32), cells // 5, cells % 5 + 902)
    bank.check_no_drops()
    return bank


def _collect(q, procs, n, timeout=600):
    out = []
    for _ in range(n):
        item = q.get(timeout=timeout)
        if isinstance(item, tuple) and isinstance(item[1], dict) and "_error" in item[1]:
            for p in procs:
                p.kill()
            pytest.fail("worker failed:\n" + item[1]["_error"])
        out.append(item)
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    return out


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
    from vlfb import dist, hip, lfb_pass
    from vlfb.engine import Engine
    from vlfb.lfb_bank import DeviceBank
    dist.init_from_env()
    calls = [0]
    forward = Engine.forward

    def counted(self):
        calls[0] += 1
        return forward(self)
    Engine.forward = counted
    out = {}
    with _cfg("charades", root, num_gpus=1):
        try:
            lfb_pass.check_world()
            out["refused"] = False
        except hip.VlfbError:
            out["refused"] = True
    for name in CASES:
        with _cfg(name, root) as cfg:
            cfg.LFB.WRITE_LFB = CASES[name][2]
            calls[0] = 0
            bank = _run_pass(name, root, ava_videos)
            out[name] = dict(_state(bank), forwards=calls[0])
            del bank
    syn = _synthetic_bank(rank)
    syn.all_gather_ranks(chunk_rows=3)                  # several rounds, chunks that begin and end inside cells
    out["synthetic"] = _state(syn)
    odd = DeviceBank(3, 5, 4, 8, "bf16", step_base=902 + rank)
    try:
        odd.all_gather_ranks()
        out["mismatch_raised"] = False
    except hip.VlfbError:
        out["mismatch_raised"] = True
    q.put((rank, out))
    dist.barrier()
    torch.distributed.destroy_process_group()


def _same_tree(a, b):
    """the reference's dictionaries: equal keys everywhere, fp32 features equal in bits"""
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(_same_tree(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(_same_tree(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    import torch.multiprocessing as mp
    from utils import checkpoints as ck
    from vlfb import lfb_pass
    from vlfb.lfb_bank import DeviceBank
    _setup_paths()
    root = str(tmp_path_factory.mktemp("ranks"))
    ava_videos = None
    for name, (kind, lengths, _) in CASES.items():
        d = os.path.join(root, name)
        os.makedirs(os.path.join(d, "out"))
        with _cfg(name, root):
            if kind == "charades":
                fc.write_charades_lists(d, lengths)
                _, eng, params = fc.engine("_infer_test", infer_only=True)
            else:
                ava_videos = avap._write_inputs(d)
                _, eng, params = avap._infer_engine(N * 3)
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
    for name, (kind, _, write) in CASES.items():
        with _cfg(name, root) as cfg:
            bank = _run_pass(name, root, ava_videos)
            res = dict(_state(bank), total=lfb_pass.pass_iterations(CLIPS[name], N))
            if write:
                out = cfg.CHECKPOINT.DIR
                res["files"] = sorted(os.listdir(out))
                res["npz"] = _state(DeviceBank.load(os.path.join(out, "train_lfb.npz")))
                with open(os.path.join(out, "train_lfb.pkl"), "rb") as f:
                    written = pickle.load(f)
                ref = (bank.to_reference(frame_level=True, sample_freq=lfb_pass.frame_sample_freq()) if kind == "charades"
                       else bank.to_reference())
                res["pkl_same"] = _same_tree(written, ref)
            single[name] = res
            del bank
    syn = _synthetic_bank(0)
    syn.merge_from(_synthetic_bank(1))
    single["synthetic"] = _state(syn)
    return ranks, single


def _check_case(runs, name, want_total):
    from vlfb.lfb_pass import rank_iterations
    ranks, single = runs
    want = single[name]
    assert want["total"] == want_total
    assert int((want["count"] > 0).sum()) == CLIPS[name]
    for rank in range(WORLD):
        got = ranks[rank][name]
        print("%s rank %d: %d forwards, %d bank rows" % (name, rank, got["forwards"], int(got["count"].sum())))
        assert np.array_equal(got["count"], want["count"]), (name, rank)
        assert np.array_equal(got["rows"], want["rows"]), (name, rank)
        assert got["forwards"] == len(rank_iterations(want_total, rank, WORLD)), (name, rank)


@pytest.mark.parametrize("name", ["charades", "ava"])
def test_two_ranks_build_the_single_process_bank_and_write_it_once(runs, name):
    _check_case(runs, name, 3)
    ranks, single = runs
    assert [ranks[r][name]["forwards"] for r in range(WORLD)] == [2, 1]           # unequal shares
    want = single[name]
    assert want["files"] == ["train_lfb.npz", "train_lfb.pkl"]
    assert _same_state(want["npz"], want) and want["pkl_same"]


def test_a_split_of_one_iteration_leaves_rank_1_without_work(runs):
    _check_case(runs, "tiny", 1)
    ranks, _ = runs
    assert ranks[1]["tiny"]["forwards"] == 0 and ranks[0]["tiny"]["forwards"] == 1


def test_ranks_that_share_cells_merge_in_rank_order(runs):
    """all_gather_ranks equals rank 0's bank after merge_from(rank 1's) on both ranks, in 3-row rounds"""
    ranks, single = runs
    for rank in range(WORLD):
        assert _same_state(ranks[rank]["synthetic"], single["synthetic"]), rank


def test_every_rank_refuses_unequal_geometry_and_a_world_that_is_not_num_gpus(runs):
    ranks, _ = runs
    assert all(ranks[r]["mismatch_raised"] for r in range(WORLD))
    assert all(ranks[r]["refused"] for r in range(WORLD))
