"""Process-group helpers: one process per GPU, `torch.distributed` (backend "nccl" = RCCL over
xGMI on ROCm; "gloo" in the CPU tests).  Replaces the reference's single-process
data_parallel_model.Parallelize_GPU(use_nccl=...) (lib/models/model_builder_video.py:142-157)."""
import os

import torch
import torch.distributed as td


def initialized():
    return td.is_available() and td.is_initialized()


def world_size():
    return td.get_world_size() if initialized() else 1


def rank():
    return td.get_rank() if initialized() else 0


def local_rank():
    """index of this process's GPU.  VLFB_FORCE_DEVICE pins every rank to one device (used by the
    single-GPU multi-process test, which then has to run over gloo)."""
    if "VLFB_FORCE_DEVICE" in os.environ:
        return int(os.environ["VLFB_FORCE_DEVICE"])
    return int(os.environ.get("LOCAL_RANK", "0"))


def forced():
    return os.environ.get("VLFB_DIST_FORCE", "0") == "1"


def init_from_env(backend=None):
    """Join the job described by RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT (torchrun).
    A one-rank job skips the process group unless VLFB_DIST_FORCE=1 (lets a single-GPU box drive the
    RCCL code path: communicator set-up, bucketed all-reduce, stream hand-over)."""
    if initialized():
        return
    if int(os.environ.get("WORLD_SIZE", "1")) <= 1 and not forced():
        return
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    os.environ.setdefault("MASTER_PORT", "29533")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if backend is None:
        backend = os.environ.get("VLFB_DIST_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")
    if backend == "nccl":
        torch.cuda.set_device(local_rank())
    td.init_process_group(backend=backend)


def barrier():
    if initialized():
        td.barrier()


def all_ok(flag):
    """logical AND of `flag` over all ranks (a barrier that also carries a success bit); plain `flag` without a group"""
    if not initialized():
        return bool(flag)
    dev = "cuda:%d" % local_rank() if td.get_backend() == "nccl" else "cpu"
    t = torch.tensor([1 if flag else 0], device=dev, dtype=torch.int32)
    td.all_reduce(t, op=td.ReduceOp.MIN)
    return bool(int(t.item()))


def sum_ints(values, device=None):
    """element-wise sum of a list of Python ints over all ranks (the meter's hit / row counters); the list itself
    without a group"""
    values = [int(v) for v in values]
    if not initialized():
        return values
    dev = device if td.get_backend() == "nccl" else "cpu"
    t = torch.tensor(values, device=dev, dtype=torch.int64)
    td.all_reduce(t, op=td.ReduceOp.SUM)
    return [int(v) for v in t.cpu().tolist()]


def sum_floats(values, device=None):
    """element-wise fp64 sum of a list of floats over all ranks, the same bits on every rank (the list must be equally long
    everywhere); the list itself without a group"""
    values = [float(v) for v in values]
    if not initialized():
        return values
    dev = device if td.get_backend() == "nccl" else "cpu"
    t = torch.tensor(values, device=dev, dtype=torch.float64)
    td.all_reduce(t, op=td.ReduceOp.SUM)
    return [float(v) for v in t.cpu().tolist()]


def gather_rows(t):
    """rows of every rank's 2-D tensor (the same number on each), concatenated in rank order; `t` without a group"""
    if not initialized():
        return t
    src = t.contiguous() if td.get_backend() == "nccl" else t.cpu().contiguous()
    parts = [torch.empty_like(src) for _ in range(world_size())]
    td.all_gather(parts, src)
    return torch.cat(parts).to(t.device)


def gather_ragged(t, rows):
    """the first rows[k] rows of rank k's 2-D tensor, for every rank, as a list in rank order on t.device.  Every rank passes
    the same `rows` and a `t` of at least max(rows) rows: max(rows) of them travel from each rank (behind its own rows[rank]
    they are padding, dropped on arrival).  Bytes travel, so the result is bit-exact whatever the element type; on backend
    nccl they stay on the device, on gloo they go through the host as in `gather_rows`.  [t[:rows[0]]] without a group."""
    rows = [int(r) for r in rows]
    if not initialized():
        return [t[:rows[0]]]
    assert len(rows) == world_size() and t.dim() == 2 and t.shape[0] >= max(rows), "gather_ragged: rows / tensor mismatch"
    src = t[:max(rows)].contiguous().view(torch.uint8)
    src = src if td.get_backend() == "nccl" else src.cpu()
    parts = [torch.empty_like(src) for _ in range(world_size())]
    td.all_gather(parts, src)
    return [p[:r].to(t.device).view(t.dtype) for p, r in zip(parts, rows)]


def gather_objects(obj):
    """every rank's picklable `obj` as a list in rank order (small host-side records: row counts, image keys, boxes);
    [obj] without a group"""
    if not initialized():
        return [obj]
    out = [None] * world_size()
    td.all_gather_object(out, obj)
    return out


def broadcast_object(obj, src=0):
    """rank `src`'s picklable `obj` on every rank; `obj` itself without a group"""
    if not initialized():
        return obj
    box = [obj]
    td.broadcast_object_list(box, src=src)
    return box[0]
