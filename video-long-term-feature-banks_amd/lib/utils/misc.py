"""Helpers the builders need from the reference's lib/utils/misc.py (batch/crop per GPU and
blob-name scoping); the Caffe2-specific debugging helpers there are out of scope."""
from core.config import config as cfg

_SCOPE_SEP = "/"


def get_batch_size(split):
    """per-GPU batch (reference: misc.py:68-72)"""
    if split in ("test", "val"):
        return int(cfg.TEST.BATCH_SIZE / cfg.NUM_GPUS)
    if split == "train":
        return int(cfg.TRAIN.BATCH_SIZE / cfg.NUM_GPUS)
    raise ValueError("unknown split %r" % (split,))


def get_crop_size(split):
    return cfg.TEST.CROP_SIZE if split in ("test", "val") else cfg.TRAIN.CROP_SIZE


def get_total_test_iters(test_model):
    """iterations of one pass over a test split, the last batch padded (reference: misc.py:279-281).  `test_model`: an
    object whose `input_db` has get_db_size(), or such an index itself (datasets.*.…Index)"""
    db = getattr(test_model, "input_db", None) or test_model
    return -(-int(db.get_db_size()) // int(cfg.TEST.BATCH_SIZE))


def generate_random_seed(node_id=0):
    """reference misc.py:275-276"""
    import numpy as np
    np.random.seed(cfg.RNG_SEED)


def get_gpu_stats():
    """the `used_gpu_memory` field of the JSON stats line (reference misc.py:150-164 parses `nvidia-smi -q`): the bytes the
    process holds on the current device, as the reference's string of MiB; 'n/a' without a device"""
    import torch
    if not torch.cuda.is_available():
        return "n/a"
    return "%d MiB" % (torch.cuda.memory_reserved() >> 20)


def log_json_stats(stats):
    """reference misc.py:82-84"""
    import json
    import logging
    line = '\njson_stats: {:s}\n'.format(json.dumps(stats, sort_keys=False))
    logging.getLogger(__name__).info(line)
    return line


def unscope_name(blob_name):
    blob_name = str(blob_name)
    return blob_name[blob_name.rfind(_SCOPE_SEP) + 1:]


def check_nan_losses(model=None, sum_ranks=False):
    """NaN guard of the training loop (reference misc.py:50-58, called every iteration from
    tools/train_net.py:160 -- one FetchBlob, i.e. one host sync, per GPU per step).

    Here the loss step keeps its last 64 values in a device ring, so the loop may call this every
    N <= 64 iterations and still see every step's loss with a single sync.  The reference logs and
    `os._exit(0)`s; a library raises instead (FloatingPointError).  Returns the losses it inspected.

    CONTRACT in a data-parallel job (a process group exists): the verdict is COLLECTIVE -- one all-reduce + one host sync --
    so every rank must call this, and at the same iterations; a call on rank 0 only, or at rank-dependent iterations,
    deadlocks where the reference's per-process check was harmless.
    sum_ranks: in such a job, return the SUM over ranks of each loss (every rank's is scaled by 1 / NUM_GPUS already: the
    reference's sum_multi_gpu_blob('loss')), the same values on every rank.  They ride on the verdict's all-reduce: no
    further collective or synchronisation."""
    import math
    if model is not None:
        engines = [model.engine]
    else:
        from vlfb import workspace
        engines = list(workspace._engines.values())
    seen = []
    bad = None
    for eng in engines:
        if eng is None:
            continue
        losses = eng.recent_losses()
        seen.extend(losses)
        if bad is None and any(math.isnan(v) for v in losses):
            bad = getattr(eng.model, "scope", "") or "gpu_0/"
    # One process per GPU: the rank whose loss went NaN first must not leave alone -- its NaN gradient reaches the others
    # only through the next all-reduce, which would then wait for a rank that is gone.  Every rank calls this at the same
    # iterations, so the verdict is taken together (one int32 all-reduce) and every rank raises.
    from vlfb import dist
    if dist.initialized() and sum_ranks:
        summed = dist.sum_floats([0.0 if bad is None else 1.0] + [0.0 if math.isnan(v) else v for v in seen],
                                 engines[0].device if engines and engines[0] is not None else None)
        if summed[0] > 0 and bad is None:
            bad = "another rank"
        seen = summed[1:]
    elif dist.initialized():
        if not dist.all_ok(bad is None) and bad is None:
            bad = "another rank"
    if bad is not None:
        raise FloatingPointError("NaN losses on %s" % bad)
    return seen
