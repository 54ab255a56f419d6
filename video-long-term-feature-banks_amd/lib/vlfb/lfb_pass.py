"""The bank-construction pass for AVA and the bank's files (reference: tools/lfb_loader.py:115-236).

The reference runs the baseline model in lfb_infer_only test mode over every keyframe, fetches `box_pooled` and `metadata`
to the host after every iteration, builds {video: {sec: [feat, ...]}} there and pickles it.  Here the features never visit
the host: `box_pooled` is appended to a vlfb.lfb_bank.DeviceBank by a kernel, with keys built from the minibatch's host
metadata and uploaded in stream order, and the files are written from the bank's packed rows.

    bank = get_lfb(cfg.LFB.MODEL_PARAMS_FILE, is_train=True, store=make_store)     # a DeviceBank, built, loaded or both
"""
import collections
import os
import pickle

import numpy as np
import torch

from core.config import config as cfg
from datasets import ava
from vlfb.lfb_bank import DeviceBank


def pass_keys(bank, minibatch, meta, rows):
    """the (rows, 2) int32 append keys of one iteration: row r of `box_pooled` belongs to the clip in column 0 of the
    minibatch's proposals, and carries that clip's video and second; the rows of a clip that only pads a short batch, and the
    rows behind the last box, get video -1 (skipped by the append)"""
    videos = np.full(int(rows), -1, dtype=np.int64)
    secs = np.full(int(rows), bank.step_base, dtype=np.int64)
    used = int(minibatch.used)
    clip_of = minibatch.proposals[:used, 0].astype(np.int64)
    v = np.asarray(meta["videos"], dtype=np.int64)[clip_of]
    v[np.asarray(meta["padded"], dtype=bool)[clip_of]] = -1
    videos[:used] = v
    secs[:used] = np.asarray(meta["secs"], dtype=np.int64)[clip_of]
    return bank.append_keys(videos, secs)


def build_ava_bank(engine, loader, index, store, bank, rng=None):
    """the loop of tools/lfb_loader.py:200-223 for AVA: `engine` an lfb_infer_only engine planned in test mode, `loader` its
    MinibatchLoader, `index` an lfb_infer_only datasets.ava.AvaIndex, `store` the FrameStore (on the loader's stream) whose
    `fetch` decodes, `bank` a DeviceBank whose rows are the index's video indices.  Per batch: next / deliver / forward /
    append_enqueue(box_pooled); nothing in the loop waits for the device, one synchronisation, check_no_drops and the store's
    check_decoded at the end.

    One deviation from the reference: the clips that pad its last short batch (indices.append(indices[0])) are run and
    APPENDED again there, so that keyframe's boxes are twice in its pickle.  Here their rows get video -1 and are skipped."""
    rng = np.random if rng is None else rng
    metas = collections.deque()                       # the source runs in the loader's thread, one minibatch ahead

    def source():
        for args in ava.minibatch_source(index, store, rng):
            metas.append(args[3])
            yield args

    feats, _ = engine.blob_tensor("box_pooled")
    rows = loader.rows
    loader.start(source())
    try:
        while True:
            try:
                mb = loader.next()
            except StopIteration:
                break
            loader.deliver(mb)
            engine.forward()
            # pinned and device buffers of the caching allocators: reused only behind the copy / the append, no waiting
            pin = torch.from_numpy(pass_keys(bank, mb, metas.popleft(), rows)).pin_memory()
            bank.append_enqueue(feats, pin.to(bank.device, non_blocking=True), rows)
    finally:
        loader.stop()
    torch.cuda.current_stream().synchronize()
    bank.check_no_drops()
    store.check_decoded()                             # frames the store decoded from JPEG bytes: none was damaged
    return bank


def lfb_paths(directory, is_train):
    """(the reference's pickle, the native file next to it)"""
    stem = os.path.join(directory, "train_lfb" if is_train else "val_lfb")
    return stem + ".pkl", stem + ".npz"


def load_lfb(is_train, dtype="bf16", device="cuda:0", capacity=None):
    """train_lfb.pkl / val_lfb.pkl under LFB.LOAD_LFB_PATH -> DeviceBank.  The native .npz next to the pickle wins when
    present (packed rows in the bank's own type, nothing converted); the pickle is the reference's {video: {sec: [feat,
    ...]}}, written by Python 2 or 3."""
    pkl, npz = lfb_paths(cfg.LFB.LOAD_LFB_PATH, is_train)
    if os.path.exists(npz):
        return DeviceBank.load(npz, device=device)
    with open(pkl, "rb") as f:
        try:
            lfb = pickle.load(f, encoding="latin1")
        except TypeError:
            f.seek(0)
            lfb = pickle.load(f)
    return DeviceBank.from_reference(lfb, capacity=capacity, dtype=dtype, device=device)


def write_lfb(bank, is_train, native=True):
    """train_lfb.pkl / val_lfb.pkl under CHECKPOINT.DIR in the reference's format (fp32 features; protocol 2, the highest
    the reference's Python 2 reads) and, next to it, the native .npz `load_lfb` prefers"""
    pkl, npz = lfb_paths(cfg.CHECKPOINT.DIR, is_train)
    with open(pkl, "wb") as f:
        pickle.dump(bank.to_reference(), f, 2)
    if native:
        bank.save(npz)
    return pkl


def get_lfb(params_file, is_train, store, dtype="bf16", bank_dtype="bf16", capacity=None, device="cuda:0", n_slots=2,
            max_src_hw=(256, 340), rng=None):
    """lfb_loader.get_lfb: the bank loaded from LFB.LOAD_LFB_PATH when LFB.LOAD_LFB, else inferred with the baseline
    parameters `params_file` over every keyframe of the train (is_train) or test LFB box lists, and written when
    LFB.WRITE_LFB.  `store(device, stream)` builds the datasets.frame_store.FrameStore (with its `fetch`) on the loader's
    stream; `max_src_hw` bounds its frames.  `capacity`: slots per second, default the most boxes any keyframe has."""
    from datasets.clip_loader import MinibatchLoader
    from models.model_builder_video import ModelBuilder
    from utils import checkpoints
    from vlfb.engine import Engine
    if cfg.LFB.LOAD_LFB:
        return load_lfb(is_train, bank_dtype, device, capacity)
    assert params_file, "LFB.MODEL_PARAMS_FILE is not specified."
    split = cfg.TEST.DATA_TYPE or "test"
    index = ava.AvaIndex.from_cfg(split, True, shift=1, get_train_lfb=is_train)
    most = max(len(index.boxes_and_labels[v][s]) for v, s, _ in index.keyframe_indices)
    suffix = "_infer_%s" % ("train" if is_train else "test")
    model = ModelBuilder(train=False, split=split, name="lfb_infer")
    model.build_model(suffix=suffix, lfb_infer_only=True, shift=1)
    engine = Engine(model, dtype, device=device, base_seed=cfg.RNG_SEED)
    n = cfg.TEST.BATCH_SIZE // cfg.NUM_GPUS
    shapes = {"data" + suffix: (n, 3, cfg.TEST.VIDEO_LENGTH, cfg.TEST.CROP_SIZE, cfg.TEST.CROP_SIZE),
              "labels" + suffix: (n * most, cfg.MODEL.NUM_CLASSES), "proposals" + suffix: (n * most, 5)}
    engine.plan(collections.OrderedDict((name, shapes[name]) for name in model.input_blob_names))
    engine.init_params()
    checkpoints.load_model_from_params_file_for_test(model, params_file)
    loader = MinibatchLoader(engine, suffix, 0, n_slots=n_slots, max_src_hw=max_src_hw, device=device)
    frames = store(loader.device, loader.stream)
    last = max(s for _, s, _ in index.keyframe_indices)
    bank = DeviceBank(index.num_videos, last - ava.AVA_VALID_FRAMES[0] + 1, capacity or most, cfg.LFB.LFB_DIM, bank_dtype,
                      device, step_base=ava.AVA_VALID_FRAMES[0])
    build_ava_bank(engine, loader, index, frames, bank, rng)
    if cfg.LFB.WRITE_LFB:
        write_lfb(bank, is_train)
    return bank
