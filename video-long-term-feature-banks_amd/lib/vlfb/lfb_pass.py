"""The bank-construction passes and the bank's files (reference: tools/lfb_loader.py:49-236).

The reference runs the baseline model in lfb_infer_only test mode over every keyframe, fetches `box_pooled` and `metadata`
to the host after every iteration, builds {video: {sec: [feat, ...]}} there and pickles it.  Here the features never visit
the host: `box_pooled` is appended to a vlfb.lfb_bank.DeviceBank by a kernel, with keys built from the minibatch's host
metadata and uploaded in stream order, and the files are written from the bank's packed rows.

    bank = get_lfb(cfg.LFB.MODEL_PARAMS_FILE, is_train=True, store=make_store)     # a DeviceBank, built, loaded or both

Charades and EPIC-Kitchens verbs (frame-level banks, construct_frame_level_lfb, :49-76): one `pool5` row per clip, under the
clip's (video, centre frame); `build_frame_bank` is the same pass on `pool5`.  EPIC nouns have no inference pass: that
bank comes from detector files and is only loaded.

The loop itself is vlfb.passes.run_pass, which the test and evaluation passes share; what a bank pass adds is the append
behind every forward (`_bank_pass`), with keys from the `meta` that the Minibatch carries over from the source.

N ranks (vlfb.dist, one process per GPU) share a pass as the reference's GPUs do (lfb_loader.py:200-223: one RunNet per
iteration feeds every gpu_k).  The single-process walk issues per-GPU slices of BATCH_SIZE // NUM_GPUS clips; iteration `it`
of it belongs to rank it % world (`rank_iterations`: slice g of global batch b on gpu_g), each rank appends what it ran to
its own bank, and DeviceBank.all_gather_ranks makes every rank's bank the merge of all of them.  That merge equals the bank
of the single-process walk bit for bit: every AVA keyframe (video, second) and every frame-level (video, centre) cell is
produced by exactly one clip, hence by one rank, so the ranks' cells are disjoint and no order between ranks is ever
visible; and a test-mode feature does not depend on its batch-mates, while the slices are the same slices.
"""
import os
import pickle

import numpy as np
import torch

from core.config import config as cfg
from datasets import ava
from vlfb import dist, hip, passes
from vlfb.lfb_bank import DeviceBank


def rank_iterations(total, rank, world):
    """the iterations of a `total`-iteration pass that rank `rank` of `world` runs: it % world == rank, in order (the
    reference's slice g of global batch b on gpu_g).  The shares are disjoint, cover range(total), differ by at most one."""
    total, rank, world = int(total), int(rank), int(world)
    assert total >= 0 and world >= 1 and 0 <= rank < world, (total, rank, world)
    return list(range(rank, total, world))


def pass_iterations(size, per_gpu):
    """iterations of the single-process walk over `size` clips in slices of `per_gpu` (the last one padded)"""
    return -(-int(size) // int(per_gpu))


def rank_source(source, total, rank=None, world=None):
    """the items of `source`, a generator of a `total`-iteration pass, at this rank's iterations (`rank_iterations`; default:
    vlfb.dist's rank and world).  A skipped item is drawn from the source and dropped: what the source draws from its rng
    per iteration is drawn as in the single-process walk, and since the clips are only (store, video, frames) references
    -- fetched and decoded by the loader that consumes what is yielded -- a skipped iteration touches no frame.
    total None: an endless source (a training walk), the same rule without an end."""
    rank = dist.rank() if rank is None else int(rank)
    world = dist.world_size() if world is None else int(world)
    assert world >= 1 and 0 <= rank < world, (rank, world)
    if total is not None:
        rank_iterations(total, rank, world)              # (its argument checks)
    for it, item in enumerate(source):
        assert total is None or it < total, "the source runs past the pass's %d iterations" % total
        if it % world == rank:
            yield item


def check_world():
    """a pass under a process group: cfg.NUM_GPUS must be its size (the per-GPU slices come from NUM_GPUS)"""
    if dist.initialized() and dist.world_size() != int(cfg.NUM_GPUS):
        raise hip.VlfbError("a pass on %d ranks but cfg.NUM_GPUS = %d (the per-GPU batch and the iterations' owners come "
                            "from NUM_GPUS)" % (dist.world_size(), int(cfg.NUM_GPUS)))


def _on_every_rank(fn):
    """fn() on this rank, then the outcome agreed by all (dist.all_ok): a rank that failed re-raises, the others raise
    too instead of waiting for it in the next collective.  fn()'s result, or its exception as is, without a group."""
    try:
        out = fn()
    except Exception:
        if not dist.initialized():
            raise
        dist.all_ok(False)
        raise
    if not dist.all_ok(True):
        raise hip.VlfbError("another rank failed its part of the pass")
    return out


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


def _bank_pass(engine, loader, index, store, bank, source, blob, rows, keys, check_finite):
    """the bank-construction pass: this rank's iterations (`rank_source`) of `source`, the single-process walk over `index`,
    through passes.run_pass, and behind every forward the first `rows` rows of `blob` appended to `bank` under keys(mb),
    the (rows, 2) int32 append keys, uploaded in stream order.  Then check_no_drops; under a process group the outcome
    agreed by all ranks and DeviceBank.all_gather_ranks, whose result is returned; with check_finite, no NaN / Inf row in
    the merged bank (a pass has no loss whose NaN guard would notice an overflowed activation)."""
    check_world()
    total = pass_iterations(index.get_db_size(), index.batch_size // cfg.NUM_GPUS)

    def run():
        feats, _ = engine.blob_tensor(blob)

        def append(it, mb):
            # pinned and device buffers of the caching allocators: reused only behind the copy / the append, no waiting
            pin = torch.from_numpy(keys(mb)).pin_memory()
            bank.append_enqueue(feats, pin.to(bank.device, non_blocking=True), rows)
        passes.run_pass(engine, loader, store, rank_source(source, total), each=append)
        bank.check_no_drops()
    _on_every_rank(run)
    merged = bank.all_gather_ranks()
    if check_finite:
        merged.check_finite()
    return merged


def build_ava_bank(engine, loader, index, store, bank, rng=None):
    """the loop of tools/lfb_loader.py:200-223 for AVA: `engine` an lfb_infer_only engine planned in test mode, `loader` its
    MinibatchLoader, `index` an lfb_infer_only datasets.ava.AvaIndex, `store` the FrameStore (on the loader's stream) whose
    `fetch` decodes, `bank` a DeviceBank whose rows are the index's video indices.  `_bank_pass` on `box_pooled` with
    `pass_keys`.

    One deviation from the reference: the clips that pad its last short batch (indices.append(indices[0])) are run and
    APPENDED again there, so that keyframe's boxes are twice in its pickle.  Here their rows get video -1 and are skipped.

    Under a process group every rank runs its `rank_iterations` of the walk and the banks are merged at the end
    (DeviceBank.all_gather_ranks): every rank returns the bank of the whole walk (module docstring)."""
    source = ava.minibatch_source(index, store, np.random if rng is None else rng)
    rows = loader.rows
    return _bank_pass(engine, loader, index, store, bank, source, "box_pooled", rows,
                      lambda mb: pass_keys(bank, mb, mb.meta, rows), False)


def frame_minibatch_source(index, store, bank_video=None):
    """generator of what FrameLoader.start takes for one pass over a Charades / EPIC index outside train: the clips
    0 .. db_size in order, in batches, the last one padded with its first clip (get_minibatch_info); clips as (store, video,
    frame_numbers); meta = dict(iteration=, videos=, centers=, padded=[bool per clip]).  bank_video: the index's video ->
    the key a sampled bank knows it by (default: the same)."""
    n = index.batch_size // cfg.NUM_GPUS
    size = index.get_db_size()
    for it, lo in enumerate(range(0, size, n)):
        batch = list(range(lo, min(lo + n, size)))
        infos = index.get_minibatch_info(batch)
        videos = [c.video if bank_video is None else bank_video(c.video) for c in infos]
        meta = dict(iteration=it, videos=videos, centers=[c.center for c in infos],
                    padded=[k >= len(batch) for k in range(len(infos))])
        yield [(store, c.video, c.seq) for c in infos], [c.labels for c in infos], meta, None, [c.shift for c in infos]


def train_index_walk(size, n, rng):
    """the endless index walk of a training loader (dataloader.py:180-221): a permutation of 0 .. size drawn with
    rng.shuffle at the start, and again whenever the next batch of n would reach or run past the end -- so the tail of a
    permutation is never used, as in the reference"""
    assert size > 0 and n > 0, "an empty training index"

    def shuffled():
        perm = list(range(size))
        rng.shuffle(perm)
        return perm
    perm, current = shuffled(), 0
    while True:
        if current + n >= size:
            perm, current = shuffled(), 0
        yield perm[current:current + n]
        current += n


def frame_train_source(index, store, rng, bank_video=None, aug_rng=None):
    """endless generator of what FrameLoader.start takes for TRAINING on a Charades / EPIC index: the batches of
    train_index_walk, get_minibatch_info(batch, rng) (which draws the clip's centre, for EPIC the annotation, from the same
    `rng`, an object with random.Random's methods), the tuple layout of frame_minibatch_source.  aug_rng: the numpy-style
    generator of the crop / flip / colour draws (default np.random, as in the reference)."""
    assert index.split == "train", "frame_train_source is the training source (other passes: frame_minibatch_source)"
    n = index.batch_size // cfg.NUM_GPUS
    aug_rng = np.random if aug_rng is None else aug_rng
    for it, batch in enumerate(train_index_walk(index.get_db_size(), n, rng)):
        infos = index.get_minibatch_info(list(batch), rng)
        videos = [c.video if bank_video is None else bank_video(c.video) for c in infos]
        meta = dict(iteration=it, videos=videos, centers=[c.center for c in infos],
                    padded=[k >= len(batch) for k in range(len(infos))])
        yield [(store, c.video, c.seq) for c in infos], [c.labels for c in infos], meta, aug_rng, 1


def frame_pass_keys(bank, kind, meta, rows):
    """the (rows, 2) int32 append keys of one iteration of a frame-level pass: row r of `pool5` is clip r of the minibatch
    and carries its (video, centre frame); the clips that only pad a short last batch get video -1 (skipped by the append).
    The reference stops at len(all_metadata) as well (lfb_loader.py:61)."""
    padded = list(meta["padded"])
    real = padded.index(True) if True in padded else len(padded)
    assert not any(not p for p in padded[real:]), "padding clips come last"
    keys = list(zip(meta["videos"], meta["centers"]))[:real]
    if kind == "charades":
        return bank.frame_keys(rows, keys, cfg.CHARADES.FPS // cfg.CHARADES.LFB_CLIPS_PER_SECOND)
    return bank.epic_frame_keys(rows, keys, cfg.EPIC.FPS // cfg.EPIC.VERB_LFB_CLIPS_PER_SECOND)


def build_frame_bank(engine, loader, index, store, bank, kind):
    """the loop of tools/lfb_loader.py:200-223 for Charades (`kind` "charades") and EPIC verbs ("epic_verb"): `engine` an
    lfb_infer_only basic-head engine planned in test mode, `loader` its FrameLoader, `index` an lfb_infer_only CharadesIndex
    / EpicIndex, `store` the FrameStore (on the loader's stream) whose `fetch` decodes, `bank` a DeviceBank of capacity 1
    whose rows are the index's video indices (Charades) or carry the video names as `video_ids` (EPIC).  `_bank_pass` on
    `pool5` with `frame_pass_keys`, and check_finite on the merged bank."""
    assert kind in ("charades", "epic_verb"), kind
    rows = loader.N
    planned = engine.blob_tensor("pool5")[0].numel()
    assert planned == rows * bank.dim, "pool5 holds %d elements, %d clips x %d planned" % (planned, rows, bank.dim)
    _bank_pass(engine, loader, index, store, bank, frame_minibatch_source(index, store), "pool5", rows,
               lambda mb: frame_pass_keys(bank, kind, mb.meta, rows), True)
    return bank


def frame_sample_freq():
    """frames between two bank clips of the configured frame-level dataset (EPIC: of the verb bank, or of the noun bank)"""
    if cfg.DATASET == "charades":
        return cfg.CHARADES.FPS // cfg.CHARADES.LFB_CLIPS_PER_SECOND
    per_second = cfg.EPIC.NOUN_LFB_FRAMES_PER_SECOND if cfg.EPIC.CLASS_TYPE == "noun" else cfg.EPIC.VERB_LFB_CLIPS_PER_SECOND
    return cfg.EPIC.FPS // per_second


def lfb_paths(directory, is_train):
    """(the reference's pickle, the native file next to it)"""
    stem = os.path.join(directory, "train_lfb" if is_train else "val_lfb")
    return stem + ".pkl", stem + ".npz"


def load_lfb(is_train, dtype="bf16", device="cuda:0", capacity=None):
    """train_lfb.pkl / val_lfb.pkl under LFB.LOAD_LFB_PATH -> DeviceBank.  The native .npz next to the pickle wins when
    present (packed rows in the bank's own type, nothing converted); the pickle is the reference's, written by Python 2 or
    3: {video: {sec: [feat, ...]}} (AVA), {video index: {frame: feat}} (Charades), {video name: {frame: feat}} (EPIC verbs)
    or {video index: {frame: (n, dim) detector features or []}} (EPIC nouns)."""
    pkl, npz = lfb_paths(cfg.LFB.LOAD_LFB_PATH, is_train)
    if os.path.exists(npz):
        return DeviceBank.load(npz, device=device)
    with open(pkl, "rb") as f:
        try:
            lfb = pickle.load(f, encoding="latin1")
        except TypeError:
            f.seek(0)
            lfb = pickle.load(f)
    if cfg.DATASET == "charades":
        return DeviceBank.from_reference(lfb, dtype=dtype, device=device, frame_level=True, sample_freq=frame_sample_freq())
    if cfg.DATASET == "epic":
        noun = cfg.EPIC.CLASS_TYPE == "noun"
        return DeviceBank.from_epic(lfb, noun=noun, sample_freq=frame_sample_freq(), capacity=capacity if noun else None,
                                    dtype=dtype, device=device)
    return DeviceBank.from_reference(lfb, capacity=capacity, dtype=dtype, device=device)


def write_lfb(bank, is_train, native=True):
    """train_lfb.pkl / val_lfb.pkl under CHECKPOINT.DIR in the reference's format (fp32 features; protocol 2, the highest
    the reference's Python 2 reads) and, next to it, the native .npz `load_lfb` prefers.  Charades and EPIC-verb banks are
    written as {video: {frame: feat}} with the reference's frame numbers.  Under a process group every rank holds the merged
    bank: rank 0 writes, and no rank returns before the files are there (a barrier, dist.all_ok: if rank 0 fails to write,
    every rank raises)."""
    pkl, npz = lfb_paths(cfg.CHECKPOINT.DIR, is_train)
    if cfg.DATASET == "epic" and cfg.EPIC.CLASS_TYPE == "noun":
        raise NotImplementedError("write_lfb: an EPIC noun bank comes from detector files, no pass infers one to write")

    def write():
        if dist.rank() != 0:
            return
        if cfg.DATASET in ("charades", "epic"):
            lfb = bank.to_reference(frame_level=True, sample_freq=frame_sample_freq(), epic=cfg.DATASET == "epic")
        else:
            lfb = bank.to_reference()
        with open(pkl, "wb") as f:
            pickle.dump(lfb, f, 2)
        if native:
            bank.save(npz)
    _on_every_rank(write)
    return pkl


def _ava_bank_plan(split, is_train, n, bank_dtype, capacity, device):
    """-> (the lfb_infer_only AvaIndex, the engine's RoI rows, the empty DeviceBank: a row per video, a step per second up to
    the last keyframe's, `capacity` slots (default: the most boxes any keyframe has))"""
    index = ava.AvaIndex.from_cfg(split, True, shift=1, get_train_lfb=is_train)
    most = passes.most_boxes(index)
    last = max(s for _, s, _ in index.keyframe_indices)
    bank = DeviceBank(index.num_videos, last - ava.AVA_VALID_FRAMES[0] + 1, capacity or most, cfg.LFB.LFB_DIM, bank_dtype,
                      device, step_base=ava.AVA_VALID_FRAMES[0])
    return index, n * most, bank


def _frame_bank_plan(split, is_train, bank_dtype, device):
    """-> (the lfb_infer_only CharadesIndex / EpicIndex, the empty DeviceBank: capacity 1, n_steps from the longest video;
    rows = video indices (Charades) or the videos in the order of the frame lists with their names as `video_ids` (EPIC
    verbs))"""
    from datasets import charades, epic
    sample_freq = frame_sample_freq()
    if cfg.DATASET == "charades":
        index = charades.CharadesIndex.from_cfg(split, True, get_train_lfb=is_train)
        n_videos, video_ids = index.num_videos, None
        n_steps = max(max(index.num_frames) // sample_freq, 1)
    else:
        index = epic.EpicIndex.from_cfg(split, True, shift=1, get_train_lfb=is_train)
        video_ids = list(index.image_paths)
        n_videos = len(video_ids)
        n_steps = max([a[2] for a in index.annotations] + [0]) // sample_freq + 1
    return index, DeviceBank(n_videos, n_steps, 1, cfg.LFB.LFB_DIM, bank_dtype, device, video_ids=video_ids)


def _check_complete(bank, index, is_train):
    """the reference's completeness conditions of a frame-level bank (construct_lfb, lfb_loader.py:140-152)"""
    occupied = bank.counts() > 0
    with_clips = int(occupied.any(axis=1).sum())
    if cfg.DATASET == "charades":
        want = cfg.TRAIN.DATASET_SIZE if is_train else cfg.TEST.DATASET_SIZE
        assert with_clips == want, "the bank holds %d videos, the split has %d" % (with_clips, want)
    assert with_clips == bank.n_videos, "%d of %d videos have no bank clip" % (bank.n_videos - with_clips, bank.n_videos)
    assert int(occupied.sum()) == index.get_db_size(), \
        "%d bank cells are occupied, the pass walked %d clips" % (int(occupied.sum()), index.get_db_size())


def get_lfb(params_file, is_train, store, dtype="bf16", bank_dtype="bf16", capacity=None, device="cuda:0", n_slots=2,
            max_src_hw=(256, 340), rng=None):
    """lfb_loader.get_lfb: the bank loaded from LFB.LOAD_LFB_PATH when LFB.LOAD_LFB, else inferred with the baseline
    parameters `params_file` and written when LFB.WRITE_LFB.  `store(device, stream)` builds the
    datasets.frame_store.FrameStore (with its `fetch`) on the loader's stream; `max_src_hw` bounds its frames.
    AVA: the lfb_infer_only engine over every keyframe of the train (is_train) or test LFB box lists (build_ava_bank);
    `capacity`: slots per second, default the most boxes any keyframe has.
    Charades and EPIC verbs: the lfb_infer_only basic-head engine (planned without `proposals`) over every bank clip of the
    train or test frame lists (build_frame_bank), checked for the reference's completeness conditions.  EPIC nouns have no
    inference pass: that bank can only be loaded."""
    from utils import checkpoints
    if cfg.LFB.LOAD_LFB:
        return load_lfb(is_train, bank_dtype, device, capacity)
    if cfg.DATASET == "epic" and cfg.EPIC.CLASS_TYPE == "noun":
        raise NotImplementedError("get_lfb: the EPIC noun bank holds detector features (the reference has no inference pass "
                                  "for it either); set LFB.LOAD_LFB and LFB.LOAD_LFB_PATH to the detector-built files")
    assert params_file, "LFB.MODEL_PARAMS_FILE is not specified."
    frame_level = cfg.DATASET in ("charades", "epic")
    split = cfg.TEST.DATA_TYPE or "test"
    n = cfg.TEST.BATCH_SIZE // cfg.NUM_GPUS
    if frame_level:
        rows = None
        index, bank = _frame_bank_plan(split, is_train, bank_dtype, device)
    else:
        index, rows, bank = _ava_bank_plan(split, is_train, n, bank_dtype, capacity, device)
    p = passes.build(store, "_infer_%s" % ("train" if is_train else "test"), dtype, n, cfg.TEST.VIDEO_LENGTH,
                     cfg.TEST.CROP_SIZE, rows, split=split, name="lfb_infer", lfb_infer_only=True, shift=1, device=device,
                     n_slots=n_slots, max_src_hw=max_src_hw)
    p.engine.init_params()
    checkpoints.load_model_from_params_file_for_test(p.model, params_file)
    if frame_level:
        build_frame_bank(p.engine, p.loader, index, p.store, bank, "charades" if cfg.DATASET == "charades" else "epic_verb")
        _check_complete(bank, index, is_train)
    else:
        build_ava_bank(p.engine, p.loader, index, p.store, bank, rng)
    if cfg.LFB.WRITE_LFB:
        write_lfb(bank, is_train)
    return bank


def get_frame_lfb(params_file, is_train, store, dtype="bf16", bank_dtype="bf16", capacity=None, device="cuda:0", n_slots=2,
                  max_src_hw=(256, 340)):
    """get_lfb for cfg.DATASET 'charades' / 'epic', under the name it had as a function of its own"""
    assert cfg.DATASET in ("charades", "epic"), cfg.DATASET
    return get_lfb(params_file, is_train, store, dtype, bank_dtype, capacity, device, n_slots, max_src_hw)
