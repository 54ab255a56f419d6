"""What the drivers of a pass over a dataset share: the planned engine with its loader and frame store (`build`, with the
one table of input shapes and the one choice of loader), and the loop that walks a source through them (`run_pass`).

    p = build(make_store, "_final_test", "bf16", n, frames, crop, split=split, name="test", bank=lfb)
    p.engine.init_params()                               # or load: the driver's own order
    ran = run_pass(p.engine, p.loader, p.store, source, iterations=total, timer=timer, each=lambda it, mb: ...)

The bank passes (vlfb.lfb_pass), the test pass (vlfb.test_pass) and the in-training evaluation (vlfb.train_pass.eval_pass)
are this loop with their own `each`; the training loop steps instead of forwarding and the AVA multi-crop pass has no
loader, so those two are not.

Under a process group the counted passes -- the test pass and the evaluation -- become `run_pass_ranks`: the same walk, of which a rank forwards its
slices (vlfb.lfb_pass.rank_source), with `each` called by every rank at every GLOBAL iteration so that a collective in
it is reached by all of them the same number of times.
"""
import collections
import time

from core.config import config as cfg


class Timer(object):
    """tic / toc around one iteration.  The loop never waits for the device, so `diff` is the time it took to ENQUEUE the
    iteration; the device's pace shows in the average, once the loader's slots throttle the loop."""

    def __init__(self):
        self.total_time, self.calls, self.start_time, self.diff, self.average_time = 0.0, 0, 0.0, 0.0, 0.0

    def tic(self):
        self.start_time = time.time()

    def toc(self):
        self.diff = time.time() - self.start_time
        self.total_time += self.diff
        self.calls += 1
        self.average_time = self.total_time / self.calls
        return self.diff


def most_boxes(index):
    """the most boxes any keyframe of an AvaIndex has: per clip, the RoI rows an engine over that index is planned with"""
    return max(len(index.boxes_and_labels[v][s]) for v, s, _ in index.keyframe_indices)


def bank_kind():
    """which window a FrameLoader samples from the bank of the configured frame-level dataset (clip_loader.BANK_KINDS)"""
    if cfg.DATASET == 'charades':
        return "charades"
    return "epic_noun" if cfg.EPIC.CLASS_TYPE == 'noun' else "epic_verb"


def bank_video(index):
    """the index's video -> the key the bank knows it by, None for "the same": the EPIC noun bank is keyed by video index,
    the verb bank (and the index) by name"""
    if cfg.DATASET == 'epic' and bank_kind() == "epic_noun":
        return index.video_name_to_idx.__getitem__
    return None


def input_shapes(model, suffix, n, frames, crop, rows=None, lfb_shape=None):
    """the shapes an engine over `model` is planned with, an OrderedDict in model.input_blob_names order, for `n` clips of
    `frames` frames cropped to `crop`.  With `rows` (AVA: RoI rows, clips x most_boxes) labels, proposals and lfb are per
    row; without (Charades / EPIC) labels and lfb are per clip and there are no proposals.  These are what the loaders
    assert of the blobs (datasets.clip_loader).  lfb_shape: instead of the configured bank window's."""
    first = n if rows is None else rows
    per_row = cfg.LFB.WINDOW_SIZE * (1 if rows is None else cfg.AVA.LFB_MAX_NUM_FEAT_PER_STEP)
    table = {"data": (n, 3, frames, crop, crop),
             "labels": (first, cfg.MODEL.NUM_CLASSES) if rows is not None or cfg.MODEL.MULTI_LABEL else (n,),
             "lfb": tuple(lfb_shape) if lfb_shape is not None else (first, per_row, cfg.LFB.LFB_DIM)}
    if rows is not None:
        table["proposals"] = (rows, 5)
    shapes = collections.OrderedDict()
    for name in model.input_blob_names:
        assert name.endswith(suffix), (name, suffix)
        shapes[name] = table[name[:len(name) - len(suffix)]]
    return shapes


def make_loader(engine, suffix, aug, bank, n_slots, max_src_hw, device):
    """the loader (not started) of a planned engine: MinibatchLoader for AVA, FrameLoader for Charades / EPIC, which samples
    `bank` (None: the engine has no `lfb` input) as `bank_kind()` says.  aug: 1 for the training augmentation."""
    from datasets.clip_loader import FrameLoader, MinibatchLoader
    if cfg.DATASET == 'ava':
        return MinibatchLoader(engine, suffix, aug, n_slots=n_slots, max_src_hw=max_src_hw, bank=bank, device=device)
    return FrameLoader(engine, suffix, aug, n_slots=n_slots, max_src_hw=max_src_hw, bank=bank,
                       bank_kind=bank_kind() if bank is not None else None, device=device)


Built = collections.namedtuple("Built", "model engine loader store")


def build(make_store, suffix, dtype, n, frames, crop, rows=None, *, split, name, train=False, force_fw_only=False,
          bank=None, lfb_infer_only=False, shift=1, aug=0, owner=None, device="cuda:0", n_slots=2, max_src_hw=(256, 340)):
    """the model (ModelBuilder(train=, split=, name=, force_fw_only=).build_model(suffix, bank, lfb_infer_only, shift)), its
    engine planned with `input_shapes(model, suffix, n, frames, crop, rows)` (owner: the engine whose parameters it
    aliases), its loader (`make_loader`; `bank` only when the model reads one) and make_store(device, stream), the frame
    store on the loader's stream.  Parameters are neither initialised nor loaded.  -> Built"""
    from models.model_builder_video import ModelBuilder
    from vlfb.engine import Engine
    model = ModelBuilder(train=train, split=split, name=name, force_fw_only=force_fw_only)
    model.build_model(suffix=suffix, lfb=bank, lfb_infer_only=lfb_infer_only, shift=shift)
    engine = Engine(model, dtype, device=device, base_seed=cfg.RNG_SEED, share_params_with=owner)
    engine.plan(input_shapes(model, suffix, n, frames, crop, rows))
    uses_bank = ("lfb" + suffix) in model.input_blob_names
    assert not uses_bank or bank is not None, "the model reads a feature bank (LFB.ENABLED): no bank was given or built"
    loader = make_loader(engine, suffix, aug, bank if uses_bank else None, n_slots, max_src_hw, device)
    return Built(model, engine, loader, make_store(loader.device, loader.stream))


def run_pass(engine, loader, store, source, iterations=None, timer=None, each=None):
    """The loop of a forward pass: `source` (what loader.start takes) walked through `loader` into `engine`.  Per iteration
    timer.tic / next / deliver / forward / timer.toc, then each(it, mb) -- behind the enqueued forward, with the Minibatch
    (mb.meta is the dict the source yielded).  iterations None: until the source ends; an integer: exactly that many (a
    source that ends sooner raises StopIteration).  Nothing in the loop waits for the device.  The loader is stopped
    whatever happens; then one synchronisation and the store's check_decoded (frames it decoded from JPEG bytes: none was
    damaged).  -> iterations run
    A COUNTED pass (`iterations` given: misc.get_total_test_iters batches of BATCH_SIZE clips, walked in per-GPU slices of
    BATCH_SIZE // NUM_GPUS) is shared by the ranks of a process group: `run_pass_ranks`.  With NUM_GPUS > 1 and no group of
    that size it is refused, since one process would cover 1 / NUM_GPUS of the split."""
    import torch
    if iterations is not None:
        from vlfb import dist, hip
        if int(cfg.NUM_GPUS) > 1 and dist.world_size() != int(cfg.NUM_GPUS):
            raise hip.VlfbError("a pass of %d iterations with cfg.NUM_GPUS = %d needs a process group of %d ranks, one per GPU "
                                "(there is %s): one process walks slices of BATCH_SIZE // NUM_GPUS clips and would cover only "
                                "1 / %d of the split" % (iterations, int(cfg.NUM_GPUS), int(cfg.NUM_GPUS),
                                                         "one of %d" % dist.world_size() if dist.initialized() else "none",
                                                         int(cfg.NUM_GPUS)))
        if dist.initialized():
            return run_pass_ranks(engine, loader, store, source, iterations, timer, each)
    ran = 0
    loader.start(source)
    try:
        while ran != iterations:
            if timer is not None:
                timer.tic()
            try:
                mb = loader.next()
            except StopIteration:
                if iterations is None:
                    break
                raise
            loader.deliver(mb)
            engine.forward()
            if timer is not None:
                timer.toc()
            if each is not None:
                each(ran, mb)
            ran += 1
    finally:
        loader.stop()
    torch.cuda.current_stream().synchronize()
    store.check_decoded()
    return ran


def run_pass_ranks(engine, loader, store, source, iterations, timer=None, each=None):
    """The counted `run_pass` under a process group: `source` is the single-process walk in per-GPU slices, slice s belongs
    to rank s % world (lfb_pass.rank_source), global iteration G is slices G * world .. G * world + world - 1, and
    `iterations` counts GLOBAL iterations: ceil(P / world) for P slices, which is misc.get_total_test_iters.  Every rank
    walks all of them; on each it forwards its slice if that exists -- the walk may end inside the LAST global iteration and
    leave the higher ranks without one; rank 0 always has one -- and calls each(G, mb), mb None where it had no slice, so a
    collective in `each` (the meter's read at LOG_PERIOD or at the last iteration) is reached by every rank alike.  The
    outcome is agreed by all ranks (lfb_pass._on_every_rank): one failing rank fails all.  -> global iterations run"""
    import torch
    from vlfb import dist, lfb_pass
    lfb_pass.check_world()
    rank, last = dist.rank(), int(iterations) - 1

    def mine():
        loader.start(lfb_pass.rank_source(source, None))
        try:
            for it in range(int(iterations)):
                if timer is not None:
                    timer.tic()
                try:
                    mb = loader.next()
                except StopIteration:
                    if rank == 0 or it != last:
                        raise                            # (the source is shorter than `iterations` global iterations)
                    mb = None
                if mb is not None:
                    loader.deliver(mb)
                    engine.forward()
                if timer is not None:
                    timer.toc()
                if each is not None:
                    each(it, mb)
        finally:
            loader.stop()
        torch.cuda.current_stream().synchronize()
        store.check_decoded()
    lfb_pass._on_every_rank(mine)
    return int(iterations)
