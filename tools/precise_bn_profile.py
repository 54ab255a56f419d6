"""What precise BN costs, for the record (no gate):

    python tools/precise_bn_profile.py profiles/precise_bn.txt

The SpatialBN charades_r50_baseline graph (MODEL.USE_AFFINE False) at 8 clips of 32 x 224 x 224, bf16, synthetic parameters
and static inputs, through vlfb.precise_bn.PreciseBN's aux engine.  ITERS = TRAIN.ITER_COMPUTE_PRECISE_BN = 200 iterations,
three ways, taking turns REPEATS times after a warm-up, wall time around each block with the device drained at both ends:
  forwards alone                      the aux forward passes, nothing collected
  + vlfb_bn_precise_accumulate        PreciseBN.compute_and_update_bn_stats: one launch per iteration, one read of `bad`
  + two host fetches per layer        the reference's way (bn_helper.py:166-182): `_bn_sm` / `_bn_siv` of every layer copied to
                                      the host after every forward, summed there in numpy
Then the training driver against the bare loop (driver_against_bare_loop): ms per step of vlfb.train_pass.train and of the
deliver / train_step loop alone on the same loader and source.
"""
import collections
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "video-long-term-feature-banks_amd", "lib"), ROOT]

ITERS, REPEATS, N, T, CROP = 200, 3, 8, 32, 224


class StaticLoader(object):
    """inputs stay what they are: the time of a data loader is not what is measured"""

    def next(self):
        return None

    def deliver(self, batch):
        pass

    def stop(self):
        pass


SHORT, LONG, VIDEOS, FRAMES, SRC_H, SRC_W = 24, 72, 4, 160, 256, 340


def driver_against_bare_loop():
    """ms per step of vlfb.train_pass.train against the bare deliver / train_step loop on the same wrapper, loader and source:
    each runs LONG + 1 iterations (no evaluation, one checkpoint at the end, LOG_PERIOD beyond the run); the device is drained
    and the clock read before step SHORT and before step LONG, so building, planning and the final checkpoint stay outside;
    the two take turns REPEATS times.  A host stall the driver added to the loop body would show as a difference."""
    import random
    import tempfile
    from core.config import config as cfg
    from datasets.frame_store import FrameStore
    from utils import misc
    from vlfb import synth, train_pass
    from vlfb.presets import load_preset
    tmp = tempfile.mkdtemp(prefix="vlfb_profile_")
    rows = ["original_vido_id video_id frame_id path labels"]
    for vi in range(VIDEOS):
        rows += ['V%d %d %d V%d/%06d.jpg "%d"' % (vi, vi, k, vi, k + 1, (vi + k // 40) % 157) for k in range(FRAMES)]
    with open(os.path.join(tmp, "frames.csv"), "w") as f:
        f.write("\n".join(rows) + "\n")
    rng = np.random.default_rng(1)
    frames = [rng.integers(0, 256, (FRAMES, SRC_H, SRC_W, 3)).astype(np.uint8) for _ in range(VIDEOS)]

    def make_store(device, stream):
        st = FrameStore(SRC_H, SRC_W, 4 * N * T, device, stream)
        st.fetch = lambda v, f: frames[v][f]
        return st

    def configure(iters):
        load_preset("charades_r50_baseline", [
            "NUM_GPUS", 1, "TRAIN.BATCH_SIZE", N, "TEST.BATCH_SIZE", N, "TRAIN.VIDEO_LENGTH", T, "TEST.VIDEO_LENGTH", T,
            "TRAIN.CROP_SIZE", CROP, "TEST.CROP_SIZE", CROP, "MODEL.USE_AFFINE", False, "NONLOCAL.USE_BN", True,
            "NONLOCAL.USE_AFFINE", False, "MODEL.DILATIONS_AFTER_CONV5", False, "SOLVER.MAX_ITER", iters,
            "SOLVER.STEP_SIZES", [iters], "SOLVER.LRS", [1], "SOLVER.WARMUP.WARMUP_ON", False, "TRAIN.EVAL_PERIOD", 10 ** 6,
            "CHECKPOINT.CHECKPOINT_PERIOD", 10 ** 6, "CHECKPOINT.RESUME", False, "CHECKPOINT.CONVERT_MODEL", False,
            "TRAIN.PARAMS_FILE", "", "TRAIN.TEST_AFTER_TRAIN", False, "TRAIN.SAMPLE_RATE", 4, "TEST.SAMPLE_RATE", 4])
        cfg.CHARADES.FRAME_LIST_DIR, cfg.CHARADES.TRAIN_LISTS, cfg.CHARADES.TEST_LISTS = tmp, ["frames.csv"], ["frames.csv"]
        cfg.CHECKPOINT.DIR, cfg.DATADIR, cfg.LOG_PERIOD = tmp, "", 10 ** 6
        cfg.TRAIN.DATASET_SIZE = cfg.TEST.DATASET_SIZE = VIDEOS

    init = lambda e: e.feed_params({k: v for k, v in synth.params(e.model, seed=2).items() if k in e.param_views})

    def driver(iters):
        configure(iters)
        train_pass.train(make_store, dtype="bf16", max_src_hw=(SRC_H, SRC_W), init_params=init)

    def bare(iters):
        configure(iters)
        misc.generate_random_seed()
        cfg.CHARADES.NUM_TEST_CLIPS = cfg.CHARADES.NUM_TEST_CLIPS_DURING_TRAINING
        try:
            tr = train_pass.create_wrapper(True, make_store, None, dtype="bf16", max_src_hw=(SRC_H, SRC_W))
            init(tr.engine)
            te = train_pass.create_wrapper(False, make_store, None, owner=tr.engine, dtype="bf16", max_src_hw=(SRC_H, SRC_W))
            tr.loader.start(train_pass.train_source(tr, random.Random(cfg.RNG_SEED), np.random))
            try:
                for it in range(iters):
                    tr.model.UpdateWorkspaceLr(it)
                    tr.loader.deliver(tr.loader.next())
                    tr.engine.train_step(float(tr.model.current_lr))
            finally:
                tr.loader.stop()
            del te
        finally:
            del cfg.CHARADES["NUM_TEST_CLIPS"]

    from vlfb.engine import Engine
    real_step = Engine.train_step
    marks = {}

    def timed_step(self, lr=None):
        # the device is drained, and the clock read, before step SHORT and before step LONG only: the steps between them
        # run as they do in training
        if self.train and marks["calls"] in (SHORT, LONG):
            torch.cuda.synchronize()
            marks[marks["calls"]] = time.perf_counter()
        marks["calls"] += 1
        return real_step(self, lr)

    def per_step(fn):
        marks.clear()
        marks["calls"] = 0
        fn(LONG + 1)
        return 1e3 * (marks[LONG] - marks[SHORT]) / (LONG - SHORT)

    Engine.train_step = timed_step
    try:
        marks["calls"] = -10 ** 6
        bare(4)                                              # warm-up: code objects, allocator, page cache of the frames
        per = {"train()": [], "bare loop": []}
        for _ in range(REPEATS):
            for name, fn in (("train()", driver), ("bare loop", bare)):
                per[name].append(per_step(fn))
    finally:
        Engine.train_step = real_step
    text = ("\nper training step, the same graph (precise BN off), %d videos of %d frames %d x %d through FrameLoader, bf16:\n"
            "(device drained and clock read before step %d and before step %d, the time between over %d steps; %d repeats taking turns)\n"
            "loop                                ms / step (median)    all repeats\n" % (VIDEOS, FRAMES, SRC_H, SRC_W, SHORT, LONG, LONG - SHORT, REPEATS))
    for name in ("train()", "bare loop"):
        text += "%-34s  %10.2f            %s\n" % (name, float(np.median(per[name])), " ".join("%.2f" % t for t in per[name]))
    return text


def main():
    from core.config import config as cfg
    from models.model_builder_video import ModelBuilder
    from vlfb import synth
    from vlfb.engine import Engine
    from vlfb.precise_bn import PreciseBN
    from vlfb.presets import load_preset
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    load_preset("charades_r50_baseline", ["NUM_GPUS", 1, "TRAIN.BATCH_SIZE", N, "TRAIN.VIDEO_LENGTH", T, "TRAIN.CROP_SIZE", CROP,
                                          "MODEL.USE_AFFINE", False, "NONLOCAL.USE_BN", True, "NONLOCAL.USE_AFFINE", False,
                                          "MODEL.DILATIONS_AFTER_CONV5", False, "TRAIN.COMPUTE_PRECISE_BN", True,
                                          "TRAIN.ITER_COMPUTE_PRECISE_BN", ITERS])
    m = ModelBuilder(train=True, split="train", name="train")
    m.build_model(suffix="_train")
    eng = Engine(m, "bf16", device="cuda:0", base_seed=2)
    shapes = {"data_train": (N, 3, T, CROP, CROP), "labels_train": (N, cfg.MODEL.NUM_CLASSES)}
    eng.plan(collections.OrderedDict((name, shapes[name]) for name in m.input_blob_names))
    eng.feed_params({k: v for k, v in synth.params(m, seed=2).items() if k in eng.param_views})
    pbn = PreciseBN(eng, lambda engine, suffix: StaticLoader())
    aux = pbn.engine
    rng = np.random.default_rng(0)
    aux.feed("data_bn_aux", rng.standard_normal(shapes["data_train"]).astype(np.float32))
    aux.feed("labels_bn_aux", (rng.uniform(size=shapes["labels_train"]) < 0.05).astype(np.int32))

    def forwards_alone():
        for _ in range(ITERS):
            aux.forward()

    def with_kernel():
        pbn.compute_and_update_bn_stats(None)

    def with_fetches():
        eps = np.float32(cfg.MODEL.BN_EPSILON)
        mean = [0] * pbn.layers
        mean2 = [0] * pbn.layers
        for _ in range(ITERS):
            aux.forward()
            for k, st in enumerate(pbn.steps):
                sm = st.save[:st.C].cpu().numpy()
                siv = st.save[st.C:].cpu().numpy()
                mean[k] = mean[k] + sm
                mean2[k] = mean2[k] + ((np.float32(1) / siv) ** 2 - eps + sm ** 2)

    ways = [("forwards alone", forwards_alone), ("+ vlfb_bn_precise_accumulate", with_kernel),
            ("+ two host fetches per layer", with_fetches)]
    for _ in range(10):
        aux.forward()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in ways}
    for _ in range(REPEATS):
        for name, fn in ways:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    text = ("precise BN, charades_r50_baseline with SpatialBN (%d layers, %d channels), %d clips x %d frames, crop %d, bf16, %s\n"
            "%d iterations per block, %d blocks per way taking turns, wall time with the device drained at both ends\n"
            "way                                 s / block (median)    ms / iteration    all blocks\n"
            % (pbn.layers, pbn.total, N, T, CROP, torch.cuda.get_device_name(0), ITERS, REPEATS))
    for name, _ in ways:
        med = float(np.median(times[name]))
        text += "%-34s  %10.3f          %10.3f        %s\n" % (name, med, 1e3 * med / ITERS, " ".join("%.3f" % t for t in times[name]))
    del pbn, aux, eng, m
    torch.cuda.empty_cache()
    text += driver_against_bare_loop()
    sys.stdout.write(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
