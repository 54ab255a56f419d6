#!/usr/bin/env python
"""What a frame store saves a bank-construction pass: the AVA pass (ava_r50_baseline, lfb_infer_only, forward only; 8 clips
of 32 frames at rate 2 from 256 x 340 uint8 frames, keyframes every 30 frames of one video, test preprocessing) fed to
datasets.clip_loader.MinibatchLoader in ONE process on one GPU three ways,

  (a) static    the inputs sit on the device and are never touched (the forward pass alone),
  (b) stacked   every clip handed over as its (32, 256, 340, 3) array: every frame staged and uploaded for every clip that
                contains it (all the loader could do before datasets.frame_store),
  (c) store     every clip handed over as (store, video, frame_numbers): only the frames that are not resident in the
                datasets.frame_store.FrameStore are fetched and uploaded, the kernels read through the slot table,

with the loader's background thread running in (b) and (c).  "Decoding" is a lookup in a pool of frames generated up
front, so the host cost of both feeds is the copies only -- a real decoder makes every fetched frame dearer and the gap
wider.  The feeds take turns, each turn is --warmup untimed steps and --steps timed ones between two device
synchronisations.  Frames fetched and bytes uploaded per clip are exact counts.

    python tools/frame_store_pass.py --steps 30 --repeats 3 > profiles/frame_store_lfb_pass.txt
"""
import argparse
import collections
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "video-long-term-feature-banks_amd", "lib"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--rate", type=int, default=2)
    ap.add_argument("--stride", type=int, default=30, help="frames between the centres of successive clips")
    ap.add_argument("--dtype", default="mix")
    ap.add_argument("--src", type=int, nargs=2, default=[256, 340])
    ap.add_argument("--pool", type=int, default=512, help="distinct frames generated on the host")
    args = ap.parse_args()

    import torch
    from vlfb import synth
    from vlfb.presets import load_preset
    from core.config import config as cfg
    from models.model_builder_video import ModelBuilder
    from vlfb.engine import Engine
    from datasets import dataset_helper
    from datasets.clip_loader import MinibatchLoader
    from datasets.frame_store import FrameStore

    N, T, PER = args.clips, args.frames, 3
    H, W = args.src
    load_preset("ava_r50_baseline", ["NUM_GPUS", 1, "TEST.BATCH_SIZE", N, "TEST.VIDEO_LENGTH", T, "TRAIN.VIDEO_LENGTH", T,
                                     "TEST.SAMPLE_RATE", args.rate])
    CROP = cfg.TEST.CROP_SIZE
    model = ModelBuilder(train=False, split="test", name="lfb_pass")
    model.build_model(suffix="_test", lfb_infer_only=True)
    eng = Engine(model, args.dtype, device="cuda:0", base_seed=cfg.RNG_SEED)
    R = N * PER
    shapes = {"data_test": (N, 3, T, CROP, CROP), "labels_test": (R, cfg.MODEL.NUM_CLASSES), "proposals_test": (R, 5)}
    eng.plan(collections.OrderedDict((k, shapes[k]) for k in model.input_blob_names))
    eng.feed_params({k: v for k, v in synth.params(model, seed=cfg.RNG_SEED).items() if k in eng.param_views})
    batch = synth.inputs(cfg, N, PER, seed=cfg.RNG_SEED, crop=CROP, frames=T, suffix="_test")
    for k in model.input_blob_names:
        eng.feed(k, batch[k])

    gen = np.random.default_rng(0)
    pool = gen.integers(0, 256, (args.pool, H, W, 3), dtype=np.uint8)
    boxes01 = [np.sort(gen.uniform(0.05, 0.95, (PER, 2, 2)), axis=1).reshape(PER, 4) for _ in range(N)]
    labels = [np.zeros((PER, cfg.MODEL.NUM_CLASSES), np.int32) for _ in range(N)]
    half = T * args.rate // 2
    video_frames = 10 ** 9                                  # (one long video: no clip is clamped)

    def sequences(k):
        """the clips of minibatch k: centres `stride` frames apart, continuing where minibatch k - 1 ended"""
        first = half + k * N * args.stride
        return [dataset_helper.get_sequence(first + n * args.stride, half, args.rate, video_frames) for n in range(N)]

    loader = MinibatchLoader(eng, "_test", 0, n_slots=2, max_src_hw=(H, W), src_sizes=[(H, W)])
    store = FrameStore(H, W, N * T, loader.device, loader.stream)        # a minibatch's distinct frames and most of the next's
    store.fetch = lambda video, f: pool[f % args.pool]
    it = {"stacked": 0, "store": 0}

    def source(name):
        while True:
            k = it[name]
            it[name] += 1
            seqs = sequences(k)
            meta = dict(iteration=k, videos=[0] * N, secs=[902 + k * N + n for n in range(N)])
            if name == "stacked":
                frames = [pool[np.array(s) % args.pool] for s in seqs]
            else:
                frames = [(store, 0, s) for s in seqs]
            yield (frames, boxes01, labels, meta, None)

    submit_s = {"stacked": [], "store": []}
    plain_submit = loader.submit
    current = [None]

    def timed_submit(*a, **kw):
        t0 = time.perf_counter()
        try:
            return plain_submit(*a, **kw)
        finally:
            submit_s[current[0]].append(time.perf_counter() - t0)
    loader.submit = timed_submit

    def run(name, steps):
        for _ in range(steps):
            if name != "static":
                loader.deliver(loader.next())
            eng.forward()

    ms = collections.OrderedDict((name, []) for name in ("static", "stacked", "store"))
    for rep in range(args.repeats):
        for name in ms:
            if name != "static":
                current[0] = name
                loader.start(source(name))
            run(name, args.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, args.steps)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / args.steps * 1e3)
            if name != "static":
                loader.stop()
    # on an otherwise idle device, five minibatches (40 clips) of a stretch of the video nothing has touched: the loader
    # stream's device time per minibatch, and the exact frame counts (the background thread above runs ahead of deliver and
    # what it prepared last is dropped by stop(), so its counts are not per delivered clip)
    loader.submit = plain_submit
    dev_ms, counts = {}, {"stacked": [5 * N, 5 * N * T]}
    for name in ("stacked", "store"):
        it[name] += 1000
        fetched0 = store.fetched
        src, v = source(name), []
        for _ in range(5):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record(loader.stream)
            mb = loader.submit(*next(src))
            ev[1].record(loader.stream)
            torch.cuda.synchronize()
            loader.deliver(mb)
            v.append(ev[0].elapsed_time(ev[1]))
        dev_ms[name] = float(np.median(v))
        if name == "store":
            counts[name] = [5 * N, store.fetched - fetched0]
    torch.cuda.synchronize()
    feat = eng.fetch("box_pooled")

    fb = H * W * 3
    print("ava_r50_baseline lfb_infer_only %s, forward only, %d clips of %d frames (rate %d, centres %d frames apart) at crop %d, "
          "%d RoIs, sources %d x %d uint8; %s; %d repeats of %d steps after %d warm-up"
          % (args.dtype, N, T, args.rate, args.stride, CROP, R, H, W, torch.cuda.get_device_name(0), args.repeats, args.steps,
             args.warmup))
    print("%-8s %s   median      min      max   (ms per step)   steps/s (median)"
          % ("feed", " ".join("%8s" % ("rep%d" % r) for r in range(args.repeats))))
    for name, v in ms.items():
        med = float(np.median(v))
        print("%-8s %s %8.3f %8.3f %8.3f %26.2f" % (name, " ".join("%8.3f" % x for x in v), med, min(v), max(v), 1e3 / med))
    for name in ("stacked", "store"):
        clips, frames = counts[name]
        print("%-8s frames fetched and uploaded per clip %.2f (%d frames for %d clips), H2D %.2f MB per clip; host time of one "
              "submit() %.2f ms (mean of %d); loader stream on an idle device %.3f ms per minibatch (median of 5)"
              % (name, frames / clips, frames, clips, frames / clips * fb / 1e6, 1e3 * float(np.mean(submit_s[name])),
                 len(submit_s[name]), dev_ms[name]))
    print("store: after the first clip (which finds the store empty) %.2f frames fetched per clip"
          % ((counts["store"][1] - T) / (counts["store"][0] - 1.0)))
    print("store: %d frames requested, %d fetched, capacity %d frames (%.1f MB on the device)"
          % (store.requested, store.fetched, store.capacity, store.capacity * fb / 1e6))
    stat = float(np.median(ms["static"]))
    for name in ("stacked", "store"):
        over = float(np.median(ms[name])) - stat
        print("%-8s over the static forward pass: %+.3f ms per step (%+.1f %%)" % (name, over, 100.0 * over / stat))
    print("box_pooled finite: %s" % bool(np.isfinite(feat).all()))


if __name__ == "__main__":
    main()
