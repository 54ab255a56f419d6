#!/usr/bin/env python
"""What the device-resident AVA multi-crop pass costs per minibatch, beside the path it replaces: 8 clips of 32 frames at
rate 2 from 256 x 340 uint8 frames, keyframes one second apart in one video, 3 boxes per keyframe, scales 224 / 256 / 320
x 2 flips x 3 shifts = 18 views, in ONE process on one GPU two ways over the SAME two engines (crops 224 and 256),

  (a) pass      vlfb.multicrop.AvaMultiCropPass.run_minibatch: clips as frame lists into a FrameStore, one indexed
                preprocess launch per view, `pred` copied on the device, vlfb_multicrop_merge, no wait in the loop,
  (b) tester    vlfb.multicrop.AvaMultiCropTester.run on the same clips as stacked host arrays: every clip uploaded and
                preprocessed once per view, a synchronisation and a fetch of `pred` per view, the merge in NumPy,
  (c) static    the 18 forward passes alone on inputs that are never touched: the floor of both.

"Decoding" is a lookup in a pool of frames generated up front, so a fetched frame costs its copy only; a real decoder makes
every fetched frame dearer and (b), which fetches each frame 18 times, slower still.  Each way runs --warmup untimed
minibatches and --steps timed ones between two device synchronisations; frames fetched are exact counts.

    python tools/multicrop_pass_profile.py --steps 10 --warmup 2 > profiles/multicrop_pass.txt
"""
import argparse
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
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--rate", type=int, default=2)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--src", type=int, nargs=2, default=[256, 340])
    ap.add_argument("--pool", type=int, default=512, help="distinct frames generated on the host")
    args = ap.parse_args()

    import torch
    from oracle import model as om
    from vlfb.presets import load_preset
    from core.config import config as cfg
    from datasets import ava
    from datasets.frame_store import FrameStore
    from vlfb import multicrop as mc

    N, T, PER = args.clips, args.frames, 3
    H, W = args.src
    load_preset("ava_r50_baseline", ["NUM_GPUS", 1, "TEST.BATCH_SIZE", N, "TEST.VIDEO_LENGTH", T, "TRAIN.VIDEO_LENGTH", T,
                                     "TEST.SAMPLE_RATE", args.rate, "AVA.TEST_MULTI_CROP", True])
    scales = list(cfg.AVA.TEST_MULTI_CROP_SCALES)
    batches = args.warmup + args.steps
    gen = np.random.default_rng(0)
    pool = gen.integers(0, 256, (args.pool, H, W, 3), dtype=np.uint8)
    secs = list(range(902, 902 + batches * N))
    n_frames = ava.sec_to_frame(secs[-1]) + T * args.rate
    per_sec = {}
    for s in ava.AVA_VALID_FRAMES:
        per_sec[s] = []
    for s in secs:
        x1 = gen.uniform(0.05, 0.6, PER)
        y1 = gen.uniform(0.05, 0.6, PER)
        per_sec[s] = [[[float(x1[k]), float(y1[k]), float(x1[k] + 0.3), float(y1[k] + 0.3)], [-1]] for k in range(PER)]
    index = ava.AvaIndex([[None] * n_frames], {0: "video"}, [per_sec], "test", False)
    assert index.get_db_size() == batches * N

    def make_store(device, stream):
        st = FrameStore(H, W, 2 * N * T, device, stream)
        st.fetch = lambda video, f: pool[f % args.pool]
        return st

    p = mc.AvaMultiCropPass(index, make_store, om.synth_params(cfg, seed=cfg.RNG_SEED), dtype=args.dtype)
    source = list(ava.minibatch_source(index, p.store, np.random))
    assert len(source) == batches
    torch.cuda.synchronize()
    fwd = [0.0]                                              # host time inside Engine.forward (issuing one view's launches)
    for _, eng in p.engines:
        def timed(plain=eng.forward):
            t = time.perf_counter()
            plain()
            fwd[0] += time.perf_counter() - t
        eng.forward = timed

    # (a) the pass
    for a in source[:args.warmup]:
        p.run_minibatch(*a)
    torch.cuda.synchronize()
    fetched0, host0, fwd0 = p.store.fetched, p.host_seconds, fwd[0]
    t0 = time.perf_counter()
    for a in source[args.warmup:]:
        p.run_minibatch(*a)
    p.stream.synchronize()
    pass_ms = (time.perf_counter() - t0) / args.steps * 1e3
    pass_host_ms = (p.host_seconds - host0) / args.steps * 1e3
    pass_frames = (p.store.fetched - fetched0) / float(args.steps)
    pass_fwd_ms = (fwd[0] - fwd0) / args.steps * 1e3
    res = p.finish(({}, {}, {}))

    # (c) the floor: the 18 forward passes alone, on whatever the engines hold (nothing fed, copied or merged)
    def forwards():
        for view in p.views:
            p.engine_of_crop[view.crop].forward()
    with torch.cuda.stream(p.stream):
        forwards()
        p.stream.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            forwards()
        p.stream.synchronize()
        static_ms = (time.perf_counter() - t0) / args.steps * 1e3
        single = []                                          # one forward pass on an idle device: host time to issue it, time until done
        for crop in sorted(p.engine_of_crop):
            t0 = time.perf_counter()
            p.engine_of_crop[crop].forward()
            t1 = time.perf_counter()
            p.stream.synchronize()
            single.append((crop, (t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3))

    # (b) the tester, on the same engines and the same clips as stacked arrays
    def stacked(a):
        return [pool[np.array(seq) % args.pool] for _, _, seq in a[0]], a[1]
    want = []
    for a in source[:args.warmup]:
        want.append(p.tester.run(*stacked(a))[0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for a in source[args.warmup:]:
        want.append(p.tester.run(*stacked(a))[0])
    torch.cuda.synchronize()
    tester_ms = (time.perf_counter() - t0) / args.steps * 1e3
    tester_frames = len(p.views) * N * T
    want = np.concatenate(want)
    rel = float(np.max(np.abs(res["scores"] - want) / np.abs(want)))

    print("ava_r50_baseline %s, forward only, %d clips of %d frames (rate %d, keyframes 1 s apart), %d RoIs, scales %r -> crops %r, "
          "%d views, sources %d x %d uint8; %s; %d timed minibatches after %d warm-up"
          % (args.dtype, N, T, args.rate, p.rows, scales, sorted(set(v.crop for v in p.views)), len(p.views), H, W,
             torch.cuda.get_device_name(0), args.steps, args.warmup))
    print("%-8s %12s %16s %22s" % ("way", "ms/minibatch", "host ms/minibatch", "frames fetched/minibatch"))
    print("%-8s %12.1f %16.1f %22.1f" % ("pass", pass_ms, pass_host_ms, pass_frames))
    print("%-8s %12.1f %16s %22.1f" % ("tester", tester_ms, "(synchronous)", tester_frames))
    print("%-8s %12.1f %16s %22.1f" % ("static", static_ms, "-", 0.0))
    print("pass over static: %+.1f ms per minibatch (%+.1f %%)" % (pass_ms - static_ms, 100.0 * (pass_ms - static_ms) / static_ms))
    for crop, issue, done in single:
        print("one forward pass at crop %d on an idle device: issued in %.2f ms of host time, done after %.2f ms" % (crop, issue, done))
    print("pass: %.1f ms of its host time per minibatch are the %d Engine.forward() calls issuing their launches"
          % (pass_fwd_ms, len(p.views)))
    print("tester / pass: %.2fx per minibatch; frames fetched %.1fx" % (tester_ms / pass_ms, tester_frames / max(pass_frames, 1e-9)))
    print("merged scores of the two ways: max relative difference %.3e over %d x %d" % ((rel,) + res["scores"].shape))


if __name__ == "__main__":
    main()
