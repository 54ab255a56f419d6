#!/usr/bin/env python
"""What feeding real frames costs a training step: ms per step of ava_r50_lfb_nl (8 clips of 32 x 224^2, `mix`, 3 RoIs per
clip) in ONE process on one GPU for three feeds,

  (a) static   the inputs sit on the device and are never touched (what bench.py times),
  (b) inline   per-clip datasets.data_input_helper.images_and_boxes_preprocessing + Engine.feed + DeviceBank.sample_window on
               the training thread before every step (all there was before datasets.clip_loader),
  (c) loader   datasets.clip_loader.MinibatchLoader with its background thread; the training thread only calls deliver(),

from 256 x 340 uint8 frames generated on the host.  The feeds take turns (a, b, c, a, b, c, ...), each turn is --warmup
untimed steps and --steps timed ones between two device synchronisations; the table gives every repeat, the median and
the spread.  For (c) the mean host time of one submit() is printed as well (planning, the copy into pinned memory and the
enqueue: what the background thread spends per minibatch).

    python tools/loader_overlap.py --steps 40 --repeats 3 > profiles/loader_overlap.txt
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
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--dtype", default="mix")
    ap.add_argument("--src", type=int, nargs=2, default=[256, 340])
    ap.add_argument("--color", action="store_true", help="TRAIN.USE_COLOR_AUGMENTATION")
    ap.add_argument("--jpeg", action="store_true", help="(c) reads its clips from a FrameStore fed JPEG bytes (fetch_jpeg), every "
                    "frame new every step: the frames are decoded on the loader's stream (tools/jpeg_decode_profile.py makes them)")
    ap.add_argument("--target-bytes", type=int, default=55000, help="--jpeg: mean file size the quality is chosen for")
    args = ap.parse_args()

    import torch
    from vlfb import synth
    from vlfb.presets import load_preset
    from core.config import config as cfg
    from models.model_builder_video import ModelBuilder
    from vlfb.engine import Engine
    from vlfb.lfb_bank import DeviceBank
    from datasets import data_input_helper as dh
    from datasets.clip_loader import MinibatchLoader
    import utils.lr_policy as lr_policy

    N, T, CROP, PER = args.clips, args.frames, args.crop, 3
    H, W = args.src
    load_preset("ava_r50_lfb_nl", ["NUM_GPUS", 1, "TRAIN.BATCH_SIZE", N, "TRAIN.VIDEO_LENGTH", T, "TRAIN.CROP_SIZE", CROP])
    cfg.TRAIN.USE_COLOR_AUGMENTATION = bool(args.color)
    model = ModelBuilder(train=True, split="train", name="overlap")
    model.build_model(suffix="_train")
    eng = Engine(model, args.dtype, device="cuda:0", base_seed=cfg.RNG_SEED)
    batch = synth.inputs(cfg, N, PER, seed=cfg.RNG_SEED, crop=CROP, frames=T)
    eng.plan(collections.OrderedDict((k, v.shape) for k, v in batch.items() if k in model.input_blob_names))
    eng.feed_params(synth.params(model, seed=cfg.RNG_SEED))
    lr = float(lr_policy.get_lr_at_iter(0))
    R = N * PER
    window, per_step = cfg.LFB.WINDOW_SIZE, cfg.AVA.LFB_MAX_NUM_FEAT_PER_STEP

    gen = np.random.default_rng(0)
    videos = [gen.integers(0, 256, (T, H, W, 3), dtype=np.uint8) for _ in range(N)]
    boxes01 = [np.sort(gen.uniform(0.05, 0.95, (PER, 2, 2)), axis=1).reshape(PER, 4) for _ in range(N)]
    labels = (gen.uniform(size=(R, cfg.MODEL.NUM_CLASSES)) < 0.05).astype(np.int32)
    secs = 902 + window // 2 + np.arange(N)
    bank = DeviceBank(N, window + N + 2, per_step, cfg.LFB.LFB_DIM, "bf16", step_base=902)
    nfeat = N * (window + N) * 3
    bank.append(torch.as_tensor(np.maximum(gen.standard_normal((nfeat, cfg.LFB.LFB_DIM)), 0).astype(np.float32)),
                np.arange(nfeat) % N, 902 + (np.arange(nfeat) // N) % (window + N))
    bank.check_no_drops()
    lfb_in, _ = eng.blob_tensor("lfb_train")
    data, (w_pad, c_pad) = eng.blob_padded("data_train")
    it = [0]

    def feed_static():
        pass

    def feed_inline():
        rng = np.random.RandomState(it[0])
        rois = []
        for n in range(N):
            _, b = dh.images_and_boxes_preprocessing(videos[n], 1, CROP, 1, boxes01[n].copy(), out=data[n], w_pad=w_pad,
                                                     c_pad=c_pad, rng=rng)
            rois.append(np.concatenate([np.full((len(b), 1), n), b], axis=1))
        props = np.concatenate(rois).astype(np.float32)
        eng.feed("proposals_train", props)
        eng.feed("labels_train", labels)
        clip_of = props[:, 0].astype(np.int64)
        bank.sample_window(clip_of, secs[clip_of], it[0] * N + clip_of, window, per_step, seed=cfg.RNG_SEED, out=lfb_in)

    loader = MinibatchLoader(eng, "_train", 1, n_slots=2, max_src_hw=(H, W), bank=bank, src_sizes=[(H, W)])
    submit_s = []
    plain_submit = loader.submit

    def timed_submit(*a, **kw):
        t0 = time.perf_counter()
        try:
            return plain_submit(*a, **kw)
        finally:
            submit_s.append(time.perf_counter() - t0)
    loader.submit = timed_submit

    store = None
    if args.jpeg:
        from datasets.frame_store import FrameStore
        from jpeg_decode_profile import make_frames
        files, _, quality = make_frames(N * T, H, W, args.target_bytes)
        store = FrameStore(H, W, 2 * N * T, loader.device, loader.stream)
        store.fetch_jpeg = lambda v, f: files[(v * T + f) % (N * T)]

    def source():
        k = 0
        while True:
            # --jpeg: clip n of step k is frames k * T .. of video n, none of them resident
            clips = videos if store is None else [(store, n, list(range(k * T, (k + 1) * T))) for n in range(N)]
            yield (clips, boxes01, [labels[n * PER:(n + 1) * PER] for n in range(N)],
                   dict(iteration=k, videos=list(range(N)), secs=list(secs)), np.random.RandomState(k))
            k += 1

    def feed_loader():
        loader.deliver(loader.next())

    def run(feed, steps):
        for _ in range(steps):
            feed()
            eng.train_step(lr)
            it[0] += 1

    for k, v in batch.items():
        if k in model.input_blob_names:
            eng.feed(k, v)
    feeds = [("static", feed_static), ("inline", feed_inline), ("loader", feed_loader)]
    ms = collections.OrderedDict((name, []) for name, _ in feeds)
    for rep in range(args.repeats):
        for name, feed in feeds:
            if name == "loader":
                loader.start(source())
            run(feed, args.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(feed, args.steps)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / args.steps * 1e3)
            if name == "loader":
                loader.stop()
    # where a minibatch's device time goes, on an otherwise idle device: the loader stream's share (copy of the frames from
    # pinned memory, the launches, the bank sample: beside the step) and deliver's copies (on the training stream: in the step)
    loader.submit = plain_submit
    dev_ms = {"loader stream": [], "deliver": []}
    src = source()
    for _ in range(5):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        torch.cuda.synchronize()
        ev[0].record(loader.stream)
        mb = loader.submit(*next(src))
        ev[1].record(loader.stream)
        torch.cuda.synchronize()
        ev[2].record()
        loader.deliver(mb)
        ev[3].record()
        torch.cuda.synchronize()
        dev_ms["loader stream"].append(ev[0].elapsed_time(ev[1]))
        dev_ms["deliver"].append(ev[2].elapsed_time(ev[3]))
    eng.train_step(lr)
    loss = float(eng.fetch("loss").reshape(-1)[0])
    print("ava_r50_lfb_nl %s, %d clips of %d x %d^2, %d RoIs, sources %d x %d uint8%s; %s; %d repeats of %d steps after %d warm-up"
          % (args.dtype, N, T, CROP, R, H, W, ", colour augmentation" if args.color else "",
             torch.cuda.get_device_name(0), args.repeats, args.steps, args.warmup))
    print("%-8s %s   median      min      max   (ms per step)" % ("feed", " ".join("%8s" % ("rep%d" % r) for r in range(args.repeats))))
    for name, v in ms.items():
        print("%-8s %s %8.3f %8.3f %8.3f" % (name, " ".join("%8.3f" % x for x in v), float(np.median(v)), min(v), max(v)))
    if store is None:
        print("loader: host time of one submit() %.2f ms (mean of %d), %.1f MB of frames per minibatch through pinned memory"
              % (1e3 * float(np.mean(submit_s)), len(submit_s), N * T * H * W * 3 / 1e6))
    else:
        store.check_decoded()
        print("loader: host time of one submit() %.2f ms (mean of %d): %d JPEG files of mean %d bytes (PIL quality %d) parsed, copied "
              "into the pinned ring and decoded on the loader's stream; %.1f MB per minibatch through pinned memory"
              % (1e3 * float(np.mean(submit_s)), len(submit_s), N * T, int(np.mean([len(f) for f in files])), quality,
                 store.uploaded_bytes / max(store.fetched, 1) * N * T / 1e6))
    print("idle device, per minibatch: loader stream %.3f ms (H2D copies + launches + bank sample), deliver %.3f ms "
          "(device-to-device copies of %.0f MB on the training stream); medians of 5"
          % (float(np.median(dev_ms["loader stream"])), float(np.median(dev_ms["deliver"])),
             sum(t.numel() * t.element_size() for t in loader.dst.values()) / 1e6))
    print("last loss %.6f (finite: %s)" % (loss, np.isfinite(loss)))


if __name__ == "__main__":
    main()
