"""Per-iteration time of an EPIC test pass with and without the kept predictions, for the record:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/epic_keep_profile.py profiles/epic_test_pass_keep.txt

The small epic_verb_r50_baseline test engine of the pass tests (crop 64, 4 frames, 2 clips, bf16, synthetic parameters and
inputs) with the meter utils.metrics.MetricsCalculator attaches: ITERS forward passes with a plain "topk" meter
(vlfb_topk_hits, the launch the pass has always had) and ITERS with keep_rows (vlfb_topk_hits_keep), timed with events
around the whole loop after a warm-up.  The kernel trace of the same run names the two instantiations of topk_hits_kernel
(<T, false> / <T, true>); their mean durations are the difference the kept table costs."""
import collections
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "video-long-term-feature-banks_amd", "lib"), ROOT]

ITERS, WARMUP, N, T, CROP = 200, 20, 2, 4, 64


def main():
    from core.config import config as cfg
    from models.model_builder_video import ModelBuilder
    from vlfb import synth
    from vlfb.engine import Engine
    from vlfb.metrics import DeviceMeter
    from vlfb.presets import load_preset
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    load_preset("epic_verb_r50_baseline", ["NUM_GPUS", 1, "TRAIN.BATCH_SIZE", N, "TEST.BATCH_SIZE", N, "TRAIN.VIDEO_LENGTH", T,
                                           "TEST.VIDEO_LENGTH", T, "TRAIN.CROP_SIZE", CROP, "TEST.CROP_SIZE", CROP, "TEST.SCALE", CROP,
                                           "TEST.SAMPLE_RATE", 4, "NONLOCAL.CONV3_NONLOCAL", False])
    sfx = "_final_test"
    m = ModelBuilder(train=False, split="test", name="test")
    m.build_model(suffix=sfx)
    eng = Engine(m, "bf16", device="cuda:0", base_seed=2)
    shapes = {"data" + sfx: (N, 3, T, CROP, CROP), "labels" + sfx: (N,)}
    eng.plan(collections.OrderedDict((name, shapes[name]) for name in m.input_blob_names))
    eng.feed_params({k: v for k, v in synth.params(m, seed=2).items() if k in eng.param_views})
    rng = np.random.default_rng(0)
    eng.feed("data" + sfx, rng.standard_normal(shapes["data" + sfx]).astype(np.float32))
    eng.feed("labels" + sfx, rng.integers(0, cfg.MODEL.NUM_CLASSES, N).astype(np.int32))

    def run(meter):
        eng.attach_meter(meter)
        for _ in range(WARMUP):
            eng.forward()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            eng.forward()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / ITERS

    rows = (WARMUP + ITERS) * N
    plain = run(DeviceMeter("topk", cfg.MODEL.NUM_CLASSES, (1, 5), device=eng.device))
    keep_meter = DeviceMeter("topk", cfg.MODEL.NUM_CLASSES, (1, 5), device=eng.device, keep_rows=rows)
    keep = run(keep_meter)
    assert keep_meter.kept()[0].shape[0] == rows
    text = ("EPIC verb test pass, %d clips x %d frames, crop %d, bf16, %s; %d iterations after %d warm-up, events around the loop\n"
            "meter                         ms / iteration\n"
            "topk (vlfb_topk_hits)         %10.4f\n"
            "topk + keep_rows (..._keep)   %10.4f\n" % (N, T, CROP, torch.cuda.get_device_name(0), ITERS, WARMUP, plain, keep))
    sys.stdout.write(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
