"""Shapes and configuration shared by tests/test_clip_loader_host.py and tests/test_clip_loader_gpu.py: the smallest
minibatches at which the batched clip kernels can still go wrong -- three clips of different sources (landscape, portrait,
and one that needs no resize when the jitter draws 64), 3 frames, crop 64, jitter scales 64..80."""
import contextlib

import numpy as np

T, CROP = 3, 64
SIZES = [(72, 96), (90, 70), (64, 88)]
RESET = ("ava_r50_lfb_nl", ["NUM_GPUS", 1])


@contextlib.contextmanager
def loader_cfg(preset="ava_r50_lfb_nl", clips=3, frames=T, color=False, pca_only=None, jitter=(CROP, CROP + 16), extra=()):
    """the product cfg for a minibatch of `clips` clips; everything is put back afterwards"""
    from vlfb.presets import load_preset
    from core.config import config as cfg
    load_preset(preset, ["NUM_GPUS", 1, "TRAIN.BATCH_SIZE", clips, "TEST.BATCH_SIZE", clips, "TRAIN.VIDEO_LENGTH", frames,
                         "TEST.VIDEO_LENGTH", frames, "TRAIN.CROP_SIZE", CROP, "TEST.CROP_SIZE", CROP, "TEST.SCALE", CROP,
                         "TRAIN.JITTER_SCALES", list(jitter)] + list(extra))
    cfg.TRAIN.USE_COLOR_AUGMENTATION = color
    if pca_only is not None:
        cfg.TRAIN.PCA_JITTER_ONLY = pca_only
    try:
        yield cfg
    finally:
        load_preset(*RESET)


# colour modes of the kernel tests: off, brightness + contrast + saturation + lighting, lighting only
COLOR_MODES = {"off": dict(color=False), "all": dict(color=True), "light": dict(color=True, pca_only=True)}


def clips(seed, sizes=SIZES, frames=T):
    """uint8 BGR clips (frames, H, W, 3), one per size; `frames` one number or one per clip"""
    rng = np.random.default_rng(1000 + seed)
    fr = frames if isinstance(frames, (list, tuple)) else [frames] * len(sizes)
    return [rng.integers(0, 256, (f, h, w, 3)).astype(np.uint8) for f, (h, w) in zip(fr, sizes)]


def boxes(seed, counts):
    """normalised boxes (k, 4) per clip, x1 < x2 and y1 < y2"""
    rng = np.random.default_rng(2000 + seed)
    out = []
    for k in counts:
        lo = rng.uniform(0.0, 0.5, (k, 2))
        hi = lo + rng.uniform(0.2, 0.5, (k, 2))
        out.append(np.concatenate([lo, hi], axis=1))
    return out
