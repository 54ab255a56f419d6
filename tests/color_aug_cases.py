"""Glue shared by tests/test_color_aug_host.py and tests/test_color_aug_gpu.py: the reference fixtures of
tools/make_ref_color_aug_golden.py and the cfg a fixture case was recorded under."""
import contextlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_color_aug.npz")

# max |restatement - reference clip| over every element of every fixture case, measured on the CPU by
# test_restatement_matches_the_reference (which prints it per case): 7.153e-07 = 3 * 2^-22, three float32 ulps of an
# output in [2, 4) (|output| goes up to 3.7; the lighting-only cases differ by nothing).  The gate is 4 x the measured value ("Colour
# augmentation").
MEASURED_MAX_ABS_DIFF = 7.153e-07
GATE = 4 * MEASURED_MAX_ABS_DIFF


def load():
    z = np.load(GOLDEN)
    meta = json.loads(bytes(z["meta"]).decode())
    cases = []
    for k, info in enumerate(meta["cases"]):
        cases.append(dict(info, k=k, frames=z["frames_" + info["shape"]], boxes_in=z["case%d_boxes_in" % k],
                          boxes_out=z["case%d_boxes_out" % k], clip=z["case%d_clip" % k]))
    return meta, cases


@contextlib.contextmanager
def case_cfg(meta, use_bgr=False, pca_only=None, color=True):
    """the product cfg with the switches of a fixture case; everything is put back afterwards.  pca_only None leaves
    TRAIN.PCA_JITTER_ONLY undefined, as the reference's config.py does."""
    from vlfb.presets import load_preset
    from core.config import config as cfg
    load_preset("ava_r50_lfb_nl", ["NUM_GPUS", 1])
    assert "PCA_JITTER_ONLY" not in cfg.TRAIN
    assert [list(map(float, np.float32(cfg.DATA_MEAN))), list(map(float, np.float32(cfg.DATA_STD)))] == meta["mean_std"]
    cfg.TRAIN.USE_COLOR_AUGMENTATION = color
    cfg.TRAIN.JITTER_SCALES = list(meta["jitter"])
    cfg.MODEL.USE_BGR = use_bgr
    if pca_only is not None:
        cfg.TRAIN.PCA_JITTER_ONLY = pca_only
    try:
        yield cfg
    finally:
        load_preset("ava_r50_lfb_nl", ["NUM_GPUS", 1])
        assert cfg.TRAIN.USE_COLOR_AUGMENTATION is False and "PCA_JITTER_ONLY" not in cfg.TRAIN
