"""Run the REFERENCE's own train-time clip preprocessing with colour augmentation on and commit inputs + outputs.

TEST INFRASTRUCTURE ONLY.  Needs the reference checkout:

    python tools/make_ref_color_aug_golden.py        # writes tests/golden/ref_color_aug.npz

Called, from where it lies (the Caffe2 / OpenCV stubs of oracle/make_ref_aux_golden.py make the module importable; the
stand-in cv2.resize is oracle.preprocess.resize_u8):
  lib/datasets/data_input_helper.py   images_and_boxes_preprocessing (:70-139) with TRAIN.USE_COLOR_AUGMENTATION on, so
                                      color_augmentation_list (:142-151) and, in lib/datasets/image_processor.py,
                                      color_jitter_list / brightness_list / contrast_list / saturation_list (:286-336)
                                      and lighting_list (:253-269) run on the cropped clip
The reference reads cfg.TRAIN.PCA_JITTER_ONLY, which its config.py does not define: the generator sets it on the
reference's cfg before every call (False for the jitter cases, True for the lighting-only cases).

Per case the file holds the seed given to np.random.seed, the switches, the boxes in and out, the clip the reference
returned (float32 (3, T, crop, crop)) and ONE np.random.uniform() drawn right after the call, which pins how many draws
of which kind the call consumed.  The frames are shared per orientation: three frames of clearly different brightness
(a clip-wide mean in place of the per-frame mean of the contrast op would show).  The generator watches np.random while
the reference runs (which permutation it drew, whether it flipped) only to choose and label the cases: it loops over
seeds until the six op orders, flip on and off and both orientations are covered, and asserts that coverage.
"""
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "ref_color_aug.npz")
sys.path.insert(0, ROOT)

CROP, JITTER, T = 24, [32, 48], 3
SHAPES = {"wide": (30, 44), "tall": (44, 30)}


def make_frames(rng, h, w):
    """blocky content (3 x 3 blocks, so edges fall off every grid) at 30 % / 65 % / 100 % brightness"""
    out = []
    for gain in (0.3, 0.65, 1.0):
        base = rng.randint(0, 256, (h // 3 + 1, w // 3 + 1, 3))
        img = np.repeat(np.repeat(base, 3, axis=0), 3, axis=1)[:h, :w]
        out.append(np.floor(img * gain).astype(np.uint8))
    return np.stack(out)


class Watch(object):
    """records np.random.permutation results and argument-less np.random.uniform() draws while it is installed"""

    def __init__(self):
        self.perms, self.flips = [], []

    def __enter__(self):
        self._perm, self._uni = np.random.permutation, np.random.uniform

        def permutation(x):
            r = self._perm(x)
            self.perms.append([int(v) for v in r])
            return r

        def uniform(*a, **k):
            r = self._uni(*a, **k)
            if not a and not k:
                self.flips.append(bool(r < 0.5))
            return r
        np.random.permutation, np.random.uniform = permutation, uniform
        return self

    def __exit__(self, *exc):
        np.random.permutation, np.random.uniform = self._perm, self._uni


def main():
    from oracle.make_ref_aux_golden import install_stubs
    config, _ = install_stubs()
    import datasets.data_input_helper as dih                     # the reference's (install_stubs put its lib/ on the path)
    assert os.path.realpath(dih.__file__).startswith(REF), dih.__file__
    cfg = config.config

    rng = np.random.RandomState(20240915)
    arrays = {"frames_" + k: make_frames(rng, h, w) for k, (h, w) in SHAPES.items()}
    for k in SHAPES:                                             # clearly different brightness per frame
        m = arrays["frames_" + k].reshape(T, -1).mean(axis=1)
        assert m[0] < 0.6 * m[1] and m[1] < 0.8 * m[2], m

    def run(seed, shape, pca_only, use_bgr):
        config.cfg_from_list(["TRAIN.USE_COLOR_AUGMENTATION", "True", "TRAIN.JITTER_SCALES", str(JITTER),
                              "MODEL.USE_BGR", str(use_bgr)])
        cfg.TRAIN.PCA_JITTER_ONLY = pca_only
        brng = np.random.RandomState(1000 + seed)
        b = brng.uniform(0, 1, (3, 4))
        boxes = np.stack([np.minimum(b[:, 0], b[:, 2]), np.minimum(b[:, 1], b[:, 3]),
                          np.maximum(b[:, 0], b[:, 2]) + 0.05, np.maximum(b[:, 1], b[:, 3]) + 0.05], 1)
        frames = arrays["frames_" + shape]
        np.random.seed(seed)
        with Watch() as w:
            clip, out_boxes = dih.images_and_boxes_preprocessing([f.copy() for f in frames], 1, CROP, 1, boxes=boxes.copy())
        nxt = float(np.random.uniform())
        clip = np.ascontiguousarray(clip)
        assert clip.shape == (3, T, CROP, CROP) and len(w.flips) == 1 and len(w.perms) == (0 if pca_only else 1)
        info = {"seed": seed, "shape": shape, "pca_only": pca_only, "use_bgr": use_bgr, "flip": w.flips[0],
                "order": w.perms[0] if w.perms else [], "next_uniform": nxt, "ref_clip_dtype": str(clip.dtype)}
        return info, boxes, clip.astype(np.float32), np.asarray(out_boxes, np.float64)

    chosen = []
    seen_orders, seen_flip_shape = set(), set()
    for seed in range(200):                                      # jitter + lighting: first seed of every op order, then
        shape = "wide" if seed % 2 == 0 else "tall"              # seeds that add a missing (flip, orientation) pair
        info, boxes, clip, out_boxes = run(seed, shape, False, use_bgr=(len(chosen) == 2))
        key_o, key_f = tuple(info["order"]), (info["flip"], shape)
        if key_o not in seen_orders or (len(seen_orders) == 6 and key_f not in seen_flip_shape):
            seen_orders.add(key_o)
            seen_flip_shape.add(key_f)
            chosen.append((info, boxes, clip, out_boxes))
        if len(seen_orders) == 6 and len(seen_flip_shape) == 4:
            break
    for seed, shape, use_bgr in ((300, "wide", False), (301, "tall", True)):      # lighting only
        chosen.append(run(seed, shape, True, use_bgr))

    infos = [c[0] for c in chosen]
    jit = [i for i in infos if not i["pca_only"]]
    assert {tuple(i["order"]) for i in jit} == {(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)}
    assert {(i["flip"], i["shape"]) for i in jit} == {(f, s) for f in (True, False) for s in SHAPES}
    assert any(i["pca_only"] for i in infos) and any(i["use_bgr"] for i in jit) and len(infos) <= 12
    for k, (info, boxes, clip, out_boxes) in enumerate(chosen):
        arrays["case%d_boxes_in" % k], arrays["case%d_boxes_out" % k], arrays["case%d_clip" % k] = boxes, out_boxes, clip
    meta = {"generator": "tools/make_ref_color_aug_golden.py", "numpy": np.__version__, "crop": CROP, "jitter": JITTER,
            "split": 1, "shift": 1, "mean_std": [list(map(float, dih.DATA_MEAN)), list(map(float, dih.DATA_STD))],
            "cases": infos}
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    with open(OUT, "wb") as f:
        f.write(buf.getvalue())
    print("wrote %s: %d arrays, %d bytes" % (os.path.normpath(OUT), len(arrays), os.path.getsize(OUT)))
    print(json.dumps(infos, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
