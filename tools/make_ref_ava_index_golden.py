"""Run the REFERENCE's own AVA dataset index on tiny synthetic lists and commit inputs + outputs.

TEST INFRASTRUCTURE ONLY.  Needs the reference checkout:

    python tools/make_ref_ava_index_golden.py        # writes tests/golden/ref_ava_index.json.gz

Called, from where they lie (the Caffe2 / OpenCV stubs of oracle/make_ref_aux_golden.py make the modules importable):
  lib/datasets/ava.py             sec_to_frame, load_boxes_and_labels, get_keyframe_indices, get_num_boxes_used,
                                  AvaDataset.get_db_size / get_minibatch_info (train with two seeds, test with FULL_EVAL on
                                  and off, lfb_infer_only for both banks, a shift; with and without a bank)
  lib/datasets/ava_data_input.py  construct_label_array
  lib/datasets/dataset_helper.py  load_image_lists, get_sequence (through AvaDataset)
The reference is Python 2: it keeps the result of `map` and of `dict.values()`.  A list-returning `map` / `range` is put into
the modules' globals here, `values()` results are listed when they are recorded; the files are not edited.  So the order of
the boxes of a second and of the seconds of a video is Python 3's dictionary order: first appearance.  The output holds
data only: the text of the synthetic input files, the settings, the seeds and what the functions returned.
"""
import builtins
import copy
import gzip
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "ref_ava_index.json.gz")
sys.path.insert(0, ROOT)

VALUES = type({}.values())


def py2_globals(module):
    module.range = lambda *a: list(builtins.range(*a))
    module.map = lambda *a: list(builtins.map(*a))


def plain(x):
    """tuples / dict views -> lists, NumPy scalars / arrays -> Python; dictionaries -> [[key, value], ...] in iteration order"""
    if isinstance(x, dict):
        return [[plain(k), plain(v)] for k, v in x.items()]
    if isinstance(x, (list, tuple, VALUES)):
        return [plain(v) for v in x]
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, np.generic):
        return x.item()
    return x


VIDEOS = [("VIDA", 500), ("VIDB", 470), ("VIDC", 290)]           # VIDC ends before its last keyframes: clamped clips

# 7 columns.  A box with several labels; the same box text in two seconds; an empty label; one box under two texts (0.100 /
# 0.1) in one second; VIDC only at seconds with sec % 4 != 0 (filtered out of the non-full evaluation altogether)
GT = """VIDA,902,0.1,0.2,0.5,0.8,12
VIDA,902,0.55,0.1,0.9,0.7,80
VIDA,902,0.1,0.2,0.5,0.8,17
VIDA,903,0.1,0.2,0.5,0.8,1
VIDA,904,0.3,0.3,0.6,0.6,
VIDA,905,0.2,0.2,0.4,0.9,5
VIDB,908,0.100,0.2,0.5,0.8,9
VIDB,908,0.1,0.2,0.5,0.8,10
VIDB,906,0.05,0.05,0.45,0.95,3
VIDB,908,0.100,0.2,0.5,0.8,11
VIDC,907,0.2,0.1,0.7,0.9,4
VIDC,909,0.25,0.15,0.75,0.95,
VIDC,909,0.25,0.15,0.75,0.95,7
"""
# 8 columns: scores above both thresholds (0.85 / 0.9), between them, at them, below both; seconds of all four residues
PRED = """VIDA,908,0.6,0.1,0.9,0.5,,0.95
VIDA,902,0.11,0.21,0.51,0.81,,0.95
VIDA,904,0.3,0.3,0.6,0.6,,0.87
VIDA,904,0.6,0.1,0.9,0.5,,0.5
VIDA,906,0.2,0.3,0.4,0.5,,0.9
VIDA,908,0.1,0.1,0.3,0.6,,0.92
VIDA,907,0.5,0.5,0.9,0.9,,0.85
VIDB,905,0.3,0.2,0.8,0.9,,0.99
VIDB,908,0.15,0.25,0.55,0.85,,0.86
VIDB,912,0.1,0.1,0.2,0.9,,0.97
VIDB,912,0.3,0.1,0.4,0.9,,0.91
VIDB,912,0.5,0.1,0.6,0.9,,0.93
VIDB,912,0.7,0.1,0.8,0.9,,0.84
VIDC,904,0.2,0.2,0.6,0.6,,0.96
VIDC,907,0.3,0.3,0.7,0.7,,0.88
VIDC,910,0.4,0.4,0.8,0.8,,0.94
VIDC,911,0.1,0.5,0.2,0.6,,0.2
VIDC,912,0.12,0.5,0.22,0.6,,0.899
"""


def frame_list_text():
    lines = ["original_vido_id video_id frame_id path labels"]
    for vi, (name, n) in enumerate(VIDEOS):
        for f in range(n):
            lines.append('%s %d %d %s/%s_%06d.jpg ""' % (name, vi, f, name, name, f + 1))
    return "\n".join(lines) + "\n"


def tiny_bank():
    """per video index {sec: [feature, ...]}, feature = [sec, slot, video, 1]: cells with fewer than K = 3 features, with
    more, and empty ones; windows of 6 around seconds 902 .. 912 leave the range on both sides"""
    fill = {0: {902: 1, 903: 5, 904: 3, 906: 2, 908: 4, 909: 1}, 1: {903: 4, 905: 2, 907: 7, 910: 3, 912: 1, 914: 2},
            2: {900: 2, 904: 6, 905: 1, 909: 3, 913: 5}}
    return [{sec: [np.array([sec, k, v, 1], dtype=np.float32) for k in range(n)] for sec, n in fill[v].items()} for v in range(3)], fill


def main():
    from oracle.make_ref_aux_golden import install_stubs
    config, _ = install_stubs()
    cfg = config.config

    def snap(d):
        return {k: snap(v) if isinstance(v, dict) else copy.deepcopy(v) for k, v in d.items()}
    defaults = snap(cfg)

    import datasets.ava as AV                        # the reference's (install_stubs put its lib/ on the path)
    import datasets.ava_data_input as AVI
    import datasets.dataset_helper as H
    for m in (AV, AVI, H):
        assert os.path.realpath(m.__file__).startswith(REF), m.__file__
        py2_globals(m)

    def load(name, overrides):
        def rec(dst, src):
            for k in list(dst.keys()):
                if k not in src:
                    del dst[k]
            for k, v in src.items():
                if isinstance(v, dict):
                    rec(dst[k], v)
                else:
                    dst[k] = copy.deepcopy(v)
        rec(cfg, defaults)
        config.cfg_from_file(os.path.join(REF, "configs", name + ".yaml"))
        config.cfg_from_list([str(o) for o in overrides])
        config.assert_and_infer_cfg()

    tmp = tempfile.mkdtemp()
    files = {"frames.csv": frame_list_text(), "gt.csv": GT, "pred.csv": PRED}
    for name, text in files.items():
        with open(os.path.join(tmp, name), "w") as f:
            f.write(text)

    settings = {"num_gpus": 1, "batch_size": 4, "video_length": 4, "sample_rate": 2, "fps": 30, "datadir": "frames",
                "detection_score_thresh": 0.85, "lfb_detection_score_thresh": 0.9, "num_classes": 80,
                "lfb_dim": 4, "window_size": 6, "max_num_feat_per_step": 3,
                "train_lists": ["frames.csv"], "test_lists": ["frames.csv"], "train_box_lists": ["gt.csv", "pred.csv"],
                "test_box_lists": ["pred.csv"], "train_lfb_box_lists": ["gt.csv", "pred.csv"], "test_lfb_box_lists": ["pred.csv"]}

    def configure(full_eval, lfb_enabled):
        load("ava_r50_lfb_nl", ["NUM_GPUS", 1, "TRAIN.BATCH_SIZE", 4, "TEST.BATCH_SIZE", 4, "TRAIN.VIDEO_LENGTH", 4,
                                "TRAIN.SAMPLE_RATE", 2, "TEST.VIDEO_LENGTH", 4, "TEST.SAMPLE_RATE", 2,
                                "LFB.ENABLED", lfb_enabled, "LFB.LFB_DIM", 4, "LFB.WINDOW_SIZE", 6,
                                "AVA.LFB_MAX_NUM_FEAT_PER_STEP", 3])
        cfg.DATADIR = "frames"
        cfg.AVA.FRAME_LIST_DIR = tmp
        cfg.AVA.ANNOTATION_DIR = tmp
        cfg.AVA.TRAIN_LISTS, cfg.AVA.TEST_LISTS = ["frames.csv"], ["frames.csv"]
        cfg.AVA.TRAIN_BOX_LISTS, cfg.AVA.TEST_BOX_LISTS = ["gt.csv", "pred.csv"], ["pred.csv"]
        cfg.AVA.TRAIN_LFB_BOX_LISTS, cfg.AVA.TEST_LFB_BOX_LISTS = ["gt.csv", "pred.csv"], ["pred.csv"]
        cfg.AVA.FULL_EVAL = full_eval                 # what the drivers set (train_net.py:107-108, test_net.py:59,101)
        cfg.AVA.DETECTION_SCORE_THRESH = 0.85
        cfg.AVA.LFB_DETECTION_SCORE_THRESH = 0.9
        cfg.GET_TRAIN_LFB = False

    configure(False, False)
    assert (cfg.AVA.FPS, cfg.MODEL.NUM_CLASSES) == (30, 80)
    out = {"generator": "tools/make_ref_ava_index_golden.py", "python": sys.version.split()[0], "numpy": np.__version__,
           "files": files, "settings": settings, "videos": [list(v) for v in VIDEOS],
           "valid_frames": [AV.AVA_VALID_FRAMES[0], AV.AVA_VALID_FRAMES[-1] + 1], "center_crop_index": AV.CENTER_CROP_INDEX}
    out["sec_to_frame"] = [[s, AV.sec_to_frame(s)] for s in (900, 901, 902, 1000, 1798)]

    # ---- load_boxes_and_labels / get_keyframe_indices / get_num_boxes_used ---------------------------------------------
    order = [v for v, _ in VIDEOS]
    loads = []
    for names, is_train, thresh, full_eval in ((["gt.csv", "pred.csv"], True, 0.85, False), (["gt.csv", "pred.csv"], True, 0.9, True),
                                               (["pred.csv"], False, 0.85, False), (["pred.csv"], False, 0.85, True),
                                               (["pred.csv"], False, 0.9, True), (["gt.csv"], False, 0.9, False),
                                               (["pred.csv", "gt.csv"], False, 0.0, True)):
        ret = AV.load_boxes_and_labels([os.path.join(tmp, n) for n in names], is_train, thresh, full_eval)
        for secs in ret.values():
            assert list(secs.keys()) == list(AV.AVA_VALID_FRAMES)
        entry = {"filenames": names, "is_train": is_train, "detect_thresh": thresh, "full_eval": full_eval,
                 "videos": list(ret.keys()),
                 "nonempty": [[v, s, plain(b)] for v, secs in ret.items() for s, b in secs.items() if len(b)]}
        if len(ret) == len(VIDEOS):
            as_list = [ret[v] for v in order]
            entry["keyframe_indices"] = plain(AV.get_keyframe_indices(as_list))
            entry["num_boxes_used"] = AV.get_num_boxes_used(AV.get_keyframe_indices(as_list), as_list)
        loads.append(entry)
    assert [len(e["videos"]) for e in loads].count(2) == 1, "one load loses VIDC altogether"
    out["loads"] = loads

    out["label_arrays"] = [[l, plain(AVI.construct_label_array(l))] for l in ([12, 17], [-1], [80, 1], [], [5, -1, 5])]

    # ---- AvaDataset ------------------------------------------------------------------------------------------------
    bank, fill = tiny_bank()
    out["bank"] = {"fill": [[v, s, n] for v in sorted(fill) for s, n in fill[v].items()], "feature": "[sec, slot, video, 1]"}

    def info(ds, indices):
        image_paths, labels, split_list, shifts, video_indices, secs, lfb = ds.get_minibatch_info(indices)
        return {"image_paths": plain(image_paths), "labels": plain(labels), "split_list": plain(split_list),
                "shifts": plain(shifts), "video_indices": plain(video_indices), "secs": plain(secs),
                "lfb": [np.asarray(x).tolist() for x in lfb]}

    walks = []

    def walk(split, lfb_infer_only, full_eval, with_bank, shift=None, get_train_lfb=False, seeds=(None,), batches=None):
        configure(full_eval, with_bank)
        cfg.GET_TRAIN_LFB = get_train_lfb
        ds = AV.AvaDataset(split, lfb_infer_only, shift=shift, lfb=bank if with_bank else None)
        size = ds.get_db_size()
        if batches is None:
            batches = [list(range(lo, min(lo + 4, size))) for lo in range(0, size, 4)]
        for seed in seeds:
            if seed is not None:
                np.random.seed(seed)
            for k, indices in enumerate(batches):
                arg = np.array(indices) if k % 2 else list(indices)          # both accepted forms
                walks.append({"split": split, "lfb_infer_only": lfb_infer_only, "full_eval": full_eval, "with_bank": with_bank,
                              "shift": shift, "get_train_lfb": get_train_lfb, "seed": seed, "first_of_seed": k == 0,
                              "indices": indices, "db_size": size, "keyframe_indices": plain(ds._keyframe_indices),
                              "num_boxes_used": ds._num_boxes_used, "info": info(ds, arg)})
        cfg.GET_TRAIN_LFB = False
        return size

    train_batches = [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]                       # (the last one is short: padded)
    walk("train", False, False, False, seeds=(0, 7), batches=train_batches)
    walk("train", False, False, True, seeds=(0, 7), batches=train_batches)
    sizes = [walk("test", False, True, False), walk("test", False, False, False), walk("test", False, True, True, seeds=(3,)),
             walk("test", False, True, False, shift=2), walk("test", True, False, False, shift=1),
             walk("test", True, False, False, shift=1, get_train_lfb=True)]
    assert any(s % 4 for s in sizes), sizes
    out["walks"] = walks

    with open(OUT, "wb") as raw:
        with gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as f:
            f.write(json.dumps(out, sort_keys=True).encode())
    print("wrote %s: %d bytes; db sizes %r" % (os.path.normpath(OUT), os.path.getsize(OUT), sizes))


if __name__ == "__main__":
    main()
