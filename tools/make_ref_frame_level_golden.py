"""Run the REFERENCE's own frame-level dataset index arithmetic on tiny synthetic lists and commit inputs + outputs.

TEST INFRASTRUCTURE ONLY.  Needs the reference checkout:

    python tools/make_ref_frame_level_golden.py        # writes tests/golden/ref_frame_level.json.gz

Called, from where they lie (the Caffe2 / OpenCV stubs of oracle/make_ref_aux_golden.py make the modules importable):
  lib/datasets/dataset_helper.py       load_image_lists (both forms), get_sequence
  lib/datasets/charades.py             sample_train_idx, sample_center_of_segments, aggregate_labels, get_lfb_frames,
                                       CharadesDataset.get_db_size / get_minibatch_info (train, test, lfb_infer_only)
  lib/datasets/charades_data_input.py  construct_label_array
  lib/datasets/epic.py                 sec_to_frame, frame_to_sec, time_to_sec, get_sequence, load_annotations,
                                       get_annotations_for_lfb_frames, filename_to_frame_id,
                                       EpicDataset.get_db_size / get_minibatch_info (test, lfb_infer_only)
The reference is Python 2: it assigns into `range(...)`, keeps the result of `map`, and reads the csv from a file opened
'rb'.  List-returning `range` / `map` and a text-mode `open` are put into those modules' globals here; the files are not
edited.  The output holds data only: the text of the synthetic input files, the settings, the seeds and what the functions
returned.
"""
import builtins
import copy
import gzip
import json
import os
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "ref_frame_level.json.gz")
sys.path.insert(0, ROOT)


def py2_globals(module):
    module.range = lambda *a: list(builtins.range(*a))
    module.map = lambda *a: list(builtins.map(*a))
    module.open = lambda name, mode="r": builtins.open(name, "r", newline="") if mode == "rb" else builtins.open(name, mode)


def plain(x):
    """tuples -> lists, NumPy scalars / arrays -> Python; dictionaries -> [[key, value], ...] in iteration order"""
    if isinstance(x, dict):
        return [[plain(k), plain(v)] for k, v in x.items()]
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, np.generic):
        return x.item()
    if isinstance(x, bytes):
        return x.decode()
    return x


def frame_list_text(videos, labels_of):
    """a frame list in the reference's format; videos = [(name, frames)], labels_of(video index, frame) -> label list"""
    lines = ["original_vido_id video_id frame_id path labels"]
    for vi, (name, n) in enumerate(videos):
        for f in range(n):
            lines.append('%s %d %d %s/%s-%06d.jpg "%s"' % (name, vi, f, name, name, f + 1, ",".join(str(l) for l in labels_of(vi, f))))
    return "\n".join(lines) + "\n"


def main():
    from oracle.make_ref_aux_golden import install_stubs
    config, _ = install_stubs()
    cfg = config.config

    def snap(d):
        return {k: snap(v) if isinstance(v, dict) else copy.deepcopy(v) for k, v in d.items()}
    defaults = snap(cfg)

    import datasets.dataset_helper as H              # the reference's (install_stubs put its lib/ on the path)
    import datasets.charades as CH
    import datasets.charades_data_input as CHI
    import datasets.epic as EP
    for m in (H, CH, CHI, EP):
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
    out = {"generator": "tools/make_ref_frame_level_golden.py", "python": sys.version.split()[0], "numpy": np.__version__}

    # ---- dataset_helper.get_sequence: clamped at the front, at the back, at both ends, not at all -----------------------
    cases = [[2, 8, 4, 40], [38, 8, 4, 40], [3, 16, 2, 7], [20, 8, 4, 40], [0, 4, 1, 1], [59, 64, 4, 60], [11, 8, 4, 60],
             [5, 3, 2, 10]]
    out["get_sequence"] = [[c, plain(H.get_sequence(*c))] for c in cases]

    # ---- charades: segment centres (exact halves: 10 frames in 10 segments), train centres -----------------------------
    cases = [[s, n, k, 8] for n, k in ((10, 10), (5, 2), (37, 3), (100, 10), (7, 2), (25, 10)) for s in range(k)]
    out["center_of_segments"] = [[c, plain(CH.sample_center_of_segments(*c))] for c in cases]
    rows = []
    for seed in range(6):
        for num_frames, seq_len in ((10, 16), (16, 16), (17, 16), (100, 16), (61, 32), (31, 32)):
            random.seed(seed)
            rows.append([seed, num_frames, seq_len, CH.sample_train_idx(num_frames, seq_len)])
    out["train_idx"] = rows
    lists = [[[1, 2], [], [2, 5]], [[]], [], [[7], [7], [3, 1, 7]]]
    out["aggregate_labels"] = [[l, plain(CH.aggregate_labels(l))] for l in lists]

    # ---- Charades frame lists, both load_image_lists forms, the three walks of CharadesDataset -------------------------
    load("charades_r50_lfb_nl", ["NUM_GPUS", 1, "LFB.ENABLED", False, "TRAIN.BATCH_SIZE", 4, "TEST.BATCH_SIZE", 4,
                                 "TRAIN.VIDEO_LENGTH", 4, "TRAIN.SAMPLE_RATE", 4, "TEST.VIDEO_LENGTH", 4, "TEST.SAMPLE_RATE", 4,
                                 "MODEL.NUM_CLASSES", 12])
    cfg.DATADIR = "frames"
    cfg.CHARADES.FRAME_LIST_DIR = tmp
    cfg.CHARADES.TRAIN_LISTS = ["ch_train_a.csv", "ch_train_b.csv"]
    cfg.CHARADES.TEST_LISTS = ["ch_val.csv"]
    cfg.CHARADES.NUM_TEST_CLIPS = 6
    rng = np.random.RandomState(20241018)

    def random_labels(n_videos, n_frames):
        table = [[sorted(rng.choice(12, rng.randint(0, 4), replace=False).tolist()) for _ in range(n_frames[v])]
                 for v in range(n_videos)]
        return lambda v, f: table[v][f]
    train_a = [("AAA11", 60), ("BBB22", 9)]
    train_b = [("CCC33", 37)]
    val = [("VAL01", 50), ("VAL02", 13)]
    files = {
        "ch_train_a.csv": frame_list_text(train_a, random_labels(2, [60, 9])),
        "ch_train_b.csv": frame_list_text(train_b, random_labels(1, [37])),
        "ch_val.csv": frame_list_text(val, random_labels(2, [50, 13])),
    }
    for name, text in files.items():
        with open(os.path.join(tmp, name), "w") as f:
            f.write(text)
    out["charades"] = {"files": files, "datadir": "frames", "fps": cfg.CHARADES.FPS,
                       "lfb_clips_per_second": cfg.CHARADES.LFB_CLIPS_PER_SECOND, "num_test_clips": 6, "num_gpus": 1,
                       "batch_size": 4, "video_length": 4, "sample_rate": 4, "num_classes": 12,
                       "train_lists": ["ch_train_a.csv", "ch_train_b.csv"], "test_lists": ["ch_val.csv"]}
    paths = [os.path.join(tmp, n) for n in cfg.CHARADES.TRAIN_LISTS]
    out["charades"]["image_lists"] = plain(H.load_image_lists(paths))
    out["charades"]["image_lists_dict"] = plain(H.load_image_lists(paths, return_dict=True))

    def info(ds, indices):
        image_paths, labels, split_list, shifts, lfb = ds.get_minibatch_info(indices)
        assert lfb == []
        return {"image_paths": plain(image_paths), "labels": plain(labels), "split_list": plain(split_list),
                "shifts": plain(shifts)}

    walks = []
    ds = CH.CharadesDataset("train", False)
    for seed, indices in ((0, [0, 1, 2, 3]), (1, [5, 1, 0, 4]), (2, [2, 0])):                # (a short last batch)
        random.seed(seed)
        walks.append({"split": "train", "lfb_infer_only": False, "seed": seed, "indices": indices, "db_size": ds.get_db_size(),
                      "info": info(ds, list(indices))})
    ds = CH.CharadesDataset("test", False)
    size = ds.get_db_size()
    for lo in range(0, size, 4):
        indices = list(range(lo, min(lo + 4, size)))
        walks.append({"split": "test", "lfb_infer_only": False, "seed": None, "indices": indices, "db_size": size,
                      "info": info(ds, np.array(indices))})
    walks.append({"split": "test", "lfb_infer_only": False, "seed": None, "indices": [9], "db_size": size, "info": info(ds, [9])})
    ds = CH.CharadesDataset("test", True)
    size = ds.get_db_size()
    out["charades"]["lfb_frames"] = plain(CH.get_lfb_frames(ds._image_paths))
    for lo in range(0, size, 4):
        indices = list(range(lo, min(lo + 4, size)))
        walks.append({"split": "test", "lfb_infer_only": True, "seed": None, "indices": indices, "db_size": size,
                      "info": info(ds, list(indices))})
    cfg.GET_TRAIN_LFB = True
    ds = CH.CharadesDataset("test", True)
    size = ds.get_db_size()
    walks.append({"split": "test", "lfb_infer_only": True, "get_train_lfb": True, "seed": None, "indices": [0, size - 1],
                  "db_size": size, "info": info(ds, [0, size - 1])})
    cfg.GET_TRAIN_LFB = False
    out["charades"]["walks"] = walks
    label_lists = [[], [3], [0, 11, 5], [2, 2, 7]]
    out["charades"]["label_arrays"] = [[l, plain(CHI.construct_label_array(l))] for l in label_lists]

    # ---- EPIC: time helpers, sequences, the csv, the bank-pass annotations, EpicDataset in test ------------------------
    load("epic_verb_r50_lfb_nl", ["NUM_GPUS", 1, "LFB.ENABLED", False, "TRAIN.BATCH_SIZE", 4, "TEST.BATCH_SIZE", 4,
                                  "TRAIN.VIDEO_LENGTH", 4, "TRAIN.SAMPLE_RATE", 2, "TEST.VIDEO_LENGTH", 4, "TEST.SAMPLE_RATE", 2])
    ep = {"fps": cfg.EPIC.FPS, "verb_lfb_clips_per_second": cfg.EPIC.VERB_LFB_CLIPS_PER_SECOND, "class_type": cfg.EPIC.CLASS_TYPE,
          "num_gpus": 1, "batch_size": 4, "video_length": 4, "sample_rate": 2, "datadir": "frames"}
    ep["sec_to_frame"] = [[s, EP.sec_to_frame(s)] for s in (0, 0.25, 1.0 / 60, 0.05, 2.5, 130.99, 3.0 / 20)]
    ep["frame_to_sec"] = [[f, EP.frame_to_sec(f)] for f in (0, 14, 15, 16, 44, 45, 46, 75, 3929)]
    ep["time_to_sec"] = [[t, EP.time_to_sec(t)] for t in ("00:00:00.00", "00:02:10.99", "01:00:03.5", "00:59:59.99")]
    ep["filename_to_frame_id"] = [[p, EP.filename_to_frame_id(p)] for p in ("frames/P01_01/P01_01-000031.jpg", "x/000900.png")]
    rows = []
    for seed in range(4):
        for c in ([10, 50, 4, 2, 200], [0, 3, 8, 2, 200], [190, 199, 8, 4, 200], [5, 5, 4, 2, 3]):
            random.seed(seed)
            seq, center = EP.get_sequence(c[0], c[1], c[2], c[3], c[4], True)
            rows.append({"seed": seed, "args": c, "is_train": True, "seq": plain(seq), "center": center})
    for c in ([10, 50, 4, 2, 200], [0, 3, 8, 2, 200], [190, 199, 8, 4, 200], [5, 5, 4, 2, 3], [7, 10, 4, 2, 200]):
        seq, center = EP.get_sequence(c[0], c[1], c[2], c[3], c[4], False)
        rows.append({"seed": None, "args": c, "is_train": False, "seq": plain(seq), "center": center})
    ep["get_sequence"] = rows

    ep_train = [("P01_01", 70), ("P25_03", 40)]
    ep_val = [("P26_02", 95), ("P31_01", 31)]
    ep["files"] = {"ep_train.csv": frame_list_text(ep_train, lambda v, f: []), "ep_val.csv": frame_list_text(ep_val, lambda v, f: [])}
    header = ("uid,participant_id,video_id,narration,start_timestamp,stop_timestamp,start_frame,stop_frame,verb,verb_class,"
              "noun,noun_class,all_nouns,all_noun_classes")
    ann = [
        (0, "P01", "P01_01", "open door", "00:00:00.14", "00:00:01.37", 8, 202, "open", 2, "door", 8, "['door']", "[8]"),
        (1, "P01", "P01_01", "take cup, then plate", "00:00:01.50", "00:00:02.20", 90, 132, "take", 0, "cup", 13, "['cup', 'plate']", "[13, 2]"),
        (2, "P25", "P25_03", "wash pan", "00:00:00.00", "00:00:00.90", 0, 54, "wash", 4, "pan", 5, "['pan']", "[5]"),
        (3, "P26", "P26_02", "close fridge", "00:00:00.51", "00:00:01.49", 30, 89, "close", 3, "fridge", 12, "['fridge']", "[12]"),
        (4, "P26", "P26_02", "put knife, fork", "00:00:02.40", "00:00:03.10", 144, 186, "put", 1, "knife", 4, "['knife', 'fork']", "[4, 14]"),
        (5, "P31", "P31_01", "cut onion", "00:00:00.05", "00:00:00.95", 3, 57, "cut", 7, "onion", 17, "['onion']", "[17]"),
    ]
    import csv
    import io
    buf = io.StringIO()
    buf.write(header + "\r\n")
    w = csv.writer(buf)
    for row in ann:
        w.writerow(row)
    ep["files"]["ep_annotations.csv"] = buf.getvalue()
    for name, text in ep["files"].items():
        with builtins.open(os.path.join(tmp, name), "w", newline="") as f:
            f.write(text)
    cfg.DATADIR = "frames"
    cfg.EPIC.FRAME_LIST_DIR = tmp
    cfg.EPIC.ANNOTATION_DIR = tmp
    cfg.EPIC.ANNOTATIONS = "ep_annotations.csv"
    cfg.EPIC.TRAIN_LISTS = ["ep_train.csv"]
    cfg.EPIC.TEST_LISTS = ["ep_val.csv"]
    cfg.TRAIN.DATASET_SIZE = 3
    cfg.TEST.DATASET_SIZE = 3
    ep["train_lists"], ep["test_lists"], ep["annotations"] = ["ep_train.csv"], ["ep_val.csv"], "ep_annotations.csv"
    ep["load_annotations_train"] = plain(EP.load_annotations(True))
    ep["load_annotations_test"] = plain(EP.load_annotations(False))
    val_paths = H.load_image_lists([os.path.join(tmp, "ep_val.csv")], return_dict=True)
    ep["image_lists_dict"] = plain(val_paths)
    ep["lfb_annotations"] = plain(EP.get_annotations_for_lfb_frames(val_paths[0]))
    walks = []
    for lfb_infer_only, shift in ((False, None), (False, 2), (True, None)):
        ds = EP.EpicDataset("test", lfb_infer_only, shift=shift)
        size = ds.get_db_size()
        for indices in ([0, 1, 2][:size], [size - 1]):
            walks.append({"split": "test", "lfb_infer_only": lfb_infer_only, "shift": shift, "indices": indices, "db_size": size,
                          "info": info(ds, list(indices))})
    ep["walks"] = walks
    out["epic"] = ep

    with open(OUT, "wb") as raw:
        with gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as f:
            f.write(json.dumps(out, sort_keys=True).encode())
    print("wrote %s: %d bytes" % (os.path.normpath(OUT), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
