"""Host side of AVA: datasets.ava against what the REFERENCE's own functions returned (tests/golden/ref_ava_index.json.gz,
tools/make_ref_ava_index_golden.py) -- integers, lists and box texts, compared exactly -- and the per-clip draw helper that
datasets.ava and vlfb.lfb_bank.reference_draw_table share."""
import contextlib
import gzip
import json
import os

import numpy as np
import pytest

import clip_loader_cases as cases

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "ref_ava_index.json.gz")
with gzip.open(GOLDEN, "rb") as _f:
    G = json.loads(_f.read().decode())
S = G["settings"]
BANK_BASE = 900             # first second of the fixture's tiny bank (one cell lies before AVA's first valid second)


def test_the_fixture_is_small_and_reference_executed():
    assert G["generator"] == "tools/make_ref_ava_index_golden.py"
    assert os.path.getsize(GOLDEN) < 64 * 1024


def plain(x):
    """as the generator's: tuples -> lists, dictionaries -> [[key, value], ...] in iteration order"""
    if isinstance(x, dict):
        return [[plain(k), plain(v)] for k, v in x.items()]
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, np.generic):
        return x.item()
    return x


@contextlib.contextmanager
def ava_cfg(tmp_path, full_eval=False):
    """the product cfg with the settings the fixture was recorded under; the input files written to tmp_path"""
    from vlfb.presets import load_preset
    from core.config import config as cfg
    load_preset("ava_r50_lfb_nl", ["NUM_GPUS", S["num_gpus"], "TRAIN.BATCH_SIZE", S["batch_size"], "TEST.BATCH_SIZE", S["batch_size"],
                                   "TRAIN.VIDEO_LENGTH", S["video_length"], "TEST.VIDEO_LENGTH", S["video_length"],
                                   "TRAIN.SAMPLE_RATE", S["sample_rate"], "TEST.SAMPLE_RATE", S["sample_rate"],
                                   "LFB.LFB_DIM", S["lfb_dim"], "LFB.WINDOW_SIZE", S["window_size"],
                                   "AVA.LFB_MAX_NUM_FEAT_PER_STEP", S["max_num_feat_per_step"]])
    cfg.DATADIR = S["datadir"]
    a = cfg.AVA
    a.FRAME_LIST_DIR = a.ANNOTATION_DIR = str(tmp_path)
    a.TRAIN_LISTS, a.TEST_LISTS = S["train_lists"], S["test_lists"]
    a.TRAIN_BOX_LISTS, a.TEST_BOX_LISTS = S["train_box_lists"], S["test_box_lists"]
    a.TRAIN_LFB_BOX_LISTS, a.TEST_LFB_BOX_LISTS = S["train_lfb_box_lists"], S["test_lfb_box_lists"]
    a.FULL_EVAL, a.DETECTION_SCORE_THRESH = full_eval, S["detection_score_thresh"]
    a.LFB_DETECTION_SCORE_THRESH = S["lfb_detection_score_thresh"]
    for name, text in G["files"].items():
        with open(os.path.join(str(tmp_path), name), "w") as f:
            f.write(text)
    try:
        yield cfg
    finally:
        load_preset(*cases.RESET)


def test_constants_and_sec_to_frame(tmp_path):
    from datasets import ava
    with ava_cfg(tmp_path):
        assert [ava.AVA_VALID_FRAMES[0], ava.AVA_VALID_FRAMES[-1] + 1] == G["valid_frames"] == [902, 1799]
        assert ava.AVA_VALID_FRAMES == range(902, 1799) and ava.CENTER_CROP_INDEX == G["center_crop_index"] == 1
        for sec, want in G["sec_to_frame"]:
            assert ava.sec_to_frame(sec) == want


def test_load_boxes_and_labels_keyframes_and_box_counts(tmp_path):
    from datasets import ava
    order = [v for v, _ in G["videos"]]
    seen = set()
    with ava_cfg(tmp_path):
        for e in G["loads"]:
            ret = ava.load_boxes_and_labels([os.path.join(str(tmp_path), n) for n in e["filenames"]], e["is_train"],
                                            e["detect_thresh"], e["full_eval"])
            assert list(ret) == e["videos"]                                        # first appearance in the files
            for secs in ret.values():
                assert list(secs) == list(ava.AVA_VALID_FRAMES)                      # every valid second, in order
            got = [[v, s, plain(b)] for v, secs in ret.items() for s, b in secs.items() if len(b)]
            assert got == e["nonempty"]                                              # boxes by text, in first-appearance order
            seen.add(len(ret))
            if "keyframe_indices" in e:
                as_list = [ret[v] for v in order]
                keyframes = ava.get_keyframe_indices(as_list)
                assert plain(keyframes) == e["keyframe_indices"]
                assert ava.get_num_boxes_used(keyframes, as_list) == e["num_boxes_used"]
    assert seen == {2, 3}            # one load loses a video whose only rows are filtered out of the non-full evaluation
    texts = [b for e in G["loads"] for _, _, boxes in e["nonempty"] for b in boxes]
    assert any(len(b[1]) > 1 for b in texts) and any(-1 in b[1] for b in texts)      # several labels; an empty label


def test_construct_label_array(tmp_path):
    from datasets import ava
    with ava_cfg(tmp_path):
        for labels, want in G["label_arrays"]:
            got = ava.construct_label_array(labels)
            assert got.dtype == np.int32 and got.shape == (S["num_classes"],) and got.tolist() == want
            assert np.array_equal(ava.construct_label_array(labels, 80), got)
        with pytest.raises(AssertionError):
            ava.construct_label_array([0])                                           # labels are 1-based


def _bank_counts():
    fill = G["bank"]["fill"]
    counts = np.zeros((len(G["videos"]), max(s for _, s, _ in fill) - BANK_BASE + 1), dtype=np.int32)
    for v, s, n in fill:
        counts[v, s - BANK_BASE] = n
    return counts


def _reference_slots(arr, sec):
    """the reference's sampled (window * K, dim) bank of a clip, whose features are [sec, slot, video, 1] -> slot table"""
    W, K = S["window_size"], S["max_num_feat_per_step"]
    arr = np.asarray(arr, dtype=np.float64).reshape(W, K, S["lfb_dim"])
    table = np.full((W, K), -1, dtype=np.int32)
    for j in range(W):
        for k in range(K):
            if arr[j, k, 3] == 1:
                assert arr[j, k, 0] == sec - W // 2 + j
                table[j, k] = int(arr[j, k, 1])
            else:
                assert not arr[j, k].any()
    return table


def test_every_walk_of_the_reference_dataset(tmp_path):
    from datasets import ava, dataset_helper
    kinds, rng, padded, drew = set(), None, 0, 0
    counts = _bank_counts()
    for w in G["walks"]:
        with ava_cfg(tmp_path, w["full_eval"]) as cfg:
            index = ava.AvaIndex.from_cfg(w["split"], w["lfb_infer_only"], w["shift"], w["get_train_lfb"])
            image_paths = dataset_helper.load_image_lists([os.path.join(str(tmp_path), "frames.csv")])[0]
            assert index.get_db_size() == w["db_size"] and plain(index.keyframe_indices) == w["keyframe_indices"]
            assert index.num_boxes_used == w["num_boxes_used"]
            if w["seed"] is not None and w["first_of_seed"]:
                # the reference seeds np.random; a RandomState of the same seed is the same stream.  Use both forms.
                rng = np.random.RandomState(w["seed"]) if w["with_bank"] else np.random
                np.random.seed(w["seed"])
            use = rng if w["seed"] is not None else np.random
            indices = list(w["indices"])
            infos = index.get_minibatch_info(indices if len(kinds) % 2 else np.array(indices), use,
                                             counts if w["with_bank"] else None, BANK_BASE)
            assert indices == w["indices"]                                             # the caller's list is not extended
            ref = w["info"]
            assert len(infos) == cfg.TEST.BATCH_SIZE // cfg.NUM_GPUS == len(ref["secs"])
            assert [c.video for c in infos] == ref["video_indices"] and [c.sec for c in infos] == ref["secs"]
            assert [[image_paths[c.video][f] for f in c.seq] for c in infos] == ref["image_paths"]
            assert [[[b, l] for b, l in zip(c.boxes, c.labels)] for c in infos] == ref["labels"]
            assert [c.center for c in infos] == [ava.sec_to_frame(s) for s in ref["secs"]]
            assert ref["split_list"] == [index.split_num] * len(infos)
            if index.split_num:
                assert all(c.shift is None for c in infos)                             # train: the crop is drawn
            else:
                assert [c.shift for c in infos] == ref["shifts"]
            if w["with_bank"]:
                assert len(ref["lfb"]) == len(infos)
                for c, arr in zip(infos, ref["lfb"]):
                    want = _reference_slots(arr, c.sec)
                    assert c.lfb_slots.dtype == np.int32 and np.array_equal(c.lfb_slots, want)
                    drew += int((want >= 0).sum())
            else:
                assert ref["lfb"] == [] and all(c.lfb_slots is None for c in infos)
            if len(indices) < len(infos):
                padded += 1
                if w["split"] != "train":                                                # padded with indices[0]
                    assert all(c[:7] == infos[0][:7] for c in infos[len(indices):])
            kinds.add((w["split"], w["lfb_infer_only"], w["full_eval"], w["with_bank"], w["shift"], w["get_train_lfb"], w["seed"]))
    assert len(kinds) == 10 and padded >= 4 and drew > 50
    assert {k[6] for k in kinds} == {None, 0, 3, 7}             # (3: the test walk that samples a bank)


def test_the_index_takes_a_dictionary_or_a_list(tmp_path):
    from datasets import ava, dataset_helper
    with ava_cfg(tmp_path, True):
        paths, _, idx_to_name, _ = dataset_helper.load_image_lists([os.path.join(str(tmp_path), "frames.csv")])
        ret = ava.load_boxes_and_labels([os.path.join(str(tmp_path), "pred.csv")], False, 0.85, True)
        a = ava.AvaIndex(paths, idx_to_name, ret, "test", False)
        b = ava.AvaIndex([[None] * len(p) for p in paths], idx_to_name, [ret[idx_to_name[i]] for i in range(3)], "test", False)
        assert a.keyframe_indices == b.keyframe_indices and a.get_db_size() == 12
        assert (a.full_eval, a.detect_thresh) == (True, 0.85)
        c = ava.AvaIndex(paths, idx_to_name, ret, "test", True)
        assert (c.full_eval, c.detect_thresh) == (True, 0.9)


def test_minibatch_source_walks_in_order_and_marks_the_padding(tmp_path):
    from datasets import ava
    with ava_cfg(tmp_path) as cfg:
        index = ava.AvaIndex.from_cfg("test", True, shift=1)
        store = object()
        batches = list(ava.minibatch_source(index, store, np.random.RandomState(0)))
        size, n = index.get_db_size(), cfg.TEST.BATCH_SIZE
        assert size % n and len(batches) == -(-size // n)
        walked = []
        for it, (clips, boxes, labels, meta, _, shift) in enumerate(batches):
            assert len(clips) == len(boxes) == len(labels) == n and meta["iteration"] == it and shift == 1
            for k, (st, video, seq) in enumerate(clips):
                assert st is store and video == meta["videos"][k] and len(seq) == cfg.TEST.VIDEO_LENGTH
                assert boxes[k].shape == (len(labels[k]), 4) and labels[k].shape[1] == cfg.MODEL.NUM_CLASSES
                assert labels[k].dtype == np.int32
                if not meta["padded"][k]:
                    walked.append((video, meta["secs"][k]))
        assert walked == [(v, s) for v, s, _ in index.keyframe_indices]
        assert [m[3]["padded"] for m in batches][-1] == [False] * (size % n) + [True] * (n - size % n)
        train = ava.AvaIndex.from_cfg("train", False)
        it = ava.minibatch_source(train, store, np.random.RandomState(1), iterations=5)
        assert [m[3]["iteration"] for m in it] == [0, 1, 2, 3, 4]                      # train passes go on until told to stop


def _draw_table_before_the_helper(counts, vid, centre, clip_index, window, K, rng):
    """reference_draw_table as it was before its per-clip loop became reference_draw_clip"""
    rows = len(vid)
    ids = np.asarray(clip_index).astype(np.int64).reshape(-1)
    table = np.full((rows, int(window), int(K)), -1, dtype=np.int32)
    prev = None
    for r in range(rows):
        if prev is None or ids[r] != ids[prev]:
            t = np.full((int(window), int(K)), -1, dtype=np.int32)
            lower = int(centre[r]) - int(window) // 2
            for j in range(int(window)):
                si = lower + j
                n = int(counts[vid[r], si]) if (0 <= vid[r] < counts.shape[0] and 0 <= si < counts.shape[1]) else 0
                if n > 0:
                    used = min(n, int(K))
                    t[j, :used] = rng.choice(range(n), used, replace=False)
            cur = t
        table[r] = cur
        prev = r
    return table


def test_reference_draw_table_is_unchanged_by_the_shared_helper():
    from vlfb.lfb_bank import reference_draw_clip, reference_draw_table
    gen = np.random.default_rng(5)
    for trial in range(20):
        counts = gen.integers(0, 9, (4, 30)).astype(np.int32) * (gen.random((4, 30)) < 0.6)
        clips = int(gen.integers(1, 6))
        per_clip = gen.integers(1, 4, clips)
        clip_index = np.repeat(np.arange(clips), per_clip)
        vid = np.repeat(gen.integers(-1, 5, clips), per_clip)                          # videos outside the bank included
        centre = np.repeat(gen.integers(-3, 33, clips), per_clip)                     # windows that leave the range
        W, K = int(gen.integers(1, 9)), int(gen.integers(1, 6))
        got = reference_draw_table(counts, vid, centre, clip_index, W, K, np.random.RandomState(trial))
        want = _draw_table_before_the_helper(counts, vid, centre, clip_index, W, K, np.random.RandomState(trial))
        assert got.dtype == np.int32 and np.array_equal(got, want)
        rng = np.random.RandomState(trial)
        first = np.concatenate([[0], np.cumsum(per_clip)[:-1]])
        for c, r in enumerate(first):
            assert np.array_equal(reference_draw_clip(counts, vid[r], centre[r], W, K, rng), got[r])
