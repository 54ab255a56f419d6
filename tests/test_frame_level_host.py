"""Host side of the frame-level datasets: the index arithmetic of datasets.{dataset_helper,charades,epic} against what the
REFERENCE's own functions returned (tests/golden/ref_frame_level.json.gz, tools/make_ref_frame_level_golden.py) -- integers
and lists, compared exactly --, the bookkeeping of datasets.frame_store, and the bank query builders."""
import contextlib
import gzip
import json
import os
import random

import numpy as np
import pytest

import clip_loader_cases as cases

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "ref_frame_level.json.gz")
with gzip.open(GOLDEN, "rb") as _f:
    G = json.loads(_f.read().decode())


def test_the_fixture_is_small_and_reference_executed():
    assert G["generator"] == "tools/make_ref_frame_level_golden.py"
    assert os.path.getsize(GOLDEN) < 64 * 1024


@contextlib.contextmanager
def dataset_cfg(preset, g, tmp_path=None):
    """the product cfg with the settings the fixture was recorded under; frame lists written to tmp_path"""
    from vlfb.presets import load_preset
    from core.config import config as cfg
    load_preset(preset, ["NUM_GPUS", g["num_gpus"], "TRAIN.BATCH_SIZE", g["batch_size"], "TEST.BATCH_SIZE", g["batch_size"],
                         "TRAIN.VIDEO_LENGTH", g["video_length"], "TEST.VIDEO_LENGTH", g["video_length"],
                         "TRAIN.SAMPLE_RATE", g["sample_rate"], "TEST.SAMPLE_RATE", g["sample_rate"]])
    cfg.DATADIR = g["datadir"]
    if tmp_path is not None:
        for name, text in g["files"].items():
            with open(os.path.join(str(tmp_path), name), "w", newline="") as f:
                f.write(text)
    try:
        yield cfg
    finally:
        load_preset(*cases.RESET)


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


# ---- dataset_helper / charades ---------------------------------------------------------------------------------------

def test_get_sequence():
    from datasets import dataset_helper
    kinds = set()
    for args, want in G["get_sequence"]:
        got = dataset_helper.get_sequence(*args)
        assert got == want and isinstance(got, list), args
        ideal = list(range(args[0] - args[1], args[0] + args[1], args[2]))
        kinds.add((ideal[0] < 0, ideal[-1] >= args[3]))
    assert kinds == {(False, False), (True, False), (False, True), (True, True)}     # clamped at neither, either, both ends


def test_center_of_segments_rounds_halves_to_even():
    from datasets import charades
    for args, want in G["center_of_segments"]:
        got = charades.sample_center_of_segments(*args)
        assert got == want and isinstance(got, int), args
    halves = {tuple(a): w for a, w in G["center_of_segments"] if a[1] == 10 and a[2] == 10}
    assert [halves[(s, 10, 10, 8)] for s in range(4)] == [0, 2, 2, 4]             # 0.5, 1.5, 2.5, 3.5


def test_sample_train_idx_draws_what_random_randint_draws():
    from datasets import charades
    drawn = set()
    for seed, num_frames, seq_len, want in G["train_idx"]:
        rng = random.Random(seed)
        assert charades.sample_train_idx(num_frames, seq_len, rng) == want, (seed, num_frames, seq_len)
        random.seed(seed)                                                          # the default rng is the module, as the reference's
        assert charades.sample_train_idx(num_frames, seq_len) == want
        drawn.add(num_frames >= seq_len)
    assert drawn == {True, False}


def test_aggregate_labels_and_label_arrays():
    from datasets import charades
    for lists, want in G["aggregate_labels"]:
        assert charades.aggregate_labels(lists) == want
    with dataset_cfg("charades_r50_lfb_nl", G["charades"]) as cfg:
        cfg.MODEL.NUM_CLASSES = G["charades"]["num_classes"]
        for labels, want in G["charades"]["label_arrays"]:
            got = charades.construct_label_array(labels)
            assert got.dtype == np.int32 and got.tolist() == want
            assert charades.construct_label_array(labels, 12).tolist() == want


def test_load_image_lists_both_forms(tmp_path):
    from datasets import dataset_helper
    g = G["charades"]
    with dataset_cfg("charades_r50_lfb_nl", g, tmp_path):
        paths = [os.path.join(str(tmp_path), n) for n in g["train_lists"]]
        assert plain(dataset_helper.load_image_lists(paths)) == g["image_lists"]
        assert plain(dataset_helper.load_image_lists(paths, return_dict=True)) == g["image_lists_dict"]
        got = dataset_helper.load_image_lists(paths)
        assert isinstance(got[0], list) and len(got[0]) == 3 and got[3] == {"AAA11": 0, "BBB22": 1, "CCC33": 2}


def test_charades_index_walks(tmp_path):
    """CharadesIndex.get_minibatch_info against CharadesDataset.get_minibatch_info: train (seeded), test (2 videos x 6 test
    clips, with a short last batch padded with indices[0]) and lfb_infer_only"""
    from datasets import charades, dataset_helper
    g = G["charades"]
    with dataset_cfg("charades_r50_lfb_nl", g, tmp_path) as cfg:
        cfg.CHARADES.NUM_TEST_CLIPS = g["num_test_clips"]
        assert (cfg.CHARADES.FPS, cfg.CHARADES.LFB_CLIPS_PER_SECOND) == (g["fps"], g["lfb_clips_per_second"])
        lists = {"train": g["train_lists"], "test": g["test_lists"]}
        seen = set()
        for w in g["walks"]:
            which = "train" if (w["split"] == "train" or w.get("get_train_lfb")) else "test"
            image_paths, image_labels, _, _ = dataset_helper.load_image_lists(
                [os.path.join(str(tmp_path), n) for n in lists[which]])
            index = charades.CharadesIndex(image_paths, image_labels, w["split"], w["lfb_infer_only"])
            assert index.get_db_size() == w["db_size"]
            given = list(w["indices"])
            info = index.get_minibatch_info(np.array(given) if w["split"] == "test" else given,
                                            random.Random(w["seed"]) if w["seed"] is not None else random)
            assert given == w["indices"]                                           # the caller's list is not padded in place
            assert len(info) == g["batch_size"] == len(w["info"]["labels"])
            assert [[image_paths[c.video][f] for f in c.seq] for c in info] == w["info"]["image_paths"]
            assert [c.labels for c in info] == w["info"]["labels"]
            assert [c.shift for c in info] == w["info"]["shifts"]
            for c in info:
                assert len(c.seq) == g["video_length"]
                if not w["lfb_infer_only"] and w["split"] == "test":
                    assert c.labels == charades.aggregate_labels(image_labels[c.video])      # video-level labels outside train
            if w["lfb_infer_only"]:
                assert [(c.video, c.center) for c in info[:len(given)]] == [index.lfb_frames[i] for i in given]
            elif w["split"] == "test":
                V = len(image_paths)
                assert [(c.video, c.shift) for c in info[:len(given)]] == [(i % V, (i // V) % 3) for i in given]
            seen.add((w["split"], w["lfb_infer_only"], len(given) < g["batch_size"]))
        assert {("train", False, True), ("test", False, True), ("test", True, True), ("test", False, False)} <= seen
        image_paths, _, _, _ = dataset_helper.load_image_lists([os.path.join(str(tmp_path), n) for n in g["test_lists"]])
        assert plain(charades.get_lfb_frames(image_paths)) == g["lfb_frames"]


# ---- EPIC ----------------------------------------------------------------------------------------------------------------

def test_epic_time_helpers_and_sequences():
    from datasets import epic
    g = G["epic"]
    with dataset_cfg("epic_verb_r50_lfb_nl", g) as cfg:
        assert cfg.EPIC.FPS == g["fps"]
        for s, want in g["sec_to_frame"]:
            assert epic.sec_to_frame(s) == want
        for f, want in g["frame_to_sec"]:
            assert epic.frame_to_sec(f) == want
        for t, want in g["time_to_sec"]:
            assert epic.time_to_sec(t) == want
        for p, want in g["filename_to_frame_id"]:
            assert epic.filename_to_frame_id(p) == want
        modes = set()
        for row in g["get_sequence"]:
            a = row["args"]
            rng = random.Random(row["seed"]) if row["is_train"] else random
            seq, center = epic.get_sequence(a[0], a[1], a[2], a[3], a[4], row["is_train"], rng)
            assert (seq, center) == (row["seq"], row["center"]), row
            modes.add(row["is_train"])
        assert modes == {True, False}


def test_epic_annotations_and_index_walks(tmp_path):
    from datasets import dataset_helper, epic
    g = G["epic"]
    with dataset_cfg("epic_verb_r50_lfb_nl", g, tmp_path) as cfg:
        assert (cfg.EPIC.CLASS_TYPE, cfg.EPIC.VERB_LFB_CLIPS_PER_SECOND) == (g["class_type"], g["verb_lfb_clips_per_second"])
        csv_path = os.path.join(str(tmp_path), g["annotations"])
        train, test = epic.load_annotations(csv_path, True), epic.load_annotations(csv_path, False)
        assert plain(train) == g["load_annotations_train"] and plain(test) == g["load_annotations_test"]
        assert len(train) == 3 and len(test) == 3 and isinstance(train[0], tuple)
        lists = dataset_helper.load_image_lists([os.path.join(str(tmp_path), n) for n in g["test_lists"]], return_dict=True)
        assert plain(lists) == g["image_lists_dict"]
        image_paths = lists[0]
        assert plain(epic.get_annotations_for_lfb_frames(image_paths)) == g["lfb_annotations"]
        for w in g["walks"]:
            index = epic.EpicIndex(image_paths, None if w["lfb_infer_only"] else test, w["split"], w["lfb_infer_only"], w["shift"])
            assert index.get_db_size() == w["db_size"]
            info = index.get_minibatch_info(list(w["indices"]))
            assert len(info) == g["batch_size"]
            assert [[image_paths[c.video][f] for f in c.seq] for c in info] == w["info"]["image_paths"]
            assert [c.labels for c in info] == w["info"]["labels"]
            assert [c.shift for c in info] == w["info"]["shifts"]
        # train: the annotation and the centre come from the one rng, in that order
        index = epic.EpicIndex(dataset_helper.load_image_lists([os.path.join(str(tmp_path), n) for n in g["train_lists"]],
                                                               return_dict=True)[0], train, "train", False)
        a, b = index.get_minibatch_info([0, 1, 2, 3], random.Random(5)), index.get_minibatch_info([3, 2, 1, 0], random.Random(5))
        assert a == b and all(c.shift is None for c in a)
        rng = random.Random(5)
        ann = train[rng.randrange(3)]
        assert (a[0].video, a[0].center, a[0].labels) == (ann[1], rng.randint(ann[2], ann[3]), ann[4])


# ---- the frame store's bookkeeping -------------------------------------------------------------------------------------

def test_store_fifo_eviction():
    from datasets.frame_store import StoreIndex
    ix = StoreIndex(4)
    slots, missing = ix.assign("v", [0, 1, 2, 3])
    assert slots == [0, 1, 2, 3] and missing == [(0, 0), (1, 1), (2, 2), (3, 3)]
    ix.release()
    slots, missing = ix.assign("v", [0, 0, 3])                      # hits: nothing to upload, and a hit does not renew
    assert slots == [0, 0, 3] and missing == []
    ix.release()
    slots, missing = ix.assign("v", [4, 5])                         # the two frames resident longest go: 0, then 1
    assert missing == [(4, 0), (5, 1)] and ix.resident() == [("v", 2), ("v", 3), ("v", 4), ("v", 5)]
    ix.release()
    slots, missing = ix.assign("w", [2])                            # another video's frame 2 is another frame
    assert missing == [(2, 2)] and ("v", 2) not in ix.resident()
    assert (ix.fetched, ix.requested) == (7, 10)


def test_store_never_evicts_frames_of_the_open_minibatch_and_raises_over_capacity():
    from datasets.frame_store import StoreIndex
    from vlfb import hip
    ix2 = StoreIndex(4)
    ix2.assign("v", [0, 1])
    ix2.release()
    ix2.assign("v", [2, 3])                                         # (open)
    assert ix2.assign("v", [0, 4])[1] == [(4, 1)]                   # 0 is a hit and open now; frame 1 (not open) goes
    before = (ix2.resident(), ix2.fetched, ix2.requested)
    with pytest.raises(hip.VlfbError, match="more than the 4 frames"):
        ix2.assign("v", [5])                                        # five distinct frames in one minibatch
    assert (ix2.resident(), ix2.fetched, ix2.requested) == before   # refused whole: nothing was overwritten or counted
    with pytest.raises(hip.VlfbError):
        ix2.assign("v", [2, 6, 7])
    assert (ix2.resident(), ix2.fetched, ix2.requested) == before
    ix2.release()
    assert ix2.assign("v", [5])[1] == [(5, 0)]                      # released: the oldest frame (0, in slot 0) goes
    ix3 = StoreIndex(2)
    with pytest.raises(hip.VlfbError):
        ix3.assign("v", [0, 1, 2])                                  # a single clip larger than the store
    assert ix3.resident() == [] and ix3.assign("v", [7, 7, 8])[0] == [0, 0, 1]


def test_store_counts_of_a_charades_style_pass():
    """centres every 12 frames, rate 4, T = 4 over 60 frames: every distinct frame number is fetched exactly once"""
    from datasets import dataset_helper
    from datasets.frame_store import StoreIndex
    T, rate, frames = 4, 4, 60
    centres = [c for c in range(frames) if (c + 1) % 12 == 0]
    seqs = [dataset_helper.get_sequence(c, T * rate // 2, rate, frames) for c in centres]
    assert len(centres) == 5 and seqs[0] == [3, 7, 11, 15] and seqs[-1] == [51, 55, 59, 59]
    distinct = len({f for s in seqs for f in s})
    assert distinct < len(seqs) * T                                 # (the clips do overlap, and the clamp repeats a frame)
    ix = StoreIndex(8)
    for lo in range(0, len(seqs), 2):                               # minibatches of two clips
        for s in seqs[lo:lo + 2]:
            slots, _ = ix.assign(0, s)
            assert len(slots) == T
        ix.release()
    assert ix.fetched == distinct and ix.requested == len(seqs) * T


# ---- the bank queries ------------------------------------------------------------------------------------------------------

def test_query_builders_equal_what_the_synchronous_samplers_upload():
    """host arrays only: DeviceBank on the CPU device allocates, the queries never touch it"""
    from vlfb import lfb_bank
    bank = lfb_bank.DeviceBank(3, 40, 2, 8, "f32", device="cpu", video_ids=[11, 5, 7])
    videos = [5, 11, 7, 99, 5]
    rows = np.array([1, 0, 2, -1, 1])
    centers = [0, 37, 500, 12, 130]

    def want(lo, hi):
        return np.ascontiguousarray(np.stack([rows, lo, hi], axis=1), dtype=np.int32)
    q = bank.frames_query(videos, centers, 8, 2)
    assert q.dtype == np.int32 and q.shape == (5, 3)
    assert np.array_equal(q, want(*lfb_bank.frame_window_steps(centers, 8, 2)))
    q = bank.epic_verb_query(videos, centers, 7, 1)
    assert q.dtype == np.int32 and np.array_equal(q, want(*lfb_bank.epic_verb_window_steps(centers, 7, 1)))
    q = bank.epic_noun_query(videos, centers, 12, 4, 1)
    assert q.dtype == np.int32 and np.array_equal(q, want(*lfb_bank.epic_noun_window_steps(centers, 12, 4, 1)))
    # the append keys: [bank row, step - step_base], and the frame-level form with its padding rows
    b2 = lfb_bank.DeviceBank(2, 10, 1, 8, "f32", device="cpu", step_base=3)
    assert bank.append_keys([7, 5], [4, 9]).tolist() == [[2, 4], [1, 9]]
    assert b2.append_keys([1, 0], [4, 9]).tolist() == [[1, 1], [0, 6]]
    k = bank.frame_keys(4, [(5, 11), (7, 35)], 12)
    assert k.dtype == np.int32 and k.tolist() == [[1, 0], [2, 2], [-1, 0], [-1, 0]]
    with pytest.raises(AssertionError):
        bank.frame_keys(2, [(5, 10)], 12)


def test_a_refused_or_failed_request_leaves_the_store_as_it_was():
    """a refusal after evictions of the same call, and a fetch that fails: resident frames, open frames and both counters
    are what they were"""
    from datasets.frame_store import StoreIndex
    from vlfb import hip
    ix = StoreIndex(4)
    ix.assign("v", [0, 1, 2, 3])
    ix.release()
    ix.assign("v", [3])                                             # (open)
    before = (ix.resident(), sorted(ix.free), set(ix.open), ix.fetched, ix.requested)
    with pytest.raises(hip.VlfbError):
        ix.assign("v", [2, 4, 5, 6, 7])                             # evicts 0 and 1, opens 2, then finds nothing to evict
    assert (ix.resident(), sorted(ix.free), set(ix.open), ix.fetched, ix.requested) == before
    assert ix.assign("v", [0, 1])[1] == []                          # still resident: hits
    slots, missing = ix.assign("v", [8])                            # what a FrameStore does when fetch() raises
    assert missing == [(8, 2)]
    ix.undo()
    assert ix.resident() == before[0] and (ix.fetched, ix.requested) == (before[3], before[4] + 2)
    assert ix.open == {("v", 3), ("v", 0), ("v", 1)}
