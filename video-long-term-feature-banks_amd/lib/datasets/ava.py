"""AVA: which keyframes there are, which boxes and labels a keyframe carries, which frames make its clip, and which bank
slots its window draws (reference: lib/datasets/ava.py and construct_label_array of ava_data_input.py).

`AvaIndex.get_minibatch_info` is what the reference's AvaDataset.get_minibatch_info computes before it touches a file; the
pixels are the clip loader's (datasets.clip_loader.MinibatchLoader), fed by `minibatch_source`.  Random draws take an explicit
`rng` with the interface of `numpy.random` (the reference calls `np.random.choice`).

Ordering.  The reference is Python 2 and leaves the order of the boxes of a second, and of the seconds of a video, to the
hash order of its dictionaries.  Here both are defined as order of first appearance -- what the reference's code yields on
Python 3: the boxes of a second in the order their box text first appears in the annotation files, the seconds of a video
in the order they enter the dictionary, which is ascending because the first row of a video creates every second of
AVA_VALID_FRAMES at once."""
import collections
import os

import numpy as np

from core.config import config as cfg
from datasets import dataset_helper

FPS = cfg.AVA.FPS
CENTER_CROP_INDEX = 1
AVA_VALID_FRAMES = range(902, 1799)

AvaClipInfo = collections.namedtuple("AvaClipInfo", "video sec center seq boxes labels shift lfb_slots")


def sec_to_frame(sec):
    """time index (second) -> frame index: second 900 is frame 0"""
    return (sec - 900) * cfg.AVA.FPS


def load_boxes_and_labels(filenames, is_train, detect_thresh, full_eval):
    """csv rows `video, sec, x1, y1, x2, y2, label[, score]` -> {video_name: {sec: [[box, [labels...]], ...]}} with every
    second of AVA_VALID_FRAMES present for a video that has any row left.  Outside train, and unless full_eval, only the
    seconds with sec % 4 == 0 are kept; a row with a score below detect_thresh is dropped; an empty label is -1.  Rows
    belong to the same box when the TEXT of their four coordinates agrees."""
    ret = {}
    for filename in filenames:
        with open(filename, "r") as f:
            for line in f:
                row = line.strip().split(",")
                assert len(row) in (7, 8), "an AVA annotation row has 7 or 8 fields: %r" % (line,)
                video_name, frame_sec = row[0], int(row[1])
                if not is_train and not full_eval and frame_sec % 4 != 0:
                    continue
                box_key = ",".join(row[2:6])
                label = -1 if row[6] == "" else int(row[6])
                if len(row) == 8 and float(row[7]) < detect_thresh:
                    continue
                if video_name not in ret:
                    ret[video_name] = {sec: {} for sec in AVA_VALID_FRAMES}
                boxes = ret[video_name][frame_sec]
                if box_key not in boxes:
                    boxes[box_key] = [[float(x) for x in row[2:6]], []]
                boxes[box_key][1].append(label)
    return {name: {sec: list(boxes.values()) for sec, boxes in secs.items()} for name, secs in ret.items()}


def get_keyframe_indices(boxes_and_labels):
    """[(video_idx, sec, frame)] of every valid second that has a box, videos in index order"""
    return [(video_idx, sec, sec_to_frame(sec)) for video_idx in range(len(boxes_and_labels))
            for sec in boxes_and_labels[video_idx].keys()
            if sec in AVA_VALID_FRAMES and len(boxes_and_labels[video_idx][sec]) > 0]


def get_num_boxes_used(keyframe_indices, boxes_and_labels):
    return sum(len(boxes_and_labels[video_idx][sec]) for video_idx, sec, _ in keyframe_indices)


def construct_label_array(labels, num_classes=None):
    """label list (1-based, -1 = none) -> multi-hot int32 row of MODEL.NUM_CLASSES"""
    n = int(num_classes if num_classes is not None else cfg.MODEL.NUM_CLASSES)
    arr = np.zeros((n,), dtype=np.int32)
    for lbl in labels:
        if lbl == -1:
            continue
        assert 1 <= lbl <= n, "AVA labels are 1 .. %d, got %r" % (n, lbl)
        arr[lbl - 1] = 1
    return arr


class AvaIndex(object):
    """image_paths: per video the per-frame list of dataset_helper.load_image_lists (only the lengths are read);
    video_idx_to_name: its third result; boxes_and_labels: what load_boxes_and_labels returns, or a list already ordered by
    video index.  split 'train' draws a keyframe per clip; any other split walks the keyframes in order.  lfb_infer_only
    (the bank pass) keeps every keyframe (full_eval) and filters boxes with AVA.LFB_DETECTION_SCORE_THRESH."""

    @staticmethod
    def thresholds(lfb_infer_only):
        """(full_eval, detect_thresh) as AvaDataset.__init__ picks them; AVA.FULL_EVAL / AVA.DETECTION_SCORE_THRESH are
        what the drivers set (train_net.py:107-108) and default to the *_DURING_TRAINING / *_TRAIN settings"""
        if lfb_infer_only:
            return True, cfg.AVA.LFB_DETECTION_SCORE_THRESH
        return (cfg.AVA.get("FULL_EVAL", cfg.AVA.FULL_EVAL_DURING_TRAINING),
                cfg.AVA.get("DETECTION_SCORE_THRESH", cfg.AVA.DETECTION_SCORE_THRESH_TRAIN))

    def __init__(self, image_paths, video_idx_to_name, boxes_and_labels, split, lfb_infer_only, shift=None):
        self.split, self.lfb_infer_only, self.shift = split, bool(lfb_infer_only), shift
        self.full_eval, self.detect_thresh = self.thresholds(self.lfb_infer_only)
        self.split_num = int(split == "train" and not self.lfb_infer_only)      # 1: train-time augmentation
        self.num_frames = [len(p) for p in image_paths]
        self.num_videos = len(self.num_frames)
        self.video_idx_to_name = dict(video_idx_to_name)
        assert len(boxes_and_labels) == self.num_videos, (len(boxes_and_labels), self.num_videos)
        if isinstance(boxes_and_labels, dict):
            boxes_and_labels = [boxes_and_labels[self.video_idx_to_name[i]] for i in range(self.num_videos)]
        self.boxes_and_labels = boxes_and_labels
        self.keyframe_indices = get_keyframe_indices(self.boxes_and_labels)
        self.num_boxes_used = get_num_boxes_used(self.keyframe_indices, self.boxes_and_labels)
        part = cfg.TRAIN if split == "train" else cfg.TEST
        self.sample_rate, self.video_length, self.batch_size = part.SAMPLE_RATE, part.VIDEO_LENGTH, part.BATCH_SIZE
        self.seq_len = self.video_length * self.sample_rate

    @classmethod
    def from_cfg(cls, split, lfb_infer_only, shift=None, get_train_lfb=False):
        """the index of the files AvaDataset._get_data reads: the train frame lists for split 'train' or a train-bank pass
        (`get_train_lfb`, the reference's cfg.GET_TRAIN_LFB), the LFB box lists for a bank pass"""
        a = cfg.AVA
        lists = a.TRAIN_LISTS if (split == "train" or get_train_lfb) else a.TEST_LISTS
        image_paths, _, video_idx_to_name, _ = dataset_helper.load_image_lists(
            [os.path.join(a.FRAME_LIST_DIR, name) for name in lists])
        if lfb_infer_only:
            ann = a.TRAIN_LFB_BOX_LISTS if get_train_lfb else a.TEST_LFB_BOX_LISTS
        else:
            ann = a.TRAIN_BOX_LISTS if split == "train" else a.TEST_BOX_LISTS
        full_eval, detect_thresh = cls.thresholds(lfb_infer_only)
        boxes_and_labels = load_boxes_and_labels([os.path.join(a.ANNOTATION_DIR, name) for name in ann],
                                                 is_train=(split == "train"), detect_thresh=detect_thresh, full_eval=full_eval)
        return cls(image_paths, video_idx_to_name, boxes_and_labels, split, lfb_infer_only, shift)

    def get_db_size(self):
        return len(self.keyframe_indices)

    def get_minibatch_info(self, indices, rng=np.random, bank_counts=None, step_base=902):
        """per clip an AvaClipInfo(video, sec, center, seq, boxes, labels, shift, lfb_slots); a short batch is padded with
        indices[0] to batch_size // NUM_GPUS clips.  In train the keyframe is `rng.choice(range(db_size))` per clip and the
        index is ignored (ava.py:208-210).  shift is None under train-time augmentation (the crop is drawn), else the
        constructor's `shift` or the centre crop.  With `bank_counts` -- the host array of DeviceBank.counts(), rows = video
        indices -- lfb_slots is the clip's int32 [LFB.WINDOW_SIZE][AVA.LFB_MAX_NUM_FEAT_PER_STEP] slot table (-1 = empty),
        drawn right after the clip's keyframe with the calls `sample_lfb` makes, so one seeded np.random reproduces the
        reference's interleaving of draws across the clips of a minibatch; without it lfb_slots is None."""
        from vlfb.lfb_bank import reference_draw_clip
        half_len = self.seq_len // 2
        indices = [int(i) for i in indices]
        while len(indices) < self.batch_size // cfg.NUM_GPUS:
            indices.append(indices[0])
        out = []
        for idx in indices:
            if self.split == "train":
                idx = rng.choice(range(len(self.keyframe_indices)))
            video, sec, center = self.keyframe_indices[idx]
            seq = dataset_helper.get_sequence(center, half_len, self.sample_rate, self.num_frames[video])
            clip = self.boxes_and_labels[video][sec]
            assert len(clip) > 0
            slots = None
            if bank_counts is not None:
                slots = reference_draw_clip(bank_counts, video, sec - int(step_base), cfg.LFB.WINDOW_SIZE,
                                            cfg.AVA.LFB_MAX_NUM_FEAT_PER_STEP, rng)
            shift = None if self.split_num else (CENTER_CROP_INDEX if self.shift is None else self.shift)
            out.append(AvaClipInfo(video, sec, center, seq, [list(b[0]) for b in clip], [list(b[1]) for b in clip], shift, slots))
        return out


def minibatch_source(index, store, rng, iterations=None, bank=None, aug_rng=None):
    """generator of what MinibatchLoader.start takes: (frames_list, boxes_list, labels_list, meta, rng, spatial_shift_pos)
    with clips as (store, video, frame_numbers) into the FrameStore `store` (decode stays the caller's, through
    store.fetch), boxes as (k, 4) normalised arrays, labels as (k, classes) int32 arrays and
    meta = dict(iteration=, videos=, secs=, padded=[bool per clip]) (+ lfb_slots per clip with `bank`, whose counts are read
    once).  Outside train: one pass over 0 .. db_size in order, in batches, the last one padded.  In train: passes without
    end (or `iterations` minibatches), the indices shuffled with `rng` at the start of every pass.
    aug_rng: the generator yielded to the loader for its augmentation draws, default `rng` itself (the reference's one
    np.random).  With its own, the walk -- the shuffles and get_minibatch_info's draws -- is `rng`'s alone, whatever thread
    consumes what is yielded: the ranks of a job seed it alike and walk alike (vlfb.lfb_pass.rank_source)."""
    if aug_rng is None:
        aug_rng = rng
    n = index.batch_size // cfg.NUM_GPUS
    size = index.get_db_size()
    counts = bank.counts() if bank is not None else None
    step_base = bank.step_base if bank is not None else 902
    it = 0
    while size:
        order = np.arange(size)
        if index.split == "train":
            rng.shuffle(order)
        for lo in range(0, size, n):
            if iterations is not None and it >= iterations:
                return
            batch = order[lo:lo + n].tolist()
            infos = index.get_minibatch_info(batch, rng, counts, step_base)
            meta = dict(iteration=it, videos=[c.video for c in infos], secs=[c.sec for c in infos],
                        padded=[k >= len(batch) for k in range(len(infos))])
            if bank is not None:
                meta["lfb_slots"] = [c.lfb_slots for c in infos]
            shift = infos[0].shift if infos[0].shift is not None else CENTER_CROP_INDEX
            yield ([(store, c.video, c.seq) for c in infos],
                   [np.asarray(c.boxes, dtype=np.float64).reshape(-1, 4) for c in infos],
                   [np.stack([construct_label_array(l) for l in c.labels]) for c in infos], meta, aug_rng, shift)
            it += 1
        if index.split != "train":
            return
