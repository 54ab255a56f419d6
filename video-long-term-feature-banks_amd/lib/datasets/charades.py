"""Charades: which frames make a clip, which clip is which test segment, which labels a clip carries (reference:
lib/datasets/charades.py and construct_label_array of charades_data_input.py).

`CharadesIndex.get_minibatch_info` is what the reference's CharadesDataset.get_minibatch_info computes before it touches a
file or the bank; the pixels and the bank window are the clip loader's (datasets.clip_loader.FrameLoader).  Random draws
take an explicit `rng` with the interface of Python's `random` module (the reference calls `random.randint`)."""
import collections
import os
import random

import numpy as np

from core.config import config as cfg
from datasets import dataset_helper

CENTER_CROP_INDEX = 1

ClipInfo = collections.namedtuple("ClipInfo", "video center seq labels shift")


def sample_train_idx(num_frames, seq_len, rng=random):
    """centre of a train clip: uniform over the centres whose clip lies inside the video (both ends included, as
    random.randint), the middle frame of a video shorter than the clip"""
    half_len = seq_len // 2
    if num_frames < seq_len:
        return num_frames // 2
    return rng.randint(half_len, num_frames - half_len)


def sample_center_of_segments(segment_id, num_frames, num_test_segments, half_len=None):
    """centre of test segment `segment_id` of `num_test_segments` equal segments (np.round: halves go to even)"""
    return int(np.round((float(num_frames) / num_test_segments) * (segment_id + 0.5)))


def aggregate_labels(label_list):
    """the distinct labels of a sequence of per-frame label lists"""
    return list(set(l for labels in label_list for l in labels))


def get_lfb_frames(image_paths):
    """(video, frame) of every clip centre of a bank-construction pass: the frames with (frame + 1) % sample_freq == 0,
    sample_freq = CHARADES.FPS // CHARADES.LFB_CLIPS_PER_SECOND"""
    sample_freq = cfg.CHARADES.FPS // cfg.CHARADES.LFB_CLIPS_PER_SECOND
    return [(v, i) for v in range(len(image_paths)) for i in range(len(image_paths[v])) if (i + 1) % sample_freq == 0]


def construct_label_array(video_labels, num_classes=None):
    """label list -> multi-hot int32 row of MODEL.NUM_CLASSES"""
    arr = np.zeros((int(num_classes if num_classes is not None else cfg.MODEL.NUM_CLASSES),), dtype=np.int32)
    for lbl in set(video_labels):
        arr[lbl] = 1
    return arr


class CharadesIndex(object):
    """image_paths / image_labels: per video the per-frame lists of dataset_helper.load_image_lists (only their lengths
    and the labels are read).  split 'train' draws a centre per video; any other split walks
    CHARADES.NUM_TEST_CLIPS = 3 shifts x segments per video and carries video-level labels; lfb_infer_only walks
    get_lfb_frames with the centre crop."""

    def __init__(self, image_paths, image_labels, split, lfb_infer_only):
        self.split, self.lfb_infer_only = split, bool(lfb_infer_only)
        self.num_frames = [len(p) for p in image_paths]
        self.labels = [[list(l) for l in video] for video in image_labels]
        if split != "train":                                  # Charades is a video-level task
            self.labels = [[aggregate_labels(video)] * len(video) for video in self.labels]
        self.num_videos = len(self.num_frames)
        self.lfb_frames = get_lfb_frames(image_paths) if self.lfb_infer_only else None
        part = cfg.TRAIN if split == "train" else cfg.TEST
        self.sample_rate, self.video_length, self.batch_size = part.SAMPLE_RATE, part.VIDEO_LENGTH, part.BATCH_SIZE
        self.seq_len = self.video_length * self.sample_rate
        self.num_test_clips = cfg.CHARADES.get("NUM_TEST_CLIPS", cfg.CHARADES.NUM_TEST_CLIPS_DURING_TRAINING)
        self.num_test_segments = self.num_test_clips // 3     # 3-crop testing: 30 clips = 3 crops x 10 segments

    @classmethod
    def from_cfg(cls, split, lfb_infer_only, get_train_lfb=False):
        """the index of the frame lists CharadesDataset._get_data reads (CHARADES.FRAME_LIST_DIR): TRAIN_LISTS for split
        'train' or a train-bank pass (`get_train_lfb`, the reference's cfg.GET_TRAIN_LFB), else TEST_LISTS.  Keeps
        `image_paths` and the video-name tables for the frame store's `fetch`."""
        c = cfg.CHARADES
        lists = c.TRAIN_LISTS if (split == "train" or get_train_lfb) else c.TEST_LISTS
        image_paths, image_labels, video_idx_to_name, video_name_to_idx = dataset_helper.load_image_lists(
            [os.path.join(c.FRAME_LIST_DIR, name) for name in lists])
        index = cls(image_paths, image_labels, split, lfb_infer_only)
        index.image_paths, index.video_idx_to_name, index.video_name_to_idx = image_paths, video_idx_to_name, video_name_to_idx
        return index

    def get_db_size(self):
        if self.lfb_infer_only:
            return len(self.lfb_frames)
        return self.num_videos if self.split == "train" else self.num_videos * self.num_test_clips

    def get_minibatch_info(self, indices, rng=random):
        """per clip a ClipInfo(video, center, seq, labels, shift); a short last batch is padded with indices[0] to
        batch_size // NUM_GPUS clips.  shift is None in train (the crop is drawn), 0 / 1 / 2 = left / centre / right
        otherwise.  Test order: video = idx % V, multi_clip_idx = idx // V = (0-left, 0-centre, 0-right, 1-left, ...)."""
        half_len = self.seq_len // 2
        indices = [int(i) for i in indices]
        while len(indices) < self.batch_size // cfg.NUM_GPUS:
            indices.append(indices[0])
        out = []
        for idx in indices:
            if self.lfb_infer_only:
                video, center = self.lfb_frames[idx]
                shift = CENTER_CROP_INDEX
            else:
                video = idx % self.num_videos
                if self.split == "train":
                    center = sample_train_idx(self.num_frames[video], self.seq_len, rng)
                    shift = None
                else:
                    multi_clip_idx = idx // self.num_videos
                    shift = multi_clip_idx % 3
                    center = sample_center_of_segments(multi_clip_idx // 3, self.num_frames[video], self.num_test_segments,
                                                       half_len)
            seq = dataset_helper.get_sequence(center, half_len, self.sample_rate, self.num_frames[video])
            labels = aggregate_labels(self.labels[video][seq[0]:seq[-1] + 1])
            out.append(ClipInfo(video, center, seq, labels, shift))
        return out
