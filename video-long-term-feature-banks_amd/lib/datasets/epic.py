"""EPIC-Kitchens: annotations, clip sequences and the clips of a bank-construction pass (reference: lib/datasets/epic.py).

Index arithmetic only, as datasets.charades.  Random draws take an explicit `rng` with the interface of Python's `random`
module (the reference draws the clip centre with `random.randint` and the train annotation with `np.random.choice`)."""
import collections
import csv
import os
import random

import numpy as np

from core.config import config as cfg
from datasets import dataset_helper

CENTER_CROP_INDEX = 1
TRAIN_PERSON_INDICES = range(1, 26)
NUM_CLASSES_VERB = 125
NUM_CLASSES_NOUN = 352

ClipInfo = collections.namedtuple("ClipInfo", "video center seq labels shift")


def sec_to_frame(sec):
    """time index (seconds) -> frame index"""
    return int(np.round(float(sec) * cfg.EPIC.FPS))


def frame_to_sec(frame):
    """frame index -> time index (seconds)"""
    return int(np.round(float(frame) / cfg.EPIC.FPS))


def time_to_sec(sec):
    """'00:02:10.99' -> seconds"""
    hour, minute, sec = sec.split(":")
    return 3600.0 * int(hour) + 60.0 * int(minute) + float(sec)


def get_sequence(start_frame, stop_frame, half_len, sample_rate, num_frames, is_train, rng=random):
    """(frames of the clip, its centre): the centre is drawn inside the annotated segment in train (both ends included)
    and is its middle otherwise; frames clamped into the video"""
    center = rng.randint(start_frame, stop_frame) if is_train else (stop_frame + start_frame) // 2
    seq = [min(max(f, 0), num_frames - 1) for f in range(center - half_len, center + half_len, sample_rate)]
    return seq, center


def load_annotations(path, is_train):
    """EPIC_train_action_labels.csv -> [(person, video, start_frame, stop_frame, verb, noun)]; participants P01..P25
    are the train split, the others the held-out one.  Columns: uid, participant_id, video_id, narration,
    start_timestamp, stop_timestamp, start_frame, stop_frame, verb, verb_class, noun, noun_class, all_nouns,
    all_noun_classes (frames are recomputed from the timestamps)."""
    annotations = []
    with open(path, "r", newline="") as f:
        f.readline()
        for row in csv.reader(f):
            person = row[1]
            if (int(person[1:]) in TRAIN_PERSON_INDICES) != bool(is_train):
                continue
            verb, noun = int(row[-5]), int(row[-3])
            assert 0 <= verb < NUM_CLASSES_VERB, verb
            assert 0 <= noun < NUM_CLASSES_NOUN, noun
            annotations.append((person, row[2], sec_to_frame(time_to_sec(row[4])), sec_to_frame(time_to_sec(row[5])),
                                verb, noun))
    return annotations


def filename_to_frame_id(img_path):
    return int(img_path[-10:-4])


def get_annotations_for_lfb_frames(image_paths):
    """the "annotations" of a bank-construction pass: one clip centred on every frame whose number (from its file name)
    is a multiple of EPIC.FPS // EPIC.VERB_LFB_CLIPS_PER_SECOND, videos in the dictionary's order"""
    sample_freq = cfg.EPIC.FPS // cfg.EPIC.VERB_LFB_CLIPS_PER_SECOND
    annotations = []
    for video_name in image_paths.keys():
        for img_path in image_paths[video_name]:
            frame = filename_to_frame_id(img_path)
            if frame % sample_freq == 0:
                annotations.append((video_name[:3], video_name, frame, frame, 0, 0))
    return annotations


class EpicIndex(object):
    """image_paths: {video name: frame paths} (load_image_lists(..., return_dict=True)); annotations: load_annotations, or
    None with lfb_infer_only (get_annotations_for_lfb_frames).  `shift` is the spatial position outside train (None: the
    centre crop)."""

    def __init__(self, image_paths, annotations, split, lfb_infer_only, shift=None):
        self.split, self.is_train, self.lfb_infer_only, self.shift = split, split == "train", bool(lfb_infer_only), shift
        self.num_frames = {v: len(p) for v, p in image_paths.items()}
        self.annotations = get_annotations_for_lfb_frames(image_paths) if self.lfb_infer_only else list(annotations)
        part = cfg.TRAIN if self.is_train else cfg.TEST
        self.sample_rate, self.video_length, self.batch_size = part.SAMPLE_RATE, part.VIDEO_LENGTH, part.BATCH_SIZE
        self.seq_len = self.video_length * self.sample_rate

    @classmethod
    def from_cfg(cls, split, lfb_infer_only, shift=None, get_train_lfb=False):
        """the index of the files EpicDataset._get_data reads: the frame lists of EPIC.FRAME_LIST_DIR (TRAIN_LISTS for
        split 'train' or a train-bank pass, `get_train_lfb`, else TEST_LISTS) and, outside a bank pass, the annotations
        EPIC.ANNOTATION_DIR / EPIC.ANNOTATIONS of the split's participants.  Keeps `image_paths` (by video name, in the
        lists' order) and the video-name tables for the frame store's `fetch`."""
        e = cfg.EPIC
        is_train = split == "train"
        lists = e.TRAIN_LISTS if (is_train or get_train_lfb) else e.TEST_LISTS
        image_paths, _, video_idx_to_name, video_name_to_idx = dataset_helper.load_image_lists(
            [os.path.join(e.FRAME_LIST_DIR, name) for name in lists], return_dict=True)
        annotations = None if lfb_infer_only else load_annotations(os.path.join(e.ANNOTATION_DIR, e.ANNOTATIONS), is_train)
        index = cls(image_paths, annotations, split, lfb_infer_only, shift)
        index.image_paths, index.video_idx_to_name, index.video_name_to_idx = image_paths, video_idx_to_name, video_name_to_idx
        return index

    def get_db_size(self):
        return len(self.annotations)

    def get_minibatch_info(self, indices, rng=random):
        """per clip a ClipInfo(video name, center, seq, label, shift): label is the verb or the noun class
        (EPIC.CLASS_TYPE).  Train ignores the index and draws an annotation (rng.randrange), then the centre
        (rng.randint); a short last batch is padded with indices[0]."""
        half_len = self.seq_len // 2
        indices = [int(i) for i in indices]
        while len(indices) < self.batch_size // cfg.NUM_GPUS:
            indices.append(indices[0])
        shift = None if self.is_train else (CENTER_CROP_INDEX if self.shift is None else self.shift)
        out = []
        for idx in indices:
            ann = rng.randrange(len(self.annotations)) if self.is_train else idx
            _, video, start, stop, verb, noun = self.annotations[ann]
            seq, center = get_sequence(start, stop, half_len, self.sample_rate, self.num_frames[video], self.is_train, rng)
            out.append(ClipInfo(video, center, seq, verb if cfg.EPIC.CLASS_TYPE == "verb" else noun, shift))
        return out
