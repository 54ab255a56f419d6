"""Frame lists and clip sequences shared by the frame-level datasets (reference: lib/datasets/dataset_helper.py).

Index arithmetic only: which frames make a clip.  Nothing here opens an image; decoding stays with the caller's `fetch`
(datasets.frame_store) or `source` (datasets.clip_loader)."""
import os
from collections import defaultdict

from core.config import config as cfg


def load_image_lists(list_filenames, return_dict=False):
    """frame lists (one header line, then `original_video_id video_id frame_id path "labels"` per frame) ->
    (image_paths, labels, video_idx_to_name, video_name_to_idx).  Videos are numbered in order of first appearance;
    image_paths / labels are lists indexed by that number, or with return_dict dictionaries keyed by the video's name.
    A frame's labels are a list of ints, [] for `""`."""
    image_paths, labels = defaultdict(list), defaultdict(list)
    video_name_to_idx, video_idx_to_name = {}, {}
    for list_filename in list_filenames:
        with open(list_filename, "r") as f:
            f.readline()
            for line in f:
                row = line.split()
                assert len(row) == 5, "a frame list row has 5 fields: %r" % (line,)
                name = row[0]
                if name not in video_name_to_idx:
                    idx = len(video_name_to_idx)
                    video_name_to_idx[name] = idx
                    video_idx_to_name[idx] = name
                key = name if return_dict else video_name_to_idx[name]
                image_paths[key].append(os.path.join(cfg.DATADIR, row[3]))
                frame_labels = row[-1].replace('"', "")
                labels[key].append([int(x) for x in frame_labels.split(",")] if frame_labels != "" else [])
    if return_dict:
        return dict(image_paths), dict(labels), video_idx_to_name, video_name_to_idx
    n = len(image_paths)
    return [image_paths[i] for i in range(n)], [labels[i] for i in range(n)], video_idx_to_name, video_name_to_idx


def get_sequence(center_idx, half_len, sample_rate, num_frames):
    """the frames of the clip around `center_idx`: every sample_rate-th of [centre - half_len, centre + half_len), each
    clamped into the video (a clip at a video's end repeats its first / last frame)"""
    return [min(max(f, 0), num_frames - 1) for f in range(center_idx - half_len, center_idx + half_len, sample_rate)]
