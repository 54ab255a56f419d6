"""Inputs shared by tests/test_frame_bank_pass_gpu.py and tests/test_test_pass_gpu.py: small Charades / EPIC data sets
written the way the product reads them (frame lists, the EPIC annotation file), synthetic frames served by a
FrameStore.fetch, and the small engines of tests/test_frame_loader_gpu.py: crop 64, 4 frames at rate 4,
NONLOCAL.CONV3_NONLOCAL off (the grouped res3 block needs 8 frames), synthetic parameters, 2 clips per batch."""
import collections
import csv
import os

import numpy as np

import clip_loader_cases as cases

CROP, T, RATE, N = cases.CROP, 4, 4, 2
H, W = 40, 56
EXTRA = ["TEST.SAMPLE_RATE", RATE, "NONLOCAL.CONV3_NONLOCAL", False]
HEADER = "original_vido_id video_id frame_id path labels"


def bits(t):
    import torch
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).cpu().numpy().reshape(-1)


def videos(lengths, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (n, H, W, 3)).astype(np.uint8) for n in lengths]


def write_charades_lists(tmp, lengths, frame_labels=None):
    """frames.csv: video Vi of lengths[i] frames; frame_labels[i][k] = the class ids of frame k"""
    rows = [HEADER]
    for vi, n in enumerate(lengths):
        for k in range(n):
            lab = ",".join(str(x) for x in frame_labels[vi][k]) if frame_labels is not None else ""
            rows.append('V%d %d %d V%d/%06d.jpg "%s"' % (vi, vi, k, vi, k + 1, lab))
    with open(os.path.join(str(tmp), "frames.csv"), "w") as f:
        f.write("\n".join(rows) + "\n")


def write_epic_lists(tmp, names, lengths):
    """frames.csv: frame files numbered from 1, as EPIC's are"""
    rows = [HEADER]
    for vi, (name, n) in enumerate(zip(names, lengths)):
        rows += ['%s %d %d %s/frame_%010d.jpg ""' % (name, vi, k, name, k + 1) for k in range(n)]
    with open(os.path.join(str(tmp), "frames.csv"), "w") as f:
        f.write("\n".join(rows) + "\n")


def write_epic_annotations(tmp, rows, name="EPIC_train_action_labels.csv"):
    """rows: (participant, video, start seconds, stop seconds, verb class, noun class) -> the 14-column file"""
    stamp = lambda s: "00:00:%05.2f" % s
    with open(os.path.join(str(tmp), name), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["uid", "participant_id", "video_id", "narration", "start_timestamp", "stop_timestamp", "start_frame",
                    "stop_frame", "verb", "verb_class", "noun", "noun_class", "all_nouns", "all_noun_classes"])
        for uid, (person, video, start, stop, verb, noun) in enumerate(rows):
            w.writerow([uid, person, video, "do it", stamp(start), stamp(stop), int(start * 60), int(stop * 60), "verb", verb,
                        "noun", noun, "['noun', 'other']", "[%d, 1]" % noun])


def point_cfg_at(cfg, tmp):
    for part in (cfg.CHARADES, cfg.EPIC):
        part.FRAME_LIST_DIR = str(tmp)
        part.TRAIN_LISTS = part.TEST_LISTS = ["frames.csv"]
    cfg.EPIC.ANNOTATION_DIR = str(tmp)
    cfg.CHECKPOINT.DIR = cfg.LFB.LOAD_LFB_PATH = str(tmp)
    cfg.DATADIR = ""
    cfg.LOG_PERIOD = 100


def engine(sfx, infer_only=False, dtype="bf16", lfb=None):
    """a planned test-mode engine for the loaded cfg with synthetic parameters -> (model, engine, params)"""
    from core.config import config as cfg
    from models.model_builder_video import ModelBuilder
    from vlfb.engine import Engine
    from vlfb import synth
    m = ModelBuilder(train=False, split="test", name="test")
    m.build_model(suffix=sfx, lfb=lfb, lfb_infer_only=infer_only, shift=1)
    eng = Engine(m, dtype, device="cuda:0", base_seed=2)
    shapes = {"data" + sfx: (N, 3, T, CROP, CROP),
              "labels" + sfx: (N, cfg.MODEL.NUM_CLASSES) if cfg.MODEL.MULTI_LABEL else (N,),
              "lfb" + sfx: (N, cfg.LFB.WINDOW_SIZE, cfg.LFB.LFB_DIM)}
    eng.plan(collections.OrderedDict((name, shapes[name]) for name in m.input_blob_names))
    params = {k: v for k, v in synth.params(m, seed=2).items() if k in eng.param_views}
    eng.feed_params(params)
    return m, eng, params


def store_factory(fetch, capacity=64):
    """make_store(device, stream) of the product's passes; the stores it made are kept in .made"""
    from datasets.frame_store import FrameStore

    def make(device, stream):
        st = FrameStore(H, W, capacity, device, stream)
        st.fetch = fetch
        make.made.append(st)
        return st
    make.made = []
    return make


def feed_clips(eng, sfx, infos, frames_of):
    """the existing single-clip path: every clip of the minibatch preprocessed on its own into the data blob"""
    from datasets import data_input_helper as dh
    data, (w_pad, c_pad) = eng.blob_padded("data" + sfx)
    for n, c in enumerate(infos):
        dh.images_and_boxes_preprocessing(frames_of(c.video)[np.array(c.seq)], 0, CROP, c.shift, out=data[n], w_pad=w_pad,
                                          c_pad=c_pad)
