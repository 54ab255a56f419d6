"""The AVA bank-construction pass (vlfb.lfb_pass) on the smallest ava_r50_baseline lfb_infer_only engine of the loader tests:
3 videos, 5 keyframes with ragged RoI counts, batches of 2 (so the last one is padded), frames served by a FrameStore.fetch.
The bank the pass builds is compared bit for bit with a host restatement of construct_ava_lfb (tools/lfb_loader.py:81-112)
over `box_pooled` fetched from the same engine fed clip by clip."""
import collections
import os
import pickle

import numpy as np
import pytest
import torch

import clip_loader_cases as cases

pytestmark = pytest.mark.gpu

CROP, T, N = cases.CROP, 8, 2
H, W, FRAMES = 40, 56, 130
# video, second, boxes: RoI counts 1, 3, 2, 3, 1 over 5 keyframes; scores at or above AVA.LFB_DETECTION_SCORE_THRESH, one below
ROWS = [("V0", 902, 1), ("V0", 903, 3), ("V1", 903, 2), ("V2", 902, 3), ("V2", 904, 1)]
CAPACITY = 4                                         # above the most RoIs of a keyframe


def _write_inputs(tmp_path):
    rng = np.random.default_rng(7)
    lines = []
    for name, sec, k in ROWS:
        for b in cases.boxes(sec + k, [k])[0]:
            lines.append("%s,%d,%.3f,%.3f,%.3f,%.3f,,%.2f" % ((name, sec) + tuple(b) + (rng.uniform(0.9, 1.0),)))
    lines.append("V1,902,0.1,0.1,0.5,0.5,,0.50")                                   # below the threshold: no keyframe
    with open(os.path.join(str(tmp_path), "boxes.csv"), "w") as f:
        f.write("\n".join(lines) + "\n")
    frames = ["original_vido_id video_id frame_id path labels"]
    for vi in range(3):
        frames += ['V%d %d %d V%d/%06d.jpg ""' % (vi, vi, k, vi, k + 1) for k in range(FRAMES)]
    with open(os.path.join(str(tmp_path), "frames.csv"), "w") as f:
        f.write("\n".join(frames) + "\n")
    return [rng.integers(0, 256, (FRAMES, H, W, 3)).astype(np.uint8) for _ in range(3)]


def _point_cfg_at(cfg, tmp_path):
    a = cfg.AVA
    a.FRAME_LIST_DIR = a.ANNOTATION_DIR = str(tmp_path)
    a.TRAIN_LISTS = a.TEST_LISTS = ["frames.csv"]
    a.TRAIN_BOX_LISTS = a.TEST_BOX_LISTS = a.TRAIN_LFB_BOX_LISTS = a.TEST_LFB_BOX_LISTS = ["boxes.csv"]
    cfg.CHECKPOINT.DIR = cfg.LFB.LOAD_LFB_PATH = str(tmp_path)


def _infer_engine(rows, sfx="_infer_test", dtype="bf16"):
    from core.config import config as cfg
    from models.model_builder_video import ModelBuilder
    from vlfb.engine import Engine
    from vlfb import synth
    m = ModelBuilder(train=False, split="test", name="infer")
    m.build_model(suffix=sfx, lfb_infer_only=True, shift=1)
    eng = Engine(m, dtype, device="cuda:0", base_seed=2)
    shapes = {"data" + sfx: (N, 3, T, CROP, CROP), "labels" + sfx: (rows, cfg.MODEL.NUM_CLASSES), "proposals" + sfx: (rows, 5)}
    eng.plan(collections.OrderedDict((name, shapes[name]) for name in m.input_blob_names))
    params = {k: v for k, v in synth.params(m, seed=2).items() if k in eng.param_views}
    eng.feed_params(params)
    return m, eng, params


def _same_lfb(a, b):
    if sorted(a) != sorted(b):
        return False
    for v in a:
        if sorted(a[v]) != sorted(b[v]):
            return False
        for s in a[v]:
            if len(a[v][s]) != len(b[v][s]) or not all(
                    x.dtype == y.dtype == np.float32 and np.array_equal(x.view(np.int32), y.view(np.int32))
                    for x, y in zip(a[v][s], b[v][s])):
                return False
    return True


def test_the_pass_builds_the_bank_construct_ava_lfb_builds_and_its_files_round_trip(tmp_path):
    from datasets import ava
    from datasets import data_input_helper as dh
    from datasets.clip_loader import MinibatchLoader
    from datasets.frame_store import FrameStore
    from utils import checkpoints as ck
    from vlfb import lfb_pass
    from vlfb.lfb_bank import DeviceBank
    videos = _write_inputs(tmp_path)
    with cases.loader_cfg("ava_r50_baseline", clips=N, frames=T) as cfg:
        _point_cfg_at(cfg, tmp_path)
        index = ava.AvaIndex.from_cfg("test", True, shift=1)
        size = index.get_db_size()
        assert size == 5 and size % N and [len(index.boxes_and_labels[v][s]) for v, s, _ in index.keyframe_indices] == [1, 3, 2, 3, 1]
        R = N * 3
        sfx = "_infer_test"
        m, eng, params = _infer_engine(R, sfx)
        data, (w_pad, c_pad) = eng.blob_padded("data" + sfx)

        # the reference's way, restated: every batch fed clip by clip, box_pooled fetched, construct_ava_lfb on the host --
        # without the clips that only pad the last batch
        want = {}
        for lo in range(0, size, N):
            infos = index.get_minibatch_info(list(range(lo, min(lo + N, size))))
            assert len(infos) == N
            boxes = []
            for n, c in enumerate(infos):
                _, b = dh.images_and_boxes_preprocessing(videos[c.video][np.array(c.seq)], 0, CROP, c.shift, np.array(c.boxes),
                                                         out=data[n], w_pad=w_pad, c_pad=c_pad)
                boxes.append(b)
            labels = [np.stack([ava.construct_label_array(l) for l in c.labels]) for c in infos]
            props, lab, used = dh.minibatch_rows(boxes, labels, R, cfg.MODEL.NUM_CLASSES)
            eng.feed("proposals" + sfx, props)
            eng.feed("labels" + sfx, lab)
            eng.forward()
            torch.cuda.synchronize()
            feats = eng.fetch("box_pooled").reshape(R, 2048)
            for r in range(used):
                n = int(props[r, 0])
                if lo + n >= size:
                    continue                                                       # a padding clip
                want.setdefault(infos[n].video, {}).setdefault(infos[n].sec, []).append(np.squeeze(feats[r]).astype(np.float32))
        assert sorted(want) == [0, 1, 2] and sum(len(l) for v in want.values() for l in v.values()) == 10

        # the pass: frame lists into a store, keys uploaded in stream order, box_pooled appended on the device
        loader = MinibatchLoader(eng, sfx, 0, n_slots=2, max_src_hw=(H, W), src_sizes=[(H, W)])
        store = FrameStore(H, W, 4 * N * T, loader.device, loader.stream)
        store.fetch = lambda v, f: videos[v][f]
        bank = DeviceBank(3, 3, CAPACITY, 2048, "fp32", step_base=902)
        assert lfb_pass.build_ava_bank(eng, loader, index, store, bank) is bank
        got = bank.to_reference()
        assert _same_lfb(got, want)
        assert bank.counts().tolist() == [[1, 3, 0], [0, 2, 0], [3, 0, 1]]           # (V2's last keyframe once, not twice)
        assert float(bank.bank.abs().max()) > 0 and store.fetched > 0

        # the files: the reference's pickle and the native file next to it
        pkl = lfb_pass.write_lfb(bank, is_train=False)
        assert pkl == os.path.join(str(tmp_path), "val_lfb.pkl") and os.path.exists(pkl[:-4] + ".npz")
        with open(pkl, "rb") as f:
            assert _same_lfb(pickle.load(f), want)
        native = lfb_pass.load_lfb(False)
        assert native.code == bank.code and (native.n_steps, native.capacity, native.step_base) == (3, CAPACITY, 902)
        assert np.array_equal(native.counts(), bank.counts()) and _same_lfb(native.to_reference(), want)
        os.remove(pkl[:-4] + ".npz")
        from_pickle = lfb_pass.load_lfb(False, dtype="fp32")
        assert _same_lfb(from_pickle.to_reference(), want)
        with open(pkl, "wb") as f:                                                  # a Python-2 pickle: protocol 2, str keys
            pickle.dump(want, f, 2)
        assert _same_lfb(lfb_pass.load_lfb(False, dtype="fp32").to_reference(), want)

        # get_lfb: the same pass from a parameter file, and the LOAD_LFB switch
        path = os.path.join(str(tmp_path), "baseline.pkl")
        ck.write_blobs(path, dict(params, lr=np.array([0.1], dtype=np.float32)))

        def make_store(device, stream):
            st = FrameStore(H, W, 4 * N * T, device, stream)
            st.fetch = lambda v, f: videos[v][f]
            return st
        del loader, eng
        inferred = lfb_pass.get_lfb(path, False, make_store, bank_dtype="fp32", max_src_hw=(H, W))
        assert inferred.capacity == 3 and _same_lfb(inferred.to_reference(), want)
        cfg.LFB.LOAD_LFB = True
        assert _same_lfb(lfb_pass.get_lfb("", False, None, bank_dtype="fp32").to_reference(), want)


def test_a_written_and_loaded_bank_feeds_the_train_loader_for_one_step(tmp_path):
    """ava_r50_lfb_nl, train: minibatch_source -> MinibatchLoader with the loaded bank -> one train step"""
    from datasets import ava
    from datasets.clip_loader import MinibatchLoader
    from datasets.frame_store import FrameStore
    from models.model_builder_video import ModelBuilder
    from vlfb import lfb_pass, synth
    from vlfb.engine import Engine
    from vlfb.lfb_bank import DeviceBank
    videos = _write_inputs(tmp_path)
    with cases.loader_cfg("ava_r50_lfb_nl", clips=N, frames=T, extra=["LFB.WINDOW_SIZE", 4]) as cfg:
        _point_cfg_at(cfg, tmp_path)
        cfg.TRAIN.PARAMS_FILE = ""
        built = DeviceBank(3, 3, CAPACITY, 2048, "bf16", step_base=902)
        rng = np.random.default_rng(3)
        feats = torch.as_tensor(rng.standard_normal((10, 2048)).astype(np.float32)).cuda()
        built.append(feats, [0, 0, 0, 0, 1, 1, 2, 2, 2, 2], [902, 903, 903, 903, 903, 903, 902, 902, 902, 904])
        lfb_pass.write_lfb(built, is_train=True)
        bank = lfb_pass.load_lfb(True)
        assert np.array_equal(bank.counts(), built.counts()) and torch.equal(bank.bank, built.bank)

        index = ava.AvaIndex.from_cfg("train", False)
        R = N * 3
        m = ModelBuilder(train=True, split="train", name="train")
        m.build_model(suffix="_train")
        eng = Engine(m, "bf16", device="cuda:0", base_seed=2)
        k = cfg.LFB.WINDOW_SIZE * cfg.AVA.LFB_MAX_NUM_FEAT_PER_STEP
        shapes = {"data_train": (N, 3, T, CROP, CROP), "labels_train": (R, cfg.MODEL.NUM_CLASSES), "proposals_train": (R, 5),
                  "lfb_train": (R, k, 2048)}
        eng.plan(collections.OrderedDict((name, shapes[name]) for name in m.input_blob_names))
        eng.feed_params(synth.params(m, seed=2))
        m.UpdateWorkspaceLr(0)
        loader = MinibatchLoader(eng, "_train", 1, n_slots=2, max_src_hw=(H, W), bank=bank, src_sizes=[(H, W)])
        store = FrameStore(H, W, 4 * N * T, loader.device, loader.stream)
        store.fetch = lambda v, f: videos[v][f]
        loader.start(ava.minibatch_source(index, store, np.random.RandomState(4), iterations=1, bank=bank))
        try:
            mb = loader.next()
            loader.deliver(mb)
            eng.train_step(float(m.current_lr))
            with pytest.raises(StopIteration):
                loader.next()
        finally:
            loader.stop()
        torch.cuda.synchronize()
        assert np.isfinite(float(eng.fetch("loss").reshape(-1)[0])) and mb.used >= N
        assert float(eng.blob_tensor("lfb_train")[0].float().abs().max()) > 0           # the head saw bank features
