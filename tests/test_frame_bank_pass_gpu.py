"""The frame-level bank-construction pass (vlfb.lfb_pass.build_frame_bank / get_lfb) for Charades and EPIC verbs on the small
lfb_infer_only engines of tests/frame_pass_cases.py.  The bank the pass builds is compared bit for bit with a host
restatement of construct_frame_level_lfb (tools/lfb_loader.py:49-76) over `pool5` of the same engine fed clip by clip: the
same kernels on the same bytes, so no tolerance."""
import os
import pickle

import numpy as np
import pytest
import torch

import clip_loader_cases as cases
import frame_pass_cases as fc

pytestmark = pytest.mark.gpu
N, T = fc.N, fc.T
SFX = "_infer_test"

# name -> (preset, video names or None, frames per video, config overrides): Charades banks hold the frames 11, 23, ... (5 + 1
# clips: the last batch is full; 4 + 1: it is padded); EPIC verb banks the frames whose FILE number is a multiple of
# EPIC.FPS // EPIC.VERB_LFB_CLIPS_PER_SECOND = 10 (3 + 2 clips, padded)
CASES = {
    "charades_full": ("charades_r50_baseline", None, [60, 23], []),
    "charades_padded": ("charades_r50_baseline", None, [48, 23], []),
    "epic_verb": ("epic_verb_r50_baseline", ["P01_01", "P02_03"], [35, 25], ["EPIC.VERB_LFB_CLIPS_PER_SECOND", 3]),
}


def _setup(cfg, tmp_path, name):
    from datasets import charades, epic
    _, names, lengths, _ = CASES[name]
    vids = fc.videos(lengths, seed=len(name))
    fc.point_cfg_at(cfg, tmp_path)
    cfg.TEST.DATASET_SIZE = len(lengths)
    if names is None:
        fc.write_charades_lists(tmp_path, lengths)
        index = charades.CharadesIndex.from_cfg("test", True)
        frames_of = lambda v: vids[v]
        kind, sample_freq = "charades", cfg.CHARADES.FPS // cfg.CHARADES.LFB_CLIPS_PER_SECOND
        keys = list(index.lfb_frames)
        step_of = lambda f: (f + 1) // sample_freq - 1
        n_steps = max(lengths) // sample_freq
    else:
        fc.write_epic_lists(tmp_path, names, lengths)
        index = epic.EpicIndex.from_cfg("test", True, shift=1)
        frames_of = lambda v: vids[names.index(v)]
        kind, sample_freq = "epic_verb", cfg.EPIC.FPS // cfg.EPIC.VERB_LFB_CLIPS_PER_SECOND
        keys = [(a[1], a[2]) for a in index.annotations]
        step_of = lambda f: f // sample_freq
        n_steps = max(f for _, f in keys) // sample_freq + 1
    return dict(index=index, frames_of=frames_of, fetch=lambda v, f: frames_of(v)[f], kind=kind, sample_freq=sample_freq,
                keys=keys, step_of=step_of, n_steps=n_steps, names=names, lengths=lengths)


def _restated(cfg, c, eng):
    """construct_frame_level_lfb over pool5 fetched after every iteration: {video: {frame: feat}} and the dense bank"""
    index, size = c["index"], c["index"].get_db_size()
    pool5, _ = eng.blob_tensor("pool5")
    all_features = []
    for lo in range(0, size, N):
        infos = index.get_minibatch_info(list(range(lo, min(lo + N, size))))
        assert len(infos) == N
        fc.feed_clips(eng, SFX, infos, c["frames_of"])
        eng.forward()
        torch.cuda.synchronize()
        all_features.append(pool5.view(N, 2048).clone())
    lfb, global_idx = {}, 0
    rows = c["names"] if c["names"] is not None else list(range(len(c["lengths"])))
    dense = torch.zeros(len(rows), c["n_steps"], 1, 2048, dtype=pool5.dtype, device=pool5.device)
    count = np.zeros((len(rows), c["n_steps"]), dtype=np.int32)
    for feats in all_features:
        for i in range(feats.shape[0]):
            if global_idx >= len(c["keys"]):
                break                                              # (the clip that pads the last batch)
            video, frame = c["keys"][global_idx]
            global_idx += 1
            lfb.setdefault(video, {})[frame] = feats[i].float().cpu().numpy()
            dense[rows.index(video), c["step_of"](frame), 0] = feats[i]
            count[rows.index(video), c["step_of"](frame)] = 1
    return lfb, dense, count


def _same(a, b):
    return sorted(a) == sorted(b) and all(
        sorted(a[v]) == sorted(b[v]) and all(
            np.asarray(a[v][f]).dtype == np.float32 and np.array_equal(np.ravel(a[v][f]).view(np.int32), np.ravel(b[v][f]).view(np.int32))
            for f in a[v]) for v in a)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_pass_builds_the_bank_construct_frame_level_lfb_builds_and_its_files_round_trip(name, tmp_path):
    from datasets.clip_loader import FrameLoader
    from utils import checkpoints as ck
    from vlfb import hip, lfb_pass
    from vlfb.lfb_bank import DeviceBank
    preset, names, lengths, extra = CASES[name]
    with cases.loader_cfg(preset, clips=N, frames=T, extra=fc.EXTRA + extra) as cfg:
        c = _setup(cfg, tmp_path, name)
        index, size = c["index"], c["index"].get_db_size()
        assert size == len(c["keys"]) == {"charades_full": 6, "charades_padded": 5, "epic_verb": 5}[name]
        m, eng, params = fc.engine(SFX, infer_only=True)
        want, want_dense, want_count = _restated(cfg, c, eng)
        assert sum(len(v) for v in want.values()) == size and float(want_dense.float().abs().max()) > 0

        # the pass: frame lists into a store, keys uploaded in stream order, pool5 appended on the device
        make_store = fc.store_factory(c["fetch"])
        loader = FrameLoader(eng, SFX, 0, n_slots=2, max_src_hw=(fc.H, fc.W), src_sizes=[(fc.H, fc.W)])
        store = make_store(loader.device, loader.stream)
        bank = DeviceBank(len(lengths), c["n_steps"], 1, 2048, "bf16", video_ids=names)
        assert lfb_pass.build_frame_bank(eng, loader, index, store, bank, c["kind"]) is bank
        assert np.array_equal(bank.counts(), want_count) and int(want_count.sum()) == size       # the padding clip is not appended
        assert np.array_equal(fc.bits(bank.bank), fc.bits(want_dense))
        assert bank.count_nonfinite() == (0, size)
        got = bank.to_reference(frame_level=True, sample_freq=c["sample_freq"], epic=names is not None)
        assert {v: sorted(f) for v, f in got.items()} == {v: sorted(f) for v, f in want.items()} and _same(got, want)
        # every distinct frame was fetched once (the clip that pads the last batch names frames the store holds)
        seqs = [(ci.video, f) for lo in range(0, size, N) for ci in index.get_minibatch_info(list(range(lo, min(lo + N, size))))
                for f in ci.seq]
        assert store.fetched == len(set(seqs)) and store.requested == len(seqs) == -(-size // N) * N * T

        # the files: the reference's {video: {frame: feat}} pickle and the native file next to it
        pkl = lfb_pass.write_lfb(bank, is_train=False)
        assert pkl == os.path.join(str(tmp_path), "val_lfb.pkl") and os.path.exists(pkl[:-4] + ".npz")
        with open(pkl, "rb") as f:
            assert _same(pickle.load(f), want)
        native = lfb_pass.load_lfb(False)
        assert native.code == bank.code and native.video_ids == bank.video_ids
        assert np.array_equal(native.counts(), want_count) and np.array_equal(fc.bits(native.bank), fc.bits(want_dense))
        os.remove(pkl[:-4] + ".npz")
        from_pickle = lfb_pass.load_lfb(False)
        assert (from_pickle.n_steps, from_pickle.capacity) == (c["n_steps"], 1)
        assert _same(from_pickle.to_reference(frame_level=True, sample_freq=c["sample_freq"], epic=names is not None), want)

        # a non-finite parameter in front of pool5: the pass itself says so (a numeric condition, not a device fault)
        poisoned = dict(params)
        poisoned["res5_2_branch2c_bn_b"] = np.full_like(params["res5_2_branch2c_bn_b"], np.inf)
        eng.feed_params(poisoned)
        sick = DeviceBank(len(lengths), c["n_steps"], 1, 2048, "bf16", video_ids=names)
        with pytest.raises(hip.VlfbError, match="%d of %d occupied rows hold a NaN or Inf" % (size, size)):
            lfb_pass.build_frame_bank(eng, loader, index, make_store(loader.device, loader.stream), sick, c["kind"])
        del loader, eng

        # get_lfb: the same pass from a parameter file with the completeness conditions, and the LOAD_LFB switch
        path = os.path.join(str(tmp_path), "baseline.pkl")
        ck.write_blobs(path, dict(params, lr=np.array([0.1], dtype=np.float32)))
        inferred = lfb_pass.get_lfb(path, False, make_store, max_src_hw=(fc.H, fc.W))
        assert np.array_equal(inferred.counts(), want_count) and np.array_equal(fc.bits(inferred.bank), fc.bits(want_dense))
        assert inferred.video_ids == names
        cfg.TEST.DATASET_SIZE = len(lengths) + 1
        if name == "charades_padded":                              # len(lfb) == TEST.DATASET_SIZE (construct_lfb)
            with pytest.raises(AssertionError, match="the split has 3"):
                lfb_pass.get_lfb(path, False, make_store, max_src_hw=(fc.H, fc.W))
        lfb_pass.write_lfb(inferred, is_train=False)
        cfg.LFB.LOAD_LFB = True
        loaded = lfb_pass.get_lfb("", False, None)
        assert np.array_equal(loaded.counts(), want_count) and np.array_equal(fc.bits(loaded.bank), fc.bits(want_dense))

