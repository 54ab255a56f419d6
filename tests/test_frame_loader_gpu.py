"""datasets.clip_loader.FrameLoader: Charades / EPIC minibatches assembled on the loader's stream -- clips (stacked, or frame
lists into a datasets.frame_store.FrameStore), labels and the bank window -- against the existing single-clip path
(datasets.data_input_helper.images_and_boxes_preprocessing + Engine.feed + the synchronous DeviceBank samplers), bit for
bit: the same kernels on the same bytes, so no tolerance.

Small engines as in tests/test_train_loop_gpu.py: crop 64, 8 frames (4 in the bank pass), synthetic parameters."""
import collections

import numpy as np
import pytest

import clip_loader_cases as cases

pytestmark = pytest.mark.gpu
CROP = cases.CROP


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).cpu().numpy().reshape(-1)


def _engine(n, frames, train=True, infer_only=False, dtype="bf16"):
    """a planned engine for the loaded cfg with synthetic parameters; -> (model, engine, suffix)"""
    from core.config import config as cfg
    from models.model_builder_video import ModelBuilder
    from vlfb.engine import Engine
    from vlfb import synth
    split = "train" if train else "test"
    sfx = "_" + split
    m = ModelBuilder(train=train, split=split, name=split)
    m.build_model(suffix=sfx, lfb_infer_only=infer_only)
    eng = Engine(m, dtype, device="cuda:0", base_seed=2)
    shapes = {"data" + sfx: (n, 3, frames, CROP, CROP),
              "labels" + sfx: (n, cfg.MODEL.NUM_CLASSES) if cfg.MODEL.MULTI_LABEL else (n,),
              "lfb" + sfx: (n, cfg.LFB.WINDOW_SIZE, cfg.LFB.LFB_DIM)}
    eng.plan(collections.OrderedDict((name, shapes[name]) for name in m.input_blob_names))
    eng.feed_params({k: v for k, v in synth.params(m, seed=2).items() if k in eng.param_views})
    return m, eng, sfx


def _bank(kind, rng):
    """a small bank of two videos with gaps, and clip centres whose windows are cut by the bank's ends and by the gaps"""
    import torch
    from vlfb.lfb_bank import DeviceBank
    if kind == "charades":                                       # bank frames 11, 23, 35, ...: step t holds frame 12 (t + 1) - 1
        bank = DeviceBank(2, 10, 1, 2048, "bf16")
        keys = [(v, 12 * (t + 1) - 1) for v in range(2) for t in range(10) if (v, t) not in ((0, 3), (1, 0))]
        bank.append_frames(torch.as_tensor(rng.standard_normal((len(keys), 2048)).astype(np.float32)), keys, 12)
        centers = [40, 9]
    elif kind == "epic_verb":                                    # one clip per second: step t holds frame 30 t
        bank = DeviceBank(2, 12, 1, 2048, "bf16")
        keys = [(v, t) for v in range(2) for t in range(12) if (v, t) not in ((0, 5), (1, 11))]
        bank.append(torch.as_tensor(rng.standard_normal((len(keys), 2048)).astype(np.float32)), [k[0] for k in keys], [k[1] for k in keys])
        centers = [170, 335]
    else:                                                        # detections: 0..3 per frame, one frame per second
        bank = DeviceBank(2, 12, 3, 2048, "bf16")
        keys = [(v, t) for v in range(2) for t in range(12) for _ in range((v + t) % 4)]
        bank.append(torch.as_tensor(rng.standard_normal((len(keys), 2048)).astype(np.float32)), [k[0] for k in keys], [k[1] for k in keys])
        centers = [95, 300]
    bank.check_no_drops()
    return bank, centers


PRESETS = {"charades": "charades_r50_lfb_nl", "epic_verb": "epic_verb_r50_lfb_nl", "epic_noun": "epic_noun_r50_lfb_nl"}


def _sample(bank, kind, videos, centers, window, cfg, out=None, out_dtype=None):
    """the existing synchronous samplers"""
    if kind == "charades":
        return bank.sample_frames(videos, centers, window, cfg.CHARADES.LFB_CLIPS_PER_SECOND, out=out, out_dtype=out_dtype)
    if kind == "epic_verb":
        return bank.sample_epic_verb(videos, centers, window, cfg.EPIC.VERB_LFB_CLIPS_PER_SECOND, out=out, out_dtype=out_dtype)
    return bank.sample_epic_noun(videos, centers, window, cfg.EPIC.MAX_NUM_FEATS_PER_NOUN_LFB_FRAME,
                                 cfg.EPIC.NOUN_LFB_FRAMES_PER_SECOND, out=out, out_dtype=out_dtype)


@pytest.mark.parametrize("kind", ["charades", "epic_verb", "epic_noun"])
def test_a_minibatch_equals_the_single_clip_path_bit_for_bit(kind):
    import torch
    from datasets import charades
    from datasets import data_input_helper as dh
    from datasets.clip_loader import FrameLoader
    N, T, WINDOW = 2, 8, 4
    extra = ["LFB.WINDOW_SIZE", WINDOW] + (["EPIC.MAX_NUM_FEATS_PER_NOUN_LFB_FRAME", 2] if kind == "epic_noun" else [])
    with cases.loader_cfg(PRESETS[kind], clips=N, frames=T, extra=extra) as cfg:
        cfg.TRAIN.PARAMS_FILE = ""
        rng = np.random.default_rng(3)
        bank, centers = _bank(kind, rng)
        clips = cases.clips(40, sizes=cases.SIZES[:N], frames=T)
        if kind == "charades":
            labels_list = [[3, 150, 3, 17], []]
            want_labels = np.stack([charades.construct_label_array(l) for l in labels_list])
            assert want_labels.shape == (N, cfg.MODEL.NUM_CLASSES) and want_labels.sum() == 3
        else:
            labels_list = [5, cfg.MODEL.NUM_CLASSES - 1]
            want_labels = np.array(labels_list, dtype=np.int32)
        _, eng, sfx = _engine(N, T)
        data, (w_pad, c_pad) = eng.blob_padded("data" + sfx)
        lfb = eng.input_tensor("lfb" + sfx)
        # the existing path: N per-clip calls on one RandomState, the synchronous sampler
        rs = np.random.RandomState(7)
        want_data = torch.stack([dh.images_and_boxes_preprocessing(c, 1, CROP, 1, out_dtype=data.dtype, w_pad=w_pad, c_pad=c_pad,
                                                                   rng=rs)[0] for c in clips])
        want_lfb = _sample(bank, kind, [0, 1], centers, WINDOW, cfg, out_dtype=lfb.dtype)
        assert float(want_lfb.float().abs().max()) > 0
        filled = want_lfb.float().abs().amax(dim=2) > 0
        assert bool(filled.any()) and not bool(filled.all()), "the windows must hold both features and zero padding"

        loader = FrameLoader(eng, sfx, 1, n_slots=2, max_src_hw=(90, 96), bank=bank, bank_kind=kind, src_sizes=cases.SIZES[:N])
        mb = loader.submit(clips, labels_list, dict(iteration=0, videos=[0, 1], centers=centers), np.random.RandomState(7))
        loader.deliver(mb)
        assert np.array_equal(_bits(data), _bits(want_data))
        assert np.array_equal(_bits(lfb), _bits(want_lfb))
        got_labels = eng.input_tensor("labels" + sfx).cpu().numpy()
        assert got_labels.dtype == np.int32 and np.array_equal(got_labels.reshape(want_labels.shape), want_labels)
        assert np.array_equal(mb.labels, want_labels) and mb.videos == [0, 1] and mb.centers == centers
        eng.forward()                                                # the engine takes what was delivered
        torch.cuda.synchronize()
        assert np.isfinite(eng.fetch("loss")).all()


def test_three_charades_train_steps_fed_by_the_loader_equal_three_fed_through_feed():
    """charades_r50_lfb_nl, 8 frames, crop 64, 2 clips, bf16, with a bank: losses, parameters and momentum are bit-identical,
    and the recorded step holds no clip or bank call"""
    import torch
    from datasets import charades
    from datasets import data_input_helper as dh
    from datasets.clip_loader import FrameLoader
    N, T, STEPS, WINDOW = 2, 8, 3, 4
    with cases.loader_cfg("charades_r50_lfb_nl", clips=N, frames=T, extra=["LFB.WINDOW_SIZE", WINDOW]) as cfg:
        cfg.TRAIN.PARAMS_FILE = ""
        rng = np.random.default_rng(0)
        bank, _ = _bank("charades", rng)
        videos = [rng.integers(0, 256, (T, 72, 96, 3)).astype(np.uint8) for _ in range(N)]
        label_lists = [[[1, 20], [33]], [[], [7, 8, 9]], [[150], [1]]]
        centers = [[40, 9], [70, 100], [23, 60]]

        m1, e1, sfx = _engine(N, T)
        data1, (w_pad, c_pad) = e1.blob_padded("data" + sfx)
        lfb1, _ = e1.blob_tensor("lfb" + sfx)
        m1.UpdateWorkspaceLr(0)
        lr = float(m1.current_lr)
        losses1 = []
        for it in range(STEPS):
            rs = np.random.RandomState(100 * it)
            for n in range(N):
                dh.images_and_boxes_preprocessing(videos[n], 1, CROP, 1, out=data1[n], w_pad=w_pad, c_pad=c_pad, rng=rs)
            e1.feed("labels" + sfx, np.stack([charades.construct_label_array(l) for l in label_lists[it]]))
            bank.sample_frames([0, 1], centers[it], WINDOW, cfg.CHARADES.LFB_CLIPS_PER_SECOND, out=lfb1)
            e1.train_step(lr)
            losses1.append(e1.fetch("loss").reshape(-1)[0])
        torch.cuda.synchronize()
        want_param, want_mom = e1.flat_param.clone(), e1.flat_mom.clone()
        del e1

        m2, e2, _ = _engine(N, T)
        m2.UpdateWorkspaceLr(0)
        loader = FrameLoader(e2, sfx, 1, n_slots=2, max_src_hw=(72, 96), bank=bank, bank_kind="charades", src_sizes=[(72, 96)])
        source = ((videos, label_lists[it], dict(iteration=it, videos=[0, 1], centers=centers[it]), np.random.RandomState(100 * it))
                  for it in range(STEPS))
        loader.start(source)
        losses2 = []
        try:
            for it in range(STEPS):
                loader.deliver(loader.next())              # between steps
                e2.train_step(lr)
                losses2.append(e2.fetch("loss").reshape(-1)[0])
        finally:
            loader.stop()
        torch.cuda.synchronize()
        assert all(np.isfinite(losses1)) and float(e2.blob_tensor("lfb" + sfx)[0].float().abs().max()) > 0
        assert [np.float32(v).tobytes() for v in losses2] == [np.float32(v).tobytes() for v in losses1]
        assert len(set(np.float32(v).tobytes() for v in losses1)) == STEPS
        assert torch.equal(e2.flat_param, want_param) and torch.equal(e2.flat_mom, want_mom)
        assert float(want_mom.abs().sum()) > 0
        assert e2._trace, "steps 2 and 3 replay a recorded step"
        names = [name for _, _, name in e2._trace]
        assert len(names) > 100 and not [n for n in names if n.startswith(("vlfb_clip_", "vlfb_lfb_"))]


def _test_videos():
    """two synthetic Charades videos (frames, per-frame labels)"""
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 256, (40, 72, 96, 3)).astype(np.uint8), rng.integers(0, 256, (23, 72, 96, 3)).astype(np.uint8)]
    labels = [[[int(x) for x in rng.choice(157, int(rng.integers(0, 3)), replace=False)] for _ in range(len(v))] for v in frames]
    return frames, labels


def test_charades_test_order_through_the_loader_and_the_meter():
    """2 videos x 6 test clips (3 shifts x 2 segments) in CharadesIndex order, as frame lists into a store: the merged score
    table and the mAP are those of the same clips preprocessed one by one and fed through Engine.feed, and the three shifts
    of a segment fetch its frames once"""
    import torch
    import utils.metrics as M
    from datasets import charades
    from datasets import data_input_helper as dh
    from datasets.clip_loader import FrameLoader
    from datasets.frame_store import FrameStore
    N, T = 2, 8
    with cases.loader_cfg("charades_r50_baseline", clips=N, frames=T, extra=["TEST.SAMPLE_RATE", 2]) as cfg:
        cfg.CHARADES.NUM_TEST_CLIPS, cfg.TEST.DATASET_SIZE, cfg.LOG_PERIOD = 6, 2, 100
        try:
            frames, frame_labels = _test_videos()
            index = charades.CharadesIndex([[None] * len(v) for v in frames], frame_labels, "test", False)
            assert index.get_db_size() == 12
            batches = [index.get_minibatch_info(list(range(lo, lo + N))) for lo in range(0, 12, N)]
            assert [c.shift for b in batches for c in b] == [0, 0, 1, 1, 2, 2] * 2
            _, eng, sfx = _engine(N, T, train=False)
            data, (w_pad, c_pad) = eng.blob_padded("data" + sfx)
            timer = type("T", (), {"diff": 0.0, "average_time": 0.0})()

            def run(feed):
                mc = M.MetricsCalculator(eng, "test")
                assert mc.meter.n_items == 2 and mc.meter.total_rows == 12
                for it, batch in enumerate(batches):
                    feed(batch)
                    eng.forward()
                    mc.calculate_and_log_all_metrics_test(it, timer, len(batches))
                mc.finalize_metrics()
                torch.cuda.synchronize()
                return mc.meter.table.cpu().numpy().copy(), mc.meter.labels.cpu().numpy().copy(), dict(mc.results)

            def by_hand(batch):
                for n, c in enumerate(batch):
                    dh.images_and_boxes_preprocessing(frames[c.video][np.array(c.seq)], 0, CROP, c.shift, out=data[n], w_pad=w_pad,
                                                      c_pad=c_pad)
                eng.feed("labels" + sfx, np.stack([charades.construct_label_array(c.labels) for c in batch]))
            want_table, want_labels, want = run(by_hand)

            loader = FrameLoader(eng, sfx, 0, n_slots=2, max_src_hw=(72, 96), src_sizes=[(72, 96)])
            store = FrameStore(72, 96, 24, loader.device, loader.stream)
            store.fetch = lambda video, f: frames[video][f]
            loader.start(([(store, c.video, c.seq) for c in b], [c.labels for c in b],
                          dict(iteration=it, videos=[c.video for c in b], centers=[c.center for c in b]), None,
                          [c.shift for c in b]) for it, b in enumerate(batches))
            try:
                got_table, got_labels, got = run(lambda batch: loader.deliver(loader.next()))
            finally:
                loader.stop()
            assert got_table.tobytes() == want_table.tobytes() and np.array_equal(got_labels, want_labels)
            assert float(np.abs(want_table).max()) > 0 and want["rows"] == 2 and want["label_mismatches"] == 0
            assert got["mean_ap"] == want["mean_ap"] and got["rows_seen"] == want["rows_seen"] == 12
            # the three shifts of a segment are the same frames: fetched once
            distinct = len({(c.video, f) for b in batches for c in b for f in c.seq})
            assert store.requested == 12 * T and store.fetched == distinct and distinct <= 4 * T
        finally:
            del cfg.CHARADES["NUM_TEST_CLIPS"]


def test_a_bank_pass_through_the_store_appends_the_bank_of_stacked_frames():
    """one video of 60 frames of 40 x 56, centres every 12 frames, 4 frames at rate 4, lfb_infer_only: (store, video,
    frame_numbers) clips + append_enqueue against stacked frames + append_frames (the 40 x 56 frames are scaled up to the
    64 x 64 crop; at 4 frames the model builds without its res3 non-local block, whose groups divide the pooled time axis)"""
    import torch
    from datasets import charades
    from datasets import data_input_helper as dh
    from datasets.clip_loader import FrameLoader
    from datasets.frame_store import FrameStore
    from vlfb.lfb_bank import DeviceBank
    N, T, RATE, FRAMES = 2, 4, 4, 60
    extra = ["TEST.SAMPLE_RATE", RATE, "NONLOCAL.CONV3_NONLOCAL", False]      # (the grouped res3 block needs 8 frames)
    with cases.loader_cfg("charades_r50_baseline", clips=N, frames=T, extra=extra) as cfg:
        rng = np.random.default_rng(5)
        video = rng.integers(0, 256, (FRAMES, 40, 56, 3)).astype(np.uint8)
        index = charades.CharadesIndex([[None] * FRAMES], [[[]] * FRAMES], "test", True)
        clips = index.get_db_size()
        assert clips == 5 and [c for _, c in index.lfb_frames] == [11, 23, 35, 47, 59]
        batches = [index.get_minibatch_info(list(range(lo, min(lo + N, clips)))) for lo in range(0, clips, N)]
        assert len(batches) == 3 and batches[-1][1] == batches[-1][0]          # the short last batch is padded with its first clip
        sample_freq = cfg.CHARADES.FPS // cfg.CHARADES.LFB_CLIPS_PER_SECOND
        _, eng, sfx = _engine(N, T, train=False, infer_only=True)
        data, (w_pad, c_pad) = eng.blob_padded("data" + sfx)
        pool5, _ = eng.blob_tensor("pool5")
        keys_of = lambda it, b: [(c.video, c.center) for c in b][:clips - it * N]    # (the padding clip is not appended)

        # the existing way: stacked frames, one clip at a time, append_frames (which synchronises)
        bank1 = DeviceBank(1, FRAMES // sample_freq, 1, 2048, "bf16")
        for it, b in enumerate(batches):
            for n, c in enumerate(b):
                dh.images_and_boxes_preprocessing(video[np.array(c.seq)], 0, CROP, c.shift, out=data[n], w_pad=w_pad, c_pad=c_pad)
            eng.forward()
            bank1.append_frames(pool5.view(N, 2048), keys_of(it, b), sample_freq)
        bank1.check_no_drops()

        # frame lists into a store, the keys uploaded in stream order, append_enqueue
        bank2 = DeviceBank(1, FRAMES // sample_freq, 1, 2048, "bf16")
        loader = FrameLoader(eng, sfx, 0, n_slots=2, max_src_hw=(40, 56), src_sizes=[(40, 56)])
        store = FrameStore(40, 56, 12, loader.device, loader.stream)
        store.fetch = lambda v, f: video[f]
        pin_keys = [torch.zeros(N, 2, dtype=torch.int32).pin_memory() for _ in batches]
        dev_keys = torch.zeros(len(batches), N, 2, dtype=torch.int32, device="cuda")
        loader.start(([(store, c.video, c.seq) for c in b], [c.labels for c in b],
                      dict(iteration=it, videos=[c.video for c in b], centers=[c.center for c in b]), None, [c.shift for c in b])
                     for it, b in enumerate(batches))
        try:
            for it, b in enumerate(batches):
                loader.deliver(loader.next())
                eng.forward()
                pin_keys[it].numpy()[:] = bank2.frame_keys(N, keys_of(it, b), sample_freq)
                dev_keys[it].copy_(pin_keys[it], non_blocking=True)
                bank2.append_enqueue(pool5, dev_keys[it], N)
        finally:
            loader.stop()
        torch.cuda.synchronize()
        bank2.check_no_drops()
        assert torch.equal(bank1.count, bank2.count) and bank2.counts().tolist() == [[1] * 5]
        assert np.array_equal(_bits(bank1.bank), _bits(bank2.bank)) and float(bank2.bank.float().abs().max()) > 0
        rows = bank2.bank.view(5, 2048).float()
        assert len({r.cpu().numpy().tobytes() for r in rows}) == 5               # five different clips reached the bank
        seqs = [c.seq for b in batches for c in b]
        distinct = len({f for s in seqs[:clips] for f in s})
        assert store.fetched == distinct == 15 and store.requested == len(seqs) * T == 24


def test_slot_contract_of_the_frame_loader():
    from datasets.clip_loader import FrameLoader
    from datasets.frame_store import FrameStore
    from vlfb import hip
    N, T = 2, 8
    with cases.loader_cfg("epic_verb_r50_baseline", clips=N, frames=T) as cfg:
        cfg.TRAIN.PARAMS_FILE = ""
        _, eng, sfx = _engine(N, T)
        clips = cases.clips(41, sizes=cases.SIZES[:N], frames=T)
        args = lambda k: (clips, [k, k + 1], dict(iteration=k, videos=[0, 1], centers=[10, 20]), np.random.RandomState(k))
        loader = FrameLoader(eng, sfx, 1, n_slots=2, max_src_hw=(90, 96))
        a = loader.submit(*args(0))
        b = loader.submit(*args(1))
        with pytest.raises(hip.VlfbError, match="not delivered"):
            loader.submit(*args(2))
        loader.deliver(a)
        assert eng.input_tensor("labels" + sfx).cpu().numpy().tolist() == [0, 1]
        with pytest.raises(hip.VlfbError, match="no submitted minibatch"):
            loader.deliver(a)
        with pytest.raises(hip.VlfbError, match="either stacked clips or"):
            loader.submit([clips[0], (FrameStore(90, 70, 8, loader.device, loader.stream), 0, [0] * T)], [0, 1],
                          dict(iteration=3, videos=[0, 1], centers=[1, 2]))
        loader.deliver(b)
        t = loader.submit([tuple(clips[0]), list(clips[1])], [3, 4], dict(iteration=4, videos=[0, 1], centers=[1, 2]),
                          np.random.RandomState(4))                # a tuple or a list of T frames is a stacked clip
        loader.deliver(t)
        assert eng.input_tensor("labels" + sfx).cpu().numpy().tolist() == [3, 4]

        def source():
            yield args(5)
            raise ValueError("decoder failed")
        loader.start(source())
        loader.deliver(loader.next())
        with pytest.raises(ValueError, match="decoder failed"):
            loader.next()
        with pytest.raises(ValueError, match="decoder failed"):
            loader.next()
        loader.stop()
        assert loader._thread is None
        loader.stop()
