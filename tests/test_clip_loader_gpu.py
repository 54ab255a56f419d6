"""The minibatch clip loader on the device: vlfb_clip_batch_channel_sums / vlfb_clip_batch_preprocess and
datasets.clip_loader.MinibatchLoader against the per-clip path (datasets.data_input_helper.images_and_boxes_preprocessing
+ Engine.feed), bit for bit -- the per-clip path is already held to the oracle and to the reference's clips
(tests/test_preprocess.py, tests/test_color_aug_gpu.py), so no tolerance is needed here.

Shapes (tests/clip_loader_cases.py): 3 frames, crop 64, jitter 64..80, three clips of different sources.  The tests that go
through an engine use 8 frames: the models do not build for fewer (the non-local groups divide the pooled time axis)."""
import collections
import ctypes as C

import numpy as np
import pytest

import clip_loader_cases as cases

pytestmark = pytest.mark.gpu
SEED = 1            # RandomState(1) draws a flipped and an unflipped clip in every colour mode (asserted below)
GAP = 64            # elements between destinations in the oversized buffer (a multiple of one 4-channel pixel)


def _per_clip(clips, seed, dtype, w_pad, c_pad):
    """the yardstick: N successive per-clip calls on one RandomState"""
    from datasets import data_input_helper as dh
    rng = np.random.RandomState(seed)
    return [dh.images_and_boxes_preprocessing(c, 1, cases.CROP, 1, out_dtype=dtype, w_pad=w_pad, c_pad=c_pad, rng=rng)[0]
            for c in clips]


def _batched(clips, seed, dtype, w_pad, c_pad, shift=0):
    """both entry points over the minibatch, destinations `GAP` apart (+ `shift` elements) inside a zero-filled buffer.
    -> (buffer, [(offset, numel)], plans, colour plans)"""
    import torch
    from datasets import data_input_helper as dh
    from vlfb import hip
    n = len(clips)
    sizes = [c.shape[1:3] for c in clips]
    frames = [c.shape[0] for c in clips]
    plans, colors, _ = dh.plan_minibatch(sizes, 1, cases.CROP, 1, None, np.random.RandomState(seed))
    dev = [torch.as_tensor(c).cuda() for c in clips]
    numel = [f * cases.CROP * (cases.CROP + 2 * w_pad) * c_pad for f in frames]
    offs = [GAP + shift + sum(numel[:i]) + GAP * i for i in range(n)]
    big = torch.zeros(offs[-1] + numel[-1] + GAP, device="cuda", dtype=dtype)
    sums = torch.full((n, max(frames), hip.CLIP_SUM_BANDS, 3), -7, device="cuda", dtype=torch.int64)
    items = (hip.ClipItem * n)()
    need_sums = dh.pack_items(items, plans, colors, frames, sizes, cases.CROP, [d.data_ptr() for d in dev],
                              [big.data_ptr() + o * big.element_size() for o in offs],
                              [sums[i].data_ptr() for i in range(n)], w_pad, c_pad, "cuda:0")
    assert need_sums == any(c is not None and 1 in c["ops"] for c in colors)
    items_dev = torch.as_tensor(np.frombuffer(items, dtype=np.uint8).copy()).cuda()
    host = C.cast(items, C.c_void_p)
    if need_sums:
        hip.call("vlfb_clip_batch_channel_sums", host, hip.ptr(items_dev), n)
    hip.call("vlfb_clip_batch_preprocess", host, hip.ptr(items_dev), n, hip.dtype_code(dtype))
    torch.cuda.synchronize()
    return big, list(zip(offs, numel)), plans, colors


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).cpu().numpy().reshape(-1)


def _assert_same(big, spans, want, w_pad):
    got = _bits(big)
    outside = np.ones(got.size, dtype=bool)
    for (o, k), w in zip(spans, want):
        assert w.numel() == k
        assert np.array_equal(got[o:o + k], _bits(w))
        outside[o:o + k] = False
        assert float(w.float().abs().max()) > 0
        if w_pad:
            rows = got[o:o + k].reshape(-1, cases.CROP + 2 * w_pad, w.shape[-1])
            assert not rows[:, :w_pad].any() and not rows[:, w_pad + cases.CROP:].any()      # W-padding is never written
        if w.shape[-1] == 4:
            assert not got[o:o + k].reshape(-1, 4)[:, 3].any()                               # the padding channel is zero
    assert not got[outside].any()                                                            # nothing outside the destinations


@pytest.mark.parametrize("mode", list(cases.COLOR_MODES))
@pytest.mark.parametrize("pad", [(4, 4), (0, 3)], ids=["w4c4", "w0c3"])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_batched_kernels_are_the_per_clip_kernels_bit_for_bit(dtype, pad, mode):
    import torch
    dtype = getattr(torch, dtype)
    clips = cases.clips(0)
    with cases.loader_cfg(**cases.COLOR_MODES[mode]):
        big, spans, plans, colors = _batched(clips, SEED, dtype, *pad)
        assert {p["flip"] for p in plans} == {0, 1}, "the minibatch must hold a flipped and an unflipped clip"
        assert len({(p["resized_h"], p["resized_w"]) for p in plans}) == 3
        if mode == "all":
            assert all(sorted(c["ops"]) == [0, 1, 2] for c in colors)
        if mode == "light":
            assert all(c["ops"] == [] and any(c["light"]) for c in colors)
        _assert_same(big, spans, _per_clip(clips, SEED, dtype, *pad), pad[0])


@pytest.mark.parametrize("mode", ["off", "all"])
def test_batched_kernels_with_a_clip_that_needs_no_resize(mode):
    """JITTER_SCALES [64, 64]: the 64 x 88 clip is used as it is (its item carries no tables), the others are resized"""
    import torch
    clips = cases.clips(1)
    with cases.loader_cfg(jitter=(64, 64), **cases.COLOR_MODES[mode]):
        big, spans, plans, _ = _batched(clips, SEED, torch.float32, 4, 4)
        assert [(p["resized_h"], p["resized_w"]) for p in plans] == [(64, 85), (82, 64), (64, 88)]
        _assert_same(big, spans, _per_clip(clips, SEED, torch.float32, 4, 4), 4)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_items_of_different_frame_counts(dtype):
    """3 and 2 frames in one launch: the workgroups of frame 2 of the shorter clip return"""
    import torch
    dtype = getattr(torch, dtype)
    clips = cases.clips(2, frames=[3, 2, 3])
    with cases.loader_cfg(color=True):
        big, spans, _, _ = _batched(clips, SEED, dtype, 4, 4)
        assert spans[1][1] * 3 == spans[0][1] * 2
        _assert_same(big, spans, _per_clip(clips, SEED, dtype, 4, 4), 4)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_a_destination_not_aligned_to_a_pixel_takes_the_scalar_stores(dtype):
    import torch
    dtype = getattr(torch, dtype)
    clips = cases.clips(3)
    with cases.loader_cfg(color=True):
        big, spans, _, _ = _batched(clips, SEED, dtype, 4, 4, shift=1)
        assert all(o % 4 == 1 for o, _ in spans)
        _assert_same(big, spans, _per_clip(clips, SEED, dtype, 4, 4), 4)


# ---- the loader ----------------------------------------------------------------------------------

def _engine(n, rois, frames=8, dtype="bf16"):
    """a planned engine for the loaded cfg in the small setup of tests/test_train_loop_gpu.py (8 frames, crop 64) with synthetic parameters"""
    from core.config import config as cfg
    from models.model_builder_video import ModelBuilder
    from vlfb.engine import Engine
    from vlfb import synth
    m = ModelBuilder(train=True, split="train", name="train")
    m.build_model(suffix="_train")
    eng = Engine(m, dtype, device="cuda:0", base_seed=2)
    k = cfg.LFB.WINDOW_SIZE * cfg.AVA.LFB_MAX_NUM_FEAT_PER_STEP
    shapes = {"data_train": (n, 3, frames, cases.CROP, cases.CROP), "labels_train": (rois, cfg.MODEL.NUM_CLASSES),
              "proposals_train": (rois, 5), "lfb_train": (rois, k, 2048)}
    eng.plan(collections.OrderedDict((name, shapes[name]) for name in m.input_blob_names))
    eng.feed_params(synth.params(m, seed=2))
    return m, eng


def test_six_minibatches_through_two_slots():
    """every minibatch arrives in the engine's data blob as the per-clip path computes it: a slot overwritten before it was
    consumed, or delivered stale, is a mismatch.  Ragged RoI rows (2 + 0 + 3 on a 6-row plan) arrive padded."""
    import torch
    from datasets.clip_loader import MinibatchLoader
    from vlfb import hip
    nbox, rows = [2, 0, 3], 6
    with cases.loader_cfg("ava_r50_baseline", clips=3, frames=8, color=True) as cfg:
        _, eng = _engine(3, rows)
        classes = cfg.MODEL.NUM_CLASSES
        batches = []
        for k in range(6):
            rng = np.random.default_rng(50 + k)
            labels = [(rng.uniform(size=(b, classes)) < 0.1).astype(np.int32) for b in nbox]
            batches.append((cases.clips(10 + k, frames=8), cases.boxes(k, nbox), labels,
                            dict(iteration=k, videos=[0, 1, 2], secs=[905, 906, 907]), np.random.RandomState(200 + k)))
        data, (w_pad, c_pad) = eng.blob_padded("data_train")
        want = [torch.stack(_per_clip(b[0], 200 + k, data.dtype, w_pad, c_pad)).clone() for k, b in enumerate(batches)]
        assert len({tuple(_bits(w)[:4096]) for w in want}) == 6
        loader = MinibatchLoader(eng, "_train", 1, n_slots=2, max_src_hw=(90, 96), src_sizes=cases.SIZES)
        loader.start(iter(batches))
        try:
            seen = []
            for k in range(6):
                slot = loader.next()
                seen.append(slot.index)
                loader.deliver(slot)
                assert np.array_equal(_bits(data), _bits(want[k])), "minibatch %d" % k      # (.cpu() waits for the stream)
                props = eng.input_tensor("proposals_train").cpu().numpy().reshape(rows, 5)
                labels = eng.input_tensor("labels_train").cpu().numpy().reshape(rows, classes)
                assert np.array_equal(props, slot.proposals) and np.array_equal(labels, slot.labels)
                assert list(props[:, 0]) == [0, 0, 2, 2, 2, 0] and not props[5].any() and np.all(labels[5] == -1)
                assert np.array_equal(labels[:5], np.concatenate(batches[k][2]))
                assert slot.used == 5 and slot.metadata.shape == (5, 4) and list(slot.metadata[2]) == [2, 907, 64, 88]
                assert slot.original_boxes.shape == (5, 5)
            assert seen == [0, 1, 0, 1, 0, 1]
            with pytest.raises(StopIteration):
                loader.next()
        finally:
            loader.stop()
        # a third submit before anything was delivered must not overwrite: it raises
        again = lambda k: batches[k][:4] + (np.random.RandomState(200 + k),)
        a = loader.submit(*again(0))
        loader.submit(*again(1))
        with pytest.raises(hip.VlfbError, match="not delivered"):
            loader.submit(*again(2))
        loader.deliver(a)
        assert np.array_equal(_bits(data), _bits(want[0]))
        with pytest.raises(hip.VlfbError, match="no submitted minibatch"):
            loader.deliver(a)
        with pytest.raises(KeyError):
            eng.input_tensor("pred")
        torch.cuda.synchronize()


@pytest.mark.parametrize("color", [False, True], ids=["plain", "color"])
def test_three_train_steps_fed_by_the_loader_equal_three_fed_the_existing_way(color):
    """ava_r50_lfb_nl, 8 frames, crop 64, 2 clips, bf16, with a bank: losses and parameters are bit-identical, and the
    recorded step holds no clip call"""
    import torch
    from datasets import data_input_helper as dh
    from datasets.clip_loader import MinibatchLoader
    from vlfb.lfb_bank import DeviceBank
    N, R, STEPS = 2, 4, 3
    with cases.loader_cfg("ava_r50_lfb_nl", clips=N, frames=8, color=color, extra=["LFB.WINDOW_SIZE", 4]) as cfg:
        cfg.TRAIN.PARAMS_FILE = ""
        rng = np.random.default_rng(0)
        videos = [rng.integers(0, 256, (8, 72, 96, 3)).astype(np.uint8) for _ in range(N)]
        boxes01 = [np.array([[0.1, 0.1, 0.6, 0.9], [0.3, 0.2, 0.95, 0.8]]) for _ in range(N)]
        labels = (rng.uniform(size=(R, cfg.MODEL.NUM_CLASSES)) < 0.05).astype(np.int32)
        bank = DeviceBank(N, 8, 4, 2048, "bf16", step_base=902)
        feats = torch.as_tensor(rng.standard_normal((2 * R, 2048)).astype(np.float32))
        bank.append(feats, np.arange(2 * R) % N, 903 + (np.arange(2 * R) % 4))
        bank.check_no_drops()
        window, per_step = cfg.LFB.WINDOW_SIZE, cfg.AVA.LFB_MAX_NUM_FEAT_PER_STEP

        # the existing way (tests/test_train_loop_gpu.py): per-clip preprocessing into the blob, feed, sample_window
        m1, e1 = _engine(N, R)
        data1, (w_pad, c_pad) = e1.blob_padded("data_train")
        lfb1, _ = e1.blob_tensor("lfb_train")
        m1.UpdateWorkspaceLr(0)
        lr = float(m1.current_lr)
        losses1 = []
        for it in range(STEPS):
            rs = np.random.RandomState(100 * it)
            rois = []
            for n in range(N):
                _, b = dh.images_and_boxes_preprocessing(videos[n], 1, cases.CROP, 1, boxes01[n].copy(), out=data1[n],
                                                         w_pad=w_pad, c_pad=c_pad, rng=rs)
                rois.append(np.concatenate([np.full((len(b), 1), n), b], axis=1))
            props = np.concatenate(rois).astype(np.float32)
            e1.feed("proposals_train", props)
            e1.feed("labels_train", labels)
            clip_of = props[:, 0].astype(np.int64)
            bank.sample_window(clip_of, np.full(R, 905), it * N + clip_of, window, per_step, seed=cfg.RNG_SEED, out=lfb1)
            e1.train_step(lr)
            losses1.append(e1.fetch("loss").reshape(-1)[0])
        want = {n: e1.fetch_param(n) for n in ("pred_w", "conv1_w")}
        del e1

        # the loader: a background thread prepares the next minibatch while a step runs
        m2, e2 = _engine(N, R)
        m2.UpdateWorkspaceLr(0)
        loader = MinibatchLoader(e2, "_train", 1, n_slots=2, max_src_hw=(72, 96), bank=bank, src_sizes=[(72, 96)])
        source = ((videos, boxes01, [labels[:2], labels[2:]], dict(iteration=it, videos=[0, 1], secs=[905, 905]),
                   np.random.RandomState(100 * it)) for it in range(STEPS))
        loader.start(source)
        losses2 = []
        try:
            for it in range(STEPS):
                loader.deliver(loader.next())              # between steps
                e2.train_step(lr)
                losses2.append(e2.fetch("loss").reshape(-1)[0])
        finally:
            loader.stop()
        assert all(np.isfinite(losses1)) and float(e2.blob_tensor("lfb_train")[0].float().abs().max()) > 0
        assert [np.float32(v).tobytes() for v in losses2] == [np.float32(v).tobytes() for v in losses1]
        assert len(set(np.float32(v).tobytes() for v in losses1)) == STEPS
        for n, v in want.items():
            assert np.array_equal(e2.fetch_param(n).view(np.uint32), v.view(np.uint32)), n
        # the step recorder saw neither the loader thread nor deliver
        assert e2._trace, "steps 2 and 3 replay a recorded step"
        names = [name for _, _, name in e2._trace]
        assert len(names) > 100 and not [n for n in names if n.startswith("vlfb_clip_")]
        torch.cuda.synchronize()


def test_an_exception_in_the_source_is_raised_by_next_and_stop_returns():
    from datasets.clip_loader import MinibatchLoader
    with cases.loader_cfg("ava_r50_baseline", clips=3, frames=8) as cfg:
        _, eng = _engine(3, 6)
        classes = cfg.MODEL.NUM_CLASSES

        def source():
            yield (cases.clips(0, frames=8), cases.boxes(0, [1, 1, 1]), [np.zeros((1, classes), np.int32)] * 3,
                   dict(iteration=0, videos=[0, 1, 2], secs=[905] * 3), np.random.RandomState(0))
            raise ValueError("decoder failed")

        loader = MinibatchLoader(eng, "_train", 1, n_slots=2, max_src_hw=(90, 96))
        loader.start(source())
        loader.deliver(loader.next())
        with pytest.raises(ValueError, match="decoder failed"):
            loader.next()
        with pytest.raises(ValueError, match="decoder failed"):
            loader.next()
        loader.stop()
        assert loader._thread is None
        loader.stop()
