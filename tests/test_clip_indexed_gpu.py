"""vlfb_clip_batch_preprocess_indexed / vlfb_clip_batch_channel_sums_indexed: clips given as frame lists into a frame store.

The yardstick is the contiguous batched entry points (held to the per-clip kernels bit for bit in
tests/test_clip_loader_gpu.py) run on store[index] gathered on the host: the same device functions and the same arithmetic,
so output and channel sums are compared bit for bit, no tolerance.

Shapes (tests/clip_loader_cases.py): three sources (72 x 96, 90 x 70, 64 x 88), stores of 7 frames, clips of 3 frames, crop
64, jitter 64..80 -- more than one tile per row and column, a flipped and an unflipped clip, three resize geometries."""
import ctypes as C

import numpy as np
import pytest

import clip_loader_cases as cases

pytestmark = pytest.mark.gpu
SEED = 1            # RandomState(1) draws a flipped and an unflipped clip in every colour mode (tests/test_clip_loader_gpu.py)
STORE = 7
SENTINEL = -7

# item i of the minibatch reads TABLES[name][i]
TABLES = {
    "identity": [[0, 1, 2]] * 3,
    "clamped": [[0, 0, 6]] * 3,                       # a sequence clamped at the video's start repeats a frame
    "descending": [[5, 3, 1]] * 3,
    "mixed": [[0, 1, 2], [6, 6, 0], [5, 3, 1]],       # every item its own row of the table
}


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).cpu().numpy().reshape(-1)


def _launch(frame_tensors, frames, plans, colors, sizes, dtype, w_pad, c_pad, table=None, stride=None, store_frames=None,
            fill=0.0):
    """one minibatch through the batched entry points -- indexed when `table` (n, stride) is given -- into a buffer filled
    with `fill`.  -> (destination buffer, sums)"""
    import torch
    from datasets import data_input_helper as dh
    from vlfb import hip
    n = len(frame_tensors)
    numel = [f * cases.CROP * (cases.CROP + 2 * w_pad) * c_pad for f in frames]
    offs = [sum(numel[:i]) for i in range(n)]
    big = torch.full((sum(numel),), fill, device="cuda", dtype=dtype)
    sums = torch.full((n, max(frames), hip.CLIP_SUM_BANDS, 3), SENTINEL, device="cuda", dtype=torch.int64)
    items = (hip.ClipItem * n)()
    need_sums = dh.pack_items(items, plans, colors, frames, sizes, cases.CROP, [t.data_ptr() for t in frame_tensors],
                              [big.data_ptr() + o * big.element_size() for o in offs],
                              [sums[i].data_ptr() for i in range(n)], w_pad, c_pad, "cuda:0")
    items_dev = torch.as_tensor(np.frombuffer(items, dtype=np.uint8).copy()).cuda()
    host = C.cast(items, C.c_void_p)
    code = hip.dtype_code(dtype)
    if table is None:
        if need_sums:
            hip.call("vlfb_clip_batch_channel_sums", host, hip.ptr(items_dev), n)
        hip.call("vlfb_clip_batch_preprocess", host, hip.ptr(items_dev), n, code)
    else:
        table = np.ascontiguousarray(table, dtype=np.int32)
        assert table.shape == (n, stride)
        table_dev = torch.as_tensor(table).cuda()
        counts = np.ascontiguousarray(store_frames, dtype=np.int32)
        args = (host, hip.ptr(items_dev), n, table.ctypes.data, hip.ptr(table_dev), stride, counts.ctypes.data)
        try:
            if need_sums:
                hip.call("vlfb_clip_batch_channel_sums_indexed", *args)
            hip.call("vlfb_clip_batch_preprocess_indexed", *(args + (code,)))
        finally:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    return big, sums


def _plans(sizes):
    from datasets import data_input_helper as dh
    plans, colors, _ = dh.plan_minibatch(sizes, 1, cases.CROP, 1, None, np.random.RandomState(SEED))
    return plans, colors


@pytest.mark.parametrize("mode", list(cases.COLOR_MODES))
@pytest.mark.parametrize("pad", [(4, 4), (0, 3)], ids=["w4c4", "w0c3"])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_indexed_kernels_are_the_contiguous_kernels_on_the_gathered_frames(dtype, pad, mode):
    import torch
    dtype = getattr(torch, dtype)
    stores = cases.clips(20, frames=STORE)
    stores_dev = [torch.as_tensor(s).cuda() for s in stores]
    with cases.loader_cfg(**cases.COLOR_MODES[mode]):
        plans, colors = _plans(cases.SIZES)
        assert {p["flip"] for p in plans} == {0, 1} and len({(p["resized_h"], p["resized_w"]) for p in plans}) == 3
        if mode == "all":
            assert all(1 in c["ops"] for c in colors)                      # the sums launch runs
        for name, table in TABLES.items():
            got, got_sums = _launch(stores_dev, [cases.T] * 3, plans, colors, cases.SIZES, dtype, *pad,
                                    table=table, stride=cases.T, store_frames=[STORE] * 3)
            gathered = [torch.as_tensor(np.ascontiguousarray(s[np.array(row)])).cuda() for s, row in zip(stores, table)]
            want, want_sums = _launch(gathered, [cases.T] * 3, plans, colors, cases.SIZES, dtype, *pad)
            assert np.array_equal(_bits(got), _bits(want)), name
            assert float(want.float().abs().max()) > 0
            assert torch.equal(got_sums, want_sums), name
            assert bool((want_sums != SENTINEL).any()) == (mode == "all")
            if name == "identity":                                         # ... and the contiguous call on the store itself
                same, same_sums = _launch(stores_dev, [cases.T] * 3, plans, colors, cases.SIZES, dtype, *pad)
                assert np.array_equal(_bits(got), _bits(same)) and torch.equal(got_sums, same_sums)
            if name == "clamped":                                          # frames 0 and 1 of a clip are one source frame
                per = got.numel() // 3 // cases.T
                assert np.array_equal(_bits(got[:per]), _bits(got[per:2 * per]))
                assert not np.array_equal(_bits(got[:per]), _bits(got[2 * per:3 * per]))


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_items_of_different_frame_counts_under_one_stride(dtype):
    """3, 2 and 3 frames, stride 4: the workgroups of frame 2 of the shorter clip return, and entries past an item's frames
    are neither checked nor read"""
    import torch
    dtype = getattr(torch, dtype)
    stores = cases.clips(21, frames=STORE)
    stores_dev = [torch.as_tensor(s).cuda() for s in stores]
    frames = [3, 2, 3]
    table = [[6, 2, 4, 99], [1, 1, -5, 99], [0, 5, 3, -1]]
    with cases.loader_cfg(color=True):
        plans, colors = _plans(cases.SIZES)
        got, got_sums = _launch(stores_dev, frames, plans, colors, cases.SIZES, dtype, 4, 4, table=table, stride=4,
                                store_frames=[STORE] * 3)
        gathered = [torch.as_tensor(np.ascontiguousarray(s[np.array(row[:f])])).cuda() for s, row, f in zip(stores, table, frames)]
        want, want_sums = _launch(gathered, frames, plans, colors, cases.SIZES, dtype, 4, 4)
        assert np.array_equal(_bits(got), _bits(want)) and torch.equal(got_sums, want_sums)
        assert bool((got_sums[1, 2] == SENTINEL).all()) and bool((got_sums[1, :2] != SENTINEL).any())


@pytest.mark.parametrize("bad", ["negative", "past_the_store", "stride"])
def test_a_bad_table_is_rejected_before_anything_is_launched(bad):
    import torch
    from vlfb import hip
    stores_dev = [torch.as_tensor(s).cuda() for s in cases.clips(22, frames=STORE)]
    table, stride, match = [[0, 1, 2], [3, 4, 5], [6, 5, 4]], cases.T, None
    if bad == "negative":
        table[1][2], match = -1, "item 1 entry 2"
    elif bad == "past_the_store":
        table[2][0], match = STORE, "item 2 entry 0"
    else:
        table, stride, match = [r[:2] for r in table], 2, "item 0 has 3 frames, index_stride is 2"
    # the destinations of a refused call are untouched: sentinel-filled buffers, written by nothing
    from datasets import data_input_helper as dh
    n, numel = 3, cases.T * cases.CROP * (cases.CROP + 8) * 4
    big = torch.full((n * numel,), float(SENTINEL), device="cuda")
    sums = torch.full((n, cases.T, hip.CLIP_SUM_BANDS, 3), SENTINEL, device="cuda", dtype=torch.int64)
    with cases.loader_cfg(color=True):
        plans, colors = _plans(cases.SIZES)
        assert any(1 in c["ops"] for c in colors)                          # (a valid table would reach both launches)
        items = (hip.ClipItem * n)()
        dh.pack_items(items, plans, colors, [cases.T] * n, cases.SIZES, cases.CROP, [t.data_ptr() for t in stores_dev],
                      [big.data_ptr() + i * numel * 4 for i in range(n)], [sums[i].data_ptr() for i in range(n)], 4, 4, "cuda:0")
    items_dev = torch.as_tensor(np.frombuffer(items, dtype=np.uint8).copy()).cuda()
    t = np.ascontiguousarray(table, dtype=np.int32)
    t_dev = torch.as_tensor(t).cuda()
    counts = np.full(n, STORE, dtype=np.int32)
    args = (C.cast(items, C.c_void_p), hip.ptr(items_dev), n, t.ctypes.data, hip.ptr(t_dev), stride, counts.ctypes.data)
    with pytest.raises(hip.VlfbError, match=match):
        hip.call("vlfb_clip_batch_channel_sums_indexed", *args)
    with pytest.raises(hip.VlfbError, match=match):
        hip.call("vlfb_clip_batch_preprocess_indexed", *(args + (hip.F32,)))
    torch.cuda.synchronize()
    assert bool((big == float(SENTINEL)).all()) and bool((sums == SENTINEL).all())
