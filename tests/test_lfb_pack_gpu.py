"""Packed export of the device bank (vlfb_lfb_pack_offsets / vlfb_lfb_pack through the C ABI, and what DeviceBank builds on
them: packed_chunks, to_reference, merge_from, save / load) against host loops over `bank.bank.cpu()` and `bank.counts()`.
Bit-exact: an integer scan and a byte mover (16-bit -> fp32 widening is exact)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TILE = 1024                 # vlfb.h VLFB_LFB_PACK_TILE: cells one workgroup of the scan covers (level 1)
MAX_CELLS = TILE * TILE     # vlfb.h VLFB_LFB_PACK_MAX_CELLS: what the single workgroup of level 2 covers
SENTINEL = 0x5A


def test_the_constants_are_the_library_s():
    from vlfb import hip
    assert (hip.LFB_PACK_TILE, hip.LFB_PACK_MAX_CELLS) == (TILE, MAX_CELLS)


def _bank(n_videos, n_steps, capacity, dim, dtype, seed, fill="random", **kw):
    """a bank whose storage is random everywhere (free slots hold junk that must never be exported) and whose counts are
    `fill`: 'random' (0 .. capacity, empty and full cells included), 'empty', or a host array"""
    from vlfb.lfb_bank import DeviceBank
    bank = DeviceBank(n_videos, n_steps, capacity, dim, dtype, **kw)
    g = torch.Generator().manual_seed(seed)
    bank.bank.copy_(torch.randn(bank.bank.numel(), generator=g).to(bank.bank.dtype))
    rng = np.random.default_rng(seed)
    if isinstance(fill, str):
        cnt = np.zeros(n_videos * n_steps, np.int32)
        if fill == "random":
            cnt = rng.integers(0, capacity + 1, n_videos * n_steps).astype(np.int32)
            cnt[rng.random(cnt.size) < 0.3] = 0
            cnt[rng.random(cnt.size) < 0.2] = capacity
    else:
        cnt = np.asarray(fill, np.int32).reshape(-1)
    bank.count.copy_(torch.as_tensor(cnt))
    return bank


def _bits(t):
    """host integer view of a tensor's elements"""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def _host_pack(bank, out_dtype=None):
    """the host loop: offsets, packed rows (in out_dtype) and keys of a bank, from bank.bank.cpu() and bank.counts()"""
    cnt = np.minimum(bank.counts().reshape(-1), bank.capacity)
    offsets = np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)])
    data = bank.bank.cpu().view(-1, bank.capacity, bank.dim)
    if out_dtype is not None:
        data = data.to(out_dtype)
    mask = np.arange(bank.capacity)[None, :] < cnt[:, None]                      # [cells][slot], cell order then slot order
    rows = _bits(data).reshape(-1, bank.dim)[mask.reshape(-1)]
    cells = np.repeat(np.arange(cnt.size), cnt)
    keys = np.stack([cells // bank.n_steps, cells % bank.n_steps], axis=1).astype(np.int32)
    return offsets, rows, keys


def _offsets(bank):
    from vlfb import hip
    off = torch.full((bank.n_videos * bank.n_steps + 1,), -7, device=bank.device, dtype=torch.int64)
    hip.call("vlfb_lfb_pack_offsets", C.byref(bank.desc), hip.ptr(bank.count), hip.ptr(off))
    return off


def _pack(bank, off, first, rows, out_dtype, alloc=None):
    """one vlfb_lfb_pack call into sentinel-filled buffers of `alloc` rows -> (row bits, keys, untouched-sentinel check)"""
    from vlfb import hip
    alloc = rows if alloc is None else alloc
    out = torch.empty((max(alloc, 1), bank.dim), device=bank.device, dtype=out_dtype)
    out.view(torch.uint8).fill_(SENTINEL)
    keys = torch.full((max(alloc, 1), 2), -9, device=bank.device, dtype=torch.int32)
    hip.call("vlfb_lfb_pack", C.byref(bank.desc), hip.ptr(bank.bank), hip.ptr(bank.count), hip.ptr(off), int(first), int(rows),
             hip.ptr(out), hip.dtype_code(out_dtype), hip.ptr(keys))
    torch.cuda.synchronize()
    return out, keys


def _untouched(out, keys, lo):
    return bool((out[lo:].view(torch.uint8) == SENTINEL).all().item()) and bool((keys[lo:] == -9).all().item())


# one cell; one below / at / one above the level-1 tile; several tiles with a short last one; one below / at the level-2 limit
# (the largest with capacity 1 and dim 8: 16 MiB of bf16)
GEOMETRIES = [(1, 1, 3), (3, 341, 3), (4, 256, 3), (25, 41, 3), (17, 181, 3), (1025, 1023, 1), (1024, 1024, 1)]
assert [v * s for v, s, _ in GEOMETRIES] == [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5, MAX_CELLS - 1, MAX_CELLS]


@pytest.mark.parametrize("n_videos,n_steps,capacity", GEOMETRIES)
def test_offsets_and_full_pack_match_the_host_loop(n_videos, n_steps, capacity):
    bank = _bank(n_videos, n_steps, capacity, 8, "bf16", seed=n_videos)
    want_off, want_rows, want_keys = _host_pack(bank)
    off = _offsets(bank)
    assert np.array_equal(off.cpu().numpy(), want_off)
    total = int(want_off[-1])
    step = (1 << 20) - 1 if total > 4096 else max(1, total // 3 + 1)          # chunks that begin and end inside cells
    got_rows, got_keys = [], []
    for first in range(0, total, step):
        n = min(step, total - first)
        out, keys = _pack(bank, off, first, n, torch.bfloat16)
        got_rows.append(_bits(out)[:n])
        got_keys.append(keys.cpu().numpy()[:n])
    if total:
        assert np.array_equal(np.concatenate(got_rows), want_rows)
        assert np.array_equal(np.concatenate(got_keys), want_keys)


def test_one_cell_above_the_scan_limit_is_rejected():
    from vlfb import hip
    from vlfb.lfb_bank import DeviceBank
    bank = DeviceBank(17, 61681, 1, 8, "bf16")
    assert bank.n_videos * bank.n_steps == MAX_CELLS + 1
    off = torch.zeros(MAX_CELLS + 2, device=bank.device, dtype=torch.int64)
    with pytest.raises(hip.VlfbError, match="cells"):
        hip.call("vlfb_lfb_pack_offsets", C.byref(bank.desc), hip.ptr(bank.count), hip.ptr(off))
    out = torch.zeros((1, 8), device=bank.device, dtype=torch.bfloat16)
    keys = torch.zeros((1, 2), device=bank.device, dtype=torch.int32)
    with pytest.raises(hip.VlfbError, match="cells"):
        hip.call("vlfb_lfb_pack", C.byref(bank.desc), hip.ptr(bank.bank), hip.ptr(bank.count), hip.ptr(off), 0, 1, hip.ptr(out),
                 hip.BF16, hip.ptr(keys))


def test_argument_checks():
    from vlfb import hip
    bank = _bank(2, 3, 2, 8, "fp32", seed=1)
    off = _offsets(bank)
    out = torch.zeros((4, 8), device=bank.device)
    keys = torch.zeros((4, 2), device=bank.device, dtype=torch.int32)
    args = lambda **kw: [kw.get("desc", C.byref(bank.desc)), hip.ptr(bank.bank), hip.ptr(bank.count), kw.get("off", hip.ptr(off)),
                         kw.get("first", 0), kw.get("rows", 4), hip.ptr(out), kw.get("dt", hip.F32), hip.ptr(keys)]
    for bad in (dict(off=None), dict(rows=-1), dict(rows=1 << 20), dict(first=-1), dict(dt=7)):
        with pytest.raises(hip.VlfbError):
            hip.call("vlfb_lfb_pack", *args(**bad))
    with pytest.raises(hip.VlfbError):
        hip.call("vlfb_lfb_pack_offsets", C.byref(bank.desc), None, hip.ptr(off))
    bad_desc = hip.LfbDesc(2, 0, 2, 8, hip.F32, 0)
    with pytest.raises(hip.VlfbError):
        hip.call("vlfb_lfb_pack_offsets", C.byref(bad_desc), hip.ptr(bank.count), hip.ptr(off))
    with pytest.raises(hip.VlfbError):
        hip.call("vlfb_lfb_pack", *args(desc=C.byref(bad_desc)))


TYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.mark.parametrize("dim", [8, 6])                       # 16-byte rows (vector path) / not (scalar path)
@pytest.mark.parametrize("widen", [False, True])              # packed to the bank's own type / to fp32
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_chunk_windows_types_and_row_widths(dtype, widen, dim):
    bank = _bank(5, 7, 3, dim, dtype, seed=11)
    odt = torch.float32 if widen else TYPES[dtype]
    want_off, want_rows, want_keys = _host_pack(bank, odt)
    off = _offsets(bank)
    assert np.array_equal(off.cpu().numpy(), want_off)
    total = int(want_off[-1])
    inside = [int(o) + 1 for o, n in zip(want_off[:-1], np.diff(want_off)) if n >= 3]      # rows strictly inside a cell
    assert len(inside) >= 2 and inside[0] < inside[-1]
    # begins and ends inside a cell; the whole bank; runs past the end; begins at the end; begins beyond it
    for first, rows in ((inside[0], inside[-1] - inside[0]), (0, total), (total - 4, 9), (total, 3), (total + 5, 2)):
        out, keys = _pack(bank, off, first, rows, odt, alloc=rows + 2)
        n = max(0, min(rows, total - first))
        assert np.array_equal(_bits(out)[:n], want_rows[first:first + n])
        assert np.array_equal(keys.cpu().numpy()[:n], want_keys[first:first + n])
        assert _untouched(out, keys, n), "rows at or beyond the bank's total were written"


def test_an_empty_bank_packs_nothing():
    bank = _bank(3, 5, 2, 8, "bf16", seed=2, fill="empty")
    off = _offsets(bank)
    assert not off.cpu().numpy().any()
    out, keys = _pack(bank, off, 0, 6, torch.bfloat16)
    assert _untouched(out, keys, 0)
    assert list(bank.packed_chunks()) == []
    assert bank.to_reference() == {0: {}, 1: {}, 2: {}}


def _same_cells(a, b):
    """equal counts and, for occupied slots, equal bits"""
    ca, cb = a.counts(), b.counts()
    if not np.array_equal(ca, cb):
        return False
    mask = (np.arange(a.capacity)[None, :] < ca.reshape(-1)[:, None]).reshape(-1)
    rows = lambda x: _bits(x.bank).reshape(-1, x.dim)[mask]
    return np.array_equal(rows(a), rows(b))


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_a_packed_chunk_appended_to_an_empty_bank_reproduces_the_cells(dtype):
    from vlfb.lfb_bank import DeviceBank
    bank = _bank(4, 9, 3, 8, dtype, seed=5)
    copy = DeviceBank(4, 9, 3, 8, dtype)
    chunks = 0
    for feats, keys, n in bank.packed_chunks(chunk_rows=7):
        copy.append_enqueue(feats, keys, n)
        chunks += 1
    copy.check_no_drops()
    assert chunks == -(-int(bank.counts().sum()) // 7) and chunks > 2
    assert _same_cells(bank, copy)


def _dense_to_reference(bank, frame_level=False, sample_freq=None):
    """the dense host loop `to_reference` was before it read packed chunks"""
    cnt = bank.counts()
    data = bank.bank.cpu().view(bank.n_videos, bank.n_steps, bank.capacity, bank.dim).float().numpy()
    out = {}
    for vi in range(bank.n_videos):
        key = bank.video_ids[vi] if bank.video_ids is not None else vi
        out[key] = {}
        for s in np.nonzero(cnt[vi])[0]:
            if frame_level:
                out[key][int(sample_freq * (s + 1) - 1)] = data[vi, s, 0].copy()
            else:
                out[key][int(s + bank.step_base)] = [data[vi, s, k].copy() for k in range(cnt[vi, s])]
    return out


def _same_reference(a, b, frame_level=False):
    if list(a) != list(b):
        return False
    for v in a:
        if list(a[v]) != list(b[v]):
            return False
        for s in a[v]:
            xs, ys = ([a[v][s]], [b[v][s]]) if frame_level else (a[v][s], b[v][s])
            if len(xs) != len(ys) or not all(x.dtype == y.dtype == np.float32 and x.shape == y.shape and
                                             np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(xs, ys)):
                return False
    return True


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_to_reference_equals_the_dense_host_loop(dtype):
    bank = _bank(4, 9, 3, 6, dtype, seed=8, step_base=902, video_ids=["c", "a", "d", "b"])
    assert _same_reference(bank.to_reference(chunk_rows=5), _dense_to_reference(bank))
    assert _same_reference(bank.to_reference(), _dense_to_reference(bank))
    frames = _bank(3, 11, 1, 8, dtype, seed=9)
    assert _same_reference(frames.to_reference(frame_level=True, sample_freq=4, chunk_rows=4),
                           _dense_to_reference(frames, True, 4), frame_level=True)


def _lists(bank):
    """{(video key, step): [row bits as fp32, ...]}: the reference's list per cell"""
    ref = _dense_to_reference(bank)
    return {(v, s): [x for x in l] for v in ref for s, l in ref[v].items()}


def test_merge_equals_a_host_replay_of_the_list_appends():
    cnt_a = np.array([[2, 0, 1, 0, 3], [0, 0, 4, 1, 0], [1, 1, 0, 0, 0]])
    cnt_b = np.array([[1, 2, 0, 0, 1], [0, 0, 0, 3, 0], [0, 2, 0, 0, 4]])           # shares (0,0) (0,4) (1,3) (2,1) with a
    a = _bank(3, 5, 4, 8, "fp32", seed=20, fill=cnt_a, step_base=902)
    b = _bank(3, 5, 4, 8, "bf16", seed=21, fill=cnt_b, step_base=902)               # another element type: widened exactly
    want = _lists(a)
    for key, l in _lists(b).items():
        want.setdefault(key, []).extend(l)
    a.merge_from(b)
    got = _lists(a)
    assert sorted(got) == sorted(want)
    for key in want:
        assert len(got[key]) == len(want[key]) and all(np.array_equal(x, y) for x, y in zip(got[key], want[key])), key
    assert np.array_equal(a.counts(), cnt_a + cnt_b)


def test_merge_maps_rows_through_video_ids():
    from vlfb import hip
    a = _bank(3, 4, 3, 8, "bf16", seed=30, fill=[[1, 0, 0, 0], [0, 0, 0, 0], [0, 2, 0, 0]], video_ids=["x", "y", "z"])
    b = _bank(2, 4, 3, 8, "bf16", seed=31, fill=[[0, 1, 0, 2], [1, 0, 0, 0]], video_ids=["z", "x"])
    want = _lists(a)
    for key, l in _lists(b).items():
        want.setdefault(key, []).extend(l)
    a.merge_from(b)
    got = _lists(a)
    assert sorted(got) == sorted(want)
    assert all(np.array_equal(x, y) for key in want for x, y in zip(got[key], want[key]))
    assert np.array_equal(a.counts(), [[2, 0, 0, 0], [0, 0, 0, 0], [0, 3, 0, 2]])
    stranger = _bank(1, 4, 3, 8, "bf16", seed=32, fill=[[1, 0, 0, 0]], video_ids=["w"])
    with pytest.raises(hip.VlfbError, match="not in this bank"):
        a.merge_from(stranger)


def test_a_merge_that_overflows_a_cell_raises():
    from vlfb import hip
    a = _bank(2, 3, 2, 8, "fp32", seed=40, fill=[[2, 0, 1], [0, 0, 0]])
    b = _bank(2, 3, 2, 8, "fp32", seed=41, fill=[[1, 0, 1], [0, 2, 0]])              # (0,0): 2 + 1 > 2
    with pytest.raises(hip.VlfbError, match="did not fit"):
        a.merge_from(b)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_save_then_load_round_trips_in_bits(dtype, tmp_path):
    from vlfb.lfb_bank import DeviceBank
    bank = _bank(4, 9, 3, 8, dtype, seed=50, step_base=902, video_ids=["v3", "v1", "v0", "v2"])
    path = str(tmp_path / "bank.npz")
    bank.save(path)
    with np.load(path) as z:
        assert z["rows"].dtype == (np.float32 if dtype == "fp32" else np.uint16)
        assert z["rows"].shape == (int(bank.counts().sum()), 8)
    back = DeviceBank.load(path)
    assert (back.n_videos, back.n_steps, back.capacity, back.dim, back.code, back.step_base, back.video_ids) == \
        (4, 9, 3, 8, bank.code, 902, ["v3", "v1", "v0", "v2"])
    assert _same_cells(bank, back)
    plain = _bank(2, 3, 2, 8, dtype, seed=51)
    plain.save(path)
    back = DeviceBank.load(path)
    assert back.video_ids is None and _same_cells(plain, back)


def test_to_reference_allocates_a_staging_chunk_not_a_dense_copy():
    """a 64 MiB bf16 bank: the dense fp32 copy the loop used to make is 128 MiB; what may be allocated now is the fp32 staging
    chunk, the offsets and the chunk's keys, plus 1 MiB of allocator slack"""
    n_videos, n_steps, capacity, dim, chunk = 16, 128, 8, 2048, 256
    cnt = np.zeros((n_videos, n_steps), np.int32)
    rng = np.random.default_rng(60)
    cnt.reshape(-1)[rng.choice(cnt.size, 150, replace=False)] = rng.integers(1, capacity + 1, 150)
    bank = _bank(n_videos, n_steps, capacity, dim, "bf16", seed=60, fill=cnt)
    assert bank.bank.numel() * 2 == 64 << 20 and int(cnt.sum()) > 2 * chunk
    cells = n_videos * n_steps
    bound = chunk * dim * 4 + 8 * (cells + 1) + chunk * 8 + (1 << 20)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ref = bank.to_reference(chunk_rows=chunk)
    rise = torch.cuda.max_memory_allocated() - before
    print("to_reference: peak device memory rose by %d bytes (bound %d)" % (rise, bound))
    assert rise <= bound
    assert sum(len(l) for v in ref.values() for l in v.values()) == int(cnt.sum())
    v, s = np.argwhere(cnt > 0)[-1]
    want = bank.bank.view(n_videos, n_steps, capacity, dim)[v, s, cnt[v, s] - 1].float().cpu().numpy()
    assert np.array_equal(ref[int(v)][int(s)][-1], want)
