"""Packed import of the device bank (vlfb_lfb_unpack / vlfb_lfb_unpack_commit through DeviceBank.unpack_enqueue /
unpack_commit): a source bank's packed rows placed into a destination bank without keys.  Bit-exact against
DeviceBank.merge_from on a copy of the destination (the keyed append path) and against a numpy restatement of the placement
rule, for every chunking of the source.  Conversions are kept exact (same type, or a 16-bit source into an fp32 bank), so
no tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TILE = 1024                 # vlfb.h VLFB_LFB_PACK_TILE
MAX_CELLS = TILE * TILE     # vlfb.h VLFB_LFB_PACK_MAX_CELLS
TYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
CHUNKS = (1, 7, 65536)      # one row per call; 7: cells straddle calls; the whole source in one call

# n_videos=3, n_steps=5, capacity=4.  DST / SRC_FIT: cells empty in both (0,0) (1,1) (1,2) (1,4) (2,3); only in the
# destination (0,1) (0,3); only in the source (0,2) (2,4); shared cells that fit (0,4) (1,0) (1,3) (2,1) (2,2); the source's
# last cell (2,4) is full.  SRC_OVER: as SRC_FIT, plus rows that overflow (0,1) by 1, (0,3) by 3 and (1,0) by 2.
GEOM = (3, 5, 4)
DST = [[0, 2, 0, 4, 1], [3, 0, 0, 1, 0], [0, 1, 2, 0, 0]]
SRC_FIT = [[0, 0, 3, 0, 2], [1, 0, 0, 2, 0], [0, 2, 1, 0, 4]]
SRC_OVER = [[0, 3, 3, 3, 2], [3, 0, 0, 2, 0], [0, 2, 1, 0, 4]]
SRC_EMPTY = [[0] * 5] * 3


def _filled(n_videos, n_steps, capacity, dim, dtype, counts, seed):
    """a bank with junk in every slot, then `counts` rows per cell appended in a random interleaving of the cells"""
    from vlfb.lfb_bank import DeviceBank
    bank = DeviceBank(n_videos, n_steps, capacity, dim, dtype)
    g = torch.Generator().manual_seed(seed)
    bank.bank.copy_(torch.randn(bank.bank.numel(), generator=g).to(bank.bank.dtype))
    cnt = np.asarray(counts, np.int64).reshape(-1)
    cells = np.repeat(np.arange(cnt.size), cnt)
    rng = np.random.default_rng(seed)
    rng.shuffle(cells)
    if cells.size:
        feats = rng.standard_normal((cells.size, dim)).astype(np.float32)
        bank.append(feats, cells // n_steps, cells % n_steps)
    bank.check_no_drops()
    assert np.array_equal(bank.counts().reshape(-1), cnt)
    return bank


def _copy(bank):
    from vlfb.lfb_bank import DeviceBank
    c = DeviceBank(bank.n_videos, bank.n_steps, bank.capacity, bank.dim, bank.bank.dtype)
    c.bank.copy_(bank.bank)
    c.count.copy_(bank.count)
    return c


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16).numpy()


def _occupied(bank):
    """(counts, bits of the occupied slots in cell / slot order)"""
    cnt = bank.counts().reshape(-1)
    mask = (np.arange(bank.capacity)[None, :] < np.minimum(cnt, bank.capacity)[:, None]).reshape(-1)
    return cnt, _bits(bank.bank).reshape(-1, bank.dim)[mask]


def _restated(dst, src):
    """the placement rule on the host: row s of cell c of the source -> slot count[c] + s, dropped at or past the
    capacity; count = min(count + min(src_count, src_capacity), capacity) -> (counts, occupied bits, dropped)"""
    cd, cs = dst.counts().reshape(-1).astype(np.int64), src.counts().reshape(-1).astype(np.int64)
    out = dst.bank.cpu().view(-1, dst.capacity, dst.dim).clone()
    rows = src.bank.cpu().view(-1, src.capacity, src.dim).to(dst.bank.dtype)
    dropped = 0
    for c in range(cd.size):
        for s in range(min(int(cs[c]), src.capacity)):
            slot = int(cd[c]) + s
            if slot < dst.capacity:
                out[c, slot] = rows[c, s]
            else:
                dropped += 1
    cnt = np.minimum(cd + np.minimum(cs, src.capacity), dst.capacity)
    mask = (np.arange(dst.capacity)[None, :] < cnt[:, None]).reshape(-1)
    return cnt, _bits(out).reshape(-1, dst.dim)[mask], dropped


def _unpacked(dst, src, chunk):
    """a copy of `dst` with `src` placed in chunks of `chunk` packed rows, then committed once"""
    got = _copy(dst)
    off = src.pack_offsets()
    first = 0
    for feats, _, n in src.packed_chunks(chunk):
        got.unpack_enqueue(feats, src.count, off, first, n, src_capacity=src.capacity)
        first += n
    assert first == int(src.counts().sum())
    got.unpack_commit(src.count, src.capacity)
    torch.cuda.synchronize()
    return got


# (dim, destination type, source type, source counts): dim 8 = 16-byte rows in 16-bit types (vector path), 20 = 40-byte
# rows in 16-bit types (scalar path), 2048 = the product's rows; a mixed pair converts on the scalar path
CASES = [
    (8, "bf16", "bf16", SRC_FIT),
    (20, "bf16", "bf16", SRC_FIT),
    (2048, "bf16", "bf16", SRC_OVER),
    (8, "fp32", "bf16", SRC_OVER),
    (20, "fp16", "fp16", SRC_OVER),
    (20, "fp32", "fp16", SRC_FIT),
    (2048, "fp32", "bf16", SRC_FIT),
    (2048, "fp16", "fp16", SRC_FIT),
    (8, "fp16", "fp16", SRC_EMPTY),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_unpack_equals_merge_from_and_the_restatement_for_every_chunking(case):
    from vlfb import hip
    dim, ddt, sdt, src_counts = CASES[case]
    dst = _filled(*GEOM, dim, ddt, DST, seed=100 + case)
    src = _filled(*GEOM, dim, sdt, src_counts, seed=200 + case)
    want_cnt, want_rows, want_dropped = _restated(dst, src)
    print("case %d: %d source rows, %d over capacity" % (case, int(src.counts().sum()), want_dropped))
    assert (want_dropped > 0) == (src_counts is SRC_OVER)

    merged = _copy(dst)
    if want_dropped:
        with pytest.raises(hip.VlfbError, match="did not fit"):
            merged.merge_from(src)
    else:
        merged.merge_from(src)
    m_cnt, m_rows = _occupied(merged)
    assert np.array_equal(m_cnt, want_cnt) and np.array_equal(m_rows, want_rows)
    assert int(merged.dropped.item()) == want_dropped

    for chunk in CHUNKS:
        got = _unpacked(dst, src, chunk)
        g_cnt, g_rows = _occupied(got)
        assert np.array_equal(g_cnt, want_cnt), chunk
        assert np.array_equal(g_rows, want_rows), chunk
        assert int(got.dropped.item()) == want_dropped, chunk
        if want_dropped:
            with pytest.raises(hip.VlfbError, match="%d features did not fit" % want_dropped):
                got.check_no_drops()
        else:
            got.check_no_drops()


def test_cells_across_a_scan_tile():
    """cells = VLFB_LFB_PACK_TILE + 3: the source's offsets cross the scan's tile; rows on both sides of it"""
    n_videos = TILE + 3
    rng = np.random.default_rng(7)
    d = (rng.random(n_videos) < 0.4).astype(np.int32)
    s = ((rng.random(n_videos) < 0.5) & (d == 0)).astype(np.int32)
    d[TILE - 2:] = [1, 0, 0, 1, 0]
    s[TILE - 2:] = [0, 1, 1, 0, 1]
    dst = _filled(n_videos, 1, 1, 8, "bf16", d.reshape(-1, 1), seed=300)
    src = _filled(n_videos, 1, 1, 8, "bf16", s.reshape(-1, 1), seed=301)
    want_cnt, want_rows, want_dropped = _restated(dst, src)
    assert want_dropped == 0 and int(s[:TILE].sum()) > 0 and int(s[TILE:].sum()) > 0
    merged = _copy(dst)
    merged.merge_from(src)
    assert np.array_equal(_occupied(merged)[0], want_cnt) and np.array_equal(_occupied(merged)[1], want_rows)
    for chunk in CHUNKS:
        got = _unpacked(dst, src, chunk)
        g_cnt, g_rows = _occupied(got)
        assert np.array_equal(g_cnt, want_cnt) and np.array_equal(g_rows, want_rows), chunk
        got.check_no_drops()


def test_the_commit_publishes_a_source_once():
    """the commit is once per source: a second one counts the source's rows twice, and the restatement sees it"""
    dst = _filled(*GEOM, 8, "bf16", DST, seed=400)
    src = _filled(*GEOM, 8, "bf16", SRC_FIT, seed=401)
    want_cnt, want_rows, _ = _restated(dst, src)
    got = _unpacked(dst, src, 7)
    assert np.array_equal(got.counts().reshape(-1), want_cnt)
    got.unpack_commit(src.count, src.capacity)
    twice = got.counts().reshape(-1)
    assert not np.array_equal(twice, want_cnt)
    cs = src.counts().reshape(-1)
    assert np.array_equal(twice, np.minimum(want_cnt + cs, got.capacity))


def test_argument_checks_need_no_kernel():
    from vlfb import hip
    from vlfb.lfb_bank import DeviceBank
    dst = _filled(*GEOM, 8, "fp32", DST, seed=500)
    src = _filled(*GEOM, 8, "fp32", SRC_FIT, seed=501)
    off = src.pack_offsets()
    feats = torch.zeros((4, 8), device=dst.device)

    def unpack(**kw):
        hip.call("vlfb_lfb_unpack", kw.get("desc", C.byref(dst.desc)), hip.ptr(dst.bank), hip.ptr(dst.count), hip.ptr(feats),
                 kw.get("dt", hip.F32), hip.ptr(src.count), kw.get("cap", src.capacity), kw.get("off", hip.ptr(off)),
                 kw.get("first", 0), kw.get("rows", 4), hip.ptr(dst.dropped))
    unpack()
    for bad, what in ((dict(rows=1 << 20), "rows"), (dict(rows=-1), "rows"), (dict(first=-1), "first_row"),
                      (dict(off=None), "NULL"), (dict(dt=7), "dtype"), (dict(cap=0), "src_capacity")):
        with pytest.raises(hip.VlfbError, match=what):
            unpack(**bad)
    with pytest.raises(hip.VlfbError, match="src_capacity"):
        hip.call("vlfb_lfb_unpack_commit", C.byref(dst.desc), hip.ptr(dst.count), hip.ptr(src.count), 0)
    with pytest.raises(hip.VlfbError, match="NULL"):
        hip.call("vlfb_lfb_unpack_commit", C.byref(dst.desc), None, hip.ptr(src.count), 4)

    big = DeviceBank(17, 61681, 1, 8, "bf16")
    assert big.n_videos * big.n_steps == MAX_CELLS + 1
    with pytest.raises(hip.VlfbError, match="cells"):
        hip.call("vlfb_lfb_unpack", C.byref(big.desc), hip.ptr(big.bank), hip.ptr(big.count), hip.ptr(feats), hip.F32,
                 hip.ptr(big.count), 1, hip.ptr(off), 0, 1, hip.ptr(big.dropped))
    with pytest.raises(hip.VlfbError, match="cells"):
        hip.call("vlfb_lfb_unpack_commit", C.byref(big.desc), hip.ptr(big.count), hip.ptr(big.count), 1)
    torch.cuda.synchronize()
    assert int(dst.dropped.item()) == 0
