"""vlfb_topk_hits_keep (csrc/vlfb_metrics.hip) through the C ABI: top-k hits and the kept prediction rows in one launch.

Everything compared is an integer or a bit pattern, so there is no tolerance:
  hits          == what vlfb_topk_hits adds for the same calls == the numpy restatement of the header's rank rule below
  table[:total] == scores.astype(float32) of the first `total` stream rows, bit for bit (16-bit -> fp32 is exact)
  table_labels  == the labels as given, out of range or not
  guard rows in front of the table and behind table[total] keep their sentinel; cursor == the sum of rows."""
import numpy as np
import pytest
import torch

from vlfb import hip
from vlfb.metrics import DeviceMeter

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KS = (1, 5)
GUARD = 3                                                   # sentinel rows in front of and behind the table
SENTINEL_F, SENTINEL_I = -1234.5, -77


def rank_rule_hits(scores, labels, ks):
    """include/vlfb.h: rank = #{j : s_j > s_label} + #{j < label : s_j == s_label}; hit iff rank < k; a row whose label is
    outside 0..cols-1 is not counted; a NaN label score is a counted miss.  -> [hits per k ..., rows counted]"""
    out = [0] * (len(ks) + 1)
    for s, l in zip(np.asarray(scores, np.float32), labels):
        l = int(l)
        if l < 0 or l >= s.shape[0]:
            continue
        out[-1] += 1
        if np.isnan(s[l]):
            continue
        rank = int(np.sum(s > s[l])) + int(np.sum(s[:l] == s[l]))
        for i, k in enumerate(ks):
            out[i] += rank < k
    return out


def stream_rows(cols, n, seed):
    """n rows with the planted ones: labels -1 and `cols`, a NaN label score, the label's score tied below and above"""
    rng = np.random.RandomState(seed)
    scores = rng.rand(n, cols).astype(np.float32)
    labels = rng.randint(0, cols, size=n).astype(np.int32)
    labels[0] = -1
    if n > 1:
        labels[1] = cols
    if n > 2:
        scores[2, labels[2]] = np.nan
    for r in (3, n - 1):                                    # one tie row inside the table, one in the dropped tail
        if 3 <= r < n:
            labels[r] = cols // 2
            scores[r, :] = 0.25
            scores[r, [0, cols // 2, cols - 1]] = 0.75      # ties at a lower and at a higher index than the label
    return scores, labels


class Kept(object):
    """table and labels with guard rows on both sides, the cursor, the hit counters"""

    def __init__(self, total, cols, alloc_extra=GUARD):
        self.total, self.cols = total, cols
        self.tbuf = torch.full((GUARD + total + alloc_extra, cols), SENTINEL_F, dtype=torch.float32, device=DEV)
        self.lbuf = torch.full((GUARD + total + alloc_extra,), SENTINEL_I, dtype=torch.int32, device=DEV)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.hits = torch.zeros(len(KS) + 1, dtype=torch.int64, device=DEV)
        self.karr, self.nk = hip.ks_array(KS)

    def args(self, scores_t, labels_t):
        return (hip.ptr(scores_t), hip.dtype_code(scores_t.dtype), hip.ptr(labels_t), scores_t.shape[0], self.cols, self.karr,
                self.nk, hip.ptr(self.hits), hip.ptr(self.tbuf[GUARD:]), hip.ptr(self.lbuf[GUARD:]), self.total,
                hip.ptr(self.cursor))

    def read(self):
        t, l = self.tbuf.cpu().numpy(), self.lbuf.cpu().numpy()
        guards_ok = (np.all(t[:GUARD] == SENTINEL_F) and np.all(t[GUARD + self.total:] == SENTINEL_F)
                     and np.all(l[:GUARD] == SENTINEL_I) and np.all(l[GUARD + self.total:] == SENTINEL_I))
        return t[GUARD:GUARD + self.total], l[GUARD:GUARD + self.total], guards_ok


def plain_hits(calls):
    hits = torch.zeros(len(KS) + 1, dtype=torch.int64, device=DEV)
    karr, nk = hip.ks_array(KS)
    for s, l in calls:
        hip.call("vlfb_topk_hits", hip.ptr(s), hip.dtype_code(s.dtype), hip.ptr(l), s.shape[0], s.shape[1], karr, nk, hip.ptr(hits))
    return hits.cpu().tolist()


# (rows of each call, total_rows): the cut inside a call; on a call boundary with the last call dropped whole; 1-row calls
PATTERNS = {"cut_inside": ((3, 3, 3), 7), "cut_on_boundary": ((3, 3, 3), 6), "one_row_calls": ((1, 1, 1), 2),
            "wider_than_the_waves": ((9,), 7)}


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("cols", [5, 125, 352])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_hits_and_kept_rows(dtype, cols, pattern):
    sizes, total = PATTERNS[pattern]
    n = sum(sizes)
    scores, labels = stream_rows(cols, n, seed=cols + n)
    st = torch.from_numpy(scores).to(DEV).to(dtype).contiguous()
    lt = torch.from_numpy(labels).to(DEV)
    as_f32 = st.cpu().float().numpy()                       # what the kernel must store: the element values, exactly
    calls, at = [], 0
    for b in sizes:
        calls.append((st[at:at + b].contiguous(), lt[at:at + b].contiguous()))
        at += b
    k = Kept(total, cols)
    for s, l in calls:
        hip.call("vlfb_topk_hits_keep", *k.args(s, l))
    table, tlab, guards_ok = k.read()
    got = k.hits.cpu().tolist()
    want = rank_rule_hits(as_f32, labels, KS)
    print(pattern, cols, dtype, "hits", got, "rule", want)
    assert got == plain_hits(calls) == want                 # every row of every call is counted, the dropped ones included
    assert want[-1] == n - (2 if n > 1 else 1)              # (the two out-of-range labels are the only rows not counted)
    assert table.tobytes() == as_f32[:total].tobytes()
    assert np.array_equal(tlab, labels[:total])
    assert guards_ok, "a row outside table[0 .. total_rows) was written"
    assert int(k.cursor.item()) == n


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_a_replayed_call_appends_consecutively(dtype):
    """the same argument list issued again (a recorded step's call list, frozen arguments): rows land behind the first"""
    cols, total = 125, 7
    scores, labels = stream_rows(cols, 3, seed=9)
    st = torch.from_numpy(scores).to(DEV).to(dtype).contiguous()
    lt = torch.from_numpy(labels).to(DEV)
    k = Kept(total, cols)
    rec = hip.trace_begin()
    try:
        hip.call("vlfb_topk_hits_keep", *k.args(st, lt))
    finally:
        hip.trace_end()
    (fn, frozen, name), = rec
    assert name == "vlfb_topk_hits_keep"
    for _ in range(2):                                      # stream positions 3..5, then 6..8 of which only 6 is kept
        assert fn(*frozen) == 0
    table, tlab, guards_ok = k.read()
    as_f32 = st.cpu().float().numpy()
    assert table.tobytes() == np.concatenate([as_f32] * 3)[:total].tobytes()
    assert np.array_equal(tlab, np.concatenate([labels] * 3)[:total]) and guards_ok
    assert int(k.cursor.item()) == 9
    assert k.hits.cpu().tolist() == [3 * h for h in rank_rule_hits(as_f32, labels, KS)]


def test_device_meter_keep_rows():
    cols, total = 352, 5
    scores, labels = stream_rows(cols, 6, seed=3)
    plain, keep = DeviceMeter("topk", cols, KS, device=DEV), DeviceMeter("topk", cols, KS, device=DEV, keep_rows=total)
    for at in (0, 2, 4):
        for m in (plain, keep):
            m.update(torch.from_numpy(scores[at:at + 2]).to(DEV), torch.from_numpy(labels[at:at + 2]).to(DEV))
    assert keep.read() == plain.read()
    t, l = keep.kept()
    assert t.cpu().numpy().tobytes() == scores[:total].tobytes() and np.array_equal(l.cpu().numpy(), labels[:total])
    keep.reset()
    assert keep.kept()[0].shape[0] == 0 and keep.read()["rows"] == 0
    with pytest.raises(hip.VlfbError, match="keep_rows"):
        plain.kept()
