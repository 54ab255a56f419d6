"""The metric kernels (csrc/vlfb_metrics.hip) through the C ABI against tests/golden/ref_metrics.npz (the reference's
own outputs) and the numpy restatement of tests/test_metrics_host.py.

Integers (hits, rows, n_pos, mismatches, cursor) are exact.  Per-class AP / AUC and the three means:
abs(dev - ref) <= (n + 8) * 2^-52 -- both sides are fixed-order fp64 sums of at most n non-negative terms that total at
most 1, one rounding per term and per add."""
import numpy as np
import pytest
import torch

import test_metrics_host as H
from vlfb import hip
from vlfb.metrics import DeviceMeter, action_topk_hits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.to(dtype).contiguous() if dtype is not None else t


def run_topk(scores_t, labels, ks, hits=None):
    karr, nk = hip.ks_array(ks)
    hits = torch.zeros(nk + 1, dtype=torch.int64, device=DEV) if hits is None else hits
    hip.call("vlfb_topk_hits", hip.ptr(scores_t), hip.dtype_code(scores_t.dtype), hip.ptr(dev(labels.astype(np.int32))),
             scores_t.shape[0], scores_t.shape[1], karr, nk, hip.ptr(hits))
    return hits


@pytest.mark.parametrize("cols", [125, 352, 400])
def test_topk_hits_match_the_reference(cols):
    z, meta = H.load()
    case = meta["cases"]["topk%d" % cols]
    preds, labels = z["topk%d_preds" % cols], z["topk%d_labels" % cols]
    got = run_topk(dev(preds), labels, (1, 5)).cpu().tolist()
    print("topk%d" % cols, got, case)
    assert got == [case["hits"]["1"], case["hits"]["5"], case["rows"]]
    # accumulation: two updates == one over the concatenation; four k at once
    hits = run_topk(dev(preds[:13]), labels[:13], (1, 5))
    run_topk(dev(preds[13:]), labels[13:], (1, 5), hits)
    assert hits.cpu().tolist() == got
    ks = (1, 2, 5, cols)
    assert run_topk(dev(preds), labels, ks).cpu().tolist() == list(H.topk_hits(preds, labels, ks)[0]) + [case["rows"]]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_topk_16bit_input_equals_the_same_values_as_f32(dtype):
    z, _ = H.load()
    preds, labels = z["topk352_preds"], z["topk352_labels"]
    q = dev(preds, dtype)                                  # rounding to 16 bits creates ties: the rule decides them
    want = H.topk_hits(q.float().cpu().numpy(), labels, (1, 5))
    assert run_topk(q, labels, (1, 5)).cpu().tolist() == run_topk(q.float(), labels, (1, 5)).cpu().tolist() == want[0] + [want[1]]


def test_topk_tie_rule_skipped_rows_and_nan():
    rows = np.array([[0.5, 0.25, 0.5, 0.5, 0.125]] * 5 + [[0.5, np.nan, 0.5, 0.1, 0.2]] * 2 + [[1, 2, 3, 4, 5]] * 2, np.float32)
    labels = np.array([0, 1, 2, 3, 4, 1, 2, -1, 5], np.int32)
    want = H.topk_hits(rows, labels, (1, 2, 3))
    assert want == ([1, 3, 4], 7)                          # (NaN label: counted miss; labels -1 and 5: not counted)
    assert run_topk(dev(rows), labels, (1, 2, 3)).cpu().tolist() == want[0] + [want[1]]


def test_action_topk_matches_the_reference():
    z, meta = H.load()
    case = meta["cases"]["actions"]
    verb, noun, vl, nl = z["act_verb"], z["act_noun"], z["act_verb_labels"], z["act_noun_labels"]
    counts = z["act_prior_counts"]
    prior = (counts / counts.sum()).astype(np.float32)
    for tag, pr in (("plain", None), ("prior", prior)):
        hits, rows = action_topk_hits(dev(verb), dev(noun), dev(vl), dev(nl), (1, 5), None if pr is None else dev(pr))
        print("actions", tag, hits, rows, case[tag])
        assert rows == case["rows"] and hits == {1: case[tag]["1"], 5: case[tag]["5"]}
    # ties (a prior with zeros) and out-of-range labels, against the restatement
    pz = prior.copy()
    pz[::2] = 0
    vl2 = vl.copy()
    vl2[:3] = (-1, 125, 7)
    want = H.topk_hits(H.action_scores(verb, noun, pz), np.where((vl2 >= 0) & (vl2 < 125), vl2 * 352 + nl, -1), (1, 5, 4000))
    hits, rows = action_topk_hits(dev(verb), dev(noun), dev(vl2), dev(nl), (1, 5, 4000), dev(pz))
    assert [hits[1], hits[5], hits[4000]] == want[0] and rows == want[1]


def class_scores(scores, labels, flags=0):
    n, cols = scores.shape
    m = DeviceMeter("map", cols, n_items=n, device=DEV)
    m.update(dev(scores), dev(labels.astype(np.int32)))
    if flags:
        m.ws_bytes = hip.query_workspace(hip.WS_CLASS_AP, (n, cols))
        m.ws = torch.empty(m.ws_bytes, dtype=torch.uint8, device=DEV)
    out = m.class_scores(n, flags)
    return tuple(a.copy() for a in out), m


@pytest.mark.parametrize("name", ["charades3", "charades1", "allpos"])
def test_class_ap_auc_matches_the_reference(name):
    z, meta = H.load()
    case = meta["cases"][name]
    scores, labels = H.multilabel_case(z, meta, name)
    n, tol = case["n"], H.bound(case["n"])
    (ap, auc, n_pos), meter = class_scores(scores, labels)
    assert np.array_equal(n_pos, (labels > 0).sum(axis=0))
    keep = n_pos > 0
    ref_aps, ref_auc = z[name + "_all_aps"], z[name + "_class_auc"]
    print(name, "max |AP - ref|", np.max(np.abs(ap[keep] - ref_aps[keep])), "max |AUC - ref|",
          np.nanmax(np.abs(auc - ref_auc)), "bound", tol)
    assert np.all(np.isnan(ap[~keep])) and np.max(np.abs(ap[keep] - ref_aps[keep])) <= tol
    assert np.array_equal(np.isnan(auc), np.isnan(ref_auc)) and np.nanmax(np.abs(auc - ref_auc)) <= tol
    r = meter.read()
    ref_mean_auc = float("nan") if case["mean_auc"] is None else case["mean_auc"]
    print(name, r["mean_ap"] - case["mean_ap"], r["mean_wap"] - case["mean_wap"], r["mean_auc"], ref_mean_auc)
    assert abs(r["mean_ap"] - case["mean_ap"]) <= tol and abs(r["mean_wap"] - case["mean_wap"]) <= tol
    assert H.same(r["mean_auc"], ref_mean_auc, tol)
    assert np.max(np.abs(r["all_aps"] - ref_aps)) <= tol and r["rows"] == n and r["label_mismatches"] == 0
    # LDS path == global path, bit for bit
    (ap_g, auc_g, pos_g), _ = class_scores(scores, labels, hip.CLASS_AP_FORCE_GLOBAL)
    assert ap_g.tobytes() == ap.tobytes() and auc_g.tobytes() == auc.tobytes() and np.array_equal(pos_g, n_pos)


def test_class_ap_auc_above_the_lds_limit_and_small_n():
    rng = np.random.RandomState(5)
    for n, cols in ((9000, 6), (1, 3), (2, 3), (513, 4)):
        scores = np.round(rng.rand(n, cols) * 32).astype(np.float32) / 32      # heavy ties
        labels = (rng.rand(n, cols) < 0.3).astype(np.int32)
        (ap, auc, n_pos), _ = class_scores(scores, labels)
        for c in range(cols):
            want = H.class_ap_auc(scores[:, c], labels[:, c])
            assert n_pos[c] == want[2] and H.same(ap[c], want[0], H.bound(n)) and H.same(auc[c], want[1], H.bound(n)), (n, c)


def test_merge_batches_wrap_and_padding():
    z, meta = H.load()
    rows = H.codes_to_f32(z["charades_codes"])[:60]
    lab = np.tile(np.unpackbits(z["charades_labels_bits"], axis=1)[:5, :157].astype(np.int32), (12, 1))
    n_items, cols, total = 5, 157, 58                      # 12 visits per item; the last 2 rows are padding
    want = H.merge_max([(rows, lab)], n_items, cols, total)
    assert want[3] == 0

    def run(sizes, dtype=torch.float32, labels=lab):
        m = DeviceMeter("map", cols, n_items=n_items, total_rows=total, device=DEV)
        at = 0
        while at < 60:
            for b in sizes:
                if at < 60:
                    m.update(dev(rows[at:at + b], dtype), dev(labels[at:at + b]))
                    at += min(b, 60 - at)
        _, _, cursor, mismatches = m.counters()
        return m.table.cpu().numpy(), m.labels.cpu().numpy(), cursor, mismatches

    for sizes in ((60,), (1,), (3,), (7,), (1, 3, 7)):     # 7 > n_items: a batch wraps onto its own items
        t, l, cursor, mismatches = run(sizes)
        assert t.tobytes() == want[0].tobytes() and np.array_equal(l, want[1]) and cursor == 60 and mismatches == 0, sizes
    assert run((7,), torch.float16)[0].tobytes() == want[0].tobytes()          # fp16 scores == the same values as fp32
    bad = lab.copy()
    bad[7, 3] ^= 1
    bad[21, 100] ^= 1
    assert run((7,), labels=bad)[3] == H.merge_max([(rows, bad)], n_items, cols, total)[3] == 2


def test_device_meter_and_the_reference_names():
    import utils.metrics as M
    z, meta = H.load()
    case = meta["cases"]["topk400"]
    preds, labels = z["topk400_preds"], z["topk400_labels"]
    assert M.compute_topk_correct_hits(5, preds, labels) == case["hits"]["5"]
    m = DeviceMeter("topk", 400, device=DEV)
    m.update(dev(preds[:20]), dev(labels[:20]))
    m.update(dev(preds[20:]), dev(labels[20:]))
    r = m.read()
    assert r["rows"] == 32 and r["top1_err"] == (1 - case["hits"]["1"] / 32.0) * 100 and r["top5_err"] == (1 - case["hits"]["5"] / 32.0) * 100
    m.reset()
    assert m.read()["rows"] == 0
    c = meta["cases"]["charades3"]
    scores, lab = H.multilabel_case(z, meta, "charades3")
    auc, ap, wap, all_aps = M.mean_ap_metric([scores[:300], scores[300:]], [lab[:300], lab[300:]])
    tol = H.bound(c["n"])
    assert abs(ap - c["mean_ap"]) <= tol and abs(wap - c["mean_wap"]) <= tol and abs(auc - c["mean_auc"]) <= tol
