"""The SPECIFICATION of the device metrics, pinned to the reference on the CPU.

tests/golden/ref_metrics.npz (tools/make_ref_metrics_golden.py) holds what the reference's own
compute_topk_correct_hits / aggregate_predictions_from_clips / mean_ap_metric (lib/utils/metrics.py) and
compute_top_k_verbs_or_nouns / compute_top_k_actions (tools/evaluate_actions.py) returned on seeded inputs.  The numpy
restatements below -- the rank rule and the two tie-grouped formulas of include/vlfb.h -- must reproduce every value;
the GPU tests then hold the kernels to the same restatements and fixtures.

Bound on AP / AUC: both sides are fixed-order fp64 sums of at most n non-negative terms that total at most 1, one
rounding per term and per add: (n + 8) * 2^-52.
"""
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_metrics.npz")


# ---- the restatement ------------------------------------------------------------------------------------------------
def rank_of_label(row, label):
    """rank = #{j : s_j > s_label} + #{j < label : s_j == s_label}"""
    s = row[label]
    return int(np.sum(row > s)) + int(np.sum(row[:label] == s))


def topk_hits(scores, labels, ks):
    """-> ([hits per k], rows counted): out-of-range labels are skipped, a NaN label score is a counted miss"""
    scores = np.asarray(scores)
    hits, rows = [0] * len(ks), 0
    for r in range(scores.shape[0]):
        l = int(labels[r])
        if l < 0 or l >= scores.shape[1]:
            continue
        rows += 1
        if np.isnan(scores[r, l]):
            continue
        rank = rank_of_label(scores[r], l)
        for i, k in enumerate(ks):
            hits[i] += rank < k
    return hits, rows


def action_scores(verb, noun, prior=None):
    """flattened (verb[v] * noun[n]) * prior[v][n], every product rounded to fp32 in that order"""
    flat = (verb.astype(np.float32)[:, :, None] * noun.astype(np.float32)[:, None, :]).reshape(verb.shape[0], -1)
    if prior is not None:
        flat = flat * prior.astype(np.float32).reshape(1, -1)
    assert flat.dtype == np.float32
    return flat


def class_ap_auc(scores, labels):
    """(AP, AUC, P) of one class: ties grouped, integer counts, one division per term, summed in index order"""
    order = np.argsort(-scores, kind="stable")
    s, y = scores[order], (labels[order] > 0).astype(np.int64)
    n = len(s)
    ends = np.flatnonzero(np.append(s[1:] != s[:-1], True))          # e_g
    tp = np.cumsum(y)[ends]
    P = int(tp[-1]) if n else 0
    if P == 0:
        return float("nan"), float("nan"), 0
    fp = ends + 1 - tp
    tp_prev, fp_prev = np.append(0, tp[:-1]), np.append(0, fp[:-1])
    ap = 0.0
    for g in range(len(ends)):
        if tp[g] != tp_prev[g]:
            ap += float((tp[g] - tp_prev[g]) * tp[g]) / float(P * (ends[g] + 1))
    if P == n:
        return ap, float("nan"), P
    auc = 0.0
    for g in range(len(ends)):
        if fp[g] != fp_prev[g]:
            auc += float((fp[g] - fp_prev[g]) * (tp[g] + tp_prev[g])) / float(2 * P * (n - P))
    return ap, auc, P


def mean_ap(scores, labels):
    """mean_ap_metric (metrics.py:444-482): (mean_auc, mean_ap, mean_wap, all_aps, per-class auc)"""
    cols = scores.shape[1]
    per = [class_ap_auc(scores[:, c], labels[:, c]) for c in range(cols)]
    ap, auc, pos = (np.array([p[i] for p in per], np.float64) for i in range(3))
    keep = pos > 0
    all_aps = np.zeros(cols)
    all_aps[keep] = ap[keep]
    w = pos[keep] / np.sum(pos[keep])
    return float(np.mean(auc[keep])), float(np.mean(ap[keep])), float(np.sum(np.multiply(ap[keep], w))), all_aps, auc


def merge_max(batches, n_items, cols, total=0):
    """the clip merge: row at stream position p goes to item p % n_items by max; positions >= total are dropped"""
    table = np.full((n_items, cols), -np.inf, np.float32)
    labels = np.full((n_items, cols), 255, np.uint8)
    pos, mismatches = 0, 0
    for s, l in batches:
        for r in range(s.shape[0]):
            if total and pos + r >= total:
                break
            i = (pos + r) % n_items
            table[i] = np.where(s[r] > table[i], s[r], table[i])
            lab = (l[r] > 0).astype(np.uint8)
            seen = labels[i] != 255
            mismatches += int(np.sum(seen & (labels[i] != lab)))
            labels[i] = np.where(seen, labels[i], lab)
        pos += s.shape[0]
    return table, labels, pos, mismatches


# ---- the fixture ------------------------------------------------------------------------------------------------------
def load():
    z = np.load(GOLDEN)
    meta = json.loads(bytes(z["meta"]).decode())
    return z, meta


def codes_to_f32(c):
    return c.view(np.float16).astype(np.float32)


def multilabel_case(z, meta, name):
    """(scores [n][cols], labels [n][cols]) as the reference's mean_ap_metric saw them"""
    case = meta["cases"][name]
    cols = case["cols"]
    if name.startswith("charades"):
        codes, bits = z["charades_codes"], z["charades_labels_bits"]
    else:
        codes, bits = z[name + "_codes"], z[name + "_labels_bits"]
    lab = np.unpackbits(bits, axis=1)[:, :cols].astype(np.int32)
    rows = codes_to_f32(codes)
    if case["clips"] > 1:
        return rows.reshape(case["clips"], case["n_videos"], cols).max(axis=0), lab
    return rows, np.tile(lab, (rows.shape[0] // lab.shape[0], 1))


def bound(n):
    return (n + 8) * 2.0 ** -52


def same(a, b, tol):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= tol


# ---- tests ------------------------------------------------------------------------------------------------------------
def test_utils_metrics_exposes_the_reference_names():
    import utils.metrics as m
    import vlfb.metrics as vm
    for name in ("compute_topk_correct_hits", "mean_ap_metric", "MetricsCalculator"):
        assert hasattr(m, name), name
    for name in ("reset", "calculate_and_log_all_metrics_train", "calculate_and_log_all_metrics_test", "finalize_metrics",
                 "get_computed_metrics"):
        assert callable(getattr(m.MetricsCalculator, name)), name
    assert hasattr(vm, "DeviceMeter")
    from vlfb.engine import Engine
    assert callable(Engine.attach_meter)
    # no scikit-learn anywhere in the package
    src = open(m.__file__.replace(".pyc", ".py")).read() + open(vm.__file__.replace(".pyc", ".py")).read()
    assert "import sklearn" not in src and "from sklearn" not in src


def test_fixture_loads_and_recorded_its_tie_check():
    z, meta = load()
    assert meta["tie_check"] is True
    assert set(meta["cases"]) >= {"topk125", "topk352", "topk400", "charades3", "charades1", "allpos", "actions"}
    for k in z.files:
        assert z[k].dtype != object, k                     # arrays and one JSON string only
    for cols in (125, 352, 400):
        p, l = z["topk%d_preds" % cols], z["topk%d_labels" % cols]
        s = p[np.arange(len(l)), l]
        assert np.all((p == s[:, None]).sum(axis=1) == 1)
    assert os.path.getsize(GOLDEN) < 770790                # below the largest committed fixture (ref_aux.npz)


@pytest.mark.parametrize("cols", [125, 352, 400])
def test_rank_rule_reproduces_the_reference_topk(cols):
    z, meta = load()
    case = meta["cases"]["topk%d" % cols]
    hits, rows = topk_hits(z["topk%d_preds" % cols], z["topk%d_labels" % cols], (1, 5))
    assert rows == case["rows"] and hits == [case["hits"]["1"], case["hits"]["5"]]


def test_rank_rule_reproduces_the_reference_actions():
    z, meta = load()
    case = meta["cases"]["actions"]
    verb, noun, vl, nl = z["act_verb"], z["act_noun"], z["act_verb_labels"], z["act_noun_labels"]
    counts = z["act_prior_counts"]
    prior = (counts / counts.sum()).astype(np.float32)
    for tag, pr in (("plain", None), ("prior", prior)):
        hits, rows = topk_hits(action_scores(verb, noun, pr), vl * case["Nn"] + nl, (1, 5))
        assert rows == case["rows"] and hits == [case[tag]["1"], case[tag]["5"]], tag
    hits, _ = topk_hits(verb, vl, (1, 5))
    assert hits == [case["verb_hits"]["1"], case["verb_hits"]["5"]]


@pytest.mark.parametrize("name", ["charades3", "charades1", "allpos"])
def test_formulas_reproduce_the_reference_map(name):
    z, meta = load()
    case = meta["cases"][name]
    scores, labels = multilabel_case(z, meta, name)
    assert scores.shape == (case["n"], case["cols"])
    auc, ap, wap, all_aps, cls_auc = mean_ap(scores, labels)
    tol = bound(case["n"])
    assert np.max(np.abs(all_aps - z[name + "_all_aps"])) <= tol
    ref_auc = z[name + "_class_auc"]
    assert np.array_equal(np.isnan(cls_auc), np.isnan(ref_auc))
    assert np.nanmax(np.abs(cls_auc - ref_auc)) <= tol
    assert abs(ap - case["mean_ap"]) <= tol and abs(wap - case["mean_wap"]) <= tol
    ref_mean_auc = float("nan") if case["mean_auc"] is None else case["mean_auc"]
    assert same(auc, ref_mean_auc, tol)
    if name == "allpos":
        assert case["mean_auc_is_nan"] and np.isnan(auc)
    from vlfb.metrics import summarize_ap                  # the host-side reductions of DeviceMeter.read()
    per = [class_ap_auc(scores[:, c], labels[:, c]) for c in range(case["cols"])]
    got = summarize_ap([p[0] for p in per], [p[1] for p in per], [p[2] for p in per])
    assert same(got[0], ref_mean_auc, tol) and abs(got[1] - case["mean_ap"]) <= tol and abs(got[2] - case["mean_wap"]) <= tol
    assert np.max(np.abs(got[3] - z[name + "_all_aps"])) <= tol


def test_tie_rule_on_a_constructed_row():
    row = np.array([0.5, 0.25, 0.5, 0.5, 0.125], np.float32)
    assert [rank_of_label(row, l) for l in range(5)] == [0, 3, 1, 2, 4]
    assert topk_hits(row[None], [2], (1, 2)) == ([0, 1], 1)
    assert topk_hits(row[None], [7], (1,)) == ([0], 0)


def test_host_side_argument_checks_need_no_gpu():
    from vlfb import hip
    if not os.path.exists(hip.LIB_PATH):
        pytest.skip("libvlfb_hip.so not built")
    L = hip.lib()
    p = 4096                                               # never dereferenced: every call is rejected on the host
    ks5, n5 = hip.ks_array((1, 2, 3, 4, 5))
    ks, nk = hip.ks_array((1, 5))
    with pytest.raises(hip.VlfbError, match="nk"):
        hip._check(L.vlfb_topk_hits(p, hip.F32, p, 2, 10, ks5, n5, p, None), "vlfb_topk_hits")
    with pytest.raises(hip.VlfbError, match="outside 1..cols"):
        hip._check(L.vlfb_topk_hits(p, hip.F32, p, 2, 4, ks, nk, p, None), "vlfb_topk_hits")
    with pytest.raises(hip.VlfbError, match="outside 1..cols"):
        hip._check(L.vlfb_action_topk_hits(p, p, None, p, p, 2, 2, 2, ks, nk, p, None), "vlfb_action_topk_hits")
    with pytest.raises(hip.VlfbError, match="null table"):
        hip._check(L.vlfb_scores_merge_max(p, hip.F32, p, 2, 4, None, None, 3, 0, p, p, None), "vlfb_scores_merge_max")
    with pytest.raises(hip.VlfbError, match="n_items"):
        hip._check(L.vlfb_scores_merge_max(p, hip.F32, p, 2, 4, p, p, 0, 0, p, p, None), "vlfb_scores_merge_max")
    with pytest.raises(hip.VlfbError, match="n = 0"):
        hip._check(L.vlfb_class_ap_auc(p, p, 0, 4, p, p, p, None, 0, 0, None), "vlfb_class_ap_auc")
    with pytest.raises(hip.VlfbError, match="null table"):
        hip._check(L.vlfb_class_ap_auc(None, p, 8, 4, p, p, p, None, 0, 0, None), "vlfb_class_ap_auc")
    with pytest.raises(hip.VlfbError, match="short workspace"):
        hip._check(L.vlfb_class_ap_auc(p, p, 10000, 4, p, p, p, p, 16, 0, None), "vlfb_class_ap_auc")
    with pytest.raises(hip.VlfbError, match="short workspace"):
        hip._check(L.vlfb_class_ap_auc(p, p, 100, 4, p, p, p, None, 0, hip.CLASS_AP_FORCE_GLOBAL, None), "vlfb_class_ap_auc")
    assert hip.query_workspace(hip.WS_CLASS_AP, (1863, 157)) == 2048 * 157 * 5
    assert hip.query_workspace(hip.WS_CLASS_AP, (5281, 352)) == 8192 * 352 * 5
    with pytest.raises(hip.VlfbError, match="class_ap"):
        hip.query_workspace(hip.WS_CLASS_AP, (0, 3))
    with pytest.raises(hip.VlfbError, match="unknown op"):
        hip.query_workspace(17, (1,))
