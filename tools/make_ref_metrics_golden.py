"""Run the REFERENCE's own metric functions on seeded synthetic inputs and commit inputs + outputs.

TEST INFRASTRUCTURE ONLY.  Needs the reference checkout and scikit-learn (what the reference's meter calls):

    python tools/make_ref_metrics_golden.py          # writes tests/golden/ref_metrics.npz

Called, from where they lie (the Caffe2 / OpenCV stubs of oracle/make_ref_aux_golden.py make the module importable):
  lib/utils/metrics.py   compute_topk_correct_hits (:485-500), MetricsCalculator.stack_predictions +
                         aggregate_predictions_from_clips (:143-186) on an object with the attributes they read,
                         mean_ap_metric (:444-482)
  tools/evaluate_actions.py   softmax (:101-105), compute_top_k_verbs_or_nouns (:63-74), compute_top_k_actions (:77-98)
                         with NUM_TEST_SEG set to the case's row count; both only LOG their accuracy ('Top-%d: %.04f%%'),
                         so the hit count is recovered from the logged figure (rows <= 1000: the figure resolves one hit)
Beside the reference's outputs the file holds scikit-learn's per-class roc_auc_score (the reference only returns the mean).

Storage: multi-label scores are fp16 values stored as their uint16 bit patterns, labels are bit-packed, action
probabilities are the reference softmax's fp32 output, the prior is stored as the integer
co-occurrence counts get_training_action_freq (:44-60) would have counted (prior = counts / counts.sum()).  For the
top-k and action cases the generator ASSERTS that in every row the label's score differs from every other score of the
row, so the reference's unstable argsort cannot decide a hit, and records that it checked (meta["tie_check"]).
"""
import importlib.util
import io
import json
import logging
import os
import re
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "ref_metrics.npz")
sys.path.insert(0, ROOT)


def f16_codes(x):
    return np.asarray(x, np.float32).astype(np.float16).view(np.uint16)


def from_codes(c):
    return c.view(np.float16).astype(np.float32)


def label_distinct(scores, idx):
    """every row's score at idx differs from every other score of the row"""
    rows = np.arange(scores.shape[0])
    same = scores == scores[rows, idx][:, None]
    return bool(np.all(same.sum(axis=1) == 1))


def main():
    from oracle.make_ref_aux_golden import install_stubs
    install_stubs()
    import sklearn.metrics as skm
    import utils.metrics as M                    # the reference's (install_stubs put its lib/ on the path)
    assert os.path.realpath(M.__file__).startswith(REF), M.__file__
    spec = importlib.util.spec_from_file_location("ref_evaluate_actions", os.path.join(REF, "tools", "evaluate_actions.py"))
    EA = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(EA)
    logged = []

    class Grab(logging.Handler):
        def emit(self, record):
            logged.append(record.getMessage())
    EA.logger.addHandler(Grab())

    def logged_hits(fn, rows, *args, **kw):
        del logged[:]
        EA.NUM_TEST_SEG = rows
        fn(*args, **kw)
        acc = float(re.match(r"Top-\d+: ([0-9.]+)%", logged[-1]).group(1))
        hits = int(round(acc * rows / 100.0))
        assert abs(100.0 * hits / rows - acc) < 1e-3 and rows <= 1000
        return hits

    meta = {"generator": "tools/make_ref_metrics_golden.py", "sklearn": __import__("sklearn").__version__, "cases": {},
            "tie_check": True}
    arrays = {}
    rng = np.random.RandomState(20240611)

    # ---- top-k ------------------------------------------------------------------------------------------------------
    for cols in (125, 352, 400):
        rows = 32
        logits = rng.randn(rows, cols).astype(np.float32) * 2.0
        labels = rng.randint(0, cols, rows).astype(np.int32)
        hot = rng.rand(rows) < 0.6                                   # the label is often near the top, not always at it
        logits[np.arange(rows)[hot], labels[hot]] += rng.uniform(1.0, 5.0, hot.sum()).astype(np.float32)
        preds = EA.softmax(logits).astype(np.float32)
        assert label_distinct(preds, labels), "top-k case %d: a label's score is tied" % cols
        name = "topk%d" % cols
        arrays[name + "_preds"], arrays[name + "_labels"] = preds, labels
        hits = {k: int(M.compute_topk_correct_hits(k, preds, labels)) for k in (1, 5)}
        hits_ea = {k: logged_hits(EA.compute_top_k_verbs_or_nouns, rows, preds, labels, k) for k in (1, 5)}
        assert hits == hits_ea, (hits, hits_ea)                      # the two spellings agree where nothing is tied
        meta["cases"][name] = {"rows": rows, "cols": cols, "hits": {str(k): v for k, v in hits.items()}}

    # ---- Charades-shaped mAP: 3 clips x 621 videos, and the same 1863 rows as one single-clip set --------------------
    def multilabel(n_videos, clips, cols, zero_classes, full_classes=()):
        lab = (rng.rand(n_videos, cols) < 0.06).astype(np.int32)
        lab[:, list(zero_classes)] = 0
        lab[:, list(full_classes)] = 1
        lab_rows = np.tile(lab, (clips, 1))
        logit = np.round((rng.randn(n_videos * clips, cols) * 1.5 - 2.0 + 2.0 * lab_rows) * 8.0) / 8.0
        return lab, lab_rows, f16_codes(1.0 / (1.0 + np.exp(-logit)))

    def ref_map(preds, labels):
        auc, ap, wap, all_aps = M.mean_ap_metric([preds], [labels])
        keep = ~np.all(labels == 0, axis=0)
        both = np.array([len(np.unique(labels[:, c])) == 2 for c in range(labels.shape[1])])
        cls_auc = np.full(labels.shape[1], np.nan)
        cls_auc[both] = skm.roc_auc_score(labels[:, both], preds[:, both], average=None)
        return {"mean_auc": float(auc), "mean_ap": float(ap), "mean_wap": float(wap)}, np.asarray(all_aps, np.float64), cls_auc, keep

    def clip_merge(preds, lab_rows, n_videos, clips, batch):
        """feed `batch`-row batches (the last one padded, as a fixed batch size does) through the reference's
        stack_predictions + aggregate_predictions_from_clips"""
        total = n_videos * clips
        pad = (-total) % batch
        p = np.vstack([preds, preds[:pad]])
        l = np.vstack([lab_rows, lab_rows[:pad]])
        o = types.SimpleNamespace(num_test_clips=clips,
                                  all_preds=[p[i:i + batch].copy() for i in range(0, total + pad, batch)],
                                  all_labels=[l[i:i + batch].copy() for i in range(0, total + pad, batch)])
        M.cfg.MODEL.MULTI_LABEL, M.cfg.TEST.DATASET_SIZE, M.cfg.TEST.BATCH_SIZE = True, n_videos, batch
        o.stack_predictions = lambda: M.MetricsCalculator.stack_predictions(o)
        M.MetricsCalculator.aggregate_predictions_from_clips(o)
        return o.all_preds, o.all_labels

    n_videos, clips, cols = 621, 3, 157
    lab, lab_rows, codes = multilabel(n_videos, clips, cols, zero_classes=(11, 140))
    preds = from_codes(codes)
    arrays["charades_codes"], arrays["charades_labels_bits"] = codes, np.packbits(lab.astype(np.uint8), axis=1)
    merged, merged_lab = clip_merge(preds, lab_rows, n_videos, clips, batch=16)
    assert np.array_equal(merged_lab, lab)
    assert np.array_equal(merged, preds.reshape(clips, n_videos, cols).max(axis=0))   # (not stored: the max over the clips)
    for name, (p, l) in (("charades3", (merged, lab)), ("charades1", (preds, lab_rows))):
        means, all_aps, cls_auc, keep = ref_map(p, l)
        arrays[name + "_all_aps"], arrays[name + "_class_auc"] = all_aps, cls_auc
        meta["cases"][name] = dict(means, n=int(p.shape[0]), cols=cols, clips=clips if name == "charades3" else 1,
                                   n_videos=n_videos, kept=int(keep.sum()))

    # ---- one all-positive class: mean_auc is NaN with this scikit-learn (older releases raised, the reference then returns 0)
    lab, lab_rows, codes = multilabel(200, 1, 20, zero_classes=(3,), full_classes=(7,))
    arrays["allpos_codes"], arrays["allpos_labels_bits"] = codes, np.packbits(lab.astype(np.uint8), axis=1)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        means, all_aps, cls_auc, keep = ref_map(from_codes(codes), lab)
    arrays["allpos_all_aps"], arrays["allpos_class_auc"] = all_aps, cls_auc
    meta["cases"]["allpos"] = dict({k: (None if v != v else v) for k, v in means.items()}, n=200, cols=20, clips=1,
                                   n_videos=200, kept=int(keep.sum()), mean_auc_is_nan=bool(means["mean_auc"] != means["mean_auc"]))

    # ---- EPIC actions ------------------------------------------------------------------------------------------------
    rows, V, Nn = 160, 125, 352
    vl, nl = rng.randint(0, V, rows).astype(np.int32), rng.randint(0, Nn, rows).astype(np.int32)
    vlog, nlog = rng.randn(rows, V).astype(np.float32) * 2.0, rng.randn(rows, Nn).astype(np.float32) * 2.0
    hot = rng.rand(rows) < 0.7
    vlog[np.arange(rows)[hot], vl[hot]] += 5.0
    nlog[np.arange(rows)[hot], nl[hot]] += 5.0
    verb, noun = EA.softmax(vlog), EA.softmax(nlog)
    assert verb.dtype == noun.dtype == np.float32
    counts = rng.randint(1, 17, (V, Nn))                              # every pair seen: no score is zeroed into a tie
    counts = counts.astype(np.uint16)
    prior = (counts / counts.sum()).astype(np.float32)
    arrays.update(act_verb=verb, act_noun=noun, act_verb_labels=vl, act_noun_labels=nl, act_prior_counts=counts)
    case = {"rows": rows, "V": V, "Nn": Nn}
    for tag, pr in (("plain", None), ("prior", prior)):
        flat = (verb[:, :, None] * noun[:, None, :]).reshape(rows, -1)
        if pr is not None:
            flat = flat * pr.reshape(1, -1)
        assert flat.dtype == np.float32
        assert label_distinct(flat, vl * Nn + nl), "an action label's score is tied (%s)" % tag
        case[tag] = {str(k): logged_hits(EA.compute_top_k_actions, rows, verb, noun, vl, nl, k, prior=pr) for k in (1, 5)}
    case["verb_hits"] = {str(k): logged_hits(EA.compute_top_k_verbs_or_nouns, rows, verb, vl, k) for k in (1, 5)}
    assert label_distinct(verb, vl)
    meta["cases"]["actions"] = case

    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    with open(OUT, "wb") as f:
        f.write(buf.getvalue())
    print("wrote %s: %d arrays, %d bytes" % (os.path.normpath(OUT), len(arrays), os.path.getsize(OUT)))
    print(json.dumps(meta["cases"], indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
