"""EPIC-Kitchens action accuracy from the kept verb and noun predictions (reference: tools/evaluate_actions.py:109-141).

The two files are what utils.metrics.MetricsCalculator(keep_predictions=True).finalize_metrics writes for the verb and for
the noun model: epic_predictions_<name>.pkl = (pred float32 [n][cols], labels int32 [n]).  The stored `pred` is already a
softmax output; the reference applies its row softmax AGAIN to both tables and ranks on those values, and so does this
module (vlfb_softmax_fwd on the device).  The (verb, noun) frequency table of the training split and the prior
v_given_n are a 125 x 352 table built once on the host; verb, noun and action top-k run on the device
(vlfb_topk_hits / vlfb_action_topk_hits, the rank rule of include/vlfb.h).

    figures = evaluate_actions("verb/epic_predictions_final.pkl", "noun/epic_predictions_final.pkl", "data/epic/annotations")
"""
import csv
import logging
import os
import pickle

import numpy as np
import torch

from vlfb import hip
from vlfb.metrics import DeviceMeter, action_topk_hits

logger = logging.getLogger(__name__)

KS = (1, 5)
TRAIN_PARTICIPANTS = 25                       # P01..P25 are the reference's training split, P26..P32 its held-out part


def training_action_counts(num_verbs, num_nouns, annotation_root):
    """int64 [num_verbs][num_nouns]: how often each (verb, noun) pair occurs in EPIC_train_action_labels.csv among the
    participants of the training split (get_training_action_freq, evaluate_actions.py:44-60, before its division)"""
    seen = np.zeros((int(num_verbs), int(num_nouns)), dtype=np.int64)
    with open(os.path.join(annotation_root, 'EPIC_train_action_labels.csv'), 'r') as f:
        f.readline()
        for row in csv.reader(f):
            assert len(row) == 14, len(row)
            person = int(row[1][1:])
            assert 1 <= person <= 32, person
            if person <= TRAIN_PARTICIPANTS:
                seen[int(row[-5]), int(row[-3])] += 1
    return seen


def get_training_action_freq(num_verbs, num_nouns, annotation_root):
    """the reference's table: float64 counts / their sum"""
    seen = training_action_counts(num_verbs, num_nouns, annotation_root).astype(np.float64)
    return seen / seen.sum()


def verb_given_noun(action_freq):
    """the prior the reference multiplies the action scores with (evaluate_actions.py:129-130), float64"""
    return action_freq / (np.sum(action_freq, axis=1, keepdims=True) + 1e-5)


def load_predictions(path):
    """(pred float32 [n][cols], labels int32 [n]) of an epic_predictions_<name>.pkl, written by Python 2 or 3"""
    with open(path, 'rb') as f:
        try:
            pred, labels = pickle.load(f, encoding='latin1')
        except TypeError:
            f.seek(0)
            pred, labels = pickle.load(f)
    pred = np.ascontiguousarray(pred, dtype=np.float32)
    labels = np.ascontiguousarray(np.asarray(labels).reshape(-1), dtype=np.int32)
    assert pred.ndim == 2 and pred.shape[0] == labels.shape[0], (path, pred.shape, labels.shape)
    return pred, labels


def softmax_rows(pred, device="cuda:0"):
    """the reference's second softmax of a stored table, on the device: float32 [n][cols] host array -> device tensor"""
    s = torch.from_numpy(pred).to(device)
    p = torch.empty_like(s)
    hip.call("vlfb_softmax_fwd", hip.ptr(s), hip.ptr(p), hip.F32, s.shape[0], s.shape[1], 1.0)
    return p


def topk_accuracies(verb, noun, verb_labels, noun_labels, prior, ks=KS):
    """verb / noun fp32 device tables, int32 device labels, prior fp32 [V][Nn] device tensor or None
    -> ({"verb": {k: hits}, "noun": ..., "action": ...}, rows); every row must carry labels inside both heads"""
    rows = int(verb.shape[0])
    hits = {}
    for name, table, labels in (("verb", verb, verb_labels), ("noun", noun, noun_labels)):
        meter = DeviceMeter("topk", table.shape[1], ks=ks, device=table.device)
        meter.update(table, labels)
        r = meter.read()
        assert r["rows"] == rows, "%s labels outside 0..%d in %d rows" % (name, table.shape[1] - 1, rows - r["rows"])
        hits[name] = {int(k): int(v) for k, v in r["hits"].items()}
    hits["action"], counted = action_topk_hits(verb, noun, verb_labels, noun_labels, ks, prior)
    assert counted == rows, (counted, rows)
    return hits, rows


def evaluate_actions(verb_file, noun_file, annotation_root, device="cuda:0"):
    """-> {"verb_top1", "verb_top5", "noun_top1", "noun_top5", "action_top1", "action_top5"} in percent, logged as the
    reference logs them.  The row counts of the two files must agree (the reference hard-codes its 5281 test segments)."""
    verb_pred, verb_labels = load_predictions(verb_file)
    noun_pred, noun_labels = load_predictions(noun_file)
    assert verb_pred.shape[0] == noun_pred.shape[0], \
        "the verb file holds %d rows, the noun file %d" % (verb_pred.shape[0], noun_pred.shape[0])
    verb, noun = softmax_rows(verb_pred, device), softmax_rows(noun_pred, device)
    action_freq = get_training_action_freq(verb_pred.shape[1], noun_pred.shape[1], annotation_root)
    prior = torch.from_numpy(verb_given_noun(action_freq).astype(np.float32)).to(device)
    hits, rows = topk_accuracies(verb, noun, torch.from_numpy(verb_labels).to(device), torch.from_numpy(noun_labels).to(device),
                                 prior)
    out = {}
    for k in KS:
        for name, title in (("verb", "Verbs:"), ("noun", "Nouns:"), ("action", "Actions:")):
            accuracy = 100.0 * float(hits[name][k]) / rows
            logger.info(title)
            logger.info('Top-%d: %.04f%%' % (k, accuracy))
            out["%s_top%d" % (name, k)] = accuracy
    return out
