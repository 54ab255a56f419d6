"""Run the REFERENCE's whole evaluate_actions (tools/evaluate_actions.py:109-141) on seeded inputs and commit inputs + outputs.

TEST INFRASTRUCTURE ONLY.  Needs the reference checkout:

    python tools/make_ref_epic_eval_golden.py          # writes tests/golden/ref_epic_eval.json.gz

Inputs: two seeded prediction pickles (verb [rows][V], noun [rows][Nn]: softmax outputs, as the test pass stores them, kept
to fp16 precision so that the file is small and every value is exact in fp32) and a small EPIC_train_action_labels.csv
with participants on both sides of P25.  NUM_TEST_SEG is set to the case's rows (<= 1000, so a logged 'Top-%d: %.04f%%'
resolves one hit).  Recorded: the inputs, get_training_action_freq's table (as the integer counts whose quotient by their sum it equals),
v_given_n (float64, as hex strings) and the six logged figures.

The reference's argsort is not stable and the product's device softmax is not numpy's, so the generator ASSERTS, and
records that it checked (meta["tie_check"]), that no hit can hinge on either: in every row the label's score differs
from every other score of its row, before and after the second softmax, and so does the label's action product; and
wherever the label sits at a top-1 / top-5 boundary (rank k - 1 or k), the two scores at the boundary are at least
MARGIN apart relatively -- 2^-14, against the few 2^-24 steps by which two fp32 softmax implementations, or the reference's
fp64 prior product and the kernel's fp32 one, can differ.  The seed is searched on the CPU until the reference alone
satisfies this."""
import base64
import gzip
import importlib.util
import json
import logging
import os
import pickle
import re
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "ref_epic_eval.json.gz")
ROWS, V, NN = 96, 12, 30
MARGIN = 2.0 ** -14
HEADER = "uid,participant_id,video_id,narration,start_timestamp,stop_timestamp,start_frame,stop_frame,verb,verb_class,noun," \
         "noun_class,all_nouns,all_noun_classes"


def label_distinct(scores, idx):
    rows = np.arange(scores.shape[0])
    return bool(np.all((scores == scores[rows, idx][:, None]).sum(axis=1) == 1))


def boundary_clear(scores, idx, ks=(1, 5)):
    """where the label's rank is k - 1 or k, the k-th and (k + 1)-th largest scores are MARGIN apart (relatively)"""
    order = -np.sort(-scores.astype(np.float64), axis=1)
    label = scores[np.arange(scores.shape[0]), idx].astype(np.float64)
    rank = (scores.astype(np.float64) > label[:, None]).sum(axis=1)
    for k in ks:
        at = (rank == k - 1) | (rank == k)
        hi, lo = order[at, k - 1], order[at, k]
        if np.any(hi - lo < MARGIN * hi):
            return False
    return True


def make_inputs(seed):
    rng = np.random.RandomState(seed)

    def head(cols):
        labels = rng.randint(0, cols, ROWS).astype(np.int32)
        logits = rng.randn(ROWS, cols).astype(np.float32) * 2.0
        hot = rng.rand(ROWS) < 0.6
        logits[np.arange(ROWS)[hot], labels[hot]] += rng.uniform(1.0, 4.0, hot.sum()).astype(np.float32)
        e = np.exp(logits - logits.max(axis=1, keepdims=True))
        pred = (e / e.sum(axis=1, keepdims=True)).astype(np.float16).astype(np.float32)
        return pred, labels
    verb, vl = head(V)
    noun, nl = head(NN)
    lines = []

    def line(person, v, n):
        uid = len(lines)
        lines.append('%d,P%02d,P%02d_%02d,do it,00:00:01.00,00:00:02.00,60,120,verb,%d,noun,%d,"[\'noun\']","[%d]"'
                     % (uid, person, person, uid % 7, v, n, n))
    for r in range(ROWS):                                     # every test row's pair is seen in training: no label product is 0
        line(int(rng.randint(1, 26)), int(vl[r]), int(nl[r]))
    for _ in range(80):                                       # ... among other pairs, a third of them of held-out participants
        line(int(rng.randint(1, 33)), int(rng.randint(0, V)), int(rng.randint(0, NN)))
    order = rng.permutation(len(lines))
    lines = [lines[i] for i in order]
    return verb, vl, noun, nl, lines


def main():
    sys.path.insert(0, ROOT)
    sys.modules.setdefault("cPickle", pickle)
    spec = importlib.util.spec_from_file_location("ref_evaluate_actions", os.path.join(REF, "tools", "evaluate_actions.py"))
    EA = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(EA)
    assert os.path.realpath(EA.__file__).startswith(REF)
    logged = []

    class Grab(logging.Handler):
        def emit(self, record):
            logged.append(record.getMessage())
    EA.logger.addHandler(Grab())
    EA.NUM_TEST_SEG = ROWS
    assert ROWS <= 1000

    for seed in range(20240700, 20240800):
        verb, vl, noun, nl, lines = make_inputs(seed)
        with tempfile.TemporaryDirectory() as tmp:
            with open(os.path.join(tmp, "EPIC_train_action_labels.csv"), "w") as f:
                f.write(HEADER + "\n" + "\n".join(lines) + "\n")
            persons = [int(l.split(",")[1][1:]) for l in lines]
            assert min(persons) <= 25 < max(persons)
            freq = EA.get_training_action_freq(V, NN, tmp)
            v_given_n = freq / (np.sum(freq, axis=1, keepdims=True) + 1e-5)
            verb2, noun2 = EA.softmax(verb), EA.softmax(noun)
            actions = np.stack([np.outer(verb2[i], noun2[i]) for i in range(ROWS)])
            actions *= v_given_n                                   # in place, as compute_top_k_actions does: fp64 product, fp32 store
            flat = actions.reshape(ROWS, -1)
            assert verb2.dtype == noun2.dtype == flat.dtype == np.float32
            ok = (label_distinct(verb, vl) and label_distinct(noun, nl) and label_distinct(verb2, vl) and label_distinct(noun2, nl)
                  and label_distinct(flat, vl * NN + nl) and boundary_clear(verb2, vl) and boundary_clear(noun2, nl)
                  and boundary_clear(flat, vl * NN + nl))
            if not ok:
                continue
            for name, pred, lab in (("verb.pkl", verb, vl), ("noun.pkl", noun, nl)):
                with open(os.path.join(tmp, name), "wb") as f:
                    pickle.dump((pred, lab), f, 2)
            del logged[:]
            EA.evaluate_actions(types.SimpleNamespace(verb_file=os.path.join(tmp, "verb.pkl"), noun_file=os.path.join(tmp, "noun.pkl"),
                                                      annotation_root=tmp))
        break
    else:
        raise SystemExit("no seed satisfies the tie conditions")

    # 'Verbs:', 'Top-1: x%', 'Nouns:', 'Top-1: x%', 'Actions:', 'Top-1: x%', then the same for K = 5
    assert [m for m in logged if not m.startswith("Top-")] == ["Verbs:", "Nouns:", "Actions:"] * 2, logged
    tops = [re.match(r"Top-(\d+): ([0-9.]+)%", m).groups() for m in logged if m.startswith("Top-")]
    assert [int(k) for k, _ in tops] == [1, 1, 1, 5, 5, 5]
    figures = {}
    for (k, acc), name in zip(tops, ["verb", "noun", "action"] * 2):
        hits = int(round(float(acc) * ROWS / 100.0))
        assert abs(100.0 * hits / ROWS - float(acc)) < 1e-3
        figures["%s_top%s" % (name, k)] = {"logged": acc, "hits": hits}
    counts = np.zeros((V, NN), dtype=np.int64)                # counted again here, from the lines themselves
    for l in lines:
        f = l.split(",")
        if int(f[1][1:]) <= 25:
            counts[int(f[9]), int(f[11])] += 1
    total = int(counts.sum())
    assert np.array_equal(counts / float(total), freq), "the table is not counts / their sum"
    b64 = lambda a: base64.b64encode(np.ascontiguousarray(a).tobytes()).decode()
    meta = {
        "generator": "tools/make_ref_epic_eval_golden.py", "seed": seed, "rows": ROWS, "V": V, "Nn": NN, "margin": MARGIN,
        "tie_check": True,
        "verb_f16": b64(verb.astype(np.float16)), "noun_f16": b64(noun.astype(np.float16)),
        "verb_labels": vl.tolist(), "noun_labels": nl.tolist(), "annotation_header": HEADER, "annotation_lines": lines,
        "counts": counts.tolist(), "count_total": total,
        "v_given_n_hex": [[float(x).hex() for x in row] for row in v_given_n],
        "figures": figures,
    }
    assert np.array_equal(verb.astype(np.float16).astype(np.float32), verb)
    data = gzip.compress(json.dumps(meta, sort_keys=True).encode(), mtime=0)
    assert len(data) <= 64 * 1024, len(data)
    with open(OUT, "wb") as f:
        f.write(data)
    print("wrote %s: %d bytes, seed %d" % (os.path.normpath(OUT), len(data), seed))
    print(json.dumps(figures, sort_keys=True))


if __name__ == "__main__":
    main()
