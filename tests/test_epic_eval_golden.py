"""vlfb.epic_eval against tests/golden/ref_epic_eval.json.gz: the reference's whole evaluate_actions
(tools/evaluate_actions.py:109-141) run by tools/make_ref_epic_eval_golden.py on seeded inputs.

Host part (no GPU): the (verb, noun) frequency table and the prior v_given_n.  Counts are compared exactly.  The prior is
what the kernel multiplies with, an fp32 table, against the reference's fp64 one: the reference forms the action score as
an fp64 product (fp32 scores times the fp64 prior) that it rounds once when it stores it, the kernel rounds the prior first,
so the two tables can differ by the rounding of one fp32 store: 1 ulp of fp32 is the bound.
GPU part: the six figures.  The generator asserted that no label score is tied and that every score pair that decides a
hit is 2^-14 apart relatively, so the device softmax and the fp32 prior product cannot move a hit: the figures are equal."""
import base64
import gzip
import json
import os
import pickle

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_epic_eval.json.gz")


def load():
    with gzip.open(GOLDEN, "rb") as f:
        g = json.loads(f.read().decode())
    assert g["tie_check"] is True and g["rows"] <= 1000
    arr = lambda key, cols: np.frombuffer(base64.b64decode(g[key]), dtype=np.float16).reshape(g["rows"], cols).astype(np.float32)
    g["verb"], g["noun"] = arr("verb_f16", g["V"]), arr("noun_f16", g["Nn"])
    g["v_given_n"] = np.array([[float.fromhex(x) for x in row] for row in g["v_given_n_hex"]], dtype=np.float64)
    return g


def write_inputs(g, tmp):
    with open(os.path.join(str(tmp), "EPIC_train_action_labels.csv"), "w") as f:
        f.write(g["annotation_header"] + "\n" + "\n".join(g["annotation_lines"]) + "\n")
    files = []
    for name, pred, lab in (("verb", g["verb"], g["verb_labels"]), ("noun", g["noun"], g["noun_labels"])):
        files.append(os.path.join(str(tmp), "epic_predictions_%s.pkl" % name))
        with open(files[-1], "wb") as f:
            pickle.dump((pred, np.asarray(lab, dtype=np.int32)), f, 2)
    return files


def test_frequency_table_and_prior_match_the_reference(tmp_path):
    from vlfb import epic_eval
    g = load()
    write_inputs(g, tmp_path)
    persons = [int(l.split(",")[1][1:]) for l in g["annotation_lines"]]
    assert min(persons) <= 25 < max(persons)                       # participants on both sides of the split
    counts = epic_eval.training_action_counts(g["V"], g["Nn"], str(tmp_path))
    assert counts.dtype == np.int64 and np.array_equal(counts, np.array(g["counts"])) and int(counts.sum()) == g["count_total"]
    assert int(counts.sum()) < len(persons)                        # (the held-out participants' rows are not counted)
    freq = epic_eval.get_training_action_freq(g["V"], g["Nn"], str(tmp_path))
    assert freq.dtype == np.float64 and np.array_equal(freq, np.array(g["counts"]) / float(g["count_total"]))
    prior32 = epic_eval.verb_given_noun(freq).astype(np.float32)
    ref = g["v_given_n"]
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    worst = float(np.max(np.abs(prior32.astype(np.float64) - ref) / ulp))
    print("prior: worst |fp32 table - reference fp64 table| = %.3f ulp of fp32" % worst)
    assert worst <= 1.0 and np.array_equal(prior32 == 0, ref == 0)


@pytest.mark.gpu
def test_the_six_figures_match_the_reference(tmp_path):
    from vlfb import epic_eval
    g = load()
    verb_file, noun_file = write_inputs(g, tmp_path)
    got = epic_eval.evaluate_actions(verb_file, noun_file, str(tmp_path))
    want = {name: 100.0 * fig["hits"] / g["rows"] for name, fig in g["figures"].items()}
    print(got, want)
    assert got == want
    for name, fig in g["figures"].items():
        assert "%.04f" % got[name] == fig["logged"]                # what the reference logged, to its four decimals
