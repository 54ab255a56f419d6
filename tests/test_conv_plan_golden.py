"""Snapshot of the conv planner (tests/golden/conv_plans.json.gz, written by tools/make_conv_plan_golden.py), with the built
library and no GPU: the planner is a pure host function of the descriptor (and of the planner's A/B switches, read once per
process), so every recorded descriptor must still give the recorded return code, plan string (or vlfb_last_error text where
planning fails) and workspace size, exactly.  The descriptors are every ConvDesc the dry-run engines of the benchmarked
presets store, their shrunk forms, each with `algo` forced to every VLFB_ALGO_* value, WGRADs with `wgrad_bias` toggled and
split-bf16 launches with pre-split operands;
one further section per planner switch, each replayed in a child process of its own with that variable set.

Run as a program (`python test_conv_plan_golden.py IN.json`): evaluates the descriptor rows of IN.json in this process and
prints [[rc, text, workspace_bytes], ...] -- the child of the switch sections, here and in the generator."""
import ctypes as C
import gzip
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "conv_plans.json.gz")
# one section of the snapshot per planner A/B switch away from its default
SWITCHES = ("VLFB_SPLIT_S2=0", "VLFB_SPLIT_S2_1X1=1", "VLFB_PAIR_PIPE256=0", "VLFB_PAIR_PIPE256=1", "VLFB_PAIR_STEM_DIRECT=0",
            "VLFB_SKINNY=0", "VLFB_PAIR_PRE_KT=8")


def evaluate(fields, rows):
    """[(rc, plan string or error text, workspace bytes)] of descriptor rows (values in the order of `fields`)"""
    from vlfb import hip
    lib = hip.lib()
    out = []
    buf = C.create_string_buffer(128)
    for row in rows:
        d = hip.conv_desc(**dict(zip(fields, row)))
        rc = lib.vlfb_conv_plan_describe(C.byref(d), buf, 128)
        text = buf.value.decode() if rc == 0 else lib.vlfb_last_error().decode()
        out.append((int(rc), text, int(lib.vlfb_conv_workspace_bytes(C.byref(d)))))
    return out


def evaluate_in_child(fields, rows, switch, tmp_dir):
    """evaluate() in a fresh process with the switch `NAME=VALUE` set"""
    path = os.path.join(str(tmp_dir), "conv_plan_rows_%s.json" % switch.replace("=", "_"))
    with open(path, "w") as f:
        json.dump({"fields": list(fields), "rows": rows}, f)
    name, value = switch.split("=")
    env = dict(os.environ)
    env[name] = value
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, stdout=subprocess.PIPE, check=True)
    return [tuple(x) for x in json.loads(r.stdout.decode())]


def load():
    with gzip.open(GOLDEN, "rt") as f:
        g = json.load(f)
    const = g["const"]
    fields = list(g["fields"]) + sorted(const)
    tail = [const[k] for k in sorted(const)]
    sections = {}
    for name, recs in g["sections"].items():
        n = len(g["fields"])
        sections[name] = ([list(r[:n]) + tail for r in recs], [(r[n], g["texts"][r[n + 1]], r[n + 2]) for r in recs])
    return g, fields, sections


def mismatches(fields, rows, want, got):
    return ["%s: recorded %r, got %r" % (dict((k, v) for k, v in zip(fields, row) if v), w, g)
            for row, w, g in zip(rows, want, got) if tuple(w) != tuple(g)]


def test_planner_reproduces_the_snapshot():
    g, fields, sections = load()
    rows, want = sections[""]
    assert len(rows) > 1000
    bad = mismatches(fields, rows, want, evaluate(fields, rows))
    assert not bad, "%d of %d records differ:\n%s" % (len(bad), len(rows), "\n".join(bad[:20]))


@pytest.mark.parametrize("switch", SWITCHES)
def test_planner_switches_reproduce_the_snapshot(switch, tmp_path):
    g, fields, sections = load()
    rows, want = sections[switch]
    assert rows
    bad = mismatches(fields, rows, want, evaluate_in_child(fields, rows, switch, tmp_path))
    assert not bad, "%d of %d records differ:\n%s" % (len(bad), len(rows), "\n".join(bad[:20]))


def test_snapshot_covers_every_family_and_the_rejections():
    """what the snapshot is for: every family name the planner can print, and planning failures, are in it"""
    g, _, sections = load()
    assert sorted(sections) == sorted(("",) + SWITCHES)
    fams = {t.split()[0] for name in sections for rc, t, _ in sections[name][1] if rc == 0}
    assert fams >= {"tn", "tn_tr", "tn8", "stem_wgrad", "wgrad_rows", "wgrad_rows_fat", "tn_split", "tn_tr_planes", "nt", "nt8",
                    "nt_stream", "conv_rows64", "stem_fprop", "nt_skinny", "nt_skinny_split", "nt_split", "nt_planes",
                    "nt_pair", "nt8_pair", "stem_fprop_pair"}, sorted(fams)
    assert any(rc != 0 and ws == -1 for rc, _, ws in sections[""][1])


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "video-long-term-feature-banks_amd", "lib"))
    with open(sys.argv[1]) as f:
        job = json.load(f)
    print(json.dumps(evaluate(job["fields"], job["rows"])))
