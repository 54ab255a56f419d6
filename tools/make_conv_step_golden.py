"""Writes the two snapshots tests/test_conv_step_golden.py replays.  tests/golden/conv_steps.json.gz: what ConvStep.setup() decides for
every conv of the dry-run engines of the benchmarked presets (the matrix of tools/make_conv_plan_golden.py) and of the grouped
model -- stored descriptors, format flags, operand buffer shapes -- with the engine's scratch requests, the fp16-copy flags
of the root blobs, the backward order and the plan table; plus one section per engine A/B switch, evaluated in a child process
with that variable set.  tests/golden/engine_plans.json.gz: what Engine.plan() decides around the convs (record_plan there)
for those engines and the variants of plan_keys(), with the sections of PLAN_SWITCHES.  Identical descriptors, step / blob
records and lists are stored once and referred to by index.  Needs the built library, no GPU.

    python tools/make_conv_step_golden.py [--commit ID] [--only steps|plans]

Regenerate a file only when what it records is MEANT to change; a refactor of the planner must pass against both as they are.
The generator is deterministic: on an unchanged engine and with the same --commit it rewrites each file byte for byte."""
import argparse
import gzip
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "video-long-term-feature-banks_amd", "lib"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import conv_desc_ref as cr                      # noqa: E402
import test_conv_step_golden as snap            # noqa: E402
from make_conv_plan_golden import MAX_BYTES     # noqa: E402


class Table(object):
    """values stored once, in order of first use"""

    def __init__(self):
        self.rows, self.index = [], {}

    def add(self, v):
        k = json.dumps(v, sort_keys=True)
        if k not in self.index:
            self.index[k] = len(self.rows)
            self.rows.append(v)
        return self.index[k]


def write(path, out):
    with gzip.GzipFile(path, "wb", compresslevel=9, mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    size = os.path.getsize(path)
    assert size < MAX_BYTES, "snapshot of %d bytes" % size
    return size


def steps_snapshot(commit):
    fields = list(cr.FIELDS)
    descs, steps, lists = Table(), Table(), Table()
    sections = {"": snap.evaluate(snap.default_keys())}
    print("default: %d engines" % len(sections[""]), flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        for sw in snap.SWITCHES:
            sections[sw] = snap.evaluate_in_child(snap.switch_keys(), sw, tmp)
            print("%s: %d engines" % (sw, len(sections[sw])), flush=True)
    out = {"commit": commit, "fields": fields, "sections": {}}
    for name, sec in sections.items():
        out["sections"][name] = {}
        for key, e in sec.items():
            if "error" in e:
                out["sections"][name][key] = e
                continue
            ix = [steps.add(dict(s, descs={k: descs.add([d[f] for f in fields]) for k, d in s["descs"].items()})) for s in e["steps"]]
            out["sections"][name][key] = {"engine": e["engine"], "steps": ix, "roots": lists.add(e["roots"]),
                                          "bwd_steps": lists.add(e["bwd_steps"]), "plan_table": lists.add(e["plan_table"])}
    out.update(descs=descs.rows, steps=steps.rows, lists=lists.rows)
    size = write(snap.GOLDEN, out)
    print("%s: commit %s, %d engines, %d step records, %d descriptors, %d bytes" % (
        os.path.relpath(snap.GOLDEN, ROOT), commit, sum(len(s) for s in sections.values()), len(steps.rows), len(descs.rows), size))


def plans_snapshot(commit):
    fields = list(cr.FIELDS)
    descs, rows, lists = Table(), Table(), Table()
    sections = {"": snap.evaluate(snap.plan_keys(), snap.record_plan)}
    print("default: %d engines" % len(sections[""]), flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        for sw in snap.PLAN_SWITCHES:
            sections[sw] = snap.evaluate_in_child(snap.switch_keys(), sw, tmp, "plans")
            print("%s: %d engines" % (sw, len(sections[sw])), flush=True)
    out = {"commit": commit, "fields": fields, "root_fields": list(snap.ROOT_FIELDS), "sections": {}}
    for name, sec in sections.items():
        out["sections"][name] = {}
        for key, e in sec.items():
            if "error" in e:
                out["sections"][name][key] = e
                continue
            e = dict(e, attention=[rows.add(dict(a, descs={k: descs.add([d[f] for f in fields]) for k, d in a["descs"].items()}))
                                   for a in e["attention"]])
            for k in ("steps", "roots", "pools"):
                e[k] = [rows.add(r) for r in e[k]]
            out["sections"][name][key] = {k: lists.add(v) for k, v in e.items()}
    out.update(descs=descs.rows, rows=rows.rows, lists=lists.rows)
    size = write(snap.PLANS_GOLDEN, out)
    print("%s: commit %s, %d engines, %d records, %d lists, %d descriptors, %d bytes" % (
        os.path.relpath(snap.PLANS_GOLDEN, ROOT), commit, sum(len(s) for s in sections.values()), len(rows.rows), len(lists.rows),
        len(descs.rows), size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="commit the snapshot is taken on (default: git rev-parse HEAD)")
    ap.add_argument("--only", choices=("steps", "plans"), default=None, help="write one of the two files")
    args = ap.parse_args()
    commit = args.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"]).decode().strip()
    if args.only != "plans":
        steps_snapshot(commit)
    if args.only != "steps":
        plans_snapshot(commit)


if __name__ == "__main__":
    main()
