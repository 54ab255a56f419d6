"""Snapshot of what ConvStep.setup() decides (tests/golden/conv_steps.json.gz, written by tools/make_conv_step_golden.py), with
the built library and no GPU: for every conv step of the dry-run engines of the benchmarked presets -- four presets x five
dtypes x {2 clips of 16 x 64^2, 8 clips of 32 x 224^2} x {train, test} -- and of the grouped model, every stored descriptor
field by field, the format decisions, the shapes and dtypes of the operand buffers; per engine the scratch requests, the
fp16-copy flags of the root blobs, the order of the backward steps and the plan table.  One further section per engine A/B
switch (the ava_r50_lfb_nl engines on mix and split), each replayed in a child process with that variable set, because the
switches are read when vlfb.engine is imported.  Everything must come out exactly as recorded.

Run as a program (`python test_conv_step_golden.py KEYS.json`): prints {key: record} of the engine keys listed in KEYS.json --
the child of the switch sections, here and in the generator."""
import gzip
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "conv_steps.json.gz")
# one section of the snapshot per engine A/B switch away from its default
SWITCHES = ("VLFB_MIX_W2=0", "VLFB_MIX_W2I=0", "VLFB_SPLIT_MATH=6,3", "VLFB_MIX_NL_F32=0", "VLFB_MIX_TRUNK2=0",
            "VLFB_GRAD_HALF_COPY=0")
GROUPED = ["RESNETS.NUM_GROUPS", 2, "RESNETS.WIDTH_PER_GROUP", 32]      # test_model_gpu.test_grouped_convolution_model
STEP_FLAGS = ("w2", "w2i", "bwd_split", "bwd_f32", "dx_f32", "x_pair", "o_pair", "sparse_dgrad", "half_by_copy",
              "dgrad_takes_planes", "fprop_takes_planes")
STEP_VALUES = ("wcode", "wf_npl", "wd_npl", "wblk", "Cog", "Cin_k", "gscale", "pack", "params")
STEP_TENSORS = ("w_f", "w_d", "x_planes", "g_planes")
ENGINE_VALUES = ("_ws_bytes", "_sf32", "_sact", "_spl", "_sjoin")


def _tools():
    p = os.path.join(ROOT, "tools")
    if p not in sys.path:
        sys.path.insert(0, p)
    import make_conv_plan_golden as plans
    return plans


def default_keys():
    """engine keys "preset|dtype|clips|frames|crop|split[|grouped]" of the section without a switch"""
    plans = _tools()
    keys = ["%s|%s|%d|%d|%d|%s" % (preset, dtype, c, f, s, split) for preset in plans.BASELINE_PRESETS for dtype in plans.DTYPES
            for c, f, s in plans.SIZES for split in ("train", "test")]
    c, f, s = plans.SIZES[0]
    return keys + ["charades_r50_baseline|%s|%d|%d|%d|train|grouped" % (dtype, c, f, s) for dtype in plans.DTYPES]


def switch_keys():
    plans = _tools()
    return ["ava_r50_lfb_nl|%s|%d|%d|%d|%s" % (dtype, c, f, s, split) for dtype in ("mix", "split") for c, f, s in plans.SIZES
            for split in ("train", "test")]


def build(key):
    plans = _tools()
    parts = key.split("|")
    preset, dtype, (clips, frames, crop), split = parts[0], parts[1], (int(x) for x in parts[2:5]), parts[5]
    return plans.dry_engine(preset, dtype, clips, frames, crop, split, overrides=GROUPED if len(parts) > 6 else ())


def record(eng):
    """everything ConvStep.setup() leaves behind, on the steps and on the engine, as plain JSON values"""
    import conv_desc_ref as cr
    from vlfb import hip
    from vlfb.engine import ConvStep
    steps = []
    for st in eng.steps:
        if not isinstance(st, ConvStep):
            continue
        r = {"name": st.name(), "taps": st.taps(), "group": st.group,
             "descs": {k: cr.desc_dict(v) for k, v in sorted(vars(st).items()) if isinstance(v, hip.ConvDesc)},
             "eff_bias": st.eff_bias is not None, "cb_tmp": getattr(st, "cb_tmp", None) is not None}
        for k in STEP_FLAGS:
            r[k] = bool(getattr(st, k, False))
        for k in STEP_VALUES:
            r[k] = getattr(st, k)
        for k in STEP_TENSORS:
            t = getattr(st, k)
            r[k] = None if t is None else [list(t.shape), str(t.dtype)]
        steps.append(r)
    roots = [[b.name] + [bool(getattr(b, k, False)) for k in ("need_half", "grad_half", "grad_half_src")]
             for b in eng.all_blobs if b.root is b]
    return {"steps": steps, "engine": {k: int(getattr(eng, k, 0)) for k in ENGINE_VALUES}, "roots": roots,
            "bwd_steps": [st.name() for st in getattr(eng, "bwd_steps", [])], "plan_table": [list(r) for r in eng.plan_table()]}


def evaluate(keys):
    """{key: record}; an engine the switch makes impossible (`mix` under VLFB_SPLIT_MATH=6,3) is recorded as its error text"""
    from vlfb import hip
    out = {}
    for k in keys:
        try:
            # (through JSON, so that what is compared is what the file can hold: lists for tuples, exact doubles)
            out[k] = json.loads(json.dumps(record(build(k))))
        except hip.VlfbError as e:
            out[k] = {"error": str(e)}
    return out


def evaluate_in_child(keys, switch, tmp_dir):
    """evaluate() in a fresh process with the switch `NAME=VALUE` set"""
    path = os.path.join(str(tmp_dir), "conv_step_keys_%s.json" % switch.replace("=", "_").replace(",", "_"))
    with open(path, "w") as f:
        json.dump(list(keys), f)
    name, value = switch.split("=")
    env = dict(os.environ)
    env[name] = value
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, stdout=subprocess.PIPE, check=True)
    return json.loads(r.stdout.decode())


def load():
    """{section: {engine key: record}} with the shared descriptors and step records put back in place"""
    with gzip.open(GOLDEN, "rt") as f:
        g = json.load(f)
    descs = [dict(zip(g["fields"], row)) for row in g["descs"]]
    steps = [dict(s, descs={k: descs[i] for k, i in s["descs"].items()}) for s in g["steps"]]
    lists = g["lists"]
    sections = {name: {key: e if "error" in e else dict(e, steps=[steps[i] for i in e["steps"]], roots=lists[e["roots"]], bwd_steps=lists[e["bwd_steps"]],
                                 plan_table=lists[e["plan_table"]]) for key, e in sec.items()}
                for name, sec in g["sections"].items()}
    return g, sections


def differences(want, got):
    out = []
    for key in want:
        w, g = want[key], got.get(key)
        if g is None:
            out.append("%s: not evaluated" % key)
            continue
        if "error" in w or "error" in g:
            if w != g:
                out.append("%s: recorded %r, got %r" % (key, w.get("error", "an engine"), g.get("error", "an engine")))
            continue
        for part in ("engine", "roots", "bwd_steps", "plan_table"):
            if w[part] != g[part]:
                out.append("%s: %s differs: recorded %r, got %r" % (key, part, w[part], g[part]) if part == "engine" else
                           "%s: %s differs, first at %r" % (key, part, next(((a, b) for a, b in zip(w[part], g[part]) if a != b),
                                                                              (len(w[part]), len(g[part])))))
        if [s["name"] for s in w["steps"]] != [s["name"] for s in g["steps"]]:
            out.append("%s: the conv steps differ" % key)
            continue
        for a, b in zip(w["steps"], g["steps"]):
            for k in a:
                if k == "descs":
                    if sorted(a[k]) != sorted(b[k]):
                        out.append("%s %s: descriptors %s, recorded %s" % (key, a["name"], sorted(b[k]), sorted(a[k])))
                        continue
                    for dn in a[k]:
                        bad = {f: (a[k][dn][f], b[k][dn][f]) for f in a[k][dn] if a[k][dn][f] != b[k][dn][f]}
                        if bad:
                            out.append("%s %s.%s: (recorded, got) %r" % (key, a["name"], dn, bad))
                elif a[k] != b.get(k):
                    out.append("%s %s: %s recorded %r, got %r" % (key, a["name"], k, a[k], b.get(k)))
    return out


def test_setup_reproduces_the_snapshot():
    g, sections = load()
    want = sections[""]
    assert sorted(want) == sorted(default_keys())
    bad = differences(want, evaluate(sorted(want)))
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:30]))


@pytest.mark.parametrize("switch", SWITCHES)
def test_setup_under_a_switch_reproduces_the_snapshot(switch, tmp_path):
    g, sections = load()
    want = sections[switch]
    assert sorted(want) == sorted(switch_keys())
    bad = differences(want, evaluate_in_child(sorted(want), switch, tmp_path))
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:30]))


def test_snapshot_covers_every_format_decision():
    """what the snapshot is for: every branch of the format decisions has at least one conv in it, and every weight-operand
    format the engines produce (hip.py: the dtype codes on the 16-bit / fp32 paths, SPLIT, MIX, MIX_W2, MIX_W2I and the
    MIXH* forms of a two-plane input) is there"""
    from vlfb import hip
    g, sections = load()
    assert sorted(sections) == sorted(("",) + SWITCHES)
    steps = [s for sec in sections.values() for e in sec.values() for s in e.get("steps", [])]
    assert len(g["steps"]) > 500
    assert any(s["w2i"] for s in steps)
    assert any(s["w2"] and not s["w2i"] for s in steps)
    for flag in ("bwd_split", "dx_f32", "x_pair", "o_pair"):
        assert any(s[flag] for s in steps), flag
    assert any("d_d_full" in s["descs"] for s in steps)
    assert any(s["group"] > 1 for s in steps)
    assert any(s["descs"]["d_w"]["wgrad_bias"] == 1 for s in steps if "d_w" in s["descs"])
    assert {s["wcode"] for s in steps} == set(WCODES(hip)), sorted({s["wcode"] for s in steps})


def WCODES(hip):
    # every wcode the engines of the snapshot's matrix give a conv (derived on the commit the snapshot was taken on)
    return (hip.F16, hip.BF16, hip.F32, hip.SPLIT, hip.MIX, hip.MIX_W2, hip.MIX_W2I, hip.MIXH, hip.MIXH_W2, hip.MIXH_W2I)


if __name__ == "__main__":
    for p in (os.path.join(ROOT, "video-long-term-feature-banks_amd", "lib"), ROOT, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    with open(sys.argv[1]) as f:
        print(json.dumps(evaluate(json.load(f))))
