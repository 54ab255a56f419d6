"""Snapshot of what ConvStep.setup() decides (tests/golden/conv_steps.json.gz, written by tools/make_conv_step_golden.py), with
the built library and no GPU: for every conv step of the dry-run engines of the benchmarked presets -- four presets x five
dtypes x {2 clips of 16 x 64^2, 8 clips of 32 x 224^2} x {train, test} -- and of the grouped model, every stored descriptor
field by field, the format decisions, the shapes and dtypes of the operand buffers; per engine the scratch requests, the
fp16-copy flags of the root blobs, the order of the backward steps and the plan table.  One further section per engine A/B
switch (the ava_r50_lfb_nl engines on mix and split), each replayed in a child process with that variable set, because the
switches are read when vlfb.engine is imported.  Everything must come out exactly as recorded.

A second snapshot (tests/golden/engine_plans.json.gz, same generator, same machinery) holds what Engine.plan() decides around
the convs, for the same engines and for the dot-product non-local model, the spatial-BN graph, a test net that shares its
parameters with the train net and the one-bank-per-clip inference plan: the step list, every root blob with its storage and
its gradient slot, the fp32 head, the two-plane blobs, the parameter layouts and solver buckets, the forward-branch and
half-copy plans, every attention and pool descriptor; with further sections for the A/B switches of the shipped paths.

Run as a program (`python test_conv_step_golden.py KEYS.json [plans]`): prints {key: record} of the engine keys listed in
KEYS.json (`plans`: the records of the second snapshot) -- the child of the switch sections, here and in the generator."""
import gzip
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "conv_steps.json.gz")
PLANS_GOLDEN = os.path.join(HERE, "golden", "engine_plans.json.gz")
# one section of the snapshot per engine A/B switch away from its default
SWITCHES = ("VLFB_MIX_W2=0", "VLFB_MIX_W2I=0", "VLFB_SPLIT_MATH=6,3", "VLFB_MIX_NL_F32=0", "VLFB_MIX_TRUNK2=0",
            "VLFB_GRAD_HALF_COPY=0")
# the sections of the plan snapshot: those, and the off-paths of the shipped two-plane / forward-branch plans
PLAN_SWITCHES = SWITCHES + ("VLFB_MIX_PAIR=0", "VLFB_PAIR_ATTN_OUT=0", "VLFB_PAIR_SCORES=0", "VLFB_FORWARD_BANK_SIDE=0")
GROUPED = ["RESNETS.NUM_GROUPS", 2, "RESNETS.WIDTH_PER_GROUP", 32]      # test_model_gpu.test_grouped_convolution_model
# the variants of an engine key (its seventh part): config overrides ...
VARIANTS = {"grouped": GROUPED,
            "dot": ["NONLOCAL.USE_SOFTMAX", False],                     # test_lowering.test_dot_product_nonlocal_variant_...
            "bn": ["MODEL.USE_AFFINE", False, "NONLOCAL.USE_BN", True, "NONLOCAL.USE_AFFINE", False,
                   "MODEL.DILATIONS_AFTER_CONV5", False],               # test_lowering.test_spatial_bn_graph_lowers_to_bn_steps
            # ... a test net that aliases the parameters of the train net, the `lfb` blob with one row per clip
            "shared": [], "clipbank": []}
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


def plan_keys():
    """engine keys of the plan snapshot's section without a switch: those of default_keys() and the variants they leave out"""
    plans = _tools()
    c, f, s = plans.SIZES[0]
    size = "%d|%d|%d" % (c, f, s)
    keys = ["charades_r50_baseline|%s|%s|%s|dot" % (dtype, size, split) for dtype in plans.DTYPES for split in ("train", "test")]
    keys += ["ava_r50_lfb_nl|%s|%s|%s|bn" % (dtype, size, split) for dtype in ("split", "fp32", "fp16", "bf16")
             for split in ("train", "test")]
    keys += ["ava_r50_lfb_nl|%s|%s|test|%s" % (dtype, size, v) for dtype in ("mix", "fp16") for v in ("shared", "clipbank")]
    # 256^2 crops: the 1024 keys of a res3 non-local block, where the library reports the fused attention backward as faster
    keys += ["charades_r50_baseline|%s|2|32|256|train" % dtype for dtype in ("mix", "fp16", "bf16")]
    return default_keys() + keys


def build(key):
    plans = _tools()
    parts = key.split("|")
    preset, dtype, (clips, frames, crop), split = parts[0], parts[1], (int(x) for x in parts[2:5]), parts[5]
    variant = parts[6] if len(parts) > 6 else None
    kw = dict(overrides=VARIANTS[variant]) if variant else {}
    if variant == "shared":
        kw.update(share_params_with=plans.dry_engine(preset, dtype, clips, frames, crop, "train"))
    if variant == "clipbank":
        kw.update(bank_per_clip=True)
    return plans.dry_engine(preset, dtype, clips, frames, crop, split, **kw)


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


ROOT_FIELDS = ("name", "kind", "shape", "caxis", "relu", "needs_grad", "dead", "is_input", "pad_c", "pad_w", "pair", "grad_f32",
               "grad_scale", "need_half", "grad_half", "grad_half_src", "half", "planes", "tensor", "expected", "two_term",
               "buf", "buf_lo", "half_buf", "slot_planes")
ENGINE_LISTS = ("head_f32", "head_f32_fbo", "pair_blobs", "train_order", "train_layout", "frozen_layout", "wd_ranges",
                "shared_params", "fwd_early", "fwd_side", "fwd_wait", "fwd_signal", "half_post", "half_inputs")
ATTENTION_FLAGS = ("single", "s_pair", "o_pair", "precise", "bsplit", "fused_fwd", "fused_bwd", "dy_f32")


def record_plan(eng):
    """everything Engine.plan() decides outside ConvStep.setup(), as plain JSON values (attributes a pass may not have set
    are read with the default their readers use)"""
    import conv_desc_ref as cr
    from vlfb import hip
    from vlfb.engine import AttentionStep, DropoutStep, PoolStep
    flag = lambda o, k: bool(getattr(o, k, False))
    exists = lambda o, k: getattr(o, k, None) is not None
    tensor = lambda t: None if t is None else [list(t.shape), str(t.dtype)]
    names = lambda bs: [b.name for b in bs]
    roots = []
    for b in eng.all_blobs:
        if b.root is not b:
            continue
        s = b.slot
        roots.append([b.name, b.kind, list(b.shape), b.caxis, flag(b, "relu"), flag(b, "needs_grad"), flag(b, "dead"),
                      flag(b, "is_input"), int(getattr(b, "pad_c", 0) or 0), int(getattr(b, "pad_w", 0) or 0), flag(b, "pair"),
                      flag(b, "grad_f32"), float(b.grad_scale), flag(b, "need_half"), flag(b, "grad_half"),
                      flag(b, "grad_half_src"), exists(b, "half"), exists(b, "planes"), tensor(b.tensor),
                      s.expected, flag(s, "two_term"), None if s.buf is None else str(s.buf.dtype), exists(s, "buf_lo"),
                      exists(s, "half_buf"), exists(s, "planes")])
    layout = lambda d: [[n, off, cnt, list(shape)] for n, (off, cnt, shape) in d.items()]
    r = {"steps": [[st.name(), type(st).__name__, names(st.inputs), names(st.outputs)] for st in eng.steps], "roots": roots,
         "head_f32": list(eng.head_f32), "head_f32_fbo": list(eng.head_f32_fbo), "pair_blobs": list(eng.pair_blobs),
         "train_order": list(eng.train_order), "train_layout": layout(eng.train_layout), "frozen_layout": layout(eng.frozen_layout),
         "wd_ranges": [list(w) for w in eng.wd_ranges], "shared_params": sorted(getattr(eng, "shared_params", ())),
         "buckets": [[b["start"], b["end"], b["ready"], [list(w) for w in b["wd"]], list(b["names"]),
                      [st.name() for st in b["bias_steps"]]] for b in getattr(eng, "sol_buckets", [])],
         "fwd_early": list(eng._fwd_early), "fwd_side": sorted(eng._fwd_side), "fwd_wait": [list(w) for w in eng._fwd_wait],
         "fwd_signal": sorted(eng._fwd_signal),
         "half_post": [[st.name(), names(st._half_post)] for st in eng.steps if st._half_post],
         "half_inputs": names(eng._half_inputs),
         "dropout": [[st.name(), st.seed_slot] for st in eng.steps if isinstance(st, DropoutStep)],
         "pools": [[st.name(), flag(st, "two_term_dx")] + [[getattr(d, f) for f, _ in hip.PoolDesc._fields_] for d in (st.desc, st.desc_b)]
                   for st in eng.steps if isinstance(st, PoolStep)],
         "attention": []}
    for st in eng.steps:
        if isinstance(st, AttentionStep):
            a = {"name": st.name(), "dot": bool(st.dot), "ds_scale": float(getattr(st, "ds_scale", 1.0)),
                 "kv_owner": getattr(st.kv_owner, "name", None),
                 "descs": {k: cr.desc_dict(v) for k, v in sorted(vars(st).items()) if isinstance(v, hip.ConvDesc)}}
            for k in ATTENTION_FLAGS:
                a[k] = flag(st, k)
            r["attention"].append(a)
    return r


def evaluate(keys, record=record):
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


def evaluate_in_child(keys, switch, tmp_dir, what="steps"):
    """evaluate() in a fresh process with the switch `NAME=VALUE` set; what: "steps" (record) or "plans" (record_plan)"""
    path = os.path.join(str(tmp_dir), "conv_step_keys_%s.json" % switch.replace("=", "_").replace(",", "_"))
    with open(path, "w") as f:
        json.dump(list(keys), f)
    name, value = switch.split("=")
    env = dict(os.environ)
    env[name] = value
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path, what], env=env, stdout=subprocess.PIPE, check=True)
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


def load_plans():
    """{section: {engine key: record}} of the plan snapshot, every part back in place"""
    with gzip.open(PLANS_GOLDEN, "rt") as f:
        g = json.load(f)
    descs = [dict(zip(g["fields"], row)) for row in g["descs"]]
    rows, lists = g["rows"], g["lists"]

    def expand(e):
        if "error" in e:
            return e
        out = {k: lists[i] for k, i in e.items()}
        for k in ("steps", "roots", "pools"):
            out[k] = [rows[i] for i in out[k]]
        out["attention"] = [dict(rows[i], descs={k: descs[j] for k, j in rows[i]["descs"].items()}) for i in out["attention"]]
        return out
    return g, {name: {key: expand(e) for key, e in sec.items()} for name, sec in g["sections"].items()}


def plan_differences(want, got):
    out = []
    for key in want:
        w, g = want[key], got.get(key)
        if g is None:
            out.append("%s: not evaluated" % key)
        elif "error" in w or "error" in g:
            if w != g:
                out.append("%s: recorded %r, got %r" % (key, w.get("error", "an engine"), g.get("error", "an engine")))
        else:
            for part in sorted(set(w) | set(g)):
                a, b = w.get(part), g.get(part)
                if a != b:
                    first = next(((x, y) for x, y in zip(a, b) if x != y), (len(a), len(b))) if a is not None and b is not None else (a, b)
                    out.append("%s: %s differs, first at (recorded, got) %r" % (key, part, first))
    return out


def test_plan_reproduces_the_snapshot():
    g, sections = load_plans()
    want = sections[""]
    assert sorted(want) == sorted(plan_keys())
    bad = plan_differences(want, evaluate(sorted(want), record_plan))
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:30]))


@pytest.mark.parametrize("switch", PLAN_SWITCHES)
def test_plan_under_a_switch_reproduces_the_snapshot(switch, tmp_path):
    g, sections = load_plans()
    want = sections[switch]
    assert sorted(want) == sorted(switch_keys())
    bad = plan_differences(want, evaluate_in_child(sorted(want), switch, tmp_path, "plans"))
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:30]))


def test_plan_snapshot_covers_every_planning_decision():
    """what the plan snapshot is for: every branch of AttentionStep.setup has a record, every recorded list is non-empty in
    at least one engine, and each kind of blob the passes single out is there"""
    g, sections = load_plans()
    assert sorted(sections) == sorted(("",) + PLAN_SWITCHES)
    engines = [e for sec in sections.values() for e in sec.values() if "error" not in e]
    att = [a for e in engines for a in e["attention"]]
    full = [a for a in att if not a["single"]]
    assert any(a["single"] and a["kv_owner"] is None for a in att) and any(a["single"] and a["kv_owner"] for a in att)
    assert all(not a["descs"] for a in att if a["single"])
    assert all(sorted(a["descs"]) == ["d_dp", "d_dth", "d_s", "d_tn", "d_tn_phi", "d_y"] for a in full)
    for flag in ("s_pair", "o_pair", "precise", "dot", "bsplit", "fused_fwd", "fused_bwd", "dy_f32"):
        assert any(a[flag] for a in full), flag
    assert any(not a["precise"] for a in full) and any(a["precise"] and a["dot"] for a in full)
    assert any(a["dot"] and not a["precise"] and a["bsplit"] for a in full)
    assert any(a["dot"] and not a["precise"] and not a["bsplit"] for a in full)
    assert any(a["ds_scale"] != 1.0 for a in full)
    for part in ENGINE_LISTS + ("steps", "roots", "buckets", "dropout", "pools", "attention"):
        assert any(e[part] for e in engines), part
    assert any(b[5] for e in engines for b in e["buckets"]), "bias steps of a bucket"
    assert any(p[1] for e in engines for p in e["pools"]), "PoolStep.two_term_dx"
    assert any(st[1] == "BNStep" for e in engines for st in e["steps"])
    roots = [dict(zip(ROOT_FIELDS, b)) for e in engines for b in e["roots"]]
    for field in ("relu", "needs_grad", "dead", "is_input", "pair", "grad_f32", "need_half", "grad_half", "grad_half_src", "half",
                  "planes", "two_term", "buf_lo", "half_buf", "slot_planes"):
        assert any(b[field] is True for b in roots), field
    assert any(b["pad_c"] and b["pad_w"] for b in roots) and any(b["grad_scale"] != 1.0 for b in roots)
    assert {b["buf"] for b in roots} >= {None, "torch.float16", "torch.bfloat16", "torch.float32"}


def WCODES(hip):
    # every wcode the engines of the snapshot's matrix give a conv (derived on the commit the snapshot was taken on)
    return (hip.F16, hip.BF16, hip.F32, hip.SPLIT, hip.MIX, hip.MIX_W2, hip.MIX_W2I, hip.MIXH, hip.MIXH_W2, hip.MIXH_W2I)


if __name__ == "__main__":
    for p in (os.path.join(ROOT, "video-long-term-feature-banks_amd", "lib"), ROOT, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    with open(sys.argv[1]) as f:
        print(json.dumps(evaluate(json.load(f), record_plan if sys.argv[2:] == ["plans"] else record)))
