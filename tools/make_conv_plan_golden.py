"""Writes tests/golden/conv_plans.json.gz, the snapshot tests/test_conv_plan_golden.py replays: what the conv planner answers
(return code, plan string or error text, workspace bytes) for every descriptor the dry-run engines of the benchmarked presets
store -- four presets x five dtypes x {2 clips of 16 x 64^2, 8 clips of 32 x 224^2} x {train, test} -- for the shrunk form of
each (conv_desc_ref.shrink), for each of those with `algo` forced to every VLFB_ALGO_* value, for the WGRADs with
`wgrad_bias` toggled and for the split-bf16 launches in the pre-split operand forms the engine switches to at run time; plus one section per planner A/B switch (the benchmark-size ava_r50_lfb_nl engines on mix and split),
evaluated in a child process with that variable set.  Needs the built library, no GPU.

    python tools/make_conv_plan_golden.py [--commit ID]

Regenerate only when a plan is MEANT to change; a refactor of the planner must pass against the file as it is."""
import argparse
import collections
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
import test_conv_plan_golden as snap            # noqa: E402
from test_conv_launch_shrink import stored_descs  # noqa: E402
from test_conv_launches_gpu import BASELINE_PRESETS  # noqa: E402

DTYPES = ("mix", "fp16", "bf16", "split", "fp32")
SIZES = ((2, 16, 64), (8, 32, 224))
ALGOS = range(6)
MAX_BYTES = 770 * 1000


def dry_engine(preset, dtype, clips, frames, crop, split, overrides=(), share_params_with=None, bank_per_clip=False):
    """a dry-run engine as tests/test_lowering.plan builds it, at `clips` clips of frames x crop^2; share_params_with: the
    engine whose parameters it aliases; bank_per_clip: the `lfb` blob with one row per clip (the inference plan of a RoI head)"""
    from vlfb.presets import load_preset
    from core.config import config as cfg
    from models.model_builder_video import ModelBuilder
    from vlfb.engine import Engine
    from vlfb import synth
    ov = ["NUM_GPUS", 1]
    for s in ("TRAIN", "TEST"):
        ov += [s + ".BATCH_SIZE", clips, s + ".VIDEO_LENGTH", frames, s + ".CROP_SIZE", crop]
    load_preset(preset, ov + list(overrides))
    m = ModelBuilder(train=(split == "train"), split=split, name=split)
    m.build_model(suffix="_" + split)
    rois = 5 if clips == 2 else sum(synth.rois_per_clip_draw(clips, seed=cfg.RNG_SEED))
    sfx = "_" + split
    sh = collections.OrderedDict()
    sh["data" + sfx] = (clips, 3, frames, crop, crop)
    if cfg.DATASET == "ava":
        sh["labels" + sfx] = (rois, cfg.MODEL.NUM_CLASSES)
        sh["proposals" + sfx] = (rois, 5)
        if "lfb" + sfx in m.input_blob_names:
            sh["lfb" + sfx] = (clips if bank_per_clip else rois, cfg.LFB.WINDOW_SIZE * cfg.AVA.LFB_MAX_NUM_FEAT_PER_STEP, 2048)
    else:
        sh["labels" + sfx] = (clips, cfg.MODEL.NUM_CLASSES) if cfg.MODEL.MULTI_LABEL else (clips,)
        if "lfb" + sfx in m.input_blob_names:
            sh["lfb" + sfx] = (clips, cfg.LFB.WINDOW_SIZE, 2048)
    eng = Engine(m, dtype, dry_run=True, share_params_with=share_params_with)
    eng.plan(sh)
    return eng


def plane_forms(b):
    """the pre-split operand forms of a split-bf16 descriptor, which the engine builds lazily at run time (ConvStep._pl_desc):
    the activation (WGRAD: and the gradient) operand as bf16 term planes, the term-plane / fp16 copies of an NT output"""
    if b["math"] not in (cr.MATH_BF16X3, cr.MATH_BF16X6) or b["dtype"] != cr.F32:
        return []
    g = cr.Geometry(b)
    up8 = lambda n: -(-n // 8) * 8
    a_ps = up8((g.batch - 1) * b["a_bstride"] + g.S * g.lda)
    if b["mode"] == cr.WGRAD:
        p_ps = up8((g.batch - 1) * b["p_bstride"] + g.M * g.ldp)
        return [dict(b, a_planes=n, a_pstride=a_ps, p_planes=2, p_pstride=p_ps, wgrad_bias=0) for n in (2, 3)]
    o_ps = up8((g.batch - 1) * b["o_bstride"] + g.orows * g.ldo)
    npl = 3 if b["math"] == cr.MATH_BF16X6 else 2
    return [dict(b, a_planes=npl, a_pstride=a_ps), dict(b, a_planes=npl, a_pstride=a_ps, o_planes=2, o_pstride=o_ps),
            dict(b, o_planes=1), dict(b, o_planes=2, o_pstride=o_ps)]


def variants(dd, pf):
    """the descriptor, its shrunk form, and each of the two with every algo, with (WGRAD) wgrad_bias toggled and in its
    pre-split operand forms"""
    base = [dd]
    try:
        e = cr.shrink(dd, pf, 0.0)
        if e != dd:
            base.append(e)
    except Exception:
        pass                                    # (a descriptor without a plan has nothing to shrink to)
    out = []
    for b in base:
        for algo in ALGOS:
            out.append(dict(b, algo=algo))
        if b["mode"] == cr.WGRAD:
            out.append(dict(b, wgrad_bias=0 if b["wgrad_bias"] else 1))
        out += plane_forms(b)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="commit the snapshot is taken on (default: git rev-parse HEAD)")
    args = ap.parse_args()
    commit = args.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"]).decode().strip()
    from vlfb import hip
    pf = lambda e: hip.conv_plan(hip.conv_desc(**e))
    key = lambda d: tuple(d[f] for f in cr.FIELDS)
    done, everything, switched = {}, {}, {}
    for preset in BASELINE_PRESETS:
        for dtype in DTYPES:
            for clips, frames, crop in SIZES:
                for split in ("train", "test"):
                    eng = dry_engine(preset, dtype, clips, frames, crop, split)
                    n = 0
                    for _, d in stored_descs(eng):
                        dd = cr.desc_dict(d)
                        k = key(dd)
                        if k not in done:
                            done[k] = [key(v) for v in variants(dd, pf)]
                        for v in done[k]:
                            everything[v] = 1
                            if preset == "ava_r50_lfb_nl" and clips == 8 and dtype in ("mix", "split"):
                                switched[v] = 1
                        n += 1
                    print("%-24s %-5s %d clips %-5s: %4d descriptors, %6d records so far" % (preset, dtype, clips, split, n, len(everything)),
                          flush=True)
    fields = list(cr.FIELDS)
    sections = {"": sorted(everything)}
    results = {"": snap.evaluate(fields, sections[""])}
    with tempfile.TemporaryDirectory() as tmp:
        for sw in snap.SWITCHES:
            sections[sw] = sorted(switched)
            results[sw] = snap.evaluate_in_child(fields, [list(r) for r in sections[sw]], sw, tmp)
    # fields that never vary leave the rows
    vary = [i for i, f in enumerate(fields) if len({r[i] for rows in sections.values() for r in rows}) > 1]
    const = {f: sections[""][0][i] for i, f in enumerate(fields) if i not in vary}
    texts = sorted({t for res in results.values() for _, t, _ in res})
    tix = {t: i for i, t in enumerate(texts)}
    out = {"commit": commit, "fields": [fields[i] for i in vary], "const": const, "texts": texts,
           "sections": {name: [[rows[j][i] for i in vary] + [res[0], tix[res[1]], res[2]] for j, res in enumerate(results[name])]
                        for name, rows in sections.items()}}
    path = snap.GOLDEN
    with gzip.GzipFile(path, "wb", compresslevel=9, mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    size = os.path.getsize(path)
    print("%s: commit %s, %d records (%s), %d bytes" % (os.path.relpath(path, ROOT), commit, sum(len(r) for r in sections.values()),
                                                         ", ".join("%s %d" % (k or "default", len(v)) for k, v in sections.items()), size))
    assert size < MAX_BYTES, "snapshot of %d bytes: drop fields or variants" % size


if __name__ == "__main__":
    main()
