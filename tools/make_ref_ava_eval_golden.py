"""Run the REFERENCE's own AVA helper functions on seeded synthetic files and commit inputs + outputs.

TEST INFRASTRUCTURE ONLY.  Needs the reference checkout:

    python tools/make_ref_ava_eval_golden.py          # writes tests/golden/ref_ava_eval.json.gz

Called, from where they lie (the Caffe2 / OpenCV stubs of oracle/make_ref_aux_golden.py make the modules importable):
  lib/utils/ava_eval_helper.py   make_image_key, read_csv (with and without scores and whitelist), read_exclusions,
                                 read_labelmap, get_ava_eval_data, write_results
  lib/utils/metrics.py           get_ava_mini_groundtruth
The helper imports utils.ava_evaluation.{object_detection_evaluation, standard_fields}, which the reference does not ship:
an EMPTY stand-in is put into sys.modules here so the import succeeds.  Nothing of the evaluator is run -- there is none;
run_evaluation / evaluate_ava are therefore not called, and the matching and AP arithmetic are pinned elsewhere
(tests/ava_eval_ref.py).  The output holds data only: the text of the synthetic input files and what the functions returned.
"""
import gzip
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "ref_ava_eval.json.gz")
sys.path.insert(0, ROOT)


def plain(triple):
    """read_csv-style dictionaries -> [[key, value list], ...] in iteration order"""
    return [[[k, list(v)] for k, v in d.items()] for d in triple]


def main():
    from oracle.make_ref_aux_golden import install_stubs
    install_stubs()
    pkg = types.ModuleType("utils.ava_evaluation")
    pkg.object_detection_evaluation = types.ModuleType("utils.ava_evaluation.object_detection_evaluation")
    pkg.standard_fields = types.ModuleType("utils.ava_evaluation.standard_fields")
    sys.modules["utils.ava_evaluation"] = pkg
    sys.modules["utils.ava_evaluation.object_detection_evaluation"] = pkg.object_detection_evaluation
    sys.modules["utils.ava_evaluation.standard_fields"] = pkg.standard_fields
    import utils.ava_eval_helper as A            # the reference's (install_stubs put its lib/ on the path)
    import utils.metrics as M
    assert os.path.realpath(A.__file__).startswith(REF), A.__file__
    assert os.path.realpath(M.__file__).startswith(REF), M.__file__

    rng = np.random.RandomState(20240923)
    videos = ["-5KQ66BBWC4", "1j20qq1JyX4", "zG7mx8KiavA", "_a9SWtcaNj8"]
    out = {"generator": "tools/make_ref_ava_eval_golden.py", "evaluator_run": False}

    # ---- make_image_key ----------------------------------------------------------------------------------------------
    cases = [["abc", 902], ["abc", "0904"], ["x_y-z", 7], ["v", 12345], ["v", "17"]]
    out["image_keys"] = [[v, t, A.make_image_key(v, t)] for v, t in cases]

    # ---- a label map, with both spellings of the id line ----------------------------------------------------------------
    names = ["bend/bow (at the waist)", "crouch/kneel", "dance", "fall down", "get up", "jump/leap", "lie/sleep", "run/jog",
             "sit", "stand", "swim", "walk"]
    ids = [1, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14]
    lines = []
    for i, (cid, name) in enumerate(zip(ids, names)):
        lines += ["item {", '  name: "%s"' % name, ("  id: %d" if i % 3 else "  label_id: %d") % cid,
                  "  label_type: PERSON_MOVEMENT", "}"]
    labelmap_text = "\n".join(lines) + "\n"

    # ---- ground truth (7 columns) and detections (8 columns) ------------------------------------------------------------
    def box_fields():
        x1, y1 = rng.uniform(0, 0.6, 2)
        w, h = rng.uniform(0.05, 0.4, 2)
        return ["%.3f" % x1, "%.3f" % y1, "%.3f" % min(x1 + w, 1.0), "%.3f" % min(y1 + h, 1.0)]

    gt_lines, det_lines = [], []
    for v in videos:
        for sec in sorted(rng.choice(np.arange(902, 930), 6, replace=False)):
            for _ in range(rng.randint(1, 4)):
                b = box_fields()
                for cid in sorted(rng.choice(np.arange(1, 16), rng.randint(1, 4), replace=False)):
                    gt_lines.append(",".join([v, "%04d" % sec] + b + [str(cid)]))
                if rng.rand() < 0.7:
                    for cid in (1, 2, 3, 10, 14):
                        det_lines.append(",".join([v, "%04d" % sec] + b + [str(cid), "%.4f" % rng.rand()]))
    gt_text, det_text = "\n".join(gt_lines) + "\n", "\n".join(det_lines) + "\n"
    excl_text = "".join("%s,%04d\n" % (v, s) for v, s in ((videos[0], 905), (videos[2], 911), ("notthere", 1)))

    tmp = tempfile.mkdtemp()
    paths = {}
    for name, text in (("labelmap", labelmap_text), ("gt", gt_text), ("det", det_text), ("excl", excl_text)):
        paths[name] = os.path.join(tmp, name)
        with open(paths[name], "w") as f:
            f.write(text)
    out["files"] = {"labelmap": labelmap_text, "gt": gt_text, "det": det_text, "excl": excl_text}

    categories, whitelist = A.read_labelmap(paths["labelmap"])
    out["labelmap"] = {"categories": categories, "class_ids": sorted(whitelist)}
    out["exclusions"] = sorted(A.read_exclusions(paths["excl"]))
    out["exclusions_none"] = sorted(A.read_exclusions(None))
    out["read_csv"] = {
        "gt_plain": plain(A.read_csv(paths["gt"])),
        "gt_whitelist": plain(A.read_csv(paths["gt"], whitelist)),
        "gt_whitelist_flag": plain(A.read_csv(paths["gt"], whitelist, load_score=False)),
        "det_scores": plain(A.read_csv(paths["det"], None, load_score=True)),
        "det_scores_whitelist": plain(A.read_csv(paths["det"], whitelist, load_score=True)),
        "det_no_scores": plain(A.read_csv(paths["det"], whitelist)),
    }
    full = A.read_csv(paths["gt"], whitelist)
    out["mini_groundtruth"] = plain(M.get_ava_mini_groundtruth(full))

    # ---- get_ava_eval_data + write_results on arrays ---------------------------------------------------------------------
    n, C = 11, 16
    scores = rng.rand(n, C).astype(np.float32)
    boxes = np.concatenate([rng.randint(0, 2, (n, 1)).astype(np.float32), (rng.rand(n, 4) * 300).astype(np.float32)], axis=1)
    metadata = np.stack([rng.randint(0, len(videos), n), rng.randint(902, 930, n)], axis=1).astype(np.float32)
    metadata += rng.uniform(-0.2, 0.2, metadata.shape).astype(np.float32)          # (the reference rounds)
    idx_to_name = {i: v for i, v in enumerate(videos)}
    det = A.get_ava_eval_data(scores, boxes, metadata, whitelist, video_idx_to_name=idx_to_name)
    res = os.path.join(tmp, "results.csv")
    A.write_results(det, res)
    out["eval_data"] = {"scores": scores.tolist(), "boxes": boxes.tolist(), "metadata": metadata.tolist(), "videos": videos,
                        "detections": plain(det), "written": open(res).read()}
    A.write_results(A.read_csv(paths["det"], whitelist, load_score=True), res)
    out["written_from_csv"] = open(res).read()

    with open(OUT, "wb") as raw:
        with gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as f:
            f.write(json.dumps(out, sort_keys=True).encode())
    print("wrote %s: %d bytes, %d gt lines, %d detection lines" % (os.path.normpath(OUT), os.path.getsize(OUT), len(gt_lines),
                                                                   len(det_lines)))


if __name__ == "__main__":
    main()
