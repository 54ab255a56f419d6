"""The reference's lib/utils/ava_eval_helper.py -- import path, names and signatures -- with the evaluator on the device.

The file-format layer (image keys, the AVA csv, the exclusion list, the label map, the detection layout, the result file)
returns what the reference's functions return, value for value: tests/golden/ref_ava_eval.json.gz holds their outputs on
seeded synthetic files (tools/make_ref_ava_eval_golden.py).  The evaluator behind run_evaluation is NOT the reference's --
it ships none (it imports utils.ava_evaluation.*, which is absent) -- but the public PASCAL-VOC protocol at IoU 0.5,
computed by vlfb_ava_match_tp and vlfb_class_ap_voc (include/vlfb.h, "AVA frame-mAP").

Detections reach run_evaluation either as read_csv's / get_ava_eval_data's triple of dictionaries or as an
AvaDetections(scores, boxes, keys) of arrays; evaluate_ava scores its arrays directly, row for row.
"""
from __future__ import absolute_import, division, print_function, unicode_literals

import collections
import csv
import logging
import pprint
import time

import numpy as np

logger = logging.getLogger(__name__)

MAP_KEY = 'PascalBoxes_Precision/mAP@0.5IOU'
CATEGORY_KEY = 'PascalBoxes_PerformanceByCategory/AP@0.5IOU/'

# scores [n][classes] (class id = column + 1), boxes [n][4] as (x1, y1, x2, y2), keys: n image keys
AvaDetections = collections.namedtuple("AvaDetections", ["scores", "boxes", "keys"])


def make_image_key(video_id, timestamp):
    """'<video id>,<timestamp as four digits>'"""
    return "{},{:04d}".format(video_id, int(timestamp))


def read_csv(csv_file, class_whitelist=None, load_score=False):
    """An AVA csv (video, second, x1, y1, x2, y2, action id[, score]) -> (boxes, labels, scores): dictionaries from image
    key to lists with one entry per line, boxes as [y1, x1, y2, x2]; lines whose action id is outside a non-empty
    `class_whitelist` are skipped; the score is 1.0 unless `load_score`."""
    boxes, labels, scores = (collections.defaultdict(list) for _ in range(3))
    with open(csv_file, 'r') as f:
        for line in csv.reader(f):
            assert len(line) in (7, 8), "Wrong number of columns: %r" % (line,)
            label = int(line[6])
            if class_whitelist and label not in class_whitelist:
                continue
            key = make_image_key(line[0], line[1])
            x1, y1, x2, y2 = (float(v) for v in line[2:6])
            boxes[key].append([y1, x1, y2, x2])
            labels[key].append(label)
            scores[key].append(float(line[7]) if load_score else 1.0)
    return boxes, labels, scores


def read_exclusions(exclusions_file):
    """the image keys of a csv of (video, second) lines; an empty set without a file"""
    keys = set()
    if not exclusions_file:
        return keys
    with open(exclusions_file, 'r') as f:
        for line in csv.reader(f):
            assert len(line) == 2, "Expected only 2 columns, got: %r" % (line,)
            keys.add(make_image_key(line[0], line[1]))
    return keys


def read_labelmap(labelmap_file):
    """a .pbtxt label map -> ([{'id': .., 'name': ..}, ...] in file order, {ids})"""
    categories, ids = [], set()
    name = ""
    with open(labelmap_file, 'r') as f:
        for line in f:
            if line.startswith("  name:"):
                name = line.split('"')[1]
            elif line.startswith("  id:") or line.startswith("  label_id:"):
                cid = int(line.strip().split(" ")[-1])
                categories.append({"id": cid, "name": name})
                ids.add(cid)
    return categories, ids


def get_ava_eval_data(scores, boxes, metadata, class_whitelist, verbose=False, video_idx_to_name=None):
    """the arrays of a test run -> the evaluator's dictionaries: for row i, key = '<video name>,<second>' from
    metadata[i] = (video index, second), the box [batch index, x1, y1, x2, y2] stored as [y1, x1, y2, x2], and one
    (score, class id) entry per whitelisted class"""
    out_boxes, out_labels, out_scores = (collections.defaultdict(list) for _ in range(3))
    for i in range(scores.shape[0]):
        video = video_idx_to_name[int(np.round(metadata[i][0]))]
        key = video + ',' + '%04d' % int(np.round(metadata[i][1]))
        b = boxes[i].tolist()
        yxyx = [b[2], b[1], b[4], b[3]]
        for col, score in enumerate(scores[i].tolist()):
            if col + 1 in class_whitelist:
                out_scores[key].append(score)
                out_labels[key].append(col + 1)
                out_boxes[key].append(yxyx)
    return out_boxes, out_labels, out_scores


def write_results(detections, filename):
    """the official csv: key, x1, y1, x2, y2 with three decimals, class id, score with four"""
    start = time.time()
    boxes, labels, scores = detections
    with open(filename, 'w') as f:
        for key in boxes.keys():
            for box, label, score in zip(boxes[key], labels[key], scores[key]):
                f.write('%s,%.03f,%.03f,%.03f,%.03f,%d,%.04f\n' % (key, box[1], box[0], box[3], box[2], label, score))
    logger.info('AVA results wrote to %s' % filename)
    logger.info('\ttook %d seconds.' % (time.time() - start))


def _table_from_dicts(detections, n_classes):
    """read_csv's dictionaries -> AvaDetections: one table row per box of an image, filled class by class.  Every box must
    carry every scored class exactly once (what get_ava_eval_data and write_results produce): the protocol ranks ALL
    boxes of an image in every class, and a table has no way to say that a box was not scored in one."""
    boxes, labels, scores = detections
    rows_box, rows_key, cells = [], [], []
    for key in boxes:
        per_box, seen = collections.defaultdict(list), collections.Counter()
        for box, label, score in zip(boxes[key], labels[key], scores[key]):
            ident = (tuple(box), int(label))
            k = seen[ident]
            seen[ident] += 1
            mine = per_box[tuple(box)]
            if k == len(mine):
                mine.append(len(rows_box))
                rows_box.append([box[1], box[0], box[3], box[2]])
                rows_key.append(key)
            cells.append((mine[k], int(label) - 1, float(score)))
    table = np.full((max(len(rows_box), 1), n_classes), np.nan, np.float32)
    for r, c, s in cells:
        table[r, c] = s
    return AvaDetections(table, np.asarray(rows_box, np.float64).reshape(-1, 4), rows_key)


def run_evaluation(categories, groundtruth, detections, excluded_keys, verbose=True):
    """-> the evaluator's dictionary: 'PascalBoxes_Precision/mAP@0.5IOU' (the mean over the categories that have ground
    truth) and one 'PascalBoxes_PerformanceByCategory/AP@0.5IOU/<name>' per category.  groundtruth: read_csv's triple;
    detections: the same, or an AvaDetections of arrays (device tensor or numpy scores)."""
    import torch
    from vlfb import metrics as vm
    ids = [int(c["id"]) for c in categories]
    if not isinstance(detections, AvaDetections):
        n_classes = max(ids + [l for ls in detections[1].values() for l in ls] + [1])
        detections = _table_from_dicts(detections, n_classes)
    scores = detections.scores
    if not isinstance(scores, torch.Tensor):
        scores = torch.from_numpy(np.ascontiguousarray(np.asarray(scores, np.float32)))
    scores = scores.to(device="cuda", dtype=torch.float32).contiguous()
    n_det = len(detections.keys)
    if n_det:
        used = scores[:n_det][:, [i - 1 for i in ids if 1 <= i <= scores.shape[1]]]
        if bool(torch.isnan(used).any()):
            raise ValueError("run_evaluation: every detected box needs one score for every category (a box misses one)")
    for key in set(excluded_keys) & (set(groundtruth[0]) | set(detections.keys)):
        logging.info("Found excluded timestamp: %s. It will be ignored.", key)
    r = vm.ava_frame_ap(scores, np.arange(n_det), list(detections.keys), detections.boxes, groundtruth, excluded_keys, ids)
    metrics = {MAP_KEY: r["mean_ap"]}
    for c in categories:
        cid = int(c["id"])
        metrics[CATEGORY_KEY + c["name"]] = float(r["ap"][cid - 1]) if 1 <= cid <= len(r["ap"]) else float("nan")
    if verbose:
        pprint.pprint(metrics, indent=2)
    return metrics


def evaluate_ava(preds, original_boxes, metadata, excluded_keys, class_whitelist, categories, groundtruth=None,
                 video_idx_to_name=None, name='latest'):
    """the mAP of a test run's arrays: preds [n][classes], original_boxes [n][5] = (batch index, x1, y1, x2, y2),
    metadata [n][2] = (video index, second); writes detections_<name>.csv as the reference does"""
    eval_start = time.time()
    import torch
    host_preds = preds.detach().cpu().numpy() if isinstance(preds, torch.Tensor) else np.asarray(preds)
    original_boxes, metadata = np.asarray(original_boxes), np.asarray(metadata)
    detections = get_ava_eval_data(host_preds, original_boxes, metadata, class_whitelist, video_idx_to_name=video_idx_to_name)
    logger.info('Evaluating with %d unique GT frames.' % len(groundtruth[0]))
    logger.info('Evaluating with %d unique detection frames' % len(detections[0]))
    write_results(detections, 'detections_%s.csv' % name)
    keys = [video_idx_to_name[int(np.round(m[0]))] + ',' + '%04d' % int(np.round(m[1])) for m in metadata]
    wanted = [c for c in categories if c["id"] in class_whitelist]
    results = run_evaluation(wanted, groundtruth, AvaDetections(preds, original_boxes[:, 1:5].astype(np.float64), keys),
                             excluded_keys, verbose=False)
    logger.info('AVA eval done in %f seconds.' % (time.time() - eval_start))
    return results[MAP_KEY]


def evaluate_ava_from_files(labelmap, groundtruth, detections, exclusions):
    """the same from annotation / prediction files"""
    categories, class_whitelist = read_labelmap(labelmap)
    excluded_keys = read_exclusions(exclusions)
    groundtruth = read_csv(groundtruth, class_whitelist, load_score=False)
    detections = read_csv(detections, class_whitelist, load_score=True)
    return run_evaluation(categories, groundtruth, detections, excluded_keys)
