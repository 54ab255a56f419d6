"""The AVA frame-mAP protocol (PASCAL VOC at IoU 0.5), restated in fp64 numpy with plain Python loops.

TEST INFRASTRUCTURE ONLY: shares no code with the product.  The reference ships no evaluator (its
lib/utils/ava_eval_helper.py imports utils.ava_evaluation.*, which is absent), so this file is what vlfb_ava_match_tp and
vlfb_class_ap_voc are held to, together with the hand-worked cases of tests/test_ava_eval_host.py.

One image, one class c (class id = column + 1):
  1. G = the image's ground-truth rows of class c in stored order; D = ALL the image's detection rows, scored scores[row][c].
  2. D is ordered by score descending, ties by table row ascending.
  3. IoU in fp64: iw = min(x2a, x2b) - max(x1a, x1b); ih likewise; inter = max(iw, 0) * max(ih, 0);
     iou = inter / (area_a + area_b - inter); area = (x2 - x1) * (y2 - y1).
  4. G empty: every detection is a false positive.
  5. Otherwise, in that order: g* = the FIRST index of the maximum IoU over G; true positive iff iou(d, g*) >= 0.5 and g* is
     not taken yet (g* becomes taken); everything else is a false positive.  No second choice when g* is taken.
  6. Images without ground truth give only false positives; images without detections only add to n_gt.
AP of a class: the padded-list form of the public evaluator's compute_average_precision -- [0] + recall + [1],
[0] + precision + [0], the backward maximum loop, the sum over where(recall[1:] != recall[:-1]).
"""
import numpy as np

NOT_SCORED = 255


def iou(a, b):
    """boxes (x1, y1, x2, y2), fp64, in the operation order of the protocol"""
    a = [np.float64(v) for v in a]
    b = [np.float64(v) for v in b]
    iw = min(a[2], b[2]) - max(a[0], b[0])
    ih = min(a[3], b[3]) - max(a[1], b[1])
    inter = max(iw, np.float64(0)) * max(ih, np.float64(0))
    area_a = (a[2] - a[0]) * (a[3] - a[1])
    area_b = (b[2] - b[0]) * (b[3] - b[1])
    return inter / (area_a + area_b - inter)


def match_tp(scores, det_box, img_det_ptr, det_rows, img_gt_ptr, gt_box, gt_class, class_mask):
    """-> (tp uint8 [n_rows][C]: 255 where no verdict was given, n_gt int64 [C])"""
    scores = np.asarray(scores, np.float32)
    n_rows, C = scores.shape
    tp = np.full((n_rows, C), NOT_SCORED, np.uint8)
    n_gt = np.zeros(C, np.int64)
    for c in range(C):
        if not class_mask[c]:
            continue
        for img in range(len(img_det_ptr) - 1):
            rows = [int(r) for r in det_rows[img_det_ptr[img]:img_det_ptr[img + 1]]]
            G = [g for g in range(img_gt_ptr[img], img_gt_ptr[img + 1]) if int(gt_class[g]) == c + 1]
            n_gt[c] += len(G)
            order = sorted(rows, key=lambda r: (-float(scores[r, c]), r))
            taken = set()
            for r in order:
                if not G:
                    tp[r, c] = 0
                    continue
                best, best_v = 0, iou(det_box[r], gt_box[G[0]])
                for k in range(1, len(G)):
                    v = iou(det_box[r], gt_box[G[k]])
                    if v > best_v:                       # strict: the first index of the maximum
                        best, best_v = k, v
                if best_v >= 0.5 and best not in taken:
                    taken.add(best)
                    tp[r, c] = 1
                else:
                    tp[r, c] = 0
    return tp, n_gt


def average_precision(precision, recall):
    """compute_average_precision of the public evaluator, on lists"""
    recall = [0.0] + [float(r) for r in recall] + [1.0]
    precision = [0.0] + [float(p) for p in precision] + [0.0]
    for i in range(len(precision) - 2, -1, -1):
        precision[i] = max(precision[i], precision[i + 1])
    recall, precision = np.array(recall, np.float64), np.array(precision, np.float64)
    idx = np.where(recall[1:] != recall[:-1])[0] + 1
    return float(np.sum((recall[idx] - recall[idx - 1]) * precision[idx]))


def class_ap(scores, tp, n_gt):
    """per-class AP: NaN where n_gt == 0, 0.0 where there is ground truth and no detection"""
    scores = np.asarray(scores, np.float32)
    C = scores.shape[1]
    ap = np.full(C, np.nan, np.float64)
    for c in range(C):
        if n_gt[c] <= 0:
            continue
        rows = [r for r in range(scores.shape[0]) if tp[r, c] != NOT_SCORED]
        rows.sort(key=lambda r: (-float(scores[r, c]), r))
        if not rows:
            ap[c] = 0.0
            continue
        hit = np.array([int(tp[r, c]) for r in rows], np.int64)
        ctp = np.cumsum(hit).astype(np.float64)
        cfp = np.cumsum(1 - hit).astype(np.float64)
        ap[c] = average_precision(ctp / (ctp + cfp), ctp / np.float64(n_gt[c]))
    return ap


def mean_ap(ap, n_gt, class_mask):
    keep = [c for c in range(len(ap)) if class_mask[c] and n_gt[c] > 0]
    return float(np.mean([ap[c] for c in keep])) if keep else float("nan")


def evaluate(scores, det_box, img_det_ptr, det_rows, img_gt_ptr, gt_box, gt_class, class_mask):
    """-> (tp, n_gt, ap, mAP)"""
    tp, n_gt = match_tp(scores, det_box, img_det_ptr, det_rows, img_gt_ptr, gt_box, gt_class, class_mask)
    ap = class_ap(scores, tp, n_gt)
    return tp, n_gt, ap, mean_ap(ap, n_gt, class_mask)


def bound(n):
    """tests/test_metrics_host.py: fixed-order fp64 sums of at most n terms that total at most 1"""
    return (n + 8) * 2.0 ** -52
