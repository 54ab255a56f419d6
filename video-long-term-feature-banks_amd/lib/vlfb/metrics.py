"""Evaluation metrics accumulated on the device (csrc/vlfb_metrics.hip).

The reference's meter (lib/utils/metrics.py) fetches `pred` and `labels` from every GPU every iteration.  A step of
this engine is a replayed call list or a captured graph that never synchronises, so the meter is a set of kernels with
constant arguments that sit inside the step and add into device state; `read()` is the one call that synchronises.

  kind "topk"  single-label heads (EPIC verbs / nouns): hits for every k of `ks` and the number of rows counted; with
               keep_rows=N also the first N prediction rows and their labels (vlfb_topk_hits_keep: what the reference's
               finalize_metrics writes as epic_predictions_<name>.pkl), `kept()`
  kind "map"   multi-label heads (Charades): a score table [n_items][cols] into which every prediction row is merged by
               max at (stream position % n_items) -- clip c of video i arrives at position i + c * n_items, which is
               aggregate_predictions_from_clips (metrics.py:165-186) done while the clips arrive -- and from which
               `read()` computes mAP / wAP / ROC-AUC (mean_ap_metric, :444-482)
  kind "ava"   the RoI head of AVA: the same table in append mode (n_items >= every row the test issues, padding rows of
               ragged batches included); `finalize()` builds the image index from the host-side metadata, and
               vlfb_ava_match_tp + vlfb_class_ap_voc turn table, boxes and ground truth into the frame-mAP (ava_frame_ap)

N ranks (one process per GPU): a rank's meter holds the rows that rank issued, in append mode; at finalisation the tables
are gathered and vlfb_rows_interleave rebuilds the stream of the single-process walk (interleave_rows), which the
single-process kernels then score (merge_map_ranks, merge_ava_ranks, merge_keep_ranks).

Tie rule of top-k: rank = #{j : s_j > s_label} + #{j < label : s_j == s_label}, hit iff rank < k (include/vlfb.h).
"""
import numpy as np
import torch

from vlfb import hip


def _align(n, a=256):
    return (n + a - 1) // a * a


def summarize_ap(ap, auc, n_pos):
    """mean_ap_metric's reductions (metrics.py:453-480) from per-class AP / AUC / positives: classes without a positive
    are dropped from the means and get 0 in all_aps; mean_wap weights by positives; mean_auc is the plain mean over the
    kept classes, NaN as soon as one of them is all-positive (what current scikit-learn returns there, with a warning;
    older releases raised ValueError, which the reference turns into 0 -- DESIGN.md).  -> (auc, ap, wap, all_aps)"""
    ap = np.asarray(ap, np.float64)
    auc = np.asarray(auc, np.float64)
    n_pos = np.asarray(n_pos, np.int64)
    keep = n_pos > 0
    all_aps = np.zeros(ap.shape[0], np.float64)
    if not keep.any():
        return 0.0, 0.0, 0.0, all_aps          # (the reference: aps = [0], mean_auc = 0)
    aps = ap[keep]
    weights = n_pos[keep].astype(np.float64)
    weights /= np.sum(weights)
    all_aps[keep] = aps
    return float(np.mean(auc[keep])), float(np.mean(aps)), float(np.sum(np.multiply(aps, weights))), all_aps


class DeviceMeter(object):
    """One device buffer: hit counters, cursor, mismatch counter, score table, label table, per-class outputs, sort
    workspace.  `update` issues kernels on the current stream and returns nothing; `read` synchronises."""

    def __init__(self, kind, cols, ks=(1, 5), n_items=None, total_rows=0, device=None, keep_rows=None, keep_labels=False):
        """keep_labels: an "ava" table whose label rows matter (a rank's share of a Charades pass, merged later by
        merge_map_ranks): Engine.attach_meter then feeds it the net's label blob, not the zeros of an AVA test."""
        assert kind in ("topk", "map", "ava"), kind
        assert not keep_labels or kind == "ava", "keep_labels belongs to an 'ava' (append-mode) meter"
        self.keep_labels = bool(keep_labels)
        assert keep_rows is None or kind == "topk", "keep_rows belongs to a 'topk' meter (the other kinds keep their table)"
        self.keep_rows = int(keep_rows) if keep_rows is not None else 0
        if keep_rows is not None and self.keep_rows < 1:
            raise hip.VlfbError("DeviceMeter: keep_rows = %r must be at least 1" % (keep_rows,))
        self.kind, self.cols = kind, int(cols)
        self.ks = tuple(int(k) for k in ks)
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self.n_items = int(n_items) if n_items is not None else 0
        self.total_rows = int(total_rows)
        if kind == "topk":
            if not (1 <= len(self.ks) <= 4 and all(1 <= k <= self.cols for k in self.ks)):
                raise hip.VlfbError("DeviceMeter: ks = %r needs 1..4 values within 1..cols = %d" % (self.ks, self.cols))
        elif self.n_items < 1:
            raise hip.VlfbError("DeviceMeter: a %r meter needs n_items >= 1 (videos, or rows when nothing is merged)" % kind)
        self._ks = hip.ks_array(self.ks)
        # layout (bytes): hits int64[5] | cursor int64 | mismatches int32 (+pad) | ap f64[cols] | auc f64[cols] |
        #                 n_pos int32[cols] | table f32[n][cols] | labels u8[n][cols] | sort workspace
        #                 ("topk" with keep_rows = N: table f32[N][cols] | labels int32[N])
        n, c = self.n_items, self.cols
        off = {"hits": 0, "cursor": 40, "mismatch": 48}
        at = 64
        sizes = [("ap", 8 * c), ("auc", 8 * c), ("n_pos", 4 * c)] if kind == "map" else []
        if kind == "map":
            self.ws_bytes = hip.query_workspace(hip.WS_CLASS_AP, (n, c)) if n > hip.CLASS_AP_LDS_MAX else 0
            sizes += [("table", 4 * n * c), ("labels", n * c), ("ws", self.ws_bytes)]
        elif kind == "ava":                          # (tp, ap, n_gt and the sort workspace belong to one ava_frame_ap call)
            sizes += [("table", 4 * n * c), ("labels", n * c)]
        elif self.keep_rows:
            sizes += [("table", 4 * self.keep_rows * c), ("labels", 4 * self.keep_rows)]
        for name, nbytes in sizes:
            off[name] = at
            at = _align(at + nbytes)
        self.buf = torch.zeros(at, dtype=torch.uint8, device=self.device)
        view = lambda name, nbytes, dtype: self.buf[off[name]:off[name] + nbytes].view(dtype)
        self.hits = view("hits", 40, torch.int64)
        self.cursor = view("cursor", 8, torch.int64)
        self.mismatch = view("mismatch", 4, torch.int32)
        self.head = self.buf[:64].view(torch.int64)          # hits, cursor, mismatches: what one read() copies first
        if kind == "map":
            self.ap, self.auc = view("ap", 8 * c, torch.float64), view("auc", 8 * c, torch.float64)
            self.n_pos = view("n_pos", 4 * c, torch.int32)
            self.table = view("table", 4 * n * c, torch.float32).view(n, c)
            self.labels = view("labels", n * c, torch.uint8).view(n, c)
            self.ws = self.buf[off["ws"]:off["ws"] + self.ws_bytes] if self.ws_bytes else None
        elif kind == "ava":
            self.table = view("table", 4 * n * c, torch.float32).view(n, c)
            self.labels = view("labels", n * c, torch.uint8).view(n, c)
        elif self.keep_rows:
            self.table = view("table", 4 * self.keep_rows * c, torch.float32).view(self.keep_rows, c)
            self.labels = view("labels", 4 * self.keep_rows, torch.int32)
        self.reset()

    def reset(self):
        """asynchronous: fills on the current stream"""
        self.head.zero_()
        if self.kind in ("map", "ava"):
            self.table.fill_(float("-inf"))
            self.labels.fill_(255)

    def update_ptr(self, scores_ptr, dtype, labels_ptr, rows):
        """scores [rows][cols] of `dtype` and int32 labels ([rows] class indices / [rows][cols] multi-hot) by address"""
        if self.kind == "topk" and self.keep_rows:
            hip.call("vlfb_topk_hits_keep", scores_ptr, dtype, labels_ptr, rows, self.cols, self._ks[0], self._ks[1],
                     hip.ptr(self.hits), hip.ptr(self.table), hip.ptr(self.labels), self.keep_rows, hip.ptr(self.cursor))
        elif self.kind == "topk":
            hip.call("vlfb_topk_hits", scores_ptr, dtype, labels_ptr, rows, self.cols, self._ks[0], self._ks[1],
                     hip.ptr(self.hits))
        else:
            hip.call("vlfb_scores_merge_max", scores_ptr, dtype, labels_ptr, rows, self.cols, hip.ptr(self.table),
                     hip.ptr(self.labels), self.n_items, self.total_rows, hip.ptr(self.cursor), hip.ptr(self.mismatch))

    def update(self, scores, labels):
        """device tensors: scores [rows][cols] (fp32 / fp16 / bf16), labels int32"""
        assert scores.is_contiguous() and labels.is_contiguous() and labels.dtype == torch.int32
        assert scores.dim() == 2 and scores.shape[1] == self.cols, (tuple(scores.shape), self.cols)
        assert labels.numel() == (scores.shape[0] if self.kind == "topk" else scores.numel())
        self.update_ptr(scores.data_ptr(), hip.dtype_code(scores.dtype), labels.data_ptr(), scores.shape[0])

    def counters(self):
        """(hits per k ..., rows, cursor, mismatches) as Python ints; one sync"""
        head = self.head.cpu().numpy()
        nk = len(self.ks) if self.kind == "topk" else 0
        return [int(v) for v in head[:nk]], int(head[nk]), int(head[5]), int(head[6] & 0xffffffff)

    def kept(self):
        """a "topk" meter with keep_rows: (table[:n], labels[:n]) device views of the rows kept so far, n = min(cursor,
        keep_rows); one sync"""
        if not self.keep_rows:
            raise hip.VlfbError("DeviceMeter.kept: this meter was built without keep_rows")
        n = min(self.counters()[2], self.keep_rows)
        return self.table[:n], self.labels[:n]

    def filled(self, cursor):
        n = min(cursor, self.total_rows) if self.total_rows > 0 else cursor
        return min(n, self.n_items)

    def class_scores(self, n, flags=0):
        """per-class (ap, auc, n_pos) of the first n table rows as numpy arrays; synchronises"""
        hip.call("vlfb_class_ap_auc", hip.ptr(self.table), hip.ptr(self.labels), n, self.cols, hip.ptr(self.ap),
                 hip.ptr(self.auc), hip.ptr(self.n_pos), hip.ptr(self.ws), self.ws_bytes, flags)
        return self.ap.cpu().numpy(), self.auc.cpu().numpy(), self.n_pos.cpu().numpy()

    def read(self, hits=None, rows=None):
        """the only call that synchronises.  `hits` / `rows`: counters to report instead of this meter's own (the sums
        over data-parallel ranks, utils.metrics.MetricsCalculator)"""
        own_hits, own_rows, cursor, mismatches = self.counters()
        if self.kind == "ava":
            raise hip.VlfbError("DeviceMeter.read: an 'ava' meter is scored by finalize(), which needs the host-side metadata")
        if self.kind == "topk":
            hits = own_hits if hits is None else hits
            rows = own_rows if rows is None else rows
            out = {"rows": rows, "hits": dict(zip(self.ks, hits))}
            for k, h in zip(self.ks, hits):
                out["top%d_err" % k] = (1.0 - float(h) / rows) * 100 if rows else float("nan")
            return out
        n = self.filled(cursor)
        if n < 1:
            raise hip.VlfbError("DeviceMeter.read: no prediction has been merged yet")
        ap, auc, n_pos = self.class_scores(n)
        mean_auc, mean_ap, mean_wap, all_aps = summarize_ap(ap, auc, n_pos)
        return {"mean_ap": mean_ap, "mean_wap": mean_wap, "mean_auc": mean_auc, "all_aps": all_aps, "rows": n,
                "rows_seen": cursor, "label_mismatches": mismatches}

    def finalize(self, det_rows, det_keys, det_boxes, groundtruth, excluded_keys=(), class_whitelist=None, flags=0):
        """kind "ava": the frame-mAP of the table rows `det_rows` (never a padding row) whose image keys and boxes
        (x1, y1, x2, y2) the host kept while the rows were issued; see ava_frame_ap.  Synchronises."""
        assert self.kind == "ava", self.kind
        _, _, cursor, _ = self.counters()
        if cursor > self.n_items:
            raise hip.VlfbError("DeviceMeter.finalize: %d rows were issued into a table of %d: early rows were overwritten"
                                % (cursor, self.n_items))
        det_rows = np.asarray(det_rows, np.int64).reshape(-1)
        if det_rows.size and (det_rows.min() < 0 or det_rows.max() >= cursor):
            raise hip.VlfbError("DeviceMeter.finalize: table row %d named, %d rows issued" % (int(det_rows.max()), cursor))
        if cursor < 1:
            raise hip.VlfbError("DeviceMeter.finalize: no prediction has been issued yet")
        r = ava_frame_ap(self.table[:cursor], det_rows, det_keys, det_boxes, groundtruth, excluded_keys, class_whitelist, flags)
        r["rows_seen"] = cursor
        return r


def ava_image_index(det_rows, det_keys, det_boxes, groundtruth, excluded_keys=()):
    """The image index of one evaluation, on the host (integer keys and annotation boxes, no model output): images = the
    ground-truth keys in their order, then the detection keys not among them, minus `excluded_keys`; detections with
    x2 < x1 or y2 < y1 are dropped (the evaluator's _remove_invalid_boxes).  groundtruth = read_csv's (boxes, labels[,
    scores]): boxes[key] = [[y1, x1, y2, x2], ...], one entry per (box, label) in file order.
    -> dict(keys, img_det_ptr, det_rows, det_boxes [n_det][4], img_gt_ptr, gt_box [n_gt][4] as (x1, y1, x2, y2), gt_class)"""
    det_rows = np.asarray(det_rows, np.int64).reshape(-1)
    det_boxes = np.asarray(det_boxes, np.float64).reshape(-1, 4)
    assert len(det_keys) == det_rows.shape[0] == det_boxes.shape[0], (len(det_keys), det_rows.shape, det_boxes.shape)
    excluded_keys = set(excluded_keys) if excluded_keys else set()
    gt_boxes, gt_labels = groundtruth[0], groundtruth[1]
    index, keys = {}, []
    for key in gt_boxes:
        if key not in excluded_keys and key not in index:
            index[key] = len(keys)
            keys.append(key)
    n_gt_img = len(keys)
    img = np.empty(det_rows.shape[0], np.int64)
    for i, key in enumerate(det_keys):
        if key in excluded_keys:
            img[i] = -1
            continue
        at = index.get(key)
        if at is None:
            at = index[key] = len(keys)
            keys.append(key)
        img[i] = at
    valid = (img >= 0) & (det_boxes[:, 2] >= det_boxes[:, 0]) & (det_boxes[:, 3] >= det_boxes[:, 1])
    sel = np.flatnonzero(valid)
    sel = sel[np.argsort(img[sel], kind="stable")]             # per image, in the order the rows were issued
    n_img = len(keys)
    img_det_ptr = np.zeros(n_img + 1, np.int64)
    np.cumsum(np.bincount(img[sel], minlength=n_img), out=img_det_ptr[1:])
    gb, gc = [], []
    img_gt_ptr = np.zeros(n_img + 1, np.int64)
    for i in range(n_gt_img):
        key = keys[i]
        assert len(gt_boxes[key]) == len(gt_labels[key]), key
        gb.extend(gt_boxes[key])
        gc.extend(gt_labels[key])
        img_gt_ptr[i + 1] = len(gc)
    img_gt_ptr[n_gt_img + 1:] = len(gc)
    gb = np.asarray(gb, np.float64).reshape(-1, 4)[:, [1, 0, 3, 2]]
    return {"keys": keys, "img_det_ptr": img_det_ptr.astype(np.int32), "det_rows": det_rows[sel].astype(np.int32),
            "det_boxes": det_boxes[sel], "img_gt_ptr": img_gt_ptr.astype(np.int32), "gt_box": np.ascontiguousarray(gb),
            "gt_class": np.asarray(gc, np.int32).reshape(-1)}


def ava_frame_ap(table, det_rows, det_keys, det_boxes, groundtruth, excluded_keys=(), class_whitelist=None, flags=0,
                 return_tp=False):
    """AVA frame-mAP (PASCAL VOC at IoU 0.5; include/vlfb.h, "AVA frame-mAP") of a device score table fp32 [n_rows][cols]:
    class id = column + 1, `det_rows` / `det_keys` / `det_boxes` name the table rows that are detections, their image
    keys and their boxes (x1, y1, x2, y2).  The index is built on the host (ava_image_index) and uploaded; the two kernels
    run on the current stream; ap and n_gt are read once.  class_whitelist: class ids that are scored (None = all).
    -> dict(mean_ap, ap [cols], n_gt [cols], class_mask, images, detections[, tp])"""
    assert table.dim() == 2 and table.dtype == torch.float32 and table.is_contiguous() and table.is_cuda
    n_rows, cols = int(table.shape[0]), int(table.shape[1])
    ix = ava_image_index(det_rows, det_keys, det_boxes, groundtruth, excluded_keys)
    for name, limit, what in (("img_det_ptr", hip.AVA_MAX_DET, "detections"), ("img_gt_ptr", hip.AVA_MAX_GT, "ground-truth rows")):
        per = np.diff(ix[name])
        if per.size and per.max() > limit:
            i = int(np.argmax(per))
            raise hip.VlfbError("ava_frame_ap: image %r has %d %s, more than the %d one workgroup holds"
                                % (ix["keys"][i], int(per[i]), what, limit))
    mask = np.zeros(cols, np.uint8)
    if class_whitelist is None:
        mask[:] = 1
    else:
        for cid in class_whitelist:
            if 1 <= int(cid) <= cols:
                mask[int(cid) - 1] = 1
    boxes = np.zeros((n_rows, 4), np.float64)
    boxes[ix["det_rows"]] = ix["det_boxes"]
    dev = table.device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if a.size else None
    d_box, d_dptr, d_rows, d_gptr = up(boxes), up(ix["img_det_ptr"]), up(ix["det_rows"]), up(ix["img_gt_ptr"])
    d_gbox, d_gcls, d_mask = up(ix["gt_box"]), up(ix["gt_class"]), up(mask)
    tp = torch.empty((n_rows, cols), dtype=torch.uint8, device=dev)
    n_gt = torch.empty(cols, dtype=torch.int32, device=dev)
    ap = torch.empty(cols, dtype=torch.float64, device=dev)
    n_img = len(ix["keys"])
    hip.call("vlfb_ava_match_tp", hip.ptr(table), hip.ptr(d_box), n_rows, cols, hip.ptr(d_dptr), hip.ptr(d_rows), hip.ptr(d_gptr),
             hip.ptr(d_gbox), hip.ptr(d_gcls), n_img, ix["img_det_ptr"].ctypes.data, ix["img_gt_ptr"].ctypes.data, hip.ptr(d_mask),
             hip.ptr(tp), hip.ptr(n_gt))
    ws_bytes = hip.query_workspace(hip.WS_CLASS_AP_VOC, (n_rows, cols)) \
        if (n_rows > hip.CLASS_AP_VOC_LDS_MAX or flags & hip.CLASS_AP_FORCE_GLOBAL) else 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
    hip.call("vlfb_class_ap_voc", hip.ptr(table), hip.ptr(tp), hip.ptr(n_gt), n_rows, cols, hip.ptr(ap), hip.ptr(ws), ws_bytes, flags)
    ap_h, n_gt_h = ap.cpu().numpy(), n_gt.cpu().numpy()
    keep = (mask == 1) & (n_gt_h > 0)
    out = {"mean_ap": float(np.mean(ap_h[keep])) if keep.any() else float("nan"), "ap": ap_h, "n_gt": n_gt_h,
           "class_mask": mask, "images": n_img, "detections": int(ix["det_rows"].shape[0])}
    if return_tp:
        out["tp"] = tp.cpu().numpy()
    return out


# ---- N ranks: every rank keeps the rows it issued; the global stream order is rebuilt at finalisation --------------------
# Slice s of the single-process walk (b rows) belongs to rank s % world, which keeps its slices in the order it issued them.

def global_row(rank, row, b, world):
    """the row of the global stream that row `row` of rank `rank`'s own table is (numbers or numpy arrays)"""
    return (row // b) * (b * world) + rank * b + row % b


def rank_row(g, b, world):
    """the inverse: global row g -> (rank, row of that rank's table); what vlfb_rows_interleave reads for row g"""
    return (g // b) % world, (g // (b * world)) * b + g % b


def rank_rows(total, b, world):
    """rows of each rank's table among the first `total` rows of the global stream"""
    full, rem = divmod(int(total), b * world)
    return [full * b + min(max(rem - r * b, 0), b) for r in range(world)]


def interleave_rows(parts, b, total=None):
    """the global stream rebuilt from the ranks' tables (vlfb_rows_interleave): `parts` contiguous device tensors in rank
    order, alike in dtype and row shape, rank r's holding the rows of its slices of `b` rows; total: rows to produce
    (default: all of them, which then must be what `rank_rows` of their sum says).  -> a new tensor [total, ...]"""
    world = len(parts)
    first = parts[0]
    assert all(p.is_cuda and p.is_contiguous() and p.dtype == first.dtype and p.shape[1:] == first.shape[1:] for p in parts)
    have = [int(p.shape[0]) for p in parts]
    if total is None:
        total = sum(have)
        if rank_rows(total, b, world) != have:
            raise hip.VlfbError("interleave_rows: tables of %r rows are not the shares of %d ranks in a stream of %d-row "
                                "slices" % (have, world, b))
    row_bytes = first.element_size()
    for d in first.shape[1:]:
        row_bytes *= int(d)
    out = torch.empty((int(total),) + tuple(first.shape[1:]), dtype=first.dtype, device=first.device)
    hip.rows_interleave([p.data_ptr() if p.shape[0] else 0 for p in parts], have, b, row_bytes, total, out.data_ptr())
    return out


def merge_map_ranks(tables, labels, b, n_items, total_rows):
    """Charades under N ranks: the ranks' append tables (fp32 [rows_r][cols]) and label rows (uint8, as an "ava" meter keeps
    them) -> the "map" meter of the whole split, fed the interleaved stream in ONE vlfb_scores_merge_max, so the clip
    merge, the cut at total_rows and the label-mismatch count are the single-process ones.  -> DeviceMeter (use read())"""
    stream = interleave_rows(tables, b)
    stream_labels = interleave_rows(labels, b).to(torch.int32)
    meter = DeviceMeter("map", stream.shape[1], n_items=n_items, total_rows=total_rows, device=stream.device)
    meter.update(stream, stream_labels)
    return meter


def merge_ava_ranks(tables, det, b):
    """AVA under N ranks: the ranks' append tables and det[r] = (det_rows numbered in rank r's table, det_keys, det_boxes)
    -> (the interleaved table, det_rows as global rows, det_keys, det_boxes), detections in global row order: the order
    the single process names them in, which ava_image_index keeps within an image."""
    world = len(tables)
    table = interleave_rows(tables, b)
    rows = np.concatenate([global_row(r, np.asarray(d[0], np.int64).reshape(-1), b, world) for r, d in enumerate(det)])
    keys = [k for d in det for k in d[1]]
    boxes = np.concatenate([np.asarray(d[2], np.float64).reshape(-1, 4) for d in det])
    order = np.argsort(rows, kind="stable")
    return table, rows[order], [keys[i] for i in order], boxes[order]


def merge_keep_ranks(tables, labels, b, keep_rows):
    """EPIC under N ranks: the ranks' kept prediction tables (fp32 [rows_r][cols]) and labels (int32 [rows_r]) -> the first
    keep_rows rows of the global stream, (table, labels)"""
    have = sum(int(t.shape[0]) for t in tables)
    if have < keep_rows:
        raise hip.VlfbError("merge_keep_ranks: %d of %d predictions were issued" % (have, keep_rows))
    full = rank_rows(have, b, len(tables))
    if full != [int(t.shape[0]) for t in tables]:
        raise hip.VlfbError("merge_keep_ranks: tables of %r rows are not the ranks' shares %r" % ([int(t.shape[0]) for t in tables], full))
    return interleave_rows(tables, b, keep_rows), interleave_rows(labels, b, keep_rows)


def action_topk_hits(verb, noun, verb_labels, noun_labels, ks=(1, 5), prior=None):
    """EPIC action accuracy from the stored verb / noun probabilities of two models (compute_top_k_actions,
    tools/evaluate_actions.py:77-98): fp32 device tensors [rows][V], [rows][Nn], optional prior [V][Nn], int32 labels.
    -> ({k: hits}, rows counted); synchronises"""
    rows, V = verb.shape
    Nn = noun.shape[1]
    assert noun.shape[0] == rows and verb.dtype == noun.dtype == torch.float32 and verb.is_contiguous() and noun.is_contiguous()
    assert verb_labels.dtype == noun_labels.dtype == torch.int32
    assert prior is None or (tuple(prior.shape) == (V, Nn) and prior.dtype == torch.float32 and prior.is_contiguous())
    karr, nk = hip.ks_array(ks)
    hits = torch.zeros(5, dtype=torch.int64, device=verb.device)
    hip.call("vlfb_action_topk_hits", hip.ptr(verb), hip.ptr(noun), hip.ptr(prior), hip.ptr(verb_labels), hip.ptr(noun_labels),
             rows, V, Nn, karr, nk, hip.ptr(hits))
    host = hits.cpu().numpy()
    return {int(k): int(host[i]) for i, k in enumerate(ks)}, int(host[nk])
