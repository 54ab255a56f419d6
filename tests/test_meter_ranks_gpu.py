"""The meters of a pass shared by W ranks, in one process: W per-rank tables are fed the slices of one synthetic stream in
rank order (slice s to rank s % W), merged by the product's merge functions with explicit parts (vlfb.metrics.merge_map_ranks
/ merge_ava_ranks / merge_keep_ranks -- what MetricsCalculator.finalize_metrics calls with the gathered tables), and compared
with ONE single-process meter fed the whole stream.  Every comparison is in bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WORLDS = (2, 3)


def bits(t):
    t = t.contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.uint8).cpu().numpy()


def slices_of(rows, b):
    return [(lo, min(lo + b, rows)) for lo in range(0, rows, b)]


def rank_capacity(P, world, b):
    """rows of a rank's table: ceil(P / world) slices"""
    return -(-P // world) * b


# ---- Charades "map" ---------------------------------------------------------------------------------------------------
def charades_stream(items, clips, cols, b, seed, mismatch):
    """items x clips rows, clip c of item i at position i + c * items, padded to whole slices of b rows with the first row
    of the last slice (what get_minibatch_info does); one class holds few distinct scores, so AP ties are present"""
    rng = np.random.default_rng(seed)
    total = items * clips
    P = -(-total // b)
    scores = rng.uniform(0.01, 0.99, (P * b, cols)).astype(np.float32)
    scores[:, 1] = rng.integers(1, 4, P * b).astype(np.float32) / 4                    # ties within the class ...
    scores[:, 2] = 0.5                                                                  # ... and a class that is one tie
    item_labels = (rng.uniform(size=(items, cols)) < 0.4).astype(np.int32)
    item_labels[0, :3] = 1
    item_labels[1, :3] = 0
    labels = item_labels[np.arange(P * b) % items].copy()
    first = (P - 1) * b
    for r in range(total, P * b):
        scores[r], labels[r] = scores[first], labels[first]
    if mismatch:
        labels[items + 1, :2] ^= 1                                                      # clip 1 of item 1 disagrees twice
    return scores, labels, total, P


@pytest.mark.parametrize("items,mismatch", [(5, False), (7, False), (5, True)])
@pytest.mark.parametrize("cols", [5, 157])
@pytest.mark.parametrize("world", WORLDS)
def test_charades_map_of_rank_tables_equals_the_single_meter(world, cols, items, mismatch):
    """5 items x 3 clips in slices of 2 rows: P = 8, the last slice padded and cut by total_rows; 7 items x 3 clips: P = 11,
    odd, so the ranks' shares differ for both world sizes"""
    from vlfb.metrics import DeviceMeter, merge_map_ranks
    clips, b = 3, 2
    scores, labels, total, P = charades_stream(items, clips, cols, b, 10 * items + cols, mismatch)
    assert P == {5: 8, 7: 11}[items] and total < P * b
    d_scores, d_labels = torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda()
    single = DeviceMeter("map", cols, n_items=items, total_rows=total)
    ranks = [DeviceMeter("ava", cols, n_items=rank_capacity(P, world, b), keep_labels=True) for _ in range(world)]
    for s, (lo, hi) in enumerate(slices_of(P * b, b)):
        single.update(d_scores[lo:hi], d_labels[lo:hi])
        ranks[s % world].update(d_scores[lo:hi], d_labels[lo:hi])
    issued = [m.counters()[2] for m in ranks]
    assert sum(issued) == P * b and len(set(issued)) == (1 if P % world == 0 else 2)
    merged = merge_map_ranks([m.table[:n] for m, n in zip(ranks, issued)], [m.labels[:n] for m, n in zip(ranks, issued)],
                             b, items, total)
    want, got = single.read(), merged.read()
    assert np.array_equal(bits(merged.table), bits(single.table))
    assert np.array_equal(bits(merged.labels), bits(single.labels))
    for key in ("mean_ap", "mean_wap", "mean_auc"):
        assert np.float64(got[key]).tobytes() == np.float64(want[key]).tobytes(), key
    assert got["all_aps"].tobytes() == want["all_aps"].tobytes()
    assert got["rows"] == want["rows"] == items and got["rows_seen"] == want["rows_seen"] == P * b
    assert got["label_mismatches"] == want["label_mismatches"] == (2 if mismatch else 0)


# ---- AVA --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", WORLDS)
def test_ava_frame_ap_of_rank_tables_equals_the_single_table(world):
    """7 slices of 4 table rows with 3, 4, 1, 2, 4, 0, 3 real rows; the image of slices 0 and 1 -- different ranks for both
    world sizes -- gets one detection from each with the same score in class 1, on the same ground-truth box, so which of
    the two is the true positive is decided by the order of the rows alone"""
    from vlfb.metrics import DeviceMeter, ava_frame_ap, merge_ava_ranks
    b, cols, real = 4, 6, [3, 4, 1, 2, 4, 0, 3]
    P = len(real)
    rng = np.random.default_rng(world)
    scores = rng.uniform(0.05, 0.95, (P * b, cols)).astype(np.float32)
    key_of = lambda s: "vid%d,%04d" % (s // 2, 902 + (s // 2))                   # slices 2k and 2k + 1 share an image
    box_of = lambda s, j: [10.0 * j, 5.0, 10.0 * j + 8.0, 13.0]                  # (x1, y1, x2, y2): box j of every slice alike
    scores[0 * b + 0, 0] = scores[1 * b + 0, 0] = 0.75                             # the tie across ranks (same box 0)
    gt_boxes, gt_labels = {}, {}
    for k in range(4):
        key = key_of(2 * k)
        gt_boxes[key] = [[5.0, 10.0 * j, 13.0, 10.0 * j + 8.0] for j in range(3)]  # (y1, x1, y2, x2)
        gt_labels[key] = [1, 1 + (k + 1) % cols, 1 + (k + 2) % cols]
    groundtruth = (gt_boxes, gt_labels)
    zeros = torch.zeros((b, cols), dtype=torch.int32, device="cuda")
    d_scores = torch.from_numpy(scores).cuda()
    single = DeviceMeter("ava", cols, n_items=P * b)
    ranks = [DeviceMeter("ava", cols, n_items=rank_capacity(P, world, b)) for _ in range(world)]
    rows, keys, boxes = [], [], []
    det = [([], [], []) for _ in range(world)]
    for s in range(P):
        part = d_scores[s * b:(s + 1) * b]
        single.update(part, zeros)
        ranks[s % world].update(part, zeros)
        for j in range(real[s]):
            rows.append(s * b + j)
            keys.append(key_of(s))
            boxes.append(box_of(s, j))
            d = det[s % world]
            d[0].append((s // world) * b + j)
            d[1].append(key_of(s))
            d[2].append(box_of(s, j))
    want = ava_frame_ap(single.table[:single.counters()[2]], rows, keys, boxes, groundtruth, return_tp=True)
    issued = [m.counters()[2] for m in ranks]
    table, g_rows, g_keys, g_boxes = merge_ava_ranks([m.table[:n] for m, n in zip(ranks, issued)], det, b)
    assert np.array_equal(bits(table), bits(single.table[:P * b]))
    assert g_rows.tolist() == rows and g_keys == keys and np.array_equal(g_boxes, np.asarray(boxes))
    got = ava_frame_ap(table, g_rows, g_keys, g_boxes, groundtruth, return_tp=True)
    assert got["ap"].tobytes() == want["ap"].tobytes()
    assert np.array_equal(got["tp"], want["tp"]) and np.array_equal(got["n_gt"], want["n_gt"])
    assert np.float64(got["mean_ap"]).tobytes() == np.float64(want["mean_ap"]).tobytes()
    # the tie was real: the earlier row took the box, the later one is a false positive
    assert want["tp"][0, 0] == 1 and want["tp"][b, 0] == 0
    assert want["n_gt"].sum() == 12 and want["detections"] == sum(real)


# ---- EPIC "topk" with kept predictions --------------------------------------------------------------------------------
@pytest.mark.parametrize("world", WORLDS)
def test_kept_predictions_of_rank_tables_equal_the_single_table(world):
    """23 predictions in slices of 4 rows: P = 6, keep_rows ends inside the last slice"""
    from vlfb.metrics import DeviceMeter, merge_keep_ranks
    b, cols, keep = 4, 125, 23
    P = -(-keep // b)
    rng = np.random.default_rng(world + 40)
    scores = rng.standard_normal((P * b, cols)).astype(np.float32)
    scores[:, 3] = scores[:, 7]                                                      # ties inside a row
    labels = rng.integers(0, cols, P * b).astype(np.int32)
    d_scores, d_labels = torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda()
    single = DeviceMeter("topk", cols, keep_rows=keep)
    ranks = [DeviceMeter("topk", cols, keep_rows=rank_capacity(P, world, b)) for _ in range(world)]
    for s, (lo, hi) in enumerate(slices_of(P * b, b)):
        single.update(d_scores[lo:hi], d_labels[lo:hi])
        ranks[s % world].update(d_scores[lo:hi], d_labels[lo:hi])
    want_table, want_labels = single.kept()
    assert want_table.shape[0] == keep
    parts = [m.kept() for m in ranks]
    table, kept_labels = merge_keep_ranks([p[0] for p in parts], [p[1] for p in parts], b, keep)
    assert np.array_equal(bits(table), bits(want_table)) and np.array_equal(bits(kept_labels), bits(want_labels))
    assert np.array_equal(bits(table), scores[:keep].view(np.int32))
    hits = np.sum([m.counters()[0] for m in ranks], axis=0).tolist()
    counted = sum(m.counters()[1] for m in ranks)
    assert hits == single.counters()[0] and counted == single.counters()[1] == P * b
    from vlfb import hip
    with pytest.raises(hip.VlfbError, match="predictions were issued"):
        merge_keep_ranks([p[0] for p in parts], [p[1] for p in parts], b, P * b + 1)
