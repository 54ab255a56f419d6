"""AVA multi-crop testing over the device engine.

Reference: tools/test_net.py:48-93 runs the test net once per (flip in {False, True}) x (scale in
AVA.TEST_MULTI_CROP_SCALES) x (spatial shift in {0, 1, 2}) with TEST.SCALE = scale and
TEST.CROP_SIZE = min(256, scale), writes the `pred` logits of every box to a csv per pass, and
lib/utils/metrics.py:599-716 merges them: for one (scale, flip) the sigmoid scores of the shifts whose
crop overlaps the box are averaged (a box may fall outside the left / right crop), then the (scale, flip)
results are summed.

Two ways through it:

  * `AvaMultiCropTester.run` takes stacked host frames, preprocesses one clip per kernel call, fetches `pred` to the
    host after each of the 18 passes and merges in NumPy (`shift_validity`, `merge_shifts`, `merge_scales_and_flips`).
    It knows nothing of the data set: the checker of the pass below, and the way to score clips one has in memory.
  * `AvaMultiCropPass` walks the keyframes of a datasets.ava.AvaIndex out of a datasets.frame_store.FrameStore: the 18
    views of a keyframe are the same source frames, so a frame is decoded and uploaded once and read 18 times (the
    reference decodes it 18 times); `pred` never visits the host -- `vlfb_multicrop_merge` merges the three shifts of a
    (scale, flip) and accumulates in fp64 on the device, and the merged scores feed a vlfb.metrics.DeviceMeter("ava")
    whose `finalize` is the frame-mAP.  `run_ava_multi_crop` is the driver around it (tools/test_net.py:57-87).  The
    reference's per-pass csv files are not written; the merged scores can be (`write_merged_scores`).
"""
import collections
import ctypes as C
import logging
import os

import numpy as np

from core.config import config as cfg

logger = logging.getLogger(__name__)


def shift_validity(boxes_norm, flip, scale, height, width, max_crop=256):
    """(3, R) bool: which spatial shifts (0 = left/top, 1 = centre, 2 = right/bottom) see each box
    (metrics.py:652-676; the reference's geometry assumes landscape frames resized to height = scale).
    boxes_norm: (R, 4) [x1, y1, x2, y2] normalised to the ORIGINAL frame."""
    b = np.asarray(boxes_norm, dtype=np.float64).copy()
    w = float(width * scale) / height
    norm_crop = float(min(scale, max_crop)) / w
    center_left, center_right = 0.5 - norm_crop / 2.0, 0.5 + norm_crop / 2.0
    lcrop_right, rcrop_left = norm_crop, 1.0 - norm_crop
    if flip:
        b[:, 0], b[:, 2] = 1.0 - b[:, 2].copy(), 1.0 - b[:, 0].copy()
    return np.stack([b[:, 0] < lcrop_right, (b[:, 2] > center_left) & (b[:, 0] < center_right), b[:, 2] > rcrop_left])


def merge_shifts(logits, valid):
    """logits (3, R, C), valid (3, R) -> (R, C): mean over the valid shifts of sigmoid(logit) (metrics.py:677)"""
    s = 1.0 / (1.0 + np.exp(-np.asarray(logits, dtype=np.float64)))
    v = np.asarray(valid, dtype=np.float64)[:, :, None]
    n = v.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (s * v).sum(axis=0) / n          # a box no crop sees gives nan, like np.mean([]) in the reference


def merge_scales_and_flips(per_pass):
    """sum over the (scale, flip) results (metrics.py:689-711)"""
    return np.sum(np.stack(per_pass), axis=0)


class AvaMultiCropTester(object):
    """Owns one forward-only Engine per crop size; `run` does the 2 x len(scales) x 3 passes for one batch
    of clips and returns the merged (R, classes) scores."""

    def __init__(self, params, dtype="bf16", device="cuda:0", scales=None, max_crop=256):
        self.params, self.dtype, self.device = params, dtype, device
        self.scales = list(scales if scales is not None else cfg.AVA.TEST_MULTI_CROP_SCALES)
        self.max_crop = int(max_crop)
        self._engines = {}

    def _engine(self, crop, n_clips, frames, n_rois, lfb_shape):
        from models.model_builder_video import ModelBuilder
        from vlfb import passes
        from vlfb.engine import Engine
        key = (crop, n_clips, frames, n_rois, lfb_shape)
        if key not in self._engines:
            cfg.TEST.CROP_SIZE = crop
            model = ModelBuilder(train=False, split=cfg.TEST.DATA_TYPE, name="final_test_%d" % crop)
            model.build_model(suffix="_final_test")
            eng = Engine(model, self.dtype, device=self.device)
            eng.plan(passes.input_shapes(model, "_final_test", n_clips, frames, crop, n_rois, lfb_shape))
            eng.feed_params({k: v for k, v in self.params.items() if k in eng.param_views})
            self._engines[key] = (model, eng)
        return self._engines[key]

    def run(self, clips, boxes, lfb=None):
        """clips: list of (T, H, W, 3) uint8 BGR frame stacks (one per clip); boxes: list of (r_i, 4) arrays
        normalised to the original frames; lfb: (R, K, D) bank rows per RoI (models with LFB.ENABLED).
        Returns (scores (R, classes) float64, per_pass {(scale, flip, shift): logits (R, classes)})."""
        import torch
        from datasets import data_input_helper as dih
        n_clips = len(clips)
        T, H, W = clips[0].shape[:3]
        n_rois = int(sum(len(b) for b in boxes))
        all_boxes = np.concatenate([np.asarray(b, dtype=np.float64).reshape(-1, 4) for b in boxes])
        per_pass, merged = {}, []
        saved = (cfg.TEST.SCALE, cfg.TEST.CROP_SIZE, cfg.AVA.FORCE_TEST_FLIP)
        try:
            for scale in self.scales:                        # metrics.combine_ava_multi_crops order: scale, then flip
                crop = min(self.max_crop, scale)
                model, eng = self._engine(crop, n_clips, T, n_rois, None if lfb is None else tuple(lfb.shape))
                names = {n.split("_")[0]: n for n in model.input_blob_names}
                if lfb is not None and "lfb" in names:
                    eng.feed(names["lfb"], lfb)
                data, (wpad, cpad) = eng.blob_padded(names["data"])
                for flip in (False, True):
                    cfg.TEST.SCALE, cfg.TEST.CROP_SIZE, cfg.AVA.FORCE_TEST_FLIP = scale, crop, flip
                    logits = []
                    for shift in range(3):
                        rows = []
                        for c in range(n_clips):
                            _, b = dih.images_and_boxes_preprocessing(clips[c], 0, crop, shift, boxes=boxes[c], out=data[c],
                                                                      out_dtype=data.dtype, w_pad=wpad, c_pad=cpad,
                                                                      device=self.device)
                            rows.append(np.concatenate([np.full((len(b), 1), c, dtype=np.float64), b], axis=1))
                        eng.feed(names["proposals"], np.concatenate(rows).astype(np.float32))
                        eng.forward()
                        torch.cuda.synchronize()
                        lg = eng.fetch("pred").reshape(n_rois, -1).astype(np.float64)
                        per_pass[(scale, flip, shift)] = lg
                        logits.append(lg)
                    merged.append(merge_shifts(np.stack(logits), shift_validity(all_boxes, flip, scale, H, W, self.max_crop)))
        finally:
            cfg.TEST.SCALE, cfg.TEST.CROP_SIZE, cfg.AVA.FORCE_TEST_FLIP = saved
        return merge_scales_and_flips(merged), per_pass


# ---- the device-resident pass ----------------------------------------------------------------------------------------------

View = collections.namedtuple("View", ["scale", "flip", "shift", "crop"])


def multi_crop_views(scales=None, max_crop=256):
    """the views of one keyframe in merge order (combine_ava_multi_crops, metrics.py:604-614): scale, then flip in
    (False, True), then shift 0..2, each with the crop min(max_crop, scale)"""
    scales = list(scales if scales is not None else cfg.AVA.TEST_MULTI_CROP_SCALES)
    return [View(int(s), flip, shift, min(int(max_crop), int(s))) for s in scales for flip in (False, True) for shift in range(3)]


class _Staging(object):
    """one set of pinned buffers of a minibatch: clip items and proposals of every view, the rows' original boxes and frame
    sizes, the store-slot table and the bank query; rewritten only behind the event of its last copy"""

    def __init__(self, n_views, N, T, R, hip, torch):
        pin = lambda n, dtype: torch.zeros(n, dtype=dtype).pin_memory()
        self.items = pin(n_views * N * hip.CLIP_ITEM_BYTES, torch.uint8)
        self.items_np = self.items.numpy()
        self.view_items = [(hip.ClipItem * N).from_buffer(self.items_np, v * N * hip.CLIP_ITEM_BYTES) for v in range(n_views)]
        self.props = pin(n_views * R * 5, torch.float32)
        self.boxes = pin(R * 4, torch.float64)
        self.hw = pin(R * 2, torch.int32)
        self.index = pin(N * T, torch.int32)
        self.query = pin(R * 3, torch.int32)
        self.done = torch.cuda.Event()
        self.in_flight = False


class AvaMultiCropPass(object):
    """The multi-crop test of AVA over a frame store, `pred` and the merge on the device.

        p = AvaMultiCropPass(index, make_store, params, dtype="bf16", bank=bank)
        result = p.run(groundtruth, excluded_keys, class_whitelist)       # frame-mAP dict + "scores"

    index: a test-split datasets.ava.AvaIndex (not lfb_infer_only); make_store(device, stream) builds the FrameStore (with
    its `fetch` / `fetch_jpeg`) on the pass's stream; params: {name: array} fed to every engine (None: the caller loads
    them, see `engines`); bank: a vlfb.lfb_bank.DeviceBank for models with LFB.ENABLED.

    One forward-only engine per distinct crop size min(max_crop, scale), built by an AvaMultiCropTester (`self.tester`,
    which can also run these engines its own way).  Per minibatch (`run_minibatch`): the clips' frames are resolved to store
    slots ONCE; the host plans the 18 views (datasets.data_input_helper.plan_minibatch / pack_items, with TEST.SCALE,
    TEST.CROP_SIZE and AVA.FORCE_TEST_FLIP set as the tester sets them and put back afterwards) into one pinned staging
    set, which goes up in one copy per array; then, per view, ONE vlfb_clip_batch_preprocess_indexed launch from the store
    into the engine's `data` blob, a device copy of the view's proposals, `forward`, and a device copy of `pred` into a
    [3][rows][classes] buffer; vlfb_multicrop_merge after shift 2.  Nothing in that loop waits for the device.  The bank
    window of every RoI is drawn once per minibatch (draw id iteration * N + clip, seed RNG_SEED) into every engine's `lfb`
    blob: the reference reseeds np.random at the start of each of its 18 passes, so they share their draws too.

    The meter is the pass's own and attached to no engine (an attached meter would be updated 18 times per minibatch); the
    host keeps, per real row, the image key, the original box and the table row (MetricsCalculator.add_ava_batch's
    bookkeeping): rows of clips that only pad the last batch and rows behind the last box are never named."""

    def __init__(self, index, make_store, params=None, dtype="bf16", device="cuda:0", scales=None, max_crop=256, bank=None,
                 rows=None, staging_sets=2, table_rows=None):
        import torch
        from datasets import data_input_helper as dh
        from vlfb import hip, passes
        from vlfb.metrics import DeviceMeter
        assert not index.lfb_infer_only and index.split != "train", "the multi-crop pass walks a test split"
        assert int(staging_sets) >= 2, "at least two staging sets"
        hip.lib()
        self.index, self.bank, self.device = index, bank, torch.device(device)
        self.views = multi_crop_views(scales, max_crop)
        self.scales = [v.scale for v in self.views[::6]]
        self.max_crop = int(max_crop)
        self.N = N = index.batch_size // cfg.NUM_GPUS
        self.T = T = int(index.video_length)
        self.rows = R = int(rows) if rows is not None else N * passes.most_boxes(index)
        self.cols = cols = int(cfg.MODEL.NUM_CLASSES)
        self.n_batches = -(-index.get_db_size() // N)
        n_items = int(table_rows) if table_rows is not None else self.n_batches * R
        lfb_shape = None
        if bank is not None:
            self.bank_window, self.bank_max = int(cfg.LFB.WINDOW_SIZE), int(cfg.AVA.LFB_MAX_NUM_FEAT_PER_STEP)
            self.bank_seed = int(cfg.RNG_SEED)
            lfb_shape = (R, self.bank_window * self.bank_max, bank.dim)
        self.tester = AvaMultiCropTester(params if params is not None else {}, dtype, device, self.scales, max_crop)
        self.engines, self._per_crop = [], {}
        saved = cfg.TEST.CROP_SIZE
        try:
            for crop in sorted(set(v.crop for v in self.views)):
                model, eng = self.tester._engine(crop, N, T, R, lfb_shape)
                names = {n.split("_")[0]: n for n in model.input_blob_names}
                if "lfb" in names and bank is None:
                    raise hip.VlfbError("AvaMultiCropPass: the model reads a feature bank (LFB.ENABLED); pass bank=")
                data, (w_pad, c_pad) = eng.blob_padded(names["data"])
                pred, code = eng.blob_tensor("pred")
                assert pred.numel() == R * cols, "pred holds %d elements, %d rows x %d classes planned" % (pred.numel(), R, cols)
                e = dict(model=model, eng=eng, data=data, w_pad=w_pad, c_pad=c_pad, code=hip.dtype_code(data.dtype),
                         clip_bytes=data[0].numel() * data.element_size(), props=eng.input_tensor(names["proposals"]),
                         pred=pred, pred_code=code, lfb=eng.input_tensor(names["lfb"]) if bank is not None else None)
                assert e["props"].numel() == R * 5
                self._per_crop[crop] = e
                self.engines.append((model, eng))
        finally:
            cfg.TEST.CROP_SIZE = saved
        self.engine_of_crop = {crop: e["eng"] for crop, e in self._per_crop.items()}
        first = next(iter(self._per_crop.values()))
        assert all(e["pred_code"] == first["pred_code"] for e in self._per_crop.values())
        self.pred_code = first["pred_code"]
        self.stream = torch.cuda.Stream(device=self.device)
        self.store = make_store(self.device, self.stream)
        assert self.store.stream is self.stream, "the frame store must be built on the pass's stream"
        self.meter = DeviceMeter("ava", cols, n_items=n_items, device=self.device)
        dev = self.device
        nv = len(self.views)
        self._sets = [_Staging(nv, N, T, R, hip, torch) for _ in range(int(staging_sets))]
        self._cur = 0
        self._store_frames = np.full(N, self.store.capacity, dtype=np.int32)
        self.dev_items = torch.zeros(nv * N * hip.CLIP_ITEM_BYTES, dtype=torch.uint8, device=dev)
        self.dev_props = torch.zeros(nv * R * 5, dtype=torch.float32, device=dev)
        self.dev_boxes = torch.zeros(R * 4, dtype=torch.float64, device=dev)
        self.dev_hw = torch.zeros(R * 2, dtype=torch.int32, device=dev)
        self.dev_index = torch.zeros(N * T, dtype=torch.int32, device=dev)
        self.dev_query = torch.zeros(R * 3, dtype=torch.int32, device=dev)
        self.logits = torch.zeros(3 * R * cols, dtype=first["pred"].dtype, device=dev)
        self.acc = torch.zeros(n_items * cols, dtype=torch.float64, device=dev)          # the merged scores of every issued row
        self.valid = torch.zeros((nv // 3) * n_items, dtype=torch.uint8, device=dev)     # [scale x flip][row]: shifts that saw the box
        self.out32 = torch.zeros(R * cols, dtype=torch.float32, device=dev)
        self.zero_labels = torch.zeros(R * cols, dtype=torch.int32, device=dev)
        self.n_items, self._pos = n_items, 0
        self._rows, self._keys, self._boxes, self._meta = [], [], [], []
        self.host_seconds = 0.0                      # host time spent in run_minibatch so far
        self.trace = None                            # a list: gets (first table row, view, a device copy of `pred`) per view
        # the engines' and this object's buffers were filled on the constructing thread's stream
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        self._dh = dh

    # ---- one minibatch ---------------------------------------------------------------------------
    def run_minibatch(self, frames_list, boxes_list, labels_list, meta, rng=np.random, spatial_shift_pos=None):
        """what datasets.ava.minibatch_source yields for a test split: clips as (store, video, frame_numbers) into the
        pass's store, (k, 4) normalised boxes and labels per clip, meta = dict(iteration=, videos=, secs=, padded=).
        Enqueues the 18 views and the merge; waits for nothing but a staging set's own last copy."""
        import time
        import torch
        from vlfb import hip
        t0 = time.perf_counter()
        dh, N, T, R, cols = self._dh, self.N, self.T, self.rows, self.cols
        assert len(frames_list) == N and len(boxes_list) == N, "a minibatch is %d clips" % N
        if self._pos + R > self.n_items:
            raise hip.VlfbError("AvaMultiCropPass: more minibatches than the %d table rows planned" % self.n_items)
        st = self._sets[self._cur]
        self._cur = (self._cur + 1) % len(self._sets)
        if st.in_flight:
            st.done.synchronize()                      # the only host wait: this set's own last copies
            st.in_flight = False
        store = self.store
        try:
            index = st.index.numpy().reshape(N, T)
            for i, f in enumerate(frames_list):
                assert isinstance(f, tuple) and len(f) == 3 and f[0] is store, "clips are (store, video, frame_numbers) of the pass's store"
                assert len(f[2]) == T, "clips of %d frames" % T
            # decode / upload what is not resident: once for the 18 views, in one call for the minibatch
            for i, slots in enumerate(store.slots_many([(f[1], f[2]) for f in frames_list])):
                index[i] = slots
            sizes = [(store.height, store.width)] * N
            ptrs = [store.data_ptr()] * N
            norm = [np.asarray(b, dtype=np.float64).reshape(-1, 4) for b in boxes_list]
            counts = [len(b) for b in norm]
            used = int(sum(counts))
            assert used <= R, "minibatch of %d RoIs, %d rows planned" % (used, R)
            clip_of = np.repeat(np.arange(N), counts)
            boxes = st.boxes.numpy().reshape(R, 4)
            boxes[:] = 0.0
            boxes[:used] = np.concatenate(norm + [np.zeros((0, 4))])
            st.hw.numpy().reshape(R, 2)[:] = (store.height, store.width)
            videos, secs = np.asarray(meta["videos"]), np.asarray(meta["secs"])
            if self.bank is not None and used:
                q = self.bank.window_query(videos[clip_of], secs[clip_of], int(meta["iteration"]) * N + clip_of)
                st.query.numpy()[:3 * used] = q.reshape(-1)
            labels = [np.zeros((k, cols), dtype=np.int32) for k in counts]
            props = st.props.numpy().reshape(len(self.views), R, 5)
            saved = (cfg.TEST.SCALE, cfg.TEST.CROP_SIZE, cfg.AVA.FORCE_TEST_FLIP)
            try:
                for v, view in enumerate(self.views):
                    e = self._per_crop[view.crop]
                    cfg.TEST.SCALE, cfg.TEST.CROP_SIZE, cfg.AVA.FORCE_TEST_FLIP = view.scale, view.crop, view.flip
                    plans, colors, tboxes = dh.plan_minibatch(sizes, 0, view.crop, view.shift, norm, rng)
                    dst = [e["data"].data_ptr() + i * e["clip_bytes"] for i in range(N)]
                    dh.pack_items(st.view_items[v], plans, colors, [T] * N, sizes, view.crop, ptrs, dst, [0] * N, e["w_pad"],
                                  e["c_pad"], self.device)
                    props[v], _, n = dh.minibatch_rows(tboxes, labels, R, cols)
                    assert n == used
                # behind what the calling thread's stream was given since the last minibatch (parameters loaded after the
                # constructor, a bank that was appended to): an event, no host wait
                self.stream.wait_stream(torch.cuda.current_stream(self.device))
                with torch.cuda.stream(self.stream):
                    self._enqueue(st, used)
            finally:
                cfg.TEST.SCALE, cfg.TEST.CROP_SIZE, cfg.AVA.FORCE_TEST_FLIP = saved
        finally:
            store.release()                            # enqueued (or abandoned): the store may evict these frames again
        # what the host keeps: the real rows only
        padded = np.asarray(meta.get("padded", [False] * N), dtype=bool)
        for r in range(used):
            c = int(clip_of[r])
            if padded[c]:
                continue
            self._rows.append(self._pos + r)
            self._keys.append("%s,%04d" % (self.index.video_idx_to_name[int(videos[c])], int(secs[c])))
            self._boxes.append(norm[c][r - int(np.sum(counts[:c]))])
            self._meta.append((int(videos[c]), int(secs[c])))
        self._pos += R
        self.host_seconds += time.perf_counter() - t0

    def _enqueue(self, st, used):
        """on the pass's stream: the staging set in one copy per array, the bank window, then per view preprocess / proposals
        / forward / pred, the merge behind every third view, the meter behind the last"""
        from vlfb import hip
        N, T, R, cols = self.N, self.T, self.rows, self.cols
        self.dev_items.copy_(st.items, non_blocking=True)
        self.dev_props.copy_(st.props, non_blocking=True)
        self.dev_boxes.copy_(st.boxes, non_blocking=True)
        self.dev_hw.copy_(st.hw, non_blocking=True)
        self.dev_index.copy_(st.index, non_blocking=True)
        if self.bank is not None and used:
            self.dev_query.copy_(st.query, non_blocking=True)
        st.done.record(self.stream)
        st.in_flight = True
        if self.bank is not None:
            per_row = self.bank_window * self.bank_max * self.bank.dim
            for e in self._per_crop.values():
                if used < R:
                    e["lfb"][used * per_row:R * per_row].zero_()      # padding rows: an empty bank window
                if used:
                    self.bank.sample_window_enqueue(self.dev_query, used, self.bank_window, self.bank_max, self.bank_seed, e["lfb"])
        item_bytes = N * hip.CLIP_ITEM_BYTES
        last = len(self.views) - 1
        for v, view in enumerate(self.views):
            e = self._per_crop[view.crop]
            cfg.TEST.SCALE, cfg.TEST.CROP_SIZE, cfg.AVA.FORCE_TEST_FLIP = view.scale, view.crop, view.flip
            hip.call("vlfb_clip_batch_preprocess_indexed", C.cast(st.view_items[v], C.c_void_p), self.dev_items.data_ptr() + v * item_bytes,
                     N, st.index.data_ptr(), self.dev_index.data_ptr(), T, self._store_frames.ctypes.data, e["code"])
            e["props"].copy_(self.dev_props[v * R * 5:(v + 1) * R * 5], non_blocking=True)
            e["eng"].forward()
            self.logits[view.shift * R * cols:(view.shift + 1) * R * cols].copy_(e["pred"], non_blocking=True)
            if self.trace is not None:
                self.trace.append((self._pos, view, e["pred"].clone()))
            if view.shift == 2:
                g = v // 3
                hip.call("vlfb_multicrop_merge", self.logits.data_ptr(), self.pred_code, R * cols, cols, self.dev_boxes.data_ptr(),
                         self.dev_hw.data_ptr(), R, cols, view.scale, self.max_crop, int(view.flip), int(g == 0),
                         self.acc.data_ptr() + self._pos * cols * 8, self.out32.data_ptr() if v == last else None,
                         self.valid.data_ptr() + g * self.n_items + self._pos)
        self.meter.update_ptr(self.out32.data_ptr(), hip.F32, self.zero_labels.data_ptr(), R)

    # ---- the whole pass --------------------------------------------------------------------------
    def run(self, groundtruth, excluded_keys=(), class_whitelist=None, rng=None):
        """every keyframe of the index, then `finish`"""
        from datasets import ava
        rng = np.random if rng is None else rng
        for args in ava.minibatch_source(self.index, self.store, rng):
            self.run_minibatch(*args)
        return self.finish(groundtruth, excluded_keys, class_whitelist)

    def detections(self):
        """(table rows, image keys, boxes [n][4], metadata [n][2] = (video index, second)) of the rows named so far"""
        return (np.asarray(self._rows, np.int64), list(self._keys), np.asarray(self._boxes, np.float64).reshape(-1, 4),
                np.asarray(self._meta, np.int64).reshape(-1, 2))

    def finish(self, groundtruth, excluded_keys=(), class_whitelist=None):
        """one synchronisation; the store's decode check; no named row may have been missed by every crop of some (scale,
        flip) (its merged score is NaN, which the meter's max-merge skips: the table row still holds -inf) -- VlfbError
        naming the image keys; then the meter's frame-mAP dict plus `scores` (the fp64 merged scores of the named rows, in
        detection order), `rows`, `keys`, `boxes` and `metadata`."""
        import torch
        from vlfb import hip
        self.stream.synchronize()
        self.store.check_decoded()
        rows, keys, boxes, meta = self.detections()
        pick = torch.from_numpy(rows).to(self.device)
        missed = torch.isneginf(self.meter.table[pick]).any(dim=1).cpu().numpy() if rows.size else np.zeros(0, bool)
        if missed.any():
            names = sorted(set(k for k, m in zip(keys, missed) if m))
            raise hip.VlfbError("AvaMultiCropPass: %d box(es) lie outside every crop of some (scale, flip): %s"
                                % (int(missed.sum()), "; ".join(names)))
        out = self.meter.finalize(rows, keys, boxes, groundtruth, excluded_keys, class_whitelist)
        out["scores"] = self.acc.view(self.n_items, self.cols)[pick].cpu().numpy()
        out.update(rows=rows, keys=keys, boxes=boxes, metadata=meta)
        return out


def write_merged_scores(path, result, video_idx_to_name, class_whitelist=None):
    """the merged scores of `AvaMultiCropPass.finish` as the reference's final_multi_crop_testing_results.csv: the lines of
    its detection files (utils.ava_eval_helper.write_results: key, box with three decimals, class id) with the score as
    '%f' (merge_ava_score_files, metrics.py:703-710)"""
    from utils import ava_eval_helper as A
    scores = result["scores"]
    whitelist = set(class_whitelist) if class_whitelist else set(range(1, scores.shape[1] + 1))
    boxes5 = np.concatenate([np.zeros((len(result["boxes"]), 1)), result["boxes"]], axis=1)
    b, l, s = A.get_ava_eval_data(scores, boxes5, result["metadata"], whitelist, video_idx_to_name=video_idx_to_name)
    with open(path, "w") as f:
        for key in b.keys():
            for box, label, score in zip(b[key], l[key], s[key]):
                f.write("%s,%.03f,%.03f,%.03f,%.03f,%d,%s\n" % (key, box[1], box[0], box[3], box[2], label, "%f" % score))
    return path


def run_ava_multi_crop(params_file, store, groundtruth, excluded_keys=(), class_whitelist=None, dtype="bf16", device="cuda:0",
                       max_crop=256, bank=None, out_csv=None, rng=None):
    """tools/test_net.py:57-87 for AVA.TEST_MULTI_CROP, the counterpart of lfb_pass.get_lfb: for every threshold of
    AVA.DETECTION_SCORE_THRESH_EVAL the test index at that threshold (AVA.FULL_EVAL), the engines with the parameters of
    `params_file`, `store(device, stream)` for the frames, the pass, the mAP logged, and with `out_csv` the merged scores in
    the reference's format (one file per threshold: the threshold goes into the name when there are several).
    -> {threshold: what AvaMultiCropPass.finish returns}"""
    from datasets import ava
    from utils import checkpoints
    assert params_file, "No params files specified for testing model."
    thresholds = list(cfg.AVA.DETECTION_SCORE_THRESH_EVAL)
    results = {}
    for threshold in thresholds:
        cfg.AVA.DETECTION_SCORE_THRESH = threshold
        cfg.AVA.FULL_EVAL = True
        index = ava.AvaIndex.from_cfg(cfg.TEST.DATA_TYPE or "test", False)
        p = AvaMultiCropPass(index, store, None, dtype, device, None, max_crop, bank)
        for model, eng in p.engines:
            eng.init_params()
            checkpoints.load_model_from_params_file_for_test(model, params_file)
        r = p.run(groundtruth, excluded_keys, class_whitelist, rng)
        logger.info("Box@%.5f multi-crop testing finished: %d detections of %d keyframes, mAP: %.3f",
                    threshold, r["detections"], index.get_db_size(), r["mean_ap"])
        if out_csv:
            path = out_csv
            if len(thresholds) > 1:
                stem, ext = os.path.splitext(out_csv)
                path = "%s_%.03f%s" % (stem, threshold, ext)
            r["csv"] = write_merged_scores(path, r, index.video_idx_to_name, class_whitelist)
        results[threshold] = r
    return results
