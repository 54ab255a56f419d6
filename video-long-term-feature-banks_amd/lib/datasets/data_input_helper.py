"""Clip preprocessing with the pixel work on the GPU.

Mirror of the reference's lib/datasets/data_input_helper.py:70-139 `images_and_boxes_preprocessing`
(+ the geometry helpers of lib/datasets/image_processor.py:66-251): the HOST decides the geometry
exactly as the reference does (jitter scale, crop offsets, flip, box transforms -- a few scalars per
clip, drawn from the same `np.random` calls in the same order), ONE kernel (`vlfb_clip_preprocess`)
does resize + crop + flip + /255 + mean/std + BGR->RGB for all frames of the clip and writes the model's
`data` input in its device layout.  The reference runs cv2.resize / flip / NumPy per frame on
cfg.MODEL.SAMPLE_THREADS host threads and ships 19.3 MB of fp32 per clip through the blob queue; here
4.8 MB of uint8 cross PCIe (or nothing, if a GPU decoder produced the frames).

TRAIN.USE_COLOR_AUGMENTATION (off in every shipped config; color_augmentation_list, :142-151, and
image_processor.py:252-336): `plan_color` draws the order of the brightness / contrast / saturation jitter, their blend
factors and the PCA lighting offsets from the reference's `np.random` calls, after the geometry as the reference does, and
two kernels replace `vlfb_clip_preprocess` for that clip: `vlfb_clip_channel_sums` (integer per-frame channel sums of the
crop window, from which the contrast op's grey mean follows exactly) and `vlfb_clip_preprocess_color` (the same walk with
the colour chain between /255 and the normalisation).  The sums stay on the device.  The reference reads
cfg.TRAIN.PCA_JITTER_ONLY, which its config.py never defines; a missing key is read as False here (jitter and lighting).
"""
import ctypes as C
import math
import threading

import numpy as np
import torch

from core.config import config as cfg
from vlfb import hip

_COEF_BITS = 11


def resize_tables(src, dst):
    """cv::resize INTER_LINEAR (8-bit path) along one axis: left source index and the two 11-bit
    weights per destination index"""
    scale = 1.0 / (float(dst) / float(src))
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    low, high = s < 0, s >= src - 1
    f[low | high] = 0.0
    s[low] = 0
    s[high] = src - 1
    one = np.float32(1 << _COEF_BITS)
    coef = np.stack([np.rint((np.float32(1.0) - f) * one), np.rint(f * one)], axis=1)
    return s.astype(np.int32), np.clip(coef, -32768, 32767).astype(np.int16)


def _scaled_size(height, width, size):
    if (width <= height and width == size) or (height <= width and height == size):
        return height, width
    if width < height:
        return int(math.floor((float(height) / width) * size)), size
    return size, int(math.floor((float(width) / height) * size))


def _clip_boxes(boxes, height, width):
    boxes[:, [0, 2]] = np.minimum(width - 1., np.maximum(0., boxes[:, [0, 2]]))
    boxes[:, [1, 3]] = np.minimum(height - 1., np.maximum(0., boxes[:, [1, 3]]))
    return boxes


def plan_clip(height, width, split, crop_size, spatial_shift_pos, boxes=None, rng=np.random):
    """geometry of one clip: dict(resized_h, resized_w, y0, x0, flip) in the kernel's convention, and
    the transformed boxes"""
    if boxes is not None:
        boxes = np.asarray(boxes, dtype=np.float64).copy()
        boxes[:, [0, 2]] *= width
        boxes[:, [1, 3]] *= height
        boxes = _clip_boxes(boxes, height, width)
    if split == 1:
        lo, hi = cfg.TRAIN.JITTER_SCALES
        size = int(round(1.0 / rng.uniform(1.0 / hi, 1.0 / lo)))
        nh, nw = _scaled_size(height, width, size)
        if (nh, nw) != (height, width) and boxes is not None:
            boxes = boxes * float(nh) / height if width < height else boxes * float(nw) / width
        y0 = x0 = 0
        if (nh, nw) != (crop_size, crop_size):
            if nh > crop_size:
                y0 = int(rng.randint(0, nh - crop_size))
            if nw > crop_size:
                x0 = int(rng.randint(0, nw - crop_size))
            if boxes is not None:
                boxes[:, [0, 2]] -= x0
                boxes[:, [1, 3]] -= y0
        flip = bool(rng.uniform() < 0.5)
        if flip:
            if boxes is not None:
                b = boxes.copy()
                b[:, 0] = crop_size - boxes[:, 2] - 1
                b[:, 2] = crop_size - boxes[:, 0] - 1
                boxes = b
            x0 = x0 + crop_size - 1            # the window is walked right to left
    else:
        nh, nw = _scaled_size(height, width, cfg.TEST.SCALE)
        if (nh, nw) != (height, width) and boxes is not None:
            boxes *= (float(nh) / height) if width < height else (float(nw) / width)
        flip = bool(cfg.AVA.FORCE_TEST_FLIP and cfg.DATASET == 'ava')
        if flip and boxes is not None:
            b = boxes.copy()
            b[:, 0] = nw - boxes[:, 2] - 1
            b[:, 2] = nw - boxes[:, 0] - 1
            boxes = b
        y0 = int(math.ceil((nh - crop_size) / 2))
        x0 = int(math.ceil((nw - crop_size) / 2))
        if nh > nw:
            y0 = 0 if spatial_shift_pos == 0 else (nh - crop_size if spatial_shift_pos == 2 else y0)
        else:
            x0 = 0 if spatial_shift_pos == 0 else (nw - crop_size if spatial_shift_pos == 2 else x0)
        if boxes is not None:
            boxes[:, [0, 2]] -= x0
            boxes[:, [1, 3]] -= y0
        if flip:
            x0 = nw - 1 - x0                   # flipped BEFORE the crop: column x0 of the mirror image
    if boxes is not None:
        boxes = _clip_boxes(boxes, crop_size, crop_size)
    return dict(resized_h=nh, resized_w=nw, y0=y0, x0=x0, flip=int(flip)), boxes


def plan_color(rng=np.random):
    """colour augmentation of one train clip: None unless cfg.TRAIN.USE_COLOR_AUGMENTATION, else dict(ops, alphas, light)
    -- the jitter ops in the order they are applied (0 brightness, 1 contrast, 2 saturation), their blend factors, and
    the PCA lighting offset per SOURCE channel (B, G, R).  Draws, in the reference's order: permutation + one uniform per
    op (color_jitter_list, image_processor.py:317-336; skipped with TRAIN.PCA_JITTER_ONLY), then the normal of
    lighting_list (:253-269)."""
    if not cfg.TRAIN.USE_COLOR_AUGMENTATION:
        return None
    ops, alphas = [], []
    if not cfg.TRAIN.get("PCA_JITTER_ONLY", False):
        for k in rng.permutation(np.arange(3)):
            ops.append(int(k))
            alphas.append(1.0 + rng.uniform(-0.4, 0.4))
    alpha = rng.normal(0, 0.1, size=(1, 3))
    eigval = np.array(cfg.TRAIN.PCA_EIGVAL).astype(np.float32).reshape(1, 3)
    eigvec = np.array(cfg.TRAIN.PCA_EIGVEC).astype(np.float32)
    rgb = np.sum(eigvec * np.repeat(alpha, 3, axis=0) * np.repeat(eigval, 3, axis=0), axis=1)
    return dict(ops=ops, alphas=alphas, light=[float(rgb[2 - c]) for c in range(3)])


def clip_desc(plan, frames, height, width, crop_size, w_pad=0, c_pad=3):
    """the kernels' descriptor of a `plan_clip` plan"""
    d = hip.ClipDesc()
    d.frames, d.src_h, d.src_w = frames, height, width
    d.resized_h, d.resized_w = plan["resized_h"], plan["resized_w"]
    d.crop_h = d.crop_w = crop_size
    d.y0, d.x0, d.flip = plan["y0"], plan["x0"], plan["flip"]
    d.to_rgb = 0 if cfg.MODEL.USE_BGR else 1
    d.w_left, d.w_total, d.c_pad = w_pad, crop_size + 2 * w_pad, c_pad
    for c in range(3):
        d.mean[c] = float(np.float32(cfg.DATA_MEAN[c]))
        d.std[c] = float(np.float32(cfg.DATA_STD[c]))
    return d


def color_desc(color):
    """the colour kernel's descriptor of a `plan_color` plan"""
    q = hip.ClipColorDesc()
    q.n_ops = len(color["ops"])
    for i, (op, a) in enumerate(zip(color["ops"], color["alphas"])):
        q.op[i], q.alpha[i] = op, float(np.float32(a))
    for c in range(3):
        q.light[c] = float(np.float32(color["light"][c]))
    return q


_table_cache = {}
_table_lock = threading.Lock()        # the training thread and a loader thread (datasets.clip_loader) share the cache


def _tables(src, dst, device):
    key = (src, dst, str(device))
    with _table_lock:
        if key not in _table_cache:
            ofs, coef = resize_tables(src, dst)
            _table_cache[key] = (torch.as_tensor(ofs).to(device), torch.as_tensor(coef).to(device))
        return _table_cache[key]


def images_and_boxes_preprocessing(imgs, split, crop_size, spatial_shift_pos, boxes=None, out=None,
                                   out_dtype=torch.float32, w_pad=0, c_pad=3, device="cuda:0", rng=np.random):
    """imgs: (T, H, W, 3) uint8 BGR frames (NumPy array, list of frames, or a device tensor).
    Returns (clip, boxes): `clip` is `out` if given (a device tensor viewing frame 0 of the destination
    clip in the layout [T][crop][w_pad + crop + w_pad][c_pad], e.g. a slice of the engine's data blob),
    else a new tensor of that layout.  split == 1 is train (reference convention)."""
    if not torch.is_tensor(imgs):
        imgs = torch.as_tensor(np.ascontiguousarray(np.stack(list(imgs)) if not isinstance(imgs, np.ndarray) else imgs))
    assert imgs.dtype == torch.uint8 and imgs.dim() == 4 and imgs.shape[3] == 3, "frames must be (T, H, W, 3) uint8"
    frames = imgs.to(device).contiguous()
    T, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    plan, boxes = plan_clip(H, W, split, crop_size, spatial_shift_pos, boxes, rng)
    color = plan_color(rng) if split == 1 else None        # the reference draws the colours after the pixels are cut
    wtot = crop_size + 2 * w_pad
    if out is None:
        out = torch.zeros(T, crop_size, wtot, c_pad, device=device, dtype=out_dtype)
    assert out.is_contiguous() and out.numel() == T * crop_size * wtot * c_pad, "destination has the wrong size"
    d = clip_desc(plan, T, H, W, crop_size, w_pad, c_pad)
    xo = xc = yo = yc = None
    if (d.resized_h, d.resized_w) != (H, W):
        xo, xc = _tables(W, d.resized_w, frames.device)
        yo, yc = _tables(H, d.resized_h, frames.device)
    src = (hip.ptr(frames), hip.ptr(xo), hip.ptr(xc), hip.ptr(yo), hip.ptr(yc))
    if color is None:
        hip.call("vlfb_clip_preprocess", C.byref(d), *src, hip.ptr(out), hip.dtype_code(out.dtype))
    else:
        sums = torch.empty(T, hip.CLIP_SUM_BANDS, 3, device=frames.device, dtype=torch.int64)
        hip.call("vlfb_clip_channel_sums", C.byref(d), *src, hip.ptr(sums))
        hip.call("vlfb_clip_preprocess_color", C.byref(d), C.byref(color_desc(color)), *src, hip.ptr(sums), hip.ptr(out),
                 hip.dtype_code(out.dtype))
    torch.cuda.current_stream().synchronize()     # `frames` may be a temporary
    return out, boxes


# ---- the clips of one minibatch on one plan (datasets.clip_loader; vlfb.h vlfb_clip_item) ----

def plan_minibatch(sizes, split, crop_size, spatial_shift_pos, boxes_list=None, rng=np.random):
    """geometry and colour plans of the clips of one minibatch: `sizes` are the (height, width) of the clips' frames,
    `boxes_list` the clips' normalised boxes (or None, or None entries), `spatial_shift_pos` one position or one per clip.
    Returns (plans, colors, boxes): per clip what `plan_clip` and `plan_color` return.

    All draws come from the ONE `rng`, in minibatch order: clip 0's geometry, clip 0's colour, clip 1's geometry, ... --
    exactly what len(sizes) successive calls of `images_and_boxes_preprocessing` with that `rng` draw.  The reference
    preprocesses each clip in a worker process with a random state of its own (ava_data_input.py:117-128) and defines no
    order across the clips of a minibatch; this order is the definition here."""
    n = len(sizes)
    if boxes_list is None:
        boxes_list = [None] * n
    shifts = list(spatial_shift_pos) if isinstance(spatial_shift_pos, (list, tuple, np.ndarray)) else [spatial_shift_pos] * n
    assert len(boxes_list) == n and len(shifts) == n, "plan_minibatch: one entry per clip"
    plans, colors, boxes = [], [], []
    for (h, w), shift, b in zip(sizes, shifts, boxes_list):
        plan, b = plan_clip(int(h), int(w), split, crop_size, shift, b, rng)
        plans.append(plan)
        colors.append(plan_color(rng) if split == 1 else None)
        boxes.append(b)
    return plans, colors, boxes


def warm_tables(sizes, split, device):
    """build the resize tables every plan of sources of these (height, width) can ask for (all TRAIN.JITTER_SCALES of a
    train split, TEST.SCALE otherwise), so that a loader thread finds them in the cache and allocates nothing"""
    lo, hi = (cfg.TRAIN.JITTER_SCALES if split == 1 else (cfg.TEST.SCALE, cfg.TEST.SCALE))
    for h, w in sizes:
        for size in range(int(lo), int(hi) + 1):
            nh, nw = _scaled_size(int(h), int(w), size)
            if (nh, nw) != (int(h), int(w)):
                _tables(int(w), nw, device)
                _tables(int(h), nh, device)


def pack_items(items, plans, colors, frames, sizes, crop_size, frame_ptrs, dst_ptrs, sums_ptrs, w_pad, c_pad, device):
    """fill `items` (a ctypes array of hip.ClipItem, e.g. over a pinned buffer) for the vlfb_clip_batch_* entry points:
    clip i has frames[i] frames of sizes[i] = (height, width) at device address frame_ptrs[i], goes to dst_ptrs[i] and,
    if its colour plan has a contrast op, sums to sums_ptrs[i].  Table pointers come from the `_tables` cache.  Returns
    True when some item needs the sums launch."""
    need_sums = False
    for i, (plan, color) in enumerate(zip(plans, colors)):
        it = items[i]
        h, w = int(sizes[i][0]), int(sizes[i][1])
        it.geo = clip_desc(plan, int(frames[i]), h, w, crop_size, w_pad, c_pad)
        it.frames, it.dst = int(frame_ptrs[i]), int(dst_ptrs[i])
        it.xofs = it.xcoef = it.yofs = it.ycoef = 0
        if (plan["resized_h"], plan["resized_w"]) != (h, w):
            xo, xc = _tables(w, plan["resized_w"], device)
            yo, yc = _tables(h, plan["resized_h"], device)
            it.xofs, it.xcoef, it.yofs, it.ycoef = xo.data_ptr(), xc.data_ptr(), yo.data_ptr(), yc.data_ptr()
        it.color = color_desc(color) if color is not None else hip.ClipColorDesc()
        contrast = color is not None and hip.COLOR_CONTRAST in color["ops"]
        it.sums = int(sums_ptrs[i]) if contrast else 0
        need_sums = need_sums or contrast
    return need_sums


def minibatch_rows(boxes, labels_list, rows, num_classes):
    """the RoI rows of a minibatch as the model's inputs take them: proposals (rows, 5) fp32 = [clip index, x1, y1, x2,
    y2] per box in clip order (ava_data_input.py:175-192) and labels (rows, num_classes) int32, padded to the planned
    `rows` as Engine.feed pads a ragged batch: labels -1, box 0 of clip 0.  Returns (proposals, labels, used rows)."""
    props = np.zeros((rows, 5), dtype=np.float32)
    labels = np.full((rows, num_classes), -1, dtype=np.int32)
    r = 0
    for n, b in enumerate(boxes):
        k = 0 if b is None else len(b)
        if k == 0:
            continue
        assert r + k <= rows, "minibatch of more than the planned %d RoI rows" % rows
        props[r:r + k, 0] = n
        props[r:r + k, 1:] = np.asarray(b)[:, :4]
        labels[r:r + k] = np.asarray(labels_list[n], dtype=np.int32).reshape(k, num_classes)
        r += k
    return props, labels, r
