"""vlfb_clip_channel_sums and vlfb_clip_preprocess_color against the fp32 restatement (tests/color_aug_ref.py) bit for
bit, the colour kernel against vlfb_clip_preprocess where it must agree with it, and the public path
(images_and_boxes_preprocessing with TRAIN.USE_COLOR_AUGMENTATION) against the reference's own clips
(tests/golden/ref_color_aug.npz) within the gate measured on the CPU (tests/color_aug_cases.py)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import color_aug_cases as cases
import color_aug_ref as R

pytestmark = pytest.mark.gpu
META, CASES = cases.load()

# geometry plans in the kernel's convention (x0 is the right edge of the window when flip is set); frames are 40 x 52
# except "big": 270 x 270 frames, a 260 x 260 crop = 67600 pixels, more than one pass of the colour kernel's 65536-thread grid
GEOMETRY = {
    "resize_flip": dict(resized_h=33, resized_w=43, y0=5, x0=30, flip=1, crop=(24, 24)),
    "noresize": dict(resized_h=40, resized_w=52, y0=3, x0=7, flip=0, crop=(24, 24)),
    "odd19x23": dict(resized_h=47, resized_w=61, y0=11, x0=2, flip=0, crop=(19, 23)),
    "rows5": dict(resized_h=33, resized_w=43, y0=28, x0=23, flip=1, crop=(5, 24)),
    "big": dict(resized_h=270, resized_w=270, y0=10, x0=0, flip=0, crop=(260, 260)),
}
_frames_cache = {}


def _frames(name):
    """three uint8 BGR frames of clearly different brightness (host array, device tensor)"""
    import torch
    h, w = (270, 270) if name == "big" else (40, 52)
    if (h, w) not in _frames_cache:
        rng = np.random.default_rng(h)
        f = rng.integers(0, 256, (3, h, w, 3)) * np.array([0.35, 0.7, 1.0]).reshape(3, 1, 1, 1)
        f = f.astype(np.uint8)
        _frames_cache[(h, w)] = (f, torch.as_tensor(f).cuda())
    return _frames_cache[(h, w)]


def _setup(name, to_rgb=1, w_pad=4, c_pad=4):
    """-> (host frames, argument tuple (frames, xofs, xcoef, yofs, ycoef) with what keeps it alive, descriptor, window)"""
    import torch
    from datasets import data_input_helper as dh
    g = GEOMETRY[name]
    crop_h, crop_w = g["crop"]
    host, dev = _frames(name)
    t, h, w = host.shape[:3]
    d = dh.clip_desc(g, t, h, w, crop_w, w_pad, c_pad)
    d.crop_h, d.to_rgb = crop_h, to_rgb
    keep = [dev]
    ptrs = [dev.data_ptr(), None, None, None, None]
    if (g["resized_h"], g["resized_w"]) != (h, w):
        xo, xc = dh.resize_tables(w, g["resized_w"])
        yo, yc = dh.resize_tables(h, g["resized_h"])
        keep += [torch.as_tensor(a).cuda() for a in (xo, xc, yo, yc)]
        ptrs[1:] = [k.data_ptr() for k in keep[1:]]
    return tuple(ptrs), keep, d, R.window_u8(host, g, crop_h, crop_w)


def _sums(src, d):
    import torch
    from vlfb import hip
    sums = torch.full((d.frames, hip.CLIP_SUM_BANDS, 3), -7, device="cuda", dtype=torch.int64)   # every slot must be written
    hip.call("vlfb_clip_channel_sums", C.byref(d), *src, hip.ptr(sums))
    return sums


def _color(src, d, color, out, sums="auto"):
    from datasets import data_input_helper as dh
    from vlfb import hip
    if sums == "auto":
        sums = _sums(src, d)
    hip.call("vlfb_clip_preprocess_color", C.byref(d), C.byref(dh.color_desc(color)), *src, hip.ptr(sums), hip.ptr(out),
             hip.dtype_code(out.dtype))
    return out


def _dst(d, dtype=None, lead=()):
    import torch
    return torch.zeros(*lead, d.frames, d.crop_h, d.w_total, d.c_pad, device="cuda", dtype=dtype or torch.float32)


def _plan(order, seed=0):
    rng = np.random.default_rng(100 + seed)
    return dict(ops=list(order), alphas=[float(a) for a in rng.uniform(0.6, 1.4, len(order))],
                light=[float(v) for v in rng.normal(0, 0.03, 3)])


def _mean_std(d):
    return [np.float32(d.mean[c]) for c in range(3)], [np.float32(d.std[c]) for c in range(3)]


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_channel_sums_are_the_integer_sums(name):
    src, keep, d, win = _setup(name)
    got = _sums(src, d).cpu().numpy()
    want = np.array(R.band_sums(win), dtype=np.int64)
    assert got.shape == want.shape == (3, 8, 3)
    assert np.array_equal(got, want)
    if name == "rows5":
        empty = [b for b in range(8) if b * 5 // 8 == (b + 1) * 5 // 8]
        assert empty == [0, 2, 5] and not got[:, empty].any() and got[:, [1, 3, 4, 6, 7]].all()
    assert want[0].sum() < 0.6 * want[1].sum() and want[1].sum() < 0.8 * want[2].sum()       # frames differ: per frame, not per clip


ORDERS = list(itertools.permutations(range(3))) + [()]


@pytest.mark.parametrize("to_rgb", [1, 0])
@pytest.mark.parametrize("order", ORDERS, ids=["".join(map(str, o)) or "pca_only" for o in ORDERS])
def test_color_kernel_matches_the_restatement_bit_for_bit(order, to_rgb):
    import torch
    name = "resize_flip" if to_rgb else "odd19x23"
    src, keep, d, win = _setup(name, to_rgb=to_rgb)
    color = _plan(order, seed=to_rgb)
    mean, std = _mean_std(d)
    want = R.color_clip(win, color, mean, std, bool(to_rgb))                       # (T, crop_h, crop_w, 3), destination order
    got = _color(src, d, color, _dst(d), sums="auto" if 1 in order else None).cpu().numpy()
    cw = d.crop_w
    assert np.all(got[:, :, :4] == 0) and np.all(got[:, :, 4 + cw:] == 0) and np.all(got[..., 3] == 0)
    assert np.array_equal(got[:, :, 4:4 + cw, :3], want)
    # bf16 destination = rounding of the fp32 result, straight into a slice of a larger buffer
    big = _dst(d, torch.bfloat16, lead=(2,))
    _color(src, d, color, big[1])
    ref16 = torch.as_tensor(want).to(torch.bfloat16).float().numpy()
    got16 = big[1].float().cpu().numpy()
    assert np.array_equal(got16[:, :, 4:4 + cw, :3], ref16)
    assert np.all(got16[:, :, :4] == 0) and np.all(got16[:, :, 4 + cw:] == 0) and np.all(got16[..., 3] == 0)
    assert float(big[0].abs().max()) == 0.0


def test_color_kernel_past_one_pass_of_its_grid():
    src, keep, d, win = _setup("big")
    color = _plan((2, 0, 1), seed=5)
    mean, std = _mean_std(d)
    got = _color(src, d, color, _dst(d)).cpu().numpy()
    assert np.array_equal(got[:, :, 4:4 + 260, :3], R.color_clip(win, color, mean, std, True))
    assert np.all(got[:, :, :4] == 0) and np.all(got[:, :, 4 + 260:] == 0) and np.all(got[..., 3] == 0)


@pytest.mark.parametrize("name", ["resize_flip", "noresize", "odd19x23"])
def test_no_ops_and_no_light_is_the_plain_kernel(name):
    from vlfb import hip
    src, keep, d, win = _setup(name)
    plain = _dst(d)
    hip.call("vlfb_clip_preprocess", C.byref(d), *src, hip.ptr(plain), hip.dtype_code(plain.dtype))
    got = _color(src, d, dict(ops=[], alphas=[], light=[0.0, 0.0, 0.0]), _dst(d), sums=None)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), plain.cpu().numpy().view(np.uint32))
    assert float(plain.abs().max()) > 0


@pytest.mark.parametrize("case", CASES, ids=["seed%d" % c["seed"] for c in CASES])
def test_public_path_matches_the_reference(case):
    """images_and_boxes_preprocessing with TRAIN.USE_COLOR_AUGMENTATION on every fixture case: every element within the
    CPU-measured gate of the clip the reference produced, and the reference's boxes"""
    from datasets import data_input_helper as dh
    crop = META["crop"]
    with cases.case_cfg(META, case["use_bgr"], True if case["pca_only"] else None):
        rng = np.random.RandomState(case["seed"])
        out, boxes = dh.images_and_boxes_preprocessing(case["frames"], META["split"], crop, META["shift"],
                                                       case["boxes_in"].copy(), w_pad=4, c_pad=4, rng=rng)
    assert float(rng.uniform()) == case["next_uniform"]
    assert np.array_equal(boxes, case["boxes_out"])
    got = out.cpu().numpy()
    assert got.shape == (3, crop, crop + 8, 4)
    assert np.all(got[:, :, :4] == 0) and np.all(got[:, :, 4 + crop:] == 0) and np.all(got[..., 3] == 0)
    clip = got[:, :, 4:4 + crop, :3].transpose(3, 0, 1, 2)
    diff = float(np.abs(clip.astype(np.float64) - case["clip"].astype(np.float64)).max())
    print("case seed %d: max abs diff %.3e (gate %.3e)" % (case["seed"], diff, cases.GATE))
    assert diff <= cases.GATE


def test_flag_off_launches_what_it_always_did():
    """with the switch off the loader's launch list is the single vlfb_clip_preprocess call"""
    from datasets import data_input_helper as dh
    from vlfb import hip
    case = CASES[0]
    with cases.case_cfg(META, color=False):
        rec = hip.trace_begin()
        try:
            dh.images_and_boxes_preprocessing(case["frames"], 1, META["crop"], 1, rng=np.random.RandomState(1))
        finally:
            hip.trace_end()
        assert [name for _, _, name in rec] == ["vlfb_clip_preprocess"]
    with cases.case_cfg(META):
        rec = hip.trace_begin()
        try:
            dh.images_and_boxes_preprocessing(case["frames"], 1, META["crop"], 1, rng=np.random.RandomState(1))
        finally:
            hip.trace_end()
        assert [name for _, _, name in rec] == ["vlfb_clip_channel_sums", "vlfb_clip_preprocess_color"]
