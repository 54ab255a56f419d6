"""The colour augmentation of the train clip, restated in NumPy float32 in the colour kernel's operation order.

TEST INFRASTRUCTURE ONLY: shares no code with the product (the resize is the oracle's restatement of cv2.resize).  This is
what vlfb_clip_channel_sums and vlfb_clip_preprocess_color are held to bit for bit; tests/test_color_aug_host.py holds
this file to the reference's own output (tests/golden/ref_color_aug.npz).

What the reference does (lib/datasets/data_input_helper.py:113-126, :142-151; lib/datasets/image_processor.py):
  the cropped, flipped frames are divided by 255 and cast to float32 (:113-118); color_jitter_list (:317-336) applies
  brightness_list (:296-303), contrast_list (:306-314) and saturation_list (:286-293) in a drawn order, each a
  blend(image, other, alpha) = image * alpha + other * (1 - alpha) (:272-273) with other = zeros / the grey image filled
  with its own mean / the grey image (grayscale, :277-283: 0.299 R + 0.587 G + 0.114 B of a BGR image); lighting_list
  (:253-269) adds rgb[2 - c] to channel c; color_normalization follows (:124-126).
It differs from the reference in rounding only: NumPy promotes the chain to float64 from the first blend on, here every
operation rounds to float32; alpha and the lighting offsets are rounded to float32 once; and the contrast op's grey mean
is the exact mean of the un-augmented uint8 window (integer band sums, one division in float64, one rounding) times the
blend factors of the brightness ops already applied, where the reference takes np.mean of the grey image it has at that
point (a saturation blend leaves a pixel's grey value unchanged up to rounding: the three weights add to one).

A geometry plan is dict(resized_h, resized_w, y0, x0, flip) in the kernel's convention (x0 is the right edge of the window
when flip is set); a colour plan is dict(ops, alphas, light): op codes 0 brightness, 1 contrast, 2 saturation in the order
applied, their blend factors, and the lighting offset per SOURCE channel (B, G, R).
"""
import numpy as np

from oracle import preprocess as op

BANDS = 8
BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2
F = np.float32


def window_u8(frames, plan, crop_h, crop_w):
    """(T, H, W, 3) uint8 BGR -> the (T, crop_h, crop_w, 3) uint8 pixels the kernels read, in output order"""
    h, w = frames.shape[1:3]
    if (plan["resized_h"], plan["resized_w"]) != (h, w):
        frames = np.stack([op.resize_u8(f, plan["resized_w"], plan["resized_h"]) for f in frames])
    cols = plan["x0"] + (-1 if plan["flip"] else 1) * np.arange(crop_w)
    assert cols.min() >= 0 and cols.max() < plan["resized_w"] and plan["y0"] + crop_h <= plan["resized_h"]
    return np.ascontiguousarray(frames[:, plan["y0"]:plan["y0"] + crop_h][:, :, cols])


def band_sums(win):
    """-> [T][BANDS][3] Python integers: the B, G, R sums over crop rows [b * crop_h // 8, (b + 1) * crop_h // 8)"""
    t, crop_h = win.shape[:2]
    return [[[int(win[f, b * crop_h // BANDS:(b + 1) * crop_h // BANDS, :, c].sum(dtype=np.int64)) for c in range(3)]
             for b in range(BANDS)] for f in range(t)]


def grey_mean(frame_sums, crop_h, crop_w):
    """the frame's mean grey value of x / 255: bands added in index order, float64, rounded to float32 once"""
    s = [sum(frame_sums[b][c] for b in range(BANDS)) for c in range(3)]
    num = np.float64(0.299) * np.float64(s[2]) + np.float64(0.587) * np.float64(s[1]) + np.float64(0.114) * np.float64(s[0])
    return F(num / (np.float64(255.0) * np.float64(crop_h * crop_w)))


def color_clip(win, color, mean, std, to_rgb):
    """win (T, crop_h, crop_w, 3) uint8 BGR -> float32 (T, crop_h, crop_w, 3) in the DESTINATION channel order"""
    t, crop_h, crop_w = win.shape[:3]
    sums = band_sums(win)
    ops = [int(o) for o in color["ops"]]
    alphas = [F(a) for a in color["alphas"]]
    light = [F(v) for v in color["light"]]
    out = np.empty(win.shape, F)
    for f in range(t):
        v = [win[f, :, :, c].astype(F) / F(255.0) for c in range(3)]                  # b, g, r
        m = grey_mean(sums[f], crop_h, crop_w)
        for k, o in enumerate(ops):                 # the mean as the contrast op meets it
            if o == CONTRAST:
                break
            if o == BRIGHTNESS:
                m = F(m * alphas[k])
        for o, a in zip(ops, alphas):
            if o == BRIGHTNESS:
                v = [x * a for x in v]
                continue
            other = m if o == CONTRAST else (F(0.299) * v[2] + F(0.587) * v[1]) + F(0.114) * v[0]
            rest = other * F(F(1.0) - a)
            v = [x * a + rest for x in v]
        for c in range(3):
            x = v[c] + light[c]
            x = x - F(mean[c])
            x = x / F(std[c])
            assert x.dtype == F
            out[f, :, :, 2 - c if to_rgb else c] = x
    return out
