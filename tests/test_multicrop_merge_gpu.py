"""vlfb_multicrop_merge (include/vlfb.h, "AVA multi-crop merge") through hip.call: the three spatial shifts of one (scale,
flip) merged and accumulated in fp64 on the device.  Held to the reference-executed fixture (tests/golden/ref_aux.npz:
lib/utils/metrics.py:623-711 run on synthetic score files) and to vlfb.multicrop.shift_validity / merge_shifts, which
tests/test_ref_aux.py pins to that fixture exactly.

Bounds.  rtol = 1e-12 is the project's bound for this arithmetic (tests/test_multicrop.py): the device's fp64 exp and the
host's differ by a few ulp (2.2e-16 each), and another spelling of the fp64 sigmoid by at most 3.7e-16 relative.  Against
`mc_final` -- the reference's sum written with '%f' -- the bound is the half unit of that format, 5e-7, plus 1e-11 for the
six fp64 additions."""
import json
import os

import numpy as np
import pytest
import torch

from vlfb import hip
from vlfb import multicrop as mc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_aux.npz")
Z = np.load(GOLDEN)
META = json.loads(bytes(Z["meta"]).decode())
RTOL = 1e-12
NP_OF = {hip.F32: np.float32, hip.F16: np.float16}


def dev():
    return torch.device("cuda:0")


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def merge(logits, code, shift_stride, ld, boxes, hw, rows, cols, scale, max_crop, flip, first, acc, out32=None, valid=None):
    hip.call("vlfb_multicrop_merge", hip.ptr(logits), code, shift_stride, ld, hip.ptr(boxes), hip.ptr(hw), rows, cols, scale,
             max_crop, int(flip), int(first), hip.ptr(acc), hip.ptr(out32), hip.ptr(valid))
    torch.cuda.synchronize()


def mask_of(valid3):
    """(3, R) bool -> the kernel's bit mask per row"""
    v = np.asarray(valid3, dtype=np.uint8)
    return v[0] | (v[1] << 1) | (v[2] << 2)


@pytest.mark.parametrize("k", range(len(META["multicrop"])))
def test_against_the_reference_executed_fixture(k):
    """the fixture's logits are the fp64 values of the reference's score files: fed as VLFB_F64"""
    case = META["multicrop"][k]
    boxes, logits = Z["mc_%d_boxes" % k], Z["mc_%d_logits" % k]
    combined, final = Z["mc_%d_combined" % k], Z["mc_%d_final" % k]
    R, Cc = boxes.shape[0], logits.shape[-1]
    assert (R, Cc) == (9, 3) and logits.dtype == np.float64
    H, W = case["height"], case["width"]
    d_boxes = up(boxes.astype(np.float64))
    d_hw = up(np.tile(np.array([H, W], np.int32), (R, 1)))
    acc = torch.full((R, Cc), 7.0, dtype=torch.float64, device=dev())         # `first` must overwrite whatever is there
    alone = torch.full((R, Cc), 8.0, dtype=torch.float64, device=dev())
    out32 = torch.zeros((R, Cc), dtype=torch.float32, device=dev())
    valid = torch.zeros(R, dtype=torch.uint8, device=dev())
    total, first = 0.0, True
    for si, scale in enumerate(case["scales"]):
        for fi, flip in enumerate((False, True)):
            d_lg = up(logits[si, fi])
            merge(d_lg, hip.F64, R * Cc, Cc, d_boxes, d_hw, R, Cc, scale, 256, flip, True, alone, None, valid)
            want_valid = mc.shift_validity(boxes, flip, scale, H, W)
            assert np.array_equal(valid.cpu().numpy(), mask_of(want_valid)), (scale, flip)
            got, want = alone.cpu().numpy(), combined[si, fi]
            print("case %d scale %d flip %d: max rel diff to mc_combined %.3e" % (
                k, scale, flip, float(np.max(np.abs(got - want) / np.abs(want)))))
            assert np.allclose(got, want, rtol=RTOL, atol=0), (scale, flip)
            merge(d_lg, hip.F64, R * Cc, Cc, d_boxes, d_hw, R, Cc, scale, 256, flip, first, acc, out32, None)
            total = total + want                                              # the sequential sum of mc_combined
            first = False
            assert np.allclose(acc.cpu().numpy(), total, rtol=RTOL, atol=0), (scale, flip)
            assert np.array_equal(out32.cpu().numpy(), acc.cpu().numpy().astype(np.float32)), (scale, flip)
    worst = float(np.abs(acc.cpu().numpy() - final).max())
    print("case %d: |acc - mc_final| max %.3e" % (k, worst))
    assert worst <= 5e-7 + 1e-11


ROWS, COLS, LD = 257, 80, 88


def _big_case(code, seed=5):
    rng = np.random.default_rng(seed)
    stride = ROWS * LD + 24
    lg = rng.standard_normal((3, ROWS, COLS)) * 3
    if code == hip.BF16:
        t = torch.from_numpy(lg.astype(np.float32)).to(torch.bfloat16)
        rounded = t.to(torch.float32).numpy().astype(np.float64)
        buf = torch.full((3 * stride,), float("nan"), dtype=torch.bfloat16)
    else:
        rounded = lg.astype(NP_OF[code]).astype(np.float64)
        t = torch.from_numpy(lg.astype(NP_OF[code]))
        buf = torch.full((3 * stride,), float("nan"), dtype=t.dtype)
    for s in range(3):                                                   # NaN in the ld padding and between the shifts
        buf[s * stride:s * stride + ROWS * LD].view(ROWS, LD)[:, :COLS] = t[s]
    x1 = rng.uniform(0.0, 0.8, ROWS)
    x2 = x1 + rng.uniform(0.02, 0.2, ROWS)
    boxes = np.stack([x1, rng.uniform(0, 0.5, ROWS), x2, rng.uniform(0.5, 1, ROWS)], axis=1)
    sizes = np.array([(240, 426), (360, 640), (640, 360), (256, 256), (100, 300)], np.int32)    # landscape, portrait, square
    hw = sizes[rng.integers(0, len(sizes), ROWS)]
    return rounded, buf, stride, boxes, hw


@pytest.mark.parametrize("code", [hip.F32, hip.F16, hip.BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
def test_shapes_strides_and_types(code, flip):
    rounded, buf, stride, boxes, hw = _big_case(code)
    scale, max_crop = 320, 256
    PAD = 3                                                              # rows behind `rows` that must stay untouched
    acc = torch.full((ROWS + PAD, COLS), -5.0, dtype=torch.float64, device=dev())
    out32 = torch.full((ROWS + PAD, COLS), -6.0, dtype=torch.float32, device=dev())
    valid = torch.full((ROWS + PAD,), 77, dtype=torch.uint8, device=dev())
    merge(buf.to(dev()), code, stride, LD, up(boxes), up(hw), ROWS, COLS, scale, max_crop, flip, True, acc, out32, valid)
    want_valid = np.zeros((3, ROWS), bool)
    for r in range(ROWS):                                                # mixed frame sizes: row by row
        want_valid[:, r] = mc.shift_validity(boxes[r:r + 1], flip, scale, int(hw[r, 0]), int(hw[r, 1]), max_crop)[:, 0]
    n_valid = want_valid.sum(axis=0)
    assert set(n_valid.tolist()) >= {1, 2, 3}, "the case must exercise every number of valid shifts"
    want = mc.merge_shifts(rounded, want_valid)
    got, got32, got_valid = acc.cpu().numpy(), out32.cpu().numpy(), valid.cpu().numpy()
    assert np.array_equal(got_valid[:ROWS], mask_of(want_valid))
    assert np.array_equal(np.isnan(got[:ROWS]), np.isnan(want)), "NaN only where no shift sees the box (the padding must not leak)"
    assert np.allclose(got[:ROWS], want, rtol=RTOL, atol=0, equal_nan=True)
    assert np.array_equal(got32[:ROWS], got[:ROWS].astype(np.float32), equal_nan=True)
    assert (got[ROWS:] == -5.0).all() and (got32[ROWS:] == -6.0).all() and (got_valid[ROWS:] == 77).all()


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
def test_the_comparisons_are_strict(flip):
    """frame 256 x 512 at scale 256: nc = 0.5 exactly, so center = (0.25, 0.75), lcrop_right = rcrop_left = 0.5, and boxes
    whose x1 / x2 sit on 0.25, 0.5, 0.75 land on every boundary"""
    edges = [0.25, 0.5, 0.75]
    xs = [0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0]
    boxes = np.array([[a, 0.1, b, 0.9] for a in xs for b in xs if a < b and (a in edges or b in edges)])
    R, Cc = len(boxes), 2
    assert mc.shift_validity(np.array([[0.5, 0, 0.9, 1]]), False, 256, 256, 512)[0, 0] == False    # noqa: E712  x1 = 0.5: not left
    assert mc.shift_validity(np.array([[0.1, 0, 0.5, 1]]), False, 256, 256, 512)[2, 0] == False    # noqa: E712  x2 = 0.5: not right
    rng = np.random.default_rng(1)
    lg = rng.standard_normal((3, R, Cc)).astype(np.float32)
    acc = torch.zeros((R, Cc), dtype=torch.float64, device=dev())
    valid = torch.zeros(R, dtype=torch.uint8, device=dev())
    merge(up(lg), hip.F32, R * Cc, Cc, up(boxes), up(np.tile(np.array([256, 512], np.int32), (R, 1))), R, Cc, 256, 256, flip,
          True, acc, None, valid)
    want_valid = mc.shift_validity(boxes, flip, 256, 256, 512)
    assert np.array_equal(valid.cpu().numpy(), mask_of(want_valid)), list(zip(boxes.tolist(), valid.cpu().tolist(), mask_of(want_valid)))
    assert len(set(mask_of(want_valid).tolist())) >= 4
    assert np.allclose(acc.cpu().numpy(), mc.merge_shifts(lg, want_valid), rtol=RTOL, atol=0)


def test_a_box_no_crop_sees_is_nan_and_its_neighbours_are_not():
    boxes = np.array([[0.0, 0.1, 0.1, 0.9], [0.2, 0.1, 0.3, 0.9], [0.45, 0.1, 0.55, 0.9]])
    R, Cc = 3, 4
    hw = np.tile(np.array([100, 1000], np.int32), (R, 1))
    rng = np.random.default_rng(2)
    lg = rng.standard_normal((3, R, Cc)).astype(np.float32)
    acc = torch.zeros((R, Cc), dtype=torch.float64, device=dev())
    out32 = torch.zeros((R, Cc), dtype=torch.float32, device=dev())
    valid = torch.full((R,), 9, dtype=torch.uint8, device=dev())
    merge(up(lg), hip.F32, R * Cc, Cc, up(boxes), up(hw), R, Cc, 224, 256, False, True, acc, out32, valid)
    want_valid = mc.shift_validity(boxes, False, 224, 100, 1000)
    assert mask_of(want_valid).tolist() == [1, 0, 2]
    got, got32 = acc.cpu().numpy(), out32.cpu().numpy()
    assert valid.cpu().tolist() == [1, 0, 2]
    assert np.isnan(got[1]).all() and np.isnan(got32[1]).all()
    want = mc.merge_shifts(lg, want_valid)
    assert np.allclose(got[[0, 2]], want[[0, 2]], rtol=RTOL, atol=0) and not np.isnan(got32[[0, 2]]).any()


def test_first_zero_adds_to_what_is_there():
    rng = np.random.default_rng(3)
    R, Cc = 70, 5
    boxes = np.tile(np.array([0.3, 0.1, 0.7, 0.9]), (R, 1))
    hw = up(np.tile(np.array([240, 320], np.int32), (R, 1)))
    lg = up(rng.standard_normal((3, R, Cc)).astype(np.float32))
    d_boxes = up(boxes)
    once = torch.zeros((R, Cc), dtype=torch.float64, device=dev())
    twice = torch.full((R, Cc), 123.0, dtype=torch.float64, device=dev())
    out32 = torch.zeros((R, Cc), dtype=torch.float32, device=dev())
    merge(lg, hip.F32, R * Cc, Cc, d_boxes, hw, R, Cc, 256, 256, False, True, once)
    merge(lg, hip.F32, R * Cc, Cc, d_boxes, hw, R, Cc, 256, 256, False, True, twice)
    merge(lg, hip.F32, R * Cc, Cc, d_boxes, hw, R, Cc, 256, 256, False, False, twice, out32)
    a, b = once.cpu().numpy(), twice.cpu().numpy()
    assert (a > 0).all() and np.array_equal(b, 2.0 * a)                  # x + x is exact: a power-of-two multiple
    assert np.array_equal(out32.cpu().numpy(), b.astype(np.float32))


def test_no_rows_is_a_success_that_launches_nothing():
    keep = torch.full((4,), 3.0, dtype=torch.float64, device=dev())
    one = torch.zeros(4, dtype=torch.float32, device=dev())
    merge(one, hip.F32, 0, 1, keep, one.view(torch.int32), 0, 1, 224, 256, False, True, keep)
    assert (keep.cpu().numpy() == 3.0).all()
