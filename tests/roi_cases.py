"""Case table, feature generators, fp64 references and error bounds shared by tests/test_roi_cases_host.py and
tests/test_roi_gpu.py (the RoI head: vlfb_roi_align_max_fwd / _bwd, csrc/vlfb_roi.hip).  CPU only; imports no vlfb.

Geometry: N = 3 clips on a 9 x 14 map (a 224-wide x 144-high image at scale 1/16), so that H != W everywhere.

Bounds (u = 2^-24, the unit roundoff of fp32; all derived from the kernel's operation count, none from its output):
  forward   a bin is sum over grid_h * grid_w samples of (w1 f1 + w2 f2 + w3 f3 + w4 f4), divided by the sample count.
            Every term passes through one rounding for its product, at most 4 * grid_h * grid_w - 1 additions up to the
            accumulator, and one division: (4 grid_h grid_w + 3) u A  with  A = the same sum over |f| (an upper bound
            with two roundings to spare; the bilinear weights are the oracle's own fp32 numbers, shared exactly).
  output    a 16-bit output rounds once more: u_out |ref| + 2^-25  (u_out = 2^-8 bf16, 2^-11 fp16; 2^-25 is half the
            smallest fp16 subnormal).
  backward  a pixel of dfeat receives at most M = max over clips of sum over the clip's RoIs of 4 grid_h grid_w
            read-modify-writes; each contribution is dout / count (one rounding) times a weight (one rounding):
            (M + 2) u S  with  S = the fp64 scatter of |dout| through the same bins (all weights are >= 0).

Channels are independent in RoIAlign, so every reference is computed once per (dtype, generator) at the widest channel
count and a case of C channels reads the first C of them.
"""
import functools

import numpy as np
import torch

from oracle.roi_align import roi_align_loop, roi_align_torch

N, H, W = 3, 9, 14
POOLED = 7
SCALE = 1.0 / 16
U32 = 2.0 ** -24

# [batch, x1, y1, x2, y2]; deliberately not sorted by clip, every clip has a RoI, every batch index is valid
ROIS = np.array([
    [0, 10, 20, 200, 130],
    [1, 0, 0, 223, 143],            # whole image
    [1, 100, 50, 108, 58],          # half a feature pixel
    [0, 3.3, 7.7, 15.2, 143],
    [1, 64, 64, 223, 100],
    [0, 0, 110, 223, 143],          # overlaps rows 0 and 3 in clip 0
    [2, -40, -40, 60, 50],          # starts beyond -1: first bins outside, then clamped at 0
    [2, -200, -200, -100, -100],    # wholly outside: every sample skipped
    [0, 150, 60, 120, 40],          # x2 < x1, y2 < y1: width and height forced to 1
    [2, 200, 100, 260, 180],        # runs off the right / bottom edge
    [1, 0, 0, 224, 144],            # last samples at exactly H, W
    [0, 37, 21, 37, 21],            # zero-area box
    [2, 0, 0, 447, 287],            # twice the image: grid 3 x 4, half the bins outside
], dtype=np.float32)
GRIDS = [(1, 2), (2, 2), (1, 1), (2, 1), (1, 2), (1, 2), (1, 1), (1, 1), (1, 1), (1, 1), (2, 2), (1, 1), (3, 4)]
R = ROIS.shape[0]
WHOLLY_OUTSIDE = 7

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
U_OUT = {"fp32": 0.0, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
VEC = {"fp32": 4, "bf16": 8, "fp16": 8}
GENERATORS = ("randn", "neg_relu", "dead")

# channel counts and the row-group count gr = min(1024 / (C / V), pooled) the host code derives for them at pooled = 7
CHANNELS = {
    "fp32": {32: 7, 640: 6, 800: 5, 1280: 3, 2048: 2, 2560: 1},
    "bf16": {32: 7, 1600: 5, 2048: 4, 4096: 2},
    "fp16": {32: 7, 1600: 5, 2048: 4, 4096: 2},
}
CMAX = {name: max(cs) for name, cs in CHANNELS.items()}
FWD_CASES = [(name, c, gen) for name in DTYPES for c in CHANNELS[name] for gen in GENERATORS]


def row_groups(dtype_name, c, pooled=POOLED):
    """the number of row groups per RoI vlfb_roi_align_max_fwd launches (csrc/vlfb_roi.hip, host side)"""
    return max(1, min(1024 // (c // VEC[dtype_name]), pooled))


def features(dtype_name, gen, c=None, seed=1234):
    """(N, c, H, W) fp32 numpy, rounded through the dtype (as q in gpu_util.py); the first c channels of the CMAX tensor"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, CMAX[dtype_name], H, W, generator=g)
    if gen == "neg_relu":
        x = -torch.relu(x - 0.3)
    elif gen == "dead":
        x[:, ::4] = 0.0
    else:
        assert gen == "randn"
    x = x.to(DTYPES[dtype_name]).to(torch.float32)
    return x[:, :c].contiguous().numpy()


def grids(rois, pooled):
    """(R,) grid_h, grid_w of the oracle for these boxes"""
    _, dbg = roi_align_loop(np.zeros((N, 1, H, W), np.float32), rois, pooled, SCALE)
    return dbg[:, 0, 0, 1].astype(np.int64), dbg[:, 0, 0, 2].astype(np.int64)


class Ref:
    """references of one (features, rois, pooled): everything is (R, C, pooled^2)"""

    def __init__(self, feat, rois=ROIS, pooled=POOLED):
        r, c = rois.shape[0], feat.shape[1]
        self.feat, self.rois, self.pooled = feat, rois, pooled
        out32, self.dbg = roi_align_loop(feat, rois, pooled, SCALE)
        self.ref32 = out32.reshape(r, c, -1)
        assert self.ref32.dtype == np.float32
        self.ref64 = roi_align_loop(feat.astype(np.float64), rois, pooled, SCALE)[0].reshape(r, c, -1)
        self.A = roi_align_loop(np.abs(feat).astype(np.float64), rois, pooled, SCALE)[0].reshape(r, c, -1)
        self.grid_h, self.grid_w = grids(rois, pooled)
        ops = 4 * self.grid_h * self.grid_w + 3
        self.fwd_bound = ops[:, None, None] * U32 * self.A

    def sliced(self, c):
        o = object.__new__(Ref)
        o.__dict__.update(self.__dict__)
        o.feat = np.ascontiguousarray(self.feat[:, :c])
        for k in ("ref32", "ref64", "A", "fwd_bound"):
            setattr(o, k, getattr(self, k)[:, :c])
        return o

    # --- what the kernel must produce
    @property
    def arg(self):
        """first maximal bin of the fp32 oracle (np.argmax returns the first of equal maxima)"""
        return self.ref32.argmax(axis=2)

    @property
    def ref64_at_arg(self):
        return np.take_along_axis(self.ref64, self.arg[:, :, None], 2)[:, :, 0]

    @property
    def fwd_bound_max(self):
        return self.fwd_bound.max(axis=2)

    def out_bound(self, dtype_name):
        """per (RoI, channel): max_bin(fwd_bound) + the rounding of a 16-bit output"""
        b = self.fwd_bound_max
        if dtype_name != "fp32":
            b = b + U_OUT[dtype_name] * np.abs(self.ref64_at_arg) + 2.0 ** -25
        return b


@functools.lru_cache(maxsize=None)
def _ref_wide(dtype_name, gen):
    return Ref(features(dtype_name, gen))


@functools.lru_cache(maxsize=None)
def ref(dtype_name, gen, c):
    return _ref_wide(dtype_name, gen).sliced(c)


@functools.lru_cache(maxsize=None)
def ref_pooled(dtype_name, gen, c, pooled):
    """another pooled resolution (smaller than 7), computed on its own"""
    return Ref(features(dtype_name, gen, c), ROIS, pooled)


def tie_stats(rf):
    """shares over (RoI, channel) pairs: exact fp32 tie for the maximum; ... whose first maximal bin is not bin 0; ... lies
    in pooled row >= 1; and near ties: the two largest fp64 bins closer than 2 max_bin(fwd_bound) WITHOUT an exact fp32 tie"""
    mx = rf.ref32.max(axis=2, keepdims=True)
    exact = (rf.ref32 == mx).sum(axis=2) >= 2
    arg = rf.arg
    top2 = np.sort(rf.ref64, axis=2)[:, :, -2:]
    near = ((top2[:, :, 1] - top2[:, :, 0]) < 2 * rf.fwd_bound_max) & ~exact
    return dict(exact=exact.mean(), exact_not_bin0=(exact & (arg != 0)).mean(),
                exact_row1=(exact & (arg >= rf.pooled)).mean(), near=near.mean())


# ---------------------------------------------------------------------------------------------------------------- backward
def dout(dtype_name, c, r=R, seed=77):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(r, CMAX[dtype_name], generator=g).to(DTYPES[dtype_name]).to(torch.float32)[:, :c].contiguous()


def bwd_ops(rois, pooled):
    """M: the largest number of read-modify-writes a pixel can receive = max over clips of sum of 4 grid_h grid_w"""
    gh, gw = grids(rois, pooled)
    per_clip = np.zeros(N, np.int64)
    np.add.at(per_clip, rois[:, 0].astype(np.int64), 4 * gh * gw)
    return int(per_clip.max())


def backward_ref(feat, rois, arg, do, pooled=POOLED):
    """fp64 autograd of (RoIAlign -> gather bin arg) w.r.t. feat: returns dfeat (N,C,H,W) fp64, S (the same scatter of
    |dout|) and bwd_bound, all numpy"""
    fd = torch.from_numpy(feat).double().requires_grad_(True)
    r, c = arg.shape
    bins = roi_align_torch(fd, rois, pooled, SCALE).reshape(r, c, pooled * pooled)
    sel = bins.gather(2, torch.from_numpy(arg).long().unsqueeze(2)).squeeze(2)
    (gf,) = torch.autograd.grad(sel, (fd,), do.double(), retain_graph=True)
    (s,) = torch.autograd.grad(sel, (fd,), do.double().abs())
    s = s.numpy()
    assert (s >= 0).all()
    return gf.numpy(), s, (bwd_ops(rois, pooled) + 2) * U32 * s
