"""Case table, generators and references shared by tests/test_pool_cases_host.py and tests/test_pool_gpu.py (the pooling
kernels of csrc/vlfb_pool.hip: vlfb_maxpool_fwd / _bwd / _relu_bwd, vlfb_avgpool_fwd / _bwd / _bwd_two_term).  CPU only;
imports no vlfb.  Written from the contract of include/vlfb.h, not from the kernels.  Tensors are channels-last
(N, T, H, W, C) throughout.

Max pools are compared BIT FOR BIT:
  forward   over the padded window in (t, h, w) order with a strict > from -inf: the value and the tap index of the first
            maximum.  The two-plane variant compares float32(hi) + float32(lo) and returns the selected element's planes.
  backward  per input element, in fp32: start at +0; add, in ascending (to, ho, wo) order, the dy of every covering window whose
            arg-max is this tap (with `y`: that dy replaced by 0 where y <= 0); add `add`; zero where mask <= 0; round once to
            the element type.  For one input element the covering windows in ascending (to, ho, wo) order are the window
            offsets (a, b, c) in DESCENDING order (a = ti + pt - to * st falls as `to` rises), and one offset maps every
            window to a different input element: so the emulation is one fp32 tensor add per offset, offsets descending, and
            every element sees exactly the additions above in exactly that order.

Average pools are compared per element with the fp64 reference under
            |got - ref| <= (n + 1) u S + 1/2 ulp_T(|ref|),       u = 2^-24,
  n = the number of fp32 additions feeding the element and S = the sum of |terms|: n additions from +0 (the first is exact)
  leave at most n - 1 roundings on any term, in any order; fl(1 / window) and the product with it are two more (one with a
  fused multiply-add): n + 1 roundings, (n + 1) u S to first order (the second-order term is below 1e-5 of the bound at the
  largest n here, 392).  A 16-bit output rounds once more (the ulp term; dropped for fp32 outputs).  Forward: the terms are
  x / window, n = window (2 * window for hi + lo planes).  Backward: the terms are dy / window per covering window, plus
  `add`; n = covering windows (+ 1 with add).
The average FORWARD pools are, beyond that bound, compared BIT FOR BIT with an fp32 emulation of their order of operations (no
multiply inside the sum, so nothing depends on fused multiply-adds):
  windowed  per output element, in fp32: start at +0; add the taps ascending in (a, b, c) -- of two planes fl32(hi + lo), formed
            before it is added; multiply once by fl32(1 / window); round once to the output type (fp32 for two planes).
  global    (one window = the whole clip) the positions in (t, h, w) order are rows 0 .. rows - 1: each of 32 row lanes sums
            rows rl, rl + 32, ... from +0, then the 32 partial sums are added in lane order from +0; multiply and round as above.
"""
import collections
import functools
import itertools
import zlib

import torch

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
ROUTE_DT = {"fp32": "f32", "bf16": "bf16", "fp16": "f16"}          # as vlfb_maxpool_bwd_describe spells them
VEC = {"fp32": 4, "bf16": 8, "fp16": 8}
MANT = {"fp32": 23, "bf16": 7, "fp16": 10}                          # stored mantissa bits
EMIN = {"fp32": -126, "bf16": -126, "fp16": -14}                    # smallest normal exponent
U32 = 2.0 ** -24
GENERATORS = ("randn", "levels", "relu_levels")
COMBOS = ("none", "add", "mask", "add_mask", "alias", "relu")       # operands of the backward; "relu" = vlfb_maxpool_relu_bwd(y)

MaxCase = collections.namedtuple("MaxCase", "name k s p shape C dtypes combos")
_ALL = tuple(DTYPES)
_PLAIN, _ADDMASK = ("none", "relu"), ("add", "mask", "add_mask", "alias")

# The smallest shapes that still reach each route of the backward (include/vlfb.h, vlfb_maxpool_bwd_describe, has the rule).
MAX_CASES = [
    # band R=3 bands=3: the last band has one row; the staging loop runs 540 (fp32: 1080) items, 9 (18) channel chunks
    MaxCase("band_r3", (1, 3, 3), (1, 2, 2), (0, 1, 1), (2, 2, 13, 23), 72, _ALL, _PLAIN),
    # Wo * C * (sizeof(T) + 1) = 13824 (fp32: 15360) bytes per pooled row: 65536 / that - 2 = 2
    MaxCase("band_r2", (1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 2, 9, 35), 256, ("bf16", "fp16"), COMBOS),
    MaxCase("band_r2_f32", (1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 2, 9, 23), 256, ("fp32",), COMBOS),
    # 16896 (fp32: 16640) bytes per pooled row: R = 1, the row kernel without add / mask -- fp32 pool1 at the real size
    MaxCase("row_133", (1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 1, 7, 43), 256, ("bf16", "fp16"), COMBOS),
    MaxCase("row_133_f32", (1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 1, 7, 25), 256, ("fp32",), COMBOS),
    # the geometry of band_r3 with add and / or mask: the row kernel, more than one trip of its 128-item loop
    MaxCase("row_133_addmask", (1, 3, 3), (1, 2, 2), (0, 1, 1), (2, 2, 13, 23), 72, _ALL, _ADDMASK),
    # ph != pw: a swapped pad moves every window
    MaxCase("pads_differ_h", (1, 3, 3), (1, 2, 2), (0, 1, 0), (1, 1, 9, 10), 24, _ALL, COMBOS),
    MaxCase("pads_differ_w", (1, 3, 3), (1, 2, 2), (0, 0, 1), (1, 1, 9, 10), 24, _ALL, COMBOS),
    # odd T: frame 4 of each clip has no window; 144 (fp32: 288) items per row
    MaxCase("temporal_odd", (2, 1, 1), (2, 1, 1), (0, 0, 0), (2, 5, 3, 9), 128, _ALL, COMBOS),
    # odd H and W: the last row and column have no window; 17 (34) chunks, 153 (306) items per row
    MaxCase("nl_odd", (1, 2, 2), (1, 2, 2), (0, 0, 0), (2, 2, 7, 9), 136, _ALL, COMBOS),
    # not a compiled window, overlapping in t as well
    MaxCase("generic_t_overlap", (2, 3, 3), (1, 2, 2), (1, 1, 1), (1, 3, 7, 7), 24, _ALL, COMBOS),
    # 256 taps: the two-byte arg-max
    MaxCase("generic_wide", (4, 8, 8), (2, 4, 4), (1, 2, 2), (1, 4, 8, 12), 8, _ALL, COMBOS),
]
MAX_BY_NAME = {c.name: c for c in MAX_CASES}
# forward on two fp16 planes, backward in fp16 with y = the hi plane of the pooled pair: the two max pools of the "mix" path
MIX_CASES = [
    MaxCase("mix_route_pool2", (2, 1, 1), (2, 1, 1), (0, 0, 0), (1, 4, 6, 7), 16, ("fp16",), ("relu",)),
    MaxCase("mix_route_pool1", (1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 4, 6, 7), 16, ("fp16",), ("relu",)),
]
MIX_GENERATORS = ("relu_randn", "relu_levels")

ALL_ROUTES = ("band R=3", "band R=2", "fixed 1x3x3/1x2x2 ymask", "fixed 1x3x3/1x2x2", "fixed 2x1x1/2x1x1", "fixed 1x2x2/1x2x2",
              "generic u8", "generic u16")


def out_dims(case):
    return tuple((n + 2 * p - k) // s + 1 for n, k, s, p in zip(case.shape[1:], case.k, case.s, case.p))


def expected_route(case, dtype_name, combo):
    """the route the table claims for this case, as vlfb_maxpool_bwd_describe spells it"""
    dt = ROUTE_DT[dtype_name]
    ym = " ymask" if combo == "relu" else ""
    taps = case.k[0] * case.k[1] * case.k[2]
    if case.name.startswith("generic"):
        return "generic %s %s%s" % ("u16" if taps > 255 else "u8", dt, ym)
    if case.name in ("temporal_odd", "mix_route_pool2"):
        return "fixed 2x1x1/2x1x1 %s%s" % (dt, ym)
    if case.name == "nl_odd":
        return "fixed 1x2x2/1x2x2 %s%s" % (dt, ym)
    if case.name.startswith("row_133") or combo in _ADDMASK:
        return "fixed 1x3x3/1x2x2 %s%s" % (dt, ym)
    bands = {"band_r3": "R=3 bands=3", "band_r2": "R=2 bands=3", "band_r2_f32": "R=2 bands=3",
             "pads_differ_h": "R=3 bands=2", "pads_differ_w": "R=3 bands=2", "mix_route_pool1": "R=3 bands=1"}[case.name]
    return "band %s %s%s" % (dt, bands, ym)


# ------------------------------------------------------------------------------------------------
# generators
# ------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def values(gen_name, shape, dtype, g):
    """fp32 tensor of values exactly representable in `dtype`"""
    if gen_name in ("randn", "relu_randn"):
        v = torch.randn(shape, generator=g)
        if gen_name == "relu_randn":
            v = torch.relu(v)
        return v if dtype is None else v.to(dtype).float()
    v = torch.randint(-3, 5, shape, generator=g).float() / 4          # {k / 4 : k = -3 .. 4}: exact in all three types
    return torch.relu(v) if gen_name == "relu_levels" else v


def operands(shape, dtype, g):
    """dy-like operand: randn rounded through the element type"""
    return torch.randn(shape, generator=g).to(dtype)


def mask_operand(shape, dtype, g):
    """about half non-positive entries, one in eight an exact zero"""
    m = torch.randn(shape, generator=g)
    m[torch.rand(shape, generator=g) < 0.125] = 0.0
    return m.to(dtype)


# ------------------------------------------------------------------------------------------------
# max pool
# ------------------------------------------------------------------------------------------------
def _window_views(t, case, fill):
    """yields (tap, view of the padded `t` holding that tap of every window)"""
    (kt, kh, kw), (st, sh, sw), (pt, ph, pw) = case.k, case.s, case.p
    N, T, H, W, C = t.shape
    To, Ho, Wo = out_dims(case)
    ext = [max(n + 2 * p, (o - 1) * s + k) for n, p, o, s, k in zip((T, H, W), case.p, (To, Ho, Wo), case.s, case.k)]
    padded = torch.full((N, ext[0], ext[1], ext[2], C), fill, dtype=t.dtype)
    padded[:, pt:pt + T, ph:ph + H, pw:pw + W] = t
    for a, b, c in itertools.product(range(kt), range(kh), range(kw)):
        yield (a * kh + b) * kw + c, padded[:, a:a + (To - 1) * st + 1:st, b:b + (Ho - 1) * sh + 1:sh, c:c + (Wo - 1) * sw + 1:sw]


def max_fwd(x, case, last=False, lo=None):
    """(y, tap) of the first maximum (last=True: of the LAST maximum, the variant the tie conditions must tell apart).
    x: values in any float type; with `lo` the two fp16 planes (x = hi): returns ((y_hi, y_lo), tap)."""
    v = x.float() if lo is None else x.float() + lo.float()
    To, Ho, Wo = out_dims(case)
    shape = (x.shape[0], To, Ho, Wo, x.shape[4])
    best = torch.full(shape, float("-inf"))
    tap = torch.zeros(shape, dtype=torch.int64)
    if lo is None:
        for t, w in _window_views(v, case, float("-inf")):
            m = ((w >= best) & (w > float("-inf"))) if last else (w > best)
            best = torch.where(m, w, best)
            tap = torch.where(m, torch.full_like(tap, t), tap)
        return best.to(x.dtype), tap
    sel_h, sel_l = torch.zeros(shape, dtype=x.dtype), torch.zeros(shape, dtype=x.dtype)
    for (t, w), (_, wh), (_, wl) in zip(_window_views(v, case, float("-inf")), _window_views(x, case, 0.0), _window_views(lo, case, 0.0)):
        m = w > best
        best = torch.where(m, w, best)
        tap = torch.where(m, torch.full_like(tap, t), tap)
        sel_h, sel_l = torch.where(m, wh, sel_h), torch.where(m, wl, sel_l)
    return (sel_h, sel_l), tap


def max_bwd(case, tap, dy, y=None, add=None, mask=None):
    """the fp32-ordered emulation of the module docstring; returns dx in dy's element type"""
    (kt, kh, kw), (st, sh, sw), (pt, ph, pw) = case.k, case.s, case.p
    N, T, H, W = case.shape
    C = dy.shape[4]
    To, Ho, Wo = out_dims(case)
    g = dy.float()
    if y is not None:
        g = torch.where(y.float() > 0, g, torch.zeros_like(g))
    ext = [max(n + 2 * p, (o - 1) * s + k) for n, p, o, s, k in zip((T, H, W), case.p, (To, Ho, Wo), case.s, case.k)]
    acc = torch.zeros((N, ext[0], ext[1], ext[2], C), dtype=torch.float32)
    zero = torch.zeros_like(g)
    for a, b, c in itertools.product(reversed(range(kt)), reversed(range(kh)), reversed(range(kw))):
        view = acc[:, a:a + (To - 1) * st + 1:st, b:b + (Ho - 1) * sh + 1:sh, c:c + (Wo - 1) * sw + 1:sw]
        view.add_(torch.where(tap == (a * kh + b) * kw + c, g, zero))
    acc = acc[:, pt:pt + T, ph:ph + H, pw:pw + W].contiguous()
    if add is not None:
        acc = acc + add.float()
    if mask is not None:
        acc = torch.where(mask.float() > 0, acc, torch.zeros_like(acc))
    return acc.to(dy.dtype)


def covered(case):
    """bool (T, H, W): the input positions some window covers"""
    axes = [torch.tensor([any(0 <= i + p - o * s < k for o in range(no)) for i in range(n)])
            for n, no, k, s, p in zip(case.shape[1:], out_dims(case), case.k, case.s, case.p)]
    return axes[0][:, None, None] & axes[1][None, :, None] & axes[2][None, None, :]


MaxData = collections.namedtuple("MaxData", "x y tap dy add mask")


@functools.lru_cache(maxsize=None)
def max_data(case_name, dtype_name, gen_name):
    """inputs and forward reference of one (case, dtype, generator), computed once and shared"""
    case = MAX_BY_NAME[case_name]
    dtype = DTYPES[dtype_name]
    g = _gen(case_name, dtype_name, gen_name)
    N, T, H, W = case.shape
    x = values(gen_name, (N, T, H, W, case.C), dtype, g).to(dtype)
    y, tap = max_fwd(x, case)
    oshape = (N,) + out_dims(case) + (case.C,)
    return MaxData(x, y, tap, operands(oshape, dtype, g), operands(x.shape, dtype, g), mask_operand(x.shape, dtype, g))


def max_bwd_combo(case, d, combo):
    """the reference dx of one operand combination"""
    if combo == "relu":
        return max_bwd(case, d.tap, d.dy, y=d.y)
    return max_bwd(case, d.tap, d.dy, add=d.add if combo in ("add", "add_mask", "alias") else None,
                   mask=d.mask if combo in ("mask", "add_mask") else None)


def pair_split(v):
    """the canonical two fp16 planes of fp32 values (vlfb_pair_split): hi = fp16(v), lo = fp16(v - hi)"""
    hi = v.to(torch.float16)
    return hi, (v - hi.float()).to(torch.float16)


def tie_stats(case, x):
    """fractions of windows: with an exact tie for the maximum and y > 0; whose first maximum is not tap 0"""
    v = x.float()
    y, tap = max_fwd(x, case)
    n_eq = torch.zeros(y.shape)
    for _, w in _window_views(v, case, float("-inf")):
        n_eq += (w == y.float()).float()
    tied = (n_eq >= 2) & (y.float() > 0)
    return {"tied_pos": tied.float().mean().item(), "not_tap0": (tap != 0).float().mean().item()}


def bits(t):
    """the storage bits of a tensor, for bit-for-bit comparisons (torch.equal calls -0 and +0 equal)"""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ------------------------------------------------------------------------------------------------
# average pool (pad 0)
# ------------------------------------------------------------------------------------------------
AvgCase = collections.namedtuple("AvgCase", "name k s shape C is_global one_window")
AVG_CASES = [
    AvgCase("win_overlap", (2, 3, 3), (1, 2, 2), (2, 3, 7, 9), 24, False, False),     # windows overlap in t, h and w; strides > 1
    AvgCase("temporal", (4, 1, 1), (1, 1, 1), (2, 4, 3, 3), 72, False, True),         # head_helper.py:92-98
    AvgCase("global_9rows", (1, 3, 3), (1, 1, 1), (3, 1, 3, 3), 72, True, True),      # fewer rows than the 32 row lanes; idle chunk lanes
    AvgCase("global_196rows", (4, 7, 7), (1, 1, 1), (1, 4, 7, 7), 8, True, True),     # head_helper.py:37-40
]
AVG_COMBOS = ("none", "add", "mask", "add_mask")


def ulp(ref, dtype_name):
    """spacing of `dtype` at |ref| (fp64 tensor), the subnormal spacing below the normal range"""
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -1000))).clamp_min(EMIN[dtype_name])
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - MANT[dtype_name])


def avg_fwd(x, case, lo=None):
    """(fp64 mean, bound): x in any float type; with `lo`, the mean of hi + lo and an fp32 output"""
    window = case.k[0] * case.k[1] * case.k[2]
    geo = MaxCase(case.name, case.k, case.s, (0, 0, 0), case.shape, case.C, None, None)
    mean = sabs = 0
    for (_, w), (_, wl) in zip(_window_views(x.double(), geo, 0.0), _window_views((x if lo is None else lo).double(), geo, 0.0)):
        mean = mean + w + (wl if lo is not None else 0)
        sabs = sabs + w.abs() + (wl.abs() if lo is not None else 0)
    n = window * (2 if lo is not None else 1)
    return mean / window, (n + 1) * U32 * sabs / window


def avg_fwd_emulated(x, case, lo=None):
    """the fp32-ordered emulation of the module docstring: sequential fp32 tensor adds.  x in any float type -> that type; with
    `lo`, the two fp16 planes -> fp32"""
    window = case.k[0] * case.k[1] * case.k[2]
    geo = MaxCase(case.name, case.k, case.s, (0, 0, 0), case.shape, case.C, None, None)
    v = x.float() if lo is None else x.float() + lo.float()
    if case.is_global:
        N, C = v.shape[0], v.shape[4]
        rows = v.reshape(N, -1, C)
        lanes = torch.zeros((N, 32, C), dtype=torch.float32)
        for r in range(rows.shape[1]):
            lanes[:, r % 32] += rows[:, r]
        acc = torch.zeros((N, C), dtype=torch.float32)
        for j in range(32):
            acc = acc + lanes[:, j]
        acc = acc.reshape(N, 1, 1, 1, C)
    else:
        acc = torch.zeros((v.shape[0],) + out_dims(geo) + (v.shape[4],), dtype=torch.float32)
        for _, w in _window_views(v, geo, 0.0):                           # (taps in ascending (a, b, c) order)
            acc = acc + w
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(window), dtype=torch.float32)
    return (acc * inv).to(x.dtype if lo is None else torch.float32)


def avg_bwd(case, dy, add=None, mask=None):
    """(fp64 dx, bound without the output rounding)"""
    window = case.k[0] * case.k[1] * case.k[2]
    geo = MaxCase(case.name, case.k, case.s, (0, 0, 0), case.shape, case.C, None, None)
    To, Ho, Wo = out_dims(geo)
    N, T, H, W = case.shape
    acc = torch.zeros((N, T, H, W, dy.shape[4]), dtype=torch.float64)
    sabs, cnt = torch.zeros_like(acc), torch.zeros_like(acc)
    g = dy.double() / window
    for a, b, c in itertools.product(range(case.k[0]), range(case.k[1]), range(case.k[2])):
        sl = (slice(None), slice(a, a + (To - 1) * case.s[0] + 1, case.s[0]), slice(b, b + (Ho - 1) * case.s[1] + 1, case.s[1]),
              slice(c, c + (Wo - 1) * case.s[2] + 1, case.s[2]))
        acc[sl] += g
        sabs[sl] += g.abs()
        cnt[sl] += 1
    if add is not None:
        acc, sabs, cnt = acc + add.double(), sabs + add.double().abs(), cnt + 1
    bound = (cnt + 1) * U32 * sabs
    if mask is not None:
        keep = mask.double() > 0
        acc, bound = torch.where(keep, acc, torch.zeros_like(acc)), torch.where(keep, bound, torch.zeros_like(bound))
    return acc, bound


def avg_bwd_one_window(case, dy32, dtype, mask=None):
    """where every input position lies in exactly one window the backward is ONE product, fl32(dy * fl32(1 / window)), and
    the two-term form hi = round_T(v), lo = round_T(v - hi): (v fp32, hi, lo) bit for bit.  dy32: fp32 (N, To, Ho, Wo, C)"""
    assert case.one_window
    window = case.k[0] * case.k[1] * case.k[2]
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(window), dtype=torch.float32)
    N, T, H, W = case.shape
    v = (dy32 * inv).expand(N, T, H, W, dy32.shape[4]).contiguous()       # (To, Ho, Wo) are 1 or the input extent
    if mask is not None:
        v = torch.where(mask.float() > 0, v, torch.zeros_like(v))
    hi = v.to(dtype)
    return v, hi, (v - hi.float()).to(dtype)
