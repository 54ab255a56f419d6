"""Case tables, input generators, fp64 references and per-element error bounds shared by tests/test_attn_cases_host.py,
tests/test_attn_gpu.py and tests/test_fbo_attn_gpu.py: the fused non-local attention kernels (vlfb_attn_scores_fwd / _bwd,
csrc/vlfb_attn.hip) and the FBO attention core (vlfb_fbo_attn_fwd / _fwd_shared / _bwd, csrc/vlfb_head.hip).  CPU only;
imports no vlfb.

Notation: u = 2^-24 (unit roundoff of fp32), u_out = 2^-8 (bf16) / 2^-11 (fp16) / 0 (fp32 output), n = the length of a dot
product (Ci, or D), L = the number of keys (L2, or K).  Every accumulation step is allowed 2u instead of u: the matrix
cores' internal additions are not documented to round to nearest.  Nothing below is derived from a kernel's output.

Forward   P_k = exp(s_k - m) / sum_j exp(s_j - m),  s_k = scale <theta, phi_k>,  m = max_j s_j.
  logit    n products and n - 1 additions of the accumulator chain, one multiplication by scale: every term of the sum
           passes through at most n + 2 roundings of 2u, so |ds_k| <= 2 (n + 2) u A_k with A_k = scale sum_c |theta_c||phi_kc|.
           The row maximum carries the same error, so s_k - m is off by at most 2 * 2 (n + 2) u max_k A_k: the first term.
  exp      the subtraction rounds once and the argument reduction of exp (a multiplication by log2 e, or the fma of the
           queries-per-wave kernel) once more, both relative to |s_k - m|: |s_k - m| u on the exponent, i.e. on the relative
           error of exp.  exp itself, the reciprocal of the sum and the final product: 6 u.
  row sum  L additions of non-negative terms in any order: L u relative; the terms carry the exp error of their own rows,
           which the first term and 6 u already cover for the numerator -- the same again for the denominator: 2 L u
           together with the additions.
  =>  |dP_k| / P_k  <=  2 * 2 (n + 2) u max_k A_k + (|s_k - m| + 2 L + 6) u      (first order)
  output   a 16-bit output rounds once more: u_out |ref|, plus 2^-25 for fp16 (half the smallest fp16 subnormal, as in
           roi_cases.py).  bf16 and fp32 share the exponent range of the fp32 arithmetic; a value under 2^-126 may be flushed
           by it, so every bound carries TINY = 2^-126 (the smallest normal number of fp32 and of bf16).

Backward  dS_k = scale P_k (dP_k - dot),  dP_k = <dY, g_k>,  dot = sum_j dP_j P_j,  with P the probabilities the kernel
  itself wrote (read back: exact inputs of the backward kernel).
  dP_k     as a logit without the scale: a term passes through its product and at most n - 1 additions, n roundings of 2u:
           2 n u B_k with B_k = sum_c |dY_c||g_kc|
  dot      inherits sum_j P_j 2 n u B_j, and its own L products and L additions: 2 (L + 1) u sum_j |dP_j| P_j
  dS_k     the subtraction and two multiplications, relative to |dP_k| + |dot|: 6 u
  =>  |d(dS_k)|  <=  scale P_k [2 n u B_k + sum_j P_j 2 n u B_j + 2 (L + 1) u sum_j |dP_j| P_j + 6 u (|dP_k| + |dot|)]
  plus the same output term.

FBO core (fp32 probabilities; theta [R][D], phi / g [R][K][ld] with ld >= D):
  p        the forward formula with n = D, L = K, no output rounding (fp32).
  t        t_d = sum_k p_k g_kd: K products and K additions, (K + 2) 2u sum_k |p_k||g_kd|, plus the error of the weights
           sum_k pbound_k |g_kd|, plus the output term.
  ds_ws    the backward formula with n = D, L = K on the kernel's own p, fp32: no output term.
  dtheta   (K + 2) 2u sum_k |ds_k||phi_kd| + sum_k dsbound_k |phi_kd| + output term.
  dphi     ds_k theta_d: one product, 2u |ds_k||theta_d| + dsbound_k |theta_d| + output term.
  dg       p_k dt_d with the kernel's own p: 2u |p_k||dt_d| + output term.
"""
import functools

import torch

U32 = 2.0 ** -24
TINY = 2.0 ** -126
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
U_OUT = {"fp32": 0.0, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}


def q(t, dtype):
    """round a fp32 CPU tensor through `dtype` (gpu_util.q; restated so that this module imports no vlfb)"""
    return t.to(dtype).to(torch.float32)


def out_term(ref, dtype_name):
    """the rounding of an output of this type: u_out |ref| (+ 2^-25 for fp16) + TINY"""
    t = U_OUT[dtype_name] * ref.abs() + TINY
    return t + 2.0 ** -25 if dtype_name == "fp16" else t


# ------------------------------------------------------------------------------------------------ fused scores
def fused_kernel(L2, Ci):
    """the kernel run_attn (csrc/vlfb_attn.hip) launches for this shape"""
    if (L2, Ci) == (784, 256):
        return "qrows"
    return "rows8" if L2 > 896 else "rows7"


def fused_supported(dtype_name, L1, L2, Ci):
    """supported() of csrc/vlfb_attn.hip"""
    return (dtype_name in ("bf16", "fp16") and 512 <= L2 <= 1024 and L2 % 8 == 0 and Ci % 64 == 0 and 64 <= Ci <= 1024
            and L1 >= 64 and L1 * Ci < 2 ** 30 and L1 * L2 < 2 ** 30)


def fused_lds(L2, Ci):
    """(bytes of the 64 x Ci query tile, bytes of the probability tile) of the rows kernels; red[] starts at the end of the
    probability tile, the workgroup's LDS ends 2 KiB behind the larger of the two"""
    fn = 8 if L2 > 896 else 7
    return 64 * Ci * 2, 64 * (8 * 16 * fn * 2 + 16)


#              (B, L1, L2, Ci)
FUSED_SHAPES = [
    (1, 64, 784, 256),      # qrows: waves 4..7 own no query
    (1, 72, 784, 256),      # qrows: a wave with 8 live rows
    (2, 129, 784, 256),     # qrows: batch stride, second workgroup with one row
    (1, 200, 784, 256),     # qrows
    (1, 64, 512, 64),       # rows7: lower key edge, waves 5..7 all padding
    (2, 65, 520, 128),      # rows7: L2 % 16 == 8
    (1, 127, 784, 512),     # rows7 on the model's key count
    (1, 64, 784, 1024),     # rows7: query tile larger than the probability tile (red[] inside the query region)
    (1, 100, 888, 192),     # rows7: ksteps = 6
    (1, 64, 896, 256),      # rows7: the last key of the last wave is live
    (1, 72, 904, 128),      # rows8: first shape above the FN switch
    (1, 64, 1016, 64),      # rows8: ragged last fragment
    (2, 129, 1024, 256),    # rows8: the test-crop shape
    (1, 64, 1024, 1024),    # rows8: red[] 1 KiB behind the query tile
]
FUSED_CASES = [(fused_kernel(s[2], s[3]),) + s for s in FUSED_SHAPES]
FUSED_GENERATORS = ("randn", "hot", "flat", "edge_peak")
FUSED_DTYPES = ("bf16", "fp16")
ENGINE_SCALE_SHAPES = [(1, 200, 784, 256), (2, 129, 1024, 256)]
COMPOSED_SHAPES = [(1, 72, 784, 256), (2, 65, 520, 128), (1, 72, 904, 128)]
PEAK = 6.0               # edge_peak: query = PEAK * key


def case_id(shape):
    return "x".join(str(v) for v in shape)


def engine_ds_scale(L2):
    """the factor the engine stores fp16 dS with (vlfb/engine.py: ds_scale of a non-local block)"""
    return float(16 << max(L2 - 1, 1).bit_length())


def edge_keys(L2, Ci):
    """keys at the edges of the ownership maps: fragment and wave boundaries of the rows kernels, the two staging halves
    (HALF = 400) of the queries-per-wave kernel"""
    fn = 8 if L2 > 896 else 7
    return [min(k, L2 - 1) for k in (0, 15, 16, 16 * fn - 1, 16 * fn, 399, 400, L2 - 4, L2 - 1)]


def edge_key_of_row(row, L2, Ci):
    ks = edge_keys(L2, Ci)
    return ks[row % len(ks)]


def ownership(kernel, qrow, key):
    """where element (qrow, key) of a batch entry is computed: a description for failure reports"""
    if kernel == "qrows":
        return "workgroup %d wave %d query lane %d, fragment %d lane group %d, staging half %d" % (
            qrow // 128, (qrow % 128) // 16, qrow % 16, key // 16, (key % 16) // 4, key // 400)
    fn = 7 if kernel == "rows7" else 8
    return "workgroup %d wave %d fragment %d lane group %d, query fragment %d lane %d" % (
        qrow // 64, key // (16 * fn), (key % (16 * fn)) // 16, (key % 16) // 4, (qrow % 64) // 16, qrow % 16)


@functools.lru_cache(maxsize=None)
def fused_inputs(shape, gen, dtype_name):
    """theta (B, L1, Ci), phi (B, L2, Ci), dY (B, L1, Ci), g (B, L2, Ci): fp32 CPU tensors holding values of the type"""
    B, L1, L2, Ci = shape
    dtype = DTYPES[dtype_name]
    rng = torch.Generator().manual_seed(L1 * 7 + L2 * 3 + Ci + 1000 * FUSED_GENERATORS.index(gen))
    theta = torch.randn(B, L1, Ci, generator=rng)
    phi = torch.randn(B, L2, Ci, generator=rng)
    if gen == "hot":
        theta, phi = theta * 3, phi * 3
    elif gen == "flat":
        # multiples of 1/8 in [-4, 4]: every product and every partial sum is exact in fp32 and fp64 in any order, so all
        # logits of a row are the same number whatever the summation order of kernel or reference
        theta = (theta * 8).round().clamp(-32, 32) / 8
        phi = ((phi[:, :1] * 8).round().clamp(-32, 32) / 8).expand(B, L2, Ci).contiguous()
    elif gen == "edge_peak":
        rows = torch.arange(L1)
        keys = torch.tensor([edge_key_of_row(int(r), L2, Ci) for r in rows])
        theta = PEAK * q(phi, dtype)[:, keys, :]
    else:
        assert gen == "randn"
    dY = torch.randn(B, L1, Ci, generator=rng)
    g = torch.randn(B, L2, Ci, generator=rng)
    return tuple(q(t, dtype).contiguous() for t in (theta, phi, dY, g))


def softmax_bound(x, y, scale, L, n):
    """fp64 reference of softmax(scale x y^T) over the last axis and its arithmetic bound (see the module docstring).
    x: (..., rows, n), y: (..., L, n) fp32 -> (P, bound), fp64"""
    xd, yd = x.double(), y.double()
    s = scale * torch.matmul(xd, yd.transpose(-1, -2))
    a = scale * torch.matmul(xd.abs(), yd.abs().transpose(-1, -2))
    m = s.max(dim=-1, keepdim=True).values
    p = torch.softmax(s, dim=-1)
    rel = 2 * 2 * (n + 2) * U32 * a.max(dim=-1, keepdim=True).values + ((s - m).abs() + 2 * L + 6) * U32
    return p, p * rel


def softmax_bwd_bound(dy, g, p, scale, L, n):
    """fp64 dS = scale p o (dP - <dP, p>) for the given probabilities, and its arithmetic bound.  p: fp64"""
    dyd, gd = dy.double(), g.double()
    dp = torch.matmul(dyd, gd.transpose(-1, -2))
    b = torch.matmul(dyd.abs(), gd.abs().transpose(-1, -2))
    dot = (dp * p).sum(dim=-1, keepdim=True)
    want = scale * p * (dp - dot)
    bound = scale * p * (2 * n * U32 * b + (p * 2 * n * U32 * b).sum(dim=-1, keepdim=True) +
                         2 * (L + 1) * U32 * (dp.abs() * p).sum(dim=-1, keepdim=True) + 6 * U32 * (dp.abs() + dot.abs()))
    return want, bound


@functools.lru_cache(maxsize=None)
def fused_forward_ref(shape, gen, dtype_name):
    """(P fp64, bound fp64 with the output term) of a fused-scores case at scale = Ci^-0.5"""
    B, L1, L2, Ci = shape
    theta, phi, _, _ = fused_inputs(shape, gen, dtype_name)
    p, bound = softmax_bound(theta, phi, Ci ** -0.5, L2, Ci)
    return p, bound + out_term(p, dtype_name)


def fused_backward_ref(shape, gen, dtype_name, p_kernel, scale):
    """(dS fp64, bound) for the probabilities the kernel wrote (any float tensor of values of the type)"""
    B, L1, L2, Ci = shape
    _, _, dY, g = fused_inputs(shape, gen, dtype_name)
    want, bound = softmax_bwd_bound(dY, g, p_kernel.double(), scale, L2, Ci)
    return want, bound + out_term(want, dtype_name)


def fused_emulation(shape, gen, dtype_name, bwd_scale=None):
    """the kernels' formulas in torch fp32 on the CPU, rounded to the type: (P, dS) as fp32 tensors"""
    B, L1, L2, Ci = shape
    dtype = DTYPES[dtype_name]
    theta, phi, dY, g = fused_inputs(shape, gen, dtype_name)
    scale = Ci ** -0.5
    p = q(torch.softmax(torch.bmm(theta, phi.transpose(1, 2)) * scale, dim=2), dtype)
    bs = scale if bwd_scale is None else bwd_scale
    dp = torch.bmm(dY, g.transpose(1, 2))
    ds = q(torch.tensor(bs, dtype=torch.float32) * p * (dp - (dp * p).sum(dim=2, keepdim=True)), dtype)
    return p, ds


def worst(err, bound):
    """(largest err / bound over the elements with bound > 0, flat index of it); err == 0 where bound == 0 is required"""
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    i = int(ratio.argmax())
    return float(ratio.flatten()[i]), i


# ------------------------------------------------------------------------------------------------ FBO core
#            (R, K, D, ld)
FBO_SHAPES = [(1, 1, 64, 64), (3, 7, 64, 80), (2, 31, 512, 512), (5, 33, 512, 576), (4, 300, 512, 520), (3, 300, 40, 48),
              (2, 12, 40, 40), (7, 300, 128, 136)]
FBO_GENERATORS = ("randn", "hot")
FBO_VEC = {"fp32": 4, "bf16": 8, "fp16": 8}
PAD = 7.0                                        # what the ld - D padding columns of phi / g hold
# shared banks: NB banks, the owner column is column 0 of an [R][5] RoI table; not sorted, bank 1 has a single reader
SHARED_NB = 3
SHARED_OWNER = (0, 0, 2, 1, 2, 2, 0)
SHARED_SHAPES = [(7, 33, 128, 136), (7, 12, 40, 48)]


def fbo_path(dtype_name, D, ld):
    """the kernels vlfb_fbo_attn_fwd / _bwd (csrc/vlfb_head.hip) pick: "chip" = dot / mix / row fix-up, "row" = one workgroup
    per row.  (The backward requires D % v == 0 and ld % v == 0 of every shape.)"""
    v = FBO_VEC[dtype_name]
    return "chip" if D % (8 * v) == 0 and ld % v == 0 else "row"


FBO_CASES = [(fbo_path(name, s[2], s[3]), name) + s for name in DTYPES for s in FBO_SHAPES]


@functools.lru_cache(maxsize=None)
def fbo_inputs(shape, gen, dtype_name, banks=None):
    """theta (R, D), phi (NB, K, D), g (NB, K, D), dt (R, D) as fp32 CPU tensors of values of the type; NB = R unless
    `banks` is given"""
    R, K, D, ld = shape
    dtype = DTYPES[dtype_name]
    nb = R if banks is None else banks
    rng = torch.Generator().manual_seed(R * 1000 + K * 7 + D + ld + 100000 * FBO_GENERATORS.index(gen))
    theta = torch.randn(R, D, generator=rng)
    phi = torch.randn(nb, K, D, generator=rng)
    if gen == "hot":
        theta, phi = theta * 3, phi * 3
    else:
        assert gen == "randn"
    g = torch.randn(nb, K, D, generator=rng)
    dt = torch.randn(R, D, generator=rng)
    return tuple(q(t, dtype).contiguous() for t in (theta, phi, g, dt))


def fbo_forward_from(theta, phi, g, dtype_name):
    """(p, pbound, t, tbound) fp64 for theta (R, D) and per-row banks phi, g (R, K, D)"""
    R, K, D = phi.shape
    p, pb = softmax_bound(theta.unsqueeze(1), phi, D ** -0.5, K, D)
    p, pb = p.squeeze(1), pb.squeeze(1) + TINY
    gd = g.double()
    t = torch.einsum("rk,rkd->rd", p, gd)
    tb = (K + 2) * 2 * U32 * torch.einsum("rk,rkd->rd", p, gd.abs()) + torch.einsum("rk,rkd->rd", pb, gd.abs())
    return p, pb, t, tb + out_term(t, dtype_name)


@functools.lru_cache(maxsize=None)
def fbo_forward_ref(shape, gen, dtype_name):
    theta, phi, g, _ = fbo_inputs(shape, gen, dtype_name)
    return fbo_forward_from(theta, phi, g, dtype_name)


@functools.lru_cache(maxsize=None)
def fbo_shared_ref(shape, gen, dtype_name):
    theta, phi, g, _ = fbo_inputs(shape, gen, dtype_name, SHARED_NB)
    own = torch.tensor(SHARED_OWNER)
    return fbo_forward_from(theta, phi[own], g[own], dtype_name)


def fbo_backward_ref(shape, gen, dtype_name, p_kernel):
    """references and bounds of the backward on the probabilities the kernel wrote: a dict name -> (want, bound), fp64, with
    dphi / dg as (R, K, D)"""
    R, K, D, ld = shape
    theta, phi, g, dt = fbo_inputs(shape, gen, dtype_name)
    scale = D ** -0.5
    p = p_kernel.double()
    ds, dsb = softmax_bwd_bound(dt.unsqueeze(1), g, p.unsqueeze(1), scale, K, D)
    ds, dsb = ds.squeeze(1), dsb.squeeze(1) + TINY
    phd, thd, dtd = phi.double(), theta.double(), dt.double()
    dth = torch.einsum("rk,rkd->rd", ds, phd)
    dthb = (K + 2) * 2 * U32 * torch.einsum("rk,rkd->rd", ds.abs(), phd.abs()) + torch.einsum("rk,rkd->rd", dsb, phd.abs())
    dphi = ds.unsqueeze(2) * thd.unsqueeze(1)
    dphib = (2 * U32 * ds.abs() + dsb).unsqueeze(2) * thd.abs().unsqueeze(1)
    dg = p.unsqueeze(2) * dtd.unsqueeze(1)
    dgb = 2 * U32 * dg.abs()
    return {"ds_ws": (ds, dsb), "dtheta": (dth, dthb + out_term(dth, dtype_name)),
            "dphi": (dphi, dphib + out_term(dphi, dtype_name)), "dg": (dg, dgb + out_term(dg, dtype_name))}


def fbo_emulation(shape, gen, dtype_name):
    """the kernels' formulas in torch fp32 on the CPU: p (fp32), t, and the backward on that p, outputs rounded to the type"""
    R, K, D, ld = shape
    dtype = DTYPES[dtype_name]
    theta, phi, g, dt = fbo_inputs(shape, gen, dtype_name)
    scale = torch.tensor(D ** -0.5, dtype=torch.float32)
    p = torch.softmax(torch.einsum("rd,rkd->rk", theta, phi) * scale, dim=1)
    t = q(torch.einsum("rk,rkd->rd", p, g), dtype)
    dp = torch.einsum("rd,rkd->rk", dt, g)
    ds = scale * p * (dp - (dp * p).sum(dim=1, keepdim=True))
    return {"p": p, "t": t, "ds_ws": ds, "dtheta": q(torch.einsum("rk,rkd->rd", ds, phi), dtype),
            "dphi": q(ds.unsqueeze(2) * theta.unsqueeze(1), dtype), "dg": q(p.unsqueeze(2) * dt.unsqueeze(1), dtype)}
