"""fp64 model of a vlfb_conv_desc launch (include/vlfb.h, "Implicit-GEMM 3-D convolution family"): the executable form of
what a descriptor means.

`Case(desc, ops)` allocates random operands in the layout the descriptor implies (seeded, values in a chosen range), every
device input with slack past its extent so that a sizing mistake here reads padding instead of faulting the card, and
computes the expected outputs in float64 on the CPU.  `ops` names the optional operands of the launch ("bias", "R", "R_lo",
"mask", "rowscale", "O_lo", "O_planes", "dbias", "class0_inplace").  `Case.run()` launches the descriptor through
vlfb_conv_run and `Case.check()` compares every output with the model:
  * every output element the launch must write is NaN before the launch and must be finite after it;
  * every element around and between the rows of an output (guard bands, ldo > Cn gaps) holds a sentinel that must survive;
  * the workspace is exactly the vlfb_conv_workspace_bytes of the descriptor, NaN-filled, between two sentinel bands that
    must survive: a slab write past the stated size shows in the bands, a slab element read but never written in the output;
  * relative L2 at the bars of the kernel tests, and an elementwise bound
        |got - ref| <= c * (u_prod + u_acc(K)) * |alpha| (|A|.|B|)  +  u_out * (|alpha| |A|.|B| + |bias| + |R|)
    tight enough that one dropped 32-wide k-tile of one output tile fails it.

The gather is written per tap with explicit index arithmetic (F.conv3d cannot express dilation 0, the doubled-tap form of
the two-term DGRAD weights).  Term planes (two fp16 planes of F16X3, bf16 planes of the split maths, the interleaved two-term
weights of F16W2) are made here with the formulas vlfb_weight_prep / vlfb_pair_split / vlfb_split_planes implement (pinned
bit-exactly by tests/test_pair_gpu.py and tests/test_split_gpu.py); the model uses the exact sum of the planes it stores, so
what it checks is the contraction, not the split.  A field combination the model does not cover raises `Unmodelled`.
"""
import math

import torch

F32, BF16, F16 = 0, 1, 2
FPROP, DGRAD, WGRAD = 0, 1, 2
BIAS_NONE, BIAS_COL, BIAS_ROW = 0, 1, 2
MATH_NATIVE, MATH_BF16X3, MATH_BF16X6, MATH_F16W2, MATH_F16X3 = 0, 3, 6, 12, 13
ALGO_CLASS0 = 5
TDT = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
UNIT = {F32: 2.0 ** -24, BF16: 2.0 ** -8, F16: 2.0 ** -11}

SLACK = 256          # elements of slack past the extent of every device input
GUARD = 64           # sentinel elements before and after every output
SENTINEL = -12288.0  # exactly representable in fp32 / fp16 / bf16

# relative-L2 bars (tests/gpu_util.TOL for the plain dtypes; tests/test_pair_gpu.py, tests/test_split_gpu.py and
# tests/test_w2i_gpu.py for the two-plane / split / two-term forms)
L2_BAR = {"f32": 2e-5, "bf16": 1e-2, "f16": 1.5e-3, "f16x3": 1.5e-6, "bf16x3": 4e-5, "bf16x6": 2e-6, "w2_f32": 2e-6,
          "w2_f16": 4e-4, "w2_pair": 3e-6}


class Unmodelled(NotImplementedError):
    pass


FIELDS = ("mode", "dtype", "out_dtype", "N", "Tr", "Hr", "Wr", "Ts", "Hs", "Ws", "Cs", "kt", "kh", "kw", "st", "sh", "sw",
          "pt", "ph", "pw", "dt", "dh", "dw", "pack_w", "Cn", "lda", "ldb", "ldo", "ldr", "ldp", "batch", "a_bstride",
          "b_bstride", "o_bstride", "r_bstride", "p_bstride", "alpha", "relu", "bias_mode", "accumulate", "splits", "algo",
          "math", "b_pstride", "a_planes", "p_planes", "o_planes", "wgrad_bias", "a_pstride", "p_pstride", "o_pstride")


def desc_dict(d):
    return {f: getattr(d, f) for f in FIELDS}


def rnd16(x, dt):
    return x.to(TDT[dt]).to(torch.float64)


def bf16_terms(x, n):
    """n bf16 terms of fp32 values: h = bf16(x), m = bf16(x - h), l = bf16(x - h - m) (vlfb_split_planes)"""
    out, r = [], x.float()
    for _ in range(n):
        t = r.to(torch.bfloat16)
        out.append(t)
        r = r - t.float()
    return out


def f16_pair(x):
    """hi = fp16(x), lo = fp16(x - hi) (vlfb_pair_split)"""
    hi = x.float().half()
    return hi, (x.float() - hi.float()).half()


def w2i_rows(v, tdt=torch.float16):
    """the two-term weight rows of VLFB_MATH_F16W2 (vlfb_weight_prep VLFB_MIX_W2I): fp32 values v [rows][K] (K a multiple of
    64) -> ([rows][2K] of `tdt`, laid out [K / 64][term][64] per row, with hi = T(v), lo = T(v - hi); fp64 value hi + lo)"""
    v = v.float()
    hi = v.to(tdt)
    lo = (v - hi.float()).to(tdt)
    rows, K = v.shape
    t = torch.stack([hi.view(rows, K // 64, 64), lo.view(rows, K // 64, 64)], 2).reshape(rows, 2 * K)
    return t, hi.double() + lo.double()


class Geometry:
    """row space, gather source and K of a descriptor (the defaults of vlfb_conv_desc resolved)"""

    def __init__(self, d):
        self.d = d
        self.batch = max(d["batch"], 1)
        self.M = d["N"] * d["Tr"] * d["Hr"] * d["Wr"]
        self.S = d["N"] * d["Ts"] * d["Hs"] * d["Ws"]
        if d["pack_w"]:
            if d["Cs"] != 4 or d["dw"] != 1 or d["mode"] == DGRAD:
                raise Unmodelled("pack_w needs Cs 4, dw 1, no DGRAD")
            self.kw, self.cpt = d["pack_w"], 4          # kw_pad taps of 4 channels, packed into the contiguous K axis
        else:
            self.kw, self.cpt = d["kw"], d["Cs"]
        self.taps = d["kt"] * d["kh"] * self.kw
        self.K = self.taps * self.cpt
        self.w2i = d["math"] == MATH_F16W2
        self.lda = d["lda"] or d["Cs"]
        self.ldb = d["ldb"] or (2 * self.K if self.w2i else self.K)
        self.ldp = d["ldp"] or d["Cn"]
        self.ldo = d["ldo"] or (self.K if d["mode"] == WGRAD else d["Cn"])
        self.ldr = d["ldr"] or self.ldo
        self.ident = (not d["pack_w"] and self.taps == 1 and (d["st"], d["sh"], d["sw"], d["pt"], d["ph"], d["pw"]) == (1, 1, 1, 0, 0, 0)
                      and (d["Ts"], d["Hs"], d["Ws"]) == (d["Tr"], d["Hr"], d["Wr"]))
        if self.batch > 1 and not self.ident:
            raise Unmodelled("batched launches are plain GEMMs")
        # output shape [batch][rows][cols]
        self.orows, self.ocols = (d["Cn"], self.K) if d["mode"] == WGRAD else (self.M, d["Cn"])

    def live_taps(self):
        """taps (a, b, c) that read data for at least one row: per axis, a tap is live when some row position of that axis
        maps it inside the source; rows enumerate the whole (N, T, H, W) grid, so a tap is live when it is live on every axis"""
        d = self.d
        n = 1
        for ax, k, s_, p, dl in (("T", d["kt"], d["st"], d["pt"], d["dt"]), ("H", d["kh"], d["sh"], d["ph"], d["dh"]),
                                 ("W", self.kw, d["sw"], d["pw"], 1 if d["pack_w"] else d["dw"])):
            pos = torch.arange(d[ax + "r"]).view(-1, 1)
            tap = torch.arange(k).view(1, -1)
            ext = d[ax + "s"]
            if d["mode"] == DGRAD:
                num = pos + p - tap * dl
                q = torch.div(num, s_, rounding_mode="floor")
                ok = (num - q * s_ == 0) & (q >= 0) & (q < ext)
            else:
                q = pos * s_ - p + tap * dl
                ok = (q >= 0) & (q < ext)
            n *= int(ok.any(0).sum())
        return n

    def gather_index(self):
        """[M, taps] source position (row of A) of every (row, tap), -1 where the tap reads padding"""
        d = self.d
        m = torch.arange(self.M)
        w = m % d["Wr"]
        h = (m // d["Wr"]) % d["Hr"]
        t = (m // (d["Wr"] * d["Hr"])) % d["Tr"]
        n = m // (d["Wr"] * d["Hr"] * d["Tr"])
        a = torch.arange(d["kt"]).view(-1, 1, 1)
        b = torch.arange(d["kh"]).view(1, -1, 1)
        c = torch.arange(self.kw).view(1, 1, -1)
        a, b, c = [x.expand(d["kt"], d["kh"], self.kw).reshape(-1) for x in (a, b, c)]
        if d["pack_w"]:
            dil = (d["dt"], d["dh"], 1)
        else:
            dil = (d["dt"], d["dh"], d["dw"])

        def src(pos, tap, s, p, dl, ext):
            if d["mode"] == DGRAD:
                num = pos.view(-1, 1) + p - tap.view(1, -1) * dl
                q = torch.div(num, s, rounding_mode="floor")
                ok = (num - q * s == 0) & (q >= 0) & (q < ext)
                return q, ok
            q = pos.view(-1, 1) * s - p + tap.view(1, -1) * dl
            return q, (q >= 0) & (q < ext)

        st, ok_t = src(t, a, d["st"], d["pt"], dil[0], d["Ts"])
        sh, ok_h = src(h, b, d["sh"], d["ph"], dil[1], d["Hs"])
        sw, ok_w = src(w, c, d["sw"], d["pw"], dil[2], d["Ws"])
        if d["pack_w"] and not bool((ok_w | ~(ok_t & ok_h)).all()):
            raise Unmodelled("pack_w needs a W-padded source: every packed kw tap inside [0, Ws)")
        idx = ((n.view(-1, 1) * d["Ts"] + st) * d["Hs"] + sh) * d["Ws"] + sw
        return torch.where(ok_t & ok_h & ok_w, idx, torch.full_like(idx, -1))


class Case:
    """operands + fp64 expectation of one descriptor.  `d`: a hip.ConvDesc or a dict of its fields."""

    def __init__(self, d, ops=(), seed=0, scale=1.0):
        self.d = dict(d) if isinstance(d, dict) else desc_dict(d)
        d = self.d
        self.ops = set(ops)
        unknown = self.ops - {"bias", "R", "R_lo", "mask", "rowscale", "O_lo", "O_planes", "dbias", "class0_inplace"}
        if unknown:
            raise Unmodelled("operands %s" % sorted(unknown))
        self.g = g = Geometry(d)
        self.gen = torch.Generator().manual_seed(seed)
        self.scale = scale
        mode, dt, math_ = d["mode"], d["dtype"], d["math"]
        if math_ not in (MATH_NATIVE, MATH_BF16X3, MATH_BF16X6, MATH_F16X3, MATH_F16W2):
            raise Unmodelled("math %d" % math_)
        if (bool(d["accumulate"]) or bool(d["wgrad_bias"])) and mode != WGRAD:
            raise Unmodelled("accumulate / wgrad_bias outside WGRAD")
        if math_ == MATH_F16X3 and (mode != FPROP or dt != F16):
            raise Unmodelled("F16X3 is an fp16 FPROP")
        if math_ in (MATH_BF16X3, MATH_BF16X6) and dt != F32:
            raise Unmodelled("split maths take fp32 operands")
        if math_ == MATH_F16W2 and (mode != DGRAD or dt == F32 or d["Cs"] % 64):
            raise Unmodelled("F16W2 is a 16-bit DGRAD with Cs % 64 == 0")
        self.sp = {MATH_BF16X3: 2, MATH_BF16X6: 3}.get(math_, 0)
        # output form
        self.pair_out = d["out_dtype"] == F16 and (math_ == MATH_F16X3 or self.sp)     # O / O_lo are the two fp16 planes
        if self.pair_out and "O_lo" not in self.ops:
            raise Unmodelled("a two-plane output needs O_lo")
        if "class0_inplace" in self.ops and (d["algo"] != ALGO_CLASS0 or "R" not in self.ops or d["relu"] or "mask" in self.ops):
            raise Unmodelled("class0_inplace is the in-place accumulate of ALGO_CLASS0 (R = O, no relu / mask)")
        if mode == WGRAD and (self.ops & {"bias", "R", "R_lo", "mask", "O_lo", "O_planes"} or d["bias_mode"] or d["relu"]):
            raise Unmodelled("FPROP / DGRAD epilogue operands on a WGRAD")
        if mode != WGRAD and self.ops & {"rowscale", "dbias"}:
            raise Unmodelled("WGRAD epilogue operands on an FPROP / DGRAD")
        if (d["bias_mode"] != BIAS_NONE) != ("bias" in self.ops):
            raise Unmodelled("bias_mode and the bias operand go together")
        if ("dbias" in self.ops) != bool(d["wgrad_bias"]):
            raise Unmodelled("wgrad_bias and dbias go together")
        if (d["o_planes"] > 0) != ("O_planes" in self.ops):
            raise Unmodelled("o_planes and O_planes go together")
        if d["o_planes"] == 2 and not self.sp or d["o_planes"] not in (0, 1, 2):
            raise Unmodelled("o_planes %d" % d["o_planes"])
        if d["a_planes"] and not self.sp or d["p_planes"] and (mode != WGRAD or not d["a_planes"]):
            raise Unmodelled("a_planes / p_planes outside the split maths")
        self._make_inputs()
        self._expect()

    # ---------------------------------------------------------------- operands
    def _rand(self, *shape):
        return (torch.rand(*shape, generator=self.gen, dtype=torch.float64) * 2 - 1) * self.scale

    def _store(self, vals, dt):
        """values rounded to the storage type of dtype `dt` (fp64 tensor of what the device holds)"""
        return vals.float().double() if dt == F32 else rnd16(vals, dt)

    def _planed(self, vals, planes, kind):
        """(device planes list, exact fp64 value) of fp32 values split into term planes"""
        if kind == "f16x3":
            hi, lo = f16_pair(vals)
            return [hi, lo], hi.double() + lo.double()
        terms = bf16_terms(vals, planes)
        return terms, sum(t.double() for t in terms)

    def _make_inputs(self):
        d, g = self.d, self.g
        mode, dt, math_ = d["mode"], d["dtype"], d["math"]
        B = g.batch
        # A: [batch][source rows][lda]; the first Cs channels carry values (pack_w: 4 channels per position)
        a_bst = d["a_bstride"] if B > 1 else g.S * g.lda
        if B > 1 and a_bst < g.S * g.lda:
            raise Unmodelled("a_bstride smaller than one batch element")
        a_ext = (B - 1) * a_bst + g.S * g.lda
        va = torch.zeros(a_ext, dtype=torch.float64)
        live = torch.zeros(a_ext, dtype=torch.bool)
        for z in range(B):
            v = live[z * a_bst: z * a_bst + g.S * g.lda].view(g.S, g.lda)
            v[:, :d["Cs"]] = True
        va[live] = self._rand(int(live.sum()))
        self.a_val, self.A_dev = self._device_operand(va, mode_kind="A", pstride=d["a_pstride"], planes=d["a_planes"])
        self.a_bst = a_bst
        # B (FPROP / DGRAD): [batch][Cn][ldb]; F16W2: rows [tap][Cs / 64][term][64]
        if mode != WGRAD:
            b_bst = d["b_bstride"] if B > 1 else d["Cn"] * g.ldb
            b_ext = (B - 1) * b_bst + d["Cn"] * g.ldb
            vb = torch.zeros(b_ext, dtype=torch.float64)
            live = torch.zeros(b_ext, dtype=torch.bool)
            kcols = 2 * g.K if g.w2i else g.K
            for z in range(B):
                live[z * b_bst: z * b_bst + d["Cn"] * g.ldb].view(d["Cn"], g.ldb)[:, :kcols] = True
            # (weights carry the inverse of alpha, as the engine's do: 2^10 for the two-term copies of `mix`, so the outputs stay
            # O(1) and clear of the 2^-24 floor of a two-plane low term)
            alpha = abs(float(d["alpha"])) or 1.0
            vb[live] = self._rand(int(live.sum())) * (1.0 / (math.sqrt(g.K) * alpha))
            self.b_bst = b_bst
            if self.sp or math_ == MATH_F16X3:
                nb = self.sp or 2
                ps = d["b_pstride"] if d["b_pstride"] > 0 else B * (b_bst if B > 1 else d["Cn"] * g.ldb)
                if ps < b_ext:
                    raise Unmodelled("b_pstride overlaps the planes")
                planes, self.b_val = self._planed(vb.float(), nb, "f16x3" if math_ == MATH_F16X3 else "bf16")
                dev = torch.zeros((nb - 1) * ps + b_ext + SLACK, dtype=planes[0].dtype)
                for i, p in enumerate(planes):
                    dev[i * ps: i * ps + b_ext] = p
                self.B_dev = dev
            elif g.w2i:
                w = torch.zeros(b_ext, dtype=TDT[dt])
                v = torch.zeros(b_ext, dtype=torch.float64)
                for z in range(B):
                    blk = slice(z * b_bst, z * b_bst + d["Cn"] * g.ldb)
                    t, val = w2i_rows(vb[blk].view(d["Cn"], g.ldb)[:, :g.K], TDT[dt])
                    w[blk].view(d["Cn"], g.ldb)[:, :2 * g.K] = t
                    v[blk].view(d["Cn"], g.ldb)[:, :g.K] = val
                self.B_dev = torch.cat([w, torch.zeros(SLACK, dtype=w.dtype)])
                self.b_val = v
            else:
                self.b_val = self._store(vb, dt)
                self.B_dev = torch.cat([self.b_val.to(TDT[dt]), torch.zeros(SLACK, dtype=TDT[dt])])
        else:
            # P (WGRAD): [batch][M][ldp]
            p_bst = d["p_bstride"] if B > 1 else g.M * g.ldp
            p_ext = (B - 1) * p_bst + g.M * g.ldp
            vp = torch.zeros(p_ext, dtype=torch.float64)
            live = torch.zeros(p_ext, dtype=torch.bool)
            for z in range(B):
                live[z * p_bst: z * p_bst + g.M * g.ldp].view(g.M, g.ldp)[:, :d["Cn"]] = True
            vp[live] = self._rand(int(live.sum()))
            self.p_bst = p_bst
            self.p_val, self.P_dev = self._device_operand(vp, mode_kind="P", pstride=d["p_pstride"], planes=d["p_planes"])
        # epilogue operands
        rows, cols = g.orows, g.ocols
        r_bst = d["r_bstride"] if B > 1 else rows * g.ldr
        self.r_bst = r_bst
        r_ext = (B - 1) * r_bst + rows * g.ldr
        self.bias = self.rowscale = None
        if "bias" in self.ops:
            self.bias = self._rand(cols if d["bias_mode"] == BIAS_COL else rows).float()
        if "rowscale" in self.ops:
            self.rowscale = (torch.rand(rows, generator=self.gen, dtype=torch.float64) + 0.5).float()
        self.R_val = self.R_dev = self.Rlo_dev = self.Mask_dev = self.mask_val = None
        r_live = torch.zeros(r_ext, dtype=torch.bool)
        for z in range(B):
            r_live[z * r_bst: z * r_bst + rows * g.ldr].view(rows, g.ldr)[:, :cols] = True
        if "R" in self.ops:
            vr = torch.zeros(r_ext, dtype=torch.float64)
            vr[r_live] = self._rand(int(r_live.sum()))
            if "R_lo" in self.ops:
                hi = vr.to(self._out16())
                lo = (vr - hi.double()).to(self._out16())
                self.R_dev, self.Rlo_dev = self._pad(hi), self._pad(lo)
                self.R_val = hi.double() + lo.double()
            else:
                rt = self._rdtype()
                self.R_val = vr.to(rt).double()
                self.R_dev = self._pad(vr.to(rt))
        if "mask" in self.ops:
            vm = torch.zeros(r_ext, dtype=torch.float64)
            vm[r_live] = torch.where(torch.rand(int(r_live.sum()), generator=self.gen) < 0.3, -1.0, 1.0).double()
            self.mask_val = vm
            self.Mask_dev = self._pad(vm.to(self._rdtype()))

    def _out16(self):
        d = self.d
        return torch.float16 if (self.pair_out or d["math"] == MATH_F16X3) else TDT[d["dtype"]]

    def _rdtype(self):
        """element type of R / Mask: the operand dtype (fp32 for the split maths and fp32 operands)"""
        return TDT[self.d["dtype"]]

    def _pad(self, t):
        return torch.cat([t, torch.zeros(SLACK, dtype=t.dtype)])

    def _device_operand(self, vals, mode_kind, pstride, planes):
        d = self.d
        dt, math_ = d["dtype"], d["math"]
        ext = vals.numel()
        if math_ == MATH_F16X3 and mode_kind == "A":
            if pstride < ext:
                raise Unmodelled("a_pstride overlaps the planes")
            hi, lo = f16_pair(vals)
            dev = torch.zeros(pstride + ext + SLACK, dtype=torch.float16)
            dev[:ext], dev[pstride:pstride + ext] = hi, lo
            return hi.double() + lo.double(), dev
        if planes:
            if pstride < ext:
                raise Unmodelled("plane stride overlaps the planes")
            terms = bf16_terms(vals.float(), planes)
            dev = torch.zeros((planes - 1) * pstride + ext + SLACK, dtype=torch.bfloat16)
            for i, t in enumerate(terms):
                dev[i * pstride: i * pstride + ext] = t
            used = self.sp if mode_kind == "A" and d["mode"] != WGRAD else 2
            return sum(t.double() for t in terms[:used]), dev
        v = self._store(vals, dt)
        return v, self._pad(v.to(TDT[dt]))

    # ---------------------------------------------------------------- expectation
    def _expect(self):
        d, g = self.d, self.g
        B = g.batch
        rows, cols = g.orows, g.ocols
        mode = d["mode"]
        idx = None if g.ident else g.gather_index()
        acc = torch.zeros(B, rows, cols, dtype=torch.float64)
        mag = torch.zeros(B, rows, cols, dtype=torch.float64)
        for z in range(B):
            a = self.a_val[z * self.a_bst: z * self.a_bst + g.S * g.lda].view(g.S, g.lda)[:, :d["Cs"]]
            if idx is None:
                ag = a
            else:
                ag = torch.cat([a, torch.zeros(1, d["Cs"], dtype=a.dtype)])[torch.where(idx < 0, g.S, idx)]
                ag = ag.reshape(g.M, g.K)
            if mode == WGRAD:
                p = self.p_val[z * self.p_bst: z * self.p_bst + g.M * g.ldp].view(g.M, g.ldp)[:, :d["Cn"]]
                acc[z] = p.t() @ ag
                mag[z] = p.abs().t() @ ag.abs()
            else:
                b = self.b_val[z * self.b_bst: z * self.b_bst + d["Cn"] * g.ldb].view(d["Cn"], g.ldb)[:, :g.K]
                acc[z] = ag @ b.t()
                mag[z] = ag.abs() @ b.abs().t()
        alpha = float(torch.tensor(d["alpha"], dtype=torch.float32))
        v = alpha * acc
        extra = torch.zeros_like(v)
        if mode == WGRAD:
            if self.rowscale is not None:
                v = v * self.rowscale.double().view(1, -1, 1)
                mag = mag * self.rowscale.double().view(1, -1, 1)
            self.lin = v.abs()
            if d["wgrad_bias"]:
                ps = torch.stack([self.p_val[z * self.p_bst: z * self.p_bst + g.M * g.ldp].view(g.M, g.ldp)[:, :d["Cn"]]
                                  for z in range(B)])
                rs = self.rowscale.double() if self.rowscale is not None else 1.0
                self.dbias_ref = alpha * ps.sum(1).sum(0) * rs
                self.dbias_mag = abs(alpha) * ps.abs().sum(1).sum(0) * (rs.abs() if self.rowscale is not None else 1.0)
            if d["accumulate"]:
                # (the launch reads the earlier O from memory: values of the output type, not fp32 ones rounded on upload)
                self.o_init = self._rand(B, rows, cols).to(TDT[d["out_dtype"]]).double()
                v = v + self.o_init
                extra = extra + self.o_init.abs()
        else:
            self.lin = v.abs()
            if self.bias is not None:
                bb = self.bias.double().view(1, 1, -1) if d["bias_mode"] == BIAS_COL else self.bias.double().view(1, -1, 1)
                v = v + bb
                extra = extra + bb.abs()
            if self.R_val is not None:
                r = self._rows_view(self.R_val, self.r_bst, g.ldr)
                v = v + r
                extra = extra + r.abs()
            if d["relu"]:
                v = torch.clamp(v, min=0)
            if self.mask_val is not None:
                v = torch.where(self._rows_view(self.mask_val, self.r_bst, g.ldr) > 0, v, torch.zeros_like(v))
        self.ref = v
        self.mag = abs(alpha) * mag
        self.extra = extra

    def _rows_view(self, flat, bst, ld):
        g = self.g
        return torch.stack([flat[z * bst: z * bst + g.orows * ld].view(g.orows, ld)[:, :g.ocols] for z in range(g.batch)])

    # ---------------------------------------------------------------- error model
    def k_steps(self):
        """sequential fp32 accumulation steps of one output element (a bound on the kernels' summation depth)"""
        d, g = self.d, self.g
        k = g.M if d["mode"] == WGRAD else g.K
        per = 4 if (d["dtype"] == F32 and not self.sp) else 16
        return k // per + 64

    def u_prod(self):
        m = self.d["math"]
        if m == MATH_F16X3:
            return 2.0 ** -21                  # lo.lo dropped: 2^-22 per product
        if m == MATH_BF16X3:
            return 2.0 ** -14                  # hh + hm + mh of two-term operands
        if m == MATH_BF16X6:
            return 2.0 ** -21
        return 2.0 ** -24 if self.d["dtype"] == F32 else 0.0

    def out_unit(self):
        """(relative rounding of the stored output value, absolute floor)"""
        d = self.d
        if self.pair_out or (d["dtype"] != F32 and d["out_dtype"] != F32 and "O_lo" in self.ops):
            return (2.0 ** -21, 2.0 ** -24) if self._out16() == torch.float16 else (2.0 ** -15, 1e-37)
        if d["out_dtype"] == F32:
            return 2.0 ** -24, 1e-37
        return UNIT[d["out_dtype"]], (2.0 ** -24 if d["out_dtype"] == F16 else 1e-37)

    def bound(self):
        """elementwise bound: the products and the fp32 accumulation (u_k of |alpha| |A|.|B|), the fp32 epilogue -- alpha
        (rowscale) times the accumulator, then + bias + R (+ R_lo, + O of an accumulate): a few fp32 roundings of those terms,
        2^-22 of their magnitudes -- and the rounding of the stored output value (u_out of |ref|, the format's floor)"""
        u_out, floor = self.out_unit()
        c = 2.0
        u_k = c * (self.u_prod() + 2.0 ** -24 * self.k_steps())
        return u_k * self.mag + 2.0 ** -22 * (self.lin + self.extra) + u_out * self.ref.abs() + floor

    def l2_bar(self):
        d = self.d
        if d["math"] == MATH_F16X3:
            return L2_BAR["f16x3"]
        if d["math"] == MATH_BF16X3:
            return L2_BAR["bf16x3"]
        if d["math"] == MATH_BF16X6:
            return L2_BAR["bf16x6"]
        if d["mode"] == DGRAD and (d["math"] == MATH_F16W2 or d["dt"] == 0):
            if d["out_dtype"] == F32:
                return L2_BAR["w2_f32"]
            return L2_BAR["w2_pair"] if "O_lo" in self.ops else L2_BAR["w2_f16"]
        if d["dtype"] == F32:
            return L2_BAR["f32"]
        if d["out_dtype"] != F32 and "O_lo" not in self.ops:
            return L2_BAR["bf16" if d["out_dtype"] == BF16 else "f16"]
        return L2_BAR["f32"] if d["out_dtype"] == F32 else (L2_BAR["w2_pair"] if d["dtype"] == F16 else L2_BAR["bf16x3"])

    # ---------------------------------------------------------------- launch and comparison
    def _out_buffer(self, dtype, planes=1, pstride=0, init=None):
        """(device buffer with guard bands, offset of the output, live mask): sentinel everywhere, NaN (or `init`) where
        the launch must write"""
        d, g = self.d, self.g
        B = g.batch
        bst = d["o_bstride"] if B > 1 else g.orows * g.ldo
        ext = (B - 1) * bst + g.orows * g.ldo
        if B > 1 and bst < g.orows * g.ldo:
            raise Unmodelled("o_bstride smaller than one batch element")
        ps = pstride if planes > 1 else 0
        if planes > 1 and ps < ext:
            raise Unmodelled("o_pstride overlaps the planes")
        total = GUARD + (planes - 1) * ps + ext + GUARD
        live = torch.zeros(total, dtype=torch.bool)
        for pl in range(planes):
            for z in range(B):
                o = GUARD + pl * ps + z * bst
                live[o: o + g.orows * g.ldo].view(g.orows, g.ldo)[:, :g.ocols] = True
        buf = torch.full((total,), SENTINEL, dtype=torch.float64)
        if init is None:
            buf[live] = float("nan")
        else:
            buf[live] = init.reshape(-1).repeat(planes)
        self.o_bst = bst
        return buf.to(dtype), live, ps

    def run(self, hip, device="cuda:0"):
        d = self.d
        dev = torch.device(device)
        desc = hip.conv_desc(**d)
        o_t = torch.float16 if self.pair_out else TDT[d["out_dtype"]]
        init = None
        if d["accumulate"]:
            init = self.o_init
        inplace = "class0_inplace" in self.ops
        if inplace:
            # (R = O and R_lo = O_lo: the rows the launch does not touch keep both terms of the earlier contribution)
            if self.r_bst != (self.g.orows * self.g.ldo) or self.g.ldr != self.g.ldo:
                raise Unmodelled("class0_inplace needs R laid out as O")
            init = self._rows_view(self.R_dev[:-SLACK].double(), self.r_bst, self.g.ldr)
        O, self.o_live, _ = self._out_buffer(o_t, init=init)
        self.O = O.to(dev)
        off = GUARD
        Ov = self.O[off:]
        kw = {}
        self.Olo = self.Opl = None
        if "O_lo" in self.ops:
            lo_t = torch.float16 if self.pair_out or d["math"] == MATH_F16X3 else TDT[d["dtype"]]
            lo_init = None
            if inplace and self.Rlo_dev is not None:
                lo_init = self._rows_view(self.Rlo_dev[:-SLACK].double(), self.r_bst, self.g.ldr)
            b, self.lo_live, _ = self._out_buffer(lo_t, init=lo_init)
            self.Olo = b.to(dev)
            kw["O_lo"] = self.Olo[off:]
        if "O_planes" in self.ops:
            if d["o_planes"] == 1:
                b, self.pl_live, _ = self._out_buffer(torch.float16)
            else:
                b, self.pl_live, _ = self._out_buffer(torch.bfloat16, planes=2, pstride=d["o_pstride"])
            self.Opl = b.to(dev)
            kw["O_planes"] = self.Opl[off:]
        R = None
        if self.R_dev is not None:
            R = Ov if "class0_inplace" in self.ops else self.R_dev.to(dev)
            if self.Rlo_dev is not None:
                kw["R_lo"] = kw["O_lo"] if (inplace and "O_lo" in kw) else self.Rlo_dev.to(dev)
        self.dbias = None
        if "dbias" in self.ops:
            self.dbias = torch.full((GUARD + d["Cn"] + GUARD,), SENTINEL, dtype=torch.float32)
            self.dbias[GUARD:GUARD + d["Cn"]] = float("nan")
            self.dbias = self.dbias.to(dev)
            kw["dbias"] = self.dbias[GUARD:]
        # the workspace: exactly vlfb_conv_workspace_bytes between two sentinel bands, NaN where the launch may write (a slab
        # element a reduce reads without any workgroup having written it turns the output NaN)
        ws_bytes = hip.conv_workspace_bytes(desc)
        self.ws = ws = None
        if ws_bytes:
            assert ws_bytes % 4 == 0, ws_bytes
            self.ws = torch.full((GUARD + ws_bytes // 4 + GUARD,), SENTINEL, dtype=torch.float32)
            self.ws[GUARD:-GUARD] = float("nan")
            self.ws = self.ws.to(dev)
            ws = self.ws[GUARD:-GUARD]
            assert ws.numel() * ws.element_size() == ws_bytes
        A = self.A_dev.to(dev)
        Bop = self.B_dev.to(dev) if d["mode"] != WGRAD else None
        P = self.P_dev.to(dev) if d["mode"] == WGRAD else None
        hip.conv_run(desc, A, Bop, P, Ov, bias=None if self.bias is None else self.bias.to(dev),
                     rowscale=None if self.rowscale is None else self.rowscale.to(dev), R=R,
                     mask=None if self.Mask_dev is None else self.Mask_dev.to(dev), workspace=ws, **kw)
        torch.cuda.synchronize(dev)

    def _live_values(self, buf, live, plane=0, pstride=0):
        g = self.g
        vals = []
        for z in range(g.batch):
            o = GUARD + plane * pstride + z * self.o_bst
            vals.append(buf[o: o + g.orows * g.ldo].view(g.orows, g.ldo)[:, :g.ocols])
        return torch.stack(vals)

    def check(self):
        """compare every output of the launch with the model; returns a dict of the worst figures (raises AssertionError)"""
        d = self.d
        out = {}
        if self.ws is not None:
            w = self.ws.cpu().double()
            live = torch.zeros(w.numel(), dtype=torch.bool)
            live[GUARD:-GUARD] = True
            self._guard("workspace", w, live)
        O = self.O.cpu().double()
        self._guard("O", O, self.o_live)
        got = self._live_values(O, self.o_live)
        if self.pair_out or (self.Olo is not None and d["out_dtype"] != F32):
            lo = self.Olo.cpu().double()
            self._guard("O_lo", lo, self.lo_live)
            got = got + self._live_values(lo, self.lo_live)
        out["O"] = self._compare("O", got, self.ref, self.bound(), self.l2_bar())
        if self.Olo is not None and d["out_dtype"] == F32:
            # fp32 output with O_lo: the output rounded to the 16-bit operand type
            lo = self.Olo.cpu().double()
            self._guard("O_lo", lo, self.lo_live)
            h = self._live_values(lo, self.lo_live)
            u = UNIT[F16] if self.Olo.dtype == torch.float16 else UNIT[BF16]
            out["O_lo"] = self._compare("O_lo", h, self.ref, self.bound() + u * self.ref.abs() + 2.0 ** -25, 1e-2)
            if d["math"] == MATH_F16X3:       # (the fp16 copy of a two-plane forward output: what the backward masks with)
                assert bool(((got > 0) <= (h > 0)).all()), "O_lo: a positive output lost its sign in the fp16 copy"
        if self.Opl is not None:
            pl = self.Opl.cpu().double()
            self._guard("O_planes", pl, self.pl_live)
            if d["o_planes"] == 1:
                h = self._live_values(pl, self.pl_live)
                out["O_planes"] = self._compare("O_planes", h, self.ref, self.bound() + UNIT[F16] * self.ref.abs(), 1e-2)
                assert bool(((got > 0) <= (h > 0)).all()), "O_planes: a positive output lost its sign in the fp16 copy"
            else:
                h = self._live_values(pl, self.pl_live, 0, d["o_pstride"]) + self._live_values(pl, self.pl_live, 1, d["o_pstride"])
                out["O_planes"] = self._compare("O_planes", h, self.ref, self.bound() + 2.0 ** -15 * self.ref.abs(), 4e-5)
        if self.dbias is not None:
            db = self.dbias.cpu().double()
            live = torch.zeros(db.numel(), dtype=torch.bool)
            live[GUARD:GUARD + d["Cn"]] = True
            self._guard("dbias", db, live)
            u = self.u_prod() + 2.0 ** -24 * (self.g.M // 16 + 64)
            out["dbias"] = self._compare("dbias", db[live].view(1, 1, -1), self.dbias_ref.view(1, 1, -1),
                                         2 * u * self.dbias_mag.view(1, 1, -1) + 1e-37, self.l2_bar())
        return out

    def _guard(self, name, buf, live):
        bad = (buf[~live] != SENTINEL)
        assert not bool(bad.any()), "%s: %d element(s) outside the output changed (first at %d)" % (
            name, int(bad.sum()), int(torch.nonzero(~live)[bad.nonzero()[0]].item()))

    def _compare(self, name, got, ref, bound, bar):
        fin = torch.isfinite(got)
        assert bool(fin.all()), "%s: %d element(s) not written or not finite (first at %s)" % (
            name, int((~fin).sum()), tuple(torch.nonzero(~fin)[0].tolist()))
        err = (got - ref).abs()
        over = err > bound
        if bool(over.any()):
            i = tuple(torch.nonzero(over)[0].tolist())
            raise AssertionError("%s: %d element(s) past the elementwise bound; first at (batch, row, col) %s: got %.9g "
                                 "ref %.9g bound %.3g" % (name, int(over.sum()), i, got[i].item(), ref[i].item(), bound[i].item()))
        den = ref.norm().item()
        rel = (got - ref).norm().item() / (den if den > 0 else 1.0)
        assert rel < bar, "%s: relative L2 %.3e >= %.1e" % (name, rel, bar)
        return rel


# ---------------------------------------------------------------------------------------------------- shrinking
def plan_key(plan):
    """plan string with the split count bucketed to 1 / >1"""
    import re
    return re.sub(r"splits=(\d+)", lambda m: "splits=1" if m.group(1) == "1" else "splits>1", plan)


def flops(d):
    g = Geometry(d)
    k = g.K // 2 if (d["mode"] == DGRAD and d["dt"] == 0) else g.K
    return 2.0 * g.M * d["Cn"] * k * g.batch


def _resize(d, n=None, t=None, h=None, w=None):
    """copy of `d` with N and the row extents of T / H / W lowered by (t, h, w) rows; the source extents follow from the
    geometry, plane and batch strides that spanned the old extents span the new ones"""
    e = dict(d)
    old = Geometry(d)
    if n is not None:
        e["N"] = n
    for ax, k in (("T", t), ("H", h), ("W", w)):
        if not k:
            continue
        s = {"T": d["st"], "H": d["sh"], "W": d["sw"]}[ax]
        if old.ident:
            e[ax + "r"] -= k
            e[ax + "s"] -= k
        elif d["mode"] == DGRAD:         # rows = conv input positions, source = conv output: k * stride rows per source row
            e[ax + "r"] -= k * s
            e[ax + "s"] -= k
        else:
            e[ax + "r"] -= k
            e[ax + "s"] -= k * s
    if min(e["N"], e["Tr"], e["Hr"], e["Wr"], e["Ts"], e["Hs"], e["Ws"]) < 1:
        return None
    new = Geometry(e)
    B = old.batch
    a_old, a_new = old.S * old.lda, new.S * new.lda
    r_old, r_new = old.orows * old.ldo, new.orows * new.ldo
    p_old, p_new = old.M * old.ldp, new.M * new.ldp
    rr_old, rr_new = old.orows * old.ldr, new.orows * new.ldr
    if B > 1:
        for f, o, nw in (("a_bstride", a_old, a_new), ("o_bstride", r_old, r_new), ("p_bstride", p_old, p_new),
                         ("r_bstride", rr_old, rr_new)):
            if e[f] == o:
                e[f] = nw
            elif e[f] and e[f] < o:
                return None            # (batch elements interleaved inside the rows: keep the extents)
    ext = lambda one, f: (B - 1) * e[f] + one if B > 1 else one
    if d["a_pstride"]:
        e["a_pstride"] = -(-ext(a_new, "a_bstride") // 8) * 8
    if d["p_pstride"]:
        e["p_pstride"] = -(-ext(p_new, "p_bstride") // 8) * 8
    if d["o_pstride"]:
        e["o_pstride"] = -(-ext(r_new, "o_bstride") // 8) * 8
    return e


MIN_ROWS = 2      # row positions kept per T / H / W axis (where the descriptor has them): the row decode past row 0


def shrink(d, plan_fn, target_flops=0.0):
    """smallest descriptor (N, then T, then H / W) with the same plan key as `d`; plan_fn(dict) -> plan string or None.
    A candidate must keep every tap that reads data in `d` reading data for some row (a shrunk gathered conv whose taps
    fall into the padding would test only the taps that are left), and at least MIN_ROWS positions on every row axis."""
    key = plan_key(plan_fn(d))
    live = Geometry(d).live_taps()
    floor = {ax: min(d[ax + "r"], MIN_ROWS) for ax in "THW"}
    cur = dict(d)

    def same(e):
        if e is None or any(e[ax + "r"] < floor[ax] for ax in "THW"):
            return False
        try:
            if Geometry(e).live_taps() != live:
                return False
            return plan_key(plan_fn(e)) == key
        except Exception:
            return False

    for axis in ("N", "T", "H", "W", "T", "H", "W"):
        while True:
            if axis == "N":
                span = cur["N"] - 1
            else:
                span = cur[axis + "r"] - 1
            if span <= 0:
                break
            moved = False
            for k in sorted({span, span * 3 // 4, span // 2, span // 4, 1}, reverse=True):
                if k <= 0:
                    continue
                e = _resize(cur, n=cur["N"] - k) if axis == "N" else _resize(cur, **{axis.lower(): k})
                if same(e):
                    cur, moved = e, True
                    break
            if not moved or flops(cur) <= target_flops:
                break
    return cur
