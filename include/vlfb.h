/*
 * vlfb.h -- C ABI of libvlfb_hip.so, the MI355X (gfx950) kernel library behind the
 * R50/R101-I3D-NL + long-term-feature-bank training path.
 *
 * The reference (facebookresearch/video-long-term-feature-banks) reaches its GPU code
 * through the Caffe2 operator registry; Caffe2 is gone, so this header IS the plug-in
 * boundary.  Every entry point cites the reference interface it replaces.
 *
 * Conventions
 *   - plain pointers + sizes only; no torch / HIP types in signatures (vlfb_stream_t is a
 *     hipStream_t passed as void*).
 *   - the caller owns every buffer; kernels are asynchronous on `stream`; the library
 *     allocates nothing.  Its only state: a thread-local error string, a thread-local conv plan cache, launch
 *     attributes set once per process and kernel, and environment switches and device properties read once
 *     (all once-initialised, thread-safe); any number of threads may call it concurrently.
 *   - every function returns VLFB_OK (0) or a negative error code; vlfb_last_error() gives text.
 *   - "NCTHW" = the reference's blob layout (kwargs['order']='NCHW',
 *     lib/models/model_builder_video.py:69).  "NTHWC" = this library's internal
 *     channels-last activation layout (rows = N*T*H*W positions, C contiguous).
 *   - element types: VLFB_BF16 / VLFB_F16 (throughput paths: 16-bit storage, bf16 / fp16 MFMA with fp32
 *     accumulation) and VLFB_F32 -- with vlfb_conv_desc.math = 0 the exact-fp32 MFMA, with math = BF16X6 /
 *     BF16X3 the parity-grade path: fp32 storage, every product as split-bf16 products on the bf16 matrix cores.
 */
#ifndef VLFB_H_
#define VLFB_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vlfb_stream_t;

enum { VLFB_F32 = 0, VLFB_BF16 = 1, VLFB_F16 = 2 };
/* Weight-operand format of the split-bf16 path (vlfb_conv_desc.math != 0; accepted by vlfb_weight_prep* only): the
 * FPROP copy is THREE bf16 planes [3][Cout][taps][Cin] (h = bf16(w), m = bf16(w - h), l = bf16(w - h - m)), the DGRAD
 * copy TWO planes [2][Cin][taps][Cout] (h, m). */
enum { VLFB_SPLIT = 3 };
/* Weight-operand formats of the "mix" path (split-bf16 FORWARD products on fp32 storage, fp16 BACKWARD; accepted by
 * vlfb_weight_prep* only): the FPROP copy as VLFB_SPLIT's three bf16 planes; the DGRAD copy
 *   VLFB_MIX     plain fp16 [Cin][taps][Cout]
 *   VLFB_MIX_W2  two fp16 terms of (w * s) * VLFB_MIX_W2_SCALE, [Cin][term][taps][Cout]: the weight of the same
 *                convolution with a doubled OUTERMOST tap dimension of dilation 0 (vlfb_conv_desc: kt' = 2 kt... with
 *                dt = 0; alpha carries 1 / VLFB_MIX_W2_SCALE), so that the plain fp16 DGRAD kernels contract the fp16
 *                gradient with 22 significant bits of W: dX = dY . Wh + dY . Wl */
enum { VLFB_MIX = 4, VLFB_MIX_W2 = 5 };
#define VLFB_MIX_W2_SCALE 1024.0f
/* ... of the two-plane fp16 forward (vlfb_conv_desc.math = VLFB_MATH_F16X3): the FPROP copy as the two fp16 terms of
 * (w * s) * VLFB_MIX_W2_SCALE, planes [term][Cout][taps][Cin] (alpha of the launch carries 1 / VLFB_MIX_W2_SCALE); the
 * DGRAD copy as VLFB_MIX (VLFB_MIXH) or VLFB_MIX_W2 (VLFB_MIXH_W2) */
enum { VLFB_MIXH = 6, VLFB_MIXH_W2 = 7 };
/* ... with the two-term DGRAD copy INTERLEAVED per 64-channel k-tile: [Cin][taps][Cout / 64][term][64] (Cout % 64 == 0),
 * the weight operand of vlfb_conv_desc.math = VLFB_MATH_F16W2 -- the two terms of a tap's 64 channels are consecutive
 * k-tiles, contracted with ONE gradient tile (fetched into LDS and read from it once).  FPROP copy as VLFB_MIX (three bf16
 * planes; VLFB_MIX_W2I) or as VLFB_MIXH (two fp16 planes; VLFB_MIXH_W2I). */
enum { VLFB_MIX_W2I = 9, VLFB_MIXH_W2I = 10 };
/* A TWO-PLANE fp16 tensor: [2][numel] fp16, value = plane 0 (hi = fp16(v)) + plane 1 (lo = fp16(v - hi)), ~22 significant
 * bits.  The storage format of the forward activations of the "mix" path: plane 0 alone is the fp16 tensor the fp16 backward
 * reads (WGRAD operand, ReLU mask).  vlfb_pool_desc.dtype of vlfb_maxpool_fwd (x, y two-plane) and vlfb_avgpool_fwd (x
 * two-plane, y fp32); produced by convolutions through O / O_lo of vlfb_conv_args, by vlfb_pair_split from fp32. */
enum { VLFB_F16PAIR = 8 };
/* vlfb_conv_desc.math: how the contraction is evaluated when dtype == VLFB_F32.
 *   VLFB_MATH_NATIVE  v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 vector rate)
 *   VLFB_MATH_BF16X6  operands expanded into three bf16 terms each, six bf16 MFMAs per product (hh hm mh mm hl lh):
 *                     fp32-grade results at 1/6 of the bf16 matrix rate (forward products of the parity path)
 *   VLFB_MATH_BF16X3  two terms each, three MFMAs (hh hm mh): ~2^-17 per product (backward products)
 * With math != 0 the B operand of FPROP / DGRAD launches is pre-split: bf16 planes (3 for BF16X6, 2 for BF16X3)
 * `b_pstride` elements apart, each laid out as the fp32 B operand would be (vlfb_weight_prep* with VLFB_SPLIT,
 * vlfb_split_planes); A, P, R, Mask and O stay fp32. */
enum { VLFB_MATH_NATIVE = 0, VLFB_MATH_BF16X3 = 3, VLFB_MATH_BF16X6 = 6,
       /* dtype VLFB_F16, FPROP / plain NT products: BOTH operands are two fp16 planes (A: a_pstride elements apart, B:
        * b_pstride, 0 = Cn * ldb), a product is hi.hi + hi.lo + lo.hi on the fp16 MFMA (~2^-21 per product, nothing is
        * converted in the k-loop; fp16 MFMA operands keep subnormals).  out_dtype VLFB_F16: the output is written as two
        * planes O / O_lo, the residual read as R / R_lo (vlfb_conv_args); out_dtype VLFB_F32: a plain fp32 output.
        * The split-bf16 maths accept out_dtype VLFB_F16 in the same sense (fp32 A operand, two-plane output / residual). */
       VLFB_MATH_F16X3 = 13,
       /* dtype VLFB_F16 / VLFB_BF16, unit-stride DGRAD with Cs % 64 == 0: the weight operand holds TWO 16-bit terms per
        * value, rows [tap][Cs / 64][term][64] (vlfb_weight_prep* VLFB_MIX_W2I; ldb = 2 K), dX = dY . (Wh + Wl) with every
        * gradient tile contracted with both terms (alpha carries 1 / VLFB_MIX_W2_SCALE).  The same product as the
        * doubled-tap form of VLFB_MIX_W2 on 3/4 of its LDS DMA bytes and 2/3 of its LDS fragment reads. */
       VLFB_MATH_F16W2 = 12 };

enum {
  VLFB_OK = 0,
  VLFB_ERR_ARG = -1,
  VLFB_ERR_LAUNCH = -2,
  VLFB_ERR_UNSUPPORTED = -3,
  VLFB_ERR_WORKSPACE = -4
};

const char* vlfb_last_error(void);
int vlfb_version(void);
/* number of bytes per element of a VLFB_* dtype (0 if unknown) */
int vlfb_dtype_size(int dtype);

/* ------------------------------------------------------------------------------------------
 * AffineNd / AffineNdGradient -- the reference's only native op, on its own layout.
 * Replaces REGISTER_CUDA_OPERATOR(AffineNd, ...) / (AffineNdGradient, ...)
 *   caffe2_customized_ops/video/affine_nd_op.cu:31-44,61-83  (y = x*s[c] + b[c])
 *   caffe2_customized_ops/video/affine_nd_op.cu:46-58,85-104 (dx = dy*s[c]; no ds/db)
 * x,y: fp32 NCTHW with `inner` = T*H*W elements per (n,c); in-place allowed (x==y, dy==dx)
 * as in the schema (affine_nd_op.cc:35-43).  numel must be < 2^31 as in the reference.
 * ------------------------------------------------------------------------------------------ */
int vlfb_affine_nd_fwd(const float* x, const float* scale, const float* bias, float* y,
                       int64_t n, int64_t c, int64_t inner, vlfb_stream_t stream);
int vlfb_affine_nd_bwd(const float* dy, const float* scale, float* dx,
                       int64_t n, int64_t c, int64_t inner, vlfb_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Implicit-GEMM 3-D convolution family (MFMA), channels-last.
 * Replaces every cuDNN `Conv` the builders emit (ModelBuilder.ConvNd call sites:
 * lib/models/model_builder_video.py:181,211; resnet_video.py:169; nonlocal_helper.py:36,58,68,131;
 * lib/models/lfb_helper.py:175,184,194,244,303,323), its auto-generated ConvGradient
 * (dgrad + wgrad), and the cuBLAS BatchMatMul calls (nonlocal_helper.py:94,121) -- a plain or
 * batched GEMM is the 1x1x1 special case.
 *
 * mode FPROP:  O[m][n]  = sum_{tap,c} A[src(m,tap)][c] * B[n][tap][c]
 *              rows m enumerate the OUTPUT positions (N,Tr,Hr,Wr);
 *              src(m,tap) = m*stride - pad + tap*dil, inside (Ts,Hs,Ws) else 0.
 * mode DGRAD:  same contraction, rows m enumerate the conv's INPUT positions (N,Tr,Hr,Wr) and
 *              A is the output-gradient (N,Ts,Hs,Ws,Cs): src = (m + pad - tap*dil)/stride when
 *              divisible and in range else 0; B is the weight in [Cin][tap][Cout] order.
 * mode WGRAD:  O[p][tap][c] = sum_m P[m][p] * A[src(m,tap)][c]
 *              (m = output positions; P = output gradient [M][Cn]; A = the conv input).
 *              If the launch is split along m, fp32 partial slabs go to `workspace` and
 *              vlfb_conv_wgrad_reduce must follow (vlfb_conv_run does it when it is given
 *              a workspace).
 * pack_w:      stem mode (conv1, Cs = 4 padded RGB): the kw taps are packed with the channel
 *              dim into the contiguous K axis, K = kt*kh*(kw_pad*Cs); requires dw == 1 and an
 *              input whose W rows are zero-padded (vlfb_ncthw_to_nthwc_wpad) so that
 *              w*sw - pw + [0, kw_pad) is always inside [0, Ws).
 * epilogue (FPROP/DGRAD): v = alpha*acc + bias + R[m][n]; relu; then v = (Mask[m][n] > 0) ? v : 0
 * epilogue (WGRAD):       v = alpha * rowscale[p] * acc (+ O if accumulate)
 * ------------------------------------------------------------------------------------------ */
enum { VLFB_CONV_FPROP = 0, VLFB_CONV_DGRAD = 1, VLFB_CONV_WGRAD = 2 };
enum { VLFB_BIAS_NONE = 0, VLFB_BIAS_COL = 1, VLFB_BIAS_ROW = 2 };
enum { VLFB_ALGO_AUTO = 0, VLFB_ALGO_TILE128 = 1, VLFB_ALGO_PIPE256 = 2, VLFB_ALGO_STREAM = 3,
       VLFB_ALGO_CLASSES = 4 /* split-math DGRAD of a (1,2,2)-strided conv: force the parity-class walk (AUTO takes it for kh*kw > 1) */,
       /* 16-bit DGRAD of a (1,2,2)-strided 1x1x1 conv (the projection shortcut of res3_0 / res4_0, resnet_helper.py:86-103) as
        * an ACCUMULATE over the rows it touches: only the input positions the conv reads (even h, even w: a quarter of the
        * rows) are computed and written, every other row of O is LEFT AS IT IS.  For a caller that passes R = O holding an
        * earlier contribution to the same gradient (in-place accumulate; R_lo = O_lo likewise), or has zero-filled O. */
       VLFB_ALGO_CLASS0 = 5 };

typedef struct vlfb_conv_desc {
  int32_t mode;
  int32_t dtype;      /* operand element type of A, B(,P), R, Mask */
  int32_t out_dtype;  /* VLFB_F32 or == dtype */
  /* row space (see mode) */
  int32_t N, Tr, Hr, Wr;
  /* gather-source extents and channels (per tap K extent = Cs, or kw_pad*Cs with pack_w) */
  int32_t Ts, Hs, Ws, Cs;
  int32_t kt, kh, kw;
  int32_t st, sh, sw;
  int32_t pt, ph, pw;
  int32_t dt, dh, dw;
  int32_t pack_w;     /* 0, or kw_pad (padded kw, power of two) */
  /* FPROP/DGRAD: number of output columns; WGRAD: channels of P (output rows) */
  int32_t Cn;
  /* leading dimensions in elements (0 = dense default) */
  int32_t lda;        /* A position stride            (default Cs)            */
  int32_t ldb;        /* B row stride                 (default K)             */
  int32_t ldo;        /* O row stride                 (default Cn, WGRAD: K)  */
  int32_t ldr;        /* R / Mask row stride          (default ldo)           */
  int32_t ldp;        /* WGRAD: P position stride     (default Cn)            */
  /* batched GEMM (blockIdx.z); strides in elements */
  int32_t batch;
  int64_t a_bstride, b_bstride, o_bstride, r_bstride, p_bstride;
  /* epilogue */
  float alpha;
  int32_t relu;
  int32_t bias_mode;
  int32_t accumulate; /* WGRAD only: O += ... */
  int32_t splits;     /* WGRAD only: 0 = library chooses */
  int32_t algo;       /* kernel family: 0 = library chooses, 1 = 128x128 tiles (one barrier per k-tile),
                         2 = 256-row phase-pipelined tiles (bf16, MFMA-bound shapes; error if the
                         problem is not eligible), 3 = weight-resident streaming kernel (FPROP / DGRAD of
                         HBM-bound layers whose weight operand fits LDS; error if not eligible).  The
                         tile families (1, 2, 3, the direct-convolution kernels AUTO may pick) give bit-identical
                         results; the one exception under AUTO is the skinny kernel for plain NT products of at
                         most 64 rows (the FBO head on one row per RoI), whose four waves split K: same products,
                         another fp32 summation order (VLFB_SKINNY=0 or algo = 1 restores the tile order). */
  int32_t math;       /* VLFB_MATH_* (dtype VLFB_F32 only) */
  int64_t b_pstride;  /* math != 0, FPROP / DGRAD: elements between the bf16 term planes of B (0 = batch * Cn * ldb) */
  /* math != 0: activations / gradients that some earlier launch already wrote as bf16 term planes next to their fp32
   * values (o_planes below) can be handed in pre-split -- the kernel then spends no VALU on the expansion:
   *   a_planes  0 = A is fp32; 2 (BF16X3) = A points at [plane][position][lda] bf16 planes, a_pstride elements apart
   *   p_planes  WGRAD only: the same for P (ldp); WGRAD takes both operands as planes or neither
   *   o_planes  FPROP / DGRAD: 2 = additionally write the first two bf16 terms of every output value to the
   *             O_planes argument of vlfb_conv_run_planes, [plane][row][ldo], o_pstride elements apart;
   *             1 = additionally write an fp16 COPY of the output to O_planes, [row][ldo] (batch stride o_bstride): what
   *             the fp16 backward of the "mix" path reads (positive values stay positive in the copy) */
  int32_t a_planes, p_planes, o_planes;
  int32_t wgrad_bias; /* WGRAD only: 1 = the launch also produces the bias gradient db[p] = alpha * rowscale[p] * sum_m P[m][p]
                         (vlfb_conv_run_wgrad_bias; a batched launch sums over its batch elements too: db stays [Cn]);
                         counted in vlfb_conv_workspace_bytes */
  int64_t a_pstride, p_pstride, o_pstride;
} vlfb_conv_desc;

/* fills the desc with zeros and safe defaults (1x1x1, stride 1, alpha 1, batch 1) */
void vlfb_conv_desc_init(vlfb_conv_desc* d);
/* bytes of fp32 workspace vlfb_conv_run needs for this desc (0 unless a split WGRAD) */
int64_t vlfb_conv_workspace_bytes(const vlfb_conv_desc* d);

/* Text description of what vlfb_conv_run launches for this descriptor -- kernel family, element type, tile, split count
 * ("nt8 bf16 256x256", "tn_tr f16 128x128 splits=24", ...).  The planner is a pure function of the descriptor.  buf: at
 * least 96 bytes. */
int vlfb_conv_plan_describe(const vlfb_conv_desc* d, char* buf, int64_t buf_bytes);

/* One scratch query for every entry point that takes caller-owned scratch (the caller owns every
 * buffer, the library never allocates).  `arg` is the op's descriptor or dimension list; returns bytes, < 0 on error.
 *   VLFB_WS_CONV           arg = const vlfb_conv_desc*            `workspace` of vlfb_conv_run (= vlfb_conv_workspace_bytes)
 *   VLFB_WS_MAXPOOL_ARGMAX arg = const vlfb_pool_desc*            the whole `argmax` tensor of vlfb_maxpool_fwd / _bwd
 *   VLFB_WS_FBO_ATTN_BWD   arg = const int64_t[2] {r, k}          `ds_ws` of vlfb_fbo_attn_bwd (r RoIs x k bank rows, fp32)
 *   VLFB_WS_ATTN_SCORES    arg = const int64_t[3] {b, l1, l2}     fp32 score matrix between the scores GEMM and
 *                                                                vlfb_softmax_fwd / _bwd when the fused kernels are not used
 *   VLFB_WS_BN             arg = const int64_t[3] {dtype, rows, C} `workspace` of vlfb_bn_fwd / _bwd (= vlfb_bn_workspace_bytes)
 *   VLFB_WS_CLASS_AP       arg = const int64_t[2] {n, cols}       `workspace` of vlfb_class_ap_auc (its global sort path)
 *   VLFB_WS_CLASS_AP_VOC   arg = const int64_t[2] {n, cols}       `workspace` of vlfb_class_ap_voc (its global sort path) */
enum { VLFB_WS_CONV = 0, VLFB_WS_MAXPOOL_ARGMAX = 1, VLFB_WS_FBO_ATTN_BWD = 2, VLFB_WS_ATTN_SCORES = 3, VLFB_WS_BN = 4,
       VLFB_WS_CLASS_AP = 5, VLFB_WS_CLASS_AP_VOC = 6 };
int64_t vlfb_query_workspace(int op, const void* arg);
/* A: activation / gradient operand; B: weight operand (FPROP/DGRAD) or unused (WGRAD);
 * P: WGRAD output-gradient operand; O: output; bias/rowscale: fp32 vectors or NULL;
 * R, Mask: optional, dtype elements. */
int vlfb_conv_run(const vlfb_conv_desc* d, const void* A, const void* B, const void* P, void* O,
                  const float* bias, const float* rowscale, const void* R, const void* Mask,
                  void* workspace, int64_t workspace_bytes, vlfb_stream_t stream);
/* the same with the destination of the output's term planes (desc.o_planes > 0; NULL otherwise) */
int vlfb_conv_run_planes(const vlfb_conv_desc* d, const void* A, const void* B, const void* P, void* O,
                         const float* bias, const float* rowscale, const void* R, const void* Mask,
                         void* workspace, int64_t workspace_bytes, void* O_planes, vlfb_stream_t stream);

/* Every operand of a launch in one struct (what the three entry points above pass, plus):
 *   R_lo / O_lo  16-bit FPROP / DGRAD launches with 16-bit outputs: a TWO-TERM residual / output.  The epilogue computes
 *                v = alpha * acc + bias + R + R_lo; relu; mask  and stores O = T(v), O_lo = T(v - O): a running sum that is
 *                re-rounded by every launch of a chain (the residual-stream gradient of the bottleneck stack) keeps ~22
 *                significant bits while its leading term O stays a plain 16-bit MFMA operand.  Either may be NULL.
 *                With an fp32 output (out_dtype VLFB_F32 on 16-bit operands) O_lo alone is accepted as well: it receives the
 *                output ROUNDED to the operand type -- the copy the next 16-bit launch reads, without a cast pass. */
typedef struct vlfb_conv_args {
  const void* A; const void* B; const void* P; void* O;
  const float* bias; const float* rowscale;
  const void* R; const void* Mask;
  void* workspace; int64_t workspace_bytes;
  void* O_planes; float* dbias;
  const void* R_lo; void* O_lo;
} vlfb_conv_args;
int vlfb_conv_run_args(const vlfb_conv_desc* d, const vlfb_conv_args* a, vlfb_stream_t stream);

/* WGRAD with desc.wgrad_bias = 1: weight gradient O and bias gradient dbias (fp32 [Cn]) of a conv that carries a bias
 * (nonlocal_helper.py:36-77, lfb_helper.py:175-200) from ONE pass over the output gradient P: the 16-bit transposed-read
 * kernel sums the P tiles it stages anyway (per-split partial rows, folded in split order: deterministic); for every other
 * kernel family the library runs a column-sum pass behind the launch -- the caller does not have to know which. */
int vlfb_conv_run_wgrad_bias(const vlfb_conv_desc* d, const void* A, const void* P, void* O, float* dbias,
                             const float* rowscale, void* workspace, int64_t workspace_bytes, vlfb_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Layout / dtype movers at the boundary.
 * ------------------------------------------------------------------------------------------ */
/* fp32 NCTHW (the `data` blob, lib/datasets/ava_data_input.py:143-161) -> NTHWC with C padded
 * to c_pad (zeros) in `dtype`. */
int vlfb_ncthw_to_nthwc(const float* src, void* dst, int dtype, int64_t n, int64_t c, int64_t thw,
                        int64_t c_pad, vlfb_stream_t stream);
/* The stem's input format: as above with `wpad_left` / (w_total - wpad_left - w) zero pixels on the
 * two sides of every W row, [N][rows = T*H][w_total][c_pad].  With it the packed conv1 kernels
 * (pack_w) never test w bounds; pass Ws = w_total and pw = pad_w - wpad_left in the conv desc. */
int vlfb_ncthw_to_nthwc_wpad(const float* src, void* dst, int dtype, int64_t n, int64_t c, int64_t rows,
                             int64_t w, int64_t c_pad, int64_t wpad_left, int64_t w_total,
                             vlfb_stream_t stream);
/* NTHWC `dtype` -> fp32 NCTHW (for FetchBlob of activations / gradients) */
int vlfb_nthwc_to_ncthw(const void* src, float* dst, int dtype, int64_t n, int64_t c, int64_t thw,
                        vlfb_stream_t stream);
/* fp32 -> two-plane fp16 (VLFB_F16PAIR: dst[0..n) = hi, dst[n..2n) = lo) and back; n % 8 == 0 */
int vlfb_pair_split(const float* src, void* dst_pair, int64_t n, vlfb_stream_t stream);
int vlfb_pair_join(const void* src_pair, float* dst, int64_t n, vlfb_stream_t stream);
/* generic cast fp32 <-> dtype, n elements */
int vlfb_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n,
              vlfb_stream_t stream);
/* fp32 -> fp16 copy whose sign pattern equals the source's (a positive value below the fp16 subnormal range becomes the
 * smallest subnormal, not +0): the activations the "mix" path's fp16 backward reads as WGRAD operands and ReLU masks */
int vlfb_half_copy(const float* src, void* dst_f16, int64_t n, vlfb_stream_t stream);
/* batched 2-D transpose of dtype elements: dst[b][j][i] = src[b][i][j], src is rows x cols */
int vlfb_transpose2d(const void* src, void* dst, int dtype, int64_t batch, int64_t rows,
                     int64_t cols, vlfb_stream_t stream);
/* strided 2-D copy of dtype elements (Concat axis=1 and its gradient, head_helper.py:55,82) */
int vlfb_copy2d(const void* src, int64_t lds, void* dst, int64_t ldd, int dtype, int64_t rows,
                int64_t cols, vlfb_stream_t stream);
int vlfb_zero_f32(float* p, int64_t n, vlfb_stream_t stream);
/* fp32 [batch][rows][cols] -> `nplanes` (2 | 3) bf16 term planes [plane][batch][rows][cols] (transpose = 0) or
 * [plane][batch][cols][rows] (transpose = 1): the B operands of split-bf16 launches that are activations (the
 * attention products, nonlocal_helper.py:94-121) */
int vlfb_split_planes(const float* src, void* dst, int nplanes, int64_t batch, int64_t rows, int64_t cols,
                      int transpose, vlfb_stream_t stream);
/* Weight preparation: fp32 master W[Cout][taps][Cin] (kernel K-order) and the frozen affine
 * scale s[Cout] (may be NULL = 1) -> operand copies in `dtype`:
 *   w_fprop[Cout][taps][Cin] = W*s          (B operand of FPROP)
 *   w_dgrad[Cin][taps][Cout] = W*s          (B operand of DGRAD; may be NULL)
 * Folding the frozen scale is exact algebra: affine(conv(x,W)) = conv(x, W*s) + b
 * (affine_nd_op.cu:31-44 has no gradient for s, affine_nd_op.cc:45-53). */
int vlfb_weight_prep(const float* w, const float* scale, void* w_fprop, void* w_dgrad, int dtype,
                     int64_t cout, int64_t taps, int64_t cin, vlfb_stream_t stream);

/* The same for every convolution of the model in ONE launch.  `items_dev` is a device array sorted
 * by tile_begin; item i owns tiles [tile_begin, tile_begin + taps*ceil(cout/32)*ceil(cin/32)). */
typedef struct vlfb_wprep_item {
  const void* w;        /* fp32 master [cout][taps][cin] */
  const void* scale;    /* fp32 [cout] or NULL */
  void* w_fprop;        /* dtype [cout][taps][cin] or NULL */
  void* w_dgrad;        /* dtype [cin][taps][cout] or NULL */
  int32_t cout, taps, cin;
  int32_t tile_begin;
} vlfb_wprep_item;
int vlfb_weight_prep_batched(const vlfb_wprep_item* items_dev, int n_items, int total_tiles,
                             int dtype, vlfb_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Pools (channels-last).  Replace Caffe2 MaxPool / AveragePool:
 * resnet_video.py:190,219; nonlocal_helper.py:49; head_helper.py:37,92,113; lfb_helper.py:112,124.
 * ------------------------------------------------------------------------------------------ */
typedef struct vlfb_pool_desc {
  int32_t dtype;
  int32_t N, Ti, Hi, Wi, C;
  int32_t To, Ho, Wo;
  int32_t kt, kh, kw, st, sh, sw, pt, ph, pw;
} vlfb_pool_desc;
/* Every pool entry point checks the descriptor against itself before anything is launched (VLFB_ERR_ARG, the message names
 * the dimension t / h / w): extents, kernels and strides positive; 0 <= pad < kernel; for max pools the last window has a tap
 * inside the input, (To-1)*st - pt <= Ti-1; for average pools (pad 0) it lies inside the input, (To-1)*st + kt <= Ti. */
/* bytes per arg-max element: 1 (window <= 255 taps) or 2 (the FBO-max head pools 300 bank rows) */
int vlfb_pool_argmax_bytes(const vlfb_pool_desc* d);
/* y[N,To,Ho,Wo,C]; argmax (tap index inside the window, first maximum in t,h,w scan order; element
 * size = vlfb_pool_argmax_bytes) may be NULL in inference. */
int vlfb_maxpool_fwd(const vlfb_pool_desc* d, const void* x, void* y, void* argmax,
                     vlfb_stream_t stream);
/* dx = (accumulate ? add : 0) + scatter(dy) ; then dx = (mask > 0) ? dx : 0 when mask != NULL.
 * `add` may alias dx. Gather formulation: deterministic, no atomics. */
int vlfb_maxpool_bwd(const vlfb_pool_desc* d, const void* dy, const void* argmax, void* dx,
                     const void* add, const void* mask, vlfb_stream_t stream);
/* The same backward for a max-pool whose INPUT is a ReLU output and has no other consumer (pool1 after conv1, pool2
 * after res2: resnet_video.py:183-194, 229-236): the selected element is the pooled value itself, so the ReLU mask
 * of the input is `y > 0` read at the window's output position -- bit-identical to vlfb_maxpool_bwd(mask = x) and
 * kt*kh*kw / (st*sh*sw) times less mask traffic. */
int vlfb_maxpool_relu_bwd(const vlfb_pool_desc* d, const void* dy, const void* argmax, const void* y, void* dx,
                          vlfb_stream_t stream);
/* Which kernel vlfb_maxpool_bwd (has_y = 0) / vlfb_maxpool_relu_bwd (has_y = 1, has_add = has_mask = 0) runs for this
 * descriptor, as text in `buf` (at least 64 bytes); launches nothing and needs no GPU.  The launch code switches on the same
 * decision, so the route a test names is the route that runs.  The rule, in this order:
 *   1. a two-byte arg-max (window > 255 taps), or >= 2^31 input rows (N*Ti*Hi) or pooled positions: "generic u16 bf16" / "generic u8 bf16"
 *   2. window 1x3x3, stride 1x2x2, pt = 0, To = Ti, neither add nor mask: with row_bytes = Wo * C * (element bytes + 1) and
 *      R = min(3, 65536 / row_bytes - 2), when R >= 2 the band kernel (2R input rows per workgroup, R + 2 pooled rows in LDS,
 *      bands = ceil(Hi / 2R) workgroups per frame): "band f16 R=3 bands=5"
 *   3. window / stride 1x3x3 / 1x2x2, 2x1x1 / 2x1x1 or 1x2x2 / 1x2x2 (any pads): the row kernel compiled for that window,
 *      "fixed 1x3x3/1x2x2 f32"
 *   4. anything else: "generic u8 f32"
 * " ymask" is appended when has_y.  All routes give identical bits: the same fp32 sum over the covering windows in ascending
 * (to, ho, wo) order, then add, then mask, then one rounding.  The descriptor is checked as by vlfb_maxpool_bwd. */
int vlfb_maxpool_bwd_describe(const vlfb_pool_desc* d, int has_add, int has_mask, int has_y, char* buf, int64_t buf_bytes);
/* A two-plane FPROP launch (math VLFB_MATH_F16X3, out_dtype VLFB_F16) and the max-pool behind it in ONE launch, for a conv
 * output that nothing but the pool reads (pool2 behind res2's last conv: resnet_video.py:229-236): the epilogue forms the two
 * planes every output row would have stored, takes the window maximum on hi + lo with a strict > in tap order -- what
 * vlfb_maxpool_fwd does on the stored planes -- and stores only the pooled planes and the arg-max bytes; the un-pooled
 * tensor is never written.  `d` and `pool` are the unchanged descriptors of the two separate launches; a->O / a->O_lo are the
 * POOLED planes (y and y + numel of vlfb_maxpool_fwd), every other operand is what vlfb_conv_run_args takes (no Mask, P,
 * O_planes, dbias); argmax as vlfb_maxpool_fwd, NULL in inference.  Bit-identical to vlfb_conv_run_args followed by
 * vlfb_maxpool_fwd.  Implemented: the temporal pool (2x1x1, stride 2x1x1, no padding) behind a plain-row conv that plans
 * on the 128 x 128 two-plane kernel with prefetched residual rows ("nt_pair f16x3 128x128 pre"); any frame size, odd frame
 * counts (the last frame has no window and is not computed), ragged column tiles.  Any other pair of descriptors is
 * VLFB_ERR_UNSUPPORTED before anything is launched; vlfb_conv_maxpool_fusable answers the same question (1 / 0) at plan
 * time. */
int vlfb_conv_maxpool_fusable(const vlfb_conv_desc* d, const vlfb_pool_desc* pool);
int vlfb_conv_run_maxpool(const vlfb_conv_desc* d, const vlfb_pool_desc* pool, const vlfb_conv_args* a, void* argmax,
                          vlfb_stream_t stream);
/* average over the window (pad 0 only, as every AveragePool in the reference) */
int vlfb_avgpool_fwd(const vlfb_pool_desc* d, const void* x, void* y, vlfb_stream_t stream);
int vlfb_avgpool_bwd(const vlfb_pool_desc* d, const void* dy, void* dx, const void* add,
                     const void* mask, vlfb_stream_t stream);

/* The average-pool backward from an fp32 pooled gradient dy into a TWO-TERM 16-bit input gradient (d->dtype = VLFB_F16 /
 * VLFB_BF16): dx = (mask > 0 ? sum dy / window : 0), dx_hi = round(dx), dx_lo = round(dx - dx_hi) -- see vlfb_conv_args.O_lo.
 * Where the "mix" path's fp32 head gradient (head_helper.py:37-40, 92-98: the pools over res5) re-enters the 16-bit backward:
 * every position of a channel receives the same value, so a one-term rounding is an error common to all positions. */
int vlfb_avgpool_bwd_two_term(const vlfb_pool_desc* d, const float* dy, void* dx_hi, void* dx_lo, const void* mask,
                              vlfb_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Row softmax with pre-scale: P[r][:] = softmax(scale * S[r][:]).
 * Replaces Scale + Softmax(axis=2, engine=CUDNN): nonlocal_helper.py:98-104, lfb_helper.py:227-230.
 * S is fp32 (the affinity is kept in fp32 on both paths); P is `dtype`.
 * bwd: dS[r][:] = scale * P .* (dP - sum(dP .* P)), dP fp32, dS `dtype`.
 * ------------------------------------------------------------------------------------------ */
int vlfb_softmax_fwd(const float* s, void* p, int dtype, int64_t rows, int64_t cols, float scale,
                     vlfb_stream_t stream);
int vlfb_softmax_bwd(const float* dp, const void* p, void* ds, int dtype, int64_t rows,
                     int64_t cols, float scale, vlfb_stream_t stream);
/* bwd with the probabilities in fp32 and ds in a 16-bit type (cols % 4 == 0, cols <= 2048): the "mix" path */
int vlfb_softmax_bwd_p32(const float* dp, const float* p, void* ds, int ds_dtype, int64_t rows, int64_t cols,
                         float scale, vlfb_stream_t stream);
/* The same two operators FUSED with the batched product that feeds them (nonlocal_helper.py:94-121), so the fp32
 * score matrix never exists in memory:
 *   fwd:  prob[b][l1][l2] = softmax_l2(scale * sum_c theta[b][l1][c] * phi[b][l2][c])
 *   bwd:  ds[b][l1][l2]   = scale * prob o (dP - sum_l2(dP o prob)),  dP = sum_c dy[b][l1][c] * g[b][l2][c]
 * operands / outputs are `dtype` (16-bit types only), row-major as indexed above.  Supported shapes:
 * 512 <= l2 <= 1024 with l2 % 8 == 0, 64 <= ci <= 1024 with ci % 64 == 0, l1 >= 64, and l1 * ci < 2^30 and
 * l1 * l2 < 2^30 (32-bit element offsets inside one batch entry); otherwise VLFB_ERR_UNSUPPORTED and the caller
 * composes vlfb_conv_run + vlfb_softmax_*.  scale must be > 0 (a kernel takes the row maximum before scaling); any
 * other value is VLFB_ERR_ARG.  Both refusals come back before anything is launched.  vlfb_attn_scores_supported returns 0 or a mask of the flags below: whether the
 * shape can run at all, and for which direction the fused kernel was MEASURED faster than the composed one on
 * MI355X (the engine fuses a direction only then). */
enum { VLFB_ATTN_CAN_RUN = 1, VLFB_ATTN_FWD_FASTER = 2, VLFB_ATTN_BWD_FASTER = 4 };
int vlfb_attn_scores_supported(int dtype, int64_t l1, int64_t l2, int64_t ci);
int vlfb_attn_scores_fwd(const void* theta, const void* phi, void* prob, int dtype, int64_t batch, int64_t l1,
                         int64_t l2, int64_t ci, float scale, vlfb_stream_t stream);
int vlfb_attn_scores_bwd(const void* dy, const void* g, const void* prob, void* ds, int dtype, int64_t batch,
                         int64_t l1, int64_t l2, int64_t ci, float scale, vlfb_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Small elementwise / reduction ops (rows x cols matrices of `dtype`, cols contiguous).
 * ------------------------------------------------------------------------------------------ */
/* y = a + b (optionally relu, optionally masked by mask>0); any of y,a,b may alias.  b may be NULL (y = a).
 * n == 0 is a no-op that returns VLFB_OK, here and in vlfb_relu_fwd / vlfb_relu_bwd (like the movers vlfb_cast,
 * vlfb_zero_f32, vlfb_half_copy: an empty activation is not an error); the solver-side ops (vlfb_sgd_update*,
 * vlfb_scale_inplace, vlfb_dropout_bwd) reject n == 0, an empty parameter bucket being a planning bug.
 * Replaces Sum (+Relu): resnet_helper.py:112-117; nonlocal_helper.py:170,201; lfb_helper.py:286 */
int vlfb_add(const void* a, const void* b, void* y, const void* mask, int dtype, int64_t n,
             int relu, vlfb_stream_t stream);
/* y = relu(x); dx = (y>0) ? dy : 0  (model_builder_video.py:169-174) */
int vlfb_relu_fwd(const void* x, void* y, int dtype, int64_t n, vlfb_stream_t stream);
int vlfb_relu_bwd(const void* dy, const void* y, void* dx, int dtype, int64_t n,
                  vlfb_stream_t stream);
/* colsum[c] (+)= sum_r g[r][c] -- bias gradients of the convs that carry a bias
 * (nonlocal_helper.py:36-77, lfb_helper.py:175-200, resnet_video.py:327).  Row slabs are folded with fp32 atomics (no scratch
 * argument): not bit-reproducible.  The engine takes its bias gradients from vlfb_conv_run_wgrad_bias, which is.
 * cols and ld must be multiples of the 16-byte vector (4 fp32 / 8 16-bit elements); ld >= cols.  A rejected call launches
 * nothing: `out` keeps its contents. */
int vlfb_colsum(const void* g, int dtype, int64_t rows, int64_t cols, int64_t ld, float* out,
                int accumulate, vlfb_stream_t stream);
/* ------------------------------------------------------------------------------------------
 * SpatialBN over channels-last rows x[rows][C] -- the graphs built with MODEL.USE_AFFINE False / NONLOCAL.USE_BN True
 * (model_builder_video.py:176-197 Conv3dBN, resnet_video.py:185-188, nonlocal_helper.py:146-155).  The operator is
 * Caffe2's spatial_batch_norm_op (a dependency, not in the reference tree); its algorithm:
 *   train (is_test = 0): mu / var = biased row moments; y = (x - mu) / sqrt(var + eps) * gamma + beta;
 *          running_mean = momentum * running_mean + (1 - momentum) * mu,
 *          running_var  = momentum * running_var  + (1 - momentum) * var * rows / (rows - 1);
 *          save_mean / save_inv_std [C] are kept for the backward pass
 *   test  (is_test = 1): y = (x - running_mean) / sqrt(running_var + eps) * gamma + beta; nothing else is written
 *   bwd:   dbeta = sum dy, dgamma = sum dy * xhat (each times grad_scale; either may be NULL),
 *          dx = gamma * inv_std * (dy - dbeta / rows - xhat * dgamma / rows)   (NULL: parameter gradients only)
 * Per-GPU statistics, as in the reference's data-parallel model.  Reductions are two-stage and ordered (no atomics).
 * x may alias y, dy may alias dx.  workspace: vlfb_bn_workspace_bytes (fp32 slab partials + coefficient rows).
 * ------------------------------------------------------------------------------------------ */
int64_t vlfb_bn_workspace_bytes(int dtype, int64_t rows, int64_t C);
int vlfb_bn_fwd(const void* x, void* y, const float* gamma, const float* beta, float* running_mean,
                float* running_var, float* save_mean, float* save_inv_std, void* workspace,
                int64_t workspace_bytes, int dtype, int64_t rows, int64_t C, float eps, float momentum,
                int is_test, vlfb_stream_t stream);
int vlfb_bn_bwd(const void* dy, const void* x, const float* gamma, const float* save_mean,
                const float* save_inv_std, void* dx, float* dgamma, float* dbeta, void* workspace,
                int64_t workspace_bytes, int dtype, int64_t rows, int64_t C, float grad_scale,
                vlfb_stream_t stream);

/* SpatialBN of the "mix" path: the same operator on VALUES in the format `xf` -- VLFB_F16PAIR (two fp16 planes, hi at x and lo
 * rows * C elements behind it; C % 8 == 0) or VLFB_F32 (C % 4 == 0) -- with the residual Sum and the ReLU behind the BN in
 * its apply pass, and a backward on the gradients the mix backward carries.
 *   fwd: the moments are those of v = hi + lo (fp32 slab partials about the row-0 pivot, finished in double); training
 *        (is_test = 0) writes save_mean / save_inv_std and updates the running statistics exactly as vlfb_bn_fwd does,
 *        is_test = 1 folds the running statistics and writes nothing but y.
 *        y = a[c] * v + b[c], + residual (NULL: none; format xf, both planes), then max(., 0) when relu != 0; y has the format
 *        of x.  A pair is written canonical: hi = fp16(y) and fp16(hi + lo) == hi (lo = fp16(y - hi), one fp16 step
 *        nearer zero where its rounding would tie hi + lo away from hi), so the hi plane is the fp16 copy of the values and,
 *        behind a ReLU, its mask (lo == 0 wherever hi == 0).
 *   bwd: x in format xf (both planes are read: xhat = ((hi - mean) + lo) * inv_std); the gradient operand has the type
 *        gt = VLFB_F16 or VLFB_F32, and with VLFB_F16 an optional low term dy_lo (NULL: none): g = dy + dy_lo.  Sums in fp32
 *        slab partials, finished in double; dgamma / dbeta fp32, times grad_scale (either may be NULL); dx in type gt (one
 *        term; NULL: parameter gradients only).  No masking: dy is the finished (already masked) output gradient.
 * y may alias x or residual, dx may alias dy.  workspace: vlfb_bn_mix_workspace_bytes(xf, rows, C) bytes (-1: bad arguments).
 * Ordered two-stage reductions, no atomics: two runs give the same bits. */
int64_t vlfb_bn_mix_workspace_bytes(int xf, int64_t rows, int64_t C);
int vlfb_bn_fwd_mix(const void* x, void* y, const void* residual, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, float* save_mean, float* save_inv_std, void* workspace,
                    int64_t workspace_bytes, int xf, int64_t rows, int64_t C, float eps, float momentum, int is_test,
                    int relu, vlfb_stream_t stream);
int vlfb_bn_bwd_mix(const void* dy, const void* dy_lo, const void* x, const float* gamma, const float* save_mean,
                    const float* save_inv_std, void* dx, float* dgamma, float* dbeta, void* workspace,
                    int64_t workspace_bytes, int xf, int gt, int64_t rows, int64_t C, float grad_scale,
                    vlfb_stream_t stream);

/* Precise BN (lib/utils/bn_helper.py): before a checkpoint or an evaluation the running statistics of every SpatialBN
 * layer are replaced by the average of the batch statistics of a number of training batches.  All three entry points
 * read one layer table in DEVICE memory, `layers` records of vlfb_bn_layer; a layer's channels occupy
 * [offset, offset + C) of the packed fp32 accumulators.  One workgroup per layer (grid-stride over the layers), one
 * thread per channel (block-stride over C): the offsets are not known on the host, and nothing but `layers` is.
 *   accumulate: per (layer, channel), fp32, unfused (bn_helper.py:170-182):
 *                 r = 1 / save_inv_std; var = r * r - eps; m2 = var + save_mean * save_mean;
 *                 sum_mean += save_mean; sum_mean2 += m2              (divisions are correctly rounded)
 *   finalize:   in place, mean = sum_mean / float(normalize); m2 = sum_mean2 / float(normalize); var = m2 - mean * mean;
 *               sum_mean <- mean, sum_mean2 <- var (bn_helper.py:187-198).  *bad (int32, device memory) is SET to the
 *               number of channels whose var is not > 0 (NaN included): zeroed on the stream, then integer atomic adds.
 *               The running statistics are not touched: the reference asserts var > 0 before it writes anything.
 *   update:     running_mean <- mean[offset ...], running_var <- var[offset ...] of every layer (bn_helper.py:200-221:
 *               the "riv" blob is the running VARIANCE).  May be repeated.
 * VLFB_ERR_ARG before anything is launched: layers <= 0, normalize <= 0, a NULL table / accumulator / bad.
 * ------------------------------------------------------------------------------------------ */
typedef struct vlfb_bn_layer {
  const float* save_mean;      /* [C] batch mean of the last training forward */
  const float* save_inv_std;   /* [C] 1 / sqrt(batch var + eps) */
  float* running_mean;         /* [C] */
  float* running_var;          /* [C] */
  int64_t offset;              /* first element of the layer in the packed accumulators */
  int32_t C;
  int32_t reserved;
} vlfb_bn_layer;
#define VLFB_BN_LAYER_BYTES 48
int vlfb_bn_precise_accumulate(const vlfb_bn_layer* table, int layers, float eps, float* sum_mean, float* sum_mean2,
                               vlfb_stream_t stream);
int vlfb_bn_precise_finalize(const vlfb_bn_layer* table, int layers, int normalize, float* sum_mean, float* sum_mean2,
                             int32_t* bad, vlfb_stream_t stream);
int vlfb_bn_precise_update(const vlfb_bn_layer* table, int layers, const float* mean, const float* var,
                           vlfb_stream_t stream);

/* LayerNorm over each row, no learnable scale/bias, eps inside sqrt (lfb_helper.py:160-166,
 * 252-256; Caffe2 LayerNorm axis=1).  rstd[r] = 1/sqrt(var+eps) saved for backward. */
int vlfb_layernorm_fwd(const void* x, void* y, float* rstd, int dtype, int64_t rows, int64_t cols,
                       float eps, vlfb_stream_t stream);
int vlfb_layernorm_bwd(const void* dy, const void* y, const float* rstd, void* dx, int dtype,
                       int64_t rows, int64_t cols, vlfb_stream_t stream);
/* Dropout (lfb_helper.py:259,314,334; resnet_video.py:323): counter-based mask
 * keep(i) = u(seed, i) >= ratio with u from vlfb's mix32 generator over the REFERENCE-layout
 * linear index i; y = keep ? x/(1-ratio) : 0.  The mask is written as bytes for backward.
 * Logical tensor is (rows, ch, inner) in reference order [(r*ch + c)*inner + k] while the
 * data is stored [(r*inner + k)*ch + c] (channels-last). */
int vlfb_dropout_fwd(const void* x, void* y, uint8_t* mask, int dtype, int64_t rows, int64_t inner,
                     int64_t ch, float ratio, uint64_t seed, vlfb_stream_t stream);
/* the same with the seed read from device memory at run time: a step captured in a HIP graph replays
 * the same launch packet every iteration, so per-iteration values cannot be kernel arguments */
int vlfb_dropout_fwd_dev(const void* x, void* y, uint8_t* mask, int dtype, int64_t rows, int64_t inner,
                         int64_t ch, float ratio, const uint64_t* seed_dev, vlfb_stream_t stream);
int vlfb_dropout_bwd(const void* dy, const uint8_t* mask, void* dx, int dtype, int64_t n,
                     float ratio, vlfb_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * FC + loss.  Replace FC, Sigmoid, SigmoidCrossEntropyLoss (resnet_video.py:327-338).
 * ------------------------------------------------------------------------------------------ */
/* logits[r][k] = sum_c x[r][c] * w[k][c] + b[k]; x `dtype`, w/b fp32 master, logits fp32 */
int vlfb_fc_fwd(const void* x, int dtype, const float* w, const float* b, float* logits,
                int64_t rows, int64_t cin, int64_t cout, vlfb_stream_t stream);
/* dx[r][c] = sum_k dl[r][k]*w[k][c] ; dw[k][c] (+)= sum_r dl[r][k]*x[r][c]; db[k] (+)= sum_r dl */
int vlfb_fc_bwd(const void* x, int dtype, const float* w, const float* dlogits, void* dx,
                float* dw, float* db, int64_t rows, int64_t cin, int64_t cout, int accumulate,
                vlfb_stream_t stream);
/* prob = sigmoid(logits); loss = scale * sum(l) / max(#(t>=0),1) with
 * l = -x*(t - (x>=0)) + log(1 + exp(x - 2x*(x>=0))), t in {0,1} (or -1 = ignore);
 * dlogits = scale * (prob - t) / normalizer (0 where ignored).  loss: 1 float. */
int vlfb_sigmoid_ce(const float* logits, const int32_t* labels, float* prob, float* loss,
                    float* dlogits, int64_t rows, int64_t cols, float scale, vlfb_stream_t stream);
/* Single-label heads (EPIC-Kitchens; Softmax / SoftmaxWithLoss, resnet_video.py:339-347): prob = softmax over
 * `cols`; with labels [rows] (class indices): loss = scale * sum_r -log(max(prob[r][label_r], 1e-20)) / rows and
 * dlogits = scale * (prob - onehot) / rows (Caffe2 SoftmaxWithLoss without weights).  labels NULL = test mode. */
int vlfb_softmax_ce(const float* logits, const int32_t* labels, float* prob, float* loss, float* dlogits,
                    int64_t rows, int64_t cols, float scale, vlfb_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * RoI head.  Replaces RoIAlign + 7x7 MaxPool (head_helper.py:88-123, lfb_helper.py:130-152).
 * feat: [N,H,W,C] channels-last `dtype`; rois: fp32 (R,5) = [batch_idx, x1,y1,x2,y2];
 * out: [R,C] = max over the pooled x pooled RoIAlign bins; argbin: uint8 [R,C].
 * argbin is the FIRST maximal bin in row-major bin order (bin = ph * pooled + pw): bins are accumulated in fp32 (from the
 * 16-bit values too) in the operator's sample / corner order and compared with a strict >, within a group of pooled rows and
 * again when the groups are folded, so equal maxima -- channels that are zero over a whole RoI, bins whose samples all
 * clamp to the same border pixel -- resolve as a serial scan does, whatever the channel count.  A RoI with no sample
 * inside the map gives out = 0, argbin = 0.  Every batch index must lie in [0, n): it is not checked.
 * Rejected without launching anything (VLFB_ERR_ARG): c not a multiple of the 16-byte vector (4 fp32 / 8 16-bit
 * elements), more than 1024 such vectors per row, pooled * pooled > 255, r <= 0, an unknown dtype.
 * dbg (optional, int32 [R][pooled][pooled][8]) receives the integer decisions of the first
 * sample of every bin: {batch, grid_h, grid_w, y_low, x_low, y_high, x_high, inside}.
 * ------------------------------------------------------------------------------------------ */
int vlfb_roi_align_max_fwd(const void* feat, int dtype, const float* rois, void* out,
                           uint8_t* argbin, int32_t* dbg, int64_t n, int64_t h, int64_t w,
                           int64_t c, int64_t r, int pooled, float spatial_scale,
                           vlfb_stream_t stream);
/* Test hook: the integer decisions of EVERY bilinear sample of every bin, from the same device functions the operator
 * uses: dbg int32 [R][pooled][pooled][max_grid][max_grid][8] = {batch, grid_h, grid_w, y_low, x_low, y_high, x_high,
 * inside}; samples beyond the RoI's adaptive grid carry {.., -2, -2, -2, -2, -1}. */
int vlfb_roi_align_decisions(const float* rois, int32_t* dbg, int64_t h, int64_t w, int64_t r, int pooled,
                             float spatial_scale, int max_grid, vlfb_stream_t stream);
/* dfeat (fp32 [N,H,W,C], must be zeroed by the caller) += scatter of dout through argbin.  Deterministic: one thread owns a
 * (clip, channel) column and adds its RoIs' contributions in RoI / sample / corner order (the reference operator scatters
 * with atomics, whose order -- overlapping RoIs of a clip -- varies from run to run). */
int vlfb_roi_align_max_bwd(const void* dout, int dtype, const float* rois, const uint8_t* argbin,
                           float* dfeat, int64_t n, int64_t h, int64_t w, int64_t c, int64_t r,
                           int pooled, float spatial_scale, vlfb_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * FBO-NL attention core for one query per row (lfb_helper.py:170-263, num_feat1 == 1):
 *   aff[r][k] = scale * <theta[r], phi[r][k]>, p = softmax_k(aff), t[r] = sum_k p[r][k] g[r][k].
 * theta [R][D], phi/g [R][K][D] (row stride ld), p fp32 [R][K], t [R][D].
 * ------------------------------------------------------------------------------------------ */
int vlfb_fbo_attn_fwd(const void* theta, const void* phi, const void* g, float* p, void* t,
                      int dtype, int64_t r, int64_t k, int64_t d, int64_t ld, float scale,
                      vlfb_stream_t stream);
/* The same with SHARED banks (inference: tools/lfb_loader.py, tools/test_net.py): the data layer hands every RoI a COPY of its
 * clip's bank (lib/datasets/ava_data_input.py:191-192) and the graph projects each copy (lib/models/lfb_helper.py:320-338);
 * without dropout the projected banks of a clip's RoIs are identical, so phi / g are computed ONCE per clip -- [n_banks][K][D]
 * -- and row r attends to bank (int)owner[r * owner_stride] (the batch-index column of the `proposals` blob: owner = rois,
 * owner_stride = 5).  Same arithmetic per row as vlfb_fbo_attn_fwd on the duplicated banks: bit-identical outputs. */
int vlfb_fbo_attn_fwd_shared(const void* theta, const void* phi, const void* g, float* p, void* t,
                             int dtype, int64_t r, int64_t k, int64_t d, int64_t ld, float scale,
                             const float* owner, int64_t owner_stride, vlfb_stream_t stream);
/* ds_ws: fp32 scratch of r*k elements (the softmax-input gradient handed from the per-row
 * kernel to the chip-wide dphi/dg writer) */
int vlfb_fbo_attn_bwd(const void* dt, const void* theta, const void* phi, const void* g,
                      const float* p, void* dtheta, void* dphi, void* dg, float* ds_ws, int dtype,
                      int64_t r, int64_t k, int64_t d, int64_t ld, float scale, vlfb_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Solver.  Replaces WeightedSum + MomentumSGDUpdate(nesterov) per parameter
 * (model_builder_video.py:348-389) with one pass over a flat fp32 bucket:
 *   g += wd*p ; m' = mu*m + lr*g ; p -= (1+mu)*m' - mu*m   (nesterov)  |  p -= m' (plain)
 * ------------------------------------------------------------------------------------------ */
int vlfb_sgd_update(float* p, float* g, float* m, int64_t n, float lr, float wd, float mu,
                    int nesterov, vlfb_stream_t stream);
/* learning rate read from device memory (captured steps, see vlfb_dropout_fwd_dev) */
int vlfb_sgd_update_dev(float* p, float* g, float* m, int64_t n, const float* lr_dev, float wd, float mu,
                        int nesterov, vlfb_stream_t stream);
/* dst[i] = values[i], i < n <= 8, in stream order; the values are copied into the launch packet before the
 * call returns (per-iteration scalars of a captured step: learning rate bits, dropout seeds) */
int vlfb_store_scalars(uint64_t* dst, int n, const uint64_t* values, vlfb_stream_t stream);
int vlfb_scale_inplace(float* x, int64_t n, float s, vlfb_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Long-term feature bank resident on the device.
 * Replaces the host dict-of-lists bank of tools/lfb_loader.py:49-112 (construct_ava_lfb,
 * construct_frame_level_lfb) and the per-clip NumPy sampling of lib/datasets/ava.py:300-323 and
 * lib/datasets/charades.py:251-276.
 *   bank  [n_videos][n_steps][capacity][dim]  elements of `dtype`, caller-owned
 *   count [n_videos][n_steps] int32, caller-owned, zero = empty
 * AVA: step = second (minus a base), capacity = most boxes kept per second.
 * Charades: step = LFB frame slot, capacity = 1.
 * ------------------------------------------------------------------------------------------ */
typedef struct vlfb_lfb_desc {
  int32_t n_videos, n_steps, capacity, dim;
  int32_t dtype;
  int32_t step_base;   /* reference time key of step 0 (AVA seconds start at 902); only the sampling
                          draw depends on it, so that it is a function of the reference's own keys */
} vlfb_lfb_desc;
int64_t vlfb_lfb_bank_bytes(const vlfb_lfb_desc* d);
/* Append `rows` features (feats [rows][dim] of feat_dtype) under keys [rows][2] = {video, step}.
 * Rows of the same key keep their batch order behind what the bank already holds (list.append of
 * lfb_loader.py:100-104); rows with video < 0 are padding and skipped; rows that do not fit
 * (bad key / cell full) are counted in *dropped (optional device int32). */
int vlfb_lfb_append(const vlfb_lfb_desc* d, void* bank, int32_t* count, const void* feats,
                    int feat_dtype, const int32_t* keys, int64_t rows, int32_t* dropped,
                    vlfb_stream_t stream);
/* AVA window sampling (ava.py:300-323): query [rows][3] = {video, centre step, sample id};
 * out [rows][window*max_per_step][dim]; time slot j holds min(n, max_per_step) distinct features
 * of step centre - window/2 + j in random order, zeros elsewhere.  The draw is a pure function of
 * (seed, sample id, video, step): rows sharing a sample id get the same features (the reference
 * repeats the clip's sample for each of its RoIs, ava_data_input.py:191-192). */
int vlfb_lfb_sample_window(const vlfb_lfb_desc* d, const void* bank, const int32_t* count,
                           const int32_t* query, int64_t rows, int window, int max_per_step,
                           uint64_t seed, void* out, int out_dtype, vlfb_stream_t stream);
/* The AVA window from a HOST-DRAWN table (stream-equal with the reference: the host makes the np.random.choice calls of
 * ava.py:316-318, the device gathers): query [rows][2] = {video, centre step}; table [rows][window][max_per_step] = slot of
 * step (centre - window/2 + j) that becomes output row j*max_per_step + k, or -1 for zeros. */
int vlfb_lfb_gather_slots(const vlfb_lfb_desc* d, const void* bank, const int32_t* count, const int32_t* query,
                          const int32_t* table, int64_t rows, int window, int max_per_step, void* out, int out_dtype,
                          vlfb_stream_t stream);
/* Frame-level sampling (charades.py:251-276): query [rows][3] = {video, first step, last step};
 * out [rows][window][dim] = the first `window` occupied steps of [first, last] packed to the
 * front, zeros behind. */
int vlfb_lfb_sample_compact(const vlfb_lfb_desc* d, const void* bank, const int32_t* count,
                            const int32_t* query, int64_t rows, int window, void* out,
                            int out_dtype, vlfb_stream_t stream);
/* The same with up to `max_per_step` features per step (slot order), packed in step order until `window`
 * rows are filled: EPIC-Kitchens verb banks (one clip feature per step, lib/datasets/epic.py:310-331,
 * max_per_step = 1) and noun banks (detector features per frame, epic.py:338-374, max_per_step =
 * EPIC.MAX_NUM_FEATS_PER_NOUN_LFB_FRAME). */
int vlfb_lfb_sample_packed(const vlfb_lfb_desc* d, const void* bank, const int32_t* count,
                           const int32_t* query, int64_t rows, int window, int max_per_step, void* out,
                           int out_dtype, vlfb_stream_t stream);
/* Packed export: the occupied rows of the bank in cell order (video-major, then step), inside a cell in slot order
 * (= append order), so that writing, loading and merging a bank touch only what it holds.
 * offsets int64 [cells + 1], cells = n_videos * n_steps: offsets[c] = sum over cells before c (video-major, then step)
 * of min(count, capacity); offsets[cells] = the number of features in the bank.  Integer scan, fixed order, no atomics.
 * Two levels: tiles of VLFB_LFB_PACK_TILE cells scanned in LDS, one workgroup scans the tile totals (kept in `offsets`
 * itself, no workspace), an add-back.  That covers cells <= VLFB_LFB_PACK_MAX_CELLS = TILE * TILE; more is VLFB_ERR_ARG
 * (the AVA train bank has 235 * 900 = 211500 cells). */
#define VLFB_LFB_PACK_TILE 1024
#define VLFB_LFB_PACK_MAX_CELLS (VLFB_LFB_PACK_TILE * VLFB_LFB_PACK_TILE)
int vlfb_lfb_pack_offsets(const vlfb_lfb_desc* d, const int32_t* count, int64_t* offsets, vlfb_stream_t stream);
/* rows [first_row, first_row + rows) of the packed order (cell order, then slot order = append order) -> out [rows][dim] of
 * out_dtype and keys [rows][2] = {video, step}: exactly what vlfb_lfb_append takes, so a packed chunk appended to an
 * empty bank of the same geometry reproduces these cells bit for bit.  Rows at or beyond offsets[cells] are not written.
 * `offsets` is what vlfb_lfb_pack_offsets wrote for the same `count`, earlier on the same stream; 0 <= rows < 2^20 per
 * call as for vlfb_lfb_append, first_row >= 0. */
int vlfb_lfb_pack(const vlfb_lfb_desc* d, const void* bank, const int32_t* count, const int64_t* offsets,
                  int64_t first_row, int64_t rows, void* out, int out_dtype, int32_t* keys, vlfb_stream_t stream);
/* Packed import, the inverse of vlfb_lfb_pack: rows [first_row, first_row + rows) of a SOURCE bank's packed order, feats
 * [rows][dim] of feat_dtype (any of the three types), are placed into this bank without keys.  The source has this bank's
 * n_videos, n_steps and dim; its capacity is src_capacity; src_count int32 [cells] is its count and src_offsets int64
 * [cells + 1] what vlfb_lfb_pack_offsets wrote for src_count.  Packed row g lies in the cell c with src_offsets[c] <= g <
 * src_offsets[c + 1], at local slot s = g - src_offsets[c], and goes to slot count[c] + s.  A row whose slot is >= capacity
 * is not written and counted in *dropped (optional device int32); rows at or beyond src_offsets[cells] are ignored; where
 * src_offsets do not belong to src_count (s >= min(src_count[c], src_capacity)) nothing is written.  One workgroup per row,
 * no atomics but *dropped: the result does not depend on the order workgroups run in.
 * Ordering contract, per source: vlfb_lfb_unpack READS count and never writes it, so every chunk of one source is placed
 * against the same base, in any chunking (chunks may begin and end inside a cell); after the source's LAST chunk, on the
 * same stream, vlfb_lfb_unpack_commit publishes it ONCE: count[c] = min(count[c] + min(src_count[c], src_capacity),
 * capacity).  The next source's chunks come after that commit.  Unpacking every source this way gives count and occupied
 * slots bit-identical to vlfb_lfb_append of the same packed chunks with their keys.  Limits as vlfb_lfb_pack: cells <=
 * VLFB_LFB_PACK_MAX_CELLS, 0 <= rows < 2^20 per call, first_row >= 0. */
int vlfb_lfb_unpack(const vlfb_lfb_desc* d, void* bank, const int32_t* count, const void* feats, int feat_dtype,
                    const int32_t* src_count, int src_capacity, const int64_t* src_offsets, int64_t first_row, int64_t rows,
                    int32_t* dropped, vlfb_stream_t stream);
int vlfb_lfb_unpack_commit(const vlfb_lfb_desc* d, int32_t* count, const int32_t* src_count, int src_capacity,
                           vlfb_stream_t stream);
/* Non-finite rows of a finished bank, counted where the bank lives (an inference pass has no loss to guard it: on the
 * 16-bit paths an activation above the format's range becomes Inf or NaN silently, and such a row poisons every training
 * step that samples it).  An occupied row is slot < min(count[cell], capacity) of a cell.  ADDS into out[0] the number of
 * occupied rows with at least one NaN or +-Inf element and into out[1] the number of occupied rows examined (int64 [2]
 * in device memory, caller-zeroed).  Unoccupied slots are not read.  Integer adds only: the result does not depend on the
 * launch geometry.  Rows whose byte length and address are multiples of 16 are read with 16-byte loads. */
int vlfb_lfb_count_nonfinite(const vlfb_lfb_desc* d, const void* bank, const int32_t* count, int64_t* out /* [2] */,
                             vlfb_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Clip preprocessing on the device.  Replaces the per-frame cv2 / NumPy chain of
 * lib/datasets/data_input_helper.py:70-139 (images_and_boxes_preprocessing) with one kernel:
 * uint8 BGR frames [frames][src_h][src_w][3] -> bilinear resize to resized_h x resized_w (OpenCV's
 * 8-bit INTER_LINEAR fixed-point algorithm; xofs/xcoef/yofs/ycoef are cv::resize's per-column / per-row
 * source index and 11-bit weight tables, may be NULL when no resize happens) -> crop: output pixel
 * (y, x) takes resized pixel (y0 + y, x0 + x), or (y0 + y, x0 - x) when flip is set (x0 is then the
 * RIGHT edge of the window: train flips after the crop, test before it) -> x / 255 -> (x - mean[c]) / std[c] (mean / std in
 * the source channel order) -> optional BGR -> RGB, written to dst rows of w_total pixels x c_pad
 * channels starting at pixel w_left (the W-padded, channel-padded layout of the model's data input;
 * padding is not touched).  dst points at frame 0 of the destination clip.
 * ------------------------------------------------------------------------------------------ */
typedef struct vlfb_clip_desc {
  int32_t frames, src_h, src_w, resized_h, resized_w;
  int32_t crop_h, crop_w, y0, x0, flip;
  int32_t to_rgb, w_left, w_total, c_pad;
  float mean[3], std[3];
} vlfb_clip_desc;
int vlfb_clip_preprocess(const vlfb_clip_desc* d, const uint8_t* frames, const int32_t* xofs,
                         const int16_t* xcoef, const int32_t* yofs, const int16_t* ycoef, void* dst,
                         int dst_dtype, vlfb_stream_t stream);

/* Colour augmentation of the train clip (cfg.TRAIN.USE_COLOR_AUGMENTATION: color_augmentation_list,
 * lib/datasets/data_input_helper.py:142-151; color_jitter_list / brightness_list / contrast_list / saturation_list /
 * lighting_list, lib/datasets/image_processor.py:252-336), between x / 255 and the normalisation of the walk above.
 * The host draws the op order, the blend factors and the lighting offsets; two kernels apply them.
 *
 * vlfb_clip_channel_sums: sums int64 [frames][VLFB_CLIP_SUM_BANDS][3] = the integer sums of the uint8 B, G, R values of
 * the pixels vlfb_clip_preprocess reads (same geometry, flip and fixed-point resize; dst fields of the descriptor are
 * not read), per frame and per band of crop rows [b * crop_h / 8, (b + 1) * crop_h / 8) (integer division; an empty
 * band gives zeros).  Every slot is written: the caller need not clear `sums`.  One workgroup per (band, frame), no
 * atomics: integers, so the sums do not depend on the launch geometry.  crop_h * crop_w must be below 2^31 (a thread's
 * 32-bit counters).
 *
 * vlfb_clip_preprocess_color: per pixel, in fp32, with (b, g, r) = x / 255 of the source channels, for i < n_ops:
 *   grey = 0.299f * r + 0.587f * g + 0.114f * b  of the pixel's current value
 *   VLFB_COLOR_BRIGHTNESS  v = v * alpha[i]
 *   VLFB_COLOR_SATURATION  v = v * alpha[i] + grey * (1 - alpha[i])
 *   VLFB_COLOR_CONTRAST    v = v * alpha[i] + M * (1 - alpha[i]),  M = m * (the alphas of the brightness ops before it),
 *                          m = (float)((0.299 * S_R + 0.587 * S_G + 0.114 * S_B) / (255 * crop_h * crop_w)) in double, S_c =
 *                          the frame's 8 band sums added in band order (the reference takes np.mean of the grey image at
 *                          that point of the chain; a saturation blend leaves a pixel's grey value unchanged up to
 *                          rounding because the weights add to one, so one pass over the un-augmented window serves)
 * then v += light[c] (AlexNet-style PCA lighting, per SOURCE channel), (v - mean[c]) / std[c], channel swap and store as
 * vlfb_clip_preprocess does.  n_ops = 0 and light = 0 give vlfb_clip_preprocess's output bit for bit.  `sums` may be NULL
 * when no contrast op is present.  An op code outside 0..2 or listed twice, and n_ops outside 0..3, are rejected. */
#define VLFB_CLIP_SUM_BANDS 8
#define VLFB_COLOR_BRIGHTNESS 0
#define VLFB_COLOR_CONTRAST 1
#define VLFB_COLOR_SATURATION 2
typedef struct vlfb_clip_color {
  int32_t n_ops;        /* 0..3 jitter ops, applied in this order */
  int32_t op[3];        /* 0 brightness, 1 contrast, 2 saturation */
  float   alpha[3];     /* blend factor of op[i] */
  float   light[3];     /* PCA offset per SOURCE channel (B, G, R), added after the ops */
} vlfb_clip_color;
int vlfb_clip_channel_sums(const vlfb_clip_desc* d, const uint8_t* frames, const int32_t* xofs,
                           const int16_t* xcoef, const int32_t* yofs, const int16_t* ycoef, int64_t* sums,
                           vlfb_stream_t stream);
int vlfb_clip_preprocess_color(const vlfb_clip_desc* d, const vlfb_clip_color* c, const uint8_t* frames,
                               const int32_t* xofs, const int16_t* xcoef, const int32_t* yofs,
                               const int16_t* ycoef, const int64_t* sums, void* dst, int dst_dtype,
                               vlfb_stream_t stream);

/* The clips of one minibatch in one launch each (lib/datasets/clip_loader.py; the reference assembles a minibatch in
 * lib/datasets/dataloader.py and the *_data_input.py modules, one worker process per clip).  An item is what the three
 * entry points above take for one clip, with every pointer as a 64-bit device address:
 *
 *   offset  0  frames                       uint8 BGR [geo.frames][geo.src_h][geo.src_w][3]
 *           8  xofs, xcoef, yofs, ycoef     resize tables; may be 0 when resized == src
 *          40  dst                          frame 0 of this clip's destination
 *          48  sums                         int64 [geo.frames][VLFB_CLIP_SUM_BANDS][3]; may be 0 without a contrast op
 *          56  geo                          vlfb_clip_desc, 80 bytes
 *         136  color                        vlfb_clip_color, 40 bytes; n_ops = 0 and light = 0: no colour chain
 *   sizeof = VLFB_CLIP_ITEM_BYTES = 176, no padding.
 *
 * Items may differ in every field (frames, source / resized size, crop window, flip, colour plan, destination row).
 * `items_host` is the array the HOST reads: every item is checked with the conditions of the per-clip entry points (crop
 * window inside the resized frame, tables present when resizing, destination row, op codes, a contrast op has its sums;
 * 1 <= n_items <= 65535) and a bad one is rejected with a message before anything is launched; both entry points check
 * the whole item.  `items_dev` is the same array in DEVICE memory, which the caller uploaded in stream order before the
 * call: each workgroup reads the record of its clip from there (uniform per workgroup), so the host array may be reused
 * as soon as the call returns and nothing is passed by value.
 *
 * vlfb_clip_batch_channel_sums: vlfb_clip_channel_sums for every item whose `sums` is not 0; grid (band, frame, item).
 * vlfb_clip_batch_preprocess: per item the arithmetic of vlfb_clip_preprocess_color (which with n_ops = 0 and light = 0 is
 * vlfb_clip_preprocess's, bit for bit); grid (32 x 8 pixel tiles of the crop, frame, item), workgroups past an item's crop
 * or frames return.  With c_pad == 4 and a destination aligned to one pixel, a pixel is ONE 8-byte (16-bit dst_dtype) or
 * 16-byte (fp32) store whose fourth channel is zero (the padding channel is zero by contract); otherwise three scalar
 * stores as in the per-clip kernels.  W-padding pixels are never written. */
#define VLFB_CLIP_ITEM_BYTES 176
typedef struct vlfb_clip_item {
  uint64_t frames;
  uint64_t xofs, xcoef, yofs, ycoef;
  uint64_t dst;
  uint64_t sums;
  vlfb_clip_desc  geo;
  vlfb_clip_color color;
} vlfb_clip_item;
int vlfb_clip_batch_channel_sums(const vlfb_clip_item* items_host, const vlfb_clip_item* items_dev, int n_items,
                                 vlfb_stream_t stream);
int vlfb_clip_batch_preprocess(const vlfb_clip_item* items_host, const vlfb_clip_item* items_dev, int n_items,
                               int dst_dtype, vlfb_stream_t stream);

/* The same two launches for clips given as frame lists into a frame store (lib/datasets/frame_store.py; the reference's
 * clips are index lists, dataset_helper.get_sequence, and the clips of a bank-construction pass share most frames):
 * `items[i].frames` points at a store uint8 BGR [store_frames_host[i]][geo.src_h][geo.src_w][3], and destination frame t
 * of item i reads source frame index[i * index_stride + t] of it.  Entries may repeat (a sequence clamped at a video's
 * ends) and come in any order; items may share a store or name different ones.  Everything else -- the item record, the
 * arithmetic, the grids, the stores, `sums` indexed by the DESTINATION frame t -- is that of the two entry points above
 * (the same device functions; with index[t] = t the output is theirs bit for bit).
 *
 * `index_host` is the table the HOST reads, `index_dev` the same int32 table in DEVICE memory, uploaded by the caller in
 * stream order as `items_dev` is; a workgroup reads its one entry from there (uniform per workgroup), nothing is passed
 * by value.  `store_frames_host` [n_items] is read by the host only.  Checked before anything is launched, beside the
 * conditions on the items: index_stride >= geo.frames, store_frames_host[i] >= 1, and 0 <= index < store_frames_host[i]
 * for the first geo.frames entries of every item (entries past geo.frames are not read); a bad table is rejected with
 * VLFB_ERR_ARG and a message that names the item and the entry. */
int vlfb_clip_batch_channel_sums_indexed(const vlfb_clip_item* items_host, const vlfb_clip_item* items_dev, int n_items,
                                         const int32_t* index_host, const int32_t* index_dev, int index_stride,
                                         const int32_t* store_frames_host, vlfb_stream_t stream);
int vlfb_clip_batch_preprocess_indexed(const vlfb_clip_item* items_host, const vlfb_clip_item* items_dev, int n_items,
                                       const int32_t* index_host, const int32_t* index_dev, int index_stride,
                                       const int32_t* store_frames_host, int dst_dtype, vlfb_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Baseline JPEG decode on the device: the frames the reference reads with cv2.imread (lib/datasets/data_input_helper.py:51-53;
 * written by ffmpeg -q:v 1, dataset_tools/ava/extract_ava_frames.sh:43), decoded into uint8 BGR [height][width][3] bit for
 * bit as libjpeg-turbo does with its defaults (integer "islow" inverse DCT, "fancy" chroma upsampling).
 *
 * Supported: SOF0, 8-bit, one scan holding all components; one component, or Y / Cb / Cr with luma sampling 1x1, 2x1 or 2x2
 * and chroma 1x1; 8-bit quantisation tables; Huffman table selectors 0 / 1; any restart interval.  The host parses the file
 * (lib/datasets/jpeg.py) and only moves bytes: an item carries the raw DQT / DHT content, the kernels build their tables.
 *
 *   offset  0  scan          the entropy-coded bytes of the scan (stuffed zeros and restart markers included)
 *           8  dst           uint8 BGR [height][width][3]; a grey file stores B = G = R
 *          16  seg_offsets   uint32 [n_segments]: where each restart interval's data begins in `scan` (the first is 0, the
 *                            others follow their RSTn marker); one entry when the file has no restart markers
 *          24  ws_offset     where this item's part of the workspace begins: the sum of vlfb_jpeg_workspace_bytes of the
 *                            items before it
 *          32  scan_bytes, n_segments, width, height, n_comp, restart_interval (MCUs; 0 = none)
 *          56  h[4], v[4]    sampling factors per component; tq[4], td[4], ta[4]: its quantisation / DC / AC table
 *          76  reserved (0)
 *          80  quant[4][64]  as in DQT (zigzag order)
 *         336  huff[4][272]  DC tables 0, 1, then AC tables 0, 1; each as in DHT: 16 counts, then up to 256 symbols
 *   sizeof = VLFB_JPEG_ITEM_BYTES = 1424, no padding.  Items of one batch may differ in every field.
 *
 * Three launches: entropy decode (one wave per restart interval, or per frame when there is none: the parallelism of a
 * minibatch of ffmpeg frames is its ~256 frames) into int16 coefficients, natural order, per component in whole MCUs;
 * dequantisation and inverse DCT into sample planes; upsampling, colour conversion and store.  Coefficients and planes live
 * in `workspace` (16-byte aligned, vlfb_jpeg_workspace_bytes of the batch).  No byte outside [scan, scan + scan_bytes) is
 * read and none outside dst's height * width * 3 is written, whatever the stream holds; loops are bounded by the MCU count.
 * A missing code, a stream that ends early or a restart marker out of place stops that restart interval: its remaining
 * coefficients are zero and the item's word of `status` (int32 [n_items], written by every call: 0 = decoded) gets
 * VLFB_JPEG_TRUNCATED / _BAD_CODE / _BAD_RESTART bits.  Nothing synchronises with the host.
 *
 * `items_host` is checked before anything is launched (VLFB_ERR_ARG, the message names the item): n_items in 1..65535, sizes
 * in 1..65535, sampling and selectors as above, non-NULL addresses, scan_bytes < 2^30, n_segments >= 1, Huffman counts that
 * form a prefix code, ws_offset as defined above, workspace_bytes large enough.  `items_dev` is the same array in device
 * memory, uploaded by the caller in stream order, as for vlfb_clip_batch_preprocess.
 *
 * vlfb_jpeg_workspace_bytes: bytes of workspace the first n_items items need (< 0 and a message for a bad item).
 * vlfb_jpeg_decode_host: the same arithmetic (csrc/vlfb_jpeg_core.h, compiled for the host) for ONE item whose scan and
 * seg_offsets are HOST addresses; single-threaded, allocates its own workspace, needs no GPU.  It is the checker that pins
 * the arithmetic against libjpeg-turbo where no GPU is present, not a loader path.
 *
 * vlfb_jpeg_decode_batch_par: as vlfb_jpeg_decode_batch (same items, workspace, status words, argument checks), with the
 * entropy decode of the items the routing rule accepts -- no restart interval, one segment, a scan of at least two
 * subsequences and at most 128 KiB (csrc/vlfb_jpeg_core.h, vlfb_jpeg_item_is_parallel) -- done by one workgroup of 256 lanes
 * per item: the scan is destuffed into LDS, every lane decodes a `subseq_bytes`-byte subsequence from a guessed state, the
 * lanes resynchronise on their neighbours' exit states (at most 256 rounds per chunk of 256 subsequences: the serial walk
 * in the worst case, so the result never rests on synchronisation happening), then write the coefficients from their
 * confirmed states; DC prediction is a prefix sum.  A missing code, a DC size above 15, a run past coefficient 63, a marker
 * or the end of the data before the last MCU, or any padding bit consumed sends the item to the serial kernel in the same
 * call, so pixels and status of a damaged stream are those of vlfb_jpeg_decode_batch.  Every other item takes the serial
 * kernel as before.  subseq_bytes: a multiple of 4 in 8..4096, 0 = the library's default (256).  stats_dev: NULL, or int32
 * [n_items][4] = {routed (0 serial by rule, 1 parallel, 2 parallel then redone serially), chunks, synchronisation rounds
 * summed over the chunks, most rounds of one chunk}.
 * vlfb_jpeg_decode_host_par: the same algorithm on the host for ONE item (host addresses), with `lanes` simulated lanes
 * per chunk (1..1024) run one after another; stats: NULL or int32 [4] as above.  The checker of the parallel arithmetic
 * where no GPU is present.
 * ------------------------------------------------------------------------------------------ */
#define VLFB_JPEG_ITEM_BYTES 1424
enum { VLFB_JPEG_TRUNCATED = 1, VLFB_JPEG_BAD_CODE = 2, VLFB_JPEG_BAD_RESTART = 4 };
typedef struct vlfb_jpeg_item {
  uint64_t scan, dst, seg_offsets, ws_offset;
  uint32_t scan_bytes, n_segments;
  int32_t  width, height, n_comp, restart_interval;
  uint8_t  h[4], v[4], tq[4], td[4], ta[4];
  uint8_t  reserved[4];
  uint8_t  quant[4][64];
  uint8_t  huff[4][272];
} vlfb_jpeg_item;
int64_t vlfb_jpeg_workspace_bytes(const vlfb_jpeg_item* items_host, int n_items);
int vlfb_jpeg_decode_batch(const vlfb_jpeg_item* items_host, const vlfb_jpeg_item* items_dev, int n_items, void* workspace,
                           int64_t workspace_bytes, int32_t* status_dev, vlfb_stream_t stream);
int vlfb_jpeg_decode_host(const vlfb_jpeg_item* item, uint8_t* dst, int32_t* status);
int vlfb_jpeg_decode_batch_par(const vlfb_jpeg_item* items_host, const vlfb_jpeg_item* items_dev, int n_items, void* workspace,
                               int64_t workspace_bytes, int32_t* status_dev, int subseq_bytes, int32_t* stats_dev,
                               vlfb_stream_t stream);
int vlfb_jpeg_decode_host_par(const vlfb_jpeg_item* item, uint8_t* dst, int32_t* status, int lanes, int subseq_bytes,
                              int32_t* stats);

/* ------------------------------------------------------------------------------------------
 * Evaluation metrics on the device.  Replace the host meter of lib/utils/metrics.py, which fetches `pred` and
 * `labels` from every GPU every iteration (get_multi_gpu_outputs, :514-540), and tools/evaluate_actions.py.
 * All state (counters, cursor, tables) is caller-owned device memory; every count is an integer and the two
 * floating-point sums are taken in a fixed order, so results do not depend on the launch geometry.
 * ------------------------------------------------------------------------------------------ */
/* Top-k hits of single-label heads (compute_topk_correct_hits, metrics.py:485-500; compute_top_k_verbs_or_nouns,
 * evaluate_actions.py:63-74).  scores [rows][cols] (`dtype`), labels [rows], ks: nk <= 4 HOST values, 1 <= k <= cols.
 * ADDS into hits [nk + 1]: hits per k, and in the last slot the number of rows counted.  A row with label < 0 or
 * >= cols is skipped.  rank = #{j : s_j > s_label} + #{j < label : s_j == s_label}; hit iff rank < k; a row whose
 * label score is NaN is a counted miss.  (The reference's two argsort spellings disagree on ties and numpy's default
 * sort is not stable: ties are pinned by this rule.) */
int vlfb_topk_hits(const void* scores, int dtype, const int32_t* labels, int64_t rows, int64_t cols, const int32_t* ks,
                   int nk, int64_t* hits, vlfb_stream_t stream);
/* vlfb_topk_hits that also KEEPS the rows (all_preds.append / stack_predictions, metrics.py:147-163, 384-388, whose table
 * finalize_metrics writes as epic_predictions_<name>.pkl, :222-226), in the same single launch.  `hits` gets exactly what
 * vlfb_topk_hits adds for the same arguments: every row of the call is counted, the padding rows of the last batch
 * included, as the reference's running error counts them.  Row r of the call is stored at row *cursor + r of table fp32
 * [total_rows][cols] (the scores converted to fp32, which is exact) and table_labels int32 [total_rows] (the label as it
 * is, out of range or not) when that row is < total_rows; rows at stream positions >= total_rows are dropped and nothing
 * outside the two tables is written.  `cursor` is an int64 IN DEVICE MEMORY that the call reads and then advances by
 * `rows`, as in vlfb_scores_merge_max: with all other arguments constant the call can sit in a replayed call list or a
 * captured graph.  total_rows >= 1. */
int vlfb_topk_hits_keep(const void* scores, int dtype, const int32_t* labels, int64_t rows, int64_t cols, const int32_t* ks,
                        int nk, int64_t* hits, float* table, int32_t* table_labels, int64_t total_rows, int64_t* cursor,
                        vlfb_stream_t stream);
/* EPIC action top-k (compute_top_k_actions, evaluate_actions.py:77-98): the same rank rule over the flattened index
 * v * Nn + n of (verb[r][v] * noun[r][n]) * prior[v][n], each product rounded to fp32 in that order; prior may be NULL.
 * A row with either label out of range is skipped. */
int vlfb_action_topk_hits(const float* verb, const float* noun, const float* prior, const int32_t* verb_labels,
                          const int32_t* noun_labels, int64_t rows, int64_t V, int64_t Nn, const int32_t* ks, int nk,
                          int64_t* hits, vlfb_stream_t stream);
/* Clip merge (aggregate_predictions_from_clips, metrics.py:165-186; all_preds.append, :384-388) while the clips
 * arrive: row r of the call goes to item (cursor + r) % n_items of table fp32 [n_items][cols] / table_labels uint8
 * [n_items][cols]; the element-wise result is max(table, row) (a NaN score leaves the table as it is), rows of one call
 * that land on one item included.  `cursor` is an int64 IN DEVICE MEMORY that the call reads and then advances by
 * `rows`, so the call can sit in a replayed call list or a captured graph with constant arguments.  total_rows > 0:
 * rows at stream positions >= total_rows are dropped (stack_predictions, :143-163, cuts the padding of the last
 * batch).  The caller fills the table with -inf and table_labels with 255 (= not visited); labels (int32 [rows][cols],
 * > 0 = positive) of a revisited item that differ from what is there are COUNTED, per element, into *mismatches
 * (the reference asserts, :178-181). */
int vlfb_scores_merge_max(const void* scores, int dtype, const int32_t* labels, int64_t rows, int64_t cols, float* table,
                          uint8_t* table_labels, int64_t n_items, int64_t total_rows, int64_t* cursor,
                          int32_t* mismatches, vlfb_stream_t stream);
/* Per class c of table [n][cols] / table_labels: average precision and ROC-AUC in fp64 and the number of positives
 * (sklearn.metrics.average_precision_score / roc_auc_score as mean_ap_metric calls them, metrics.py:444-482), ties
 * grouped: the column sorted descending, e_g = last index of the g-th run of equal scores, tp_g = positives in
 * [0, e_g], P = tp_last, fp_g = e_g + 1 - tp_g:
 *   AP  = sum_g (tp_g - tp_{g-1}) * tp_g / (P * (e_g + 1))
 *   AUC = sum_g (fp_g - fp_{g-1}) * (tp_g + tp_{g-1}) / (2 * P * (n - P))
 * (integer numerators and denominators, one division per term).  P == 0: AP = AUC = NaN; P == n: AUC = NaN.
 * n <= 8192: the column is sorted in LDS and `workspace` is not used; above that, or with VLFB_CLASS_AP_FORCE_GLOBAL
 * in `flags`, the same network runs over `workspace` (vlfb_query_workspace(VLFB_WS_CLASS_AP, {n, cols}) bytes).  Both
 * paths give bit-identical results. */
#define VLFB_CLASS_AP_MAX_N (1 << 20)
enum { VLFB_CLASS_AP_FORCE_GLOBAL = 1 };
int vlfb_class_ap_auc(const float* table, const uint8_t* table_labels, int64_t n, int64_t cols, double* ap, double* auc,
                      int32_t* n_pos, void* workspace, int64_t workspace_bytes, int flags, vlfb_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * AVA frame-mAP: the PASCAL-VOC detection protocol at IoU 0.5, as the AVA evaluator applies it.  The
 * reference ships no evaluator (utils/ava_eval_helper.py imports utils.ava_evaluation.*, which is absent), so what is
 * pinned here is the protocol itself; tests/ava_eval_ref.py restates it in fp64.
 * ------------------------------------------------------------------------------------------ */
/* True / false positive of every (detection row, class).  scores fp32 [n_rows][cols] is the meter's score table (class id
 * = column + 1); det_box fp64 [n_rows][4] = (x1, y1, x2, y2) by table row.  Images are two CSRs over n_img images:
 * img_det_ptr / det_rows (the table rows of each image's detections; a row is named at most once) and img_gt_ptr /
 * gt_box fp64 [.][4] / gt_class int32 [.] (one row per (box, label), in file order within an image).  Both pointer arrays
 * are given twice: in device memory for the kernel, and as HOST copies (host_img_*_ptr) the entry point checks before it
 * launches -- an image with more than VLFB_AVA_MAX_DET detections or VLFB_AVA_MAX_GT ground-truth rows is refused with a
 * message that names it; nothing is ever truncated.  The device and the host copy of a pointer array MUST be identical
 * (vlfb.metrics.ava_frame_ap uploads the array it passes): if they differ the outputs are undefined -- the kernel only
 * keeps its own reads and writes inside the arrays it was given.  class_mask uint8 [cols]: 1 = whitelisted.
 * Outputs: tp uint8 [n_rows][cols], first filled with 255, then 0 / 1 for every (row of det_rows, whitelisted class);
 * n_gt int32 [cols], the ground-truth rows of every whitelisted class (0 for the others).
 * One image, one class c: G = its ground-truth rows of class c in stored order; D = all its detection rows by
 * (scores[row][c] descending, row ascending).  IoU in fp64: iw = min(x2a, x2b) - max(x1a, x1b), ih likewise,
 * inter = max(iw, 0) * max(ih, 0), iou = inter / (area_a + area_b - inter), area = (x2 - x1) * (y2 - y1).  G empty: every
 * detection is a false positive.  Otherwise, in that order, g* = the FIRST index of the maximum IoU over G; the detection is
 * a true positive iff iou(d, g*) >= 0.5 and g* is not yet taken, and g* then becomes taken.  A detection whose best box is
 * taken does NOT fall back to its second-best box.  Scores must not be NaN.  No atomics: every output byte has one writer. */
#define VLFB_AVA_MAX_DET 128
#define VLFB_AVA_MAX_GT 128
int vlfb_ava_match_tp(const float* scores, const double* det_box, int64_t n_rows, int64_t cols, const int32_t* img_det_ptr,
                      const int32_t* det_rows, const int32_t* img_gt_ptr, const double* gt_box, const int32_t* gt_class,
                      int64_t n_img, const int32_t* host_img_det_ptr, const int32_t* host_img_gt_ptr, const uint8_t* class_mask,
                      uint8_t* tp, int32_t* n_gt, vlfb_stream_t stream);
/* PASCAL AP per class c from scores [n][cols], tp [n][cols] and n_gt [cols] (compute_average_precision of the public
 * evaluator: sentinels 0 and 1, precision made non-increasing from the right, summed where recall changes): the rows
 * whose tp is 0 or 1, sorted by (score descending, row ascending); ctp_i = true positives in positions 0..i,
 * p_i = ctp_i / (i + 1);  AP = (1 / n_gt) * sum over true-positive positions i of max_{j >= i} p_j.  The maximum is taken
 * over exact integer fractions; every term is one fp64 division ctp_j / ((j + 1) * n_gt), summed in a fixed order.
 * n_gt[c] <= 0 (a class without ground truth, a masked class): NaN; n_gt[c] > 0 and no detection: 0.
 * n <= 4096: the column is sorted in LDS; above that, or with VLFB_CLASS_AP_FORCE_GLOBAL, the same network runs over
 * `workspace` (vlfb_query_workspace(VLFB_WS_CLASS_AP_VOC, {n, cols}) bytes), up to n = VLFB_CLASS_AP_MAX_N.  Both paths
 * give bit-identical results. */
int vlfb_class_ap_voc(const float* scores, const uint8_t* tp, const int32_t* n_gt, int64_t n, int64_t cols, double* ap,
                      void* workspace, int64_t workspace_bytes, int flags, vlfb_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * AVA multi-crop merge: the last stage of the reference's multi-crop test (tools/test_net.py:57-87 runs scales x 2 flips x 3
 * spatial shifts; lib/utils/metrics.py:599-711 merges their csv files).  One call merges the three shifts of ONE (scale,
 * flip) and accumulates the result; it restates metrics.py:654-677 and :703-705 on arrays, in fp64 and in the reference's
 * operation order, so that every decision is the reference's.
 *
 * logits: the `pred` rows of shift 0, 1, 2: shift s begins at element s * shift_stride, row r ld elements further on,
 * cols <= ld.  `dtype` is VLFB_F32 / VLFB_F16 / VLFB_BF16 (what an engine's `pred` holds; converted to fp64 exactly) or
 * VLFB_F64, which only this entry point takes: logits parsed from score files, as the reference merges them.  boxes fp64 [rows][4] = (x1, y1, x2, y2) normalised to the ORIGINAL frame;
 * frame_hw int32 [rows][2] = (height, width) of the row's source frames.  Per row:
 *   w = (double)(width * scale) / height;  nc = (double)min(scale, max_crop) / w
 *   center_left = 0.5 - nc / 2.0, center_right = 0.5 + nc / 2.0, lcrop_right = nc, rcrop_left = 1.0 - nc
 *   with `flip`: x1' = 1.0 - x2, x2' = 1.0 - x1
 *   shift 1 (centre) sees the box iff x2 > center_left && x1 < center_right; shift 0 (left) iff x1 < lcrop_right;
 *   shift 2 (right) iff x2 > rcrop_left -- all strict
 *   combined = (sum over the shifts that see the box, in shift order 0, 1, 2, of 1 / (1 + exp(-logit))) / their number
 * (the reference adds the centre first; fp64 addition is commutative and the third term is last either way, so the sums are
 * the same bits).  A box no shift sees gives NaN, like np.mean([]); logits of a shift that does not see the box are not read.
 * acc fp64 [rows][cols] becomes combined when `first` is set, else acc + combined: over the calls of a keyframe in merge
 * order (scale, then flip) that is the reference's sequential np.sum.  out32 (may be NULL) gets (float)acc after the update;
 * valid (may be NULL) uint8 [rows] gets the mask of the shifts that see the box (bit s = shift s), written by one thread
 * per row.  No atomics: every output element has one writer.
 * VLFB_ERR_ARG before anything is launched: a NULL logits / boxes / frame_hw / acc, cols < 1, rows < 0, ld < cols,
 * scale < 1, max_crop < 1, an unknown dtype.  rows == 0 succeeds and launches nothing.  frame_hw is device memory the host
 * cannot check: a height of 0 gives NaN / inf geometry, never an access outside the arrays. */
enum { VLFB_F64 = 11 };
int vlfb_multicrop_merge(const void* logits, int dtype, int64_t shift_stride, int64_t ld, const double* boxes,
                         const int32_t* frame_hw, int64_t rows, int64_t cols, int scale, int max_crop, int flip, int first,
                         double* acc, float* out32, uint8_t* valid, vlfb_stream_t stream);

/* Rank interleave: the global stream order of a data-parallel pass rebuilt from the ranks' own row tables.  Rank p of `world`
 * issued slices p, p + world, p + 2 * world, ... of the single-process walk, `b` rows each, and kept them in that order in
 * parts[p] (DEVICE address, part_rows[p] rows of row_bytes bytes; `parts` and `part_rows` themselves are HOST arrays of
 * `world` entries).  Destination row g, 0 <= g < total, becomes row (g / (b * world)) * b + g % b of part (g / b) % world:
 * per global iteration, rank 0 .. world-1, which is the order the reference's get_multi_gpu_outputs sees the rows in.
 * Destination rows at or after `total` are not touched.  A pure copy of bytes: every destination byte has one writer, no
 * atomics, no dependence on launch order.  16-byte accesses when row_bytes, dst and every part that is read allow them,
 * else 4-byte accesses, else bytes.
 * VLFB_ERR_ARG before anything is launched: world outside 1..VLFB_ROWS_INTERLEAVE_MAX_WORLD, b < 1, row_bytes < 1,
 * total < 0, a NULL parts / part_rows, a NULL dst with total > 0, a part that is shorter than the last row asked of it
 * (or NULL while rows are asked of it).  total == 0 succeeds and launches nothing. */
#define VLFB_ROWS_INTERLEAVE_MAX_WORLD 64
int vlfb_rows_interleave(const void* const* parts, const int64_t* part_rows, int world, int64_t b, int64_t row_bytes,
                         int64_t total, void* dst, vlfb_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VLFB_H_ */
