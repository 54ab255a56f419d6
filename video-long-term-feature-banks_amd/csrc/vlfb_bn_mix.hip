// SpatialBN on the "mix" path: the kernels of vlfb_bn.hip for VALUES stored as two fp16 planes (VLFB_F16PAIR: hi = fp16(v),
// lo = fp16(v - hi), planes rows * C elements apart) or as fp32, with the residual Sum and the ReLU behind the BN folded
// into the apply pass, and a backward that reads the fp16 (optionally two-term) or fp32 gradients the mix backward carries.
//   fwd:  moments of v = hi + lo about the row-0 pivot (fp32 slab partials, folded in order, finished in double)
//         y = a[c] * v + b[c]  [+ R]  [max(., 0)]   written in the format of x; a pair is canonical: fp16(hi + lo) == hi
//   bwd:  g = dy [+ dy_lo];  dbeta = sum g, dgamma = sum g * xhat, xhat = ((hi - mean) + lo) * inv_std
//         dx = ca * g + cb * ((hi - mean) + lo) + cc,  ca = gamma * inv_std, cb = -ca * inv_std * dgamma / rows, cc = -ca * dbeta / rows
// Same structure as vlfb_bn.hip: 8 chunk lanes x 32 row lanes per block, slab partials, one thread per channel that folds the
// slabs in order -- no atomics, the same bits every run; every lane moves 16 bytes per access (8 channels of a plane, 4 of an
// fp32 row).  Three HBM passes per direction: the moments / sums read x (and dy), the apply reads them again and writes.
#include <type_traits>
#include "vlfb_common.h"

namespace vlfb {
namespace {

constexpr int kCL = 8;                  // chunk lanes per block
constexpr int kRL = 256 / kCL;          // row lanes
enum { GT_F16 = 0, GT_F16X2 = 1, GT_F32 = 2 };       // gradient operand: fp16, fp16 + low term, fp32

template <int V> __device__ __forceinline__ void ld_h(const unsigned short* p, float (&v)[V]);
template <> __device__ __forceinline__ void ld_h<8>(const unsigned short* p, float (&v)[8]) {
  const uint4 t = *reinterpret_cast<const uint4*>(p);
  const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) { v[2 * i] = h2f((unsigned short)(w[i] & 0xffffu)); v[2 * i + 1] = h2f((unsigned short)(w[i] >> 16)); }
}
template <> __device__ __forceinline__ void ld_h<4>(const unsigned short* p, float (&v)[4]) {
  const uint2 t = *reinterpret_cast<const uint2*>(p);
  v[0] = h2f((unsigned short)(t.x & 0xffffu)); v[1] = h2f((unsigned short)(t.x >> 16));
  v[2] = h2f((unsigned short)(t.y & 0xffffu)); v[3] = h2f((unsigned short)(t.y >> 16));
}
template <int V> __device__ __forceinline__ void ld_f(const float* p, float (&v)[V]) {
#pragma unroll
  for (int i = 0; i < V / 4; ++i) {
    const float4 t = *reinterpret_cast<const float4*>(p + 4 * i);
    v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
  }
}
template <int V> __device__ __forceinline__ void st_bits(unsigned short* p, const unsigned short (&h)[V]);
template <> __device__ __forceinline__ void st_bits<8>(unsigned short* p, const unsigned short (&h)[8]) {
  *reinterpret_cast<uint4*>(p) = make_uint4((uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16),
                                            (uint32_t)h[4] | ((uint32_t)h[5] << 16), (uint32_t)h[6] | ((uint32_t)h[7] << 16));
}
template <> __device__ __forceinline__ void st_bits<4>(unsigned short* p, const unsigned short (&h)[4]) {
  *reinterpret_cast<uint2*>(p) = make_uint2((uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16));
}
template <int V> __device__ __forceinline__ void st_f(float* p, const float (&v)[V]) {
#pragma unroll
  for (int i = 0; i < V / 4; ++i) *reinterpret_cast<float4*>(p + 4 * i) = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
}

// the canonical pair of y: hi = fp16(y), lo = fp16(y - hi) -- except where that low term, rounded UP to half an ulp of hi,
// would make fp16(hi + lo) the even neighbour of an odd hi: there lo is the next fp16 towards zero (2^-24 of y)
__device__ __forceinline__ void pair_of(float y, unsigned short& hi, unsigned short& lo) {
  split2_h(y, hi, lo);
  if ((lo & 0x7fffu) != 0 && f2h(h2f(hi) + h2f(lo)) != hi) lo -= 1;
}

// values in the format of the tensor: two fp16 planes `n` elements apart (8 channels per lane) or fp32 (4 per lane)
template <bool PAIR> struct Val {
  static constexpr int V = PAIR ? 8 : 4;
  // hi and lo separately (an fp32 value: lo = 0), for the consumers that subtract the mean from hi first
  __device__ static __forceinline__ void load2(const void* x, long long off, long long n, float (&hi)[V], float (&lo)[V]) {
    if (PAIR) {
      ld_h<V>((const unsigned short*)x + off, hi);
      ld_h<V>((const unsigned short*)x + n + off, lo);
    } else {
      ld_f<V>((const float*)x + off, hi);
#pragma unroll
      for (int k = 0; k < V; ++k) lo[k] = 0.f;
    }
  }
  __device__ static __forceinline__ void load(const void* x, long long off, long long n, float (&v)[V]) {
    float lo[V];
    load2(x, off, n, v, lo);
    if (PAIR) {
#pragma unroll
      for (int k = 0; k < V; ++k) v[k] += lo[k];
    }
  }
  __device__ static __forceinline__ void store(void* y, long long off, long long n, const float (&v)[V]) {
    if (PAIR) {
      unsigned short h[V], l[V];
#pragma unroll
      for (int k = 0; k < V; ++k) pair_of(v[k], h[k], l[k]);
      st_bits<V>((unsigned short*)y + off, h);
      st_bits<V>((unsigned short*)y + n + off, l);
    } else {
      st_f<V>((float*)y + off, v);
    }
  }
};

// the gradient operand g = dy [+ dy_lo] at element `off`
template <int GT, int V>
__device__ __forceinline__ void load_grad(const void* dy, const void* dy_lo, long long off, float (&g)[V]) {
  if (GT == GT_F32) {
    ld_f<V>((const float*)dy + off, g);
  } else {
    ld_h<V>((const unsigned short*)dy + off, g);
    if (GT == GT_F16X2) {
      float l[V];
      ld_h<V>((const unsigned short*)dy_lo + off, l);
#pragma unroll
      for (int k = 0; k < V; ++k) g[k] += l[k];
    }
  }
}

// partial[slab][0 | 1][C]: sums of (MOMENTS) d = v - pivot, d^2 or (GRADS) g, g * xhat
template <bool PAIR, bool GRADS, int GT>
__global__ void __launch_bounds__(256)
bnm_partial_kernel(const void* __restrict__ x, const void* __restrict__ dy, const void* __restrict__ dy_lo,
                   const float* __restrict__ mean, const float* __restrict__ inv_std, long long rows, int C,
                   float* __restrict__ partial) {
  constexpr int V = Val<PAIR>::V;
  __shared__ float red[2][kRL][kCL * 8 + 1];
  const int cl = threadIdx.x % kCL, rl = threadIdx.x / kCL;
  const int c0 = (blockIdx.x * kCL + cl) * V;
  const long long n = rows * C;
  const long long per = (rows + gridDim.y - 1) / gridDim.y;
  const long long r0 = (long long)blockIdx.y * per, r1 = min(rows, r0 + per);
  float a0[V], a1[V], piv[V], sc[V];
#pragma unroll
  for (int k = 0; k < V; ++k) { a0[k] = a1[k] = 0.f; piv[k] = 0.f; sc[k] = 1.f; }
  if (c0 < C) {
    if (GRADS) {
#pragma unroll
      for (int k = 0; k < V; ++k) { piv[k] = mean[c0 + k]; sc[k] = inv_std[c0 + k]; }
    } else {
      Val<PAIR>::load(x, c0, n, piv);       // row 0: the pivot of every slab
    }
    for (long long r = r0 + rl; r < r1; r += kRL) {
      const long long off = r * C + c0;
      if (GRADS) {
        float hi[V], lo[V], g[V];
        Val<PAIR>::load2(x, off, n, hi, lo);
        load_grad<GT, V>(dy, dy_lo, off, g);
#pragma unroll
        for (int k = 0; k < V; ++k) { a0[k] += g[k]; a1[k] += g[k] * (((hi[k] - piv[k]) + lo[k]) * sc[k]); }
      } else {
        float v[V];
        Val<PAIR>::load(x, off, n, v);
#pragma unroll
        for (int k = 0; k < V; ++k) { const float d = v[k] - piv[k]; a0[k] += d; a1[k] += d * d; }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < V; ++k) { red[0][rl][cl * 8 + k] = a0[k]; red[1][rl][cl * 8 + k] = a1[k]; }
  __syncthreads();
  if (rl < 2 * V && c0 < C) {             // row lanes 0 .. V-1 fold sum 0 of channel rl, V .. 2V-1 sum 1
    const int which = rl / V, k = rl % V;
    float s = 0.f;
    for (int j = 0; j < kRL; ++j) s += red[which][j][cl * 8 + k];
    partial[((long long)blockIdx.y * 2 + which) * C + c0 + k] = s;
  }
}

// one thread per channel: fold the slabs in order; mean / inv_std (saved), running statistics, and the apply coefficients
// a = gamma * inv_std, b = beta - mean * a -- the arithmetic of bn_finish_train_kernel (vlfb_bn.hip)
template <bool PAIR>
__global__ void bnm_finish_train_kernel(const float* __restrict__ partial, int slabs, const void* __restrict__ x, long long rows,
                                        int C, const float* __restrict__ gamma, const float* __restrict__ beta,
                                        float* __restrict__ running_mean, float* __restrict__ running_var,
                                        float* __restrict__ save_mean, float* __restrict__ save_inv_std,
                                        float* __restrict__ coef, float eps, float momentum) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s = 0.0, q = 0.0;
  for (int j = 0; j < slabs; ++j) { s += partial[((long long)j * 2) * C + c]; q += partial[((long long)j * 2 + 1) * C + c]; }
  float pf;
  if (PAIR) pf = h2f(((const unsigned short*)x)[c]) + h2f(((const unsigned short*)x)[rows * C + c]);
  else pf = ((const float*)x)[c];
  const double piv = (double)pf;
  const double n = (double)rows;
  const double md = s / n;                                   // mean of (v - pivot)
  double var = q / n - md * md;
  if (var < 0.0) var = 0.0;
  const float mu = (float)(piv + md);
  const float istd = (float)(1.0 / sqrt(var + (double)eps));
  save_mean[c] = mu;
  save_inv_std[c] = istd;
  const double unbiased = rows > 1 ? var * n / (n - 1.0) : var;
  running_mean[c] = momentum * running_mean[c] + (1.f - momentum) * mu;
  running_var[c] = momentum * running_var[c] + (1.f - momentum) * (float)unbiased;
  const float a = gamma[c] * istd;
  coef[c] = a;
  coef[C + c] = beta[c] - mu * a;
}

// (the fold of bn_fold_test_kernel)
__global__ void bnm_fold_test_kernel(int C, const float* __restrict__ gamma, const float* __restrict__ beta,
                                     const float* __restrict__ running_mean, const float* __restrict__ running_var,
                                     float* __restrict__ coef, float eps) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float a = gamma[c] / sqrtf(running_var[c] + eps);
  coef[c] = a;
  coef[C + c] = beta[c] - running_mean[c] * a;
}

// dbeta, dgamma out; coefficient rows ca, cb, mean, cc of the backward apply
__global__ void bnm_finish_grad_kernel(const float* __restrict__ partial, int slabs, long long rows, int C,
                                       const float* __restrict__ gamma, const float* __restrict__ mean,
                                       const float* __restrict__ inv_std, float* __restrict__ dgamma,
                                       float* __restrict__ dbeta, float* __restrict__ coef, float gscale) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double sb = 0.0, sg = 0.0;
  for (int j = 0; j < slabs; ++j) { sb += partial[((long long)j * 2) * C + c]; sg += partial[((long long)j * 2 + 1) * C + c]; }
  if (dbeta) dbeta[c] = (float)sb * gscale;
  if (dgamma) dgamma[c] = (float)sg * gscale;
  const double n = (double)rows;
  const double ca = (double)gamma[c] * inv_std[c];
  coef[c] = (float)ca;
  coef[C + c] = (float)(-ca * inv_std[c] * sg / n);
  coef[2 * C + c] = mean[c];
  coef[3 * C + c] = (float)(-ca * sb / n);
}

// y = a[c] * v + b[c] [+ R] [max(., 0)], all tensors in the format of x
template <bool PAIR>
__global__ void __launch_bounds__(256)
bnm_apply_fwd_kernel(const void* x, const void* res, void* y,
                     const float* __restrict__ coef, long long rows, int C, int relu) {
  constexpr int V = Val<PAIR>::V;
  const long long n = rows * C;
  const int cpr = C / V;
  const long long chunks = rows * cpr;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < chunks; i += (long long)gridDim.x * blockDim.x) {
    const int c0 = (int)(i % cpr) * V;
    float v[V], o[V];
    Val<PAIR>::load(x, i * V, n, v);
#pragma unroll
    for (int k = 0; k < V; ++k) o[k] = coef[c0 + k] * v[k] + coef[C + c0 + k];
    if (res) {
      float r[V];
      Val<PAIR>::load(res, i * V, n, r);
#pragma unroll
      for (int k = 0; k < V; ++k) o[k] += r[k];
    }
    if (relu) {
#pragma unroll
      for (int k = 0; k < V; ++k) o[k] = fmaxf(o[k], 0.f);
    }
    Val<PAIR>::store(y, i * V, n, o);
  }
}

// dx = ca[c] * g + cb[c] * ((hi - mean[c]) + lo) + cc[c], written in the type of the gradient
template <bool PAIR, int GT>
__global__ void __launch_bounds__(256)
bnm_apply_bwd_kernel(const void* x, const void* dy, const void* dy_lo, void* dx, const float* __restrict__ coef, long long rows, int C) {
  constexpr int V = Val<PAIR>::V;
  const long long n = rows * C;
  const int cpr = C / V;
  const long long chunks = rows * cpr;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < chunks; i += (long long)gridDim.x * blockDim.x) {
    const int c0 = (int)(i % cpr) * V;
    float hi[V], lo[V], g[V], o[V];
    Val<PAIR>::load2(x, i * V, n, hi, lo);
    load_grad<GT, V>(dy, dy_lo, i * V, g);
#pragma unroll
    for (int k = 0; k < V; ++k)
      o[k] = coef[c0 + k] * g[k] + coef[C + c0 + k] * ((hi[k] - coef[2 * C + c0 + k]) + lo[k]) + coef[3 * C + c0 + k];
    if (GT == GT_F32) {
      st_f<V>((float*)dx + i * V, o);
    } else {
      unsigned short h[V];
#pragma unroll
      for (int k = 0; k < V; ++k) h[k] = f2h(o[k]);
      st_bits<V>((unsigned short*)dx + i * V, h);
    }
  }
}

int slabs_for(int64_t rows, int64_t C, int v) {
  const int cblocks = (int)((C / v + kCL - 1) / kCL);
  int64_t slabs = (rows + 1023) / 1024;
  const int64_t want = (2048 + cblocks - 1) / cblocks;      // ~2048 blocks: 8 per CU, the rest of the rows by the row loop
  if (slabs > want) slabs = want;
  if (slabs < 1) slabs = 1;
  return (int)slabs;
}

bool xf_ok(int xf) { return xf == VLFB_F16PAIR || xf == VLFB_F32; }

int check(int xf, int64_t rows, int64_t C, const void* ws, int64_t ws_bytes, const char* who) {
  VLFB_REQUIRE(xf_ok(xf), "%s: the value format must be VLFB_F16PAIR or VLFB_F32, got %d", who, xf);
  const int v = xf == VLFB_F16PAIR ? 8 : 4;
  VLFB_REQUIRE(rows > 0 && C > 0 && C % v == 0, "%s: rows > 0 and C a multiple of %d expected (%s values)", who, v,
               xf == VLFB_F16PAIR ? "two-plane" : "fp32");
  VLFB_REQUIRE(C <= INT32_MAX && rows * C < (1ll << 40), "%s: tensor too large", who);
  VLFB_REQUIRE(ws && ws_bytes >= vlfb_bn_mix_workspace_bytes(xf, rows, C), "%s: workspace too small (vlfb_bn_mix_workspace_bytes)", who);
  return VLFB_OK;
}

// f(std::integral_constant<bool, PAIR>{})
template <typename F>
void with_format(int xf, F&& f) {
  if (xf == VLFB_F16PAIR) f(std::true_type{}); else f(std::false_type{});
}
template <typename F>
void with_grad(int gt, bool lo, F&& f) {
  if (gt == VLFB_F32) f(std::integral_constant<int, GT_F32>{});
  else if (lo) f(std::integral_constant<int, GT_F16X2>{});
  else f(std::integral_constant<int, GT_F16>{});
}

}  // namespace
}  // namespace vlfb

using namespace vlfb;

extern "C" int64_t vlfb_bn_mix_workspace_bytes(int xf, int64_t rows, int64_t C) {
  if (!xf_ok(xf) || rows <= 0 || C <= 0) return -1;
  const int v = xf == VLFB_F16PAIR ? 8 : 4;
  return ((int64_t)slabs_for(rows, C, v) * 2 + 4) * C * 4;        // slab partials + four coefficient rows
}

extern "C" int vlfb_bn_fwd_mix(const void* x, void* y, const void* residual, const float* gamma, const float* beta,
                               float* running_mean, float* running_var, float* save_mean, float* save_inv_std,
                               void* workspace, int64_t workspace_bytes, int xf, int64_t rows, int64_t C, float eps,
                               float momentum, int is_test, int relu, vlfb_stream_t stream) {
  VLFB_REQUIRE(x, "bn_fwd_mix: null x");
  VLFB_REQUIRE(y || !residual, "bn_fwd_mix: a residual without an output");
  VLFB_REQUIRE(y && gamma && beta && running_mean && running_var, "bn_fwd_mix: null argument");
  VLFB_REQUIRE(is_test || (save_mean && save_inv_std), "bn_fwd_mix: training needs save_mean / save_inv_std");
  if (int rc = check(xf, rows, C, workspace, workspace_bytes, "bn_fwd_mix")) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int v = xf == VLFB_F16PAIR ? 8 : 4;
  const int slabs = slabs_for(rows, C, v);
  float* partial = (float*)workspace;
  float* coef = partial + (int64_t)slabs * 2 * C;
  const dim3 cgrid((unsigned)((C + 255) / 256));
  const int agrid = grid_for(rows * (C / v), 256);
  with_format(xf, [&](auto pair) {
    constexpr bool PAIR = decltype(pair)::value;
    if (is_test) {
      hipLaunchKernelGGL(bnm_fold_test_kernel, cgrid, dim3(256), 0, s, (int)C, gamma, beta, running_mean, running_var, coef, eps);
    } else {
      const dim3 grid((unsigned)((C / v + kCL - 1) / kCL), (unsigned)slabs);
      hipLaunchKernelGGL((bnm_partial_kernel<PAIR, false, GT_F16>), grid, dim3(256), 0, s, x, nullptr, nullptr, nullptr, nullptr,
                         (long long)rows, (int)C, partial);
      hipLaunchKernelGGL(bnm_finish_train_kernel<PAIR>, cgrid, dim3(256), 0, s, partial, slabs, x, (long long)rows, (int)C, gamma,
                         beta, running_mean, running_var, save_mean, save_inv_std, coef, eps, momentum);
    }
    hipLaunchKernelGGL(bnm_apply_fwd_kernel<PAIR>, dim3(agrid), dim3(256), 0, s, x, residual, y, coef, (long long)rows, (int)C,
                       relu ? 1 : 0);
  });
  return check_launch("bn_fwd_mix");
}

extern "C" int vlfb_bn_bwd_mix(const void* dy, const void* dy_lo, const void* x, const float* gamma, const float* save_mean,
                               const float* save_inv_std, void* dx, float* dgamma, float* dbeta, void* workspace,
                               int64_t workspace_bytes, int xf, int gt, int64_t rows, int64_t C, float grad_scale,
                               vlfb_stream_t stream) {
  VLFB_REQUIRE(x, "bn_bwd_mix: null x");
  VLFB_REQUIRE(dy && gamma && save_mean && save_inv_std, "bn_bwd_mix: null argument");
  VLFB_REQUIRE(gt == VLFB_F16 || gt == VLFB_F32, "bn_bwd_mix: the gradient type must be VLFB_F16 or VLFB_F32, got %d", gt);
  VLFB_REQUIRE(!dy_lo || gt == VLFB_F16, "bn_bwd_mix: dy_lo (a two-term gradient) goes with VLFB_F16 gradients only");
  VLFB_REQUIRE(dx || dgamma || dbeta, "bn_bwd_mix: nothing to compute");
  if (int rc = check(xf, rows, C, workspace, workspace_bytes, "bn_bwd_mix")) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int v = xf == VLFB_F16PAIR ? 8 : 4;
  const int slabs = slabs_for(rows, C, v);
  float* partial = (float*)workspace;
  float* coef = partial + (int64_t)slabs * 2 * C;
  const dim3 grid((unsigned)((C / v + kCL - 1) / kCL), (unsigned)slabs);
  const dim3 cgrid((unsigned)((C + 255) / 256));
  const int agrid = grid_for(rows * (C / v), 256);
  with_format(xf, [&](auto pair) {
    constexpr bool PAIR = decltype(pair)::value;
    with_grad(gt, dy_lo != nullptr, [&](auto g) {
      constexpr int GT = decltype(g)::value;
      hipLaunchKernelGGL((bnm_partial_kernel<PAIR, true, GT>), grid, dim3(256), 0, s, x, dy, dy_lo, save_mean, save_inv_std,
                         (long long)rows, (int)C, partial);
      hipLaunchKernelGGL(bnm_finish_grad_kernel, cgrid, dim3(256), 0, s, partial, slabs, (long long)rows, (int)C, gamma, save_mean,
                         save_inv_std, dgamma, dbeta, coef, grad_scale);
      if (dx)
        hipLaunchKernelGGL((bnm_apply_bwd_kernel<PAIR, GT>), dim3(agrid), dim3(256), 0, s, x, dy, dy_lo, dx, coef, (long long)rows,
                           (int)C);
    });
  });
  return check_launch("bn_bwd_mix");
}
