// HBM-bound operators of the hot path: AffineNd (the reference's only native op), layout movers,
// row softmax, residual add / ReLU, column sums (the pools: vlfb_pool.hip).  All are one-pass, 16-byte-per-lane
// vectorised kernels; the roofline that bounds them is HBM bandwidth.
#include "vlfb_common.h"
#include <type_traits>
#include <math.h>

namespace vlfb {

static thread_local char g_err[512] = "";
int set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

namespace {

// ---------------------------------------------------------------------------------------------
// AffineNd: y[n][c][i] = x*s[c] + b[c]   (affine_nd_op.cu:31-44), dx = dy*s[c] (46-58)
// grid.y walks the (n,c) rows so the per-row scale/bias are scalar loads.
// ---------------------------------------------------------------------------------------------
template <bool HAS_BIAS>
__global__ void affine_nd_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                 const float* __restrict__ bias, float* __restrict__ y,
                                 long long rows, int C, long long inner) {
  for (long long row = blockIdx.y; row < rows; row += gridDim.y) {
    const int c = (int)(row % C);
    const float s = scale[c];
    const float b = HAS_BIAS ? bias[c] : 0.f;
    const float* xr = x + row * inner;
    float* yr = y + row * inner;
    const bool vec = ((inner & 3) == 0) && ((((uintptr_t)xr | (uintptr_t)yr) & 15) == 0);
    if (vec) {
      const long long n4 = inner >> 2;
      for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
           i += (long long)gridDim.x * blockDim.x) {
        float4 v = reinterpret_cast<const float4*>(xr)[i];
        v.x = v.x * s + b; v.y = v.y * s + b; v.z = v.z * s + b; v.w = v.w * s + b;
        reinterpret_cast<float4*>(yr)[i] = v;
      }
    } else {
      for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < inner;
           i += (long long)gridDim.x * blockDim.x)
        yr[i] = xr[i] * s + b;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// layout movers
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void ncthw_to_nthwc_kernel(const float* __restrict__ src, T* __restrict__ dst,
                                      long long n, int c, long long thw, int c_pad) {
  const long long total = n * thw;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long b = i / thw, pos = i - b * thw;
    const float* s = src + b * c * thw + pos;
    T* d = dst + i * c_pad;
    for (int k = 0; k < c_pad; ++k) Elem<T>::st(d + k, k < c ? s[(long long)k * thw] : 0.f);
  }
}
// the same with zero pixels on both sides of every W row (the stem kernels then never need a
// w-bounds test: [N][rows][wl + W + wr][c_pad])
template <typename T>
__global__ void ncthw_to_nthwc_wpad_kernel(const float* __restrict__ src, T* __restrict__ dst,
                                           long long n, int c, long long rows, int w, int c_pad,
                                           int wl, int wtot) {
  const long long total = n * rows * wtot;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int wp = (int)(i % wtot);
    const long long nr = i / wtot;
    const long long b = nr / rows, r = nr - b * rows;
    const int x = wp - wl;
    const bool in = x >= 0 && x < w;
    const float* sp = src + (b * c * rows + r) * w + x;
    T* d = dst + i * c_pad;
    for (int k = 0; k < c_pad; ++k) Elem<T>::st(d + k, (in && k < c) ? sp[(long long)k * rows * w] : 0.f);
  }
}
template <typename T>
__global__ void nthwc_to_ncthw_kernel(const T* __restrict__ src, float* __restrict__ dst,
                                      long long n, int c, long long thw) {
  const long long total = n * c * thw;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long pos = i % thw;
    const long long bc = i / thw;
    const long long b = bc / c;
    const int k = (int)(bc - b * c);
    dst[i] = Elem<T>::ld(src + (b * thw + pos) * c + k);
  }
}
template <typename S, typename D>
__global__ void cast_kernel(const S* __restrict__ src, D* __restrict__ dst, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    Elem<D>::st(dst + i, Elem<S>::ld(src + i));
}
template <typename T>
__global__ void transpose2d_kernel(const T* __restrict__ src, T* __restrict__ dst, long long rows,
                                   long long cols) {
  __shared__ T tile[32][33];
  const long long b = blockIdx.z;
  const T* s = src + b * rows * cols;
  T* d = dst + b * rows * cols;
  const long long c0 = (long long)blockIdx.x * 32, r0 = (long long)blockIdx.y * 32;
  for (int j = threadIdx.y; j < 32; j += blockDim.y) {
    long long r = r0 + j, c = c0 + threadIdx.x;
    if (r < rows && c < cols) tile[j][threadIdx.x] = s[r * cols + c];
  }
  __syncthreads();
  for (int j = threadIdx.y; j < 32; j += blockDim.y) {
    long long c = c0 + j, r = r0 + threadIdx.x;
    if (r < rows && c < cols) d[c * rows + r] = tile[threadIdx.x][j];
  }
}

// bf16 term planes of the split-bf16 path: value v -> h = bf16(v), m = bf16(v - h), l = bf16(v - h - m)
// rounded_mul: the fp32-ROUNDED product (hipcc contracts `w * s - h` into an fma otherwise and the remainder terms
// would expand the unrounded product; the planes are defined as the expansion of the fp32 operand value)
__device__ __forceinline__ float rounded_mul(float a, float b) {
  float v = a * b;
  asm volatile("" : "+v"(v));
  return v;
}
template <int NPL>
__device__ __forceinline__ void store_terms(bf16_t* dst, long long idx, long long plane, float v) {
#pragma unroll
  for (int pl = 0; pl < NPL; ++pl) {
    const bf16_t t = f2bf(v);
    dst[pl * plane + idx] = t;
    v -= bf2f(t);
  }
}
// the two fp16 terms of v * VLFB_MIX_W2_SCALE, `stride` elements apart: h = fp16(sv), l = fp16(sv - h).  The scale keeps
// the low term of a small weight in the fp16 normal range; the launch's alpha carries its inverse.
__device__ __forceinline__ void store_scaled2(unsigned short* o, long long stride, float v) {
  split2_h(v * VLFB_MIX_W2_SCALE, o[0], o[stride]);
}

// ---- weight operand formats -------------------------------------------------------------------
// A weight code of include/vlfb.h names a PAIR: the format of the FPROP copy and the format of the DGRAD copy
// (with_weight_format below is the table).  Each format owns its addressing and its rounding; `plane` is
// Cout * taps * Cin, the elements of one copy.
//
// FPROP copies, order [Cout][taps][Cin] (idx is the element's index in the fp32 master):
template <typename T> struct WfElems {          // elements of T
  __device__ static __forceinline__ void st(void* base, long long idx, long long, float v) { Elem<T>::st(reinterpret_cast<T*>(base) + idx, v); }
};
struct WfTerms3 {                               // the three bf16 term planes of the split-bf16 forward, [term][...]
  __device__ static __forceinline__ void st(void* base, long long idx, long long plane, float v) { store_terms<3>(reinterpret_cast<bf16_t*>(base), idx, plane, v); }
};
struct WfScaled2 {                              // the two-plane fp16 forward (VLFB_MATH_F16X3): two scaled fp16 planes, [term][...]
  __device__ static __forceinline__ void st(void* base, long long idx, long long plane, float v) { store_scaled2(reinterpret_cast<unsigned short*>(base) + idx, plane, v); }
};
// DGRAD copies, order [Cin][taps][Cout]:
template <typename T> struct WdElems {          // elements of T
  static constexpr int kCoutMultiple = 1;
  __device__ static __forceinline__ void st(void* base, int ci, int tap, int co, int taps, int cout, long long, float v) {
    Elem<T>::st(reinterpret_cast<T*>(base) + ((long long)ci * taps + tap) * cout + co, v);
  }
};
struct WdTerms2 {                               // two bf16 term planes, [term][...]
  static constexpr int kCoutMultiple = 1;
  __device__ static __forceinline__ void st(void* base, int ci, int tap, int co, int taps, int cout, long long plane, float v) {
    store_terms<2>(reinterpret_cast<bf16_t*>(base), ((long long)ci * taps + tap) * cout + co, plane, v);
  }
};
// two scaled fp16 terms as [Cin][term][taps][Cout] -- the weight of a convolution with a doubled outermost tap dimension
// of dilation 0 (every tap is visited once per term), which the plain fp16 DGRAD kernels contract with the fp16 gradient:
// dX = dY . (Wh + Wl), 22 significant bits of W
struct WdScaled2 {
  static constexpr int kCoutMultiple = 1;
  __device__ static __forceinline__ void st(void* base, int ci, int tap, int co, int taps, int cout, long long, float v) {
    store_scaled2(reinterpret_cast<unsigned short*>(base) + ((long long)ci * 2 * taps + tap) * cout + co, (long long)taps * cout, v);
  }
};
// ... interleaved per 64-channel k-tile, [Cin][taps][Cout / 64][term][64] (the weight operand of VLFB_MATH_F16W2:
// gemm_nt_kernel<.., W2I>)
struct WdScaled2I {
  static constexpr int kCoutMultiple = 64;
  __device__ static __forceinline__ void st(void* base, int ci, int tap, int co, int taps, int cout, long long, float v) {
    store_scaled2(reinterpret_cast<unsigned short*>(base) + (((long long)ci * taps + tap) * cout + (co & ~63)) * 2 + (co & 63), 64, v);
  }
};

// w[Cout][taps][Cin] fp32 (+ scale[Cout]) -> fprop copy (same order) in the FPROP format F
template <typename F>
__global__ void weight_prep_fprop_kernel(const float* __restrict__ w, const float* __restrict__ scale,
                                         void* __restrict__ out, long long per_cout, long long total) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const float s = scale ? scale[i / per_cout] : 1.f;
    F::st(out, i, total, rounded_mul(w[i], s));
  }
}
// -> dgrad copy [Cin][taps][Cout] in the DGRAD format D; blockIdx.z = tap; 32x32 LDS tile transpose
template <typename D>
__global__ void weight_prep_dgrad_kernel(const float* __restrict__ w, const float* __restrict__ scale,
                                         void* __restrict__ out, int cout, int taps, int cin) {
  __shared__ float tile[32][33];
  const int tap = blockIdx.z;
  const int ci0 = blockIdx.x * 32, co0 = blockIdx.y * 32;
  for (int j = threadIdx.y; j < 32; j += blockDim.y) {
    int co = co0 + j, ci = ci0 + threadIdx.x;
    if (co < cout && ci < cin)
      tile[j][threadIdx.x] = rounded_mul(w[((long long)co * taps + tap) * cin + ci], scale ? scale[co] : 1.f);
  }
  __syncthreads();
  for (int j = threadIdx.y; j < 32; j += blockDim.y) {
    int ci = ci0 + j, co = co0 + threadIdx.x;
    if (co < cout && ci < cin)
      D::st(out, ci, tap, co, taps, cout, (long long)cout * taps * cin, tile[threadIdx.x][j]);
  }
}

// All convolutions of the model in ONE launch: blockIdx.x walks 32x32 (cout x cin) tiles of every
// (layer, tap); the tile is read once (coalesced along cin) and written twice: fprop order
// [cout][tap][cin] and dgrad order [cin][tap][cout] (transposed through LDS).
template <typename F, typename D>
__global__ void weight_prep_batched_kernel(const vlfb_wprep_item* __restrict__ items, int n_items) {
  __shared__ float tile[32][33];
  const int b = blockIdx.x;
  int lo = 0, hi = n_items - 1;          // last item whose first tile is <= b
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (items[mid].tile_begin <= b) lo = mid; else hi = mid - 1;
  }
  const vlfb_wprep_item it = items[lo];
  const int t = b - it.tile_begin;
  const int tiles_ci = (it.cin + 31) >> 5, tiles_co = (it.cout + 31) >> 5;
  const int ci0 = (t % tiles_ci) << 5;
  const int co0 = ((t / tiles_ci) % tiles_co) << 5;
  const int tap = t / (tiles_ci * tiles_co);
  const float* w = reinterpret_cast<const float*>(it.w);
  const float* scale = reinterpret_cast<const float*>(it.scale);
  void* wf = it.w_fprop;
  void* wd = it.w_dgrad;
  const long long plane = (long long)it.cout * it.taps * it.cin;
  for (int j = threadIdx.y; j < 32; j += blockDim.y) {
    const int co = co0 + j, ci = ci0 + threadIdx.x;
    if (co < it.cout && ci < it.cin) {
      const long long idx = ((long long)co * it.taps + tap) * it.cin + ci;
      const float v = rounded_mul(w[idx], scale ? scale[co] : 1.f);     // (no fma contraction into the term remainders)
      tile[j][threadIdx.x] = v;
      if (wf) F::st(wf, idx, plane, v);
    }
  }
  if (!wd) return;
  __syncthreads();
  for (int j = threadIdx.y; j < 32; j += blockDim.y) {
    const int ci = ci0 + j, co = co0 + threadIdx.x;
    if (co < it.cout && ci < it.cin)
      D::st(wd, ci, tap, co, it.taps, it.cout, plane, tile[threadIdx.x][j]);
  }
}

// THE table of weight codes, in the order of include/vlfb.h: code -> (FPROP copy format, DGRAD copy format).  Runs
// f(F{}, D{}); false, and no call, for a code that names no weight format.
template <typename Fn>
bool with_weight_format(int code, Fn&& f) {
  switch (code) {
    case VLFB_F32: f(WfElems<float>{}, WdElems<float>{}); return true;
    case VLFB_BF16: f(WfElems<bf16_t>{}, WdElems<bf16_t>{}); return true;
    case VLFB_F16: f(WfElems<f16_t>{}, WdElems<f16_t>{}); return true;
    case VLFB_SPLIT: f(WfTerms3{}, WdTerms2{}); return true;
    case VLFB_MIX: f(WfTerms3{}, WdElems<f16_t>{}); return true;
    case VLFB_MIX_W2: f(WfTerms3{}, WdScaled2{}); return true;
    case VLFB_MIXH: f(WfScaled2{}, WdElems<f16_t>{}); return true;
    case VLFB_MIXH_W2: f(WfScaled2{}, WdScaled2{}); return true;
    case VLFB_MIX_W2I: f(WfTerms3{}, WdScaled2I{}); return true;
    case VLFB_MIXH_W2I: f(WfScaled2{}, WdScaled2I{}); return true;
    default: return false;
  }
}
template <typename F, typename D>
int weight_prep_as(const float* w, const float* scale, void* w_fprop, void* w_dgrad, int64_t cout, int64_t taps, int64_t cin, hipStream_t s) {
  VLFB_REQUIRE(!w_dgrad || cout % D::kCoutMultiple == 0, "weight_prep: the interleaved two-term DGRAD copy needs Cout %% 64 == 0");
  VLFB_REQUIRE(taps < 65536, "weight_prep: too many taps");
  const long long total = cout * taps * cin;
  if (w_fprop)
    hipLaunchKernelGGL(weight_prep_fprop_kernel<F>, dim3(grid_for(total, 256)), dim3(256), 0, s, w, scale, w_fprop, (long long)(taps * cin), total);
  if (w_dgrad) {
    dim3 grid((unsigned)((cin + 31) / 32), (unsigned)((cout + 31) / 32), (unsigned)taps);
    hipLaunchKernelGGL(weight_prep_dgrad_kernel<D>, grid, dim3(32, 8), 0, s, w, scale, w_dgrad, (int)cout, (int)taps, (int)cin);
  }
  return check_launch("weight_prep");
}

// fp32 -> the two fp16 planes, and back
// (pure streaming passes, often next to a GEMM on the other stream: non-temporal accesses keep them out of the L2 that the
// GEMM's operand panels live in -- stream_ld / stream_st below; VLFB_NT_EPI=0 switches the hint off, as in the GEMM epilogues)
typedef unsigned int u32x4_s __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2_s __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint4 stream_ld16(bool nt, const void* p) {
  if (nt) { const u32x4_s t = __builtin_nontemporal_load(reinterpret_cast<const u32x4_s*>(p)); return make_uint4(t.x, t.y, t.z, t.w); }
  return *reinterpret_cast<const uint4*>(p);
}
__device__ __forceinline__ uint2 stream_ld8(bool nt, const void* p) {
  if (nt) { const u32x2_s t = __builtin_nontemporal_load(reinterpret_cast<const u32x2_s*>(p)); return make_uint2(t.x, t.y); }
  return *reinterpret_cast<const uint2*>(p);
}
__device__ __forceinline__ void stream_st16(bool nt, void* p, uint4 v) {
  if (nt) { const u32x4_s t = {v.x, v.y, v.z, v.w}; __builtin_nontemporal_store(t, reinterpret_cast<u32x4_s*>(p)); }
  else *reinterpret_cast<uint4*>(p) = v;
}
__device__ __forceinline__ void stream_st8(bool nt, void* p, uint2 v) {
  if (nt) { const u32x2_s t = {v.x, v.y}; __builtin_nontemporal_store(t, reinterpret_cast<u32x2_s*>(p)); }
  else *reinterpret_cast<uint2*>(p) = v;
}
static bool stream_nt() {
  static const bool on = env_int("VLFB_NT_EPI", 1) != 0;
  return on;
}
__global__ void pair_split_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst, long long n, bool nt) {
  for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (long long)gridDim.x * blockDim.x * 4) {
    const uint4 u = stream_ld16(nt, src + i);
    const float v[4] = {__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w)};
    uint32_t hi[2], lo[2];
    split2<f16_t>(v, hi, lo);
    stream_st8(nt, dst + i, make_uint2(hi[0], hi[1]));
    stream_st8(nt, dst + n + i, make_uint2(lo[0], lo[1]));
  }
}
__global__ void pair_join_kernel(const unsigned short* __restrict__ src, float* __restrict__ dst, long long n, bool nt) {
  for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (long long)gridDim.x * blockDim.x * 4) {
    const uint2 h = stream_ld8(nt, src + i), l = stream_ld8(nt, src + n + i);
    const float4 o = make_float4(h2f((unsigned short)(h.x & 0xffffu)) + h2f((unsigned short)(l.x & 0xffffu)), h2f((unsigned short)(h.x >> 16)) + h2f((unsigned short)(l.x >> 16)),
                                                      h2f((unsigned short)(h.y & 0xffffu)) + h2f((unsigned short)(l.y & 0xffffu)), h2f((unsigned short)(h.y >> 16)) + h2f((unsigned short)(l.y >> 16)));
    stream_st16(nt, dst + i, make_uint4(__float_as_uint(o.x), __float_as_uint(o.y), __float_as_uint(o.z), __float_as_uint(o.w)));
  }
}

// ---------------------------------------------------------------------------------------------
// row softmax (one wave per row; rows stay L1/L2-resident between the passes)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// 4 consecutive elements of T (16 / 8 bytes, naturally aligned) as floats
template <typename T>
__device__ __forceinline__ void load_elems4(const T* p, float (&v)[4]) {
  if (sizeof(T) == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    const uint2 t = *reinterpret_cast<const uint2*>(p);
    v[0] = Elem<T>::lo(t.x); v[1] = Elem<T>::hi(t.x);
    v[2] = Elem<T>::lo(t.y); v[3] = Elem<T>::hi(t.y);
  }
}

template <typename T>
__global__ void softmax_fwd_kernel(const float* __restrict__ s, T* __restrict__ p, long long rows,
                                   int cols, float scale) {
  const int lane = threadIdx.x & 63;
  const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
  for (long long r = wave; r < rows; r += nwaves) {
    const float* sr = s + r * cols;
    float m = -INFINITY;
    for (int c = lane; c < cols; c += 64) m = fmaxf(m, sr[c] * scale);
    m = wave_max(m);
    float sum = 0.f;
    for (int c = lane; c < cols; c += 64) sum += __expf(sr[c] * scale - m);
    sum = wave_sum(sum);
    const float inv = 1.0f / sum;
    T* pr = p + r * cols;
    for (int c = lane; c < cols; c += 64) Elem<T>::st(pr + c, __expf(sr[c] * scale - m) * inv);
  }
}
// Rows of at most 64*4*NV columns (cols % 4 == 0): the row is read ONCE with 16-byte loads and stays in
// registers (same arithmetic as above: max, exp, sum, scale), the result leaves as 4 packed elements
// per lane.  The non-local blocks have 784 (train) / 1024 (test crop) / 1568 (64 frames) columns.
template <typename T, int NV>
__global__ void softmax_fwd_rowreg_kernel(const float* __restrict__ s, T* __restrict__ p, long long rows,
                                          int cols, float scale) {
  const int lane = threadIdx.x & 63;
  const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
  const int nvec = cols >> 2;
  for (long long r = wave; r < rows; r += nwaves) {
    const float4* sr = reinterpret_cast<const float4*>(s + r * cols);
    float4 v[NV];
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (c < nvec) {
        float4 t = sr[c];
        t.x *= scale; t.y *= scale; t.z *= scale; t.w *= scale;
        v[i] = t;
        m = fmaxf(m, fmaxf(fmaxf(t.x, t.y), fmaxf(t.z, t.w)));
      }
    }
    m = wave_max(m);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      if (lane + 64 * i < nvec) {
        v[i].x = __expf(v[i].x - m); v[i].y = __expf(v[i].y - m);
        v[i].z = __expf(v[i].z - m); v[i].w = __expf(v[i].w - m);
        sum += (v[i].x + v[i].y) + (v[i].z + v[i].w);
      }
    }
    sum = wave_sum(sum);
    const float inv = 1.0f / sum;
    T* pr = p + r * cols;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (c < nvec) {
        if (sizeof(T) == 4) {
          *reinterpret_cast<float4*>(pr + 4 * c) = make_float4(v[i].x * inv, v[i].y * inv, v[i].z * inv, v[i].w * inv);
        } else {
          *reinterpret_cast<uint2*>(pr + 4 * c) = make_uint2(Elem<T>::pack2(v[i].x * inv, v[i].y * inv), Elem<T>::pack2(v[i].z * inv, v[i].w * inv));
        }
      }
    }
  }
}
template <typename T>
__global__ void softmax_bwd_kernel(const float* __restrict__ dp, const T* __restrict__ p,
                                   T* __restrict__ ds, long long rows, int cols, float scale) {
  const int lane = threadIdx.x & 63;
  const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
  for (long long r = wave; r < rows; r += nwaves) {
    const float* dr = dp + r * cols;
    const T* pr = p + r * cols;
    float dot = 0.f;
    for (int c = lane; c < cols; c += 64) dot += dr[c] * Elem<T>::ld(pr + c);
    dot = wave_sum(dot);
    T* o = ds + r * cols;
    for (int c = lane; c < cols; c += 64)
      Elem<T>::st(o + c, scale * Elem<T>::ld(pr + c) * (dr[c] - dot));
  }
}

// backward with the row resident in registers (same conditions as softmax_fwd_rowreg_kernel)
template <typename T, int NV, typename TD = T>
__global__ void softmax_bwd_rowreg_kernel(const float* __restrict__ dp, const T* __restrict__ p,
                                          TD* __restrict__ ds, long long rows, int cols, float scale) {
  const int lane = threadIdx.x & 63;
  const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
  const int nvec = cols >> 2;
  for (long long r = wave; r < rows; r += nwaves) {
    const float4* dr = reinterpret_cast<const float4*>(dp + r * cols);
    const T* pr = p + r * cols;
    float4 d[NV], q[NV];
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (c < nvec) {
        d[i] = dr[c];
        float t[4];
        load_elems4<T>(pr + 4 * c, t);
        q[i] = make_float4(t[0], t[1], t[2], t[3]);
        dot += (d[i].x * q[i].x + d[i].y * q[i].y) + (d[i].z * q[i].z + d[i].w * q[i].w);
      }
    }
    dot = wave_sum(dot);
    TD* o = ds + r * cols;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (c < nvec) {
        const float a = scale * q[i].x * (d[i].x - dot), b = scale * q[i].y * (d[i].y - dot);
        const float e = scale * q[i].z * (d[i].z - dot), f = scale * q[i].w * (d[i].w - dot);
        if (sizeof(TD) == 4) *reinterpret_cast<float4*>(o + 4 * c) = make_float4(a, b, e, f);
        else *reinterpret_cast<uint2*>(o + 4 * c) = make_uint2(Elem<TD>::pack2(a, b), Elem<TD>::pack2(e, f));
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// small elementwise
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void add_kernel(const T* a, const T* b, T* y, const T* __restrict__ mask, long long n,
                           int relu) {
  constexpr int V = Vec16<T>::N;
  const long long nv = n / V;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nv;
       i += (long long)gridDim.x * blockDim.x) {
    float x[V], z[V];
    Vec16<T>::load(a + i * V, x);
    if (b) {
      Vec16<T>::load(b + i * V, z);
#pragma unroll
      for (int k = 0; k < V; ++k) x[k] += z[k];
    }
    if (relu) {
#pragma unroll
      for (int k = 0; k < V; ++k) x[k] = fmaxf(x[k], 0.f);
    }
    if (mask) {
      Vec16<T>::load(mask + i * V, z);
#pragma unroll
      for (int k = 0; k < V; ++k) x[k] = z[k] > 0.f ? x[k] : 0.f;
    }
    Vec16<T>::store(y + i * V, x);
  }
  // tail
  for (long long i = nv * V + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    float x = Elem<T>::ld(a + i) + (b ? Elem<T>::ld(b + i) : 0.f);
    if (relu) x = fmaxf(x, 0.f);
    if (mask) x = Elem<T>::ld(mask + i) > 0.f ? x : 0.f;
    Elem<T>::st(y + i, x);
  }
}

// column sums: block = 16-byte channel-chunk lanes x row lanes over one row slab; 16-byte loads,
// LDS reduction over the row lanes, then one fp32 atomic per channel and slab.
// PARTIAL: every row slab leaves its sums in out[slab][cols] instead (a later pass folds the slabs in order: deterministic)
template <typename T, bool PARTIAL = false>
__global__ void colsum_kernel(const T* __restrict__ g, long long rows, int cols, long long ld,
                              float* __restrict__ out) {
  constexpr int V = Vec16<T>::N;
  constexpr int CL = 8;                 // chunk lanes (8 * V channels per block)
  constexpr int RL = 256 / CL;          // row lanes
  __shared__ float red[RL][CL * 8 + 1];
  const int cl = threadIdx.x % CL, rl = threadIdx.x / CL;
  const int c0 = (blockIdx.x * CL + cl) * V;
  const long long per = (rows + gridDim.y - 1) / gridDim.y;
  const long long r0 = (long long)blockIdx.y * per, r1 = min(rows, r0 + per);
  float acc[V];
#pragma unroll
  for (int k = 0; k < V; ++k) acc[k] = 0.f;
  if (c0 < cols) {
    for (long long r = r0 + rl; r < r1; r += RL) {
      float v[V];
      Vec16<T>::load(g + r * ld + c0, v);
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] += v[k];
    }
  }
#pragma unroll
  for (int k = 0; k < V; ++k) red[rl][cl * 8 + k] = acc[k];
  __syncthreads();
  if (rl < V && c0 < cols) {            // row lane k sums channel k of this chunk
    float sum = 0.f;
    for (int j = 0; j < RL; ++j) sum += red[j][cl * 8 + rl];
    if (PARTIAL) out[(long long)blockIdx.y * cols + c0 + rl] = sum;
    else atomicAdd(out + c0 + rl, sum);
  }
}

// strided 2-D copy (Concat along channels and its backward): dst[r*ldd + c] = src[r*lds + c]
template <typename T>
__global__ void copy2d_kernel(const T* __restrict__ src, long long lds, T* __restrict__ dst,
                              long long ldd, long long rows, long long cols) {
  const long long total = rows * cols;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / cols, c = i - r * cols;
    dst[r * ldd + c] = src[r * lds + c];
  }
}

__global__ void zero_kernel(float* p, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    p[i] = 0.f;
}

}  // namespace
}  // namespace vlfb

using namespace vlfb;

extern "C" const char* vlfb_last_error(void) { return g_err; }
extern "C" int vlfb_version(void) { return 100; }
extern "C" int vlfb_dtype_size(int dtype) { return dtype == VLFB_F32 ? 4 : is16(dtype) ? 2 : 0; }

extern "C" int vlfb_affine_nd_fwd(const float* x, const float* scale, const float* bias, float* y,
                                  int64_t n, int64_t c, int64_t inner, vlfb_stream_t stream) {
  VLFB_REQUIRE(x && scale && bias && y, "affine_nd_fwd: null pointer");
  VLFB_REQUIRE(n > 0 && c > 0 && inner > 0, "affine_nd_fwd: empty tensor");
  VLFB_REQUIRE(n * c * inner < (1ll << 31), "affine_nd_fwd: numel must stay below 2^31 (affine_nd_op.cu:69)");
  const long long rows = n * c;
  dim3 grid((unsigned)grid_for((inner + 3) / 4, 256, 64), (unsigned)(rows < 16384 ? rows : 16384));
  hipLaunchKernelGGL(affine_nd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, scale, bias,
                     y, rows, (int)c, (long long)inner);
  return check_launch("affine_nd_fwd");
}
extern "C" int vlfb_affine_nd_bwd(const float* dy, const float* scale, float* dx, int64_t n,
                                  int64_t c, int64_t inner, vlfb_stream_t stream) {
  VLFB_REQUIRE(dy && scale && dx, "affine_nd_bwd: null pointer");
  VLFB_REQUIRE(n > 0 && c > 0 && inner > 0, "affine_nd_bwd: empty tensor");
  VLFB_REQUIRE(n * c * inner < (1ll << 31), "affine_nd_bwd: numel must stay below 2^31");
  const long long rows = n * c;
  dim3 grid((unsigned)grid_for((inner + 3) / 4, 256, 64), (unsigned)(rows < 16384 ? rows : 16384));
  hipLaunchKernelGGL(affine_nd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, dy, scale,
                     (const float*)nullptr, dx, rows, (int)c, (long long)inner);
  return check_launch("affine_nd_bwd");
}

extern "C" int vlfb_ncthw_to_nthwc(const float* src, void* dst, int dtype, int64_t n, int64_t c,
                                   int64_t thw, int64_t c_pad, vlfb_stream_t stream) {
  VLFB_REQUIRE(src && dst && c_pad >= c && n > 0 && c > 0 && thw > 0, "ncthw_to_nthwc: bad args");
  int grid = grid_for(n * thw, 256);
  if (!with_elem(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(ncthw_to_nthwc_kernel<T>, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, (T*)dst, (long long)n, (int)c,
                           (long long)thw, (int)c_pad);
      }))
    return set_error(VLFB_ERR_ARG, "ncthw_to_nthwc: bad dtype");
  return check_launch("ncthw_to_nthwc");
}
extern "C" int vlfb_nthwc_to_ncthw(const void* src, float* dst, int dtype, int64_t n, int64_t c,
                                   int64_t thw, vlfb_stream_t stream) {
  VLFB_REQUIRE(src && dst && n > 0 && c > 0 && thw > 0, "nthwc_to_ncthw: bad args");
  int grid = grid_for(n * c * thw, 256);
  if (!with_elem(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(nthwc_to_ncthw_kernel<T>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const T*)src, dst, (long long)n, (int)c,
                           (long long)thw);
      }))
    return set_error(VLFB_ERR_ARG, "nthwc_to_ncthw: bad dtype");
  return check_launch("nthwc_to_ncthw");
}
// fp32 -> fp16 copy for the "mix" engine's backward (16 bytes read, 8 written per lane and step; positive values stay
// positive, f2h_pos)
__global__ void half_copy_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst, long long n4, long long n, bool nt) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const uint4 u = stream_ld16(nt, reinterpret_cast<const float4*>(src) + i);
    stream_st8(nt, reinterpret_cast<uint2*>(dst) + i, make_uint2(pack_h2_pos(__uint_as_float(u.x), __uint_as_float(u.y)), pack_h2_pos(__uint_as_float(u.z), __uint_as_float(u.w))));
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) dst[(n4 << 2) + threadIdx.x] = f2h_pos(src[(n4 << 2) + threadIdx.x]);
}
extern "C" int vlfb_half_copy(const float* src, void* dst, int64_t n, vlfb_stream_t stream) {
  VLFB_REQUIRE(src && dst && n >= 0, "half_copy: bad args");
  if (n == 0) return VLFB_OK;
  hipLaunchKernelGGL(half_copy_kernel, dim3(grid_for(n / 4 + 1, 256)), dim3(256), 0, (hipStream_t)stream, src,
                     (unsigned short*)dst, (long long)(n / 4), (long long)n, stream_nt());
  return check_launch("half_copy");
}
extern "C" int vlfb_pair_split(const float* src, void* dst_pair, int64_t n, vlfb_stream_t stream) {
  VLFB_REQUIRE(src && dst_pair && n >= 0 && n % 8 == 0, "pair_split: bad args (n must be a multiple of 8)");
  if (n == 0) return VLFB_OK;
  hipLaunchKernelGGL(pair_split_kernel, dim3(grid_for(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, src, (unsigned short*)dst_pair, (long long)n, stream_nt());
  return check_launch("pair_split");
}
extern "C" int vlfb_pair_join(const void* src_pair, float* dst, int64_t n, vlfb_stream_t stream) {
  VLFB_REQUIRE(src_pair && dst && n >= 0 && n % 8 == 0, "pair_join: bad args (n must be a multiple of 8)");
  if (n == 0) return VLFB_OK;
  hipLaunchKernelGGL(pair_join_kernel, dim3(grid_for(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)src_pair, dst, (long long)n, stream_nt());
  return check_launch("pair_join");
}
extern "C" int vlfb_cast(const void* src, int sd, void* dst, int dd, int64_t n, vlfb_stream_t stream) {
  VLFB_REQUIRE(src && dst && n >= 0, "cast: bad args");
  if (n == 0) return VLFB_OK;
  int grid = grid_for(n, 256);
  hipStream_t s = (hipStream_t)stream;
  if (sd == VLFB_F32 && is16(dd))
    VLFB_WITH_T16(dd, hipLaunchKernelGGL((cast_kernel<float, T16>), dim3(grid), dim3(256), 0, s, (const float*)src, (T16*)dst, (long long)n));
  else if (is16(sd) && dd == VLFB_F32)
    VLFB_WITH_T16(sd, hipLaunchKernelGGL((cast_kernel<T16, float>), dim3(grid), dim3(256), 0, s, (const T16*)src, (float*)dst, (long long)n));
  else if (sd == VLFB_F32 && dd == VLFB_F32)
    hipLaunchKernelGGL((cast_kernel<float, float>), dim3(grid), dim3(256), 0, s, (const float*)src, (float*)dst, (long long)n);
  else if (is16(sd) && sd == dd)
    VLFB_WITH_T16(dd, hipLaunchKernelGGL((cast_kernel<T16, T16>), dim3(grid), dim3(256), 0, s, (const T16*)src, (T16*)dst, (long long)n));
  else return set_error(VLFB_ERR_ARG, "cast: bad dtypes %d -> %d", sd, dd);
  return check_launch("cast");
}
extern "C" int vlfb_transpose2d(const void* src, void* dst, int dtype, int64_t batch, int64_t rows,
                                int64_t cols, vlfb_stream_t stream) {
  VLFB_REQUIRE(src && dst && batch > 0 && rows > 0 && cols > 0, "transpose2d: bad args");
  VLFB_REQUIRE(batch < 65536 && (rows + 31) / 32 < 65536, "transpose2d: grid too large");
  dim3 grid((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32), (unsigned)batch);
  dim3 block(32, 8);
  if (!with_elem(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(transpose2d_kernel<T>, grid, block, 0, (hipStream_t)stream, (const T*)src, (T*)dst, (long long)rows, (long long)cols);
      }))
    return set_error(VLFB_ERR_ARG, "transpose2d: bad dtype");
  return check_launch("transpose2d");
}
extern "C" int vlfb_weight_prep(const float* w, const float* scale, void* w_fprop, void* w_dgrad,
                                int dtype, int64_t cout, int64_t taps, int64_t cin,
                                vlfb_stream_t stream) {
  VLFB_REQUIRE(w && (w_fprop || w_dgrad) && cout > 0 && taps > 0 && cin > 0, "weight_prep: bad args");
  int rc = VLFB_OK;
  if (!with_weight_format(dtype, [&](auto f, auto d) {
        rc = weight_prep_as<decltype(f), decltype(d)>(w, scale, w_fprop, w_dgrad, cout, taps, cin, (hipStream_t)stream);
      }))
    return set_error(VLFB_ERR_ARG, "weight_prep: bad dtype");
  return rc;
}

extern "C" int vlfb_softmax_fwd(const float* s, void* p, int dtype, int64_t rows, int64_t cols,
                                float scale, vlfb_stream_t stream) {
  VLFB_REQUIRE(s && p && rows > 0 && cols > 0 && cols < (1ll << 31), "softmax_fwd: bad args");
  const dim3 grid(grid_for(rows * 64, 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  // rows of at most 1024 / 2048 columns stay in registers (4 / 8 values per lane); longer or ragged rows are re-read
  const bool rowreg = cols % 4 == 0 && cols <= 64 * 4 * 8, small = cols <= 64 * 4 * 4;
  if (!with_elem(dtype, [&](auto t) {
        using T = decltype(t);
        if (rowreg && small) hipLaunchKernelGGL((softmax_fwd_rowreg_kernel<T, 4>), grid, block, 0, st, s, (T*)p, (long long)rows, (int)cols, scale);
        else if (rowreg) hipLaunchKernelGGL((softmax_fwd_rowreg_kernel<T, 8>), grid, block, 0, st, s, (T*)p, (long long)rows, (int)cols, scale);
        else hipLaunchKernelGGL(softmax_fwd_kernel<T>, grid, block, 0, st, s, (T*)p, (long long)rows, (int)cols, scale);
      }))
    return set_error(VLFB_ERR_ARG, "softmax_fwd: bad dtype");
  return check_launch("softmax_fwd");
}
// probabilities in fp32, ds in a 16-bit type (the "mix" path: the softmax Jacobian cancels the common part of dP, so P
// is read at full precision and only the result is rounded)
extern "C" int vlfb_softmax_bwd_p32(const float* dp, const float* p, void* ds, int ds_dtype, int64_t rows,
                                    int64_t cols, float scale, vlfb_stream_t stream) {
  VLFB_REQUIRE(dp && p && ds && rows > 0 && cols > 0, "softmax_bwd_p32: bad args");
  VLFB_REQUIRE(is16(ds_dtype) && cols % 4 == 0 && cols <= 64 * 4 * 8, "softmax_bwd_p32: 16-bit ds and cols %% 4 == 0, cols <= 2048");
  const int grid = grid_for(rows * 64, 256);
  hipStream_t st = (hipStream_t)stream;
  if (cols <= 64 * 4 * 4)
    VLFB_WITH_T16(ds_dtype, hipLaunchKernelGGL((softmax_bwd_rowreg_kernel<float, 4, T16>), dim3(grid), dim3(256), 0, st, dp, p, (T16*)ds, (long long)rows, (int)cols, scale));
  else
    VLFB_WITH_T16(ds_dtype, hipLaunchKernelGGL((softmax_bwd_rowreg_kernel<float, 8, T16>), dim3(grid), dim3(256), 0, st, dp, p, (T16*)ds, (long long)rows, (int)cols, scale));
  return check_launch("softmax_bwd_p32");
}
extern "C" int vlfb_softmax_bwd(const float* dp, const void* p, void* ds, int dtype, int64_t rows,
                                int64_t cols, float scale, vlfb_stream_t stream) {
  VLFB_REQUIRE(dp && p && ds && rows > 0 && cols > 0 && cols < (1ll << 31), "softmax_bwd: bad args");
  const dim3 grid(grid_for(rows * 64, 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  const bool rowreg = cols % 4 == 0 && cols <= 64 * 4 * 8, small = cols <= 64 * 4 * 4;       // (as vlfb_softmax_fwd)
  if (!with_elem(dtype, [&](auto t) {
        using T = decltype(t);
        if (rowreg && small) hipLaunchKernelGGL((softmax_bwd_rowreg_kernel<T, 4>), grid, block, 0, st, dp, (const T*)p, (T*)ds, (long long)rows, (int)cols, scale);
        else if (rowreg) hipLaunchKernelGGL((softmax_bwd_rowreg_kernel<T, 8>), grid, block, 0, st, dp, (const T*)p, (T*)ds, (long long)rows, (int)cols, scale);
        else hipLaunchKernelGGL(softmax_bwd_kernel<T>, grid, block, 0, st, dp, (const T*)p, (T*)ds, (long long)rows, (int)cols, scale);
      }))
    return set_error(VLFB_ERR_ARG, "softmax_bwd: bad dtype");
  return check_launch("softmax_bwd");
}

extern "C" int vlfb_add(const void* a, const void* b, void* y, const void* mask, int dtype,
                        int64_t n, int relu, vlfb_stream_t stream) {
  VLFB_REQUIRE(a && y && n >= 0, "add: bad args");
  if (n == 0) return VLFB_OK;
  const int v = dtype == VLFB_F32 ? 4 : 8;
  int grid = grid_for((n + v - 1) / v, 256);
  if (!with_elem(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(add_kernel<T>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const T*)a, (const T*)b, (T*)y, (const T*)mask, (long long)n, relu);
      }))
    return set_error(VLFB_ERR_ARG, "add: bad dtype");
  return check_launch("add");
}
extern "C" int vlfb_relu_fwd(const void* x, void* y, int dtype, int64_t n, vlfb_stream_t stream) {
  return vlfb_add(x, nullptr, y, nullptr, dtype, n, 1, stream);
}
extern "C" int vlfb_relu_bwd(const void* dy, const void* yv, void* dx, int dtype, int64_t n,
                             vlfb_stream_t stream) {
  VLFB_REQUIRE(yv != nullptr, "relu_bwd: y is required");
  return vlfb_add(dy, nullptr, dx, yv, dtype, n, 0, stream);
}
namespace vlfb {
// row slabs of a column-sum launch over (rows x cols) elements of `dtype` (the grid's y extent)
int colsum_slabs(int dtype, long long rows, long long cols) {
  const int v = dtype == VLFB_F32 ? 4 : 8;
  const int cblocks = (int)((cols / v + 7) / 8);
  int slabs = (int)((rows + 1023) / 1024);
  const int want = (2048 + cblocks - 1) / cblocks;
  if (slabs > want) slabs = want;
  return slabs < 1 ? 1 : slabs;
}
// per-slab column sums into partials[colsum_slabs][cols] (no atomics: the caller folds the slabs in a fixed order)
int colsum_partials(const void* g, int dtype, long long rows, long long cols, long long ld, float* partials, hipStream_t s) {
  const int v = dtype == VLFB_F32 ? 4 : 8;
  VLFB_REQUIRE(g && partials && rows > 0 && cols > 0 && ld >= cols && cols % v == 0 && ld % v == 0 && dtype_ok(dtype), "colsum_partials: bad args");
  dim3 grid((unsigned)((cols / v + 7) / 8), (unsigned)colsum_slabs(dtype, rows, cols));
  with_elem(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((colsum_kernel<T, true>), grid, dim3(256), 0, s, (const T*)g, rows, (int)cols, ld, partials);
  });
  return check_launch("colsum (partials)");
}
}  // namespace vlfb

extern "C" int vlfb_colsum(const void* g, int dtype, int64_t rows, int64_t cols, int64_t ld,
                           float* out, int accumulate, vlfb_stream_t stream) {
  VLFB_REQUIRE(g && out && rows > 0 && cols > 0 && ld >= cols, "colsum: bad args");
  VLFB_REQUIRE(dtype_ok(dtype), "colsum: bad dtype");
  hipStream_t s = (hipStream_t)stream;
  const int v = dtype == VLFB_F32 ? 4 : 8;
  VLFB_REQUIRE(cols % v == 0 && ld % v == 0, "colsum: cols and ld must be multiples of %d", v);
  // (every argument check comes before the first launch: a rejected call leaves `out` as it was)
  if (!accumulate)
    hipLaunchKernelGGL(zero_kernel, dim3(grid_for(cols, 256)), dim3(256), 0, s, out, (long long)cols);
  const int cblocks = (int)((cols / v + 7) / 8);
  int slabs = (int)((rows + 1023) / 1024);
  const int want = (2048 + cblocks - 1) / cblocks;
  if (slabs > want) slabs = want;
  if (slabs < 1) slabs = 1;
  dim3 grid((unsigned)cblocks, (unsigned)slabs);
  with_elem(dtype, [&](auto t) {          // (dtype_ok above)
    using T = decltype(t);
    hipLaunchKernelGGL(colsum_kernel<T>, grid, dim3(256), 0, s, (const T*)g, (long long)rows, (int)cols, (long long)ld, out);
  });
  return check_launch("colsum");
}

extern "C" int vlfb_copy2d(const void* src, int64_t lds, void* dst, int64_t ldd, int dtype,
                           int64_t rows, int64_t cols, vlfb_stream_t stream) {
  VLFB_REQUIRE(src && dst && rows > 0 && cols > 0 && lds >= cols && ldd >= cols, "copy2d: bad args");
  int grid = grid_for(rows * cols, 256);
  if (!with_elem(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(copy2d_kernel<T>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const T*)src, (long long)lds, (T*)dst, (long long)ldd, (long long)rows, (long long)cols);
      }))
    return set_error(VLFB_ERR_ARG, "copy2d: bad dtype");
  return check_launch("copy2d");
}
extern "C" int vlfb_zero_f32(float* p, int64_t n, vlfb_stream_t stream) {
  VLFB_REQUIRE(p && n >= 0, "zero_f32: bad args");
  if (n == 0) return VLFB_OK;
  hipLaunchKernelGGL(zero_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, p, (long long)n);
  return check_launch("zero_f32");
}

extern "C" int vlfb_weight_prep_batched(const vlfb_wprep_item* items_dev, int n_items, int total_tiles,
                                        int dtype, vlfb_stream_t stream) {
  VLFB_REQUIRE(items_dev && n_items > 0 && total_tiles > 0, "weight_prep_batched: bad args");
  // (the items live on the device: the caller keeps Cout % 64 == 0 for those of an interleaved code, which
  // vlfb_weight_prep checks per conv)
  if (!with_weight_format(dtype, [&](auto f, auto d) {
        hipLaunchKernelGGL((weight_prep_batched_kernel<decltype(f), decltype(d)>), dim3((unsigned)total_tiles), dim3(32, 8), 0,
                           (hipStream_t)stream, items_dev, n_items);
      }))
    return set_error(VLFB_ERR_ARG, "weight_prep_batched: bad dtype");
  return check_launch("weight_prep_batched");
}

extern "C" int vlfb_ncthw_to_nthwc_wpad(const float* src, void* dst, int dtype, int64_t n, int64_t c,
                                        int64_t rows, int64_t w, int64_t c_pad, int64_t wpad_left,
                                        int64_t w_total, vlfb_stream_t stream) {
  VLFB_REQUIRE(src && dst && c_pad >= c && n > 0 && c > 0 && rows > 0 && w > 0 && wpad_left >= 0 &&
               w_total >= wpad_left + w, "ncthw_to_nthwc_wpad: bad args");
  int grid = grid_for(n * rows * w_total, 256);
  if (!with_elem(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(ncthw_to_nthwc_wpad_kernel<T>, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, (T*)dst, (long long)n, (int)c, (long long)rows, (int)w, (int)c_pad, (int)wpad_left, (int)w_total);
      }))
    return set_error(VLFB_ERR_ARG, "ncthw_to_nthwc_wpad: bad dtype");
  return check_launch("ncthw_to_nthwc_wpad");
}
