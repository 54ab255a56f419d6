// Pools (channels-last): max / average / global-average forward, the gather backwards.  One thread = one position x one
// 16-byte channel chunk; all are one-pass and HBM-bound (DESIGN.md section 3.7 has the routing of the max-pool backward and
// the order-of-operations contract of every kernel here; tests/pool_cases.py restates it on the CPU).
//
// Every piece more than one kernel needs is defined ONCE, in front of the kernels: the position decode (pool_pos), the
// element sources of the forward pools (PlainSrc / PairSrc), the arg-max format (ArgMax), the "keep where positive" select
// and the mask step of a dx.  A new pool variant is an instantiation of these.  What stays written more than once, and why,
// is said at the place (the covering-window walks of pool_bwd_kernel and avgpool_bwd_two_term_kernel; the dx tail and the
// y-mask of the fixed-window and band kernels; the packed-word code of the band kernel); profiles/pool_dedup_resources.txt
// and profiles/pool_dedup_ab.txt have the figures.
#include "vlfb_common.h"
#include <algorithm>
#include <type_traits>
#include <math.h>

namespace vlfb {
namespace {

struct PoolP {
  int N, Ti, Hi, Wi, C, To, Ho, Wo;
  int kt, kh, kw, st, sh, sw, pt, ph, pw;
};

// ---- position decode ----------------------------------------------------------------------------
// flat item index -> (n, t, h, w, channel chunk) of a [N][T][H][W][chunks] enumeration; pos = ((n * T + t) * H + h) * W + w
struct PoolPos {
  int n, t, h, w, cc;
  long long pos;
};
__device__ __forceinline__ PoolPos pool_pos(long long i, int T, int H, int W, int chunks) {
  PoolPos q;
  q.cc = (int)(i % chunks);
  q.pos = i / chunks;
  q.w = (int)(q.pos % W); long long r = q.pos / W;
  q.h = (int)(r % H); r /= H;
  q.t = (int)(r % T);
  q.n = (int)(r / T);
  return q;
}

// ---- element sources of the forward pools -------------------------------------------------------
// A source reads one chunk of V channels: Chunk::v holds the values the pool compares or sums.  For the max pool it also
// says what "nothing selected yet" is (none), how element k of a chunk is kept (take) and how the kept chunk is stored
// (store: the pooled value IS an input value, so it leaves in the format it came in).  avg_out is the type the average
// pools store.  `plane` is the element count of one plane of a two-plane tensor (unused by the plain source).
template <typename T>
struct PlainSrc {
  typedef T elem;
  typedef T avg_out;
  static constexpr int V = Vec16<T>::N;
  struct Chunk { float v[V]; };
  __device__ static __forceinline__ void load(const T* x, long long, Chunk& c) { Vec16<T>::load(x, c.v); }
  __device__ static __forceinline__ void none(Chunk& c) {
#pragma unroll
    for (int k = 0; k < V; ++k) c.v[k] = -INFINITY;
  }
  __device__ static __forceinline__ void take(Chunk& best, const Chunk& c, int k) { best.v[k] = c.v[k]; }
  __device__ static __forceinline__ void store(T* y, long long, const Chunk& c) { Vec16<T>::store(y, c.v); }
};
// Two-plane fp16 tensors (VLFB_F16PAIR: [2][numel] fp16, value = hi + lo; the forward activations of the "mix" path): the
// value is fl32(hi + lo); the max pool keeps the selected element's two planes (a copy, never a re-split of the sum); the
// average pools store fp32 (the head reads res5 through them: head_helper.py:37-40, 92-98)
struct PairSrc {
  typedef f16_t elem;
  typedef float avg_out;
  static constexpr int V = 8;
  struct Chunk { float v[V], h[V], l[V]; };
  __device__ static __forceinline__ void load(const f16_t* x, long long plane, Chunk& c) {
    Vec16<f16_t>::load(x, c.h);
    Vec16<f16_t>::load(x + plane, c.l);
#pragma unroll
    for (int k = 0; k < V; ++k) c.v[k] = c.h[k] + c.l[k];
  }
  __device__ static __forceinline__ void none(Chunk& c) {
#pragma unroll
    for (int k = 0; k < V; ++k) { c.v[k] = -INFINITY; c.h[k] = c.l[k] = 0.f; }
  }
  __device__ static __forceinline__ void take(Chunk& best, const Chunk& c, int k) { best.v[k] = c.v[k]; best.h[k] = c.h[k]; best.l[k] = c.l[k]; }
  __device__ static __forceinline__ void store(f16_t* y, long long plane, const Chunk& c) {
    Vec16<f16_t>::store(y, c.h);
    Vec16<f16_t>::store(y + plane, c.l);
  }
};
// V floats as V elements of O, 16 bytes per store (O = float with V = 8: two stores)
template <typename O, int V>
__device__ __forceinline__ void store_chunk(O* y, const float (&v)[V]) {
  constexpr int N = Vec16<O>::N;
  static_assert(V % N == 0, "whole 16-byte stores");
#pragma unroll
  for (int j = 0; j < V; j += N) {
    float t[N];
#pragma unroll
    for (int k = 0; k < N; ++k) t[k] = v[j + k];
    Vec16<O>::store(y + j, t);
  }
}

// ---- the arg-max format -------------------------------------------------------------------------
// What the max-pool forward saves for the backward: per pooled element the tap (a * kh + b) * kw + c of the first maximum,
// in the element order of the pooled tensor.  uint8_t (windows of at most 255 taps): one byte per element, the V bytes of a
// chunk written and read as one uint2 (V == 8) or one uint32 (V == 4).  uint16_t: one IdxT per element.
// store: the writer; load + tap: the reader (the taps of a chunk as loaded; tap k of them).
template <typename IdxT, int V> struct ArgMax;
template <int V> struct ArgMax<uint8_t, V> {
  typedef uint2 Taps;                      // (y unused for V == 4)
  __device__ static __forceinline__ void store(uint8_t* am, const int (&arg)[V]) {
    const uint32_t w0 = arg[0] | (arg[1] << 8) | (arg[2] << 16) | (arg[3] << 24);
    if (V == 8) *reinterpret_cast<uint2*>(am) = make_uint2(w0, arg[4 % V] | (arg[5 % V] << 8) | (arg[6 % V] << 16) | (arg[7 % V] << 24));
    else *reinterpret_cast<uint32_t*>(am) = w0;
  }
  __device__ static __forceinline__ Taps load(const uint8_t* am) {
    return V == 8 ? *reinterpret_cast<const uint2*>(am) : make_uint2(*reinterpret_cast<const uint32_t*>(am), 0u);
  }
  __device__ static __forceinline__ int tap(const Taps& t, int k) { return (int)(((k < 4 ? t.x : t.y) >> (8 * (k & 3))) & 0xff); }
};
template <int V> struct ArgMax<uint16_t, V> {
  struct Taps { uint16_t t[V]; };
  __device__ static __forceinline__ void store(uint16_t* am, const int (&arg)[V]) {
#pragma unroll
    for (int k = 0; k < V; ++k) am[k] = (uint16_t)arg[k];
  }
  __device__ static __forceinline__ Taps load(const uint16_t* am) {
    Taps t;
#pragma unroll
    for (int k = 0; k < V; ++k) t.t[k] = am[k];
    return t;
  }
  __device__ static __forceinline__ int tap(const Taps& t, int k) { return (int)t.t[k]; }
};

// ---- pieces of the backwards --------------------------------------------------------------------
// v = m > 0 ? v : 0 per element: the ReLU mask of a dx (m = the mask operand) and of a pooled gradient (m = the pooled
// values y: the selected element IS the pooled value, so "the input passed its ReLU" can be read from the window-times
// smaller pooled tensor instead of the input)
template <int V>
__device__ __forceinline__ void keep_where_positive(float (&v)[V], const float (&m)[V]) {
#pragma unroll
  for (int k = 0; k < V; ++k) v[k] = m[k] > 0.f ? v[k] : 0.f;
}
// the mask step of a backward alone: acc = mask > 0 ? acc : 0 (mask may be null)
template <typename T>
__device__ __forceinline__ void mask_dx(const T* mask, long long off, float (&acc)[Vec16<T>::N]) {
  if (mask) {
    float mk[Vec16<T>::N];
    Vec16<T>::load(mask + off, mk);
    keep_where_positive(acc, mk);
  }
}
// 16 bytes of T as floats
template <typename T>
__device__ __forceinline__ void unpack_vec(const uint4& t, float (&v)[Vec16<T>::N]) {
  if (sizeof(T) == 4) {
    v[0] = __uint_as_float(t.x); v[1] = __uint_as_float(t.y); v[2 % Vec16<T>::N] = __uint_as_float(t.z); v[3 % Vec16<T>::N] = __uint_as_float(t.w);
  } else {
    const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[(2 * i) % Vec16<T>::N] = Elem<T>::lo(w[i]);
      v[(2 * i + 1) % Vec16<T>::N] = Elem<T>::hi(w[i]);
    }
  }
}

// ---- forward ------------------------------------------------------------------------------------
// The window maximum: over the padded window in (a, b, c) order with a strict > from -inf -- the value and the tap of the
// FIRST maximum.
template <typename Src, typename IdxT>
__global__ void maxpool_fwd_kernel(const typename Src::elem* __restrict__ x, typename Src::elem* __restrict__ y,
                                   IdxT* __restrict__ argmax, PoolP p) {
  constexpr int V = Src::V;
  const int cchunks = p.C / V;
  const long long total = (long long)p.N * p.To * p.Ho * p.Wo * cchunks;
  const long long xplane = (long long)p.N * p.Ti * p.Hi * p.Wi * p.C, yplane = (long long)p.N * p.To * p.Ho * p.Wo * p.C;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const PoolPos o = pool_pos(i, p.To, p.Ho, p.Wo, cchunks);
    typename Src::Chunk best;
    Src::none(best);
    int arg[V];
#pragma unroll
    for (int k = 0; k < V; ++k) arg[k] = 0;
    for (int a = 0; a < p.kt; ++a) {
      const int ti = o.t * p.st - p.pt + a;
      if ((unsigned)ti >= (unsigned)p.Ti) continue;
      for (int b = 0; b < p.kh; ++b) {
        const int hi = o.h * p.sh - p.ph + b;
        if ((unsigned)hi >= (unsigned)p.Hi) continue;
        for (int c = 0; c < p.kw; ++c) {
          const int wi = o.w * p.sw - p.pw + c;
          if ((unsigned)wi >= (unsigned)p.Wi) continue;
          typename Src::Chunk v;
          Src::load(x + ((((long long)o.n * p.Ti + ti) * p.Hi + hi) * p.Wi + wi) * p.C + o.cc * V, xplane, v);
          const int tap = (a * p.kh + b) * p.kw + c;
#pragma unroll
          for (int k = 0; k < V; ++k)
            if (v.v[k] > best.v[k]) { Src::take(best, v, k); arg[k] = tap; }
        }
      }
    }
    const long long off = o.pos * p.C + o.cc * V;
    Src::store(y + off, yplane, best);
    if (argmax) ArgMax<IdxT, V>::store(argmax + off, arg);
  }
}

// The window mean (pad 0): taps ascending in (a, b, c) from +0, the value of a tap formed before it is added, one multiply
// by fl32(1 / window), one rounding to the output type.  No multiply inside the sum: nothing for the compiler to contract.
template <typename Src>
__global__ void avgpool_fwd_kernel(const typename Src::elem* __restrict__ x, typename Src::avg_out* __restrict__ y, PoolP p) {
  constexpr int V = Src::V;
  const int cchunks = p.C / V;
  const long long total = (long long)p.N * p.To * p.Ho * p.Wo * cchunks;
  const long long xplane = (long long)p.N * p.Ti * p.Hi * p.Wi * p.C;
  const float inv = 1.0f / (float)(p.kt * p.kh * p.kw);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const PoolPos o = pool_pos(i, p.To, p.Ho, p.Wo, cchunks);
    float acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
    for (int a = 0; a < p.kt; ++a)
      for (int b = 0; b < p.kh; ++b)
        for (int c = 0; c < p.kw; ++c) {
          const int ti = o.t * p.st + a, hi = o.h * p.sh + b, wi = o.w * p.sw + c;
          typename Src::Chunk v;
          Src::load(x + ((((long long)o.n * p.Ti + ti) * p.Hi + hi) * p.Wi + wi) * p.C + o.cc * V, xplane, v);
#pragma unroll
          for (int k = 0; k < V; ++k) acc[k] += v.v[k];
        }
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] *= inv;
    store_chunk(y + o.pos * p.C + o.cc * V, acc);
  }
}

// global average: y[n][c] = mean over `rows` positions.  block = (8 chunk lanes) x (32 row lanes): row lane rl sums rows
// rl, rl + 32, ... from +0, then the 32 partial sums are added in lane order from +0
template <typename Src>
__global__ void global_avgpool_kernel(const typename Src::elem* __restrict__ x, typename Src::avg_out* __restrict__ y, long long rows,
                                      int C, long long xplane) {
  constexpr int V = Src::V;
  __shared__ float red[32][8 * 8 + 1];
  const int cl = threadIdx.x & 7, rl = threadIdx.x >> 3;
  const int n = blockIdx.y;
  const int c0 = (blockIdx.x * 8 + cl) * V;
  float acc[V];
#pragma unroll
  for (int k = 0; k < V; ++k) acc[k] = 0.f;
  if (c0 < C) {
    const typename Src::elem* base = x + (long long)n * rows * C + c0;
    for (long long r = rl; r < rows; r += 32) {
      typename Src::Chunk v;
      Src::load(base + r * C, xplane, v);
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] += v.v[k];
    }
  }
#pragma unroll
  for (int k = 0; k < V; ++k) red[rl][cl * 8 + k] = acc[k];
  __syncthreads();
  if (rl == 0 && c0 < C) {
    const float inv = 1.0f / (float)rows;
    float out[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      float s = 0.f;
      for (int j = 0; j < 32; ++j) s += red[j][cl * 8 + k];
      out[k] = s * inv;
    }
    store_chunk(y + (long long)n * C + c0, out);
  }
}

// ---- backward -----------------------------------------------------------------------------------
// gather formulation of the pool backward: every input position sums the output gradients
// of the windows that (a) cover it and (b) for max pooling selected it.
template <typename T, bool IS_MAX, typename IdxT>
__global__ void pool_bwd_kernel(const T* __restrict__ dy, const IdxT* __restrict__ argmax,
                                T* dx, const T* add, const T* __restrict__ mask, PoolP p,
                                float inv_window, const T* __restrict__ ymask = nullptr) {
  constexpr int V = Vec16<T>::N;
  const int cchunks = p.C / V;
  const long long total = (long long)p.N * p.Ti * p.Hi * p.Wi * cchunks;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const PoolPos q = pool_pos(i, p.Ti, p.Hi, p.Wi, cchunks);
    float acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
    // The covering-window walk is written here and, without the pads, in avgpool_bwd_two_term_kernel.  As ONE function
    // that calls back per window it cost the max instances of this kernel SGPR spills the parent does not have (f16 / u8:
    // 0 -> 10, f16 / u16: 0 -> 5, fp32 / u16: 0 -> 1; they sit at the 106-SGPR limit), so each kernel keeps its text.
    // windows `to` with to*st - pt <= ti <= to*st - pt + kt - 1
    const int t_lo = max(0, (q.t + p.pt - p.kt + p.st) / p.st), t_hi = min(p.To - 1, (q.t + p.pt) / p.st);
    const int h_lo = max(0, (q.h + p.ph - p.kh + p.sh) / p.sh), h_hi = min(p.Ho - 1, (q.h + p.ph) / p.sh);
    const int w_lo = max(0, (q.w + p.pw - p.kw + p.sw) / p.sw), w_hi = min(p.Wo - 1, (q.w + p.pw) / p.sw);
    for (int to = t_lo; to <= t_hi; ++to) {
      const int a = q.t + p.pt - to * p.st;
      if (a < 0 || a >= p.kt) continue;
      for (int ho = h_lo; ho <= h_hi; ++ho) {
        const int b = q.h + p.ph - ho * p.sh;
        if (b < 0 || b >= p.kh) continue;
        for (int wo = w_lo; wo <= w_hi; ++wo) {
          const int c = q.w + p.pw - wo * p.sw;
          if (c < 0 || c >= p.kw) continue;
          const long long ooff = ((((long long)q.n * p.To + to) * p.Ho + ho) * p.Wo + wo) * p.C + q.cc * V;
          float g[V];
          Vec16<T>::load(dy + ooff, g);
          if constexpr (IS_MAX) {
            if (ymask) {
              float yv[V];
              Vec16<T>::load(ymask + ooff, yv);
              keep_where_positive(g, yv);
            }
            const int tap = (a * p.kh + b) * p.kw + c;
            const typename ArgMax<IdxT, V>::Taps taps = ArgMax<IdxT, V>::load(argmax + ooff);
#pragma unroll
            for (int k = 0; k < V; ++k)
              if (ArgMax<IdxT, V>::tap(taps, k) == tap) acc[k] += g[k];
          } else {
#pragma unroll
            for (int k = 0; k < V; ++k) acc[k] += g[k] * inv_window;
          }
        }
      }
    }
    // the tail: dx = mask > 0 ? acc + add : 0, rounded once (add and mask may be null; add may be dx itself)
    const long long off = q.pos * p.C + q.cc * V;
    if (add) {
      float a2[V];
      Vec16<T>::load(add + off, a2);
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] += a2[k];
    }
    mask_dx(mask, off, acc);
    Vec16<T>::store(dx + off, acc);
  }
}

// Max-pool backward for the window shapes the models use (pool1 1x3x3 / 1x2x2, pool2 2x1x1 / 2x1x1, the non-local
// 1x2x2 / 1x2x2 pools), with the window geometry as compile-time constants: the generic kernel above spends its time
// in 64-bit index divisions and data-dependent window loops (pool1 of the 8-clip step: 532 us for 0.57 GB of
// traffic).  One workgroup per input row (n, t, h): the row decode is scalar, the candidate windows of a position
// are at most ceil(k / s) per dimension and unroll completely, and the accumulation order (windows ascending in
// t, h, w) is the one of the generic kernel, so both give identical bits.
template <typename T, int KT, int KH, int KW, int ST, int SH, int SW, bool YMASK>
__global__ __launch_bounds__(128) void maxpool_bwd_fixed_kernel(const T* __restrict__ dy, const uint8_t* __restrict__ argmax,
                                                                T* dx, const T* add, const T* __restrict__ mask, PoolP p,
                                                                const T* __restrict__ ymask) {
  constexpr int V = Vec16<T>::N;
  constexpr int CT = (KT + ST - 1) / ST, CH = (KH + SH - 1) / SH, CW = (KW + SW - 1) / SW;
  const int cchunks = p.C / V;
  const int row = blockIdx.x;                       // (n * Ti + ti) * Hi + hi
  const int hi = row % p.Hi;
  const int r2 = row / p.Hi;
  const int ti = r2 % p.Ti;
  const int n = r2 / p.Ti;
  const int items = p.Wi * cchunks;
  const int to_hi = (ti + p.pt) / ST, ho_hi = (hi + p.ph) / SH;
  for (int it = threadIdx.x; it < items; it += 128) {
    // item -> (w, channel chunk), w running through one residue class mod SW after the other
    const int wj = it / cchunks, cc = it - wj * cchunks;
    int wi = wj;
    if (SW > 1) {
      // classes 0 .. SW-1 hold ceil / floor (Wi / SW) positions; walk them in order
      int cls = 0, base = 0;
#pragma unroll
      for (int q = 0; q < SW - 1; ++q) {
        const int cnt = (p.Wi - q + SW - 1) / SW;
        if (wj >= base + cnt) { base += cnt; cls = q + 1; }
      }
      wi = (wj - base) * SW + cls;
    }
    const int wo_hi = (wi + p.pw) / SW;
    float acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
    // Candidate windows in t and h are workgroup-uniform: those that do not exist are skipped by scalar branches.
    // The w candidates of a position are all loaded, unconditionally and before any of them is used (a window that
    // does not exist reads window 0 and is compared against a tap no arg-max holds): the loads of a position are
    // in flight together instead of one round trip after the other.
#pragma unroll
    for (int jt = CT - 1; jt >= 0; --jt) {
      const int to = to_hi - jt, a = ti + p.pt - to * ST;
      if (to < 0 || to >= p.To || a >= KT) continue;
#pragma unroll
      for (int jh = CH - 1; jh >= 0; --jh) {
        const int ho = ho_hi - jh, b = hi + p.ph - ho * SH;
        if (ho < 0 || ho >= p.Ho || b >= KH) continue;
        const int orow = ((n * p.To + to) * p.Ho + ho) * p.Wo;
        uint4 gq[CW], yq[CW];
        typename ArgMax<uint8_t, V>::Taps aq[CW];
        int tapq[CW];
#pragma unroll
        for (int jw = 0; jw < CW; ++jw) {
          const int wo = wo_hi - (CW - 1 - jw), c = wi + p.pw - wo * SW;
          const bool ok = wo >= 0 && wo < p.Wo && c < KW;
          const long long o = ok ? (long long)(orow + wo) * p.C + cc * V : (long long)(cc * V);
          tapq[jw] = ok ? (a * KH + b) * KW + c : 255;
          gq[jw] = *reinterpret_cast<const uint4*>(dy + o);
          if (YMASK) yq[jw] = *reinterpret_cast<const uint4*>(ymask + o);
          aq[jw] = ArgMax<uint8_t, V>::load(argmax + o);
        }
#pragma unroll
        for (int jw = 0; jw < CW; ++jw) {
          float g[V];
          unpack_vec<T>(gq[jw], g);
          if (YMASK) {
            float yv[V];
            unpack_vec<T>(yq[jw], yv);
#pragma unroll
            for (int k = 0; k < V; ++k) g[k] = yv[k] > 0.f ? g[k] : 0.f;       // (own text, as the dx tail below)
          }
#pragma unroll
          for (int k = 0; k < V; ++k) acc[k] += ArgMax<uint8_t, V>::tap(aq[jw], k) == tapq[jw] ? g[k] : 0.f;
        }
      }
    }
    // (the dx tail in this kernel's own text: through the shared functions the compiler schedules this kernel differently,
    // measured +2 % on the pool launches of the mix step -- profiles/pool_dedup_ab.txt)
    const long long off = ((long long)row * p.Wi + wi) * p.C + cc * V;
    if (add) {
      float a2[V];
      Vec16<T>::load(add + off, a2);
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] += a2[k];
    }
    if (mask) {
      float mk[V];
      Vec16<T>::load(mask + off, mk);
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] = mk[k] > 0.f ? acc[k] : 0.f;
    }
    Vec16<T>::store(dx + off, acc);
  }
}

// pool1 (1x3x3 windows, stride 1x2x2): overlapping windows, so the row kernel above reads every pooled row for up to
// three input rows (PMC: 762 MB fetched for 257 MB of pooled gradient / arg-max / pooled output at 8 clips).  Here a
// workgroup owns a band of 2R input rows of one frame: the R + 2 pooled rows the band can touch are staged in LDS once
// -- the gradient already masked by the pooled output's sign, the arg-max bytes beside it -- and every input position
// then sums its (at most 2 x 2) candidate windows out of LDS, in the order of the kernels above (windows ascending in h,
// then w), so the bits are the same.  Pooled rows are read (R + 2) / R times per 2R input rows instead of 3 times per 2.
// (The y-mask of the staging loop and the tap compare of the sum work on PACKED words -- other algorithms than
// keep_where_positive / ArgMax::tap on the same formats -- and keep their own text.)
template <typename T, bool YMASK>
__global__ __launch_bounds__(256) void maxpool_bwd_band_kernel(const T* __restrict__ dy, const uint8_t* __restrict__ argmax,
                                                               T* dx, const T* add, const T* __restrict__ mask, PoolP p,
                                                               const T* __restrict__ ymask, int R, int bands) {
  constexpr int V = Vec16<T>::N;                      // elements per 16 bytes
  extern __shared__ __attribute__((aligned(16))) unsigned char band_lds[];
  const int cch = p.C / V;
  const int NR = R + 2;
  const int rowv = p.Wo * cch;                        // 16-byte vectors per pooled row
  uint4* g_l = reinterpret_cast<uint4*>(band_lds);
  unsigned char* t_l = band_lds + (size_t)NR * rowv * 16;
  const int band = blockIdx.x % bands, frame = blockIdx.x / bands;       // frame = n * Ti + ti  (kt = st = 1, pt = 0)
  const int h0 = band * 2 * R;
  const int hb = (h0 + p.ph) / 2 - 1;                 // first pooled row staged
  for (int i = threadIdx.x; i < NR * rowv; i += 256) {
    const int r = i / rowv, ho = hb + r;
    uint4 g = make_uint4(0u, 0u, 0u, 0u);
    uint2 tp = make_uint2(0xffffffffu, 0xffffffffu);
    if (ho >= 0 && ho < p.Ho) {
      const long long o = ((long long)(frame * p.Ho + ho) * rowv + (i - r * rowv)) * V;
      g = *reinterpret_cast<const uint4*>(dy + o);
      tp = ArgMax<uint8_t, V>::load(argmax + o);
      if (YMASK) {
        const uint4 yq = *reinterpret_cast<const uint4*>(ymask + o);
        float yv[V];
        unpack_vec<T>(yq, yv);
        uint32_t w[4] = {g.x, g.y, g.z, g.w};
        if (sizeof(T) == 4) {
#pragma unroll
          for (int k = 0; k < 4; ++k) w[k] = yv[k % V] > 0.f ? w[k] : 0u;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            w[k] = (yv[(2 * k) % V] > 0.f ? (w[k] & 0xffffu) : 0u) | (yv[(2 * k + 1) % V] > 0.f ? (w[k] & 0xffff0000u) : 0u);
        }
        g = make_uint4(w[0], w[1], w[2], w[3]);
      }
    }
    g_l[i] = g;
    if (V == 8) *reinterpret_cast<uint2*>(t_l + (size_t)i * 8) = tp;
    else *reinterpret_cast<uint32_t*>(t_l + (size_t)i * 4) = tp.x;
  }
  __syncthreads();
  const int rows = min(2 * R, p.Hi - h0);
  const int rowi = p.Wi * cch;                        // items per input row
  for (int it = threadIdx.x; it < rows * rowi; it += 256) {
    const int hr = it / rowi, rem = it - hr * rowi;
    const int wi = rem / cch, cc = rem - wi * cch;
    const int hi = h0 + hr;
    const int ho_hi = (hi + p.ph) / 2, wo_hi = (wi + p.pw) / 2;
    float acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
#pragma unroll
    for (int jh = 1; jh >= 0; --jh) {
      const int ho = ho_hi - jh, b = hi + p.ph - ho * 2;
      const bool okh = ho >= 0 && ho < p.Ho && b < 3;
      const int lr = okh ? ho - hb : 0;
#pragma unroll
      for (int jw = 1; jw >= 0; --jw) {
        const int wo = wo_hi - jw, c = wi + p.pw - wo * 2;
        const bool ok = okh && wo >= 0 && wo < p.Wo && c < 3;
        const int idx = ok ? (lr * p.Wo + wo) * cch + cc : cc;
        const int tap = ok ? b * 3 + c : 255;
        const uint4 gq = g_l[idx];
        uint2 aq;
        if (V == 8) aq = *reinterpret_cast<const uint2*>(t_l + (size_t)idx * 8);
        else aq = make_uint2(*reinterpret_cast<const uint32_t*>(t_l + (size_t)idx * 4), 0u);
        // keep the elements whose arg-max byte equals this tap, on the packed words: bytes of (arg-max ^ tap) that
        // are zero -> 0xff, widened to the element width by a byte permute, AND-ed onto the gradient bits (a dropped
        // element adds +0.0f exactly like the select of the kernels above)
        const uint32_t tapw = (uint32_t)tap * 0x01010101u;
        uint32_t fullb[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const uint32_t t = (q ? aq.y : aq.x) ^ tapw;
          const uint32_t nz = (((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t) & 0x80808080u;     // 0x80 where the byte differs
          fullb[q] = ((nz ^ 0x80808080u) >> 7) * 0xffu;                                   // 0xff where it matches
        }
        uint32_t w[4] = {gq.x, gq.y, gq.z, gq.w};
        if (sizeof(T) == 4) {
#pragma unroll
          for (int k = 0; k < 4; ++k) w[k] &= __builtin_amdgcn_perm(fullb[0], fullb[0], 0x01010101u * (uint32_t)k);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            w[k] &= __builtin_amdgcn_perm(fullb[k >> 1], fullb[k >> 1], (k & 1) ? 0x03030202u : 0x01010000u);
        }
        float g[V];
        unpack_vec<T>(make_uint4(w[0], w[1], w[2], w[3]), g);
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] += g[k];
      }
    }
    // (the dx tail in this kernel's own text: through the shared functions the compiler schedules this kernel differently,
    // measured +2 % on the pool launches of the mix step -- profiles/pool_dedup_ab.txt)
    const long long off = (((long long)frame * p.Hi + hi) * p.Wi + wi) * p.C + cc * V;
    if (add) {
      float a2[V];
      Vec16<T>::load(add + off, a2);
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] += a2[k];
    }
    if (mask) {
      float mk[V];
      Vec16<T>::load(mask + off, mk);
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] = mk[k] > 0.f ? acc[k] : 0.f;
    }
    Vec16<T>::store(dx + off, acc);
  }
}

// Average-pool backward from an fp32 pooled gradient into a TWO-TERM 16-bit input gradient: dx = mask > 0 ? sum dy / window : 0,
// hi = T(dx), lo = T(dx - hi).  Where the "mix" path's fp32 head gradient re-enters the 16-bit backward (the temporal / global
// average pool over res5): every position of a channel receives the SAME value, so a one-term rounding is an error common to all
// positions -- and to every backbone gradient behind it (it was their median error).
template <typename T>
__global__ void avgpool_bwd_two_term_kernel(const float* __restrict__ dy, T* __restrict__ dx_hi, T* __restrict__ dx_lo,
                                            const T* __restrict__ mask, PoolP p, float inv_window) {
  constexpr int V = 8;
  const int cchunks = p.C / V;
  const long long total = (long long)p.N * p.Ti * p.Hi * p.Wi * cchunks;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const PoolPos q = pool_pos(i, p.Ti, p.Hi, p.Wi, cchunks);
    float acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
    // (the walk of pool_bwd_kernel with the pads at 0, which leaves one test per dimension; the reason it is written twice
    // is given there)
    const int t_lo = max(0, (q.t - p.kt + p.st) / p.st), t_hi = min(p.To - 1, q.t / p.st);
    const int h_lo = max(0, (q.h - p.kh + p.sh) / p.sh), h_hi = min(p.Ho - 1, q.h / p.sh);
    const int w_lo = max(0, (q.w - p.kw + p.sw) / p.sw), w_hi = min(p.Wo - 1, q.w / p.sw);
    for (int to = t_lo; to <= t_hi; ++to) {
      if (q.t - to * p.st >= p.kt) continue;
      for (int ho = h_lo; ho <= h_hi; ++ho) {
        if (q.h - ho * p.sh >= p.kh) continue;
        for (int wo = w_lo; wo <= w_hi; ++wo) {
          if (q.w - wo * p.sw >= p.kw) continue;
          const float* g = dy + ((((long long)q.n * p.To + to) * p.Ho + ho) * p.Wo + wo) * p.C + q.cc * V;
          const float4 g0 = *reinterpret_cast<const float4*>(g), g1 = *reinterpret_cast<const float4*>(g + 4);
          acc[0] += g0.x * inv_window; acc[1] += g0.y * inv_window; acc[2] += g0.z * inv_window; acc[3] += g0.w * inv_window;
          acc[4] += g1.x * inv_window; acc[5] += g1.y * inv_window; acc[6] += g1.z * inv_window; acc[7] += g1.w * inv_window;
        }
      }
    }
    const long long off = q.pos * p.C + q.cc * V;
    mask_dx(mask, off, acc);
    Vec16<T>::store(dx_hi + off, acc);
    float h[V];
    Vec16<T>::load(dx_hi + off, h);                  // (the rounded values, as stored)
#pragma unroll
    for (int k = 0; k < V; ++k) h[k] = acc[k] - h[k];
    Vec16<T>::store(dx_lo + off, h);
  }
}

// ---- host ---------------------------------------------------------------------------------------
// Which kernel the max-pool backward runs: ONE pure host function, read by the launch code below and printed by
// vlfb_maxpool_bwd_describe (include/vlfb.h states the rule), so the route a test names is the route that runs.
enum class PoolBwdKind : int { generic, fixed, band };
struct PoolBwdRoute {
  PoolBwdKind kind;
  int window;          // fixed: index into kPoolFixedWindows
  int R, bands;        // band: input-row pairs per workgroup, workgroups per frame
  bool ymask, wide;    // the pooled values are the ReLU mask; two-byte arg-max
};
struct PoolWindow { int kt, kh, kw, st, sh, sw; };
constexpr PoolWindow kPoolFixedWindows[3] = {{1, 3, 3, 1, 2, 2}, {2, 1, 1, 2, 1, 1}, {1, 2, 2, 1, 2, 2}};
PoolBwdRoute maxpool_bwd_route(const PoolP& p, int elem_bytes, int argmax_bytes, bool has_add, bool has_mask, bool has_y) {
  PoolBwdRoute r = {PoolBwdKind::generic, -1, 0, 0, has_y, argmax_bytes == 2};
  if (r.wide) return r;
  // (the fixed-shape kernels index rows and pooled positions with 32 bits)
  if ((long long)p.N * p.Ti * p.Hi >= (1ll << 31) || (long long)p.N * p.To * p.Ho * p.Wo >= (1ll << 31)) return r;
  // (with a residual operand and a ReLU mask streamed beside it the row kernel is the faster one: 271 vs 357 us)
  if (p.kt == 1 && p.kh == 3 && p.kw == 3 && p.st == 1 && p.sh == 2 && p.sw == 2 && p.pt == 0 && p.To == p.Ti && !has_add &&
      !has_mask) {
    // band kernel: as many input-row pairs per workgroup as 64 KB of LDS hold pooled rows for (R + 2 rows staged)
    const long long row_bytes = (long long)p.Wo * p.C * (elem_bytes + 1);
    // R = 3: measured 226 us at R = 2 and 3, 259 us at R = 4 (two 64 KB workgroups per CU leave the load and the store
    // phases of a CU unbalanced) against 285 us for the row kernel, pool1 of the 8-clip step in isolation
    const int R = (int)std::min<long long>(3, 65536 / row_bytes - 2);
    if (R >= 2) {
      const int bands = (p.Hi + 2 * R - 1) / (2 * R);
      if ((long long)p.N * p.Ti * bands < (1ll << 31)) {
        r.kind = PoolBwdKind::band; r.R = R; r.bands = bands;
        return r;
      }
    }
  }
  for (int i = 0; i < 3; ++i) {
    const PoolWindow& w = kPoolFixedWindows[i];
    if (p.kt == w.kt && p.kh == w.kh && p.kw == w.kw && p.st == w.st && p.sh == w.sh && p.sw == w.sw) {
      r.kind = PoolBwdKind::fixed; r.window = i;
      return r;
    }
  }
  return r;
}

// f(std::true_type / std::false_type): a runtime condition as a template argument of the launch (YMASK)
template <typename F>
void with_flag(bool on, F&& f) {
  if (on) f(std::true_type{}); else f(std::false_type{});
}
// f(Src{}) with the element source of the forward pools `dtype` names (check_pool has accepted the code)
template <typename F>
void with_src(int dtype, F&& f) {
  if (dtype == VLFB_F16PAIR) f(PairSrc{});
  else with_elem(dtype, [&](auto t) { f(PlainSrc<decltype(t)>{}); });
}
// elements per 16-byte chunk of a tensor of `dtype` (the two-plane format: per plane)
int vec_of(int dtype) { return dtype == VLFB_F32 ? 4 : 8; }

// launches the band / fixed-shape kernel the route names (one-byte arg-max); the generic kernel is the caller's
template <typename T>
void launch_maxpool_bwd_fixed(const PoolBwdRoute& r, const PoolP& p, const void* dy, const void* argmax, void* dx, const void* add,
                              const void* mask, const void* ymask, hipStream_t s) {
  if (r.kind == PoolBwdKind::band) {
    const int R = r.R, bands = r.bands;
    const long long row_bytes = (long long)p.Wo * p.C * (sizeof(T) + 1);
    const long long wgs = (long long)p.N * p.Ti * bands;
    const size_t lds = (size_t)(R + 2) * row_bytes;
    with_flag(ymask != nullptr, [&](auto ym) {
      hipLaunchKernelGGL((maxpool_bwd_band_kernel<T, decltype(ym)::value>), dim3((unsigned)wgs), dim3(256), lds, s, (const T*)dy,
                         (const uint8_t*)argmax, (T*)dx, (const T*)add, (const T*)mask, p, (const T*)ymask, R, bands);
    });
    return;
  }
  const dim3 grid((unsigned)((long long)p.N * p.Ti * p.Hi)), block(128);
#define VLFB_POOL_FIXED(I_, KT_, KH_, KW_, ST_, SH_, SW_)                                                                  \
  static_assert(kPoolFixedWindows[I_].kt == KT_ && kPoolFixedWindows[I_].kh == KH_ && kPoolFixedWindows[I_].kw == KW_ &&   \
                kPoolFixedWindows[I_].st == ST_ && kPoolFixedWindows[I_].sh == SH_ && kPoolFixedWindows[I_].sw == SW_,     \
                "the compiled windows are the routed windows");                                                           \
  if (r.window == I_) {                                                                                                  \
    with_flag(ymask != nullptr, [&](auto ym) {                                                                           \
      hipLaunchKernelGGL((maxpool_bwd_fixed_kernel<T, KT_, KH_, KW_, ST_, SH_, SW_, decltype(ym)::value>), grid, block, 0, s, \
                         (const T*)dy, (const uint8_t*)argmax, (T*)dx, (const T*)add, (const T*)mask, p, (const T*)ymask); \
    });                                                                                                                  \
    return;                                                                                                              \
  }
  VLFB_POOL_FIXED(0, 1, 3, 3, 1, 2, 2)
  VLFB_POOL_FIXED(1, 2, 1, 1, 2, 1, 1)
  VLFB_POOL_FIXED(2, 1, 2, 2, 1, 2, 2)
#undef VLFB_POOL_FIXED
}

PoolP to_poolp(const vlfb_pool_desc* d) {
  PoolP p;
  p.N = d->N; p.Ti = d->Ti; p.Hi = d->Hi; p.Wi = d->Wi; p.C = d->C;
  p.To = d->To; p.Ho = d->Ho; p.Wo = d->Wo;
  p.kt = d->kt; p.kh = d->kh; p.kw = d->kw; p.st = d->st; p.sh = d->sh; p.sw = d->sw;
  p.pt = d->pt; p.ph = d->ph; p.pw = d->pw;
  return p;
}
// Descriptor checks shared by every pool entry point, before anything is launched.  The kernels trust the descriptor: the
// average pools read hi = ho*sh + b with no bounds test, the max-pool forward would write -inf / tap 0 for a window with no
// valid tap -- so an output extent the input does not carry is an argument error here, with the dimension named.
int check_pool(const vlfb_pool_desc* d, bool is_max) {
  VLFB_REQUIRE(d->dtype == VLFB_F32 || is16(d->dtype) || d->dtype == VLFB_F16PAIR, "pool: bad dtype");
  const int v = vec_of(d->dtype);
  VLFB_REQUIRE(d->N > 0 && d->C > 0, "pool: N=%d and C=%d must be positive", d->N, d->C);
  VLFB_REQUIRE(d->C % v == 0, "pool: C=%d must be a multiple of %d", d->C, v);
  const struct { const char* n; int in, out, k, s, p; } dims[3] = {{"t", d->Ti, d->To, d->kt, d->st, d->pt},
                                                                   {"h", d->Hi, d->Ho, d->kh, d->sh, d->ph},
                                                                   {"w", d->Wi, d->Wo, d->kw, d->sw, d->pw}};
  for (const auto& a : dims) {
    VLFB_REQUIRE(a.in > 0 && a.out > 0 && a.k > 0 && a.s > 0, "pool: dimension %s: input %d, output %d, kernel %d and stride %d must be positive",
                 a.n, a.in, a.out, a.k, a.s);
    VLFB_REQUIRE(a.p >= 0 && a.p < a.k, "pool: dimension %s: pad %d must be in [0, kernel %d)", a.n, a.p, a.k);
    if (is_max)
      VLFB_REQUIRE((long long)(a.out - 1) * a.s - a.p <= a.in - 1,
                   "pool: dimension %s: the last of %d windows (stride %d, pad %d) has no tap inside the input extent %d", a.n, a.out,
                   a.s, a.p, a.in);
    else
      VLFB_REQUIRE((long long)(a.out - 1) * a.s + a.k <= a.in,
                   "pool: dimension %s: the last of %d windows (kernel %d, stride %d) leaves the input extent %d", a.n, a.out, a.k,
                   a.s, a.in);
  }
  VLFB_REQUIRE((long long)d->kt * d->kh * d->kw <= 65535, "pool: window too large for a 16-bit argmax");
  return VLFB_OK;
}
// ... of the average pools: every window inside the input, no padding
int check_avgpool(const vlfb_pool_desc* d) {
  const int rc = check_pool(d, false);
  if (rc) return rc;
  VLFB_REQUIRE(d->pt == 0 && d->ph == 0 && d->pw == 0, "avgpool: padding is not supported (none in the reference)");
  return VLFB_OK;
}

}  // namespace
}  // namespace vlfb

using namespace vlfb;

extern "C" int vlfb_pool_argmax_bytes(const vlfb_pool_desc* d) {
  return d->kt * d->kh * d->kw <= 255 ? 1 : 2;
}
extern "C" int vlfb_maxpool_fwd(const vlfb_pool_desc* d, const void* x, void* y, void* argmax,
                                vlfb_stream_t stream) {
  int rc = check_pool(d, true);
  if (rc) return rc;
  VLFB_REQUIRE(x && y, "maxpool_fwd: null pointer");
  PoolP p = to_poolp(d);
  const bool wide = vlfb_pool_argmax_bytes(d) == 2;
  int grid = grid_for((long long)p.N * p.To * p.Ho * p.Wo * (p.C / vec_of(d->dtype)), 256);
  with_src(d->dtype, [&](auto src) {
    with_argmax(wide, [&](auto i) {
      using S = decltype(src);
      using E = typename S::elem;
      using I = decltype(i);
      hipLaunchKernelGGL((maxpool_fwd_kernel<S, I>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const E*)x, (E*)y, (I*)argmax, p);
    });
  });
  return check_launch(d->dtype == VLFB_F16PAIR ? "maxpool_fwd (fp16 planes)" : "maxpool_fwd");
}
// max-pool backward: the gradient gathered through the arg-max, plus `add` and masked by `mask > 0` (vlfb_maxpool_bwd), or
// masked by the pooled values `y` themselves (vlfb_maxpool_relu_bwd); the pointers the other form has are null
static int maxpool_bwd_impl(const vlfb_pool_desc* d, const void* dy, const void* argmax, void* dx, const void* add, const void* mask,
                            const void* y, hipStream_t s, const char* what_fixed, const char* what) {
  PoolP p = to_poolp(d);
  const bool wide = vlfb_pool_argmax_bytes(d) == 2;
  int grid = grid_for((long long)p.N * p.Ti * p.Hi * p.Wi * (p.C / vec_of(d->dtype)), 256);
  const PoolBwdRoute route = maxpool_bwd_route(p, d->dtype == VLFB_F32 ? 4 : 2, wide ? 2 : 1, add != nullptr, mask != nullptr, y != nullptr);
  const bool fixed = route.kind != PoolBwdKind::generic;
  if (!with_elem(d->dtype, [&](auto t) {
        using T = decltype(t);
        if (fixed) return launch_maxpool_bwd_fixed<T>(route, p, dy, argmax, dx, add, mask, y, s);
        with_argmax(wide, [&](auto i) {
          using I = decltype(i);
          hipLaunchKernelGGL((pool_bwd_kernel<T, true, I>), dim3(grid), dim3(256), 0, s, (const T*)dy, (const I*)argmax, (T*)dx, (const T*)add,
                             (const T*)mask, p, 1.f, (const T*)y);
        });
      }))
    return set_error(VLFB_ERR_ARG, "pool: bad dtype");        // (VLFB_F16PAIR: the backward runs on one plane)
  return check_launch(fixed ? what_fixed : what);
}
extern "C" int vlfb_maxpool_bwd(const vlfb_pool_desc* d, const void* dy, const void* argmax,
                                void* dx, const void* add, const void* mask, vlfb_stream_t stream) {
  int rc = check_pool(d, true);
  if (rc) return rc;
  VLFB_REQUIRE(dy && argmax && dx, "maxpool_bwd: null pointer");
  return maxpool_bwd_impl(d, dy, argmax, dx, add, mask, nullptr, (hipStream_t)stream, "maxpool_bwd (fixed window)", "maxpool_bwd");
}
extern "C" int vlfb_maxpool_relu_bwd(const vlfb_pool_desc* d, const void* dy, const void* argmax, const void* y,
                                     void* dx, vlfb_stream_t stream) {
  int rc = check_pool(d, true);
  if (rc) return rc;
  VLFB_REQUIRE(dy && argmax && dx && y, "maxpool_relu_bwd: null pointer");
  return maxpool_bwd_impl(d, dy, argmax, dx, nullptr, nullptr, y, (hipStream_t)stream, "maxpool_relu_bwd (fixed window)", "maxpool_relu_bwd");
}
extern "C" int vlfb_maxpool_bwd_describe(const vlfb_pool_desc* d, int has_add, int has_mask, int has_y, char* buf, int64_t buf_bytes) {
  VLFB_REQUIRE(d && buf && buf_bytes >= 64, "maxpool_bwd_describe: buf of at least 64 bytes");
  int rc = check_pool(d, true);
  if (rc) return rc;
  VLFB_REQUIRE(d->dtype == VLFB_F32 || is16(d->dtype), "pool: bad dtype");        // (VLFB_F16PAIR: the backward runs on one plane)
  VLFB_REQUIRE(!(has_y && (has_add || has_mask)), "maxpool_bwd_describe: y (vlfb_maxpool_relu_bwd) comes without add and mask");
  const PoolBwdRoute r = maxpool_bwd_route(to_poolp(d), d->dtype == VLFB_F32 ? 4 : 2, vlfb_pool_argmax_bytes(d), has_add != 0, has_mask != 0,
                                           has_y != 0);
  const char* dt = d->dtype == VLFB_F32 ? "f32" : d->dtype == VLFB_F16 ? "f16" : "bf16";
  const char* ym = r.ymask ? " ymask" : "";
  if (r.kind == PoolBwdKind::band) {
    snprintf(buf, (size_t)buf_bytes, "band %s R=%d bands=%d%s", dt, r.R, r.bands, ym);
  } else if (r.kind == PoolBwdKind::fixed) {
    const PoolWindow& w = kPoolFixedWindows[r.window];
    snprintf(buf, (size_t)buf_bytes, "fixed %dx%dx%d/%dx%dx%d %s%s", w.kt, w.kh, w.kw, w.st, w.sh, w.sw, dt, ym);
  } else {
    snprintf(buf, (size_t)buf_bytes, "generic %s %s%s", r.wide ? "u16" : "u8", dt, ym);
  }
  return VLFB_OK;
}
extern "C" int vlfb_avgpool_fwd(const vlfb_pool_desc* d, const void* x, void* y, vlfb_stream_t stream) {
  int rc = check_avgpool(d);
  if (rc) return rc;
  VLFB_REQUIRE(x && y, "avgpool_fwd: null pointer");
  PoolP p = to_poolp(d);
  const int v = vec_of(d->dtype);
  const bool global = p.To == 1 && p.Ho == 1 && p.Wo == 1 && p.kt == p.Ti && p.kh == p.Hi && p.kw == p.Wi;
  with_src(d->dtype, [&](auto src) {       // (two planes: x is two fp16 planes, y is fp32)
    using S = decltype(src);
    using E = typename S::elem;
    using O = typename S::avg_out;
    if (global && p.N < 65536) {
      dim3 grid((unsigned)((p.C / v + 7) / 8), (unsigned)p.N);
      hipLaunchKernelGGL(global_avgpool_kernel<S>, grid, dim3(256), 0, (hipStream_t)stream, (const E*)x, (O*)y, (long long)p.Ti * p.Hi * p.Wi,
                         p.C, (long long)p.N * p.Ti * p.Hi * p.Wi * p.C);
    } else {
      int grid = grid_for((long long)p.N * p.To * p.Ho * p.Wo * (p.C / v), 256);
      hipLaunchKernelGGL(avgpool_fwd_kernel<S>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const E*)x, (O*)y, p);
    }
  });
  return check_launch(d->dtype == VLFB_F16PAIR ? "avgpool_fwd (fp16 planes)" : "avgpool_fwd");
}
extern "C" int vlfb_avgpool_bwd(const vlfb_pool_desc* d, const void* dy, void* dx, const void* add,
                                const void* mask, vlfb_stream_t stream) {
  int rc = check_avgpool(d);
  if (rc) return rc;
  VLFB_REQUIRE(dy && dx, "avgpool_bwd: null pointer");
  PoolP p = to_poolp(d);
  const float inv = 1.0f / (float)(p.kt * p.kh * p.kw);
  int grid = grid_for((long long)p.N * p.Ti * p.Hi * p.Wi * (p.C / vec_of(d->dtype)), 256);
  if (!with_elem(d->dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((pool_bwd_kernel<T, false, uint8_t>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const T*)dy,
                           (const uint8_t*)nullptr, (T*)dx, (const T*)add, (const T*)mask, p, inv);
      }))
    return set_error(VLFB_ERR_ARG, "pool: bad dtype");        // (VLFB_F16PAIR: the backward runs on one plane)
  return check_launch("avgpool_bwd");
}
extern "C" int vlfb_avgpool_bwd_two_term(const vlfb_pool_desc* d, const float* dy, void* dx_hi, void* dx_lo, const void* mask,
                                         vlfb_stream_t stream) {
  int rc = check_avgpool(d);
  if (rc) return rc;
  VLFB_REQUIRE(dy && dx_hi && dx_lo, "avgpool_bwd_two_term: null pointer");
  VLFB_REQUIRE(d->dtype == VLFB_F16 || d->dtype == VLFB_BF16, "avgpool_bwd_two_term: the input gradient is 16-bit (hi + lo)");
  PoolP p = to_poolp(d);
  VLFB_REQUIRE(p.C % 8 == 0, "avgpool_bwd_two_term: channels must be a multiple of 8");
  const float inv = 1.0f / (float)(p.kt * p.kh * p.kw);
  int grid = grid_for((long long)p.N * p.Ti * p.Hi * p.Wi * (p.C / 8), 256);
  VLFB_WITH_T16(d->dtype, hipLaunchKernelGGL((avgpool_bwd_two_term_kernel<T16>), dim3(grid), dim3(256), 0, (hipStream_t)stream,
                                             dy, (T16*)dx_hi, (T16*)dx_lo, (const T16*)mask, p, inv));
  return check_launch("avgpool_bwd_two_term");
}
