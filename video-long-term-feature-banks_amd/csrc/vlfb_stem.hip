// Stem FPROP (conv1: 3 -> 64 channels, 5x7x7 windows, stride 1x2x2, input packed to 4 channels and W-padded) as a
// direct convolution on the matrix cores (gfx950 only).
//
// As an implicit GEMM the stem is M = 3.2 M positions x N = 64 x K = kt*kh*(8 kw x 4 c) = 1120 at 8 clips.  The
// 128x64 tiled kernel is LDS-bound on it: with 64 output channels a wave owns a 32x32 register tile, so every MFMA
// needs 1 KB of fragment reads, and the im2col'd activation tile (7.2 GB per launch, every input pixel ~70 times) is
// written into LDS on top of that -- 1.4 KB of LDS traffic per MFMA against the 0.5 KB the LDS can deliver in the 4
// clocks a CU needs per MFMA (measured: 586 us, 0.31 of the MFMA roof).  Here
//   * one WAVE owns one whole output row (Wr = 112 positions = 7 fragments) x all 64 channels: 7 x 4 accumulator
//     fragments (112 VGPRs), so a k-step reads 7 + 4 fragments for 28 MFMAs = 0.39 KB per MFMA;
//   * a workgroup = 8 waves = 8 consecutive output rows of one frame.  Per temporal tap a the RAW input rows those 8
//     rows touch (7 * sh + kh = 21 rows of frame t + a - pt, contiguous 16-byte DMAs, out-of-range rows arrive as
//     zeros from the buffer range check) and the weights of that tap (kh k-steps x 64 channels x 64 B) are staged,
//     double-buffered: 2 x 66 KB.  The activation fragment of position w for tap (a, b) is 64 contiguous bytes of
//     a staged row (8 pixels x 4 channels) at pixel w * sw: the MFMA operand layout (lane = position l & 15, k
//     chunk l >> 4) reads it with one ds_read_b128 per lane, neighbouring positions simply overlap;
//   * input rows are staged shifted by -pw pixels so that those reads are 16-byte aligned (the engine stores the
//     clip with 4 zero pixels left of every row and passes pw = 3 - 4);
//   * weight rows (64 B per k-step, chunks XOR-swizzled against bank conflicts) sit in LDS in the permuted channel
//     order of the streaming kernel (vlfb_gemm_s.hip): two
//     neighbouring 16-channel fragments give a lane 8 consecutive channels of one position, so alpha / bias / ReLU
//     and the 16-byte store happen in registers;
//   * XCD x takes clip-contiguous frames: the five frames that read an input row run on the same L2.
// k is accumulated in ascending (a, b, kw, c) order, 32 k per v_mfma_f32_16x16x32, and the epilogue applies
// alpha, bias, ReLU in the order of the tiled kernel: the outputs are bit-identical (tests/test_stem_gpu.py).
#include "vlfb_gemm_common.h"

namespace vlfb {
namespace {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4_s;

constexpr int kStemWaves = 8;        // output rows per workgroup tile

// MT: 16-position fragments per output row (Wr = 16 * MT); KH: filter height (k-steps per temporal tap)
template <typename T, int MT, int KH>
__global__ __launch_bounds__(512) void stem_fprop_kernel(const GP p, const int hblocks, const int ntiles, const int tpw) {
  typedef typename V16<T>::V vec_t;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, g = lane >> 4;
  const int rbytes = p.Ws * 8;                              // pitch of a staged input row (4 elements per pixel)
  const int ppr = rbytes >> 4;                              // 16-byte pieces per row
  const int nrows = (kStemWaves - 1) * p.sh + KH;           // input rows of one frame a tile touches
  const int in_bytes = nrows * rbytes;
  constexpr int wbytes = KH * 4096;                         // one temporal tap: KH k-steps x 64 channels x 64 B
  const int stage = in_bytes + wbytes;
  float* bias_l = reinterpret_cast<float*>(smem + 2 * stage);
  if (tid < 64) bias_l[tid] = p.bias_mode == VLFB_BIAS_COL ? p.bias[tid] : 0.f;
  __syncthreads();

  const __amdgpu_buffer_rsrc_t rsX = make_rsrc(p.A, p.a_bytes);
  const __amdgpu_buffer_rsrc_t rsW = make_rsrc(p.B, p.b_bytes);
  const __amdgpu_buffer_rsrc_t rsO = make_rsrc(p.O, (unsigned)p.M * (unsigned)p.ldo * 2u);
  const unsigned shift = (unsigned)(-p.pw) * 8u;            // rows are staged from pixel -pw on

  // ---- per-lane DMA assignment (tile-invariant) ----------------------------------------------------
  // The input rows a tile touches are consecutive rows of one frame = one contiguous run of nrows * rbytes bytes, so
  // piece id of a stage is simply byte id * 16 of that run: no per-lane table, and "row above / below the frame" is a
  // range check of the byte position against the frame (padding rows arrive as zeros).
  constexpr int RI = 5, WI = (KH * 256 + 511) / 512;        // host checks RI * 512 >= nrows * ppr
  const int tid16 = tid * 16;
  unsigned woff[WI];
#pragma unroll
  for (int i = 0; i < WI; ++i) {
    const int id = tid + 512 * i;
    const int chunk = id & 3, r = (id >> 2) & 63, ks = id >> 8;
    const int c = (r & ~31) | (((r >> 2) & 3) << 3) | (((r >> 4) & 1) << 2) | (r & 3);     // permuted channel order
    // 64-byte rows: the four 16-byte chunks of LDS row r are stored at slot chunk ^ ((-(r >> 2)) & 3).  A ds_read_b128
    // is served in lane groups {0-3, 12-15, 20-27}, ... (MI355X_MICROARCH.md, LDS): a group holds rows 0-3 and 12-15 at
    // chunk X and rows 4-11 at chunk X ^ 1, and the four rows that share a bank window (r, r+4, r+8, r+12) must land on
    // four different slots: keys 0, 3, 2, 1 do that for every X
    woff[i] = ks < KH ? (unsigned)(c * p.ldb + ks * 32 + (chunk ^ ((0 - (r >> 2)) & 3)) * 8) * 2u : kOOB;
  }

  // ---- this workgroup's tiles: contiguous, XCD x owns stripe x -----------------------------------------
  const int nwg = gridDim.x;
  const int wg = (blockIdx.x & 7) * (nwg >> 3) + (blockIdx.x >> 3);
  const int tile_beg = wg * tpw, tile_end = min(ntiles, tile_beg + tpw);
  const int nst = max(0, tile_end - tile_beg) * p.kt;

  // a stage = (tile, temporal tap a); its DMA pieces are issued one or two per k-step of the previous stage, between
  // the MFMAs (an LDS-DMA piece costs ~60 cycles of issue among MFMAs, 100-185 in a burst of its own)
  struct StageSrc { int rel0; unsigned fbyte; bool tok; unsigned wsoff, base; };
  auto stage_src = [&](int s, int buf) {
    StageSrc q;
    const int tile = tile_beg + s / p.kt, a = s - (s / p.kt) * p.kt;
    const int hb = tile % hblocks, nt = tile / hblocks;
    const int t = nt % p.Tr, n = nt / p.Tr;
    const int tin = t * p.st - p.pt + a;
    q.tok = (unsigned)tin < (unsigned)p.Ts;
    q.rel0 = (hb * kStemWaves * p.sh - p.ph) * rbytes;      // byte position of the first staged row inside its frame
    q.fbyte = (unsigned)((n * p.Ts + tin) * p.Hs) * (unsigned)rbytes + shift;
    q.wsoff = (unsigned)(a * KH * 64);                      // bytes: KH k-steps x 32 k x 2 B
    q.base = lds_addr_of(smem) + (unsigned)(buf * stage);
    return q;
  };
  auto issue_piece = [&](const StageSrc& q, int k) {        // k = 0 .. RI + WI - 1 (compile-time after unrolling)
    if (k < RI) {
      if (tid + 512 * k < nrows * ppr) {                    // (inactive lanes of the LDS DMA write nothing)
        const int rel = q.rel0 + k * 8192 + tid16;
        const bool ok = q.tok && (unsigned)rel < (unsigned)(p.Hs * rbytes);
        const unsigned off = ok ? q.fbyte + (unsigned)rel : kOOB;
        bufglds16_hidden(rsX, off, 0u, (unsigned)__builtin_amdgcn_readfirstlane((int)(q.base + (k * 512 + wave * 64) * 16)));
      }
    } else {
      const int i = k - RI;
      if (tid + 512 * i < KH * 256)
        bufglds16_hidden(rsW, woff[i], q.wsoff,
                         (unsigned)__builtin_amdgcn_readfirstlane((int)(q.base + in_bytes + (i * 512 + wave * 64) * 16)));
    }
  };
  constexpr int NP = RI + WI;                               // DMA pieces per lane and stage

  f32x4_v acc[MT][4];
  // fragment addresses inside a stage: activation row of this wave for filter row b, weight fragments of k-step b
  const int a_lane = l15 * p.sw * 8 + g * 16;
  const int w_lane = in_bytes + l15 * 64 + ((g ^ ((0 - (l15 >> 2)) & 3)) << 4);

  if (nst > 0) {
    const StageSrc q = stage_src(0, 0);
#pragma unroll
    for (int k = 0; k < NP; ++k) issue_piece(q, k);
  }
  int buf = 0;
  for (int s = 0; s < nst; ++s) {
    const int tile = tile_beg + s / p.kt, a = s - (s / p.kt) * p.kt;
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    const bool more = s + 1 < nst;
    const StageSrc q = stage_src(more ? s + 1 : s, buf ^ 1);
    if (a == 0) {
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[m][j] = f32x4_v{0.f, 0.f, 0.f, 0.f};
    }
    const char* st = smem + buf * stage;
    const char* arow = st + wave * p.sh * rbytes + a_lane;
    const char* wrow = st + w_lane;
    // fragments of k-step b + 1 are requested before the 28 MFMAs of k-step b (two register sets; the scheduling
    // barriers keep the compiler from folding the reads back into the MFMA run one wait at a time)
    vec_t wf[2][4], af[2][MT];
    auto read_step = [&](int b, vec_t (&w)[4], vec_t (&x)[MT]) {
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = *reinterpret_cast<const vec_t*>(wrow + b * 4096 + j * 1024);
#pragma unroll
      for (int m = 0; m < MT; ++m) x[m] = *reinterpret_cast<const vec_t*>(arow + b * rbytes + m * 16 * p.sw * 8);
    };
    read_step(0, wf[0], af[0]);
#pragma unroll
    for (int b = 0; b < KH; ++b) {
      if (b + 1 < KH) read_step(b + 1, wf[(b + 1) & 1], af[(b + 1) & 1]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[m][j] = V16<T>::mma(wf[b & 1][j], af[b & 1][m], acc[m][j]);
      __builtin_amdgcn_sched_barrier(0);
      // this k-step's share of the next stage's DMA pieces (issued behind the MFMAs, which keep the pipe busy meanwhile)
      if (more) {
#pragma unroll
        for (int k = b * NP / KH; k < (b + 1) * NP / KH; ++k) issue_piece(q, k);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (a == p.kt - 1) {
      // ---- epilogue in registers: lane = position l15 of fragment m, channels q*32 + g*8 .. +7 ---------------
      const int hb = tile % hblocks, nt = tile / hblocks;
      const int h = hb * kStemWaves + wave;
      if (h < p.Hr) {
        const int row0 = (nt * p.Hr + h) * p.Wr;               // nt = n * Tr + t
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const unsigned oo = (unsigned)((row0 + m * 16 + l15) * p.ldo + g * 8) * 2u;
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
              for (int r = 0; r < 4; ++r) v[e * 4 + r] = __fmul_rn(acc[m][2 * q + e][r], p.alpha);
            nt_apply<8>(p, v, aligned16(bias_l + q * 32 + g * 8), row0 + m * 16 + l15, NoRows{}, NoRows{}, NoRows{});
            const u32x4_s o = {Elem<T>::pack2(v[0], v[1]), Elem<T>::pack2(v[2], v[3]), Elem<T>::pack2(v[4], v[5]), Elem<T>::pack2(v[6], v[7])};
            __builtin_amdgcn_raw_buffer_store_b128(o, rsO, (int)(oo + q * 64u), 0, 0);
          }
        }
      }
    }
    buf ^= 1;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The same direct convolution on TWO fp16 planes per operand (VLFB_MATH_F16X3: conv1 of the "mix" forward; the tiled
// two-plane kernel runs it at 1.27-1.41 ms, bound by the 14 GB of im2col'd activation tiles it DMAs).  Both planes of the
// raw input rows and of the tap's weights make one stage of 2 x (39 + 28) KB = 134 KB, so there is no second stage: a
// stage is loaded, waited for and computed in turn (the load is ~1/4 of the compute, and the rows come out of the L2 the
// neighbouring frames of the XCD stripe just filled).  A k-step is 22 fragment reads for 84 MFMAs -- per accumulator
// wl.xh, wh.xl, wh.xh, in the (a, b) order of the tiled kernel, so the two planes written (O = hi, O2 = lo) are
// bit-identical to its output (tests/test_pair_gpu.py).
template <int MT, int KH>
__global__ __launch_bounds__(512) void stem_fprop_pair_kernel(const GP p, const int hblocks, const int ntiles, const int tpw) {
  typedef f16x8_v vec_t;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, g = lane >> 4;
  const int rbytes = p.Ws * 8;
  const int ppr = rbytes >> 4;
  const int nrows = (kStemWaves - 1) * p.sh + KH;
  const int in_bytes = nrows * rbytes;                       // one plane of the staged rows
  constexpr int wbytes = KH * 4096;                          // one plane of a tap's weights
  // stage: [rows hi][rows lo][W hi][W lo]
  float* bias_l = reinterpret_cast<float*>(smem + 2 * (in_bytes + wbytes));
  if (tid < 64) bias_l[tid] = p.bias_mode == VLFB_BIAS_COL ? p.bias[tid] : 0.f;

  const __amdgpu_buffer_rsrc_t rsX = make_rsrc(p.A, p.a_bytes);
  const __amdgpu_buffer_rsrc_t rsW = make_rsrc(p.B, p.b_bytes);
  const __amdgpu_buffer_rsrc_t rsO = make_rsrc(p.O, (unsigned)p.M * (unsigned)p.ldo * 2u);
  const __amdgpu_buffer_rsrc_t rsO2 = make_rsrc(p.O2, (unsigned)p.M * (unsigned)p.ldo * 2u);
  const unsigned shift = (unsigned)(-p.pw) * 8u;
  const unsigned x_plane = (unsigned)p.a_ps * 2u, w_plane = (unsigned)p.b_ps * 2u;     // byte distance of the lo planes

  constexpr int RI = 5, WI = (KH * 256 + 511) / 512;
  const int tid16 = tid * 16;
  unsigned woff[WI];
#pragma unroll
  for (int i = 0; i < WI; ++i) {
    const int id = tid + 512 * i;
    const int chunk = id & 3, r = (id >> 2) & 63, ks = id >> 8;
    const int c = (r & ~31) | (((r >> 2) & 3) << 3) | (((r >> 4) & 1) << 2) | (r & 3);     // permuted channel order (see above)
    woff[i] = ks < KH ? (unsigned)(c * p.ldb + ks * 32 + (chunk ^ ((0 - (r >> 2)) & 3)) * 8) * 2u : kOOB;
  }

  const int nwg = gridDim.x;
  const int wg = (blockIdx.x & 7) * (nwg >> 3) + (blockIdx.x >> 3);
  const int tile_beg = wg * tpw, tile_end = min(ntiles, tile_beg + tpw);
  const int nst = max(0, tile_end - tile_beg) * p.kt;
  const unsigned lds0 = lds_addr_of(smem);

  f32x4_v acc[MT][4];
  const int a_lane = l15 * p.sw * 8 + g * 16;
  const int w_lane = 2 * in_bytes + l15 * 64 + ((g ^ ((0 - (l15 >> 2)) & 3)) << 4);

  for (int s = 0; s < nst; ++s) {
    const int tile = tile_beg + s / p.kt, a = s - (s / p.kt) * p.kt;
    const int hb = tile % hblocks, nt = tile / hblocks;
    const int t = nt % p.Tr, n = nt / p.Tr;
    // ---- load the stage (every wave is done with the previous one behind the barrier) ----------------------------
    asm volatile("s_barrier" ::: "memory");
    {
      const int tin = t * p.st - p.pt + a;
      const bool tok = (unsigned)tin < (unsigned)p.Ts;
      const int rel0 = (hb * kStemWaves * p.sh - p.ph) * rbytes;
      const unsigned fbyte = (unsigned)((n * p.Ts + tin) * p.Hs) * (unsigned)rbytes + shift;
      const unsigned wsoff = (unsigned)(a * KH * 64);
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) {
#pragma unroll
        for (int k = 0; k < RI; ++k) {
          if (tid + 512 * k < nrows * ppr) {
            const int rel = rel0 + k * 8192 + tid16;
            const bool ok = tok && (unsigned)rel < (unsigned)(p.Hs * rbytes);
            const unsigned off = ok ? fbyte + (unsigned)rel + (pl ? x_plane : 0u) : kOOB;
            bufglds16_hidden(rsX, off, 0u, (unsigned)__builtin_amdgcn_readfirstlane((int)(lds0 + pl * in_bytes + (k * 512 + wave * 64) * 16)));
          }
        }
#pragma unroll
        for (int i = 0; i < WI; ++i) {
          if (tid + 512 * i < KH * 256)
            bufglds16_hidden(rsW, woff[i] == kOOB ? kOOB : woff[i] + (pl ? w_plane : 0u), wsoff,
                             (unsigned)__builtin_amdgcn_readfirstlane((int)(lds0 + 2 * in_bytes + pl * wbytes + (i * 512 + wave * 64) * 16)));
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    if (a == 0) {
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[m][j] = f32x4_v{0.f, 0.f, 0.f, 0.f};
    }
    const char* arow = smem + wave * p.sh * rbytes + a_lane;
    const char* wrow = smem + w_lane;
#pragma unroll
    for (int b = 0; b < KH; ++b) {
      vec_t wh[4], wl[4], xh[MT], xl[MT];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        wh[j] = *reinterpret_cast<const vec_t*>(wrow + b * 4096 + j * 1024);
        wl[j] = *reinterpret_cast<const vec_t*>(wrow + wbytes + b * 4096 + j * 1024);
      }
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        xh[m] = *reinterpret_cast<const vec_t*>(arow + b * rbytes + m * 16 * p.sw * 8);
        xl[m] = *reinterpret_cast<const vec_t*>(arow + in_bytes + b * rbytes + m * 16 * p.sw * 8);
      }
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[m][j] = V16<f16_t>::mma(wl[j], xh[m], acc[m][j]);
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[m][j] = V16<f16_t>::mma(wh[j], xl[m], acc[m][j]);
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[m][j] = V16<f16_t>::mma(wh[j], xh[m], acc[m][j]);
    }
    if (a == p.kt - 1) {
      // ---- epilogue in registers (lane = position l15 of fragment m, channels q*32 + g*8 .. +7): hi and lo planes ----
      const int h = hb * kStemWaves + wave;
      if (h < p.Hr) {
        const int row0 = (nt * p.Hr + h) * p.Wr;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const unsigned oo = (unsigned)((row0 + m * 16 + l15) * p.ldo + g * 8) * 2u;
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
              for (int r = 0; r < 4; ++r) v[e * 4 + r] = __fmul_rn(acc[m][2 * q + e][r], p.alpha);
            nt_apply<8>(p, v, aligned16(bias_l + q * 32 + g * 8), row0 + m * 16 + l15, NoRows{}, NoRows{}, NoRows{});
            uint32_t w4[4], l4[4];
            split2<f16_t>(v, w4, l4);
            const u32x4_s o = {w4[0], w4[1], w4[2], w4[3]}, ol = {l4[0], l4[1], l4[2], l4[3]};
            if (p.nt_epi) {            // (aux = 2: the non-temporal hint, GP::nt_epi)
              __builtin_amdgcn_raw_buffer_store_b128(o, rsO, (int)(oo + q * 64u), 0, 2);
              __builtin_amdgcn_raw_buffer_store_b128(ol, rsO2, (int)(oo + q * 64u), 0, 2);
            } else {
              __builtin_amdgcn_raw_buffer_store_b128(o, rsO, (int)(oo + q * 64u), 0, 0);
              __builtin_amdgcn_raw_buffer_store_b128(ol, rsO2, (int)(oo + q * 64u), 0, 0);
            }
          }
        }
      }
    }
  }
}

int launch_stem_fprop_pair_t(const GP& gp, int hblocks, int ntiles, int tpw, unsigned nwg, size_t lds, hipStream_t s) {
  return launch_lds<stem_fprop_pair_kernel<7, 7>, 160 * 1024>(dim3(nwg), dim3(512), lds, s, "conv kernel (stem, direct, fp16 planes)",
                                                              gp, hblocks, ntiles, tpw);
}

template <typename T>
int launch_stem_fprop_t(const GP& gp, int hblocks, int ntiles, int tpw, unsigned nwg, size_t lds, hipStream_t s) {
  return launch_lds<stem_fprop_kernel<T, 7, 7>, 160 * 1024>(dim3(nwg), dim3(512), lds, s, "conv kernel (stem, direct)",
                                                            gp, hblocks, ntiles, tpw);
}

}  // namespace

// the stem shapes the direct kernel is compiled for: 64 output channels, 7-row filters over 8 packed kw, 112-wide
// output rows, W stride 2, left padding stored in the row (pw <= 0), everything the 16-bit epilogue needs
bool stem_fprop_ok(const GP& gp, int pack_w, int dtype, int out_dtype, long long batch) {
  if (!(dtype == VLFB_BF16 || dtype == VLFB_F16) || out_dtype != dtype || batch != 1) return false;
  if (pack_w != 8 || gp.Ncols != 64 || gp.kh != 7 || gp.Wr != 112 || gp.sw != 2 || gp.pw > 0 || gp.dt != 1 || gp.dh != 1) return false;
  if (gp.ldo % 8 || gp.ldb % 8 || gp.K != gp.kt * 7 * 32) return false;   // (residual / mask operands: checked per call)
  // every position's window must lie inside the staged row: (Wr - 1) * sw + 8 pixels from pixel -pw on
  if ((gp.Wr - 1) * gp.sw + 8 - gp.pw > gp.Ws) return false;
  const int nrows = (kStemWaves - 1) * gp.sh + 7;
  const long long ppr = (long long)gp.Ws * 8 / 16;
  if ((gp.Ws * 8) % 16 || nrows * ppr > 5 * 512) return false;
  const size_t lds = 2 * ((size_t)nrows * gp.Ws * 8 + 7 * 4096) + 256;
  if (lds > 160 * 1024) return false;
  if ((long long)gp.M * gp.ldo * 2 >= (1ll << 31)) return false;
  return true;
}

// ... and the two-plane form: fp16 planes in and out, one 134-KB stage
bool stem_fprop_pair_ok(const GP& gp, int pack_w, long long batch) {
  if (batch != 1) return false;
  if (pack_w != 8 || gp.Ncols != 64 || gp.kh != 7 || gp.Wr != 112 || gp.sw != 2 || gp.pw > 0 || gp.dt != 1 || gp.dh != 1) return false;
  if (gp.ldo % 8 || gp.ldb % 8 || gp.K != gp.kt * 7 * 32) return false;
  if ((gp.Wr - 1) * gp.sw + 8 - gp.pw > gp.Ws) return false;
  const int nrows = (kStemWaves - 1) * gp.sh + 7;
  const long long ppr = (long long)gp.Ws * 8 / 16;
  if ((gp.Ws * 8) % 16 || nrows * ppr > 5 * 512) return false;
  const size_t lds = 2 * ((size_t)nrows * gp.Ws * 8 + 7 * 4096) + 256;
  if (lds > 160 * 1024) return false;
  if ((long long)gp.M * gp.ldo * 2 >= (1ll << 31)) return false;
  return true;
}

int launch_stem_fprop_pair(const GP& gp, hipStream_t s) {
  const int ncu = device_cus8();
  const int hblocks = (gp.Hr + kStemWaves - 1) / kStemWaves;
  const long long ntiles = (long long)(gp.M / (gp.Hr * gp.Wr)) * hblocks;
  long long nwg = (ntiles + 7) / 8 * 8;
  if (nwg > ncu) nwg = ncu;
  const int tpw = (int)((ntiles + nwg - 1) / nwg);
  const int nrows = (kStemWaves - 1) * gp.sh + 7;
  const size_t lds = 2 * ((size_t)nrows * gp.Ws * 8 + 7 * 4096) + 256;
  return launch_stem_fprop_pair_t(gp, hblocks, (int)ntiles, tpw, (unsigned)nwg, lds, s);
}

int launch_stem_fprop(const GP& gp, int dtype, hipStream_t s) {
  const int ncu = device_cus8();
  const int hblocks = (gp.Hr + kStemWaves - 1) / kStemWaves;
  const long long ntiles = (long long)(gp.M / (gp.Hr * gp.Wr)) * hblocks;      // (n, t) frames x row blocks
  long long nwg = (ntiles + 7) / 8 * 8;
  if (nwg > ncu) nwg = ncu;
  const int tpw = (int)((ntiles + nwg - 1) / nwg);
  const int nrows = (kStemWaves - 1) * gp.sh + 7;
  const size_t lds = 2 * ((size_t)nrows * gp.Ws * 8 + 7 * 4096) + 256;
  if (dtype == VLFB_F16) return launch_stem_fprop_t<f16_t>(gp, hblocks, (int)ntiles, tpw, (unsigned)nwg, lds, s);
  return launch_stem_fprop_t<bf16_t>(gp, hblocks, (int)ntiles, tpw, (unsigned)nwg, lds, s);
}

}  // namespace vlfb
