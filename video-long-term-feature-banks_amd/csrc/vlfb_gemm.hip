// Implicit-GEMM 3-D convolution / batched GEMM on CDNA4 matrix cores (gfx950).
//
// One kernel family covers every contraction on the hot path (SURVEY.md 8a rows M1, M4-M6, M10,
// H3-H5): conv fprop, conv dgrad (NT form: both operands K-contiguous) and conv wgrad / the
// "contract over positions" attention products (TN form: both operands are stored with the
// contraction index as the slow dimension, so the stager transposes 8x8 (bf16) / 4x4 (fp32)
// register blocks on the way into LDS).
//
// Data layout: activations are channels-last [N,T,H,W,C] so a 16-byte global load is a run of
// consecutive K for one output row; weights are [Cout][tap][Cin].  LDS tiles are rows of 128
// bytes (64 bf16 / 32 fp32 of K) with the 16-byte chunk index XOR-ed by (row & 7), which makes
// both the ds_write_b128 of the stager and the ds_read_b128 of the fragment reader
// conflict-free (cdna_hip_programming.md, T2).  Wave tile 64x64 (2x2 waves, 128x128 block) out
// of 16x16 MFMA fragments: v_mfma_f32_16x16x32_bf16 on the throughput path,
// v_mfma_f32_16x16x4_f32 (exact fp32 FMA chain) on the parity path.  The two paths share the
// same lane<->k mapping: lane l owns 8 consecutive k of row (l & 15) at k-offset (l >> 4) * 8.
// MFMA operands are swapped (weights as A, activations as B) so that each lane ends up holding
// 4 consecutive output channels of one output row -> 8/16-byte epilogue stores.
#include "vlfb_conv_plan.h"
#include "vlfb_gemm_nt.h"

namespace vlfb {
namespace {

// =============================================================================================
// TN kernel: O[pp][qq] = sum_m P[m][pp] * Xg[m][qq]   (qq = (tap, channel) of the gathered input)
// =============================================================================================
// register-block transposes: `in[j]` = 16 bytes of consecutive channels for position j;
// `out[c]` = 16 bytes of consecutive positions for channel c.
__device__ __forceinline__ uint32_t word_of(const uint4& v, int i) {
  return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;
}
__device__ __forceinline__ void transpose_block(const uint4 (&in)[8], uint4 (&out)[8], bf16_t) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    uint32_t o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t w0 = word_of(in[2 * q], c >> 1), w1 = word_of(in[2 * q + 1], c >> 1);
      o[q] = (c & 1) ? ((w0 >> 16) | (w1 & 0xffff0000u)) : ((w0 & 0xffffu) | (w1 << 16));
    }
    out[c] = make_uint4(o[0], o[1], o[2], o[3]);
  }
}
__device__ __forceinline__ void transpose_block(const uint4 (&in)[8], uint4 (&out)[8], f16_t) {
  transpose_block(in, out, bf16_t());      // a pure 16-bit shuffle
}
__device__ __forceinline__ void transpose_block(const uint4 (&in)[4], uint4 (&out)[4], float) {
  out[0] = make_uint4(in[0].x, in[1].x, in[2].x, in[3].x);
  out[1] = make_uint4(in[0].y, in[1].y, in[2].y, in[3].y);
  out[2] = make_uint4(in[0].z, in[1].z, in[2].z, in[3].z);
  out[3] = make_uint4(in[0].w, in[1].w, in[2].w, in[3].w);
}

// TN gather state of one staging block: the tap is fixed per thread, positions advance, so the
// (n, t, h) part of the source address and its validity are cached and only refreshed when the
// position wraps to a new output row -- no integer division inside the k loop.
struct QRow {
  int n, t, h, w;
  long long base;   // pixel index of source row (n, ts, hs, 0)
  bool hv;          // ts, hs inside the source
};
__device__ __forceinline__ void qrow_refresh(const GP& p, QRow& r, const TapC& tp) {
  const int ts = r.t * p.st - p.pt + tp.a * p.dt;
  const int hs = r.h * p.sh - p.ph + tp.b * p.dh;
  r.hv = (unsigned)ts < (unsigned)p.Ts && (unsigned)hs < (unsigned)p.Hs;
  r.base = ((long long)(r.n * p.Ts + ts) * p.Hs + hs) * p.Ws;
}
__device__ __forceinline__ void qrow_next(const GP& p, QRow& r, const TapC& tp) {
  if (++r.w == p.Wr) {
    r.w = 0;
    if (++r.h == p.Hr) {
      r.h = 0;
      if (++r.t == p.Tr) { r.t = 0; ++r.n; }
    }
    qrow_refresh(p, r, tp);
  }
}
// r += (dn, dt, dh, dw) in the mixed radix (Tr, Hr, Wr)
__device__ __forceinline__ void qrow_jump(const GP& p, QRow& r, const RowC& d, const TapC& tp) {
  r.w += d.w; if (r.w >= p.Wr) { r.w -= p.Wr; ++r.h; }
  r.h += d.h; if (r.h >= p.Hr) { r.h -= p.Hr; ++r.t; }
  r.t += d.t; if (r.t >= p.Tr) { r.t -= p.Tr; ++r.n; }
  r.n += d.n;
  qrow_refresh(p, r, tp);
}
template <typename T, bool PACKW>
__device__ __forceinline__ uint4 qrow_load(const GP& p, const char* base, const QRow& r, const TapC& tp, bool ok) {
  ok = ok && tp.ok && r.hv;
  if (PACKW) {   // W-padded stem input: always inside the row
    const int w0 = r.w * p.sw - p.pw + tp.c;
    return ld16_if(base, (r.base + w0) * 4 * (long long)sizeof(T), ok);
  } else {
    const int ws = r.w * p.sw - p.pw + tp.c * p.dw;
    return ld16_if(base, ((r.base + ws) * p.lda + tp.ci) * (long long)sizeof(T), ok && (unsigned)ws < (unsigned)p.Ws);
  }
}

template <typename T, typename OutT, int BP, int BQ, bool IDENT, bool PACKW>
__global__ __launch_bounds__(kThreads) void gemm_tn_kernel(const GP p) {
  constexpr int EPC = Elem<T>::EPC;
  constexpr int BK = kRowBytes / (int)sizeof(T);
  constexpr int NPB = BP / EPC * 8, NQB = BQ / EPC * 8;  // staging blocks per tile
  constexpr int ITER = (NPB + NQB + kThreads - 1) / kThreads;
  constexpr int WP = BP / 2, WQ = BQ / 2;
  constexpr int FP = WP / 16, FQ = WQ / 16;
  constexpr int BUF = (BP + BQ) * kRowBytes;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wp = wave >> 1, wq = wave & 1;
  const int l15 = lane & 15, g = lane >> 4;

  const int nwg = p.tiles_m * p.tiles_n;
  int bid, split;
  if (p.splits > 1 && (p.splits & 7) == 0) {
    // 1-D grid, XCD-grouped: workgroup id -> (xcd = id % 8, slot = id / 8).  All output tiles of
    // one position-split run back to back on ONE XCD, so the P / X panels of that split are
    // fetched from HBM once and re-used out of that XCD's L2 by the other tiles.
    const int id = blockIdx.x;
    const int xcd = id & 7, slot = id >> 3;
    bid = slot % nwg;
    split = (slot / nwg) * 8 + xcd;
  } else {
    bid = xcd_remap(blockIdx.x, nwg);
    split = blockIdx.y;
  }
  const int tile_p = bid / p.tiles_n, tile_q = bid - tile_p * p.tiles_n;
  const int p0 = tile_p * BP, q0 = tile_q * BQ;
  const int z = blockIdx.z;

  const char* Pb = p.P + (long long)z * p.p_bs * (long long)sizeof(T);
  const char* Ab = p.A + (long long)z * p.a_bs * (long long)sizeof(T);

  const int kbeg = split * p.kper;
  const int kend = min(p.M, kbeg + p.kper);
  const int ktiles = (kend - kbeg + BK - 1) / BK;

  // static per-thread block assignment
  int blk_kind[ITER], blk_r[ITER], blk_k[ITER];
  TapC qtap[ITER];
#pragma unroll
  for (int it = 0; it < ITER; ++it) {
    int id = tid + it * kThreads;
    if (id < NPB) { blk_kind[it] = 0; blk_r[it] = id >> 3; blk_k[it] = id & 7; }
    else if (id < NPB + NQB) { id -= NPB; blk_kind[it] = 1; blk_r[it] = id >> 3; blk_k[it] = id & 7; }
    else { blk_kind[it] = 2; blk_r[it] = 0; blk_k[it] = 0; }
    if (blk_kind[it] == 1) {
      int kc = (q0 + blk_r[it] * EPC) / EPC;
      if (IDENT) { qtap[it].ok = kc * EPC < p.K; qtap[it].a = qtap[it].b = qtap[it].c = 0; qtap[it].ci = 0; }
      else qtap[it] = decode_tap<T, PACKW>(p, kc);
    }
  }
  // gather cursors (generic path): first position of the block in k-tile 0, and the BK jump
  QRow qrow[ITER];
  RowC jump;
  if (!IDENT) {
    jump = decode_row(p, BK - EPC);   // after a tile the cursor already moved EPC positions
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
      if (blk_kind[it] == 1) {
        const RowC r0 = decode_row(p, min(kbeg + blk_k[it] * EPC, p.M - 1));
        qrow[it].n = r0.n; qrow[it].t = r0.t; qrow[it].h = r0.h; qrow[it].w = r0.w;
        qrow_refresh(p, qrow[it], qtap[it]);
      }
    }
  }

  uint4 stg[ITER][EPC];

  auto load_tile = [&](int kt) {
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
      const int kk = kbeg + kt * BK + blk_k[it] * EPC;  // first position of the block
      if (blk_kind[it] == 0) {
        const int pc = p0 + blk_r[it] * EPC;
        const bool cok = pc < p.Ncols;
#pragma unroll
        for (int j = 0; j < EPC; ++j) {
          const int k = kk + j;
          stg[it][j] = ld16_if(Pb, ((long long)k * p.ldp + pc) * (long long)sizeof(T), cok && k < kend);
        }
      } else if (blk_kind[it] == 1) {
        const int kc = (q0 + blk_r[it] * EPC) / EPC;
        if (IDENT) {
          RowC unused;
#pragma unroll
          for (int j = 0; j < EPC; ++j) {
            const int k = kk + j;
            stg[it][j] = load_act_chunk<T, true, false, false>(p, Ab, k, k < kend, unused, qtap[it], kc);
          }
        } else {
#pragma unroll
          for (int j = 0; j < EPC; ++j) {
            stg[it][j] = qrow_load<T, PACKW>(p, Ab, qrow[it], qtap[it], kk + j < kend);
            qrow_next(p, qrow[it], qtap[it]);
          }
          qrow_jump(p, qrow[it], jump, qtap[it]);   // to this block's slot in the next k-tile
        }
      }
    }
  };
  auto store_tile = [&](int buf) {
    char* pt = smem + buf * BUF;
    char* qt = pt + BP * kRowBytes;
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
      if (blk_kind[it] == 2) continue;
      uint4 tr[EPC];
      transpose_block(stg[it], tr, T());
      char* dst = blk_kind[it] == 0 ? pt : qt;
#pragma unroll
      for (int c = 0; c < EPC; ++c)
        *reinterpret_cast<uint4*>(dst + lds_off(blk_r[it] * EPC + c, blk_k[it])) = tr[c];
    }
  };

  f32x4_v acc[FQ][FP];
#pragma unroll
  for (int a = 0; a < FQ; ++a)
#pragma unroll
    for (int b = 0; b < FP; ++b) acc[a][b] = f32x4_v{0.f, 0.f, 0.f, 0.f};

  if (ktiles > 0) {
    load_tile(0);
    store_tile(0);
  }
  __syncthreads();
  for (int kt = 0; kt < ktiles; ++kt) {
    const bool more = kt + 1 < ktiles;
    if (more) load_tile(kt + 1);
    const char* pt = smem + (kt & 1) * BUF;
    const char* qt = pt + BP * kRowBytes;
#pragma unroll
    for (int ks = 0; ks < Mma<T>::KSTEPS; ++ks) {
      typename Mma<T>::Frag pf[FP], qf[FQ];
#pragma unroll
      for (int i = 0; i < FP; ++i) pf[i] = Mma<T>::load(pt, wp * WP + i * 16 + l15, ks, g);
#pragma unroll
      for (int j = 0; j < FQ; ++j) qf[j] = Mma<T>::load(qt, wq * WQ + j * 16 + l15, ks, g);
#pragma unroll
      for (int j = 0; j < FQ; ++j)
#pragma unroll
        for (int i = 0; i < FP; ++i) acc[j][i] = Mma<T>::mma(qf[j], pf[i], acc[j][i]);
    }
    if (more) store_tile((kt + 1) & 1);
    __syncthreads();
  }

  // ---- epilogue: lane holds qq = qb + 0..3 for output row pp ---------------------------------
#pragma unroll
  for (int i = 0; i < FP; ++i) {
    const int pp = p0 + wp * WP + i * 16 + l15;
    if (pp >= p.Ncols) continue;
    const float rs = tn_row_scale(p, pp);
#pragma unroll
    for (int j = 0; j < FQ; ++j) tn_store<OutT>(p, acc[j][i], z, split, pp, q0 + wq * WQ + j * 16 + g * 4, rs);
  }
}


// =============================================================================================
// TN kernel, bf16, DMA + LDS transpose-read variant.
// The operand tiles are copied as they lie in HBM ([position][channel], 16-byte pieces by
// global_load_lds) -- no VGPR staging, no register transposes, no ds_write -- and the MFMA fragments
// (8 consecutive positions of one channel per lane) are produced by ds_read_b64_tr_b16, which
// returns to lane i of a 16-lane group column i of a 4(k) x 16(channel) block.
// LDS rows are RS = 2*B bytes (one position); the 32-byte segment index is XOR-ed with a key of
// the row so that the 8 rows touched by a 32-lane half of a tr-read fall on 8 different 32-byte
// bank segments (the DMA destination is lane-linear, so the XOR is applied on the SOURCE chunk).
// The DMAs are issued through bufglds16_hidden: with the builtin, hipcc put s_waitcnt vmcnt(0) in front of the
// transposed reads of every k-tile, i.e. it waited for the NEXT tile's DMA right after issuing it.
// =============================================================================================
template <typename T, typename OutT, int BP, int BQ, bool IDENT, bool PACKW, int NW = 4, bool SP = false>
__global__ __launch_bounds__(64 * NW) void gemm_tn_tr_kernel(const GP p) {
  // NW = 4: waves 2 (p) x 2 (q).  NW = 8: waves 2 x 4 on the same tile -- twice the wavefronts per CU.
  // SP (split-bf16 math on fp32 storage, vlfb_gemm_split.hip): BOTH operands arrive as two bf16 term planes [plane][position]
  // [channel] (h = bf16(x), m = bf16(x - h); a_ps / p_ps elements apart) and a fragment pair issues three MFMAs
  // (m.h, h.m, h.h); k-tiles of 32 positions keep the two-plane tiles at the LDS footprint of the plain kernel.
  typedef typename V16<T>::V vec_t;
  constexpr int NTHR = 64 * NW;
  constexpr int NWQ = NW / 2;
  constexpr int NPL = SP ? 2 : 1;
  constexpr int BK = SP ? 32 : 64;               // positions per k-tile
  constexpr int RSP = BP * 2, RSQ = BQ * 2;      // LDS row bytes (one position)
  constexpr int CP = BP / 8, CQ = BQ / 8;        // 16-byte chunks per row
  constexpr int PI = BK * CP / NTHR, QI = BK * CQ / NTHR;   // DMA pieces per thread
  constexpr int RPP_P = NTHR / CP, RPP_Q = NTHR / CQ;       // rows per pass
  constexpr int WP = BP / 2, WQ = BQ / NWQ;
  static_assert(PI >= 1 && QI >= 1 && WQ >= 16, "tile too small for this many waves");
  constexpr int FP = WP / 16, FQ = WQ / 16;
  constexpr int PLP = BK * RSP, PLQ = BK * RSQ;  // bytes of one plane tile
  constexpr int BUF = NPL * (PLP + PLQ);
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int wp = wave / NWQ, wq = wave % NWQ;
  const int l15 = lane & 15, g = lane >> 4;

  const int nwg = p.tiles_m * p.tiles_n;
  int bid, split;
  if (p.splits > 1 && (p.splits & 7) == 0) {
    const int id = blockIdx.x;
    const int xcd = id & 7, slot = id >> 3;
    bid = slot % nwg;
    split = (slot / nwg) * 8 + xcd;
  } else {
    bid = xcd_remap(blockIdx.x, nwg);
    split = blockIdx.y;
  }
  const int tile_p = bid / p.tiles_n, tile_q = bid - tile_p * p.tiles_n;
  const int p0 = tile_p * BP, q0 = tile_q * BQ;
  const int z = blockIdx.z;
  const char* Pb = p.P + (long long)z * p.p_bs * 2;
  const char* Ab = p.A + (long long)z * p.a_bs * 2;
  const int kbeg = split * p.kper;
  const int kend = min(p.M, kbeg + p.kper);
  const int ktiles = (kend - kbeg + BK - 1) / BK;

  // ---- per-thread DMA assignment ---------------------------------------------------------------
  const int pslot = tid % CP, prow = tid / CP;               // LDS slot (row, 16-byte slot) of the P tile
  const int pc = (((pslot >> 1) ^ tr_key<RSP>(prow)) << 1) | (pslot & 1);   // global channel chunk
  const int pch = p0 + pc * 8;
  const bool pok = pch < p.Ncols;
  const int qslot = tid % CQ, qrow0 = tid / CQ;
  const int qc = (((qslot >> 1) ^ tr_key<RSQ>(qrow0)) << 1) | (qslot & 1);
  const int kc = q0 / 8 + qc;                                 // global 16-byte chunk index along K
  TapC qtap;
  if (IDENT) { qtap.ok = kc * 8 < p.K; qtap.a = qtap.b = qtap.c = 0; qtap.ci = 0; }
  else qtap = decode_tap<T, PACKW>(p, kc);
  QRow qcur[QI];
  RowC jump;
  if (!IDENT) {
    jump = decode_row(p, BK);
#pragma unroll
    for (int i = 0; i < QI; ++i) {
      const RowC r = decode_row(p, min(kbeg + qrow0 + RPP_Q * i, p.M - 1));
      qcur[i].n = r.n; qcur[i].t = r.t; qcur[i].h = r.h; qcur[i].w = r.w;
      qrow_refresh(p, qcur[i], qtap);
    }
  }

  // DMA through buffer descriptors whose extent ends at position `kend`: rows past the end of this
  // split's slab (only the last k-tile can have them) are zero-filled by the range check, the k-tile
  // advance is the scalar offset, and the per-lane part is a loop-invariant 32-bit byte offset.
  // (one descriptor per term plane: the range check that zero-fills the ragged last k-tile is per plane)
  __amdgpu_buffer_rsrc_t rsP[NPL], rsQ[NPL];
#pragma unroll
  for (int pl = 0; pl < NPL; ++pl) {
    rsP[pl] = make_rsrc(Pb + (long long)pl * p.p_ps * 2, (unsigned)kend * (unsigned)p.ldp * 2u);
    rsQ[pl] = make_rsrc(Ab + (long long)pl * p.a_ps * 2, IDENT ? (unsigned)kend * (unsigned)p.lda * 2u : p.a_bytes);
  }
  unsigned poff[PI], qoff[IDENT ? QI : 1];
#pragma unroll
  for (int i = 0; i < PI; ++i)
    poff[i] = pok ? (unsigned)((kbeg + prow + RPP_P * i) * p.ldp + pch) * 2u : kOOB;
  if (IDENT) {
#pragma unroll
    for (int i = 0; i < QI; ++i)
      qoff[i] = qtap.ok ? (unsigned)((kbeg + qrow0 + RPP_Q * i) * p.lda + kc * 8) * 2u : kOOB;
  }

  auto load_tile = [&](int kt, int buf) {
    char* pt = smem + buf * BUF + wave_u * 1024;
    char* qt = smem + buf * BUF + NPL * PLP + wave_u * 1024;
    const int kb = kbeg + kt * BK;
    const unsigned pstep = (unsigned)(kt * BK) * (unsigned)p.ldp * 2u;
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
      for (int i = 0; i < PI; ++i) bufglds16_hidden(rsP[pl], poff[i], pstep, pt + pl * PLP + i * (NTHR * 16));
    if (IDENT) {
      const unsigned qstep = (unsigned)(kt * BK) * (unsigned)p.lda * 2u;
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
        for (int i = 0; i < QI; ++i) bufglds16_hidden(rsQ[pl], qoff[i], qstep, qt + pl * PLQ + i * (NTHR * 16));
    } else {
#pragma unroll
      for (int i = 0; i < QI; ++i) {
        const int k = kb + qrow0 + RPP_Q * i;
        unsigned off;
        if (PACKW) {   // W-padded stem input: the two pixels of the chunk are always inside the row
          const int w0 = qcur[i].w * p.sw - p.pw + qtap.c;
          off = (qtap.ok && qcur[i].hv && k < kend) ? (unsigned)(qcur[i].base + w0) * 8u : kOOB;
        } else {
          const int ws = qcur[i].w * p.sw - p.pw + qtap.c * p.dw;
          const bool ok = qtap.ok && qcur[i].hv && k < kend && (unsigned)ws < (unsigned)p.Ws;
          off = ok ? (unsigned)((qcur[i].base + ws) * p.lda + qtap.ci) * 2u : kOOB;
        }
        qrow_jump(p, qcur[i], jump, qtap);
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) bufglds16_hidden(rsQ[pl], off, 0, qt + pl * PLQ + i * (NTHR * 16));
      }
    }
  };

  f32x4_v acc[FQ][FP];
#pragma unroll
  for (int a = 0; a < FQ; ++a)
#pragma unroll
    for (int b = 0; b < FP; ++b) acc[a][b] = f32x4_v{0.f, 0.f, 0.f, 0.f};

  // bias gradient (GP::dbias): the workgroups of column tile 0 also sum the P tiles over the positions.  Thread -> one
  // 16-byte channel chunk (bc) of BK / BG consecutive-stride positions; 8 fp32 partial sums per thread, folded at the end.
  constexpr int BG = NTHR / CP;                 // position groups
  constexpr int BPP = BK / BG;                  // positions per thread and k-tile
  static_assert(SP || (BK % BG == 0 && BPP >= 1), "bias-gradient thread map");
  const bool do_bias = !SP && p.dbias != nullptr && tile_q == 0;     // workgroup-uniform
  const int bc = tid % CP, bg = tid / CP;
  float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  if (ktiles > 0) load_tile(0, 0);
  for (int kt = 0; kt < ktiles; ++kt) {
    // own DMA of tile kt landed, then a bare barrier (see gemm_nt_kernel): tile kt is complete and
    // the other buffer, last read for tile kt-1, may be refilled
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    if (kt + 1 < ktiles) load_tile(kt + 1, (kt + 1) & 1);
    const char* pt = smem + (kt & 1) * BUF;
    const char* qt = pt + NPL * PLP;
    if constexpr (!SP) {
      if (do_bias) {
#pragma unroll
        for (int j = 0; j < BPP; ++j) {
          const int r = bg + BG * j;            // position inside the tile (rows past the slab end were zero-filled)
          const int slot = (((bc >> 1) ^ tr_key<RSP>(r)) << 1) | (bc & 1);
          float v[8];
          Vec16<T>::load(reinterpret_cast<const T*>(pt + r * RSP + slot * 16), v);
#pragma unroll
          for (int e = 0; e < 8; ++e) bsum[e] += v[e];
        }
      }
    }
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      vec_t pf[NPL][FP], qf[NPL][FQ];
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) {
#pragma unroll
        for (int i = 0; i < FP; ++i) pf[pl][i] = tr_frag<RSP, vec_t>(pt + pl * PLP, wp * WP + i * 16, ks, lane);
#pragma unroll
        for (int j = 0; j < FQ; ++j) qf[pl][j] = tr_frag<RSQ, vec_t>(qt + pl * PLQ, wq * WQ + j * 16, ks, lane);
      }
      if constexpr (SP) {      // cross terms first, then the leading product (16 accumulators between two MFMAs on one)
#pragma unroll
        for (int j = 0; j < FQ; ++j)
#pragma unroll
          for (int i = 0; i < FP; ++i) acc[j][i] = V16<T>::mma(qf[NPL - 1][j], pf[0][i], acc[j][i]);
#pragma unroll
        for (int j = 0; j < FQ; ++j)
#pragma unroll
          for (int i = 0; i < FP; ++i) acc[j][i] = V16<T>::mma(qf[0][j], pf[NPL - 1][i], acc[j][i]);
      }
#pragma unroll
      for (int j = 0; j < FQ; ++j)
#pragma unroll
        for (int i = 0; i < FP; ++i)
          acc[j][i] = V16<T>::mma(qf[0][j], pf[0][i], acc[j][i]);
    }
  }

  // ---- epilogue: lane holds qq = qb + 0..3 for output row pp.  This kernel keeps its own text of tn_store
  // (vlfb_gemm_common.h): through the shared function the <bf16, float, 64, 128, IDENT, 4 waves, bias> instance went from 82
  // to 85 VGPRs (50 + 32 AGPRs -> 53 + 32) ----
  const bool vec_ok = (p.ldo & 3) == 0;
  const bool to_ws = p.splits > 1;
  if constexpr (!SP) {
    if (do_bias) {                               // (workgroup-uniform) fold the BG position groups through LDS, in order
      __syncthreads();                           // every wave is done with the last tile
      float* red = reinterpret_cast<float*>(smem);
#pragma unroll
      for (int e = 0; e < 8; ++e) red[bg * BP + bc * 8 + e] = bsum[e];
      __syncthreads();
      if (tid < BP && p0 + tid < p.Ncols) {
        float sum = 0.f;
        for (int j = 0; j < BG; ++j) sum += red[j * BP + tid];
        const int pp = p0 + tid;
        if (to_ws) p.ws[(long long)p.splits * ((long long)p.Ncols * p.ldo) + (long long)split * p.Ncols + pp] = sum;
        else p.dbias[pp] = sum * p.alpha * (p.rowscale ? p.rowscale[pp] : 1.f);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < FP; ++i) {
    const int pp = p0 + wp * WP + i * 16 + l15;
    if (pp >= p.Ncols) continue;
    const float rs = (to_ws || !p.rowscale) ? 1.f : p.rowscale[pp];
#pragma unroll
    for (int j = 0; j < FQ; ++j) {
      const int qb = q0 + wq * WQ + j * 16 + g * 4;
      if (qb >= p.K) continue;
      const int cnt = (p.K - qb) < 4 ? (p.K - qb) : 4;
      const long long idx = (long long)pp * p.ldo + qb;
      float v[4];
      if (to_ws) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = acc[j][i][r];
        store4<float>(reinterpret_cast<char*>(p.ws),
                      (long long)split * ((long long)p.Ncols * p.ldo) + idx, v, cnt, vec_ok);
      } else {
        char* Ob = p.O + (long long)z * p.o_bs * (long long)sizeof(OutT);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float x = acc[j][i][r] * p.alpha * rs;
          if (p.accumulate && r < cnt) x += ld_elem<OutT>(Ob, idx + r);
          v[r] = x;
        }
        store4<OutT>(Ob, idx, v, cnt, vec_ok);
      }
    }
  }
}

// =============================================================================================
// Stem WGRAD (conv1, bf16): dW[co][a][b][kw][c] = sum_pos G[pos][co] * X[t+a][2h+b][2w+kw][c].
// With Cin = 3 (packed to 4) the K = (kt*kh) x (8 kw x 4 c) gathered columns of a position come from
// only kt*kh short input rows, so the generic TN kernel spends its time issuing 16-byte gather DMAs
// (9 column tiles x 6 pieces per lane per 64 positions) and re-reads the 411 MB gradient once per
// column tile.  Here one workgroup takes whole OUTPUT ROWS (n, t, h): it stages the kt*kh raw input
// rows that row touches (Ws*8 bytes each, contiguous DMA) plus the Wr x 64 gradient tile, and every
// wave builds its MFMA fragments straight from the raw rows with ds_read_b64_tr_b16 -- the 16 columns
// (4 kw x 4 c) of a position are 32 contiguous bytes, consecutive positions are sw pixels apart.
// 8 waves x 9 column tiles of 16 x all 64 output channels = the whole 64 x K gradient stays in
// registers (144 accumulator VGPRs) across the workgroup's rows; slabs + wgrad_reduce as usual.
// 6x fewer DMA pieces, the gradient is read once.
// =============================================================================================
template <typename T>
__global__ __launch_bounds__(512) void stem_wgrad_kernel(const GP p) {
  typedef typename V16<T>::V vec_t;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int l15 = lane & 15, g = lane >> 4;
  const int taps = p.K >> 5;                       // (a, b) pairs
  const int rbytes = p.Ws * 8;                     // one staged input row (Cs = 4 bf16 per pixel)
  const int ppr = rbytes >> 4;                     // 16-byte pieces per row
  const int npieces = taps * ppr;
  const int poff_lds = npieces * 16;               // gradient tile behind the rows
  const int stage = poff_lds + p.Wr * 128;         // Cn = 64 bf16 per position
  const int split = blockIdx.x;
  const int tiles_total = p.tiles_m, tpw = p.kper;
  const int tile_beg = split * tpw;
  const int tile_end = min(tiles_total, tile_beg + tpw);

  const __amdgpu_buffer_rsrc_t rsX = make_rsrc(p.A, p.a_bytes);
  const __amdgpu_buffer_rsrc_t rsG = make_rsrc(p.P, p.b_bytes);

  // ---- per-lane DMA assignment (tile-invariant part) -------------------------------------------
  constexpr int RI = 8;                            // row pieces per lane (RI * 512 >= npieces, host-checked)
  int ra[RI], rb[RI], rj[RI];
#pragma unroll
  for (int i = 0; i < RI; ++i) {
    const int id = tid + 512 * i;
    const int tap = id / ppr;
    ra[i] = tap / p.kh;
    rb[i] = tap - ra[i] * p.kh;
    rj[i] = (id - tap * ppr) * 16;
  }
  // gradient tile: piece id -> (position row, 16-byte slot); the source chunk is XOR-swizzled so
  // that tr_frag<128> reads conflict-free (same layout as gemm_tn_tr_kernel with BP = 64)
  unsigned gvoff[2];
  bool gok[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int id = tid + 512 * i;
    const int row = id >> 3, slot = id & 7;
    const int pc = (((slot >> 1) ^ tr_key<128>(row)) << 1) | (slot & 1);
    gok[i] = row < p.Wr;
    gvoff[i] = (unsigned)(row * p.ldp + pc * 8) * 2u;
  }

  auto load_tile = [&](int tile, int buf) {
    const int h = tile % p.Hr;
    const int nt = tile / p.Hr;
    const int t = nt % p.Tr, n = nt / p.Tr;
    char* base = smem + buf * stage;
#pragma unroll
    for (int i = 0; i < RI; ++i) {
      if (tid + 512 * i < npieces) {
        const int tin = t * p.st - p.pt + ra[i], hin = h * p.sh - p.ph + rb[i];
        const bool ok = (unsigned)tin < (unsigned)p.Ts && (unsigned)hin < (unsigned)p.Hs;
        const unsigned off = ok ? (unsigned)(((n * p.Ts + tin) * p.Hs + hin) * rbytes + rj[i]) : kOOB;
        bufglds16_hidden(rsX, off, 0, base + (i * 512 + wave_u * 64) * 16);
      }
    }
    const unsigned gstep = (unsigned)(tile * p.Wr) * (unsigned)p.ldp * 2u;
#pragma unroll
    for (int i = 0; i < 2; ++i)
      if (gok[i]) bufglds16_hidden(rsG, gvoff[i], gstep, base + poff_lds + (i * 512 + wave_u * 64) * 16);
  };

  f32x4_v acc[kStemCT][4];
#pragma unroll
  for (int j = 0; j < kStemCT; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[j][i] = f32x4_v{0.f, 0.f, 0.f, 0.f};

  // this wave's column tiles: ct = wave * 9 + j  ->  tap = ct >> 1, kw half = ct & 1
  const int ct0 = wave_u * kStemCT;
  const int ncts = 2 * taps;
  const int pl = lane & 15;
  const int ksteps = (p.Wr + 31) >> 5;

  if (tile_beg < tile_end) load_tile(tile_beg, 0);
  for (int tile = tile_beg; tile < tile_end; ++tile) {
    const int buf = (tile - tile_beg) & 1;
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    if (tile + 1 < tile_end) load_tile(tile + 1, buf ^ 1);
    const char* rows = smem + buf * stage;
    const char* gt = rows + poff_lds;
    for (int ks = 0; ks < ksteps; ++ks) {
      const int r0 = ks * 32 + 8 * g + (pl >> 2);            // position read by this lane (first half)
      const bool live = ks * 32 + 8 * g < p.Wr;              // Wr % 8 == 0: the 8 positions of a group live or die together
      vec_t pf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        pf[i] = tr_frag<128, vec_t>(gt, i * 16, ks, lane);
        if (!live) pf[i] = vec_t{0, 0, 0, 0, 0, 0, 0, 0};
      }
      // dead positions read position Wr-1 instead (finite data x the zeroed gradient fragment)
      const int q0 = min(r0, p.Wr - 1), q1 = min(r0 + 4, p.Wr - 1);
      const int a0 = (q0 * p.sw - p.pw) * 8 + (pl & 3) * 8;
      const int a1 = (q1 * p.sw - p.pw) * 8 + (pl & 3) * 8;
      // all 9 fragments first, then the 36 MFMAs (no control flow in between: the column tiles past
      // the end of K, on the last wave only, recompute the last real tile and are dropped at the store)
      vec_t qf[kStemCT];
#pragma unroll
      for (int j = 0; j < kStemCT; ++j) {
        const int ct = min(ct0 + j, ncts - 1);
        const char* rowp = rows + (ct >> 1) * rbytes + (ct & 1) * 32;
        union { struct { s16x4_v a, b; } s; vec_t v; } u;
        u.s.a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_v*)(rowp + a0));
        u.s.b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_v*)(rowp + a1));
        qf[j] = u.v;
      }
#pragma unroll
      for (int j = 0; j < kStemCT; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          acc[j][i] = V16<T>::mma(qf[j], pf[i], acc[j][i]);
    }
  }

  // ---- slab of this workgroup: ws[split][co][K], lane holds 4 consecutive columns of row co -------
  float* slab = p.ws + (long long)split * ((long long)p.Ncols * p.ldo);
#pragma unroll
  for (int j = 0; j < kStemCT; ++j) {
    const int ct = ct0 + j;
    if (ct >= ncts) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int co = i * 16 + l15;
      *reinterpret_cast<float4*>(slab + (long long)co * p.ldo + ct * 16 + g * 4) =
          make_float4(acc[j][i][0], acc[j][i][1], acc[j][i][2], acc[j][i][3]);
    }
  }
}

// split-K slab reduction: a workgroup owns CL float4 columns (CL*16 contiguous bytes of every slab
// row); its G lane groups stride over the splits (4 loads in flight each) and fold through LDS; group
// 0 applies the epilogue.  Many splits (skinny weights: few columns, hundreds of slabs) use narrow
// 16-column workgroups so the grid still covers the chip.
// ws_b / dbias / nb (optional): the bias-gradient partial rows of the same split launch (GP::dbias: ws_b[split][nb] behind the
// weight slabs) are folded by the workgroups past the weight part of the grid, splits in order -- one launch per split WGRAD
// instead of two (the stand-alone wgrad_bias_reduce_kernel stays for the families whose column sums are a separate pass).
template <typename OutT, int G, int CL>
__global__ __launch_bounds__(CL * G) void wgrad_reduce_kernel(const float* ws, char* O, const float* rowscale,
                                                              long long n, int ldo, int splits, float alpha,
                                                              int accumulate, const float* __restrict__ ws_b = nullptr,
                                                              float* __restrict__ dbias = nullptr, int nb = 0, int wblocks = 0) {
  if (ws_b != nullptr && (int)blockIdx.x >= wblocks) {
    const int i = ((int)blockIdx.x - wblocks) * (CL * G) + (int)threadIdx.x;
    if (i < nb) {
      float s = 0.f;
      for (int k = 0; k < splits; ++k) s += ws_b[(long long)k * nb + i];
      dbias[i] = s * alpha * (rowscale ? rowscale[i] : 1.f);
    }
    return;
  }
  __shared__ float4 part[G > 1 ? (G - 1) * CL : 1];
  const int lane = threadIdx.x % CL, g = threadIdx.x / CL;
  const long long i = ((long long)blockIdx.x * CL + lane) * 4;
  float4 s = {0.f, 0.f, 0.f, 0.f};
  if (i < n) {
    const float* src = ws + i;
    int k = g;
    for (; k + 3 * G < splits; k += 4 * G) {
      float4 t0 = *reinterpret_cast<const float4*>(src + (long long)k * n);
      float4 t1 = *reinterpret_cast<const float4*>(src + (long long)(k + G) * n);
      float4 t2 = *reinterpret_cast<const float4*>(src + (long long)(k + 2 * G) * n);
      float4 t3 = *reinterpret_cast<const float4*>(src + (long long)(k + 3 * G) * n);
      s.x += (t0.x + t1.x) + (t2.x + t3.x); s.y += (t0.y + t1.y) + (t2.y + t3.y);
      s.z += (t0.z + t1.z) + (t2.z + t3.z); s.w += (t0.w + t1.w) + (t2.w + t3.w);
    }
    for (; k < splits; k += G) {
      float4 t = *reinterpret_cast<const float4*>(src + (long long)k * n);
      s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
    }
  }
  if (G > 1) {
    if (g > 0) part[(g - 1) * CL + lane] = s;
    __syncthreads();
    if (g == 0) {
#pragma unroll
      for (int j = 0; j < G - 1; ++j) {
        float4 t = part[j * CL + lane];
        s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
      }
    }
  }
  if (g == 0 && i < n) {
    float rs = alpha * (rowscale ? rowscale[i / ldo] : 1.f);
    float v[4] = {s.x * rs, s.y * rs, s.z * rs, s.w * rs};
    if (accumulate) {
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] += ld_elem<OutT>(O, i + r);
    }
    store4<OutT>(O, i, v, 4, true);
  }
}

// bias-gradient partial rows of a split WGRAD (GP::dbias): ws_b[split][n] -> out[n], splits folded in order
// (add: out[n] += ..., the further batch elements of a batched launch)
__global__ void wgrad_bias_reduce_kernel(const float* __restrict__ ws_b, float* __restrict__ out,
                                         const float* __restrict__ rowscale, int n, int splits, float alpha, int add) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int k = 0; k < splits; ++k) s += ws_b[(long long)k * n + i];
  const float v = s * alpha * (rowscale ? rowscale[i] : 1.f);
  out[i] = add ? out[i] + v : v;
}

// ---- host side: the launch of a plan (the planner is vlfb_conv_plan.hip) -------------------------
// every instance declares the LDS it needs once (64 KiB for the 128x128 tile)
template <auto Kernel>
int launch_k(const Plan& pl, hipStream_t s, const char* what) {
  return launch_lds<Kernel, 80 * 1024>(pl.grid, dim3(pl.threads), pl.lds, s, what, pl.gp);
}
// one tile shape, with or without the uniform-tap gather (UT only exists for gathered, unpacked operands)
template <typename T, typename OutT, int BM, int BN, bool IDENT, bool DGRAD, bool PACKW, int RB, bool PRE, int NW>
int launch_nt_shape(const Plan& pl, hipStream_t s, const char* what) {
  if constexpr (!IDENT && !PACKW) {
    if constexpr (DGRAD && sizeof(T) == 2) {
      if (pl.w2i) return launch_k<gemm_nt_kernel<T, OutT, BM, BN, IDENT, DGRAD, PACKW, RB, PRE, NW, 2, true, false, true>>(pl, s, what);
    }
    if (pl.ut) return launch_k<gemm_nt_kernel<T, OutT, BM, BN, IDENT, DGRAD, PACKW, RB, PRE, NW, 2, true>>(pl, s, what);
  }
  return launch_k<gemm_nt_kernel<T, OutT, BM, BN, IDENT, DGRAD, PACKW, RB, PRE, NW, 2, false>>(pl, s, what);
}

template <typename T, typename OutT, bool IDENT, bool DGRAD, bool PACKW>
int launch_nt(const Plan& pl, hipStream_t s, const char* what) {
  constexpr bool BF = sizeof(T) == 2;
  constexpr bool CAN_PRE = BF && sizeof(OutT) == 2 && !PACKW;
  constexpr int NW = BF ? 8 : 4;        // bf16: 8 waves (2 x 4) per workgroup; fp32 parity path: 4 (2 x 2)
  if (pl.bn == 64) {
    if (CAN_PRE && pl.pre) return launch_nt_shape<T, OutT, 128, 64, IDENT, DGRAD, PACKW, 128, CAN_PRE, NW>(pl, s, what);
    return launch_nt_shape<T, OutT, 128, 64, IDENT, DGRAD, PACKW, 128, false, NW>(pl, s, what);
  }
  if (CAN_PRE && pl.pre) return launch_nt_shape<T, OutT, 128, 128, IDENT, DGRAD, PACKW, 128, CAN_PRE, NW>(pl, s, what);
  return launch_nt_shape<T, OutT, 128, 128, IDENT, DGRAD, PACKW, 128, false, NW>(pl, s, what);
}
template <typename T, typename OutT, bool IDENT, bool PACKW>
int launch_tn(const Plan& pl, hipStream_t s, const char* what) {
  if (pl.bm == 128 && pl.bn == 128) return launch_k<gemm_tn_kernel<T, OutT, 128, 128, IDENT, PACKW>>(pl, s, what);
  if (pl.bm == 64 && pl.bn == 256) return launch_k<gemm_tn_kernel<T, OutT, 64, 256, IDENT, PACKW>>(pl, s, what);
  if (pl.bm == 64 && pl.bn == 128) return launch_k<gemm_tn_kernel<T, OutT, 64, 128, IDENT, PACKW>>(pl, s, what);
  if (pl.bm == 128 && pl.bn == 64) return launch_k<gemm_tn_kernel<T, OutT, 128, 64, IDENT, PACKW>>(pl, s, what);
  return launch_k<gemm_tn_kernel<T, OutT, 64, 64, IDENT, PACKW>>(pl, s, what);
}

template <typename T, typename OutT, bool IDENT, bool PACKW, bool SP>
int launch_tn_tr_as(const Plan& pl, hipStream_t s, const char* what) {
  if (pl.bm == 128 && pl.bn == 128) return launch_k<gemm_tn_tr_kernel<T, OutT, 128, 128, IDENT, PACKW, 8, SP>>(pl, s, what);   // 8 waves
  if (pl.bm == 64 && pl.bn == 128) return launch_k<gemm_tn_tr_kernel<T, OutT, 64, 128, IDENT, PACKW, 4, SP>>(pl, s, what);
  if (pl.bm == 128 && pl.bn == 64) return launch_k<gemm_tn_tr_kernel<T, OutT, 128, 64, IDENT, PACKW, 4, SP>>(pl, s, what);
  return launch_k<gemm_tn_tr_kernel<T, OutT, 64, 64, IDENT, PACKW, 4, SP>>(pl, s, what);
}
template <typename T, typename OutT, bool SP = false>
int launch_tn_tr(const Plan& pl, hipStream_t s, const char* what) {
  return pl.ident ? launch_tn_tr_as<T, OutT, true, false, SP>(pl, s, what)
         : pl.packw ? launch_tn_tr_as<T, OutT, false, true, SP>(pl, s, what)
                    : launch_tn_tr_as<T, OutT, false, false, SP>(pl, s, what);
}

template <typename T>
int launch_stem_wgrad(const Plan& pl, hipStream_t s) {
  return launch_lds<stem_wgrad_kernel<T>, 160 * 1024>(pl.grid, dim3(512), pl.lds, s, "conv wgrad (stem) kernel", pl.gp);
}

// the tiled families (tn, tn_tr, nt) in the instance of the element types
template <typename T, typename OutT>
int launch_tiled(const vlfb_conv_desc* d, const Plan& pl, hipStream_t s) {
  if constexpr (sizeof(T) == 2) {
    if (pl.family == Family::tn_tr) return launch_tn_tr<T, OutT>(pl, s, "conv wgrad (tr) kernel");
  }
  const char* what = "conv kernel";
  if (d->mode == VLFB_CONV_WGRAD) {
    if (pl.ident) return launch_tn<T, OutT, true, false>(pl, s, what);
    if (pl.packw) return launch_tn<T, OutT, false, true>(pl, s, what);
    return launch_tn<T, OutT, false, false>(pl, s, what);
  }
  if (d->mode == VLFB_CONV_DGRAD) {
    if (pl.ident) return launch_nt<T, OutT, true, false, false>(pl, s, what);
    return launch_nt<T, OutT, false, true, false>(pl, s, what);
  }
  if (pl.ident) return launch_nt<T, OutT, true, false, false>(pl, s, what);
  if (pl.packw) return launch_nt<T, OutT, false, false, true>(pl, s, what);
  return launch_nt<T, OutT, false, false, false>(pl, s, what);
}

// the kernel of the plan's family
int launch_plan(const vlfb_conv_desc* d, const Plan& pl, hipStream_t s) {
  const GP& g = pl.gp;
  const bool out_f32 = d->out_dtype == VLFB_F32;
  switch (pl.family) {
    case Family::tn:
    case Family::tn_tr:
    case Family::nt:
      if (d->dtype == VLFB_F32) return launch_tiled<float, float>(d, pl, s);
      if (d->dtype == VLFB_F16) return out_f32 ? launch_tiled<f16_t, float>(d, pl, s) : launch_tiled<f16_t, f16_t>(d, pl, s);
      return out_f32 ? launch_tiled<bf16_t, float>(d, pl, s) : launch_tiled<bf16_t, bf16_t>(d, pl, s);
    case Family::tn8: return launch_tn8(g, pl.grid, d->dtype, out_f32, s);
    case Family::stem_wgrad: VLFB_WITH_T16(d->dtype, return launch_stem_wgrad<T16>(pl, s));
    case Family::wgrad_rows: return launch_wgrad_rows(g, pl.splits, pl.lds, d->dtype, s);
    case Family::wgrad_rows_fat: return launch_wgrad_rows_fat(g, pl.splits, d->dtype, s);
    case Family::tn_split: return launch_tn_split(g, pl.bm, pl.bn, pl.ident, pl.packw, pl.grid, pl.lds, s);
    case Family::tn_tr_planes: return launch_tn_tr<bf16_t, float, true>(pl, s, "conv wgrad (planes) kernel");
    case Family::nt8:
      return launch_nt8(g, pl.bm, pl.bn, pl.nt8_mode, d->dtype, out_f32, (unsigned)(d->batch > 0 ? d->batch : 1), s);
    case Family::nt_stream: return launch_nts(g, pl.nts_mode, d->dtype, s);
    case Family::conv_rows64: return launch_conv_rows64(g, d->mode, d->dtype, s);
    case Family::stem_fprop: return launch_stem_fprop(g, d->dtype, s);
    case Family::nt_skinny: return launch_skinny_nt(g, d->dtype, out_f32, s);
    case Family::nt_skinny_split: return launch_skinny_nt_split(g, s);
    case Family::nt_split: return launch_nt_split(g, pl.sp, pl.bn, pl.sp_kind, pl.ut != 0, pl.grid, pl.lds, s);
    case Family::nt_planes: return launch_nt_planes(g, pl.sp, pl.bn, pl.sp_kind, pl.grid, pl.lds, s);
    case Family::nt_pair: return launch_nt_pair(g, pl.bn, pl.ident, pl.pre != 0, out_f32, pl.grid, pl.lds, s);
    case Family::nt8_pair: return launch_nt8_pair(g, pl.bm, pl.bn, pl.nt8_mode, out_f32, s);
    case Family::stem_fprop_pair: return launch_stem_fprop_pair(g, s);
  }
  return set_error(VLFB_ERR_ARG, "conv: plan without a kernel family");
}

}  // namespace
}  // namespace vlfb

using namespace vlfb;

int64_t vlfb_class_ap_workspace_bytes_impl(int64_t n, int64_t cols);   // vlfb_metrics.hip
int64_t vlfb_class_ap_voc_workspace_bytes_impl(int64_t n, int64_t cols);
extern "C" int64_t vlfb_query_workspace(int op, const void* arg) {
  if (!arg) { set_error(VLFB_ERR_ARG, "query_workspace: arg is required"); return -1; }
  switch (op) {
    case VLFB_WS_CONV: return vlfb_conv_workspace_bytes(static_cast<const vlfb_conv_desc*>(arg));
    case VLFB_WS_MAXPOOL_ARGMAX: {
      const vlfb_pool_desc* d = static_cast<const vlfb_pool_desc*>(arg);
      const int es = vlfb_pool_argmax_bytes(d);
      if (es <= 0) return -1;
      return (int64_t)d->N * d->To * d->Ho * d->Wo * d->C * es;
    }
    case VLFB_WS_FBO_ATTN_BWD: {
      const int64_t* v = static_cast<const int64_t*>(arg);
      if (v[0] <= 0 || v[1] <= 0) { set_error(VLFB_ERR_ARG, "query_workspace: r, k must be positive"); return -1; }
      return v[0] * v[1] * 4;
    }
    case VLFB_WS_ATTN_SCORES: {
      const int64_t* v = static_cast<const int64_t*>(arg);
      if (v[0] <= 0 || v[1] <= 0 || v[2] <= 0) { set_error(VLFB_ERR_ARG, "query_workspace: b, l1, l2 must be positive"); return -1; }
      return v[0] * v[1] * v[2] * 4;
    }
    case VLFB_WS_BN: {
      const int64_t* v = static_cast<const int64_t*>(arg);
      const int64_t n = vlfb_bn_workspace_bytes((int)v[0], v[1], v[2]);
      if (n < 0) set_error(VLFB_ERR_ARG, "query_workspace: bad dtype / rows / C for SpatialBN");
      return n;
    }
    case VLFB_WS_CLASS_AP: {
      const int64_t* v = static_cast<const int64_t*>(arg);
      const int64_t n = vlfb_class_ap_workspace_bytes_impl(v[0], v[1]);
      if (n < 0) set_error(VLFB_ERR_ARG, "query_workspace: class_ap needs 1 <= n <= %d and cols >= 1", VLFB_CLASS_AP_MAX_N);
      return n;
    }
    case VLFB_WS_CLASS_AP_VOC: {
      const int64_t* v = static_cast<const int64_t*>(arg);
      const int64_t n = vlfb_class_ap_voc_workspace_bytes_impl(v[0], v[1]);
      if (n < 0) set_error(VLFB_ERR_ARG, "query_workspace: class_ap_voc needs 1 <= n <= %d and cols >= 1", VLFB_CLASS_AP_MAX_N);
      return n;
    }
    default: set_error(VLFB_ERR_ARG, "query_workspace: unknown op %d", op); return -1;
  }
}

extern "C" int vlfb_conv_run(const vlfb_conv_desc* d, const void* A, const void* B, const void* P,
                             void* O, const float* bias, const float* rowscale, const void* R,
                             const void* Mask, void* workspace, int64_t workspace_bytes,
                             vlfb_stream_t stream) {
  return vlfb_conv_run_planes(d, A, B, P, O, bias, rowscale, R, Mask, workspace, workspace_bytes, nullptr, stream);
}

static int conv_run_impl(const vlfb_conv_desc* d, const void* A, const void* B, const void* P,
                         void* O, const float* bias, const float* rowscale, const void* R,
                         const void* Mask, void* workspace, int64_t workspace_bytes, void* O_planes, float* dbias,
                         vlfb_stream_t stream, const void* R_lo = nullptr, void* O_lo = nullptr);

extern "C" int vlfb_conv_run_args(const vlfb_conv_desc* d, const vlfb_conv_args* a, vlfb_stream_t stream) {
  VLFB_REQUIRE(d && a, "conv_run_args: descriptor and arguments are required");
  VLFB_REQUIRE(!d->wgrad_bias == !a->dbias, "conv_run_args: dbias goes with desc.wgrad_bias");
  return conv_run_impl(d, a->A, a->B, a->P, a->O, a->bias, a->rowscale, a->R, a->Mask, a->workspace, a->workspace_bytes,
                       a->O_planes, a->dbias, stream, a->R_lo, a->O_lo);
}

// conv + max-pool in one launch (vlfb_conv_run_maxpool): the plan of `d` and, when the pair cannot be fused, the reason.
// Implemented: the temporal pool (2x1x1, stride 2x1x1, no padding) behind a two-plane plain-row conv that plans on the
// 128 x 128 kernel with prefetched residual rows (gemm_nt_kernel POOL2).
static int conv_maxpool_plan(const vlfb_conv_desc* d, const vlfb_pool_desc* pd, Plan* pl, const char** why) {
  *why = nullptr;
  VLFB_REQUIRE(d && pd, "conv_maxpool: both descriptors are required");
  const int rc = cached_plan(d, pl);
  if (rc != VLFB_OK) return rc;
  const GP& g = pl->gp;
  if (d->mode != VLFB_CONV_FPROP || d->dtype != VLFB_F16 || d->math != VLFB_MATH_F16X3 || d->out_dtype != VLFB_F16)
    *why = "the conv is not a two-plane fp16 FPROP with a two-plane output";
  else if (pd->dtype != VLFB_F16PAIR || pd->N != d->N || pd->Ti != d->Tr || pd->Hi != d->Hr || pd->Wi != d->Wr || pd->C != d->Cn)
    *why = "the pool does not read the conv's two-plane output";
  else if (pd->kt != 2 || pd->kh != 1 || pd->kw != 1 || pd->st != 2 || pd->sh != 1 || pd->sw != 1 || pd->pt || pd->ph || pd->pw ||
           pd->To < 1 || pd->To != d->Tr / 2 || pd->Ho != d->Hr || pd->Wo != d->Wr)
    *why = "only the 2x1x1 pool with stride 2x1x1 and no padding is fused";
  else if (pl->family != Family::nt_pair || !pl->ident || pl->bm != 128 || pl->bn != 128 || !pl->pre || !g.vec_epi)
    *why = "the conv does not plan on the 128 x 128 two-plane plain-row kernel with prefetched residual rows";
  else if (d->batch > 1 || d->o_planes || d->bias_mode == VLFB_BIAS_ROW || g.ldo != d->Cn)
    *why = "batched launches, plane copies, row biases and strided output rows are not fused";
  return VLFB_OK;
}

extern "C" int vlfb_conv_maxpool_fusable(const vlfb_conv_desc* d, const vlfb_pool_desc* pool) {
  Plan pl;
  const char* why;
  if (conv_maxpool_plan(d, pool, &pl, &why) != VLFB_OK) return 0;
  return why == nullptr;
}

extern "C" int vlfb_conv_run_maxpool(const vlfb_conv_desc* d, const vlfb_pool_desc* pool, const vlfb_conv_args* a,
                                     void* argmax, vlfb_stream_t stream) {
  VLFB_REQUIRE(a, "conv_run_maxpool: arguments are required");
  Plan pl;
  const char* why;
  int rc = conv_maxpool_plan(d, pool, &pl, &why);
  if (rc != VLFB_OK) return rc;
  if (why) return set_error(VLFB_ERR_UNSUPPORTED, "conv_run_maxpool: %s", why);
  VLFB_REQUIRE(a->A && a->B && a->O && a->O_lo, "conv_run_maxpool: A, B and both pooled planes (O, O_lo) are required");
  VLFB_REQUIRE(!a->Mask && !a->O_planes && !a->dbias && !a->P, "conv_run_maxpool: no mask, plane copy, dbias or P operand");
  VLFB_REQUIRE(!a->R_lo || a->R, "conv: R_lo without R");
  VLFB_REQUIRE(d->bias_mode == VLFB_BIAS_NONE || a->bias != nullptr, "conv: bias_mode set but bias is NULL");
  GP& g = pl.gp;
  g.A = (const char*)a->A; g.B = (const char*)a->B; g.O = (char*)a->O; g.O2 = (char*)a->O_lo;
  g.bias = a->bias; g.R = (const char*)a->R; g.R2 = (const char*)a->R_lo;
  g.AM = (unsigned char*)argmax;
  g.p2_hw = d->Hr * d->Wr;
  g.p2_chunks = (g.p2_hw + 63) / 64;
  g.p2_to = pool->To;
  g.tiles_m = d->N * pool->To * g.p2_chunks;       // one row tile per (frame pair, chunk of 64 positions)
  static const int nt_epi = env_int("VLFB_NT_EPI", 1);
  g.nt_epi = nt_epi >= 1;                          // (a two-plane launch: the rule of conv_run_impl)
  // the fp32 tile is staged through LDS in ONE pass (the epilogue visits rows r and r + 64 back to back): 64 KiB, what a
  // launch with two k-tiles or more has anyway
  const size_t tile = (size_t)128 * 128 * 4;
  g.epi = 1;
  return launch_nt_pair_pool2(g, dim3((unsigned)(g.tiles_m * g.tiles_n), 1, 1), pl.lds < tile ? tile : pl.lds, (hipStream_t)stream);
}

extern "C" int vlfb_conv_run_planes(const vlfb_conv_desc* d, const void* A, const void* B, const void* P,
                                    void* O, const float* bias, const float* rowscale, const void* R,
                                    const void* Mask, void* workspace, int64_t workspace_bytes, void* O_planes,
                                    vlfb_stream_t stream) {
  VLFB_REQUIRE(!d->wgrad_bias, "conv: a descriptor with wgrad_bias runs through vlfb_conv_run_wgrad_bias");
  return conv_run_impl(d, A, B, P, O, bias, rowscale, R, Mask, workspace, workspace_bytes, O_planes, nullptr, stream);
}

extern "C" int vlfb_conv_run_wgrad_bias(const vlfb_conv_desc* d, const void* A, const void* P, void* O, float* dbias,
                                        const float* rowscale, void* workspace, int64_t workspace_bytes,
                                        vlfb_stream_t stream) {
  VLFB_REQUIRE(d->mode == VLFB_CONV_WGRAD && d->wgrad_bias && dbias, "conv_run_wgrad_bias: a WGRAD descriptor with wgrad_bias = 1 and dbias");
  return conv_run_impl(d, A, nullptr, P, O, nullptr, rowscale, nullptr, nullptr, workspace, workspace_bytes, nullptr, dbias, stream);
}

static int conv_run_impl(const vlfb_conv_desc* d, const void* A, const void* B, const void* P,
                         void* O, const float* bias, const float* rowscale, const void* R,
                         const void* Mask, void* workspace, int64_t workspace_bytes, void* O_planes, float* dbias,
                         vlfb_stream_t stream, const void* R_lo, void* O_lo) {
  Plan pl;
  int rc = cached_plan(d, &pl);
  if (rc != VLFB_OK) return rc;
  const bool h2 = d->math == VLFB_MATH_F16X3;
  const bool sp_pair = pl.sp && d->out_dtype == VLFB_F16;     // split launch writing (and adding) two fp16 planes
  VLFB_REQUIRE(!sp_pair || (O_lo && (!R || R_lo)), "conv: a two-plane fp16 output needs O_lo (and R_lo with R)");
  VLFB_REQUIRE(!h2 || d->out_dtype == VLFB_F32 || O_lo, "conv: F16X3 math with a 16-bit output writes two planes (O, O_lo)");
  VLFB_REQUIRE(!h2 || !Mask, "conv: F16X3 launches take no mask");
  // (a 16-bit FPROP / DGRAD with an fp32 output: O_lo = the same values rounded to the operand type, for the 16-bit launches
  // that read this tensor next)
  const bool copy16 = O_lo && !R_lo && !pl.sp && !h2 && is16(d->dtype) && d->out_dtype == VLFB_F32 && d->mode != VLFB_CONV_WGRAD;
  if ((R_lo || O_lo) && !sp_pair && !(h2 && d->out_dtype == VLFB_F32 && !R_lo)) {
    // two-term residual / output: the epilogues of the tiled NT families (128 x 128, 256-row pipelined) carry it
    VLFB_REQUIRE(d->mode != VLFB_CONV_WGRAD && is16(d->dtype) && (d->out_dtype == d->dtype || copy16) && !pl.sp,
                 "conv: R_lo / O_lo belong to 16-bit FPROP / DGRAD launches with 16-bit outputs (O_lo alone: also with an fp32 output)");
    VLFB_REQUIRE(!R_lo || R, "conv: R_lo without R");
    VLFB_REQUIRE(pl.gp.vec_epi, "conv: R_lo / O_lo need 16-byte aligned output rows");
  }
  VLFB_REQUIRE(A && O, "conv: A and O are required");
  if (d->mode == VLFB_CONV_WGRAD) VLFB_REQUIRE(P != nullptr, "conv: WGRAD needs P");
  else VLFB_REQUIRE(B != nullptr, "conv: FPROP/DGRAD need B");
  VLFB_REQUIRE(d->bias_mode == VLFB_BIAS_NONE || bias != nullptr, "conv: bias_mode set but bias is NULL");
  if (pl.ws_elems > 0 && (workspace == nullptr || workspace_bytes < pl.ws_elems * 4))
    return set_error(VLFB_ERR_WORKSPACE, "conv: split WGRAD needs %lld workspace bytes, got %lld",
                     (long long)pl.ws_elems * 4, (long long)workspace_bytes);
  VLFB_REQUIRE((d->o_planes > 0) == (O_planes != nullptr), "conv: O_planes goes with desc.o_planes");
  rc = resolve_for_operands(d, &pl, R != nullptr, Mask != nullptr, R_lo != nullptr, O_lo != nullptr);
  if (rc != VLFB_OK) return rc;
  GP& g = pl.gp;
  g.A = (const char*)A; g.B = (const char*)B; g.P = (const char*)P; g.O = (char*)O;
  g.bias = bias; g.rowscale = rowscale; g.R = (const char*)R; g.Mask = (const char*)Mask;
  g.ws = (float*)workspace;
  g.OP = (char*)O_planes;
  g.dbias = pl.bias_fused ? dbias : nullptr;
  g.R2 = (const char*)R_lo; g.O2 = (char*)O_lo;
  g.pair_io = sp_pair ? 1 : 0;
  // Non-temporal epilogue rows (GP::nt_epi) where a launch moves at least 4 bytes per output element through its epilogue
  // -- fp32 or two-plane outputs / residuals, two-term gradients: the "mix" and "split" launches, +1.0-1.3 % on their steps --
  // and not on plain 16-bit launches, whose steps measured -0.25 % with it (their rows are half as large, the next launch
  // finds more of them still cached).  VLFB_NT_EPI: 0 never, 1 this rule (default), 2 every launch.
  static const int nt_epi = env_int("VLFB_NT_EPI", 1);
  const bool wide_epi = h2 || pl.sp || pl.w2i || d->dt == 0 || d->out_dtype == VLFB_F32 || R_lo || O_lo;
  g.nt_epi = nt_epi >= 2 || (nt_epi == 1 && wide_epi);
  hipStream_t s = (hipStream_t)stream;
  rc = launch_plan(d, pl, s);
  if (rc != VLFB_OK) return rc;
  if (dbias && !pl.bias_fused) {
    // families without the fused column sums: one pass over P behind the launch -- per-slab partial rows behind the
    // weight slabs, folded in slab order (then alpha * rowscale, as the weights): deterministic
    VLFB_REQUIRE(!d->a_planes, "conv: wgrad_bias with pre-split operands is not supported (pass the fp32 operands)");
    const int slabs = colsum_slabs(d->dtype, g.M, d->Cn);
    float* part = g.ws + (pl.splits > 1 ? (long long)pl.splits * ((long long)d->Cn * g.ldo) : 0);
    // (a batched launch: db sums over the batch elements as well -- one pass per element through the same partial rows,
    // added in batch order on the stream)
    const int batch = d->batch > 0 ? d->batch : 1;
    const long long p_es = d->dtype == VLFB_F32 ? 4 : 2;
    for (int z = 0; z < batch; ++z) {
      rc = colsum_partials((const char*)P + (long long)z * g.p_bs * p_es, d->dtype, g.M, d->Cn, g.ldp, part, s);
      if (rc != VLFB_OK) return rc;
      hipLaunchKernelGGL(wgrad_bias_reduce_kernel, dim3((unsigned)((d->Cn + 63) / 64)), dim3(64), 0, s, part, dbias, rowscale,
                         d->Cn, slabs, d->alpha, z > 0 ? 1 : 0);
    }
  }
  // (a launch with fused column sums and splits: its bias partial rows are folded by the weight reduce below)
  const float* bias_rows = (dbias && pl.bias_fused && pl.splits > 1) ? g.ws + (long long)pl.splits * ((long long)d->Cn * g.ldo) : nullptr;
  if (pl.splits > 1) {
    const long long n = (long long)d->Cn * g.K;
    VLFB_REQUIRE(n % 4 == 0, "conv: split WGRAD output size must be a multiple of 4");
    const int G = pl.splits >= 32 ? 16 : pl.splits >= 8 ? 4 : 1;
#define VLFB_REDUCE(OT, GG, CC)                                                                                         \
  do {                                                                                                                  \
    const unsigned wblocks = (unsigned)((n / 4 + CC - 1) / CC);                                                         \
    const unsigned bblocks = bias_rows ? (unsigned)((d->Cn + CC * GG - 1) / (CC * GG)) : 0u;                            \
    hipLaunchKernelGGL((wgrad_reduce_kernel<OT, GG, CC>), dim3(wblocks + bblocks), dim3(CC * GG), 0, s, g.ws, g.O,     \
                       rowscale, n, g.ldo, pl.splits, d->alpha, d->accumulate, bias_rows, bias_rows ? dbias : nullptr,  \
                       (int)d->Cn, (int)wblocks);                                                                       \
  } while (0)
    with_elem(d->out_dtype, [&](auto t) {         // (the plan holds one of the three element types)
      using OT = decltype(t);
      if (G == 16) VLFB_REDUCE(OT, 16, 16); else if (G == 4) VLFB_REDUCE(OT, 4, 64); else VLFB_REDUCE(OT, 1, 64);
    });
#undef VLFB_REDUCE
    return check_launch("wgrad reduce");
  }
  return VLFB_OK;
}
