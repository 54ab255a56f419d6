// Host planner of the implicit-GEMM family: vlfb_conv_desc -> Plan (vlfb_conv_plan.h).  Every contraction of the step --
// forward convs, DGRAD, WGRAD, the attention products, the FBO convs -- is planned here; nothing in this file runs on the
// device.  make_plan is a list of steps: validate the descriptor, fill the launch geometry, collect the forms the
// NT (FPROP / DGRAD) or TN (WGRAD) side can run, size operands and LDS, resolve the ONE family that runs.
#include "vlfb_conv_plan.h"
#include <string>
#include <unordered_map>

namespace vlfb {

const char* family_name(Family f) {
  static const char* const names[] = {
      "tn", "tn_tr", "tn8", "stem_wgrad", "wgrad_rows", "wgrad_rows_fat", "tn_split", "tn_tr_planes",
      "nt", "nt8", "nt_stream", "conv_rows64", "stem_fprop", "nt_skinny", "nt_skinny_split", "nt_split", "nt_planes", "nt_pair",
      "nt8_pair", "stem_fprop_pair"};
  static_assert(sizeof(names) / sizeof(names[0]) == (size_t)Family::stem_fprop_pair + 1, "one name per Family value");
  return names[(int)f];
}

namespace {

int ilog2_exact(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return ((1 << l) == v) ? l : -1;
}

// what the descriptor says about the problem (validate_desc)
struct Problem {
  bool h2;        // VLFB_MATH_F16X3: both operands as two fp16 planes, three fp16 MFMAs per product (vlfb_gemm_pair.hip)
  bool sp_pl;     // split-bf16 math with operands that arrive as bf16 term planes (WGRAD: both; FPROP / DGRAD: the activation operand)
  int es, epc;    // bytes per element of the address arithmetic, elements per 16-byte chunk
  int batch, taps;
  int cpt;        // 16-byte chunks per tap
  long long M, K;
};

// the forms the choose_* steps found both legal and wanted; resolve_family picks the one that runs
struct Forms {
  int tn_tr;      // WGRAD: DMA + LDS transpose-read kernel (bf16)
  int stem;       // WGRAD: packed-stem kernel (whole output rows per workgroup, raw input rows in LDS)
  int rows;       // WGRAD: whole-row kernel for thin 64 -> 64 channel convs (vlfb_wgrad_rows.hip); 2 = its fat-input variant
  int tn8;        // WGRAD: 256 x 256 phase-pipelined kernel (plain rows)
  int nt8;        // NT: 256-row phase-pipelined kernel with this tile width (256 / 128), 0 = 128x128 kernel
  int nt8_bm;     //     rows per tile: 256 or 196
  int nts;        // NT: weight-resident streaming kernel (vlfb_gemm_s.hip)
  int rows64;     // FPROP / unit-stride DGRAD of 1x3x3 64 -> 64 convs: direct-convolution kernel (vlfb_conv_rows.hip)
  int stemf;      // FPROP of the packed stem: direct-convolution kernel (vlfb_stem.hip) when the call has no residual / mask
  int skinny;     // NT: at most 64 plain rows (vlfb_gemm_skinny.hip)
  int skinny_sp;  //     ... with split-bf16 math on fp32 rows (two terms, fp32 output without a copy)
  size_t rows_lds;  // LDS of the whole-row WGRAD forms (stem, rows)
};

int validate_desc(const vlfb_conv_desc* d, Plan* pl, Problem* pb) {
  VLFB_REQUIRE(dtype_ok(d->dtype), "conv: bad dtype %d", d->dtype);
  VLFB_REQUIRE(d->out_dtype == VLFB_F32 || d->out_dtype == d->dtype || (d->out_dtype == VLFB_F16 && d->math != VLFB_MATH_NATIVE), "conv: bad out_dtype");
  VLFB_REQUIRE(d->mode >= 0 && d->mode <= 2, "conv: bad mode %d", d->mode);
  VLFB_REQUIRE(d->math == VLFB_MATH_NATIVE || d->math == VLFB_MATH_BF16X3 || d->math == VLFB_MATH_BF16X6 || d->math == VLFB_MATH_F16X3 ||
                   d->math == VLFB_MATH_F16W2, "conv: bad math %d", d->math);
  pb->h2 = d->math == VLFB_MATH_F16X3;
  pl->w2i = d->math == VLFB_MATH_F16W2;
  VLFB_REQUIRE(!pl->w2i || (is16(d->dtype) && d->mode == VLFB_CONV_DGRAD && d->st == 1 && d->sh == 1 && d->sw == 1 && !d->pack_w &&
                            d->Cs % 64 == 0 && d->batch <= 1 && (d->algo == VLFB_ALGO_AUTO || d->algo == VLFB_ALGO_TILE128)),
               "conv: F16W2 math is the 16-bit DGRAD of a unit-stride conv with Cs %% 64 == 0 (two-term weights, VLFB_MIX_W2I)");
  VLFB_REQUIRE(!pb->h2 || (d->dtype == VLFB_F16 && d->mode == VLFB_CONV_FPROP && d->a_pstride > 0 && d->algo != VLFB_ALGO_STREAM &&
                           d->algo != VLFB_ALGO_CLASSES && d->algo != VLFB_ALGO_CLASS0),
               "conv: F16X3 math is an FPROP / NT product on fp16 planes (dtype VLFB_F16, a_pstride > 0)");
  // (split-bf16 FPROP / DGRAD with out_dtype VLFB_F16: the output -- and the residual, if any -- are two fp16 planes,
  // O / O_lo and R / R_lo of vlfb_conv_args: where an fp32 tensor enters the two-plane forward of the "mix" path)
  VLFB_REQUIRE(d->math == VLFB_MATH_NATIVE || pb->h2 || pl->w2i ||
                   (d->dtype == VLFB_F32 && (d->out_dtype == VLFB_F32 || (d->out_dtype == VLFB_F16 && d->mode != VLFB_CONV_WGRAD && !d->o_planes))),
               "conv: split-bf16 math needs fp32 operands and an fp32 (or two-plane fp16) output");
  VLFB_REQUIRE(d->math != VLFB_MATH_BF16X6 || d->mode != VLFB_CONV_WGRAD, "conv: WGRAD has no BF16X6 form (use BF16X3)");
  VLFB_REQUIRE(!d->accumulate || d->mode == VLFB_CONV_WGRAD, "conv: accumulate (O += ...) is a WGRAD epilogue");
  VLFB_REQUIRE(!d->wgrad_bias || d->mode == VLFB_CONV_WGRAD, "conv: wgrad_bias belongs to WGRAD descriptors");
  pl->sp = d->math == VLFB_MATH_BF16X6 ? 3 : d->math == VLFB_MATH_BF16X3 ? 2 : 0;     // (0 for F16X3 / F16W2)
  pl->sp_kind = 0;
  VLFB_REQUIRE(pl->sp || (!d->a_planes && !d->p_planes && !d->o_planes), "conv: a_planes / p_planes / o_planes belong to split-bf16 math");
  VLFB_REQUIRE(d->mode == VLFB_CONV_WGRAD ? (d->a_planes ? d->a_planes >= 2 && d->p_planes == 2 : d->p_planes == 0) && !d->o_planes
                                         : (d->a_planes == 0 || d->a_planes >= pl->sp) && !d->p_planes && (d->o_planes >= 0 && d->o_planes <= 2),
               "conv: bad a_planes / p_planes / o_planes for this mode");
  pb->sp_pl = d->a_planes > 0;
  // operands handed in as bf16 term planes are 2-byte elements for all address arithmetic below
  pb->es = (d->dtype == VLFB_F32 && !pb->sp_pl) ? 4 : 2;
  pb->epc = 16 / pb->es;
  pb->batch = d->batch > 0 ? d->batch : 1;
  VLFB_REQUIRE(d->N > 0 && d->Tr > 0 && d->Hr > 0 && d->Wr > 0, "conv: empty row space");
  VLFB_REQUIRE(d->Cs > 0 && d->Cn > 0, "conv: Cs/Cn must be positive");
  pb->M = (long long)d->N * d->Tr * d->Hr * d->Wr;
  VLFB_REQUIRE(pb->M < (1ll << 31), "conv: too many rows");
  pb->taps = d->kt * d->kh * d->kw;
  VLFB_REQUIRE(pb->taps >= 1, "conv: bad kernel size");
  pl->packw = d->pack_w != 0;
  if (pl->packw) {
    VLFB_REQUIRE(d->Cs == 4 && d->dw == 1 && d->pack_w >= d->kw && ilog2_exact(d->pack_w) >= 0,
                 "conv: pack_w needs Cs==4, dw==1 and a power-of-two kw_pad >= kw");
    VLFB_REQUIRE(d->mode != VLFB_CONV_DGRAD, "conv: pack_w has no DGRAD");
    pb->K = (long long)d->kt * d->kh * d->pack_w * 4;
    pb->cpt = d->pack_w * 4 / pb->epc;
  } else {
    VLFB_REQUIRE(d->Cs % pb->epc == 0, "conv: Cs=%d must be a multiple of %d", d->Cs, pb->epc);
    pb->K = (long long)pb->taps * d->Cs;
    pb->cpt = d->Cs / pb->epc;
  }
  pl->ident = !pl->packw && pb->taps == 1 && d->st == 1 && d->sh == 1 && d->sw == 1 && d->pt == 0 &&
              d->ph == 0 && d->pw == 0 && d->Ts == d->Tr && d->Hs == d->Hr && d->Ws == d->Wr;
  if (pl->w2i) pl->ident = false;        // (a 1x1x1 conv walks the tap cursor over its one tap)
  if (!pl->ident) {
    VLFB_REQUIRE(ilog2_exact(pb->cpt) >= 0, "conv: channels per tap must give a power-of-two chunk count");
    VLFB_REQUIRE(ilog2_exact(d->st) >= 0 && ilog2_exact(d->sh) >= 0 && ilog2_exact(d->sw) >= 0,
                 "conv: strides must be powers of two");
    VLFB_REQUIRE(pb->batch == 1, "conv: batched launches must be plain GEMMs");
  }
  return VLFB_OK;
}

// GP geometry and leading dimensions (the defaults of vlfb_conv_desc resolved)
int fill_geometry(const vlfb_conv_desc* d, const Problem& pb, Plan* pl) {
  GP& g = pl->gp;
  const long long K = pb.K;
  g.M = (int)pb.M; g.Ncols = d->Cn; g.K = (int)K;
  g.Tr = d->Tr; g.Hr = d->Hr; g.Wr = d->Wr; g.Ts = d->Ts; g.Hs = d->Hs; g.Ws = d->Ws; g.Cs = d->Cs;
  g.kt = d->kt; g.kh = d->kh; g.kw = d->kw;
  g.inv_khw = 1.0f / (float)(d->kh * d->kw); g.inv_kw = 1.0f / (float)d->kw; g.inv_kh = 1.0f / (float)d->kh;
  g.st = d->st; g.sh = d->sh; g.sw = d->sw; g.pt = d->pt; g.ph = d->ph; g.pw = d->pw;
  g.dt = d->dt; g.dh = d->dh; g.dw = d->dw;
  g.lst = ilog2_exact(d->st); g.lsh = ilog2_exact(d->sh); g.lsw = ilog2_exact(d->sw);
  g.cpt_shift = pl->ident ? 0 : ilog2_exact(pb.cpt);
  g.lda = d->lda ? d->lda : d->Cs;
  g.ldb = d->ldb ? d->ldb : (int)(pl->w2i ? 2 * K : K);      // (F16W2: a weight row holds both terms)
  g.ldp = d->ldp ? d->ldp : d->Cn;
  g.ldo = d->ldo ? d->ldo : (d->mode == VLFB_CONV_WGRAD ? (int)K : d->Cn);
  g.ldr = d->ldr ? d->ldr : g.ldo;
  g.a_bs = d->a_bstride; g.b_bs = d->b_bstride; g.o_bs = d->o_bstride; g.r_bs = d->r_bstride;
  g.p_bs = d->p_bstride;
  g.alpha = d->alpha; g.relu = d->relu; g.bias_mode = d->bias_mode; g.accumulate = d->accumulate;
  g.s2 = 0; g.s2_mq = 0; g.s2_tpc = 0;
  g.a_ps = d->a_pstride; g.p_ps = d->p_pstride; g.o_ps = d->o_pstride; g.op_n = d->o_planes; g.OP = nullptr;
  VLFB_REQUIRE((pl->packw || g.lda % pb.epc == 0) && (d->mode == VLFB_CONV_WGRAD || g.ldb % pb.epc == 0) &&
                   (d->mode != VLFB_CONV_WGRAD || g.ldp % pb.epc == 0),
               "conv: leading dimensions must keep 16-byte alignment");
  return VLFB_OK;
}

// rows enumerated parity class by parity class (GP::s2): n_classes = 4, or 1 when only class (0, 0) is launched
void set_parity_classes(GP& g, Plan* pl, long long M, int n_classes) {
  g.s2 = 1;
  g.s2_mq = (int)(M / 4);
  g.s2_tpc = (g.s2_mq + pl->bm - 1) / pl->bm;
  g.tiles_m = n_classes * g.s2_tpc;
  pl->grid = dim3((unsigned)(g.tiles_m * g.tiles_n), 1, 1);
}

// FPROP / DGRAD: the NT tile and the parity classes, then the 256-row, streaming, direct and skinny forms
int choose_nt_forms(const vlfb_conv_desc* d, const Problem& pb, Plan* pl, Forms* f) {
  GP& g = pl->gp;
  const long long M = pb.M, K = pb.K;
  const int es = pb.es, batch = pb.batch, taps = pb.taps;
  pl->bm = 128;
  pl->bn = d->Cn > 64 ? 128 : 64;
  g.tiles_m = (int)((M + pl->bm - 1) / pl->bm);
  g.tiles_n = (d->Cn + pl->bn - 1) / pl->bn;
  pl->grid = dim3((unsigned)(g.tiles_m * g.tiles_n), 1, (unsigned)batch);
  const int ept = d->out_dtype == VLFB_F32 ? 4 : 8;   // elements per 16-byte output store
  g.vec_epi = (d->Cn % ept == 0) && (g.ldo % ept == 0) && (g.ldr % ept == 0) &&
              (d->o_bstride % ept == 0) && (d->r_bstride % ept == 0);
  // DGRAD of a (1, 2, 2)-strided conv: three quarters of the (row, tap) pairs are structural zeros (an input
  // position only meets the taps of its own parity).  Rows enumerated class by class make every tile class-pure,
  // and a tile then walks only its class's taps: 9 -> 1 / 2 / 2 / 4 taps for the 3x3 convs of res3_0 / res4_0,
  // Measured at 8 clips (scratch/nts_probe.cpp): res3_0 2b 161 -> 110 us, res4_0 2b 156 -> 95 us.  NOT for the 1x1x1
  // shortcuts, where one class would do the whole GEMM and the other three only the epilogue: their residual /
  // output rows are then visited as 256-byte pieces of four different passes over the tensor instead of one
  // stream (198 -> 248 us, 153 -> 175 us).  Classes over h only (odd lines epilogue-only, as whole contiguous lines) are
  // no better (246 / 167 us): a tile without a k-loop has nothing to hide its residual loads behind.
  // (dt == 0: the doubled term dimension of two-term fp16 weights, VLFB_MIX_W2 -- the walk is the same per term)
  if (d->mode == VLFB_CONV_DGRAD && d->algo == VLFB_ALGO_AUTO && !pl->sp && !pl->ident && !pl->packw && batch == 1 && d->kh * d->kw > 1 &&
      d->st == 1 && d->sh == 2 && d->sw == 2 && (d->dt == 1 || d->dt == 0) && d->dh == 1 && d->dw == 1 && d->Hr % 2 == 0 &&
      d->Wr % 2 == 0 && ((long long)d->Cs * es) % 128 == 0 && d->bias_mode == VLFB_BIAS_NONE)
    set_parity_classes(g, pl, M, 4);
  // The strided 1x1x1 shortcut (VLFB_ALGO_CLASS0): only class (0, 0) meets its one tap, so ONLY that class's tiles are
  // launched -- a quarter of the rows, the whole k-loop, no epilogue-only tiles -- and the other rows of O stay as the
  // caller left them (the engine runs this DGRAD as the SECOND contribution to the block-input gradient, in place on the
  // first).  The "classes" form above lost on these convs because three of four tiles were epilogue-only passes.
  if (d->algo == VLFB_ALGO_CLASS0) {
    const bool ok = d->mode == VLFB_CONV_DGRAD && !pl->sp && !pl->ident && !pl->packw && batch == 1 && d->kh * d->kw == 1 &&
                    is16(d->dtype) && d->out_dtype == d->dtype && d->st == 1 && d->sh == 2 && d->sw == 2 && d->ph == 0 &&
                    d->pw == 0 && (d->dt == 1 || d->dt == 0) && d->Hr % 2 == 0 && d->Wr % 2 == 0 &&
                    ((long long)d->Cs * es) % 128 == 0 && d->bias_mode == VLFB_BIAS_NONE && !d->relu && g.vec_epi;
    VLFB_REQUIRE(ok, "conv: algo = CLASS0 is the 16-bit DGRAD of an unpadded (1, 2, 2)-strided 1x1x1 conv (even H, W; whole 128-byte taps)");
    set_parity_classes(g, pl, M, 1);                // class (0, 0) only
  }
  // The split-bf16 form of the same walk (gemm_nt_sp_kernel<.., S2>): a scalar tap cursor over the class's taps instead
  // of the per-lane decode.  Measured in the step (8 clips): res3_0 2b 502 -> 321 us, res4_0 2b 486 -> 240 us.  The 1x1x1
  // shortcuts stay on the plain walk here too (VLFB_SPLIT_S2_1X1=1 to try: 466 -> 513 us, 386 -> 380 us).
  static const bool s2_sp_off = env_int("VLFB_SPLIT_S2", 1) == 0;
  static const bool s2_sp_1x1_off = env_int("VLFB_SPLIT_S2_1X1", 0) != 1;
  const bool s2_sp_want = d->algo == VLFB_ALGO_CLASSES || (d->algo == VLFB_ALGO_AUTO && !s2_sp_off && (d->kh * d->kw > 1 || !s2_sp_1x1_off));
  if (d->mode == VLFB_CONV_DGRAD && s2_sp_want && pl->sp == 2 && !pb.sp_pl && !pl->ident && !pl->packw &&
      batch == 1 && d->st == 1 && d->sh == 2 && d->sw == 2 && d->dt == 1 && d->dh == 1 &&
      d->dw == 1 && d->Hr % 2 == 0 && d->Wr % 2 == 0 && d->Cs % 32 == 0 && d->bias_mode == VLFB_BIAS_NONE)
    set_parity_classes(g, pl, M, 4);
  VLFB_REQUIRE(d->algo != VLFB_ALGO_CLASSES || g.s2, "conv: algo = CLASSES is the split-math DGRAD of a (1, 2, 2)-strided conv (even H, W; Cs % 32 == 0)");

  if (d->algo != VLFB_ALGO_TILE128) {
    // 256-row phase-pipelined kernel (vlfb_gemm8.hip): bf16, 16-byte epilogue legal, at least 128 output
    // channels and 128 k; gathered operands need taps that span whole 64-element k-tiles (and unit stride
    // for DGRAD) and at most 32 taps (one validity bit per tap and row)
    // (two fp16 planes, pb.h2: a k-tile is 32 k of both planes -- taps of whole 32-channel runs; FPROP / plain rows only)
    const bool gather_ok = pl->ident || (!d->pack_w && ((long long)d->Cs * es) % (pb.h2 ? 64 : 128) == 0 && taps <= 32 &&
                                         (d->mode == VLFB_CONV_FPROP || (d->st == 1 && d->sh == 1 && d->sw == 1)));
    const bool ok = is16(d->dtype) && g.vec_epi && gather_ok && d->Cn >= 128 && K >= 128 && M >= 1024 && !pl->w2i &&
                    (!pb.h2 || (K % 32 == 0 && batch == 1));
    if (d->algo == VLFB_ALGO_PIPE256)
      VLFB_REQUIRE(ok, "conv: algo = PIPE256 needs bf16 / f16, Cn >= 128, K >= 128, M >= 1024, 16-byte aligned rows and "
                       "taps spanning whole k-tiles");
    // Library choice (measured per layer on MI355X at the 8-clip shapes, scratch/nt8_probe.cpp, tables in
    // profiles/): with ONE 128-160 KiB workgroup per CU the prologue and the epilogue of a tile are exposed,
    // so the pipelined kernel only wins where the k-loop is long and the tile count fills whole rounds of
    // CUs without a heavy epilogue: 512-column outputs with K >= 1024 (res5 3x3 / 3x1x1 / 1x1x1, the
    // non-local theta conv: 1.07-1.20x) and the batched P.g products of the non-local blocks (1.15-1.20x).
    // Elsewhere (Cn = 2048 with residual + mask epilogues, K <= 512, the res3 / res4 shapes whose tiles
    // fill half the chip) the 128x128 kernel with 2-3 co-resident workgroups is 1.1-1.6x faster.
    static const int pair8 = env_int("VLFB_PAIR_PIPE256", -1);     // (A/B switch: 0 never, 1 every eligible launch)
    // Two fp16 planes (pb.h2): 24 MFMAs per phase on the fragment reads and DMA pieces of the plain form's 16, so the
    // pipelined kernel pays on more shapes (measured per launch at 8 clips, scratch/r6/pair_probe.py: K >= 512 0.74-0.95x the
    // time of the 128-row kernel -- res5 3x3 361 -> 270 us = 1.31 PFLOP/s of MFMA issue, res5 3x1x1 494 -> 364 us -- except
    // the 2048-column layers with K = 512, whose residual epilogue dominates: 231 -> 250 us; K <= 256 0.94-1.36x)
    const bool want_h2 = pb.h2 && ok && (pair8 == 1 || (pair8 != 0 && K >= 512 && (d->Cn <= 1024 || K >= 1024)));
    const bool want = d->algo == VLFB_ALGO_PIPE256 || want_h2 ||
                      (ok && !pb.h2 && ((d->Cn == 512 && K >= 1024) ||
                              (batch > 1 && K >= 768 && d->Cn >= 256 && d->Cn <= 512 && d->out_dtype == d->dtype)));
    if (ok && want) {
      // tile shape: 256 / 196 rows (196 = two wave rows of 98: 7 of 8 fragment rows useful) x 256 / 128 columns,
      // whichever needs the fewest MFMA slots over whole rounds of 256 workgroups (one per CU)
      long long best = -1;
      for (int bn = 256; bn >= 128; bn -= 128)
        for (int bm = 256; bm >= 196; bm -= 60) {
          const long long tn = (d->Cn + bn - 1) / bn, tm = (M + bm - 1) / bm;
          const long long cost = (tn * tm * batch + 255) / 256 * (bm == 196 ? 7 : 8) * (bn / 128);
          if (best < 0 || cost < best) { best = cost; f->nt8 = bn; f->nt8_bm = bm; }
        }
      pl->nt8_mode = pl->ident ? 0 : (d->mode == VLFB_CONV_FPROP ? 1 : 2);
      g.tiles_n = (d->Cn + f->nt8 - 1) / f->nt8;
      g.tiles_m = (int)((M + f->nt8_bm - 1) / f->nt8_bm);
    }
  }
  if (d->algo != VLFB_ALGO_TILE128 && d->algo != VLFB_ALGO_PIPE256) {
    // weight-resident streaming kernel (vlfb_gemm_s.hip): the whole weight operand (<= ~150 KiB) lives in LDS,
    // every wave streams its own 16 / 32-position blocks without workgroup barriers -- for the HBM-bound layers
    const int mode = pl->ident ? 0 : (d->mode == VLFB_CONV_FPROP ? 1 : 2);
    const bool gather_ok = pl->ident || (!d->pack_w && taps <= 32 &&
                                         (d->mode == VLFB_CONV_FPROP || (d->st == 1 && d->sh == 1 && d->sw == 1)));
    const int uk = nts_chunk(mode, K);
    const bool shape_ok = (d->Cn == 64 || d->Cn == 128 || d->Cn == 256) && d->Cs % 64 == 0 && uk > 0 && M < (1ll << 24);
    const bool ok = is16(d->dtype) && !pb.h2 && !pl->w2i && d->out_dtype == d->dtype && batch == 1 && shape_ok && gather_ok &&
                    g.lda % 8 == 0 && g.ldb % 8 == 0 && g.ldo % 8 == 0 && g.ldr % 8 == 0 &&
                    (d->bias_mode == VLFB_BIAS_NONE || d->bias_mode == VLFB_BIAS_COL) &&
                    (long long)d->Cn * K * 2 + d->Cn * 4 <= 156 * 1024 &&
                    M * g.ldo * 2 < (1ll << 31) && M * g.ldr * 2 < (1ll << 31);
    if (d->algo == VLFB_ALGO_STREAM)
      VLFB_REQUIRE(ok, "conv: algo = STREAM needs bf16 / f16 in and out, batch 1, Cn in {64, 128, 256}, Cs %% 64 == 0, a weight "
                       "operand of at most 156 KiB, fewer than 2^24 rows, 16-byte aligned rows and operands below 2 GiB");
    // Library choice (measured at the 8-clip shapes, scratch/nts_probe.cpp and bench.py --detail): the 256-column
    // layers of res2 (0.8 M positions: 2c / shortcut fprop 1.04-1.08x alone, the 3x1x1 dgrad with residual + mask
    // 1.19x alone and 1.4x under the concurrent wgrad stream).  The 64-column variants are VALU-bound by the
    // per-block row decode and lose to the tiled kernel, res3 (0.1 M positions) has 3 blocks per wave.
    const bool want = d->algo == VLFB_ALGO_STREAM || (ok && M >= 400000 && d->Cn == 256);
    if (ok && want) { f->nts = 1; pl->nts_mode = mode; f->nt8 = 0; }
  }
  // packed stem FPROP: direct convolution, whole output rows per wave (vlfb_stem.hip)
  f->stemf = d->mode == VLFB_CONV_FPROP && pl->packw && d->algo == VLFB_ALGO_AUTO && !pb.h2 &&
             (d->bias_mode == VLFB_BIAS_NONE || d->bias_mode == VLFB_BIAS_COL) &&
             stem_fprop_ok(g, d->pack_w, d->dtype, d->out_dtype, batch);
  // ... and its two-plane form (fp16 planes in and out; one 134-KB stage, vlfb_stem.hip)
  static const bool pair_stem_off = env_int("VLFB_PAIR_STEM_DIRECT", 1) == 0;     // (A/B switch)
  if (pb.h2 && !pair_stem_off && d->mode == VLFB_CONV_FPROP && pl->packw && d->algo == VLFB_ALGO_AUTO && d->out_dtype == VLFB_F16 &&
      (d->bias_mode == VLFB_BIAS_NONE || d->bias_mode == VLFB_BIAS_COL) && stem_fprop_pair_ok(g, d->pack_w, batch))
    f->stemf = 1;
  f->rows64 = !pl->packw && !pl->ident && d->algo == VLFB_ALGO_AUTO && !pb.h2 && !pl->w2i &&
              (d->bias_mode == VLFB_BIAS_NONE || d->bias_mode == VLFB_BIAS_COL) &&
              conv_rows64_ok(g, d->mode, d->dtype, d->out_dtype, batch);
  // a handful of plain rows (the FBO head on one row per RoI): 16-column workgroups whose waves split K
  static const bool skinny_off = env_int("VLFB_SKINNY", 1) == 0;      // (A/B switch)
  f->skinny = d->algo == VLFB_ALGO_AUTO && !skinny_off && !pl->sp && !pb.h2 && !pl->w2i && !f->rows64 &&
              (d->out_dtype == d->dtype || d->out_dtype == VLFB_F32) && skinny_nt_ok(g, d->dtype, batch, pl->ident);
  // ... and the same rows in the fp32 head of the "mix" / "split" paths: two-term split-bf16 products (FPROP and DGRAD of the
  // FBO convs on one row per RoI: 26-29 us each on four 128 x 128 workgroups, 77 us for K = 2048)
  f->skinny_sp = d->algo == VLFB_ALGO_AUTO && !skinny_off && pl->sp == 2 && !pb.sp_pl &&
                 d->out_dtype == VLFB_F32 && d->o_planes <= 1 && skinny_nt_split_ok(g, batch, pl->ident);
  return VLFB_OK;
}

// whole-row WGRAD forms: each workgroup takes `kper` consecutive output rows (n, t, h) and writes one fp32 slab
void whole_row_splits(const vlfb_conv_desc* d, long long K, long long tiles_total, Plan* pl) {
  GP& g = pl->gp;
  const long long wgs = tiles_total < 256 ? tiles_total : 256;          // one workgroup per CU
  const long long tpw = (tiles_total + wgs - 1) / wgs;
  const int splits = (int)((tiles_total + tpw - 1) / tpw);
  g.tiles_m = (int)tiles_total;
  g.tiles_n = 1;
  g.kper = (int)tpw;
  g.splits = splits;
  pl->splits = splits;
  pl->ws_elems = (long long)splits * d->Cn * K;
}

// WGRAD: the TN tile, the 8-phase and whole-row forms, and the split count
int choose_tn_forms(const vlfb_conv_desc* d, const Problem& pb, Plan* pl, Forms* f) {
  GP& g = pl->gp;
  const long long M = pb.M, K = pb.K;
  const int es = pb.es, batch = pb.batch;
  pl->bm = d->Cn > 64 ? 128 : 64;             // P tile (output rows)
  pl->bn = K > 64 ? 128 : 64;                 // Q tile (output columns)
  // 256 x 256 phase-pipelined kernel (vlfb_gemm8.hip): plain-row bf16 operands with at least 128 of each
  {
    const bool ok = is16(d->dtype) && pl->ident && d->Cn % 8 == 0 && K % 8 == 0 && d->Cn >= 128 && K >= 128 &&
                    g.lda % 8 == 0 && g.ldp % 8 == 0;
    if (d->algo == VLFB_ALGO_PIPE256)
      VLFB_REQUIRE(ok, "conv: algo = PIPE256 WGRAD needs bf16 / f16 plain-row operands with Cn, K >= 128 (multiples of 8)");
    // library choice: every workgroup writes a 256 KiB fp32 slab, so only the large weights win
    // (Cn * K >= 1 M elements: res5 1x1x1 wgrads 1.3-1.66x; 0.5 M and below 0.6-0.97x, scratch/nt8_probe.cpp)
    f->tn8 = ok && d->algo != VLFB_ALGO_TILE128 &&
             (d->algo == VLFB_ALGO_PIPE256 || (batch == 1 && (long long)d->Cn * K >= (1ll << 20) && d->Cn >= 512 && K >= 512));
    if (f->tn8) pl->bm = pl->bn = 256;
  }
  // few output rows (res2 / stem, Cout = 64): widen the Q tile so a workgroup still has
  // 32 MFMAs per wave per k-tile of staging and the P panel is re-read half as often
  f->tn_tr = is16(d->dtype) && d->Cn % 8 == 0;
  if (f->tn8) f->tn_tr = 1;
  if (pb.sp_pl) {       // two-plane operands: the DMA + transposed-read kernel in its SP form
    VLFB_REQUIRE(d->Cn % 8 == 0 && (g.lda % 8 == 0 || pl->packw) && g.ldp % 8 == 0 && d->a_pstride % 8 == 0 && d->p_pstride % 8 == 0,
                 "conv: plane operands need channel counts / strides in multiples of 8");
    f->tn_tr = 1;
  }
  if (!f->tn_tr && pl->bm == 64 && K >= 256 && is16(d->dtype)) pl->bn = 256;
  if (f->tn_tr && !pl->sp && pl->packw && d->Cn == 64 && d->pack_w == 8 && d->Wr % 8 == 0 && d->Wr <= 128 &&
      d->dt == 1 && d->dh == 1 && d->splits <= 0 && batch == 1 && g.ldo == (int)K && (d->Ws * 8) % 16 == 0) {
    const int taps_ab = d->kt * d->kh;
    const long long npieces = (long long)taps_ab * (d->Ws * 8 / 16);
    const long long stage = npieces * 16 + (long long)d->Wr * 128;
    const long long tiles_total = (long long)d->N * d->Tr * d->Hr;
    if (npieces <= 4096 && taps_ab * 2 <= 8 * kStemCT && 2 * stage <= 160 * 1024 && tiles_total >= 2) {
      whole_row_splits(d, K, tiles_total, pl);
      f->stem = 1;
      f->rows_lds = (size_t)(2 * stage);
    }
  }
  // whole-row kernel (vlfb_wgrad_rows.hip): 64 -> 64 channels, unit stride, same-size output, rows of <= 64
  // positions (res2 3x3 / 3x1x1): every operand byte is read once, taps are LDS row offsets
  if (!f->stem && f->tn_tr && !pl->sp && !pl->packw && !pl->ident && d->algo == VLFB_ALGO_AUTO && d->Cs == 64 && d->Cn == 64 &&
      d->st == 1 && d->sh == 1 && d->sw == 1 && d->dt == 1 && d->dh == 1 && d->dw == 1 && d->Tr == d->Ts &&
      d->Hr == d->Hs && d->Wr == d->Ws && d->Wr % 8 == 0 && d->Ws + d->kw - 1 <= 64 && d->pw < d->kw &&
      wgrad_rows_ct(K) > 0 && d->kt * d->kh == 3 && d->splits <= 0 && batch == 1 && g.ldo == (int)K && g.lda == 64 && g.ldp == 64) {
    const long long tiles_total = (long long)d->N * d->Tr * d->Hr;
    if (tiles_total >= 2) {
      whole_row_splits(d, K, tiles_total, pl);            // one 128 KiB workgroup per CU
      f->rows = 1;
      f->rows_lds = (size_t)2 * ((size_t)d->kt * d->kh * (d->Ws + d->kw - 1) * 128 + (size_t)d->Wr * 128) + 1024;
    }
  }
  if (!f->stem && !f->rows && f->tn_tr && !pl->sp && !pl->packw && !pl->ident && d->algo == VLFB_ALGO_AUTO && d->Cs == 256 &&
      d->Cn == 64 && d->kt == 3 && d->kh == 1 && d->kw == 1 && d->st == 1 && d->sh == 1 && d->sw == 1 && d->dt == 1 &&
      d->Tr == d->Ts && d->Hr == d->Hs && d->Wr == d->Ws && d->ph == 0 && d->pw == 0 && d->pt < 3 && d->Wr % 8 == 0 &&
      d->Wr <= 64 && d->splits <= 0 && batch == 1 && g.ldo == (int)K && g.lda == 256 && g.ldp == 64) {
    const long long tiles_total = (long long)d->N * d->Ts * d->Hs;
    if (tiles_total >= 2) {
      whole_row_splits(d, K, tiles_total, pl);
      f->rows = 2;
      f->rows_lds = 0;
    }
  }
  if (f->stem || f->rows) {
    pl->grid = dim3((unsigned)pl->splits, 1, 1);
    return VLFB_OK;
  }
  g.tiles_m = (d->Cn + pl->bm - 1) / pl->bm;
  g.tiles_n = (int)((K + pl->bn - 1) / pl->bn);
  const int bk = pb.sp_pl ? 32 : 128 / es;          // positions per k-tile of the kernel that will run
  int splits = d->splits;
  if (splits <= 0) {
    // Pick the split count that fills whole rounds of `slots` workgroups best (every extra split
    // costs one more fp32 slab pass), keeping at least 8 k-tiles of work per split.  Two 64 KiB-LDS
    // workgroups fit a CU (512 slots), but these launches share the chip with the dgrad chain of
    // the main stream: rounds of 256 (one workgroup per CU, half the slab traffic) measured best
    // end to end (336 vs 331 clips/s at 512, 323 at 128).
    const long long tiles = (long long)g.tiles_m * g.tiles_n * batch;
    // (split-bf16 math: one 4-wave workgroup per CU leaves every SIMD with a single wave, whose staging and MFMA
    // phases then run back to back; two per CU -- 2 x 64 KiB of LDS -- overlap them)
    // (re-measured in round 3 on the bf16 path, one box: 256 -> 448.7, 384 -> 436.8, 512 -> 429.9, 768 -> 426.0 clips/s)
    const long long slots = (pl->sp && pl->bm > 64) ? 512 : 256;   // (the 64-row tiles of res2 measured slower at 512)
    long long maxs = (M + 8 * bk - 1) / (8 * bk);
    const long long slab_cap = (96ll << 20) / ((long long)d->Cn * K * 4);   // <= 96 MiB of fp32 slabs
    if (maxs > slab_cap) maxs = slab_cap;
    if (maxs > 1024) maxs = 1024;
    if (batch > 1 || maxs < 1) maxs = 1;
    double best = -1.0;
    splits = 1;
    for (long long sp = 1; sp <= maxs; sp = (sp < 8 ? sp + 1 : sp + 8)) {   // 1..8, then multiples of 8
      const long long total = tiles * sp;
      const double eff = (double)total / (double)(((total + slots - 1) / slots) * slots);
      if (eff > best + 0.03) { best = eff; splits = (int)sp; }
    }
  }
  VLFB_REQUIRE(splits == 1 || batch == 1, "conv: split WGRAD cannot be batched");
  long long kper = (M + splits - 1) / splits;
  kper = (kper + bk - 1) / bk * bk;
  splits = (int)((M + kper - 1) / kper);
  g.kper = (int)kper;
  g.splits = splits;
  pl->splits = splits;
  if (splits > 1) {
    VLFB_REQUIRE(g.ldo == (int)K, "conv: split WGRAD needs a dense output (ldo == K)");
    pl->ws_elems = (long long)splits * d->Cn * K;
  }
  if (splits > 1 && splits % 8 == 0)
    pl->grid = dim3((unsigned)(g.tiles_m * g.tiles_n * splits), 1, 1);
  else
    pl->grid = dim3((unsigned)(g.tiles_m * g.tiles_n), (unsigned)splits, (unsigned)batch);
  return VLFB_OK;
}

// operand extents behind the buffer descriptors, workgroup size, tap cursor and LDS of the tiled kernels
int size_operands_and_lds(const vlfb_conv_desc* d, const Problem& pb, const Forms& f, Plan* pl) {
  GP& g = pl->gp;
  const long long M = pb.M, K = pb.K;
  const int es = pb.es, batch = pb.batch;
  const int rb = 128;    // NT tile-row bytes (64-byte tile rows were measured slower: 314 vs 348 TFLOP/s at the time, twice the barriers)
  pl->pre = 0;
  pl->threads = kThreads;
  if (d->mode == VLFB_CONV_WGRAD && f.tn_tr && pl->bm == 128 && pl->bn == 128) {
    pl->threads = 512;       // 8 waves per workgroup
  }
  if (d->mode != VLFB_CONV_WGRAD && is16(d->dtype)) pl->threads = 512;   // 8 waves (2 x 4), both tile widths
  {
    // extents behind the buffer descriptors of the DMA kernels (one batch element)
    const long long a_rows = pl->ident ? M : (long long)d->N * d->Ts * d->Hs * d->Ws;
    long long a_bytes = a_rows * (pl->packw ? 4 : g.lda) * es;
    long long b_bytes = d->mode == VLFB_CONV_WGRAD ? M * g.ldp * es : (long long)d->Cn * g.ldb * es;
    if (pl->sp && d->mode != VLFB_CONV_WGRAD) {
      // the weight operand is pl->sp bf16 planes b_ps elements apart; one descriptor spans all of them
      g.b_ps = d->b_pstride > 0 ? d->b_pstride : (long long)batch * (batch > 1 ? d->b_bstride : (long long)d->Cn * g.ldb);
      VLFB_REQUIRE(K % 8 == 0 && g.ldb % 8 == 0 && g.b_ps % 8 == 0 && d->b_bstride % 8 == 0,
                   "conv: split-bf16 math needs K, ldb and the plane / batch strides of B in multiples of 8");
      VLFB_REQUIRE(g.vec_epi, "conv: split-bf16 math needs 16-byte aligned output rows (Cn, ldo, ldr multiples of 4)");
      b_bytes = ((long long)(pl->sp - 1) * g.b_ps + (long long)d->Cn * g.ldb) * 2;
    }
    long long a_bytes_all = a_bytes;
    if (pb.h2) {
      // (batched plain products -- the attention scores of a non-local block, theta x phi^T: the planes of ALL batch elements lie
      // a_pstride / b_pstride apart, a batch element a_bstride / b_bstride inside its plane)
      g.b_ps = d->b_pstride > 0 ? d->b_pstride : (long long)batch * (batch > 1 ? d->b_bstride : (long long)d->Cn * g.ldb);
      VLFB_REQUIRE(K % 8 == 0 && g.ldb % 8 == 0 && (pl->packw || g.lda % 8 == 0) && g.b_ps % 8 == 0 && d->a_pstride % 8 == 0 && g.vec_epi &&
                       d->a_bstride % 8 == 0 && d->b_bstride % 8 == 0,
                   "conv: F16X3 math needs K, lda, ldb, the plane / batch strides and the output rows in multiples of 8 elements");
      a_bytes_all = g.a_ps * 2 + a_bytes;          // one descriptor spans both planes
      b_bytes = (g.b_ps + (long long)d->Cn * g.ldb) * 2;
    }
    a_bytes = a_bytes_all;
    VLFB_REQUIRE(a_bytes < (1ll << 31) && b_bytes < (1ll << 31),
                 "conv: an operand of %lld / %lld bytes exceeds the 2 GiB a buffer descriptor addresses; split the batch",
                 a_bytes, b_bytes);
    g.a_bytes = (unsigned)a_bytes;
    g.b_bytes = (unsigned)b_bytes;
  }
  pl->ut = 0;
  if (d->mode != VLFB_CONV_WGRAD) {
    pl->ut = !pl->ident && !d->pack_w && ((pl->sp || pb.h2) ? d->Cs % 32 == 0 : ((long long)d->Cs * es) % rb == 0) &&
             (d->mode == VLFB_CONV_FPROP || (d->st == 1 && d->sh == 1 && d->sw == 1));
    const long long ktiles = pb.h2 ? (K + 31) / 32 : (pl->w2i ? 2 : 1) * ((K * es + rb - 1) / rb);   // (two planes: a 128-byte row is 32 k)
    if (pb.h2) {
      if (pl->packw && d->pack_w == 8) {
        // the packed stem as a kw = 1 conv of 32 "channels" per (a, b) tap row (see the split-bf16 form below)
        g.kw = 1; g.Cs = d->pack_w * 4; g.lda = 4;
        pl->ut = 1;
      }
      VLFB_REQUIRE(pl->ident || pl->ut, "conv: F16X3 math needs plain rows or taps that span whole 32-element k-tiles");
    }
    VLFB_REQUIRE(!pl->w2i || (pl->ut && g.vec_epi), "conv: F16W2 math needs taps of whole 64-channel runs and 16-byte aligned output rows");
    const size_t buf = (size_t)(pl->bm + pl->bn) * rb;
    pl->lds = (ktiles <= 1 ? 1 : 2) * buf;           // a single k-tile needs no second buffer
    const size_t tile = (size_t)pl->bm * pl->bn * 4;
    g.epi = (int)((tile + pl->lds - 1) / pl->lds);
    if (g.epi > 2) { pl->lds = tile / 2; g.epi = 2; }
    // (re-measured in round 3: prefetching for <= 16 / 36 / all k-tiles instead of 8 moves the bf16 step by -0.1 .. -0.7 %)
    static const int pre_kt = env_int("VLFB_PAIR_PRE_KT", 16);       // (A/B switch)
    pl->pre = g.vec_epi && ktiles <= (pb.h2 ? pre_kt : 8);   // host decides; only launches with R / Mask use it (two planes: 32-k tiles)
    if (pl->sp) {
      pl->sp_kind = pl->ident ? 0 : pl->packw ? 3 : d->mode == VLFB_CONV_FPROP ? 1 : 2;
      pl->threads = kThreads;
      pl->pre = 0;
      if (pl->packw && d->mode == VLFB_CONV_FPROP && d->pack_w == 8) {
        // The packed stem at k-tiles of 32 elements: one k-tile IS one (a, b) tap row (8 kw pixels x 4 channels), so the
        // gather is the scalar-cursor one of a conv with kw = 1, 32 "channels" per tap and 4 elements per pixel -- no
        // per-lane tap decode (it cost ~100 VALU per k-tile next to 48 MFMAs).  The W-padded input keeps every w in range.
        g.kw = 1; g.Cs = d->pack_w * 4; g.lda = 4;
        pl->ut = 1;
        pl->sp_kind = 1;
      }
      if (g.s2) { pl->ut = 1; pl->sp_kind = 2; }
      VLFB_REQUIRE(!pb.sp_pl || ((pl->ident || pl->ut) && d->a_pstride % 8 == 0 && (g.lda % 8 == 0 || pl->packw)),
                   "conv: a pre-split activation operand needs plain rows or taps that span whole 32-element k-tiles");
      VLFB_REQUIRE(d->o_planes != 2 || (d->o_pstride % 4 == 0 && batch == 1), "conv: o_planes = 2 needs batch 1 and an aligned o_pstride");
      const size_t sbuf = (pb.sp_pl ? (size_t)pl->sp * 128 * 64 : (size_t)128 * 128) + (size_t)pl->sp * pl->bn * 64;
      pl->lds = 2 * sbuf;
      if (pl->lds < (size_t)128 * pl->bn * 4) pl->lds = (size_t)128 * pl->bn * 4;
    }
  } else {
    pl->lds = (size_t)2 * (pl->bm + pl->bn) * 128;
    if (f.stem || f.rows) { pl->lds = f.rows_lds; pl->threads = 512; }
  }
  return VLFB_OK;
}

// THE priority order among the forms: which family runs, and the tile it runs with
void resolve_family(const vlfb_conv_desc* d, const Problem& pb, const Forms& f, Plan* pl) {
  const bool h16 = is16(d->dtype);
  Family fam;
  if (d->mode == VLFB_CONV_WGRAD) {
    fam = pl->sp ? (pb.sp_pl ? Family::tn_tr_planes : Family::tn_split)
          : (h16 && f.stem) ? Family::stem_wgrad : (h16 && f.rows == 2) ? Family::wgrad_rows_fat : (h16 && f.rows) ? Family::wgrad_rows
          : (h16 && f.tn8) ? Family::tn8 : (h16 && f.tn_tr) ? Family::tn_tr : Family::tn;
  } else {
    if (f.skinny_sp) fam = Family::nt_skinny_split;
    else if (pl->sp) fam = pb.sp_pl ? Family::nt_planes : Family::nt_split;
    else if (pb.h2 && f.stemf) fam = Family::stem_fprop_pair;
    else if (pb.h2 && f.nt8) fam = Family::nt8_pair;
    else if (pb.h2) fam = Family::nt_pair;
    else if (h16 && f.skinny) fam = Family::nt_skinny;
    else if (h16 && d->mode == VLFB_CONV_FPROP && f.stemf) fam = Family::stem_fprop;
    else if (h16 && f.rows64) fam = Family::conv_rows64;
    else if (h16 && f.nts) fam = Family::nt_stream;
    else if (h16 && f.nt8) fam = Family::nt8;
    else fam = Family::nt;
  }
  pl->family = fam;
  if (fam == Family::nt_skinny_split) { pl->bm = 64; pl->bn = 16; }
  if (fam == Family::nt8 || fam == Family::nt8_pair) { pl->bm = f.nt8_bm; pl->bn = f.nt8; }
}

int make_plan(const vlfb_conv_desc* d, Plan* pl) {
  ::memset(&pl->gp, 0, sizeof(pl->gp));
  pl->splits = 1;
  pl->ws_elems = 0;
  pl->nt8_mode = pl->nts_mode = 0;
  Problem pb;
  Forms f = {};
  int rc = validate_desc(d, pl, &pb);
  if (rc == VLFB_OK) rc = fill_geometry(d, pb, pl);
  if (rc == VLFB_OK) rc = d->mode != VLFB_CONV_WGRAD ? choose_nt_forms(d, pb, pl, &f) : choose_tn_forms(d, pb, pl, &f);
  if (rc == VLFB_OK) rc = size_operands_and_lds(d, pb, f, pl);
  if (rc != VLFB_OK) return rc;
  resolve_family(d, pb, f, pl);
  // bias gradient next to the weight gradient (vlfb_conv_run_wgrad_bias): inside the transposed-read kernel where that
  // is what runs; every other family gets a column-sum pass behind it
  pl->bias_fused = d->wgrad_bias && pl->family == Family::tn_tr && pb.batch == 1 && !d->accumulate;
  if (pl->bias_fused && pl->splits > 1) pl->ws_elems += (long long)pl->splits * d->Cn;
  // (other families: per-slab column sums behind the weight slabs, folded in order -- no atomics)
  if (d->mode == VLFB_CONV_WGRAD && d->wgrad_bias && !pl->bias_fused)
    pl->ws_elems += (long long)colsum_slabs(pb.sp_pl ? VLFB_BF16 : d->dtype, pb.M, d->Cn) * d->Cn;
  return VLFB_OK;
}

}  // namespace

// (a training step replays the same ~280 descriptors; the planner's split search is not free)
int cached_plan(const vlfb_conv_desc* d, Plan* out) {
  static thread_local std::unordered_map<std::string, Plan> cache;
  const std::string key(reinterpret_cast<const char*>(d), sizeof(*d));
  auto it = cache.find(key);
  if (it != cache.end()) { *out = it->second; return VLFB_OK; }
  const int rc = make_plan(d, out);
  if (rc == VLFB_OK) {
    if (cache.size() > 4096) cache.clear();
    cache.emplace(key, *out);
  }
  return rc;
}

int resolve_for_operands(const vlfb_conv_desc* d, Plan* pl, bool has_R, bool has_Mask, bool has_R_lo, bool has_O_lo) {
  // two-term residual / output: the epilogues of the tiled NT families (128 x 128, 256-row pipelined) carry it
  // (only 16-bit native launches plan these four; the two-plane and split launches take R_lo / O_lo as their own planes)
  if ((has_R_lo || has_O_lo) && (pl->family == Family::nt_skinny || pl->family == Family::conv_rows64 ||
                                 pl->family == Family::nt_stream || pl->family == Family::stem_fprop)) {
    vlfb_conv_desc d2 = *d;
    d2.algo = VLFB_ALGO_TILE128;
    const int rc = cached_plan(&d2, pl);
    if (rc != VLFB_OK) return rc;
  }
  if (has_R || has_Mask) {
    if (pl->family == Family::stem_fprop) pl->family = Family::nt;
    if (pl->family == Family::stem_fprop_pair) pl->family = Family::nt_pair;
  } else {
    pl->pre = 0;
  }
  return VLFB_OK;
}

}  // namespace vlfb

using namespace vlfb;

extern "C" void vlfb_conv_desc_init(vlfb_conv_desc* d) {
  ::memset(d, 0, sizeof(*d));
  d->dtype = VLFB_BF16; d->out_dtype = VLFB_BF16;
  d->N = d->Tr = d->Hr = d->Wr = 1;
  d->Ts = d->Hs = d->Ws = 1;
  d->kt = d->kh = d->kw = 1;
  d->st = d->sh = d->sw = 1;
  d->dt = d->dh = d->dw = 1;
  d->batch = 1;
  d->alpha = 1.0f;
}

extern "C" int64_t vlfb_conv_workspace_bytes(const vlfb_conv_desc* d) {
  Plan pl;
  if (cached_plan(d, &pl) != VLFB_OK) return -1;
  return pl.ws_elems * 4;
}

// Which kernel family, tile shape and split count the library runs for a descriptor (the planner is a pure function
// of the descriptor, so this IS what vlfb_conv_run launches; R / Mask only decide between the direct stem FPROP and the
// tiled kernel).  Test / bench support: "the plan under test is the plan under the stopwatch".
extern "C" int vlfb_conv_plan_describe(const vlfb_conv_desc* d, char* buf, int64_t buf_bytes) {
  VLFB_REQUIRE(d && buf && buf_bytes >= 96, "conv_plan_describe: buf of at least 96 bytes");
  Plan pl;
  const int rc = cached_plan(d, &pl);
  if (rc != VLFB_OK) return rc;
  const char* dt = d->dtype == VLFB_F32 ? (pl.sp ? (pl.sp == 3 ? "f32x6" : "f32x3") : "f32")
                   : d->math == VLFB_MATH_F16X3 ? "f16x3" : d->dtype == VLFB_F16 ? "f16" : "bf16";
  if (d->mode == VLFB_CONV_WGRAD)
    snprintf(buf, (size_t)buf_bytes, "%s %s %dx%d splits=%d", family_name(pl.family), dt, pl.bm, pl.bn, pl.splits);
  else
    snprintf(buf, (size_t)buf_bytes, "%s %s %dx%d%s%s%s%s", family_name(pl.family), dt, pl.bm, pl.bn, pl.ut ? " ut" : "",
             pl.gp.s2 ? (d->algo == VLFB_ALGO_CLASS0 ? " class0" : " classes") : "", pl.w2i ? " w2" : "", pl.pre ? " pre" : "");
  return VLFB_OK;
}
