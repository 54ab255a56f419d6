// Host planner of the implicit-GEMM family (vlfb_conv_plan.hip): a descriptor resolves to ONE kernel family, with its
// tile, split count, grid and LDS size.  vlfb_gemm.hip launches what the plan names (one switch over Plan::family) and
// vlfb_conv_plan_describe prints it, so the plan under test is the plan under the stopwatch.
#pragma once
#include "vlfb_gemm_common.h"

namespace vlfb {

// One value per kernel family; family_name() is the only place their names are spelled.
enum class Family : int {
  tn, tn_tr, tn8, stem_wgrad, wgrad_rows, wgrad_rows_fat, tn_split, tn_tr_planes,                          // WGRAD
  nt, nt8, nt_stream, conv_rows64, stem_fprop, nt_skinny, nt_skinny_split, nt_split, nt_planes, nt_pair,   // FPROP / DGRAD
  nt8_pair, stem_fprop_pair
};
const char* family_name(Family f);

struct Plan {
  GP gp;
  Family family;  // the kernel family that runs (resolve_family, vlfb_conv_plan.hip)
  bool ident, packw;
  int bm, bn;     // tile of that family (NT: m x n; TN: p x q)
  int splits;
  int pre;        // NT: prefetch residual / mask rows before the k-loop (thin-K, epilogue-bound launches)
  int threads;    // workgroup size (NT: 256 or 512)
  int ut;         // NT: taps span whole k-tiles (and DGRAD has unit stride): scalar tap cursor
  int nt8_mode;   // nt8 / nt8_pair: 0 plain rows, 1 gathered FPROP, 2 gathered unit-stride DGRAD
  int nts_mode;   // nt_stream: as nt8_mode
  int sp;         // split-bf16 math (vlfb_gemm_split.hip): bf16 terms per operand (2 | 3), 0 = native MFMA of the dtype
  int sp_kind;    //   NT: 0 plain rows, 1 gathered FPROP, 2 gathered DGRAD, 3 packed stem
  int bias_fused; // WGRAD with desc.wgrad_bias: the launch itself produces the column sums of P (gemm_tn_tr_kernel)
  int w2i;        // VLFB_MATH_F16W2: unit-stride 16-bit DGRAD, two-term weights interleaved per 64-channel k-tile (gemm_nt_kernel<.., W2I>)
  dim3 grid;
  size_t lds;
  long long ws_elems;
};

// Plans are pure functions of the descriptor: cached per thread, keyed by the descriptor bytes.
int cached_plan(const vlfb_conv_desc* d, Plan* out);

// What the operands of one call change about the plan of its descriptor -- and nothing else does:
//   * a 16-bit launch with a two-term residual / output (R_lo / O_lo) runs the tiled kernel, whose epilogue carries them,
//     where the plan is a direct / streaming / skinny family: the plan of the same descriptor with algo = TILE128;
//   * the direct stem FPROP (either form) has no residual / mask epilogue: with R or Mask the tiled kernel runs;
//   * without R and Mask there are no rows to prefetch (Plan::pre).
int resolve_for_operands(const vlfb_conv_desc* d, Plan* pl, bool has_R, bool has_Mask, bool has_R_lo, bool has_O_lo);

}  // namespace vlfb
