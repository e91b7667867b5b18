// What one DiT score call runs: the kernel family and the launch geometry of every layer GEMM, decided by a pure
// function of (configuration, precision, B, T) and the switches.  Host-only -- no HIP -- so that the plan can be read and
// tested without a GPU (dsn_dit_plan, tests/test_dit_plan_host.py).  dsn_ctx::dit_forward (engine.hip) calls dit_plan
// once per score call and then only allocates, fills descriptors from the plan and launches.
#pragma once
#include <algorithm>

#include "../../include/ditsep_hip.h"
#include "switches.h"

using DitPlan = DsnDitPlan;  // (field comments: include/ditsep_hip.h)

// Limits the kernel files own and the plan must stay inside; dit_limits() (engine.hip) fills them from igemm.h /
// kernels.h, where each is named once
struct DitLimits {
  int qa_max_rows;     // qkv_attention_max_rows(): tallest panel of the fused to_qkv + attention kernel
  int qa_shared_rows;  // qkv_attention_panel_rows(1): its short tile, the one in which several items share a panel
  int panel_rows;      // PANEL_ROWS_MAX: tallest row panel
  int panel_fp8_rows;  // PANEL_FP8_ROWS_MAX: tallest fp8 row panel that keeps 16 waves (QKV, FF-out)
  int stats_rows;      // PANEL_STATS_ROWS_MAX: tallest panel of a to_out that writes the LayerNorm statistics
  int slabs;           // RESIDUAL_NORM_MAX_SLABS: split-K slabs the residual_norm kernel reduces
};

inline int prec_planes(int precision) { return precision == DSN_PREC_BF16X3 || precision == DSN_PREC_FP16X3 ? 2 : 1; }
inline bool prec_fp8(int precision) { return precision == DSN_PREC_FP8; }
// ff_norm folded into FF-in (to_out without split-K writes the residual stream and its row statistics): the single-plane
// 16-bit modes, and the fp8 mode.  Decided at finalize, which packs the folded weights.
inline bool dit_fold_ln(const dsn_config& c, const Switches& sw) {
  return prec_planes(c.precision) == 1 && !prec_fp8(c.precision) && c.dit_embed_dim % 64 == 0 && !sw.no_ln_fold;
}
inline bool dit_fold_ln8(const dsn_config& c, const Switches& sw) {
  return prec_fp8(c.precision) && c.dit_embed_dim % 128 == 0 && !sw.no_ln_fold;
}

inline DitPlan dit_plan(const dsn_config& cfg, int B, int T, bool fold_ln, bool fold_ln8, const Switches& sw,
                        const DitLimits& lim) {
  auto cdiv = [](int a, int b) { return (a + b - 1) / b; };
  const int D = cfg.dit_embed_dim, H = cfg.dit_heads, P = prec_planes(cfg.precision);
  const bool fp8 = prec_fp8(cfg.precision);
  DitPlan p = {};
  const int S = p.S = T + 1, M = p.M = B * S;
  // Single mixtures and pairs (up to 80 token rows = 5 sub-tiles; DSN_SKINNY_MAX moves the limit, at most 128): the
  // weight-streaming skinny kernels, split-K over all the slabs for the two N = D GEMMs so that every CU streams a share
  // of their weights.  Measured (scripts/score_time.py, one score call): M = 33: 1.52 ms vs 2.27 ms with the panel
  // kernels; M = 17 (config C1): 1.37 vs 2.02 ms; M = 9: 1.28 vs 2.01 ms; M = 61 (4 sub-tiles): 1.77 vs 2.10 ms; M = 66
  // (5): 1.72 vs 2.07; M = 99 (7): 2.03 vs 2.08; M = 126 (8): 2.22 vs 2.10.  (The window used to start at 33 rows:
  // below it the launcher picked the 1- / 2-sub-tile instantiations, which run 2.5x slower than the 3-sub-tile one on the
  // same data -- see igemm_skinny_launch.)
  const bool skinny = P == 1 && !fp8 && M <= sw.skinny_max && D % 256 == 0;
  p.skinny = skinny;
  const bool use_panel = D % 64 == 0;  // row-panel kernels
  // Folded ff_norm (panels of at most 80 rows that fill whole rounds): to_out runs WITHOUT split-K in 128-column tiles,
  // adds the residual itself and writes x' (fp32), its raw operand plane and per-row statistics; FF-in then applies the
  // LayerNorm algebraically in its epilogue -- the LayerNorm launch between them is gone.  At M = 2112: 32 panels of
  // 66 rows x 8 column tiles = 256 workgroups.
  if ((fold_ln || fold_ln8) && use_panel && !skinny) {
    for (int rounds = 1; rounds <= 4 && !p.fold_rows; ++rounds) {
      const int np = 256 * rounds / std::max(1, cdiv(D, 128));
      if (np >= 1 && cdiv(M, np) <= lim.stats_rows) p.fold_rows = cdiv(M, np);
    }
  }
  // Fused to_qkv + attention (single-plane 16-bit operands, 64-wide heads, panels of whole items up to 144 rows -- 240
  // for one long item, the 2-stage-ring variant): as many items per panel as keep panels x heads at a full round of the
  // chip; small batches (fewer than half a round of workgroups) and the skinny window keep the separate kernels.
  // DSN_QA_IPP forces it with that many items per panel wherever such a panel fits the tallest tile.
  if (P == 1 && !skinny && D == H * 64 && S <= lim.qa_max_rows) {
    int ipp = std::min(B, std::max(1, lim.qa_shared_rows / S));  // several items share a panel only in the short tile
    while (ipp > 1 && cdiv(B, ipp) * H < 256) --ipp;
    if (cdiv(B, ipp) * H >= 128) p.qa_ipp = ipp;
    if (sw.qa_ipp >= 1 && sw.qa_ipp * S <= lim.qa_max_rows) p.qa_ipp = sw.qa_ipp;
  }
  // Short row panels for the three narrower GEMMs in the single-plane modes (the split modes: measured, no gain), sized
  // so that panels x column tiles x split-K is whole balanced rounds of 256 workgroups: at M = 2112 out-proj 16 x 8 x
  // split-K 2 and FF-out 16 x 4 x split-K 4 (136-row panels, 9 sub-tiles) = 256, QKV 21 x 12 (104-row panels, 7
  // sub-tiles) = 252 (sweep: profiles/r01_gemm_sweep_dit_panel132.log).  Also for small batches: many short panels keep
  // every CU streaming weights -- B = 8: 197 -> 145 ms per step.
  const bool short_panel = use_panel && P == 1;
  // panel height for a GEMM with `wg_per_panel` = column tiles x split-K workgroups per row panel: as many panels as fill
  // whole rounds of 256 workgroups, a multiple of 8 rows, at most max_rows tall
  auto panel_rows_for = [&](int wg_per_panel, int max_rows) {
    for (int rounds = 1;; ++rounds) {
      const int np = std::max(1, 256 * rounds / std::max(1, wg_per_panel));
      const int rows = (cdiv(M, np) + 7) / 8 * 8;
      if (rows <= max_rows) return rows;
    }
  };
  // A residual-stream GEMM (out-proj, FF-out; K = its contraction length) has N = D only: at M ~ 2k rows that is too few
  // 128 x 128 tiles to fill 256 CUs, so it runs split-K into fp32 slabs (the residual_norm that follows reduces them).
  // Skinny: over all the slabs; short panels and fp8: `ks`, in bn-column tiles; the two-plane modes: as many as bring
  // the 128 x 128 tiles to about 400 workgroups, k-slices of at least 8 k-tiles.
  auto stream_gemm = [&](int bn, int ks, int K, int max_rows, int* ksplit, int* rows) {
    const int tiles = cdiv(M, 128) * cdiv(D, 128);
    const int picked = std::max(1, std::min((400 + tiles / 2) / tiles, std::min(lim.slabs, K / 32 / 8)));
    *ksplit = skinny ? lim.slabs : ((short_panel || fp8) ? ks : picked);
    *rows = !skinny && (short_panel || fp8) ? panel_rows_for(cdiv(D, bn) * ks, max_rows) : 0;
  };
  if (p.fold_rows) p.attn_out_ksplit = 1;  // (fold_rows is its panel height)
  else stream_gemm(128, 2, D, lim.panel_rows, &p.attn_out_ksplit, &p.attn_out_rows);
  stream_gemm(256, 4, 4 * D, fp8 ? lim.panel_fp8_rows : lim.panel_rows, &p.ff_out_ksplit, &p.ff_out_rows);
  if (!skinny) {
    if (!p.qa_ipp && (short_panel || fp8))
      p.qkv_rows = panel_rows_for(cdiv(3 * D, 256), fp8 ? lim.panel_fp8_rows : lim.panel_rows);
    // FF-in in 256-column tiles: short panels as above -- for the benchmark shape (M = 2112 -> 8 panels of 264 rows,
    // N = 8192) exactly 256 workgroups, one round; fp8: up to 17 row sub-tiles (8 waves x 256 registers, branch-free main
    // loop), one round at C2 -- or, in the two-plane modes, ceil(M / 272) equal panels
    if (short_panel || fp8) p.ff_in_rows = panel_rows_for(cdiv(4 * D * 2, 256), lim.panel_rows);
    else if (use_panel) p.ff_in_rows = (cdiv(M, cdiv(M, lim.panel_rows)) + 7) / 8 * 8;
  }
  // project_out: N = n_src * latent_dim is ONE 128-column tile: 128-row tiles leave B*T/128 (17 at C2) workgroups walking
  // the whole K alone; 64-row panels x 8 waves with a 4-stage ring double the workgroups and the loads in flight
  if (use_panel && P == 1 && cfg.n_src * cfg.latent_dim <= 128 && B * T >= 1024) p.project_out_rows = 64;
  return p;
}
