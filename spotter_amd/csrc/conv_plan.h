// The conv / linear dispatch: which kernel instantiation a descriptor runs (ConvPlan), chosen by one pure
// function (plan_conv, conv_plan.hip) and launched by a switch on the plan (launch_plan). sp_conv_plan
// (spotter_hip.h) exports the choice, so it can be read and tested without a GPU.
//
// Tile configuration ids (sp_set_conv_config, sp_set_splitk_config, tile_table.h, tools/tune_*.py):
//
//   id                  family                       meaning
//   -1                  -                            by shape (the product default)
//   <TM><TN><DB>        fp32 GEMM (planes 0 only)    2×2 waves of (32·TM)×(32·TN), DB = double-buffered LDS:
//                                                    110 111 120 121 210 211 220 221
//   1<TM><TN><DB>       fp32 GEMM                    1×4 wave grid, tile 32 × (128·TN): 1110 1111 1120 1121
//   4<TM><TN><DB>       fp32 GEMM                    4×1 wave grid, tile (128·TM) × (32·TN):
//                                                    4110 4111 4120 4121 4210 4211
//   1-6                 register-staged mfma16       1 = 128×128, 2 = 256×128, 3 = 64×128, 4 = 64×64, 5 = 128×256,
//                                                    6 = 128×64 (the only family that takes A2; 0 runs 4)
//   11-20 33-38 41-56   LDS-DMA (SP_GLDS_CONFIGS)    see the list below; 52-56 with bf16 A rows only
//   62-65
//   100+id              LDS-DMA                      the same tile with the slab epilogue requested (variant 2,
//                                                    or 3 on bf16 rows), where its conditions hold
//   200+id              LDS-DMA                      ... its direct-store form (variant 4) requested
//   21-26 31-32 70-75   retired                      the conv_pipe / conv_pp / conv_x3s / conv_x3p kernels, removed
//                                                    (DESIGN.md "Retired GEMM kernel families"): an error, or
//                                                    the by-shape rule where plan_conv says so; not reused
//
// With bf16 / split operands (planes 1 / 2 / 3) a forced id is read as id, 100+id or 200+id only, so the fp32
// digit codes mean something else there (220 = 200+20); with fp32 operands only the eighteen digit codes are
// ids. An id that cannot apply falls back to the by-shape rule (plan_conv says where); with the 2-way split
// (planes 2) that includes every LDS-DMA id outside kGldsX2Ids.
#pragma once

#include "conv_common.h"

namespace sp {

// The instantiation a conv / linear launch runs: sp_conv_plan_info (spotter_hip.h) field for field.
typedef sp_conv_plan_info ConvPlan;

// The calling thread's test / tuning overrides (sp_set_conv_config, sp_set_splitk_config, sp_set_tuning
// SP_TUNE_GLDS_EPILOGUE), set explicitly per thread and never from the environment.
struct ConvOverrides {
  int cfg = -1;           // forced tile id; -1 = by shape (the production choice)
  int splitk_cfg = -1;    // bs1 tuning: the tile of split-K launches (bf16 / split operands)
  int splitk_max = 16;    // ... the split-factor cap
  int splitk_min_nk = 8;  // ... the fewest k-tiles that split
  int glds_epv = -1;      // the split mode's slab-epilogue form: 4 = direct stores, else the slab store pass
};
const ConvOverrides& conv_overrides();

// sp_set_plan_batch (spotter_hip.h) of the calling thread: while batch > 0, launches of `batch` images are planned
// as launches of `plan` images. fold (sp_set_tuning SP_TUNE_FOLD, tests and A/B only): 0 = the rule (conv_args),
// 1 = never the folded split-K form, 2 = every split that the register-staged 64×64 tile runs.
struct PlanBatch {
  int batch = 0, plan = 0, fold = 0;
};
const PlanBatch& plan_batch();
// The rows a launch of `rows` rows is planned as: rows, or rows · plan / batch under sp_set_plan_batch (rows that
// are no multiple of the batch: -1 with the error set). The one place every size-dependent choice of the conv /
// linear planner and of the Winograd stages takes its row count from.
int plan_rows(const char* what, int64_t rows, int64_t* out);

// sp_conv2d's argument checks and the derived launch arguments (M, K, fast, vec_epi, split-K factor):
// 0, or -1 with the error set. `planes`: 0 fp32, 1 bf16, 2 the 2-way split, 3 the 3-way split.
int conv_args(const sp_conv_desc* d, const ConvOverrides& o, ConvArgs* a, int* planes);
// The planner: a pure function of its arguments (no HIP call; of the descriptor's pointers it reads only
// nullness and alignment). 0, or -1 with the error set.
int plan_conv(const ConvArgs& a, int planes, const ConvOverrides& o, ConvPlan* p);
// The LDS-DMA part of it for one tile (`cfg`: id, 100+id or 200+id), shared with the batched Winograd GEMMs
// (winograd.hip), which choose their tile by their own measured rule. `what` prefixes the not-a-tile error.
int plan_glds(const ConvArgs& a, int planes, int cfg, const char* what, ConvPlan* p);
// Launches the plan (and the split-K reduce where the plan asks for it).
int launch_plan(const ConvArgs& a, const ConvPlan& p, hipStream_t s);
// The per-family launchers launch_plan switches over (conv_gemm.hip, conv_mfma16.hip, conv_glds.hip).
int launch_fp32(const ConvArgs& a, const ConvPlan& p, hipStream_t s);
int launch_mfma16(const ConvArgs& a, const ConvPlan& p, hipStream_t s);
int launch_glds(const ConvArgs& a, const ConvPlan& p, hipStream_t s);

// LDS layout of one LDS-DMA tile (conv_glds.h); SMEM (16-byte units) decides which operand modes fit.
template <int WM, int WN, int TM, int TN, int PL, int NS, int BK, int APL = 0>
struct GldsCfg {
  // (64-deep stages were built and measured at 0.70-0.92x of the same wave tile at k32 for both operand
  // modes, profiles/r3/bf16/ab_bk64_*.jsonl: the larger stages cost workgroups per CU; removed in round 4)
  static_assert(BK == 32 || BK == 16, "k per stage");
  static constexpr int NT = 64 * WM * WN;
  static constexpr int BM = 32 * TM * WM;
  static constexpr int BN = 32 * TN * WN;
  // APL: A in memory — 0: fp32 A, split / rounded per fragment; 1: bf16 rows (ConvArgs::A16, bf16 mode)
  static_assert(APL == 0 || APL == PL, "bf16 A planes match the operand mode");
  static constexpr int RA = APL ? BK / 8 : BK / 4;  // 16-byte chunks per A row of one plane
  static constexpr int RB = BK / 8;  // 16-byte chunks per bf16 B row (4 / 2)
  static constexpr int CAP = BM * RA;  // 16-byte chunks of one A plane
  static constexpr int CA = CAP * (APL ? APL : 1);  // ... of the whole A stage
  static constexpr int CB = BN * RB;  // 16-byte chunks of one bf16 B plane
  static constexpr int GAP = CAP / NT;  // DMA pieces per thread per A plane
  static constexpr int GA = CA / NT;
  static constexpr int GB = CB / NT;
  static_assert(GAP * NT == CAP && GB * NT == CB && GB >= 1 && GAP >= 1, "DMA pieces must tile the workgroup");
  static constexpr int GLDS = GA + PL * GB;  // DMA instructions per thread per stage
  static constexpr int STAGE = CA + PL * CB;
  static constexpr int NB = (WM * WN * TM * 32 * TN * 32 / 4 <= NS * STAGE) ? TM : 1;
  static constexpr int EPI = WM * WN * NB * 32 * TN * 32 / 4;
  static constexpr int SMEM = NS * STAGE > EPI ? NS * STAGE : EPI;
  static_assert(NS >= 2 && NS <= 6, "stages");
};

// The LDS-DMA tile configurations: (id, WM, WN, TM, TN, NS, BK, M16, OCC, AB). Tile BM × BN = 32·TM·WM ×
// 32·TN·WN, WM × WN waves, NS stages of BK-deep k, M16: v_mfma_f32_16x16x32_bf16 blocks, OCC: the
// register budget of the 1×1 fast path (waves per SIMD), AB: bf16-A-plane variants compiled.
#define SP_GLDS_CONFIGS(X)              \
  X(11, 2, 2, 2, 2, 3, 32, false, 1, false)    \
  X(12, 4, 2, 2, 2, 2, 32, false, 1, true)    \
  X(13, 2, 2, 1, 2, 3, 32, false, 1, true)    \
  X(14, 2, 2, 1, 1, 3, 32, false, 1, true)    \
  X(15, 2, 4, 2, 2, 2, 32, false, 1, false)    \
  X(16, 2, 2, 2, 1, 3, 32, false, 1, true)    /* 128×64, 3 stages */ \
  X(17, 4, 1, 2, 4, 2, 32, false, 1, false)    /* 256×128, 4 waves of 64×128 */ \
  X(18, 2, 2, 2, 4, 2, 32, false, 1, false)    /* 128×256, 4 waves of 64×128 */ \
  X(19, 2, 1, 2, 4, 2, 32, false, 1, false)    /* 128×128, 2 waves of 64×128, 2 stages */ \
  X(20, 2, 1, 2, 4, 3, 32, false, 1, false)    /* 128×128, 2 waves of 64×128 */ \
  X(33, 4, 2, 2, 4, 2, 32, false, 1, true)    /* 256×256, 8 waves of 64×128 */ \
  X(34, 2, 4, 4, 2, 2, 32, false, 1, false)    /* 256×256, 8 waves of 128×64 */ \
  X(35, 4, 1, 2, 4, 4, 16, false, 1, false)    /* 256×128, k16 × 4 stages */ \
  X(36, 4, 1, 2, 4, 5, 16, false, 1, false)    /* 256×128, k16 × 5 stages */ \
  X(37, 4, 2, 2, 4, 3, 16, false, 1, false)    /* 256×256, k16 × 3 */ \
  X(38, 4, 2, 2, 4, 4, 16, false, 1, false)    /* 256×256, k16 × 4 */ \
  X(41, 4, 2, 2, 2, 2, 32, true, 1, true)     /* cfg 12 on 16x16x32 MFMAs */ \
  X(42, 4, 2, 2, 4, 2, 32, true, 1, true)     /* cfg 33 on 16x16x32 MFMAs */ \
  X(43, 2, 2, 2, 2, 3, 32, true, 1, false)     /* cfg 11 on 16x16x32 MFMAs */ \
  X(44, 4, 1, 2, 4, 2, 16, false, 1, true)    /* 256×128, 4 waves of 64×128, k16 × 2 */ \
  X(45, 2, 2, 2, 2, 2, 32, false, 1, true)    /* 128×128, k32 × 2 */ \
  X(46, 2, 2, 2, 2, 2, 16, false, 4, true)    /* 128×128, k16 × 2, four workgroups per CU (see below) */ \
  X(47, 2, 2, 2, 2, 2, 32, true, 1, true)     /* cfg 45 on 16x16x32 MFMAs */ \
  X(48, 2, 2, 2, 4, 2, 16, false, 1, false)    /* 128×256, 4 waves of 64×128, k16 × 2 */ \
  X(49, 4, 1, 2, 4, 2, 32, true, 1, false)     /* cfg 17 on 16x16x32 MFMAs */ \
  X(50, 4, 1, 2, 2, 3, 32, false, 1, false)    /* 256×64, k32 × 3 */ \
  X(51, 4, 1, 2, 2, 2, 32, false, 1, true)    /* 256×64, k32 × 2 */ \
  X(62, 4, 1, 1, 8, 2, 32, false, 1, false)    /* 128×256, 4 waves of 32×256 */ \
  X(63, 8, 1, 1, 4, 2, 32, false, 1, true)    /* 256×128, 8 waves of 32×128 */ \
  X(64, 4, 1, 1, 4, 3, 32, false, 1, true)    /* 128×128, 4 waves of 32×128, 3 stages */ \
  X(65, 8, 1, 1, 4, 2, 32, true, 1, false)     /* cfg 63 on 16x16x32 MFMAs */ \
  /* round 4, bf16-row candidates (deeper DMA pipelines; x3 stages do not fit at 256 rows) */ \
  X(52, 4, 2, 2, 2, 3, 32, false, 1, true)    /* 256×128, k32 × 3 */ \
  X(53, 4, 2, 2, 2, 3, 32, true, 1, true)     /* cfg 52 on 16x16x32 MFMAs */ \
  X(54, 4, 2, 2, 2, 4, 32, true, 1, true)     /* 256×128, k32 × 4, 16x16x32 */ \
  X(55, 4, 2, 2, 4, 3, 32, true, 1, true)     /* 256×256, k32 × 3, 16x16x32 */ \
  X(56, 2, 2, 2, 2, 4, 32, true, 1, true)     /* 128×128, k32 × 4, 16x16x32 */
// (round 5 also built 256×256 bf16-row tiles with 4 and 5 stages of 32 KB at one workgroup per CU, for the
// long-K 3x3s: 1.1-2.3× slower than the table's tiles on all 35 C3 / C2-bf16 shapes above 0.3 ms per step,
// 0.71 against 0.61 ms even at 102400×512×4608, profiles/r5/bf16/retune_*_256x256.json. Removed.)
// (round 5 built 224-row tiles — 224×256 with four waves of 224×64, its 16x16x32 form, 224×128 with two
// waves — so the 51200-row C2 GEMMs would fill the 256 CUs in one wave of 229 tiles: 1.2-2.3× slower than
// the table's tiles on all ten 51200-row shapes, profiles/r5/x3/tune_224.json; one wave per SIMD and the
// A split repeated by every wave cost more than the full wave of CUs gains. Removed.)
// cfg 46's OCC = 4: registers for 4 waves per SIMD (four workgroups per CU): bit-identical, 1.02-1.09x
// over the unconstrained allocation (3 per SIMD) on the short-K shapes it serves
// (profiles/r3/x3/ab_glds_occupancy.jsonl); 122 VGPRs, no spill, on the 1×1 fast path (the general path
// would spill: it keeps the unconstrained allocation).

// Membership sets of the list above. Slab epilogue (100+id) measured faster on the split mode's launches
// with a BN affine or a residual: 1.02-1.28x on the bottleneck expands (the res1 band fetched by LDS-DMA;
// profiles/r3/x3/ab_residual_dma_epilogue.jsonl), 1.02-1.19x without a residual (the BN constants hoisted per
// lane; ab_slab_epilogue_nores.jsonl), bit-identical either way; 0.59-0.96x on the 256-wide-N / TN = 4
// four-wave tiles (33, 44), which are therefore not in it.
constexpr int kGldsSlabIds[] = {12, 14, 41, 45, 46, 47, 63, 64};
// The round-4 bf16-row candidates: taken as a forced / table id with bf16 A rows only (with fp32 A rows
// sp_conv2d falls back by shape; the Winograd GEMMs take them).
constexpr int kGldsBf16AOnlyIds[] = {52, 53, 54, 55, 56};
// The tiles compiled for the 2-way split (SP_PREC_F32X2, PL = 2): the ids the 3-way split mode reaches — the
// by-shape rule of plan_conv (12 13 14 16 33 41 45 46 51), the Winograd rule (winograd.hip: 14 45 46 47 63) and
// the split-operand entries of tile_table.h (14 33 44 45 46 47 63 64) — so the new mode starts from the split
// mode's tile for every shape without instantiating all of SP_GLDS_CONFIGS a third time. With two planes any
// other forced / tabled id falls back to the by-shape rule, as inapplicable ids do.
constexpr int kGldsX2Ids[] = {12, 13, 14, 16, 33, 41, 44, 45, 46, 47, 51, 63, 64};

struct GldsTile {
  int id, BM, BN, BK;
  bool fit3, fit1, fit1a;  // the stages fit the 160 KB LDS: split operands, bf16 operands, bf16 A rows (AB tiles)
  bool slab, a16_only;     // in kGldsSlabIds / kGldsBf16AOnlyIds
  bool fit2;               // built for the 2-way split: in kGldsX2Ids and its stages fit the LDS
};
template <int N>
constexpr bool id_in(const int (&set)[N], int id) {
  for (int v : set)
    if (v == id) return true;
  return false;
}
template <int WM, int WN, int TM, int TN, int NS, int BK, bool AB>
constexpr bool glds_fit1a() {  // bf16 A rows: the bf16 operand mode only (not instantiated unless AB)
  if constexpr (AB) return GldsCfg<WM, WN, TM, TN, 1, NS, BK, 1>::SMEM * 16 <= 163840;
  else return false;
}
constexpr GldsTile kGldsTiles[] = {
#define SP_GLDS_TILE(id, WM, WN, TM, TN, NS, BK, M16, OCC, AB)                                                   \
  {id, 32 * TM * WM, 32 * TN * WN, BK, GldsCfg<WM, WN, TM, TN, 3, NS, BK>::SMEM * 16 <= 163840,                  \
   GldsCfg<WM, WN, TM, TN, 1, NS, BK>::SMEM * 16 <= 163840, glds_fit1a<WM, WN, TM, TN, NS, BK, AB>(),            \
   id_in(kGldsSlabIds, id), id_in(kGldsBf16AOnlyIds, id),                                                        \
   id_in(kGldsX2Ids, id) && GldsCfg<WM, WN, TM, TN, 2, NS, BK>::SMEM * 16 <= 163840},
    SP_GLDS_CONFIGS(SP_GLDS_TILE)
#undef SP_GLDS_TILE
};
// The LDS-DMA tile `id`, or null ("is an LDS-DMA id").
constexpr const GldsTile* glds_tile(int id) {
  for (const GldsTile& t : kGldsTiles)
    if (t.id == id) return &t;
  return nullptr;
}

// The 1×1 fast path (V = 2) applies: KH = KW = 1, stride 1, no padding (A row m is A + m·lda), and
// every byte offset of a batch member's A and weight plane fits 32 bits.
inline bool t1_ok(const ConvArgs& a) {
  const sp_conv_desc& d = a.d;
  return d.KH == 1 && d.KW == 1 && d.stride == 1 && d.pad == 0 && d.Ho == d.H && d.Wo == d.W &&
         a.M * d.lda * (a.A16 ? 2 : 4) < (int64_t(1) << 32) && (int64_t)d.Cout * a.K * 2 < (int64_t(1) << 32);
}

}  // namespace sp
