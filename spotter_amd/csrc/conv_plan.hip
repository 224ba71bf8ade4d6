// The conv / linear planner (conv_plan.h): sp_conv2d's argument checks, the tile choice as one pure function
// (plan_conv), the launch switch, and the per-thread test / tuning overrides. Host code only: no kernel lives
// here, and nothing below the launch switch makes a HIP call.
#include "conv_plan.h"
#include "tile_table.h"

namespace sp {

namespace {

constexpr int BK = 32;
// Split-K target for long-K GEMMs on mid-size grids (bs1 /detect path: the CCFM 3×3 at M = 6400 ran
// 300 workgroups × 108 k-tiles; split 2 takes it from 213 to 143 µs).
#ifndef SP_SPLITK_BLOCKS
#define SP_SPLITK_BLOCKS 1024
#endif

thread_local ConvOverrides g_overrides;
thread_local PlanBatch g_plan_batch;

// BM × BN of the register-staged tiles 1-6 (conv_mfma16.hip launch_mfma16); 0 runs 4
constexpr int kRegTile[7][2] = {{64, 64}, {128, 128}, {256, 128}, {64, 128}, {64, 64}, {128, 256}, {128, 64}};

// tiles of the grid the launch runs (M rows: the grid limit, the counters' length) ...
int64_t tiles_of(const ConvArgs& a, int bm, int bn) { return ((a.M + bm - 1) / bm) * ((a.d.Cout + bn - 1) / bn); }
// ... and of the rows the choice is made for (Mp: every fill threshold of the by-shape rules)
int64_t plan_tiles_of(const ConvArgs& a, int bm, int bn) { return ((a.Mp + bm - 1) / bm) * ((a.d.Cout + bn - 1) / bn); }

// The split-K factor a GEMM of `rows` rows asks for, before the descriptor's conditions and the cap
// (measured at bs1, profiles/r1/bs1_detail_*.json): short grids split to ~512 workgroups with >= 8 k-tiles
// each; tiny-M linears (< 64 tiles) split even at K = 256; grids of up to SP_SPLITK_BLOCKS tiles split only
// when each workgroup would walk >= 64 k-tiles.
int split_for(int64_t rows, int cout, int nk, const ConvOverrides& o) {
  const int64_t blocks64 = ((rows + 63) / 64) * ((cout + 63) / 64);
  int sp = 1;
  if (nk < o.splitk_min_nk) sp = 1;
  else if (blocks64 < 64 && nk >= 8 && nk < 16) sp = nk / 4;
  else if (blocks64 < 256 && nk >= 16) sp = (int)((512 + blocks64 - 1) / blocks64), sp = sp < nk / 8 ? sp : nk / 8;
  else if (blocks64 < SP_SPLITK_BLOCKS && nk >= 64) sp = (int)((SP_SPLITK_BLOCKS + blocks64 - 1) / blocks64);
  return sp;
}

// A split-K launch of `tiles` output tiles combines in the launch: the descriptor's counter array has one
// entry per tile, and the partial slabs are addressable by 32-bit buffer offsets (at most 16 splits); else the
// separate reduce launch.
bool counters_ok(const ConvArgs& a, int64_t tiles) {
  return a.splits > 1 && a.splits <= 16 && a.d.splitk_counters && tiles <= a.d.splitk_counters_len &&
         (int64_t)a.splits * a.M * a.ldp * 4 < (int64_t(1) << 31);
}

// A bf16 / split tile id as forced or tabled: id, 100+id (slab epilogue requested: req 2) or 200+id (its
// direct-store form: req 4); anything from 300 up is no id.
void decode_cfg(int cfg, int* id, int* req) {
  *id = cfg;
  *req = 1;
  if (cfg >= 300) *id = -1;
  else if (cfg >= 200) *id -= 200, *req = 4;
  else if (cfg >= 100) *id -= 100, *req = 2;
}

// LDS-DMA tile t with epilogue request req → the instance compiled for it (callers with bf16 A rows pass
// tiles with a bf16-A form only: t.fit1a).
int plan_glds_tile(const ConvArgs& a, int planes, const GldsTile& t, int req, ConvPlan* p) {
  const sp_conv_desc& d = a.d;
  if (d.Cin % t.BK || a.K % t.BK) {
    set_error("sp_conv2d: LDS-DMA kernel needs Cin %% %d == 0 (Cin=%d)", t.BK, d.Cin);
    return -1;
  }
  const int64_t tiles = tiles_of(a, t.BM, t.BN) * a.batch;
  if (tiles > 0x7fffffff || (a.batch > 1 && a.splits > 1)) {
    set_error("sp_conv2d: %lld tiles exceed the grid (or split-K on a batched GEMM)", (long long)tiles);
    return -1;
  }
  const bool a16 = a.A16 != nullptr;
  if ((planes == 3 && !t.fit3) || (planes == 2 && (a16 || !t.fit2)) ||
      (planes < 2 && !(a16 ? t.fit1a : t.fit1))) {
    set_error("sp_conv2d: tile configuration not built for %d operand plane(s)%s (LDS or bf16-A variant)", planes,
              a16 ? " with bf16 A planes" : "");
    return -1;
  }
  // the slab epilogues: fp32 rows (2: res1 fp32 or none) or bf16 rows (3: C_bf16, res1_bf16 or none, no res2);
  // float4 epilogue, no split-K / row_scale
  int epv = 1;
  if (req >= 2) {
    const bool base = a.vec_epi && a.splits == 1 && !d.row_scale;
    const bool f32ok = base && !d.C_bf16 && !d.res1_bf16 && !d.res2_bf16;
    const bool bf16ok = base && d.C_bf16 && !d.res1 && !d.res2 && !d.res2_bf16 &&
                        (!d.res1_bf16 || ((reinterpret_cast<uintptr_t>(d.res1_bf16) & 15) == 0 && d.ldr1 % 8 == 0));
    // variant 4 (direct stores) on request, where its extra conditions hold; else variant 2
    const bool f32dd = f32ok && !d.res2 && d.out_rows_per_group <= 0 &&
                       ((a.M - 1) * d.ldc + d.Cout) * 4 < (int64_t(1) << 31) - 4;
    epv = (req == 4 && f32dd) ? 4 : f32ok ? 2 : bf16ok ? 3 : 1;
  }
  p->family = SP_CONV_GLDS;
  p->tile = t.id;
  p->generic = 0;
  p->a_bf16 = a16;
  p->fast_1x1 = t1_ok(a);
  // the instances compiled: variants 2 / 4 for split operands (two or three planes) on the 1×1 fast path, 3 for
  // bf16 A rows; every other combination runs the plain epilogue
  if (a16) p->epilogue = epv == 3 ? 3 : 1;
  else p->epilogue = (planes >= 2 && p->fast_1x1 && (epv == 2 || epv == 4)) ? epv : 1;
  p->counters = 0;
  return 0;
}

}  // namespace

const ConvOverrides& conv_overrides() { return g_overrides; }
const PlanBatch& plan_batch() { return g_plan_batch; }

int plan_rows(const char* what, int64_t rows, int64_t* out) {
  const PlanBatch& b = g_plan_batch;
  *out = rows;
  if (b.batch <= 0) return 0;
  SP_ARG_CHECK(rows % b.batch == 0, "%s: %lld rows are no multiple of the batch %d of sp_set_plan_batch", what,
               (long long)rows, b.batch);
  *out = rows / b.batch * b.plan;
  return 0;
}

int conv_args(const sp_conv_desc* d, const ConvOverrides& o, ConvArgs* out, int* out_planes) {
  SP_ARG_CHECK(d != nullptr, "sp_conv2d: null descriptor");
  SP_ARG_CHECK((d->A || d->A_bf16) && d->Wt && (d->C || d->C_bf16), "sp_conv2d: null A/W/C");
  SP_ARG_CHECK(!(d->res1 && d->res1_bf16) && !(d->res2 && d->res2_bf16) &&
                   !(d->ln_gamma && (d->C_bf16 || d->res1_bf16 || d->res2_bf16)),
               "sp_conv2d: res1 and res1_bf16 together, or bf16 rows with the fused LayerNorm");
  SP_ARG_CHECK(d->N > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0,
               "sp_conv2d: bad shape N=%d H=%d W=%d Cin=%d Cout=%d", d->N, d->H, d->W, d->Cin,
               d->Cout);
  SP_ARG_CHECK(d->KH > 0 && d->KW > 0 && d->stride > 0 && d->pad >= 0, "sp_conv2d: bad kernel");
  const int ho = (d->H + 2 * d->pad - d->KH) / d->stride + 1;
  const int wo = (d->W + 2 * d->pad - d->KW) / d->stride + 1;
  SP_ARG_CHECK(ho == d->Ho && wo == d->Wo, "sp_conv2d: Ho/Wo %dx%d != expected %dx%d", d->Ho,
               d->Wo, ho, wo);
  SP_ARG_CHECK(d->lda >= d->Cin, "sp_conv2d: lda %lld < Cin %d", (long long)d->lda, d->Cin);
  SP_ARG_CHECK(d->act >= 0 && d->act <= 3, "sp_conv2d: bad act %d", d->act);
  SP_ARG_CHECK(!d->row_scale || d->row_period > 0, "sp_conv2d: row_period");
  SP_ARG_CHECK(d->precision == SP_PREC_FP32 || d->precision == SP_PREC_BF16 ||
                   d->precision == SP_PREC_F32X3 || d->precision == SP_PREC_F32X2,
               "sp_conv2d: precision %d", d->precision);
  const int planes = d->precision == SP_PREC_BF16    ? 1
                     : d->precision == SP_PREC_F32X3 ? 3
                     : d->precision == SP_PREC_F32X2 ? 2
                                                     : 0;
  SP_ARG_CHECK(!(d->C_bf16 || d->res1_bf16 || d->res2_bf16) || planes == 1,
               "sp_conv2d: bf16 output / residual rows need the bf16 operand mode (SP_PREC_BF16)");
  SP_ARG_CHECK(planes == 0 || d->Wt_bf16, "sp_conv2d: bf16 / split precision needs Wt_bf16");
  const int64_t K = (int64_t)d->KH * d->KW * d->Cin;
  SP_ARG_CHECK(planes < 2 || d->wt_plane_stride >= (int64_t)d->Cout * K,
               "sp_conv2d: wt_plane_stride %lld < Cout*K", (long long)d->wt_plane_stride);
  auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  if (d->A_bf16) {
    SP_ARG_CHECK(planes == 1 && !d->A2 && !d->ln_gamma && d->Cin % BK == 0 && d->lda % 8 == 0 && al16(d->A_bf16),
                 "sp_conv2d: bf16 A rows need the bf16 operand mode, Cin %% 32 == 0, lda %% 8 == 0, 16-byte "
                 "alignment, no A2 / LayerNorm");
  }
  ConvArgs& a = *out;  // freshly constructed by the caller
  a.d = *d;
  a.A16 = d->A_bf16;
  a.M = (int64_t)d->N * ho * wo;
  if (plan_rows("sp_conv2d", a.M, &a.Mp)) return -1;
  a.K = (int32_t)K;
  a.HoWo = ho * wo;
  // fast operand path: every 32-deep k-tile lies in one filter tap, and the rows loaded as
  // float4 / 8 x bf16 are 16-byte aligned.
  a.fast = (d->Cin % BK == 0) ? 1 : 0;
  if (a.fast) {
    bool al = d->A_bf16 || ((d->lda % 4 == 0) && al16(d->A) && (!d->A2 || ((d->lda2 % 4 == 0) && al16(d->A2))));
    al = al && (planes ? (al16(d->Wt_bf16) && (planes == 1 || d->wt_plane_stride % 8 == 0)) : al16(d->Wt));
    if (!al) a.fast = 0;
  }
  {
    auto al8 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 7) == 0; };
    bool v = (d->ldc % 4 == 0) && (d->C_bf16 ? al8(d->C_bf16) : al16(d->C)) && (d->Cout % 4 == 0);
    v = v && (!d->res1 || (d->ldr1 % 4 == 0 && al16(d->res1)));
    v = v && (!d->res1_bf16 || (d->ldr1 % 4 == 0 && al8(d->res1_bf16)));
    v = v && (!d->res2_bf16 || (d->ldr2 % 4 == 0 && al8(d->res2_bf16)));
    v = v && (!d->res2 || (d->ldr2 % 4 == 0 && al16(d->res2)));
    v = v && (!d->scale || al16(d->scale)) && (!d->shift || al16(d->shift));
    v = v && (d->out_rows_per_group == 0 || d->out_group_stride % 4 == 0);
    a.vec_epi = v ? 1 : 0;
  }
  // Split-K when the output tile grid cannot fill the chip (small batches: the /detect bs1
  // path) and the K loop is long: partial sums go to the caller's workspace.
  a.splits = 1;
  a.ldp = (d->Cout + 3) & ~3;
  a.partial = d->workspace;
  {
    const int nk = (a.K + BK - 1) / BK;
    int sp = split_for(a.Mp, d->Cout, nk, o);
    // split-K runs on the register-staged tiles (fp32 A) and reduces through the fp32-row epilogue
    if (d->workspace && sp > 1 && !d->A_bf16 && !d->C_bf16 && !d->res1_bf16 && !d->res2_bf16) {
      if (sp > o.splitk_max) sp = o.splitk_max;
      // a workspace too short for sp slabs of the planned rows lowers the factor ...
      while (sp > 1 && (int64_t)sp * a.Mp * a.ldp > d->workspace_elems) --sp;
      // ... but under sp_set_plan_batch never one too short for the rows of this launch: that would make the
      // factor, and with it the order of the sum, depend on the batch
      SP_ARG_CHECK(g_plan_batch.batch <= 0 || sp == 1 || (int64_t)sp * a.M * a.ldp <= d->workspace_elems,
                   "sp_conv2d: workspace %lld < %lld elements (the %d-way split-K planned for %lld rows, on %lld rows; "
                   "sp_set_plan_batch does not lower the factor)", (long long)d->workspace_elems,
                   (long long)((int64_t)sp * a.M * a.ldp), sp, (long long)a.Mp, (long long)a.M);
      if (sp > 1) a.splits = sp;
      // planned for fewer rows than the launch has, on a grid that would not split: the folded form
      a.fold = sp > 1 && g_plan_batch.fold != 1 &&
               (g_plan_batch.fold == 2 || (a.Mp != a.M && split_for(a.M, d->Cout, nk, o) == 1));
    }
  }
  if (d->ln_gamma) {  // Linear → +residual → LayerNorm in one launch: 32-row tiles holding whole rows
    SP_ARG_CHECK(planes == 0 && d->Cout % 128 == 0 && d->Cout <= 512 && d->act == SP_ACT_NONE && !d->res2 &&
                     d->out_rows_per_group == 0 && d->ln_beta && a.fast,
                 "sp_conv2d: fused LayerNorm needs fp32 weights, Cout %% 128 == 0 <= 512, no act / res2 / "
                 "grouped rows, Cin %% 32 == 0 (Cout=%d)", d->Cout);
    a.splits = 1;
    a.fold = 0;
  }
  *out_planes = planes;
  return 0;
}

int plan_conv(const ConvArgs& a, int planes, const ConvOverrides& o, ConvPlan* p) {
  const sp_conv_desc& d = a.d;
  // the fill thresholds below count the tiles of the planned rows (Mp); grid limits count the launch's own
  const auto tiles = [&](int bm, int bn) { return plan_tiles_of(a, bm, bn); };
  *p = ConvPlan{};
  p->planes = planes;
  p->epilogue = 1;
  p->splits = a.splits;
  if (d.ln_gamma) {
    if (!conv_gemm_has_fused_ln()) {
      set_error("sp_conv2d: the fused LayerNorm epilogue (ln_gamma) is in the diagnostic build only");
      return -1;
    }
    p->family = SP_CONV_FUSED_LN;
    p->tile = 1101 + 10 * (d.Cout / 128);  // 1×4 waves of 32 × 32·TN, TN = Cout / 128: 1111 … 1141
    return 0;
  }
  // tile choice: a test / tuning override, else the measured exact-shape table (tile_table.h), else by shape.
  // The 2-way split (planes 2) has no measurements of its own yet: it takes every choice the 3-way split takes
  // for the same descriptor (the table key, the by-shape rule, the slab epilogue), sp: "split operands".
  const bool sp = planes >= 2;
  int cfg = o.cfg;
  if (cfg < 0 && a.splits == 1) cfg = tile_table_lookup(a.Mp, d.Cout, a.K, d.KH, d.stride, sp ? 3 : planes);
  if (cfg < 0 && a.splits > 1 && planes && o.splitk_cfg >= 0) cfg = o.splitk_cfg;

  if (planes == 0) {  // ---- fp32 MFMA
    p->family = SP_CONV_FP32;
    p->generic = !a.fast;
    if (a.splits > 1) {  // split-K runs the 64×64 tile whatever id is forced; combined in the launch with counters
      p->tile = 110;
      p->counters = counters_ok(a, tiles_of(a, 64, 64));
      return 0;
    }
    switch (cfg) {
      case 110: case 111: case 120: case 121: case 210: case 211: case 220: case 221:
      case 1110: case 1111: case 1120: case 1121:
      case 4110: case 4111: case 4120: case 4121: case 4210: case 4211:
        p->tile = cfg;
        return 0;
      default: break;  // every other integer: by shape
    }
    // By shape (measured on MI355X, tools/conv_bench.py): the kernel is latency-bound, so
    // occupancy beats operand reuse except for long-K, wide-N, tall-M convs.
    // Cout <= 32 (stem): the 4×1 wave grid's 128×32 tile, no idle N half (1.69× on the stem 3×3,
    // 1.23× on the Cin = 3 stem conv; profiles/r1/conv_bench_thin_fp32.jsonl).
    if (d.Cout <= 32) p->tile = 4110;
    else if (d.Cout <= 64 && a.Mp >= 500000 && a.K >= 288) p->tile = 210;
    else if (a.K >= 3000 && d.Cout >= 384 && a.Mp >= 100000) p->tile = 220;
    else if (a.K <= 128 || d.Cout <= 64 || tiles(64, 64) < 3000) p->tile = 110;
    else p->tile = 120;
    return 0;
  }

  // ---- bf16 / split operands. The id decoded once; t: its LDS-DMA tile, if it is one.
  int id, req;
  decode_cfg(cfg, &id, &req);
  const GldsTile* t = glds_tile(id);
  // two planes: an LDS-DMA tile outside kGldsX2Ids, or a retired id (21-32, 70-75: refused below for one and
  // three planes), is no id: it falls back by shape, where every tile the rule names is in the set
  if (planes == 2 && ((t && !t->a16_only && !t->fit2) || (req == 1 && id >= 21 && id <= 32) ||
                      (req == 1 && id >= 70 && id <= 75))) {
    id = -1;
    req = 1;
    t = nullptr;
  }

  if (a.A16) {  // bf16 A rows: the LDS-DMA tiles with a bf16-A form only
    // bf16 output rows (the bf16 variant's maps) request the slab epilogue (variant 3: res1 by LDS-DMA, rounded
    // outputs staged as bf16 quads), bit-identical, 1.0-2.1x on every tile measured
    // (profiles/r3/bf16/ab_slab_epilogue_bf16_rows.jsonl); plan_glds_tile falls back where it does not apply
    const int ep = d.C_bf16 ? 2 : 1;
    if (req == 1) req = ep;
    if (!(t && t->fit1a)) {
      // a forced / tabled id without a bf16-A form (or no id) falls to this by-shape rule
      if (d.Cout <= 64) id = tiles(128, 64) >= 192 ? 16 : 14;
      // 3×3s on bf16 rows: 256×128 on 16x16x32 MFMAs beat 256×256 by 1.2-1.3× (profiles/r4/bf16/)
      else if (d.KH == 3 && d.Cout % 128 == 0 && tiles(256, 128) >= 192) id = 41;
      else if (d.Cout % 256 == 0 && a.K >= 512 && tiles(256, 256) >= 192) id = 33;
      else if (d.Cout % 128 == 0 && tiles(128, 128) >= 192) id = planes == 3 ? 46 : 45;
      else if (tiles(256, 128) >= 192) id = 12;
      else if (tiles(64, 128) >= 192) id = 13;
      else id = 14;
      t = glds_tile(id);
      req = ep;
      if (!(t && t->fit1a)) {
        set_error("sp_conv2d: no LDS-DMA tile for bf16 A planes");
        return -1;
      }
    }
    return plan_glds_tile(a, planes, *t, req, p);
  }

  p->family = SP_CONV_MFMA16;
  if (!a.fast) {  // generic gather: one small-tile instance per operand mode, whatever id is forced
    p->tile = 4;
    p->generic = 1;
    return 0;
  }

  const bool a2 = d.A2 != nullptr;
  const bool reg_id = req == 1 && id >= 0 && id <= 6;  // a register-staged tile (0 runs 4)
  bool by_shape = false;
  if (a2) {
    // only the register-staged tiles take A2: every other forced id (any id >= 11) falls back by shape
    by_shape = !reg_id;
  } else if (req == 1 && ((id >= 21 && id <= 26) || (id >= 31 && id <= 32) || (id >= 70 && id <= 75))) {
    // retired ids: the conv_pipe / conv_pp / conv_x3s / conv_x3p kernels are gone (DESIGN.md "Retired GEMM
    // kernel families"). The refusal keeps the words it had while they were a diagnostic build:
    // tests/golden/conv_plan.jsonl.gz pins the text.
    set_error("sp_conv2d: tile configuration %d (%s) is in the diagnostic build only", cfg,
              id >= 70 ? "conv_x3s / conv_x3p" : "conv_pipe / conv_pp");
    return -1;
  } else if (t && !t->a16_only) {
    // an LDS-DMA tile. (52-56 are honoured with bf16 A rows only: with fp32 A they fall back by shape below.)
  } else if (req > 1 && id >= 11 && id <= 65) {
    // 100+id / 200+id of an id in the LDS-DMA range that is no usable LDS-DMA tile (121, 152-156, 221, ...)
    // runs the register-staged 64×64 tile: kept from the dispatcher this planner replaced
    id = 4;
    t = nullptr;
  } else if (!reg_id) {
    by_shape = true;  // no id (-1), or an integer that names no tile
  }

  if (by_shape) {
    // By shape (tools/conv_bench.py sweeps): the LDS-DMA kernel whenever the operands allow it,
    // the largest tile that still gives >= 192 workgroups, a 64-wide N tile for Cout <= 64;
    // 256×256 where Cout is a multiple of 256 and K >= 512 (+10-16 % there; a 384-wide N wastes
    // half of its second column of tiles, and at K = 256 the 256×128 tile stays ahead).
    const bool dma = !a2;
    // f32x3, measured (profiles/r1/conv_sweep_2wg_x3.jsonl): short-K wide-N layers (the K = 128 / 256
    // bottleneck expands, the decoder value projection) and 384 / 128-wide outputs on mid-size grids
    // run best with two workgroups per CU (LDS <= 80 KB), where one workgroup's prologue and residual
    // epilogue overlap the other's MFMAs: 1.32× on the stage-3 expand, 1.10× on the CCFM 3×3 @ 40².
    const bool x3 = sp;
    if (a.splits > 1) id = 4;
    else if (dma && x3 && a.K <= 256 && d.Cout >= 512 && tiles(128, 128) >= 192) id = 46;
    else if (dma && x3 && d.Cout % 128 == 0 && d.Cout % 256 != 0 && a.Mp >= 40000 &&
             (a.Mp < 150000 || d.Cout == 128) && tiles(128, 128) >= 192) id = 45;
    else if (d.Cout <= 64)
      id = dma ? (x3 && d.Cout == 64 && tiles(256, 64) >= 192 ? 51 : (tiles(128, 64) >= 192 ? 16 : 14)) : 4;
    else if (dma && d.Cout % 256 == 0 && a.K >= 512 && tiles(256, 256) >= 192) id = 33;
    else if (tiles(256, 128) >= 192) id = dma ? (a.Mp >= 150000 ? 41 : 12) : 2;  // tall M: 16x16x32 +6 %
    else if (tiles(64, 128) >= 192) id = dma ? 13 : 3;
    else id = dma ? 14 : 4;
    req = 1;
    t = id >= 11 ? glds_tile(id) : nullptr;
  }

  if (t) {
    // The slab epilogue on the split mode's launches with a BN affine or a residual, for the tiles where it
    // measured faster (kGldsSlabIds), whether the id was forced, tabled or chosen by shape
    if (req == 1 && t->slab && sp && (d.res1 || d.scale || d.shift) && !d.row_scale && a.vec_epi &&
        a.splits == 1 && !d.C_bf16)
      req = o.glds_epv == 4 ? 4 : 2;
    return plan_glds_tile(a, planes, *t, req, p);
  }
  const int r = (id >= 1 && id <= 6) ? id : 4;
  const int64_t nt = tiles_of(a, kRegTile[r][0], kRegTile[r][1]);
  if (nt > 0x7fffffff) {
    set_error("sp_conv2d: %lld tiles exceed the grid", (long long)nt);
    return -1;
  }
  p->tile = r;
  p->counters = counters_ok(a, nt);
  return 0;
}

int plan_glds(const ConvArgs& a, int planes, int cfg, const char* what, ConvPlan* p) {
  int id, req;
  decode_cfg(cfg, &id, &req);
  const GldsTile* t = glds_tile(id);
  if (!t || a.d.A2) {
    set_error("%s: tile configuration %d is not an LDS-DMA configuration", what, cfg);
    return -1;
  }
  *p = ConvPlan{};
  p->planes = planes;
  p->splits = a.splits;
  return plan_glds_tile(a, planes, *t, req, p);
}

int launch_plan(const ConvArgs& a, const ConvPlan& p, hipStream_t s) {
  switch (p.family) {
    case SP_CONV_FP32:
    case SP_CONV_FUSED_LN: return launch_fp32(a, p, s);
    case SP_CONV_GLDS: return launch_glds(a, p, s);
    default: return launch_mfma16(a, p, s);  // register-staged; it refuses any other family
  }
}

}  // namespace sp

extern "C" int sp_conv2d(const sp_conv_desc* d, void* stream) {
  sp::ConvArgs a;
  sp::ConvPlan p;
  int planes;
  if (sp::conv_args(d, sp::g_overrides, &a, &planes) || sp::plan_conv(a, planes, sp::g_overrides, &p)) return -1;
  return sp::launch_plan(a, p, sp::as_stream(stream));
}

extern "C" int sp_conv_plan(const sp_conv_desc* d, sp_conv_plan_info* out) {
  SP_ARG_CHECK(out != nullptr, "sp_conv_plan: null out");
  sp::ConvArgs a;
  int planes;
  if (sp::conv_args(d, sp::g_overrides, &a, &planes)) return -1;
  return sp::plan_conv(a, planes, sp::g_overrides, out);
}

// Tile override for tests and tuning tools, set explicitly per thread (never from the environment): an id of
// conv_plan.h's table; -1 = by shape (the production choice).
extern "C" int sp_set_conv_config(int cfg) {
  sp::g_overrides.cfg = cfg < 0 ? -1 : cfg;
  return 0;
}

// bs1 tuning hooks: the tile of split-K launches, the split-factor cap and the fewest k-tiles that split
extern "C" int sp_set_splitk_config(int cfg, int max_splits, int min_ktiles) {
  sp::g_overrides.splitk_cfg = cfg < 0 ? -1 : cfg;
  sp::g_overrides.splitk_max = max_splits < 1 ? 16 : (max_splits > 16 ? 16 : max_splits);
  sp::g_overrides.splitk_min_nk = min_ktiles < 1 ? 8 : min_ktiles;
  return 0;
}

extern "C" int sp_set_tuning(int knob, int value) {
  switch (knob) {
    case SP_TUNE_GLDS_EPILOGUE:
      sp::g_overrides.glds_epv = value == 4 ? 4 : -1;
      return 0;
    case SP_TUNE_FOLD:
      sp::g_plan_batch.fold = value == 1 || value == 2 ? value : 0;
      return 0;
    case SP_TUNE_MSDA_GENERIC:
      sp::set_msda_generic(value == 1 ? 1 : 0);
      return 0;
    default:
      sp::set_error("sp_set_tuning: unknown knob %d", knob);
      return -1;
  }
}

// Batch-invariant planning (product path; per thread like the overrides above): while batch > 0, every launch
// of `batch` images is planned as one of `plan_batch` images. (0, 0) restores planning from the launch's own rows.
extern "C" int sp_set_plan_batch(int batch, int plan_batch) {
  if (batch == 0 && plan_batch == 0) {
    sp::g_plan_batch.batch = sp::g_plan_batch.plan = 0;
    return 0;
  }
  SP_ARG_CHECK(batch >= 1 && plan_batch >= 1, "sp_set_plan_batch: batch %d, plan_batch %d (both >= 1, or 0, 0)", batch,
               plan_batch);
  sp::g_plan_batch.batch = batch;
  sp::g_plan_batch.plan = plan_batch;
  return 0;
}
