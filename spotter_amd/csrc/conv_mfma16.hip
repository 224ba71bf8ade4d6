// Implicit-GEMM convolution / linear layer on bf16-operand MFMA (v_mfma_f32_32x32x16_bf16,
// fp32 accumulate) for gfx950. Two operand modes share one kernel body:
//
//   PL = 1  bf16: activations rounded RNE to bf16 while staging, weights pre-rounded bf16
//           (sp_precision SP_PREC_BF16, the separately reported bf16 variant);
//   PL = 3  fp32 via a 3-way split (SP_PREC_F32X3): each fp32 operand x = hi + mid + lo with
//           hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid) (both differences are exact
//           in fp32), so the three planes hold all 24 significand bits. Per 16-deep k step the
//           wave issues the six products down to the 2^-17 |a b| scale:
//             lo·hi, hi·lo, mid·mid, mid·hi, hi·mid, hi·hi   (smallest first)
//           With round-to-nearest |mid| <= 2^-8 |x| and |lo| <= 2^-17 |x|, so the dropped mid·lo,
//           lo·mid, lo·lo terms sum to <= 2^-24 |a b| — one fp32 rounding of the product — and
//           every bf16×bf16 product is exact in the fp32 accumulator. The MFMA
//           accumulator is rounded 6 times per 16 k here versus 16 times for the fp32 MFMA
//           (v_mfma_f32_32x32x2_f32 ≡ an fmaf chain), so the result is fp32-accurate while the
//           matrix core runs 6 × 32 = 192 cycles per 32×32×16 block instead of 8 × 64 = 512.
//   PL = 2  TF32-class fp32 via a 2-way split (SP_PREC_F32X2): x = hi + lo + ρ with hi = bf16(x),
//           lo = bf16(x - hi), |ρ| <= 2^-16 |x|, and the three products lo·hi, hi·lo, hi·hi (smallest
//           first). The dropped lo·lo, ρ_a·b and a·ρ_b sum to <= 3·2^-16 |a b| (1 + 2^-7) per product:
//           256× tighter than one bf16 plane, half the MFMAs and 24 instead of 44 split VALU per 8 elements.
//
// Same GEMM contract and fused epilogue as conv_gemm.hip (conv_common.h): A gathered on the fly
// from NHWC activations (implicit im2col), W as [Cout][K] bf16 planes (k contiguous).
//
// Tiling: WM×WN waves per workgroup, each wave a (32·TM)×(32·TN) patch of 32×32 accumulators;
// BK = 32 k per LDS stage (two 16-deep MFMA steps). Operand tiles are staged global → registers
// (fp32 A split into planes on the way) → LDS, double-buffered with one barrier per k-tile.
// LDS planes are [rows][32 bf16] = four 16-byte chunks per row; chunk c of row r lives at
// r·4 + (c ^ ((r >> 2) & 3)), which makes the 16-lane groups of every ds_read_b128 fragment
// read (lanes r = 0..31 of one chunk) hit 16 distinct bank slots, and keeps the 8-lane groups
// of the ds_write_b128 staging stores conflict-free.
// The 1-D grid is remapped XCD-aware (MI355X dispatches consecutive workgroups round-robin over
// the 8 XCDs): each XCD receives a contiguous run of output tiles, N fastest, so workgroups that
// share an A row-panel share one L2.
#include "conv_plan.h"
#include "mfma16_common.h"

namespace sp {

namespace {

// CNT: a split-K instance, which may combine in the launch (splitk_combine); other instances keep the plain
// epilogue.
// FOLD: folded split-K (ConvArgs::fold = S > 1, splits = 1, grid z = 1). The workgroup walks the S k-ranges a
// split launch would give its S workgroups (the same boundaries, nk·z / S), each into a freshly zeroed accumulator,
// and adds the partial tiles in z order — tot = acc₀, tot += acc_z: splitk_reduce_kernel's sum, element by element,
// on the registers that hold the element (no cross-lane exchange, no workspace) — then runs the epilogue once.
// Bit-identical to the split launch + reduce. Registers: the 64×64 tile's wave holds one f32x16 accumulator, so the
// running sum costs 16 VGPRs more.
template <int WM, int WN, int TM, int TN, int PL, bool FAST, bool CNT = false, bool FOLD = false>
__global__ __launch_bounds__(64 * WM * WN) void conv_mfma16_kernel(const ConvArgs p) {
  constexpr int NT = 64 * WM * WN;
  constexpr int BM = 32 * TM * WM;
  constexpr int BN = 32 * TN * WN;
  constexpr int TA = BM * 4 / NT;             // A chunk tasks (8 k each) per thread
  constexpr int TB = (BN * 4 + NT - 1) / NT;  // B chunk tasks per thread (last may be partial)
  constexpr bool BFULL = (BN * 4) % NT == 0;
  static_assert(TA * NT == BM * 4, "A staging must tile the workgroup");
  constexpr int PA = BM * 4;  // uint4 per A plane
  constexpr int PB = BN * 4;  // uint4 per B plane
  constexpr int STAGE = PL * (PA + PB);
  constexpr int NB = (WM * WN * TM * 32 * TN * 32 / 4 <= 2 * STAGE) ? TM : 1;  // epilogue bands per round
  constexpr int EPI = WM * WN * NB * 32 * TN * 32 / 4;
  constexpr int SMEM = 2 * STAGE > EPI ? 2 * STAGE : EPI;
  __shared__ uint4 smem[SMEM];

  const sp_conv_desc& d = p.d;
  const int64_t wps = d.wt_plane_stride;
  const int tid = threadIdx.x;
  const int c = tid & 3;  // this thread's 8-k chunk of every staged row

  // XCD-aware tile order (bijective for any grid size).
  const int wg = xcd_index(blockIdx.x, gridDim.x);
  const TileOrigin org = tile_origin<BM, BN>(p, wg);
  const int64_t m0 = org.m0;
  const int n0 = org.n0;

  // Per A task: the im2col row's origin (iy0, ix0) and a pointer to its tap-(0,0) pixel
  // (+ this thread's chunk).
  int a_iy0[TA], a_ix0[TA];
  const float* a_ptr[TA];
  const float* a2_ptr[TA];
#pragma unroll
  for (int i = 0; i < TA; ++i) {
    const Im2colRow row = im2col_row(p, m0 + ((tid + NT * i) >> 2));
    a_iy0[i] = row.iy0;
    a_ix0[i] = row.ix0;
    a_ptr[i] = d.A + row.pix * d.lda + c * 8;
    a2_ptr[i] = d.A2 ? d.A2 + row.pix * d.lda2 + c * 8 : nullptr;
  }
  const uint16_t* b_ptr[TB];
#pragma unroll
  for (int i = 0; i < TB; ++i) {
    const int n = n0 + ((tid + NT * i) >> 2);
    b_ptr[i] = d.Wt_bf16 + (int64_t)(n < d.Cout ? n : 0) * p.K + c * 8;
  }

  float4 ra[TA][2];
  uint4 rb[TB][PL];

  // FAST (Cin % 32 == 0): a 32-deep k-tile lies inside one filter tap, so the tap walk is
  // wave-uniform scalar state (kh, kw, c0) advanced once per tile.
  TapWalk walk;

  auto load_tile = [&](int kt) {
    const int k0 = kt * KT;
    if constexpr (FAST) {
      const int64_t off = ((int64_t)walk.kh * d.W + walk.kw) * d.lda + walk.c0;
      const int64_t off2 = ((int64_t)walk.kh * d.W + walk.kw) * d.lda2 + walk.c0;
#pragma unroll
      for (int i = 0; i < TA; ++i) {
        float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
        if ((unsigned)(a_iy0[i] + walk.kh) < (unsigned)d.H && (unsigned)(a_ix0[i] + walk.kw) < (unsigned)d.W) {
          const float* src = a_ptr[i] + off;
          v0 = *reinterpret_cast<const float4*>(src);
          v1 = *reinterpret_cast<const float4*>(src + 4);
          if (d.A2) {
            const float* s2 = a2_ptr[i] + off2;
            const float4 w0 = *reinterpret_cast<const float4*>(s2);
            const float4 w1 = *reinterpret_cast<const float4*>(s2 + 4);
            v0.x += w0.x; v0.y += w0.y; v0.z += w0.z; v0.w += w0.w;
            v1.x += w1.x; v1.y += w1.y; v1.z += w1.z; v1.w += w1.w;
          }
        }
        ra[i][0] = v0;
        ra[i][1] = v1;
      }
#pragma unroll
      for (int i = 0; i < TB; ++i) {
        const int t = tid + NT * i;
        const bool ok = (BFULL || t < BN * 4) && n0 + (t >> 2) < d.Cout;
#pragma unroll
        for (int pl = 0; pl < PL; ++pl)
          rb[i][pl] = ok ? *reinterpret_cast<const uint4*>(b_ptr[i] + k0 + pl * wps) : make_uint4(0u, 0u, 0u, 0u);
      }
      walk.advance(d, KT);
    } else {  // generic gather (Cin = 3 stem, K = 4 query-pos head): element-wise, k < K checked
      const int k = k0 + c * 8;
#pragma unroll
      for (int i = 0; i < TA; ++i) {
        float e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int kk = k + j;
          float v = 0.f;
          if (kk < p.K) {
            const int tap = kk / d.Cin;
            const int ch = kk - tap * d.Cin;
            const int kh = tap / d.KW;
            const int kw = tap - kh * d.KW;
            if ((unsigned)(a_iy0[i] + kh) < (unsigned)d.H && (unsigned)(a_ix0[i] + kw) < (unsigned)d.W) {
              const int64_t o = ((int64_t)kh * d.W + kw) * d.lda + ch - c * 8;
              v = a_ptr[i][o];
              if (d.A2) v += a2_ptr[i][((int64_t)kh * d.W + kw) * d.lda2 + ch - c * 8];
            }
          }
          e[j] = v;
        }
        ra[i][0] = make_float4(e[0], e[1], e[2], e[3]);
        ra[i][1] = make_float4(e[4], e[5], e[6], e[7]);
      }
#pragma unroll
      for (int i = 0; i < TB; ++i) {
        const int t = tid + NT * i;
        const bool nok = (BFULL || t < BN * 4) && n0 + (t >> 2) < d.Cout;
#pragma unroll
        for (int pl = 0; pl < PL; ++pl) {
          uint16_t e[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) e[j] = (nok && k + j < p.K) ? b_ptr[i][k0 + j + pl * wps] : (uint16_t)0;
          rb[i][pl] = make_uint4(e[0] | (uint32_t)e[1] << 16, e[2] | (uint32_t)e[3] << 16,
                                 e[4] | (uint32_t)e[5] << 16, e[6] | (uint32_t)e[7] << 16);
        }
      }
    }
  };

  auto store_tile = [&](uint4* st) {
#pragma unroll
    for (int i = 0; i < TA; ++i) {
      bf16x8 pv[PL];
      split_frag_pk<PL>(ra[i][0], ra[i][1], pv);
      const int row = (tid + NT * i) >> 2;
#pragma unroll
      for (int pl = 0; pl < PL; ++pl) *reinterpret_cast<bf16x8*>(st + pl * PA + sw16(row, c)) = pv[pl];
    }
#pragma unroll
    for (int i = 0; i < TB; ++i) {
      const int t = tid + NT * i;
      if (BFULL || t < BN * 4) {
#pragma unroll
        for (int pl = 0; pl < PL; ++pl) st[PL * PA + pl * PB + sw16(t >> 2, c)] = rb[i][pl];
      }
    }
  };

  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int wm = wave / WN;
  const int wn = wave - wm * WN;
  const int r = lane & 31;
  const int h = lane >> 5;

  f32x16 acc[TM][TN];
  zero_acc(acc);

  auto compute_tile = [&](const uint4* st) {
#pragma unroll
    for (int s = 0; s < KT / 16; ++s) {
      bf16x8 fa[TM][PL], fb[TN][PL];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int pl = 0; pl < PL; ++pl)
          fa[i][pl] = *reinterpret_cast<const bf16x8*>(st + pl * PA + sw16(wm * TM * 32 + i * 32 + r, 2 * s + h));
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int pl = 0; pl < PL; ++pl)
          fb[j][pl] = *reinterpret_cast<const bf16x8*>(st + PL * PA + pl * PB +
                                                       sw16(wn * TN * 32 + j * 32 + r, 2 * s + h));
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = mfma_planes<PL>(fa[i], fb[j], acc[i][j]);
    }
  };

  // one k-range [kt0, kt0 + nk) into acc; every wave has passed the last barrier when it returns, so the next
  // range may overwrite stage 0
  auto run_range = [&](int kt0, int nk) {
    if constexpr (FAST) walk.seek(d, kt0 * KT);
    if (nk > 0) {
      load_tile(kt0);
      store_tile(smem);
    }
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      if (kt + 1 < nk) load_tile(kt0 + kt + 1);
      compute_tile(smem + (kt & 1) * STAGE);
      if (kt + 1 < nk) store_tile(smem + ((kt + 1) & 1) * STAGE);
      __syncthreads();
    }
  };
  const int nk_all = (p.K + KT - 1) / KT;
  if constexpr (FOLD) {
    f32x16 tot[TM][TN];
    const int S = p.fold;
    for (int z = 0; z < S; ++z) {
      const int kt0 = (int)(((int64_t)nk_all * z) / S);
      const int kt1 = (int)(((int64_t)nk_all * (z + 1)) / S);
      if (z) zero_acc(acc);
      run_range(kt0, kt1 - kt0);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int q = 0; q < 16; ++q) tot[i][j][q] = z ? tot[i][j][q] + acc[i][j][q] : acc[i][j][q];
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = tot[i][j];
  } else {
    const KRange kr = splitk_range(p, nk_all);
    run_range(kr.kt0, kr.kt1 - kr.kt0);
  }

  float* smemf = reinterpret_cast<float*>(smem);
  epilogue_tile<TM, TN, NB, false, PL == 1, CNT>(p, smemf + wave * (NB * 32 * TN * 32), acc, m0 + wm * TM * 32,
                                                  n0 + wn * TN * 32, lane);
  if constexpr (CNT) {
    if (p.counters)  // split-K, combined in this launch by the tile's last workgroup
      splitk_combine<NT, BM, BN>(p, reinterpret_cast<int*>(smem), wg, m0, n0);
  }
}

template <int WM, int WN, int TM, int TN>
int launch_cfg(const ConvArgs& a, const ConvPlan& p, hipStream_t s) {
  constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
  const int64_t tiles = ((a.M + BM - 1) / BM) * ((a.d.Cout + BN - 1) / BN);
  dim3 grid((unsigned)tiles, 1, p.splits);
  ConvArgs b = a;
  b.counters = p.counters ? a.d.splitk_counters : nullptr;
  if constexpr (WM == 2 && WN == 2 && TM == 1 && TN == 1) {
    if (a.fold && p.splits > 1) {  // the folded 64×64 split tile: one launch, no partial slabs, no reduce
      b.fold = p.splits;
      b.splits = 1;
      b.counters = nullptr;
      grid.z = 1;
      if (p.planes == 3)
        hipLaunchKernelGGL((conv_mfma16_kernel<2, 2, 1, 1, 3, true, false, true>), grid, dim3(256), 0, s, b);
      else if (p.planes == 2)
        hipLaunchKernelGGL((conv_mfma16_kernel<2, 2, 1, 1, 2, true, false, true>), grid, dim3(256), 0, s, b);
      else
        hipLaunchKernelGGL((conv_mfma16_kernel<2, 2, 1, 1, 1, true, false, true>), grid, dim3(256), 0, s, b);
      return check_launch("sp_conv2d(folded split-K)");
    }
  }
  if (p.counters && p.planes == 3)
    hipLaunchKernelGGL((conv_mfma16_kernel<WM, WN, TM, TN, 3, true, true>), grid, dim3(64 * WM * WN), 0, s, b);
  else if (p.counters && p.planes == 2)
    hipLaunchKernelGGL((conv_mfma16_kernel<WM, WN, TM, TN, 2, true, true>), grid, dim3(64 * WM * WN), 0, s, b);
  else if (p.counters)
    hipLaunchKernelGGL((conv_mfma16_kernel<WM, WN, TM, TN, 1, true, true>), grid, dim3(64 * WM * WN), 0, s, b);
  else if (p.planes == 3)
    hipLaunchKernelGGL((conv_mfma16_kernel<WM, WN, TM, TN, 3, true>), grid, dim3(64 * WM * WN), 0, s, b);
  else if (p.planes == 2)
    hipLaunchKernelGGL((conv_mfma16_kernel<WM, WN, TM, TN, 2, true>), grid, dim3(64 * WM * WN), 0, s, b);
  else
    hipLaunchKernelGGL((conv_mfma16_kernel<WM, WN, TM, TN, 1, true>), grid, dim3(64 * WM * WN), 0, s, b);
  int rc = check_launch(p.planes == 3 ? "sp_conv2d(f32x3)" : p.planes == 2 ? "sp_conv2d(f32x2)" : "sp_conv2d(bf16)");
  if (rc || p.splits == 1 || p.counters) return rc;
  return launch_splitk_reduce(a, s);
}

// generic gather: one small-tile instance per operand mode
int launch_generic(const ConvArgs& a, const ConvPlan& p, hipStream_t s) {
  const int64_t tiles = ((a.M + 63) / 64) * ((a.d.Cout + 63) / 64);
  dim3 grid((unsigned)tiles, 1, p.splits);
  if (p.planes == 3)
    hipLaunchKernelGGL((conv_mfma16_kernel<2, 2, 1, 1, 3, false>), grid, dim3(256), 0, s, a);
  else if (p.planes == 2)
    hipLaunchKernelGGL((conv_mfma16_kernel<2, 2, 1, 1, 2, false>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((conv_mfma16_kernel<2, 2, 1, 1, 1, false>), grid, dim3(256), 0, s, a);
  int rc = check_launch(p.planes == 3   ? "sp_conv2d(f32x3 generic)"
                        : p.planes == 2 ? "sp_conv2d(f32x2 generic)"
                                        : "sp_conv2d(bf16 generic)");
  if (rc || p.splits == 1) return rc;
  return launch_splitk_reduce(a, s);
}

}  // namespace

// The register-staged tiles (ids 1-6, conv_plan.h).
int launch_mfma16(const ConvArgs& a, const ConvPlan& p, hipStream_t s) {
  if (p.family != SP_CONV_MFMA16) {
    set_error("sp_conv2d: plan names family %d, which the register-staged launcher is not built with", (int)p.family);
    return -1;
  }
  if (p.generic) return launch_generic(a, p, s);
  switch (p.tile) {
    case 1: return launch_cfg<2, 2, 2, 2>(a, p, s);
    case 2: return launch_cfg<4, 2, 2, 2>(a, p, s);
    case 3: return launch_cfg<2, 2, 1, 2>(a, p, s);
    case 5: return launch_cfg<2, 4, 2, 2>(a, p, s);
    case 6: return launch_cfg<2, 2, 2, 1>(a, p, s);
    default: return launch_cfg<2, 2, 1, 1>(a, p, s);
  }
}

}  // namespace sp
