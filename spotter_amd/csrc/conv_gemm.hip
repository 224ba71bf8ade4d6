// Implicit-GEMM convolution / linear layer on fp32 MFMA (gfx950).
//
// One kernel covers every conv and nn.Linear on the RT-DETRv2 path: the
// ResNet-vd backbone (RN:38-68, RN:179-231), encoder input projections
// (M2:1350-1360), CCFM convs (M2:817-835, M2:907-952), AIFI / decoder
// projections and FFNs (M2:228-242, M2:273-336), MSDA value/offset/weight/
// output projections (M2:144-147) and the heads (M2:1376-1381, M2:1777-1787).
//
// Math: out[m, n] = epilogue(Σ_k A[m, k] · W[n, k]) with A gathered on the fly
// from NHWC activations (im2col never materialised) and W stored [Cout][K]
// (k contiguous). Tile BM×BN×32 per 256-thread workgroup (2×2 waves), each
// wave a (32·TM)×(32·TN) patch of v_mfma_f32_32x32x2f32 accumulators (exact
// fp32 fmaf chains, 64 FLOP/clk/SIMD). A and B tiles are staged through LDS as
// row-major [row][32 k] with a 16-byte-chunk XOR swizzle so the per-lane
// ds_read_b128 fragment reads are conflict-free; the k order inside an 8-deep
// slab is permuted (lane half h owns k = 8s + 4h + j) identically for A and B,
// which lets one ds_read_b128 feed four MFMAs. Global loads for tile t+1 are
// issued before the MFMAs of tile t (register staging).
//
// Epilogue (fused): row mask (query-selection valid_mask, M2:1592), per-channel
// BatchNorm scale/shift (FrozenBN M2:748-758 / eval BN), residual, activation,
// post-activation residual, and a grouped output row map so projections write
// straight into concatenated / flattened buffers (M2:1553-1555).
#include "conv_plan.h"

#ifndef SP_DIAG_KERNELS
#define SP_DIAG_KERNELS 0
#endif

bool sp::conv_gemm_has_fused_ln() { return SP_DIAG_KERNELS != 0; }

namespace sp {

namespace {

constexpr int BK = 32;

__device__ __forceinline__ int swz(int row, int chunk) { return row * BK + ((chunk ^ ((row >> 1) & 7)) << 2); }


// WM × WN waves (WM·WN = 4), each a (32·TM) × (32·TN) patch: 2×2 is the square default, 4×1 gives
// the 32- and 64-wide N tiles that thin outputs (Cout = 32 / 64: stem, stage 1) need without idle MFMAs.
// CNT: the split-K launches, which may combine in the launch (splitk_combine); every other instance keeps the
// plain epilogue.
template <int TM, int TN, int DB, int WM = 2, bool LN = false, bool CNT = false>
__global__ __launch_bounds__(256) void conv_gemm_kernel(const ConvArgs p) {
  constexpr int WN = 4 / WM;
  static_assert(WM * WN == 4, "four waves per workgroup");
  constexpr int BM = 32 * WM * TM;
  constexpr int BN = 32 * WN * TN;
  constexpr int PA = BM / 32;  // loader passes (32 rows per pass)
  constexpr int PB = BN / 32;
  constexpr int STAGE = (BM + BN) * BK;
  constexpr int EPI = LN ? 32 * (BN + 4) : 4 * 32 * (TN * 32);  // epilogue: one 32×(32·TN) slab per wave,
                                                                 // or the 32 whole rows of a LayerNorm tile
  constexpr int SMEM = STAGE * (DB ? 2 : 1) > EPI ? STAGE * (DB ? 2 : 1) : EPI;
  __shared__ __attribute__((aligned(16))) float smem[SMEM];

  const sp_conv_desc& d = p.d;
  const int tid = threadIdx.x;
  const int lrow = tid >> 3;   // 0..31
  const int lchunk = tid & 7;  // 16-byte chunk of the 32-wide k slab
  const int64_t m0 = (int64_t)blockIdx.y * BM;
  const int n0 = blockIdx.x * BN;

  // Per-row implicit-im2col state for this thread's A rows (fixed across k).
  int a_iy0[PA], a_ix0[PA], a_base[PA];
  bool a_ok[PA];
#pragma unroll
  for (int i = 0; i < PA; ++i) {
    int64_t m = m0 + i * 32 + lrow;
    a_ok[i] = m < p.M;
    int64_t mm = a_ok[i] ? m : 0;
    int b = (int)(mm / p.HoWo);
    int rem = (int)(mm - (int64_t)b * p.HoWo);
    int oy = rem / d.Wo;
    int ox = rem - oy * d.Wo;
    a_iy0[i] = oy * d.stride - d.pad;
    a_ix0[i] = ox * d.stride - d.pad;
    a_base[i] = b * d.H;
  }

  float4 ra[PA], rb[PB];

  auto load_tile = [&](int kt) {
    const int k0 = kt * BK;
    if (p.fast) {
      const int tap = k0 / d.Cin;
      const int c0 = k0 - tap * d.Cin + lchunk * 4;
      const int kh = tap / d.KW;
      const int kw = tap - kh * d.KW;
#pragma unroll
      for (int i = 0; i < PA; ++i) {
        const int iy = a_iy0[i] + kh;
        const int ix = a_ix0[i] + kw;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a_ok[i] && (unsigned)iy < (unsigned)d.H && (unsigned)ix < (unsigned)d.W) {
          const int64_t pix = (int64_t)(a_base[i] + iy) * d.W + ix;
          SP_BCHECK(pix, (int64_t)d.N * d.H * d.W);
          SP_BCHECK(c0 + 3, d.Cin);
          v = *reinterpret_cast<const float4*>(d.A + pix * d.lda + c0);
          if (d.A2) {
            float4 w = *reinterpret_cast<const float4*>(d.A2 + pix * d.lda2 + c0);
            v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
          }
        }
        ra[i] = v;
      }
#pragma unroll
      for (int i = 0; i < PB; ++i) {
        const int n = n0 + i * 32 + lrow;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n < d.Cout) SP_BCHECK(k0 + lchunk * 4 + 3, p.K);
        if (n < d.Cout) v = *reinterpret_cast<const float4*>(d.Wt + (int64_t)n * p.K + k0 + lchunk * 4);
        rb[i] = v;
      }
    } else {
#pragma unroll
      for (int i = 0; i < PA; ++i) {
        float e[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = k0 + lchunk * 4 + j;
          float v = 0.f;
          if (a_ok[i] && k < p.K) {
            const int tap = k / d.Cin;
            const int c = k - tap * d.Cin;
            const int kh = tap / d.KW;
            const int kw = tap - kh * d.KW;
            const int iy = a_iy0[i] + kh;
            const int ix = a_ix0[i] + kw;
            if ((unsigned)iy < (unsigned)d.H && (unsigned)ix < (unsigned)d.W) {
              const int64_t pix = (int64_t)(a_base[i] + iy) * d.W + ix;
              v = d.A[pix * d.lda + c];
              if (d.A2) v += d.A2[pix * d.lda2 + c];
            }
          }
          e[j] = v;
        }
        ra[i] = make_float4(e[0], e[1], e[2], e[3]);
      }
#pragma unroll
      for (int i = 0; i < PB; ++i) {
        const int n = n0 + i * 32 + lrow;
        float e[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = k0 + lchunk * 4 + j;
          e[j] = (n < d.Cout && k < p.K) ? d.Wt[(int64_t)n * p.K + k] : 0.f;
        }
        rb[i] = make_float4(e[0], e[1], e[2], e[3]);
      }
    }
  };

  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int wm = wave / WN;
  const int wn = wave % WN;
  const int r = lane & 31;
  const int h = lane >> 5;

  f32x16 acc[TM][TN];
  zero_acc(acc);

  const KRange kr = splitk_range(p, (p.K + BK - 1) / BK);
  const int kt0 = kr.kt0;
  const int nk = kr.kt1 - kt0;

  auto store_tile = [&](float* st) {
    float* As = st;
    float* Bs = st + BM * BK;
#pragma unroll
    for (int i = 0; i < PA; ++i)
      *reinterpret_cast<float4*>(As + swz(i * 32 + lrow, lchunk)) = ra[i];
#pragma unroll
    for (int i = 0; i < PB; ++i)
      *reinterpret_cast<float4*>(Bs + swz(i * 32 + lrow, lchunk)) = rb[i];
  };

  auto compute_tile = [&](const float* st) {
    const float* As = st;
    const float* Bs = st + BM * BK;
#pragma unroll
    for (int s = 0; s < BK / 8; ++s) {
      float4 fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i)
        fa[i] = *reinterpret_cast<const float4*>(As + swz(wm * TM * 32 + i * 32 + r, s * 2 + h));
#pragma unroll
      for (int j = 0; j < TN; ++j)
        fb[j] = *reinterpret_cast<const float4*>(Bs + swz(wn * TN * 32 + j * 32 + r, s * 2 + h));
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].x, fb[j].x, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].y, fb[j].y, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].z, fb[j].z, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].w, fb[j].w, acc[i][j], 0, 0, 0);
        }
    }
  };

  if (nk > 0) load_tile(kt0);
  if (DB && nk > 0) {
    // two LDS stages, one barrier per k-tile: tile t+1's global loads and LDS
    // store overlap tile t's MFMAs.
    store_tile(smem);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      if (kt + 1 < nk) load_tile(kt0 + kt + 1);
      compute_tile(smem + (kt & 1) * STAGE);
      if (kt + 1 < nk) store_tile(smem + ((kt + 1) & 1) * STAGE);
      __syncthreads();
    }
  } else if (!DB) {
    for (int kt = 0; kt < nk; ++kt) {
      __syncthreads();
      store_tile(smem);
      __syncthreads();
      if (kt + 1 < nk) load_tile(kt0 + kt + 1);
      compute_tile(smem);
    }
  }

  // Epilogue, staged through LDS so every lane applies it to a contiguous float4
  // of one output row (16-byte loads of res1/res2/scale/shift, 16-byte stores):
  // pass i moves each wave's 32-row band acc[i][*] to its private LDS slab.
  __syncthreads();  // main loop done with the operand stages
  if constexpr (LN) {
    static_assert(WM == 1 && TM == 1, "row LayerNorm tiles are 32 rows × the whole N");
    epilogue_rowln<TN>(p, smem, acc[0], m0, wave, lane);
    return;
  }
#pragma unroll
  for (int i = 0; i < TM; ++i)
    epilogue_band<TN, false, CNT>(p, smem + wave * (32 * TN * 32), acc[i], m0 + wm * TM * 32 + i * 32,
                                  n0 + wn * TN * 32, lane);
  if constexpr (CNT) {
    if (p.counters)  // split-K, combined in this launch by the tile's last workgroup
      splitk_combine<256, BM, BN>(p, reinterpret_cast<int*>(smem), blockIdx.y * gridDim.x + blockIdx.x, m0, n0);
  }
}

// Split-K combine: out = epilogue(Σ_z partial[z]) in fixed z order (deterministic).
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const ConvArgs p) {
  const int n4 = (p.d.Cout + 3) / 4;
  const int64_t total = p.M * n4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = i / n4;
    const int n = (int)(i - m * n4) * 4;
    SP_BCHECK(((int64_t)(p.splits - 1) * p.M + m) * p.ldp + n + 3, p.d.workspace_elems);
    float4 v = *reinterpret_cast<const float4*>(p.partial + m * p.ldp + n);
    for (int z = 1; z < p.splits; ++z) {
      float4 u = *reinterpret_cast<const float4*>(p.partial + ((int64_t)z * p.M + m) * p.ldp + n);
      v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
    }
    epilogue_store(p, m, n, v);
  }
}

template <int TM, int TN, int DB, int WM = 2, bool LN = false, bool CNT = false>
int launch(const ConvArgs& a, const ConvPlan& p, hipStream_t s) {
  constexpr int BM = 32 * WM * TM, BN = 32 * (4 / WM) * TN;
  dim3 grid((a.d.Cout + BN - 1) / BN, (unsigned)((a.M + BM - 1) / BM), p.splits);
  ConvArgs b = a;
  b.counters = CNT ? a.d.splitk_counters : nullptr;
  hipLaunchKernelGGL((conv_gemm_kernel<TM, TN, DB, WM, LN, CNT>), grid, dim3(256), 0, s, b);
  int rc = check_launch("sp_conv2d");
  if (rc || p.splits == 1 || CNT) return rc;
  return launch_splitk_reduce(a, s);
}

}  // namespace

int launch_splitk_reduce(const ConvArgs& a, hipStream_t s) {
  int64_t work = a.M * ((a.d.Cout + 3) / 4);
  int64_t g = (work + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)g), dim3(256), 0, s, a);
  return check_launch("sp_conv2d(split-K reduce)");
}

// The fp32 tiles by their "<WM?><TM><TN><DB>" id (conv_plan.h).
int launch_fp32(const ConvArgs& a, const ConvPlan& p, hipStream_t s) {
#if SP_DIAG_KERNELS
  // Linear → +residual → LayerNorm in one launch: 32-row tiles holding whole rows. Measured slower than the
  // unfused LayerNorm (58.1 vs 56.7 ms per step): compiled into diagnostic builds only
  // (UNIT=conv_gemm tools/build_diag.sh ... -DSP_DIAG_KERNELS=1)
  if (p.family == SP_CONV_FUSED_LN) switch (p.tile) {
      case 1111: return launch<1, 1, 1, 1, true>(a, p, s);
      case 1121: return launch<1, 2, 1, 1, true>(a, p, s);
      case 1131: return launch<1, 3, 1, 1, true>(a, p, s);
      default: return launch<1, 4, 1, 1, true>(a, p, s);
    }
#endif
  if (p.counters) return launch<1, 1, 0, 2, false, true>(a, p, s);  // split-K combined in the launch: 64×64 tiles
  switch (p.tile) {
    case 220: return launch<2, 2, 0>(a, p, s);
    case 221: return launch<2, 2, 1>(a, p, s);
    case 210: return launch<2, 1, 0>(a, p, s);
    case 211: return launch<2, 1, 1>(a, p, s);
    case 120: return launch<1, 2, 0>(a, p, s);
    case 121: return launch<1, 2, 1>(a, p, s);
    case 111: return launch<1, 1, 1>(a, p, s);
    case 1110: return launch<1, 1, 0, 1>(a, p, s);
    case 1111: return launch<1, 1, 1, 1>(a, p, s);
    case 1120: return launch<1, 2, 0, 1>(a, p, s);
    case 1121: return launch<1, 2, 1, 1>(a, p, s);
    case 4110: return launch<1, 1, 0, 4>(a, p, s);
    case 4111: return launch<1, 1, 1, 4>(a, p, s);
    case 4210: return launch<2, 1, 0, 4>(a, p, s);
    case 4211: return launch<2, 1, 1, 4>(a, p, s);
    case 4120: return launch<1, 2, 0, 4>(a, p, s);
    case 4121: return launch<1, 2, 1, 4>(a, p, s);
    default: return launch<1, 1, 0>(a, p, s);  // 110
  }
}

}  // namespace sp
