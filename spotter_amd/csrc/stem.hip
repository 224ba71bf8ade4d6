// Backbone stem conv 1 (RN:71-114, first RTDetrResNetConvLayer: 3x3 stride 2, Cin 3 → 32, FrozenBN
// M2:748-758, ReLU) read straight from the processor's NCHW pixel_values (IPP:461-462).
//
// K = 27 leaves an implicit GEMM nothing to tile (the MFMA kernels ran it at 12 TF/s, plus an
// NCHW→NHWC pass over the 157 MB batch), so this is a direct VALU convolution: one lane per output
// pixel, the 27 taps in registers, the Cout×27 weights uniform across the wave (scalar-cache loads),
// fmaf chains in the khwc tap order, BN affine + ReLU; the workgroup's NHWC rows go out through LDS
// as coalesced float4 stores.
// Work per image at 640²: 320²·Cout·27·2 FLOP = 177 MFLOP; compulsory bytes 3·640²·4 in +
// 320²·Cout·4 out (18 MB at Cout 32) — the output write bounds it.
#include "direct3x3.h"

namespace sp {
namespace {

constexpr int STEM_BLOCK = 256;

// Each lane computes one pixel's CO outputs; the workgroup's 256 consecutive NHWC rows are one
// contiguous span of y, so the results are staged in LDS (row stride CO+4 floats: 16-byte aligned,
// rows spread over the banks) and written back as consecutive float4s across the lanes.
// OT: float (fp32 rows) or uint16_t (bf16 rows, RNE at the store: the bf16 variant, ABI v10).
template <int CO, typename OT>
__global__ __launch_bounds__(STEM_BLOCK) void stem_conv_nchw_kernel(
    const float* __restrict__ x, const float* __restrict__ wt, const float* __restrict__ scale,
    const float* __restrict__ shift, OT* __restrict__ y, int n, int h, int w, int ho, int wo,
    int relu) {
  constexpr int LD = CO + 4;
  __shared__ float4 tile4[STEM_BLOCK * LD / 4];
  float* tile = reinterpret_cast<float*>(tile4);
  const int64_t p0 = (int64_t)blockIdx.x * STEM_BLOCK;
  const int64_t total = (int64_t)n * ho * wo;
  const int rows = (int)min<int64_t>(STEM_BLOCK, total - p0);
  const int t = threadIdx.x;
  if (t < rows) {
    const int64_t p = p0 + t;
    const int ox = (int)(p % wo);
    const int64_t q = p / wo;
    const int oy = (int)(q % ho);
    const int b = (int)(q / ho);
    const int64_t hw = (int64_t)h * w;
    SP_BCHECK(b, n);
    const float* xb = x + (int64_t)b * 3 * hw;

    float in[27];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int iy = 2 * oy - 1 + kh;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int ix = 2 * ox - 1 + kw;
        const bool ok = (unsigned)iy < (unsigned)h && (unsigned)ix < (unsigned)w;
        const int64_t off = ok ? (int64_t)iy * w + ix : 0;
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
          const float v = xb[ci * hw + off];
          in[(kh * 3 + kw) * 3 + ci] = ok ? v : 0.f;
        }
      }
    }

#pragma unroll
    for (int c0 = 0; c0 < CO; c0 += 4) {
      float a[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float* wr = wt + (c0 + j) * 27;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 27; ++k) s = fmaf(in[k], wr[k], s);
        s = fmaf(s, scale[c0 + j], shift[c0 + j]);
        a[j] = relu ? fmaxf(s, 0.f) : s;
      }
      *reinterpret_cast<float4*>(tile + t * LD + c0) = make_float4(a[0], a[1], a[2], a[3]);
    }
  }
  __syncthreads();
  constexpr int C4 = CO / 4;
  const int n4 = rows * C4;
  if constexpr (sizeof(OT) == 4) {
    float4* yo = reinterpret_cast<float4*>(y + p0 * CO);
    for (int i = t; i < n4; i += STEM_BLOCK) {
      const int r = i / C4, c = i - r * C4;
      yo[i] = *reinterpret_cast<const float4*>(tile + r * LD + 4 * c);
    }
  } else {
    uint2* yo = reinterpret_cast<uint2*>(y + p0 * CO);
    for (int i = t; i < n4; i += STEM_BLOCK) {
      const int r = i / C4, c = i - r * C4;
      const float4 v = *reinterpret_cast<const float4*>(tile + r * LD + 4 * c);
      yo[i] = make_uint2(cvt_pk_bf16(v.x, v.y), cvt_pk_bf16(v.z, v.w));
    }
  }
}

}  // namespace
}  // namespace sp

using namespace sp;

namespace sp {
namespace {
template <typename OT>
int stem_launch(const char* what, const float* x, const float* wt, const float* scale, const float* shift, OT* y,
                int n, int h, int w, int cout, int act, void* stream) {
  SP_ARG_CHECK(x && wt && scale && shift && y && n > 0 && h > 0 && w > 0 && (act == 0 || act == 1) &&
                   (cout == 32 || cout == 64),
               "%s: bad args (cout must be 32 or 64, act none/relu)", what);
  // the workgroup's rows leave as float4 (fp32 rows) / uint2 (bf16 rows) stores
  SP_ARG_CHECK(((uintptr_t)y & (4 * sizeof(OT) - 1)) == 0, "%s: y must be %d-byte aligned", what, (int)(4 * sizeof(OT)));
  const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
  const int64_t total = (int64_t)n * ho * wo;
  const unsigned grid = (unsigned)((total + STEM_BLOCK - 1) / STEM_BLOCK);
  if (cout == 32)
    hipLaunchKernelGGL((stem_conv_nchw_kernel<32, OT>), dim3(grid), dim3(STEM_BLOCK), 0, as_stream(stream), x, wt,
                       scale, shift, y, n, h, w, ho, wo, act);
  else
    hipLaunchKernelGGL((stem_conv_nchw_kernel<64, OT>), dim3(grid), dim3(STEM_BLOCK), 0, as_stream(stream), x, wt,
                       scale, shift, y, n, h, w, ho, wo, act);
  return check_launch(what);
}
}  // namespace
}  // namespace sp

extern "C" int sp_stem_conv3x3s2_nchw(const float* x, const float* wt, const float* scale, const float* shift,
                                      float* y, int n, int h, int w, int cout, int act, void* stream) {
  return stem_launch("sp_stem_conv3x3s2_nchw", x, wt, scale, shift, y, n, h, w, cout, act, stream);
}

extern "C" int sp_stem_conv3x3s2_nchw_bf16(const float* x, const float* wt, const float* scale, const float* shift,
                                           uint16_t* y, int n, int h, int w, int cout, int act, void* stream) {
  return stem_launch("sp_stem_conv3x3s2_nchw_bf16", x, wt, scale, shift, y, n, h, w, cout, act, stream);
}

// ---------------------------------------------------------------------------------------------
// Stem convs 2 and 3 of the bf16 variant (RN:78-103: 3×3 stride 1 pad 1, Cin 32 → Cout 32 / 64, FrozenBN,
// ReLU) as a direct LDS-halo convolution on bf16 rows (ABI v10); the pipeline is direct3x3.h's. As an implicit
// GEMM these ran at 179 / 361 TF (C3, 26.2 M output rows): K = 288 gives a 64-wide tile little reuse, a 32-wide
// Cout wastes half of it, and every A row is fetched once per tap.
// Tile: 4 rows × 64 pixels, four waves, wave v computes row v (64 pixels × Cout). The grid is persistent (2 or 3
// workgroups per CU walk the tiles), since per 256-pixel tile the weights are as many bytes as the input halo.
// LDS: the (4 + 2) × (64 + 2) × 32 bf16 halo (25,344 B), all 9·Cout·32 weights (18,432 / 36,864 B), the affine.
// v_mfma_f32_32x32x16_bf16, k in (tap, 16-channel) order. 2.8-2.9x (Cout 32) and 1.4-1.8x (Cout 64) the implicit
// GEMM (profiles/r3/bf16/ab_stem_c32_direct_prefetch.jsonl) against 1.9x and 1.03-1.16x with a synchronous halo
// load per tile.
namespace sp {
namespace {

constexpr int C3_TW = 64;  // output pixels per wave row
constexpr int C3_TH = 4;   // output rows of a tile: one per wave

template <int CO>
__global__ __launch_bounds__(256, 2) void conv3x3_c32_bf16_kernel(const uint16_t* __restrict__ x,
                                                                  const uint16_t* __restrict__ w16,
                                                                  const float* __restrict__ scale,
                                                                  const float* __restrict__ shift,
                                                                  uint16_t* __restrict__ y, int nimg, int h, int w,
                                                                  int tiles_x, int tiles_y, int act) {
  using Halo = HaloPrefetch<256, C3_TH, C3_TW, 4, 8>;
  constexpr int HC = Halo::HC;
  constexpr int TMN = CO / 32;  // 32-channel blocks
  __shared__ uint4 lds[Halo::UNITS + 9 * CO * 4];
  __shared__ float aff[2 * CO];
  static_assert(sizeof(lds) + sizeof(aff) == (CO == 32 ? 44032 : 62720), "static LDS bytes");
  uint4* halo = lds;
  uint4* wl = lds + Halo::UNITS;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  stage_weights<CO, 4, 256>(wl, w16);
  stage_affine<CO>(aff, scale, shift);
  const int64_t ntiles = (int64_t)nimg * tiles_x * tiles_y;
  Halo pf;
  if ((int64_t)blockIdx.x < ntiles) pf.fetch(x, 32, blockIdx.x, tiles_x, tiles_y, nimg, h, w);
  const int r = lane & 31, hh = lane >> 5;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const TileAt t = tile_at<C3_TH, C3_TW>(tile, tiles_x, tiles_y, nimg);
    __syncthreads();  // the previous tile's halo reads are done
    pf.stash(halo);
    __syncthreads();
    if (tile + gridDim.x < ntiles) pf.fetch(x, 32, tile + gridDim.x, tiles_x, tiles_y, nimg, h, w);

    f32x16 acc[TMN][2];
    zero_acc(acc);
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int tap = kh * 3 + kw;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int ch = 2 * s + hh;  // k chunk: ci 16s + 8hh .. +7
          bf16x8 fa[TMN], fb[2];
#pragma unroll
          for (int i = 0; i < TMN; ++i) {
            const int n = i * 32 + r;
            fa[i] = *reinterpret_cast<const bf16x8*>(wl + (tap * CO + n) * 4 + swz<4>(n, ch));
          }
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int col = j * 32 + r + kw;
            fb[j] = *reinterpret_cast<const bf16x8*>(halo + ((wave + kh) * HC + col) * 4 + swz<4>(col, ch));
          }
#pragma unroll
          for (int i = 0; i < TMN; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
      }
    const int oy = t.oy0 + wave;
    if (oy < h) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int ox = t.ox0 + j * 32 + r;
        if (ox >= w) continue;
        uint16_t* yrow = y + (((int64_t)t.b * h + oy) * w + ox) * CO;
#pragma unroll
        for (int i = 0; i < TMN; ++i)
#pragma unroll
          for (int p = 0; p < 2; ++p) {
            // one v_permlane32_swap per value pair gives lane hh channels base .. base + 7 (16-byte stores,
            // as in the Cin-64 kernel below): 1.11x / 1.16x per launch at C3 (profiles/r4/bf16/ab_c32_swap.json)
            float v[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[i][j][8 * p + e]),
                                                               __float_as_uint(acc[i][j][8 * p + 4 + e]), false, false);
              v[e] = __uint_as_float(sw[0]);
              v[4 + e] = __uint_as_float(sw[1]);
            }
            const int base = i * 32 + 16 * p + 8 * hh;
            unsigned pk[4];
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
              const float u0 = fmaf(v[e], aff[base + e], aff[CO + base + e]);
              const float u1 = fmaf(v[e + 1], aff[base + e + 1], aff[CO + base + e + 1]);
              pk[e / 2] = cvt_pk_bf16(act ? fmaxf(u0, 0.f) : u0, act ? fmaxf(u1, 0.f) : u1);
            }
            *reinterpret_cast<uint4*>(yrow + base) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
          }
      }
    }
  }  // tiles
}

}  // namespace
}  // namespace sp

extern "C" int sp_conv3x3_c32_bf16(const uint16_t* x, const uint16_t* w16, const float* scale, const float* shift,
                                   uint16_t* y, int n, int h, int w, int cout, int act, void* stream) {
  using namespace sp;
  SP_ARG_CHECK(x && w16 && scale && shift && y && n > 0 && h > 0 && w > 0 && (cout == 32 || cout == 64) &&
                   (act == 0 || act == 1) && ((uintptr_t)x & 15) == 0 && ((uintptr_t)w16 & 15) == 0 &&
                   ((uintptr_t)y & 15) == 0,
               "sp_conv3x3_c32_bf16: bad args (Cin 32, Cout 32 or 64, act none/relu, aligned dense bf16 rows)");
  // persistent grid: as many workgroups as fit on the chip at once (2 per CU at Cout 64, 3 at Cout 32)
  const int64_t cap = (int64_t)g_num_cus * (cout == 32 ? 3 : 2);
  const DirectGrid g = direct_grid<C3_TH, C3_TW>(n, h, w, cap);
  if (cout == 32)
    hipLaunchKernelGGL((conv3x3_c32_bf16_kernel<32>), dim3(g.grid), dim3(256), 0, as_stream(stream), x, w16, scale,
                       shift, y, n, h, w, g.tiles_x, g.tiles_y, act);
  else
    hipLaunchKernelGGL((conv3x3_c32_bf16_kernel<64>), dim3(g.grid), dim3(256), 0, as_stream(stream), x, w16, scale,
                       shift, y, n, h, w, g.tiles_x, g.tiles_y, act);
  return check_launch("sp_conv3x3_c32_bf16");
}

// ---------------------------------------------------------------------------------------------
// The same two stem convs in the fp32 modes (ABI v10) on fp32 rows with v_mfma_f32_32x32x2_f32 (exact fp32
// products, fp32 accumulate); the pipeline is direct3x3.h's. As fp32-MFMA implicit GEMMs they ran at 93 / 106 TF
// of 157.3 (C2, profiles/r3/conv_detail_c2_fp32_r3g.json).
// Tile: 8 rows × 64 pixels, one persistent workgroup per CU, eight waves, wave v computes row v (64 pixels × Cout).
// LDS: all 9·Cout·32 fp32 weights (36 / 72 KB), the (8 + 2) × (64 + 2) × 32 fp32 halo (82.5 KB), the affine.
// k order: per tap, chunk pairs q = 0..3: lane (r, half hh) reads a float4 (4 consecutive channels of chunk
// 2q + hh) of its weight row and of its pixel; MFMA e of the four takes component e, so MFMA e contracts
// channels 8q + e and 8q + 4 + e.
namespace sp {
namespace {

constexpr int F3_TH = 8, F3_HC = C3_TW + 2;

template <int CO>
__global__ __launch_bounds__(512, 1) void conv3x3_c32_f32_kernel(const float* __restrict__ x,
                                                                 const float* __restrict__ wt,
                                                                 const float* __restrict__ scale,
                                                                 const float* __restrict__ shift,
                                                                 float* __restrict__ y, int nimg, int h, int w,
                                                                 int tiles_x, int tiles_y, int act) {
  using Halo = HaloPrefetch<512, F3_TH, C3_TW, 8, 4>;
  constexpr int TMN = CO / 32;
  __shared__ uint4 lds[Halo::UNITS + 9 * CO * 8];
  __shared__ float aff[2 * CO];
  static_assert(sizeof(lds) + sizeof(aff) == (CO == 32 ? 121600 : 158720), "static LDS bytes");
  uint4* halo = lds;
  uint4* wl = lds + Halo::UNITS;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  stage_affine<CO>(aff, scale, shift);
  stage_weights<CO, 8, 512>(wl, wt);
  const int64_t ntiles = (int64_t)nimg * tiles_x * tiles_y;
  Halo pf;
  if ((int64_t)blockIdx.x < ntiles) pf.fetch(x, 32, blockIdx.x, tiles_x, tiles_y, nimg, h, w);
  const int r = lane & 31, hh = lane >> 5;

  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    __syncthreads();  // the previous tile's halo reads are done
    pf.stash(halo);
    __syncthreads();
    if (tile + gridDim.x < ntiles) pf.fetch(x, 32, tile + gridDim.x, tiles_x, tiles_y, nimg, h, w);  // overlaps the MFMAs
    const TileAt t = tile_at<F3_TH, C3_TW>(tile, tiles_x, tiles_y, nimg);
    const int oy = t.oy0 + wave;
    f32x16 acc[TMN][2];
    zero_acc(acc);
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int tap = kh * 3 + kw;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int ch = 2 * q + hh;  // chunk: ci 8q + 4hh .. +3
          f32x4 fa[TMN], fb[2];
#pragma unroll
          for (int i = 0; i < TMN; ++i) {
            const int n = i * 32 + r;
            fa[i] = *reinterpret_cast<const f32x4*>(wl + (tap * CO + n) * 8 + swz<8>(n, ch));
          }
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int col = j * 32 + r + kw;
            fb[j] = *reinterpret_cast<const f32x4*>(halo + ((wave + kh) * F3_HC + col) * 8 + swz<8>(col, ch));
          }
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int i = 0; i < TMN; ++i)
#pragma unroll
              for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][e], fb[j][e], acc[i][j], 0, 0, 0);
        }
      }
    if (oy < h) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int ox = t.ox0 + j * 32 + r;
        if (ox >= w) continue;
        float* yrow = y + (((int64_t)t.b * h + oy) * w + ox) * CO;
#pragma unroll
        for (int i = 0; i < TMN; ++i) epilogue_f32<CO>(acc[i][j], i * 32, hh, aff, yrow, act);
      }
    }
  }  // tiles
}

}  // namespace
}  // namespace sp

extern "C" int sp_conv3x3_c32(const float* x, const float* wt, const float* scale, const float* shift, float* y,
                              int n, int h, int w, int cout, int act, void* stream) {
  using namespace sp;
  SP_ARG_CHECK(x && wt && scale && shift && y && n > 0 && h > 0 && w > 0 && (cout == 32 || cout == 64) &&
                   (act == 0 || act == 1) && ((uintptr_t)x & 15) == 0 && ((uintptr_t)wt & 15) == 0 &&
                   ((uintptr_t)y & 15) == 0,
               "sp_conv3x3_c32: bad args (Cin 32, Cout 32 or 64, act none/relu, aligned dense fp32 rows)");
  const DirectGrid g = direct_grid<F3_TH, C3_TW>(n, h, w, g_num_cus);  // persistent: one per CU
  if (cout == 32)
    hipLaunchKernelGGL((conv3x3_c32_f32_kernel<32>), dim3(g.grid), dim3(512), 0, as_stream(stream), x, wt, scale,
                       shift, y, n, h, w, g.tiles_x, g.tiles_y, act);
  else
    hipLaunchKernelGGL((conv3x3_c32_f32_kernel<64>), dim3(g.grid), dim3(512), 0, as_stream(stream), x, wt, scale,
                       shift, y, n, h, w, g.tiles_x, g.tiles_y, act);
  return check_launch("sp_conv3x3_c32");
}

// ---------------------------------------------------------------------------------------------
// The stage-0 3×3 (Cin 64 → Cout 64) of the bf16 variant on bf16 rows, rows ldx / ldy elements apart (the fused
// bottleneck tail reads this output as a channel slice); the pipeline is direct3x3.h's.
// Tile: 16 rows × 32 pixels, one persistent workgroup per CU, eight waves, each two output rows × 32 pixels.
// Tiles are 32 pixels wide so the 160- / 320-pixel stage-0 maps tile exactly (64-wide tiles computed 192 columns
// of every 160). LDS: all 9·64·64 bf16 weights (73.7 KB), the (16 + 2) × (32 + 2) × 64 bf16 halo (78.3 KB), the
// affine. v_mfma_f32_32x32x16_bf16, the 576-deep k in (tap, 16-channel) order, as the implicit GEMM sums it.
// The residual (template RES) is read as 16-byte row pieces, once per tile, after the MFMAs: issued ahead of them
// its 32 more live VGPRs spill. At C3's shape (bs256 160², 0.48 TFLOP): 0.60 / 0.71 ms without / with the residual
// against 0.70 / 0.91 for 64-wide tiles with 8-byte epilogue accesses (profiles/r4/bf16/ab_c64_tw32.json).
namespace sp {
namespace {

constexpr int B6_TH = 16, B6_TW = 32, B6_HC = B6_TW + 2;

template <bool RES>
__global__ __launch_bounds__(512, 1) void conv3x3_c64_bf16_kernel(const uint16_t* __restrict__ x,
                                                                  const uint16_t* __restrict__ w16,
                                                                  const float* __restrict__ scale,
                                                                  const float* __restrict__ shift,
                                                                  uint16_t* __restrict__ y, int64_t ldx,
                                                                  int64_t ldy, const uint16_t* __restrict__ res,
                                                                  int64_t ldr, int nimg, int h, int w, int tiles_x,
                                                                  int tiles_y, int act) {
  using Halo = HaloPrefetch<512, B6_TH, B6_TW, 8, 8>;
  __shared__ uint4 lds[Halo::UNITS + 9 * 64 * 8];
  __shared__ float aff[128];
  static_assert(sizeof(lds) + sizeof(aff) == 152576, "static LDS bytes");
  uint4* halo = lds;
  uint4* wl = lds + Halo::UNITS;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  stage_weights<64, 8, 512>(wl, w16);
  stage_affine<64>(aff, scale, shift);
  const int64_t ntiles = (int64_t)nimg * tiles_x * tiles_y;
  Halo pf;
  if ((int64_t)blockIdx.x < ntiles) pf.fetch(x, ldx, blockIdx.x, tiles_x, tiles_y, nimg, h, w);
  const int r = lane & 31, hh = lane >> 5;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    __syncthreads();  // the previous tile's halo reads are done
    pf.stash(halo);
    __syncthreads();
    const TileAt t = tile_at<B6_TH, B6_TW>(tile, tiles_x, tiles_y, nimg);
    const int oy0 = t.oy0 + 2 * wave, ox = t.ox0 + r;
    int64_t pix[2];
    bool in[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      in[j] = oy0 + j < h && ox < w;
      pix[j] = in[j] ? ((int64_t)t.b * h + oy0 + j) * w + ox : 0;
      if (in[j]) SP_BCHECK(pix[j], (int64_t)nimg * h * w);
    }
    uint4 rq[2][2][2];  // [row j][channel half i][16-channel group p]: this lane's 8 residual channels
    auto fetch_res = [&]() {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int p = 0; p < 2; ++p)
            rq[j][i][p] = *reinterpret_cast<const uint4*>(res + pix[j] * ldr + i * 32 + 16 * p + 8 * hh);
    };
    if (tile + gridDim.x < ntiles)  // overlaps the MFMAs below
      pf.fetch(x, ldx, tile + gridDim.x, tiles_x, tiles_y, nimg, h, w);
    f32x16 acc[2][2];
    zero_acc(acc);
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int tap = kh * 3 + kw;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int ch = 2 * s + hh;  // k chunk: ci 16s + 8hh .. +7
          bf16x8 fa[2], fb[2];
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const int n = i * 32 + r;
            fa[i] = *reinterpret_cast<const bf16x8*>(wl + (tap * 64 + n) * 8 + swz<8>(n, ch));
          }
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int col = r + kw;
            fb[j] = *reinterpret_cast<const bf16x8*>(halo + ((2 * wave + j + kh) * B6_HC + col) * 8 + swz<8>(col, ch));
          }
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
      }
    if constexpr (RES) fetch_res();  // issued here, not ahead of the MFMAs: 32 more live VGPRs there spill
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      uint16_t* yrow = y + pix[j] * ldy;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          // accumulator element 4g + e of lane (r, hh) is channel i·32 + 8g + 4hh + e: swap the upper half's
          // g = 2p run with the lower half's g = 2p + 1 run, so lane hh holds channels base .. base + 7
          float v[8];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[i][j][8 * p + e]),
                                                             __float_as_uint(acc[i][j][8 * p + 4 + e]), false, false);
            v[e] = __uint_as_float(sw[0]);
            v[4 + e] = __uint_as_float(sw[1]);
          }
          const int base = i * 32 + 16 * p + 8 * hh;
          float rv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          if constexpr (RES) {  // pre-activation residual (the basic block's shortcut), bf16 rows
            const uint4 q = rq[j][i][p];
            const unsigned qq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              rv[2 * e] = __uint_as_float(qq[e] << 16);
              rv[2 * e + 1] = __uint_as_float(qq[e] & 0xffff0000u);
            }
          }
          unsigned pk[4];
#pragma unroll
          for (int e = 0; e < 8; e += 2) {
            float u0 = fmaf(v[e], aff[base + e], aff[64 + base + e]);
            float u1 = fmaf(v[e + 1], aff[base + e + 1], aff[64 + base + e + 1]);
            if constexpr (RES) {
              u0 += rv[e];
              u1 += rv[e + 1];
            }
            pk[e / 2] = cvt_pk_bf16(act ? fmaxf(u0, 0.f) : u0, act ? fmaxf(u1, 0.f) : u1);
          }
          if (in[j]) *reinterpret_cast<uint4*>(yrow + base) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
        }
    }
  }  // tiles
}

}  // namespace
}  // namespace sp

extern "C" int sp_conv3x3_c64_bf16(const uint16_t* x, int64_t ldx, const uint16_t* w16, const float* scale,
                                   const float* shift, uint16_t* y, int64_t ldy, const uint16_t* res, int64_t ldr,
                                   int n, int h, int w, int act, void* stream) {
  using namespace sp;
  SP_ARG_CHECK(x && w16 && scale && shift && y && n > 0 && h > 0 && w > 0 && (act == 0 || act == 1) &&
                   ldx >= 64 && ldy >= 64 && ldx % 8 == 0 && ldy % 8 == 0 && ((uintptr_t)x & 15) == 0 &&
                   ((uintptr_t)w16 & 15) == 0 && ((uintptr_t)y & 15) == 0 &&
                   (!res || (ldr >= 64 && ldr % 8 == 0 && ((uintptr_t)res & 15) == 0)),
               "sp_conv3x3_c64_bf16: bad args (act none/relu, 16-byte aligned bf16 rows, ld % 8, ld >= 64)");
  const DirectGrid g = direct_grid<B6_TH, B6_TW>(n, h, w, g_num_cus);  // persistent: one per CU
  if (res)
    hipLaunchKernelGGL(conv3x3_c64_bf16_kernel<true>, dim3(g.grid), dim3(512), 0, as_stream(stream), x, w16, scale,
                       shift, y, ldx, ldy, res, ldr, n, h, w, g.tiles_x, g.tiles_y, act);
  else
    hipLaunchKernelGGL(conv3x3_c64_bf16_kernel<false>, dim3(g.grid), dim3(512), 0, as_stream(stream), x, w16, scale,
                       shift, y, ldx, ldy, res, ldr, n, h, w, g.tiles_x, g.tiles_y, act);
  return check_launch("sp_conv3x3_c64_bf16");
}
