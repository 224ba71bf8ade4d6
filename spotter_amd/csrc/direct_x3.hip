// The fp32 path's thin 3×3 stride-1 pad-1 convs (Cin 32 → 32 / 64: stem convs 2 and 3; Cin 64 → 64: the
// stage-0 bottleneck 3×3) as direct LDS-halo convolutions on the 3-way bf16 split (ABI v17): fp32 rows in,
// fp32 rows out, bit-identical to the x3 implicit GEMM (conv_glds.h) on the same operands.
//
// As an implicit GEMM the Cin-64 conv fetches every activation row nine times from L2 and splits every A
// fragment once per tap and wave. Here one persistent workgroup per CU (eight waves) walks 8-row × 32-pixel
// output tiles. The next tile's fp32 halo ((8 + 2) × (32 + 2) pixels × Cin) is fetched into registers during
// the MFMAs; at the stash it is split ONCE into hi / mid / lo bf16 (split_frag_pk's RNE chain) and written as
// three plane images (rows of Cin bf16, 16-byte chunks swizzled for conflict-free ds_read_b128). The weights are
// the packed hi / mid / lo planes [3][Cout][9·Cin] (ops.split_bf16x3_host). They do not fit beside the halo at
// Cin 64 (221 KB), so they stream from their L2-resident planes by LDS-DMA in stages of 32 k (one tap's half
// at Cin 64: 3 · Cout · 64 B) through a two-stage ring that runs on across tiles; the Cin 32 → 32 weights
// (55 KB) stay resident. LDS: Cin 64: 130,560 B halo + 2 × 12,288 B ring; Cin 32 → 64: 65,280 + 24,576;
// Cin 32 → 32: 65,280 + 55,296 resident.
// Wave v computes output row v of the tile: 32 pixels × Cout with the roles transposed (A = weights, B =
// pixels) on v_mfma_f32_32x32x16_bf16. Sums run in (tap, 16-channel step) order with the six products of
// mfma_planes<3> in its (activation plane, weight plane) sequence lo·hi, hi·lo, mid·mid, mid·hi, hi·mid, hi·hi;
// the epilogue is epilogue_vec's fmaf(acc, scale, shift) then act, stored as float4 runs.
#include "direct3x3.h"
#include "mfma16_common.h"

namespace sp {
namespace {

constexpr int DX_TH = 8, DX_TW = 32, DX_HC = DX_TW + 2;

// RES: all weight stages resident in LDS (loaded once per workgroup) instead of the two-stage ring.
template <int CIN, int CO, bool RES>
__global__ __launch_bounds__(512, 1) void conv3x3_x3_kernel(const float* __restrict__ x,
                                                            const uint16_t* __restrict__ wp, int64_t wps,
                                                            const float* __restrict__ scale,
                                                            const float* __restrict__ shift, float* __restrict__ y,
                                                            int64_t ldx, int64_t ldy, int nimg, int h, int w,
                                                            int tiles_x, int tiles_y, int act) {
  constexpr int CPP = CIN / 8;           // 16-byte chunks per pixel per plane
  using Halo = HaloPrefetch<512, DX_TH, DX_TW, CPP, 4, 2>;  // a unit: 8 fp32 in, one chunk of each plane out
  constexpr int PLANE = Halo::UNITS;     // chunks of one halo plane
  constexpr int SPT = CIN / 32;          // weight stages (32 k each) per tap
  constexpr int NST = 9 * SPT;
  constexpr int WPL = CO * 4;            // chunks of one weight plane of a stage
  constexpr int WST = 3 * WPL;           // chunks of a stage
  constexpr int NBUF = RES ? NST : 2;
  constexpr int WDMA = WST / 64;         // wave-wide DMAs per stage
  constexpr int TMN = CO / 32;
  __shared__ uint4 lds[3 * PLANE + NBUF * WST];
  __shared__ float aff[2 * CO];
  static_assert(sizeof(lds) + sizeof(aff) == (CIN == 64 ? 155648 : RES ? 120832 : 90368), "static LDS bytes");
  uint4* halo = lds;
  uint4* wl = lds + 3 * PLANE;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  stage_affine<CO>(aff, scale, shift);
  // weight stage st (k = 32·st .. +31 of every Cout row, three planes) → ring slot buf: LDS [plane][n][4 chunks],
  // position q of row n holds global chunk q ^ ((n >> 2) & 3) = swz<4>(n, q) (the DMA destination is lane-linear)
  const uint32_t wl0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint4*)wl;
  auto issue_w = [&](int st, int buf) {
#pragma unroll
    for (int jj = 0; jj < (WDMA + 7) / 8; ++jj) {
      const int j = wave + 8 * jj;
      if (j < WDMA) {
        const int idx = j * 64 + lane;
        const int pl = idx / WPL, rem = idx - pl * WPL, n = rem >> 2, q = rem & 3;
        const int64_t off = pl * wps + (int64_t)n * (9 * CIN) + st * 32 + ((q ^ ((n >> 2) & 3)) * 8);
        SP_BCHECK(off + 7, 3 * wps);
        glds16(wp + off, wl0 + (uint32_t)((buf * WST + j * 64) * 16));
      }
    }
  };
  const int64_t ntiles = (int64_t)nimg * tiles_x * tiles_y;
  Halo pf;
  // Halo::fetch written out: through the shared function this kernel's wait counts change and its Cin-64
  // instance spills 28 bytes for 24 (profiles/direct_share/README.md)
  auto fetch = [&](int64_t t) {
    const int tx = (int)(t % tiles_x);
    t /= tiles_x;
    const int ty = (int)(t % tiles_y);
    const int b = (int)(t / tiles_y);
    SP_BCHECK(b, nimg);
    const int oy0 = ty * DX_TH, ox0 = tx * DX_TW;
#pragma unroll
    for (int k = 0; k < Halo::PFN; ++k) {
      const int i = tid + k * 512;
      const int c = i % CPP, rc = i / CPP, r = rc / DX_HC, col = rc - r * DX_HC;
      const int iy = oy0 - 1 + r, ix = ox0 - 1 + col;
      const bool ok = i < PLANE && (unsigned)iy < (unsigned)h && (unsigned)ix < (unsigned)w;
      const int64_t off = ok ? (((int64_t)b * h + iy) * w + ix) * ldx + c * 8 : 0;
      SP_BCHECK(off + 7, ((int64_t)nimg * h * w - 1) * ldx + CIN);
      pf.pf[k][0] = *reinterpret_cast<const uint4*>(x + off);
      pf.pf[k][1] = *reinterpret_cast<const uint4*>(x + off + 4);
      pf.okm = k == 0 ? (unsigned)ok : (pf.okm | ((unsigned)ok << k));
    }
  };
  // split each fetched unit once (hi / mid / lo, RNE) into the three plane images
  auto stash = [&]() {
#pragma unroll
    for (int k = 0; k < Halo::PFN; ++k) {
      const int i = Halo::unit(k);
      if (i < PLANE) {
        const uint4 z = make_uint4(0u, 0u, 0u, 0u);
        bf16x8 pl[3];
        split_frag_pk<3>(__builtin_bit_cast(float4, pf.in_map(k) ? pf.pf[k][0] : z),
                         __builtin_bit_cast(float4, pf.in_map(k) ? pf.pf[k][1] : z), pl);
        const int pos = Halo::slot(i);
#pragma unroll
        for (int q = 0; q < 3; ++q) halo[q * PLANE + pos] = __builtin_bit_cast(uint4, pl[q]);
      }
    }
  };
  if constexpr (RES) {
#pragma unroll
    for (int st = 0; st < NST; ++st) issue_w(st, st);
  } else {
    issue_w(0, 0);
  }
  if ((int64_t)blockIdx.x < ntiles) fetch(blockIdx.x);
  const int r = lane & 31, hh = lane >> 5;
  int par = 0;  // ring slot of this tile's stage 0 (NST is odd at Cin 32)

  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    __syncthreads();  // the previous tile's halo reads are done
    stash();
    const TileAt t = tile_at<DX_TH, DX_TW>(tile, tiles_x, tiles_y, nimg);
    const int oy = t.oy0 + wave, ox = t.ox0 + r;
    f32x16 acc[TMN];
    zero_acc(acc);
#pragma unroll
    for (int st = 0; st < NST; ++st) {
      const int buf = RES ? st : (st + par) & 1;
      if (!RES || st == 0) {
        wait_vmcnt<0>();   // this wave's DMA pieces of stage st have landed ...
        __syncthreads();   // ... and everyone's; the other slot's (and, at stage 0, the old halo's) readers are done
      }
      if constexpr (!RES) issue_w(st + 1 < NST ? st + 1 : 0, buf ^ 1);  // the ring runs on into the next tile
      if (st == 0 && tile + gridDim.x < ntiles) fetch(tile + gridDim.x);  // overlaps the MFMAs below
      const int tap = st / SPT, cq = st - tap * SPT, kh = tap / 3, kw = tap - 3 * kh;
      const uint4* wb = wl + buf * WST;
      const int col = r + kw;
      const uint4* hp = halo + ((wave + kh) * DX_HC + col) * CPP;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const int chw = 2 * s2 + hh;  // k chunk of the stage: channels 32cq + 16s2 + 8hh .. +7
        bf16x8 xa[3], wf[TMN][3];
#pragma unroll
        for (int q = 0; q < 3; ++q)
          xa[q] = *reinterpret_cast<const bf16x8*>(hp + q * PLANE + swz<CPP>(col, cq * 4 + chw));
#pragma unroll
        for (int i = 0; i < TMN; ++i) {
          const int n = i * 32 + r;
#pragma unroll
          for (int q = 0; q < 3; ++q)
            wf[i][q] = *reinterpret_cast<const bf16x8*>(wb + q * WPL + n * 4 + swz<4>(n, chw));
        }
#pragma unroll
        for (int i = 0; i < TMN; ++i) {
          // mfma_planes<3>'s sequence in (activation, weight) plane pairs, the weights as the first operand
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[i][0], xa[2], acc[i], 0, 0, 0);
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[i][2], xa[0], acc[i], 0, 0, 0);
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[i][1], xa[1], acc[i], 0, 0, 0);
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[i][0], xa[1], acc[i], 0, 0, 0);
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[i][1], xa[0], acc[i], 0, 0, 0);
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[i][0], xa[0], acc[i], 0, 0, 0);
        }
      }
    }
    if constexpr (!RES) par = (par + NST) & 1;
    if (oy < h && ox < w) {
      const int64_t pix = ((int64_t)t.b * h + oy) * w + ox;
      SP_BCHECK(pix, (int64_t)nimg * h * w);
      float* yrow = y + pix * ldy;
#pragma unroll
      for (int i = 0; i < TMN; ++i) epilogue_f32<CO>(acc[i], i * 32, hh, aff, yrow, act);
    }
  }  // tiles
  wait_vmcnt<0>();  // the ring's last DMA (issued for a tile that does not come) lands before the LDS is released
}

template <int CIN, int CO, bool RES>
int dx_launch(const char* what, const float* x, int64_t ldx, const uint16_t* wp, int64_t wps, const float* scale,
              const float* shift, float* y, int64_t ldy, int n, int h, int w, int act, void* stream) {
  const DirectGrid g = direct_grid<DX_TH, DX_TW>(n, h, w, g_num_cus);  // persistent: one per CU
  hipLaunchKernelGGL((conv3x3_x3_kernel<CIN, CO, RES>), dim3(g.grid), dim3(512), 0, as_stream(stream), x, wp, wps,
                     scale, shift, y, ldx, ldy, n, h, w, g.tiles_x, g.tiles_y, act);
  return check_launch(what);
}

}  // namespace
}  // namespace sp

extern "C" int sp_conv3x3_c64_x3(const float* x, int64_t ldx, const uint16_t* w_planes, int64_t plane_stride,
                                 const float* scale, const float* shift, float* y, int64_t ldy, int n, int h, int w,
                                 int act, void* stream) {
  using namespace sp;
  SP_ARG_CHECK(x && w_planes && scale && shift && y && n > 0 && h > 0 && w > 0 && (act == 0 || act == 1) &&
                   ldx >= 64 && ldy >= 64 && ldx % 4 == 0 && ldy % 4 == 0 && plane_stride >= 64 * 576 &&
                   plane_stride % 8 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)w_planes & 15) == 0 &&
                   ((uintptr_t)y & 15) == 0,
               "sp_conv3x3_c64_x3: bad args (act none/relu, 16-byte aligned fp32 rows, ld % 4, ld >= 64, planes [3][64][576])");
  return dx_launch<64, 64, false>("sp_conv3x3_c64_x3", x, ldx, w_planes, plane_stride, scale, shift, y, ldy, n, h, w,
                                  act, stream);
}

extern "C" int sp_conv3x3_c32_x3(const float* x, const uint16_t* w_planes, int64_t plane_stride, const float* scale,
                                 const float* shift, float* y, int n, int h, int w, int cout, int act, void* stream) {
  using namespace sp;
  SP_ARG_CHECK(x && w_planes && scale && shift && y && n > 0 && h > 0 && w > 0 && (cout == 32 || cout == 64) &&
                   (act == 0 || act == 1) && plane_stride >= (int64_t)cout * 288 && plane_stride % 8 == 0 &&
                   ((uintptr_t)x & 15) == 0 && ((uintptr_t)w_planes & 15) == 0 && ((uintptr_t)y & 15) == 0,
               "sp_conv3x3_c32_x3: bad args (Cin 32, Cout 32 or 64, act none/relu, aligned dense fp32 rows, planes [3][Cout][288])");
  if (cout == 32)
    return dx_launch<32, 32, true>("sp_conv3x3_c32_x3", x, 32, w_planes, plane_stride, scale, shift, y, 32, n, h, w, act,
                                   stream);
  return dx_launch<32, 64, false>("sp_conv3x3_c32_x3", x, 32, w_planes, plane_stride, scale, shift, y, 64, n, h, w, act,
                                  stream);
}
