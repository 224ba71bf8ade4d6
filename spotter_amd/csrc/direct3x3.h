// The pipeline the direct 3×3 stride-1 pad-1 kernels share (stem.hip: conv3x3_c32_bf16 / conv3x3_c32_f32 /
// conv3x3_c64_bf16; direct_x3.hip: conv3x3_x3). A persistent workgroup walks TH × TW output tiles. Per tile it
// holds the input halo, (TH + 2) × (TW + 2) pixels, in LDS as rows of 16-byte chunks, swizzled so a 16-lane
// group's b128 reads of 16 consecutive pixels (or weight rows) cover all 64 banks; the next tile's halo is
// fetched into registers while the MFMAs of this one run and is stashed after the barrier that ends them.
// The MFMAs run with the roles transposed (A = weights [Cout × k], B = pixels [k × 32]), so lane (r, hh) of a
// v_mfma_f32_32x32x* block holds channels 8g + 4hh .. +3 of pixel r in accumulator elements 4g .. 4g + 3: the
// epilogues start from that layout.
#pragma once

#include "conv_common.h"

namespace sp {
namespace {

// LDS slot of 16-byte chunk `chunk` in a row of CPP chunks (a halo pixel, a weight row), by the row's index.
template <int CPP>
__host__ __device__ constexpr int swz(int row, int chunk) {
  static_assert(CPP == 4 || CPP == 8, "chunks per row");
  return CPP == 8 ? chunk ^ ((row >> 1) & 7) : chunk ^ ((row >> 2) & 3);
}
template <int CPP>
constexpr bool swz_permutes() {
  for (int row = 0; row < 16; ++row) {
    unsigned seen = 0;
    for (int c = 0; c < CPP; ++c) seen |= 1u << swz<CPP>(row, c);
    if (seen != (1u << CPP) - 1) return false;
  }
  return true;
}
static_assert(swz_permutes<4>() && swz_permutes<8>(), "swz permutes the chunks of a row, for every row 0..15");

// Tile t of the persistent walk, x fastest: its image and the first output row / pixel.
struct TileAt {
  int b, oy0, ox0;
};
template <int TH, int TW>
__device__ __forceinline__ TileAt tile_at(int64_t t, int tiles_x, int tiles_y, int nimg) {
  const int tx = (int)(t % tiles_x);
  t /= tiles_x;
  const int ty = (int)(t % tiles_y);
  const int b = (int)(t / tiles_y);
  SP_BCHECK(b, nimg);
  return {b, ty * TH, tx * TW};
}

// The register prefetch of a tile's halo (rows oy0-1 .. oy0+TH, pixels ox0-1 .. ox0+TW; zero outside the map)
// by NT threads. A unit is what one thread moves at a time: REGS 16-byte registers of EPC elements each, CPP
// units per pixel; thread t holds units t, t + NT, ... The loads are unconditional (out-of-map units read x[0]
// and are zeroed at the stash), so nothing waits for them before the MFMAs that follow the fetch.
template <int NT, int TH, int TW, int CPP, int EPC, int REGS = 1>
struct HaloPrefetch {
  static constexpr int HC = TW + 2;
  static constexpr int UNITS = (TH + 2) * HC * CPP;
  static constexpr int PFN = (UNITS + NT - 1) / NT;  // units per thread
  static_assert(PFN <= 32, "one bit of okm per unit");
  uint4 pf[PFN][REGS];
  unsigned okm = 0;  // bit k: unit k is inside the map

  static __device__ __forceinline__ int unit(int k) { return threadIdx.x + k * NT; }
  __device__ __forceinline__ bool in_map(int k) const { return (okm >> k) & 1u; }
  // LDS slot of unit i (< UNITS) in a halo image of CPP chunks per pixel
  static __device__ __forceinline__ int slot(int i) {
    const int c = i % CPP, rc = i / CPP, col = rc % HC;
    return rc * CPP + swz<CPP>(col, c);
  }

  // rows of x are ld elements apart and hold CPP · REGS · EPC channels
  template <typename T>
  __device__ __forceinline__ void fetch(const T* __restrict__ x, int64_t ld, int64_t tile, int tiles_x, int tiles_y,
                                        int nimg, int h, int w) {
    static_assert(sizeof(T) * EPC == 16, "a register is 16 bytes");
    const TileAt t = tile_at<TH, TW>(tile, tiles_x, tiles_y, nimg);
#pragma unroll
    for (int k = 0; k < PFN; ++k) {
      const int i = unit(k);
      const int c = i % CPP, rc = i / CPP, r = rc / HC, col = rc - r * HC;
      const int iy = t.oy0 - 1 + r, ix = t.ox0 - 1 + col;
      const bool ok = i < UNITS && (unsigned)iy < (unsigned)h && (unsigned)ix < (unsigned)w;
      const int64_t off = ok ? (((int64_t)t.b * h + iy) * w + ix) * ld + c * (REGS * EPC) : 0;
      SP_BCHECK(off + REGS * EPC - 1, ((int64_t)nimg * h * w - 1) * ld + CPP * REGS * EPC);
#pragma unroll
      for (int q = 0; q < REGS; ++q) pf[k][q] = *reinterpret_cast<const uint4*>(x + off + q * EPC);
      okm = k == 0 ? (unsigned)ok : (okm | ((unsigned)ok << k));
    }
  }

  __device__ __forceinline__ void stash(uint4* halo) const {
    static_assert(REGS == 1, "a unit is one LDS chunk");
#pragma unroll
    for (int k = 0; k < PFN; ++k) {
      const int i = unit(k);
      if (i < UNITS) halo[slot(i)] = in_map(k) ? pf[k][0] : make_uint4(0u, 0u, 0u, 0u);
    }
  }
};

// All weights of a conv, global [CO][9 taps][CPP chunks] (the packed [Cout][K] form) → LDS [tap][n][swz(n, chunk)],
// once per workgroup of NT threads.
template <int CO, int CPP, int NT>
__device__ __forceinline__ void stage_weights(uint4* wl, const void* __restrict__ wt) {
  for (int i = threadIdx.x; i < 9 * CO * CPP; i += NT) {
    const int c = i % CPP, tn = i / CPP, n = tn / 9, tap = tn - n * 9;
    wl[(tap * CO + n) * CPP + swz<CPP>(n, c)] = static_cast<const uint4*>(wt)[i];
  }
}

// The BN affine → LDS [scale | shift]: per-tile global loads of it would wait behind the halo prefetch.
template <int CO>
__device__ __forceinline__ void stage_affine(float* aff, const float* __restrict__ scale,
                                             const float* __restrict__ shift) {
  if (threadIdx.x < CO) {
    aff[threadIdx.x] = scale[threadIdx.x];
    aff[CO + threadIdx.x] = shift[threadIdx.x];
  }
}

// fp32 epilogue of one accumulator block (channels n0 .. n0 + 31 of the pixel whose row is yrow):
// fmaf(acc, scale, shift), act, stored as float4 runs.
template <int CO>
__device__ __forceinline__ void epilogue_f32(const f32x16& acc, int n0, int hh, const float* aff,
                                             float* __restrict__ yrow, int act) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int n = n0 + 8 * g + 4 * hh;
    float4 v;
    float* vv = &v.x;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float u = fmaf(acc[4 * g + e], aff[n + e], aff[CO + n + e]);
      vv[e] = act ? fmaxf(u, 0.f) : u;
    }
    *reinterpret_cast<float4*>(yrow + n) = v;
  }
}

// Host: the tile counts of an n × h × w map and the persistent grid, min(tiles, cap) workgroups.
struct DirectGrid {
  int tiles_x, tiles_y;
  unsigned grid;
};
template <int TH, int TW>
inline DirectGrid direct_grid(int n, int h, int w, int64_t cap) {
  const int tiles_x = (w + TW - 1) / TW, tiles_y = (h + TH - 1) / TH;
  const int64_t tiles = (int64_t)n * tiles_x * tiles_y;
  return {tiles_x, tiles_y, (unsigned)(tiles < cap ? tiles : cap)};
}

}  // namespace
}  // namespace sp
