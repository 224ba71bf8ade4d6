// Fused preprocess: PIL-exact BILINEAR resize + rescale(1/255) + HWC→CHW.
//
// Restates RTDetrImageProcessorPil._preprocess (IPP:451-462): Pillow's
// ImagingResample (Resample.c) — separable triangle filter, support
// max(in/out, 1), 22-bit fixed-point coefficients, horizontal pass first over
// the source rows the vertical pass needs, clip8 after each pass — then
// f32(f64(u8) * (1/255)) (IT:118-122) and channel-first packing. Bit-exact.
//
// One workgroup produces a band of T output rows of one image: it runs the
// horizontal pass for exactly the source rows that band needs into LDS (u8),
// then the vertical pass + rescale + NCHW store (coalesced along x). The
// coefficient tables are computed on the host with Pillow's double-precision
// recipe and cached on the device per (in, out) size.
#include <algorithm>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "common.h"

namespace sp {
namespace {

constexpr int kPrecisionBits = 32 - 8 - 2;
constexpr int kLdsBytes = 48 * 1024;
constexpr int kMaxImgs = 32;

struct Coeffs {
  int ksize = 0;
  int* d_bounds = nullptr;  // [out][2] (xmin, n)
  int* d_k = nullptr;       // [out][ksize]
  std::vector<int> h_bounds;
};

std::mutex g_mu;
std::map<std::pair<int, int>, Coeffs> g_cache;
const Coeffs c_failed;

// Resample.c precompute_coeffs + normalize_coeffs_8bpc for the bilinear filter.
void precompute(int in_size, int out_size, Coeffs& c) {
  const double scale = (double)in_size / out_size;
  double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  const int ksize = (int)__builtin_ceil(support) * 2 + 1;
  std::vector<int> bounds(out_size * 2), kk((size_t)out_size * ksize, 0);
  std::vector<double> w(ksize);
  const double ss = 1.0 / filterscale;
  for (int xx = 0; xx < out_size; ++xx) {
    volatile double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
      volatile double t = (x + xmin - center + 0.5) * ss;
      double a = t < 0.0 ? -t : t;
      double f = a < 1.0 ? 1.0 - a : 0.0;
      w[x] = f;
      ww += f;
    }
    for (int x = 0; x < xmax; ++x) {
      double k = ww != 0.0 ? w[x] / ww : w[x];
      kk[(size_t)xx * ksize + x] =
          k < 0 ? (int)(-0.5 + k * (1 << kPrecisionBits)) : (int)(0.5 + k * (1 << kPrecisionBits));
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
  }
  c.ksize = ksize;
  c.h_bounds = bounds;
  if (hipMalloc(&c.d_bounds, bounds.size() * sizeof(int)) != hipSuccess ||
      hipMalloc(&c.d_k, kk.size() * sizeof(int)) != hipSuccess ||
      hipMemcpy(c.d_bounds, bounds.data(), bounds.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(c.d_k, kk.data(), kk.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
    if (c.d_bounds) hipFree(c.d_bounds);
    if (c.d_k) hipFree(c.d_k);
    c.d_bounds = nullptr;
    c.d_k = nullptr;
  }
}

const Coeffs* get_coeffs(int in_size, int out_size) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto key = std::make_pair(in_size, out_size);
  auto it = g_cache.find(key);
  if (it != g_cache.end()) return &it->second;
  Coeffs c;
  precompute(in_size, out_size, c);
  if (!c.d_k) return &c_failed;  // not cached: the next call retries the upload
  return &(g_cache[key] = std::move(c));
}

struct PreImg {
  const uint8_t* src;
  int h, w, stride;
  const int* hb;
  const int* hk;
  int ksh;
  const int* vb;
  const int* vk;
  int ksv;
  int rows_per_tile;
  int ntiles;
  float* out;
};

struct PreArgs {
  PreImg img[kMaxImgs];
  int out_h, out_w;
  int vec4;  // out_w % 4 == 0 and a 16-byte aligned output: the vertical pass stores float4s
};

__device__ __forceinline__ int clip8(int acc) {
  int v = acc >> kPrecisionBits;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// Thread mapping: every pass walks output columns with the threads and rows with a loop, so the
// per-column coefficients are loaded once and reused down the band (no index divisions).
// MAXT > 0: every image of the launch has at most MAXT horizontal taps; the column's coefficients sit
// in registers and all 3·MAXT source bytes of a row are loaded at once (taps past n are predicated
// off and weigh 0, so the integer sums are unchanged). MAXT = 0: generic tap loop.
// The u8 band buffer is dynamic LDS sized to the launch's tallest band (a 10-row band of a 640-wide
// output needs 21 KB, not the 48 KB cap), so more workgroups share a CU and hide the byte-load latency.
// Column tiles (round 6): a workgroup covers a band of T output rows × kColTile output columns (one column per
// thread), so the LDS band holds rows × kColTile × 3 bytes instead of whole output rows and the grid has
// bands × column tiles workgroups per image: a 4K source resized to 1280² is 400 workgroups of ~30 source rows
// instead of 256 whole-width bands, each thread's chain of row loads 5× shorter.
constexpr int kColTile = 256;

// dword window of a thread's source bytes [p, p + 3·MAXT): NW aligned dwords from p & ~3 (clamped to the image's
// last dword, whose bytes only feed taps of weight 0), re-aligned with v_alignbyte so byte b of the window is
// bits 8(b & 3) of word b >> 2. Taps past the column's n weigh 0, so the integer sums are Pillow's.
template <int MAXT>
struct Window {
  static constexpr int NW = (3 * MAXT + 6) / 4;
  uint32_t w[NW];
  __device__ __forceinline__ void load(const uint8_t* p, uintptr_t last) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uintptr_t base = a & ~uintptr_t(3);
    const uint32_t sh = (uint32_t)(a & 3);
    uint32_t d[NW + 1];
#pragma unroll
    for (int k = 0; k <= NW; ++k) {
      uintptr_t q = base + 4 * k;
      q = q > last ? last : q;
      d[k] = *reinterpret_cast<const uint32_t*>(q);
    }
#pragma unroll
    for (int k = 0; k < NW; ++k) w[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
  }
  __device__ __forceinline__ int byte(int b) const { return (int)((w[b >> 2] >> (8 * (b & 3))) & 255u); }
};

// Thread mapping: every pass walks output columns with the threads and rows with a loop, so the
// per-column coefficients are loaded once and reused down the band (no index divisions).
// MAXT > 0: every image of the launch has at most MAXT horizontal taps; the column's coefficients sit
// in registers and its 3·MAXT source bytes of a row arrive as one dword window (taps past n weigh 0, so the
// integer sums are unchanged). MAXT = 0: generic tap loop with byte loads.
// The u8 band buffer is dynamic LDS sized to the launch's tallest band.
template <int MAXT>
__global__ __launch_bounds__(256) void preprocess_kernel(const PreArgs a) {
  extern __shared__ uint8_t tmp[];
  __shared__ float lut[256];
  const PreImg& im = a.img[blockIdx.y];
  const int ow = a.out_w, oh = a.out_h;
  const int ncol = (ow + kColTile - 1) / kColTile;
  const int tile = blockIdx.x / ncol;
  const int x0 = (blockIdx.x - tile * ncol) * kColTile;
  if (tile >= im.ntiles) return;
  // rescale table: f32(f64(v) * (1/255)), exactly IT:118-122's arithmetic
  lut[threadIdx.x] = (float)((double)threadIdx.x * (1.0 / 255.0));
  const int cw = min(kColTile, ow - x0);
  const int y0 = tile * im.rows_per_tile;
  const int y1 = min(y0 + im.rows_per_tile, oh);
  const int r0 = im.vb[2 * y0];
  const int r1 = im.vb[2 * (y1 - 1)] + im.vb[2 * (y1 - 1) + 1];
  const int row_elems = cw * 3;
  // the band's source rows lie inside the image (and the LDS band was sized for them on the host)
  SP_BCHECK(r0, im.h);
  SP_BCHECK(r1 - 1, im.h);
  // horizontal pass: source rows [r0, r1) → tmp [row][x - x0][c] (u8)
  const int xx = x0 + (int)threadIdx.x;
  if (threadIdx.x < cw) {
    const int xmin = im.hb[2 * xx];
    const int n = im.hb[2 * xx + 1];
    SP_BCHECK(xmin + n - 1, im.w);
    uint8_t* t = tmp + threadIdx.x * 3;
    if constexpr (MAXT > 0) {
      SP_BCHECK(n, MAXT + 1);
      int kr[MAXT];
#pragma unroll
      for (int j = 0; j < MAXT; ++j) kr[j] = j < n ? im.hk[xx * im.ksh + j] : 0;
      const uint8_t* s = im.src + (int64_t)r0 * im.stride + xmin * 3;
      const uintptr_t last = (reinterpret_cast<uintptr_t>(im.src + (int64_t)(im.h - 1) * im.stride + 3 * im.w - 1)) &
                             ~uintptr_t(3);
      // groups of RG rows: every row's window loads are issued before any of them is used
      constexpr int RG = 4;
      auto row_out = [&](const Window<MAXT>& win, uint8_t* tt) {
        int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
#pragma unroll
        for (int j = 0; j < MAXT; ++j) {
          a0 += win.byte(3 * j) * kr[j];
          a1 += win.byte(3 * j + 1) * kr[j];
          a2 += win.byte(3 * j + 2) * kr[j];
        }
        tt[0] = (uint8_t)clip8(a0);
        tt[1] = (uint8_t)clip8(a1);
        tt[2] = (uint8_t)clip8(a2);
      };
      int rr = r0;
      for (; rr + RG <= r1; rr += RG, s += RG * (int64_t)im.stride, t += RG * row_elems) {
        Window<MAXT> win[RG];
#pragma unroll
        for (int g = 0; g < RG; ++g) win[g].load(s + g * (int64_t)im.stride, last);
#pragma unroll
        for (int g = 0; g < RG; ++g) row_out(win[g], t + g * row_elems);
      }
      for (; rr < r1; ++rr, s += im.stride, t += row_elems) {
        Window<MAXT> win;
        win.load(s, last);
        row_out(win, t);
      }
    } else {
      SP_BCHECK(n, im.ksh + 1);
      const int* k = im.hk + xx * im.ksh;
      const uint8_t* s = im.src + (int64_t)r0 * im.stride + xmin * 3;
#pragma unroll 4
      for (int rr = r0; rr < r1; ++rr, s += im.stride, t += row_elems) {
        int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
        for (int j = 0; j < n; ++j) {
          const int kj = k[j];
          a0 += (int)s[3 * j] * kj;
          a1 += (int)s[3 * j + 1] * kj;
          a2 += (int)s[3 * j + 2] * kj;
        }
        t[0] = (uint8_t)clip8(a0);
        t[1] = (uint8_t)clip8(a1);
        t[2] = (uint8_t)clip8(a2);
      }
    }
  }
  __syncthreads();
  // vertical pass + rescale + CHW store (coalesced along x in each plane)
  const int64_t plane = (int64_t)oh * ow;
  if (a.vec4) {
    // four adjacent columns per thread (12 band bytes = 3 aligned LDS dwords per tap), float4 stores per plane;
    // the four 64-thread groups take every fourth output row. Same integer sums: bit-identical.
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int xl = 4 * tx;
    if (xl >= cw) return;
    float* ob = im.out + x0 + xl;
    for (int yy = y0 + ty; yy < y1; yy += 4) {
      const int ymin = im.vb[2 * yy] - r0;
      const int n = im.vb[2 * yy + 1];
      SP_BCHECK(ymin, r1 - r0);
      SP_BCHECK(ymin + n - 1, r1 - r0);
      const int* k = im.vk + yy * im.ksv;
      const uint32_t* tp = reinterpret_cast<const uint32_t*>(tmp + ymin * row_elems + xl * 3);
      int acc[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) acc[i] = 1 << (kPrecisionBits - 1);
      for (int j = 0; j < n; ++j, tp += row_elems / 4) {
        const int kj = k[j];
        const uint32_t u[3] = {tp[0], tp[1], tp[2]};
#pragma unroll
        for (int i = 0; i < 12; ++i) acc[i] += (int)((u[i >> 2] >> (8 * (i & 3))) & 255u) * kj;
      }
      float* o = ob + (int64_t)yy * ow;
#pragma unroll
      for (int c = 0; c < 3; ++c)
        *reinterpret_cast<float4*>(o + c * plane) = make_float4(lut[clip8(acc[c])], lut[clip8(acc[3 + c])],
                                                                lut[clip8(acc[6 + c])], lut[clip8(acc[9 + c])]);
    }
    return;
  }
  if (threadIdx.x >= cw) return;
  float* o = im.out + (int64_t)y0 * ow + xx;
#pragma unroll 4
  for (int yy = y0; yy < y1; ++yy, o += ow) {
    const int ymin = im.vb[2 * yy] - r0;
    const int n = im.vb[2 * yy + 1];
    SP_BCHECK(ymin, r1 - r0);  // the vertical taps read rows of this band's LDS buffer
    SP_BCHECK(ymin + n - 1, r1 - r0);
    const int* k = im.vk + yy * im.ksv;
    const uint8_t* t = tmp + ymin * row_elems + threadIdx.x * 3;
    int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
    for (int j = 0; j < n; ++j, t += row_elems) {
      const int kj = k[j];
      a0 += (int)t[0] * kj;
      a1 += (int)t[1] * kj;
      a2 += (int)t[2] * kj;
    }
    o[0] = lut[clip8(a0)];
    o[plane] = lut[clip8(a1)];
    o[2 * plane] = lut[clip8(a2)];
  }
}

// Same-size sources (h, w) == (out_h, out_w): Pillow's resize returns the image unchanged (and the
// BILINEAR coefficients are the identity: one tap of weight 2^22), so the whole op is the rescale LUT
// and the HWC → CHW scatter. One thread per 4 pixels of a row: three aligned 4-byte loads, one
// float4 store per plane.
__global__ __launch_bounds__(256) void preprocess_same_size_kernel(const PreArgs a) {
  __shared__ float lut[256];
  lut[threadIdx.x] = (float)((double)threadIdx.x * (1.0 / 255.0));
  __syncthreads();
  const PreImg& im = a.img[blockIdx.y];
  const int ow = a.out_w, oh = a.out_h;
  const int q4 = ow >> 2;
  const int64_t plane = (int64_t)oh * ow;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)oh * q4; i += (int64_t)gridDim.x * 256) {
    const int y = (int)(i / q4);
    const int x = (int)(i - (int64_t)y * q4) * 4;
    SP_BCHECK(y, oh);
    SP_BCHECK(x + 3, ow);
    const uint32_t* s = reinterpret_cast<const uint32_t*>(im.src + (int64_t)y * im.stride + x * 3);
    const uint32_t w0 = s[0], w1 = s[1], w2 = s[2];  // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
    float* o = im.out + (int64_t)y * ow + x;
    *reinterpret_cast<float4*>(o) = make_float4(lut[w0 & 255], lut[(w0 >> 24) & 255], lut[(w1 >> 16) & 255], lut[(w2 >> 8) & 255]);
    *reinterpret_cast<float4*>(o + plane) =
        make_float4(lut[(w0 >> 8) & 255], lut[w1 & 255], lut[(w1 >> 24) & 255], lut[(w2 >> 16) & 255]);
    *reinterpret_cast<float4*>(o + 2 * plane) =
        make_float4(lut[(w0 >> 16) & 255], lut[(w1 >> 8) & 255], lut[w2 & 255], lut[(w2 >> 24) & 255]);
  }
}

// Largest band height whose source rows fit the LDS staging buffer.
int band_rows(const Coeffs& v, int out_h, int row_bytes, int* ntiles) {
  const int cap = kLdsBytes / row_bytes;
  auto fits = [&](int T) {
    for (int y0 = 0; y0 < out_h; y0 += T) {
      int y1 = y0 + T < out_h ? y0 + T : out_h;
      int r0 = v.h_bounds[2 * y0];
      int r1 = v.h_bounds[2 * (y1 - 1)] + v.h_bounds[2 * (y1 - 1) + 1];
      if (r1 - r0 > cap) return false;
    }
    return true;
  };
  if (!fits(1)) return 0;
  int lo = 1, hi = out_h;
  while (lo < hi) {  // monotone in practice; verified below
    int mid = (lo + hi + 1) / 2;
    if (fits(mid)) lo = mid; else hi = mid - 1;
  }
  while (lo > 1 && !fits(lo)) --lo;
  *ntiles = (out_h + lo - 1) / lo;
  return lo;
}

}  // namespace

// sp_shutdown: release the device coefficient tables (the only state the ABI keeps).
void free_coeff_cache() {
  std::lock_guard<std::mutex> lk(g_mu);
  for (auto& kv : g_cache) {
    hipFree(kv.second.d_bounds);
    hipFree(kv.second.d_k);
  }
  g_cache.clear();
}
}  // namespace sp

extern "C" int sp_preprocess_u8(const sp_image_u8* images, int n, int out_h, int out_w, float* out,
                                void* stream) {
  using namespace sp;
  SP_ARG_CHECK(images && out && n > 0, "sp_preprocess_u8: null args");
  SP_ARG_CHECK(out_h > 0 && out_w > 0, "sp_preprocess_u8: bad out size");
  hipStream_t s = as_stream(stream);
  for (int base = 0; base < n; base += kMaxImgs) {
    PreArgs a;
    memset(&a, 0, sizeof(a));
    a.out_h = out_h;
    a.out_w = out_w;
    int cnt = n - base < kMaxImgs ? n - base : kMaxImgs;
    bool same = out_w % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    for (int i = 0; i < cnt && same; ++i) {
      const sp_image_u8& im = images[base + i];
      // a row_stride below 3·width is left to the generic path, which refuses it
      same = im.data && im.height == out_h && im.width == out_w && im.row_stride % 4 == 0 &&
             im.row_stride >= 3 * im.width && (reinterpret_cast<uintptr_t>(im.data) & 3) == 0;
    }
    if (same) {  // every source already has the output size: rescale + CHW only
      for (int i = 0; i < cnt; ++i) {
        const sp_image_u8& im = images[base + i];
        a.img[i].src = im.data;
        a.img[i].stride = im.row_stride;
        a.img[i].out = out + (int64_t)(base + i) * 3 * out_h * out_w;
      }
      const int64_t work = (int64_t)out_h * (out_w / 4);
      const int gx = (int)std::min<int64_t>((work + 255) / 256, std::max(1, 2048 / cnt));
      hipLaunchKernelGGL(preprocess_same_size_kernel, dim3(gx, cnt), dim3(256), 0, s, a);
      int rc = check_launch("sp_preprocess_u8(same size)");
      if (rc) return rc;
      continue;
    }
    int max_tiles = 0, max_ksh = 0, lds = 0;
    for (int i = 0; i < cnt; ++i) {
      const sp_image_u8& im = images[base + i];
      SP_ARG_CHECK(im.data && im.height > 0 && im.width > 0 && im.row_stride >= 3 * im.width,
                   "sp_preprocess_u8: bad image %d", base + i);
      const Coeffs* hc = get_coeffs(im.width, out_w);
      const Coeffs* vc = get_coeffs(im.height, out_h);
      if (!hc->d_k || !vc->d_k) {
        set_error("sp_preprocess_u8: coefficient upload failed");
        return -3;
      }
      int ntiles = 0;
      const int cwmax = std::min(out_w, kColTile);
      int T = band_rows(*vc, out_h, cwmax * 3, &ntiles);
      SP_ARG_CHECK(T > 0, "sp_preprocess_u8: %dx%d -> %dx%d needs more LDS than available",
                   im.height, im.width, out_h, out_w);
      // shorter bands when the batch is small, so the launch still spreads over ~2k workgroups (bands × column
      // tiles × images), but at least 8 output rows per band where the LDS allows (the band's extra source rows,
      // ~2 at any scale, are read twice)
      const int ncol = (out_w + kColTile - 1) / kColTile;
      int cap = std::max(8, (out_h * cnt * ncol + 2047) / 2048);
      // a downscaled source's band stays near 24 source rows (a 4K → 1280² band of 25 output rows read ~47): the
      // horizontal pass is a chain of row loads per thread, and the launch waits for its longest band
      const double vscale = (double)im.height / out_h;
      if (vscale > 1.0) cap = std::min(cap, std::max(4, (int)(24.0 / vscale)));
      if (T > cap) {
        T = cap;
        ntiles = (out_h + T - 1) / T;
      }
      for (int y0 = 0; y0 < out_h; y0 += T) {  // LDS bytes of this image's tallest band
        const int y1 = y0 + T < out_h ? y0 + T : out_h;
        const int rows = vc->h_bounds[2 * (y1 - 1)] + vc->h_bounds[2 * (y1 - 1) + 1] - vc->h_bounds[2 * y0];
        if (rows * cwmax * 3 > lds) lds = rows * cwmax * 3;
      }
      PreImg& p = a.img[i];
      p.src = im.data;
      p.h = im.height;
      p.w = im.width;
      p.stride = im.row_stride;
      p.hb = hc->d_bounds;
      p.hk = hc->d_k;
      p.ksh = hc->ksize;
      p.vb = vc->d_bounds;
      p.vk = vc->d_k;
      p.ksv = vc->ksize;
      p.rows_per_tile = T;
      p.ntiles = ntiles;
      p.out = out + (int64_t)(base + i) * 3 * out_h * out_w;
      if (ntiles > max_tiles) max_tiles = ntiles;
      if (hc->ksize > max_ksh) max_ksh = hc->ksize;
    }
    const dim3 grid(max_tiles * ((out_w + kColTile - 1) / kColTile), cnt);
    a.vec4 = out_w % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    lds = (lds + 15) & ~15;
    if (max_ksh <= 3)  // up-scaling and same-size sources
      hipLaunchKernelGGL(preprocess_kernel<3>, grid, dim3(256), lds, s, a);
    else if (max_ksh <= 5)
      hipLaunchKernelGGL(preprocess_kernel<5>, grid, dim3(256), lds, s, a);
    else if (max_ksh <= 7)  // down-scaling by up to 3x (1920 → 640, 3840 → 1280)
      hipLaunchKernelGGL(preprocess_kernel<7>, grid, dim3(256), lds, s, a);
    else
      hipLaunchKernelGGL(preprocess_kernel<0>, grid, dim3(256), lds, s, a);
    int rc = check_launch("sp_preprocess_u8");
    if (rc) return rc;
  }
  return 0;
}
