// The F(4×4, 3×3) output transform of a bottleneck's 3×3 conv fused into the 1×1 expand that follows it
// (SP_PREC_F32X3 operands): M [36][T][K] → act(expand(act2(Aᵀ M A · scale2 + shift2)) · scale + shift + res1),
// bit-identical to sp_winograd_f43_output followed by sp_conv2d on a 32x32x16 LDS-DMA tile.
//
// Unfused, the output transform writes the K-channel map and the expand reads it back at once; the expand's
// 128×128 tiles then fetch every A fragment from L2 and split it once per N tile. Here one persistent workgroup
// per CU (eight waves) owns a contiguous run of 32-pixel units (two 4×4 Winograd tiles, one MFMA row block) and
// walks it in pixel tiles of up to three units:
//  - transform phase: each (Winograd tile, 4-channel group) item runs wino_out_f43_kernel's arithmetic (the
//    s[p][bb] fma chain over a, the y chain over bb, fma(y, scale2, shift2), act2) on non-temporal M loads, splits
//    the sixteen results ONCE into hi / mid / lo bf16 (split_frag_pk<3>) and writes them into three resident
//    plane images [96 pixels][K] (16-byte chunks swizzled by pixel so a 16-lane group's b128 fragment reads cover
//    all 64 banks). 96 · K · 2 B · 3 = 147,456 B at K = 256.
//  - GEMM phase: A = the pixels from the planes, B = the weights. Wave v owns output channels 256c + 32v .. +31 of
//    chunk c, so its weight fragments go L2 → registers (two k16 steps ahead) from a host repack of the hi / mid /
//    lo planes into fragment order ([Cout/32][K/16][3][64 lanes][8], ops.pack_expand_frag): no LDS, no barrier.
//    The chunk's residual segment is fetched during its k loop; outputs are stored from the accumulator layout
//    (two 128-byte row segments per instruction).
// Only the stash of a new pixel tile takes workgroup barriers. No lane exchanges data with another except through
// the plane images. Per output element: one accumulator chain over k16 steps in ascending k, lane half h holding
// k = 16s + 8h .. +7 (glds_main's fragment), mfma_planes<3>'s six-product order, then fmaf(acc, scale, shift),
// + res1, act (epilogue_vec's order).
#include <type_traits>

#include "conv_plan.h"
#include "mfma16_common.h"

namespace sp {

// winograd.hip: the F(4×4) stages' argument checks for conv2's descriptor (all of wino_check), the tile grid.
int wino43_geometry(const char* what, const sp_conv_desc* d, const float* work, int64_t work_elems, bool ptrs,
                    int* th, int* tw, int64_t* T);

namespace {

constexpr int WX_PX = 96;     // pixels of a full pixel tile: three units
constexpr int WX_NCHUNK = 256;  // output channels per chunk: eight waves × 32

struct WxArgs {
  const float* M;          // the M half of the Winograd workspace, [36][T][K]
  int64_t T, units;
  int th, tw, H, W;
  const float* sc2;        // conv2's BN affine (null: 1 / 0) and act
  const float* sh2;
  int act2;
  const uint4* wf;         // the expand's planes in fragment order
  const float* scale;
  const float* shift;
  int act;
  const float* res1;
  int64_t ldr1;
  float* C;
  int64_t ldc;
  int Cout;
  int wbytes;              // bytes of the fragment-order planes: 3 · Cout · K · 2
  int rbytes, cbytes;      // bytes of the residual / output rows: ((N·H·W − 1) · ld + Cout) · 4 < 2^31 − 4
};

typedef float v4f __attribute__((ext_vector_type(4)));

// wino_out_f43_kernel's transform matrix (winograd.hip kAT43)
constexpr float kAT[4][6] = {{1.f, 1.f, 1.f, 1.f, 1.f, 0.f},
                             {0.f, -1.f, 1.f, 0.5f, -2.f, 0.f},
                             {0.f, 1.f, 1.f, 0.25f, 4.f, 0.f},
                             {0.f, -1.f, 1.f, 0.125f, -8.f, 1.f}};

// LDS slot of 16-byte chunk `chunk` of pixel row `row` (K / 8 chunks per row, a multiple of 16): the lane groups
// of a ds_read_b128 ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} of each half wave) hold 16 distinct row & 15.
__device__ __forceinline__ int wx_swz(int row, int chunk) { return chunk ^ (row & 15); }

template <int K>
__global__ __launch_bounds__(512, 1) void wino_expand_kernel(const WxArgs a) {
  constexpr int CPP = K / 8;   // 16-byte chunks per pixel per plane
  constexpr int NS = K / 16;   // k16 steps
  constexpr int C4 = K / 4;    // 4-channel groups per Winograd tile
  constexpr int PLANE = WX_PX * CPP;
  static_assert(CPP % 16 == 0, "the swizzle permutes 16 chunks");
  __shared__ uint4 lds[3 * PLANE];
  static_assert(sizeof(lds) == (K == 256 ? 147456 : 73728), "static LDS bytes");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;

  // this workgroup's contiguous run of units, cut into pixel tiles of near-equal size (at most three units)
  const int64_t u0 = a.units * blockIdx.x / gridDim.x, u1 = a.units * (blockIdx.x + 1) / gridDim.x;
  const int nrun = (int)(u1 - u0);
  const int ntile = (nrun + 2) / 3;
  const int64_t mplane = a.T * K;
  const int tht = a.th * a.tw;
  // residual and output rows through buffer descriptors (spans below 2^31 bytes: the host checks): a pixel's
  // offset is a scalar, the lane adds its row of the pair and its channel; lanes outside the map take an offset
  // past the bound, which the hardware drops
  const int ldr = (int)a.ldr1, ldc = (int)a.ldc;
  const __amdgpu_buffer_rsrc_t rrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.res1), 0, a.rbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t crs = __builtin_amdgcn_make_buffer_rsrc(a.C, 0, a.cbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t wrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4*>(a.wf), 0, a.wbytes, 0x00020000);
  const int vres = (h * a.W * ldr + r) * 4, vout = (h * a.W * ldc + r) * 4;

  for (int tile = 0; tile < ntile; ++tile) {
    const int64_t ub = u0 + (int64_t)nrun * tile / ntile;
    const int nu = (int)(u0 + (int64_t)nrun * (tile + 1) / ntile - ub);
    __syncthreads();  // the previous pixel tile's fragment reads are done
    // ---- transform phase
    for (int it = tid; it < 2 * nu * C4; it += 512) {
      const int tt = it / C4, c = (it - tt * C4) * 4;
      const int64_t t = 2 * ub + tt;
      v4f s[4][6];
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int bb = 0; bb < 6; ++bb) s[p][bb] = v4f(0.f);
      const bool tok = t < a.T;
      if (tok) {
        const float* src = a.M + t * K + c;
        SP_BCHECK(35 * mplane + t * K + c + 3, 36 * mplane);
        v4f mr[2][6];  // two rows of M in flight: all six would hold 144 registers beside s
#pragma unroll
        for (int bb = 0; bb < 6; ++bb)
          mr[0][bb] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(src + bb * mplane));
#pragma unroll
        for (int aa = 0; aa < 6; ++aa) {
          if (aa + 1 < 6) {
#pragma unroll
            for (int bb = 0; bb < 6; ++bb)
              mr[(aa + 1) & 1][bb] =
                  __builtin_nontemporal_load(reinterpret_cast<const v4f*>(src + ((aa + 1) * 6 + bb) * mplane));
          }
#pragma unroll
          for (int p = 0; p < 4; ++p)
            if (kAT[p][aa] != 0.f)
#pragma unroll
              for (int bb = 0; bb < 6; ++bb)
                s[p][bb] = __builtin_elementwise_fma(v4f(kAT[p][aa]), mr[aa & 1][bb], s[p][bb]);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      const v4f sc = a.sc2 ? *reinterpret_cast<const v4f*>(a.sc2 + c) : v4f(1.f);
      const v4f sh = a.sh2 ? *reinterpret_cast<const v4f*>(a.sh2 + c) : v4f(0.f);
      uint2* dst = reinterpret_cast<uint2*>(lds);
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          v4f y = v4f(0.f);
#pragma unroll
          for (int bb = 0; bb < 6; ++bb)
            if (kAT[qq][bb] != 0.f) y = __builtin_elementwise_fma(v4f(kAT[qq][bb]), s[p][bb], y);
          y = __builtin_elementwise_fma(y, sc, sh);
#pragma unroll
          for (int e = 0; e < 4; ++e) y[e] = tok ? (a.act2 ? fmaxf(y[e], 0.f) : y[e]) : 0.f;
          bf16x8 pl[3];
          split_frag_pk<3>(make_float4(y[0], y[1], y[2], y[3]), make_float4(0.f, 0.f, 0.f, 0.f), pl);
          const int row = tt * 16 + p * 4 + qq;
          const int pos = (row * CPP + wx_swz(row, c >> 3)) * 2 + ((c >> 2) & 1);
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            const uint4 v = __builtin_bit_cast(uint4, pl[q]);
            dst[q * PLANE * 2 + pos] = make_uint2(v.x, v.y);
          }
        }
    }
    __syncthreads();

    // ---- the pixels of this tile: per unit and Winograd tile, the first pixel's row index and the rows / columns
    // inside the map (wave-uniform)
    int pix0[3][2], hrem[3][2], wrem[3][2];
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const int t = 2 * ((int)ub + u) + tt;  // T < 2^31
        const bool ok = u < nu && t < (int)a.T;
        const int tc = ok ? t : 0;
        const int b = tc / tht, rem = tc - b * tht;
        const int ty = rem / a.tw, tx = rem - ty * a.tw;
        pix0[u][tt] = (b * a.H + 4 * ty) * a.W + 4 * tx;
        hrem[u][tt] = ok ? a.H - 4 * ty : 0;
        wrem[u][tt] = a.W - 4 * tx;
      }

    // ---- GEMM phase: chunk by chunk, this wave's 32 channels of each; one straight-line instance per unit count
    auto gemm = [&](auto nuc) {
      constexpr int NU = decltype(nuc)::value;
      for (int n0 = wave * 32; n0 < a.Cout; n0 += WX_NCHUNK) {
        const int wb = (n0 >> 5) * (NS * 3 * 1024);  // this wave's 32 channels: NS · 3 fragments of 1 KB
        SP_BCHECK(wb + (NS * 3 - 1) * 1024 + lane * 16 + 15, a.wbytes);
        // the tile's pixel geometry as this chunk's own scalars: left loop-invariant, the 96 residual / output
        // offsets and masks derived from it are hoisted out of the chunk loop and spilled
        int p0[NU][2], hr[NU][2], wr[NU][2];
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
          for (int tt = 0; tt < 2; ++tt) {
            p0[u][tt] = pix0[u][tt];
            hr[u][tt] = hrem[u][tt];
            wr[u][tt] = wrem[u][tt];
            asm volatile("" : "+s"(p0[u][tt]), "+s"(hr[u][tt]), "+s"(wr[u][tt]));
          }
        f32x16 acc[NU];
        zero_acc(acc);
        bf16x8 wfr[3][3];      // the weight fragments of three k16 steps: two ahead of the MFMAs
        bf16x8 xa[2][3];       // the pixel fragments of two (step, unit) blocks: one ahead
        float res[NU][16];
        auto load_w = [&](int s) {
#pragma unroll
          for (int q = 0; q < 3; ++q)
            wfr[s % 3][q] = __builtin_bit_cast(
                bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wrs, lane * 16, wb + (s * 3 + q) * 1024, 0));
        };
        // fragment (s, u, plane q) of lane (r, h) sits at row 32u + r, chunk wx_swz(row, 2s + h): with x0 the byte
        // address of step 0, unit 0, plane 0 that is (x0 ^ 32s) + 32u · CPP · 16 + q · PLANE · 16. x0 is made this
        // chunk's own value: left loop-invariant, all NS · NU addresses are computed once and spilled
        int x0 = (r * CPP + wx_swz(r, h)) * 16;
        asm volatile("" : "+v"(x0));
        auto load_x = [&](int i) {  // block i = s · NU + u
          const int s = i / NU, u = i - s * NU;
          const char* base = reinterpret_cast<const char*>(lds) + ((x0 ^ (s << 5)) + u * (32 * CPP * 16));
#pragma unroll
          for (int q = 0; q < 3; ++q) xa[i & 1][q] = *reinterpret_cast<const bf16x8*>(base + q * (PLANE * 16));
        };
        load_w(0);
        load_w(1);
        load_x(0);
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
          for (int q = 0; q < 16; ++q) res[u][q] = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          if (s + 2 < NS) load_w(s + 2);
          if (s == NS / 2 && a.res1) {  // the chunk's residual segment, in the accumulator layout
#pragma unroll
            for (int u = 0; u < NU; ++u)
#pragma unroll
              for (int q = 0; q < 16; ++q) {
                const int tt = q >> 3, pp = (q >> 2) & 1, qq = q & 3;
                const bool ok = 2 * pp + h < hr[u][tt] && qq < wr[u][tt];
                const int so = (p0[u][tt] + 2 * pp * a.W + qq) * (ldr * 4) + n0 * 4;
                res[u][q] = __builtin_bit_cast(
                    float, __builtin_amdgcn_raw_buffer_load_b32(rrs, ok ? vres : 0x7ffffffc, so, 0));
              }
          }
#pragma unroll
          for (int u = 0; u < NU; ++u) {
            const int i = s * NU + u;
            if (i + 1 < NS * NU) load_x(i + 1);
            acc[u] = mfma_planes<3>(xa[i & 1], wfr[s % 3], acc[u]);
            __builtin_amdgcn_sched_barrier(0);
          }
          __builtin_amdgcn_sched_barrier(0);  // keep the loads one / two steps ahead, not all of them up front
        }
        const float sc = a.scale ? a.scale[n0 + r] : 1.0f;
        const float sh = a.shift ? a.shift[n0 + r] : 0.0f;
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int tt = q >> 3, pp = (q >> 2) & 1, qq = q & 3;
            const bool ok = 2 * pp + h < hr[u][tt] && qq < wr[u][tt];
            const int so = (p0[u][tt] + 2 * pp * a.W + qq) * (ldc * 4) + n0 * 4;
            if (ok) SP_BCHECK((int64_t)so + vout, a.cbytes);
            float v = fmaf(acc[u][q], sc, sh);
            if (a.res1) v += res[u][q];
            v = a.act ? fmaxf(v, 0.f) : v;
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), crs, ok ? vout : 0x7ffffffc, so, 0);
          }
      }
    };
    if (nu == 3) gemm(std::integral_constant<int, 3>{});
    else if (nu == 2) gemm(std::integral_constant<int, 2>{});
    else gemm(std::integral_constant<int, 1>{});
  }
}

// an LDS-DMA tile on v_mfma_f32_16x16x32_bf16 (SP_GLDS_CONFIGS' M16 column): another sum order
constexpr bool glds_is_m16(int id) {
  switch (id) {
#define SP_WX_M16(id, WM, WN, TM, TN, NS, BK, M16, OCC, AB) \
  case id:                                                  \
    return M16;
    SP_GLDS_CONFIGS(SP_WX_M16)
#undef SP_WX_M16
    default:
      return false;
  }
}

constexpr bool wx_k_built(int k) { return k == 256 || k == 128; }

// Everything the entry point launches from (the plan query reports it): conv2's tile grid, the expand's launch
// arguments and plan, and whether the fused kernel runs.
struct WxPlan {
  int th, tw;
  int64_t T;
  ConvArgs ea;
  ConvPlan ep;
  int fused;
};

int wx_plan(const char* what, const sp_conv_desc* c2, const float* work, int64_t work_elems, bool ptrs,
            const sp_conv_desc* ex, bool has_frag, const uint16_t* frag, int64_t frag_elems, int64_t min_pixels,
            WxPlan* w) {
  SP_ARG_CHECK(c2 != nullptr && ex != nullptr, "%s: null descriptor", what);
  if (int rc = wino43_geometry(what, c2, work, work_elems, ptrs, &w->th, &w->tw, &w->T)) return rc;
  int planes;
  if (conv_args(ex, conv_overrides(), &w->ea, &planes) || plan_conv(w->ea, planes, conv_overrides(), &w->ep)) return -1;
  SP_ARG_CHECK(ex->KH == 1 && ex->KW == 1 && ex->stride == 1 && ex->pad == 0 && ex->N == c2->N && ex->H == c2->H &&
                   ex->W == c2->W && ex->Cin == c2->Cout && ex->A == c2->C && ex->lda == c2->ldc,
               "%s: the expand must be a 1x1 stride-1 conv reading conv2's output rows (A = conv2's C, lda = its ldc, "
               "Cin = its Cout, the same N, H, W)", what);
  SP_ARG_CHECK(!has_frag || (frag_elems >= (int64_t)3 * ex->Cout * ex->Cin &&
                             (!ptrs || (frag && (reinterpret_cast<uintptr_t>(frag) & 15) == 0))),
               "%s: fragment-order planes: %lld < 3*Cout*K elements, or null / not 16-byte aligned", what,
               (long long)frag_elems);
  const ConvPlan& p = w->ep;
  w->fused = has_frag && p.family == SP_CONV_GLDS && p.planes == 3 && p.splits == 1 && !p.a_bf16 &&
             !glds_is_m16(p.tile) && wx_k_built(ex->Cin) && ex->Cout % 32 == 0 && !ex->res2 && !ex->res2_bf16 &&
             !ex->res1_bf16 && !ex->C_bf16 && !ex->A2 && !ex->row_scale && ex->out_rows_per_group == 0 &&
             (int64_t)ex->Cout * ex->Cin * 6 < (int64_t(1) << 31) && !ex->ln_gamma && !c2->res1 && !c2->res2 && ex->act <= SP_ACT_RELU && c2->act <= SP_ACT_RELU &&
             ((w->ea.M - 1) * ex->ldc + ex->Cout) * 4 < (int64_t(1) << 31) - 4 &&
             (!ex->res1 || ((w->ea.M - 1) * ex->ldr1 + ex->Cout) * 4 < (int64_t(1) << 31) - 4) &&
             w->ea.Mp >= min_pixels;
  return 0;
}

template <int K>
int wx_launch(const WxArgs& a, hipStream_t s) {
  const int64_t cap = g_num_cus > 0 ? g_num_cus : 1;  // persistent: one workgroup per CU
  const unsigned grid = (unsigned)(a.units < cap ? a.units : cap);
  hipLaunchKernelGGL(wino_expand_kernel<K>, dim3(grid), dim3(512), 0, s, a);
  return check_launch("sp_winograd_f43_expand");
}

}  // namespace
}  // namespace sp

extern "C" int sp_winograd_f43_expand(const sp_conv_desc* conv2, const float* work, int64_t work_elems,
                                      const sp_conv_desc* expand, const uint16_t* expand_frag, int64_t frag_elems,
                                      int64_t min_pixels, void* stream) {
  using namespace sp;
  const char* what = "sp_winograd_f43_expand";
  WxPlan w;
  if (int rc = wx_plan(what, conv2, work, work_elems, true, expand, expand_frag != nullptr, expand_frag, frag_elems,
                       min_pixels, &w))
    return rc;
  if (!w.fused) {
    if (int rc = sp_winograd_f43_output(conv2, work, work_elems, stream)) return rc;
    return launch_plan(w.ea, w.ep, as_stream(stream));
  }
  WxArgs a;
  a.M = work + (int64_t)36 * w.T * conv2->Cin;
  a.T = w.T;
  a.units = (w.T + 1) / 2;
  a.th = w.th;
  a.tw = w.tw;
  a.H = conv2->H;
  a.W = conv2->W;
  a.sc2 = conv2->scale;
  a.sh2 = conv2->shift;
  a.act2 = conv2->act;
  a.wf = reinterpret_cast<const uint4*>(expand_frag);
  a.scale = expand->scale;
  a.shift = expand->shift;
  a.act = expand->act;
  a.res1 = expand->res1;
  a.ldr1 = expand->ldr1;
  a.C = expand->C;
  a.ldc = expand->ldc;
  a.Cout = expand->Cout;
  a.wbytes = 3 * expand->Cout * expand->Cin * 2;
  a.cbytes = (int)(((w.ea.M - 1) * expand->ldc + expand->Cout) * 4);
  a.rbytes = expand->res1 ? (int)(((w.ea.M - 1) * expand->ldr1 + expand->Cout) * 4) : 0;
  return expand->Cin == 256 ? wx_launch<256>(a, as_stream(stream)) : wx_launch<128>(a, as_stream(stream));
}

extern "C" int sp_winograd_expand_plan(const sp_conv_desc* conv2, int64_t work_elems, const sp_conv_desc* expand,
                                       int has_frag, int64_t min_pixels, sp_winograd_expand_plan_info* out) {
  using namespace sp;
  SP_ARG_CHECK(out != nullptr, "sp_winograd_expand_plan: null out");
  WxPlan w;
  if (int rc = wx_plan("sp_winograd_expand_plan", conv2, nullptr, work_elems, false, expand, has_frag != 0, nullptr,
                       expand ? (int64_t)3 * expand->Cout * expand->Cin : 0, min_pixels, &w))
    return rc;
  out->expand = w.ep;
  out->fused = w.fused;
  out->reserved = 0;
  out->tiles = w.T;
  out->units = (w.T + 1) / 2;
  return 0;
}
