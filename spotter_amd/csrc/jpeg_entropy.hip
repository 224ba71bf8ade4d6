// GPU entropy decode of baseline Huffman JPEG scans (include/spotter_hip.h sp_jpeg_entropy_decode): the scan
// package the host wrote (jpeg_host.h pack_scan: unstuffed bytes, restart segment table, Huffman tables) → the
// int16 coefficient array sp_jpeg_decode_coefs writes, which the unchanged sp_jpeg_to_rgb consumes.
//
// Self-synchronising parallel Huffman decode (Weißenberger & Schmidt; Klein & Wiseman). One thread per subsequence
// of kSubBits bits of a restart segment, the per-subsequence code in jpeg_entropy_core.h:
//   1. hipMemsetAsync zeroes the coefficients.
//   2. ent_sync_kernel, kLaunches times. The first launch decodes every subsequence from its first bit in state
//      (slot 0, k 0) (the first one of a segment from the true state) and records its exit; then, in a loop of at
//      most `inner` rounds with barriers, thread t re-decodes from thread t-1's exit (through LDS) until no exit in
//      the workgroup changes. Later launches start from the recorded states, thread 0 taking the exit the
//      previous workgroup recorded in the launch before (exits are double-buffered, so a launch only reads what
//      an earlier launch wrote). No kernel waits on another workgroup; every loop is bounded by a launch argument.
//   3. ent_scan_kernel: exclusive prefix sum of the completed-block counts (one workgroup, `trips` rounds).
//   4. ent_write_kernel: each thread checks that its entry is its predecessor's exit (else status), decodes once
//      more and stores the coefficients, the DC difference at [0]; where a segment ends, its block count and that
//      the decoder stands at a block boundary are checked (segment_end_status).
//   5. ent_dc_sum_kernel / ent_scan_kernel / ent_dc_apply_kernel: per-component prefix sum of the DC differences
//      in scan order, restarting at restart boundaries, 64-bit.
// sp_jpeg_entropy_batch_decode runs the same chain over up to SP_JPEG_BATCH_MAX images, one launch per pass, on
// the same device functions.
// A corrupt stream cannot fault: stream reads are clamped to the padded buffer, coefficient stores are bounded
// by the segment's block range and by total_blocks, table indices are bounded by construction.
#include <cstdint>

#include "common.h"

#if SP_BOUNDS && defined(__HIP_DEVICE_COMPILE__)
#define SP_ENT_BCHECK(idx, ext) SP_BCHECK(idx, ext)
#endif
#include "jpeg_entropy_core.h"
#include "jpeg_entropy_host.h"
#include "jpeg_host.h"

namespace sp {
namespace {
using namespace jpeg_entropy;

struct Pkg {
  Stream S;
  const DevHuff* tabs;
  const SegEnt* segs;
  int64_t nseg, nsub;
  Geom G;
  __device__ __forceinline__ const Geom& geom() const { return G; }
};
// The kernels' bodies are device functions over either form of an image: Pkg, which the single-image kernels get
// in their arguments, or View (jpeg_entropy_host.h), which the batched kernels build from the image's table row
// (its Geom stays in the table, in device memory). Every index in them is local to the image: subsequence i of
// workgroup wg of this image, arrays that start at this image's workspace.

// Every decode of a subsequence reads the same few stream words and the same tables: both are staged in LDS once
// per kernel (the tables as words, each thread's own window of the stream), so a symbol costs LDS latency, not
// L2's. Ends with a barrier; every thread of the workgroup calls it.
constexpr int kTabWords = 6 * sizeof(DevHuff) / 4;
template <class P>
__device__ __forceinline__ Stream stage(const P& Pk, uint32_t* ltabs, uint32_t* lwin, bool active, int64_t start) {
  const int t = threadIdx.x;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(Pk.tabs);
  const int nw = (int)(2 * Pk.geom().ncomp * sizeof(DevHuff) / 4);
  for (int j = t; j < nw; j += kBlock) ltabs[j] = src[j];
  Stream S = Stream{lwin + t * kWinWords, kWinWords, start >> 5};
  if (active) {
#pragma unroll
    for (int j = 0; j < kWinWords; ++j) {
      const int64_t w = S.base + j;
      SP_BCHECK(w < Pk.S.nwords ? w : 0, Pk.S.nwords);
      lwin[t * kWinWords + j] = w < Pk.S.nwords ? Pk.S.words[w] : 0u;
    }
  }
  __syncthreads();
  return S;
}

template <class P>
__device__ __forceinline__ void sync_workgroup(const P& Pk, int64_t wg, Rec* __restrict__ E,
                                               const Rec* __restrict__ Xprev, Rec* __restrict__ Xnext,
                                               int32_t* __restrict__ segid, int first, int inner) {
  __shared__ Rec lds[kBlock];
  __shared__ uint32_t ltabs[kTabWords];
  __shared__ uint32_t lwin[kBlock * kWinWords];
  const Geom& G = Pk.geom();
  const int t = threadIdx.x;
  const int64_t i = wg * kBlock + t;
  const bool active = i < Pk.nsub;
  NullSink null;
  Rec e = Rec{0, 0, 0}, x = Rec{0, 0, 0};
  SubSpan sp = SubSpan{0, 0, 0, true, true};
  if (active) {
    int32_t seg;
    if (first) {
      seg = find_seg(Pk.segs, Pk.nseg, i);
      segid[i] = seg;
    } else {
      seg = segid[i];
    }
    sp = sub_span(Pk.segs, seg, i);
  }
  const DevHuff* tabs = reinterpret_cast<const DevHuff*>(ltabs);
  const Stream S = stage(Pk, ltabs, lwin, active, sp.start);
  if (active) {
    if (first) {
      e = Rec{sp.start, 0, 0};
      x = decode_sub(S, tabs, G, e, sp.end, sp.seg_end, null).exit;
    } else {
      e = E[i];
      x = Xprev[i];
    }
  }
  lds[t] = x;
  __syncthreads();
  for (int r = 0; r < inner; ++r) {
    int changed = 0;
    if (active && !sp.first) {
      bool have = true;
      Rec p = Rec{0, 0, 0};
      if (t > 0) p = lds[t - 1];
      else if (!first && i > 0) p = Xprev[i - 1];  // i is local: never the previous image's records
      else have = false;
      if (have && !same_state(p, e)) {
        e = Rec{p.bit, 0, p.sk};
        x = decode_sub(S, tabs, G, e, sp.end, sp.seg_end, null).exit;
        changed = 1;
      }
    }
    if (!__syncthreads_or(changed)) break;  // uniform: every thread sees the same vote
    lds[t] = x;
    __syncthreads();
  }
  if (active) {
    E[i] = e;
    Xnext[i] = x;
  }
}

__global__ __launch_bounds__(kBlock) void ent_sync_kernel(const Pkg P, Rec* __restrict__ E,
                                                          const Rec* __restrict__ Xprev, Rec* __restrict__ Xnext,
                                                          int32_t* __restrict__ segid, int first, int inner) {
  sync_workgroup(P, (int64_t)blockIdx.x, E, Xprev, Xnext, segid, first, inner);
}

// Exclusive prefix sum by one workgroup of 256 threads x 4 items, `trips` rounds with a running carry, for each
// of `lanes` interleaved int64 lanes, in place: buf[i * lanes + l] ← sum of the values before i, buf[n * lanes + l]
// ← the total. With X the values are X[i].nblk (lanes = 1) instead of buf's.
__device__ __forceinline__ void scan_workgroup(const Rec* __restrict__ X, int64_t* __restrict__ buf, int64_t n,
                                               int lanes, int64_t trips) {
  __shared__ int64_t sh[256];
  const int t = threadIdx.x;
  for (int l = 0; l < lanes; ++l) {
    int64_t carry = 0;
    for (int64_t trip = 0; trip < trips; ++trip) {
      const int64_t i0 = (trip * 256 + t) * 4;
      int64_t v[4], sum = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t i = i0 + j;
        v[j] = i < n ? (X ? (int64_t)X[i].nblk : buf[i * lanes + l]) : 0;
        sum += v[j];
      }
      sh[t] = sum;
      __syncthreads();
      for (int o = 1; o < 256; o <<= 1) {
        const int64_t add = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
      }
      int64_t run = carry + sh[t] - sum;
      carry += sh[255];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t i = i0 + j;
        if (i < n) {
          SP_BCHECK(i * lanes + l, (n + 1) * lanes);
          buf[i * lanes + l] = run;
        }
        run += v[j];
      }
      __syncthreads();
    }
    if (t == 0) buf[n * lanes + l] = carry;
  }
}

__global__ __launch_bounds__(256) void ent_scan_kernel(const Rec* __restrict__ X, int64_t* __restrict__ buf, int64_t n,
                                                       int lanes, int64_t trips) {
  scan_workgroup(X, buf, n, lanes, trips);
}

template <class P>
__device__ __forceinline__ void write_workgroup(const P& Pk, int64_t wg, const Rec* __restrict__ E,
                                                const Rec* __restrict__ X, const int32_t* __restrict__ segid,
                                                const int64_t* __restrict__ excl, int16_t* __restrict__ coefs,
                                                int32_t* __restrict__ status) {
  __shared__ uint32_t ltabs[kTabWords];
  __shared__ uint32_t lwin[kBlock * kWinWords];
  const Geom& G = Pk.geom();
  const int64_t i = wg * kBlock + threadIdx.x;
  const bool active = i < Pk.nsub;
  const int32_t seg = active ? segid[i] : 0;
  const SubSpan sp = sub_span(Pk.segs, seg, active ? i : 0);
  const DevHuff* tabs = reinterpret_cast<const DevHuff*>(ltabs);
  const Stream S = stage(Pk, ltabs, lwin, active, sp.start);
  if (!active) return;
  const SegEnt a = Pk.segs[seg], b = Pk.segs[seg + 1];
  const Rec e = E[i];
  int st = 0;
  if (!sp.first && !same_state(X[i - 1], e)) st |= kStUnsync;
  const int64_t done = excl[i] - excl[a.sub0];
  CoefSink sink{coefs, &G, (int64_t)a.mcu * G.bpm + done, (int64_t)b.mcu * G.bpm, -1, 0};
  sink.seek();
  const SubResult res = decode_sub(S, tabs, G, e, sp.end, sp.seg_end, sink);
  st |= res.err;
  if (sp.last) st |= segment_end_status(res.exit, done + res.exit.nblk, (int64_t)(b.mcu - a.mcu) * G.bpm);
  if (st) atomicOr(status, st);
}

__global__ __launch_bounds__(kBlock) void ent_write_kernel(const Pkg P, const Rec* __restrict__ E,
                                                           const Rec* __restrict__ X,
                                                           const int32_t* __restrict__ segid,
                                                           const int64_t* __restrict__ excl,
                                                           int16_t* __restrict__ coefs, int32_t* __restrict__ status) {
  write_workgroup(P, (int64_t)blockIdx.x, E, X, segid, excl, coefs, status);
}

// DC chunk g of an image: the sums of its DC differences per component
__device__ __forceinline__ void dc_sum_chunk(const Geom& G, int64_t nchunk, int64_t g,
                                             const int16_t* __restrict__ coefs, int64_t* __restrict__ dcs) {
  if (g >= nchunk) return;
  int64_t m0, m1, sum[3] = {0, 0, 0};
  bool first;
  dc_chunk_span(G, g, m0, m1, first);
  for (int64_t m = m0; m < m1; ++m)
    for (int s = 0; s < G.bpm; ++s) {
      const int64_t b = block_index(G, m, s);
      SP_BCHECK(b, G.total_blocks);
      if (b >= 0 && b < G.total_blocks) sum[G.slot_comp[s]] += coefs[b * 64];
    }
  for (int c = 0; c < 3; ++c) dcs[g * 3 + c] = sum[c];
}

__global__ __launch_bounds__(256) void ent_dc_sum_kernel(const Geom G, int64_t nchunk,
                                                         const int16_t* __restrict__ coefs, int64_t* __restrict__ dcs) {
  dc_sum_chunk(G, nchunk, (int64_t)blockIdx.x * 256 + threadIdx.x, coefs, dcs);
}

// DC chunk g of an image: the differences become the DC values, from the scanned sums
__device__ __forceinline__ void dc_apply_chunk(const Geom& G, int64_t nchunk, int64_t cps, int64_t g,
                                               const int64_t* __restrict__ dcs, int16_t* __restrict__ coefs,
                                               int32_t* __restrict__ status) {
  if (g >= nchunk) return;
  int64_t m0, m1, pred[3];
  bool first, range = false;
  dc_chunk_span(G, g, m0, m1, first);
  const int64_t g0 = g / cps * cps;
  for (int c = 0; c < 3; ++c) pred[c] = dcs[g * 3 + c] - dcs[g0 * 3 + c];
  for (int64_t m = m0; m < m1; ++m)
    for (int s = 0; s < G.bpm; ++s) {
      const int64_t b = block_index(G, m, s);
      SP_BCHECK(b, G.total_blocks);
      if (b < 0 || b >= G.total_blocks) continue;
      int64_t& p = pred[G.slot_comp[s]];
      p += coefs[b * 64];
      range |= p > 0x7fffffffLL || p < -0x80000000LL;
      coefs[b * 64] = (int16_t)p;
    }
  if (range) atomicOr(status, (int)kStDcRange);
}

__global__ __launch_bounds__(256) void ent_dc_apply_kernel(const Geom G, int64_t nchunk, int64_t cps,
                                                           const int64_t* __restrict__ dcs, int16_t* __restrict__ coefs,
                                                           int32_t* __restrict__ status) {
  dc_apply_chunk(G, nchunk, cps, (int64_t)blockIdx.x * 256 + threadIdx.x, dcs, coefs, status);
}

// ------------------------------------------------------------------------------------------------ batched
// The same chain over a batch of images, one launch per pass: a workgroup serves one image, found by the uniform
// binary search of a first-workgroup column (batch_row: the exclusive prefix sums are strictly increasing, every
// image has at least one subsequence and one DC chunk), and runs the single-image body on that image's package,
// workspace and coefficient range. The host has checked every range of the table (batch_check) before a launch.
struct Bufs {  // the shared buffers and their sizes, for the bounds build's checks
  const uint8_t* pkgs;
  int64_t pkg_bytes;
  uint8_t* work;
  int64_t work_bytes;
  int16_t* coefs;
  int64_t coef_elems;
};

__device__ __forceinline__ const sp_jpeg_entropy_item& batch_item(const sp_jpeg_entropy_item* __restrict__ items, int n,
                                                                  int img, const Bufs& B) {
  SP_BCHECK(img, n);
  const sp_jpeg_entropy_item& it = items[img];
  SP_BCHECK(it.pkg_off + it.scan.pkg_bytes - 1, B.pkg_bytes);
  SP_BCHECK(it.work_off + work_layout(it.scan.nsub, it.dc_nchunk).bytes - 1, B.work_bytes);
  SP_BCHECK(it.coef_off + it.total_blocks * 64 - 1, B.coef_elems);
  return it;
}

__global__ __launch_bounds__(kBlock) void ent_sync_batch_kernel(const sp_jpeg_entropy_item* __restrict__ items, int n,
                                                                const Bufs B, int launch, int inner) {
  const int img = batch_row(items, n, &sp_jpeg_entropy_item::first_wg_sub, (int64_t)blockIdx.x);
  const sp_jpeg_entropy_item& it = batch_item(items, n, img, B);
  const int64_t wg = (int64_t)blockIdx.x - it.first_wg_sub;
  SP_BCHECK(wg, sub_wgs(it.scan.nsub));
  SP_BCHECK(wg * kBlock, it.scan.nsub);
  const View P = make_view(B.pkgs + it.pkg_off, it.scan, &row_geom(it));
  const RowWork W = row_work(B.work, it);
  // (selected, not indexed: a dynamic index would put the row's pointers in scratch)
  const bool odd = launch & 1;
  sync_workgroup(P, wg, W.E, odd ? W.X[0] : W.X[1], odd ? W.X[1] : W.X[0], W.segid, launch == 0 ? 1 : 0, inner);
}

// one workgroup per image: which = 0 the block counts of the final exits, 1 the three DC lanes
__global__ __launch_bounds__(256) void ent_scan_batch_kernel(const sp_jpeg_entropy_item* __restrict__ items, int n,
                                                             const Bufs B, int which, int xf, int64_t trips) {
  const sp_jpeg_entropy_item& it = batch_item(items, n, (int)blockIdx.x, B);
  const RowWork W = row_work(B.work, it);
  const int64_t cnt = which == 0 ? it.scan.nsub : it.dc_nchunk;
  int64_t own = (cnt + 1023) / 1024;
  if (own > trips) own = trips;  // bounded by the launch argument
  const Rec* X = which == 0 ? (xf ? W.X[1] : W.X[0]) : nullptr;
  scan_workgroup(X, which == 0 ? W.cnt : W.dcs, cnt, which == 0 ? 1 : 3, own);
}

__global__ __launch_bounds__(kBlock) void ent_write_batch_kernel(const sp_jpeg_entropy_item* __restrict__ items, int n,
                                                                 const Bufs B, int xf, int32_t* __restrict__ status) {
  const int img = batch_row(items, n, &sp_jpeg_entropy_item::first_wg_sub, (int64_t)blockIdx.x);
  const sp_jpeg_entropy_item& it = batch_item(items, n, img, B);
  const int64_t wg = (int64_t)blockIdx.x - it.first_wg_sub;
  SP_BCHECK(wg, sub_wgs(it.scan.nsub));
  SP_BCHECK(wg * kBlock, it.scan.nsub);
  const View P = make_view(B.pkgs + it.pkg_off, it.scan, &row_geom(it));
  const RowWork W = row_work(B.work, it);
  write_workgroup(P, wg, W.E, xf ? W.X[1] : W.X[0], W.segid, W.cnt, B.coefs + it.coef_off, status + img);
}

__global__ __launch_bounds__(256) void ent_dc_batch_kernel(const sp_jpeg_entropy_item* __restrict__ items, int n,
                                                           const Bufs B, int apply, int32_t* __restrict__ status) {
  const int img = batch_row(items, n, &sp_jpeg_entropy_item::first_wg_dc, (int64_t)blockIdx.x);
  const sp_jpeg_entropy_item& it = batch_item(items, n, img, B);
  const int64_t wg = (int64_t)blockIdx.x - it.first_wg_dc;
  SP_BCHECK(wg, dc_wgs(it.dc_nchunk));
  const Geom& G = row_geom(it);
  const RowWork W = row_work(B.work, it);
  const int64_t g = wg * 256 + threadIdx.x;
  if (apply) dc_apply_chunk(G, it.dc_nchunk, dc_chunks_per_seg(G), g, W.dcs, B.coefs + it.coef_off, status + img);
  else dc_sum_chunk(G, it.dc_nchunk, g, B.coefs + it.coef_off, W.dcs);
}

}  // namespace
}  // namespace sp

extern "C" int sp_jpeg_entropy_pack(const uint8_t* data, int64_t len, sp_jpeg_layout* lay, sp_jpeg_scan* scan,
                                    uint8_t* pkg, int64_t pkg_cap) {
  using namespace sp;
  using namespace sp::jpeg_host;
  SP_ARG_CHECK(data && lay && scan && len > 0 && pkg_cap >= 0, "sp_jpeg_entropy_pack: null args");
  memset(scan, 0, sizeof(*scan));
  // one parse for a file that is packed; a file that is not (not eligible, buffer too small) left the parser at
  // its first scan with *lay half filled, and gets the header-only pass sp_jpeg_decode_coefs(.., NULL, 0) runs
  Decoder d{data, len, lay, nullptr};
  d.pk = scan;
  d.pkg = pkg;
  d.pkg_cap = pkg ? pkg_cap : 0;
  const int rc = d.run(true);
  if (rc == SP_JPEG_NOT_ELIGIBLE || rc == SP_JPEG_PKG_SMALL) {
    Decoder d2{data, len, lay, nullptr};
    const int rc2 = d2.run(false);
    if (rc2) return rc2;
  }
  return rc;
}

extern "C" int sp_jpeg_entropy_emulate(const uint8_t* pkg, const sp_jpeg_scan* scan, const sp_jpeg_layout* lay,
                                       int16_t* coefs, int64_t coef_elems, int32_t* status, int32_t* rounds) {
  using namespace sp;
  SP_ARG_CHECK(pkg && scan && lay && coefs && status, "sp_jpeg_entropy_emulate: null args");
  const char* why = jpeg_entropy::check_scan(*scan, *lay);
  SP_ARG_CHECK(!why, "sp_jpeg_entropy_emulate: %s", why);
  SP_ARG_CHECK(coef_elems >= lay->total_blocks * 64, "sp_jpeg_entropy_emulate: coefficient buffer holds %lld < %lld",
               (long long)coef_elems, (long long)(lay->total_blocks * 64));
  jpeg_entropy::emulate(pkg, *scan, *lay, coefs, status, rounds);
  return 0;
}

extern "C" int sp_jpeg_entropy_decode(const uint8_t* pkg, const sp_jpeg_scan* scan, const sp_jpeg_layout* lay,
                                      uint8_t* work, int64_t work_bytes, int16_t* coefs, int64_t coef_elems,
                                      int32_t* status, void* stream) {
  using namespace sp;
  using namespace sp::jpeg_entropy;
  SP_ARG_CHECK(pkg && scan && lay && work && coefs && status, "sp_jpeg_entropy_decode: null args");
  const char* why = check_scan(*scan, *lay);
  SP_ARG_CHECK(!why, "sp_jpeg_entropy_decode: %s", why);
  SP_ARG_CHECK(coef_elems >= lay->total_blocks * 64, "sp_jpeg_entropy_decode: coefficient buffer holds %lld < %lld",
               (long long)coef_elems, (long long)(lay->total_blocks * 64));
  SP_ARG_CHECK(((reinterpret_cast<uintptr_t>(pkg) | reinterpret_cast<uintptr_t>(work)) & 15) == 0,
               "sp_jpeg_entropy_decode: pkg and work must be 16-byte aligned");
  Pkg P;
  P.G = make_geom(*scan, *lay);
  const int64_t nsub = scan->nsub, nchunk = dc_nchunk(P.G);
  const WorkLayout wl = work_layout(nsub, nchunk);
  SP_ARG_CHECK(work_bytes >= wl.bytes, "sp_jpeg_entropy_decode: work %lld < %lld bytes", (long long)work_bytes,
               (long long)wl.bytes);
  P.S = Stream{reinterpret_cast<const uint32_t*>(pkg + scan->stream_off), scan->stream_bytes / 4, 0};
  P.tabs = reinterpret_cast<const DevHuff*>(pkg + scan->tab_off);
  P.segs = reinterpret_cast<const SegEnt*>(pkg + scan->seg_off);
  P.nseg = scan->nseg;
  P.nsub = nsub;
  Rec* E = reinterpret_cast<Rec*>(work + wl.entry);
  Rec* X[2] = {reinterpret_cast<Rec*>(work + wl.exit0), reinterpret_cast<Rec*>(work + wl.exit1)};
  int32_t* segid = reinterpret_cast<int32_t*>(work + wl.segid);
  int64_t* cnt = reinterpret_cast<int64_t*>(work + wl.cnt);
  int64_t* dcs = reinterpret_cast<int64_t*>(work + wl.dcs);
  hipStream_t s = as_stream(stream);
  const hipError_t ez = hipMemsetAsync(coefs, 0, (size_t)lay->total_blocks * 64 * sizeof(int16_t), s);
  if (ez != hipSuccess) {
    set_error("sp_jpeg_entropy_decode(zero): %s", hipGetErrorString(ez));
    return static_cast<int>(ez);
  }
  const unsigned gsub = (unsigned)((nsub + kBlock - 1) / kBlock);
  int rc;
  for (int launch = 0; launch < kLaunches; ++launch) {
    hipLaunchKernelGGL(ent_sync_kernel, dim3(gsub), dim3(kBlock), 0, s, P, E, X[(launch + 1) & 1], X[launch & 1], segid,
                       launch == 0 ? 1 : 0, kBlock);
    if ((rc = check_launch("sp_jpeg_entropy_decode(sync)"))) return rc;
  }
  const Rec* XF = X[(kLaunches - 1) & 1];
  hipLaunchKernelGGL(ent_scan_kernel, dim3(1), dim3(256), 0, s, XF, cnt, nsub, 1, (nsub + 1023) / 1024);
  if ((rc = check_launch("sp_jpeg_entropy_decode(scan)"))) return rc;
  hipLaunchKernelGGL(ent_write_kernel, dim3(gsub), dim3(kBlock), 0, s, P, E, XF, segid, cnt, coefs, status);
  if ((rc = check_launch("sp_jpeg_entropy_decode(write)"))) return rc;
  const unsigned gdc = (unsigned)((nchunk + 255) / 256);
  hipLaunchKernelGGL(ent_dc_sum_kernel, dim3(gdc), dim3(256), 0, s, P.G, nchunk, coefs, dcs);
  if ((rc = check_launch("sp_jpeg_entropy_decode(dc sum)"))) return rc;
  hipLaunchKernelGGL(ent_scan_kernel, dim3(1), dim3(256), 0, s, (const Rec*)nullptr, dcs, nchunk, 3,
                     (nchunk + 1023) / 1024);
  if ((rc = check_launch("sp_jpeg_entropy_decode(dc scan)"))) return rc;
  hipLaunchKernelGGL(ent_dc_apply_kernel, dim3(gdc), dim3(256), 0, s, P.G, nchunk, dc_chunks_per_seg(P.G), dcs, coefs,
                     status);
  return check_launch("sp_jpeg_entropy_decode(dc apply)");
}

extern "C" int sp_jpeg_entropy_batch_plan(const sp_jpeg_scan* scans, const sp_jpeg_layout* lays,
                                          const sp_jpeg_batch_item* batch_items, int n,
                                          sp_jpeg_entropy_item* ent_items, sp_jpeg_entropy_totals* ent_totals) {
  return sp::jpeg_entropy::batch_plan(scans, lays, batch_items, n, ent_items, ent_totals);
}

extern "C" int sp_jpeg_entropy_batch_check(const sp_jpeg_entropy_item* items, int n,
                                           const sp_jpeg_entropy_totals* totals, int64_t pkg_bytes, int64_t work_bytes,
                                           int64_t coef_elems) {
  return sp::jpeg_entropy::batch_check(items, n, totals, pkg_bytes, work_bytes, coef_elems);
}

extern "C" int sp_jpeg_entropy_batch_emulate(const uint8_t* pkgs, int64_t pkg_bytes, const sp_jpeg_entropy_item* items,
                                             int n, const sp_jpeg_entropy_totals* totals, uint8_t* work,
                                             int64_t work_bytes, int16_t* coefs, int64_t coef_elems, int32_t* status) {
  using namespace sp;
  SP_ARG_CHECK(pkgs && items && totals && work && coefs && status, "sp_jpeg_entropy_batch_emulate: null args");
  SP_ARG_CHECK(((reinterpret_cast<uintptr_t>(pkgs) | reinterpret_cast<uintptr_t>(work)) & 15) == 0,
               "sp_jpeg_entropy_batch_emulate: pkgs and work must be 16-byte aligned");
  if (int rc = jpeg_entropy::batch_check(items, n, totals, pkg_bytes, work_bytes, coef_elems)) return rc;
  jpeg_entropy::batch_emulate(pkgs, items, n, *totals, work, coefs, status);
  return 0;
}

extern "C" int sp_jpeg_entropy_batch_decode(const uint8_t* pkgs_dev, int64_t pkg_bytes,
                                            const sp_jpeg_entropy_item* items_dev,
                                            const sp_jpeg_entropy_item* items_host, int n,
                                            const sp_jpeg_entropy_totals* totals, uint8_t* work, int64_t work_bytes,
                                            int16_t* coefs, int64_t coef_elems, int32_t* status, void* stream) {
  using namespace sp;
  using namespace sp::jpeg_entropy;
  SP_ARG_CHECK(pkgs_dev && items_dev && items_host && totals && work && coefs && status,
               "sp_jpeg_entropy_batch_decode: null args");
  SP_ARG_CHECK(((reinterpret_cast<uintptr_t>(pkgs_dev) | reinterpret_cast<uintptr_t>(work)) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(items_dev) & 7) == 0 && (reinterpret_cast<uintptr_t>(coefs) & 1) == 0 &&
                   (reinterpret_cast<uintptr_t>(status) & 3) == 0,
               "sp_jpeg_entropy_batch_decode: misaligned buffer");
  if (int rc = batch_check(items_host, n, totals, pkg_bytes, work_bytes, coef_elems)) return rc;
  hipStream_t s = as_stream(stream);
  // zero the coefficients: one memset per contiguous run of ranges — one for a table as sp_jpeg_batch_plan packs it
  int order[SP_JPEG_BATCH_MAX];
  for (int i = 0; i < n; ++i) {
    int k = i;
    for (; k > 0 && items_host[order[k - 1]].coef_off > items_host[i].coef_off; --k) order[k] = order[k - 1];
    order[k] = i;
  }
  int64_t trips_sub = 1, trips_dc = 1;
  for (int k = 0; k < n;) {
    const int64_t lo = items_host[order[k]].coef_off;
    int64_t hi = lo;
    for (; k < n && items_host[order[k]].coef_off == hi; ++k) hi += items_host[order[k]].total_blocks * 64;
    const hipError_t ez = hipMemsetAsync(coefs + lo, 0, (size_t)(hi - lo) * sizeof(int16_t), s);
    if (ez != hipSuccess) {
      set_error("sp_jpeg_entropy_batch_decode(zero): %s", hipGetErrorString(ez));
      return static_cast<int>(ez);
    }
  }
  for (int i = 0; i < n; ++i) {
    const int64_t a = (items_host[i].scan.nsub + 1023) / 1024, b = (items_host[i].dc_nchunk + 1023) / 1024;
    if (a > trips_sub) trips_sub = a;
    if (b > trips_dc) trips_dc = b;
  }
  const Bufs B{pkgs_dev, pkg_bytes, work, work_bytes, coefs, coef_elems};
  const unsigned gsub = (unsigned)totals->wg_sub, gdc = (unsigned)totals->wg_dc;
  int rc;
  for (int launch = 0; launch < kLaunches; ++launch) {
    hipLaunchKernelGGL(ent_sync_batch_kernel, dim3(gsub), dim3(kBlock), 0, s, items_dev, n, B, launch, kBlock);
    if ((rc = check_launch("sp_jpeg_entropy_batch_decode(sync)"))) return rc;
  }
  const int xf = (kLaunches - 1) & 1;
  hipLaunchKernelGGL(ent_scan_batch_kernel, dim3((unsigned)n), dim3(256), 0, s, items_dev, n, B, 0, xf, trips_sub);
  if ((rc = check_launch("sp_jpeg_entropy_batch_decode(scan)"))) return rc;
  hipLaunchKernelGGL(ent_write_batch_kernel, dim3(gsub), dim3(kBlock), 0, s, items_dev, n, B, xf, status);
  if ((rc = check_launch("sp_jpeg_entropy_batch_decode(write)"))) return rc;
  hipLaunchKernelGGL(ent_dc_batch_kernel, dim3(gdc), dim3(256), 0, s, items_dev, n, B, 0, status);
  if ((rc = check_launch("sp_jpeg_entropy_batch_decode(dc sum)"))) return rc;
  hipLaunchKernelGGL(ent_scan_batch_kernel, dim3((unsigned)n), dim3(256), 0, s, items_dev, n, B, 1, xf, trips_dc);
  if ((rc = check_launch("sp_jpeg_entropy_batch_decode(dc scan)"))) return rc;
  hipLaunchKernelGGL(ent_dc_batch_kernel, dim3(gdc), dim3(256), 0, s, items_dev, n, B, 1, status);
  return check_launch("sp_jpeg_entropy_batch_decode(dc apply)");
}
