// Host side of the GPU entropy decode (jpeg_entropy.hip) that is not the scan packer (jpeg_host.h pack_scan): the
// argument checks and the kernel geometry both sides share, and the emulation that runs the kernels' passes in
// their order on the CPU over the same per-subsequence core (jpeg_entropy_core.h) — what the CPU tests and the
// sanitizer harness (tools/sanitize/jpeg_entropy_fuzz.cpp) run — and the host half of the batched chain
// (sp_jpeg_entropy_batch_*: the table's plan, its check and the emulation that walks it), run by
// tools/sanitize/jpeg_entropy_batch.cpp. Plain C++, no HIP dependency.
#pragma once

#include <cstddef>
#include <cstring>
#include <vector>

#include "../../include/spotter_hip.h"
#include "jpeg_entropy_core.h"

namespace sp {
void set_error(const char* fmt, ...);
namespace jpeg_entropy {

// nullptr when scan / lay describe a package the kernels can walk safely, else what is wrong
inline const char* check_scan(const sp_jpeg_scan& sc, const sp_jpeg_layout& lay) {
  if (sc.ncomp != lay.ncomp || (sc.ncomp != 1 && sc.ncomp != 3)) return "component count";
  if (sc.bpm < 1 || sc.bpm > kMaxSlots || sc.mcux < 1 || sc.mcuy < 1 || sc.restart_interval < 0) return "MCU geometry";
  if (sc.sub_bits != kSubBits) return "subsequence size";
  if (sc.nmcu != (int64_t)sc.mcux * sc.mcuy || sc.nseg < 1 || sc.nsub < sc.nseg || sc.nsub > 0x7fffffff)
    return "segment counts";
  if (sc.nseg != (sc.restart_interval ? (sc.nmcu + sc.restart_interval - 1) / sc.restart_interval : 1))
    return "segment counts";
  int64_t blocks = 0;
  for (int c = 0; c < lay.ncomp; ++c) {
    if (lay.h[c] < 1 || lay.v[c] < 1 || lay.bw[c] != (int64_t)sc.mcux * lay.h[c] ||
        lay.bh[c] != (int64_t)sc.mcuy * lay.v[c])
      return "layout does not match the scan";
    if (lay.block_off[c] != blocks) return "layout does not match the scan";
    blocks += (int64_t)lay.bw[c] * lay.bh[c];
  }
  if (blocks != lay.total_blocks) return "layout does not match the scan";
  for (int s = 0; s < sc.bpm; ++s) {
    const int c = sc.slot_comp[s];
    if (c < 0 || c >= lay.ncomp || sc.slot_v[s] < 0 || sc.slot_v[s] >= lay.v[c] || sc.slot_h[s] < 0 ||
        sc.slot_h[s] >= lay.h[c])
      return "slot table";
  }
  if (sc.tab_off != 0 || sc.seg_off != 6 * (int64_t)sizeof(DevHuff) ||
      sc.stream_off != sc.seg_off + (sc.nseg + 1) * (int64_t)sizeof(SegEnt) || sc.stream_bytes < 16 ||
      sc.stream_bytes % 16 || sc.stream_bits < 0 || sc.stream_bits / 8 + (sc.stream_bits % 8 != 0) > sc.stream_bytes - 16 ||
      sc.pkg_bytes < sc.stream_off || sc.pkg_bytes - sc.stream_off != sc.stream_bytes)
    return "package offsets";
  return nullptr;
}

inline Geom make_geom(const sp_jpeg_scan& sc, const sp_jpeg_layout& lay) {
  Geom G;
  memset(&G, 0, sizeof(G));
  G.bpm = sc.bpm;
  G.ncomp = sc.ncomp;
  G.mcux = sc.mcux;
  G.mcuy = sc.mcuy;
  G.ri = sc.restart_interval;
  for (int s = 0; s < kMaxSlots; ++s) {
    G.slot_comp[s] = sc.slot_comp[s];
    G.slot_v[s] = sc.slot_v[s];
    G.slot_h[s] = sc.slot_h[s];
    G.slot_comp_bits |= (uint32_t)(sc.slot_comp[s] & 3) << (2 * s);
  }
  for (int c = 0; c < 3; ++c) {
    G.comp_h[c] = lay.h[c];
    G.comp_v[c] = lay.v[c];
    G.bw[c] = lay.bw[c];
    G.block_off[c] = lay.block_off[c];
  }
  G.total_blocks = lay.total_blocks;
  G.nmcu = sc.nmcu;
  return G;
}

inline int64_t dc_nchunk(const Geom& G) { return dc_nseg(G) * dc_chunks_per_seg(G); }

// The kernels' passes as functions of one workgroup (or one launch) each, over plain pointers: the single-image
// emulation below runs them over vectors, the batched one (batch_emulate) over the ranges its table names.
struct View {  // what a kernel knows of one image: its package and geometry
  Stream S;
  const DevHuff* tabs;
  const SegEnt* segs;
  int64_t nseg, nsub;
  const Geom* G;
  SP_ENT_HD const Geom& geom() const { return *G; }
};
SP_ENT_HD View make_view(const uint8_t* pkg, const sp_jpeg_scan& sc, const Geom* G) {
  return View{Stream{reinterpret_cast<const uint32_t*>(pkg + sc.stream_off), sc.stream_bytes / 4, 0},
              reinterpret_cast<const DevHuff*>(pkg + sc.tab_off), reinterpret_cast<const SegEnt*>(pkg + sc.seg_off),
              sc.nseg, sc.nsub, G};
}

// ent_sync_kernel, workgroup wg of launch `launch`: an in-workgroup loop of at most kBlock rounds that reads the
// previous round's exits only, thread 0 the exit the previous workgroup recorded in the launch before
inline void emu_sync_wg(const View& P, int launch, int64_t wg, Rec* E, const Rec* prev, Rec* next, int32_t* segid,
                        int* last_changed, int* max_inner) {
  const Geom& G = *P.G;
  const int64_t b0 = wg * kBlock;
  const int n = (int)(P.nsub - b0 < kBlock ? P.nsub - b0 : kBlock);
  NullSink null;
  Rec lds[kBlock], e[kBlock], x[kBlock];
  SubSpan sp[kBlock];
  for (int t = 0; t < n; ++t) {
    const int64_t i = b0 + t;
    if (launch == 0) segid[i] = find_seg(P.segs, P.nseg, i);
    sp[t] = sub_span(P.segs, segid[i], i);
    if (launch == 0) {
      e[t] = Rec{sp[t].start, 0, 0};
      x[t] = decode_sub(P.S, P.tabs, G, e[t], sp[t].end, sp[t].seg_end, null).exit;
    } else {
      e[t] = E[i];
      x[t] = prev[i];
    }
    lds[t] = x[t];
  }
  int r = 0;
  for (; r < kBlock; ++r) {
    bool any = false;
    for (int t = 0; t < n; ++t) {
      const int64_t i = b0 + t;
      if (sp[t].first) continue;
      Rec p;
      if (t > 0) p = lds[t - 1];
      else if (launch > 0 && i > 0) p = prev[i - 1];
      else continue;
      if (same_state(p, e[t])) continue;
      e[t] = Rec{p.bit, 0, p.sk};
      const Rec nx = decode_sub(P.S, P.tabs, G, e[t], sp[t].end, sp[t].seg_end, null).exit;
      if (launch > 0 && !same_state(nx, x[t])) *last_changed = launch;
      x[t] = nx;
      any = true;
    }
    if (!any) break;
    for (int t = 0; t < n; ++t) lds[t] = x[t];
  }
  if (r > *max_inner) *max_inner = r;
  for (int t = 0; t < n; ++t) {
    E[b0 + t] = e[t];
    next[b0 + t] = x[t];
  }
}

// ent_scan_kernel over the block counts: excl[i] = blocks completed before subsequence i, excl[nsub] the total
inline void emu_count_scan(const Rec* XF, int64_t nsub, int64_t* excl) {
  excl[0] = 0;
  for (int64_t i = 0; i < nsub; ++i) excl[i + 1] = excl[i] + XF[i].nblk;
}

// ent_write_kernel, subsequences [i0, i1): the status bits they raise
inline int emu_write(const View& P, int64_t i0, int64_t i1, const Rec* E, const Rec* XF, const int32_t* segid,
                     const int64_t* excl, int16_t* coefs) {
  const Geom& G = *P.G;
  int st = 0;
  for (int64_t i = i0; i < i1; ++i) {
    const int32_t seg = segid[i];
    const SubSpan sp = sub_span(P.segs, seg, i);
    const SegEnt a = P.segs[seg], b = P.segs[seg + 1];
    if (!sp.first && !same_state(XF[i - 1], E[i])) st |= kStUnsync;
    const int64_t done = excl[i] - excl[a.sub0];
    CoefSink sink{coefs, &G, (int64_t)a.mcu * G.bpm + done, (int64_t)b.mcu * G.bpm, -1, 0};
    sink.seek();
    const SubResult res = decode_sub(P.S, P.tabs, G, E[i], sp.end, sp.seg_end, sink);
    st |= res.err;
    if (sp.last) st |= segment_end_status(res.exit, done + res.exit.nblk, (int64_t)(b.mcu - a.mcu) * G.bpm);
  }
  return st;
}

// ent_dc_sum_kernel, chunks [g0, g1)
inline void emu_dc_sum(const Geom& G, int64_t g0, int64_t g1, const int16_t* coefs, int64_t* dcs) {
  for (int64_t g = g0; g < g1; ++g) {
    int64_t m0, m1, sum[3] = {0, 0, 0};
    bool first;
    dc_chunk_span(G, g, m0, m1, first);
    for (int64_t m = m0; m < m1; ++m)
      for (int s = 0; s < G.bpm; ++s) sum[G.slot_comp[s]] += coefs[block_index(G, m, s) * 64];
    for (int c = 0; c < 3; ++c) dcs[g * 3 + c] = sum[c];
  }
}

// ent_scan_kernel over the three DC lanes, in place
inline void emu_dc_scan(int64_t nchunk, int64_t* dcs) {
  for (int c = 0; c < 3; ++c) {
    int64_t carry = 0;
    for (int64_t g = 0; g <= nchunk; ++g) {
      const int64_t v = g < nchunk ? dcs[g * 3 + c] : 0;
      dcs[g * 3 + c] = carry;
      carry += v;
    }
  }
}

// ent_dc_apply_kernel, chunks [g0, g1): the status bits they raise
inline int emu_dc_apply(const Geom& G, int64_t g0, int64_t g1, const int64_t* dcs, int16_t* coefs) {
  const int64_t cps = dc_chunks_per_seg(G);
  int st = 0;
  for (int64_t g = g0; g < g1; ++g) {
    int64_t m0, m1, pred[3];
    bool first;
    dc_chunk_span(G, g, m0, m1, first);
    const int64_t gs = g / cps * cps;
    for (int c = 0; c < 3; ++c) pred[c] = dcs[g * 3 + c] - dcs[gs * 3 + c];
    for (int64_t m = m0; m < m1; ++m)
      for (int s = 0; s < G.bpm; ++s) {
        int16_t* blk = coefs + block_index(G, m, s) * 64;
        int64_t& p = pred[G.slot_comp[s]];
        p += blk[0];
        if (p > 0x7fffffffLL || p < -0x80000000LL) st |= kStDcRange;
        blk[0] = (int16_t)p;
      }
  }
  return st;
}

// The kernels' passes, in their order: zero, kLaunches synchronisation launches of workgroups of kBlock
// subsequences, the prefix sum of block counts, the write pass, the DC sums, their prefix sum, the DC pass.
inline void emulate(const uint8_t* pkg, const sp_jpeg_scan& sc, const sp_jpeg_layout& lay, int16_t* coefs,
                    int32_t* status, int32_t* rounds) {
  const Geom G = make_geom(sc, lay);
  const View P = make_view(pkg, sc, &G);
  const int64_t nsub = sc.nsub;
  memset(coefs, 0, (size_t)lay.total_blocks * 64 * sizeof(int16_t));
  std::vector<Rec> E((size_t)nsub), X[2] = {std::vector<Rec>((size_t)nsub), std::vector<Rec>((size_t)nsub)};
  std::vector<int32_t> segid((size_t)nsub);
  int st = 0, last_changed = 0, max_inner = 0;
  for (int launch = 0; launch < kLaunches; ++launch)
    for (int64_t wg = 0; wg * kBlock < nsub; ++wg)
      emu_sync_wg(P, launch, wg, E.data(), X[(launch + 1) & 1].data(), X[launch & 1].data(), segid.data(),
                  &last_changed, &max_inner);
  const std::vector<Rec>& XF = X[(kLaunches - 1) & 1];
  std::vector<int64_t> excl((size_t)nsub + 1);
  emu_count_scan(XF.data(), nsub, excl.data());
  st |= emu_write(P, 0, nsub, E.data(), XF.data(), segid.data(), excl.data(), coefs);
  const int64_t nchunk = dc_nchunk(G);
  std::vector<int64_t> dcs((size_t)(nchunk + 1) * 3, 0);
  emu_dc_sum(G, 0, nchunk, coefs, dcs.data());
  emu_dc_scan(nchunk, dcs.data());
  st |= emu_dc_apply(G, 0, nchunk, dcs.data(), coefs);
  *status |= st;
  if (rounds) {
    rounds[0] = last_changed;
    rounds[1] = max_inner;
  }
}

// ------------------------------------------------------------------------------------------------ batched
// Host half of the batched chain (sp_jpeg_entropy_batch_plan / _check / _emulate): one table row per image, the
// workgroups of the per-subsequence and of the DC launches numbered through the batch by two prefix columns.
// Plain C++ like the rest of this file: tools/sanitize/jpeg_entropy_batch.cpp runs it under ASan / UBSan.
#define SP_ENT_REQUIRE(cond, ...)    \
  do {                               \
    if (!(cond)) {                   \
      ::sp::set_error(__VA_ARGS__);  \
      return -1;                     \
    }                                \
  } while (0)

static_assert(sizeof(Geom) == sizeof(((sp_jpeg_entropy_item*)nullptr)->geom), "sp_jpeg_entropy_item.geom holds a Geom");
static_assert(sizeof(sp_jpeg_entropy_item) % 8 == 0 && offsetof(sp_jpeg_entropy_item, geom) % 8 == 0,
              "table rows and their Geom are 8-byte aligned");

SP_ENT_HD const Geom& row_geom(const sp_jpeg_entropy_item& it) { return *reinterpret_cast<const Geom*>(it.geom); }

// the part of a layout check_scan and make_geom read, from a row's fields
inline sp_jpeg_layout row_layout(const sp_jpeg_entropy_item& it) {
  sp_jpeg_layout lay;
  memset(&lay, 0, sizeof(lay));
  lay.ncomp = it.scan.ncomp;
  for (int c = 0; c < 3; ++c) {
    lay.h[c] = it.h[c], lay.v[c] = it.v[c], lay.bw[c] = it.bw[c], lay.bh[c] = it.bh[c];
    lay.block_off[c] = it.block_off[c];
  }
  lay.total_blocks = it.total_blocks;
  return lay;
}

// The frame bounds the sums below rely on (the largest frame libjpeg accepts is 8188 MCUs across), then check_scan.
constexpr int kMaxMcusAcross = 1 << 14;
inline const char* check_row_scan(const sp_jpeg_scan& sc, const sp_jpeg_layout& lay) {
  if (sc.mcux < 1 || sc.mcuy < 1 || sc.mcux > kMaxMcusAcross || sc.mcuy > kMaxMcusAcross ||
      sc.restart_interval < 0)
    return "MCU geometry";
  for (int c = 0; c < 3; ++c)
    if (lay.h[c] < 0 || lay.h[c] > 4 || lay.v[c] < 0 || lay.v[c] > 4) return "sampling factors";
  return check_scan(sc, lay);
}

SP_ENT_HD int64_t sub_wgs(int64_t nsub) { return (nsub + kBlock - 1) / kBlock; }
SP_ENT_HD int64_t dc_wgs(int64_t nchunk) { return (nchunk + 255) / 256; }
inline int64_t align16(int64_t v) { return (v + 15) & ~15LL; }

inline int batch_plan(const sp_jpeg_scan* scans, const sp_jpeg_layout* lays, const sp_jpeg_batch_item* bitems, int n,
                      sp_jpeg_entropy_item* items, sp_jpeg_entropy_totals* totals) {
  SP_ENT_REQUIRE(scans && lays && bitems && items && totals, "sp_jpeg_entropy_batch_plan: null args");
  SP_ENT_REQUIRE(n >= 1 && n <= SP_JPEG_BATCH_MAX, "sp_jpeg_entropy_batch_plan: n = %d outside [1, %d]", n,
                 SP_JPEG_BATCH_MAX);
  sp_jpeg_entropy_totals t = {0, 0, 0, 0};
  for (int i = 0; i < n; ++i) {
    const sp_jpeg_scan& sc = scans[i];
    const sp_jpeg_layout& lay = lays[i];
    const char* why = check_row_scan(sc, lay);
    SP_ENT_REQUIRE(!why, "sp_jpeg_entropy_batch_plan: image %d: %s", i, why);
    const int64_t need = lay.total_blocks * 64, off = bitems[i].coef_off;
    SP_ENT_REQUIRE(off >= 0 && off <= INT64_MAX - need && bitems[i].lay.total_blocks >= lay.total_blocks,
                   "sp_jpeg_entropy_batch_plan: image %d: coefficient range at %lld holds %lld blocks, the scan has %lld",
                   i, (long long)off, (long long)bitems[i].lay.total_blocks, (long long)lay.total_blocks);
    for (int k = 0; k < i; ++k)
      SP_ENT_REQUIRE(off + need <= bitems[k].coef_off || bitems[k].coef_off + lays[k].total_blocks * 64 <= off,
                     "sp_jpeg_entropy_batch_plan: coefficient ranges of images %d and %d overlap: [%lld, +%lld) does "
                     "not hold total_blocks * 64", k, i, (long long)off, (long long)need);
    sp_jpeg_entropy_item& it = items[i];
    memset(&it, 0, sizeof(it));
    it.scan = sc;
    for (int c = 0; c < 3; ++c) {
      it.h[c] = lay.h[c], it.v[c] = lay.v[c], it.bw[c] = lay.bw[c], it.bh[c] = lay.bh[c];
      it.block_off[c] = lay.block_off[c];
    }
    it.total_blocks = lay.total_blocks;
    const sp_jpeg_layout rl = row_layout(it);  // the fields the row keeps: what the check will see
    const Geom G = make_geom(sc, rl);
    memcpy(it.geom, &G, sizeof(G));
    it.dc_nchunk = dc_nchunk(G);
    it.pkg_off = t.pkg_bytes;
    it.work_off = t.work_bytes;
    it.coef_off = off;
    it.first_wg_sub = (int32_t)t.wg_sub;
    it.first_wg_dc = (int32_t)t.wg_dc;
    t.pkg_bytes += align16(sc.pkg_bytes);
    t.work_bytes += align16(work_layout(sc.nsub, it.dc_nchunk).bytes);
    t.wg_sub += sub_wgs(sc.nsub);
    t.wg_dc += dc_wgs(it.dc_nchunk);
    SP_ENT_REQUIRE(t.wg_sub <= INT32_MAX && t.wg_dc <= INT32_MAX,
                   "sp_jpeg_entropy_batch_plan: more than 2^31 - 1 workgroups at image %d", i);
  }
  *totals = t;
  return 0;
}

// What sp_jpeg_entropy_batch_decode checks on the host copy of the table before it launches anything.
inline int batch_check(const sp_jpeg_entropy_item* items, int n, const sp_jpeg_entropy_totals* totals,
                       int64_t pkg_bytes, int64_t work_bytes, int64_t coef_elems) {
  SP_ENT_REQUIRE(items && totals, "sp_jpeg_entropy_batch: null args");
  SP_ENT_REQUIRE(n >= 1 && n <= SP_JPEG_BATCH_MAX, "sp_jpeg_entropy_batch: n = %d outside [1, %d]", n,
                 SP_JPEG_BATCH_MAX);
  SP_ENT_REQUIRE(pkg_bytes >= 0 && work_bytes >= 0 && coef_elems >= 0, "sp_jpeg_entropy_batch: negative buffer size");
  int64_t wg_sub = 0, wg_dc = 0;
  for (int i = 0; i < n; ++i) {
    const sp_jpeg_entropy_item& it = items[i];
    const sp_jpeg_layout lay = row_layout(it);
    const char* why = check_row_scan(it.scan, lay);
    SP_ENT_REQUIRE(!why, "sp_jpeg_entropy_batch: image %d: %s", i, why);
    const Geom G = make_geom(it.scan, lay);
    SP_ENT_REQUIRE(memcmp(&G, it.geom, sizeof(G)) == 0 && it.dc_nchunk == dc_nchunk(G),
                   "sp_jpeg_entropy_batch: image %d: geometry does not match the scan", i);
    const int64_t wbytes = work_layout(it.scan.nsub, it.dc_nchunk).bytes, cneed = it.total_blocks * 64;
    SP_ENT_REQUIRE(it.pkg_off >= 0 && (it.pkg_off & 15) == 0 && it.pkg_off <= pkg_bytes &&
                       it.scan.pkg_bytes <= pkg_bytes - it.pkg_off,
                   "sp_jpeg_entropy_batch: image %d: package [%lld, +%lld) misaligned or outside %lld bytes", i,
                   (long long)it.pkg_off, (long long)it.scan.pkg_bytes, (long long)pkg_bytes);
    SP_ENT_REQUIRE(it.work_off >= 0 && (it.work_off & 15) == 0 && it.work_off <= work_bytes &&
                       wbytes <= work_bytes - it.work_off,
                   "sp_jpeg_entropy_batch: image %d: workspace [%lld, +%lld) misaligned or outside %lld bytes", i,
                   (long long)it.work_off, (long long)wbytes, (long long)work_bytes);
    SP_ENT_REQUIRE(it.coef_off >= 0 && it.coef_off <= coef_elems && cneed <= coef_elems - it.coef_off,
                   "sp_jpeg_entropy_batch: image %d: coefficients [%lld, +%lld) outside %lld elements", i,
                   (long long)it.coef_off, (long long)cneed, (long long)coef_elems);
    SP_ENT_REQUIRE(it.first_wg_sub == wg_sub && it.first_wg_dc == wg_dc,
                   "sp_jpeg_entropy_batch: image %d: first workgroups %d / %d, its predecessors give %lld / %lld", i,
                   it.first_wg_sub, it.first_wg_dc, (long long)wg_sub, (long long)wg_dc);
    wg_sub += sub_wgs(it.scan.nsub);
    wg_dc += dc_wgs(it.dc_nchunk);
    SP_ENT_REQUIRE(wg_sub <= INT32_MAX && wg_dc <= INT32_MAX, "sp_jpeg_entropy_batch: too many workgroups");
    for (int k = 0; k < i; ++k) {
      const sp_jpeg_entropy_item& o = items[k];
      SP_ENT_REQUIRE(it.pkg_off + it.scan.pkg_bytes <= o.pkg_off || o.pkg_off + o.scan.pkg_bytes <= it.pkg_off,
                     "sp_jpeg_entropy_batch: packages of images %d and %d overlap", k, i);
      SP_ENT_REQUIRE(it.work_off + wbytes <= o.work_off ||
                         o.work_off + work_layout(o.scan.nsub, o.dc_nchunk).bytes <= it.work_off,
                     "sp_jpeg_entropy_batch: workspaces of images %d and %d overlap", k, i);
      SP_ENT_REQUIRE(it.coef_off + cneed <= o.coef_off || o.coef_off + o.total_blocks * 64 <= it.coef_off,
                     "sp_jpeg_entropy_batch: coefficients of images %d and %d overlap", k, i);
    }
  }
  SP_ENT_REQUIRE(totals->wg_sub == wg_sub && totals->wg_dc == wg_dc,
                 "sp_jpeg_entropy_batch: totals give %lld / %lld workgroups, the table %lld / %lld",
                 (long long)totals->wg_sub, (long long)totals->wg_dc, (long long)wg_sub, (long long)wg_dc);
  SP_ENT_REQUIRE(totals->pkg_bytes <= pkg_bytes && totals->work_bytes <= work_bytes,
                 "sp_jpeg_entropy_batch: totals give %lld package / %lld workspace bytes, the buffers hold %lld / %lld",
                 (long long)totals->pkg_bytes, (long long)totals->work_bytes, (long long)pkg_bytes,
                 (long long)work_bytes);
  return 0;
}

// the row of workgroup wg: the kernels' uniform binary search of a first-workgroup column
SP_ENT_HD int batch_row(const sp_jpeg_entropy_item* items, int n, int32_t sp_jpeg_entropy_item::*first, int64_t wg) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (items[mid].*first <= wg) lo = mid; else hi = mid;
  }
  return lo;
}

struct RowWork {  // an image's workspace arrays inside the shared workspace
  Rec* E;
  Rec* X[2];
  int32_t* segid;
  int64_t* cnt;
  int64_t* dcs;
};
SP_ENT_HD RowWork row_work(uint8_t* work, const sp_jpeg_entropy_item& it) {
  const WorkLayout wl = work_layout(it.scan.nsub, it.dc_nchunk);
  uint8_t* w = work + it.work_off;
  return RowWork{reinterpret_cast<Rec*>(w + wl.entry),
                 {reinterpret_cast<Rec*>(w + wl.exit0), reinterpret_cast<Rec*>(w + wl.exit1)},
                 reinterpret_cast<int32_t*>(w + wl.segid), reinterpret_cast<int64_t*>(w + wl.cnt),
                 reinterpret_cast<int64_t*>(w + wl.dcs)};
}

// sp_jpeg_entropy_batch_decode's launches in their order, each walked workgroup by workgroup (a checked table:
// batch_check has passed). status[img] gets image img's bits.
inline void batch_emulate(const uint8_t* pkgs, const sp_jpeg_entropy_item* items, int n,
                          const sp_jpeg_entropy_totals& tot, uint8_t* work, int16_t* coefs, int32_t* status) {
  using Item = sp_jpeg_entropy_item;
  for (int i = 0; i < n; ++i)  // one memset over the chunk on the device; per range here, the sentinels stay
    memset(coefs + items[i].coef_off, 0, (size_t)items[i].total_blocks * 64 * sizeof(int16_t));
  int unused[2] = {0, 0};
  for (int launch = 0; launch < kLaunches; ++launch)
    for (int64_t wg = 0; wg < tot.wg_sub; ++wg) {
      const Item& it = items[batch_row(items, n, &Item::first_wg_sub, wg)];
      const View P = make_view(pkgs + it.pkg_off, it.scan, &row_geom(it));
      const RowWork W = row_work(work, it);
      emu_sync_wg(P, launch, wg - it.first_wg_sub, W.E, W.X[(launch + 1) & 1], W.X[launch & 1], W.segid, &unused[0],
                  &unused[1]);
    }
  const int xf = (kLaunches - 1) & 1;
  for (int img = 0; img < n; ++img) {  // one workgroup per image
    const RowWork W = row_work(work, items[img]);
    emu_count_scan(W.X[xf], items[img].scan.nsub, W.cnt);
  }
  for (int64_t wg = 0; wg < tot.wg_sub; ++wg) {
    const int img = batch_row(items, n, &Item::first_wg_sub, wg);
    const Item& it = items[img];
    const View P = make_view(pkgs + it.pkg_off, it.scan, &row_geom(it));
    const RowWork W = row_work(work, it);
    const int64_t i0 = (wg - it.first_wg_sub) * kBlock, i1 = i0 + kBlock < P.nsub ? i0 + kBlock : P.nsub;
    status[img] |= emu_write(P, i0, i1, W.E, W.X[xf], W.segid, W.cnt, coefs + it.coef_off);
  }
  for (int pass = 0; pass < 2; ++pass) {
    for (int64_t wg = 0; wg < tot.wg_dc; ++wg) {
      const int img = batch_row(items, n, &Item::first_wg_dc, wg);
      const Item& it = items[img];
      const RowWork W = row_work(work, it);
      const int64_t g0 = (wg - it.first_wg_dc) * 256, g1 = g0 + 256 < it.dc_nchunk ? g0 + 256 : it.dc_nchunk;
      if (pass == 0) emu_dc_sum(row_geom(it), g0, g1, coefs + it.coef_off, W.dcs);
      else status[img] |= emu_dc_apply(row_geom(it), g0, g1, W.dcs, coefs + it.coef_off);
    }
    if (pass == 0)
      for (int img = 0; img < n; ++img) emu_dc_scan(items[img].dc_nchunk, row_work(work, items[img]).dcs);
  }
}

}  // namespace jpeg_entropy
}  // namespace sp
