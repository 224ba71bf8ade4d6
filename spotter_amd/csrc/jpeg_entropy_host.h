// Host side of the GPU entropy decode (jpeg_entropy.hip) that is not the scan packer (jpeg_host.h pack_scan): the
// argument checks and the kernel geometry both sides share, and the emulation that runs the kernels' passes in
// their order on the CPU over the same per-subsequence core (jpeg_entropy_core.h) — what the CPU tests and the
// sanitizer harness (tools/sanitize/jpeg_entropy_fuzz.cpp) run. Plain C++, no HIP dependency.
#pragma once

#include <cstring>
#include <vector>

#include "../../include/spotter_hip.h"
#include "jpeg_entropy_core.h"

namespace sp {
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
    if (lay.h[c] < 1 || lay.v[c] < 1 || lay.bw[c] != sc.mcux * lay.h[c] || lay.bh[c] != sc.mcuy * lay.v[c])
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
      sc.stream_bytes % 16 || sc.stream_bits < 0 || sc.stream_bits > (sc.stream_bytes - 16) * 8 ||
      sc.pkg_bytes != sc.stream_off + sc.stream_bytes)
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

// The kernels' passes, in their order: zero, kLaunches synchronisation launches of workgroups of kBlock
// subsequences (each an in-workgroup loop of at most kBlock rounds that reads the previous round's exits only),
// the prefix sum of block counts, the write pass, the DC sums, their prefix sum, the DC pass.
inline void emulate(const uint8_t* pkg, const sp_jpeg_scan& sc, const sp_jpeg_layout& lay, int16_t* coefs,
                    int32_t* status, int32_t* rounds) {
  const Geom G = make_geom(sc, lay);
  const Stream S{reinterpret_cast<const uint32_t*>(pkg + sc.stream_off), sc.stream_bytes / 4, 0};
  const DevHuff* tabs = reinterpret_cast<const DevHuff*>(pkg + sc.tab_off);
  const SegEnt* segs = reinterpret_cast<const SegEnt*>(pkg + sc.seg_off);
  const int64_t nsub = sc.nsub;
  memset(coefs, 0, (size_t)lay.total_blocks * 64 * sizeof(int16_t));
  std::vector<Rec> E((size_t)nsub), X[2] = {std::vector<Rec>((size_t)nsub), std::vector<Rec>((size_t)nsub)};
  std::vector<int32_t> segid((size_t)nsub);
  int st = 0, last_changed = 0, max_inner = 0;
  NullSink null;
  for (int launch = 0; launch < kLaunches; ++launch) {
    const std::vector<Rec>& prev = X[(launch + 1) & 1];
    std::vector<Rec>& next = X[launch & 1];
    for (int64_t b0 = 0; b0 < nsub; b0 += kBlock) {
      const int n = (int)(nsub - b0 < kBlock ? nsub - b0 : kBlock);
      Rec lds[kBlock], e[kBlock], x[kBlock];
      SubSpan sp[kBlock];
      for (int t = 0; t < n; ++t) {
        const int64_t i = b0 + t;
        if (launch == 0) segid[i] = find_seg(segs, sc.nseg, i);
        sp[t] = sub_span(segs, segid[i], i);
        if (launch == 0) {
          e[t] = Rec{sp[t].start, 0, 0};
          x[t] = decode_sub(S, tabs, G, e[t], sp[t].end, sp[t].seg_end, null).exit;
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
          const Rec nx = decode_sub(S, tabs, G, e[t], sp[t].end, sp[t].seg_end, null).exit;
          if (launch > 0 && !same_state(nx, x[t])) last_changed = launch;
          x[t] = nx;
          any = true;
        }
        if (!any) break;
        for (int t = 0; t < n; ++t) lds[t] = x[t];
      }
      if (r > max_inner) max_inner = r;
      for (int t = 0; t < n; ++t) {
        E[b0 + t] = e[t];
        next[b0 + t] = x[t];
      }
    }
  }
  const std::vector<Rec>& XF = X[(kLaunches - 1) & 1];
  std::vector<int64_t> excl((size_t)nsub + 1);
  excl[0] = 0;
  for (int64_t i = 0; i < nsub; ++i) excl[i + 1] = excl[i] + XF[i].nblk;
  for (int64_t i = 0; i < nsub; ++i) {
    const int32_t seg = segid[i];
    const SubSpan sp = sub_span(segs, seg, i);
    const SegEnt a = segs[seg], b = segs[seg + 1];
    if (!sp.first && !same_state(XF[i - 1], E[i])) st |= kStUnsync;
    const int64_t done = excl[i] - excl[a.sub0];
    CoefSink sink{coefs, &G, (int64_t)a.mcu * G.bpm + done, (int64_t)b.mcu * G.bpm, -1, 0};
    sink.seek();
    const SubResult res = decode_sub(S, tabs, G, E[i], sp.end, sp.seg_end, sink);
    st |= res.err;
    if (sp.last) st |= segment_end_status(res.exit, done + res.exit.nblk, (int64_t)(b.mcu - a.mcu) * G.bpm);
  }
  const int64_t nchunk = dc_nchunk(G), cps = dc_chunks_per_seg(G);
  std::vector<int64_t> dcs((size_t)(nchunk + 1) * 3, 0);
  for (int64_t g = 0; g < nchunk; ++g) {
    int64_t m0, m1, sum[3] = {0, 0, 0};
    bool first;
    dc_chunk_span(G, g, m0, m1, first);
    for (int64_t m = m0; m < m1; ++m)
      for (int s = 0; s < G.bpm; ++s) sum[G.slot_comp[s]] += coefs[block_index(G, m, s) * 64];
    for (int c = 0; c < 3; ++c) dcs[g * 3 + c] = sum[c];
  }
  for (int c = 0; c < 3; ++c) {
    int64_t carry = 0;
    for (int64_t g = 0; g <= nchunk; ++g) {
      const int64_t v = g < nchunk ? dcs[g * 3 + c] : 0;
      dcs[g * 3 + c] = carry;
      carry += v;
    }
  }
  for (int64_t g = 0; g < nchunk; ++g) {
    int64_t m0, m1, pred[3];
    bool first;
    dc_chunk_span(G, g, m0, m1, first);
    const int64_t g0 = g / cps * cps;
    for (int c = 0; c < 3; ++c) pred[c] = dcs[g * 3 + c] - dcs[g0 * 3 + c];
    for (int64_t m = m0; m < m1; ++m)
      for (int s = 0; s < G.bpm; ++s) {
        int16_t* blk = coefs + block_index(G, m, s) * 64;
        int64_t& p = pred[G.slot_comp[s]];
        p += blk[0];
        if (p > 0x7fffffffLL || p < -0x80000000LL) st |= kStDcRange;
        blk[0] = (int16_t)p;
      }
  }
  *status |= st;
  if (rounds) {
    rounds[0] = last_changed;
    rounds[1] = max_inner;
  }
}

}  // namespace jpeg_entropy
}  // namespace sp
