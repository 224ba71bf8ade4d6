// The per-subsequence core of the parallel baseline-JPEG Huffman decode (jpeg_entropy.hip): the bit reader over
// an unstuffed scan buffer, the table lookup, the symbol loop with its exit state, and the index arithmetic that
// maps a subsequence to its restart segment and a scan-order block to its place in the coefficient array.
// Compiles as device code (hipcc) and as plain host C++: the kernels, the host emulation that runs them in the
// same order without a GPU (jpeg_entropy_host.h) and the sanitizer harness (tools/sanitize/jpeg_entropy_fuzz.cpp)
// all run this text.
//
// The method is the self-synchronising decode of Weißenberger & Schmidt (after Klein & Wiseman: a Huffman
// decoder started at a wrong bit falls into step with the true one after a few symbols). The scan is cut into
// subsequences of kSubBits bits; every subsequence is decoded from a guessed state first, then from its
// predecessor's exit state until that exit no longer changes. The state here is (bit, MCU slot, zig-zag index).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SP_ENT_HD __host__ __device__ __forceinline__
#else
#define SP_ENT_HD inline
#endif

// the bounds build's index check (csrc/common.h SP_BCHECK) where the including unit provides it
#ifndef SP_ENT_BCHECK
#define SP_ENT_BCHECK(idx, ext) \
  do {                          \
  } while (0)
#endif

namespace sp {
namespace jpeg_entropy {

constexpr int kLook = 11;       // lookahead bits of the first-level table (jpeg_host::kLook)
constexpr int kSubBits = 256;   // subsequence size s; a symbol is at most 31 bits, so an exit overshoots by < s
constexpr int kBlock = 256;     // subsequences per workgroup
constexpr int kLaunches = 3;    // the speculative launch + 2 cross-workgroup rounds (the round budget)
constexpr int kMaxSlots = 10;   // libjpeg's D_MAX_BLOCKS_IN_MCU
constexpr int kDcChunk = 2;     // MCUs one thread walks in the DC pass (its loads are serial: keep the walk short)

// status word reason codes (1 is sp_jpeg_to_rgb's IDCT envelope flag)
enum : int32_t {
  kStUnsync = 2,    // a subsequence whose entry is not its predecessor's exit after the round budget
  kStBadCode = 4,   // invalid Huffman code, value index out of range, or a coefficient index past 63
  kStOverrun = 8,   // bits consumed past the end of a restart segment
  kStCount = 16,    // a segment's block count is not its MCUs x blocks per MCU
  kStDcRange = 32,  // a DC prediction outside int32
  kStTail = 64,     // a segment that does not end at a block boundary: data after its last block
};

// one Huffman table as the device reads it: the host decoder's look / maxcode / valoff / vals
struct DevHuff {
  uint16_t look[1 << kLook];  // (code length << 8) | symbol; length 0: longer than kLook bits
  int32_t maxcode[18];
  int32_t valoff[18];
  uint8_t vals[256];
};
static_assert(sizeof(DevHuff) == 4496, "DevHuff is part of the scan package layout");

struct SegEnt {  // one restart segment: where it starts in the unstuffed stream, its first MCU and subsequence
  int64_t bit;
  int32_t mcu;
  int32_t sub0;
};
static_assert(sizeof(SegEnt) == 16, "SegEnt is part of the scan package layout");

struct Geom {
  int32_t bpm, ncomp, mcux, mcuy, ri;
  int32_t slot_comp[kMaxSlots], slot_v[kMaxSlots], slot_h[kMaxSlots];
  uint32_t slot_comp_bits;  // slot_comp packed 2 bits per slot: the symbol loop's lookup stays in a register
  int32_t comp_h[3], comp_v[3], bw[3];
  int64_t block_off[3];
  int64_t total_blocks, nmcu;
};

struct Stream {
  const uint32_t* words;  // the unstuffed scan bytes, zero padded to whole words — or a window of them
  int64_t nwords;
  int64_t base;           // index in the whole stream of words[0] (a window staged in LDS; 0 for the buffer itself)
};
constexpr int kWinWords = 11;  // words a subsequence's symbols can touch: <= 10 (a byte-aligned start, kSubBits
                               // bits, one more word for the window's second half); 11 keeps LDS rows on odd banks

// exit (or entry) record of a subsequence, 16 bytes: sk = slot | k << 8
struct Rec {
  int64_t bit;
  int32_t nblk;
  int32_t sk;
};
SP_ENT_HD bool same_state(const Rec& a, const Rec& b) { return a.bit == b.bit && a.sk == b.sk; }

constexpr uint8_t kNat[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// 32 bits of the stream from `bit` on, MSB first; reads are clamped to the padded buffer (zeros past it)
SP_ENT_HD uint32_t peek32(const Stream& s, int64_t bit) {
  const int64_t w = (bit >> 5) - s.base;
  if (w < 0 || w > s.nwords - 2) return 0;
  SP_ENT_BCHECK(w + 1, s.nwords);
  const uint64_t v = ((uint64_t)__builtin_bswap32(s.words[w]) << 32) | __builtin_bswap32(s.words[w + 1]);
  return (uint32_t)((v << (bit & 31)) >> 32);
}

// jdhuff.c HUFF_DECODE on a 32-bit window: the symbol and its code length (jpeg_host::huff_decode's paths)
SP_ENT_HD int huff_sym(const DevHuff& h, uint32_t w, int& len, int& err) {
  const uint16_t e = h.look[w >> (32 - kLook)];
  if (e >> 8) {
    len = e >> 8;
    return e & 0xFF;
  }
  const uint32_t code = w >> 16;
  int l = kLook + 1;
  while (l <= 16 && (int32_t)(code >> (16 - l)) > h.maxcode[l]) ++l;
  if (l > 16) {
    len = 16;
    err |= kStBadCode;
    return 0;
  }
  len = l;
  const int idx = (int)(code >> (16 - l)) + h.valoff[l];
  if (idx < 0 || idx >= 256) {
    err |= kStBadCode;
    return 0;
  }
  return h.vals[idx];
}

// the s magnitude bits after an l-bit code in window w (l + s <= 31), HUFF_EXTENDed
SP_ENT_HD int magnitude(uint32_t w, int l, int s) {
  if (s == 0) return 0;
  const int v = (int)((w << l) >> (32 - s));
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

struct NullSink {
  SP_ENT_HD void dc(int) {}
  SP_ENT_HD void ac(int, int) {}
  SP_ENT_HD void next_block() {}
  SP_ENT_HD bool expects_more() const { return false; }
};

struct SubResult {
  Rec exit;
  int err;
};

// Decode the symbols that begin in [entry.bit, sub_end) from state `entry`; tabs[2c] / tabs[2c + 1] are the DC /
// AC tables of component c. A block ends at EOB or past k = 63 (jdhuff.c decode_mcu). At a block boundary with
// fewer than 8 bits left in the segment, all ones, the rest is the encoder's padding (an all-ones prefix is
// never a code: build_huff refuses such tables), so the segment ends there — unless the write pass still expects
// blocks of this segment: then the next symbol is decoded from those bits and the zeros after them, which flags the
// overrun. Such a file is discarded either way; nothing is promised about its coefficients.
template <class Sink>
SP_ENT_HD SubResult decode_sub(const Stream& S, const DevHuff* tabs, const Geom& G, const Rec& entry, int64_t sub_end,
                               int64_t seg_end, Sink& sink) {
  int64_t bit = entry.bit;
  int slot = entry.sk & 0xFF, k = (entry.sk >> 8) & 0xFF;
  if (slot >= G.bpm) slot = 0;
  int nblk = 0, err = 0;
  while (bit < sub_end) {
    // past the segment's end the stream reads as zeros, as the host reader supplies them at a marker
    const int64_t left = seg_end - bit;
    const uint32_t w = left >= 32 ? peek32(S, bit) : peek32(S, bit) & ~(0xFFFFFFFFu >> left);
    const int c = (int)((G.slot_comp_bits >> (2 * slot)) & 3);
    int l;
    bool end = false;
    if (k == 0) {
      if (left < 8 && !sink.expects_more() && (w >> (32 - left)) == (1u << left) - 1) {
        bit = seg_end;
        break;
      }
      const int s = huff_sym(tabs[2 * c], w, l, err) & 15;
      bit += l + s;
      sink.dc(magnitude(w, l, s));
      k = 1;
    } else {
      const int rs = huff_sym(tabs[2 * c + 1], w, l, err);
      const int r = rs >> 4, sz = rs & 15;
      bit += l + sz;
      if (sz) {
        k += r;
        if (k > 63) {
          err |= kStBadCode;
          end = true;
        } else {
          sink.ac(k, magnitude(w, l, sz));
          end = ++k > 63;
        }
      } else if (r == 15) {
        k += 16;
        end = k > 63;
      } else {
        end = true;
      }
    }
    if (end) {
      k = 0;
      ++nblk;
      sink.next_block();
      slot = slot + 1 == G.bpm ? 0 : slot + 1;
    }
  }
  if (bit > seg_end) err |= kStOverrun;
  return SubResult{Rec{bit, nblk, slot | (k << 8)}, err};
}

// What the write pass checks where a segment ends (its last subsequence): the blocks completed are the segment's
// MCUs x blocks per MCU, and the decoder stands at a block boundary. Bytes after the last block that are no
// padding (8 bits or more, or not all ones) start a further block: finished, it is counted; unfinished, it leaves
// k != 0; running past the end, it is an overrun. The host decoder refuses such bytes as extraneous data.
SP_ENT_HD int segment_end_status(const Rec& exit, int64_t blocks, int64_t expected) {
  int st = 0;
  if (blocks != expected) st |= kStCount;
  if (((exit.sk >> 8) & 0xFF) != 0) st |= kStTail;
  return st;
}

// the restart segment of subsequence i: the last entry of segs[0 .. nseg) whose sub0 <= i
SP_ENT_HD int32_t find_seg(const SegEnt* segs, int64_t nseg, int64_t i) {
  int64_t lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (segs[mid].sub0 <= i) lo = mid;
    else hi = mid - 1;
  }
  return (int32_t)lo;
}

struct SubSpan {
  int64_t start, end, seg_end;
  bool first, last;
};
// segs has nseg + 1 entries: the last one closes the stream (bit = its end, mcu = nmcu, sub0 = nsub)
SP_ENT_HD SubSpan sub_span(const SegEnt* segs, int32_t seg, int64_t i) {
  const SegEnt a = segs[seg], b = segs[seg + 1];
  SubSpan s;
  s.start = a.bit + (i - a.sub0) * kSubBits;
  s.seg_end = b.bit;
  s.end = s.start + kSubBits < b.bit ? s.start + kSubBits : b.bit;
  s.first = i == a.sub0;
  s.last = i == (int64_t)b.sub0 - 1;
  return s;
}

// block (mcu, slot) of the scan → its index in the coefficient array (component-major, row-major blocks)
SP_ENT_HD int64_t block_index(const Geom& G, int64_t mcu, int slot) {
  const int c = G.slot_comp[slot];
  const int64_t my = mcu / G.mcux, mx = mcu - my * G.mcux;
  return G.block_off[c] + (my * G.comp_v[c] + G.slot_v[slot]) * G.bw[c] + mx * G.comp_h[c] + G.slot_h[slot];
}

// Write pass sink: coefficients at kNat[k] of the current block, the DC difference at [0]. Blocks at or past
// `limit` (the segment's last block + 1, in scan order) are not written: the count check reports them.
struct CoefSink {
  int16_t* coefs;
  const Geom* G;
  int64_t n, limit;  // scan-order block number, and its bound
  int64_t base;      // element offset of the current block, -1: none
  int64_t violations;
  SP_ENT_HD void seek() {
    base = -1;
    if (n >= 0 && n < limit) {
      const int64_t mcu = n / G->bpm;
      const int64_t b = block_index(*G, mcu, (int)(n - mcu * G->bpm));
      SP_ENT_BCHECK(b, G->total_blocks);
      if (b >= 0 && b < G->total_blocks) base = b * 64;
      else ++violations;
    }
  }
  SP_ENT_HD void dc(int v) {
    if (base >= 0) coefs[base] = (int16_t)v;
  }
  SP_ENT_HD void ac(int k, int v) {
    if (base >= 0) coefs[base + kNat[k & 63]] = (int16_t)v;
  }
  SP_ENT_HD void next_block() {
    ++n;
    seek();
  }
  SP_ENT_HD bool expects_more() const { return n < limit; }
};

// DC pass geometry: chunks of kDcChunk MCUs that never cross a restart boundary
SP_ENT_HD int64_t dc_chunks_per_seg(const Geom& G) {
  const int64_t ri = G.ri > 0 ? G.ri : G.nmcu;
  return (ri + kDcChunk - 1) / kDcChunk;
}
SP_ENT_HD int64_t dc_nseg(const Geom& G) { return G.ri > 0 ? (G.nmcu + G.ri - 1) / G.ri : 1; }
SP_ENT_HD void dc_chunk_span(const Geom& G, int64_t g, int64_t& m0, int64_t& m1, bool& seg_first) {
  const int64_t ri = G.ri > 0 ? G.ri : G.nmcu, cps = dc_chunks_per_seg(G);
  const int64_t seg = g / cps, j = g - seg * cps;
  m0 = seg * ri + j * kDcChunk;
  m1 = m0 + kDcChunk;
  if (m1 > (seg + 1) * ri) m1 = (seg + 1) * ri;
  if (m1 > G.nmcu) m1 = G.nmcu;
  if (m0 > m1) m0 = m1;
  seg_first = j == 0;
}

// device workspace layout (bytes), shared by the packer (work_bytes), the kernels and the emulation
struct WorkLayout {
  int64_t entry, exit0, exit1, segid, cnt, dcs, bytes;
};
SP_ENT_HD WorkLayout work_layout(int64_t nsub, int64_t nchunk) {
  WorkLayout w;
  int64_t o = 0;
  w.entry = o, o += nsub * 16;
  w.exit0 = o, o += nsub * 16;
  w.exit1 = o, o += nsub * 16;
  w.cnt = o, o += (nsub + 1) * 8;
  w.dcs = o, o += (nchunk + 1) * 3 * 8;
  w.segid = o, o += (nsub + 1) / 2 * 8;
  w.bytes = o;
  return w;
}

}  // namespace jpeg_entropy
}  // namespace sp
