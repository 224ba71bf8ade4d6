// Label drawing on the device image: the pixel half of Pillow's ImageDraw for serve.py:119-137.
//
// Restates ImagingDrawRectangle's fills (Draw.c hline32 / point32: the pixel's bytes = the ink's) and
// ImagingFill2 with an "L" mask (Paste.c fill_mask_L: per channel BLEND8 = DIV255(out * (255 - m) + ink * m), one
// rounding of the sum). The Python half — colours, text layout, anchors, stroke then fill — stays Pillow's
// (spotter_amd/draw.py records the calls its C core object would receive). Bit-exact.
//
// The operations composite in list order and the blend does not commute, so one launch keeps the order per
// pixel instead of one launch per operation: sp_draw_pack (host) bins the operations into the 64 x 8 pixel
// tiles they touch; sp_draw_rgb launches one workgroup per touched tile, every thread owns four adjacent pixels
// of one tile row (12 bytes: three aligned dwords where the row allows), holds them in registers and walks the
// tile's operations in list order. The operation records are uniform across the workgroup (scalar loads).
#include <algorithm>
#include <vector>

#include "common.h"

namespace sp {
namespace {

constexpr int kTileW = SP_DRAW_TILE_W;
constexpr int kTileH = SP_DRAW_TILE_H;
constexpr int kPix = 4;                                  // adjacent pixels per thread
constexpr int kThreads = (kTileW / kPix) * kTileH;       // 128
static_assert(kTileW % kPix == 0 && kThreads % kWave == 0, "tile / thread mapping");

struct DrawArgs {
  uint8_t* rgb;
  int h, w;
  int64_t stride;
  const sp_draw_op* ops;
  const sp_draw_tile* tiles;
  const int32_t* refs;
  const uint8_t* masks;
  int n_ops, n_tiles, n_refs;
  int64_t mask_bytes;
};

// ImagingUtils.h BLEND8: DIV255(out * (255 - m) + ink * m), DIV255(a) = (t = a + 128, ((t >> 8) + t) >> 8)
__device__ __forceinline__ uint32_t blend8(uint32_t m, uint32_t out, uint32_t ink) {
  const uint32_t t = out * (255u - m) + ink * m + 128u;
  return ((t >> 8) + t) >> 8;
}

// One workgroup's work: touched tile `t` of the image `a` describes. Shared by the single-image and the batched kernel,
// so both write the same pixels by construction.
__device__ __forceinline__ void draw_tile(const DrawArgs& a, const int t) {
  SP_BCHECK(t, a.n_tiles);
  const sp_draw_tile tile = a.tiles[t];
  const int y = tile.ty * kTileH + (int)threadIdx.x / (kTileW / kPix);
  const int x = tile.tx * kTileW + ((int)threadIdx.x % (kTileW / kPix)) * kPix;
  if (y >= a.h || x >= a.w) return;
  const int npx = min(kPix, a.w - x);
  const int64_t off = (int64_t)y * a.stride + (int64_t)x * 3;
  const int64_t extent = (int64_t)(a.h - 1) * a.stride + (int64_t)a.w * 3;
  SP_BCHECK(off, extent);
  SP_BCHECK(off + npx * 3 - 1, extent);
  uint8_t* p = a.rgb + off;
  // x*3 is a multiple of 12, so the four pixels are three aligned dwords whenever the row start is aligned
  const bool dwords = npx == kPix && (reinterpret_cast<uintptr_t>(p) & 3) == 0;
  uint32_t c[kPix * 3];
  if (dwords) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
    const uint32_t u[3] = {q[0], q[1], q[2]};
#pragma unroll
    for (int i = 0; i < kPix * 3; ++i) c[i] = (u[i >> 2] >> (8 * (i & 3))) & 255u;
  } else {
#pragma unroll
    for (int i = 0; i < kPix * 3; ++i) c[i] = i < npx * 3 ? p[i] : 0u;
  }
  bool dirty = false;
  SP_BCHECK(tile.first, a.n_refs);
  SP_BCHECK(tile.first + tile.count - 1, a.n_refs);
  for (int r = tile.first; r < tile.first + tile.count; ++r) {
    const int oi = a.refs[r];
    SP_BCHECK(oi, a.n_ops);
    const sp_draw_op op = a.ops[oi];
    if (y < op.y0 || y > op.y1 || x > op.x1 || x + kPix - 1 < op.x0) continue;
    const uint32_t ink[3] = {op.ink & 255u, (op.ink >> 8) & 255u, (op.ink >> 16) & 255u};
    if (op.kind == SP_DRAW_FILL) {
#pragma unroll
      for (int k = 0; k < kPix; ++k) {
        if (x + k >= op.x0 && x + k <= op.x1) {
          c[3 * k] = ink[0];
          c[3 * k + 1] = ink[1];
          c[3 * k + 2] = ink[2];
          dirty = true;
        }
      }
    } else {
      const int64_t mrow = op.mask_off + ((int64_t)op.sy + (y - op.y0)) * op.mask_stride + ((int64_t)op.sx - op.x0);
#pragma unroll
      for (int k = 0; k < kPix; ++k) {
        if (x + k >= op.x0 && x + k <= op.x1) {
          SP_BCHECK(mrow + x + k, a.mask_bytes);
          const uint32_t m = a.masks[mrow + x + k];
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) c[3 * k + ch] = blend8(m, c[3 * k + ch], ink[ch]);
          dirty = true;
        }
      }
    }
  }
  if (!dirty) return;
  if (dwords) {
    uint32_t u[3] = {0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < kPix * 3; ++i) u[i >> 2] |= (c[i] & 255u) << (8 * (i & 3));
    uint32_t* q = reinterpret_cast<uint32_t*>(p);
    q[0] = u[0];
    q[1] = u[1];
    q[2] = u[2];
  } else {
#pragma unroll
    for (int i = 0; i < kPix * 3; ++i)
      if (i < npx * 3) p[i] = (uint8_t)c[i];
  }
}

__global__ __launch_bounds__(kThreads) void draw_kernel(const DrawArgs a) { draw_tile(a, (int)blockIdx.x); }

// The batch: the workgroup finds its image's row (uniform binary search over first_wg), builds that image's DrawArgs
// from the row and from the table header at tables + table_off (both uniform across the workgroup: scalar loads) and
// runs the single-image body on its own tile of it. The extents SP_BCHECK sees are the image's own, not the buffer's.
__global__ __launch_bounds__(kThreads) void draw_batch_kernel(const sp_draw_batch_item* __restrict__ items, const int n,
                                                              const uint8_t* __restrict__ tables) {
  const int img = batch_image(items, n, &sp_draw_batch_item::first_wg, (int)blockIdx.x);
  SP_BCHECK(img, n);
  const sp_draw_batch_item it = items[img];
  const uint8_t* tb = tables + it.table_off;
  const sp_draw_table hd = *reinterpret_cast<const sp_draw_table*>(tb);
  DrawArgs a;
  a.rgb = it.rgb;
  a.h = it.height;
  a.w = it.width;
  a.stride = it.row_stride;
  a.ops = reinterpret_cast<const sp_draw_op*>(tb + hd.ops_off);
  a.tiles = reinterpret_cast<const sp_draw_tile*>(tb + hd.tiles_off);
  a.refs = reinterpret_cast<const int32_t*>(tb + hd.refs_off);
  a.masks = tb + hd.masks_off;
  a.n_ops = hd.n_ops;
  a.n_tiles = hd.n_tiles;
  a.n_refs = hd.n_refs;
  a.mask_bytes = hd.mask_bytes;
  draw_tile(a, (int)blockIdx.x - it.first_wg);
}

inline int64_t align16(int64_t v) { return (v + 15) & ~int64_t(15); }

}  // namespace
}  // namespace sp

extern "C" int sp_draw_pack(const sp_draw_op* ops, int32_t n_ops, const uint8_t* masks, int64_t mask_bytes,
                            int32_t height, int32_t width, void* out, int64_t out_cap, int64_t* need) {
  using namespace sp;
  SP_ARG_CHECK(need && n_ops >= 0 && mask_bytes >= 0 && (ops || n_ops == 0) && (masks || mask_bytes == 0),
               "sp_draw_pack: null args");
  SP_ARG_CHECK(height > 0 && width > 0, "sp_draw_pack: bad image size %dx%d", width, height);
  const int tw = (width + kTileW - 1) / kTileW, th = (height + kTileH - 1) / kTileH;
  for (int i = 0; i < n_ops; ++i) {
    const sp_draw_op& o = ops[i];
    SP_ARG_CHECK(o.x0 >= 0 && o.x0 <= o.x1 && o.x1 < width && o.y0 >= 0 && o.y0 <= o.y1 && o.y1 < height,
                 "sp_draw_pack: operation %d (%d, %d)-(%d, %d) outside the %dx%d image", i, o.x0, o.y0, o.x1, o.y1,
                 width, height);
  }
  // pass 1: operations per tile (host scratch kept per thread: a planning call, like sp_jpeg_enc_plan)
  thread_local std::vector<int32_t> cnt;
  cnt.assign((size_t)tw * th, 0);
  int64_t n_refs = 0;
  for (int i = 0; i < n_ops; ++i) {
    const sp_draw_op& o = ops[i];
    for (int ty = o.y0 / kTileH; ty <= o.y1 / kTileH; ++ty)
      for (int tx = o.x0 / kTileW; tx <= o.x1 / kTileW; ++tx) ++cnt[(size_t)ty * tw + tx];
    n_refs += (int64_t)(o.y1 / kTileH - o.y0 / kTileH + 1) * (o.x1 / kTileW - o.x0 / kTileW + 1);
  }
  SP_ARG_CHECK(n_refs < (int64_t(1) << 31), "sp_draw_pack: too many tile references");
  int64_t n_tiles = 0;
  for (size_t t = 0; t < cnt.size(); ++t) n_tiles += cnt[t] != 0;
  sp_draw_table hd;
  memset(&hd, 0, sizeof(hd));
  hd.n_ops = n_ops;
  hd.n_tiles = (int32_t)n_tiles;
  hd.n_refs = (int32_t)n_refs;
  hd.height = height;
  hd.width = width;
  hd.ops_off = align16(sizeof(sp_draw_table));
  hd.tiles_off = align16(hd.ops_off + (int64_t)n_ops * sizeof(sp_draw_op));
  hd.refs_off = align16(hd.tiles_off + n_tiles * (int64_t)sizeof(sp_draw_tile));
  hd.masks_off = align16(hd.refs_off + n_refs * (int64_t)sizeof(int32_t));
  hd.mask_bytes = mask_bytes;
  hd.total_bytes = align16(hd.masks_off + mask_bytes);
  *need = hd.total_bytes;
  if (!out || out_cap < hd.total_bytes) return 0;
  uint8_t* base = static_cast<uint8_t*>(out);
  memcpy(base, &hd, sizeof(hd));
  if (n_ops) memcpy(base + hd.ops_off, ops, (size_t)n_ops * sizeof(sp_draw_op));
  if (mask_bytes) memcpy(base + hd.masks_off, masks, (size_t)mask_bytes);
  // pass 2: the touched tiles in (ty, tx) order, their ref ranges back to back; cnt becomes each tile's cursor
  sp_draw_tile* tiles = reinterpret_cast<sp_draw_tile*>(base + hd.tiles_off);
  int32_t* refs = reinterpret_cast<int32_t*>(base + hd.refs_off);
  int32_t first = 0, nt = 0;
  for (int ty = 0; ty < th; ++ty)
    for (int tx = 0; tx < tw; ++tx) {
      int32_t& c = cnt[(size_t)ty * tw + tx];
      if (!c) continue;
      tiles[nt++] = sp_draw_tile{tx, ty, first, c};
      const int32_t n = c;
      c = first;
      first += n;
    }
  // pass 3: operation indices in list order, so every tile's refs ascend
  for (int i = 0; i < n_ops; ++i) {
    const sp_draw_op& o = ops[i];
    for (int ty = o.y0 / kTileH; ty <= o.y1 / kTileH; ++ty)
      for (int tx = o.x0 / kTileW; tx <= o.x1 / kTileW; ++tx) refs[cnt[(size_t)ty * tw + tx]++] = i;
  }
  return 0;
}

// Every check sp_draw_rgb and sp_draw_batch_rgb make of one image and the host copy of its packed table before
// anything launches; *out is the table's header. `fn` names the entry point in the message.
static int check_table(const char* fn, const uint8_t* rgb, int32_t height, int32_t width, int64_t row_stride,
                       const void* table_host, int64_t table_bytes, sp_draw_table* out) {
  using namespace sp;
  SP_ARG_CHECK(rgb && table_host, "%s: null args", fn);
  SP_ARG_CHECK(height > 0 && width > 0 && row_stride >= (int64_t)3 * width, "%s: bad image %dx%d stride %lld", fn,
               width, height, (long long)row_stride);
  SP_ARG_CHECK(table_bytes >= (int64_t)sizeof(sp_draw_table), "%s: table shorter than its header", fn);
  sp_draw_table hd;
  memcpy(&hd, table_host, sizeof(hd));
  SP_ARG_CHECK(hd.height == height && hd.width == width, "%s: table packed for %dx%d, image is %dx%d", fn, hd.width,
               hd.height, width, height);
  SP_ARG_CHECK(hd.n_ops >= 0 && hd.n_tiles >= 0 && hd.n_refs >= 0 && hd.mask_bytes >= 0 &&
                   hd.total_bytes <= table_bytes,
               "%s: bad table counts", fn);
  auto section = [&](int64_t off, int64_t bytes) {
    return off >= (int64_t)sizeof(sp_draw_table) && off % 16 == 0 && bytes >= 0 && off <= hd.total_bytes &&
           bytes <= hd.total_bytes - off;
  };
  SP_ARG_CHECK(section(hd.ops_off, (int64_t)hd.n_ops * sizeof(sp_draw_op)) &&
                   section(hd.tiles_off, (int64_t)hd.n_tiles * sizeof(sp_draw_tile)) &&
                   section(hd.refs_off, (int64_t)hd.n_refs * sizeof(int32_t)) && section(hd.masks_off, hd.mask_bytes),
               "%s: a table section lies outside the table", fn);
  const uint8_t* hb = static_cast<const uint8_t*>(table_host);
  const sp_draw_op* ops = reinterpret_cast<const sp_draw_op*>(hb + hd.ops_off);
  const sp_draw_tile* tiles = reinterpret_cast<const sp_draw_tile*>(hb + hd.tiles_off);
  const int32_t* refs = reinterpret_cast<const int32_t*>(hb + hd.refs_off);
  for (int i = 0; i < hd.n_ops; ++i) {
    const sp_draw_op& o = ops[i];
    SP_ARG_CHECK(o.kind == SP_DRAW_FILL || o.kind == SP_DRAW_BLEND, "%s: operation %d has kind %d", fn, i, o.kind);
    SP_ARG_CHECK(o.x0 >= 0 && o.x0 <= o.x1 && o.x1 < width && o.y0 >= 0 && o.y0 <= o.y1 && o.y1 < height,
                 "%s: operation %d (%d, %d)-(%d, %d) outside the %dx%d image", fn, i, o.x0, o.y0, o.x1, o.y1, width,
                 height);
    if (o.kind == SP_DRAW_BLEND) {
      // first and last mask byte the rectangle reads (rows sy .. sy + y1 - y0, columns sx .. sx + x1 - x0)
      SP_ARG_CHECK(o.mask_stride >= 0 && o.sx >= 0 && o.sy >= 0 && o.mask_off >= 0 && o.mask_off <= hd.mask_bytes,
                   "%s: operation %d has a negative mask field", fn, i);
      const int64_t last = o.mask_off + ((int64_t)o.sy + (o.y1 - o.y0)) * o.mask_stride + o.sx + (o.x1 - o.x0);
      SP_ARG_CHECK(last < hd.mask_bytes, "%s: operation %d reads mask byte %lld of %lld", fn, i, (long long)last,
                   (long long)hd.mask_bytes);
    }
  }
  const int tw = (width + kTileW - 1) / kTileW, th = (height + kTileH - 1) / kTileH;
  int64_t next = 0, prev_key = -1;
  for (int t = 0; t < hd.n_tiles; ++t) {
    const sp_draw_tile& tl = tiles[t];
    SP_ARG_CHECK(tl.tx >= 0 && tl.tx < tw && tl.ty >= 0 && tl.ty < th, "%s: tile %d (%d, %d) outside the image", fn, t,
                 tl.tx, tl.ty);
    const int64_t key = (int64_t)tl.ty * tw + tl.tx;
    SP_ARG_CHECK(key > prev_key, "%s: tile %d repeats or is out of order", fn, t);
    prev_key = key;
    SP_ARG_CHECK(tl.count > 0 && tl.first == next && (int64_t)tl.first + tl.count <= hd.n_refs,
                 "%s: tile %d has an unordered reference range [%d, +%d)", fn, t, tl.first, tl.count);
    next = (int64_t)tl.first + tl.count;
    for (int r = tl.first; r < tl.first + tl.count; ++r) {
      SP_ARG_CHECK(refs[r] >= 0 && refs[r] < hd.n_ops, "%s: tile %d references operation %d of %d", fn, t, refs[r],
                   hd.n_ops);
      SP_ARG_CHECK(r == tl.first || refs[r] > refs[r - 1], "%s: tile %d lists its operations out of order", fn, t);
    }
  }
  *out = hd;
  return 0;
}

extern "C" int sp_draw_rgb(uint8_t* rgb, int32_t height, int32_t width, int64_t row_stride, const void* table_host,
                           const void* table_dev, int64_t table_bytes, void* stream) {
  using namespace sp;
  SP_ARG_CHECK(table_dev, "sp_draw_rgb: null args");
  sp_draw_table hd;
  if (check_table("sp_draw_rgb", rgb, height, width, row_stride, table_host, table_bytes, &hd)) return -1;
  if (hd.n_tiles == 0) return 0;
  const uint8_t* db = static_cast<const uint8_t*>(table_dev);
  DrawArgs a;
  a.rgb = rgb;
  a.h = height;
  a.w = width;
  a.stride = row_stride;
  a.ops = reinterpret_cast<const sp_draw_op*>(db + hd.ops_off);
  a.tiles = reinterpret_cast<const sp_draw_tile*>(db + hd.tiles_off);
  a.refs = reinterpret_cast<const int32_t*>(db + hd.refs_off);
  a.masks = db + hd.masks_off;
  a.n_ops = hd.n_ops;
  a.n_tiles = hd.n_tiles;
  a.n_refs = hd.n_refs;
  a.mask_bytes = hd.mask_bytes;
  hipLaunchKernelGGL(draw_kernel, dim3(hd.n_tiles), dim3(kThreads), 0, as_stream(stream), a);
  return check_launch("sp_draw_rgb");
}

extern "C" int64_t sp_draw_batch_plan(sp_draw_batch_item* items, int n, const void* tables_host,
                                      int64_t tables_bytes) {
  using namespace sp;
  SP_ARG_CHECK(items && tables_host, "sp_draw_batch_plan: null args");
  SP_ARG_CHECK(n >= 1 && n <= SP_DRAW_BATCH_MAX, "sp_draw_batch_plan: n = %d outside [1, %d]", n, SP_DRAW_BATCH_MAX);
  int64_t wg = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t off = items[i].table_off;
    SP_ARG_CHECK(off >= 0 && off % 16 == 0 && tables_bytes >= (int64_t)sizeof(sp_draw_table) &&
                     off <= tables_bytes - (int64_t)sizeof(sp_draw_table),
                 "sp_draw_batch_plan: image %d: table offset %lld misaligned or outside the %lld-byte buffer", i,
                 (long long)off, (long long)tables_bytes);
    sp_draw_table hd;
    memcpy(&hd, static_cast<const uint8_t*>(tables_host) + off, sizeof(hd));
    SP_ARG_CHECK(hd.n_tiles > 0, "sp_draw_batch_plan: image %d: its table has %d touched tiles", i, hd.n_tiles);
    wg += hd.n_tiles;
    SP_ARG_CHECK(wg < (int64_t(1) << 31), "sp_draw_batch_plan: more than 2^31 - 1 workgroups");
  }
  wg = 0;
  for (int i = 0; i < n; ++i) {  // (written only once every row has passed)
    sp_draw_table hd;
    memcpy(&hd, static_cast<const uint8_t*>(tables_host) + items[i].table_off, sizeof(hd));
    items[i].n_tiles = hd.n_tiles;
    items[i].first_wg = (int32_t)wg;
    wg += hd.n_tiles;
  }
  return wg;
}

extern "C" int sp_draw_batch_rgb(const sp_draw_batch_item* items_dev, const sp_draw_batch_item* items_host, int n,
                                 const void* tables_host, const void* tables_dev, int64_t tables_bytes,
                                 void* stream) {
  using namespace sp;
  SP_ARG_CHECK(items_dev && items_host && tables_host && tables_dev, "sp_draw_batch_rgb: null args");
  SP_ARG_CHECK(n >= 1 && n <= SP_DRAW_BATCH_MAX, "sp_draw_batch_rgb: n = %d outside [1, %d]", n, SP_DRAW_BATCH_MAX);
  SP_ARG_CHECK(reinterpret_cast<uintptr_t>(items_dev) % 8 == 0 && reinterpret_cast<uintptr_t>(tables_dev) % 16 == 0,
               "sp_draw_batch_rgb: misaligned device table");
  int64_t wg = 0;
  for (int i = 0; i < n; ++i) {
    const sp_draw_batch_item& it = items_host[i];
    SP_ARG_CHECK(it.table_off >= 0 && it.table_off % 16 == 0 && it.table_bytes >= 0 && it.table_off <= tables_bytes &&
                     it.table_bytes <= tables_bytes - it.table_off,
                 "sp_draw_batch_rgb: image %d: table range [%lld, +%lld) misaligned or outside the %lld-byte buffer", i,
                 (long long)it.table_off, (long long)it.table_bytes, (long long)tables_bytes);
    sp_draw_table hd;
    if (check_table("sp_draw_batch_rgb", it.rgb, it.height, it.width, it.row_stride,
                    static_cast<const uint8_t*>(tables_host) + it.table_off, it.table_bytes, &hd)) {
      char msg[400];
      snprintf(msg, sizeof(msg), "%s", sp_last_error());
      set_error("image %d: %s", i, msg);
      return -1;
    }
    SP_ARG_CHECK(it.n_tiles > 0 && it.n_tiles == hd.n_tiles,
                 "sp_draw_batch_rgb: image %d: n_tiles %d, its table has %d (an image without draws is left out)", i,
                 it.n_tiles, hd.n_tiles);
    SP_ARG_CHECK(it.first_wg == wg, "sp_draw_batch_rgb: image %d: first_wg %d is not the prefix sum %lld", i,
                 it.first_wg, (long long)wg);
    wg += it.n_tiles;
    SP_ARG_CHECK(wg < (int64_t(1) << 31), "sp_draw_batch_rgb: more than 2^31 - 1 workgroups");
    // pairwise disjoint table ranges and pixel byte ranges (n <= 64: the quadratic check is a few thousand compares)
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(it.rgb);
    const uintptr_t p1 = p0 + (uintptr_t)((int64_t)(it.height - 1) * it.row_stride + (int64_t)3 * it.width);
    for (int j = 0; j < i; ++j) {
      const sp_draw_batch_item& o = items_host[j];
      SP_ARG_CHECK(it.table_off + it.table_bytes <= o.table_off || o.table_off + o.table_bytes <= it.table_off,
                   "sp_draw_batch_rgb: the tables of images %d and %d overlap", j, i);
      const uintptr_t q0 = reinterpret_cast<uintptr_t>(o.rgb);
      const uintptr_t q1 = q0 + (uintptr_t)((int64_t)(o.height - 1) * o.row_stride + (int64_t)3 * o.width);
      SP_ARG_CHECK(p1 <= q0 || q1 <= p0, "sp_draw_batch_rgb: images %d and %d share pixel bytes", j, i);
    }
  }
  hipLaunchKernelGGL(draw_batch_kernel, dim3((unsigned)wg), dim3(kThreads), 0, as_stream(stream), items_dev, n,
                     static_cast<const uint8_t*>(tables_dev));
  return check_launch("sp_draw_batch_rgb");
}
