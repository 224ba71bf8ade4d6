// AddressSanitizer + UBSan harness for the host half of the batched JPEG decode (spotter_amd/csrc/jpeg_host.h
// batch_plan, the body of sp_jpeg_batch_plan): the layouts of a corpus of files, as the parser fills them, planned
// in batches of every size the record count allows, into exact-size heap arrays. Built and run on the CPU:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
//       tools/sanitize/jpeg_batch_plan.cpp -o <out>
//   <out> corpus.bin        (corpus.bin: tests/jpeg_corpus.py pack(): [uint32 little-endian length][bytes] records)
//
// Prints "<layouts> <plans> <refused>" and checks every accepted plan: aligned offsets, ranges in order inside the
// totals, prefix columns that sum the per-image workgroup counts. Exit status 1 on a broken plan.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../spotter_amd/csrc/jpeg_host.h"

namespace sp {
static char g_err[512];
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
}  // namespace sp

static bool plan_ok(const std::vector<sp_jpeg_layout>& lays, const std::vector<sp_jpeg_batch_item>& items,
                    const sp_jpeg_batch_totals& t) {
  int64_t coef = 0, work = 0, rgb = 0, wi = 0, wc = 0;
  for (size_t i = 0; i < lays.size(); ++i) {
    const sp_jpeg_batch_item& it = items[i];
    const sp_jpeg_layout& L = lays[i];
    if (memcmp(&it.lay, &L, sizeof(L)) != 0) return false;
    if (it.coef_off < coef || it.work_off < work || it.rgb_off < rgb) return false;
    if ((it.work_off & 15) || (it.rgb_off & 255) || it.rgb_stride != 3LL * L.width) return false;
    if (it.first_wg_idct != wi || it.first_wg_color != wc) return false;
    coef = it.coef_off + L.total_blocks * 64;
    work = it.work_off + L.plane_bytes;
    rgb = it.rgb_off + it.rgb_stride * L.height;
    wi += (L.total_blocks + 31) / 32;
    wc += ((int64_t)L.width * L.height + 1023) / 1024;
  }
  return coef <= t.coef_elems && work <= t.work_bytes && rgb <= t.rgb_bytes && wi == t.wg_idct && wc == t.wg_color;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s corpus.bin\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> all;
  uint8_t tmp[65536];
  size_t n;
  while ((n = fread(tmp, 1, sizeof(tmp), f)) > 0) all.insert(all.end(), tmp, tmp + n);
  fclose(f);
  std::vector<sp_jpeg_layout> lays;  // every layout the parser accepts, huge frames included
  size_t pos = 0;
  while (pos + 4 <= all.size()) {
    const uint32_t len = all[pos] | (all[pos + 1] << 8) | (all[pos + 2] << 16) | ((uint32_t)all[pos + 3] << 24);
    pos += 4;
    if (pos + len > all.size()) return 3;
    std::vector<uint8_t> rec(all.begin() + pos, all.begin() + pos + len);
    pos += len;
    sp_jpeg_layout lay;
    memset(&lay, 0, sizeof(lay));
    sp::jpeg_host::Decoder d{rec.data(), (int64_t)rec.size(), &lay, nullptr};
    if (!rec.empty() && d.run(false) == 0) lays.push_back(lay);
  }
  long plans = 0, refused = 0;
  sp_jpeg_batch_totals tot;
  // batches of 1, 2, 3, ... SP_JPEG_BATCH_MAX + 1 consecutive layouts, sliding through the list
  for (size_t start = 0, size = 1; start < lays.size(); start += size, size = size % (SP_JPEG_BATCH_MAX + 1) + 1) {
    const size_t cnt = start + size <= lays.size() ? size : lays.size() - start;
    std::vector<sp_jpeg_layout> in(lays.begin() + start, lays.begin() + start + cnt);
    std::vector<sp_jpeg_batch_item> items(cnt);  // exact size: ASan sees a write past the n-th row
    const int rc = sp::jpeg_host::batch_plan(in.data(), (int)cnt, items.data(), &tot);
    if (rc == 0 && cnt > SP_JPEG_BATCH_MAX) return 1;
    if (rc == 0 && !plan_ok(in, items, tot)) return 1;
    rc == 0 ? ++plans : ++refused;
  }
  // damaged layouts: one field of an accepted layout overwritten by each of a few extreme values
  const int32_t bad[] = {0, -1, 1, 3, 5, INT32_MAX, INT32_MIN};
  for (size_t i = 0; i < lays.size(); i += 7) {
    for (size_t field = 0; field < offsetof(sp_jpeg_layout, quant) / 4; ++field)
      for (int32_t v : bad) {
        std::vector<sp_jpeg_layout> in(1, lays[i]);
        reinterpret_cast<int32_t*>(in.data())[field] = v;
        std::vector<sp_jpeg_batch_item> items(1);
        const int rc = sp::jpeg_host::batch_plan(in.data(), 1, items.data(), &tot);
        if (rc == 0 && !plan_ok(in, items, tot)) return 1;
        rc == 0 ? ++plans : ++refused;
      }
  }
  if (sp::jpeg_host::batch_plan(nullptr, 1, nullptr, &tot) != -1) return 1;
  printf("%zu %ld %ld\n", lays.size(), plans, refused);
  return lays.empty() ? 1 : 0;
}
