// AddressSanitizer + UBSan harness for the host half of the batched JPEG encode (spotter_amd/csrc/jpeg_host.h
// enc_batch_plan and enc_batch_check, the bodies of sp_jpeg_enc_batch_plan and of sp_jpeg_enc_batch_rgb's argument
// check): layouts of a grid of sizes, qualities and subsamplings planned in batches of every size into exact-size
// heap arrays, then damaged layouts and damaged table rows. Built and run on the CPU:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
//       tools/sanitize/jpeg_enc_batch_plan.cpp -o <out>
//   <out>
//
// Prints "<layouts> <accepted> <refused>". Exit status 1 on a broken plan or a damaged table the check lets through.
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

using sp::jpeg_host::enc_batch_check;
using sp::jpeg_host::enc_batch_plan;

static bool plan_ok(const std::vector<sp_jpeg_enc_layout>& lays, const std::vector<sp_jpeg_enc_batch_item>& items,
                    const sp_jpeg_enc_batch_totals& t) {
  int64_t work = 0, cap = 0, wf = 0, wm = 0;
  for (size_t i = 0; i < lays.size(); ++i) {
    const sp_jpeg_enc_batch_item& it = items[i];
    const sp_jpeg_enc_layout& L = lays[i];
    const int64_t nmcu = (int64_t)L.mcux * L.mcuy;
    if (memcmp(&it.lay, &L, sizeof(L)) != 0) return false;
    if (it.work_off < work || (it.work_off & 255) || it.first_wg_fdct != wf || it.first_wg_mcu != wm) return false;
    work = it.work_off + L.work_bytes;
    cap += (L.bits_cap + 15) & ~15LL;
    wf += (nmcu + 3) / 4;
    wm += (nmcu + 255) / 256;
  }
  return work <= t.work_bytes && cap == t.bits_cap && wf == t.wg_fdct && wm == t.wg_mcu;
}

int main() {
  const int sizes[] = {1, 7, 8, 9, 16, 17, 255, 256, 257, 640, 717, 1200, 2056, 8200, 65500};
  const int quals[] = {-1, 1, 50, 100};
  std::vector<sp_jpeg_enc_layout> lays;
  for (int w : sizes)
    for (int h : sizes)
      for (int q : quals)
        for (int sub = -1; sub <= 2; ++sub) {
          sp_jpeg_enc_layout lay;
          if (sp::jpeg_host::enc_plan(w, h, q, sub, &lay) == 0) lays.push_back(lay);
        }
  long accepted = 0, refused = 0;
  sp_jpeg_enc_batch_totals tot;
  uint8_t pixel = 0;
  // batches of 1, 2, 3, ... SP_JPEG_BATCH_MAX + 1 consecutive layouts, sliding through the list
  for (size_t start = 0, size = 1; start < lays.size(); start += size, size = size % (SP_JPEG_BATCH_MAX + 1) + 1) {
    const size_t cnt = start + size <= lays.size() ? size : lays.size() - start;
    std::vector<sp_jpeg_enc_layout> in(lays.begin() + start, lays.begin() + start + cnt);
    std::vector<sp_jpeg_enc_batch_item> items(cnt);  // exact size: ASan sees a write past the n-th row
    const int rc = enc_batch_plan(in.data(), (int)cnt, items.data(), &tot);
    if (rc == 0 && (cnt > SP_JPEG_BATCH_MAX || !plan_ok(in, items, tot))) return 1;
    rc == 0 ? ++accepted : ++refused;
    if (rc) continue;
    for (size_t i = 0; i < cnt; ++i) {
      items[i].src = &pixel;
      items[i].pixel_bytes = 3 + (int)(i & 1);
      items[i].row_stride = (int64_t)items[i].pixel_bytes * in[i].width + (int64_t)(i % 3);
    }
    if (enc_batch_check(items.data(), (int)cnt, &tot, tot.work_bytes, tot.bits_cap) != 0) return 1;
    // damaged rows: each must be refused
    const size_t k = cnt / 2;
    const sp_jpeg_enc_batch_item keep = items[k];
    for (int what = 0; what < 8; ++what) {
      sp_jpeg_enc_batch_item& it = items[k];
      switch (what) {
        case 0: it.src = nullptr; break;
        case 1: it.pixel_bytes = 5; break;
        case 2: it.row_stride = (int64_t)it.pixel_bytes * it.lay.width - 1; break;
        case 3: it.work_off += 16; break;
        case 4: it.work_off = INT64_MAX - 255; break;
        case 5: it.first_wg_fdct += 1; break;
        case 6: it.first_wg_mcu = INT32_MIN; break;
        case 7: it.work_off = -256; break;
      }
      if (enc_batch_check(items.data(), (int)cnt, &tot, tot.work_bytes, tot.bits_cap) != -1) return 1;
      ++refused;
      items[k] = keep;
    }
    if (cnt > 1) {
      items[cnt - 1].work_off = items[0].work_off;  // overlapping workspaces
      if (enc_batch_check(items.data(), (int)cnt, &tot, tot.work_bytes, tot.bits_cap) != -1) return 1;
      ++refused;
    }
  }
  // damaged layouts: one 32-bit word of an accepted layout's scalar fields overwritten by each of a few extreme values
  const int32_t bad[] = {0, -1, 1, 3, 5, INT32_MAX, INT32_MIN};
  for (size_t i = 0; i < lays.size(); i += 5)
    for (size_t field = 0; field < offsetof(sp_jpeg_enc_layout, quant) / 4; ++field)
      for (int32_t v : bad) {
        std::vector<sp_jpeg_enc_layout> in(1, lays[i]);
        if (reinterpret_cast<int32_t*>(in.data())[field] == v) continue;
        reinterpret_cast<int32_t*>(in.data())[field] = v;
        std::vector<sp_jpeg_enc_batch_item> items(1);
        // refused unless the damaged bytes are enc_plan's layout of the damaged parameters (7 -> 5 pixels wide)
        const int rc = enc_batch_plan(in.data(), 1, items.data(), &tot);
        if (rc == 0 && !plan_ok(in, items, tot)) return 1;
        rc == 0 ? ++accepted : ++refused;
      }
  if (enc_batch_plan(nullptr, 1, nullptr, &tot) != -1 || enc_batch_check(nullptr, 1, &tot, 0, 0) != -1) return 1;
  printf("%zu %ld %ld\n", lays.size(), accepted, refused);
  return lays.empty() ? 1 : 0;
}
