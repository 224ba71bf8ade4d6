// AddressSanitizer + UBSan harness for the host half of the batched GPU entropy decode
// (spotter_amd/csrc/jpeg_entropy_host.h batch_plan, batch_check, batch_emulate: the bodies of
// sp_jpeg_entropy_batch_plan / _check / _emulate). Same pattern as jpeg_entropy_fuzz.cpp; built and run on the CPU by
// tests/test_jpeg_entropy_batch_host.py over the corrupt-input corpus:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
//       tools/sanitize/jpeg_entropy_batch.cpp -o <out>
//   <out> corpus.bin        (corpus.bin: a sequence of [uint32 little-endian length][bytes] records)
//
// 1. The files of the corpus the packer accepts, in one batch of every size from 1 to SP_JPEG_BATCH_MAX = 64, each
//    starting where the one before ended and wrapping around the list: planned, checked, emulated with packages,
//    workspace and coefficients in exact-size heap blocks, and compared per image with the single-image emulation
//    (coefficients and status word). Exit status 1 on a difference.
// 2. Single table rows with one 32-bit field overwritten by each of a few extreme values, against the buffer sizes of
//    the undamaged row: the check refuses the row, or the emulation runs over it inside those buffers.
// Prints "<eligible files> <batches> <largest batch> <images with a non-zero status> <damaged rows> <refused rows>".
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../spotter_amd/csrc/jpeg_entropy_host.h"
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

using namespace sp::jpeg_entropy;

struct File {
  sp_jpeg_layout lay;
  sp_jpeg_scan scan;
  std::vector<uint8_t> pkg;
  std::vector<int16_t> coefs;  // the single-image emulation's
  int32_t status;
};

static int pack(const uint8_t* data, int64_t len, sp_jpeg_layout* lay, sp_jpeg_scan* scan, uint8_t* pkg, int64_t cap) {
  sp::jpeg_host::Decoder d{data, len, lay, nullptr};
  d.pk = scan;
  d.pkg = pkg;
  d.pkg_cap = cap;
  return d.run(true);
}

// 16-byte aligned exact-size blocks (the kernels' buffers are): ASan sees any access past nbytes
struct Block {
  uint8_t* p;
  explicit Block(size_t nbytes) : p(static_cast<uint8_t*>(aligned_alloc(16, (nbytes + 15) / 16 * 16))) {}
  ~Block() { free(p); }
  Block(const Block&) = delete;
};

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s corpus.bin\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> all;
  uint8_t tmp[65536];
  size_t nr;
  while ((nr = fread(tmp, 1, sizeof(tmp), f)) > 0) all.insert(all.end(), tmp, tmp + nr);
  fclose(f);
  constexpr int64_t kMaxBlocks = 20000;  // larger frames are left out: the run stays short
  std::vector<File> files;
  size_t pos = 0;
  while (pos + 4 <= all.size()) {
    const uint32_t len = all[pos] | (all[pos + 1] << 8) | (all[pos + 2] << 16) | ((uint32_t)all[pos + 3] << 24);
    pos += 4;
    if (pos + len > all.size()) return 3;
    std::vector<uint8_t> rec(all.begin() + pos, all.begin() + pos + len);
    pos += len;
    if (rec.empty()) continue;
    File fl;
    memset(&fl.lay, 0, sizeof(fl.lay));
    memset(&fl.scan, 0, sizeof(fl.scan));
    int rc = pack(rec.data(), (int64_t)rec.size(), &fl.lay, &fl.scan, nullptr, 0);
    if (rc != SP_JPEG_PKG_SMALL || fl.lay.total_blocks > kMaxBlocks) continue;
    fl.pkg.resize((size_t)fl.scan.pkg_bytes);
    if (pack(rec.data(), (int64_t)rec.size(), &fl.lay, &fl.scan, fl.pkg.data(), (int64_t)fl.pkg.size()) != 0) continue;
    if (check_scan(fl.scan, fl.lay)) return 4;  // the packer's own output must pass the checks
    sp_jpeg_batch_item one;
    sp_jpeg_batch_totals one_t;
    if (sp::jpeg_host::batch_plan(&fl.lay, 1, &one, &one_t)) continue;  // a layout the RGB pass refuses: no batch has it
    fl.pkg.resize((size_t)fl.scan.pkg_bytes);   // exact size: a read past the package is a report
    fl.coefs.resize((size_t)fl.lay.total_blocks * 64);
    fl.status = 0;
    emulate(fl.pkg.data(), fl.scan, fl.lay, fl.coefs.data(), &fl.status, nullptr);
    files.push_back(std::move(fl));
  }
  if (files.empty()) return 1;
  long batches = 0, largest = 0, flagged = 0, rows = 0, refused = 0;
  size_t next = 0;  // the first file of the next batch; indices wrap around the list
  for (int n = 1; n <= SP_JPEG_BATCH_MAX; ++n) {
    std::vector<const File*> in;
    for (int k = 0; k < n; ++k) in.push_back(&files[(next + k) % files.size()]);
    next = (next + n) % files.size();
    std::vector<sp_jpeg_layout> lays;
    std::vector<sp_jpeg_scan> scans;
    for (const File* fl : in) lays.push_back(fl->lay), scans.push_back(fl->scan);
    std::vector<sp_jpeg_batch_item> bitems(n);
    std::vector<sp_jpeg_entropy_item> items(n);  // exact size: ASan sees a write past the n-th row
    sp_jpeg_batch_totals bt;
    sp_jpeg_entropy_totals et;
    if (sp::jpeg_host::batch_plan(lays.data(), n, bitems.data(), &bt)) return 5;
    if (batch_plan(scans.data(), lays.data(), bitems.data(), n, items.data(), &et)) return 5;
    if (batch_check(items.data(), n, &et, et.pkg_bytes, et.work_bytes, bt.coef_elems)) return 6;
    Block pkgs((size_t)et.pkg_bytes), work((size_t)et.work_bytes);
    std::vector<int16_t> coefs((size_t)bt.coef_elems, 0x5A5A);
    std::vector<int32_t> status(n, 0);
    for (int k = 0; k < n; ++k) memcpy(pkgs.p + items[k].pkg_off, in[k]->pkg.data(), in[k]->pkg.size());
    memset(work.p, 0xA5, (size_t)et.work_bytes);
    batch_emulate(pkgs.p, items.data(), n, et, work.p, coefs.data(), status.data());
    for (int k = 0; k < n; ++k) {
      const File& fl = *in[k];
      if (status[k] != fl.status) return 1;
      if (memcmp(coefs.data() + items[k].coef_off, fl.coefs.data(), fl.coefs.size() * sizeof(int16_t)) != 0) return 1;
      flagged += status[k] != 0;
    }
    ++batches;
    if (n > largest) largest = n;
  }
  // damaged rows
  const int32_t bad[] = {0, -1, 1, 3, 5, INT32_MAX, INT32_MIN};
  for (size_t i = 0; i < files.size(); i += 9) {
    const File& fl = files[i];
    if (fl.lay.total_blocks > 600) continue;
    sp_jpeg_batch_item bitem;
    sp_jpeg_batch_totals bt;
    sp_jpeg_entropy_item good;
    sp_jpeg_entropy_totals et;
    if (sp::jpeg_host::batch_plan(&fl.lay, 1, &bitem, &bt)) continue;
    if (batch_plan(&fl.scan, &fl.lay, &bitem, 1, &good, &et)) return 5;
    for (size_t field = 0; field < sizeof(good) / 4; ++field)
      for (int32_t v : bad) {
        std::vector<sp_jpeg_entropy_item> row(1, good);
        reinterpret_cast<int32_t*>(row.data())[field] = v;
        ++rows;
        if (batch_check(row.data(), 1, &et, et.pkg_bytes, et.work_bytes, bt.coef_elems)) {
          ++refused;
          continue;
        }
        Block pkgs((size_t)et.pkg_bytes), work((size_t)et.work_bytes);
        std::vector<int16_t> coefs((size_t)bt.coef_elems);
        int32_t status = 0;
        memset(pkgs.p, 0, (size_t)et.pkg_bytes);
        memcpy(pkgs.p + row[0].pkg_off, fl.pkg.data(), fl.pkg.size());
        batch_emulate(pkgs.p, row.data(), 1, et, work.p, coefs.data(), &status);
      }
  }
  sp_jpeg_entropy_totals et0 = {0, 0, 0, 0};
  if (batch_check(nullptr, 1, &et0, 0, 0, 0) != -1) return 1;
  printf("%zu %ld %ld %ld %ld %ld\n", files.size(), batches, largest, flagged, rows, refused);
  return 0;
}
