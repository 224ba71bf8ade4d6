// AddressSanitizer + UBSan harness for the GPU entropy decode's host-compilable half: the scan packer
// (spotter_amd/csrc/jpeg_host.h pack_scan) and the emulation that runs the kernels' passes in their order over
// the shared per-subsequence core (csrc/jpeg_entropy_host.h, csrc/jpeg_entropy_core.h). Same pattern as
// jpeg_fuzz.cpp; built and run on the CPU by tests/test_jpeg_entropy_host.py over the corrupt-input corpus:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
//       tools/sanitize/jpeg_entropy_fuzz.cpp -o <out>
//   <out> corpus.bin        (corpus.bin: a sequence of [uint32 little-endian length][bytes] records)
//
// Prints one line per record: "<index> <pack rc> <status> <host rc> <equal>": the packer's return (0 packed,
// 1 not eligible, -10 refused), the emulation's status word, the host decoder's return, and whether the two
// coefficient arrays are equal ("-" where one of them was not produced; "big": the layout asks for more than
// kMaxCoefs coefficients and nothing is decoded, as in jpeg_fuzz.cpp).
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

static int pack(const uint8_t* data, int64_t len, sp_jpeg_layout* lay, sp_jpeg_scan* scan, uint8_t* pkg, int64_t cap) {
  sp::jpeg_host::Decoder d{data, len, lay, nullptr};
  d.pk = scan;
  d.pkg = pkg;
  d.pkg_cap = cap;
  return d.run(true);
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
  constexpr int64_t kMaxCoefs = int64_t(1) << 26;
  size_t pos = 0;
  int idx = 0;
  while (pos + 4 <= all.size()) {
    const uint32_t len = all[pos] | (all[pos + 1] << 8) | (all[pos + 2] << 16) | ((uint32_t)all[pos + 3] << 24);
    pos += 4;
    if (pos + len > all.size()) return 3;
    // each record, package and coefficient array in its own exact-size heap block, so ASan sees any access past it
    std::vector<uint8_t> rec(all.begin() + pos, all.begin() + pos + len);
    pos += len;
    sp_jpeg_layout lay, hlay;
    sp_jpeg_scan scan;
    memset(&lay, 0, sizeof(lay));
    memset(&hlay, 0, sizeof(hlay));
    memset(&scan, 0, sizeof(scan));
    int rc = rec.empty() ? -1 : pack(rec.data(), (int64_t)rec.size(), &lay, &scan, nullptr, 0);
    if (rc == SP_JPEG_PKG_SMALL && lay.total_blocks * 64 > kMaxCoefs) {
      printf("%d big 0 0 -\n", idx++);
      continue;
    }
    std::vector<uint8_t> pkg;
    if (rc == SP_JPEG_PKG_SMALL) {
      pkg.resize((size_t)scan.pkg_bytes);
      rc = pack(rec.data(), (int64_t)rec.size(), &lay, &scan, pkg.data(), (int64_t)pkg.size());
    }
    int32_t status = 0;
    std::vector<int16_t> coefs;
    bool ran = false;
    if (rc == 0) {
      if (sp::jpeg_entropy::check_scan(scan, lay)) return 4;  // the packer's own output must pass the checks
      pkg.resize((size_t)scan.pkg_bytes);  // exact size: a read past the package is a report
      coefs.resize((size_t)lay.total_blocks * 64);
      sp::jpeg_entropy::emulate(pkg.data(), scan, lay, coefs.data(), &status, nullptr);
      ran = true;
    }
    int hrc = -1;
    std::vector<int16_t> href;
    if (!rec.empty()) {
      sp::jpeg_host::Decoder h0{rec.data(), (int64_t)rec.size(), &hlay, nullptr};
      hrc = h0.run(false);
      if (hrc == 0 && hlay.total_blocks * 64 <= kMaxCoefs) {
        href.resize((size_t)hlay.total_blocks * 64);
        sp::jpeg_host::Decoder h1{rec.data(), (int64_t)rec.size(), &hlay, href.data()};
        hrc = h1.run(true);
      }
    }
    const char* eq = "-";
    if (ran && hrc == 0) eq = coefs == href ? "1" : "0";
    printf("%d %d %d %d %s\n", idx, rc, (int)status, hrc, eq);
    ++idx;
  }
  return 0;
}
