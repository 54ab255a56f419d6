// Host-only sanitizer check of the JPEG format arithmetic (csrc/vlfb_jpeg_core.h) through vlfb_jpeg_decode_host
// (include/vlfb.h): every file named on the command line is decoded whole, and the first two also at EVERY prefix length --
// each prefix copied into a heap block of exactly its size, the destination a heap block of exactly height * width * 3, so
// that AddressSanitizer sees any read or write outside them and UBSan any overflow or bad shift on the way.  Needs no GPU.
// Built with the host side of csrc/vlfb_jpeg.hip, from the repository root (tools/make_jpeg_golden.py --dump writes the files):
//
//   mkdir -p build && python tools/make_jpeg_golden.py --dump build/jpeg_cases && \
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude -Ivideo-long-term-feature-banks_amd/csrc \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       video-long-term-feature-banks_amd/csrc/vlfb_jpeg.hip tools/jpeg_host_check.cpp -o build/jpeg_host_check && \
//   build/jpeg_host_check build/jpeg_cases/420_40x56.jpg build/jpeg_cases/420_24x40_rst1.jpg build/jpeg_cases/*.jpg
//
// The error sink of the library (csrc/vlfb_ops.hip) is replaced by the one of tools/jpeg_check_common.h, so that only the file
// under test is linked.  The marker walk there is the tools' own (the product's is lib/datasets/jpeg.py); a prefix it cannot
// walk is skipped.
#include "jpeg_check_common.h"

// decodes the first `n` bytes from a heap block of exactly n bytes; -1: not walked, -2: refused, else the status word
static int run(const uint8_t* data, size_t n, uint32_t* sum) {
  uint8_t* copy = (uint8_t*)malloc(n ? n : 1);
  memcpy(copy, data, n);
  vlfb_jpeg_item it;
  std::vector<uint32_t> seg;
  int result = -1;
  if (walk(copy, n, &it, &seg)) {
    const size_t bytes = (size_t)it.width * it.height * 3;
    uint8_t* dst = (uint8_t*)malloc(bytes ? bytes : 1);
    int32_t status = -1;
    const int rc = vlfb_jpeg_decode_host(&it, dst, &status);
    result = rc == VLFB_OK ? status : -2;
    if (rc == VLFB_OK && sum) {
      uint32_t s = 0;
      for (size_t k = 0; k < bytes; ++k) s = s * 31u + dst[k];
      *sum = s;
    }
    free(dst);
  }
  free(copy);
  return result;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s FILE.jpg ...   (the first two also at every prefix length)\n", argv[0]);
    return 2;
  }
  int failures = 0;
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
    std::vector<uint8_t> data;
    uint8_t buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof(buf), f)) > 0;) data.insert(data.end(), buf, buf + got);
    fclose(f);
    uint32_t sum = 0;
    const int st = run(data.data(), data.size(), &sum);
    printf("%-44s %6zu bytes  %s", argv[a], data.size(), st == -1 ? "not walked" : st == -2 ? "refused" : st ? "status" : "decoded");
    if (st > 0) printf(" %d", st);
    if (st == 0) printf("  checksum %08x", sum);
    if (a <= 2) {
      long walked = 0, clean = 0, flagged = 0;
      for (size_t n = 0; n < data.size(); ++n) {
        const int p = run(data.data(), n, nullptr);
        walked += p >= 0;
        clean += p == 0;
        flagged += p > 0;
      }
      printf("  | prefixes: %ld decoded, %ld with a non-zero status, %ld complete", walked, flagged, clean);
      // a prefix may only decode clean when nothing but the EOI marker (or its second byte) is missing
      if (clean > 2 || (st == 0 && walked == 0)) ++failures;
    }
    printf("\n");
  }
  printf("%s\n", failures ? "FAILED" : "no sanitizer report: every read and write stayed inside its block");
  return failures ? 1 : 0;
}
