// Host-only sanitizer check of the lane-parallel JPEG entropy decode (csrc/vlfb_jpeg_core.h, "lane-parallel entropy decode")
// through vlfb_jpeg_decode_host_par (include/vlfb.h): every file named on the command line is decoded whole, and the first
// two also at EVERY prefix length, each with (lanes, subseq_bytes) = (1, 8), (5, 12) and (256, 64) -- the prefix copied into
// a heap block of exactly its size, the destination a heap block of exactly height * width * 3, so that AddressSanitizer
// sees any read or write outside them and UBSan any overflow or bad shift on the way.  Every result is compared byte for byte
// and status for status with the serial checker vlfb_jpeg_decode_host; any difference ends the run with a non-zero exit
// code.  Needs no GPU and is never run on one.  Built with the host side of csrc/vlfb_jpeg.hip, from the repository root:
//
//   mkdir -p build && python tools/make_jpeg_golden.py --dump build/jpeg_cases && \
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude -Ivideo-long-term-feature-banks_amd/csrc \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       video-long-term-feature-banks_amd/csrc/vlfb_jpeg.hip tools/jpeg_par_host_check.cpp -o build/jpeg_par_host_check && \
//   build/jpeg_par_host_check build/jpeg_cases/420_40x56.jpg build/jpeg_cases/420_32x340.jpg build/jpeg_cases/*.jpg
#include "jpeg_check_common.h"

static const int CONFIGS[3][2] = {{1, 8}, {5, 12}, {256, 64}};

struct Tally { long walked, equal, parallel, redone, serial; };

// the first `n` bytes from a heap block of exactly n bytes through both checkers; false on any difference
static bool run(const uint8_t* data, size_t n, Tally* t) {
  uint8_t* copy = (uint8_t*)malloc(n ? n : 1);
  memcpy(copy, data, n);
  vlfb_jpeg_item it;
  std::vector<uint32_t> seg;
  bool same = true;
  if (walk(copy, n, &it, &seg)) {
    const size_t bytes = (size_t)it.width * it.height * 3;
    uint8_t* ref = (uint8_t*)malloc(bytes ? bytes : 1);
    int32_t ref_status = -1;
    const int ref_rc = vlfb_jpeg_decode_host(&it, ref, &ref_status);
    for (int c = 0; c < 3; ++c) {
      uint8_t* dst = (uint8_t*)malloc(bytes ? bytes : 1);
      int32_t status = -1, stats[4] = {-1, -1, -1, -1};
      const int rc = vlfb_jpeg_decode_host_par(&it, dst, &status, CONFIGS[c][0], CONFIGS[c][1], stats);
      bool ok = rc == ref_rc;
      if (ok && rc == VLFB_OK) {
        ok = status == ref_status && memcmp(dst, ref, bytes) == 0;
        ok = ok && stats[0] >= 0 && stats[0] <= 2 && (stats[0] == 0 || stats[3] <= CONFIGS[c][0]);
        t->parallel += stats[0] == 1;
        t->redone += stats[0] == 2;
        t->serial += stats[0] == 0;
      }
      if (!ok) {
        fprintf(stderr, "DIFFERENT at %zu bytes, lanes %d subseq %d: rc %d / %d, status %d / %d, routed %d\n", n, CONFIGS[c][0],
                CONFIGS[c][1], rc, ref_rc, status, ref_status, stats[0]);
        same = false;
      }
      t->walked += 1;
      t->equal += ok;
      free(dst);
    }
    free(ref);
  }
  free(copy);
  return same;
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
    Tally whole = {0, 0, 0, 0, 0}, pre = {0, 0, 0, 0, 0};
    if (!run(data.data(), data.size(), &whole)) ++failures;
    printf("%-44s %6zu bytes  %ld of %ld runs equal the serial checker (%ld parallel, %ld redone, %ld serial by rule)", argv[a], data.size(),
           whole.equal, whole.walked, whole.parallel, whole.redone, whole.serial);
    if (a <= 2) {
      for (size_t n = 0; n < data.size(); ++n)
        if (!run(data.data(), n, &pre)) ++failures;
      printf("  | prefixes: %ld of %ld runs equal (%ld parallel, %ld redone, %ld serial by rule)", pre.equal, pre.walked, pre.parallel,
             pre.redone, pre.serial);
    }
    printf("\n");
  }
  printf("%s\n", failures ? "FAILED" : "no sanitizer report and no difference: the parallel checker is the serial one on every file and prefix");
  return failures ? 1 : 0;
}
