// What the two host-only sanitizer checks of the JPEG code (tools/jpeg_host_check.cpp, tools/jpeg_par_host_check.cpp) share:
// the error sink that stands in for the library's (csrc/vlfb_ops.hip), so that only csrc/vlfb_jpeg.hip is linked, and the
// tools' own marker walk (the product's is lib/datasets/jpeg.py).
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vlfb.h"

namespace vlfb {
static char g_err[512];
int set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
}  // namespace vlfb

// fills everything of `it` but dst; false when the header cannot be walked or names something unsupported
static bool walk(const uint8_t* d, size_t n, vlfb_jpeg_item* it, std::vector<uint32_t>* seg) {
  memset(it, 0, sizeof(*it));
  if (n < 4 || d[0] != 0xff || d[1] != 0xd8) return false;
  size_t i = 2;
  bool sof = false;
  for (;;) {
    if (i + 4 > n || d[i] != 0xff) return false;
    const int m = d[i + 1];
    const size_t len = ((size_t)d[i + 2] << 8) | d[i + 3], s = i + 4, e = i + 2 + len;
    if (len < 2 || e > n) return false;
    if (m == 0xdb) {
      for (size_t p = s; p < e; p += 65) {
        if (p + 65 > e || d[p] > 3) return false;
        memcpy(it->quant[d[p]], d + p + 1, 64);
      }
    } else if (m == 0xc4) {
      for (size_t p = s; p < e;) {
        if (p + 17 > e) return false;
        size_t cnt = 0;
        for (int k = 1; k <= 16; ++k) cnt += d[p + k];
        const int cls = d[p] >> 4, id = d[p] & 15;
        if (cls > 1 || id > 1 || cnt > 256 || p + 17 + cnt > e) return false;
        memcpy(it->huff[2 * cls + id], d + p + 1, 16 + cnt);
        p += 17 + cnt;
      }
    } else if (m == 0xc0) {
      if (len < 8 || d[s] != 8) return false;
      it->height = (d[s + 1] << 8) | d[s + 2];
      it->width = (d[s + 3] << 8) | d[s + 4];
      it->n_comp = d[s + 5];
      if ((it->n_comp != 1 && it->n_comp != 3) || len != 8 + 3 * (size_t)it->n_comp) return false;
      for (int c = 0; c < it->n_comp; ++c) {
        it->h[c] = it->n_comp == 1 ? 1 : d[s + 7 + 3 * c] >> 4;
        it->v[c] = it->n_comp == 1 ? 1 : d[s + 7 + 3 * c] & 15;
        it->tq[c] = d[s + 8 + 3 * c];
      }
      sof = true;
    } else if (m == 0xdd) {
      if (len != 4) return false;
      it->restart_interval = (d[s] << 8) | d[s + 1];
    } else if (m == 0xda) {
      if (!sof || d[s] != it->n_comp || len != 6 + 2 * (size_t)it->n_comp) return false;
      for (int c = 0; c < it->n_comp; ++c) {
        it->td[c] = d[s + 2 + 2 * c] >> 4;
        it->ta[c] = d[s + 2 + 2 * c] & 15;
      }
      size_t end = n;
      seg->assign(1, 0u);
      for (size_t j = e; j + 1 < n; ++j) {
        if (d[j] != 0xff || d[j + 1] == 0 || d[j + 1] == 0xff) continue;
        if (d[j + 1] >= 0xd0 && d[j + 1] <= 0xd7) { seg->push_back((uint32_t)(j + 2 - e)); continue; }
        end = j;
        break;
      }
      it->scan = (uint64_t)(uintptr_t)(d + e);
      it->scan_bytes = (uint32_t)(end - e);
      it->n_segments = (uint32_t)seg->size();
      it->seg_offsets = (uint64_t)(uintptr_t)seg->data();
      return true;
    } else if (m >= 0xc1 && m <= 0xcf) {
      return false;
    }
    i = e;
  }
}
