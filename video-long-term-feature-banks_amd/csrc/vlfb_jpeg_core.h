// Baseline JPEG format arithmetic (include/vlfb.h, vlfb_jpeg_*): the bit reader, Huffman symbol decode, one block's
// coefficient decode, the 8x8 inverse DCT, the upsampling taps and the colour conversion, as __host__ __device__ functions.
// csrc/vlfb_jpeg.hip compiles this text twice: for the kernels, and for vlfb_jpeg_decode_host (the single-threaded checker).
// Everything is integer; every index is bounded by the function that forms it, whatever the stream holds.
#pragma once
#include <stdint.h>
#include "vlfb.h"

#if defined(__HIPCC__)
#define VLFB_HD __host__ __device__ inline
#else
#define VLFB_HD inline
#endif

namespace vlfb {
namespace jpeg {

constexpr int LOOK_BITS = 9;                 // codes of up to 9 bits are decoded by one table read
constexpr int MAX_MCU_BLOCKS = 6;            // 4:2:0: four luma blocks and two chroma blocks
// the most stream bytes one MCU can take: per coefficient a code of <= 16 bits and <= 15 value bits, every byte stuffed
constexpr int MAX_MCU_BYTES = MAX_MCU_BLOCKS * 64 * 8;

// ---- geometry of one item -----------------------------------------------------------------------------------------------
struct Geo {
  int32_t n_comp, hmax, vmax;
  int32_t mcu_cols, mcu_rows, mcu_blocks;
  int32_t h[3], v[3];
  int32_t bw[3], bh[3];                      // the component's block grid, in whole MCUs
  int32_t cw[3], ch[3];                      // its real size in samples: ceil(W * h / hmax), ceil(H * v / vmax)
  int64_t first_block[4];                    // blocks before component c; [n_comp] = all blocks
};

// the supported sampling: one component 1x1, or luma 1x1 / 2x1 / 2x2 with both chroma 1x1
VLFB_HD bool sampling_ok(const vlfb_jpeg_item& it) {
  if (it.n_comp == 1) return it.h[0] == 1 && it.v[0] == 1;
  if (it.n_comp != 3) return false;
  if (it.h[1] != 1 || it.v[1] != 1 || it.h[2] != 1 || it.v[2] != 1) return false;
  return (it.h[0] == 1 && it.v[0] == 1) || (it.h[0] == 2 && it.v[0] == 1) || (it.h[0] == 2 && it.v[0] == 2);
}

// false, and a grey 1x1 geometry of one block, for a record outside the supported set (the host refuses such a record before
// any launch; the device copy is re-checked so that a kernel never forms an index from an unchecked field)
VLFB_HD bool geometry(const vlfb_jpeg_item& it, Geo* g) {
  const bool ok = sampling_ok(it) && it.width >= 1 && it.width <= 65535 && it.height >= 1 && it.height <= 65535;
  g->n_comp = ok ? it.n_comp : 1;
  g->hmax = ok ? it.h[0] : 1;
  g->vmax = ok ? it.v[0] : 1;
  const int W = ok ? it.width : 1, H = ok ? it.height : 1;
  g->mcu_cols = (W + 8 * g->hmax - 1) / (8 * g->hmax);
  g->mcu_rows = (H + 8 * g->vmax - 1) / (8 * g->vmax);
  g->mcu_blocks = 0;
  int64_t blocks = 0;
  for (int c = 0; c < 3; ++c) {
    const bool on = c < g->n_comp;
    g->h[c] = on && ok ? it.h[c] : (on ? 1 : 0);
    g->v[c] = on && ok ? it.v[c] : (on ? 1 : 0);
    g->bw[c] = g->mcu_cols * g->h[c];
    g->bh[c] = g->mcu_rows * g->v[c];
    g->cw[c] = on ? (W * g->h[c] + g->hmax - 1) / g->hmax : 0;
    g->ch[c] = on ? (H * g->v[c] + g->vmax - 1) / g->vmax : 0;
    g->first_block[c] = blocks;
    blocks += (int64_t)g->bw[c] * g->bh[c];
    g->mcu_blocks += g->h[c] * g->v[c];
  }
  g->first_block[3] = blocks;
  for (int c = g->n_comp; c < 3; ++c) g->first_block[c] = blocks;
  return ok;
}
// An item's part of the workspace: int16 coefficients [block][64] of all components, then uint8 sample planes
// [bh * 8][bw * 8] per component: 192 bytes per block.
VLFB_HD int64_t item_workspace_bytes(const Geo& g) { return g.first_block[3] * 192; }
VLFB_HD int64_t coef_offset(const Geo& g, int c) { return g.first_block[c] * 128; }
VLFB_HD int64_t plane_offset(const Geo& g, int c) { return g.first_block[3] * 128 + g.first_block[c] * 64; }

VLFB_HD int64_t total_mcus(const Geo& g) { return (int64_t)g.mcu_cols * g.mcu_rows; }
VLFB_HD int64_t expected_segments(const Geo& g, int32_t restart_interval) {
  const int64_t n = total_mcus(g);
  return restart_interval > 0 ? (n + restart_interval - 1) / restart_interval : 1;
}

// ---- Huffman tables -------------------------------------------------------------------------------------------------------
// built from the raw DHT content: 16 counts (codes of length 1..16), then the symbols in code order
struct Huff {
  uint16_t look[1 << LOOK_BITS];             // (length << 8) | symbol of the code the next 9 bits begin with; 0: longer
  int32_t maxcode[17];                       // largest code of length l, -1 when there is none
  int32_t valoff[17];                        // index of the first symbol of length l, minus its code
  uint8_t sym[256];
};

// the counts alone: no more than 256 symbols, and no length with more codes than are left (Kraft)
VLFB_HD bool huff_counts_ok(const uint8_t* raw) {
  int code = 0, total = 0;
  for (int l = 1; l <= 16; ++l) {
    code += raw[l - 1];
    total += raw[l - 1];
    if (code > (1 << l)) return false;
    code <<= 1;
  }
  return total <= 256;
}

VLFB_HD bool huff_build(const uint8_t* raw, Huff* t) {
  for (int i = 0; i < (1 << LOOK_BITS); ++i) t->look[i] = 0;
  for (int i = 0; i < 256; ++i) t->sym[i] = raw[16 + i];
  const bool ok = huff_counts_ok(raw);
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int n = ok ? raw[l - 1] : 0;
    t->valoff[l] = k - code;
    for (int i = 0; i < n; ++i, ++k, ++code) {
      if (l <= LOOK_BITS) {
        const int first = code << (LOOK_BITS - l), span = 1 << (LOOK_BITS - l);
        for (int j = 0; j < span; ++j) t->look[(first + j) & ((1 << LOOK_BITS) - 1)] = (uint16_t)((l << 8) | raw[16 + (k & 255)]);
      }
    }
    t->maxcode[l] = n ? code - 1 : -1;
    code <<= 1;
  }
  t->maxcode[0] = -1;
  t->valoff[0] = 0;
  return ok;
}

// ---- bit reader -----------------------------------------------------------------------------------------------------------
// Bytes pos..hi-1 of the stream are at p[pos - base]; `hi` is the end of the segment, or of the window of it that p holds
// (`windowed`).  Past the end, or at a marker, the reader feeds zero bytes and counts them in `pad`: a decode that has used
// any of them (nbits < pad) ran past its data.
struct Bits {
  const uint8_t* p;
  int32_t base, pos, hi;
  int32_t windowed;                          // hi is a window's end, not the segment's: reaching it is a starved reader
  uint64_t acc;
  int32_t nbits, pad, starved;
  int32_t ended;                             // a marker was met: hi is where the data ends, whatever window comes next
};

VLFB_HD void bits_init(Bits* b, const uint8_t* p, int32_t base, int32_t pos, int32_t hi, int32_t windowed) {
  b->p = p; b->base = base; b->pos = pos; b->hi = hi; b->windowed = windowed;
  b->acc = 0; b->nbits = 0; b->pad = 0; b->starved = 0; b->ended = 0;
}

VLFB_HD void bits_refill(Bits* b) {
  while (b->nbits <= 56) {
    uint32_t byte = 0;
    if (b->pos < b->hi) {
      byte = b->p[b->pos - b->base];
      if (byte == 0xff) {
        if (b->pos + 1 < b->hi && b->p[b->pos + 1 - b->base] == 0) {
          b->pos += 2;                       // a stuffed zero
        } else {                             // a marker, or 0xff as the last byte: the data ends here
          if (b->pos + 1 >= b->hi && b->windowed) b->starved = 1;
          b->windowed = 0;
          b->ended = 1;
          b->hi = b->pos;
          byte = 0;
          b->pad += 8;
        }
      } else {
        b->pos += 1;
      }
    } else {
      if (b->windowed) b->starved = 1;
      b->pad += 8;
    }
    b->acc = (b->acc << 8) | byte;
    b->nbits += 8;
  }
}
// n <= 16 bits; the caller has refilled
VLFB_HD uint32_t bits_peek(const Bits* b, int n) { return (uint32_t)(b->acc >> (b->nbits - n)) & ((1u << n) - 1u); }
VLFB_HD void bits_skip(Bits* b, int n) { b->nbits -= n; }
VLFB_HD bool bits_overrun(const Bits* b) { return b->nbits < b->pad || b->starved; }

// the next symbol, or -1 when no code of up to 16 bits matches
VLFB_HD int huff_decode(Bits* b, const Huff* t) {
  const uint32_t v = bits_peek(b, 16);
  const uint32_t e = t->look[v >> (16 - LOOK_BITS)];
  if (e) {
    bits_skip(b, (int)(e >> 8));
    return (int)(e & 255u);
  }
  for (int l = LOOK_BITS + 1; l <= 16; ++l) {
    const int32_t code = (int32_t)(v >> (16 - l));
    if (code <= t->maxcode[l]) {
      bits_skip(b, l);
      return t->sym[(t->valoff[l] + code) & 255];
    }
  }
  return -1;
}

VLFB_HD int extend(uint32_t v, int s) { return v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

// zigzag position -> natural (row-major) position
VLFB_HD int natural_order(int k) {
  const uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                          41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                          30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return zz[k & 63];
}

// One block: the DC difference and the AC run/size pairs into out[64] (natural order, zeroed by the caller).  Returns 0, or
// VLFB_JPEG_BAD_CODE for a missing code, a DC size above 15 or a run that leaves the block.
VLFB_HD int decode_block(Bits* b, const Huff* dc, const Huff* ac, int* pred, int16_t* out) {
  bits_refill(b);
  int s = huff_decode(b, dc);
  if (s < 0 || s > 15) return VLFB_JPEG_BAD_CODE;
  if (s) {
    bits_refill(b);
    const int diff = extend(bits_peek(b, s), s);
    bits_skip(b, s);
    *pred = (int16_t)(*pred + diff);
  }
  out[0] = (int16_t)*pred;
  for (int k = 1; k < 64;) {
    bits_refill(b);
    const int rs = huff_decode(b, ac);
    if (rs < 0) return VLFB_JPEG_BAD_CODE;
    const int r = rs >> 4;
    s = rs & 15;
    if (s) {
      k += r;
      if (k > 63) return VLFB_JPEG_BAD_CODE;
      out[natural_order(k)] = (int16_t)extend(bits_peek(b, s), s);
      bits_skip(b, s);
      ++k;
    } else {
      if (r != 15) break;                    // end of block
      k += 16;
    }
  }
  return 0;
}

// One MCU: out[mcu_blocks][64], component after component, a component's blocks row by row.  tabs: DC tables 0, 1, then AC
// tables 0, 1.  Returns 0 or a status bit; a decode that used bits past its data is VLFB_JPEG_TRUNCATED.
VLFB_HD int decode_mcu(Bits* b, const Geo& g, const Huff* tabs, const uint8_t* td, const uint8_t* ta, int* pred, int16_t* out) {
  int blk = 0;
  for (int c = 0; c < g.n_comp; ++c) {
    const Huff* dc = tabs + (td[c] & 1);
    const Huff* ac = tabs + 2 + (ta[c] & 1);
    for (int i = 0; i < g.h[c] * g.v[c] && blk < MAX_MCU_BLOCKS; ++i, ++blk) {
      const int rc = decode_block(b, dc, ac, pred + c, out + blk * 64);
      if (rc) return rc;
    }
  }
  return bits_overrun(b) ? VLFB_JPEG_TRUNCATED : 0;
}

// block i of an MCU -> component and the block's index in the component's grid
VLFB_HD void mcu_block_place(const Geo& g, int64_t mcu, int i, int* comp, int64_t* block) {
  const int my = (int)(mcu / g.mcu_cols), mx = (int)(mcu % g.mcu_cols);
  int c = 0;
  while (c < g.n_comp - 1 && i >= g.h[c] * g.v[c]) { i -= g.h[c] * g.v[c]; ++c; }
  const int by = my * g.v[c] + i / g.h[c], bx = mx * g.h[c] + i % g.h[c];
  *comp = c;
  *block = (int64_t)by * g.bw[c] + bx;
}

// Segment s of the scan: bytes [*lo, *hi) and 0, or a status bit and an empty range.  seg: the n_seg segment starts the host
// found (offsets into the scan; seg[0] = 0), want: the segments the frame's MCU count and restart interval call for.
VLFB_HD int segment_range(const uint8_t* scan, uint32_t scan_bytes, const uint32_t* seg, uint32_t n_seg, int64_t want, int64_t s,
                          int32_t* lo, int32_t* hi) {
  *lo = *hi = 0;
  if (s >= (int64_t)n_seg) return (int64_t)n_seg < want ? VLFB_JPEG_TRUNCATED : VLFB_JPEG_BAD_RESTART;
  const uint32_t a = seg[s];
  if (a > scan_bytes) return VLFB_JPEG_TRUNCATED;
  uint32_t e = scan_bytes;
  if (s + 1 < (int64_t)n_seg) {
    e = seg[s + 1];
    if (e < a + 2 || e > scan_bytes) return VLFB_JPEG_BAD_RESTART;
    e -= 2;                                  // the restart marker that ends this segment
  }
  if (s > 0 && (a < 2 || scan[a - 2] != 0xff || scan[a - 1] != (0xd0 | ((s - 1) & 7)))) return VLFB_JPEG_BAD_RESTART;
  *lo = (int32_t)a;
  *hi = (int32_t)e;
  return (int64_t)n_seg != want ? VLFB_JPEG_BAD_RESTART : 0;   // the range is given all the same: the caller may decode it
}

// ---- lane-parallel entropy decode (vlfb_jpeg_decode_batch_par, vlfb_jpeg_decode_host_par) ---------------------------------
// The self-synchronising decode of Weissenberger and Schmidt on the DESTUFFED scan: the bytes before the first marker with
// the zero of every FF 00 pair removed, kept as big-endian 32-bit words, so that a bit position is a plain number every lane
// shares and any 32 bits of the stream are two word reads.  The stream is cut into subsequences of `subseq_bytes`; a lane
// walks one subsequence symbol by symbol from a state (bit position, block inside the MCU, zigzag index k; k = 0: a DC
// symbol comes next) to the first symbol boundary at or past the subsequence's end.  The functions below are one lane's
// work; the kernel and the host checker differ only in how they run the lanes (side by side / one after another).
constexpr int PAR_LANES = 256;                       // lanes of the kernel's workgroup = subsequences of one chunk
constexpr int PAR_SUBSEQ_DEFAULT = 256;              // profiles/jpeg_decode.txt: the sweep this default comes from
constexpr uint32_t PAR_MAX_SCAN = 128u * 1024u;      // the destuffed scan lives in LDS beside the tables and lane states
constexpr int32_t PAR_REDO_BIT = 1 << 30;            // private to one call: "decode this item serially"; never left set
constexpr uint32_t PAR_NO_STATE = 0xffffffffu;       // a walk that met a bad code, a bad run or the end of the data

VLFB_HD bool par_subseq_ok(int subseq_bytes) { return subseq_bytes >= 8 && subseq_bytes <= 4096 && (subseq_bytes & 3) == 0; }

// THE routing rule, read by both entropy kernels and the host checker: one segment without restart intervals, at least two
// subsequences long, and a scan that fits the LDS buffer.  Everything else is decoded by the serial kernel.
VLFB_HD bool vlfb_jpeg_item_is_parallel(const vlfb_jpeg_item& it, int subseq_bytes) {
  return it.restart_interval == 0 && it.n_segments == 1 && it.scan_bytes >= 2u * (uint32_t)subseq_bytes && it.scan_bytes <= PAR_MAX_SCAN;
}
// words the destuffed stream of a scan of n bytes takes at most: its bytes, and two words of zeros behind them
VLFB_HD uint32_t par_stream_words(uint32_t scan_bytes) { return (scan_bytes + 3u) / 4u + 2u; }

// byte i of the scan is a marker (FF not followed by 00, or FF as the last byte): the data ends in front of the first one
VLFB_HD bool par_is_marker(const uint8_t* scan, uint32_t n, uint32_t i) { return scan[i] == 0xff && (i + 1 >= n || scan[i + 1] != 0); }
// byte i is the zero of an FF 00 pair.  An FF in front of the first marker is always read as a fresh byte (only zeros are
// ever skipped), so the byte before decides alone.
VLFB_HD bool par_is_stuffing(const uint8_t* scan, uint32_t i) { return scan[i] == 0 && i > 0 && scan[i - 1] == 0xff; }
// byte j of the destuffed stream goes here, so that a native 32-bit read gives the big-endian word
VLFB_HD uint32_t par_byte_slot(uint32_t j) { return j ^ 3u; }

struct ParState { uint32_t pos, bk; };               // bit position; block * 64 + k.  pos = PAR_NO_STATE: no state (bk = 0)
VLFB_HD bool par_same(const ParState& a, const ParState& b) { return a.pos == b.pos && a.bk == b.bk; }

struct ParCtx {
  const uint32_t* words;                             // the destuffed stream, par_stream_words() long
  uint32_t data_bits;
  const Huff* tabs;                                  // DC 0, 1, AC 0, 1
  uint32_t sel;                                      // two bits per block of the MCU: DC table, AC table
  int32_t mcu_blocks;
};
VLFB_HD uint32_t par_table_select(const Geo& g, const uint8_t* td, const uint8_t* ta) {
  uint32_t sel = 0;
  int blk = 0;
  for (int c = 0; c < g.n_comp; ++c)
    for (int i = 0; i < g.h[c] * g.v[c] && blk < MAX_MCU_BLOCKS; ++i, ++blk) sel |= (uint32_t)((td[c] & 1) | ((ta[c] & 1) << 1)) << (2 * blk);
  return sel;
}

// One symbol at bit `pos` of block `blk`, zigzag index k: its code and its value bits are at most 31 bits, one 32-bit look.
// PAR_SYM_BAD: no such code, a DC size above 15 or a run past coefficient 63 -- an error to the write pass; a speculative
// walk goes on as *o says (one bit further, or behind the block the run left), which costs it nothing but its guess.
// PAR_SYM_END: the symbol would use bits past the data.
enum { PAR_SYM_OK = 0, PAR_SYM_BAD = 1, PAR_SYM_END = 2 };
struct ParSym { int32_t bits, k_next, at, value; }; // at: the zigzag index `value` belongs to, -1 for none; k_next >= 64: block done
VLFB_HD int par_symbol(const ParCtx& c, uint32_t pos, int blk, int k, ParSym* o) {
  if (pos >= c.data_bits) return PAR_SYM_END;
  o->bits = 1;
  o->k_next = k;
  o->at = -1;
  o->value = 0;
  const uint32_t w = pos >> 5, sh = pos & 31u;
  const uint32_t v = (uint32_t)(((((uint64_t)c.words[w] << 32) | c.words[w + 1]) << sh) >> 32);
  const uint32_t pick = (c.sel >> (2 * blk)) & 3u;
  const Huff* t = k == 0 ? c.tabs + (pick & 1u) : c.tabs + 2 + (pick >> 1);
  const uint32_t v16 = v >> 16;
  const uint32_t e = t->look[v16 >> (16 - LOOK_BITS)];
  int len = 0, sym = -1;
  if (e) {
    len = (int)(e >> 8);
    sym = (int)(e & 255u);
  } else {
    for (int l = LOOK_BITS + 1; l <= 16 && sym < 0; ++l) {
      const int32_t code = (int32_t)(v16 >> (16 - l));
      if (code <= t->maxcode[l]) {
        len = l;
        sym = t->sym[(t->valoff[l] + code) & 255];
      }
    }
    if (sym < 0) return PAR_SYM_BAD;
  }
  int s;
  if (k == 0) {
    s = sym;
    if (s > 15) return PAR_SYM_BAD;
    o->at = 0;
    o->k_next = 1;
  } else {
    const int r = sym >> 4;
    s = sym & 15;
    if (s) {
      const int kk = k + r;
      if (kk > 63) {
        o->bits = len + s;
        o->k_next = 64;
        return pos + (uint32_t)o->bits <= c.data_bits ? PAR_SYM_BAD : PAR_SYM_END;
      }
      o->at = kk;
      o->k_next = kk + 1;
    } else {
      o->k_next = r == 15 ? k + 16 : 64;             // sixteen zeros, or the end of the block
    }
  }
  if (s) o->value = extend((v << len) >> (32 - s), s);
  o->bits = len + s;
  return pos + (uint32_t)o->bits <= c.data_bits ? PAR_SYM_OK : PAR_SYM_END;
}

// The speculative / synchronising walk of one lane: from `in` to the first symbol boundary at or past end_bit (<= data_bits).
// A state at or past end_bit passes through; no state, or a walk that meets the end of the data, gives no state.  max_syms: 8 * subseq_bytes, the
// bits between the subsequence's start (no valid `in` lies before it) and its end.
VLFB_HD void par_walk(const ParCtx& c, ParState in, uint32_t end_bit, int32_t max_syms, ParState* out, int32_t* mcus) {
  *mcus = 0;
  *out = in;
  if (in.pos == PAR_NO_STATE || in.pos >= end_bit) return;
  uint32_t pos = in.pos;
  int blk = (int)(in.bk >> 6), k = (int)(in.bk & 63u);
  int32_t done = 0;
  bool ok = blk < c.mcu_blocks;
  for (int32_t n = 0; ok && n < max_syms && pos < end_bit; ++n) {
    ParSym s;
    ok = par_symbol(c, pos, blk, k, &s) != PAR_SYM_END;
    if (!ok) break;
    pos += (uint32_t)s.bits;
    k = s.k_next;
    if (k >= 64) {
      k = 0;
      if (++blk == c.mcu_blocks) { blk = 0; ++done; }
    }
  }
  *mcus = done;                                      // of a failed walk too: the write pass completes the same MCUs before it fails
  if (!ok || pos < end_bit) {
    out->pos = PAR_NO_STATE;
    out->bk = 0;
    return;
  }
  out->pos = pos;
  out->bk = (uint32_t)(blk * 64 + k);
}
// the lanes of a chunk whose subsequence begins inside the data; the others take no part (a state would need a round per lane
// to pass through them), and the chunk hands on the exit state of its last live lane
VLFB_HD int32_t par_live_lanes(uint32_t data_bits, uint32_t chunk_start_bit, int32_t lanes, int32_t subseq_bytes) {
  if (chunk_start_bit >= data_bits) return 0;
  const uint32_t bits = 8u * (uint32_t)subseq_bytes, live = (data_bits - chunk_start_bit + bits - 1u) / bits;
  return live < (uint32_t)lanes ? (int32_t)live : lanes;
}

// The write pass of one lane: the same walk from its CONFIRMED start state, whose MCU is `mcu`, into the cleared coefficient
// area: every non-zero AC coefficient, and each block's DC DIFFERENCE at index 0.  false: the item must be decoded serially.
VLFB_HD bool par_write(const ParCtx& c, const Geo& g, ParState in, uint32_t end_bit, int32_t max_syms, int64_t mcu, int64_t total,
                       uint8_t* ws) {
  if (mcu >= total) return true;                     // behind the last MCU: whatever follows is no error
  if (in.pos == PAR_NO_STATE) return false;
  if (in.pos >= end_bit) return true;
  uint32_t pos = in.pos;
  int blk = (int)(in.bk >> 6), k = (int)(in.bk & 63u);
  if (blk >= c.mcu_blocks) return false;
  int comp;
  int64_t block;
  mcu_block_place(g, mcu, blk, &comp, &block);
  int16_t* out = reinterpret_cast<int16_t*>(ws + coef_offset(g, comp) + block * 128);
  for (int32_t n = 0; n < max_syms && pos < end_bit; ++n) {
    ParSym s;
    if (par_symbol(c, pos, blk, k, &s) != PAR_SYM_OK) return false;
    if (s.at >= 0 && s.value != 0) out[natural_order(s.at)] = (int16_t)s.value;
    pos += (uint32_t)s.bits;
    k = s.k_next;
    if (k >= 64) {
      k = 0;
      if (++blk == c.mcu_blocks) {
        blk = 0;
        if (++mcu >= total) return true;
      }
      mcu_block_place(g, mcu, blk, &comp, &block);
      out = reinterpret_cast<int16_t*>(ws + coef_offset(g, comp) + block * 128);
    }
  }
  return pos >= end_bit;
}

// DC prediction as a prefix sum of the differences in decode order, modulo 2^16 (the serial (int16_t)(pred + diff) wraps the
// same way, and the wrap is associative).  sum: the differences of MCUs [m0, m1) per component; apply: the coefficients of
// those MCUs from pred[], the sums of everything before m0.
VLFB_HD void par_dc_sum(const Geo& g, const uint8_t* ws, int64_t m0, int64_t m1, uint32_t* sums) {
  for (int64_t m = m0; m < m1; ++m)
    for (int b = 0; b < g.mcu_blocks && b < MAX_MCU_BLOCKS; ++b) {
      int comp;
      int64_t block;
      mcu_block_place(g, m, b, &comp, &block);
      sums[comp] += (uint32_t)(int32_t) * reinterpret_cast<const int16_t*>(ws + coef_offset(g, comp) + block * 128);
    }
}
VLFB_HD void par_dc_apply(const Geo& g, uint8_t* ws, int64_t m0, int64_t m1, uint32_t* pred) {
  for (int64_t m = m0; m < m1; ++m)
    for (int b = 0; b < g.mcu_blocks && b < MAX_MCU_BLOCKS; ++b) {
      int comp;
      int64_t block;
      mcu_block_place(g, m, b, &comp, &block);
      int16_t* p = reinterpret_cast<int16_t*>(ws + coef_offset(g, comp) + block * 128);
      pred[comp] += (uint32_t)(int32_t)*p;
      *p = (int16_t)(uint16_t)(pred[comp] & 0xffffu);
    }
}

// ---- inverse DCT: jpeg_idct_islow (CONST_BITS 13, PASS1_BITS 2) ----------------------------------------------------------
// one pass over eight values: out = (x + 2^(shift - 1)) >> shift.  64-bit intermediates as libjpeg's JLONG, so that no stream
// can overflow them; on coefficients a real encoder writes they equal the 32-bit ones.
VLFB_HD void idct_pass(const int32_t* in, int32_t* out, int shift) {
  typedef long long L;
  L z2 = in[2], z3 = in[6];
  L z1 = (z2 + z3) * 4433;
  L tmp2 = z1 + z3 * -15137;
  L tmp3 = z1 + z2 * 6270;
  z2 = in[0]; z3 = in[4];
  L tmp0 = (z2 + z3) * 8192;
  L tmp1 = (z2 - z3) * 8192;
  const L tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
  z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
  L z4 = tmp1 + tmp3;
  const L z5 = (z3 + z4) * 9633;
  tmp0 *= 2446; tmp1 *= 16819; tmp2 *= 25172; tmp3 *= 12299;
  z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
  z3 += z5; z4 += z5;
  tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
  const L half = (L)1 << (shift - 1);
  out[0] = (int32_t)((tmp10 + tmp3 + half) >> shift);
  out[7] = (int32_t)((tmp10 - tmp3 + half) >> shift);
  out[1] = (int32_t)((tmp11 + tmp2 + half) >> shift);
  out[6] = (int32_t)((tmp11 - tmp2 + half) >> shift);
  out[2] = (int32_t)((tmp12 + tmp1 + half) >> shift);
  out[5] = (int32_t)((tmp12 - tmp1 + half) >> shift);
  out[3] = (int32_t)((tmp13 + tmp0 + half) >> shift);
  out[4] = (int32_t)((tmp13 - tmp0 + half) >> shift);
}
constexpr int IDCT_SHIFT_COLUMNS = 11, IDCT_SHIFT_ROWS = 18;
VLFB_HD uint8_t clamp255(int32_t v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }
VLFB_HD uint8_t idct_sample(int32_t v) { return clamp255(v + 128); }

// ---- upsampling and colour ------------------------------------------------------------------------------------------------
// chroma component c at output pixel (y, x): libjpeg's "fancy" triangle filter where the component is more than two samples
// wide, replication where it is not.  plane: the component's uint8 samples, rows of bw * 8.
VLFB_HD int chroma_at(const Geo& g, int c, const uint8_t* plane, int y, int x) {
  const int stride = g.bw[c] * 8;
  const int hs = g.hmax / g.h[c], vs = g.vmax / g.v[c];
  if (hs == 1) return plane[(int64_t)y * stride + x];              // vs is 1 as well: 4:4:4
  const int j = x >> 1, i = vs == 2 ? y >> 1 : y;
  const int cw = g.cw[c], ch = g.ch[c];
  if (cw <= 2) return plane[(int64_t)i * stride + j];
  const uint8_t* near = plane + (int64_t)i * stride;
  const int jn = (x & 1) ? (j + 1 < cw ? j + 1 : -1) : j - 1;      // the neighbour column, -1 at the edge
  if (vs == 1) {                                                   // 2x1
    if (jn < 0) return near[j];
    return (3 * near[j] + near[jn] + ((x & 1) ? 2 : 1)) >> 2;
  }
  int fi = (y & 1) ? i + 1 : i - 1;                                // 2x2: the far row, inside the component's real height
  fi = fi < 0 ? 0 : (fi > ch - 1 ? ch - 1 : fi);
  const uint8_t* far = plane + (int64_t)fi * stride;
  const int cj = 3 * near[j] + far[j];
  const int round = (x & 1) ? 7 : 8;
  if (jn < 0) return (4 * cj + round) >> 4;
  return (3 * cj + 3 * near[jn] + far[jn] + round) >> 4;
}

// output pixel (y, x) as B, G, R
VLFB_HD void pixel_bgr(const Geo& g, const uint8_t* const* planes, int y, int x, uint8_t* bgr) {
  const int Y = planes[0][(int64_t)y * (g.bw[0] * 8) + x];
  if (g.n_comp == 1) {
    bgr[0] = bgr[1] = bgr[2] = (uint8_t)Y;
    return;
  }
  const int cb = chroma_at(g, 1, planes[1], y, x) - 128, cr = chroma_at(g, 2, planes[2], y, x) - 128;
  bgr[2] = clamp255(Y + ((91881 * cr + 32768) >> 16));
  bgr[0] = clamp255(Y + ((116130 * cb + 32768) >> 16));
  bgr[1] = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
}

}  // namespace jpeg
}  // namespace vlfb
