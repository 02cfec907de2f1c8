// Host half of the baseline JPEG decoder (msl_jpeg_info / msl_jpeg_entropy_decode, include/msl_hip.h): the
// marker parser and the Huffman decoder, the serial part of a decode.  What they leave - quantised
// coefficients in natural order, the quantisation tables and a header - is finished on the device (jpeg.hip).
//
// Plain C++17, no HIP: jpeg.hip includes it for the library, tests/jpeg_host_main.cpp for a stand-alone
// program a host compiler builds with its sanitizers.  No global state, no allocation; every function is
// re-entrant.  The two memory rules, held by construction and not by trusting the stream:
//   - a byte of the file is read only through an index checked against n (segment bodies: the segment's
//     length is checked against n once, then indices against the length; the scan: Bits::next);
//   - a coefficient is written only at block base + kZigzag[k] with k checked <= 63, the block base from
//     MCU indices below the grid the header was sized by, after coef_elems was checked against that grid.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/msl_hip.h"

namespace msl {
namespace jpeg {

static const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int kLook = 9;  // bits of the one-step code table

struct Huff {
  bool defined;
  uint8_t look_len[1 << kLook], look_sym[1 << kLook];  // by the next kLook bits: the code's length (0: longer) and symbol
  int32_t maxcode[18];                                 // largest code of each length, -1 if none; [17] ends the search
  int32_t valoff[17];                                  // index of a length's first symbol minus its first code
  uint8_t vals[256];
};

// counts[16] codes per length, then the symbols: a canonical Huffman table as DHT carries it
static inline int build_huff(Huff& t, const uint8_t* counts, const uint8_t* syms, int nsyms, bool dc) {
  memset(&t, 0, sizeof(t));
  int32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    t.valoff[l] = k - code;
    t.maxcode[l] = counts[l - 1] ? code + counts[l - 1] - 1 : -1;
    for (int i = 0; i < counts[l - 1]; ++i, ++k, ++code) {
      if (k >= nsyms) return MSL_ERR_ARG;
      const uint8_t sym = syms[k];
      if (dc && sym > 15) return MSL_ERR_ARG;  // a DC category above 15 (libjpeg: JERR_BAD_HUFF_TABLE)
      t.vals[k] = sym;
      if (l <= kLook) {
        if (code >= (1 << l)) return MSL_ERR_ARG;
        const int first = code << (kLook - l);
        for (int j = 0; j < (1 << (kLook - l)); ++j) {
          t.look_len[first + j] = (uint8_t)l;
          t.look_sym[first + j] = sym;
        }
      }
    }
    if (code > (1 << l)) return MSL_ERR_ARG;  // more codes than l bits hold
    code <<= 1;
  }
  t.maxcode[17] = 0x7fffffff;
  t.defined = true;
  return MSL_OK;
}

// The entropy-coded segment as a bit stream: FF 00 is a data byte FF, FF FF.. is fill, FF and anything else a
// marker.  At a marker or the end of the file the reader stops advancing and feeds zero bits, counted in
// `fake`; a decoder that has consumed one of them (nbits < fake) has run off the data.
struct Bits {
  const uint8_t* d;
  size_t n, p;
  uint64_t acc;  // the low nbits bits are unread, the oldest on top
  int nbits, fake;
  bool hit;      // at a marker or at the end of the file

  int next() {
    while (!hit) {
      if (p >= n) break;
      const uint8_t b = d[p];
      if (b != 0xFF) {
        ++p;
        return b;
      }
      if (p + 1 >= n) break;
      const uint8_t b2 = d[p + 1];
      if (b2 == 0) {
        p += 2;
        return 0xFF;
      }
      if (b2 != 0xFF) break;
      ++p;  // fill
    }
    hit = true;
    fake += 8;
    return 0;
  }
  void fill() {  // at least 49 unread bits: one code (16) and its value bits (15) at the most between fills
    if (nbits <= 32 && !hit && p + 4 <= n) {
      // four data bytes at once when none of them is FF (no stuffing, no marker among them)
      const uint32_t v = (uint32_t)d[p] << 24 | (uint32_t)d[p + 1] << 16 | (uint32_t)d[p + 2] << 8 | (uint32_t)d[p + 3];
      const uint32_t x = ~v;  // a zero byte of x is an FF byte of v
      if (!((x - 0x01010101u) & ~x & 0x80808080u)) {
        acc = (acc << 32) | v;
        nbits += 32;
        p += 4;
      }
    }
    while (nbits <= 48) {
      acc = (acc << 8) | (uint64_t)next();
      nbits += 8;
    }
  }
  int peek(int k) const { return (int)((acc >> (nbits - k)) & ((1u << k) - 1)); }
  void skip(int k) { nbits -= k; }
  int get(int k) {
    const int v = peek(k);
    nbits -= k;
    return v;
  }
  bool overrun() const { return nbits < fake; }
  void reset() {
    acc = 0;
    nbits = fake = 0;
    hit = false;
  }
};

// the next symbol, -1 if no code of the table matches the next 16 bits; call after fill()
static inline int decode_symbol(Bits& b, const Huff& t) {
  const int look = b.peek(kLook);
  int l = t.look_len[look];
  if (l) {
    b.skip(l);
    return t.look_sym[look];
  }
  l = kLook + 1;
  int32_t code = b.peek(l);
  while (code > t.maxcode[l]) {
    ++l;
    if (l > 16) return -1;
    code = b.peek(l);
  }
  const uint32_t at = (uint32_t)(code + t.valoff[l]);
  if (at >= 256u) return -1;
  b.skip(l);
  return t.vals[at];
}

// a value of category s >= 1 from its s bits (T.81 F.2.2.1 EXTEND)
static inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

struct Parsed {
  msl_jpeg_header hdr;
  uint16_t quant[4][64];  // natural order
  bool quant_defined[4];
  struct {
    const uint8_t* counts;  // into the file: 16 counts, then the symbols
    int nsyms;
  } dht[2][4];              // [DC | AC][table]
  int td[3], ta[3];         // the scan's table selectors per component
  size_t scan;              // index of the first entropy-coded byte
};

static inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Fill the block grid and offsets of a header whose size, ncomp, hmax, vmax and per-component h, v are set.
static inline void lay_out(msl_jpeg_header& h) {
  h.mcus_w = (h.width + 8 * h.hmax - 1) / (8 * h.hmax);
  h.mcus_h = (h.height + 8 * h.vmax - 1) / (8 * h.vmax);
  int64_t off = 0;
  for (int c = 0; c < h.ncomp; ++c) {
    h.comp[c].blocks_w = h.mcus_w * h.comp[c].h;
    h.comp[c].blocks_h = h.mcus_h * h.comp[c].v;
    h.comp[c].reserved = 0;
    h.comp[c].offset = off;
    off += (int64_t)h.comp[c].blocks_w * h.comp[c].blocks_h * 64;
  }
}

static inline size_t coef_elems(const msl_jpeg_header& h) {
  size_t e = 0;
  for (int c = 0; c < h.ncomp && c < 3; ++c) e += (size_t)h.comp[c].blocks_w * (size_t)h.comp[c].blocks_h * 64;
  return e;
}

// MSL_OK if h is a header parse() writes for its own width, height, ncomp and sampling
static inline int check_header(const msl_jpeg_header& h) {
  if (h.width < 1 || h.height < 1 || h.width > 65535 || h.height > 65535) return MSL_ERR_ARG;
  if (h.ncomp != 1 && h.ncomp != 3) return MSL_ERR_ARG;
  msl_jpeg_header want = h;
  if (h.ncomp == 1) {
    if (h.hmax != 1 || h.vmax != 1 || h.comp[0].h != 1 || h.comp[0].v != 1) return MSL_ERR_ARG;
  } else {
    const bool luma = (h.hmax == 1 && h.vmax == 1) || (h.hmax == 2 && h.vmax == 1) || (h.hmax == 2 && h.vmax == 2);
    if (!luma || h.comp[0].h != h.hmax || h.comp[0].v != h.vmax) return MSL_ERR_ARG;
    for (int c = 1; c < 3; ++c)
      if (h.comp[c].h != 1 || h.comp[c].v != 1) return MSL_ERR_ARG;
  }
  lay_out(want);
  if (want.mcus_w != h.mcus_w || want.mcus_h != h.mcus_h) return MSL_ERR_ARG;
  for (int c = 0; c < h.ncomp; ++c) {
    if ((unsigned)h.comp[c].tq > 3u || want.comp[c].blocks_w != h.comp[c].blocks_w ||
        want.comp[c].blocks_h != h.comp[c].blocks_h || want.comp[c].offset != h.comp[c].offset)
      return MSL_ERR_ARG;
  }
  return MSL_OK;
}

// The markers from SOI to the end of the scan header.
static inline int parse(const uint8_t* d, size_t n, Parsed& P) {
  memset(&P, 0, sizeof(P));
  if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8) return MSL_ERR_ARG;
  size_t i = 2;
  bool sof = false, jfif = false, adobe = false;
  int transform = -1, ids[3] = {0, 0, 0};
  for (;;) {
    if (i + 1 >= n || d[i] != 0xFF) return MSL_ERR_ARG;
    while (i + 1 < n && d[i + 1] == 0xFF) ++i;  // fill bytes before a marker
    if (i + 1 >= n) return MSL_ERR_ARG;
    const int m = d[i + 1];
    i += 2;
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;  // TEM, a stray RSTn: no body
    if (m == 0xD8 || m == 0xD9 || m == 0x00) return MSL_ERR_ARG;  // a second SOI, EOI before any scan
    if (i + 2 > n) return MSL_ERR_ARG;
    const size_t L = (size_t)be16(d + i);
    if (L < 2 || i + L > n) return MSL_ERR_ARG;
    const uint8_t* s = d + i + 2;  // the body: s[0 .. len)
    const size_t len = L - 2;
    i += L;
    if (m == 0xC0 || m == 0xC1) {
      if (sof || len < 6) return MSL_ERR_ARG;
      sof = true;
      const int prec = s[0], H = be16(s + 1), W = be16(s + 3), nc = s[5];
      if (nc < 1 || len != 6 + 3 * (size_t)nc || W == 0) return MSL_ERR_ARG;
      if (prec != 8) return prec == 12 ? MSL_ERR_SHAPE : MSL_ERR_ARG;
      if (H == 0) return MSL_ERR_SHAPE;  // the height comes in a DNL marker
      for (int c = 0; c < nc; ++c) {
        const int h = s[7 + 3 * c] >> 4, v = s[7 + 3 * c] & 15, tq = s[8 + 3 * c];
        if (h < 1 || h > 4 || v < 1 || v > 4 || tq > 3) return MSL_ERR_ARG;
      }
      if (nc != 1 && nc != 3) return MSL_ERR_SHAPE;
      msl_jpeg_header& h = P.hdr;
      h.width = W;
      h.height = H;
      h.ncomp = nc;
      for (int c = 0; c < nc; ++c) {
        ids[c] = s[6 + 3 * c];
        h.comp[c].h = s[7 + 3 * c] >> 4;
        h.comp[c].v = s[7 + 3 * c] & 15;
        h.comp[c].tq = s[8 + 3 * c];
      }
      if (nc == 1) {
        h.comp[0].h = h.comp[0].v = 1;  // one component: its scan is not interleaved, an MCU is one block
      } else {
        const int lh = h.comp[0].h, lv = h.comp[0].v;
        const bool luma = (lh == 1 && lv == 1) || (lh == 2 && lv == 1) || (lh == 2 && lv == 2);
        if (!luma || h.comp[1].h != 1 || h.comp[1].v != 1 || h.comp[2].h != 1 || h.comp[2].v != 1) return MSL_ERR_SHAPE;
        if (ids[0] == ids[1] || ids[0] == ids[2] || ids[1] == ids[2]) return MSL_ERR_ARG;
      }
      h.hmax = h.comp[0].h;
      h.vmax = h.comp[0].v;
      lay_out(h);
    } else if ((m >= 0xC2 && m <= 0xCF && m != 0xC4) || m == 0xDC || m == 0xDE || m == 0xDF) {
      return MSL_ERR_SHAPE;  // progressive, lossless, differential, arithmetic (and DAC), DNL, hierarchical
    } else if (m == 0xDB) {
      size_t p = 0;
      while (p < len) {
        const int pq = s[p] >> 4, tq = s[p] & 15;
        ++p;
        if (pq > 1 || tq > 3 || p + (pq ? 128u : 64u) > len) return MSL_ERR_ARG;
        for (int k = 0; k < 64; ++k, p += pq ? 2 : 1) P.quant[tq][kZigzag[k]] = (uint16_t)(pq ? be16(s + p) : s[p]);
        P.quant_defined[tq] = true;
      }
    } else if (m == 0xC4) {
      size_t p = 0;
      while (p < len) {
        const int tc = s[p] >> 4, th = s[p] & 15;
        if (tc > 1 || th > 3 || p + 17 > len) return MSL_ERR_ARG;
        int cnt = 0;
        for (int k = 0; k < 16; ++k) cnt += s[p + 1 + k];
        if (cnt > 256 || p + 17 + (size_t)cnt > len) return MSL_ERR_ARG;
        P.dht[tc][th].counts = s + p + 1;
        P.dht[tc][th].nsyms = cnt;
        p += 17 + (size_t)cnt;
      }
    } else if (m == 0xDD) {
      if (len != 2) return MSL_ERR_ARG;
      P.hdr.restart_interval = be16(s);
    } else if (m == 0xE0) {
      if (len >= 14 && !memcmp(s, "JFIF\0", 5)) jfif = true;
    } else if (m == 0xEE) {
      if (len >= 12 && !memcmp(s, "Adobe", 5)) {
        adobe = true;
        transform = s[11];
      }
    } else if (m == 0xDA) {
      if (!sof || len < 1) return MSL_ERR_ARG;
      const int ns = s[0];
      if (ns < 1 || ns > 4 || len != 4 + 2 * (size_t)ns) return MSL_ERR_ARG;
      const msl_jpeg_header& h = P.hdr;
      if (ns != h.ncomp) return MSL_ERR_SHAPE;  // one of several scans
      for (int c = 0; c < ns; ++c) {
        if (s[1 + 2 * c] != ids[c]) return MSL_ERR_ARG;  // scan components come in frame order
        P.td[c] = s[2 + 2 * c] >> 4;
        P.ta[c] = s[2 + 2 * c] & 15;
        if (P.td[c] > 3 || P.ta[c] > 3) return MSL_ERR_ARG;
        if (!P.dht[0][P.td[c]].counts || !P.dht[1][P.ta[c]].counts || !P.quant_defined[h.comp[c].tq]) return MSL_ERR_ARG;
      }
      if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return MSL_ERR_ARG;  // Ss, Se, Ah/Al
      if (h.ncomp == 3) {
        // libjpeg's rule for a 3-component file (jdapimin.c default_decompress_parms)
        const bool rgb_ids = ids[0] == 'R' && ids[1] == 'G' && ids[2] == 'B';
        const bool ycc = jfif || (adobe ? transform == 1 : !rgb_ids);
        if (!ycc) return MSL_ERR_SHAPE;
      }
      P.scan = i;
      return MSL_OK;
    }
    // APPn, COM and anything else with a length: skipped
  }
}

static inline int info(const uint8_t* file, size_t n, msl_jpeg_header* header) {
  if (!file || !header) return MSL_ERR_ARG;
  Parsed P;
  const int st = parse(file, n, P);
  if (st != MSL_OK) return st;
  *header = P.hdr;
  return MSL_OK;
}

static inline int entropy_decode(const uint8_t* file, size_t n, msl_jpeg_header* header, int16_t* coef,
                                 size_t n_coef, uint16_t* quant) {
  if (!file || !header || !coef || !quant) return MSL_ERR_ARG;
  Parsed P;
  int st = parse(file, n, P);
  if (st != MSL_OK) return st;
  const msl_jpeg_header& h = P.hdr;
  if (n_coef < coef_elems(h)) return MSL_ERR_WORKSPACE;
  Huff dc[3], ac[3];
  for (int c = 0; c < h.ncomp; ++c) {
    if ((st = build_huff(dc[c], P.dht[0][P.td[c]].counts, P.dht[0][P.td[c]].counts + 16, P.dht[0][P.td[c]].nsyms,
                         true)) != MSL_OK)
      return st;
    if ((st = build_huff(ac[c], P.dht[1][P.ta[c]].counts, P.dht[1][P.ta[c]].counts + 16, P.dht[1][P.ta[c]].nsyms,
                         false)) != MSL_OK)
      return st;
  }
  Bits b;
  b.d = file;
  b.n = n;
  b.p = P.scan;
  b.reset();
  int32_t pred[3] = {0, 0, 0};
  const int ri = h.restart_interval;
  int todo = ri, rst = 0;
  for (int my = 0; my < h.mcus_h; ++my) {
    for (int mx = 0; mx < h.mcus_w; ++mx) {
      if (ri && todo == 0) {
        // every data byte before the marker is consumed (at most the last byte's padding bits are left)
        if (b.overrun() || b.nbits - b.fake >= 8) return MSL_ERR_ARG;
        size_t p = b.p;
        if (p + 1 >= n || file[p] != 0xFF) return MSL_ERR_ARG;
        while (p + 1 < n && file[p + 1] == 0xFF) ++p;
        if (p + 1 >= n || file[p + 1] != 0xD0 + rst) return MSL_ERR_ARG;
        b.p = p + 2;
        b.reset();
        rst = (rst + 1) & 7;
        pred[0] = pred[1] = pred[2] = 0;
        todo = ri;
      }
      --todo;
      for (int c = 0; c < h.ncomp; ++c) {
        const msl_jpeg_comp& cc = h.comp[c];
        for (int v = 0; v < cc.v; ++v) {
          for (int hh = 0; hh < cc.h; ++hh) {
            int16_t* blk = coef + cc.offset + ((size_t)(my * cc.v + v) * cc.blocks_w + (size_t)(mx * cc.h + hh)) * 64;
            memset(blk, 0, 64 * sizeof(int16_t));
            b.fill();
            int s = decode_symbol(b, dc[c]);
            if (s < 0) return MSL_ERR_ARG;  // (a DC symbol is <= 15: build_huff)
            const int diff = s ? extend(b.get(s), s) : 0;
            pred[c] = (int32_t)((uint32_t)pred[c] + (uint32_t)diff);
            blk[0] = (int16_t)(uint16_t)(uint32_t)pred[c];  // libjpeg keeps the low 16 bits too (JCOEF)
            for (int k = 1; k < 64;) {
              b.fill();
              const int rs = decode_symbol(b, ac[c]);
              if (rs < 0) return MSL_ERR_ARG;
              const int r = rs >> 4;
              s = rs & 15;
              if (s == 0) {
                if (r != 15) break;  // EOB
                k += 16;
                continue;
              }
              k += r;
              if (k > 63) return MSL_ERR_ARG;
              blk[kZigzag[k]] = (int16_t)extend(b.get(s), s);
              ++k;
            }
            if (b.overrun()) return MSL_ERR_ARG;  // the data ended inside this block
          }
        }
      }
    }
  }
  *header = h;
  memcpy(quant, P.quant, sizeof(P.quant));
  return MSL_OK;
}

}  // namespace jpeg
}  // namespace msl
