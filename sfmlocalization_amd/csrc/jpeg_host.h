// The host half of a JPEG decode that every route shares: header parsing and the entropy stage (Huffman, baseline /
// extended-sequential / progressive, restart intervals) down to the quantised coefficient blocks, natural order.
// image_io.hip reconstructs pixels from them on the host (sfmloc_image_decode); imread_dev.hip lets them land in a
// pinned staging buffer and reconstructs on the device (sfmloc_imread_decode).  No HIP here, nothing but the standard
// library: tests/cpp/jpeg_coef.cpp builds it under the host sanitizers.
//
// Coefficients live where the caller says: with JpegEntropy::coef_mem set, the components' blocks are laid one after
// the other in that memory (component 0 first, each bw*bh*64 int16) and zeroed; without it each component owns a vector.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

namespace sfmloc {

inline constexpr uint8_t kZigzag[64 + 16] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33,
                                             40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36,
                                             29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                                             47, 55, 62, 63,
                                             // a run that overshoots the block lands here (jutils.c jpeg_natural_order)
                                             63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63};

struct HuffTable {
  bool defined = false;
  uint8_t bits[17] = {0};
  uint8_t vals[256] = {0};
  // canonical decoding (ITU T.81 F.2.2.3): code lengths 1..16
  int32_t maxcode[18];
  int32_t valoffset[17];
  // 9-bit lookahead: (length << 8) | symbol, 0 when the code is longer
  uint16_t look[512];

  bool build() {
    int32_t code = 0;
    int k = 0;
    memset(look, 0, sizeof(look));
    for (int l = 1; l <= 16; ++l) {
      valoffset[l] = k - code;
      for (int i = 0; i < bits[l]; ++i, ++k, ++code) {
        if (k >= 256) return false;
        if (l <= 9) {
          const int first = code << (9 - l), cnt = 1 << (9 - l);
          if (first + cnt > 512) return false;
          for (int j = 0; j < cnt; ++j) look[first + j] = (uint16_t)((l << 8) | vals[k]);
        }
      }
      if (code > (1 << l)) return false;
      maxcode[l] = bits[l] ? code - 1 : -1;
      code <<= 1;
    }
    maxcode[17] = 0x7FFFFFFF;
    return true;
  }
};

struct BitReader {
  const uint8_t *p, *end;
  uint64_t acc = 0;
  int n = 0;         // valid bits in acc (right-aligned)
  int marker = 0;    // a marker met in the entropy-coded data (0 = none)
  bool overrun = false;

  void fill() {
    while (n <= 56) {
      int byte = 0;
      if (!marker && p < end) {
        byte = *p++;
        if (byte == 0xFF) {
          while (p < end && *p == 0xFF) ++p;  // fill bytes
          const int nx = p < end ? *p++ : 0xD9;
          if (nx != 0) {
            marker = nx;
            byte = 0;
          }
        }
      } else if (!marker) {
        marker = 0xD9;
      }
      acc = (acc << 8) | (uint64_t)byte;
      n += 8;
      if (marker) break;  // zeros are fed one byte at a time past a marker
    }
  }
  inline int peek(int k) {
    if (n < k) {
      fill();
      if (n < k) {  // past a marker: pad with zeros (jdhuff.c does the same and warns)
        acc <<= (k - n) + 8;
        n += (k - n) + 8;
        overrun = true;
      }
    }
    return (int)((acc >> (n - k)) & ((1u << k) - 1));
  }
  inline void skip(int k) { n -= k; }
  inline int get(int k) {
    if (k == 0) return 0;
    const int v = peek(k);
    n -= k;
    return v;
  }
  void reset() {
    acc = 0;
    n = 0;
    marker = 0;
  }
};

inline int huff_decode(BitReader &br, const HuffTable &t) {
  const int look = br.peek(9);
  const uint16_t e = t.look[look];
  if (e) {
    br.skip(e >> 8);
    return e & 0xFF;
  }
  int32_t code = look;
  int l = 9;
  br.skip(9);
  while (l < 17 && code > t.maxcode[l]) {
    code = (code << 1) | br.get(1);
    ++l;
  }
  if (l > 16) return 0;  // corrupt data: libjpeg warns and uses 0
  return t.vals[(code + t.valoffset[l]) & 0xFF];
}

inline int jpeg_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

struct JpegComponent {
  int id = 0, hs = 1, vs = 1, tq = 0;
  int td = 0, ta = 0;           // current scan's tables
  int bw = 0, bh = 0;           // blocks allocated (padded to whole MCUs)
  int rw = 0, rh = 0;           // downsampled_width / _height: the real samples
  int last_dc = 0;
  int16_t *coef = nullptr;      // bw*bh*64, natural order: in coef_own, or in the caller's memory (JpegEntropy::coef_mem)
  std::vector<int16_t> coef_own;
  std::vector<uint8_t> plane;   // (bw*8) x (bh*8), the host reconstruction's
};

struct JpegEntropy {
  int w = 0, h = 0, ncomp = 0;
  bool progressive = false, have_sof = false;
  bool jfif = false, adobe = false;
  int adobe_transform = 0;
  int hmax = 1, vmax = 1, mcus_x = 0, mcus_y = 0;
  int restart_interval = 0;
  uint16_t quant[4][64];
  bool quant_defined[4] = {false, false, false, false};
  HuffTable dc[4], ac[4];
  JpegComponent comp[3];
  std::string err;
  // the caller's coefficient memory (null: each component owns its blocks) and how many int16 it holds
  int16_t *coef_mem = nullptr;
  size_t coef_cap = 0;

  bool fail(const char *m) {
    err = std::string("JPEG: ") + m;
    return false;
  }

  // jdapimin.c default_decompress_parms: is a three-component file YCbCr (true) or RGB as stored (false)
  bool is_ycc() const {
    if (ncomp != 3) return true;
    if (jfif) return true;
    if (adobe) return adobe_transform != 0;
    return !(comp[0].id == 'R' && comp[1].id == 'G' && comp[2].id == 'B');
  }

  bool read_dqt(const uint8_t *d, size_t len) {
    size_t p = 0;
    while (p < len) {
      const int pq = d[p] >> 4, tq = d[p] & 15;
      ++p;
      if (tq > 3 || pq > 1) return fail("bad quantisation table");
      if (p + (pq ? 128 : 64) > len) return fail("truncated quantisation table");
      for (int i = 0; i < 64; ++i) {
        const int v = pq ? (d[p] << 8) | d[p + 1] : d[p];
        p += pq ? 2 : 1;
        quant[tq][kZigzag[i]] = (uint16_t)v;
      }
      quant_defined[tq] = true;
    }
    return true;
  }

  bool read_dht(const uint8_t *d, size_t len) {
    size_t p = 0;
    while (p < len) {
      if (p + 17 > len) return fail("truncated Huffman table");
      const int tc = d[p] >> 4, th = d[p] & 15;
      if (tc > 1 || th > 3) return fail("bad Huffman table index");
      HuffTable &t = tc ? ac[th] : dc[th];
      int total = 0;
      t.bits[0] = 0;
      for (int i = 1; i <= 16; ++i) {
        t.bits[i] = d[p + i];
        total += t.bits[i];
      }
      p += 17;
      if (total > 256 || p + total > len) return fail("bad Huffman table");
      memset(t.vals, 0, sizeof(t.vals));
      memcpy(t.vals, d + p, total);
      p += total;
      if (!t.build()) return fail("bad Huffman code lengths");
      t.defined = true;
    }
    return true;
  }

  bool read_sof(const uint8_t *d, size_t len, bool allocate) {
    if (have_sof) return fail("more than one frame header");
    if (len < 6) return fail("truncated frame header");
    if (d[0] != 8) return fail("only 8-bit precision is supported");
    h = (d[1] << 8) | d[2];
    w = (d[3] << 8) | d[4];
    ncomp = d[5];
    if (w <= 0 || h <= 0) return fail("empty image");
    if (ncomp != 1 && ncomp != 3) return fail("only 1- and 3-component images are supported");
    if (len < 6 + 3 * (size_t)ncomp) return fail("truncated frame header");
    for (int i = 0; i < ncomp; ++i) {
      JpegComponent &c = comp[i];
      c.id = d[6 + 3 * i];
      c.hs = d[7 + 3 * i] >> 4;
      c.vs = d[7 + 3 * i] & 15;
      c.tq = d[8 + 3 * i];
      if (c.tq > 3) return fail("bad quantisation table index");
    }
    if (ncomp == 1) comp[0].hs = comp[0].vs = 1;  // a single component is never subsampled (jdinput.c)
    const bool ok_first = (comp[0].hs == 1 || comp[0].hs == 2) && (comp[0].vs == 1 || comp[0].vs == 2);
    bool ok_rest = true;
    for (int i = 1; i < ncomp; ++i) ok_rest = ok_rest && comp[i].hs == 1 && comp[i].vs == 1;
    if (!ok_first || !ok_rest || (ncomp == 3 && comp[0].hs == 1 && comp[0].vs == 2))
      return fail("unsupported chroma subsampling (4:4:4, 4:2:2 and 4:2:0 are)");
    hmax = comp[0].hs;
    vmax = comp[0].vs;
    mcus_x = (w + 8 * hmax - 1) / (8 * hmax);
    mcus_y = (h + 8 * vmax - 1) / (8 * vmax);
    size_t used = 0;
    for (int i = 0; i < ncomp; ++i) {
      JpegComponent &c = comp[i];
      c.bw = mcus_x * c.hs;
      c.bh = mcus_y * c.vs;
      c.rw = (w * c.hs + hmax - 1) / hmax;
      c.rh = (h * c.vs + vmax - 1) / vmax;
      if (!allocate) continue;
      const size_t n = (size_t)c.bw * c.bh * 64;
      if (coef_mem) {
        if (used + n > coef_cap) return fail("frame larger than the coefficient buffer");
        c.coef = coef_mem + used;
        memset(c.coef, 0, n * sizeof(int16_t));
        used += n;
      } else {
        c.coef_own.assign(n, 0);
        c.coef = c.coef_own.data();
      }
    }
    have_sof = true;
    return true;
  }

  // ----- entropy decoding of one scan into the coefficient arrays -----
  struct Scan {
    int n = 0;
    int ci[3];
    int ss = 0, se = 63, ah = 0, al = 0;
  };

  bool decode_block_sequential(BitReader &br, JpegComponent &c, int16_t *blk) {
    const HuffTable &dt = dc[c.td], &at = ac[c.ta];
    int s = huff_decode(br, dt);
    if (s) {
      if (s > 15) return fail("bad DC difference");
      s = jpeg_extend(br.get(s), s);
    }
    c.last_dc = (int)((unsigned)c.last_dc + (unsigned)s);  // wraps on hostile data instead of overflowing
    blk[0] = (int16_t)c.last_dc;
    for (int k = 1; k < 64;) {
      const int rs = huff_decode(br, at), r = rs >> 4;
      s = rs & 15;
      if (s) {
        k += r;
        blk[kZigzag[k]] = (int16_t)jpeg_extend(br.get(s), s);
        ++k;
      } else {
        if (r != 15) break;
        k += 16;
      }
    }
    return true;
  }

  // jdphuff.c decode_mcu_DC_first / _AC_first / _DC_refine / _AC_refine for one block
  bool decode_block_progressive(BitReader &br, JpegComponent &c, int16_t *blk, const Scan &sc, unsigned &eobrun) {
    if (sc.ss == 0) {
      if (sc.ah == 0) {
        int s = huff_decode(br, dc[c.td]);
        if (s) {
          if (s > 15) return fail("bad DC difference");
          s = jpeg_extend(br.get(s), s);
        }
        c.last_dc = (int)((unsigned)c.last_dc + (unsigned)s);  // wraps on hostile data instead of overflowing
        blk[0] = (int16_t)((int64_t)c.last_dc * (1 << sc.al));
      } else if (br.get(1)) {
        blk[0] |= (int16_t)(1 << sc.al);
      }
      return true;
    }
    const HuffTable &at = ac[c.ta];
    if (sc.ah == 0) {
      if (eobrun > 0) {
        --eobrun;
        return true;
      }
      for (int k = sc.ss; k <= sc.se; ++k) {
        const int rs = huff_decode(br, at), r = rs >> 4;
        int s = rs & 15;
        if (s) {
          k += r;
          s = jpeg_extend(br.get(s), s);
          blk[kZigzag[k]] = (int16_t)(s * (1 << sc.al));
        } else if (r == 15) {
          k += 15;
        } else {
          eobrun = 1u << r;
          if (r) eobrun += (unsigned)br.get(r);
          --eobrun;
          break;
        }
      }
      return true;
    }
    const int p1 = 1 << sc.al, m1 = -(1 << sc.al);
    int k = sc.ss;
    if (eobrun == 0) {
      for (; k <= sc.se; ++k) {
        const int rs = huff_decode(br, at);
        int r = rs >> 4, s = rs & 15;
        if (s) {
          s = br.get(1) ? p1 : m1;  // the size must be 1
        } else if (r != 15) {
          eobrun = 1u << r;
          if (r) eobrun += (unsigned)br.get(r);
          break;  // force end-of-band
        }
        do {
          int16_t *co = blk + kZigzag[k];
          if (*co != 0) {
            if (br.get(1) && (*co & p1) == 0) *co = (int16_t)(*co + (*co >= 0 ? p1 : m1));
          } else if (--r < 0) {
            break;
          }
          ++k;
        } while (k <= sc.se);
        if (s) blk[kZigzag[k]] = (int16_t)s;
      }
    }
    if (eobrun > 0) {
      for (; k <= sc.se; ++k) {
        int16_t *co = blk + kZigzag[k];
        if (*co != 0 && br.get(1) && (*co & p1) == 0) *co = (int16_t)(*co + (*co >= 0 ? p1 : m1));
      }
      --eobrun;
    }
    return true;
  }

  bool decode_scan(const uint8_t *d, size_t len, const uint8_t *data, const uint8_t *data_end, const uint8_t **next) {
    if (!have_sof) return fail("scan before the frame header");
    if (len < 1) return fail("truncated scan header");
    Scan sc;
    sc.n = d[0];
    if (sc.n < 1 || sc.n > ncomp || len < 1 + 2 * (size_t)sc.n + 3) return fail("bad scan header");
    for (int i = 0; i < sc.n; ++i) {
      const int id = d[1 + 2 * i];
      int ci = -1;
      for (int j = 0; j < ncomp; ++j)
        if (comp[j].id == id) ci = j;
      if (ci < 0) return fail("scan names an unknown component");
      sc.ci[i] = ci;
      comp[ci].td = d[2 + 2 * i] >> 4;
      comp[ci].ta = d[2 + 2 * i] & 15;
      if (comp[ci].td > 3 || comp[ci].ta > 3) return fail("bad table selector");
    }
    sc.ss = d[1 + 2 * sc.n];
    sc.se = d[2 + 2 * sc.n];
    sc.ah = d[3 + 2 * sc.n] >> 4;
    sc.al = d[3 + 2 * sc.n] & 15;
    if (progressive) {
      if (sc.ss > sc.se || sc.se > 63 || sc.al > 13 || (sc.ss == 0 && sc.se != 0) || (sc.ss != 0 && sc.n != 1))
        return fail("bad progressive scan parameters");
    } else {
      sc.ss = 0;
      sc.se = 63;
      sc.ah = sc.al = 0;
    }
    for (int i = 0; i < sc.n; ++i) {
      const JpegComponent &c = comp[sc.ci[i]];
      const bool need_dc = sc.ss == 0 && sc.ah == 0, need_ac = progressive ? sc.ss != 0 : true;
      if ((need_dc && !dc[c.td].defined) || (need_ac && !ac[c.ta].defined)) return fail("scan uses an undefined Huffman table");
    }
    BitReader br;
    br.p = data;
    br.end = data_end;
    unsigned eobrun = 0;
    for (int i = 0; i < ncomp; ++i) comp[i].last_dc = 0;
    // a one-component scan walks that component's own blocks (ceil(real size / 8)), not the padded MCU grid
    int nx, ny;
    if (sc.n == 1) {
      const JpegComponent &c = comp[sc.ci[0]];
      nx = (c.rw + 7) / 8;
      ny = (c.rh + 7) / 8;
    } else {
      nx = mcus_x;
      ny = mcus_y;
    }
    long until_restart = restart_interval;
    int next_rst = 0;
    for (int my = 0; my < ny; ++my) {
      for (int mx = 0; mx < nx; ++mx) {
        if (restart_interval && until_restart == 0) {
          // RSTn: byte-align, expect the marker, reset the predictors (jdhuff.c process_restart)
          br.n = 0;
          br.acc = 0;
          if (!br.marker) {  // the marker may not have been reached yet when the last MCU ended on a byte boundary
            br.fill();
            br.n = 0;
            br.acc = 0;
          }
          if (br.marker != 0xD0 + next_rst) return fail("missing restart marker");
          br.marker = 0;
          next_rst = (next_rst + 1) & 7;
          for (int i = 0; i < ncomp; ++i) comp[i].last_dc = 0;
          eobrun = 0;
          until_restart = restart_interval;
        }
        if (sc.n == 1) {
          JpegComponent &c = comp[sc.ci[0]];
          int16_t *blk = &c.coef[((size_t)my * c.bw + mx) * 64];
          const bool ok = progressive ? decode_block_progressive(br, c, blk, sc, eobrun) : decode_block_sequential(br, c, blk);
          if (!ok) return false;
        } else {
          for (int i = 0; i < sc.n; ++i) {
            JpegComponent &c = comp[sc.ci[i]];
            for (int by = 0; by < c.vs; ++by)
              for (int bx = 0; bx < c.hs; ++bx) {
                int16_t *blk = &c.coef[((size_t)(my * c.vs + by) * c.bw + (mx * c.hs + bx)) * 64];
                const bool ok =
                    progressive ? decode_block_progressive(br, c, blk, sc, eobrun) : decode_block_sequential(br, c, blk);
                if (!ok) return false;
              }
          }
        }
        --until_restart;
      }
    }
    // position after the scan: the marker the bit reader stopped at, if any, else search for the next one
    if (br.marker) {
      *next = br.p - 2;
    } else {
      const uint8_t *q = br.p;
      while (q + 1 < data_end && !(q[0] == 0xFF && q[1] != 0x00 && q[1] != 0xFF && !(q[1] >= 0xD0 && q[1] <= 0xD7))) ++q;
      *next = q;
    }
    return true;
  }

  bool parse(const uint8_t *raw, size_t n, bool header_only) {
    size_t p = 2;
    bool seen_scan = false;
    while (p + 4 <= n) {
      if (raw[p] != 0xFF) {
        ++p;  // garbage between segments: libjpeg skips it with a warning
        continue;
      }
      const int m = raw[p + 1];
      if (m == 0xFF) {
        ++p;
        continue;
      }
      if (m == 0xD9) break;
      if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) {
        p += 2;
        continue;
      }
      const size_t len = ((size_t)raw[p + 2] << 8) | raw[p + 3];
      if (len < 2 || p + 2 + len > n) return fail("truncated segment");
      const uint8_t *d = raw + p + 4;
      const size_t dl = len - 2;
      p += 2 + len;
      switch (m) {
        case 0xDB:
          if (!read_dqt(d, dl)) return false;
          break;
        case 0xC4:
          if (!read_dht(d, dl)) return false;
          break;
        case 0xC0:
        case 0xC1:
        case 0xC2:
          progressive = (m == 0xC2);
          if (!read_sof(d, dl, !header_only)) return false;
          if (header_only) return true;
          break;
        case 0xC3: case 0xC5: case 0xC6: case 0xC7: case 0xC9: case 0xCA: case 0xCB: case 0xCD: case 0xCE: case 0xCF:
          return fail("lossless, hierarchical and arithmetic-coded files are not supported");
        case 0xDD:
          if (dl < 2) return fail("truncated restart interval");
          restart_interval = (d[0] << 8) | d[1];
          break;
        case 0xE0:
          if (dl >= 5 && !memcmp(d, "JFIF", 5)) jfif = true;
          break;
        case 0xEE:
          if (dl >= 12 && !memcmp(d, "Adobe", 5)) {
            adobe = true;
            adobe_transform = d[11];
          }
          break;
        case 0xDA: {
          if (header_only) return have_sof ? true : fail("scan before the frame header");
          const uint8_t *next = nullptr;
          if (!decode_scan(d, dl, raw + p, raw + n, &next)) return false;
          seen_scan = true;
          p = (size_t)(next - raw);
        } break;
        default: break;  // APPn, COM, DNL ...
      }
    }
    if (!have_sof || !seen_scan) return fail("no image data");
    return true;
  }
};

// image_io.hip, for callers inside the library and for tests/cpp/jpeg_coef.cpp:
// a JPEG decode in its two halves -- the entropy stage into the caller's coef_mem (coef_cap int16), then the host
// reconstruction (islow IDCT, fancy upsampling, colour) from that memory; px: h x w gray, or h x w x 3 B G R.  The same
// bytes as sfmloc_image_decode, and on failure the text that follows "sfmloc_image_decode: "
bool jpeg_decode_split_host(const uint8_t *raw, size_t n, bool color, int16_t *coef_mem, size_t coef_cap, int *w, int *h,
                            std::vector<uint8_t> *px, std::string *err);
// what sfmloc_image_decode does between its argument check and its copy-out (any format); false: *err has the text that
// follows "sfmloc_image_decode: "
bool image_decode_host(const uint8_t *raw, size_t n, bool color, int *w, int *h, std::vector<uint8_t> *px, std::string *err);

}  // namespace sfmloc
