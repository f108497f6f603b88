// cv::imread for the query image (AKAZEOpenCV.cpp:60 IMREAD_GRAYSCALE; DenseLocalFeatureWrapper.cpp:85 and
// localizeImage.cc:463 IMREAD_COLOR), host code: sfmloc_image_decode / sfmloc_image_read of include/sfmloc.h.
//
// The reference gets its pixels from OpenCV's image codecs, i.e. from libjpeg and libpng; neither has headers in this
// image, so the containers the reference's tools accept (localization.cpp:204-206: jpg/jpeg/png) are decoded here:
//   JPEG  baseline, extended-sequential and progressive Huffman, 8 bit, 1 or 3 components, h/v sampling 1 or 2 for
//         the first component and 1x1 for the others (4:4:4, 4:2:2, 4:2:0), restart intervals.  The arithmetic is a
//         restatement of libjpeg's default decompression path so that the pixels are the ones imread returns:
//         jidctint.c (jpeg_idct_islow: 13-bit constants, two passes, range-limit table), jdsample.c (h2v1 / h2v2
//         "fancy" triangle upsampling incl. its edge rules and alternating rounding), jdcolor.c (16-bit fixed-point
//         YCbCr -> RGB tables).  IMREAD_GRAYSCALE asks libjpeg for JCS_GRAYSCALE (grfmt_jpeg.cpp), which is the
//         Y plane itself -- no colour conversion, no upsampling.  tests/test_image_io.py pins every mode against
//         libjpeg-turbo (through PIL) bit for bit.
//   PNG   8 bit, non-interlaced: gray, gray+alpha, RGB, RGBA, palette.  IMREAD_GRAYSCALE on a colour PNG is libpng's
//         png_set_rgb_to_gray(1, 0.299, 0.587) (grfmt_png.cpp): (9797 R + 19234 G + 3737 B) >> 15 (truncated), and the
//         pixel itself when R == G == B.
//   PGM/PPM binary, maxval 255 (cvtColor BGR2GRAY for colour, as grfmt_pxm.cpp does through icvCvt_BGR2Gray).
#include <zlib.h>

#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "jpeg_host.h"
#include "sfmloc_internal.h"

namespace sfmloc {
namespace {

struct Image {
  int w = 0, h = 0, ch = 0;  // ch = channels of `px` (1 gray, 3 B G R)
  std::vector<uint8_t> px;
};

// ---------------------------------------------------------------------------------------------------------
// PNM
// ---------------------------------------------------------------------------------------------------------
inline uint8_t cv_bgr2gray(int r, int g, int b) { return (uint8_t)((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14); }

bool decode_pnm(const uint8_t *raw, size_t n_raw, bool color, Image *im, std::string *err) {
  size_t p = 2;
  int vals[3], nv = 0;
  while (nv < 3 && p < n_raw) {
    while (p < n_raw && isspace(raw[p])) ++p;
    if (p < n_raw && raw[p] == '#') {
      while (p < n_raw && raw[p] != '\n') ++p;
      continue;
    }
    int v = 0;
    bool any = false;
    while (p < n_raw && isdigit(raw[p]) && v < 100000000) {
      v = v * 10 + (raw[p++] - '0');
      any = true;
    }
    if (!any) break;
    vals[nv++] = v;
  }
  if (nv < 3 || vals[2] != 255 || p >= n_raw || vals[0] <= 0 || vals[1] <= 0) {
    *err = "PNM: only binary P5/P6 with maxval 255";
    return false;
  }
  ++p;  // the single whitespace after maxval
  const size_t n = (size_t)vals[0] * vals[1], sch = raw[1] == '6' ? 3 : 1;
  if (n_raw < p + n * sch) {
    *err = "PNM: truncated";
    return false;
  }
  im->w = vals[0];
  im->h = vals[1];
  im->ch = color ? 3 : 1;
  im->px.resize(n * im->ch);
  for (size_t i = 0; i < n; ++i) {
    const int r = raw[p + sch * i], g = sch == 1 ? r : raw[p + 3 * i + 1], b = sch == 1 ? r : raw[p + 3 * i + 2];
    if (color) {
      im->px[3 * i] = (uint8_t)b;
      im->px[3 * i + 1] = (uint8_t)g;
      im->px[3 * i + 2] = (uint8_t)r;
    } else {
      im->px[i] = sch == 1 ? (uint8_t)r : cv_bgr2gray(r, g, b);
    }
  }
  return true;
}

// ---------------------------------------------------------------------------------------------------------
// PNG
// ---------------------------------------------------------------------------------------------------------
inline uint32_t be32(const uint8_t *p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

// libpng png_do_rgb_to_gray, 8 bit, no gamma; coefficients of png_set_rgb_to_gray_fixed(29900, 58700); libpng
// truncates ("the historical approach"), it does not round -- pinned against libpng 1.6 itself in tests/test_image_io.py
inline uint8_t png_rgb_to_gray(int r, int g, int b) {
  if (r == g && r == b) return (uint8_t)r;
  return (uint8_t)((9797 * r + 19234 * g + 3737 * b) >> 15);
}

bool decode_png(const uint8_t *raw, size_t n_raw, bool color, Image *im, std::string *err) {
  size_t p = 8;
  int bit_depth = 0, ctype = 0, interlace = 0, w = 0, h = 0;
  std::vector<uint8_t> idat, plte;
  bool have_hdr = false;
  while (p + 12 <= n_raw) {
    const uint32_t len = be32(raw + p);
    const char *type = reinterpret_cast<const char *>(raw + p + 4);
    if ((size_t)len > n_raw - p - 12) {
      *err = "PNG: truncated chunk";
      return false;
    }
    const uint8_t *data = raw + p + 8;
    if (!memcmp(type, "IHDR", 4) && len >= 13) {
      w = (int)be32(data);
      h = (int)be32(data + 4);
      bit_depth = data[8];
      ctype = data[9];
      interlace = data[12];
      have_hdr = true;
    } else if (!memcmp(type, "PLTE", 4)) {
      plte.assign(data, data + len);
    } else if (!memcmp(type, "IDAT", 4)) {
      idat.insert(idat.end(), data, data + len);
    } else if (!memcmp(type, "IEND", 4)) {
      break;
    }
    p += 12 + (size_t)len;
  }
  if (!have_hdr || w <= 0 || h <= 0 || w > 65535 || h > 65535) {
    *err = "PNG: bad header";
    return false;
  }
  if (interlace != 0) {
    *err = "PNG: interlaced files are not supported";
    return false;
  }
  const int sch = ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : ctype == 6 ? 4 : 0;
  const bool depth_ok = bit_depth == 8 || (bit_depth == 16 && ctype != 3) ||
                        ((bit_depth == 1 || bit_depth == 2 || bit_depth == 4) && (ctype == 0 || ctype == 3));
  if (!sch || !depth_ok) {
    *err = "PNG: unsupported colour type / bit depth";
    return false;
  }
  const size_t row_bytes = ((size_t)w * sch * bit_depth + 7) / 8;  // one filtered scanline
  const size_t fbpp = std::max<size_t>(1, (size_t)sch * bit_depth / 8);
  std::vector<uint8_t> buf((row_bytes + 1) * (size_t)h);
  uLongf out_len = buf.size();
  if (uncompress(buf.data(), &out_len, idat.data(), idat.size()) != Z_OK || out_len != buf.size()) {
    *err = "PNG: image data does not inflate to width x height";
    return false;
  }
  std::vector<uint8_t> lines(row_bytes * (size_t)h);
  for (int y = 0; y < h; ++y) {  // undo the scanline filters
    const uint8_t ft = buf[(row_bytes + 1) * y];
    const uint8_t *src = &buf[(row_bytes + 1) * y + 1];
    uint8_t *dst = &lines[row_bytes * y];
    const uint8_t *up = y ? &lines[row_bytes * (y - 1)] : nullptr;
    for (size_t x = 0; x < row_bytes; ++x) {
      const int a = x >= fbpp ? dst[x - fbpp] : 0, b = up ? up[x] : 0, c = (up && x >= fbpp) ? up[x - fbpp] : 0;
      int pred = 0;
      switch (ft) {
        case 0: pred = 0; break;
        case 1: pred = a; break;
        case 2: pred = b; break;
        case 3: pred = (a + b) >> 1; break;
        case 4: {
          const int pa = std::abs(b - c), pb = std::abs(a - c), pc = std::abs(a + b - 2 * c);
          pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
        } break;
        default: *err = "PNG: bad filter type"; return false;
      }
      dst[x] = (uint8_t)(src[x] + pred);
    }
  }
  // 8 bits per sample: png_set_strip_16 keeps the high byte, png_set_expand_gray_1_2_4_to_8 scales to 0..255,
  // palette indices stay indices
  const size_t stride = (size_t)w * sch;
  std::vector<uint8_t> img(stride * (size_t)h);
  for (int y = 0; y < h; ++y) {
    const uint8_t *src = &lines[row_bytes * y];
    uint8_t *dst = &img[stride * y];
    if (bit_depth == 8) {
      memcpy(dst, src, stride);
    } else if (bit_depth == 16) {
      for (size_t x = 0; x < stride; ++x) dst[x] = src[2 * x];
    } else {
      const int mask = (1 << bit_depth) - 1, scale = ctype == 0 ? 255 / mask : 1;
      for (int x = 0; x < w; ++x) {
        const int bit = x * bit_depth, v = (src[bit >> 3] >> (8 - bit_depth - (bit & 7))) & mask;
        dst[x] = (uint8_t)(v * scale);
      }
    }
  }
  const size_t n = (size_t)w * h;
  im->w = w;
  im->h = h;
  im->ch = color ? 3 : 1;
  im->px.resize(n * im->ch);
  for (size_t i = 0; i < n; ++i) {
    const uint8_t *px = &img[i * sch];
    int r, g, b;
    if (ctype == 0 || ctype == 4) {
      r = g = b = px[0];
    } else if (ctype == 3) {
      if ((size_t)px[0] * 3 + 2 >= plte.size()) {
        *err = "PNG: palette index out of range";
        return false;
      }
      r = plte[px[0] * 3], g = plte[px[0] * 3 + 1], b = plte[px[0] * 3 + 2];
    } else {
      r = px[0], g = px[1], b = px[2];
    }
    if (color) {
      im->px[3 * i] = (uint8_t)b;  // imread(IMREAD_COLOR) order
      im->px[3 * i + 1] = (uint8_t)g;
      im->px[3 * i + 2] = (uint8_t)r;
    } else {
      im->px[i] = png_rgb_to_gray(r, g, b);
    }
  }
  return true;
}

// ---------------------------------------------------------------------------------------------------------
// JPEG
// ---------------------------------------------------------------------------------------------------------
// jidctint.c jpeg_idct_islow on one dequantised block -> 8x8 samples
void idct_islow(const int16_t *in, const uint16_t *q, uint8_t *out, int out_stride) {
  constexpr int CB = 13, P1 = 2;
  constexpr long F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633,
                 F1_501 = 12299, F1_847 = 15137, F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;
  auto descale = [](long x, int n) { return (x + (1L << (n - 1))) >> n; };
  int ws[64];
  for (int c = 0; c < 8; ++c) {  // pass 1: columns
    if ((in[8 + c] | in[16 + c] | in[24 + c] | in[32 + c] | in[40 + c] | in[48 + c] | in[56 + c]) == 0) {
      // a column with only its DC term: the arithmetic below reduces to dc << PASS1_BITS in every row
      const int dcv = (int)((long)in[c] * (long)q[c] * (1L << P1));
      for (int r = 0; r < 8; ++r) ws[8 * r + c] = dcv;
      continue;
    }
    long d[8];
    for (int r = 0; r < 8; ++r) d[r] = (long)in[8 * r + c] * (long)q[8 * r + c];
    long z2 = d[2], z3 = d[6];
    long z1 = (z2 + z3) * F0_541;
    long tmp2 = z1 + z3 * (-F1_847);
    long tmp3 = z1 + z2 * F0_765;
    z2 = d[0];
    z3 = d[4];
    long tmp0 = (z2 + z3) * (1L << CB);
    long tmp1 = (z2 - z3) * (1L << CB);
    const long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = d[7];
    tmp1 = d[5];
    tmp2 = d[3];
    tmp3 = d[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    long z4 = tmp1 + tmp3;
    const long z5 = (z3 + z4) * F1_175;
    tmp0 *= F0_298;
    tmp1 *= F2_053;
    tmp2 *= F3_072;
    tmp3 *= F1_501;
    z1 *= -F0_899;
    z2 *= -F2_562;
    z3 *= -F1_961;
    z4 *= -F0_390;
    z3 += z5;
    z4 += z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    ws[8 * 0 + c] = (int)descale(tmp10 + tmp3, CB - P1);
    ws[8 * 7 + c] = (int)descale(tmp10 - tmp3, CB - P1);
    ws[8 * 1 + c] = (int)descale(tmp11 + tmp2, CB - P1);
    ws[8 * 6 + c] = (int)descale(tmp11 - tmp2, CB - P1);
    ws[8 * 2 + c] = (int)descale(tmp12 + tmp1, CB - P1);
    ws[8 * 5 + c] = (int)descale(tmp12 - tmp1, CB - P1);
    ws[8 * 3 + c] = (int)descale(tmp13 + tmp0, CB - P1);
    ws[8 * 4 + c] = (int)descale(tmp13 - tmp0, CB - P1);
  }
  // the post-IDCT range-limit table (jdmaster.c prepare_range_limit_table), indexed with 10 bits
  auto limit = [](long v) -> uint8_t {
    const int i = (int)(v & 1023);
    return i < 128 ? (uint8_t)(128 + i) : i < 512 ? 255 : i < 896 ? 0 : (uint8_t)(i - 896);
  };
  for (int r = 0; r < 8; ++r) {  // pass 2: rows
    const int *w = ws + 8 * r;
    uint8_t *o = out + (size_t)r * out_stride;
    if ((w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) == 0) {  // same value as the full computation
      const uint8_t v = limit(descale((long)w[0], P1 + 3));
      for (int x = 0; x < 8; ++x) o[x] = v;
      continue;
    }
    long z2 = w[2], z3 = w[6];
    long z1 = (z2 + z3) * F0_541;
    long tmp2 = z1 + z3 * (-F1_847);
    long tmp3 = z1 + z2 * F0_765;
    long tmp0 = ((long)w[0] + (long)w[4]) * (1L << CB);
    long tmp1 = ((long)w[0] - (long)w[4]) * (1L << CB);
    const long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = w[7];
    tmp1 = w[5];
    tmp2 = w[3];
    tmp3 = w[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    long z4 = tmp1 + tmp3;
    const long z5 = (z3 + z4) * F1_175;
    tmp0 *= F0_298;
    tmp1 *= F2_053;
    tmp2 *= F3_072;
    tmp3 *= F1_501;
    z1 *= -F0_899;
    z2 *= -F2_562;
    z3 *= -F1_961;
    z4 *= -F0_390;
    z3 += z5;
    z4 += z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    constexpr int SH = CB + P1 + 3;
    o[0] = limit(descale(tmp10 + tmp3, SH));
    o[7] = limit(descale(tmp10 - tmp3, SH));
    o[1] = limit(descale(tmp11 + tmp2, SH));
    o[6] = limit(descale(tmp11 - tmp2, SH));
    o[2] = limit(descale(tmp12 + tmp1, SH));
    o[5] = limit(descale(tmp12 - tmp1, SH));
    o[3] = limit(descale(tmp13 + tmp0, SH));
    o[4] = limit(descale(tmp13 - tmp0, SH));
  }
}

struct Jpeg : JpegEntropy {
  void reconstruct(int n_planes) {
    for (int i = 0; i < n_planes; ++i) {
      JpegComponent &c = comp[i];
      const uint16_t *q = quant[c.tq];
      const int stride = c.bw * 8;
      c.plane.resize((size_t)stride * c.bh * 8);
      for (int by = 0; by < c.bh; ++by)
        for (int bx = 0; bx < c.bw; ++bx)
          idct_islow(&c.coef[((size_t)by * c.bw + bx) * 64], q, &c.plane[(size_t)by * 8 * stride + bx * 8], stride);
    }
  }

  // jdsample.c: one output row `y` (full resolution) of component c, `out` has room for 2*rw+2 samples
  void upsample_row(const JpegComponent &c, int y, uint8_t *out) const {
    const int stride = c.bw * 8;
    const int hx = hmax / c.hs, vx = vmax / c.vs;
    if (hx == 1 && vx == 1) {
      memcpy(out, &c.plane[(size_t)y * stride], (size_t)w);
      return;
    }
    const int n = c.rw;
    if (n <= 2) {  // jdsample.c jinit_upsampler: the triangle filters need downsampled_width > 2, else replication
      const uint8_t *in = &c.plane[(size_t)(vx == 2 ? y >> 1 : y) * stride];
      for (int x = 0; x < 2 * n; ++x) out[x] = in[x >> 1];
      return;
    }
    if (hx == 2 && vx == 1) {  // h2v1_fancy_upsample
      const uint8_t *in = &c.plane[(size_t)y * stride];
      out[0] = in[0];
      out[1] = (uint8_t)((in[0] * 3 + in[1] + 2) >> 2);
      for (int i = 1; i < n - 1; ++i) {
        const int v = in[i] * 3;
        out[2 * i] = (uint8_t)((v + in[i - 1] + 1) >> 2);
        out[2 * i + 1] = (uint8_t)((v + in[i + 1] + 2) >> 2);
      }
      out[2 * n - 2] = (uint8_t)((in[n - 1] * 3 + in[n - 2] + 1) >> 2);
      out[2 * n - 1] = in[n - 1];
      return;
    }
    // h2v2_fancy_upsample: the nearer input row counts 3/4, the farther 1/4; rows beyond the image replicate the edge
    const int r0 = y >> 1;
    int r1 = (y & 1) ? r0 + 1 : r0 - 1;
    r1 = std::max(0, std::min(c.rh - 1, r1));
    const uint8_t *in0 = &c.plane[(size_t)r0 * stride], *in1 = &c.plane[(size_t)r1 * stride];
    int thiscol = in0[0] * 3 + in1[0], nextcol = in0[1] * 3 + in1[1], lastcol;
    out[0] = (uint8_t)((thiscol * 4 + 8) >> 4);
    out[1] = (uint8_t)((thiscol * 3 + nextcol + 7) >> 4);
    lastcol = thiscol;
    thiscol = nextcol;
    for (int i = 1; i < n - 1; ++i) {
      nextcol = in0[i + 1] * 3 + in1[i + 1];
      out[2 * i] = (uint8_t)((thiscol * 3 + lastcol + 8) >> 4);
      out[2 * i + 1] = (uint8_t)((thiscol * 3 + nextcol + 7) >> 4);
      lastcol = thiscol;
      thiscol = nextcol;
    }
    out[2 * n - 2] = (uint8_t)((thiscol * 3 + lastcol + 8) >> 4);
    out[2 * n - 1] = (uint8_t)((thiscol * 4 + 7) >> 4);
  }

  bool to_image(bool color, Image *im) {
    // jdapimin.c default_decompress_parms: the file's colour space
    const bool ycc = is_ycc();
    im->w = w;
    im->h = h;
    im->ch = color ? 3 : 1;
    im->px.resize((size_t)w * h * im->ch);
    const bool y_only = ncomp == 1 || (!color && ycc);
    reconstruct(y_only ? 1 : ncomp);
    if (y_only) {  // JCS_GRAYSCALE out of a gray or YCbCr file is the first plane (jdcolor.c grayscale_convert)
      const int stride = comp[0].bw * 8;
      for (int y = 0; y < h; ++y) {
        const uint8_t *src = &comp[0].plane[(size_t)y * stride];
        uint8_t *dst = &im->px[(size_t)y * w * im->ch];
        if (!color) memcpy(dst, src, (size_t)w);
        else
          for (int x = 0; x < w; ++x) dst[3 * x] = dst[3 * x + 1] = dst[3 * x + 2] = src[x];
      }
      return true;
    }
    // jdcolor.c build_ycc_rgb_table
    struct YccTables {
      int cr_r[256], cb_b[256];
      long cr_g[256], cb_g[256];
      YccTables() {
        for (int i = 0; i < 256; ++i) {
          const long x = i - 128;
          cr_r[i] = (int)((91881L * x + 32768L) >> 16);
          cb_b[i] = (int)((116130L * x + 32768L) >> 16);
          cr_g[i] = -46802L * x;
          cb_g[i] = -22554L * x + 32768L;
        }
      }
    };
    static const YccTables ycc_tab;  // built once, safely, whichever thread decodes first (server workers decode concurrently)
    const int *const cr_r = ycc_tab.cr_r, *const cb_b = ycc_tab.cb_b;
    const long *const cr_g = ycc_tab.cr_g, *const cb_g = ycc_tab.cb_g;
    auto clamp = [](int v) -> uint8_t { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); };
    std::vector<uint8_t> rows[3];
    for (int i = 0; i < 3; ++i) rows[i].resize((size_t)2 * comp[i].bw * 8 + 16);
    for (int y = 0; y < h; ++y) {
      for (int i = 0; i < 3; ++i) upsample_row(comp[i], y, rows[i].data());
      uint8_t *dst = &im->px[(size_t)y * w * im->ch];
      for (int x = 0; x < w; ++x) {
        const int a = rows[0][x], b = rows[1][x], c = rows[2][x];
        int R, G, B;
        if (ycc) {
          R = clamp(a + cr_r[c]);
          G = clamp(a + (int)((cb_g[b] + cr_g[c]) >> 16));
          B = clamp(a + cb_b[b]);
        } else {
          R = a, G = b, B = c;
        }
        if (color) {
          dst[3 * x] = (uint8_t)B;
          dst[3 * x + 1] = (uint8_t)G;
          dst[3 * x + 2] = (uint8_t)R;
        } else {  // jdcolor.c rgb_gray_convert
          dst[x] = (uint8_t)((19595L * R + 38470L * G + 7471L * B + 32768L) >> 16);
        }
      }
    }
    return true;
  }
};

bool decode_any(const uint8_t *raw, size_t n, bool color, bool size_only, Image *im, std::string *err) {
  static const uint8_t png_sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  if (n >= 33 && !memcmp(raw, png_sig, 8)) {
    if (size_only && !memcmp(raw + 12, "IHDR", 4)) {
      im->w = (int)be32(raw + 16);
      im->h = (int)be32(raw + 20);
      if (im->w > 0 && im->h > 0 && im->w <= 65535 && im->h <= 65535) return true;
    }
    return decode_png(raw, n, color, im, err);
  }
  if (n >= 4 && raw[0] == 0xFF && raw[1] == 0xD8) {
    Jpeg j;
    if (size_only) {
      if (!j.parse(raw, n, true)) {
        *err = j.err;
        return false;
      }
      im->w = j.w;
      im->h = j.h;
      return true;
    }
    if (!j.parse(raw, n, false) || !j.to_image(color, im)) {
      *err = j.err;
      return false;
    }
    return true;
  }
  if (n >= 8 && raw[0] == 'P' && (raw[1] == '5' || raw[1] == '6')) return decode_pnm(raw, n, color, im, err);
  *err = "not a JPEG, PNG or binary PGM/PPM image";
  return false;
}

}  // namespace

// (jpeg_host.h) the two halves of a JPEG decode with the coefficients in the caller's memory between them
bool jpeg_decode_split_host(const uint8_t *raw, size_t n, bool color, int16_t *coef_mem, size_t coef_cap, int *w, int *h,
                            std::vector<uint8_t> *px, std::string *err) {
  Jpeg j;
  j.coef_mem = coef_mem;
  j.coef_cap = coef_cap;
  Image im;
  if (!j.parse(raw, n, false) || !j.to_image(color, &im)) {
    *err = j.err;
    return false;
  }
  *w = im.w;
  *h = im.h;
  px->swap(im.px);
  return true;
}

bool image_decode_host(const uint8_t *raw, size_t n, bool color, int *w, int *h, std::vector<uint8_t> *px, std::string *err) {
  Image im;
  if (!decode_any(raw, n, color, false, &im, err)) return false;
  *w = im.w;
  *h = im.h;
  px->swap(im.px);
  return true;
}

}  // namespace sfmloc

using namespace sfmloc;

extern "C" int sfmloc_image_decode(const uint8_t *bytes, uint64_t n_bytes, int32_t color, uint8_t *out, uint64_t cap,
                                   int32_t *width, int32_t *height) {
  SFM_CHECK(bytes && width && height, SFMLOC_EINVAL, "sfmloc_image_decode: null argument");
  Image im;
  std::string err;
  try {
    if (!decode_any(bytes, (size_t)n_bytes, color != 0, out == nullptr, &im, &err)) {
      set_error("sfmloc_image_decode: %s", err.c_str());
      return SFMLOC_EIO;
    }
  } catch (const std::bad_alloc &) {
    set_error("sfmloc_image_decode: out of host memory");
    return SFMLOC_ENOMEM;
  }
  *width = im.w;
  *height = im.h;
  if (!out) return SFMLOC_OK;  // size query
  SFM_CHECK(cap >= im.px.size(), SFMLOC_ECAP, "sfmloc_image_decode: buffer holds %llu bytes, the image needs %llu",
            (unsigned long long)cap, (unsigned long long)im.px.size());
  memcpy(out, im.px.data(), im.px.size());
  return SFMLOC_OK;
}

extern "C" int sfmloc_image_read(const char *path, int32_t color, uint8_t *out, uint64_t cap, int32_t *width,
                                 int32_t *height) {
  SFM_CHECK(path && width && height, SFMLOC_EINVAL, "sfmloc_image_read: null argument");
  FILE *f = fopen(path, "rb");
  SFM_CHECK(f != nullptr, SFMLOC_EIO, "sfmloc_image_read: cannot open %s", path);
  std::vector<uint8_t> raw;
  uint8_t buf[65536];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) raw.insert(raw.end(), buf, buf + got);
  fclose(f);
  return sfmloc_image_decode(raw.data(), raw.size(), color, out, cap, width, height);
}
