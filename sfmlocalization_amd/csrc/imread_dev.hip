// cv::imread whose pixels are born on the device: sfmloc_imread_* of include/sfmloc.h.
//
// A JPEG's header parsing and entropy stage run on the host (jpeg_host.h, the code sfmloc_image_decode runs) with the
// coefficient blocks landing in a pinned staging buffer; ONE upload carries a small header (quantisation tables, the
// components' block table, the colour decision) and the dense int16 blocks; two kernels reconstruct:
//   k_idct        dequantisation + jidctint.c jpeg_idct_islow + the 10-bit range limit -> the padded component planes
//   k_upsample    jdsample.c h2v1 / h2v2 fancy upsampling (or replication), jdcolor.c YCbCr -> RGB, and the up to three
//                 images a decode leaves resident: GRAY = imread(IMREAD_GRAYSCALE), BGR = imread(IMREAD_COLOR),
//                 BGR2GRAY = cvtColor(BGR, COLOR_BGR2GRAY)
// All arithmetic is integer and restates image_io.hip's host path statement by statement, which tests/test_image_io.py
// pins against libjpeg-turbo: every pixel equals sfmloc_image_decode's (tests/test_gpu_imread.py).  The IDCT computes in
// 64 bits as the host does (`long`): a 16-bit quantisation table times a large coefficient leaves 32 bits.
// PNG and PGM / PPM files are decoded on the host as sfmloc_image_decode does and uploaded.
//
// Nothing is allocated per JPEG call; a call queues its work on the reader's stream and returns -- the only host wait is
// for the PREVIOUS call's upload to have left the staging buffer before the entropy stage overwrites it.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <ctime>
#include <string>
#include <vector>

#include "jpeg_host.h"
#include "sfmloc_internal.h"

namespace sfmloc {
namespace {

constexpr uint32_t kGray = SFMLOC_IMREAD_GRAY, kBgr = SFMLOC_IMREAD_BGR, kBgr2Gray = SFMLOC_IMREAD_BGR2GRAY;
constexpr uint32_t kAllImages = kGray | kBgr | kBgr2Gray;

// what the kernels know about the frame: the head of the staging buffer, uploaded with the blocks
struct ImreadComp {
  int32_t blk0;       // first block of the component in the dense block array
  int32_t bw, bh;     // blocks per row / rows of blocks (whole MCUs)
  int32_t rw, rh;     // real samples
  int32_t tq;         // quantisation table
  int32_t hx, vx;     // upsampling factors to the full resolution (1 or 2)
  uint32_t plane_off; // where its padded plane (bw*8) x (bh*8) starts in d_plane
  int32_t pad[3];
};
struct ImreadHdr {
  uint16_t quant[4][64];
  int32_t w, h, ncomp, ycc;
  int32_t n_idct_comp;  // components the IDCT launch covers (1: the Y plane alone)
  int32_t n_blocks;     // blocks of those components
  uint32_t want;
  int32_t pad;
  ImreadComp c[3];
};
constexpr size_t kHdrBytes = 1024;  // the blocks start here in the staging buffer and in its device copy
static_assert(sizeof(ImreadHdr) <= kHdrBytes, "header larger than its slot");

constexpr int kIdctBlocksPerGroup = 32;  // 8 lanes per 8x8 block, 256 threads
constexpr int kWsStride = 72;            // ints per block in LDS: 64 + 8, so that four blocks' rows fall on distinct banks

// jidctint.c jpeg_idct_islow, one pass over eight values (a column of dequantised coefficients, or a row of the
// workspace): the even and odd parts exactly as image_io.hip's idct_islow writes them, in 64 bits
__device__ __forceinline__ void islow_pass(const long long d[8], long long o[8]) {
  constexpr int CB = 13;
  constexpr long long F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633,
                      F1_501 = 12299, F1_847 = 15137, F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;
  long long z2 = d[2], z3 = d[6];
  long long z1 = (z2 + z3) * F0_541;
  long long tmp2 = z1 + z3 * (-F1_847);
  long long tmp3 = z1 + z2 * F0_765;
  long long tmp0 = (d[0] + d[4]) * (1LL << CB);
  long long tmp1 = (d[0] - d[4]) * (1LL << CB);
  const long long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = d[7];
  tmp1 = d[5];
  tmp2 = d[3];
  tmp3 = d[1];
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  long long z4 = tmp1 + tmp3;
  const long long z5 = (z3 + z4) * F1_175;
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
  o[0] = tmp10 + tmp3;
  o[7] = tmp10 - tmp3;
  o[1] = tmp11 + tmp2;
  o[6] = tmp11 - tmp2;
  o[2] = tmp12 + tmp1;
  o[5] = tmp12 - tmp1;
  o[3] = tmp13 + tmp0;
  o[4] = tmp13 - tmp0;
}

__device__ __forceinline__ long long descale(long long x, int n) { return (x + (1LL << (n - 1))) >> n; }

// the post-IDCT range-limit table (jdmaster.c prepare_range_limit_table), indexed with 10 bits
__device__ __forceinline__ uint32_t range_limit(long long v) {
  const int i = (int)(v & 1023);
  return i < 128 ? (uint32_t)(128 + i) : i < 512 ? 255u : i < 896 ? 0u : (uint32_t)(i - 896);
}

// Eight lanes per block: lane j takes column j in pass 1 and row j in pass 2, the 8x8 workspace goes through LDS.
// The host's zero-AC shortcuts are left out: they give the value of the full computation (image_io.hip).
__global__ __launch_bounds__(256) void k_idct(const ImreadHdr *__restrict__ H, const int16_t *__restrict__ coef,
                                              uint8_t *__restrict__ planes) {
  __shared__ int ws[kIdctBlocksPerGroup * kWsStride];
  const int j = threadIdx.x & 7, slot = threadIdx.x >> 3;
  const int blk = blockIdx.x * kIdctBlocksPerGroup + slot;
  const bool live = blk < H->n_blocks;
  int ci = 0;
  if (live) {
    if (H->n_idct_comp > 1 && blk >= H->c[1].blk0) ci = 1;
    if (H->n_idct_comp > 2 && blk >= H->c[2].blk0) ci = 2;
  }
  const ImreadComp C = H->c[ci];
  int *w = ws + slot * kWsStride;
  if (live) {  // pass 1: column j
    const int16_t *in = coef + (size_t)blk * 64;
    const uint16_t *q = H->quant[C.tq];
    long long d[8], o[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) d[r] = (long long)in[8 * r + j] * (long long)q[8 * r + j];
    islow_pass(d, o);
#pragma unroll
    for (int r = 0; r < 8; ++r) w[8 * r + j] = (int)descale(o[r], 13 - 2);  // (narrowed to int as the host's workspace is)
  }
  __syncthreads();
  if (live) {  // pass 2: row j
    long long d[8], o[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) d[x] = (long long)w[8 * j + x];
    islow_pass(d, o);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      lo |= range_limit(descale(o[x], 13 + 2 + 3)) << (8 * x);
      hi |= range_limit(descale(o[x + 4], 13 + 2 + 3)) << (8 * x);
    }
    const int b = blk - C.blk0, by = b / C.bw, bx = b - by * C.bw;
    const size_t stride = (size_t)C.bw * 8;
    // (8-byte aligned: plane_off and stride are multiples of 8)
    *reinterpret_cast<uint2 *>(planes + C.plane_off + ((size_t)by * 8 + j) * stride + (size_t)bx * 8) = make_uint2(lo, hi);
  }
}

// jdsample.c: the sample of component C at full-resolution pixel (x, y) -- image_io.hip's upsample_row, per pixel
__device__ __forceinline__ int upsampled(const ImreadComp &C, const uint8_t *__restrict__ planes, int x, int y) {
  const uint8_t *P = planes + C.plane_off;
  const size_t stride = (size_t)C.bw * 8;
  if (C.hx == 1 && C.vx == 1) return P[(size_t)y * stride + x];
  const int n = C.rw, i = x >> 1;
  if (n <= 2) return P[(size_t)(C.vx == 2 ? y >> 1 : y) * stride + i];  // replication: the triangle filters need width > 2
  if (C.vx == 1) {  // h2v1_fancy_upsample
    const uint8_t *in = P + (size_t)y * stride;
    if (x & 1) return i == n - 1 ? in[i] : (in[i] * 3 + in[i + 1] + 2) >> 2;
    return i == 0 ? in[0] : (in[i] * 3 + in[i - 1] + 1) >> 2;
  }
  // h2v2_fancy_upsample: the nearer input row counts 3/4, the farther 1/4; rows beyond the image replicate the edge
  const int r0 = y >> 1;
  int r1 = (y & 1) ? r0 + 1 : r0 - 1;
  r1 = r1 < 0 ? 0 : (r1 > C.rh - 1 ? C.rh - 1 : r1);
  const uint8_t *in0 = P + (size_t)r0 * stride, *in1 = P + (size_t)r1 * stride;
  const int thiscol = in0[i] * 3 + in1[i];
  if (x & 1) return i == n - 1 ? (thiscol * 4 + 7) >> 4 : (thiscol * 3 + (in0[i + 1] * 3 + in1[i + 1]) + 7) >> 4;
  return i == 0 ? (thiscol * 4 + 8) >> 4 : (thiscol * 3 + (in0[i - 1] * 3 + in1[i - 1]) + 8) >> 4;
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// one thread per output pixel: image_io.hip's to_image for every image asked for
__global__ __launch_bounds__(256) void k_upsample_color(const ImreadHdr *__restrict__ H, const uint8_t *__restrict__ planes,
                                                       uint8_t *__restrict__ gray, uint8_t *__restrict__ bgr,
                                                       uint8_t *__restrict__ bgr2gray) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  const int w = H->w, h = H->h;
  if (x >= w || y >= h) return;
  const uint32_t want = H->want;
  const bool ycc = H->ycc != 0, three = H->ncomp == 3;
  const int a = upsampled(H->c[0], planes, x, y);
  int R = a, G = a, B = a;
  // (a gray file, or the Y plane alone of a YCbCr file: jdcolor.c grayscale_convert)
  const bool need_rgb = three && ((want & (kBgr | kBgr2Gray)) || !ycc);
  if (need_rgb) {
    const int b = upsampled(H->c[1], planes, x, y), c = upsampled(H->c[2], planes, x, y);
    if (ycc) {  // jdcolor.c build_ycc_rgb_table, as arithmetic
      R = clamp255(a + ((91881 * (c - 128) + 32768) >> 16));
      G = clamp255(a + ((-22554 * (b - 128) + 32768 + -46802 * (c - 128)) >> 16));
      B = clamp255(a + ((116130 * (b - 128) + 32768) >> 16));
    } else {
      R = a, G = b, B = c;
    }
  }
  const size_t p = (size_t)y * w + x;
  if (want & kGray)  // jdcolor.c rgb_gray_convert for an RGB file, the first plane otherwise
    gray[p] = (uint8_t)((three && !ycc) ? (19595 * R + 38470 * G + 7471 * B + 32768) >> 16 : a);
  if (want & kBgr) {
    bgr[3 * p] = (uint8_t)B;
    bgr[3 * p + 1] = (uint8_t)G;
    bgr[3 * p + 2] = (uint8_t)R;
  }
  if (want & kBgr2Gray) bgr2gray[p] = (uint8_t)((R * 4899 + G * 9617 + B * 1868 + 8192) >> 14);
}

}  // namespace

constexpr int kImreadConsumers = 4;

struct Imread {
  int device = 0;
  uint32_t max_w = 0, max_h = 0;
  Stream own_stream;  // before the buffers (devmem.h, order of destruction)
  hipStream_t stream = nullptr;  // where work is queued: its own, or a context's (sfmloc_imread_share_stream)
  size_t cap_coef = 0;           // int16 the staging buffer holds after its header
  HostBuf<uint8_t> h_stage;      // pinned: ImreadHdr in kHdrBytes, then the dense blocks (or a host-decoded image)
  DevBuf<uint8_t> d_stage;       // its device copy
  DevBuf<uint8_t> d_plane;       // the components' padded planes, one after the other
  DevBuf<uint8_t> d_gray, d_bgr, d_bgr2gray;
  Event staged;                  // the last upload has left h_stage
  Event done;                    // the last decode's images are complete
  Event consumed[kImreadConsumers];  // consumers on other streams have read the images (imread_consumed)
  int n_consumed = 0;
  bool staged_pending = false;
  int w = 0, h = 0;
  uint32_t have = 0;             // the images of the last decode
  // timing of the last JPEG decode, when asked for (sfmloc_imread_timing)
  bool timing = false;
  Event t0, t1, t2, t3;
  double host_parse_ms = 0.0;
  bool timed = false;
};

namespace {

size_t round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }

double now_ms() {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec * 1e3 + 1e-6 * (double)ts.tv_nsec;
}

uint8_t *image_of(const Imread *r, uint32_t which) {
  return which == kGray ? r->d_gray.get() : which == kBgr ? r->d_bgr.get() : which == kBgr2Gray ? r->d_bgr2gray.get() : nullptr;
}

// the reader's next writes wait for the consumers that read its images on other streams
int wait_for_consumers(Imread *r) {
  for (int i = 0; i < r->n_consumed; ++i) SFM_HIP(hipStreamWaitEvent(r->stream, r->consumed[i], 0));
  r->n_consumed = 0;
  return SFMLOC_OK;
}

// PNG / PNM: decoded on the host as sfmloc_image_decode does, staged and uploaded
int decode_other(Imread *r, const uint8_t *bytes, size_t n, uint32_t want, int32_t *w, int32_t *h) {
  std::vector<uint8_t> gray, bgr;
  std::string err;
  int iw = 0, ih = 0;
  try {
    if ((want & kGray) && !image_decode_host(bytes, n, false, &iw, &ih, &gray, &err)) {
      set_error("sfmloc_imread_decode: %s", err.c_str());
      return SFMLOC_EIO;
    }
    if ((want & (kBgr | kBgr2Gray)) && !image_decode_host(bytes, n, true, &iw, &ih, &bgr, &err)) {
      set_error("sfmloc_imread_decode: %s", err.c_str());
      return SFMLOC_EIO;
    }
  } catch (const std::bad_alloc &) {
    set_error("sfmloc_imread_decode: out of host memory");
    return SFMLOC_ENOMEM;
  }
  SFM_CHECK((uint32_t)iw <= r->max_w && (uint32_t)ih <= r->max_h, SFMLOC_ECAP,
            "sfmloc_imread_decode: the frame is %d x %d, the reader was made for %u x %u", iw, ih, r->max_w, r->max_h);
  const size_t np = (size_t)iw * ih;
  if (r->staged_pending) SFM_HIP(hipEventSynchronize(r->staged));
  uint8_t *s_gray = r->h_stage, *s_bgr = s_gray + np, *s_b2g = s_bgr + 3 * np;  // (5 * np <= the staging buffer: create)
  if (want & kGray) memcpy(s_gray, gray.data(), np);
  if (want & (kBgr | kBgr2Gray)) memcpy(s_bgr, bgr.data(), 3 * np);
  if (want & kBgr2Gray)
    for (size_t i = 0; i < np; ++i)
      s_b2g[i] = (uint8_t)((s_bgr[3 * i + 2] * 4899 + s_bgr[3 * i + 1] * 9617 + s_bgr[3 * i] * 1868 + 8192) >> 14);
  SFM_RC(wait_for_consumers(r));
  hipStream_t s = r->stream;
  if (want & kGray) SFM_RC(r->d_gray.upload(s_gray, np, s));
  if (want & kBgr) SFM_RC(r->d_bgr.upload(s_bgr, 3 * np, s));
  if (want & kBgr2Gray) SFM_RC(r->d_bgr2gray.upload(s_b2g, np, s));
  SFM_HIP(hipEventRecord(r->staged, s));
  r->staged_pending = true;
  SFM_HIP(hipEventRecord(r->done, s));
  r->w = iw;
  r->h = ih;
  r->have = want;
  r->timed = false;
  *w = iw;
  *h = ih;
  return SFMLOC_OK;
}

int decode_jpeg(Imread *r, const uint8_t *bytes, size_t n, uint32_t want, int32_t *w, int32_t *h) {
  const double t_host0 = r->timing ? now_ms() : 0.0;
  {  // the size first: a frame the buffers cannot hold is refused before the staging buffer is touched
    JpegEntropy head;
    if (!head.parse(bytes, n, true)) {
      set_error("sfmloc_imread_decode: %s", head.err.c_str());
      return SFMLOC_EIO;
    }
    SFM_CHECK((uint32_t)head.w <= r->max_w && (uint32_t)head.h <= r->max_h, SFMLOC_ECAP,
              "sfmloc_imread_decode: the frame is %d x %d, the reader was made for %u x %u", head.w, head.h, r->max_w, r->max_h);
  }
  if (r->staged_pending) SFM_HIP(hipEventSynchronize(r->staged));
  r->staged_pending = false;
  JpegEntropy j;
  j.coef_mem = reinterpret_cast<int16_t *>(r->h_stage + kHdrBytes);
  j.coef_cap = r->cap_coef;
  if (!j.parse(bytes, n, false)) {  // (nothing has been queued: the previous images stand)
    set_error("sfmloc_imread_decode: %s", j.err.c_str());
    return SFMLOC_EIO;
  }
  ImreadHdr *H = reinterpret_cast<ImreadHdr *>(r->h_stage.get());
  memset(H, 0, sizeof(*H));
  memcpy(H->quant, j.quant, sizeof(H->quant));
  H->w = j.w;
  H->h = j.h;
  H->ncomp = j.ncomp;
  H->ycc = j.is_ycc() ? 1 : 0;
  H->want = want;
  // image_io.hip to_image: a gray request of a gray or YCbCr file reconstructs the first plane alone
  const bool y_only = j.ncomp == 1 || (want == kGray && j.is_ycc());
  H->n_idct_comp = y_only ? 1 : j.ncomp;
  int blk = 0;
  uint32_t off = 0;
  for (int i = 0; i < j.ncomp; ++i) {
    const JpegComponent &c = j.comp[i];
    ImreadComp &C = H->c[i];
    C.blk0 = blk;
    C.bw = c.bw;
    C.bh = c.bh;
    C.rw = c.rw;
    C.rh = c.rh;
    C.tq = c.tq;
    C.hx = j.hmax / c.hs;
    C.vx = j.vmax / c.vs;
    C.plane_off = off;
    blk += c.bw * c.bh;
    off += (uint32_t)c.bw * 8u * (uint32_t)c.bh * 8u;
    if (i < H->n_idct_comp) H->n_blocks = blk;
  }
  SFM_CHECK((size_t)off <= r->d_plane.bytes() && (size_t)blk * 64 <= r->cap_coef, SFMLOC_ECAP,
            "sfmloc_imread_decode: the frame's blocks exceed the reader's buffers");
  const double t_host1 = r->timing ? now_ms() : 0.0;
  SFM_RC(wait_for_consumers(r));
  hipStream_t s = r->stream;
  if (r->timing) SFM_HIP(hipEventRecord(r->t0, s));
  const size_t up = kHdrBytes + (size_t)H->n_blocks * 64 * sizeof(int16_t);
  SFM_RC(r->d_stage.upload(r->h_stage.get(), up, s));
  SFM_HIP(hipEventRecord(r->staged, s));
  r->staged_pending = true;
  if (r->timing) SFM_HIP(hipEventRecord(r->t1, s));
  const ImreadHdr *dH = reinterpret_cast<const ImreadHdr *>(r->d_stage.get());
  const int16_t *d_coef = reinterpret_cast<const int16_t *>(r->d_stage.get() + kHdrBytes);
  SFM_RC(dev_launch(k_idct, dim3((H->n_blocks + kIdctBlocksPerGroup - 1) / kIdctBlocksPerGroup), dim3(256), 0, s, dH,
                    d_coef, r->d_plane));
  if (r->timing) SFM_HIP(hipEventRecord(r->t2, s));
  SFM_RC(dev_launch(k_upsample_color, dim3((j.w + 255) / 256, j.h), dim3(256), 0, s, dH, r->d_plane, r->d_gray,
                    r->d_bgr, r->d_bgr2gray));
  if (r->timing) SFM_HIP(hipEventRecord(r->t3, s));
  SFM_HIP(hipEventRecord(r->done, s));
  r->w = j.w;
  r->h = j.h;
  r->have = want;
  r->host_parse_ms = t_host1 - t_host0;
  r->timed = r->timing;
  *w = j.w;
  *h = j.h;
  return SFMLOC_OK;
}

}  // namespace

// for the consumers inside the library (akaze.hip, imgbow.hip): see sfmloc_internal.h
int imread_feed(Imread *r, uint32_t which, int device, uint32_t w, uint32_t h, hipStream_t s, const uint8_t **dev, const char *who) {
  SFM_CHECK(which == kGray || which == kBgr || which == kBgr2Gray, SFMLOC_EINVAL, "%s: `which` names one image (1, 2 or 4), got %u",
            who, which);
  SFM_CHECK(r->have & which, SFMLOC_EINVAL, "%s: the reader's last decode did not leave image %u (it left mask %u)", who, which,
            r->have);
  SFM_CHECK(r->device == device, SFMLOC_EINVAL, "%s: reader and extractor on different devices", who);
  SFM_CHECK((uint32_t)r->w == w && (uint32_t)r->h == h, SFMLOC_EINVAL, "%s: the frame is %d x %d, the extractor was made for %u x %u",
            who, r->w, r->h, w, h);
  if (s != r->stream) SFM_HIP(hipStreamWaitEvent(s, r->done, 0));
  *dev = image_of(r, which);
  return SFMLOC_OK;
}

int imread_consumed(Imread *r, hipStream_t s) {
  if (s == r->stream) return SFMLOC_OK;  // (stream order already)
  if (r->n_consumed == kImreadConsumers) {  // (more readers of one frame than events: wait for this one here)
    SFM_HIP(hipStreamSynchronize(s));
    return SFMLOC_OK;
  }
  SFM_HIP(hipEventRecord(r->consumed[r->n_consumed], s));
  ++r->n_consumed;
  return SFMLOC_OK;
}

}  // namespace sfmloc

using namespace sfmloc;

extern "C" {

int sfmloc_imread_create(int device, uint32_t max_width, uint32_t max_height, sfmloc_imread **out) {
  SFM_CHECK(out, SFMLOC_EINVAL, "sfmloc_imread_create: null argument");
  *out = nullptr;
  SFM_CHECK(max_width >= 1 && max_height >= 1 && max_width <= 16384 && max_height <= 16384, SFMLOC_EINVAL,
            "sfmloc_imread_create: frames of at most %u x %u", max_width, max_height);
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  SFM_CHECK(e == hipSuccess && ndev > 0, SFMLOC_ENODEV, "no HIP device visible; this library has no CPU fallback");
  SFM_HIP(hipSetDevice(device));
  return make_handle<Imread>("sfmloc_imread_create", out, [&](Imread *r) -> int {
    r->device = device;
    r->max_w = max_width;
    r->max_h = max_height;
    // every component has at most 2 * ceil(W / 16) blocks per row and 2 * ceil(H / 16) rows of blocks, in every sampling
    const size_t pw = 2 * ((size_t)(max_width + 15) / 16) * 8, ph = 2 * ((size_t)(max_height + 15) / 16) * 8;
    r->cap_coef = 3 * pw * ph;  // int16: 64 per block of 64 samples
    const size_t stage = kHdrBytes + r->cap_coef * sizeof(int16_t);  // (>= 5 * W * H, what a host-decoded image stages)
    SFM_RC(r->own_stream.create());
    r->stream = r->own_stream;
    SFM_RC(r->h_stage.alloc(stage));
    SFM_RC(r->d_stage.alloc(nullptr, stage));
    SFM_RC(r->d_plane.alloc(nullptr, 3 * pw * ph));
    const size_t np = round_up((size_t)max_width * max_height, 16);
    SFM_RC(r->d_gray.alloc(nullptr, np));
    SFM_RC(r->d_bgr.alloc(nullptr, 3 * np));
    SFM_RC(r->d_bgr2gray.alloc(nullptr, np));
    SFM_RC(r->staged.create(kOrderingEvent));
    SFM_RC(r->done.create(kOrderingEvent));
    for (int i = 0; i < kImreadConsumers; ++i) SFM_RC(r->consumed[i].create(kOrderingEvent));
    return SFMLOC_OK;
  });
}

void sfmloc_imread_destroy(sfmloc_imread *p) {
  Imread *r = reinterpret_cast<Imread *>(p);
  if (!r) return;
  hipSetDevice(r->device);
  if (r->stream) (void)hipStreamSynchronize(r->stream);  // (a context's too)
  delete r;
}

int sfmloc_imread_share_stream(sfmloc_imread *p, sfmloc_context *ctx) {
  SFM_CHECK(p, SFMLOC_EINVAL, "sfmloc_imread_share_stream: null reader");
  Imread *r = reinterpret_cast<Imread *>(p);
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  SFM_CHECK(!c || c->map->device == r->device, SFMLOC_EINVAL, "sfmloc_imread_share_stream: reader and context on different devices");
  SFM_HIP(hipSetDevice(r->device));
  SFM_HIP(hipStreamSynchronize(r->stream));
  r->stream = c ? c->stream.own : r->own_stream.get();
  return SFMLOC_OK;
}

int sfmloc_imread_decode(sfmloc_imread *p, const uint8_t *bytes, uint64_t n, uint32_t want, int32_t *w, int32_t *h) {
  SFM_CHECK(p && bytes && w && h, SFMLOC_EINVAL, "sfmloc_imread_decode: null argument");
  SFM_CHECK(want != 0 && (want & ~kAllImages) == 0, SFMLOC_EINVAL, "sfmloc_imread_decode: `want` is a mask of GRAY 1, BGR 2, BGR2GRAY 4, got %u",
            want);
  Imread *r = reinterpret_cast<Imread *>(p);
  SFM_HIP(hipSetDevice(r->device));
  if (n >= 4 && bytes[0] == 0xFF && bytes[1] == 0xD8) return decode_jpeg(r, bytes, (size_t)n, want, w, h);
  return decode_other(r, bytes, (size_t)n, want, w, h);
}

int sfmloc_imread_file(sfmloc_imread *p, const char *path, uint32_t want, int32_t *w, int32_t *h) {
  SFM_CHECK(p && path && w && h, SFMLOC_EINVAL, "sfmloc_imread_file: null argument");
  FILE *f = fopen(path, "rb");
  SFM_CHECK(f != nullptr, SFMLOC_EIO, "sfmloc_imread_file: cannot open %s", path);
  std::vector<uint8_t> raw;
  try {
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) raw.insert(raw.end(), buf, buf + got);
  } catch (const std::bad_alloc &) {
    fclose(f);
    set_error("sfmloc_imread_file: out of host memory");
    return SFMLOC_ENOMEM;
  }
  fclose(f);
  return sfmloc_imread_decode(p, raw.data(), raw.size(), want, w, h);
}

int sfmloc_imread_read(sfmloc_imread *p, uint32_t which, uint8_t *out, uint64_t cap) {
  SFM_CHECK(p && out, SFMLOC_EINVAL, "sfmloc_imread_read: null argument");
  Imread *r = reinterpret_cast<Imread *>(p);
  const uint8_t *src = image_of(r, which);
  SFM_CHECK(src, SFMLOC_EINVAL, "sfmloc_imread_read: `which` names one image (1, 2 or 4), got %u", which);
  SFM_CHECK(r->have & which, SFMLOC_EINVAL, "sfmloc_imread_read: the reader's last decode did not leave image %u (it left mask %u)",
            which, r->have);
  const size_t nb = (size_t)r->w * r->h * (which == kBgr ? 3 : 1);
  SFM_CHECK(cap >= nb, SFMLOC_ECAP, "sfmloc_imread_read: buffer holds %llu bytes, the image needs %llu", (unsigned long long)cap,
            (unsigned long long)nb);
  SFM_HIP(hipSetDevice(r->device));
  SFM_RC(dev_download(out, src, nb, r->stream));
  SFM_HIP(hipStreamSynchronize(r->stream));
  return SFMLOC_OK;
}

const void *sfmloc_imread_dev(const sfmloc_imread *p, uint32_t which) {
  const Imread *r = reinterpret_cast<const Imread *>(p);
  if (!r || !(r->have & which)) return nullptr;
  return image_of(r, which);
}

int sfmloc_imread_timing(sfmloc_imread *p, int32_t enable, double *out4) {
  SFM_CHECK(p, SFMLOC_EINVAL, "sfmloc_imread_timing: null reader");
  Imread *r = reinterpret_cast<Imread *>(p);
  SFM_HIP(hipSetDevice(r->device));
  if (out4) {
    SFM_CHECK(r->timed, SFMLOC_EINVAL, "sfmloc_imread_timing: no timed JPEG decode yet");
    SFM_HIP(hipEventSynchronize(r->t3));
    float up = 0.f, idct = 0.f, color = 0.f;
    SFM_HIP(hipEventElapsedTime(&up, r->t0, r->t1));
    SFM_HIP(hipEventElapsedTime(&idct, r->t1, r->t2));
    SFM_HIP(hipEventElapsedTime(&color, r->t2, r->t3));
    out4[0] = r->host_parse_ms;
    out4[1] = up;
    out4[2] = idct;
    out4[3] = color;
  }
  if (enable && !r->t0) {
    SFM_RC(r->t0.create(kTimingEvent));
    SFM_RC(r->t1.create(kTimingEvent));
    SFM_RC(r->t2.create(kTimingEvent));
    SFM_RC(r->t3.create(kTimingEvent));
  }
  r->timing = enable != 0;
  return SFMLOC_OK;
}

}  // extern "C"
