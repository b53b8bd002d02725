// Validation metrics on the device: SSIM and the squared error behind PSNR in ONE pass over the two images.
//
// Replaces torchmetrics' StructuralSimilarityIndexMeasure(data_range=1.0, reduction="none") and
// PeakSignalNoiseRatio(data_range=1.0, reduction="none") as /root/reference/trainer.py:46-51 builds them and
// :53-69 feeds them with (1 + G(lr)) / 2 and (1 + hr) / 2.  torchmetrics (pinned 1.4.0, Pipfile) is not a dependency;
// its published algorithm, restated:
//   SSIM : gaussian window 11x11 (size int(3.5 sigma + .5) * 2 + 1), sigma 1.5, k1 .01, k2 .03; the images are
//          reflect-padded by 5, the five moments E[a], E[b], E[aa], E[bb], E[ab] are depthwise convolutions with the
//          window, var = max(E[xx] - E[x]^2, 0), cov = E[ab] - E[a]E[b],
//          ssim = (2 E[a]E[b] + c1)(2 cov + c2) / ((E[a]^2 + E[b]^2 + c1)(var_a + var_b + c2)),
//          and the map is CROPPED by 5 on every side before the per-image mean -- i.e. only windows that lie entirely
//          inside the image count, so the padding never contributes;
//   PSNR : 10 log10(1 / (sum of squared errors / number of elements)) over everything the metric has seen.
// HBM-bound: both images are read once (24 B per pixel of 3 float channels).  The window is separable: a workgroup
// stages a 42x42 patch of one channel of both images in LDS, runs the 11-tap horizontal pass for the five moments into
// LDS, then the vertical pass for its 32x32 output pixels.  Tile sums go to per-workgroup partial slots and are added
// in a fixed order (reduce.hip): bit-reproducible.
//
// The body is a template over a pixel LOADER; the staging loop, the two passes and the epilogue exist once:
//   FloatLoader      fsr_ssim_sse: strided float tensors in [-1, 1], read as (1 + x) / 2, data range 1;
//   U8Loader<true>   fsr_quality_u8, FSR_QUALITY_Y: interleaved RGB bytes -> BT.601 studio luma in code units, data range 255;
//   U8Loader<false>  fsr_quality_u8, FSR_QUALITY_RGB: one of the three byte channels as it is, data range 255.
// The byte loaders are the benchmark protocol of the super-resolution literature (whole images, Y, a shaved border, Wang's SSIM)
// on the frames Generator.forward_u8 produces: 6 B per pixel pair and no float plane in between.
#include "fsr_common.h"
#include "fsr_host.h"

#include <math.h>
#include <stdint.h>

namespace {

constexpr int KW = 11, PADW = 5, TILE = 32, REG = TILE + KW - 1;   // 42
constexpr int RAWW = (3 * REG + 3 + 3) / 4;                       // 33: the dwords a tile row's 126 bytes touch at any alignment

struct GaussTaps {
  float g[KW];
};

// What the shared body needs besides the pixels: the extent (h, w) the windows and the squared error run over, and the tiling.
struct MetricArgs {
  int h, w, tiles_x, tiles_y, channels;
  float* part;                    // [n][channels * tiles][2]  (ssim sum, squared-error sum)
  float c1, c2;
  float shift_mean, shift_eps, shift_var;   // byte loaders only: see U8Loader
  GaussTaps taps;
};

struct FloatLoader {
  static constexpr bool kRaw = false, kShifted = false;
  const float* a;
  const float* b;
  long long asn, asc, ash, asw;   // element strides of a (n, c, h, w)
  long long bsn, bsc, bsh, bsw;
  const float* pa;
  const float* pb;
  __device__ __forceinline__ void begin(int n, int ch, int, int, int, int, unsigned*, int) {
    pa = a + n * asn + ch * asc;
    pb = b + n * bsn + ch * bsc;
  }
  // (va, vb): the values the squared error takes; (sa, sb): the values the windows take -- the same here
  __device__ __forceinline__ void load(int y, int x, int, int, float& va, float& vb, float& sa, float& sb) const {
    va = (1.f + pa[y * ash + x * asw]) * 0.5f;      // trainer.py:63-65
    vb = (1.f + pb[y * bsh + x * bsw]) * 0.5f;
    sa = va;
    sb = vb;
  }
};

// y = 16 + (65.481 r + 128.553 g + 24.966 b) / 255: the quotients as float32 constants, every term positive.
constexpr float Y_R = (float)(65.481 / 255.0), Y_G = (float)(128.553 / 255.0), Y_B = (float)(24.966 / 255.0);

// a, b point at the first pixel of the evaluated region; rows and images are strided in bytes, pixels by 3.
// begin() copies the bytes of the tile's rows, as they lie in memory, into `raw` (LDS the horizontal pass has not written yet:
// 2 x REG rows of RAWW dwords): every whole dword of a row segment with one aligned 4-byte load, its first and last partial
// dword assembled from byte loads of the bytes inside the segment.  No load addresses a byte outside
// [3 x0, 3 min(x0 + REG, w)) of a region row, whatever the row's alignment.
//
// kShifted: in code units the means sit near 128 and var = E[xx] - E[x]^2 would cancel five digits of float32 (E[xx] ~ 2e4 against
// variances of a few hundred: 2e-5 relative per window, 4e-6 on a whole image's SSIM).  The windows therefore take x' = x - 128
// (exact for a byte; for luma -112 + t, one rounding like 16 + t), and the epilogue restores the documented formula EXACTLY, for
// taps whose sum G over the 11 x 11 window is not quite 1 (eps = 1 - G, from the float32 taps in double on the host):
//   E[x] = E[x'] + 128 G,   var = (E[x'x'] - E[x']^2) + eps (256 E[x'] + 128^2 G),   cov likewise with 128 (E[a'] + E[b']).
// The squared error takes the unshifted values.
constexpr float SHIFT = 128.f;
template <bool LUMA>
struct U8Loader {
  static constexpr bool kRaw = true, kShifted = true;
  const unsigned char* a;
  const unsigned char* b;
  long long a_image, a_row, b_image, b_row;
  const unsigned char* ta;        // the tile's first row segment in a and b
  const unsigned char* tb;
  const unsigned char* raw;
  int ch;
  __device__ __forceinline__ void begin(int n, int ch_, int y0, int x0, int h, int w, unsigned* raw_, int tid) {
    ch = ch_;
    raw = (const unsigned char*)raw_;
    ta = a + n * a_image + y0 * a_row + 3 * x0;
    tb = b + n * b_image + y0 * b_row + 3 * x0;
    const int rows = h - y0 < REG ? h - y0 : REG;
    const int len = 3 * (w - x0 < REG ? w - x0 : REG);          // bytes of a row segment, <= 126
    for (int i = tid; i < 2 * REG * RAWW; i += 256) {
      const int img = i / (REG * RAWW), j = i - img * (REG * RAWW);
      const int r = j / RAWW, k = j - r * RAWW;
      if (r >= rows) continue;
      const unsigned char* seg = img ? tb + r * b_row : ta + r * a_row;
      const int lo = 4 * k - (int)((uintptr_t)seg & 3);          // dword k of the row holds the segment's bytes [lo, lo + 4)
      if (lo >= len) continue;
      unsigned v = 0;
      if (lo >= 0 && lo + 4 <= len) {
        v = *(const unsigned*)(seg + lo);                        // 4-byte aligned by construction
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (lo + q >= 0 && lo + q < len) v |= (unsigned)seg[lo + q] << (8 * q);
      }
      raw_[i] = v;
    }
  }
  __device__ __forceinline__ void value(const unsigned char* seg, int slot, int c, float& v, float& s) const {
    const unsigned char* p = raw + slot * (RAWW * 4) + (int)((uintptr_t)seg & 3) + 3 * c;
    if (LUMA) {
      // explicit fused multiply-adds in a fixed order: left to the compiler's contraction, a and b came out with DIFFERENT products
      // fused (fma(g, Y_G, Y_R r) beside fma(r, Y_R, Y_G g)), and identical images had a squared error of 2e-9 instead of 0
      const float t = fmaf(Y_B, (float)p[2], fmaf(Y_G, (float)p[1], Y_R * (float)p[0]));
      v = 16.f + t;
      s = (16.f - SHIFT) + t;
    } else {
      v = (float)p[ch];
      s = v - SHIFT;
    }
  }
  __device__ __forceinline__ void load(int, int, int r, int c, float& va, float& vb, float& sa, float& sb) const {
    value(ta + r * a_row, r, c, va, sa);
    value(tb + r * b_row, REG + r, c, vb, sb);
  }
};

template <class Loader>
__global__ __launch_bounds__(256) void ssim_sse_kernel(const MetricArgs p, Loader ld) {
  __shared__ float A[REG][REG + 1], B[REG][REG + 1];
  __shared__ float Hm[5][REG][TILE + 1];
  __shared__ float red[2][4];
  const int tid = threadIdx.x;
  const int tx = blockIdx.x % p.tiles_x, ty = blockIdx.x / p.tiles_x;
  const int ch = blockIdx.y, n = blockIdx.z;
  const int y0 = ty * TILE, x0 = tx * TILE;
  ld.begin(n, ch, y0, x0, p.h, p.w, (unsigned*)&Hm[0][0][0], tid);
  if (Loader::kRaw) __syncthreads();
  // the last tile row / column also owns the image's last rows / columns for the squared error
  const int own_y1 = (ty == p.tiles_y - 1) ? p.h : (y0 + TILE < p.h ? y0 + TILE : p.h);
  const int own_x1 = (tx == p.tiles_x - 1) ? p.w : (x0 + TILE < p.w ? x0 + TILE : p.w);
  float sse = 0.f;
  for (int i = tid; i < REG * REG; i += 256) {
    const int r = i / REG, c = i - r * REG;
    const int y = y0 + r, x = x0 + c;
    float va = 0.f, vb = 0.f, sa = 0.f, sb = 0.f;
    if (y < p.h && x < p.w) {
      ld.load(y, x, r, c, va, vb, sa, sb);
      if (y < own_y1 && x < own_x1) {
        const float d = va - vb;
        sse += d * d;
      }
    }
    A[r][c] = sa;
    B[r][c] = sb;
  }
  __syncthreads();
  for (int i = tid; i < REG * TILE; i += 256) {
    const int r = i / TILE, c = i - r * TILE;
    float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
    for (int k = 0; k < KW; ++k) {
      const float g = p.taps.g[k], va = A[r][c + k], vb = B[r][c + k];
      m0 += g * va;
      m1 += g * vb;
      m2 += g * (va * va);
      m3 += g * (vb * vb);
      m4 += g * (va * vb);
    }
    Hm[0][r][c] = m0;
    Hm[1][r][c] = m1;
    Hm[2][r][c] = m2;
    Hm[3][r][c] = m3;
    Hm[4][r][c] = m4;
  }
  __syncthreads();
  float ssim = 0.f;
  const int vh = p.h - 2 * PADW, vw = p.w - 2 * PADW;     // windows entirely inside the image
  for (int i = tid; i < TILE * TILE; i += 256) {
    const int r = i / TILE, c = i - r * TILE;
    if (y0 + r < vh && x0 + c < vw) {
      float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < KW; ++k) {
        const float g = p.taps.g[k];
#pragma unroll
        for (int q = 0; q < 5; ++q) m[q] += g * Hm[q][r + k][c];
      }
      float mu_aa = m[0] * m[0], mu_bb = m[1] * m[1], mu_ab = m[0] * m[1];
      float var_a = m[2] - mu_aa, var_b = m[3] - mu_bb, cov = m[4] - mu_ab;
      if (Loader::kShifted) {                  // m[] are moments of x - 128: back to the moments of x (U8Loader)
        var_a += p.shift_eps * (2.f * SHIFT * m[0] + p.shift_var);
        var_b += p.shift_eps * (2.f * SHIFT * m[1] + p.shift_var);
        cov += p.shift_eps * (SHIFT * (m[0] + m[1]) + p.shift_var);
        const float fa = m[0] + p.shift_mean, fb = m[1] + p.shift_mean;
        mu_aa = fa * fa;
        mu_bb = fb * fb;
        mu_ab = fa * fb;
      }
      var_a = fmaxf(var_a, 0.f);
      var_b = fmaxf(var_b, 0.f);
      ssim += ((2.f * mu_ab + p.c1) * (2.f * cov + p.c2)) / ((mu_aa + mu_bb + p.c1) * (var_a + var_b + p.c2));
    }
  }
  ssim = wave_sum(ssim);
  sse = wave_sum(sse);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = ssim;
    red[1][tid >> 6] = sse;
  }
  __syncthreads();
  if (tid < 2) {
    const int ntile = p.tiles_x * p.tiles_y;
    const size_t slot = (size_t)n * p.channels * ntile + (size_t)ch * ntile + blockIdx.x;
    p.part[slot * 2 + tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
  }
}

int metric_tiles(int h, int w, int* tx, int* ty) {
  const int vh = h - 2 * PADW, vw = w - 2 * PADW;
  if (vh <= 0 || vw <= 0) return 0;
  *tx = (vw + TILE - 1) / TILE;
  *ty = (vh + TILE - 1) / TILE;
  return *tx * *ty;
}

void gauss_taps(GaussTaps* t) {
  float s = 0.f;
  for (int k = 0; k < KW; ++k) {          // torchmetrics _gaussian: exp(-(d / sigma)^2 / 2), normalised, float32
    const float d = (float)(k - PADW) / 1.5f;
    t->g[k] = expf(-(d * d) / 2.f);
    s += t->g[k];
  }
  for (int k = 0; k < KW; ++k) t->g[k] /= s;
}

// tiles of the region an image of h x w leaves after `shave` pixels on every side; 0 when it has no 11 x 11 window
int quality_tiles(int h, int w, int shave, int* tx, int* ty) {
  if (shave < 0 || h <= 0 || w <= 0 || shave > (h < w ? h : w) / 2) return 0;
  return metric_tiles(h - 2 * shave, w - 2 * shave, tx, ty);
}

template <bool LUMA>
int quality_launch(const MetricArgs& p, const U8Loader<LUMA>& ld, int ntile, int n, hipStream_t stream) {
  hipLaunchKernelGGL(ssim_sse_kernel<U8Loader<LUMA>>, dim3(ntile, p.channels, n), dim3(256), 0, stream, p, ld);
  return fsr_check_launch(LUMA ? "quality_u8_kernel<y>" : "quality_u8_kernel<rgb>");
}

}  // namespace

extern "C" size_t fsr_ssim_sse_scratch(int n, int h, int w) {
  int tx, ty;
  const int t = metric_tiles(h, w, &tx, &ty);
  return (n > 0 && t > 0) ? (size_t)n * 3 * t * 2 * sizeof(float) : 0;
}

extern "C" int fsr_ssim_sse(const float* a, long long asn, long long asc, long long ash, long long asw, const float* b,
                            long long bsn, long long bsc, long long bsh, long long bsw, int n, int h, int w, float* out,
                            void* scratch, fsr_stream_t stream_) {
  if (!a || !b || !out || !scratch) return fsr_fail(-1, "fsr_ssim_sse: null argument");
  if (n <= 0) return fsr_fail(-2, "fsr_ssim_sse: empty batch");
  MetricArgs p;
  p.tiles_x = p.tiles_y = 0;
  const int ntile = metric_tiles(h, w, &p.tiles_x, &p.tiles_y);
  if (ntile <= 0) return fsr_fail(-2, "fsr_ssim_sse: images must be larger than the 11x11 window (got %dx%d)", h, w);
  if (n > 65535) return fsr_fail(-2, "fsr_ssim_sse: batch too large");
  FloatLoader ld;
  ld.a = a; ld.asn = asn; ld.asc = asc; ld.ash = ash; ld.asw = asw;
  ld.b = b; ld.bsn = bsn; ld.bsc = bsc; ld.bsh = bsh; ld.bsw = bsw;
  ld.pa = ld.pb = nullptr;
  p.h = h; p.w = w; p.channels = 3;
  p.part = (float*)scratch;
  p.c1 = 0.01f * 0.01f;   // (k1 * data_range)^2, data_range 1.0 (trainer.py:46-48)
  p.c2 = 0.03f * 0.03f;
  p.shift_mean = p.shift_eps = p.shift_var = 0.f;
  gauss_taps(&p.taps);
  hipLaunchKernelGGL(ssim_sse_kernel<FloatLoader>, dim3(ntile, 3, n), dim3(256), 0, (hipStream_t)stream_, p, ld);
  if (int rc = fsr_check_launch("ssim_sse_kernel")) return rc;
  // out[n][2] = (sum of the ssim map over channels and valid pixels, sum of squared errors over the whole image)
  return fsr_launch_reduce_partials((const float*)scratch, out, n, 3 * ntile, 2, 2, 0, 0, 1.f, 0, (hipStream_t)stream_);
}

extern "C" size_t fsr_quality_u8_scratch(int n, int h, int w, int shave, int channel) {
  int tx, ty;
  if (n <= 0 || (channel != FSR_QUALITY_Y && channel != FSR_QUALITY_RGB)) return 0;
  const int t = quality_tiles(h, w, shave, &tx, &ty);
  return t > 0 ? (size_t)n * (channel == FSR_QUALITY_Y ? 1 : 3) * t * 2 * sizeof(float) : 0;
}

extern "C" int fsr_quality_u8(const unsigned char* a, long long a_image_bytes, long long a_row_bytes, const unsigned char* b,
                              long long b_image_bytes, long long b_row_bytes, int n, int h, int w, int shave, int channel,
                              float* out, void* scratch, fsr_stream_t stream_) {
  if (!a || !b || !out || !scratch) return fsr_fail(-1, "fsr_quality_u8: null argument");
  if (n <= 0 || n > 65535) return fsr_fail(-2, "fsr_quality_u8: batch n = %d outside 1 .. 65535", n);
  if (channel != FSR_QUALITY_Y && channel != FSR_QUALITY_RGB) return fsr_fail(-2, "fsr_quality_u8: unknown channel %d", channel);
  if (shave < 0) return fsr_fail(-2, "fsr_quality_u8: negative shave %d", shave);
  MetricArgs p;
  p.tiles_x = p.tiles_y = 0;
  const int ntile = quality_tiles(h, w, shave, &p.tiles_x, &p.tiles_y);
  if (ntile <= 0)
    return fsr_fail(-2, "fsr_quality_u8: the region left by shave %d of %dx%d is smaller than the 11x11 window", shave, h, w);
  if (a_row_bytes < 3LL * w || b_row_bytes < 3LL * w)
    return fsr_fail(-2, "fsr_quality_u8: row_bytes %lld / %lld below 3 w = %lld", a_row_bytes, b_row_bytes, 3LL * w);
  p.h = h - 2 * shave; p.w = w - 2 * shave; p.channels = channel == FSR_QUALITY_Y ? 1 : 3;
  p.part = (float*)scratch;
  const float k1 = 0.01f * 255.f, k2 = 0.03f * 255.f;   // Wang's SSIM at data range 255
  p.c1 = k1 * k1;
  p.c2 = k2 * k2;
  gauss_taps(&p.taps);
  double g1 = 0.0;
  for (int k = 0; k < KW; ++k) g1 += (double)p.taps.g[k];
  const double G = g1 * g1;                              // the sum of the 11 x 11 window
  p.shift_mean = (float)(SHIFT * G);
  p.shift_eps = (float)(1.0 - G);
  p.shift_var = (float)(SHIFT * SHIFT * G);
  U8Loader<true> ly;
  ly.a = a + shave * a_row_bytes + 3 * shave; ly.a_image = a_image_bytes; ly.a_row = a_row_bytes;
  ly.b = b + shave * b_row_bytes + 3 * shave; ly.b_image = b_image_bytes; ly.b_row = b_row_bytes;
  ly.ta = ly.tb = ly.raw = nullptr; ly.ch = 0;
  int rc;
  if (channel == FSR_QUALITY_Y) {
    rc = quality_launch(p, ly, ntile, n, (hipStream_t)stream_);
  } else {
    U8Loader<false> lc;
    lc.a = ly.a; lc.a_image = ly.a_image; lc.a_row = ly.a_row;
    lc.b = ly.b; lc.b_image = ly.b_image; lc.b_row = ly.b_row;
    lc.ta = lc.tb = lc.raw = nullptr; lc.ch = 0;
    rc = quality_launch(p, lc, ntile, n, (hipStream_t)stream_);
  }
  if (rc) return rc;
  // out[n][2] = (sum of the SSIM map over the channels and the windows inside the region, sum of squared errors over the region)
  return fsr_launch_reduce_partials((const float*)scratch, out, n, p.channels * ntile, 2, 2, 0, 0, 1.f, 0, (hipStream_t)stream_);
}
