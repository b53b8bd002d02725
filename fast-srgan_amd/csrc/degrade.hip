// Training degradations on the device: LR = JPEG(blur(LR) + n) with per-sample strengths, on the float NCHW batch in
// [-1,1] that data.hip writes.  Three kernels: the two passes of a separable Gaussian blur (the noise is added in the epilogue of the
// second; a template form of it is the noise-only launch), and a JPEG round trip without the entropy coder in which a workgroup owns
// 16x16 pixels -- one 4:2:0 MCU, or four 4:4:4 MCUs -- and runs colour transform, DCT, quantisation and the inverse out of LDS.
// The launch sequence never depends on the parameters drawn: a sample whose stage is off passes through the same launches as a copy.
#include "fsr_common.h"
#include "fsr_host.h"

namespace {

__device__ __forceinline__ unsigned mix32(unsigned x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// Box-Muller on two 24-bit uniforms of a stateless hash of (seed words, element index): U1 in (0, 1], U2 in [0, 1)
__device__ __forceinline__ float hash_normal(unsigned s0, unsigned s1, unsigned e) {
  const unsigned a = mix32(mix32(s0 + 2u * e) ^ s1);
  const unsigned b = mix32(mix32(s0 + 2u * e + 1u) ^ s1);
  const float u1 = (float)((a >> 8) + 1u) * 5.9604644775390625e-08f;   // 2^-24; both conversions are exact
  const float u2 = (float)(b >> 8) * 5.9604644775390625e-08f;
  return sqrtf(-2.0f * logf(u1)) * cosf(6.2831855f * u2);
}

__device__ __forceinline__ int blur_radius(const int* radii, int n) {
  const int r = radii[n];
  return r < 0 ? 0 : (r > FSR_BLUR_MAX_RADIUS ? FSR_BLUR_MAX_RADIUS : r);
}

// pass 1: tmp[n][c][y][x] = sum_j taps[n][j + r] * in[n][c][y][clamp(x + j)], j = -r..r
__global__ __launch_bounds__(256) void blur_hpass_kernel(const float* __restrict__ in, float* __restrict__ tmp, int h, int w,
                                                         const float* __restrict__ taps, const int* __restrict__ radii, long long total) {
  const long long plane3 = 3LL * h * w;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int n = (int)(i / plane3);
    const int x = (int)(i % w);
    const int r = blur_radius(radii, n);
    if (r == 0) {
      tmp[i] = in[i];
      continue;
    }
    const float* t = taps + (size_t)n * FSR_BLUR_TAPS + r;
    const float* row = in + (i - x);
    float s = 0.f;
    for (int j = -r; j <= r; ++j) {
      int xs = x + j;
      xs = xs < 0 ? 0 : (xs > w - 1 ? w - 1 : xs);
      s += t[j] * row[xs];
    }
    tmp[i] = s;
  }
}

// pass 2 (BLUR): out = sum_j taps[n][j + r] * tmp[clamp(y + j)][x]; then (NOISE) out += z * sigma_n * (2 / 255).  BLUR = false is the
// noise-only launch: `src` is the input itself.
template <bool BLUR, bool NOISE>
__global__ __launch_bounds__(256) void blur_vpass_noise_kernel(const float* __restrict__ src, float* __restrict__ out, int h, int w,
                                                               const float* __restrict__ taps, const int* __restrict__ radii,
                                                               const float* __restrict__ noise_sigma, const unsigned* __restrict__ seeds,
                                                               long long total) {
  const long long plane3 = 3LL * h * w;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int n = (int)(i / plane3);
    const unsigned e = (unsigned)(i - (long long)n * plane3);      // (c h + y) w + x  < 2^31 (host checked)
    float s = src[i];
    if constexpr (BLUR) {
      const int r = blur_radius(radii, n);
      if (r != 0) {
        const int y = (int)((e / (unsigned)w) % (unsigned)h);
        const float* t = taps + (size_t)n * FSR_BLUR_TAPS + r;
        const float* col = src + (i - (long long)y * w);
        s = 0.f;
        for (int j = -r; j <= r; ++j) {
          int ys = y + j;
          ys = ys < 0 ? 0 : (ys > h - 1 ? h - 1 : ys);
          s += t[j] * col[(size_t)ys * w];
        }
      }
    }
    if constexpr (NOISE) {
      const float sg = noise_sigma[n];
      if (sg > 0.f) s = fmaf(hash_normal(seeds[2 * n], seeds[2 * n + 1], e), sg * (2.0f / 255.0f), s);
    }
    out[i] = s;
  }
}

// ---------------------------------------------------------------------------------------------------------------- JPEG
// C[u][x] of the orthonormal 8-point DCT-II: sqrt(1/8) for u = 0, else 0.5 cos((2x + 1) u pi / 16)
__device__ const float kDct[64] = {
    0.35355339059327373f, 0.35355339059327373f, 0.35355339059327373f, 0.35355339059327373f, 0.35355339059327373f, 0.35355339059327373f, 0.35355339059327373f, 0.35355339059327373f,
    0.49039264020161522f, 0.41573480615127262f, 0.27778511650980114f, 0.09754516100806417f, -0.09754516100806417f, -0.27778511650980114f, -0.41573480615127262f, -0.49039264020161522f,
    0.46193976625564337f, 0.19134171618254492f, -0.19134171618254492f, -0.46193976625564337f, -0.46193976625564337f, -0.19134171618254492f, 0.19134171618254492f, 0.46193976625564337f,
    0.41573480615127262f, -0.09754516100806417f, -0.49039264020161522f, -0.27778511650980114f, 0.27778511650980114f, 0.49039264020161522f, 0.09754516100806417f, -0.41573480615127262f,
    0.35355339059327373f, -0.35355339059327373f, -0.35355339059327373f, 0.35355339059327373f, 0.35355339059327373f, -0.35355339059327373f, -0.35355339059327373f, 0.35355339059327373f,
    0.27778511650980114f, -0.49039264020161522f, 0.09754516100806417f, 0.41573480615127262f, -0.41573480615127262f, -0.09754516100806417f, 0.49039264020161522f, -0.27778511650980114f,
    0.19134171618254492f, -0.46193976625564337f, 0.46193976625564337f, -0.19134171618254492f, -0.19134171618254492f, 0.46193976625564337f, -0.46193976625564337f, 0.19134171618254492f,
    0.09754516100806417f, -0.27778511650980114f, 0.41573480615127262f, -0.49039264020161522f, 0.49039264020161522f, -0.41573480615127262f, 0.27778511650980114f, -0.09754516100806417f};
// Annex K base tables, row-major; [0] luminance, [1] chrominance
__device__ const unsigned char kQuantBase[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
     18, 22, 37, 56, 68, 109, 103,  77,  24, 35, 55, 64, 81, 104, 113,  92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// One workgroup = 16x16 pixels of one sample; thread t = pixel (t / 16, t % 16).  Blocks of 64 floats in LDS: 0..3 the Y blocks
// ((row / 8) * 2 + col / 8), then Cb, Cr -- one block each (S420: the 2x2 means) or four each.  The four 8-point passes walk the
// NB * 64 block elements, 256 at a time, ping-ponging between `pa` and `pb`.
template <bool S420>
__global__ __launch_bounds__(256) void jpeg_roundtrip_kernel(const float* __restrict__ in, float* __restrict__ out, int h, int w, int tiles_x,
                                                             int tiles_y, const int* __restrict__ quality) {
  constexpr int NB = S420 ? 6 : 12;
  __shared__ float pa[12 * 64];
  __shared__ float pb[12 * 64];
  __shared__ float dct[64];
  __shared__ float qt[2][64];
  const int t = threadIdx.x;
  int b = blockIdx.x;
  const int tx = b % tiles_x;
  b /= tiles_x;
  const int ty = b % tiles_y;
  const int n = b / tiles_y;
  const int py = t >> 4, px = t & 15;
  const int y = ty * 16 + py, x = tx * 16 + px;
  const bool inside = y < h && x < w;
  const int ys = y < h ? y : h - 1, xs = x < w ? x : w - 1;                     // edge replication of the padding
  const size_t plane = (size_t)h * w;
  const size_t src = (size_t)n * 3 * plane + (size_t)ys * w + xs;
  const size_t dst = (size_t)n * 3 * plane + (size_t)y * w + x;
  const float i0 = in[src], i1 = in[src + plane], i2 = in[src + 2 * plane];
  int q = quality[n];                                                           // uniform over the workgroup
  if (q <= 0) {
    if (inside) {
      out[dst] = i0;
      out[dst + plane] = i1;
      out[dst + 2 * plane] = i2;
    }
    return;
  }
  if (q > 100) q = 100;
  if (t < 64) dct[t] = kDct[t];
  if (t < 128) {
    const int s = q < 50 ? 5000 / q : 200 - 2 * q;
    int v = ((int)kQuantBase[t >> 6][t & 63] * s + 50) / 100;
    v = v < 1 ? 1 : (v > 255 ? 255 : v);
    qt[t >> 6][t & 63] = (float)v;
  }
  const float r = fminf(fmaxf((i0 + 1.0f) * 127.5f, 0.f), 255.f);
  const float g = fminf(fmaxf((i1 + 1.0f) * 127.5f, 0.f), 255.f);
  const float bl = fminf(fmaxf((i2 + 1.0f) * 127.5f, 0.f), 255.f);
  const float yy = 0.299f * r + 0.587f * g + 0.114f * bl;
  const float cb = 128.0f - 0.168736f * r - 0.331264f * g + 0.5f * bl;
  const float cr = 128.0f + 0.5f * r - 0.418688f * g - 0.081312f * bl;
  const int yblk = (py >> 3) * 2 + (px >> 3), pos = (py & 7) * 8 + (px & 7);
  pa[yblk * 64 + pos] = yy - 128.0f;
  if constexpr (S420) {
    pb[t] = cb;
    pb[256 + t] = cr;
    __syncthreads();
    if (t < 128) {
      const float* p = pb + (t >> 6) * 256;
      const int cy = (t & 63) >> 3, cx = t & 7;
      const float* tl = p + (2 * cy) * 16 + 2 * cx;
      pa[(4 + (t >> 6)) * 64 + (t & 63)] = ((tl[0] + tl[1]) + (tl[16] + tl[17])) * 0.25f - 128.0f;
    }
  } else {
    pa[(4 + yblk) * 64 + pos] = cb - 128.0f;
    pa[(8 + yblk) * 64 + pos] = cr - 128.0f;
  }
  __syncthreads();
  // forward rows: pb[blk][y][v] = sum_x pa[blk][y][x] C[v][x]
  for (int i = t; i < NB * 64; i += 256) {
    const float* row = pa + (i & ~7);
    const float* c = dct + (i & 7) * 8;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += row[k] * c[k];
    pb[i] = s;
  }
  __syncthreads();
  // forward columns, then quantise: pa[blk][u][v] = rint((sum_y C[u][y] pb[blk][y][v]) / Q[u][v]) * Q[u][v]
  for (int i = t; i < NB * 64; i += 256) {
    const int u = (i >> 3) & 7, v = i & 7;
    const float* col = pb + (i & ~63) + v;
    const float* c = dct + u * 8;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += c[k] * col[k * 8];
    const float qv = qt[i >= 4 * 64 ? 1 : 0][i & 63];
    pa[i] = rintf(s / qv) * qv;
  }
  __syncthreads();
  // inverse rows: pb[blk][u][x] = sum_v pa[blk][u][v] C[v][x]
  for (int i = t; i < NB * 64; i += 256) {
    const float* row = pa + (i & ~7);
    const int xx = i & 7;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += row[k] * dct[k * 8 + xx];
    pb[i] = s;
  }
  __syncthreads();
  // inverse columns: pa[blk][y][x] = sum_u C[u][y] pb[blk][u][x] + 128
  for (int i = t; i < NB * 64; i += 256) {
    const int yr = (i >> 3) & 7;
    const float* col = pb + (i & ~63) + (i & 7);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += dct[k * 8 + yr] * col[k * 8];
    pa[i] = s + 128.0f;
  }
  __syncthreads();
  if (!inside) return;
  const float yo = pa[yblk * 64 + pos];
  float cbo, cro;
  if constexpr (S420) {
    const int cpos = (py >> 1) * 8 + (px >> 1);                                 // replication
    cbo = pa[4 * 64 + cpos] - 128.0f;
    cro = pa[5 * 64 + cpos] - 128.0f;
  } else {
    cbo = pa[(4 + yblk) * 64 + pos] - 128.0f;
    cro = pa[(8 + yblk) * 64 + pos] - 128.0f;
  }
  const float ro = yo + 1.402f * cro;
  const float go = yo - 0.344136f * cbo - 0.714136f * cro;
  const float bo = yo + 1.772f * cbo;
  out[dst] = fminf(fmaxf(rintf(ro), 0.f), 255.f) / 127.5f - 1.0f;
  out[dst + plane] = fminf(fmaxf(rintf(go), 0.f), 255.f) / 127.5f - 1.0f;
  out[dst + 2 * plane] = fminf(fmaxf(rintf(bo), 0.f), 255.f) / 127.5f - 1.0f;
}

int batch_check(const char* who, int n, int h, int w) {
  if (n <= 0 || h <= 0 || w <= 0) return fsr_fail(-2, "%s: n, h and w must be positive (n = %d, h = %d, w = %d)", who, n, h, w);
  if (3LL * h * w >= 0x80000000LL) return fsr_fail(-2, "%s: a sample of 3 x %d x %d elements does not fit in 31 bits", who, h, w);
  return 0;
}

unsigned stride_blocks(long long total) {
  const long long blocks = (total + 255) / 256;
  return (unsigned)(blocks > 4096 ? 4096 : blocks);
}

}  // namespace

extern "C" int fsr_degrade_blur_noise(const float* in, float* out, float* tmp, int n, int h, int w, const float* taps, const int* radii,
                                      const float* noise_sigma, const unsigned* seeds, fsr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const bool blur = taps || radii, noise = noise_sigma || seeds;
  if (!in || !out) return fsr_fail(-1, "fsr_degrade_blur_noise: null argument");
  if (blur && (!taps || !radii || !tmp)) return fsr_fail(-1, "fsr_degrade_blur_noise: the blur needs taps, radii and tmp");
  if (noise && (!noise_sigma || !seeds)) return fsr_fail(-1, "fsr_degrade_blur_noise: the noise needs noise_sigma and seeds");
  if (!blur && !noise) return fsr_fail(-1, "fsr_degrade_blur_noise: neither blur (taps, radii) nor noise (noise_sigma, seeds) given");
  if (blur && (tmp == in || tmp == out)) return fsr_fail(-2, "fsr_degrade_blur_noise: tmp must not be the input or the output");
  if (int rc = batch_check("fsr_degrade_blur_noise", n, h, w)) return rc;
  const long long total = 3LL * h * w * n;
  const unsigned blocks = stride_blocks(total);
  if (!blur) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(blur_vpass_noise_kernel<false, true>), dim3(blocks), dim3(256), 0, stream, in, out, h, w, taps, radii,
                       noise_sigma, seeds, total);
    fsr_note_kernel("noise_kernel");
    return fsr_check_launch("noise_kernel");
  }
  hipLaunchKernelGGL(blur_hpass_kernel, dim3(blocks), dim3(256), 0, stream, in, tmp, h, w, taps, radii, total);
  if (int rc = fsr_check_launch("blur_hpass_kernel")) return rc;
  if (noise)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(blur_vpass_noise_kernel<true, true>), dim3(blocks), dim3(256), 0, stream, (const float*)tmp, out, h, w,
                       taps, radii, noise_sigma, seeds, total);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(blur_vpass_noise_kernel<true, false>), dim3(blocks), dim3(256), 0, stream, (const float*)tmp, out, h, w,
                       taps, radii, noise_sigma, seeds, total);
  fsr_note_kernel(noise ? "blur_hpass_kernel+blur_vpass_noise_kernel" : "blur_hpass_kernel+blur_vpass_kernel");
  return fsr_check_launch("blur_vpass_noise_kernel");
}

extern "C" int fsr_jpeg_roundtrip(const float* in, float* out, int n, int h, int w, const int* quality, int subsampling, fsr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!in || !out || !quality) return fsr_fail(-1, "fsr_jpeg_roundtrip: null argument");
  if (subsampling != FSR_CHROMA_420 && subsampling != FSR_CHROMA_444)
    return fsr_fail(-2, "fsr_jpeg_roundtrip: subsampling must be FSR_CHROMA_420 or FSR_CHROMA_444 (got %d)", subsampling);
  if (int rc = batch_check("fsr_jpeg_roundtrip", n, h, w)) return rc;
  const int tiles_x = (w + 15) / 16, tiles_y = (h + 15) / 16;
  const long long blocks = (long long)n * tiles_x * tiles_y;
  if (blocks > 0x7fffffffLL) return fsr_fail(-2, "fsr_jpeg_roundtrip: %lld workgroups do not fit in one launch", blocks);
  if (subsampling == FSR_CHROMA_420)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(jpeg_roundtrip_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, stream, in, out, h, w, tiles_x, tiles_y,
                       quality);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(jpeg_roundtrip_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, stream, in, out, h, w, tiles_x, tiles_y,
                       quality);
  fsr_note_kernel(subsampling == FSR_CHROMA_420 ? "jpeg_roundtrip_kernel<420>" : "jpeg_roundtrip_kernel<444>");
  return fsr_check_launch("jpeg_roundtrip_kernel");
}
