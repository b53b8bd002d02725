// Training degradations on the device: LR = JPEG(blur(LR) + n) with per-sample strengths, on the float NCHW batch in
// [-1,1] that data.hip writes.  Three kernels: the two passes of a separable Gaussian blur (the noise is added in the epilogue of the
// second; a template form of it is the noise-only launch), and a JPEG round trip without the entropy coder in which a workgroup owns
// 16x16 pixels -- one 4:2:0 MCU, or four 4:4:4 MCUs -- and runs colour transform, DCT, quantisation and the inverse out of LDS.
// The launch sequence never depends on the parameters drawn: a sample whose stage is off passes through the same launches as a copy.
// The high-order model adds a per-sample K x K filter out of LDS (filter2d_kernel), a separable resize with a tap table
// chosen per sample, and the noise-only launch with a kind (shot, grey) per sample.
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
// noise-only launch: `src` is the input itself.  KINDS reads a flag word per sample beside its strength: FSR_NOISE_SHOT
// scales z by sqrt(g v) of the element's own code v (the normal approximation of shot noise), FSR_NOISE_GREY hashes y w + x so that the
// channels of a pixel share z; without a flag the arithmetic is that of KINDS = false.
template <bool BLUR, bool NOISE, bool KINDS = false>
__global__ __launch_bounds__(256) void blur_vpass_noise_kernel(const float* __restrict__ src, float* __restrict__ out, int h, int w,
                                                               const float* __restrict__ taps, const int* __restrict__ radii,
                                                               const float* __restrict__ noise_sigma, const unsigned* __restrict__ seeds,
                                                               const int* __restrict__ flags, long long total) {
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
      if (sg > 0.f) {
        float amp = sg;
        unsigned ei = e;
        if constexpr (KINDS) {
          const int f = flags[n];
          if (f & FSR_NOISE_GREY) ei = e % ((unsigned)h * (unsigned)w);
          if (f & FSR_NOISE_SHOT) amp = sqrtf(sg * fminf(fmaxf((s + 1.0f) * 127.5f, 0.f), 255.f));
        }
        s = fmaf(hash_normal(seeds[2 * n], seeds[2 * n + 1], ei), amp * (2.0f / 255.0f), s);
      }
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

// ---------------------------------------------------------------------------------------------- per-sample K x K filter
// out[n][c][y][x] = sum_dy sum_dx k_n[dy + r][dx + r] in[n][c][clamp(y + dy)][clamp(x + dx)], K = 2 r + 1 <= 21.  One workgroup owns
// FSR_FILTER2D_TILE_H x FSR_FILTER2D_TILE_W outputs of one (sample, channel): it stages the tile and its r-pixel halo in LDS once, the
// borders already clamped, then thread (t / 8, t % 8) produces the 8 adjacent outputs of row t / 8 that start at column 8 (t % 8).  Per
// kernel row it reads its 8 + 2 r source values from LDS into registers once (16-byte reads: the pitch and the run start are multiples
// of four floats) and slides the K taps of that row over them, so one LDS row read feeds 8 K FMAs.  The taps and the radius are uniform
// over the workgroup and come through the scalar data path; the body is instantiated per radius and chosen by a uniform switch, so the
// loops run to the sample's own r with every register index static.  No atomics, no scratch.
constexpr int F2D_TH = FSR_FILTER2D_TILE_H, F2D_TW = FSR_FILTER2D_TILE_W, F2D_RUN = 8;
constexpr int F2D_PITCH = F2D_TW + 2 * FSR_FILTER2D_MAX_RADIUS;                      // 84 floats = 21 x 16 bytes
static_assert(F2D_TH * (F2D_TW / F2D_RUN) == 256 && F2D_PITCH % 4 == 0 && F2D_PITCH <= 128, "filter2d_kernel's thread layout");

template <int R>
__device__ __forceinline__ void filter2d_rows(const float* tile, const float* __restrict__ taps, int ly, int x0, float (&acc)[F2D_RUN]) {
  constexpr int K = 2 * R + 1, NV = (F2D_RUN + 2 * R + 3) / 4;                       // x0 + 4 NV <= F2D_PITCH: the last read stays in its row
#pragma unroll 1
  for (int dy = 0; dy < K; ++dy) {
    const float4* row = (const float4*)(tile + (ly + dy) * F2D_PITCH + x0);
    float win[4 * NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const float4 v = row[j];
      win[4 * j] = v.x;
      win[4 * j + 1] = v.y;
      win[4 * j + 2] = v.z;
      win[4 * j + 3] = v.w;
    }
    const float* tr = taps + dy * K;
#pragma unroll
    for (int dx = 0; dx < K; ++dx) {
      const float tv = tr[dx];
#pragma unroll
      for (int i = 0; i < F2D_RUN; ++i) acc[i] += tv * win[dx + i];
    }
  }
}

__global__ __launch_bounds__(256) void filter2d_kernel(const float* __restrict__ in, float* __restrict__ out, int h, int w, int tiles_x,
                                                       int tiles_y, const float* __restrict__ taps, const int* __restrict__ radii, int vec) {
  __shared__ __attribute__((aligned(16))) float tile[(F2D_TH + 2 * FSR_FILTER2D_MAX_RADIUS) * F2D_PITCH];
  const int t = threadIdx.x;
  int b = blockIdx.x;
  const int X0 = (b % tiles_x) * F2D_TW;
  b /= tiles_x;
  const int Y0 = (b % tiles_y) * F2D_TH;
  const int nc = b / tiles_y;                                                        // 3 n + c
  const int n = nc / 3;
  int r = radii[n];                                                                  // uniform over the workgroup
  r = r < 0 ? 0 : (r > FSR_FILTER2D_MAX_RADIUS ? FSR_FILTER2D_MAX_RADIUS : r);
  const size_t plane = (size_t)h * w;
  const float* src = in + (size_t)nc * plane;
  const int ly = t >> 3, x0 = (t & 7) * F2D_RUN;
  const int y = Y0 + ly, x = X0 + x0;
  float* dst = out + (size_t)nc * plane + (size_t)y * w + x;
  if (r == 0) {                                                                      // a copy, bit for bit
    if (y < h) {
      const float* s = src + (size_t)y * w + x;
#pragma unroll
      for (int i = 0; i < F2D_RUN; ++i)
        if (x + i < w) dst[i] = s[i];
    }
    return;
  }
  const int rows = (h - Y0 < F2D_TH ? h - Y0 : F2D_TH) + 2 * r, cols = (w - X0 < F2D_TW ? w - X0 : F2D_TW) + 2 * r;
  const int lx = t & 127;
  if (lx < cols) {
    int xs = X0 + lx - r;
    xs = xs < 0 ? 0 : (xs > w - 1 ? w - 1 : xs);
    for (int yy = t >> 7; yy < rows; yy += 2) {
      int ys = Y0 + yy - r;
      ys = ys < 0 ? 0 : (ys > h - 1 ? h - 1 : ys);
      tile[yy * F2D_PITCH + lx] = src[(size_t)ys * w + xs];
    }
  }
  __syncthreads();
  float acc[F2D_RUN];
#pragma unroll
  for (int i = 0; i < F2D_RUN; ++i) acc[i] = 0.f;
  const float* tp = taps + (size_t)n * FSR_FILTER2D_TAPS;
  switch (r) {
    case 1: filter2d_rows<1>(tile, tp, ly, x0, acc); break;
    case 2: filter2d_rows<2>(tile, tp, ly, x0, acc); break;
    case 3: filter2d_rows<3>(tile, tp, ly, x0, acc); break;
    case 4: filter2d_rows<4>(tile, tp, ly, x0, acc); break;
    case 5: filter2d_rows<5>(tile, tp, ly, x0, acc); break;
    case 6: filter2d_rows<6>(tile, tp, ly, x0, acc); break;
    case 7: filter2d_rows<7>(tile, tp, ly, x0, acc); break;
    case 8: filter2d_rows<8>(tile, tp, ly, x0, acc); break;
    case 9: filter2d_rows<9>(tile, tp, ly, x0, acc); break;
    default: filter2d_rows<10>(tile, tp, ly, x0, acc); break;
  }
  if (y >= h) return;
  if (vec && x + F2D_RUN <= w) {                                                     // w % 4 == 0 and a 16-byte aligned batch (host checked)
    ((float4*)dst)[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    ((float4*)dst)[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    return;
  }
#pragma unroll
  for (int i = 0; i < F2D_RUN; ++i)
    if (x + i < w) dst[i] = acc[i];
}

// ------------------------------------------------------------------------------------------ resize with a table per sample
__device__ __forceinline__ int table_index(const int* sel, int n, int nf) {
  const int f = sel[n];
  return f < 0 ? 0 : (f > nf - 1 ? nf - 1 : f);
}

// pass 1: tmp[n][c][y][xo] = sum_k wx[f][xo][k] * in[n][c][y][xmin[f][xo] + k], f = sel[n]
__global__ __launch_bounds__(256) void resize_select_hpass_kernel(const float* __restrict__ in, float* __restrict__ tmp, int ih, int iw, int ow,
                                                                  const float* __restrict__ wx, const int* __restrict__ xmin,
                                                                  const int* __restrict__ xsize, int kx, int nf, const int* __restrict__ sel,
                                                                  long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int xo = (int)(i % ow);
  const long long row = i / ow;                                     // (n 3 + c) ih + y
  const int n = (int)(row / (3LL * ih));
  const int f = table_index(sel, n, nf);
  const float* wt = wx + ((size_t)f * ow + xo) * kx;
  const int x0 = xmin[f * ow + xo], ks = xsize[f * ow + xo];
  const float* src = in + (size_t)row * iw + x0;
  float s = 0.f;
  for (int k = 0; k < ks; ++k) s += wt[k] * src[k];
  tmp[i] = s;
}

// pass 2: out[n][c][yo][xo] = sum_k wy[f][yo][k] * tmp[n][c][ymin[f][yo] + k][xo]
__global__ __launch_bounds__(256) void resize_select_vpass_kernel(const float* __restrict__ tmp, float* __restrict__ out, int ih, int oh, int ow,
                                                                  const float* __restrict__ wy, const int* __restrict__ ymin,
                                                                  const int* __restrict__ ysize, int ky, int nf, const int* __restrict__ sel,
                                                                  long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int xo = (int)(i % ow);
  const int yo = (int)((i / ow) % oh);
  const long long nc = i / ((long long)ow * oh);
  const int f = table_index(sel, (int)(nc / 3), nf);
  const float* wt = wy + ((size_t)f * oh + yo) * ky;
  const int y0 = ymin[f * oh + yo], ks = ysize[f * oh + yo];
  const float* col = tmp + ((size_t)nc * ih + y0) * ow + xo;
  float s = 0.f;
  for (int k = 0; k < ks; ++k) s += wt[k] * col[(size_t)k * ow];
  out[i] = s;
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
                       noise_sigma, seeds, (const int*)nullptr, total);
    fsr_note_kernel("noise_kernel");
    return fsr_check_launch("noise_kernel");
  }
  hipLaunchKernelGGL(blur_hpass_kernel, dim3(blocks), dim3(256), 0, stream, in, tmp, h, w, taps, radii, total);
  if (int rc = fsr_check_launch("blur_hpass_kernel")) return rc;
  if (noise)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(blur_vpass_noise_kernel<true, true>), dim3(blocks), dim3(256), 0, stream, (const float*)tmp, out, h, w,
                       taps, radii, noise_sigma, seeds, (const int*)nullptr, total);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(blur_vpass_noise_kernel<true, false>), dim3(blocks), dim3(256), 0, stream, (const float*)tmp, out, h, w,
                       taps, radii, noise_sigma, seeds, (const int*)nullptr, total);
  fsr_note_kernel(noise ? "blur_hpass_kernel+blur_vpass_noise_kernel" : "blur_hpass_kernel+blur_vpass_kernel");
  return fsr_check_launch("blur_vpass_noise_kernel");
}

extern "C" int fsr_filter2d(const float* in, float* out, int n, int h, int w, const float* taps, const int* radii, fsr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!in || !out || !taps || !radii) return fsr_fail(-1, "fsr_filter2d: null argument");
  if (in == out) return fsr_fail(-2, "fsr_filter2d: the output must not be the input (a workgroup reads its neighbours' pixels)");
  if (int rc = batch_check("fsr_filter2d", n, h, w)) return rc;
  const int tiles_x = (w + F2D_TW - 1) / F2D_TW, tiles_y = (h + F2D_TH - 1) / F2D_TH;
  const long long blocks = 3LL * n * tiles_x * tiles_y;
  if (blocks > 0x7fffffffLL) return fsr_fail(-2, "fsr_filter2d: %lld workgroups do not fit in one launch", blocks);
  const int vec = (w % 4 == 0) && ((uintptr_t)out % 16 == 0);
  hipLaunchKernelGGL(filter2d_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, in, out, h, w, tiles_x, tiles_y, taps, radii, vec);
  fsr_note_kernel("filter2d_kernel");
  return fsr_check_launch("filter2d_kernel");
}

extern "C" int fsr_degrade_noise_kinds(const float* in, float* out, int n, int h, int w, const float* strength, const int* flags,
                                       const unsigned* seeds, fsr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!in || !out || !strength || !flags || !seeds) return fsr_fail(-1, "fsr_degrade_noise_kinds: null argument");
  if (int rc = batch_check("fsr_degrade_noise_kinds", n, h, w)) return rc;
  const long long total = 3LL * h * w * n;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(blur_vpass_noise_kernel<false, true, true>), dim3(stride_blocks(total)), dim3(256), 0, stream, in, out, h, w,
                     (const float*)nullptr, (const int*)nullptr, strength, seeds, flags, total);
  fsr_note_kernel("noise_kinds_kernel");
  return fsr_check_launch("noise_kinds_kernel");
}

extern "C" int fsr_resize_select(const float* in, float* out, float* tmp, int n, int ih, int iw, int oh, int ow, const float* wx, const int* xmin,
                                 const int* xsize, int kx, const float* wy, const int* ymin, const int* ysize, int ky, int nf, const int* sel,
                                 fsr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!in || !out || !tmp || !wx || !xmin || !xsize || !wy || !ymin || !ysize || !sel) return fsr_fail(-1, "fsr_resize_select: null argument");
  if (tmp == in || tmp == out || in == out) return fsr_fail(-2, "fsr_resize_select: in, tmp and out must be three buffers");
  if (int rc = batch_check("fsr_resize_select", n, ih, iw)) return rc;
  if (oh <= 0 || ow <= 0 || kx <= 0 || ky <= 0 || nf <= 0)
    return fsr_fail(-2, "fsr_resize_select: oh, ow, kx, ky and nf must be positive (got %d, %d, %d, %d, %d)", oh, ow, kx, ky, nf);
  if (3LL * ih * ow >= 0x80000000LL) return fsr_fail(-2, "fsr_resize_select: an intermediate sample of 3 x %d x %d elements does not fit in 31 bits", ih, ow);
  if (3LL * oh * ow >= 0x80000000LL) return fsr_fail(-2, "fsr_resize_select: an output sample of 3 x %d x %d elements does not fit in 31 bits", oh, ow);
  const long long total1 = 3LL * n * ih * ow, total2 = 3LL * n * oh * ow;
  const long long blocks1 = (total1 + 255) / 256, blocks2 = (total2 + 255) / 256;
  if (blocks1 > 0x7fffffffLL || blocks2 > 0x7fffffffLL) return fsr_fail(-2, "fsr_resize_select: %lld workgroups do not fit in one launch", blocks1 > blocks2 ? blocks1 : blocks2);
  hipLaunchKernelGGL(resize_select_hpass_kernel, dim3((unsigned)blocks1), dim3(256), 0, stream, in, tmp, ih, iw, ow, wx, xmin, xsize, kx, nf, sel,
                     total1);
  if (int rc = fsr_check_launch("resize_select_hpass_kernel")) return rc;
  hipLaunchKernelGGL(resize_select_vpass_kernel, dim3((unsigned)blocks2), dim3(256), 0, stream, (const float*)tmp, out, ih, oh, ow, wy, ymin,
                     ysize, ky, nf, sel, total2);
  fsr_note_kernel("resize_select_hpass_kernel+resize_select_vpass_kernel");
  return fsr_check_launch("resize_select_vpass_kernel");
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
