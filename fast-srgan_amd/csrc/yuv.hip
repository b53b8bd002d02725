// Planar YUV frames in and out of the generator's float image (the colour contract is DESIGN.md §6c): the decode and encode kernels of
// 4:2:0, 4:2:2 and 4:4:4 payloads at 8 to 16 bits, and their five entry points.  fsr_yuv_to_image and fsr_image_to_yuv are the
// implementation; the I420-named entry points forward into them, and the _ex forms add the payload layout: FSR_LAYOUT_NV12, the
// semi-planar 4:2:0 payload of DESIGN.md §6f (NV12, P010, P012, P016).  The arithmetic lives in fsr_yuv.h, shared with the head kernels'
// I420 epilogue and with the resampler (resample.hip), which also shares fsr_yuv_out_check below.
#include "fsr_yuv.h"
#include "fsr_host.h"

namespace {

// I420 frames -> float [n,h,w,3] = 2 c - 1 of the decoded RGB c in [0, 1] (fsr_i420_to_image; the colour contract is DESIGN.md
// "Video"): one thread per pixel, chroma upsampled bilinearly with edge clamp at the declared siting -- luma pixel (y, x) reads
// chroma at ((y - 1/2) / 2, (x - 1/2) / 2) (C420jpeg) or ((y - 1/2) / 2, x / 2) (C420mpeg2); then the inverse of the encode
// matrix, R, G, B clamped to [0, 1] (no 8-bit RGB in between).
// S: the sample type -- unsigned char, or unsigned short for the 9..16-bit payloads of fsr_i420_to_image_deep (little-endian, the
// value in the low `depth` bits; a stored value above 2^depth - 1 is taken as it is, the clamp of R, G, B deals with it).  The
// coefficients scale with the depth: limited Y = (16 + 219 E_Y) 2^(d-8), C = (128 + 224 E_C) 2^(d-8); full Y = (2^d - 1) E_Y,
// C = 2^(d-1) + (2^d - 1) E_C -- for S = unsigned char d is the constant 8.
// SEMI (FSR_LAYOUT_NV12): the chroma planes are ONE plane of ch rows of cw (Cb, Cr) pairs -- pair stride 2, Cr at + 1 --, and a 16-bit
// sample holds its code in the HIGH d bits: every sample read is stored >> (16 - d), whatever the low bits hold.  Same arithmetic.
template <typename S, bool SEMI = false>
__global__ __launch_bounds__(256) void i420_to_image_kernel(const S* __restrict__ src, float* __restrict__ dst, int n, int h,
                                                            int w, int mpeg2, int matrix, int full, int depth) {
  const int d = sizeof(S) == 1 ? 8 : depth;
  const int sh = SEMI && sizeof(S) == 2 ? 16 - d : 0;
  const int ch = (h + 1) >> 1, cw = (w + 1) >> 1;
  const long long plane = (long long)h * w, cplane = (long long)ch * cw, fbytes = plane + 2 * cplane;   // (samples)
  const i420_coef kc = yuv_decode_coefs(matrix, full, d);
  const long long total = (long long)n * plane;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long img = i / plane;
    const int p = (int)(i - img * plane), y = p / w, x = p - y * w;
    const S* f = src + img * fbytes;
    const float cy = 0.5f * (float)y - 0.25f, cx = mpeg2 ? 0.5f * (float)x : 0.5f * (float)x - 0.25f;
    const float fy0 = floorf(cy), fx0 = floorf(cx);
    const float fy = cy - fy0, fx = cx - fx0;
    const int iy = (int)fy0, ix = (int)fx0;      // >= -1
    const int y0 = iy < 0 ? 0 : iy, y1 = iy + 1 < ch ? iy + 1 : ch - 1, x0 = ix < 0 ? 0 : ix, x1 = ix + 1 < cw ? ix + 1 : cw - 1;
    float c[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      float s00, s01, s10, s11;
      if constexpr (SEMI) {
        const S* q = f + plane + k;
        s00 = (float)(q[2 * ((long long)y0 * cw + x0)] >> sh);
        s01 = (float)(q[2 * ((long long)y0 * cw + x1)] >> sh);
        s10 = (float)(q[2 * ((long long)y1 * cw + x0)] >> sh);
        s11 = (float)(q[2 * ((long long)y1 * cw + x1)] >> sh);
      } else {
        const S* q = f + plane + k * cplane;
        s00 = (float)q[y0 * cw + x0];
        s01 = (float)q[y0 * cw + x1];
        s10 = (float)q[y1 * cw + x0];
        s11 = (float)q[y1 * cw + x1];
      }
      const float top = (1.f - fx) * s00 + fx * s01;
      const float bot = (1.f - fx) * s10 + fx * s11;
      c[k] = (1.f - fy) * top + fy * bot;
    }
    yuv_decode_pixel(kc, SEMI ? (float)(f[p] >> sh) : (float)f[p], c[0], c[1], dst + i * 3);
  }
}

// float tanh output t [n,h,w,3] -> I420 planes (fsr_image_to_i420; the encode of DESIGN.md §6c at any depth 8..16, what the head's
// FSR_OUT_I420 epilogue computes for 8 bits): a streaming kernel in the shape of the resampler's I420 stage.  A thread owns 4 columns x
// 2 rows -- two whole 2x2 blocks, so no LDS, no shuffle, no atomics: three 16-byte loads per row (the rows are only 8-byte aligned when
// w is not a multiple of 4; 6 floats per row in the last unit of such a row), c = clamp((t + 1) / 2, 0, 1), then i420_store_2x4: one
// 4- or 8-byte Y store per row and 2 + 2 chroma samples.  Grid-stride over the n * (h / 2) * ceil(w / 4) units (< 2^31: host checked).
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef float f32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));
// SEMI (FSR_LAYOUT_NV12): the semi-planar payload -- the unit's Cb0, Cr0, Cb1, Cr1 leave as one store, 16-bit codes in the high bits
template <typename C, bool SEMI = false>
__global__ __launch_bounds__(256) void image_to_i420_kernel(const float* __restrict__ t, C* __restrict__ out, int n, int h, int w, int matrix,
                                                            int full, int depth) {
  const i420_coef kc = i420_coefs(matrix, full, sizeof(C) == 1 ? 8 : depth);
  const unsigned wq = (unsigned)(w + 3) >> 2, hp = (unsigned)h >> 1;
  const unsigned units = (unsigned)n * hp * wq;
  const size_t fsamples = (size_t)h * w + 2 * ((size_t)(h >> 1) * (size_t)(w >> 1));
  for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < units; u += gridDim.x * 256u) {
    const unsigned row = u / wq, xq = u - row * wq;
    const unsigned img = row / hp, yp = row - img * hp;
    const int x = (int)xq * 4, y = (int)yp * 2;
    const int cnt = w - x < 4 ? w - x : 4;       // 2 or 4: w is even
    float v[2][12];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const float* p = t + (((size_t)img * h + (y + m)) * w + x) * 3;
      f32x4_a4 q0 = *(const f32x4_a4*)p, q1, q2 = {0.f, 0.f, 0.f, 0.f};
      if (cnt == 4) {
        q1 = *(const f32x4_a4*)(p + 4);
        q2 = *(const f32x4_a4*)(p + 8);
      } else {
        const f32x2_a4 e = *(const f32x2_a4*)(p + 4);
        q1 = (f32x4_a4){e[0], e[1], 0.f, 0.f};
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[m][k] = fminf(fmaxf((q0[k] + 1.f) / 2.f, 0.f), 1.f);
        v[m][4 + k] = fminf(fmaxf((q1[k] + 1.f) / 2.f, 0.f), 1.f);
        v[m][8 + k] = fminf(fmaxf((q2[k] + 1.f) / 2.f, 0.f), 1.f);
      }
    }
    i420_store_2x4<C, SEMI>(kc, v, out + (size_t)img * fsamples, h, w, y, x, cnt, SEMI && sizeof(C) == 2 ? 16 - depth : 0);
  }
}

// 4:2:2 / 4:4:4 frames -> float [n,h,w,3] (fsr_yuv_to_image): the decode of i420_to_image_kernel without the vertical
// interpolation.  A thread takes 4 consecutive pixels of a row: one 4- or 8-byte Y load, per chroma plane the same (4:4:4) or the samples
// j0 - 1 .. j0 + 2 around its two chroma columns (4:2:2, j0 = x / 2, edge clamp; luma column x reads chroma at x / 2 (mpeg2) or
// (x - 1/2) / 2 (jpeg), linear), and three 16-byte stores.  Rows of odd-width frames are not aligned and the last unit of a row may hold
// fewer than 4 pixels: narrower accesses there.  Grid-stride over the n * h * ceil(w / 4) units (< 2^31: host checked).
template <typename S>
__device__ __forceinline__ void load_samples4(const S* p, int cnt, float (&v)[4]) {
  typedef typename std::conditional<sizeof(S) == 1, unsigned, u32x2>::type quad_t;
  if (cnt == 4 && ((size_t)p & (4 * sizeof(S) - 1)) == 0) {
    const quad_t q = *(const quad_t*)p;
    if constexpr (sizeof(S) == 1) {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = (float)((q >> (8 * i)) & 0xffu);
    } else {
      v[0] = (float)(q.x & 0xffffu);
      v[1] = (float)(q.x >> 16);
      v[2] = (float)(q.y & 0xffffu);
      v[3] = (float)(q.y >> 16);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = i < cnt ? (float)p[i] : 0.f;
  }
}
template <typename S, int CHROMA>
__global__ __launch_bounds__(256) void yuv_to_image_kernel(const S* __restrict__ src, float* __restrict__ dst, int n, int h, int w, int mpeg2,
                                                           int matrix, int full, int depth) {
  const int d = sizeof(S) == 1 ? 8 : depth;
  const int cw = CHROMA == FSR_CHROMA_444 ? w : (w + 1) >> 1;
  const size_t plane = (size_t)h * w, cplane = (size_t)h * cw, fsamples = plane + 2 * cplane;
  const i420_coef kc = yuv_decode_coefs(matrix, full, d);
  const unsigned wq = (unsigned)(w + 3) >> 2;
  const unsigned units = (unsigned)n * (unsigned)h * wq;
  for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < units; u += gridDim.x * 256u) {
    const unsigned row = u / wq, xq = u - row * wq;
    const unsigned img = row / (unsigned)h, y = row - img * (unsigned)h;
    const int x = (int)xq * 4;
    const int cnt = w - x < 4 ? w - x : 4;
    const S* f = src + (size_t)img * fsamples;
    float yv[4], c[2][4];
    load_samples4(f + (size_t)y * w + x, cnt, yv);
    if constexpr (CHROMA == FSR_CHROMA_444) {
      load_samples4(f + plane + (size_t)y * w + x, cnt, c[0]);
      load_samples4(f + 2 * plane + (size_t)y * w + x, cnt, c[1]);
    } else {
      const int j0 = x >> 1;
      const int ja = j0 > 0 ? j0 - 1 : 0, jb = j0 + 1 < cw ? j0 + 1 : cw - 1, jc = j0 + 2 < cw ? j0 + 2 : cw - 1;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const S* q = f + plane + k * cplane + (size_t)y * cw;
        const float s0 = (float)q[ja], s1 = (float)q[j0], s2 = (float)q[jb], s3 = (float)q[jc];
        // (1 - fx) * left + fx * right, as i420_to_image_kernel: mpeg2 fx = 0, 1/2, 0, 1/2 from s1; jpeg fx = 3/4, 1/4, 3/4, 1/4 from s0
        c[k][0] = mpeg2 ? s1 : 0.25f * s0 + 0.75f * s1;
        c[k][1] = mpeg2 ? 0.5f * s1 + 0.5f * s2 : 0.75f * s1 + 0.25f * s2;
        c[k][2] = mpeg2 ? s2 : 0.25f * s1 + 0.75f * s2;
        c[k][3] = mpeg2 ? 0.5f * s2 + 0.5f * s3 : 0.75f * s2 + 0.25f * s3;
      }
    }
    float o[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) yuv_decode_pixel(kc, yv[i], c[0][i], c[1][i], o + 3 * i);
    float* p = dst + ((size_t)row * w + x) * 3;
    if (cnt == 4 && ((size_t)p & 15) == 0) {
#pragma unroll
      for (int i = 0; i < 3; ++i) *(f32x4*)(p + 4 * i) = (f32x4){o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]};
    } else if (cnt == 4 && ((size_t)p & 7) == 0) {
#pragma unroll
      for (int i = 0; i < 6; ++i) *(f32x2*)(p + 2 * i) = (f32x2){o[2 * i], o[2 * i + 1]};
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i)
        if (i < 3 * cnt) p[i] = o[i];
    }
  }
}

// float tanh output t [n,h,w,3] -> 4:2:2 / 4:4:4 planes (fsr_image_to_yuv; the encode of DESIGN.md §6c at any depth 8..16), in the shape of
// image_to_i420_kernel and of the resampler's planar-YUV stage: a thread owns 4 columns x 1 row -- three 16-byte loads (narrower at the end
// of a row whose width is no multiple of 4), c = clamp((t + 1) / 2, 0, 1), then yuv_store_1x4.  4:2:2 also takes the clamped pixel of
// column x - 1 (column 0 at the left edge); the right neighbour of its last pair is inside the unit.  No LDS, no atomics.  Grid-stride
// over the n * h * ceil(w / 4) units (< 2^31: host checked).
template <typename C, int CHROMA>
__global__ __launch_bounds__(256) void image_to_yuv_kernel(const float* __restrict__ t, C* __restrict__ out, int n, int h, int w, int matrix,
                                                           int full, int depth) {
  const i420_coef kc = i420_coefs(matrix, full, sizeof(C) == 1 ? 8 : depth);
  const unsigned wq = (unsigned)(w + 3) >> 2;
  const unsigned units = (unsigned)n * (unsigned)h * wq;
  const size_t fsamples = (size_t)h * w + 2 * ((size_t)h * (size_t)(CHROMA == FSR_CHROMA_444 ? w : w >> 1));
  for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < units; u += gridDim.x * 256u) {
    const unsigned row = u / wq, xq = u - row * wq;
    const unsigned img = row / (unsigned)h, y = row - img * (unsigned)h;
    const int x = (int)xq * 4;
    const int cnt = w - x < 4 ? w - x : 4;
    const float* p = t + ((size_t)row * w + x) * 3;
    float q[12], v[12], vl[3] = {0.f, 0.f, 0.f};
    if (cnt == 4) {
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const f32x4_a4 e = *(const f32x4_a4*)(p + 4 * i);
#pragma unroll
        for (int k = 0; k < 4; ++k) q[4 * i + k] = e[k];
      }
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i) q[i] = i < 3 * cnt ? p[i] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) v[i] = fminf(fmaxf((q[i] + 1.f) / 2.f, 0.f), 1.f);
    if constexpr (CHROMA == FSR_CHROMA_422) {
      const float* l = x > 0 ? p - 3 : p;
#pragma unroll
      for (int k = 0; k < 3; ++k) vl[k] = fminf(fmaxf((l[k] + 1.f) / 2.f, 0.f), 1.f);
    }
    yuv_store_1x4<C, CHROMA>(kc, v, vl, out + (size_t)img * fsamples, h, w, (int)y, x, cnt);
  }
}

bool known_chroma(int chroma) { return chroma == FSR_CHROMA_420 || chroma == FSR_CHROMA_422 || chroma == FSR_CHROMA_444; }
unsigned capped_blocks(long long units) {
  const long long blocks = (units + 255) / 256;
  return (unsigned)(blocks > 4096 ? 4096 : blocks);
}

// ---- decode.  `who`: the entry point the messages name.  The 4:2:0 kernel walks pixels with 64-bit indices and stores single
// floats; the 4:2:2 / 4:4:4 kernel walks 4-pixel units with 32-bit indices and stores 16 bytes: the last two checks are its own.
int decode_check(const char* who, const void* frames, const float* img, int n, int h, int w, int chroma, int siting, int matrix,
                 int full_range) {
  if (!frames || !img || n <= 0 || h <= 0 || w <= 0) return fsr_fail(-1, "%s: bad argument", who);
  if ((siting != FSR_SITING_JPEG && siting != FSR_SITING_MPEG2) || (matrix != FSR_YUV_BT601 && matrix != FSR_YUV_BT709) ||
      (full_range != 0 && full_range != 1))
    return fsr_fail(-2, "%s: unknown siting %d / matrix %d / range %d", who, siting, matrix, full_range);
  if ((long long)h * w >= (1LL << 31) || (chroma != FSR_CHROMA_420 && (long long)n * h * w >= (1LL << 31)))
    return fsr_fail(-2, "%s: frames of 2^31 or more pixels are not supported", who);
  if (chroma != FSR_CHROMA_420 && ((size_t)img & 3) != 0) return fsr_fail(-2, "%s: misaligned tensor", who);
  return 0;
}
template <typename S>
void decode_kernel(int chroma, int layout, unsigned blocks, hipStream_t stream, const void* frames, float* img, int n, int h, int w, int mpeg2,
                   int matrix, int full_range, int depth) {
  const dim3 grid(blocks), block(256);
  const S* src = (const S*)frames;
  if (layout == FSR_LAYOUT_NV12)      // (4:2:0: the entry point has seen to it)
    hipLaunchKernelGGL((i420_to_image_kernel<S, true>), grid, block, 0, stream, src, img, n, h, w, mpeg2, matrix, full_range, depth);
  else if (chroma == FSR_CHROMA_420)
    hipLaunchKernelGGL(i420_to_image_kernel<S>, grid, block, 0, stream, src, img, n, h, w, mpeg2, matrix, full_range, depth);
  else if (chroma == FSR_CHROMA_422)
    hipLaunchKernelGGL((yuv_to_image_kernel<S, FSR_CHROMA_422>), grid, block, 0, stream, src, img, n, h, w, mpeg2, matrix, full_range, depth);
  else
    hipLaunchKernelGGL((yuv_to_image_kernel<S, FSR_CHROMA_444>), grid, block, 0, stream, src, img, n, h, w, mpeg2, matrix, full_range, depth);
}
// chroma is one of the three, depth in 8..16 and a 16-bit payload 2-byte aligned; layout FSR_LAYOUT_NV12 comes with 4:2:0 only: the
// entry points have seen to it
int yuv_to_image_launch(const char* who, const void* frames, float* img, int n, int h, int w, int chroma, int siting, int matrix,
                        int full_range, int depth, fsr_stream_t stream_, int layout = FSR_LAYOUT_PLANAR) {
  const bool c420 = chroma == FSR_CHROMA_420, deep = depth > 8;
  if (chroma == FSR_CHROMA_444) siting = FSR_SITING_JPEG;   // (no interpolation: ignored)
  if (int rc = decode_check(who, frames, img, n, h, w, chroma, siting, matrix, full_range)) return rc;
  const unsigned blocks = capped_blocks(c420 ? (long long)n * h * w : (long long)n * h * ((w + 3) / 4));
  const int mpeg2 = siting == FSR_SITING_MPEG2 ? 1 : 0;
  (deep ? decode_kernel<unsigned short> : decode_kernel<unsigned char>)(chroma, layout, blocks, (hipStream_t)stream_, frames, img, n, h, w, mpeg2,
                                                                        matrix, full_range, depth);
  if (layout == FSR_LAYOUT_NV12) {
    fsr_note_kernel("nv12_to_image_kernel<%s>", deep ? "u16" : "u8");
    return fsr_check_launch("nv12_to_image_kernel");
  }
  if (!c420) {
    fsr_note_kernel("yuv_to_image_kernel<%s,%s>", deep ? "u16" : "u8", chroma == FSR_CHROMA_422 ? "422" : "444");
    return fsr_check_launch("yuv_to_image_kernel");
  }
  if (deep) fsr_note_kernel("i420_to_image_kernel<%s>", "u16");   // (the 8-bit 4:2:0 decode leaves no note)
  return fsr_check_launch(deep ? "i420_to_image_kernel<u16>" : "i420_to_image_kernel");
}

// ---- encode
int encode_check(const char* who, const float* t, const void* out, int n, int h, int w, int chroma, int matrix, int full_range, int depth) {
  if (!t || !out) return fsr_fail(-1, "%s: null argument", who);
  if (n <= 0 || h <= 0 || w <= 0) return fsr_fail(-2, "%s: bad sizes (n %d, %d x %d)", who, n, h, w);
  if (int rc = fsr_yuv_out_check(who, "", chroma, h, w, matrix, full_range)) return rc;
  if (depth < 8 || depth > 16) return fsr_fail(-2, "%s: depth %d is outside 8..16", who, depth);
  if ((long long)h * w >= (1LL << 31) || (long long)n * h * w >= (1LL << 31))
    return fsr_fail(-2, "%s: frames of 2^31 or more pixels are not supported", who);
  if (((size_t)t & 3) != 0 || (depth > 8 && ((size_t)out & 1) != 0)) return fsr_fail(-2, "%s: misaligned tensor", who);
  return 0;
}
template <typename C>
void encode_kernel(int chroma, int layout, unsigned blocks, hipStream_t stream, const float* t, void* out, int n, int h, int w, int matrix,
                   int full_range, int depth) {
  const dim3 grid(blocks), block(256);
  if (layout == FSR_LAYOUT_NV12)      // (4:2:0: the entry point has seen to it)
    hipLaunchKernelGGL((image_to_i420_kernel<C, true>), grid, block, 0, stream, t, (C*)out, n, h, w, matrix, full_range, depth);
  else if (chroma == FSR_CHROMA_420)
    hipLaunchKernelGGL(image_to_i420_kernel<C>, grid, block, 0, stream, t, (C*)out, n, h, w, matrix, full_range, depth);
  else if (chroma == FSR_CHROMA_422)
    hipLaunchKernelGGL((image_to_yuv_kernel<C, FSR_CHROMA_422>), grid, block, 0, stream, t, (C*)out, n, h, w, matrix, full_range, depth);
  else
    hipLaunchKernelGGL((image_to_yuv_kernel<C, FSR_CHROMA_444>), grid, block, 0, stream, t, (C*)out, n, h, w, matrix, full_range, depth);
}
// chroma is one of the three; layout FSR_LAYOUT_NV12 comes with 4:2:0 only
int image_to_yuv_launch(const char* who, const float* t, int n, int h, int w, int chroma, int matrix, int full_range, int depth, void* out,
                        fsr_stream_t stream_, int layout = FSR_LAYOUT_PLANAR) {
  const bool c420 = chroma == FSR_CHROMA_420, deep = depth > 8;
  if (int rc = encode_check(who, t, out, n, h, w, chroma, matrix, full_range, depth)) return rc;
  const unsigned blocks = capped_blocks((long long)n * (c420 ? h / 2 : h) * ((w + 3) / 4));   // units of 4 columns x 2 rows (4:2:0) or x 1 row
  (deep ? encode_kernel<unsigned short> : encode_kernel<unsigned char>)(chroma, layout, blocks, (hipStream_t)stream_, t, out, n, h, w, matrix,
                                                                        full_range, depth);
  if (layout == FSR_LAYOUT_NV12) {
    fsr_note_kernel("image_to_nv12_kernel<%s>", deep ? "u16" : "u8");
    return fsr_check_launch("image_to_nv12_kernel");
  }
  if (c420) fsr_note_kernel("image_to_i420_kernel<%s>", deep ? "u16" : "u8");
  else fsr_note_kernel("image_to_yuv_kernel<%s,%s>", deep ? "u16" : "u8", chroma == FSR_CHROMA_422 ? "422" : "444");
  return fsr_check_launch(c420 ? "image_to_i420_kernel" : "image_to_yuv_kernel");
}

}  // namespace

int fsr_yuv_out_check(const char* who, const char* what, int chroma, int h, int w, int matrix, int full_range) {
  if (chroma == FSR_CHROMA_420 && ((h & 1) || (w & 1))) return fsr_fail(-2, "%s: I420 output needs even output extents (%d x %d)", who, h, w);
  if (chroma == FSR_CHROMA_422 && (w & 1)) return fsr_fail(-2, "%s: 4:2:2 output needs an even output width (%d)", who, w);
  if ((matrix != FSR_YUV_BT601 && matrix != FSR_YUV_BT709) || (full_range != 0 && full_range != 1))
    return fsr_fail(-2, "%s: %sunknown colour matrix %d / range %d", who, what, matrix, full_range);
  return 0;
}

extern "C" int fsr_yuv_to_image(const uint8_t* frames, float* img, int n, int h, int w, int chroma, int siting, int matrix, int full_range,
                                int depth, fsr_stream_t stream_) {
  if (!known_chroma(chroma)) return fsr_fail(-2, "fsr_yuv_to_image: unknown chroma subsampling %d", chroma);
  if (depth < 8 || depth > 16) return fsr_fail(-2, "fsr_yuv_to_image: depth %d is outside 8..16", depth);
  if (depth > 8 && ((size_t)frames & 1) != 0)
    return fsr_fail(-2, "fsr_yuv_to_image: the payloads of 16-bit samples must be 2-byte aligned");
  return yuv_to_image_launch("fsr_yuv_to_image", frames, img, n, h, w, chroma, siting, matrix, full_range, depth, stream_);
}

// The payload layout of the _ex entry points: known, and semi-planar with 4:2:0 only
int fsr_yuv_layout_check(const char* who, int chroma, int layout) {
  if (layout != FSR_LAYOUT_PLANAR && layout != FSR_LAYOUT_NV12) return fsr_fail(-2, "%s: unknown payload layout %d", who, layout);
  if (layout == FSR_LAYOUT_NV12 && chroma != FSR_CHROMA_420)
    return fsr_fail(-2, "%s: the semi-planar layout (NV12, P010 ...) is for 4:2:0 chroma only (chroma %d)", who, chroma);
  return 0;
}

extern "C" int fsr_yuv_to_image_ex(const uint8_t* frames, float* img, int n, int h, int w, int chroma, int layout, int siting, int matrix,
                                   int full_range, int depth, fsr_stream_t stream_) {
  if (!known_chroma(chroma)) return fsr_fail(-2, "fsr_yuv_to_image_ex: unknown chroma subsampling %d", chroma);
  if (int rc = fsr_yuv_layout_check("fsr_yuv_to_image_ex", chroma, layout)) return rc;
  if (depth < 8 || depth > 16) return fsr_fail(-2, "fsr_yuv_to_image_ex: depth %d is outside 8..16", depth);
  if (depth > 8 && ((size_t)frames & 1) != 0)
    return fsr_fail(-2, "fsr_yuv_to_image_ex: the payloads of 16-bit samples must be 2-byte aligned");
  return yuv_to_image_launch("fsr_yuv_to_image_ex", frames, img, n, h, w, chroma, siting, matrix, full_range, depth, stream_, layout);
}

extern "C" int fsr_image_to_yuv_ex(const float* t, int n, int h, int w, int chroma, int layout, int matrix, int full_range, int depth,
                                   void* out, fsr_stream_t stream_) {
  if (!known_chroma(chroma)) return fsr_fail(-2, "fsr_image_to_yuv_ex: unknown chroma subsampling %d", chroma);
  if (int rc = fsr_yuv_layout_check("fsr_image_to_yuv_ex", chroma, layout)) return rc;
  return image_to_yuv_launch("fsr_image_to_yuv_ex", t, n, h, w, chroma, matrix, full_range, depth, out, stream_, layout);
}

extern "C" int fsr_i420_to_image(const uint8_t* frames, float* img, int n, int h, int w, int siting, int matrix, int full_range,
                                 fsr_stream_t stream_) {
  return yuv_to_image_launch("fsr_i420_to_image", frames, img, n, h, w, FSR_CHROMA_420, siting, matrix, full_range, 8, stream_);
}

extern "C" int fsr_i420_to_image_deep(const uint8_t* frames, float* img, int n, int h, int w, int siting, int matrix, int full_range,
                                      int depth, fsr_stream_t stream_) {
  if (depth < 9 || depth > 16) return fsr_fail(-2, "fsr_i420_to_image_deep: depth %d is outside 9..16", depth);
  if (((size_t)frames & 1) != 0) return fsr_fail(-2, "fsr_i420_to_image_deep: the payloads of 16-bit samples must be 2-byte aligned");
  return yuv_to_image_launch("fsr_i420_to_image_deep", frames, img, n, h, w, FSR_CHROMA_420, siting, matrix, full_range, depth, stream_);
}

// (4:2:0 through this entry point has always been refused in fsr_image_to_i420's name)
extern "C" int fsr_image_to_yuv(const float* t, int n, int h, int w, int chroma, int matrix, int full_range, int depth, void* out,
                                fsr_stream_t stream_) {
  if (!known_chroma(chroma)) return fsr_fail(-2, "fsr_image_to_yuv: unknown chroma subsampling %d", chroma);
  return image_to_yuv_launch(chroma == FSR_CHROMA_420 ? "fsr_image_to_i420" : "fsr_image_to_yuv", t, n, h, w, chroma, matrix, full_range, depth,
                             out, stream_);
}

extern "C" int fsr_image_to_i420(const float* t, int n, int h, int w, int matrix, int full_range, int depth, void* out,
                                 fsr_stream_t stream_) {
  return image_to_yuv_launch("fsr_image_to_i420", t, n, h, w, FSR_CHROMA_420, matrix, full_range, depth, out, stream_);
}
