// Device helpers of the planar-YUV paths (the colour contract is DESIGN.md §6c): the encode of a tanh output to Y, Cb, Cr codes at
// 4:2:0, 4:2:2 and 4:4:4 and any depth 8..16, and the decode of such samples to the generator's input.  Included by yuv.hip (the decode
// and encode kernels), resample.hip (the planar stages of the resampler) and the head kernels that have the I420 epilogue
// (conv_igemm.hip, conv64_persistent.hip).
#pragma once
#include "fsr_common.h"

// ---- I420 output of a 3-channel tanh head (FSR_OUT_I420; the colour contract is DESIGN.md §6c).  A lane holds the (R, G, B) tanh
// values t[m][c] of two vertically adjacent pixels (rows 2k and 2k + 1, m = 0, 1) of one column; the lane `lane ^ 1` holds the
// neighbouring column of the same 2x2 block.  Every lane of the wave must call this (the shuffle), stores are guarded by the caller.
// Out: the two pixels' Y codes, and the block's Cb / Cr codes -- the mean of E_C over the block, C420jpeg siting -- in both lanes.
//   c = clamp((t + 1) / 2, 0, 1);  E_Y = Kr R + Kg G + Kb B;  E_Cb = (B - E_Y) / (2 (1 - Kb));  E_Cr = (R - E_Y) / (2 (1 - Kr))
//   limited: Y = 16 + 219 E_Y, C = 128 + 224 E_C;  full: Y = 255 E_Y, C = 128 + 255 E_C;  code = clamp(floor(v + 0.5), 0, 255)
// Deeper samples (9..16 bits, fsr_image_to_i420 and the 16-bit form of the resampler's I420 stage) use the same helpers with the
// depth's coefficients and a 16-bit code type C:  limited Y = (16 + 219 E_Y) 2^(d-8), C = (128 + 224 E_C) 2^(d-8);
// full Y = (2^d - 1) E_Y, C = 2^(d-1) + (2^d - 1) E_C;  code = clamp(floor(v + 0.5), 0, 2^d - 1).  depth = 8 (the default, a
// constant in the head kernels) gives the numbers above.
template <typename C = unsigned char>
__device__ __forceinline__ C yuv_code(float v, float cmax = 255.f) { return (C)fminf(fmaxf(floorf(v + 0.5f), 0.f), cmax); }
// The per-pixel and per-block parts, shared with the resampler (resample.hip), whose threads hold whole 2x2 blocks:
//   i420_pixel : clamped (R, G, B) in [0, 1] -> the pixel's Y code; db = B - E_Y, dr = R - E_Y
//   i420_chroma: the sums of db and dr over the four pixels of a block (the vertical pair first, then the two columns) -> Cb, Cr codes
struct i420_coef {
  float kr, kg, kb, ys, yo, cs, co, cmax;
};
__device__ __forceinline__ i420_coef i420_coefs(int matrix, int full, int depth = 8) {
  const float kr = matrix == FSR_YUV_BT709 ? 0.2126f : 0.299f, kb = matrix == FSR_YUV_BT709 ? 0.0722f : 0.114f;
  const float kg = 1.f - kr - kb;
  const float up = (float)(1 << (depth - 8)), top = (float)((1 << depth) - 1);   // exact: depth <= 16
  const float ys = full ? top : 219.f * up, yo = full ? 0.f : 16.f * up, cs = full ? top : 224.f * up;
  return i420_coef{kr, kg, kb, ys, yo, cs, 128.f * up, top};
}
template <typename C = unsigned char>
__device__ __forceinline__ C i420_pixel(const i420_coef& k, float r, float g, float b, float& db, float& dr) {
  const float ey = k.kr * r + k.kg * g + k.kb * b;
  db = b - ey;
  dr = r - ey;
  return yuv_code<C>(k.yo + k.ys * ey, k.cmax);
}
template <typename C>
__device__ __forceinline__ void i420_chroma(const i420_coef& k, float sb, float sr, C& cb, C& cr) {
  cb = yuv_code<C>(k.co + k.cs * (sb * 0.25f / (2.f * (1.f - k.kb))), k.cmax);
  cr = yuv_code<C>(k.co + k.cs * (sr * 0.25f / (2.f * (1.f - k.kr))), k.cmax);
}
__device__ __forceinline__ void i420_quad(const float (&t)[2][3], int matrix, int full, unsigned char (&y)[2], unsigned char& cb,
                                          unsigned char& cr) {
  const i420_coef k = i420_coefs(matrix, full);
  float sb = 0.f, sr = 0.f;   // sums of B - E_Y and R - E_Y over the lane's two pixels
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const float r = fminf(fmaxf((t[m][0] + 1.f) * 0.5f, 0.f), 1.f);
    const float g = fminf(fmaxf((t[m][1] + 1.f) * 0.5f, 0.f), 1.f);
    const float b = fminf(fmaxf((t[m][2] + 1.f) * 0.5f, 0.f), 1.f);
    float db, dr;
    y[m] = i420_pixel(k, r, g, b, db, dr);
    sb += db;
    sr += dr;
  }
  sb += __shfl_xor(sb, 1, 64);
  sr += __shfl_xor(sr, 1, 64);
  i420_chroma(k, sb, sr, cb, cr);
}
// The chroma store of the even-column lane of a block at rows gy, gy + 1 (gy even), column gx (even) of an 8-bit frame `o` of fow
// columns whose Y plane holds `plane` bytes: one byte into each of the Cb and Cr planes (FSR_OUT_I420), or -- nv12: FSR_OUT_NV12,
// DESIGN.md §6f -- the (Cb, Cr) pair into the one chroma plane of fow bytes per row, as one 2-byte store where the address allows.
__device__ __forceinline__ void i420_store_chroma(unsigned char* o, size_t plane, int fow, int gy, int gx, unsigned char cb, unsigned char cr,
                                                  bool nv12) {
  if (nv12) {
    unsigned char* q = o + plane + (size_t)(gy >> 1) * fow + gx;
    if (((size_t)q & 1) == 0) {
      *(unsigned short*)q = (unsigned short)((unsigned)cb | ((unsigned)cr << 8));
    } else {
      q[0] = cb;
      q[1] = cr;
    }
  } else {
    const size_t c = (size_t)(gy >> 1) * (fow >> 1) + (gx >> 1);
    o[plane + c] = cb;
    o[plane + (plane >> 2) + c] = cr;
  }
}

// ---- I420 planes from a thread that holds 4 columns x 2 rows -- two whole 2x2 blocks, no shuffle (the resampler's I420 stage and
// fsr_image_to_i420).  C = unsigned char (8-bit samples) or unsigned short (9..16 bits, little-endian, the value in the low bits).
// `count` (1..4) codes b[0..count) to p: one 4 * sizeof(C)-byte store, halves of it or single codes, whatever p's alignment allows
template <typename C>
__device__ __forceinline__ void store_codes4(C* p, const C (&b)[4], int count) {
  constexpr int S = 8 * (int)sizeof(C);
  typedef typename std::conditional<sizeof(C) == 1, unsigned short, unsigned>::type pair_t;
  const size_t ad = (size_t)p;
  const pair_t lo = (pair_t)((pair_t)b[0] | ((pair_t)b[1] << S)), hi = (pair_t)((pair_t)b[2] | ((pair_t)b[3] << S));
  if (count == 4 && (ad & (4 * sizeof(C) - 1)) == 0) {
    if constexpr (sizeof(C) == 1) *(unsigned*)p = (unsigned)lo | ((unsigned)hi << 16);
    else *(u32x2*)p = (u32x2){lo, hi};
  } else if ((ad & (2 * sizeof(C) - 1)) == 0 && (count & 1) == 0) {
    *(pair_t*)p = lo;
    if (count == 4) *(pair_t*)(p + 2) = hi;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < count) p[i] = b[i];
  }
}
// v[m][3 c + ch]: clamped (R, G, B) in [0, 1] of row yo + m, column xg + c of a frame of oh x ow (both even; yo, xg even); cnt = 2 or 4
// valid columns.  Per column the vertical pair first, then the two columns of a block (i420_quad's order of the chroma sum).
// SEMI: the semi-planar payload -- the same codes, shifted left by sh = 16 - depth for 16-bit samples (the code in the
// HIGH bits: P010, P012, P016; sh = 0 for NV12's bytes), Cb0, Cr0, Cb1, Cr1 into the one chroma plane of ow samples per row as ONE
// store_codes4 where the planar form makes 2 + 2 stores.
template <typename C, bool SEMI = false>
__device__ __forceinline__ void i420_store_2x4(const i420_coef& kc, const float (&v)[2][12], C* frame, int oh, int ow, int yo, int xg,
                                               int cnt, int sh = 0) {
  const size_t plane = (size_t)oh * ow, cw = (size_t)(ow >> 1), cplane = (size_t)(oh >> 1) * cw;
  C yv[2][4], cb[2], cr[2];
  float sb[4], sr[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    sb[c] = 0.f;
    sr[c] = 0.f;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      float db, dr;
      yv[m][c] = i420_pixel<C>(kc, v[m][3 * c], v[m][3 * c + 1], v[m][3 * c + 2], db, dr);
      sb[c] += db;
      sr[c] += dr;
    }
  }
#pragma unroll
  for (int p = 0; p < 2; ++p) i420_chroma(kc, sb[2 * p] + sb[2 * p + 1], sr[2 * p] + sr[2 * p + 1], cb[p], cr[p]);
  if constexpr (SEMI) {
    C cc[4] = {(C)(cb[0] << sh), (C)(cr[0] << sh), (C)(cb[1] << sh), (C)(cr[1] << sh)};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      yv[0][c] = (C)(yv[0][c] << sh);
      yv[1][c] = (C)(yv[1][c] << sh);
    }
    store_codes4(frame + (size_t)yo * ow + xg, yv[0], cnt);
    store_codes4(frame + (size_t)(yo + 1) * ow + xg, yv[1], cnt);
    store_codes4(frame + plane + (size_t)(yo >> 1) * ow + xg, cc, cnt);   // (cnt = 2: one pair, cnt = 4: two)
    return;
  }
  store_codes4(frame + (size_t)yo * ow + xg, yv[0], cnt);
  store_codes4(frame + (size_t)(yo + 1) * ow + xg, yv[1], cnt);
  C* c0 = frame + plane + (size_t)(yo >> 1) * cw + (xg >> 1);
  if (cnt == 4 && ((size_t)c0 & (2 * sizeof(C) - 1)) == 0 && (cplane & 1) == 0) {
    typedef typename std::conditional<sizeof(C) == 1, unsigned short, unsigned>::type pair_t;
    *(pair_t*)c0 = (pair_t)((pair_t)cb[0] | ((pair_t)cb[1] << (8 * sizeof(C))));
    *(pair_t*)(c0 + cplane) = (pair_t)((pair_t)cr[0] | ((pair_t)cr[1] << (8 * sizeof(C))));
  } else {
    c0[0] = cb[0];
    c0[cplane] = cr[0];
    if (cnt == 4) {
      c0[1] = cb[1];
      c0[cplane + 1] = cr[1];
    }
  }
}

// ---- 4:2:2 and 4:4:4 planes (fsr_image_to_yuv and the resampler's planar-YUV stage).  CHROMA is FSR_CHROMA_422 or
// FSR_CHROMA_444; Y per pixel as above (i420_pixel).
//   yuv444_chroma: one pixel's db = B - E_Y, dr = R - E_Y -> its Cb, Cr codes
//   yuv422_chroma: db / dr of the pixels left of, at and right of an even luma column -> the Cb, Cr codes co-sited with it (what a C422
//                  stream declares): s = (left + right) + 2 centre, then i420_chroma's scaling s * 0.25 / (2 (1 - K))
template <typename C>
__device__ __forceinline__ void yuv444_chroma(const i420_coef& k, float db, float dr, C& cb, C& cr) {
  cb = yuv_code<C>(k.co + k.cs * (db / (2.f * (1.f - k.kb))), k.cmax);
  cr = yuv_code<C>(k.co + k.cs * (dr / (2.f * (1.f - k.kr))), k.cmax);
}
template <typename C>
__device__ __forceinline__ void yuv422_chroma(const i420_coef& k, float bl, float bc, float br, float rl, float rc, float rr, C& cb, C& cr) {
  i420_chroma(k, (bl + br) + 2.f * bc, (rl + rr) + 2.f * rc, cb, cr);
}
// A thread that holds 4 columns x 1 row.  v[3 c + ch]: clamped (R, G, B) in [0, 1] of row yo, column xg + c (xg a multiple of 4) of a
// frame of oh x ow; cnt valid columns (1..4; 2 or 4 for 4:2:2, whose ow is even -- so the right neighbour of a chroma sample is always
// a column of the same thread).  vl (4:2:2 only): the clamped (R, G, B) of column max(xg - 1, 0), the left neighbour of the first pair.
// Planes: Y [oh][ow], then Cb and Cr [oh][ow / 2] (4:2:2) or [oh][ow] (4:4:4).
template <typename C, int CHROMA>
__device__ __forceinline__ void yuv_store_1x4(const i420_coef& kc, const float (&v)[12], const float (&vl)[3], C* frame, int oh, int ow,
                                              int yo, int xg, int cnt) {
  const size_t plane = (size_t)oh * ow;
  C yv[4], cb[4] = {0, 0, 0, 0}, cr[4] = {0, 0, 0, 0};
  float db[4], dr[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) yv[c] = i420_pixel<C>(kc, v[3 * c], v[3 * c + 1], v[3 * c + 2], db[c], dr[c]);
  store_codes4(frame + (size_t)yo * ow + xg, yv, cnt);
  if constexpr (CHROMA == FSR_CHROMA_444) {
#pragma unroll
    for (int c = 0; c < 4; ++c) yuv444_chroma(kc, db[c], dr[c], cb[c], cr[c]);
    C* c0 = frame + plane + (size_t)yo * ow + xg;
    store_codes4(c0, cb, cnt);
    store_codes4(c0 + plane, cr, cnt);
  } else {
    float dbl, drl;
    i420_pixel<C>(kc, vl[0], vl[1], vl[2], dbl, drl);
    yuv422_chroma(kc, dbl, db[0], db[1], drl, dr[0], dr[1], cb[0], cr[0]);
    yuv422_chroma(kc, db[1], db[2], db[3], dr[1], dr[2], dr[3], cb[1], cr[1]);
    const size_t cw = (size_t)(ow >> 1), cplane = (size_t)oh * cw;
    C* c0 = frame + plane + (size_t)yo * cw + (xg >> 1);
    store_codes4(c0, cb, cnt >> 1);
    store_codes4(c0 + cplane, cr, cnt >> 1);
  }
}

// ---- decode (yuv.hip).  yuv_decode_coefs: i420_coefs' values for the decode kernels (cmax unused), in the order those kernels have
// always computed them.  yuv_decode_pixel: the samples of one pixel -- Y, and Cb, Cr interpolated to its position -- -> o[0..3) = 2 c - 1
// of the inverse matrix's R, G, B, each clamped to [0, 1]
__device__ __forceinline__ i420_coef yuv_decode_coefs(int matrix, int full, int d) {
  const float kr = matrix == FSR_YUV_BT709 ? 0.2126f : 0.299f, kb = matrix == FSR_YUV_BT709 ? 0.0722f : 0.114f;
  const float kg = 1.f - kr - kb;
  const float up = (float)(1 << (d - 8)), top = (float)((1 << d) - 1), co = 128.f * up;
  const float ys = full ? top : 219.f * up, yo = full ? 0.f : 16.f * up, cs = full ? top : 224.f * up;
  return i420_coef{kr, kg, kb, ys, yo, cs, co, top};
}
__device__ __forceinline__ void yuv_decode_pixel(const i420_coef& k, float yv, float cbv, float crv, float* o) {
  const float ey = (yv - k.yo) / k.ys, ecb = (cbv - k.co) / k.cs, ecr = (crv - k.co) / k.cs;
  const float r = ey + 2.f * (1.f - k.kr) * ecr, b = ey + 2.f * (1.f - k.kb) * ecb;
  const float g = (ey - k.kr * r - k.kb * b) / k.kg;
  o[0] = 2.f * fminf(fmaxf(r, 0.f), 1.f) - 1.f;
  o[1] = 2.f * fminf(fmaxf(g, 0.f), 1.f) - 1.f;
  o[2] = 2.f * fminf(fmaxf(b, 0.f), 1.f) - 1.f;
}
