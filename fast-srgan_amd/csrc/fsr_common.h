// Shared device-side helpers for the gfx950 (CDNA4) Fast-SRGAN kernels.
//
// Conventions used by every kernel in this directory:
//   * activations are NHWC ("pixel-major, channels contiguous"), element type
//     T = float (exact-f32 parity mode) or bf16 stored as unsigned short;
//   * a wavefront is 64 lanes; workgroups are 256 threads (4 waves, one per SIMD);
//   * MFMA shapes: v_mfma_f32_16x16x32_bf16 (bf16 mode) and v_mfma_f32_16x16x4_f32
//     (f32 mode, exact fmaf-chain numerics at the f32 vector rate);
//   * accumulator layout (both shapes): lane l, reg r -> row (l>>4)*4+r, col l&15.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

typedef unsigned short bf16_t;  // raw bf16 bits
typedef _Float16 f16_t;         // IEEE half (FSR_F16: the fp16-MFMA mode of BASELINE configs[4])

typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));  // one 16-byte staging unit
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8_hw __attribute__((ext_vector_type(8)));

#ifndef FSR_LDS_PTR
#define FSR_LDS_PTR(T, p) ((__attribute__((address_space(3))) T*)(p))
#endif
// gfx9 counts loads AND stores on vmcnt, and the two kinds complete out of order with each other, so the compiler waits
// vmcnt(0) -- for every store in flight as well -- wherever a loaded register is first used.  A persistent kernel that
// prefetches the next tile before its epilogue therefore waits for the prefetch HERE, before the epilogue's stores are
// issued (the loads have had the whole tile to land): the later use of the prefetched registers then needs no wait and
// the stores drain under the next tile.   0x0F70 = vmcnt(0), expcnt / lgkmcnt untouched.
#ifndef FSR_WAIT_LOADS
#define FSR_WAIT_LOADS() __builtin_amdgcn_s_waitcnt(0x0F70)
#endif
#ifndef FSR_GLOBAL_PTR
#define FSR_GLOBAL_PTR(T, p) ((__attribute__((address_space(1))) T*)(p))
#endif
// One LDS-DMA piece: every lane copies 16 bytes from ITS global address to (LDS address) + 16 * lane (global_load_lds_dwordx4).
// Issued from inline asm ON PURPOSE.  hipcc's waitcnt pass treats the builtin as a FLAT operation that touches two address
// spaces ("pending flat"): while one is in flight on vmcnt -- by design the whole stage -- every s_waitcnt lgkmcnt it emits is
// forced to 0, so software-pipelined ds_read -> MFMA sequences collapse into {reads, wait for ALL of them, MFMAs}.  Hidden in
// asm, the DMA is invisible to that pass: the fragment reads get counted lgkmcnt(N) waits, and the kernel waits for its DMA
// pieces itself (FSR_WAIT_DMA before the barrier that publishes the buffer).
#ifndef FSR_WAIT_DMA
#define FSR_WAIT_DMA() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#endif
// The piece is addressed the way the hardware wants it: destination = a 32-bit LDS byte address (FSR_LDS_ADDR of a shared
// pointer, taken ONCE per kernel, plus integer offsets -- every generic-pointer -> LDS cast in a loop costs a null check and
// 64-bit scalar adds), source = a wave-uniform 64-bit base in SGPRs + a 32-bit per-lane byte offset (no vector 64-bit add).
// M0 is declared clobbered instead of saved and restored.
#ifndef FSR_GLDS16_AT
typedef unsigned fsr_lds_addr_t;
#define FSR_LDS_ADDR(p) ((unsigned)(size_t)FSR_LDS_PTR(char, (p)))
__device__ __forceinline__ void fsr_glds16_at(const void* gsrc, unsigned lds_addr) {
  const unsigned dst = __builtin_amdgcn_readfirstlane(lds_addr);
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gsrc), "s"(dst) : "memory", "m0");
}
__device__ __forceinline__ void fsr_glds16_sat(const void* sbase, unsigned voff, unsigned lds_addr) {
  const unsigned dst = __builtin_amdgcn_readfirstlane(lds_addr);
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %0" ::"s"(sbase), "v"(voff), "s"(dst) : "memory", "m0");
}
#define FSR_GLDS16_AT(g, a) fsr_glds16_at((g), (a))
#define FSR_GLDS16_SAT(sb, vo, a) fsr_glds16_sat((sb), (vo), (a))
#endif
// ---- buffer-addressed LDS-DMA (conv_tall3.hip).  buffer_load_dwordx4 ... offen lds: every lane copies 16 bytes from
// (descriptor base + voffset + soffset) to (LDS address in M0) + 16 * lane; a lane whose voffset lies beyond the descriptor's
// byte count gets ZEROS (hardware range check on voffset only -- soffset is not checked): image borders need no zero page and
// no branch.  Issued from inline asm for the same reason as FSR_GLDS16_*: hipcc never sees the piece, so its own
// lgkmcnt / vmcnt bookkeeping stays counted, and the kernel waits for its pieces itself (FSR_WAIT_VM(n): at most n of the
// YOUNGEST vector-memory operations of this wave are still in flight; loads retire in order).
#ifndef FSR_BLDS16
struct fsr_buf_t { u32x4 v; };
__device__ __forceinline__ fsr_buf_t fsr_make_buf(const void* p, unsigned bytes) {
  const unsigned long long x = (unsigned long long)(size_t)p;
  fsr_buf_t b;
  b.v = (u32x4){(unsigned)x, (unsigned)(x >> 32) & 0xffffu, bytes, 0x00020000u};   // raw buffer, stride 0, 32-bit data format
  return b;
}
__device__ __forceinline__ void fsr_blds16(fsr_buf_t b, unsigned voff, unsigned soff, unsigned lds_addr) {
  asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %0, %2 offen lds" ::"s"(b.v), "v"(voff), "s"(soff), "s"(lds_addr)
               : "memory", "m0");
}
#define FSR_BLDS16(b, vo, so, a) fsr_blds16((b), (vo), (so), (a))
#define FSR_WAIT_VM(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory")
#define FSR_WAIT_LGKM0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#define FSR_BARRIER() __builtin_amdgcn_s_barrier()
#endif
// Orders the LDS traffic of ONE wave around a wave-private exchange (write in one lane mapping, read back in another): the
// hardware runs a wave's LDS instructions in order, so this only has to stop the compiler from moving them across it.
#ifndef FSR_WAVE_SYNC
#define FSR_WAVE_SYNC() __builtin_amdgcn_wave_barrier()
#endif
// Bulk output stores.  FSR_NT (compile-time bit mask, one bit per kernel family) puts the non-temporal hint on them: a conv
// epilogue streams hundreds of MB through 4 MB L2s whose hot content is the filter and halo lines the LDS-DMA keeps re-reading
// (measured on conv_s2d3.hip's 128-channel layer: +8..10 % with `nt` stores, profiles/r04_nt_stores.txt).
//   1 conv_tall3   2 conv64 family   4 first-layer kernels   8 elementwise   16 conv_s2d3   32 conv_igemm
#ifndef FSR_NT
#define FSR_NT 20
#endif
template <int BIT, typename V>
__device__ __forceinline__ void fsr_st(V* p, V v) {
  if constexpr ((FSR_NT & BIT) != 0) __builtin_nontemporal_store(v, p);
  else *p = v;
}
// A register "use" with no instruction: pins where the compiler places its s_waitcnt for a load's result.
#ifndef FSR_TOUCH
#define FSR_TOUCH(v) asm volatile("" : "+v"(v))
#endif

// dtype / activation / mode enums come from the public ABI header
#include "fsr_hip.h"

__device__ __forceinline__ float bf2f(bf16_t h) {
  return __uint_as_float(((unsigned)h) << 16);
}
// round-to-nearest-even (v_cvt_pk_bf16_f32 on gfx950)
typedef __bf16 bf16x2_hw __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ bf16_t f2bf(float f) { return __builtin_bit_cast(unsigned short, (__bf16)f); }
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
  const f32x2 v = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_hw));
}

template <typename T> struct ElemIO;
template <> struct ElemIO<float> {
  static __device__ __forceinline__ float ld(const float* p) { return *p; }
  static __device__ __forceinline__ void st(float* p, float v) { *p = v; }
};
template <> struct ElemIO<bf16_t> {
  static __device__ __forceinline__ float ld(const bf16_t* p) { return bf2f(*p); }
  static __device__ __forceinline__ void st(bf16_t* p, float v) { *p = f2bf(v); }
};
template <> struct ElemIO<f16_t> {
  static __device__ __forceinline__ float ld(const f16_t* p) { return (float)*p; }
  static __device__ __forceinline__ void st(f16_t* p, float v) { *p = (f16_t)v; }
};

__device__ __forceinline__ f32x4 mfma_bf16_16x16x32(s16x8 a, s16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_hw, a),
                                                 __builtin_bit_cast(bf16x8_hw, b), c, 0, 0, 0);
}
// ---- 16-bit storage types, generically (T = bf16_t or f16_t): two elements of a packed 32-bit word to float, two floats to
// a packed word (round to nearest even), one MFMA step v_mfma_f32_16x16x32_{bf16,f16}.
typedef _Float16 f16x8_hw __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2_hw __attribute__((ext_vector_type(2)));
template <typename T> struct Num16;
template <> struct Num16<bf16_t> {
  static __device__ __forceinline__ float lo(unsigned w) { return __uint_as_float(w << 16); }
  static __device__ __forceinline__ float hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }
  static __device__ __forceinline__ unsigned pack(float a, float b) { return pack_bf16x2(a, b); }
  static __device__ __forceinline__ f32x4 mfma(s16x8 a, s16x8 b, f32x4 c) { return mfma_bf16_16x16x32(a, b, c); }
};
template <> struct Num16<f16_t> {
  static __device__ __forceinline__ float lo(unsigned w) { return (float)__builtin_bit_cast(f16x2_hw, w)[0]; }
  static __device__ __forceinline__ float hi(unsigned w) { return (float)__builtin_bit_cast(f16x2_hw, w)[1]; }
  static __device__ __forceinline__ unsigned pack(float a, float b) {
    const f16x2_hw v = {(_Float16)a, (_Float16)b};
    return __builtin_bit_cast(unsigned, v);
  }
  static __device__ __forceinline__ f32x4 mfma(s16x8 a, s16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_hw, a), __builtin_bit_cast(f16x8_hw, b), c, 0, 0, 0);
  }
};
template <typename T> __device__ __forceinline__ unsigned pack2(float a, float b) { return Num16<T>::pack(a, b); }
template <typename T> __device__ __forceinline__ float cvt_lo(unsigned w) { return Num16<T>::lo(w); }
template <typename T> __device__ __forceinline__ float cvt_hi(unsigned w) { return Num16<T>::hi(w); }
template <typename T> __device__ __forceinline__ f32x4 mfma16(s16x8 a, s16x8 b, f32x4 c) { return Num16<T>::mfma(a, b, c); }

// ---- FSR_X3, the split-bf16 storage type (include/fsr_hip.h): a logical element is 4 bytes; per pixel and per group of 32
// channels the tensor holds 64 bytes of hi[32] (bf16(v)) followed by 64 bytes of lo[32] (bf16(v - hi)).  x3_t is only a
// pointer type: `p + e` is the logical element e (4-byte steps), and the helpers below turn that pointer into the two physical
// addresses -- byte b of the logical (float-like) layout lies in the 128-byte block b & ~127; its hi half word sits at
// (b & 127) / 2 inside the block and its lo half word 64 bytes later.  Tensor bases are 128-byte aligned (host checked), and
// every vector access covers 4 or 8 consecutive channels of one group, so a V16 unit is two 16-byte accesses 64 bytes apart.
struct x3_t { unsigned raw; };
static_assert(sizeof(x3_t) == 4, "x3_t is a 4-byte element");
template <typename P> __device__ __forceinline__ P* x3_hi_ptr(P* p) {
  const size_t b = (size_t)p;
  return (P*)((b & ~(size_t)127) | ((b & (size_t)127) >> 1));
}
// two floats -> packed bf16 pair of the hi parts and packed pair of the lo parts (both round to nearest even)
__device__ __forceinline__ void x3_split2(float a, float b, unsigned& hi, unsigned& lo) {
  hi = pack_bf16x2(a, b);
  lo = pack_bf16x2(a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u));
}
__device__ __forceinline__ float x3_join_lo(unsigned hi, unsigned lo) { return __uint_as_float(hi << 16) + __uint_as_float(lo << 16); }
__device__ __forceinline__ float x3_join_hi(unsigned hi, unsigned lo) { return __uint_as_float(hi & 0xffff0000u) + __uint_as_float(lo & 0xffff0000u); }
template <> struct ElemIO<x3_t> {
  static __device__ __forceinline__ float ld(const x3_t* p) {
    const bf16_t* h = (const bf16_t*)x3_hi_ptr(p);
    return bf2f(h[0]) + bf2f(h[32]);
  }
  static __device__ __forceinline__ void st(x3_t* p, float v) {
    bf16_t* h = (bf16_t*)x3_hi_ptr(p);
    const bf16_t hi = f2bf(v);
    h[0] = hi;
    h[32] = f2bf(v - bf2f(hi));
  }
};
// 4 consecutive channels (one lane's accumulator tile row): two 8-byte accesses
__device__ __forceinline__ void x3_st4(x3_t* p, f32x4 v) {
  unsigned h0, l0, h1, l1;
  x3_split2(v[0], v[1], h0, l0);
  x3_split2(v[2], v[3], h1, l1);
  char* h = (char*)x3_hi_ptr(p);
  *(u32x2*)h = (u32x2){h0, h1};
  *(u32x2*)(h + 64) = (u32x2){l0, l1};
}
__device__ __forceinline__ f32x4 x3_ld4(const x3_t* p) {
  const char* h = (const char*)x3_hi_ptr(p);
  const u32x2 hi = *(const u32x2*)h, lo = *(const u32x2*)(h + 64);
  return (f32x4){x3_join_lo(hi.x, lo.x), x3_join_hi(hi.x, lo.x), x3_join_lo(hi.y, lo.y), x3_join_hi(hi.y, lo.y)};
}

// ---- one 16-byte unit of a storage type viewed as floats (the HBM-bound kernels move one unit per lane and access):
// 8 elements of a 16-bit type, 4 floats, or 8 x3 elements (16 bytes of hi + 16 bytes of lo)
template <typename T, int NTBIT = 0> struct V16 {   // the 16-bit storage types (bf16_t, f16_t)
  static constexpr int N = 8;
  static __device__ __forceinline__ void ld(const T* p, float (&v)[8]) {
    const u32x4 t = *(const u32x4*)p;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = cvt_lo<T>(t[i]);
      v[2 * i + 1] = cvt_hi<T>(t[i]);
    }
  }
  static __device__ __forceinline__ void st(T* p, const float (&v)[8]) {
    u32x4 t;
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = pack2<T>(v[2 * i], v[2 * i + 1]);
    fsr_st<NTBIT>((u32x4*)p, t);
  }
};
template <int NTBIT> struct V16<float, NTBIT> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void ld(const float* p, float (&v)[4]) {
    const f32x4 t = *(const f32x4*)p;
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  }
  static __device__ __forceinline__ void st(float* p, const float (&v)[4]) {
    *(f32x4*)p = (f32x4){v[0], v[1], v[2], v[3]};
  }
};
template <int NTBIT> struct V16<x3_t, NTBIT> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void ld(const x3_t* p, float (&v)[8]) {
    const char* h = (const char*)x3_hi_ptr(p);
    const u32x4 hi = *(const u32x4*)h, lo = *(const u32x4*)(h + 64);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = x3_join_lo(hi[i], lo[i]);
      v[2 * i + 1] = x3_join_hi(hi[i], lo[i]);
    }
  }
  static __device__ __forceinline__ void st(x3_t* p, const float (&v)[8]) {
    u32x4 hi, lo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned a, b;
      x3_split2(v[2 * i], v[2 * i + 1], a, b);
      hi[i] = a;
      lo[i] = b;
    }
    char* h = (char*)x3_hi_ptr(p);
    fsr_st<NTBIT>((u32x4*)h, hi);
    fsr_st<NTBIT>((u32x4*)(h + 64), lo);
  }
};

__device__ __forceinline__ f32x4 mfma_f32_16x16x4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// v > 0 ? v : v * slope (ReLU: slope 0, identity: slope 1).  NOT max(v, 0) + slope * min(v, 0): v_max_f32 / v_min_f32 return the
// non-NaN operand, so that form turns a NaN into 0 -- in a DATA-GRADIENT epilogue that silently zeroed the NaNs of an overflowed fp16
// backward on their way to the optimizer's non-finite check (round 6: the x3v mode's fp16 perceptual branch; found by
// tests/test_x3.py::test_x3v_overflow_in_the_fp16_perceptual_branch_skips_the_iteration).  Same result on every finite input.
__device__ __forceinline__ float act_slope(float v, float slope) { return v > 0.f ? v : v * slope; }

__device__ __forceinline__ float act_apply(float v, int act, float slope) {
  switch (act) {
    case FSR_ACT_RELU: return v > 0.f ? v : 0.f;
    case FSR_ACT_LEAKY:
    case FSR_ACT_PRELU: return v > 0.f ? v : v * slope;
    case FSR_ACT_TANH: return tanhf(v);
    default: return v;
  }
}

// inference.py:53-56 on one head output y = tanh(z) in (-1,1): ((y + 1) / 2) * 255 in f32, then the C cast to uint8
// (truncation toward zero; the value lies in [0, 255))
__device__ __forceinline__ unsigned char image_u8(float y) {
  const float w = ((y + 1.f) / 2.f) * 255.f;
  return (unsigned char)w;
}

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
template <typename C>
__device__ __forceinline__ void i420_store_2x4(const i420_coef& kc, const float (&v)[2][12], C* frame, int oh, int ow, int yo, int xg,
                                               int cnt) {
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

// sum over the 64 lanes of a wave; every lane gets the total
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// compile-time loop: f(std::integral_constant<int, I>) for I in [I0, N).  Keeps every index into
// register arrays (accumulators) a constant -- a runtime index sends the whole array to scratch.
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// XCD-aware bijective remap of a linear workgroup id: consecutive logical ids land on
// the same XCD (dispatcher places hardware block b on XCD b % 8), so neighbouring tiles
// that share halo rows / filter slices hit the same 4 MiB L2. Speed only, never correctness.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7;
  const int xcd = bid & 7, idx = bid >> 3;
  const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + idx;
}
