// Host-side helpers shared by the C-ABI entry points (error reporting, launch checks).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include "fsr_hip.h"

struct ConvKArgs;

// Records a message retrievable through fsr_last_error() and returns `code` (negative).
int fsr_fail(int code, const char* fmt, ...);
// Returns 0 if the most recent launch was accepted by the runtime, else records and returns -3.
int fsr_check_launch(const char* what);
// Records the name of the kernel configuration a dispatch picked (fsr_last_kernel(): per-kernel attribution in bench.py).
void fsr_note_kernel(const char* fmt, ...);

// ---- dtype dispatch of the streaming kernels' host code (elementwise.hip, losses.hip): T is the element type inside the braces.
// The last branch is float: the caller has refused unknown dtypes (fsr_known_dtype, check_c) BEFORE it dispatches.
#define FSR_DISPATCH_T(dtype, ...)                    \
  if ((dtype) == FSR_BF16) {                          \
    typedef bf16_t T;                                 \
    __VA_ARGS__                                       \
  } else if ((dtype) == FSR_F16) {                    \
    typedef f16_t T;                                  \
    __VA_ARGS__                                       \
  } else if ((dtype) == FSR_X3) {                     \
    typedef x3_t T;                                   \
    __VA_ARGS__                                       \
  } else {                                            \
    typedef float T;                                  \
    __VA_ARGS__                                       \
  }
template <typename T> inline T* P(void* p) { return (T*)p; }
template <typename T> inline const T* P(const void* p) { return (const T*)p; }

inline bool fsr_known_dtype(int dtype) { return dtype == FSR_F32 || dtype == FSR_BF16 || dtype == FSR_F16 || dtype == FSR_X3; }
inline int fsr_unit_elems(int dtype) { return dtype != FSR_F32 ? 8 : 4; }                     // elements per 16-byte unit
inline int fsr_multiple(int dtype) { return dtype == FSR_X3 ? 32 : fsr_unit_elems(dtype); }   // x3: whole hi / lo groups of 32 channels
inline int check_c(const char* what, int dtype, int c) {
  if (!fsr_known_dtype(dtype)) return fsr_fail(-2, "%s: unknown dtype %d", what, dtype);
  if (c <= 0 || c % fsr_multiple(dtype) != 0) return fsr_fail(-2, "%s: channel count %d is not a multiple of %d", what, c, fsr_multiple(dtype));
  return 0;
}
// a flat tensor of `count` elements: whole units (x3: whole groups)
inline int check_count(const char* what, int dtype, long long count) {
  if (!fsr_known_dtype(dtype)) return fsr_fail(-2, "%s: unknown dtype %d", what, dtype);
  if (count % fsr_multiple(dtype)) return fsr_fail(-2, "%s: count %lld is not a multiple of %d", what, count, fsr_multiple(dtype));
  return 0;
}
// x3 tensors: the split hi / lo addressing needs 128-byte aligned bases
inline int check_x3(const char* what, int dtype, const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
  if (dtype != FSR_X3) return 0;
  if ((((size_t)a | (size_t)b | (size_t)c | (size_t)d) & 127) != 0) return fsr_fail(-2, "%s: x3 tensors must be 128-byte aligned", what);
  return 0;
}

// Planar-YUV output of h x w (yuv.hip; the encode entry points and the resampler): 4:2:0 needs even extents, 4:2:2 an even width, and
// the matrix / range pair must be known.  0, or the refusal recorded in `who`'s name (`what`: a word put in front of the colour message).
int fsr_yuv_out_check(const char* who, const char* what, int chroma, int h, int w, int matrix, int full_range);
int fsr_yuv_layout_check(const char* who, int chroma, int layout);   // yuv.hip: a known payload layout, semi-planar with 4:2:0 only

int fsr_conv_igemm_dispatch(int dtype, ConvKArgs& a, int S, hipStream_t stream);
// `n` launches that differ only in output grid / taps / output offset (stride-2 data-gradient classes) as ONE launch
int fsr_conv_igemm_dispatch_classes(int dtype, ConvKArgs* cls, int n, hipStream_t stream);
int fsr_conv_stage_mode();   // FSR_CONV_STAGE tuning / test switch, see conv_igemm.hip
// 1 = launched, 0 = shape not handled by the LDS-resident-filter kernel, < 0 = error
int fsr_conv64_persistent_try(int dtype, ConvKArgs& a, int S, hipStream_t stream);
int fsr_conv_tall3_try(int dtype, ConvKArgs& a, int S, hipStream_t stream);        // 128..512 channels, stride 1: 32x32x16 MFMA, all-DMA (conv_tall3.hip)
int fsr_conv64_s2fwd_try(int dtype, ConvKArgs& a, int S, hipStream_t stream);     // stride-2 forward, 64 -> 64, persistent streaming
int fsr_conv_s2d3_try(int dtype, ConvKArgs& a, hipStream_t stream);        // stride-2 data gradient, 64..512 channels, all parity classes (conv_s2d3.hip)
// Second level of every cross-workgroup reduction (reduce.hip): out[b][i] (+)= scale * sum_p part[(b*P + p)*stride + i]
// for i < len, p in a fixed order.  per > 0: batch b owns only the slots of the tile ranges [w*per, (w+1)*per) that
// intersect its tpi tiles.
int fsr_launch_reduce_partials(const float* part, float* out, int batches, int P, int len, int stride, int tpi, int per,
                               float scale, int accumulate, hipStream_t stream);
