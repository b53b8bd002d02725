// The eight symmetries of the rectangle on 3-channel NHWC images, for self-ensemble inference.
//
// Code k in 0..7 acts on an H x W image in three steps: k & 1 flips the width axis, k & 2 flips the height axis, then k & 4
// transposes H and W (codes 4..7 produce a W x H image):
//   k < 4 :  D_k(x)[y][x'] = x[fy(y)][fx(x')]                      fy(y) = k & 2 ? H - 1 - y : y,  fx(x) = k & 1 ? W - 1 - x : x
//   k >= 4:  D_k(x)[a][b]  = x[fy(b)][fx(a)]                       a < W, b < H
// and the image a member's output y_k contributes to the sum, in the orientation of x, is
//   k < 4 :  y_k'[Y][X] = y_k[fy(Y)][fx(X)]        k >= 4:  y_k'[Y][X] = y_k[fx(X)][fy(Y)]       (the inverse: transpose first, then flip).
//
// Two entry points, each one launch per orientation group (codes 0..3 or 4..7) or sub-range of it:
//   fsr_dihedral_members    : uint8 or float [n,h,w,3] -> the float [-1,1] images of members k0..k1, member-major [(k - k0) n + i];
//   fsr_dihedral_accumulate : adds the float outputs of members k0..k1 through the inverse transforms onto the running float sum in
//                             code order; the launch that holds code 7 multiplies by 0.125f and stores the float or uint8 mean.
// Memory access: a flip keeps a row segment a row segment (reversed), so codes 0..3 are plain streaming kernels, one thread per
// float of a row.  A transpose turns rows into columns: codes 4..7 go through an LDS tile of 32 x 32 pixels of 12 bytes with a pitch
// of 33 pixels (99 floats = 3 modulo 32 banks), filled from whole 384-byte row segments and read back along the other axis -- both
// global sides are runs of contiguous row segments, and the 32 lanes of an LDS access (3 floats per pixel, pixels 99 floats apart)
// touch 32 consecutive banks.
#include "fsr_common.h"
#include "fsr_host.h"

namespace {

constexpr int DT = 32;              // tile edge in pixels
constexpr int DPITCH = 3 * DT + 3;  // floats per LDS tile row: 33 pixels
constexpr int DROW = 3 * DT;        // floats of a full tile row

// the exact expression of u8_to_image_kernel (elementwise.hip)
__device__ __forceinline__ float member_value(const unsigned char* s, size_t i) { return (float)s[i] / 127.5f - 1.0f; }
__device__ __forceinline__ float member_value(const float* s, size_t i) { return s[i]; }

// ---------------------------------------------------------------- member input, codes 0..3: out[k][n][y][x] = src[n][fy(y)][fx(x)]
template <typename T>
__global__ __launch_bounds__(256) void dihedral_members_flip_kernel(const T* __restrict__ src, int n, int h, int w, int k0, int k1,
                                                                    float* __restrict__ out, long long total) {
  const long long rw = 3LL * w;
  const size_t member = (size_t)n * h * rw;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int e = (int)(i % rw);
    const long long row = i / rw;           // image * h + y
    const int y = (int)(row % h);
    const long long img = row / h;
    const int px = e / 3, c = e - 3 * px;
    const float v = member_value(src, (size_t)i);
    for (int k = k0; k <= k1; ++k) {
      const int oy = (k & 2) ? h - 1 - y : y;
      const int ox = (k & 1) ? w - 1 - px : px;
      out[(size_t)(k - k0) * member + ((size_t)img * h + oy) * rw + 3 * ox + c] = v;
    }
  }
}

// ---------------------------------------------------------------- member input, codes 4..7: out[k][n][a][b] = src[n][fy(b)][fx(a)]
// one workgroup per 32 x 32 source tile of one image: the tile is read once and written for every code of the range
template <typename T>
__global__ __launch_bounds__(256) void dihedral_members_transpose_kernel(const T* __restrict__ src, int n, int h, int w, int k0, int k1,
                                                                         float* __restrict__ out) {
  __shared__ float tile[DT * DPITCH];
  const int x0 = blockIdx.x * DT, y0 = blockIdx.y * DT, img = blockIdx.z;
  const int tw = w - x0 < DT ? w - x0 : DT, th = h - y0 < DT ? h - y0 : DT;
  const size_t image = (size_t)h * w * 3;
  const T* s = src + (size_t)img * image;
  for (int idx = threadIdx.x; idx < DT * DROW; idx += 256) {
    const int r = idx / DROW, e = idx - r * DROW;
    if (r < th && e < 3 * tw) tile[r * DPITCH + e] = member_value(s, ((size_t)(y0 + r) * w + x0) * 3 + e);
  }
  __syncthreads();
  for (int k = k0; k <= k1; ++k) {
    float* o = out + ((size_t)(k - k0) * n + img) * image;   // [w][h][3]
    const int b0 = (k & 2) ? h - y0 - th : y0;                // first output column of the segment this tile fills
    for (int idx = threadIdx.x; idx < DT * DROW; idx += 256) {
      const int j = idx / DROW, e = idx - j * DROW;            // j: source column of the tile = output row; e: float of the segment
      const int pb = e / 3, c = e - 3 * pb;
      if (j < tw && pb < th) {
        const int r = (k & 2) ? th - 1 - pb : pb;
        const int a = (k & 1) ? w - 1 - (x0 + j) : x0 + j;
        o[((size_t)a * h + b0) * 3 + e] = tile[r * DPITCH + 3 * j + c];
      }
    }
  }
}

// (unsigned char)(clamp((m + 1) / 2, 0, 1) * 255): the truncating cast of resample.hip's FSR_OUT_U8 on c = (m + 1) / 2, and, for
// m in [-1, 1], image_u8's bytes
__device__ __forceinline__ unsigned char mean_u8(float m) { return (unsigned char)(fminf(fmaxf((m + 1.f) / 2.f, 0.f), 1.f) * 255.f); }

// ---------------------------------------------------------------- accumulate, codes 0..3: s += y_k[n][fy(Y)][fx(X)] in code order
// (code 7 is not in this group: the result is always the running sum)
__global__ __launch_bounds__(256) void dihedral_accumulate_flip_kernel(const float* __restrict__ y, int n, int h, int w, int k0, int k1,
                                                                       const float* acc_in, float* acc_out, long long total) {
  const long long rw = 3LL * w;
  const size_t member = (size_t)n * h * rw;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int e = (int)(i % rw);
    const long long row = i / rw;
    const int Y = (int)(row % h);
    const long long img = row / h;
    const int px = e / 3, c = e - 3 * px;
    float s = 0.f;
    for (int k = k0; k <= k1; ++k) {
      const int sy = (k & 2) ? h - 1 - Y : Y;
      const int sx = (k & 1) ? w - 1 - px : px;
      const float v = y[(size_t)(k - k0) * member + ((size_t)img * h + sy) * rw + 3 * sx + c];
      s = (k == 0) ? v : (k == k0 ? acc_in[i] + v : s + v);
    }
    acc_out[i] = s;
  }
}

// ---------------------------------------------------------------- accumulate, codes 4..7: s += y_k[n][fx(X)][fy(Y)] in code order
// y_k is [w][h][3]; one workgroup per 32 x 32 tile of the sum; each thread owns 12 floats of it
template <bool U8>
__global__ __launch_bounds__(256) void dihedral_accumulate_transpose_kernel(const float* __restrict__ y, int n, int h, int w, int k0, int k1,
                                                                            const float* acc_in, float* acc_out, void* out) {
  __shared__ float tile[DT * DPITCH];
  constexpr int PER = DT * DROW / 256;
  const int x0 = blockIdx.x * DT, y0 = blockIdx.y * DT, img = blockIdx.z;
  const int tw = w - x0 < DT ? w - x0 : DT, th = h - y0 < DT ? h - y0 : DT;
  const size_t image = (size_t)h * w * 3;
  float s[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int idx = threadIdx.x + 256 * i;
    const int r = idx / DROW, e = idx - r * DROW;
    s[i] = (r < th && e < 3 * tw) ? acc_in[(size_t)img * image + ((size_t)(y0 + r) * w + x0) * 3 + e] : 0.f;
  }
  for (int k = k0; k <= k1; ++k) {
    const float* m = y + ((size_t)(k - k0) * n + img) * image;     // [w][h][3]
    const int a0 = (k & 1) ? w - x0 - tw : x0;                      // rows a0 .. a0 + tw, columns b0 .. b0 + th of the member
    const int b0 = (k & 2) ? h - y0 - th : y0;
    __syncthreads();
    for (int idx = threadIdx.x; idx < DT * DROW; idx += 256) {
      const int r = idx / DROW, e = idx - r * DROW;
      if (r < tw && e < 3 * th) tile[r * DPITCH + e] = m[((size_t)(a0 + r) * h + b0) * 3 + e];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int idx = threadIdx.x + 256 * i;
      const int r = idx / DROW, e = idx - r * DROW;                 // r: row of the sum's tile, e: float of its row segment
      const int px = e / 3, c = e - 3 * px;
      if (r < th && px < tw) {
        const int al = (k & 1) ? tw - 1 - px : px;
        const int bl = (k & 2) ? th - 1 - r : r;
        s[i] += tile[al * DPITCH + 3 * bl + c];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int idx = threadIdx.x + 256 * i;
    const int r = idx / DROW, e = idx - r * DROW;
    if (r < th && e < 3 * tw) {
      const size_t o = (size_t)img * image + ((size_t)(y0 + r) * w + x0) * 3 + e;
      if (k1 < 7) acc_out[o] = s[i];
      else if constexpr (U8) ((unsigned char*)out)[o] = mean_u8(s[i] * 0.125f);
      else ((float*)out)[o] = s[i] * 0.125f;
    }
  }
}

int check_codes(const char* who, int n, int h, int w, int k0, int k1) {
  if (n <= 0 || h <= 0 || w <= 0) return fsr_fail(-2, "%s: n, h and w must be positive, got %d, %d, %d", who, n, h, w);
  if (n > 65535) return fsr_fail(-2, "%s: at most 65535 images per call, got %d", who, n);
  if (k0 < 0 || k1 > 7 || k0 > k1) return fsr_fail(-2, "%s: codes must satisfy 0 <= k0 <= k1 <= 7, got %d..%d", who, k0, k1);
  if ((k0 >> 2) != (k1 >> 2))
    return fsr_fail(-2, "%s: codes %d..%d span both orientation groups (0..3 and 4..7 take a launch each)", who, k0, k1);
  return 0;
}

unsigned stream_blocks(long long total) {
  long long blocks = (total + 255) / 256;
  return (unsigned)(blocks > 8192 ? 8192 : blocks);
}

}  // namespace

extern "C" int fsr_dihedral_members(const void* src, int src_is_u8, int n, int h, int w, int k0, int k1, float* out,
                                    fsr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!src || !out) return fsr_fail(-1, "fsr_dihedral_members: null argument");
  if (int rc = check_codes("fsr_dihedral_members", n, h, w, k0, k1)) return rc;
  if (k0 < 4) {
    const long long total = 3LL * n * h * w;
    const dim3 grid(stream_blocks(total));
    if (src_is_u8)
      hipLaunchKernelGGL(dihedral_members_flip_kernel<unsigned char>, grid, dim3(256), 0, stream, (const unsigned char*)src, n, h, w, k0, k1,
                         out, total);
    else
      hipLaunchKernelGGL(dihedral_members_flip_kernel<float>, grid, dim3(256), 0, stream, (const float*)src, n, h, w, k0, k1, out, total);
    return fsr_check_launch("dihedral_members_flip_kernel");
  }
  const long long ty = ((long long)h + DT - 1) / DT;
  if (ty > 65535) return fsr_fail(-2, "fsr_dihedral_members: h = %d is too large", h);
  const dim3 grid((unsigned)((w + DT - 1) / DT), (unsigned)ty, (unsigned)n);
  if (src_is_u8)
    hipLaunchKernelGGL(dihedral_members_transpose_kernel<unsigned char>, grid, dim3(256), 0, stream, (const unsigned char*)src, n, h, w, k0,
                       k1, out);
  else
    hipLaunchKernelGGL(dihedral_members_transpose_kernel<float>, grid, dim3(256), 0, stream, (const float*)src, n, h, w, k0, k1, out);
  return fsr_check_launch("dihedral_members_transpose_kernel");
}

extern "C" int fsr_dihedral_accumulate(const float* y, int n, int h, int w, int k0, int k1, float* acc, void* out, int out_kind,
                                       fsr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!y) return fsr_fail(-1, "fsr_dihedral_accumulate: null argument");
  if (int rc = check_codes("fsr_dihedral_accumulate", n, h, w, k0, k1)) return rc;
  const bool last = k1 == 7;
  if ((!last || k0 > 0) && !acc) return fsr_fail(-1, "fsr_dihedral_accumulate: null accumulator");
  if (last && !out) return fsr_fail(-1, "fsr_dihedral_accumulate: null output");
  if (last && out_kind != FSR_OUT_F32 && out_kind != FSR_OUT_U8)
    return fsr_fail(-2, "fsr_dihedral_accumulate: out_kind must be FSR_OUT_F32 or FSR_OUT_U8, got %d", out_kind);
  if (k0 < 4) {
    const long long total = 3LL * n * h * w;
    hipLaunchKernelGGL(dihedral_accumulate_flip_kernel, dim3(stream_blocks(total)), dim3(256), 0, stream, y, n, h, w, k0, k1,
                       (const float*)acc, acc, total);
    return fsr_check_launch("dihedral_accumulate_flip_kernel");
  }
  const long long ty = ((long long)h + DT - 1) / DT;
  if (ty > 65535) return fsr_fail(-2, "fsr_dihedral_accumulate: h = %d is too large", h);
  const dim3 grid((unsigned)((w + DT - 1) / DT), (unsigned)ty, (unsigned)n);
  if (last && out_kind == FSR_OUT_U8)
    hipLaunchKernelGGL(dihedral_accumulate_transpose_kernel<true>, grid, dim3(256), 0, stream, y, n, h, w, k0, k1, (const float*)acc, acc,
                       out);
  else
    hipLaunchKernelGGL(dihedral_accumulate_transpose_kernel<false>, grid, dim3(256), 0, stream, y, n, h, w, k0, k1, (const float*)acc, acc,
                       out);
  return fsr_check_launch("dihedral_accumulate_transpose_kernel");
}
