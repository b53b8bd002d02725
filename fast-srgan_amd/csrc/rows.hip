// Strided row-block copy: the gather and the scatter of the generator's banded tail.
//
// A frame of H2 rows is covered by nwin = ceil(H2 / R) windows of Hw rows each.  Window k owns the core rows [k R, min((k + 1) R, H2))
// and starts at s_k = clamp(k R - 2, 0, H2 - Hw).  The windows of all images are numbered f = image * nwin + k; one launch moves the
// `count` windows f = first .. first + count - 1, window j = f - first of the group being the j-th image of the group buffer.
//   gather : rows [s_k, s_k + Hw) of image i                    -> rows [0, Hw) of window j
//   scatter: rows [(k R - s_k) mul, (core_hi - s_k) mul) of window j -> rows [k R mul, core_hi mul) of image i
// Rows are row_bytes bytes and lie back to back inside an image, so a window's rows are ONE run of bytes on either side; images are
// src_pitch / dst_pitch bytes apart (a plane of a planar payload: the payload's size, not the plane's).  Every offset is computed
// here from (H2, Hw, R, f) -- no index table, nothing to upload inside a captured graph -- and in 64 bits: the tensor in front of the
// last up-sampling convolution alone is 4.2 GB at 2160p, which the 32-bit indices of the convolution kernels could not address.
#include "fsr_common.h"
#include "fsr_host.h"

template <int W> struct RowUnit;
template <> struct RowUnit<16> { typedef u32x4 type; };
template <> struct RowUnit<4> { typedef unsigned type; };
template <> struct RowUnit<1> { typedef unsigned char type; };

// grid = (blocks per window, windows of the group); W = bytes per access (host-checked alignment of bases, pitches and row_bytes)
template <int W>
__global__ __launch_bounds__(256) void copy_rows_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                        long long src_pitch, long long dst_pitch, long long row_bytes, int first, int nwin,
                                                        int H2, int Hw, int R, int mul, int scatter) {
  typedef typename RowUnit<W>::type V;
  const int j = blockIdx.y;
  const int f = first + j;
  const int img = f / nwin, k = f - img * nwin;
  const int lo = k * R;
  const int hi = lo + R < H2 ? lo + R : H2;
  int s = lo - 2;
  if (s > H2 - Hw) s = H2 - Hw;
  if (s < 0) s = 0;
  long long so, dof, rows;
  if (!scatter) {
    so = (long long)img * src_pitch + (long long)s * row_bytes;
    dof = (long long)j * dst_pitch;
    rows = Hw;
  } else {
    so = (long long)j * src_pitch + (long long)(lo - s) * mul * row_bytes;
    dof = (long long)img * dst_pitch + (long long)lo * mul * row_bytes;
    rows = (long long)(hi - lo) * mul;
  }
  const long long units = rows * row_bytes / W;
  const V* __restrict__ sp = (const V*)(src + so);
  V* __restrict__ dp = (V*)(dst + dof);
  for (long long u = (long long)blockIdx.x * 256 + threadIdx.x; u < units; u += (long long)gridDim.x * 256) dp[u] = sp[u];
}

extern "C" int fsr_copy_rows(const void* src, long long src_pitch, void* dst, long long dst_pitch, long long row_bytes, int first, int count,
                             int H2, int Hw, int R, int mul, int scatter, fsr_stream_t stream_) {
  if (!src || !dst) return fsr_fail(-1, "fsr_copy_rows: null argument");
  if (src_pitch <= 0 || dst_pitch <= 0 || row_bytes <= 0 || count <= 0 || H2 <= 0 || Hw <= 0 || mul <= 0 || first < 0)
    return fsr_fail(-2, "fsr_copy_rows: extents must be positive (pitches %lld / %lld, row_bytes %lld, count %d, H2 %d, Hw %d, mul %d, first %d)",
                    src_pitch, dst_pitch, row_bytes, count, H2, Hw, mul, first);
  if (R < 1) return fsr_fail(-2, "fsr_copy_rows: a band has at least one core row (R = %d)", R);
  if (Hw > H2) return fsr_fail(-2, "fsr_copy_rows: a window of %d rows does not fit in a frame of %d", Hw, H2);
  if (Hw < R + 4) return fsr_fail(-2, "fsr_copy_rows: a window holds its %d core rows and a halo of 2 on each side (Hw = %d)", R, Hw);
  if (count > 65535) return fsr_fail(-2, "fsr_copy_rows: at most 65535 windows per launch (count = %d)", count);
  if ((long long)first + count > 0x7fffffffLL) return fsr_fail(-2, "fsr_copy_rows: window numbers must fit in 31 bits");
  const int nwin = (H2 + R - 1) / R;
  const long long rows = scatter ? (long long)R * mul : (long long)Hw;   // the most rows any window of the launch moves
  const size_t align = (size_t)src | (size_t)dst | (size_t)src_pitch | (size_t)dst_pitch | (size_t)row_bytes;
  const int W = (align & 15) == 0 ? 16 : ((align & 3) == 0 ? 4 : 1);
  long long bx = (rows * row_bytes / W + 1023) / 1024;      // four units per thread before the grid stride wraps
  if (bx > 1024) bx = 1024;
  if (bx < 1) bx = 1;
  const dim3 grid((unsigned)bx, (unsigned)count);
  hipStream_t stream = (hipStream_t)stream_;
  const unsigned char* s = (const unsigned char*)src;
  unsigned char* d = (unsigned char*)dst;
  if (W == 16)
    hipLaunchKernelGGL(copy_rows_kernel<16>, grid, dim3(256), 0, stream, s, d, src_pitch, dst_pitch, row_bytes, first, nwin, H2, Hw, R, mul, scatter);
  else if (W == 4)
    hipLaunchKernelGGL(copy_rows_kernel<4>, grid, dim3(256), 0, stream, s, d, src_pitch, dst_pitch, row_bytes, first, nwin, H2, Hw, R, mul, scatter);
  else
    hipLaunchKernelGGL(copy_rows_kernel<1>, grid, dim3(256), 0, stream, s, d, src_pitch, dst_pitch, row_bytes, first, nwin, H2, Hw, R, mul, scatter);
  fsr_note_kernel("copy_rows_kernel<%d>", W);
  return fsr_check_launch("copy_rows_kernel");
}
