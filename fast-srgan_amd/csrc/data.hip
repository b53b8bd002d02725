// Crop + antialiased bicubic down-scale of uint8 CHW images, on the device.
//
// Replaces NumpyImagesDataset.__getitem__ (/root/reference/dataloader.py:24-38): random HR crop of a
// uint8 (3,H,W) array -> float32 -> torchvision v2.Resize(BICUBIC, antialias=True) (= torch's
// separable upsample_bicubic2d_aa kernel: horizontal pass, then vertical pass, cubic a = -0.5,
// support 2*scale, taps normalised; dataloader.py:15-19,34) -> both images mapped to [-1,1] by
// x/127.5 - 1 (dataloader.py:36-37; true division, as torch does).
//
// Two bandwidth-bound kernels per batch; the tap table (identical for rows and columns of a square
// crop) is built once on the host and passed in.  The source images stay resident in HBM as uint8
// (a DIV2K training set is ~3.5 GB of 288 GB), so a batch costs 3*hr^2 bytes of reads per sample.
#include "fsr_common.h"
#include "fsr_host.h"

namespace {

// pass 1: hr_out[n][c][y][x] = crop/127.5-1 ; tmp[n][c][y][xo] = sum_k w[xo][k] * crop[y][xmin[xo]+k]
__global__ __launch_bounds__(256) void crop_hpass_kernel(const uint8_t* const* __restrict__ images, const int* __restrict__ img_h,
                                                         const int* __restrict__ img_w, const int* __restrict__ crop_y,
                                                         const int* __restrict__ crop_x, int hr, int lr,
                                                         const float* __restrict__ wtab, const int* __restrict__ xmin,
                                                         const int* __restrict__ xsize, int kmax, float* __restrict__ hr_out,
                                                         float* __restrict__ tmp) {
  // one workgroup per (sample, channel, crop row)
  int b = blockIdx.x;
  const int y = b % hr;
  b /= hr;
  const int c = b % 3;
  const int n = b / 3;
  const int H = img_h[n], W = img_w[n];
  const uint8_t* row = images[n] + ((size_t)c * H + crop_y[n] + y) * W + crop_x[n];
  HIP_DYNAMIC_SHARED(float, line)
  for (int x = threadIdx.x; x < hr; x += 256) {
    const float v = (float)row[x];
    line[x] = v;
    hr_out[(((size_t)n * 3 + c) * hr + y) * hr + x] = v / 127.5f - 1.0f;
  }
  __syncthreads();
  for (int xo = threadIdx.x; xo < lr; xo += 256) {
    const float* w = wtab + (size_t)xo * kmax;
    const int x0 = xmin[xo], ks = xsize[xo];
    float s = 0.f;
    for (int k = 0; k < ks; ++k) s += w[k] * line[x0 + k];
    tmp[(((size_t)n * 3 + c) * hr + y) * lr + xo] = s;
  }
}

// pass 2: lr_out[n][c][yo][xo] = (sum_k w[yo][k] * tmp[ymin[yo]+k][xo]) / 127.5 - 1
__global__ __launch_bounds__(256) void crop_vpass_kernel(const float* __restrict__ tmp, int hr, int lr,
                                                         const float* __restrict__ wtab, const int* __restrict__ xmin,
                                                         const int* __restrict__ xsize, int kmax, float* __restrict__ lr_out,
                                                         long long total) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int xo = (int)(i % lr);
    const int yo = (int)((i / lr) % lr);
    const long long nc = i / ((long long)lr * lr);
    const float* w = wtab + (size_t)yo * kmax;
    const int y0 = xmin[yo], ks = xsize[yo];
    const float* col = tmp + ((size_t)nc * hr + y0) * lr + xo;
    float s = 0.f;
    for (int k = 0; k < ks; ++k) s += w[k] * col[(size_t)k * lr];
    lr_out[i] = s / 127.5f - 1.0f;
  }
}

// pass 1 of fsr_crop_resize_aug: crop_hpass_kernel on D_k(crop), k = xform[n] (the dihedral codes of dihedral.hip: k & 1 flips the
// width axis, k & 2 the height axis, then k & 4 transposes).  One workgroup per (sample, channel, block of `rb` rows of D_k(crop)):
// the rows are gathered into LDS lines of `pitch` floats (odd: a column of lines lies on distinct banks) and everything behind the
// line -- the [-1,1] mapping of hr_out and the tap sums of tmp -- is crop_hpass_kernel's arithmetic in its order.  A flip reads each
// source row segment backwards; a transposing code reads, for every source row, the `rb` contiguous bytes its block of columns
// holds and stores them down the lines, so no global access is strided by a row on either side.
__global__ __launch_bounds__(256) void crop_hpass_aug_kernel(const uint8_t* const* __restrict__ images, const int* __restrict__ img_h,
                                                             const int* __restrict__ img_w, const int* __restrict__ crop_y,
                                                             const int* __restrict__ crop_x, const int* __restrict__ xform, int hr,
                                                             int lr, int rb, int pitch, const float* __restrict__ wtab,
                                                             const int* __restrict__ xmin, const int* __restrict__ xsize, int kmax,
                                                             float* __restrict__ hr_out, float* __restrict__ tmp) {
  const int nblk = (hr + rb - 1) / rb;
  int b = blockIdx.x;
  const int y0 = (b % nblk) * rb;
  b /= nblk;
  const int c = b % 3;
  const int n = b / 3;
  const int rows = hr - y0 < rb ? hr - y0 : rb;
  const int H = img_h[n], W = img_w[n], k = xform[n] & 7;
  const uint8_t* crop = images[n] + ((size_t)c * H + crop_y[n]) * W + crop_x[n];
  HIP_DYNAMIC_SHARED(float, lines)
  if (k < 4) {      // line r = row fy(y0 + r) of the crop, read through fx
    for (int idx = threadIdx.x; idx < rows * hr; idx += 256) {
      const int r = idx / hr, x = idx - r * hr;
      const int sy = (k & 2) ? hr - 1 - (y0 + r) : y0 + r;
      const int sx = (k & 1) ? hr - 1 - x : x;
      lines[r * pitch + x] = (float)crop[(size_t)sy * W + sx];
    }
  } else {          // line r = column fx(y0 + r) of the crop, read through fy: D_k(crop)[a][b] = crop[fy(b)][fx(a)]
    const int c0 = (k & 1) ? hr - y0 - rows : y0;      // the block's columns c0 .. c0 + rows of the crop
    for (int idx = threadIdx.x; idx < rows * hr; idx += 256) {
      const int x = idx / rows, j = idx - x * rows;      // x: position along the lines; j: column c0 + j of the crop
      const int sy = (k & 2) ? hr - 1 - x : x;
      const int r = (k & 1) ? rows - 1 - j : j;
      lines[r * pitch + x] = (float)crop[(size_t)sy * W + c0 + j];
    }
  }
  __syncthreads();
  const size_t plane = (size_t)n * 3 + c;
  for (int idx = threadIdx.x; idx < rows * hr; idx += 256) {
    const int r = idx / hr, x = idx - r * hr;
    const float v = lines[r * pitch + x];
    hr_out[(plane * hr + y0 + r) * hr + x] = v / 127.5f - 1.0f;
  }
  for (int idx = threadIdx.x; idx < rows * lr; idx += 256) {
    const int r = idx / lr, xo = idx - r * lr;
    const float* line = lines + r * pitch;
    const float* w = wtab + (size_t)xo * kmax;
    const int x0 = xmin[xo], ks = xsize[xo];
    float s = 0.f;
    for (int t = 0; t < ks; ++t) s += w[t] * line[x0 + t];
    tmp[(plane * hr + y0 + r) * lr + xo] = s;
  }
}

}  // namespace

extern "C" int fsr_crop_resize_aug(const uint8_t* const* images, const int* img_h, const int* img_w, const int* crop_y,
                                   const int* crop_x, const int* xform, int n, int hr_size, int scale, const float* wtab,
                                   const int* xmin, const int* xsize, int kmax, float* hr_out, float* lr_out, float* tmp,
                                   fsr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!images || !img_h || !img_w || !crop_y || !crop_x || !xform || !wtab || !xmin || !xsize || !hr_out || !lr_out || !tmp)
    return fsr_fail(-1, "fsr_crop_resize_aug: null argument");
  if (n <= 0 || hr_size <= 0 || scale <= 0 || hr_size % scale) return fsr_fail(-2, "fsr_crop_resize_aug: bad sizes");
  if (hr_size * sizeof(float) > 60 * 1024) return fsr_fail(-2, "fsr_crop_resize_aug: crop row does not fit in LDS");
  const int lr = hr_size / scale, pitch = hr_size | 1;
  int rb = 32;      // rows per workgroup: 32 lines of the crop in at most 60 KB of LDS, fewer for very wide crops
  while (rb > 1 && (size_t)rb * pitch * sizeof(float) > 60 * 1024) rb /= 2;
  if (rb > hr_size) rb = hr_size;
  const long long blocks1 = (long long)n * 3 * ((hr_size + rb - 1) / rb);
  if (blocks1 > 0x7fffffffLL) return fsr_fail(-2, "fsr_crop_resize_aug: batch too large");
  hipLaunchKernelGGL(crop_hpass_aug_kernel, dim3((unsigned)blocks1), dim3(256), (size_t)rb * pitch * sizeof(float), stream, images, img_h,
                     img_w, crop_y, crop_x, xform, hr_size, lr, rb, pitch, wtab, xmin, xsize, kmax, hr_out, tmp);
  if (int rc = fsr_check_launch("crop_hpass_aug_kernel")) return rc;
  const long long total = (long long)n * 3 * lr * lr;
  long long blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(crop_vpass_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, tmp, hr_size, lr, wtab, xmin, xsize, kmax,
                     lr_out, total);
  return fsr_check_launch("crop_vpass_kernel");
}

extern "C" int fsr_crop_resize(const uint8_t* const* images, const int* img_h, const int* img_w, const int* crop_y,
                               const int* crop_x, int n, int hr_size, int scale, const float* wtab, const int* xmin,
                               const int* xsize, int kmax, float* hr_out, float* lr_out, float* tmp, fsr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!images || !img_h || !img_w || !crop_y || !crop_x || !wtab || !xmin || !xsize || !hr_out || !lr_out || !tmp)
    return fsr_fail(-1, "fsr_crop_resize: null argument");
  if (n <= 0 || hr_size <= 0 || scale <= 0 || hr_size % scale) return fsr_fail(-2, "fsr_crop_resize: bad sizes");
  if (hr_size * sizeof(float) > 60 * 1024) return fsr_fail(-2, "fsr_crop_resize: crop row does not fit in LDS");
  const int lr = hr_size / scale;
  hipLaunchKernelGGL(crop_hpass_kernel, dim3((unsigned)(n * 3 * hr_size)), dim3(256), hr_size * sizeof(float), stream, images,
                     img_h, img_w, crop_y, crop_x, hr_size, lr, wtab, xmin, xsize, kmax, hr_out, tmp);
  if (int rc = fsr_check_launch("crop_hpass_kernel")) return rc;
  const long long total = (long long)n * 3 * lr * lr;
  long long blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(crop_vpass_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, tmp, hr_size, lr, wtab, xmin, xsize, kmax,
                     lr_out, total);
  return fsr_check_launch("crop_vpass_kernel");
}
