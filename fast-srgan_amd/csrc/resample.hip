// Arbitrary output size: antialiased bicubic resize of the generator's head output, fused with the output conversion.
//
// fsr_resample_image takes the head's float tanh output t [n,h,w,3] (what FSR_OUT_F32 stores in every compute mode) to an
// oh x ow frame -- float (2 v - 1), uint8 RGB (the truncating cast of image_u8) or I420 planes (the colour contract of
// DESIGN.md §6c) -- with the arithmetic of torch's upsample_bicubic2d_aa on c = (t + 1) / 2: separable, the horizontal sum
// first, taps normalised in float32 (the tables of dataloader.aa_bicubic_taps, one per axis), float32 accumulation.
//
// One kernel, no global intermediate, no atomics.  A 256-thread workgroup owns a tile of RS_TW = 64 output
// columns x `th` output rows (th = 32, 16, 8, 4 or 2: the largest whose source-row window fits the LDS budget; tile origins are
// even, so a 2x2 chroma block never leaves its workgroup):
//   1. horizontal pass: thread e < 192 owns the float e = 3 * column + channel of the tile's rows, keeps its taps in registers
//      (rows of up to 5 or 9 taps: up-scales, down-scales up to 2) and walks the source rows [r0, r1) of the tile's window: lds[row][e] = sum_k wx[k] * c[row][xmin + k];
//   2. vertical pass from LDS: a thread takes 4 consecutive floats of an output row (one ds_read_b128 per tap, the row and its
//      taps wave-uniform), converts and stores 16 bytes of floats or one dword of bytes; for I420 it takes 4 columns x 2 rows --
//      two whole 2x2 blocks, no shuffle -- and stores a dword of Y per row and two bytes of Cb and of Cr (i420_store_2x4,
//      fsr_yuv.h; fsr_resample_image_i420_deep: the same stage with 16-bit samples at depth 9..16, 8 and 4 bytes);
//      for 4:2:2 / 4:4:4 planes (fsr_resample_image_yuv) it takes 4 columns x 1 row (yuv_store_1x4).  A 4:2:2 chroma sample also needs
//      the column left of its pair: the horizontal pass of that instantiation computes a 65th column -- the tile's left neighbour,
//      clamped at the image edge -- with three of its idle threads and stores it behind the 64 (LDS rows of 196 floats, still a
//      multiple of 16 bytes), in the neighbouring tile's own arithmetic.
// Every table value is clamped to the image and to the LDS window before it is used as an index: tables that are not the ones
// the contract names give wrong pixels, never an access outside the tensors.
#include "fsr_yuv.h"
#include "fsr_host.h"

namespace {

constexpr int RS_TW = 64;                  // output columns of a tile
constexpr int RS_ROWF = RS_TW * 3;         // floats of one LDS row
constexpr int RS_LDS_BUDGET = 64 * 1024;   // bytes of dynamic LDS a workgroup may take (several workgroups per CU stay resident)
constexpr int RS_MAX_RATIO = 8;            // supported down-scaling ratio per axis (tap rows of up to 33)
// template kinds of the planar 4:2:2 / 4:4:4 stages, next to the FSR_OUT_* values of the public kinds
constexpr int RS_YUV422 = 8 + FSR_CHROMA_422, RS_YUV444 = 8 + FSR_CHROMA_444;
constexpr int RS_NV12 = 12;                // the I420 stage storing the semi-planar payload (FSR_LAYOUT_NV12)
constexpr int rs_rowf(int kind) { return kind == RS_YUV422 ? RS_ROWF + 4 : RS_ROWF; }   // floats of one LDS row: 4:2:2 keeps a 65th column

struct ResampleArgs {
  const float* t;
  int n, h, w, oh, ow;
  const float* wy;
  const int* ymin;
  const int* ysize;
  int ky;
  const float* wx;
  const int* xmin;
  const int* xsize;
  int kx;
  int th;                 // output rows of a tile (even)
  int tiles_x, tiles_y;
  int rows_cap;           // source rows the LDS allocation holds
  int matrix, full;
  void* out;
  int depth;              // FSR_OUT_I420 with 16-bit samples: bits per sample (9..16)
};

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// KIND: FSR_OUT_F32 / FSR_OUT_U8 / FSR_OUT_I420.  KXS = 5 / 9: rows of at most 5 (every up-scale) / 9 (down-scales up to 2: the
// network's 4x taken to 3x or 2x of the input) horizontal taps, held in registers; KXS = 0: any tap count, read per use.
// RS_NV12: FSR_OUT_I420's stage with the semi-planar store (16-bit codes in the high bits).
// C (FSR_OUT_I420, RS_NV12, RS_YUV422, RS_YUV444): the sample type of the planes -- unsigned char, or unsigned short for 9..16-bit samples (a.depth).
template <int KIND, int KXS, typename C = unsigned char>
__global__ __launch_bounds__(256) void resample_kernel(const ResampleArgs a) {
  HIP_DYNAMIC_SHARED(float, lds)
  constexpr int ROWF = rs_rowf(KIND);
  constexpr int HT = KIND == RS_YUV422 ? RS_ROWF + 3 : RS_ROWF;   // threads of the horizontal pass
  int b = blockIdx.x;
  const int tx = b % a.tiles_x;
  b /= a.tiles_x;
  const int ty = b % a.tiles_y;
  const int n = b / a.tiles_y;
  const int x0 = tx * RS_TW, y0 = ty * a.th;
  const int tw = imin(RS_TW, a.ow - x0), th = imin(a.th, a.oh - y0);
  // the tile's source-row window (the tables are monotonic: first row's start to last row's end), inside the image and the LDS
  const int r0 = imin(imax(a.ymin[y0], 0), a.h);
  const int r1 = imin(a.ymin[y0 + th - 1] + a.ysize[y0 + th - 1], a.h);
  const int nrows = imin(r1 - r0, a.rows_cap);
  const int tid = threadIdx.x;

  // ---- 1. horizontal pass into LDS
  if (tid < HT) {
    const int xo = tid / 3, ch = tid - xo * 3;
    const bool left = KIND == RS_YUV422 && xo == RS_TW;   // the column left of the tile
    if (left || xo < tw) {
      const int xg = left ? imax(x0 - 1, 0) : x0 + xo;
      const int xs = imin(imax(a.xmin[xg], 0), a.w - 1);
      const int ks = imin(imin(a.xsize[xg], a.kx), a.w - xs);
      const float* wrow = a.wx + (size_t)xg * a.kx;
      const float* p = a.t + (((size_t)n * a.h + r0) * a.w + xs) * 3 + ch;
      const size_t pitch = (size_t)a.w * 3;
      if constexpr (KXS > 0) {
        float wk[KXS];
#pragma unroll
        for (int k = 0; k < KXS; ++k) wk[k] = k < ks ? wrow[k] : 0.f;
        for (int row = 0; row < nrows; ++row, p += pitch) {
          float s = 0.f;
#pragma unroll
          for (int k = 0; k < KXS; ++k)
            if (k < ks) s += wk[k] * ((p[3 * k] + 1.f) / 2.f);
          lds[row * ROWF + tid] = s;
        }
      } else {
        for (int row = 0; row < nrows; ++row, p += pitch) {
          float s = 0.f;
          for (int k = 0; k < ks; ++k) s += wrow[k] * ((p[3 * k] + 1.f) / 2.f);
          lds[row * ROWF + tid] = s;
        }
      }
    } else {
      for (int row = 0; row < nrows; ++row) lds[row * ROWF + tid] = 0.f;   // (the 16-byte reads of the last unit of a partial tile)
    }
  }
  __syncthreads();

  // ---- 2. vertical pass from LDS, conversion, store
  if constexpr (KIND == FSR_OUT_F32 || KIND == FSR_OUT_U8) {
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int run = tw * 3, e0 = lane * 4;
    for (int r = wave; r < th; r += 4) {
      const int yo = y0 + r;
      const int j0 = imax(a.ymin[yo] - r0, 0);
      const int ks = imin(imin(a.ysize[yo], a.ky), nrows - j0);
      if (e0 >= run) continue;
      const float* wrow = a.wy + (size_t)yo * a.ky;
      const float* col = lds + j0 * RS_ROWF + e0;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int j = 0; j < ks; ++j) acc += wrow[j] * *(const f32x4*)(col + j * RS_ROWF);
      const size_t o = (((size_t)n * a.oh + yo) * a.ow + x0) * 3 + e0;
      const int cnt = imin(4, run - e0);
      if constexpr (KIND == FSR_OUT_F32) {
        float* q = (float*)a.out + o;
        const f32x4 v = 2.f * acc - 1.f;
        if (cnt == 4 && ((size_t)q & 15) == 0) {
          *(f32x4*)q = v;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (i < cnt) q[i] = v[i];
        }
      } else {
        unsigned char by[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) by[i] = (unsigned char)(clamp01(acc[i]) * 255.f);
        store_codes4((unsigned char*)a.out + o, by, cnt);
      }
    }
  } else if constexpr (KIND == RS_YUV422 || KIND == RS_YUV444) {
    constexpr int CHROMA = KIND - 8;
    const i420_coef kc = i420_coefs(a.matrix, a.full, sizeof(C) == 1 ? 8 : a.depth);
    const size_t plane = (size_t)a.oh * a.ow;
    C* frame = (C*)a.out + (size_t)n * (plane + 2 * ((size_t)a.oh * (size_t)(CHROMA == FSR_CHROMA_444 ? a.ow : a.ow >> 1)));
    const int nitems = th * (RS_TW / 4);
    for (int i = tid; i < nitems; i += 256) {
      const int r = i / (RS_TW / 4), xl = (i - r * (RS_TW / 4)) * 4;
      if (xl >= tw) continue;
      const int yo = y0 + r;
      const int j0 = imax(a.ymin[yo] - r0, 0);
      const int ks = imin(imin(a.ysize[yo], a.ky), nrows - j0);
      const float* wrow = a.wy + (size_t)yo * a.ky;
      const float* col = lds + j0 * ROWF + xl * 3;
      // 4:2:2: the three floats of the column to the left end the 16 bytes in front of the lane's own, or are the row's 65th column
      const float* lcol = lds + j0 * ROWF + (xl ? xl * 3 - 4 : RS_ROWF);
      f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, al = a0;
      for (int j = 0; j < ks; ++j) {
        const float wj = wrow[j];
        const f32x4* q = (const f32x4*)(col + j * ROWF);
        a0 += wj * q[0];
        a1 += wj * q[1];
        a2 += wj * q[2];
        if constexpr (CHROMA == FSR_CHROMA_422) al += wj * *(const f32x4*)(lcol + j * ROWF);
      }
      float v[12], vl[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[k] = clamp01(a0[k]);
        v[4 + k] = clamp01(a1[k]);
        v[8 + k] = clamp01(a2[k]);
      }
      if constexpr (CHROMA == FSR_CHROMA_422) {
#pragma unroll
        for (int k = 0; k < 3; ++k) vl[k] = clamp01(xl ? al[k + 1] : al[k]);
      }
      yuv_store_1x4<C, CHROMA>(kc, v, vl, frame, a.oh, a.ow, yo, x0 + xl, imin(4, tw - xl));
    }
  } else {
    const i420_coef kc = i420_coefs(a.matrix, a.full, sizeof(C) == 1 ? 8 : a.depth);
    const size_t plane = (size_t)a.oh * a.ow;
    C* frame = (C*)a.out + (size_t)n * (plane + 2 * ((size_t)(a.oh >> 1) * (size_t)(a.ow >> 1)));
    const int nitems = (th >> 1) * (RS_TW / 4);
    for (int i = tid; i < nitems; i += 256) {
      const int rp = i / (RS_TW / 4), xl = (i - rp * (RS_TW / 4)) * 4;
      if (xl >= tw) continue;
      float v[2][12];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const int yo = y0 + 2 * rp + m;
        const int j0 = imax(a.ymin[yo] - r0, 0);
        const int ks = imin(imin(a.ysize[yo], a.ky), nrows - j0);
        const float* wrow = a.wy + (size_t)yo * a.ky;
        const float* col = lds + j0 * RS_ROWF + xl * 3;
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0;
        for (int j = 0; j < ks; ++j) {
          const float wj = wrow[j];
          const f32x4* q = (const f32x4*)(col + j * RS_ROWF);
          a0 += wj * q[0];
          a1 += wj * q[1];
          a2 += wj * q[2];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          v[m][k] = clamp01(a0[k]);
          v[m][4 + k] = clamp01(a1[k]);
          v[m][8 + k] = clamp01(a2[k]);
        }
      }
      // the lane's columns xl .. xl + 3 are two 2x2 blocks; cnt = 2 or 4: ow and the tile origin are even
      i420_store_2x4<C, KIND == RS_NV12>(kc, v, frame, a.oh, a.ow, y0 + 2 * rp, x0 + xl, imin(4, tw - xl),
                                         KIND == RS_NV12 && sizeof(C) == 2 ? 16 - a.depth : 0);
    }
  }
}

// Largest source-row window of any tile of `th` output rows: the tap ranges of dataloader.aa_bicubic_taps, in its arithmetic.
int window_rows(int in, int out, int th) {
  const double scale = (double)in / (double)out;
  const double support = scale >= 1.0 ? 2.0 * scale : 2.0;
  int rows = 1;
  for (long long y0 = 0; y0 < out; y0 += th) {
    const long long y1 = (y0 + th < out ? y0 + th : out) - 1;
    int lo = (int)(scale * ((double)y0 + 0.5) - support + 0.5);
    int hi = (int)(scale * ((double)y1 + 0.5) + support + 0.5);
    lo = lo < 0 ? 0 : lo;
    hi = hi > in ? in : hi;
    if (hi - lo > rows) rows = hi - lo;
  }
  return rows;
}

template <int KIND, typename C = unsigned char>
void launch_kind(const ResampleArgs& a, long long grid, size_t lds_bytes, hipStream_t stream) {
  if (a.kx <= 5)
    hipLaunchKernelGGL((resample_kernel<KIND, 5, C>), dim3((unsigned)grid), dim3(256), lds_bytes, stream, a);
  else if (a.kx <= 9)
    hipLaunchKernelGGL((resample_kernel<KIND, 9, C>), dim3((unsigned)grid), dim3(256), lds_bytes, stream, a);
  else
    hipLaunchKernelGGL((resample_kernel<KIND, 0, C>), dim3((unsigned)grid), dim3(256), lds_bytes, stream, a);
}

// The planar stages at the sample type C: 4:2:0 (FSR_OUT_I420), 4:2:2 or 4:4:4
template <typename C>
void launch_planar(int kind, const ResampleArgs& a, long long grid, size_t lds_bytes, hipStream_t stream) {
  if (kind == FSR_OUT_I420) launch_kind<FSR_OUT_I420, C>(a, grid, lds_bytes, stream);
  else if (kind == RS_NV12) launch_kind<RS_NV12, C>(a, grid, lds_bytes, stream);
  else if (kind == RS_YUV422) launch_kind<RS_YUV422, C>(a, grid, lds_bytes, stream);
  else launch_kind<RS_YUV444, C>(a, grid, lds_bytes, stream);
}

// chroma, depth (FSR_OUT_I420 only; FSR_CHROMA_420 and 8 otherwise): the subsampling of the planes and their bits per sample -- 8, or 9..16
// for 16-bit samples (fsr_resample_image_i420_deep, fsr_resample_image_yuv)
int resample_launch(const float* t, int n, int h, int w, int oh, int ow, const float* wy, const int* ymin, const int* ysize, int ky,
                    const float* wx, const int* xmin, const int* xsize, int kx, int out_kind, int chroma, int yuv_matrix, int yuv_full_range,
                    int depth, void* out, fsr_stream_t stream_, int layout = FSR_LAYOUT_PLANAR) {
  if (!t || !wy || !ymin || !ysize || !wx || !xmin || !xsize || !out) return fsr_fail(-1, "fsr_resample_image: null argument");
  if (n <= 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0 || ky <= 0 || kx <= 0)
    return fsr_fail(-2, "fsr_resample_image: bad sizes (n %d, %d x %d -> %d x %d, taps %d x %d)", n, h, w, oh, ow, ky, kx);
  if (out_kind != FSR_OUT_F32 && out_kind != FSR_OUT_U8 && out_kind != FSR_OUT_I420)
    return fsr_fail(-2, "fsr_resample_image: unknown output kind %d", out_kind);
  if (out_kind == FSR_OUT_I420)
    if (int rc = fsr_yuv_out_check("fsr_resample_image", "I420 output: ", chroma, oh, ow, yuv_matrix, yuv_full_range)) return rc;
  if ((long long)h * w >= (1LL << 31) || (long long)n * oh * ow >= (1LL << 31))
    return fsr_fail(-2, "fsr_resample_image: frames of 2^31 or more pixels are not supported");
  if ((long long)h > (long long)RS_MAX_RATIO * oh || (long long)w > (long long)RS_MAX_RATIO * ow)
    return fsr_fail(-2, "fsr_resample_image: down-scaling ratio %.3f x %.3f (%d x %d -> %d x %d) is beyond the supported %d", (double)h / oh,
                    (double)w / ow, h, w, oh, ow, RS_MAX_RATIO);
  // the kernel's KIND (FSR_LAYOUT_NV12 comes with FSR_OUT_I420 and 4:2:0 only: fsr_resample_image_yuv_ex has seen to it)
  const int kind = out_kind == FSR_OUT_I420 && chroma != FSR_CHROMA_420 ? 8 + chroma : (layout == FSR_LAYOUT_NV12 ? RS_NV12 : out_kind);
  const int rowf = rs_rowf(kind);
  int th = 32, rows = 0;
  for (;; th >>= 1) {
    rows = window_rows(h, oh, th);
    if ((size_t)rows * rowf * sizeof(float) <= (size_t)RS_LDS_BUDGET) break;
    if (th == 2)
      return fsr_fail(-2, "fsr_resample_image: down-scaling ratio %.3f (%d -> %d rows): the %d source rows of a tile do not fit %d bytes of LDS",
                      (double)h / oh, h, oh, rows, RS_LDS_BUDGET);
  }
  ResampleArgs a;
  a.t = t; a.n = n; a.h = h; a.w = w; a.oh = oh; a.ow = ow;
  a.wy = wy; a.ymin = ymin; a.ysize = ysize; a.ky = ky;
  a.wx = wx; a.xmin = xmin; a.xsize = xsize; a.kx = kx;
  a.th = th;
  a.tiles_x = (ow + RS_TW - 1) / RS_TW;
  a.tiles_y = (oh + th - 1) / th;
  a.rows_cap = rows;
  a.matrix = yuv_matrix; a.full = yuv_full_range;
  a.out = out;
  a.depth = depth;
  const long long grid = (long long)n * a.tiles_x * a.tiles_y;
  if (grid >= (1LL << 31)) return fsr_fail(-2, "fsr_resample_image: too many tiles (%lld)", grid);
  const size_t lds_bytes = (size_t)rows * rowf * sizeof(float);
  hipStream_t stream = (hipStream_t)stream_;
  if (kind == FSR_OUT_F32) launch_kind<FSR_OUT_F32>(a, grid, lds_bytes, stream);
  else if (kind == FSR_OUT_U8) launch_kind<FSR_OUT_U8>(a, grid, lds_bytes, stream);
  else if (depth == 8) launch_planar<unsigned char>(kind, a, grid, lds_bytes, stream);
  else launch_planar<unsigned short>(kind, a, grid, lds_bytes, stream);
  const char* name = kind == FSR_OUT_F32 ? "f32" : kind == FSR_OUT_U8 ? "u8" : kind == FSR_OUT_I420 ? "i420" : kind == RS_NV12 ? "nv12" : kind == RS_YUV422 ? "yuv422" : "yuv444";
  // the sample type: named for 16-bit samples, and for the 4:2:2 / 4:4:4 planes at either
  fsr_note_kernel("resample_kernel<%s,%d%s>", name, kx <= 5 ? 5 : (kx <= 9 ? 9 : 0), depth != 8 ? ",u16" : (kind > FSR_OUT_I420 ? ",u8" : ""));
  return fsr_check_launch("resample_kernel");
}

}  // namespace

extern "C" int fsr_resample_image(const float* t, int n, int h, int w, int oh, int ow, const float* wy, const int* ymin,
                                  const int* ysize, int ky, const float* wx, const int* xmin, const int* xsize, int kx, int out_kind,
                                  int yuv_matrix, int yuv_full_range, void* out, fsr_stream_t stream_) {
  return resample_launch(t, n, h, w, oh, ow, wy, ymin, ysize, ky, wx, xmin, xsize, kx, out_kind, FSR_CHROMA_420, yuv_matrix, yuv_full_range, 8, out, stream_);
}

extern "C" int fsr_resample_image_i420_deep(const float* t, int n, int h, int w, int oh, int ow, const float* wy, const int* ymin,
                                            const int* ysize, int ky, const float* wx, const int* xmin, const int* xsize, int kx,
                                            int yuv_matrix, int yuv_full_range, int depth, void* out, fsr_stream_t stream_) {
  if (depth < 9 || depth > 16) return fsr_fail(-2, "fsr_resample_image_i420_deep: depth %d is outside 9..16", depth);
  return resample_launch(t, n, h, w, oh, ow, wy, ymin, ysize, ky, wx, xmin, xsize, kx, FSR_OUT_I420, FSR_CHROMA_420, yuv_matrix, yuv_full_range, depth,
                         out, stream_);
}

extern "C" int fsr_resample_image_yuv(const float* t, int n, int h, int w, int oh, int ow, const float* wy, const int* ymin, const int* ysize,
                                      int ky, const float* wx, const int* xmin, const int* xsize, int kx, int chroma, int yuv_matrix,
                                      int yuv_full_range, int depth, void* out, fsr_stream_t stream_) {
  if (chroma != FSR_CHROMA_420 && chroma != FSR_CHROMA_422 && chroma != FSR_CHROMA_444)
    return fsr_fail(-2, "fsr_resample_image_yuv: unknown chroma subsampling %d", chroma);
  if (depth < 8 || depth > 16) return fsr_fail(-2, "fsr_resample_image_yuv: depth %d is outside 8..16", depth);
  if (depth > 8 && ((size_t)out & 1) != 0)
    return fsr_fail(-2, "fsr_resample_image_yuv: the payloads of 16-bit samples must be 2-byte aligned");
  return resample_launch(t, n, h, w, oh, ow, wy, ymin, ysize, ky, wx, xmin, xsize, kx, FSR_OUT_I420, chroma, yuv_matrix, yuv_full_range, depth, out,
                         stream_);
}

extern "C" int fsr_resample_image_yuv_ex(const float* t, int n, int h, int w, int oh, int ow, const float* wy, const int* ymin, const int* ysize,
                                         int ky, const float* wx, const int* xmin, const int* xsize, int kx, int chroma, int layout,
                                         int yuv_matrix, int yuv_full_range, int depth, void* out, fsr_stream_t stream_) {
  if (chroma != FSR_CHROMA_420 && chroma != FSR_CHROMA_422 && chroma != FSR_CHROMA_444)
    return fsr_fail(-2, "fsr_resample_image_yuv_ex: unknown chroma subsampling %d", chroma);
  if (int rc = fsr_yuv_layout_check("fsr_resample_image_yuv_ex", chroma, layout)) return rc;
  if (depth < 8 || depth > 16) return fsr_fail(-2, "fsr_resample_image_yuv_ex: depth %d is outside 8..16", depth);
  if (depth > 8 && ((size_t)out & 1) != 0)
    return fsr_fail(-2, "fsr_resample_image_yuv_ex: the payloads of 16-bit samples must be 2-byte aligned");
  return resample_launch(t, n, h, w, oh, ow, wy, ymin, ysize, ky, wx, xmin, xsize, kx, FSR_OUT_I420, chroma, yuv_matrix, yuv_full_range, depth, out,
                         stream_, layout);
}
