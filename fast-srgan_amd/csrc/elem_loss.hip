// Strided element-wise losses between two float32 [n,c,h,w] operands: the pixel term of the training objective
// and the least-squares adversarial term.
//
//   loss = sum psi(a - b) / count            da = gscale[0] / count * psi'(a - b)            count = n c h w
//
//   FSR_LOSS_L1           psi(d) = |d|                      psi'(d) = sign(d), 0 at 0 (torch's convention)
//   FSR_LOSS_SMOOTH_L1    the expressions of smooth_l1_fwd_kernel / smooth_l1_bwd_kernel (losses.hip), beta 1
//   FSR_LOSS_CHARBONNIER  psi(d) = sqrt(d d + eps eps)      psi'(d) = d / sqrt(d d + eps eps)
//   FSR_LOSS_MSE          psi(d) = d d                      psi'(d) = 2 d
//
// Each operand is read through its own four strides (in elements): the generator's output is the (N,3,H,W) view of an NHWC buffer,
// the loader's batch is planar, a label tensor is a slice -- nothing is copied into a common layout first.  Lanes map to PIXELS and
// the channel loop runs inside the thread: on an NHWC operand the 64 lanes of a wave cover one contiguous run of 64 c floats (c
// loads, every fetched line used whole), on a planar operand each of the c loads is a coalesced 256-byte run of one plane.  The
// gradient is written through a's strides by the same mapping.  Pixels are taken in a grid-stride loop by at most 1024 workgroups
// (the cap of losses.hip's red_blocks()); the loss is the project's order-fixed two-level sum: lane partials -> wave shuffle -> LDS ->
// one slot of `scratch` per workgroup, added in slot order by reduce.hip (no float atomics, bit-reproducible).
#include "fsr_common.h"
#include "fsr_host.h"
#include "fsr_hip.h"

namespace {

constexpr int ELEM_MAX_BLOCKS = 1024;

struct ElemOperand {
  const float* p;
  long long sn, sc, sh, sw;
};
// pixels = n * hw; a pixel index splits into image / row / column only as far as the strides need it (the host merges h and w
// into one axis of hw "columns" when both operands step through them uniformly)
struct ElemShape {
  unsigned pixels, hw, w;   // the entry points refuse 2^31 elements and more: 32-bit index arithmetic (two divisions per pixel)
  int c;
};

template <int KIND>
__device__ __forceinline__ float elem_psi(float d, float e2) {
  if constexpr (KIND == FSR_LOSS_L1) return fabsf(d);
  if constexpr (KIND == FSR_LOSS_SMOOTH_L1) {
    const float ad = fabsf(d);
    return ad < 1.f ? 0.5f * ad * ad : ad - 0.5f;
  }
  if constexpr (KIND == FSR_LOSS_CHARBONNIER) return sqrtf(d * d + e2);
  return d * d;
}

template <int KIND>
__device__ __forceinline__ float elem_dpsi(float d, float e2) {
  if constexpr (KIND == FSR_LOSS_L1) return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  if constexpr (KIND == FSR_LOSS_SMOOTH_L1) return fminf(fmaxf(d, -1.f), 1.f);
  if constexpr (KIND == FSR_LOSS_CHARBONNIER) return d / sqrtf(d * d + e2);
  return 2.f * d;
}

__device__ __forceinline__ void elem_offsets(const ElemShape& s, const ElemOperand& a, const ElemOperand& b, unsigned p,
                                             long long& oa, long long& ob) {
  const unsigned img = p / s.hw, r = p - img * s.hw;
  const unsigned y = s.w == s.hw ? 0u : r / s.w, x = r - y * s.w;   // merged rows (uniform branch): one division per pixel
  oa = (long long)img * a.sn + (long long)y * a.sh + (long long)x * a.sw;
  ob = (long long)img * b.sn + (long long)y * b.sh + (long long)x * b.sw;
}

template <int KIND>
__global__ __launch_bounds__(256) void elem_loss_fwd_kernel(ElemShape s, ElemOperand a, ElemOperand b, float e2,
                                                            float* __restrict__ partial) {
  __shared__ float red4[4];
  float sum = 0.f;
  for (unsigned p = blockIdx.x * 256 + threadIdx.x; p < s.pixels; p += gridDim.x * 256) {   // < 2^31 + 2^18: no wrap
    long long oa, ob;
    elem_offsets(s, a, b, p, oa, ob);
    for (int ch = 0; ch < s.c; ++ch) sum += elem_psi<KIND>(a.p[oa + ch * a.sc] - b.p[ob + ch * b.sc], e2);
  }
  sum = wave_sum(sum);
  if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = red4[0] + red4[1] + red4[2] + red4[3];   // the mean is finished by reduce.hip
}

template <int KIND>
__global__ __launch_bounds__(256) void elem_loss_bwd_kernel(ElemShape s, ElemOperand a, ElemOperand b, float e2,
                                                            const float* __restrict__ gscale, float* __restrict__ da, float inv) {
  const float gs = gscale[0] * inv;
  for (unsigned p = blockIdx.x * 256 + threadIdx.x; p < s.pixels; p += gridDim.x * 256) {   // < 2^31 + 2^18: no wrap
    long long oa, ob;
    elem_offsets(s, a, b, p, oa, ob);
    for (int ch = 0; ch < s.c; ++ch)
      da[oa + ch * a.sc] = gs * elem_dpsi<KIND>(a.p[oa + ch * a.sc] - b.p[ob + ch * b.sc], e2);
  }
}

// every axis longer than 1 must step over the whole extent of the axes below it: no negative, zero or interleaved strides
int strides_ok(const long long st[4], const int sz[4]) {
  int order[4], k = 0;
  for (int i = 0; i < 4; ++i)
    if (sz[i] > 1) {
      if (st[i] <= 0) return 0;
      int j = k++;
      for (; j > 0 && st[order[j - 1]] > st[i]; --j) order[j] = order[j - 1];
      order[j] = i;
    }
  long long extent = 1;   // one past the largest offset the axes so far can reach
  for (int j = 0; j < k; ++j) {
    if (st[order[j]] < extent) return 0;
    extent = st[order[j]] * (sz[order[j]] - 1) + extent;
  }
  return 1;
}

int elem_prepare(const char* who, int kind, float param, const float* a, const long long sa[4], const float* b, const long long sb[4],
                 int n, int c, int h, int w, ElemShape& s, ElemOperand& oa, ElemOperand& ob, float& e2, int& blocks) {
  if (!a || !b) return fsr_fail(-1, "%s: null argument", who);
  if (kind != FSR_LOSS_L1 && kind != FSR_LOSS_SMOOTH_L1 && kind != FSR_LOSS_CHARBONNIER && kind != FSR_LOSS_MSE)
    return fsr_fail(-2, "%s: unknown loss kind %d", who, kind);
  if (kind == FSR_LOSS_CHARBONNIER && !(param > 0.f && param <= 3.0e38f))
    return fsr_fail(-2, "%s: Charbonnier's eps must be positive and finite, got %g", who, (double)param);
  if (n <= 0 || c <= 0 || h <= 0 || w <= 0) return fsr_fail(-2, "%s: n, c, h and w must be positive, got %d, %d, %d, %d", who, n, c, h, w);
  const long long count = (long long)n * c * h * w;
  if (count >= (1LL << 31)) return fsr_fail(-2, "%s: %lld elements, the limit is 2^31 - 1", who, count);
  const int sz[4] = {n, c, h, w};
  if (!strides_ok(sa, sz) || !strides_ok(sb, sz))
    return fsr_fail(-2, "%s: strides must be positive and must not overlap (a: %lld %lld %lld %lld, b: %lld %lld %lld %lld)", who, sa[0],
                    sa[1], sa[2], sa[3], sb[0], sb[1], sb[2], sb[3]);
  oa = ElemOperand{a, sa[0], sa[1], sa[2], sa[3]};
  ob = ElemOperand{b, sb[0], sb[1], sb[2], sb[3]};
  s = ElemShape{(unsigned)(count / c), (unsigned)(h * w), (unsigned)w, c};
  if (sa[2] == sa[3] * w && sb[2] == sb[3] * w) s.w = s.hw;   // rows follow each other uniformly in both operands: one axis
  e2 = param * param;
  const unsigned need = (s.pixels + 255) / 256;
  blocks = (int)(need > ELEM_MAX_BLOCKS ? ELEM_MAX_BLOCKS : need);
  return 0;
}

}  // namespace

extern "C" size_t fsr_elem_loss_scratch(void) { return ELEM_MAX_BLOCKS * sizeof(float); }

#define FSR_ELEM_DISPATCH(KERNEL, ...)                                                                                    \
  switch (kind) {                                                                                                         \
    case FSR_LOSS_L1: hipLaunchKernelGGL(KERNEL<FSR_LOSS_L1>, dim3(blocks), dim3(256), 0, stream, __VA_ARGS__); break;    \
    case FSR_LOSS_SMOOTH_L1: hipLaunchKernelGGL(KERNEL<FSR_LOSS_SMOOTH_L1>, dim3(blocks), dim3(256), 0, stream, __VA_ARGS__); break; \
    case FSR_LOSS_CHARBONNIER: hipLaunchKernelGGL(KERNEL<FSR_LOSS_CHARBONNIER>, dim3(blocks), dim3(256), 0, stream, __VA_ARGS__); break; \
    default: hipLaunchKernelGGL(KERNEL<FSR_LOSS_MSE>, dim3(blocks), dim3(256), 0, stream, __VA_ARGS__); break;            \
  }

extern "C" int fsr_elem_loss_fwd(int kind, float param, const float* a, long long sa_n, long long sa_c, long long sa_h, long long sa_w,
                                 const float* b, long long sb_n, long long sb_c, long long sb_h, long long sb_w, int n, int c, int h,
                                 int w, float* loss, void* scratch, fsr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!loss || !scratch) return fsr_fail(-1, "fsr_elem_loss_fwd: null argument");
  const long long sa[4] = {sa_n, sa_c, sa_h, sa_w}, sb[4] = {sb_n, sb_c, sb_h, sb_w};
  ElemShape s;
  ElemOperand oa, ob;
  float e2;
  int blocks;
  if (int rc = elem_prepare("fsr_elem_loss_fwd", kind, param, a, sa, b, sb, n, c, h, w, s, oa, ob, e2, blocks)) return rc;
  FSR_ELEM_DISPATCH(elem_loss_fwd_kernel, s, oa, ob, e2, (float*)scratch)
  if (int rc = fsr_check_launch("elem_loss_fwd_kernel")) return rc;
  return fsr_launch_reduce_partials((const float*)scratch, loss, 1, blocks, 1, 1, 0, 0, 1.f / (float)((long long)s.pixels * c), 0, stream);
}

extern "C" int fsr_elem_loss_bwd(int kind, float param, const float* a, long long sa_n, long long sa_c, long long sa_h, long long sa_w,
                                 const float* b, long long sb_n, long long sb_c, long long sb_h, long long sb_w, const float* gscale,
                                 float* da, int n, int c, int h, int w, fsr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!gscale || !da) return fsr_fail(-1, "fsr_elem_loss_bwd: null argument");
  const long long sa[4] = {sa_n, sa_c, sa_h, sa_w}, sb[4] = {sb_n, sb_c, sb_h, sb_w};
  ElemShape s;
  ElemOperand oa, ob;
  float e2;
  int blocks;
  if (int rc = elem_prepare("fsr_elem_loss_bwd", kind, param, a, sa, b, sb, n, c, h, w, s, oa, ob, e2, blocks)) return rc;
  FSR_ELEM_DISPATCH(elem_loss_bwd_kernel, s, oa, ob, e2, gscale, da, 1.f / (float)((long long)s.pixels * c))
  return fsr_check_launch("elem_loss_bwd_kernel");
}
