// The AdamW step of a flat float arena: ONE update kernel behind fsr_adamw_step, fsr_adamw_step_scaled and
// fsr_adamw_step_ex, with the dynamic loss scale's two small kernels (fsr_grad_nonfinite, fsr_loss_scale_update).
//
//   AdamW(lr, fused=True)           /root/reference/trainer.py:33-38
//
// The learning rate comes by value (SCHED = false: the first two entry points; a captured hipGraph replays the rate of the capture)
// or from a schedule block in DEVICE memory (SCHED = true): every wave evaluates the schedule from the block's clock (uniform,
// redundant, a few scalar operations), so multistep / cosine / warm-up schedules and a host rewrite of the block all take effect
// under replay.  An optional exponential moving average of the parameters is fused into the same pass (EMA).  No atomics and no
// cross-workgroup dependency: the kernel only reads the step count and the clock; a one-thread tick kernel enqueued behind it
// advances them.
//
// Memory: 128-bit loads and stores over the 16-byte aligned body, a scalar grid-stride loop for the tail (and for the whole
// range when any pointer is not 16-byte aligned).  The element update is fsr_adamw_update (fsr_adamw.h).
#include "fsr_adamw.h"
#include "fsr_common.h"
#include "fsr_host.h"

namespace {

// The learning rate of the update applied at clock e (updates applied so far): include/fsr_hip.h states the contract.
__device__ __forceinline__ float sched_lr(const float* __restrict__ s, float e) {
  float val;
  if (s[FSR_SCHED_KIND] == 2.f) {
    const float base = s[FSR_SCHED_BASE], T = s[FSR_SCHED_TOTAL], lo = s[FSR_SCHED_MIN];
    val = lo + 0.5f * (base - lo) * (1.f + cosf(3.14159265358979f * fminf(e, T) / T));
  } else {
    const int nb = (int)s[FSR_SCHED_NB];
    int k = 0;
    for (int i = 0; i < FSR_SCHED_MAX_BOUNDARIES; ++i) k += (i < nb && s[FSR_SCHED_BOUNDS + i] <= e) ? 1 : 0;
    val = s[FSR_SCHED_VALUES + k];
  }
  const float W = s[FSR_SCHED_WARMUP];
  return e < W ? val * ((e + 1.f) / W) : val;
}

// ema + (p' - ema) (1 - decay); one fused multiply-add on the device in the 128-bit and the scalar loop alike (fsr_adamw.h says why)
__device__ __forceinline__ float ema_update(float ema, float p, float om) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_fmaf(p - ema, om, ema);
#else
  return ema + (p - ema) * om;
#endif
}

// SCHED: the rate is sched_lr(sched, clock) and is reported in lr_used; else `lr` as passed, and the block is never touched.
// state (nullable): the loss-scale state; non-null divides the gradients by the scale and skips the whole step while the flag is up.
template <bool SCHED, bool EMA>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, float* __restrict__ ema, long long count, long long nvec,
                                                    float* sched, float lr, float b1, float b2, float eps, float wd,
                                                    const float* __restrict__ step, float gscale, const float* __restrict__ state,
                                                    float ema_decay) {
  if (state && state[2] != 0.f) return;     // a gradient overflowed: nothing is touched, lr_used included
  if (SCHED) {
    lr = sched_lr(sched, sched[FSR_SCHED_CLOCK]);
    if (blockIdx.x == 0 && threadIdx.x == 0) sched[FSR_SCHED_LR_USED] = lr;    // the one writer; no thread reads this word
  }
  const float t = step[0] + 1.f;            // adamw_tick_kernel, enqueued behind this kernel, advances step and clock
  const float gs = state ? gscale / state[0] : gscale;
  const float bc1 = 1.f - powf(b1, t);
  const float rsqrt_bc2 = 1.f / sqrtf(1.f - powf(b2, t));
  const float om = 1.f - ema_decay;
  const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  float4* __restrict__ p4 = reinterpret_cast<float4*>(p);
  const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
  float4* __restrict__ m4 = reinterpret_cast<float4*>(m);
  float4* __restrict__ v4 = reinterpret_cast<float4*>(v);
  float4* __restrict__ e4 = reinterpret_cast<float4*>(ema);
  for (long long i = tid; i < nvec; i += stride) {
    float4 pi = p4[i], mi = m4[i], vi = v4[i];
    const float4 gi = g4[i];
    fsr_adamw_update(pi.x, gi.x, gs, mi.x, vi.x, lr, b1, b2, eps, wd, bc1, rsqrt_bc2);
    fsr_adamw_update(pi.y, gi.y, gs, mi.y, vi.y, lr, b1, b2, eps, wd, bc1, rsqrt_bc2);
    fsr_adamw_update(pi.z, gi.z, gs, mi.z, vi.z, lr, b1, b2, eps, wd, bc1, rsqrt_bc2);
    fsr_adamw_update(pi.w, gi.w, gs, mi.w, vi.w, lr, b1, b2, eps, wd, bc1, rsqrt_bc2);
    m4[i] = mi;
    v4[i] = vi;
    p4[i] = pi;
    if (EMA) {
      float4 ei = e4[i];
      ei.x = ema_update(ei.x, pi.x, om);
      ei.y = ema_update(ei.y, pi.y, om);
      ei.z = ema_update(ei.z, pi.z, om);
      ei.w = ema_update(ei.w, pi.w, om);
      e4[i] = ei;
    }
  }
  for (long long i = nvec * 4 + tid; i < count; i += stride) {
    float pi = p[i], mi = m[i], vi = v[i];
    fsr_adamw_update(pi, g[i], gs, mi, vi, lr, b1, b2, eps, wd, bc1, rsqrt_bc2);
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
    if (EMA) ema[i] = ema_update(ema[i], pi, om);
  }
}

// The step count (and the clock, where there is a block) live in device memory as floats so that a captured hipGraph replays
// correctly.  Plain form (state = null): always; scaled form: only when the step was clean.
__global__ void adamw_tick_kernel(float* __restrict__ step, float* __restrict__ sched, const float* __restrict__ state) {
  if (threadIdx.x == 0 && (!state || state[2] == 0.f)) {
    step[0] += 1.f;
    if (sched) sched[FSR_SCHED_CLOCK] += 1.f;
  }
}

// ---- dynamic loss scaling (fp16 mode).  state: float[4] on the device = {scale, clean steps, non-finite flag, skipped steps}.
// Everything is decided on the device, so a captured hipGraph keeps adapting while it replays.
__global__ __launch_bounds__(256) void grad_nonfinite_kernel(const float* __restrict__ g, long long count, float* __restrict__ state) {
  bool bad = false;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
    const float x = g[i];
    bad |= !(fabsf(x) <= 3.0e38f);   // inf or NaN
  }
  if (bad) state[2] = 1.f;           // every writer stores the same value: no atomic needed
}

__global__ void loss_scale_update_kernel(float* __restrict__ state, float growth_interval, float growth, float backoff) {
  if (threadIdx.x != 0) return;
  if (state[2] != 0.f) {             // overflow in this iteration: back off, start counting again
    state[0] = fmaxf(state[0] * backoff, 1.f);
    state[1] = 0.f;
    state[3] += 1.f;
    state[2] = 0.f;
  } else {
    state[1] += 1.f;
    if (state[1] >= growth_interval) {
      state[0] = fminf(state[0] * growth, 16777216.f);
      state[1] = 0.f;
    }
  }
}

// The update and its tick for all three entry points (sched null: the rate is `lr`; ema and state nullable).  Returns nvec, the
// 128-bit units of the body: 0 when a pointer is not 16-byte aligned.
long long adamw_launch(float* p, const float* g, float* m, float* v, float* ema, long long count, float* sched, float lr, float b1,
                       float b2, float eps, float wd, float* step, float gscale, const float* state, float ema_decay,
                       hipStream_t stream) {
  const bool aligned = ((((size_t)p | (size_t)g | (size_t)m | (size_t)v | (size_t)ema) & 15) == 0);
  const long long nvec = aligned ? count / 4 : 0;
  long long blocks = (count + 256 * 4 - 1) / (256 * 4);
  if (blocks > 2048) blocks = 2048;
  auto kernel = sched ? (ema ? adamw_kernel<true, true> : adamw_kernel<true, false>)
                      : (ema ? adamw_kernel<false, true> : adamw_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, stream, p, g, m, v, ema, count, nvec, sched, lr, b1, b2, eps, wd,
                     step, gscale, state, ema_decay);
  // The tick runs BEHIND the update, which reads step[0] + 1.  (fsr_adamw_step used to tick first and read step[0]: the same float.)
  hipLaunchKernelGGL(adamw_tick_kernel, dim3(1), dim3(64), 0, stream, step, sched, state);
  return nvec;
}

}  // namespace

extern "C" int fsr_adamw_step(float* p, const float* g, float* m, float* v, long long count, float lr, float beta1,
                              float beta2, float eps, float weight_decay, float* step_counter, float grad_scale,
                              fsr_stream_t stream_) {
  if (!p || !g || !m || !v || !step_counter || count <= 0) return fsr_fail(-1, "fsr_adamw_step: bad argument");
  adamw_launch(p, g, m, v, nullptr, count, nullptr, lr, beta1, beta2, eps, weight_decay, step_counter, grad_scale, nullptr, 0.f,
               (hipStream_t)stream_);
  fsr_note_kernel("adamw_kernel");
  return fsr_check_launch("adamw_kernel");
}

extern "C" int fsr_adamw_step_scaled(float* p, const float* g, float* m, float* v, long long count, float lr, float beta1,
                                     float beta2, float eps, float weight_decay, float* step_counter, float grad_scale,
                                     const float* scale_state, fsr_stream_t stream_) {
  if (!p || !g || !m || !v || !step_counter || !scale_state || count <= 0) return fsr_fail(-1, "fsr_adamw_step_scaled: bad argument");
  adamw_launch(p, g, m, v, nullptr, count, nullptr, lr, beta1, beta2, eps, weight_decay, step_counter, grad_scale, scale_state, 0.f,
               (hipStream_t)stream_);
  fsr_note_kernel("adamw_scaled_kernel");
  return fsr_check_launch("adamw_scaled_kernel");
}

extern "C" int fsr_adamw_step_ex(float* p, const float* g, float* m, float* v, float* ema, long long count, float* sched,
                                 float beta1, float beta2, float eps, float weight_decay, float* step_counter, float grad_scale,
                                 const float* scale_state, float ema_decay, fsr_stream_t stream_) {
  if (!p || !g || !m || !v || !sched || !step_counter) return fsr_fail(-1, "fsr_adamw_step_ex: null argument");
  if (count <= 0) return fsr_fail(-1, "fsr_adamw_step_ex: count %lld must be positive", count);
  if (ema && !(ema_decay >= 0.f && ema_decay < 1.f)) return fsr_fail(-1, "fsr_adamw_step_ex: ema_decay %g is outside [0, 1)", (double)ema_decay);
  const long long nvec = adamw_launch(p, g, m, v, ema, count, sched, 0.f, beta1, beta2, eps, weight_decay, step_counter, grad_scale,
                                      scale_state, ema_decay, (hipStream_t)stream_);
  fsr_note_kernel("adamw_ex_kernel<%s,%s,%s>", ema ? "ema" : "noema", scale_state ? "scaled" : "plain", nvec ? "x4" : "x1");
  return fsr_check_launch("adamw_ex_kernel");
}

extern "C" int fsr_grad_nonfinite(const float* g, long long count, float* scale_state, fsr_stream_t stream_) {
  if (!g || !scale_state || count <= 0) return fsr_fail(-1, "fsr_grad_nonfinite: bad argument");
  long long blocks = (count + 256 * 8 - 1) / (256 * 8);
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(grad_nonfinite_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, g, count, scale_state);
  return fsr_check_launch("grad_nonfinite_kernel");
}

extern "C" int fsr_loss_scale_update(float* scale_state, float growth_interval, float growth, float backoff, fsr_stream_t stream_) {
  if (!scale_state || !(growth_interval >= 1.f) || !(growth >= 1.f) || !(backoff > 0.f && backoff <= 1.f))
    return fsr_fail(-1, "fsr_loss_scale_update: bad argument");
  hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream_, scale_state, growth_interval, growth, backoff);
  return fsr_check_launch("loss_scale_update_kernel");
}
