// The AdamW element update of adamw_kernel (optim.hip): its 128-bit loop, its scalar loop and all four instantiations.
//
// Their results are pinned bit for bit (tests/golden/adamw_bits.npz, tests/test_optim_ex.py), and the library is built with
// -ffp-contract=fast, under which a*b - c*d may become fma(a, b, -(c*d)) in one loop and fma(-c, d, a*b) in another (the 128-bit and
// the scalar loop did differ that way).  So on the device every rounding is spelled out: the fused operations are explicit fmaf calls,
// and a product that must be rounded on its own goes through FSR_ROUNDED, an empty asm statement the compiler cannot contract across.
// The sequence is the one the first, scalar AdamW kernels compiled to, which the recorded bits come from:
//   gi = g gs;  m' = fma(1 - b1, fma(gs, g, -m), m);  v' = rnd(v b2) + rnd(((1 - b2) gi) gi);
//   denom = fma(sqrt(v'), rsqrt_bc2, eps);  p' = rnd(p fma(-lr, wd, 1)) - rnd((lr / bc1) (m' / denom)).
// The host build of the emulator keeps the plain expressions (one rounding per operation).
#pragma once
#include <hip/hip_runtime.h>

#if defined(__HIP_DEVICE_COMPILE__)
#define FSR_ROUNDED(x) asm("" : "+v"(x))
#endif

// g: the raw gradient, gs: grad_scale (/ loss scale); bc1 = 1 - b1^t, rsqrt_bc2 = 1 / sqrt(1 - b2^t)
__device__ __forceinline__ void fsr_adamw_update(float& p, float g, float gs, float& m, float& v, float lr, float b1, float b2,
                                                 float eps, float wd, float bc1, float rsqrt_bc2) {
#if defined(__HIP_DEVICE_COMPILE__)
  const float gi = g * gs;
  const float mi = __builtin_fmaf(1.f - b1, __builtin_fmaf(gs, g, -m), m);   // torch: exp_avg.lerp_(grad, 1 - beta1)
  float vb = v * b2, gg = ((1.f - b2) * gi) * gi;
  FSR_ROUNDED(vb);
  FSR_ROUNDED(gg);
  const float vi = vb + gg;
  const float denom = __builtin_fmaf(sqrtf(vi), rsqrt_bc2, eps);
  float pd = p * __builtin_fmaf(-lr, wd, 1.f), up = (lr / bc1) * (mi / denom);
  FSR_ROUNDED(pd);
  FSR_ROUNDED(up);
  m = mi;
  v = vi;
  p = pd - up;
#else
  const float gi = g * gs;
  float pi = p * (1.f - lr * wd);
  const float mi = m + (gi - m) * (1.f - b1);   // torch: exp_avg.lerp_(grad, 1 - beta1)
  const float vi = v * b2 + (1.f - b2) * gi * gi;
  m = mi;
  v = vi;
  const float denom = sqrtf(vi) * rsqrt_bc2 + eps;
  pi -= (lr / bc1) * (mi / denom);
  p = pi;
#endif
}
