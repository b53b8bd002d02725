// Stand-alone host program for sanitizer runs of every entry point of csrc/optim.hip (fsr_adamw_step, fsr_adamw_step_scaled,
// fsr_adamw_step_ex, fsr_grad_nonfinite, fsr_loss_scale_update), compiled through the emulator's headers, no Python.
//
//   E=tests/emu; C=fast-srgan_amd/csrc
//   clang++ -x c++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -I $E/include -I include -I $C $E/adamw_ex_host.cpp $C/optim.hip $E/emu_runtime.cpp -o adamw_ex_host && ASAN_OPTIONS=detect_leaks=0 ./adamw_ex_host
//
// (detect_leaks=0: the emulator keeps its fiber stacks for the next launch and never frees the last set, emu_runtime.cpp run_workgroups.)
//
// Every buffer is a heap allocation of EXACTLY the bytes the call may touch (a read or write one element past the end is
// reported), at counts 1, 5 and 1025, 16-byte aligned and offset by one float, with and without the EMA and the loss-scale state;
// the by-value entry points and the loss-scale pair run on the same buffers behind the ten block-rate steps.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <stdarg.h>

#include "fsr_hip.h"

// the three host helpers of csrc/fsr_host.h that optim.hip calls (csrc/fsr_api.hip would pull every kernel family in)
static char g_err[256], g_kernel[160];
int fsr_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
int fsr_check_launch(const char*) { return 0; }
void fsr_note_kernel(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_kernel, sizeof(g_kernel), fmt, ap);
  va_end(ap);
}

int main() {
  const long long counts[3] = {1, 5, 1025};
  int calls = 0;
  for (int ci = 0; ci < 3; ++ci)
    for (int offset = 0; offset < 2; ++offset)
      for (int with_ema = 0; with_ema < 2; ++with_ema)
        for (int scaled = 0; scaled < 2; ++scaled) {
          const long long n = counts[ci];
          // the tail of a malloc block is only poisoned from its requested size on: request exactly (n + offset) floats
          float* p = (float*)malloc((size_t)(n + offset) * 4);
          float* g = (float*)malloc((size_t)(n + offset) * 4);
          float* m = (float*)malloc((size_t)(n + offset) * 4);
          float* v = (float*)malloc((size_t)(n + offset) * 4);
          float* e = (float*)malloc((size_t)(n + offset) * 4);
          for (long long i = 0; i < n + offset; ++i) {
            p[i] = 1e-3f * (float)(i % 11 - 5);
            g[i] = 0.1f * (float)(i % 5 - 2) * (scaled ? 1024.f : 1.f);
            m[i] = 0.f;
            v[i] = 0.f;
            e[i] = p[i];
          }
          float* sched = (float*)calloc(FSR_SCHED_WORDS, 4);
          sched[FSR_SCHED_KIND] = 1.f;
          sched[FSR_SCHED_BASE] = 1e-4f;
          sched[FSR_SCHED_WARMUP] = 2.f;
          sched[FSR_SCHED_NB] = 8.f;
          for (int i = 0; i < 8; ++i) sched[FSR_SCHED_BOUNDS + i] = (float)(i + 1);
          for (int i = 0; i < 9; ++i) sched[FSR_SCHED_VALUES + i] = 1e-4f * powf(0.5f, (float)i);
          float* step = (float*)calloc(1, 4);
          float* state = (float*)calloc(4, 4);
          state[0] = 1024.f;
          for (int it = 0; it < 10; ++it) {
            const int rc = fsr_adamw_step_ex(p + offset, g + offset, m + offset, v + offset, with_ema ? e + offset : nullptr, n, sched, 0.9f,
                                             0.999f, 1e-8f, 0.01f, step, 1.f, scaled ? state : nullptr, 0.9f, nullptr);
            if (rc != 0) {
              fprintf(stderr, "fsr_adamw_step_ex failed: %s\n", g_err);
              return 1;
            }
            ++calls;
          }
          if (step[0] != 10.f || sched[FSR_SCHED_CLOCK] != 10.f || sched[FSR_SCHED_LR_USED] != sched[FSR_SCHED_VALUES + 8] || !(p[offset] == p[offset])) {
            fprintf(stderr, "count %lld offset %d: step %g clock %g lr_used %g\n", n, offset, step[0], sched[FSR_SCHED_CLOCK], sched[FSR_SCHED_LR_USED]);
            return 1;
          }
          // the by-value entry points on the same buffers (once per EMA setting is enough: they take none), then the loss-scale pair
          if (!with_ema) {
            const int rc = scaled ? (fsr_grad_nonfinite(g + offset, n, state, nullptr) ||
                                     fsr_adamw_step_scaled(p + offset, g + offset, m + offset, v + offset, n, 1e-4f, 0.9f, 0.999f, 1e-8f, 0.01f,
                                                           step, 1.f, state, nullptr) ||
                                     fsr_loss_scale_update(state, 2.f, 2.f, 0.5f, nullptr))
                                  : fsr_adamw_step(p + offset, g + offset, m + offset, v + offset, n, 1e-4f, 0.9f, 0.999f, 1e-8f, 0.01f, step, 1.f,
                                                   nullptr);
            if (rc != 0) {
              fprintf(stderr, "by-value entry point failed: %s\n", g_err);
              return 1;
            }
            calls += scaled ? 3 : 1;
            if (step[0] != 11.f || sched[FSR_SCHED_CLOCK] != 10.f || (scaled && (state[1] != 1.f || state[2] != 0.f)) || !(p[offset] == p[offset])) {
              fprintf(stderr, "count %lld offset %d by value: step %g clock %g\n", n, offset, step[0], sched[FSR_SCHED_CLOCK]);
              return 1;
            }
          }
          free(p), free(g), free(m), free(v), free(e), free(sched), free(step), free(state);
        }
  printf("adamw_ex_host: %d calls, kernel %s\n", calls, g_kernel);
  return 0;
}
