/* Per-call latency through the C ABI of the calls whose kernel form, grid and workspace come from csrc/spx_plan.hpp: the top-r
 * select, ShiftedNormL1B2 and one large group on a team of workgroups.  The method of tools/r4/c_latency.c: 1000 back-to-back
 * calls per row, best of 5 rounds after a warm-up round; stream time (spx_timer_*) and host issue time (clock_gettime around
 * the loop), us per call.  One process = one series; profiles/plan_c_latency.txt interleaves series of two builds.
 * Build: gcc -O2 -std=c11 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include tools/plan_c_latency.c -o plan_c_latency \
 *        -Lshiftedproximaloperators.jl_amd/lib -lspx -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,... */
#define _POSIX_C_SOURCE 200809L
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

#include "spx.h"

#define CHECK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, spx_last_error()); return 2; } } while (0)
#define HIPCHECK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return 3; } } while (0)
static double now_us(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec * 1e6 + t.tv_nsec * 1e-3; }

enum { TOPR, B2, GROUP1 };
static const struct { const char* name; int op; int64_t n; } rows[] = {
    {"spx_prox_indball_l0_binf r=n/100   1e4", TOPR, 10000},   {"spx_prox_indball_l0_binf r=n/100   1e5", TOPR, 100000},
    {"spx_prox_indball_l0_binf r=n/100   3e6", TOPR, 3000000}, {"spx_prox_indball_l0_binf r=n/100   1e7", TOPR, 10000000},
    {"spx_prox_l1_b2                     1e4", B2, 10000},     {"spx_prox_l1_b2                     3e6", B2, 3000000},
    {"spx_prox_l1_b2                     1e7", B2, 10000000},  {"spx_prox_group_l2_binf (1 group)   1e6", GROUP1, 1000000},
};

int main(void) {
  spx_ctx* ctx = NULL;
  CHECK(spx_ctx_create(0, &ctx));
  const int64_t nmax = 10000000;
  double *q, *x, *s, *y, *lam;
  HIPCHECK(hipMalloc((void**)&q, nmax * 8)); HIPCHECK(hipMalloc((void**)&x, nmax * 8)); HIPCHECK(hipMalloc((void**)&s, nmax * 8));
  HIPCHECK(hipMalloc((void**)&y, nmax * 8)); HIPCHECK(hipMalloc((void**)&lam, 8));
  CHECK(spx_synth_fill(ctx, x, nmax, 1, 0, 1, 1.0)); CHECK(spx_synth_fill(ctx, s, nmax, 1, 1, 0, 1.0));
  CHECK(spx_synth_fill(ctx, q, nmax, 1, 2, 1, 1.0));
  const double one_lambda = 100.0;
  HIPCHECK(hipMemcpy(lam, &one_lambda, 8, hipMemcpyHostToDevice));
  CHECK(spx_sync(ctx));
  printf("us per call through the C ABI: stream time (host issue time), 1000 back-to-back calls, best of 5\n");
  for (unsigned k = 0; k < sizeof(rows) / sizeof(rows[0]); ++k) {
    const int64_t n = rows[k].n;
    double best_ev = 1e30, best_host = 1e30;
    for (int rnd = 0; rnd < 6; ++rnd) {
      float ms = 0.0f;
      const double t0 = now_us();
      CHECK(spx_timer_start(ctx));
      for (int it = 0; it < 1000; ++it) {
        switch (rows[k].op) {
          case TOPR: CHECK(spx_prox_indball_l0_binf(ctx, y, q, x, s, n, n / 100, 1.0)); break;
          case B2: CHECK(spx_prox_l1_b2(ctx, y, q, x, s, n, 1.0, 1.0, 1.0, 1.0)); break;
          default: CHECK(spx_prox_group_l2_binf(ctx, y, q, x, s, n, NULL, n, 1, lam, 1.0, 1.0)); break;
        }
      }
      const double t1 = now_us();
      CHECK(spx_timer_stop(ctx, &ms));
      if (rnd == 0) continue; /* warm-up */
      if (ms < best_ev) best_ev = ms;
      if ((t1 - t0) / 1000.0 < best_host) best_host = (t1 - t0) / 1000.0;
    }
    printf("%-40s %9.2f (%7.2f)\n", rows[k].name, best_ev, best_host);
  }
  CHECK(spx_ctx_destroy(ctx));
  return 0;
}
