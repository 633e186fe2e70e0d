/* Stand-alone driver of the Float32 psi(y) / ShiftedGroupNormL2.prox! restatements (oracle/spx_oracle_f32.c), built with
 * -fsanitize=address,undefined (oracle/Makefile: f32_driver_asan) and run as a child by tests/test_oracle_f32_forms.py.
 * Every vector is a heap block of exactly its length: a read or write one element outside is a sanitizer report.
 * Covers n = 0, n = 1, odd n, CSR offsets with empty groups, and a head and a tail in no group.  Prints "ok" and returns 0. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

int orc32_obj_terms(double* terms, int kind, int mode, const float* y, const float* xk, const float* sj, int64_t n,
                    const float* lvec, const float* uvec, float lscal, float uscal, const uint8_t* mask, float delta);
int orc32_obj_group_terms(double* terms, const float* y, const float* xk, const float* sj, int64_t n, const int64_t* offsets,
                          int64_t gsize, int64_t ngroups, const float* lambda, int binf, float delta);
void orc32_prox_group_l2(float* y, const float* q, const float* xk, const float* sj, int64_t n, const int64_t* offsets,
                         int64_t gsize, int64_t ngroups, const float* lambda, float sigma, const float* snorm_override);

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static float* fvec(int64_t n, float a, float step) {
  float* v = (float*)malloc((size_t)n * sizeof(float)); /* n = 0: a zero-length block (or NULL): never dereferenced */
  for (int64_t i = 0; i < n; ++i) v[i] = a + step * (float)(i % 7) * ((i & 1) ? -1.0f : 1.0f);
  return v;
}

static void separable(int64_t n) {
  float *y = fvec(n, 0.125f, 0.0625f), *x = fvec(n, -0.5f, 0.25f), *s = fvec(n, 0.25f, 0.03125f);
  float *l = fvec(n, -4.0f, 0.0f), *u = fvec(n, 4.0f, 0.0f);
  uint8_t* m = (uint8_t*)malloc((size_t)n);
  double* t = (double*)malloc((size_t)n * sizeof(double));
  for (int64_t i = 0; i < n; ++i) m[i] = (uint8_t)(i % 3 != 0);
  for (int kind = 0; kind < 3; ++kind) {
    CHECK(orc32_obj_terms(t, kind, 0, y, x, s, n, NULL, NULL, 0, 0, NULL, 0) == 0);
    for (int64_t i = 0; i < n; ++i) CHECK(t[i] >= 0.0 && isfinite(t[i]));
    CHECK(orc32_obj_terms(t, kind, 1, y, x, s, n, l, u, 0, 0, m, 0) == 0);
    for (int64_t i = 0; i < n; ++i) CHECK(m[i] || t[i] == 0.0);
    CHECK(orc32_obj_terms(t, kind, 1, y, x, s, n, NULL, u, -4.0f, 0, NULL, 0) == 0);
    CHECK(orc32_obj_terms(t, kind, 1, y, x, s, n, l, NULL, 0, -4.0f, NULL, 0) == (n > 0)); /* u = -4: infeasible unless empty */
    CHECK(orc32_obj_terms(t, kind, 2, y, x, s, n, NULL, NULL, 0, 0, NULL, 4.0f) == 0);
    CHECK(orc32_obj_terms(t, kind, 2, y, x, s, n, NULL, NULL, 0, 0, NULL, 0.0f) == (n > 0));
  }
  free(y); free(x); free(s); free(l); free(u); free(m); free(t);
}

static void groups(int64_t n, const int64_t* offsets, int64_t gsize, int64_t ngroups, int64_t head, int64_t tail0) {
  float *q = fvec(n, 1.0f, 0.5f), *x = fvec(n, -0.5f, 0.25f), *s = fvec(n, 0.25f, 0.03125f), *y = fvec(n, 3.0f, 0.0f);
  float* lam = fvec(ngroups, 0.5f, 0.03125f);
  float* sn = fvec(ngroups, NAN, 0.0f);
  double* t = (double*)malloc((size_t)ngroups * sizeof(double));
  int64_t* off = NULL;
  if (offsets) { /* exactly ngroups + 1 offsets on the heap */
    off = (int64_t*)malloc((size_t)(ngroups + 1) * sizeof(int64_t));
    for (int64_t g = 0; g <= ngroups; ++g) off[g] = offsets[g];
  }
  CHECK(orc32_obj_group_terms(t, q, x, s, n, off, gsize, ngroups, lam, 0, 0) == 0);
  CHECK(orc32_obj_group_terms(t, q, x, s, n, off, gsize, ngroups, lam, 1, 100.0f) == 0);
  CHECK(orc32_obj_group_terms(t, q, x, s, n, off, gsize, ngroups, lam, 1, 0.0f) == (n > 0 ? 1 : 0));
  for (int64_t g = 0; g < ngroups; ++g) CHECK(t[g] >= 0.0);
  orc32_prox_group_l2(y, q, x, s, n, off, gsize, ngroups, lam, 0.75f, NULL);
  for (int64_t i = 0; i < head; ++i) CHECK(y[i] == 3.0f - (x[i] + s[i]));          /* in no group: y on entry - (xk + sj) */
  for (int64_t i = tail0; i < n; ++i) CHECK(y[i] == 3.0f - (x[i] + s[i]));
  if (ngroups > 0) sn[0] = 0.0f; /* an overridden norm of zero: the group's y is 0 - (xk + sj) */
  orc32_prox_group_l2(q, q, x, s, n, off, gsize, ngroups, lam, 0.75f, sn);          /* y === q */
  if (ngroups > 0) {
    int64_t lo = off ? off[0] : 0, hi = off ? off[1] : gsize;
    for (int64_t i = lo; i < hi; ++i) CHECK(q[i] == 0.0f - (x[i] + s[i]));
  }
  free(q); free(x); free(s); free(y); free(lam); free(sn); free(t); free(off);
}

int main(void) {
  const int64_t sizes[] = {0, 1, 7, 1001};
  for (int k = 0; k < 4; ++k) separable(sizes[k]);
  groups(0, NULL, 1, 0, 0, 0);
  groups(1, NULL, 1, 1, 0, 1);
  groups(21, NULL, 3, 7, 0, 21);
  groups(1001, NULL, 7, 143, 0, 1001);
  { const int64_t off[] = {0, 0, 5, 5, 5, 12, 13, 13}; groups(13, off, 0, 7, 0, 13); }      /* empty groups, first and last too */
  { const int64_t off[] = {3, 3, 9, 20, 20, 31}; groups(37, off, 0, 5, 3, 31); }           /* head [0, 3) and tail [31, 37) uncovered */
  { const int64_t off[] = {4}; groups(9, off, 0, 0, 4, 4); }                               /* ngroups = 0: every index uncovered */
  { const int64_t off[] = {0, 1}; groups(1, off, 0, 1, 0, 1); }
  { /* offsets that break the contract are reported, and nothing outside the vectors is read */
    const int64_t off[] = {0, 9, 4, 13};
    float *v = fvec(13, 1.0f, 0.5f), *lam = fvec(3, 1.0f, 0.0f);
    double t[3];
    int64_t* o = (int64_t*)malloc(sizeof off);
    for (int g = 0; g < 4; ++g) o[g] = off[g];
    CHECK(orc32_obj_group_terms(t, v, v, v, 13, o, 0, 3, lam, 0, 0) == 2);
    o[2] = 9; o[3] = 14;
    CHECK(orc32_obj_group_terms(t, v, v, v, 13, o, 0, 3, lam, 0, 0) == 2);
    free(v); free(lam); free(o);
  }
  if (failures) return 1;
  puts("ok");
  return 0;
}
