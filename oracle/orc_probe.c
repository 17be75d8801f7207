/* orc_probe.c — TEST INFRASTRUCTURE: array loops over the oracle's math primitives, so that a test can run millions of points through each
 * (tests/test_gpu_devmath.py holds the device's twins to them bit for bit, tests/test_devmath_definition.py holds them to float64 definitions).
 * No formula lives here: every loop calls the function the chains call. */
#include "orc.h"

void orc_probe_sincosf(const float* x, size_t n, float* c, float* s)
{
#pragma omp parallel for schedule(static)
    for (size_t i = 0; i < n; i++) orc_sincosf(x[i], &s[i], &c[i]);
}
void orc_probe_sincos_turn(const uint64_t* a, size_t n, float* c, float* s)
{
#pragma omp parallel for schedule(static)
    for (size_t i = 0; i < n; i++) orc_sincos_turn(a[i], &s[i], &c[i]);
}
void orc_probe_fast_atan2f(const float* y, const float* x, size_t n, float* out)
{
    (void)orc_atan_table();   /* the table is made before the threads start */
#pragma omp parallel for schedule(static)
    for (size_t i = 0; i < n; i++) out[i] = orc_fast_atan2f(y[i], x[i]);
}
void orc_probe_tanhf_lut(const float* x, size_t n, float* out)
{
    (void)orc_tanh_table();
#pragma omp parallel for schedule(static)
    for (size_t i = 0; i < n; i++) out[i] = orc_tanhf_lut(x[i]);
}
void orc_probe_clip(const float* x, const float* limit, size_t n, float* out)
{
#pragma omp parallel for schedule(static)
    for (size_t i = 0; i < n; i++) out[i] = orc_branchless_clip(x[i], limit[i]);
}
void orc_probe_ted_error(const float* u, size_t n, float* ff, float* cc)
{
#pragma omp parallel for schedule(static)
    for (size_t i = 0; i < n; i++) { ff[i] = orc_ted_error_ff(u[i]); cc[i] = orc_ted_error_cc(u[i]); }
}
void orc_probe_phase_wrap(const float* x, size_t n, float* out)
{
#pragma omp parallel for schedule(static)
    for (size_t i = 0; i < n; i++) out[i] = orc_phase_wrap(x[i]);
}
void orc_probe_det_log2f(const float* x, size_t n, float* out)
{
#pragma omp parallel for schedule(static)
    for (size_t i = 0; i < n; i++) out[i] = orc_det_log2f(x[i]);
}
void orc_probe_det_log10f(const float* x, size_t n, float* out)
{
#pragma omp parallel for schedule(static)
    for (size_t i = 0; i < n; i++) out[i] = orc_det_log10f(x[i]);
}
void orc_probe_f2s(const float* x, const float* scale, size_t n, int16_t* out)
{
#pragma omp parallel for schedule(static)
    for (size_t i = 0; i < n; i++) out[i] = orc_f2s(x[i], scale[i]);
}
