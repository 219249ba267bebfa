/* A plain-C consumer of the matched filter's full normalisation (flag BPMF_MF_NORMALIZE_FULL of include/bpmf_hip.h):
 * no Python, no torch, no C++.  Built and run by tests/test_gpu_mf_full.py like tests/c_abi/abi_smoke.c:
 *
 *   gcc -std=c99 -O1 -I include tests/c_abi/abi_mf_full.c -o abi_mf_full -L seismic_bpmf_amd/lib -lbpmf_hip -lm
 *
 * Channels with offsets of hundreds of standard deviations and one constant-filled run go through bpmf_mf_run_multi
 * with the flag; every per-channel value is compared with the Pearson correlation of its window in double precision --
 * to 2e-5, the tolerance of the north star: this program checks linking and semantics, the sharp a priori bound is
 * tests/mf_full_definition.py's -- windows inside the run must be +0 bit for bit, the network sums must be the fmaf
 * chain of the per-channel values, and short mode on the same arrays must be far from the correlation. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bpmf_hip.h"

static unsigned long long g_state = 88172645463325252ull;
static float rnd(void)
{ /* xorshift: uniform in [-1, 1) */
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return (float)((double)(g_state >> 11) / 9007199254740992.0 * 2.0 - 1.0);
}

int main(void)
{
    enum { T = 3, S = 2, C = 2, L = 40, N = 3000, NC = N - L + 1, NCH = S * C, RUN0 = 1200, RUN_LEN = 100 };
    const int n = bpmf_device_count();
    if (n < 1) { fprintf(stderr, "no HIP device: %s\n", bpmf_last_error()); return 2; }
    if (BPMF_MF_NORMALIZE_FULL != 4 || BPMF_MF_LAUNCH_INFO_FIELDS != 13) { fprintf(stderr, "flag values\n"); return 1; }
    if (bpmf_mf_full_workspace_bytes(L, N, T, S, C) < bpmf_mf_workspace_bytes(L, N, T, S, C) + 16u * NCH * N) {
        fprintf(stderr, "bpmf_mf_full_workspace_bytes: smaller than short mode plus 16 bytes a sample\n");
        return 1;
    }
    float *tp = malloc(sizeof(float) * T * NCH * L), *d = malloc(sizeof(float) * NCH * N);
    float *w = malloc(sizeof(float) * T * NCH), *cc = malloc(sizeof(float) * T * NC * NCH);
    float *sums = malloc(sizeof(float) * T * NC), *shrt = malloc(sizeof(float) * T * NC * NCH);
    int32_t *mv = malloc(sizeof(int32_t) * T * NCH);
    for (int i = 0; i < T * NCH * L; ++i) tp[i] = rnd() + 0.5f;
    for (int ch = 0; ch < NCH; ++ch)
        for (int i = 0; i < N; ++i) d[ch * N + i] = rnd() + 150.0f * (float)(ch + 1) * (ch % 2 ? -1.0f : 1.0f);
    for (int i = 0; i < RUN_LEN; ++i) d[1 * N + RUN0 + i] = -7.5f;          /* a constant-filled gap on channel 1 */
    for (int i = 0; i < T * NCH; ++i) { w[i] = 0.1f + fabsf(rnd()); mv[i] = (int32_t)(fabsf(rnd()) * 90.0f); }
    w[1 * NCH + 2] = 0.0f;                                                  /* a zero-weight channel */
    const int dev[1] = {0};
    int rc = bpmf_mf_run_multi(tp, mv, w, d, 1, L, N, T, S, C, NC, 0, BPMF_MF_NORMALIZE_FULL, 1, dev, cc);
    if (rc) { fprintf(stderr, "bpmf_mf_run_multi (full, per channel): %d %s\n", rc, bpmf_last_error()); return 1; }
    rc = bpmf_mf_run_multi(tp, mv, w, d, 1, L, N, T, S, C, NC, 1, BPMF_MF_NORMALIZE_FULL, 1, dev, sums);
    if (rc) { fprintf(stderr, "bpmf_mf_run_multi (full, network sum): %d %s\n", rc, bpmf_last_error()); return 1; }
    rc = bpmf_mf_run_multi(tp, mv, w, d, 1, L, N, T, S, C, NC, 0, 0, 1, dev, shrt);
    if (rc) { fprintf(stderr, "bpmf_mf_run_multi (short): %d %s\n", rc, bpmf_last_error()); return 1; }
    int n_flat = 0, n_far = 0, n_values = 0;
    double worst = 0.0;
    for (int t = 0; t < T; ++t) {
        int mv_max = 0;
        for (int ch = 0; ch < NCH; ++ch)
            if (w[t * NCH + ch] != 0.0f && mv[t * NCH + ch] > mv_max) mv_max = mv[t * NCH + ch];
        const int last = N - L - mv_max;                                    /* last valid lag, inclusive */
        for (int i = 0; i < NC; ++i) {
            float sum = 0.0f;
            for (int ch = 0; ch < NCH; ++ch) {
                const float got = cc[(t * NC + i) * NCH + ch];
                if (i > last || w[t * NCH + ch] == 0.0f) {
                    if (memcmp(&got, &(float){0.0f}, sizeof(float))) { fprintf(stderr, "a value outside the range is not +0\n"); return 1; }
                    continue;
                }
                const float *x = tp + (t * NCH + ch) * L, *y = d + ch * N + i + mv[t * NCH + ch];
                double mx = 0.0, my = 0.0, sxy = 0.0, sxx = 0.0, syy = 0.0;
                int flat = 1;
                for (int l = 0; l < L; ++l) { mx += x[l]; my += y[l]; flat = flat && y[l] == y[0]; }
                mx /= L; my /= L;
                for (int l = 0; l < L; ++l) {
                    sxy += (x[l] - mx) * (y[l] - my); sxx += (x[l] - mx) * (x[l] - mx); syy += (y[l] - my) * (y[l] - my);
                }
                if (flat) {
                    ++n_flat;
                    if (memcmp(&got, &(float){0.0f}, sizeof(float))) { fprintf(stderr, "a flat window is not +0\n"); return 1; }
                } else {
                    const double want = sxy / sqrt(sxx * syy), err = fabs((double)got - want);
                    if (err > worst) worst = err;
                    if (fabs((double)shrt[(t * NC + i) * NCH + ch] - want) > 1e-2) ++n_far;
                    ++n_values;
                }
                sum = fmaf(w[t * NCH + ch], got, sum);
            }
            if (memcmp(&sum, &sums[t * NC + i], sizeof(float))) { fprintf(stderr, "a network sum is not the chain of its channels\n"); return 1; }
        }
    }
    if (!(worst <= 2e-5)) { fprintf(stderr, "full mode is %g from the Pearson correlation\n", worst); return 1; }
    if (n_flat < 100 || n_far * 2 < n_values) { fprintf(stderr, "the inputs do not test: %d flat, %d of %d far\n", n_flat, n_far, n_values); return 1; }
    free(tp); free(d); free(w); free(cc); free(sums); free(shrt); free(mv);
    printf("ok: full normalisation from plain C, worst |cc - pearson| %.3g over %d values, %d flat windows\n", worst, n_values, n_flat);
    return 0;
}
