// Host-side interface of the matched filter's full normalisation (mf_full.hip; flag BPMF_MF_NORMALIZE_FULL) for
// the entry points of mf.hip: where its arrays live in the full-mode workspace and its two preparations.  The main
// kernels of mf.hip run unchanged on what these leave behind: the centred day d', the centred templates t' and the
// reciprocal norms of the centred window energies.
#pragma once
#include "common.h"

namespace bpmf {
namespace full {

// The per-day extras (behind the window norms, in front of everything that depends on the template count).
struct DayRegion {
    float* dprime;      // [n_ch, N]   d - c, c = float32(float64 mean of the channel)
    double* local_p;    // [n_ch, N]   chunk-local prefix sums of d'  (the workspace's own `local` holds those of d'^2)
    double* tot_p;      // [n_ch, nq]
    double* off_p;      // [n_ch, nq]
    int* local_eq;      // [n_ch, N]   chunk-local prefix counts of d[n] == d[n - 1]
    int* tot_eq;        // [n_ch, nq]
    int* off_eq;        // [n_ch, nq]
    double* part;       // [n_ch, n_parts] partial sums of the channel
    float* mean;        // [n_ch]      c
    size_t bytes;
};
DayRegion carve_day(void* base, size_t N, size_t n_ch);
// the per-batch extra (at the end): t' [T, n_ch, L]
size_t batch_region_bytes(size_t T, size_t n_ch, size_t L);

// once per day: c, d', the three prefix hierarchies, the norms r_c[ch, j] = 1 / sqrtf((float)(Q - P * P / L)) -- +Inf for a
// window of L equal samples -- into e_d [n_ch, nwin]; local_q / tot_q / off_q: the workspace's prefix arrays
int prepare_day(const float* d_data, size_t L, size_t N, size_t n_ch, const DayRegion& day, double* local_q,
                double* tot_q, double* off_q, float* e_d, hipStream_t stream);

// once per template batch: t' = t - float32(float64 mean) of every template channel (all zeros for a flat one)
int prepare_templates(const float* d_templates, size_t n_rows, size_t L, float* tprime, hipStream_t stream);

}  // namespace full
}  // namespace bpmf
