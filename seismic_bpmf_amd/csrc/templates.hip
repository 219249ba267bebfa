// Matched-filter templates cut from a day's located events (BPMF/dataset.py: Event.read_waveforms(time_shifted=True)
// :1929-2069, Event.set_availability :2556-2607, Template.moveouts_arr :3451-3475, TemplateGroup.normalize :4152-4166,
// Event.compute_snr :1441-1475): for event e and channel (s, c), with i0 = origin[e] + moveouts[e, s, c],
//     window[l]          = data[s, c, i0 + l] where 0 <= i0 + l < N, else +0.0   (l = 0 .. L-1; day_rows.h)
//     available          = any(window != 0)            (a NaN counts as data)
//     complete           = 0 <= i0 and i0 + L <= N
//     norm               = np.std(window) | np.max(np.abs(window)) | 1;   0 -> 1
//     templates[e,s,c,:] = window / norm
//     snr                = np.std(window) / np.std(noise window),  noise std 0 -> 1; the noise window is the
//                          noise_samples samples from origin[e] - noise_offset, clipped the same way
// The day is already in HBM when the events are located, so this is a gather of E x S x C windows like peak_amp.hip,
// with one difference: the results are compared with NumPy bit for bit, so the arithmetic is NumPy's, operation for
// operation (postprocess.templates_from_events_host is the definition):
//     mean = pairwise_sum(x) / L;   d = x - mean;   d = d * d;   var = pairwise_sum(d) / L;   std = sqrt(var)
// in float32, every operation rounded on its own.  pairwise_sum is NumPy's order of additions (np_order.h is its
// definition, np_sums.h the workgroup's layout of it); it is one tree up to NP_CHUNK elements, so L and noise_samples
// stop there.
//
// One workgroup of 256 threads per (event, channel); i0 is uniform.  The window is read once, lane-strided, 64
// consecutive floats per load instruction, all loads of a thread issued before the first use (addresses clamped into
// the day, values outside it replaced by 0 afterwards), kept in registers for the final division and staged in LDS
// for the sums.  np.max propagates NaN and v_max_f32 drops it:
// a "saw a NaN" flag travels beside the maximum, as in peak_amp.hip.  No atomics, plain vector stores, and every
// output element is written, the zeros of a clipped window included.
#include "common.h"
#include "day_rows.h"
#include "np_sums.h"
#include <cmath>
#include <vector>
#include "../../include/bpmf_hip.h"

namespace bpmf {

template <int NU>   // window samples per thread: L <= 256 * NU
__global__ __launch_bounds__(TP_THREADS) void templates_kernel(
    const float* __restrict__ data, int n_channels, long long n, const long long* __restrict__ origin,
    const int32_t* __restrict__ moveouts, int L, int mode, long long noise_offset, int n_noise, const LeafTable sig,
    const LeafTable noi, float* __restrict__ templates, float* __restrict__ norm_out,
    unsigned char* __restrict__ flags, float* __restrict__ snr)
{
    extern __shared__ __align__(16) float win[];                   // max(L, n_noise) floats
    __shared__ SumScratch scratch;
    __shared__ float wave_max[TP_THREADS / 64];
    __shared__ int wave_bits[TP_THREADS / 64];
    const size_t item = blockIdx.x;                                // (e, s, c) flattened
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t e = item / (size_t)n_channels;
    const float* __restrict__ x = data + (item - e * (size_t)n_channels) * (size_t)n;
    const long long t0 = origin[e];                                // |t0| <= 2^40 (checked by the entry point)
    const long long i0 = t0 + (long long)moveouts[item];

    float xr[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) xr[u] = clipped_sample(x, i0 + tid + TP_THREADS * u, n);
    bool nonzero = false, saw_nan = false;
    float amax = 0.0f;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int l = tid + TP_THREADS * u;
        if (l < L) {
            win[l] = xr[u];
            nonzero |= xr[u] != 0.0f;                              // true for a NaN too: np.any(window != 0)
            saw_nan |= xr[u] != xr[u];
            amax = fmaxf(amax, fabsf(xr[u]));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    const int bits = (__ballot(nonzero) != 0ull ? 1 : 0) | (__ballot(saw_nan) != 0ull ? 2 : 0);
    if (lane == 0) {
        wave_max[wave] = amax;
        wave_bits[wave] = bits;
    }
    __syncthreads();
    const int all_bits = wave_bits[0] | wave_bits[1] | wave_bits[2] | wave_bits[3];
    amax = fmaxf(fmaxf(wave_max[0], wave_max[1]), fmaxf(wave_max[2], wave_max[3]));
    if (all_bits & 2) amax = __builtin_nanf("");

    const float sd = block_std(win, L, sig, scratch, tid);         // (ends behind a barrier: win is free again)
    float norm = mode == 1 ? sd : (mode == 2 ? amax : 1.0f);
    if (norm == 0.0f) norm = 1.0f;
    float* __restrict__ out = templates + item * (size_t)L;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int l = tid + TP_THREADS * u;
        if (l < L) out[l] = __fdiv_rn(xr[u], norm);
    }
    if (tid == 0) {
        norm_out[item] = norm;
        flags[item] = (unsigned char)((all_bits & 1) | ((i0 >= 0 && i0 + L <= n) ? 2 : 0));
    }
    if (snr) {
        const long long j0 = t0 - noise_offset;
        for (int l = tid; l < n_noise; l += TP_THREADS) win[l] = clipped_sample(x, j0 + l, n);
        __syncthreads();
        float noise_sd = block_std(win, n_noise, noi, scratch, tid);
        if (noise_sd == 0.0f) noise_sd = 1.0f;
        if (tid == 0) snr[item] = __fdiv_rn(sd, noise_sd);
    }
}

}  // namespace bpmf

using namespace bpmf;

extern "C" int bpmf_templates_from_events_dev(const float* d_data, size_t S, size_t C, size_t N, size_t n_events,
                                              const int64_t* d_origin, const int32_t* d_moveouts, size_t n_samples,
                                              int normalize, int64_t noise_offset, size_t noise_samples,
                                              bpmf_stream_t stream_, float* d_templates, float* d_norm,
                                              uint8_t* d_flags, float* d_snr_or_null)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n_events == 0) return 0;
    if (!d_data || !d_origin || !d_moveouts || !d_templates || !d_norm || !d_flags) {
        set_error("bpmf_templates_from_events_dev: null pointer");
        return -1;
    }
    if ((noise_samples != 0) != (d_snr_or_null != nullptr)) {
        set_error("bpmf_templates_from_events_dev: d_snr goes with noise_samples > 0 and only with it "
                  "(noise_samples=%zu)", noise_samples);
        return -1;
    }
    if (n_samples == 0 || n_samples > (size_t)NP_CHUNK || noise_samples > (size_t)NP_CHUNK) {
        set_error("bpmf_templates_from_events_dev: need 1 <= n_samples <= %d and noise_samples <= %d, the lengths NumPy "
                  "sums in one pairwise tree (n_samples=%zu noise_samples=%zu)", NP_CHUNK, NP_CHUNK,
                  n_samples, noise_samples);
        return -1;
    }
    if (S == 0 || C == 0 || S > 0x7fffffffull / C || n_events > 0x7fffffffull / (S * C) || N == 0 ||
        N > (size_t)DAY_INDEX_LIMIT || noise_offset > DAY_INDEX_LIMIT || noise_offset < -DAY_INDEX_LIMIT ||
        normalize < 0 || normalize > 2) {
        set_error("bpmf_templates_from_events_dev: bad argument (S=%zu C=%zu N=%zu events=%zu normalize=%d "
                  "noise_offset=%lld)", S, C, N, n_events, normalize, (long long)noise_offset);
        return -1;
    }
    // the origins bound every index of the kernel: checked here, on a copy of 8 E bytes, before anything is launched
    std::vector<int64_t> origin(n_events);
    BPMF_HIP_CHECK(hipMemcpyAsync(origin.data(), d_origin, n_events * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    BPMF_HIP_CHECK(hipStreamSynchronize(stream));
    for (size_t e = 0; e < n_events; ++e)
        if (origin[e] > DAY_INDEX_LIMIT || origin[e] < -DAY_INDEX_LIMIT) {
            set_error("bpmf_templates_from_events_dev: event %zu has origin sample %lld, outside +-2^40", e,
                      (long long)origin[e]);
            return -1;
        }
    LeafTable sig{}, noi{};
    if (!list_leaves((int)n_samples, sig) || (noise_samples && !list_leaves((int)noise_samples, noi))) {
        set_error("bpmf_templates_from_events_dev: the pairwise tree has more than %d leaves", NP_MAX_LEAVES);
        return -1;
    }
    const size_t n_items = n_events * S * C;
    // option debug.poison_output (tests): an element the kernel skips comes back as NaN (flags: 0xFF)
    if (option(OPT_DEBUG_POISON_OUTPUT) != 0) {
        BPMF_HIP_CHECK(hipMemsetAsync(d_templates, 0xFF, n_items * n_samples * sizeof(float), stream));
        BPMF_HIP_CHECK(hipMemsetAsync(d_norm, 0xFF, n_items * sizeof(float), stream));
        BPMF_HIP_CHECK(hipMemsetAsync(d_flags, 0xFF, n_items, stream));
        if (d_snr_or_null) BPMF_HIP_CHECK(hipMemsetAsync(d_snr_or_null, 0xFF, n_items * sizeof(float), stream));
    }
    const size_t lds = (n_samples > noise_samples ? n_samples : noise_samples) * sizeof(float);
    const dim3 grid((unsigned)n_items), block(TP_THREADS);
#define TP_LAUNCH(NU)                                                                                                  \
    templates_kernel<NU><<<grid, block, lds, stream>>>(d_data, (int)(S * C), (long long)N, (const long long*)d_origin, \
                                                       d_moveouts, (int)n_samples, normalize, (long long)noise_offset, \
                                                       (int)noise_samples, sig, noi, d_templates, d_norm, d_flags,    \
                                                       d_snr_or_null)
    if (n_samples <= 256) TP_LAUNCH(1);
    else if (n_samples <= 1024) TP_LAUNCH(4);
    else TP_LAUNCH(32);
#undef TP_LAUNCH
    BPMF_LAUNCH_CHECK();
    return 0;
}
