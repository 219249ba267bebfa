// Peak amplitudes of matched-filter detections (BPMF/similarity_search.py:695-714): for detection q = (template
// row t, data sample k) and channel (s, c), the maximum of the continuous data in
//     data[s, c, i1:i2],   i1 = k + moveouts[t, s, c] - offset,   i2 = i1 + duration,
// times data_norm[s, c] -- or 0.0 when the slice is empty.  The day of data is already in HBM when the detections are
// known, so this is a gather: D x S x C windows of a few hundred samples (2500 x 60 x 300 x 4 B = 180 MB at
// BASELINE configs[1]).
//
// The slice is a NumPy BASIC slice and the reference does not guard it, so its rule is the contract
// (slice_bound): each of i1, i2 on its own gets N added when negative and is then clipped to [0, N]; the window is
// [a, b), empty when b <= a.  Hence a window that straddles sample 0 is EMPTY (a lands near N, b near 0), a window
// wholly before sample 0 WRAPS to the end of the day, and a window past N is clipped at N (of day_rows.h: the limit).
//
// np.max propagates NaN and v_max_f32 drops it: every lane carries a "saw a NaN" flag beside its running maximum, the
// flags meet in one __ballot, and a window that holds a NaN yields a quiet NaN.  +-Inf are ordinary values.  One
// case NumPy itself leaves open: a window whose maximum is a zero and that holds zeros of BOTH signs (np.max returns
// whichever its SIMD reduction order meets last); this kernel returns +0.0 there.
//
// Shape: one workgroup of 256 threads per detection; its 4 waves take the S*C channels round robin.  t, k and the
// channel are wave-uniform, so the moveout and the window bounds live in SGPRs and the address of a load is SGPR base
// + lane.  A window starts at any sample: the wave reads it lane-strided from a, 64 consecutive floats per load
// instruction, PA_UNROLL independent loads per lane before the first compare -- a 300-sample window is ONE round
// trip to memory.  Loads past the end of the window are not predicated but clamped to its last sample: a maximum
// (and the flag) may see a sample twice.  Across lanes: __shfl_xor maxima and one ballot; lane 0 stores the result
// with a plain vector store.  No LDS, no atomics, and every (q, s, c) is written, the 0.0 of an empty window included.
#include "common.h"
#include "day_rows.h"
#include <cmath>
#include <vector>
#include "../../include/bpmf_hip.h"

namespace bpmf {

constexpr int PA_UNROLL = 8;                       // loads in flight per lane: 512 samples per round of a wave
constexpr long long PA_SAMPLE_LIMIT = 1ll << 61;   // |k| the kernel clamps to

// One bound of the Python slice x[i1:i2] of a series of n samples.
__device__ __forceinline__ long long slice_bound(long long v, long long n)
{
    if (v < 0) v += n;
    return v < 0 ? 0 : (v > n ? n : v);
}

__global__ __launch_bounds__(256) void peak_amplitudes_kernel(const float* __restrict__ data, int n_channels, long long n,
                                                              const int32_t* __restrict__ rows,
                                                              const long long* __restrict__ samples,
                                                              const int32_t* __restrict__ moveouts, int n_templates,
                                                              long long offset, long long duration,
                                                              const float* __restrict__ norm, float* __restrict__ out)
{
    const size_t q = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t = rows[q];
    const bool bad_row = t < 0 || t >= n_templates;            // (the entry point has refused these: never read past the table)
    // a sample beyond +-2^61 puts both ends of every window on the same side of the day as the clamped one does
    // (|moveout| < 2^31, N, |offset|, |duration| <= 2^40): the sums below cannot overflow
    long long k = samples[q];
    k = k < -PA_SAMPLE_LIMIT ? -PA_SAMPLE_LIMIT : (k > PA_SAMPLE_LIMIT ? PA_SAMPLE_LIMIT : k);
    for (int ch = wave; ch < n_channels; ch += 4) {
        float result = 0.0f;                                     // the reference's np.zeros entry of an empty window
        if (bad_row) {
            result = __builtin_nanf("");
        } else {
            const long long i1 = k + (long long)moveouts[(size_t)t * n_channels + ch] - offset;
            const long long a = slice_bound(i1, n), b = slice_bound(i1 + duration, n);
            if (b > a) {
                const float* __restrict__ x = data + (size_t)ch * (size_t)n;
                const long long last = b - 1;
                float m = -INFINITY;
                bool saw_nan = false;
                for (long long base = a; base < b; base += 64 * PA_UNROLL) {
                    float v[PA_UNROLL];
#pragma unroll
                    for (int u = 0; u < PA_UNROLL; ++u) {
                        const long long i = base + 64 * u + lane;
                        v[u] = x[i < last ? i : last];
                    }
#pragma unroll
                    for (int u = 0; u < PA_UNROLL; ++u) {
                        saw_nan |= v[u] != v[u];
                        m = fmaxf(m, v[u]);
                    }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
                if (__ballot(saw_nan) != 0ull) result = __builtin_nanf("");
                else result = norm ? __fmul_rn(m, norm[ch]) : m;
            }
        }
        if (lane == 0) out[q * (size_t)n_channels + ch] = result;
    }
}

}  // namespace bpmf

using namespace bpmf;

extern "C" int bpmf_peak_amplitudes_dev(const float* d_data, size_t S, size_t C, size_t N, size_t n_detections,
                                        const int32_t* d_rows, const int64_t* d_samples, const int32_t* d_moveouts,
                                        size_t T, int64_t offset, int64_t duration, const float* d_norm_or_null,
                                        bpmf_stream_t stream_, float* d_out)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n_detections == 0) return 0;
    if (!d_data || !d_rows || !d_samples || !d_moveouts || !d_out) {
        set_error("bpmf_peak_amplitudes_dev: null pointer");
        return -1;
    }
    if (S == 0 || C == 0 || S > 0x7fffffffull / C || T == 0 || T > 0x7fffffffull || n_detections > 0x7fffffffull ||
        N > (size_t)DAY_INDEX_LIMIT || offset > DAY_INDEX_LIMIT || offset < -DAY_INDEX_LIMIT ||
        duration > DAY_INDEX_LIMIT || duration < -DAY_INDEX_LIMIT) {
        set_error("bpmf_peak_amplitudes_dev: bad argument (S=%zu C=%zu N=%zu T=%zu detections=%zu offset=%lld "
                  "duration=%lld)", S, C, N, T, n_detections, (long long)offset, (long long)duration);
        return -1;
    }
    // the template rows index the moveout table: checked here, on a copy of the few KB, before anything is launched
    std::vector<int32_t> rows(n_detections);
    BPMF_HIP_CHECK(hipMemcpyAsync(rows.data(), d_rows, n_detections * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    BPMF_HIP_CHECK(hipStreamSynchronize(stream));
    for (size_t q = 0; q < n_detections; ++q)
        if (rows[q] < 0 || (size_t)rows[q] >= T) {
            set_error("bpmf_peak_amplitudes_dev: detection %zu names template row %d, outside [0, %zu)", q, rows[q], T);
            return -1;
        }
    // option debug.poison_output (tests): an element the kernel skips comes back as NaN
    if (option(OPT_DEBUG_POISON_OUTPUT) != 0)
        BPMF_HIP_CHECK(hipMemsetAsync(d_out, 0xFF, n_detections * S * C * sizeof(float), stream));
    peak_amplitudes_kernel<<<dim3((unsigned)n_detections), dim3(256), 0, stream>>>(
        d_data, (int)(S * C), (long long)N, d_rows, (const long long*)d_samples, d_moveouts, (int)T, (long long)offset,
        (long long)duration, d_norm_or_null, d_out);
    BPMF_LAUNCH_CHECK();
    return 0;
}
