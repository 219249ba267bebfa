// Multi-band displacement spectra of a day's events on the device (BPMF/spectrum.py: Spectrum.compute_multi_band_spectrum
// :387-505; the definition is postprocess.multiband_spectrum_host).  The day is float32, every operation float64.
//
// A row is one window (e, s, c): r = (e S + s) C + c, cut by the rule of day_rows.h.  Rows go through the
// kernels in slabs of a multiple of 64 that fit the caller's workspace; a slab holds, per row, four scalars, the
// prepared row and one forward pass per active band, all TIME-MAJOR (element t of row r at [t * slab + r]) so that the
// 64 lanes of a wave -- 64 consecutive rows -- touch one 512-byte line per sample:
//   1. mb_stats_kernel    one wave per row, the day read coalesced: the mean, then (on the row less its mean) the slope
//                         about the middle index and the mean that is left, in compensated sums; a window that is not
//                         wholly inside the day is marked (valid = 0).  Also writes +0 to the row's skipped bands.
//   2. mb_prepare_kernel  a 64 rows x 64 samples tile per workgroup through LDS: v = (x - mean) - (slope (t - c) + rest),
//                         times the half-Hann taper of `taper` samples at either end; zeros for a marked row.
//   3. mb_filter_kernel   one thread per (row, active band), a wave 64 consecutive rows of one band: the band's
//                         sections are wave-uniform, the 2 n_sections state values sit in registers.  Forward from zero
//                         state over P, stored to F; then from zero state down F, keeping max |y| over
//                         buffer <= t < n - buffer (a NaN stays), never storing y; out = max / bandwidth.
// The cascade is sos_cascade.h's, built with -ffp-contract=off: from an equal prepared row it equals SciPy's sosfilt bit
// for bit.  A row's arithmetic depends on its own samples only: the same bits in any slab and any batch.  Plain vector
// stores, no atomics on global memory; every element of every output is written.
#include "common.h"
#include "day_rows.h"
#include "sos_cascade.h"
#include <cmath>
#include "../../include/bpmf_hip.h"

namespace bpmf {

constexpr int MB_MAX_SAMPLES = 16384;
constexpr int MB_MAX_BANDS = 64;
constexpr int MB_ROW_SCALARS = 4;                      // mean, slope, rest, valid
constexpr size_t MB_MAX_SLAB = 65535 * 64;            // rows: gridDim.y of the prepare kernel is slab / 64

struct MbBands {
    int index[MB_MAX_BANDS];        // the active bands in ascending order
    double bandwidth[MB_MAX_BANDS];
};

struct MbCall {
    const float* data;              // (S, C, N)
    const long long* start;         // (n_windows)
    double* scalars;                // (slab, 4)
    double* P;                      // (n, slab)
    double* F;                      // (n_active, n, slab)
    size_t slab;                    // rows the slab has room for, a multiple of 64
    long long row0, rows, N;        // the slab's first row; rows in all
    int S, C, n, taper, buffer, B;
};

// Neumaier's sum of the 64 lanes' values in lane order; every lane gets the same result
__device__ inline double mb_wave_sum(double v, double* lds, int lane)
{
    __syncthreads();
    lds[lane] = v;
    __syncthreads();
    SvSum s;
#pragma unroll 8
    for (int i = 0; i < 64; ++i) s.add(lds[i]);
    return s.value();
}

__global__ __launch_bounds__(64) void mb_stats_kernel(const MbCall call, unsigned long long skip_mask,
                                                      double* __restrict__ out, uint8_t* __restrict__ valid)
{
    __shared__ double lds[64];
    const int lane = threadIdx.x, n = call.n;
    const long long in_slab = blockIdx.x, r = call.row0 + in_slab;
    const DayRow dr = day_row(call.S, call.C, call.N, call.start, (unsigned)r);
    const bool inside = day_window_inside(dr.start, n, call.N);
    if (lane < call.B && ((skip_mask >> lane) & 1ull)) out[(size_t)r * call.B + lane] = 0.0;
    if (lane == 0 && dr.c == 0) valid[dr.win] = inside ? 1 : 0;
    double* sc = call.scalars + (size_t)in_slab * MB_ROW_SCALARS;
    if (!inside) {
        if (lane < MB_ROW_SCALARS) sc[lane] = 0.0;
        return;
    }
    const float* __restrict__ x = call.data + dr.trace + dr.start;
    SvSum s0;
    for (int t = lane; t < n; t += 64) s0.add((double)x[t]);
    const double mean = mb_wave_sum(s0.value(), lds, lane) / (double)n;
    const double centre = (double)(n - 1) / 2.0;
    SvSum num, den, left;
    for (int t = lane; t < n; t += 64) {
        const double d = (double)t - centre, v = (double)x[t] - mean;
        num.add(v * d);
        den.add(d * d);
        left.add(v);
    }
    const double sum_num = mb_wave_sum(num.value(), lds, lane), sum_den = mb_wave_sum(den.value(), lds, lane);
    const double rest = mb_wave_sum(left.value(), lds, lane) / (double)n;
    const double slope = sum_den > 0.0 ? sum_num / sum_den : 0.0;
    if (lane == 0) sc[0] = mean, sc[1] = slope, sc[2] = rest, sc[3] = 1.0;
}

__global__ __launch_bounds__(256) void mb_prepare_kernel(const MbCall call)
{
    __shared__ double tile[64][65];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = call.n;
    const int t0 = blockIdx.x * 64;
    const long long in_slab0 = (long long)blockIdx.y * 64;
    const double centre = (double)(n - 1) / 2.0, pi = 3.141592653589793;
    for (int i = 0; i < 16; ++i) {
        const int local = wave * 16 + i, t = t0 + lane;
        const long long r = call.row0 + in_slab0 + local;
        double v = 0.0;
        if (r < call.rows && t < n) {
            const double* sc = call.scalars + (size_t)(in_slab0 + local) * MB_ROW_SCALARS;
            if (sc[3] != 0.0) {
                const DayRow dr = day_row(call.S, call.C, call.N, call.start, (unsigned)r);    // (valid: inside the day)
                const float* __restrict__ x = call.data + dr.trace + dr.start;
                v = ((double)x[t] - sc[0]) - (sc[1] * ((double)t - centre) + sc[2]);
                const int edge = t < n - 1 - t ? t : n - 1 - t;
                if (edge < call.taper) v = v * (0.5 * (1.0 - cos(pi * (double)edge / (double)call.taper)));
            }
        }
        tile[lane][local] = v;
    }
    __syncthreads();
    for (int i = 0; i < 16; ++i) {
        const int t = t0 + wave * 16 + i;
        if (t < n) call.P[(size_t)t * call.slab + (size_t)in_slab0 + lane] = tile[wave * 16 + i][lane];
    }
}

__global__ __launch_bounds__(64) void mb_filter_kernel(const MbCall call, const double* __restrict__ d_sos,
                                                       int n_sections, const MbBands bands, double* __restrict__ out)
{
    const size_t in_slab = (size_t)blockIdx.x * 64 + threadIdx.x;
    const long long r = call.row0 + (long long)in_slab;
    if (r >= call.rows) return;
    const int a = blockIdx.y, b = bands.index[a], n = call.n;
    SvFilter f{};
    f.sos = d_sos + (size_t)b * n_sections * 6;
    f.n_sections = n_sections;
    SvCascade cas;
    cas.load(f);
    const size_t slab = call.slab;
    const double* __restrict__ P = call.P + in_slab;
    double* __restrict__ F = call.F + (size_t)a * n * slab + in_slab;
    cas.reset();
    int t = 0;
    for (; t + 4 <= n; t += 4) {                                       // four loads in flight ahead of the recursion
        const double x0 = P[(size_t)t * slab], x1 = P[(size_t)(t + 1) * slab], x2 = P[(size_t)(t + 2) * slab],
                     x3 = P[(size_t)(t + 3) * slab];
        F[(size_t)t * slab] = cas.step(x0);
        F[(size_t)(t + 1) * slab] = cas.step(x1);
        F[(size_t)(t + 2) * slab] = cas.step(x2);
        F[(size_t)(t + 3) * slab] = cas.step(x3);
    }
    for (; t < n; ++t) F[(size_t)t * slab] = cas.step(P[(size_t)t * slab]);
    cas.reset();
    const int lo = call.buffer, hi = n - call.buffer;
    double best = 0.0;
    t = n - 1;
    for (; t >= 3; t -= 4) {
        const double x0 = F[(size_t)t * slab], x1 = F[(size_t)(t - 1) * slab], x2 = F[(size_t)(t - 2) * slab],
                     x3 = F[(size_t)(t - 3) * slab];
        const double y[4] = {cas.step(x0), cas.step(x1), cas.step(x2), cas.step(x3)};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double m = fabs(y[k]);
            const bool in = t - k >= lo && t - k < hi;
            best = in && (m > best || m != m) ? m : best;              // (a NaN is taken and then stays)
        }
    }
    for (; t >= 0; --t) {
        const double m = fabs(cas.step(F[(size_t)t * slab]));
        best = t >= lo && t < hi && (m > best || m != m) ? m : best;
    }
    out[(size_t)r * call.B + b] = best / bands.bandwidth[a];
}

static size_t mb_row_bytes(size_t n_samples, size_t n_active)
{
    return (MB_ROW_SCALARS + (1 + n_active) * n_samples) * sizeof(double);
}

}  // namespace bpmf

using namespace bpmf;

extern "C" size_t bpmf_multiband_workspace_bytes(size_t n_rows, size_t n_samples, size_t n_active_bands)
{
    if (n_samples == 0 || n_samples > (size_t)MB_MAX_SAMPLES || n_active_bands > (size_t)MB_MAX_BANDS ||
        n_rows >= (1ull << 31))
        return 0;
    return align_up(n_rows ? n_rows : 1, 64) * mb_row_bytes(n_samples, n_active_bands);
}

extern "C" int bpmf_multiband_spectrum_dev(const float* d_data, size_t S, size_t C, size_t N, size_t n_windows,
                                           const int64_t* d_start, size_t n_samples, size_t taper, size_t buffer,
                                           const double* d_sos, size_t n_bands, size_t n_sections,
                                           const double* bandwidths, const uint8_t* skip, void* d_workspace,
                                           size_t workspace_bytes, bpmf_stream_t stream_, double* d_out,
                                           uint8_t* d_valid)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n_windows == 0) return 0;
    const bool null_pointer = !d_data || !d_start || !d_sos || !bandwidths || !skip || !d_workspace || !d_out || !d_valid;
    if (day_rows_refused("bpmf_multiband_spectrum_dev", true, null_pointer, S, C, N, n_windows, set_error)) return -1;
    if (n_samples == 0 || n_samples > (size_t)MB_MAX_SAMPLES || buffer == 0 || n_samples <= 2 * buffer ||
        taper > n_samples / 4) {
        set_error("bpmf_multiband_spectrum_dev: need 1 .. %d samples, 1 <= buffer, 2 buffer < n_samples and a taper of "
                  "at most n_samples / 4 (n_samples=%zu taper=%zu buffer=%zu)", MB_MAX_SAMPLES, n_samples, taper,
                  buffer);
        return -1;
    }
    if (n_bands == 0 || n_bands > (size_t)MB_MAX_BANDS || n_sections == 0 || n_sections > (size_t)SV_MAX_SECTIONS) {
        set_error("bpmf_multiband_spectrum_dev: need 1 .. %d bands of 1 .. %d sections (bands=%zu sections=%zu)",
                  MB_MAX_BANDS, SV_MAX_SECTIONS, n_bands, n_sections);
        return -1;
    }
    const size_t rows = n_windows * C;
    if (rows > 0x7fffffffull / n_bands) {
        set_error("bpmf_multiband_spectrum_dev: %zu rows x %zu bands; fewer than 2^31 values fit", rows, n_bands);
        return -1;
    }
    MbBands bands{};
    unsigned long long skip_mask = 0;
    size_t n_active = 0;
    for (size_t b = 0; b < n_bands; ++b) {
        if (skip[b]) {
            skip_mask |= 1ull << b;
            continue;
        }
        if (!(bandwidths[b] > 0.0) || bandwidths[b] - bandwidths[b] != 0.0) {
            set_error("bpmf_multiband_spectrum_dev: band %zu has the bandwidth %g; a positive number is needed", b,
                      bandwidths[b]);
            return -1;
        }
        bands.index[n_active] = (int)b;
        bands.bandwidth[n_active] = bandwidths[b];
        ++n_active;
    }
    const size_t row_bytes = mb_row_bytes(n_samples, n_active);
    if (workspace_bytes < 64 * row_bytes) {
        set_error("bpmf_multiband_spectrum_dev: the workspace holds %zu bytes; 64 rows of %zu samples and %zu active "
                  "bands take %zu (bpmf_multiband_workspace_bytes)", workspace_bytes, n_samples, n_active,
                  64 * row_bytes);
        return -1;
    }
    // option debug.poison_output (tests): an element the kernels skip comes back as NaN / 255
    if (option(OPT_DEBUG_POISON_OUTPUT) != 0) {
        BPMF_HIP_CHECK(hipMemsetAsync(d_out, 0xFF, rows * n_bands * sizeof(double), stream));
        BPMF_HIP_CHECK(hipMemsetAsync(d_valid, 0xFF, n_windows, stream));
    }
    size_t slab = workspace_bytes / row_bytes / 64 * 64;
    slab = slab > align_up(rows, 64) ? align_up(rows, 64) : slab;
    slab = slab > MB_MAX_SLAB ? MB_MAX_SLAB : slab;

    MbCall call{};
    call.data = d_data;
    call.start = (const long long*)d_start;
    call.scalars = (double*)d_workspace;
    call.P = call.scalars + slab * MB_ROW_SCALARS;
    call.F = call.P + slab * n_samples;
    call.slab = slab;
    call.rows = (long long)rows, call.N = (long long)N;
    call.S = (int)S, call.C = (int)C, call.n = (int)n_samples, call.taper = (int)taper, call.buffer = (int)buffer;
    call.B = (int)n_bands;
    const unsigned time_tiles = (unsigned)((n_samples + 63) / 64);
    for (size_t row0 = 0; row0 < rows; row0 += slab) {
        const size_t here = rows - row0 < slab ? rows - row0 : slab;
        const unsigned groups = (unsigned)((here + 63) / 64);
        call.row0 = (long long)row0;
        mb_stats_kernel<<<dim3((unsigned)here), dim3(64), 0, stream>>>(call, skip_mask, d_out, d_valid);
        if (n_active) {
            mb_prepare_kernel<<<dim3(time_tiles, groups), dim3(256), 0, stream>>>(call);
            mb_filter_kernel<<<dim3(groups, (unsigned)n_active), dim3(64), 0, stream>>>(call, d_sos, (int)n_sections,
                                                                                       bands, d_out);
        }
        BPMF_LAUNCH_CHECK();
    }
    return 0;
}
