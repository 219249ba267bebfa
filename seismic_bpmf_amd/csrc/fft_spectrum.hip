// FFT-method displacement spectra of a day's events on the device (BPMF/spectrum.py: Spectrum.compute_spectrum :507-599
// and Spectrum.resample :851-887, method "regular" of compute_moment_magnitude; the definition is
// postprocess.fft_spectrum_host).  The day is float32, every operation float64.
//
// Only the bins next to a target frequency are ever read, so the transform is a DFT PRUNED to the caller's list of
// bins: per row a (n x K_b) float64 product with twiddles from an exact table of n entries (cos, -sin of 2 pi m / n).
// A row is one window (e, s, c): r = (e S + s) C + c, cut by the rule of day_rows.h.  Rows go through in
// slabs of a multiple of 64 that fit the caller's workspace:
//   1. fs_dft_kernel       a workgroup of 4 waves takes 64 rows x up to 64 bins (blockIdx.y: the group of 64 bins;
//                          32 or 16 where no more are asked for).
//                          Per chunk of 64 samples wave w stages its 16 rows as (double)x_j w_j in LDS (the day read
//                          coalesced and one chunk ahead, zeros behind sample n - 1, for a window that leaves the day
//                          and for a row past the last), then runs 16 k-steps of v_mfma_f64_16x16x4_f64: A = 16 rows x
//                          4 samples from LDS, read once per k-step for all bin tiles; B = 4 samples x 16 bins of the
//                          table at (j k) mod n, advanced by 4 k mod n and one conditional subtract, read one k-step
//                          ahead.  The table lies in LDS
//                          while n <= FS_TABLE_LDS_MAX (16 n bytes beside the 33 KB of rows); above, it is read
//                          through L2.  Re and Im of 16 x 16 per accumulator pair, stored to the workspace as
//                          (slab, K_b) pairs.  A row's sums run over j = 0, 4, 8, ... in that order whatever the
//                          batch, the slab and the workspace: the same bits everywhere.  Group 0 also writes a status
//                          per row (0 live, 1 holds a non-finite sample, 2 window not inside the day) and `valid`.
//   2. fs_epilogue_kernel  one thread per output element: times delta (one rounded multiply each on re and im), the
//                          modulus, with multi_component the root of the components' summed squares in component
//                          order, with targets np.interp's formula on the pair of bins; NaN for status 1, +0 for
//                          status 2 and for a target at or beyond 0.99 f_max.
// Operands are padded with zeros (samples behind n - 1, rows past the last, bins past K_b); nothing is read past a
// buffer.  Plain vector stores, no atomics; every element of both outputs is written.
#include "common.h"
#include "day_rows.h"
#include <cmath>
#include "../../include/bpmf_hip.h"

namespace bpmf {

constexpr int FS_MIN_SAMPLES = 2;
constexpr int FS_MAX_SAMPLES = 16384;
constexpr int FS_MAX_TARGETS = 1024;
constexpr int FS_ROWS = 64;                             // rows of a workgroup: 16 per wave
constexpr int FS_CHUNK = 64;                            // samples staged at a time
constexpr int FS_ROW_STRIDE = FS_CHUNK + 2;             // doubles; 16 rows x 2 samples of a half wave fall on 64 banks
constexpr int FS_TILES = 4;                             // bin tiles of 16 a wave walks per staged chunk, at most
constexpr size_t FS_ROWS_LDS = (size_t)FS_ROWS * FS_ROW_STRIDE * sizeof(double);           // 33792
constexpr size_t FS_LDS_LIMIT = 160 * 1024;
constexpr int FS_TABLE_LDS_MAX = 8064;                  // 16 n + 33792 <= 163840 - 1024: the table beside the rows
static_assert(16 * (size_t)FS_TABLE_LDS_MAX + FS_ROWS_LDS <= FS_LDS_LIMIT, "table and rows must fit in LDS");
constexpr size_t FS_MAX_SLAB = 65535ull * 64;

constexpr unsigned char FS_LIVE = 0, FS_NONFINITE = 1, FS_OUTSIDE_DAY = 2;
constexpr unsigned char FS_FLAG_EXACT = 1, FS_FLAG_OUTSIDE = 2;

typedef double fs_v4 __attribute__((ext_vector_type(4)));

struct FsCall {
    const float* data;              // (S, C, N)
    const long long* start;         // (n_windows)
    const double* taper;            // (n)
    const double2* twiddles;        // (n): cos, -sin of 2 pi m / n
    const int* bins;                // (K_b) ascending
    double2* result;                // (slab, K_b): the unscaled sums
    unsigned char* status;          // (slab)
    long long row0, rows, N;        // the slab's first row; rows in all
    int S, C, n, n_bins;
};

struct FsLayout {
    double2* result;
    unsigned char* status;
};

// the one statement of the workspace: bpmf_fft_spectrum_workspace_size runs it on a null base
static size_t fs_carve(void* base, size_t slab, size_t n_bins, FsLayout& l)
{
    Carver c(base);
    l.result = (double2*)c.take<double>(slab * n_bins * 2);
    l.status = c.take<unsigned char>(slab);
    return c.bytes();
}

template <bool TABLE_IN_LDS, int TILES>
__global__ __launch_bounds__(256) void fs_dft_kernel(const FsCall call, unsigned char* __restrict__ valid)
{
    extern __shared__ double fs_lds[];
    double* rows_lds = fs_lds;                                             // [64][FS_ROW_STRIDE]
    const double2* table = call.twiddles;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = call.n;
    if (TABLE_IN_LDS) {
        double2* t = (double2*)(fs_lds + FS_ROWS * FS_ROW_STRIDE);
        for (int m = threadIdx.x; m < n; m += 256) t[m] = call.twiddles[m];
        table = t;
    }
    const long long in_slab0 = (long long)blockIdx.x * FS_ROWS + wave * 16;
    const int bin0 = blockIdx.y * (TILES * 16);

    // lane i < 16: where row i of this wave begins in the day, or -1 (past the last row, or a window not inside the day)
    long long my_base = -1;
    int my_state = -1;                                                     // -1: no such row
    long long my_win = 0;
    int my_c = 0;
    if (lane < 16) {
        const long long r = call.row0 + in_slab0 + lane;
        if (r < call.rows) {
            const DayRow dr = day_row(call.S, call.C, call.N, call.start, (unsigned)r);
            my_win = dr.win, my_c = dr.c;
            const bool inside = day_window_inside(dr.start, n, call.N);
            my_state = inside ? FS_LIVE : FS_OUTSIDE_DAY;
            if (inside) my_base = dr.trace + dr.start;
        }
    }

    // B: lane l holds sample (l >> 4) of the k-step and bin (l & 15) of the tile
    const int col = lane & 15, kk = lane >> 4;
    int idx[TILES], step[TILES];
    bool live_bin[TILES];
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
        const int b = bin0 + t * 16 + col;
        live_bin[t] = b < call.n_bins;
        int k = live_bin[t] ? call.bins[b] : 0;
        k = k < 0 ? 0 : k;                                                 // (whatever the list holds, idx stays in the table)
        idx[t] = (int)(((long long)kk * k) % n);
        step[t] = (int)((4ll * k) % n);
    }
    fs_v4 re[TILES], im[TILES];
#pragma unroll
    for (int t = 0; t < TILES; ++t) re[t] = im[t] = fs_v4{0.0, 0.0, 0.0, 0.0};

    unsigned bad = 0;                                                      // bit i: row i of this wave, my samples
    const double* a_row = rows_lds + (size_t)(wave * 16 + col) * FS_ROW_STRIDE + kk;
    // The day's samples of a chunk are fetched one chunk ahead, all 16 loads of a lane issued together, and are in
    // flight while the chunk before is multiplied; a lane without a sample (row past the last, window outside the
    // day, j >= n) reads element 0 of the day and drops it.
    float xs[16];
    double w = 0.0;
    {
        const bool in = lane < n;
        w = in ? call.taper[lane] : 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const long long base = __shfl(my_base, i);
            xs[i] = call.data[base >= 0 && in ? base + lane : 0];
        }
    }
    double2 tw[TILES];                                                  // B of the k-step to come, one step ahead
    for (int j0 = 0; j0 < n; j0 += FS_CHUNK) {
        __syncthreads();                                                   // the chunk before is read (and the table loaded)
        const int j = j0 + lane;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const bool have = __shfl(my_base, i) >= 0 && j < n;
            const float x = xs[i];
            const bool finite = x - x == 0.0f;
            if (have && !finite) bad |= 1u << i;
            rows_lds[(size_t)(wave * 16 + i) * FS_ROW_STRIDE + lane] = have && finite ? (double)x * w : 0.0;
        }
        __syncthreads();
        if (j0 + FS_CHUNK < n) {
            const int jn = j + FS_CHUNK;
            const bool in = jn < n;
            w = in ? call.taper[jn] : 0.0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const long long base = __shfl(my_base, i);
                xs[i] = call.data[base >= 0 && in ? base + jn : 0];
            }
        }
        const int left = n - j0;
        const int k_steps = left >= FS_CHUNK ? FS_CHUNK / 4 : (left + 3) / 4;
        double a = a_row[0];
        if (j0 == 0) {
#pragma unroll
            for (int t = 0; t < TILES; ++t) tw[t] = table[idx[t]];
        }
        for (int ks = 0; ks < k_steps; ++ks) {
            // A and B of the next k-step are read while this one is multiplied (behind the last: read and dropped)
            const double a_next = a_row[4 * (ks + 1 < k_steps ? ks + 1 : ks)];
            double2 tw_next[TILES];
#pragma unroll
            for (int t = 0; t < TILES; ++t) {
                const int next = idx[t] + step[t];
                idx[t] = next >= n ? next - n : next;
                tw_next[t] = table[idx[t]];
            }
#pragma unroll
            for (int t = 0; t < TILES; ++t) {
                const double b_re = live_bin[t] ? tw[t].x : 0.0, b_im = live_bin[t] ? tw[t].y : 0.0;
                re[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b_re, re[t], 0, 0, 0);
                im[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b_im, im[t], 0, 0, 0);
                asm volatile("" : "+a"(re[t]), "+a"(im[t]));               // the sums stay in accumulator registers
            }
            a = a_next;
#pragma unroll
            for (int t = 0; t < TILES; ++t) tw[t] = tw_next[t];
        }
    }

    // C/D of the f64 form: lane l holds bin (l & 15) of rows (l >> 4) + 4 g, g = 0 .. 3
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
        const int b = bin0 + t * 16 + col;
        if (b < call.n_bins) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const long long in_slab = in_slab0 + kk + 4 * g;
                if (call.row0 + in_slab < call.rows)
                    call.result[(size_t)in_slab * call.n_bins + b] = make_double2(re[t][g], im[t][g]);
            }
        }
    }
    if (blockIdx.y == 0) {
        int state = my_state;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const bool any = __ballot((bad >> i) & 1u) != 0ull;
            if (lane == i && any && state == FS_LIVE) state = FS_NONFINITE;
        }
        if (lane < 16 && state >= 0) {
            call.status[in_slab0 + lane] = (unsigned char)state;
            if (my_c == 0) valid[my_win] = state == FS_OUTSIDE_DAY ? 0 : 1;
        }
    }
}

struct FsEpilogue {
    const double2* result;          // (slab, K_b)
    const unsigned char* status;    // (slab)
    const int* pair;                // (F): the index in `bins` of the bin at or below the target
    const double* dx;               // (F): target - freq[bin]
    const double* span;             // (F): freq[bin + 1] - freq[bin]
    const unsigned char* flags;     // (F): FS_FLAG_EXACT | FS_FLAG_OUTSIDE
    double* out;
    double delta;
    long long row0, units;          // the slab's first row; rows (or, multi_component, windows) of this slab
    int C, n_bins, n_targets, multi;
};

// |X| delta at bin b of one row; np.abs of a complex is hypot
__device__ inline double fs_modulus(const FsEpilogue& e, long long in_slab, int b)
{
    const double2 v = e.result[(size_t)in_slab * e.n_bins + b];
    return hypot(v.x * e.delta, v.y * e.delta);
}

// the spectrum a target is interpolated in: a row's modulus, or the root of a window's summed squares
__device__ inline double fs_level(const FsEpilogue& e, long long unit, int b)
{
    if (!e.multi) return fs_modulus(e, unit, b);
    double total = 0.0;
    for (int c = 0; c < e.C; ++c) {
        const double m = fs_modulus(e, unit * e.C + c, b);
        total = total + m * m;
    }
    return sqrt(total);
}

__global__ __launch_bounds__(256) void fs_epilogue_kernel(const FsEpilogue e)
{
    const int per_unit = e.n_targets ? e.n_targets : e.n_bins;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= e.units * per_unit) return;
    const long long unit = i / per_unit;
    const int q = (int)(i - unit * per_unit);
    int state = FS_LIVE;
    if (e.multi) {
        for (int c = 0; c < e.C; ++c) {
            const int s = e.status[unit * e.C + c];
            state = s > state ? s : state;                                 // (a window outside the day: all its rows)
        }
    } else {
        state = e.status[unit];
    }
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const long long out_unit = e.row0 / (e.multi ? e.C : 1) + unit;
    if (e.n_targets == 0) {
        if (e.multi) {
            e.out[(size_t)out_unit * e.n_bins + q] = state == FS_OUTSIDE_DAY ? 0.0 : state == FS_NONFINITE ? nan
                                                                                    : fs_level(e, unit, q);
            return;
        }
        const double2 v = e.result[(size_t)unit * e.n_bins + q];
        double2 o = make_double2(v.x * e.delta, v.y * e.delta);
        if (state == FS_OUTSIDE_DAY) o = make_double2(0.0, 0.0);
        if (state == FS_NONFINITE) o = make_double2(nan, nan);
        ((double2*)e.out)[(size_t)out_unit * e.n_bins + q] = o;
        return;
    }
    const unsigned char f = e.flags[q];
    double o;
    if ((f & FS_FLAG_OUTSIDE) || state == FS_OUTSIDE_DAY) {
        o = 0.0;
    } else if (state == FS_NONFINITE) {
        o = nan;
    } else {
        int p = e.pair[q];
        p = p < 0 ? 0 : (p > e.n_bins - 1 ? e.n_bins - 1 : p);             // (whatever the list holds, inside the slab)
        const double lo = fs_level(e, unit, p);
        if (f & FS_FLAG_EXACT) {
            o = lo;
        } else {
            const double hi = fs_level(e, unit, p + 1 < e.n_bins ? p + 1 : p);
            const double slope = (hi - lo) / e.span[q];
            o = slope * e.dx[q] + lo;                                      // (built with -ffp-contract=off: two roundings)
        }
    }
    e.out[(size_t)out_unit * e.n_targets + q] = o;
}

static bool fs_sizes_ok(size_t n_samples, size_t n_bins, size_t n_targets)
{
    return n_samples >= (size_t)FS_MIN_SAMPLES && n_samples <= (size_t)FS_MAX_SAMPLES && n_bins >= 1 &&
           n_bins <= n_samples / 2 + 1 && n_targets <= (size_t)FS_MAX_TARGETS;
}

}  // namespace bpmf

using namespace bpmf;

extern "C" size_t bpmf_fft_spectrum_workspace_size(size_t n_rows, size_t n_samples, size_t n_bins, size_t n_targets)
{
    if (!fs_sizes_ok(n_samples, n_bins, n_targets) || n_rows >= (1ull << 31)) return 0;
    const size_t widest = 2 * n_bins > n_targets ? 2 * n_bins : n_targets;
    if (n_rows > 0x7fffffffull / widest) return 0;
    FsLayout l;
    return fs_carve(nullptr, align_up(n_rows ? n_rows : 1, 64), n_bins, l);
}

extern "C" int bpmf_fft_spectrum_dev(const float* d_data, size_t S, size_t C, size_t N, size_t n_windows,
                                     const long long* d_starts, size_t n_samples, const double* d_taper,
                                     const double* d_twiddles, double delta, const int* d_bins, size_t n_bins,
                                     const int* d_pair, const double* d_dx, const double* d_span,
                                     const unsigned char* d_flags, size_t n_targets, int multi_component,
                                     void* d_workspace, size_t workspace_bytes, bpmf_stream_t stream_, double* d_out,
                                     unsigned char* d_valid)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n_windows == 0) return 0;
    const bool null_pointer = !d_data || !d_starts || !d_taper || !d_twiddles || !d_bins || !d_workspace || !d_out ||
                              !d_valid || (n_targets && (!d_pair || !d_dx || !d_span || !d_flags));
    if (day_rows_refused("bpmf_fft_spectrum_dev", true, null_pointer, S, C, N, n_windows, set_error)) return -1;
    if (!fs_sizes_ok(n_samples, n_bins, n_targets)) {
        set_error("bpmf_fft_spectrum_dev: need %d .. %d samples, 1 .. n_samples / 2 + 1 bins and at most %d targets "
                  "(n_samples=%zu n_bins=%zu n_targets=%zu)", FS_MIN_SAMPLES, FS_MAX_SAMPLES, FS_MAX_TARGETS,
                  n_samples, n_bins, n_targets);
        return -1;
    }
    if (multi_component && C > 64) {
        set_error("bpmf_fft_spectrum_dev: multi_component takes at most 64 components (C=%zu)", C);
        return -1;
    }
    if (!(delta - delta == 0.0)) {
        set_error("bpmf_fft_spectrum_dev: delta = %g; a finite number is needed", delta);
        return -1;
    }
    const size_t rows = n_windows * C;
    const size_t widest = 2 * n_bins > n_targets ? 2 * n_bins : n_targets;
    if (rows > 0x7fffffffull / widest) {
        set_error("bpmf_fft_spectrum_dev: %zu rows x %zu values; fewer than 2^31 values fit", rows, widest);
        return -1;
    }
    FsLayout layout;
    const size_t least = fs_carve(nullptr, 64, n_bins, layout);
    if (workspace_bytes < least) {
        set_error("bpmf_fft_spectrum_dev: the workspace holds %zu bytes; 64 rows of %zu bins take %zu "
                  "(bpmf_fft_spectrum_workspace_size)", workspace_bytes, n_bins, least);
        return -1;
    }
    const size_t per_row = multi_component ? 1 : 2;                        // doubles of d_out per bin without targets
    const size_t out_values = n_targets ? (multi_component ? n_windows : rows) * n_targets
                                        : (multi_component ? n_windows : rows) * n_bins * per_row;
    // option debug.poison_output (tests): an element the kernels skip comes back as NaN / 255
    if (option(OPT_DEBUG_POISON_OUTPUT) != 0) {
        BPMF_HIP_CHECK(hipMemsetAsync(d_out, 0xFF, out_values * sizeof(double), stream));
        BPMF_HIP_CHECK(hipMemsetAsync(d_valid, 0xFF, n_windows, stream));
    }
    // the largest multiple of 64 rows whose layout fits (the layout is monotone in the rows)
    size_t slab = workspace_bytes / (n_bins * 2 * sizeof(double)) / 64 * 64;
    slab = slab > align_up(rows, 64) ? align_up(rows, 64) : slab;
    slab = slab > FS_MAX_SLAB ? FS_MAX_SLAB : slab;
    slab = slab < 64 ? 64 : slab;
    while (slab > 64 && fs_carve(nullptr, slab, n_bins, layout) > workspace_bytes) slab -= 64;
    fs_carve(d_workspace, slab, n_bins, layout);

    FsCall call{};
    call.data = d_data;
    call.start = d_starts;
    call.taper = d_taper;
    call.twiddles = (const double2*)d_twiddles;
    call.bins = d_bins;
    call.result = layout.result;
    call.status = layout.status;
    call.rows = (long long)rows, call.N = (long long)N;
    call.S = (int)S, call.C = (int)C, call.n = (int)n_samples, call.n_bins = (int)n_bins;

    FsEpilogue ep{};
    ep.result = layout.result;
    ep.status = layout.status;
    ep.pair = d_pair, ep.dx = d_dx, ep.span = d_span, ep.flags = d_flags;
    ep.out = d_out;
    ep.delta = delta;
    ep.C = (int)C, ep.n_bins = (int)n_bins, ep.n_targets = (int)n_targets, ep.multi = multi_component ? 1 : 0;

    // 1, 2 or 4 bin tiles per wave: the fewest that leave one group of bins where 64 or fewer are asked for
    const int tiles = n_bins > 32 ? FS_TILES : (n_bins > 16 ? 2 : 1);
    const bool in_lds = n_samples <= (size_t)FS_TABLE_LDS_MAX;
    const size_t lds = FS_ROWS_LDS + (in_lds ? n_samples * sizeof(double2) : 0);
    void (*kernel)(const FsCall, unsigned char*) =
        in_lds ? (tiles == 4 ? fs_dft_kernel<true, 4> : tiles == 2 ? fs_dft_kernel<true, 2> : fs_dft_kernel<true, 1>)
               : (tiles == 4 ? fs_dft_kernel<false, 4> : tiles == 2 ? fs_dft_kernel<false, 2> : fs_dft_kernel<false, 1>);
    if (lds > 64 * 1024)   // a long table: opt in to > 64 KB dynamic LDS
        BPMF_HIP_CHECK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)FS_LDS_LIMIT));
    // with multi_component a slab holds whole windows only
    const size_t advance = multi_component ? slab / C * C : slab;
    const unsigned bin_groups = (unsigned)((n_bins + tiles * 16 - 1) / (tiles * 16));
    const size_t per_unit = n_targets ? n_targets : n_bins;
    for (size_t row0 = 0; row0 < rows; row0 += advance) {
        const size_t here = rows - row0 < advance ? rows - row0 : advance;
        const dim3 grid((unsigned)((here + FS_ROWS - 1) / FS_ROWS), bin_groups);
        call.row0 = (long long)row0;
        call.rows = (long long)(row0 + here);                              // (rows behind this slab's are not touched)
        kernel<<<grid, dim3(256), lds, stream>>>(call, d_valid);
        ep.row0 = (long long)row0;
        ep.units = (long long)(multi_component ? here / C : here);
        const size_t threads = (size_t)ep.units * per_unit;
        fs_epilogue_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream>>>(ep);
        BPMF_LAUNCH_CHECK();
    }
    return 0;
}
