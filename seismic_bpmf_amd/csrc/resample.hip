// Polyphase resampling on the device: scipy.signal.resample_poly(x, up, down) of float32 rows, the step between the
// cut windows and the deep-learning picker in Event.pick_PS_phases (BPMF/dataset.py:1801-1804, 5596-5599).  The
// definition is postprocess.resample_poly_host and the device equals it bit for bit.
//
// bpmf_resample_poly_dev -- row (r, c) is cut by the rule of day_rows.h, +0.0 outside the day, exactly the rows of
// bpmf_normalize_batch_dev.  The caller brings the plan of
// postprocess.resample_poly_plan: the float32 tap table (hp taps for each of the `up` phases: the Kaiser filter times
// up, with the zeros upfirdn runs it with in front and behind) and n_pre_remove.  Output q of a row has
//     m = q + n_pre_remove,  j_hi = m down / up,  t = m down % up,
//     acc = +0;  for k = hp - 1 .. 0:  j = j_hi - k;  acc = fl(acc + fl(x[j] * table[t + k up]))  where 0 <= j < n_in
// One workgroup of 256 threads per (row, tile of outputs), so a row of any length works:
//   1. the tap table and the input span of the tile, x[j_hi(first) - hp + 1 .. j_hi(last)], are staged in LDS.  The
//      WINDOW is cut first: a sample beside the window enters as +0.0 although the day holds it, as the reference
//      filters the cut window with zero padding (and a thread never reaches it: its k range ends at the window);
//   2. one thread per output runs the chain, input index ascending, with one rounded multiply and one rounded add per
//      tap (__fmul_rn / __fadd_rn: never contracted into a fused multiply-add, which would change the bits).  The zero
//      taps of the padding do multiply: a NaN sample spreads as far as SciPy spreads it.
// The host picks the tile -- a multiple of 64 outputs, at most 1024 -- so that table + span stay within
// RS_LDS_FLOATS (bpmf_resample_poly_tile).  Index arithmetic in 64 bits.  Plain vector stores, no atomics; every
// output element is written.
#include "common.h"
#include "day_rows.h"
#include <numeric>
#include "../../include/bpmf_hip.h"

namespace bpmf {

constexpr int RS_THREADS = 256;
constexpr size_t RS_MAX_RATE = 64;                     // max(up, down), reduced
constexpr size_t RS_MAX_TABLE = 2048;                  // hp * up floats; the plan needs at most 22 * 64 + 64
constexpr size_t RS_LDS_FLOATS = 12288;                // table + span: 48 KB
constexpr size_t RS_MAX_TILE = 1024, RS_TILE_STEP = 64;

// the input samples a tile of `tile` outputs can span: j_hi(last) - j_hi(first) <= ceil((tile - 1) down / up)
inline size_t rs_span(size_t tile, size_t up, size_t down, size_t hp)
{
    return ((tile - 1) * down + up - 1) / up + hp;
}

inline size_t rs_tile(size_t up, size_t down, size_t hp)
{
    size_t tile = RS_MAX_TILE;
    while (tile > RS_TILE_STEP && hp * up + rs_span(tile, up, down, hp) > RS_LDS_FLOATS) tile -= RS_TILE_STEP;
    return tile;
}

__global__ __launch_bounds__(RS_THREADS) void resample_poly_kernel(
    const float* __restrict__ data, int S, int C, long long N, const long long* __restrict__ start, long long n_in,
    int up, int down, const float* __restrict__ table, int hp, long long n_pre_remove, long long n_out, int tile,
    long long n_tiles, float* __restrict__ out)
{
    extern __shared__ __align__(16) float rs_lds[];
    float* tab = rs_lds;                                           // hp * up taps
    float* xs = rs_lds + hp * up;                                  // the tile's input span, at most rs_span samples
    const int tid = threadIdx.x;
    const size_t item = (size_t)blockIdx.x / (size_t)n_tiles;      // (r, c) flattened
    const long long q0 = (long long)((size_t)blockIdx.x % (size_t)n_tiles) * tile;
    const DayRow dr = day_row(S, C, N, start, item);
    const float* __restrict__ x = data + dr.trace;
    const int nq = n_out - q0 < tile ? (int)(n_out - q0) : tile;   // >= 1: n_tiles = ceil(n_out / tile)
    const long long md0 = (q0 + n_pre_remove) * down;              // the tile's first output, in upsampled samples
    const long long j_first = md0 / up;
    const int t_first = (int)(md0 - j_first * up);
    const long long j_base = j_first - (hp - 1);
    const int span = (t_first + (nq - 1) * down) / up + hp;        // up to j_hi of the tile's last output

    for (int p = tid; p < hp * up; p += RS_THREADS) tab[p] = table[p];
    for (int p = tid; p < span; p += RS_THREADS) {
        const long long j = j_base + p;
        xs[p] = j >= 0 && j < n_in ? clipped_sample(x, dr.start + j, N) : 0.0f;
    }
    __syncthreads();

    float* __restrict__ o = out + item * (size_t)n_out + (size_t)q0;
    for (int l = tid; l < nq; l += RS_THREADS) {
        const int md = t_first + l * down;                         // < 64 + 1024 * 64: 32 bits do from here
        const int j_rel = md / up, t = md - j_rel * up;
        const long long j_hi = j_first + j_rel;
        // the taps whose sample lies in the window: 0 <= j_hi - k < n_in
        const int k_first = j_hi < hp - 1 ? (int)j_hi : hp - 1;
        const long long past = j_hi - (n_in - 1);
        const int k_last = past > hp ? hp : (past > 0 ? (int)past : 0);
        const float* __restrict__ xj = xs + (hp - 1 + j_rel);      // xj[-k] = x[j_hi - k]
        float acc = 0.0f;
        for (int k = k_first; k >= k_last; --k) acc = __fadd_rn(acc, __fmul_rn(xj[-k], tab[t + k * up]));
        o[l] = acc;
    }
}

}  // namespace bpmf

using namespace bpmf;

extern "C" size_t bpmf_resample_poly_tile(size_t up, size_t down, size_t taps_per_phase)
{
    if (up < 1 || down < 1 || up > RS_MAX_RATE || down > RS_MAX_RATE || taps_per_phase < 1 ||
        taps_per_phase * up > RS_MAX_TABLE)
        return 0;
    return rs_tile(up, down, taps_per_phase);
}

extern "C" int bpmf_resample_poly_dev(const float* d_data, size_t S, size_t C, size_t N, size_t n_rows,
                                      const int64_t* d_start_or_null, size_t n_in, size_t up, size_t down,
                                      const float* d_table, size_t taps_per_phase, size_t n_pre_remove, size_t n_out,
                                      bpmf_stream_t stream_, float* d_out)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n_rows == 0) return 0;
    if (day_rows_refused("bpmf_resample_poly_dev", false, !d_data || !d_table || !d_out, S, C, N, n_rows, set_error))
        return -1;
    if (up < 1 || down < 1 || up > RS_MAX_RATE || down > RS_MAX_RATE || std::gcd(up, down) != 1 || up == down) {
        set_error("bpmf_resample_poly_dev: need 1 <= up, down <= %zu, reduced by their gcd and not both 1 (up=%zu "
                  "down=%zu)", RS_MAX_RATE, up, down);
        return -1;
    }
    const size_t rate = up > down ? up : down;
    if (n_in < 1 || n_in > ((size_t)DAY_INDEX_LIMIT - 1) / rate) {
        set_error("bpmf_resample_poly_dev: need n_in >= 1 and n_in * max(up, down) below 2^40 (n_in=%zu up=%zu "
                  "down=%zu)", n_in, up, down);
        return -1;
    }
    if (n_out != (n_in * up + down - 1) / down) {
        set_error("bpmf_resample_poly_dev: %zu samples up %zu down %zu make %zu; n_out = %zu given", n_in, up, down,
                  (n_in * up + down - 1) / down, n_out);
        return -1;
    }
    // the plan's table holds 2 * 10 rate + 1 taps and the padding (under 2 rate); n_pre_remove = (10 rate + pad) / down
    if (taps_per_phase < 1 || taps_per_phase * up > RS_MAX_TABLE || n_pre_remove > taps_per_phase * up) {
        set_error("bpmf_resample_poly_dev: a table of %zu taps per phase x %zu phases (at most %zu taps) and "
                  "n_pre_remove = %zu are not a plan of postprocess.resample_poly_plan", taps_per_phase, up,
                  RS_MAX_TABLE, n_pre_remove);
        return -1;
    }
    const size_t tile = rs_tile(up, down, taps_per_phase), n_tiles = (n_out + tile - 1) / tile;
    const size_t n_items = n_rows * C;
    if (n_tiles > 0x7fffffffull / n_items) {
        set_error("bpmf_resample_poly_dev: %zu rows x %zu tiles of %zu outputs; fewer than 2^31 workgroups fit", n_items,
                  n_tiles, tile);
        return -1;
    }
    const size_t lds = (taps_per_phase * up + rs_span(tile, up, down, taps_per_phase)) * sizeof(float);   // <= 48 KB
    // option debug.poison_output (tests): an element the kernel skips comes back as NaN
    if (option(OPT_DEBUG_POISON_OUTPUT) != 0)
        BPMF_HIP_CHECK(hipMemsetAsync(d_out, 0xFF, n_items * n_out * sizeof(float), stream));
    resample_poly_kernel<<<dim3((unsigned)(n_items * n_tiles)), dim3(RS_THREADS), lds, stream>>>(
        d_data, (int)S, (int)C, (long long)N, (const long long*)d_start_or_null, (long long)n_in, (int)up, (int)down,
        d_table, (int)taps_per_phase, (long long)n_pre_remove, (long long)n_out, (int)tile, (long long)n_tiles,
        d_out);
    BPMF_LAUNCH_CHECK();
    return 0;
}
