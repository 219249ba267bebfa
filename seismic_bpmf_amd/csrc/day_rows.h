// The single statement in csrc/ of "row r of a batch of windows cut from the (S, C, N) float32 day"; the rule, and
// which entry points take it whole and which the limit alone, are in DESIGN.md, "Rows of day windows".  Nothing but
// <cstddef> is needed: a host compiler compiles the same text (tests/day_rows_check.cpp).
#pragma once
#include <cstddef>

#ifdef __HIPCC__
#define DAY_ROWS_FN __host__ __device__ __forceinline__
#else
#define DAY_ROWS_FN inline
#endif

namespace bpmf {

constexpr long long DAY_INDEX_LIMIT = 1ll << 40;       // N and |start| (|origin|, |offset|, ...) of every entry point

struct DayRow {
    int win, c, s;                  // the window item / C, its component, its station win % S
    long long trace, start;         // element offset of data[s, c, 0]; the first sample start[win] (none: 0), clamped
};

// Divided in the caller's type: 32 bits do (day_rows_refused); picker.hip and resample.hip keep their size_t.
template <typename Index>
DAY_ROWS_FN DayRow day_row(int S, int C, long long N, const long long* start, Index item)
{
    const Index win = item / (Index)C, c = item - win * (Index)C, s = win % (Index)S;
    const long long trace = (long long)(s * (Index)C + c) * N, i0 = start ? start[win] : 0;
    return {(int)win, (int)c, (int)s, trace,
            i0 > DAY_INDEX_LIMIT ? DAY_INDEX_LIMIT : (i0 < -DAY_INDEX_LIMIT ? -DAY_INDEX_LIMIT : i0)};
}

DAY_ROWS_FN bool day_window_inside(long long i0, long long n, long long N) { return i0 >= 0 && i0 + n <= N; }

// x[i] inside the trace of n samples, +0.0 outside; the address is clamped, so the load is never predicated (n >= 1)
DAY_ROWS_FN float clipped_sample(const float* __restrict__ x, long long i, long long n)
{
    const long long ic = i < 0 ? 0 : (i >= n ? n - 1 : i);
    const float v = x[ic];
    return ic == i ? v : 0.0f;
}

// True after report(format, ...) of what no kernel here can address: `null_pointer` (the entry point's own test), no
// data, N above the limit, 2^31 rows (windows x C) or traces (S x C), or, with `whole_events`, windows % S != 0.
template <typename Report>
inline bool day_rows_refused(const char* name, bool whole_events, bool null_pointer, size_t S, size_t C, size_t N,
                             size_t windows, Report report)
{
    if (null_pointer)
        report("%s: null pointer", name);
    else if (S == 0 || C == 0 || N == 0 || N > (size_t)DAY_INDEX_LIMIT || windows > 0x7fffffffull / C ||
             S > 0x7fffffffull / C || (whole_events && windows % S != 0))
        report(whole_events ? "%s: bad argument (S=%zu C=%zu N=%zu windows=%zu): need data, a whole number of events "
                              "and fewer than 2^31 rows" : "%s: bad argument (S=%zu C=%zu N=%zu rows=%zu)",
               name, S, C, N, windows);
    else
        return false;
    return true;
}

}  // namespace bpmf
