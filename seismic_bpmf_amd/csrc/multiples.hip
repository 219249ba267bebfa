// Events detected by several templates (TemplateGroup.remove_multiples, BPMF/dataset.py:5214-5282): the reference
// walks its time-sorted catalog and, for every event n1 that is still unique, gathers the neighbours n1, n1+1, ...
// for as long as the running float64 sum of the inter-event times stays < dt_criterion, keeps those still unique and
// pair_ok[row(n1), row(m)], and -- when two or more remain -- flags them all and restores the one with the largest cc
// (the earliest on equal cc).  The host definition is postprocess.flag_multiples; the result here equals it element
// for element.
//
// Two kernels on arrays that are ALREADY in the stable order of the origin times:
//
//   span kernel   one thread per event: end[n1] = first index past the neighbours of n1, by the same sequential
//                 float64 additions ie[n1+1] + ie[n1+2] + ... (ie[k] = t[k] - t[k-1]); independent of the flags.  It
//                 also writes unique[n1] = 1 and reports a template row outside [0, T) into the workspace.
//   flag kernel   event n starts a SEGMENT when n == 0 or !(ie[n] < dt_criterion).  ie[k] >= 0 and a rounded sum of
//                 non-negative terms is never below one of them, so no window crosses a segment boundary: segments
//                 are independent.  One wave per event; the waves of non-heads exit.  The head's wave walks the n1
//                 of its segment IN ORDER: its 64 lanes stride over [n1, end[n1]), test unique and pair_ok, a ballot
//                 counts the multiples, a wave reduction on (cc, then index) finds the keeper, and the lanes that
//                 hold a multiple store its flag.
//
// The flags one iteration stores are loaded by OTHER lanes of the same wave in the next: all flag accesses are
// relaxed atomics of workgroup scope (plain byte loads / stores on the vector path, never the scalar cache) and a
// workgroup-scope fence (the wave is the workgroup) stands between the stores of one n1 and the loads of the next.
//
// Limit: one segment -- a swarm without a gap of dt_criterion -- is walked by ONE wave, about three dependent
// round trips to memory per visited event.
#include "common.h"
#include "../../include/bpmf_hip.h"

namespace bpmf {

constexpr size_t FM_ERROR_BYTES = 16;         // the row-check word, a block of its own at the workspace's start
constexpr int FM_NO_EVENT = 0x7fffffff;

__device__ __forceinline__ unsigned flag_load(const uint8_t* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ void flag_store(uint8_t* p, uint8_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__global__ __launch_bounds__(256) void multiples_span_kernel(const double* __restrict__ t,
                                                             const int32_t* __restrict__ rows, int n, int n_templates,
                                                             double dt, int* __restrict__ end, int* __restrict__ bad_row,
                                                             uint8_t* __restrict__ unique)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int n1 = (int)i;
    const int r = rows[n1];
    if (r < 0 || r >= n_templates) atomicMax(bad_row, n1);
    unique[n1] = 1;
    int n2 = n1 + 1;
    if (n2 < n) {
        // the reference's loop: dt_n1n2 = ie[n1+1]; while dt_n1n2 < dt: take n2, dt_n1n2 += ie[n2+1]
        double prev = t[n2];
        double acc = prev - t[n1];
        while (acc < dt) {
            ++n2;
            if (n2 >= n) break;
            const double cur = t[n2];
            acc = __dadd_rn(acc, __dsub_rn(cur, prev));
            prev = cur;
        }
    }
    end[n1] = n2;
}

__global__ __launch_bounds__(64) void multiples_flag_kernel(const double* __restrict__ t,
                                                            const int32_t* __restrict__ rows,
                                                            const float* __restrict__ cc, int n,
                                                            const uint8_t* __restrict__ pair_ok, int n_templates,
                                                            double dt, const int* __restrict__ end, uint8_t* unique)
{
    const int head = (int)blockIdx.x;
    const int lane = (int)threadIdx.x;
    if (head > 0 && __dsub_rn(t[head], t[head - 1]) < dt) return;         // not the first event of a segment
    for (int n1 = head; n1 < n; ++n1) {
        // everything the visit of n1 needs, requested at once (all of it wave-uniform)
        const int e = end[n1];
        const int r1 = rows[n1];
        const unsigned u1 = flag_load(unique + n1);
        if (n1 > head && !(__dsub_rn(t[n1], t[n1 - 1]) < dt)) break;      // the next segment: its own wave's
        if (e - n1 < 2) continue;                                         // no neighbour
        if (u1 == 0) continue;                                            // flagged by an earlier n1: not visited
        if (r1 < 0 || r1 >= n_templates) continue;                        // (the call fails; never read past the table)
        const uint8_t* __restrict__ ok_row = pair_ok + (size_t)r1 * (size_t)n_templates;
        // a multiple: a neighbour that is still unique and whose template passes the pair test with n1's.  The flag,
        // the row and the cc of a lane's event are independent loads (a lane past the window reads n1's); only the
        // pair test waits for the row.
        auto is_multiple = [&](int m, float* c) -> bool {
            const bool inside = m < e;
            const int mm = inside ? m : n1;
            const unsigned u = flag_load(unique + mm);
            const int rm = rows[mm];
            if (c) *c = cc[mm];
            const bool valid = inside && u != 0 && rm >= 0 && rm < n_templates;
            return ok_row[valid ? rm : 0] != 0 && valid;
        };
        int count = 0;
        float best_cc = -INFINITY;
        int best = FM_NO_EVENT;
        for (int base = n1; base < e; base += 64) {
            const int m = base + lane;
            float c;
            const bool mult = is_multiple(m, &c);
            count += __popcll(__ballot(mult));
            if (mult && (best == FM_NO_EVENT || c > best_cc)) {           // m grows within a lane: `>` keeps the earliest
                best_cc = c;
                best = m;
            }
        }
        if (count < 2) continue;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float oc = __shfl_xor(best_cc, o);
            const int ob = __shfl_xor(best, o);
            if (ob != FM_NO_EVENT && (best == FM_NO_EVENT || oc > best_cc || (oc == best_cc && ob < best))) {
                best_cc = oc;
                best = ob;
            }
        }
        // no flag has changed since the first pass: the same test names the same multiples
        for (int base = n1; base < e; base += 64) {
            const int m = base + lane;
            if (is_multiple(m, nullptr)) flag_store(unique + m, m == best ? 1 : 0);
        }
        // the stores above before the flag loads of the next n1, whichever lanes issue them: the fence orders them
        // in the memory model, the wait holds the wave until the stores are acknowledged
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
}

}  // namespace bpmf

using namespace bpmf;

struct FmWs { int *bad_row, *end; size_t bytes; };      // the row-check word, the span ends of the n events
static FmWs fm_carve(void* base, size_t n)
{
    FmWs w;
    Carver c(base);
    w.bad_row = (int*)c.nest(FM_ERROR_BYTES, 16);
    w.end = c.take<int>(n, 0, 16);
    w.bytes = c.bytes();
    return w;
}

extern "C" size_t bpmf_flag_multiples_workspace_bytes(size_t n)
{
    if (n > 0x7ffffffeull) return 0;                      // (more events than the call takes)
    return fm_carve(nullptr, n).bytes;
}

extern "C" int bpmf_flag_multiples_dev(const double* d_t_sorted, const int32_t* d_rows_sorted, const float* d_cc_sorted,
                                       size_t n, const uint8_t* d_pair_ok, size_t T, double dt_criterion,
                                       void* d_workspace, size_t workspace_bytes, bpmf_stream_t stream_,
                                       uint8_t* d_unique_out)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n == 0) return 0;
    if (!d_t_sorted || !d_rows_sorted || !d_cc_sorted || !d_pair_ok || !d_workspace || !d_unique_out) {
        set_error("bpmf_flag_multiples_dev: null pointer");
        return -1;
    }
    if (n > 0x7ffffffeull || T == 0 || T > 0x7fffffffull) {
        set_error("bpmf_flag_multiples_dev: bad argument (n=%zu T=%zu)", n, T);
        return -1;
    }
    const FmWs ws = fm_carve(d_workspace, n);
    if (workspace_bytes < ws.bytes) {
        set_error("bpmf_flag_multiples_dev: workspace of %zu bytes, %zu needed", workspace_bytes, ws.bytes);
        return -1;
    }
    BPMF_HIP_CHECK(hipMemsetAsync(ws.bad_row, 0xFF, FM_ERROR_BYTES, stream));        // -1: below every index
    multiples_span_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(
        d_t_sorted, d_rows_sorted, (int)n, (int)T, dt_criterion, ws.end, ws.bad_row, d_unique_out);
    BPMF_LAUNCH_CHECK();
    multiples_flag_kernel<<<dim3((unsigned)n), dim3(64), 0, stream>>>(
        d_t_sorted, d_rows_sorted, d_cc_sorted, (int)n, d_pair_ok, (int)T, dt_criterion, ws.end, d_unique_out);
    BPMF_LAUNCH_CHECK();
    // the one synchronisation of the call: the row check comes back, and the flags are complete behind it
    int bad_row = 0;
    BPMF_HIP_CHECK(hipMemcpyAsync(&bad_row, ws.bad_row, sizeof(int), hipMemcpyDeviceToHost, stream));
    BPMF_HIP_CHECK(hipStreamSynchronize(stream));
    if (bad_row >= 0) {
        set_error("bpmf_flag_multiples_dev: event %d (in sorted order) names a template row outside [0, %zu)", bad_row, T);
        return -1;
    }
    return 0;
}
