// Backprojection hot path for MI355X (gfx950): beam-power shift-and-stack of S*C feature
// traces over K candidate sources and P phases, with per-sample max / arg-max.
//
// Serves beampower.beampower.beamform as called by the reference at
// BPMF/template_search.py:549-558 (reduce="max") and :560-569 (reduce="none"); the beam
// definition is the reference's own (tutorial notebook 5, cells 27/30/32).  The arithmetic
// is not in the reference tree.  Conventions = oracle/bpmf_oracle.c:bp_cpu, bit for bit.
//
// Design (DESIGN.md section "BP"): the path is an on-chip gather, not a GEMM.
//   1. prestack  U[s,p,t] = sum_c alpha[s,c,p] * feat[s,c,t]            (HBM streaming)
//   2. beam      a workgroup owns a tile of consecutive time samples and walks ALL
//      sources, grouped by the host-side plan so that for one group the needed window of
//      every used (station, phase) trace fits in LDS together.  Per source the threads
//      gather lds[window(s,p) + tau[k,s,p] - tau_min + t] (consecutive lanes -> consecutive
//      banks) and accumulate with the source weight in registers, keeping a running
//      (max, arg-max) per time sample: no atomics, no cross-workgroup merge, and the
//      sequential source order gives the "lowest index wins ties" rule for free.
#include "bp_plan.h"
#include "bp_plan_cache.h"
#include "host_call.h"
#include <mutex>
#include <cstring>
#include <type_traits>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace bpmf {

// ------------------------------------------------------------------- prestack ---
// One thread per (station, time sample): reads the C components once, writes P phases.
template <int MAXP>
__global__ __launch_bounds__(256) void bp_prestack_kernel(const float* __restrict__ feat,
                                                          const float* __restrict__ w_ph,
                                                          long long N, int C, int P,
                                                          float* __restrict__ U, long long t_lo, long long t_hi)
{
    // (samples [t_lo, t_hi): the whole series, or one piece of a day that is still arriving from the host)
    const long long t = t_lo + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int s = blockIdx.y;
    if (t >= t_hi) return;
    float acc[MAXP];
#pragma unroll
    for (int p = 0; p < MAXP; ++p) acc[p] = 0.0f;
    for (int c = 0; c < C; ++c) {
        const float f = feat[((size_t)s * C + c) * (size_t)N + t];
#pragma unroll
        for (int p = 0; p < MAXP; ++p)
            if (p < P) acc[p] = __fmaf_rn(w_ph[((size_t)s * C + c) * P + p], f, acc[p]);
    }
#pragma unroll
    for (int p = 0; p < MAXP; ++p)
        if (p < P) U[((size_t)s * P + p) * (size_t)N + t] = acc[p];
}

// Generic P (slow path, P > 4): one thread per (s, p, t).
__global__ void bp_prestack_any_kernel(const float* __restrict__ feat,
                                       const float* __restrict__ w_ph, long long N, int C, int P,
                                       float* __restrict__ U, long long t_lo, long long t_hi)
{
    const long long t = t_lo + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int s = blockIdx.y / P, p = blockIdx.y % P;
    if (t >= t_hi) return;
    float acc = 0.0f;
    for (int c = 0; c < C; ++c)
        acc = __fmaf_rn(w_ph[((size_t)s * C + c) * P + p], feat[((size_t)s * C + c) * (size_t)N + t],
                        acc);
    U[((size_t)s * P + p) * (size_t)N + t] = acc;
}

// ----------------------------------------------------------------------- beam ---
// A batch of short series (event relocation, bp_relocate.hip): gridDim.z = events, every one with its own
// prestack `u_estride` floats and its own outputs `out_estride` elements behind the previous event's.  N
// and all bounds stay those of ONE event, so a window never reads its neighbour's samples.  The kernels take
// this as a template flag (BATCH, reduce="max" only): a day runs the instantiation without it, whose code is
// what it was before batches existed -- the packed kernel sits at the edge of its scalar registers.
__device__ __forceinline__ void bp_select_event(const float* __restrict__& U, float* __restrict__& out_beam,
                                                int* __restrict__& out_arg, long long u_estride, long long out_estride)
{
    U += (size_t)blockIdx.z * (size_t)u_estride;
    out_beam += (size_t)blockIdx.z * (size_t)out_estride;
    out_arg += (size_t)blockIdx.z * (size_t)out_estride;
}

template <int NBLK>
struct BpMeta {  // one source's wave-uniform metadata, spread over the lanes of a wave
    int hd;
    int mo[NBLK];
    float mb[NBLK];
    __device__ __forceinline__ void load(const int* __restrict__ srcs,
                                         const int* __restrict__ term_off,
                                         const float* __restrict__ term_beta, int NT, int k,
                                         int lane)
    {
        hd = srcs[(size_t)k * 4 + (lane & 3)];
#pragma unroll
        for (int q = 0; q < NBLK; ++q) {
            const int l = lane + 64 * q;
            mo[q] = l < NT ? term_off[(size_t)k * NT + l] : 0;
            mb[q] = l < NT ? term_beta[(size_t)k * NT + l] : 0.0f;
        }
    }
};

__device__ __forceinline__ int lane_bcast(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ float lane_bcast(float v, int lane)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// LDS layout of a group: [0, tile) is a slab of zeros that padded terms point at, then one
// window per used (station, phase) row: lds[base + x] = U[row][t0 + tau_min(row) + x].
//
// All per-source / per-chunk metadata is wave-uniform.  It is fetched with ONE coalesced
// vector load per wave (lane l <- entry l) one source ahead of its use and broadcast with
// v_readlane: no scalar-memory round trip sits between the LDS gathers (SMEM and LDS share
// the lgkm counter; round 3 found that ONE lgkmcnt(0) per source is cheap with 16 waves per CU --
// bp_fast.hip keeps its records in SGPRs -- but these general kernels predate that and only run the
// edge tiles of a day, reduce="none" and the P != 2 grids).
template <int TPT, int CHUNK, int NBLK, int OOB, int REDUCE, bool BATCH = false>
__global__ __launch_bounds__(BP_THREADS) void bp_beam_kernel(
    const float* __restrict__ U, long long N, const BpGroup* __restrict__ groups, int n_groups,
    const int4* __restrict__ chunks, const int* __restrict__ srcs,
    const int* __restrict__ term_off, const float* __restrict__ term_beta, int NT,
    int id_offset, float* __restrict__ out_beam, int* __restrict__ out_arg, long long tile_base, float best0,
    long long u_estride, long long out_estride)
{
    extern __shared__ float lds[];
    if constexpr (BATCH) bp_select_event(U, out_beam, out_arg, u_estride, out_estride);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    constexpr int TILE = BP_THREADS * TPT;
    const long long t0 = (tile_base + (long long)blockIdx.x) * TILE;

    float best[TPT];
    int arg[TPT];
#pragma unroll
    for (int j = 0; j < TPT; ++j) {
        best[j] = best0;
        arg[j] = id_offset;
        lds[tid + j * BP_THREADS] = 0.0f;  // the zero slab (never overwritten)
    }

    for (int g = 0; g < n_groups; ++g) {
        const BpGroup grp = groups[g];
        // Per-source metadata (header word l&3, term offsets, term weights: lane l <- entry l).
        // Three register sets rotate through the source loop (unrolled x3, no copies), so a
        // set is loaded two sources before it is consumed.  The first two are issued before
        // the staging.
        const int k_last = grp.first_src + grp.n_src - 1;
        BpMeta<NBLK> m0, m1, m2;
        m0.load(srcs, term_off, term_beta, NT, grp.first_src, lane);
        m1.load(srcs, term_off, term_beta, NT, min(grp.first_src + 1, k_last), lane);
        __syncthreads();  // previous group's gathers are done
        // ---- stage the group's windows: descriptors by readlane, 4 loads in flight per thread
        for (int cb = 0; cb < grp.n_chunk; cb += 64) {
            const int nb = min(64, grp.n_chunk - cb);
            int4 d = make_int4(0, 0, 0, 0);
            if (lane < nb) d = chunks[grp.first_chunk + cb + lane];
            for (int c = 0; c < nb; c += 4) {
                // descriptors first (readlane), then 4 unconditional loads from clamped
                // addresses (no branch between them, so all four stay in flight), then the
                // LDS writes with the out-of-range samples zeroed
                int row[4], dd[4], n[4];
                long long gi[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int cc = min(c + u, nb - 1);
                    row[u] = lane_bcast(d.x, cc);
                    gi[u] = t0 + lane_bcast(d.y, cc) + tid;
                    dd[u] = lane_bcast(d.z, cc);
                    n[u] = c + u < nb ? lane_bcast(d.w, cc) : 0;
                }
                float v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const long long gc = gi[u] < 0 ? 0 : (gi[u] >= N ? N - 1 : gi[u]);
                    v[u] = U[(size_t)row[u] * (size_t)N + gc];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (tid < n[u]) lds[dd[u] + tid] = (gi[u] >= 0 && gi[u] < N) ? v[u] : 0.0f;
            }
        }
        __syncthreads();
        // ---- walk the sources of the group, three per trip.  Past the end of the group the
        // clamped index re-processes the last source, which changes nothing (same id, same
        // value), so the trip needs no branch between its loads and their waits.
        auto process = [&](const BpMeta<NBLK>& m) {
            const int sid = lane_bcast(m.hd, 0), tmin = lane_bcast(m.hd, 1), tmax = lane_bcast(m.hd, 2);
            const int nterm = lane_bcast(m.hd, 3);  // terms padded to CHUNK; 0 = unused source
            float acc[TPT];
#pragma unroll
            for (int j = 0; j < TPT; ++j) acc[j] = 0.0f;

#define BP_LOAD(X, B, Q, C0)                                                          \
    _Pragma("unroll") for (int i = 0; i < CHUNK; ++i) {                               \
        const float* lp = lds + lane_bcast(m.mo[Q], (C0) + i) + tid;                  \
        B[i] = lane_bcast(m.mb[Q], (C0) + i);                                         \
        _Pragma("unroll") for (int j = 0; j < TPT; ++j) X[i][j] = lp[j * BP_THREADS]; \
    }
#define BP_FMA(X, B)                                                                  \
    _Pragma("unroll") for (int i = 0; i < CHUNK; ++i)                                 \
        _Pragma("unroll") for (int j = 0; j < TPT; ++j) acc[j] = __fmaf_rn(B[i], X[i][j], acc[j]);

#pragma unroll
            for (int q = 0; q < NBLK; ++q) {
                // chunks of block q, software-pipelined: the gathers of chunk i+1 are in
                // flight while chunk i is accumulated (same ascending fmaf order)
                const int nc = (min(64, nterm - 64 * q)) / CHUNK;
                if (nc <= 0) continue;
                float xa[CHUNK][TPT], xb[CHUNK][TPT], ba[CHUNK], bb[CHUNK];
                BP_LOAD(xa, ba, q, 0)
                for (int i2 = 1; i2 < nc; i2 += 2) {
                    BP_LOAD(xb, bb, q, i2 * CHUNK)
                    BP_FMA(xa, ba)
                    if (i2 + 1 < nc) { BP_LOAD(xa, ba, q, (i2 + 1) * CHUNK) }
                    BP_FMA(xb, bb)
                }
                if (nc & 1) { BP_FMA(xa, ba) }
            }
#undef BP_LOAD
#undef BP_FMA
#pragma unroll
            for (int j = 0; j < TPT; ++j) {
                const long long t = t0 + tid + j * BP_THREADS;
                bool computed = nterm > 0;
                if (OOB == BPMF_BP_STRICT) computed = computed && (t + tmin >= 0) && (t + tmax < N);
                if (REDUCE == BPMF_BP_REDUCE_MAX) {
                    // sources arrive in plan order, not index order: ties go to the lower id
                    const bool better = acc[j] > best[j] || (acc[j] == best[j] && sid < arg[j]);
                    if (computed && better) { best[j] = acc[j]; arg[j] = sid; }
                } else {
                    if (t < N)
                        out_beam[(size_t)(sid - id_offset) * (size_t)N + t] = computed ? acc[j] : 0.0f;
                }
            }
        };
        for (int k = grp.first_src; k <= k_last; k += 3) {
            m2.load(srcs, term_off, term_beta, NT, min(k + 2, k_last), lane);
            process(m0);
            m0.load(srcs, term_off, term_beta, NT, min(k + 3, k_last), lane);
            process(m1);
            m1.load(srcs, term_off, term_beta, NT, min(k + 4, k_last), lane);
            process(m2);
        }
    }
    if (REDUCE == BPMF_BP_REDUCE_MAX) {
#pragma unroll
        for (int j = 0; j < TPT; ++j) {
            const long long t = t0 + tid + j * BP_THREADS;
            if (t < N) { out_beam[t] = best[j]; out_arg[t] = arg[j]; }
        }
    }
}

// ------------------------------------------------ beam, one wave per source ---
// For sources with at most NTV (station, phase) terms (NTV <= 32).  The per-term metadata
// {LDS byte offset, weight} is loaded with VECTOR loads from a wave-uniform address (every lane
// receives the same value), ahead of its use, so that a term costs one address add, its gathers
// and their fmas.  (Round 1 ruled scalar loads out here -- SMEM shares the lgkm counter with the
// LDS gathers -- see the note above bp_beam_kernel; v_readlane broadcasting costs two more VALU
// issues per term.)

template <int NTV>
struct BpMetaV {
    int4 hd;  // id, tmin, tmax, nterm (padded to 4)
    int4 t[NTV / 2];  // two BpTermV per int4
    __device__ __forceinline__ void load(const int4* __restrict__ srcs4,
                                         const int4* __restrict__ terms, int k, int vzero)
    {
        // `vzero` is 0 held in a VGPR the compiler cannot see through: it keeps these loads on
        // the vector-memory path although their address is wave-uniform
        const size_t kk = (size_t)(k + vzero);
        hd = srcs4[kk];
#pragma unroll
        for (int i = 0; i < NTV / 2; ++i) t[i] = terms[kk * (NTV / 2) + i];
    }
};

// Inside a workgroup the four waves take DIFFERENT sources (k, k+1, k+2, k+3, then +4 ...) and
// each wave covers the whole time tile (TPW samples per lane, tile = 64 * TPW).  The wave-uniform
// metadata of a source is then fetched by one wave only, which divides the vector-memory return
// traffic of the metadata broadcast (the limiter of the earlier time-split layout: 13 x 1 KiB per
// source per wave) by four, and one address add serves TPW gathers.  Every wave keeps its own
// running (max, arg-max) for the tile; they are merged through LDS at the end with the same
// (value, lowest id) order.
template <int TPW, int NTV, int OOB, int REDUCE, bool BATCH = false>
__global__ __launch_bounds__(BP_THREADS) void bp_beam_wps_kernel(
    const float* __restrict__ U, long long N, const BpGroup* __restrict__ groups, int n_groups,
    const int4* __restrict__ chunks, const int4* __restrict__ srcs4,
    const int4* __restrict__ terms, int id_offset, float* __restrict__ out_beam,
    int* __restrict__ out_arg, long long tile_base, float best0, long long u_estride, long long out_estride)
{
    extern __shared__ float lds[];
    if constexpr (BATCH) bp_select_event(U, out_beam, out_arg, u_estride, out_estride);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    constexpr int NW = BP_THREADS / 64;
    constexpr int TILE = 64 * TPW;
    const long long t0 = (tile_base + (long long)blockIdx.x) * TILE;
    int vzero;
    asm volatile("v_mov_b32 %0, 0" : "=v"(vzero));
    // sample j of this lane inside the tile
    auto tmap = [&](int j) { return lane + 64 * j; };
    const char* lds_l = (const char*)lds + lane * 4;

    float best[TPW];
    int arg[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) { best[j] = best0; arg[j] = id_offset; }
    for (int x = tid; x < TILE; x += BP_THREADS) lds[x] = 0.0f;  // the zero slab

    for (int g = 0; g < n_groups; ++g) {
        const BpGroup grp = groups[g];
        const int k_last = grp.first_src + grp.n_src - 1;
        const int k_first = grp.first_src + wv;  // this wave's first source (may be > k_last)
        BpMetaV<NTV> m0, m1, m2;
        m0.load(srcs4, terms, min(k_first, k_last), vzero);
        m1.load(srcs4, terms, min(k_first + NW, k_last), vzero);
        __syncthreads();  // previous group's gathers are done
        for (int cb = 0; cb < grp.n_chunk; cb += 64) {
            const int nb = min(64, grp.n_chunk - cb);
            int4 d = make_int4(0, 0, 0, 0);
            if (lane < nb) d = chunks[grp.first_chunk + cb + lane];
            for (int c = 0; c < nb; c += 4) {
                int row[4], dd[4], n[4];
                long long gi[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int cc = min(c + u, nb - 1);
                    row[u] = lane_bcast(d.x, cc);
                    gi[u] = t0 + lane_bcast(d.y, cc) + tid;
                    dd[u] = lane_bcast(d.z, cc);
                    n[u] = c + u < nb ? lane_bcast(d.w, cc) : 0;
                }
                float v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const long long gc = gi[u] < 0 ? 0 : (gi[u] >= N ? N - 1 : gi[u]);
                    v[u] = U[(size_t)row[u] * (size_t)N + gc];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (tid < n[u]) lds[dd[u] + tid] = (gi[u] >= 0 && gi[u] < N) ? v[u] : 0.0f;
            }
        }
        __syncthreads();

        auto process = [&](const BpMetaV<NTV>& m, bool live) {
            const int nterm = live ? __builtin_amdgcn_readfirstlane(m.hd.w) : 0;
            float acc[TPW];
#pragma unroll
            for (int j = 0; j < TPW; ++j) acc[j] = 0.0f;
#pragma unroll
            for (int c = 0; c < NTV / 2; ++c) {
                if (c * 2 < nterm) {  // wave-uniform
                    const int4 tt = m.t[c];
                    const float* lp0 = (const float*)(lds_l + tt.x);
                    const float* lp1 = (const float*)(lds_l + tt.z);
                    float x0[TPW], x1[TPW];
#pragma unroll
                    for (int j = 0; j < TPW; ++j) { x0[j] = lp0[j * 64]; x1[j] = lp1[j * 64]; }
                    const float b0 = __int_as_float(tt.y), b1 = __int_as_float(tt.w);
#pragma unroll
                    for (int j = 0; j < TPW; ++j) acc[j] = __fmaf_rn(b0, x0[j], acc[j]);
#pragma unroll
                    for (int j = 0; j < TPW; ++j) acc[j] = __fmaf_rn(b1, x1[j], acc[j]);
                }
            }
            const int sid = m.hd.x;
#pragma unroll
            for (int j = 0; j < TPW; ++j) {
                const long long t = t0 + tmap(j);
                bool computed = nterm > 0;
                if (OOB == BPMF_BP_STRICT) computed = computed && (t + m.hd.y >= 0) && (t + m.hd.z < N);
                if (REDUCE == BPMF_BP_REDUCE_MAX) {
                    const bool better = acc[j] > best[j] || (acc[j] == best[j] && sid < arg[j]);
                    if (computed && better) { best[j] = acc[j]; arg[j] = sid; }
                } else {
                    if (live && t < N)
                        out_beam[(size_t)(sid - id_offset) * (size_t)N + t] = computed ? acc[j] : 0.0f;
                }
            }
        };
        for (int k = k_first; k <= k_last; k += 3 * NW) {
            m2.load(srcs4, terms, min(k + 2 * NW, k_last), vzero);
            process(m0, true);
            m0.load(srcs4, terms, min(k + 3 * NW, k_last), vzero);
            process(m1, k + NW <= k_last);
            m1.load(srcs4, terms, min(k + 4 * NW, k_last), vzero);
            process(m2, k + 2 * NW <= k_last);
        }
    }
    if (REDUCE == BPMF_BP_REDUCE_MAX) {
        // merge the four waves' running maxima through LDS (window area is free now)
        __syncthreads();
        float* mb = lds;                       // [NW][TILE]
        int* ma = (int*)(lds + NW * TILE);     // [NW][TILE]
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
            mb[wv * TILE + tmap(j)] = best[j];
            ma[wv * TILE + tmap(j)] = arg[j];
        }
        __syncthreads();
        for (int x = tid; x < TILE; x += BP_THREADS) {
            float b = mb[x];
            int a = ma[x];
#pragma unroll
            for (int w = 1; w < NW; ++w) {
                const float bw = mb[w * TILE + x];
                const int aw = ma[w * TILE + x];
                if (bw > b || (bw == b && aw < a)) { b = bw; a = aw; }
            }
            const long long t = t0 + x;
            if (t < N) { out_beam[t] = b; out_arg[t] = a; }
        }
    }
}

// ------------------------------------- beam, one wave per source, packed metadata (P = 2) ---
// The production kernel for two-phase (P, S) grids.  Same flow as bp_beam_wps_kernel, but a
// source's metadata is packed per STATION as {off_P | off_S << 16, weight} (LDS float offsets
// fit 16 bits; both phases share the station weight): half the registers and half the
// vector-memory traffic of the per-term table, two prefetched sets instead of three.
// WPB = waves per workgroup (all waves share the group's LDS windows and take different
// sources).  Measured on cfg3 with the metadata in VGPRs: WPB 4 (8 waves/CU) 0.342 s, more waves
// spill; with the metadata in SGPRs (BpMetaS, <= 80 VGPRs): WPB 4 0.280 s, WPB 8 (16 waves/CU)
// 0.241 s, WPB 12 (24 waves/CU) 0.236 s.
//
// The metadata of a source in scalar registers: ONE set of 4 + 2 NSV SGPRs (NSV <= 16), filled by
// inline-asm s_load_dwordx4/x8 for the NEXT source right after the last gather of the current
// one, so the scalar-cache latency hides behind the max/arg-max epilogue.  SMEM shares lgkmcnt
// with the LDS gathers and returns out of order, hence the placement: nothing else is in flight
// between the issue and the lgkmcnt(0) that closes the source.  Frees 2 x (4 + 2 NSV) VGPRs,
// which is what lets 16 waves/CU (128 VGPRs) run without spills.
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
template <int NSV>
struct BpMetaS {
    static constexpr int NS = NSV < 16 ? NSV : 16;  // stations held at a time; records have NSV slots
    i32x4 hd;
    i32x8 r[NS / 4];    // station s of the part: dword 2 s = offs, 2 s + 1 = weight
    __device__ __forceinline__ void issue(const int4* __restrict__ srcs4,
                                          const int4* __restrict__ recs, int k)
    {
        const int4* ph = srcs4 + k;
        const int4* pr = recs + (size_t)k * (NSV / 2);
        asm volatile("s_load_dwordx4 %0, %1, 0x0" : "=s"(hd) : "s"(ph));
#pragma unroll
        for (int i = 0; i < NS / 4; ++i) {
            const int4* pi = pr + 2 * i;
            asm volatile("s_load_dwordx8 %0, %1, 0x0" : "=s"(r[i]) : "s"(pi));
        }
    }
    // stations 16 part .. 16 part + 15 of source k (NSV > 16: a source is gathered in parts)
    __device__ __forceinline__ void issue_part(const int4* __restrict__ recs, int k, int part)
    {
        const int4* pr = recs + (size_t)k * (NSV / 2) + 8 * part;
#pragma unroll
        for (int i = 0; i < NS / 4; ++i) {
            const int4* pi = pr + 2 * i;
            asm volatile("s_load_dwordx8 %0, %1, 0x0" : "=s"(r[i]) : "s"(pi));
        }
    }
    // s_waitcnt lgkmcnt(0) with every register of the set as an INPUT: no part of the set is
    // dead (= free for the register allocator to hand out as a temporary) while the loads are
    // in flight.  Inputs only -- a "+s" tie makes the compiler copy the in-flight registers in
    // front of the wait.  The sched_barrier keeps later uses behind the wait.
    __device__ __forceinline__ void wait() const
    {
        static_assert(NSV % 4 == 0 && (NSV <= 16 || NSV % 16 == 0), "BpMetaS: NSV in {4, 8, 12, 16, 32, ...}");
        if constexpr (NS / 4 == 1)
            asm volatile("s_waitcnt lgkmcnt(0)" : : "s"(hd), "s"(r[0]) : "memory");
        else if constexpr (NS / 4 == 2)
            asm volatile("s_waitcnt lgkmcnt(0)" : : "s"(hd), "s"(r[0]), "s"(r[1]) : "memory");
        else if constexpr (NS / 4 == 3)
            asm volatile("s_waitcnt lgkmcnt(0)" : : "s"(hd), "s"(r[0]), "s"(r[1]), "s"(r[2]) : "memory");
        else
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : : "s"(hd), "s"(r[0]), "s"(r[1]), "s"(r[2]), "s"(r[3]) : "memory");
        __builtin_amdgcn_sched_barrier(0);
    }
    __device__ __forceinline__ unsigned offs(int s) const { return (unsigned)r[(2 * s) >> 3][(2 * s) & 7]; }
    // {offs, weight} as one aligned SGPR pair: v_pk_fma_f32 takes the weight from its high half
    __device__ __forceinline__ i32x2 pair(int s) const
    {
        i32x2 p;
        p[0] = r[(2 * s) >> 3][(2 * s) & 7];
        p[1] = r[(2 * s + 1) >> 3][(2 * s + 1) & 7];
        return p;
    }
    __device__ __forceinline__ int id() const { return hd[0]; }
    __device__ __forceinline__ int tmin() const { return hd[1]; }
    __device__ __forceinline__ int tmax() const { return hd[2]; }
    __device__ __forceinline__ int nsta() const { return hd[3]; }
};

// B64 (plans with dual windows, see build_plan): every LDS offset is even, a lane owns the
// sample PAIRS 128 j + 2 lane + {0, 1} and gathers them with ds_read_b64 -- 256 B/clk/CU instead of
// the 128 B/clk/CU of the 4-byte gathers.
template <int WPB, int NSV, int OOB, int REDUCE, bool B64 = false, bool BATCH = false>
__global__ __launch_bounds__(64 * WPB, WPB >= 16 ? WPB / 4 : (WPB * 2 + 3) / 4) void bp_beam_wps2_kernel(
    const float* __restrict__ U, long long N, const BpGroup* __restrict__ groups, int n_groups,
    const int4* __restrict__ chunks, const int4* __restrict__ srcs4,
    const int4* __restrict__ recs, int id_offset, float* __restrict__ out_beam,
    int* __restrict__ out_arg, long long tile_base, long long n_tiles, long long split_stride, float best0,
    long long u_estride, long long out_estride)
{
    extern __shared__ float lds[];
    // BATCH: the event's prestack now; its outputs are selected where they are written (two more pointers alive
    // through the source loop would crowd the scalar registers of the metadata set)
    if constexpr (BATCH) U += (size_t)blockIdx.z * (size_t)u_estride;
    constexpr int TPW = 8;
    constexpr int TILE = 64 * TPW;
    constexpr int NTHREADS = 64 * WPB;
    // Short series (an event relocation: 3-6 tiles) leave most of the 256 CUs without a tile: the
    // launch then carries gridDim.y > 1 and workgroup (tile, y) walks only the groups
    // [n_groups y / Y, n_groups (y + 1) / Y).  reduce="none": every source still belongs to exactly
    // one workgroup of a tile; reduce="max": partial maxima go to out + y * split_stride and
    // bp_merge_splits_kernel folds them (value, then lowest id -- the rule of the 16-wave merge below).
    const int g_lo = (int)((long long)n_groups * blockIdx.y / gridDim.y);
    const int g_hi = (int)((long long)n_groups * (blockIdx.y + 1) / gridDim.y);
    if (REDUCE == BPMF_BP_REDUCE_MAX) {
        out_beam += (size_t)blockIdx.y * (size_t)split_stride;
        out_arg += (size_t)blockIdx.y * (size_t)split_stride;
    }
    constexpr bool GLOCAL = B64 && REDUCE == BPMF_BP_REDUCE_MAX;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // Consecutive workgroup ids go round-robin to the 8 XCDs (one L2 each): give every XCD a
    // contiguous run of tiles, so that each L2 stages its own eighth of the prestack instead of
    // all of it.  (The grid is rounded up to a multiple of 8; tiles past N see only zero fill.)
    const long long tiles_per_xcd = (gridDim.x + 7) >> 3;
    const long long tile_i = (long long)(blockIdx.x & 7) * tiles_per_xcd + (blockIdx.x >> 3);
    if (tile_i >= n_tiles) return;          // the launch covers the tiles [tile_base, tile_base + n_tiles)
    const long long t0 = (tile_base + tile_i) * TILE;
    if (t0 >= N) return;
    int vzero;
    asm volatile("v_mov_b32 %0, 0" : "=v"(vzero));
    const char* lds_l = (const char*)lds + lane * (B64 ? 8 : 4);
    // tile sample held in accumulator slot j of this lane
    auto slot_x = [&](int j) { return B64 ? 128 * (j >> 1) + 2 * lane + (j & 1) : lane + 64 * j; };

    float best[TPW];
    int arg[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) { best[j] = best0; arg[j] = id_offset; }
    for (int x = tid; x < TILE; x += NTHREADS) lds[x] = 0.0f;  // the zero slab

    for (int g = g_lo; g < g_hi; ++g) {
        const BpGroup grp = groups[g];
        const int k_last = grp.first_src + grp.n_src - 1;
        const int k_first = grp.first_src + wv;
        using Meta = BpMetaS<NSV>;
        Meta meta;
        // GLOCAL: the plan lists a group's sources by ascending id, so inside a group a plain
        // strict > keeps the lowest id on ties; the full tie rule runs once per group.
        float bestg[GLOCAL ? TPW : 1];
        int argg[GLOCAL ? TPW : 1];
        if constexpr (GLOCAL) {
#pragma unroll
            for (int j = 0; j < TPW; ++j) { bestg[j] = -INFINITY; argg[j] = 0x7fffffff; }
        }
        __syncthreads();  // previous group's gathers are done
        // the first source's metadata travels while the windows are staged (the staging uses no
        // scalar registers of its own, so nothing tempts the compiler to spill this set in flight:
        // tools/check_inflight.py)
        if (k_first <= k_last) meta.issue(srcs4, recs, k_first);
        // Staging, one chunk per wave and 16 bytes per lane: a chunk is <= 256 consecutive floats
        // of one prestacked row (the plan cuts windows to multiples of 4 floats at 16-byte
        // aligned LDS offsets), so it is one unaligned global_load_dwordx4 + one ds_write_b128
        // per lane.  Each wave issues the loads of STG_R chunks before it writes any of them:
        // a group of ~240 chunks is two memory round trips for the 16 waves, where the former
        // 256-thread / 4-byte version paid fifteen (staging was 7 % of the kernel at cfg3 and a
        // quarter at 80 station-phase rows).  Chunks that reach outside [0, N) -- the first and
        // last tiles of a trace -- take a per-element path with zero fill.
        {
            constexpr int STG_R = WPB >= 16 ? 8 : 4;   // 12-wave workgroups run under an 80-VGPR cap
            typedef float f32x4u4 __attribute__((ext_vector_type(4), aligned(4)));
            typedef float f32x4v __attribute__((ext_vector_type(4)));
            const int nck = grp.n_chunk;
            for (int c0 = wv; c0 < nck; c0 += WPB * STG_R) {
                int4 dsc[STG_R];
                f32x4v v[STG_R];
#pragma unroll
                for (int r = 0; r < STG_R; ++r) {
                    const int c = c0 + r * WPB;
                    // wave-uniform, but fetched with a vector load (index through the opaque zero):
                    // eight descriptors in SGPRs on top of the metadata set make the compiler
                    // spill in-flight scalar loads (tools/check_inflight.py)
                    dsc[r] = chunks[grp.first_chunk + min(c, nck - 1) + vzero];
                    if (c >= nck) dsc[r].w = 0;
                }
#pragma unroll
                for (int r = 0; r < STG_R; ++r) {
                    const long long g0 = t0 + dsc[r].y;
                    const float* src = U + (size_t)dsc[r].x * (size_t)N;
                    v[r] = (f32x4v){0.0f, 0.0f, 0.0f, 0.0f};
                    if (4 * lane < dsc[r].w) {
                        if (g0 >= 0 && g0 + 256 <= N) {     // wave-uniform: whole chunk span inside
                            v[r] = *(const f32x4u4*)(src + g0 + 4 * lane);
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const long long gi = g0 + 4 * lane + e;
                                if (gi >= 0 && gi < N) v[r][e] = src[gi];
                            }
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < STG_R; ++r)
                    if (4 * lane < dsc[r].w) *(f32x4v*)(lds + dsc[r].z + 4 * lane) = v[r];
            }
        }
        if (k_first <= k_last) meta.wait();
        __syncthreads();

        // Gathers of one station (2 phases x 8 samples = 8 ds_read2st64_b32) are inline asm with
        // counted waits, software-pipelined one station ahead: while station s is accumulated the
        // 8 reads of station s+1 are already queued, so the LDS never drains between stations
        // (hipcc's own schedule is [16 reads][wait][16 fma] per pair of stations, which leaves the
        // LDS idle during the fma / issue phases of all 8 waves: 62 % busy).  LDS returns in
        // order: with 16 reads outstanding, lgkmcnt(8) = "station s has landed".
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        const unsigned lds_lu = (unsigned)(size_t)lds_l;
#define BP_RD2(dst, addr, o0, o1) \
    asm volatile("ds_read2st64_b32 %0, %1 offset0:" #o0 " offset1:" #o1 : "=v"(dst) : "v"(addr))
#define BP_PKFMA_S(acc2, sp2, x2)                                                      \
    asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]"        \
                 : "+v"(acc2) : "s"(sp2), "v"(x2))
#define BP_RD64(dst, addr, o) \
    asm volatile("ds_read_b64 %0, %1 offset:" #o : "=v"(dst) : "v"(addr))
        // One straight-line body per station count (no control flow between the asm reads and
        // their uses: with phis in between, the compiler copies the destination registers of
        // reads that are still in flight).
        // The fma chain is asm volatile as well: plain fmaf()s are pure and get sunk below the
        // later reads at IR level (every station then needs its own 16 destination VGPRs).
        // A unit = one phase of one station = 4 reads (8 samples per lane).  Three units are kept in
        // flight ahead of the one being accumulated (lgkmcnt counts to 15: 12 younger reads may
        // stay outstanding while the wait retires the oldest 4).
        auto gather = [&](auto nst_c, auto first_c, const Meta& m, float (&acc)[TPW]) {
            constexpr int NST = decltype(nst_c)::value;
            constexpr bool FIRST = decltype(first_c)::value;  // false: continue the sums of acc
            constexpr int NU = 2 * NST, AH = 3;
            f32x2 X[4][4];  // ring of 4 units
            f32x2 ac[4];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                ac[jj][0] = FIRST ? 0.0f : acc[2 * jj];
                ac[jj][1] = FIRST ? 0.0f : acc[2 * jj + 1];
            }
#define BP_ISSUE_U(u)                                                                          \
    {                                                                                          \
        const unsigned o_ = m.offs((u) >> 1);                                                  \
        const unsigned a_ = lds_lu + ((((u) & 1) ? (o_ >> 16) : (o_ & 0xffffu)) << 2);         \
        if constexpr (B64) {                                                                   \
            BP_RD64(X[(u) & 3][0], a_, 0); BP_RD64(X[(u) & 3][1], a_, 512);                    \
            BP_RD64(X[(u) & 3][2], a_, 1024); BP_RD64(X[(u) & 3][3], a_, 1536);                \
        } else {                                                                               \
            BP_RD2(X[(u) & 3][0], a_, 0, 1); BP_RD2(X[(u) & 3][1], a_, 2, 3);                  \
            BP_RD2(X[(u) & 3][2], a_, 4, 5); BP_RD2(X[(u) & 3][3], a_, 6, 7);                  \
        }                                                                                      \
    }
#pragma unroll
            for (int u = 0; u < AH; ++u) BP_ISSUE_U(u)
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const i32x2 sp = m.pair(u >> 1);
                if (u + AH < NU) BP_ISSUE_U(u + AH)
                const int left = NU - 1 - u < AH ? NU - 1 - u : AH;  // units that may stay in flight
                if (left == 3) asm volatile("s_waitcnt lgkmcnt(12)" ::: "memory");
                else if (left == 2) asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
                else if (left == 1) asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");
                else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)  // phase P then phase S of a station, as the oracle
                    BP_PKFMA_S(ac[jj], sp, X[u & 3][jj]);
            }
#undef BP_ISSUE_U
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) { acc[2 * jj] = ac[jj][0]; acc[2 * jj + 1] = ac[jj][1]; }
        };
        // k_next: refill m with that source once its own gathers are done
        constexpr int NS = Meta::NS;  // stations per gather() call
        auto process = [&](Meta& m, int k_cur, int k_next) {
            const int nsta = __builtin_amdgcn_readfirstlane(m.nsta());
            const int sid = m.id(), tmin = m.tmin(), tmax = m.tmax();
            float acc[TPW];
#pragma unroll
            for (int j = 0; j < TPW; ++j) acc[j] = 0.0f;
#define BP_CASE(n) \
    case n: if constexpr (2 * n <= NS) gather(std::integral_constant<int, 2 * n>{}, first_c, m, acc); break;
#define BP_SWITCH(npairs)                                                                              \
    switch (npairs) { /* wave-uniform; station records come in pairs */                               \
        BP_CASE(1) BP_CASE(2) BP_CASE(3) BP_CASE(4) BP_CASE(5) BP_CASE(6) BP_CASE(7) BP_CASE(8)        \
        BP_CASE(9) BP_CASE(10) BP_CASE(11) BP_CASE(12) BP_CASE(13) BP_CASE(14) BP_CASE(15) BP_CASE(16) \
        default: break;                                                                                \
    }
            {
                constexpr std::true_type first_c{};
                BP_SWITCH((nsta < NS ? nsta : NS) >> 1)
            }
            if constexpr (NSV > NS) {  // more than 16 stations: refill the set, keep summing
                constexpr std::false_type first_c{};
                for (int part = 1; part * NS < nsta; ++part) {
                    m.issue_part(recs, k_cur, part);
                    m.wait();
                    const int rest = nsta - part * NS;
                    BP_SWITCH((rest < NS ? rest : NS) >> 1)
                }
            }
#undef BP_SWITCH
#undef BP_CASE
            m.issue(srcs4, recs, k_next);
            // strict bounds as a wave-uniform window [lo, hi) of the tile: 0 <= t + tmin and
            // t + tmax < N with t = t0 + x
            int lo = 0, hi = TILE;
            if (OOB == BPMF_BP_STRICT) {
                const long long lo64 = -(t0 + tmin), hi64 = N - t0 - tmax;
                lo = (int)(lo64 < 0 ? 0 : (lo64 > TILE ? TILE : lo64));
                hi = (int)(hi64 < 0 ? 0 : (hi64 > TILE ? TILE : hi64));
            }
            if (nsta <= 0) hi = 0;
            if (GLOCAL && lo == 0 && hi == TILE) {  // whole tile inside the bounds (wave-uniform)
#pragma unroll
                for (int j = 0; j < TPW; ++j) {
                    const bool take = acc[j] > bestg[j];
                    bestg[j] = take ? acc[j] : bestg[j];
                    argg[j] = take ? sid : argg[j];
                }
            } else {
#pragma unroll
                for (int j = 0; j < TPW; ++j) {
                    const int x = slot_x(j);
                    // bitwise, not short-circuit: keeps the epilogue free of branches
                    const bool computed = (x >= lo) & (x < hi);
                    if (GLOCAL) {
                        const bool take = computed & (acc[j] > bestg[j]);
                        bestg[j] = take ? acc[j] : bestg[j];
                        argg[j] = take ? sid : argg[j];
                    } else if (REDUCE == BPMF_BP_REDUCE_MAX) {
                        const bool take =
                            computed & ((acc[j] > best[j]) | ((acc[j] == best[j]) & (sid < arg[j])));
                        best[j] = take ? acc[j] : best[j];
                        arg[j] = take ? sid : arg[j];
                    } else {
                        const long long t = t0 + x;
                        if (t < N)
                            out_beam[(size_t)(sid - id_offset) * (size_t)N + t] = computed ? acc[j] : 0.0f;
                    }
                }
            }
            m.wait();
        };
        for (int k = k_first; k <= k_last; k += WPB) process(meta, k, min(k + WPB, k_last));
        if constexpr (GLOCAL) {
#pragma unroll
            for (int j = 0; j < TPW; ++j) {
                const bool take = (bestg[j] > best[j]) | ((bestg[j] == best[j]) & (argg[j] < arg[j]));
                best[j] = take ? bestg[j] : best[j];
                arg[j] = take ? argg[j] : arg[j];
            }
        }
#undef BP_RD2
#undef BP_PKFMA_S
#undef BP_RD64
    }
    if (REDUCE == BPMF_BP_REDUCE_MAX) {
        __syncthreads();
        float* mb = lds;                        // [WPB][TILE]
        int* ma = (int*)(lds + WPB * TILE);     // [WPB][TILE]
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
            mb[wv * TILE + slot_x(j)] = best[j];
            ma[wv * TILE + slot_x(j)] = arg[j];
        }
        __syncthreads();
        for (int x = tid; x < TILE; x += NTHREADS) {
            float b = mb[x];
            int a = ma[x];
#pragma unroll
            for (int w = 1; w < WPB; ++w) {
                const float bw = mb[w * TILE + x];
                const int aw = ma[w * TILE + x];
                if (bw > b || (bw == b && aw < a)) { b = bw; a = aw; }
            }
            const long long t = t0 + x;
            const size_t eo = BATCH ? (size_t)blockIdx.z * (size_t)out_estride : 0;
            if (t < N) { out_beam[eo + t] = b; out_arg[eo + t] = a; }
        }
    }
}

// ------------------------------------------------- multi-GPU max exchange keys ---
__device__ __forceinline__ unsigned f32_to_ordered(float f)
{
    unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_to_f32(unsigned k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// reduce="max" of a short series computed in `n_split` group ranges per tile: fold the partial
// (beam, arg) rows -- larger beam wins, lowest source id on equal beams, the rule of every other merge
// Interior samples [lo_s, hi_s) hold `rows` partial rows (station-count classes x group ranges), the
// edge samples around them -- computed by the general kernel over all sources -- `rows_edge`.
// blockIdx.y: the event of a batch of series, its partial rows `pstride` elements behind the previous event's.
__global__ void bp_merge_splits_kernel(const float* __restrict__ pbeam, const int* __restrict__ parg,
                                       int rows, int rows_edge, long long lo_s, long long hi_s,
                                       size_t N, float* __restrict__ beam, int* __restrict__ arg, size_t pstride)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    pbeam += (size_t)blockIdx.y * pstride;
    parg += (size_t)blockIdx.y * pstride;
    beam += (size_t)blockIdx.y * N;
    arg += (size_t)blockIdx.y * N;
    const int n_split = ((long long)i >= lo_s && (long long)i < hi_s) ? rows : rows_edge;
    float b = pbeam[i];
    int a = parg[i];
    for (int y = 1; y < n_split; ++y) {
        const float bw = pbeam[(size_t)y * N + i];
        const int aw = parg[(size_t)y * N + i];
        if (bw > b || (bw == b && aw < a)) { b = bw; a = aw; }
    }
    beam[i] = b;
    arg[i] = a;
}

// option bp.compat_first_computed: samples on which no beam was computed still hold the start value
__global__ void bp_finish_first_computed_kernel(float* __restrict__ beam, int* __restrict__ arg, size_t N,
                                                int id_offset)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    if (beam[i] == -INFINITY) { beam[i] = 0.0f; arg[i] = id_offset; }
}

__global__ void bp_pack_kernel(const float* __restrict__ beam, const int* __restrict__ arg, size_t N,
                               unsigned long long flip, unsigned long long* __restrict__ packed)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    unsigned long long key = ((unsigned long long)f32_to_ordered(beam[i]) << 32) |
                             (unsigned long long)(0xffffffffu - (unsigned)arg[i]);
    packed[i] = key ^ flip;
}

__global__ void bp_unpack_kernel(const unsigned long long* __restrict__ packed, size_t N,
                                 unsigned long long flip, float* __restrict__ beam,
                                 int* __restrict__ arg)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    unsigned long long key = packed[i] ^ flip;
    beam[i] = ordered_to_f32((unsigned)(key >> 32));
    arg[i] = (int)(0xffffffffu - (unsigned)(key & 0xffffffffu));
}

}  // namespace bpmf

using namespace bpmf;

// ---------------------------------------------------------------- plan upload ---
namespace {

// The tables of a plan travel through ONE pinned scratch buffer of the process (grow-only, under a mutex), not
// straight from the std::vectors that hold them: a pageable source makes the runtime page-lock the vector's pages for
// the copy, the vector is freed when the plan is built, and the NEXT host-pointer call of the process found its
// first piece of the day stalled for 20-40 ms (tools/probe_bp_e2e.py, profiles/r06_bp_e2e.txt: always the call
// behind the one that built a plan, never later ones).
struct PlanScratch {
    std::mutex m;
    char* p = nullptr;
    size_t cap = 0;
};
PlanScratch& plan_scratch()
{
    static PlanScratch* s = new PlanScratch();      // (leaked: pinned memory must not be freed from a static destructor)
    return *s;
}

template <typename Tv>
int upload(const std::vector<Tv>& v, Tv** d)
{
    size_t b = std::max<size_t>(v.size(), 1) * sizeof(Tv);
    BPMF_HIP_CHECK(hipMalloc((void**)d, b));
    if (v.empty()) return 0;
    const size_t bytes = v.size() * sizeof(Tv);
    PlanScratch& sc = plan_scratch();
    std::lock_guard<std::mutex> g(sc.m);
    if (sc.cap < bytes) {
        if (sc.p) (void)hipHostFree(sc.p);
        sc.p = nullptr;
        sc.cap = 0;
        const size_t want = align_up(std::max<size_t>(bytes + bytes / 4, (size_t)4 << 20), (size_t)1 << 20);
        if (hipHostMalloc((void**)&sc.p, want, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            sc.p = nullptr;
            // (no pinned memory to be had: the runtime's own pageable path)
            BPMF_HIP_CHECK(hipMemcpy(*d, v.data(), bytes, hipMemcpyHostToDevice));
            return 0;
        }
        sc.cap = want;
    }
    memcpy(sc.p, v.data(), bytes);
    BPMF_HIP_CHECK(hipMemcpy(*d, sc.p, bytes, hipMemcpyHostToDevice));
    return 0;
}

void free_fast_class(BpFastClass& fc)
{
    (void)hipFree(fc.d_groups);
    (void)hipFree(fc.d_runs);
    (void)hipFree(fc.d_wins);
    (void)hipFree(fc.d_recs);
    fc = BpFastClass();
}

// The device side of a plan: binds the device, copies the host tables as they are, takes the device's side
// stream and creates the fork / join events.
int bp_plan_upload(const BpPlanHost& h, int device, bpmf_bp_plan** plan_out)
{
    BPMF_BIND_DEVICE(device);
    bpmf_bp_plan* pl = new bpmf_bp_plan();
    pl->device = device;
    pl->shape = h.shape;
    const BpPlanShape& sh = h.shape;
    auto tables = [&]() -> int {
        int rc = 0;
        if (sh.direct) {
            (void)((rc = upload(h.dhdr, &pl->d_dhdr)) || (rc = upload(h.dfirst, &pl->d_dfirst)) ||
                   (rc = upload(h.dterms, &pl->d_dterms)));
            return rc;
        }
        if (sh.nsv && ((rc = upload(h.recs, &pl->d_recs)) || (rc = upload(h.hdr2, &pl->d_hdr2)))) return rc;
        if (sh.ntv && (rc = upload(h.termsv, &pl->d_termsv))) return rc;
        if (sh.fast) {
            // interior-tile classes
            for (int c = 0; c < sh.n_classes; ++c) {
                const FastHost& fh = h.classes[c].fh;
                const BpClassShape& cs = sh.cls[c];
                BpFastClass& fc = pl->cls[c];
                fc.tile = cs.tile;
                fc.halves = cs.halves;
                fc.n_pass = cs.n_pass;
                fc.uniform = fh.uniform;
                fc.rec_dw = fh.rec_dw;
                fc.n_groups = cs.n_groups;
                fc.lds_bytes = cs.lds_bytes;
                fc.n_sources = cs.n_sources;
                fc.max_stations = cs.max_stations;
                fc.desc_waves = (int)std::min<size_t>(BPF_DESC_MAX, (2 * sh.S * sh.P + 63) / 64 * 64) / 64;
                if ((rc = upload(fh.fg, &fc.d_groups)) || (rc = upload(fh.fr, &fc.d_runs)) ||
                    (rc = upload(fh.fw, &fc.d_wins)) || (rc = upload(fh.rec, &fc.d_recs)))
                    return rc;
            }
            // the side stream is the device's (context.h: created once per device, never destroyed);
            // the fork / join events are the plan's own
            pl->side_stream = device_side_stream(device);
            if (!pl->side_stream) return -2;
            hipError_t e2 = hipEventCreateWithFlags(&pl->ev_fork, hipEventDisableTiming);
            hipError_t e3 = hipEventCreateWithFlags(&pl->ev_join, hipEventDisableTiming);
            if (e2 != hipSuccess || e3 != hipSuccess) {
                set_error("bpmf_bp_plan_create: fork / join events: %s",
                          hipGetErrorString(e2 != hipSuccess ? e2 : e3));
                return -2;
            }
        }
        const PlanHost& ph = h.general();
        (void)((rc = upload(ph.groups, &pl->d_groups)) || (rc = upload(ph.chunks, &pl->d_chunks)) ||
               (rc = upload(ph.srcs, &pl->d_srcs)) || (rc = upload(ph.off, &pl->d_off)) ||
               (rc = upload(ph.beta, &pl->d_beta)));
        return rc;
    };
    if (const int rc = tables()) {
        bpmf_bp_plan_destroy(pl);
        return rc;
    }
    *plan_out = pl;
    return 0;
}

}  // namespace

extern "C" int bpmf_bp_plan_create(const int32_t* moveouts, const float* w_sources, size_t K,
                                   size_t S, size_t P, int device, int32_t source_id_offset,
                                   bpmf_bp_plan** plan_out)
{
    const char* why = plan_out ? bp_plan_refusal(moveouts, w_sources, K, S, P) : "bad argument";
    if (why) {
        set_error("bpmf_bp_plan_create: %s", why);
        return -1;
    }
    // decided on the host (bp_plan.hip), then copied to the device as it is
    return bp_plan_upload(bp_plan_host(moveouts, w_sources, K, S, P, source_id_offset), device, plan_out);
}

extern "C" void bpmf_bp_plan_destroy(bpmf_bp_plan* pl)
{
    if (!pl) return;
    (void)hipFree(pl->d_dhdr);
    (void)hipFree(pl->d_dfirst);
    (void)hipFree(pl->d_dterms);
    (void)hipFree(pl->d_groups);
    (void)hipFree(pl->d_chunks);
    (void)hipFree(pl->d_srcs);
    (void)hipFree(pl->d_off);
    (void)hipFree(pl->d_beta);
    (void)hipFree(pl->d_termsv);
    (void)hipFree(pl->d_recs);
    (void)hipFree(pl->d_hdr2);
    if (pl->ev_fork) (void)hipEventDestroy(pl->ev_fork);
    if (pl->ev_join) (void)hipEventDestroy(pl->ev_join);
    for (int c = 0; c < BPF_MAX_CLASSES; ++c) free_fast_class(pl->cls[c]);
    delete pl;
}

// workspace of one call: the prestacked traces + the partial maxima (bp_schedule: sized for either `reduce`)
extern "C" size_t bpmf_bp_workspace_bytes(const bpmf_bp_plan* pl, size_t N, size_t C)
{
    (void)C;
    if (!pl) return 0;
    return bp_schedule(pl->shape, N, BPMF_BP_REDUCE_MAX, (int)option(OPT_BP_SPLIT), 0).total;
}

namespace {

// Launch values of the general kernels.  The caller (interior / edge split of bp_run_dev) may restrict a
// launch to the samples [samp_lo, samp_hi) -- multiples of 1024, i.e. whole tiles of every kernel -- and
// then places the profile marks itself; samp_hi < 0: the whole series.
struct BpLaunch {
    long long samp_lo = 0, samp_hi = -1;
    int n_split = 1;                 // group ranges per tile (short series, see bp_split_count)
    long long split_stride = 0;      // elements between the partial outputs of reduce="max"
    // start value of the running maximum: 0 (the build's convention: a beam that is not > 0 never
    // becomes the maximum) or -inf (option bp.compat_first_computed: the maximum over the computed
    // beams whatever their sign; samples without any computed beam are set to (0, first id) at the end)
    float best0 = 0.0f;
    // a batch of series (bp_select_event): events, floats between their prestacks, elements between their outputs
    int n_events = 1;
    long long u_estride = 0, out_estride = 0;
};

// tiles [base, base + count) of a kernel with `tile` samples per workgroup
void tile_range(size_t N, size_t tile, const BpLaunch& lc, long long& base, long long& count)
{
    base = 0;
    count = (long long)((N + tile - 1) / tile);
    if (lc.samp_hi >= 0) {
        const long long hi = std::min<long long>(lc.samp_hi, (long long)N);
        base = lc.samp_lo / (long long)tile;
        count = hi > lc.samp_lo ? (hi + (long long)tile - 1) / (long long)tile - base : 0;
    }
}

// What every launch of a general kernel does around the kernel itself: more than 64 KB of dynamic LDS
// where needed, the tiles of lc's samples, profile marks around a whole-series launch, the launch check.
// enqueue(tile_base, n_tiles) launches the kernel.
template <typename Kernel, typename Enqueue>
int launch_general(Kernel kern, size_t lds, size_t tile, size_t N, const BpLaunch& lc, hipStream_t stream,
                   Enqueue enqueue)
{
    if (lds > 64 * 1024)
        BPMF_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)BP_LDS_MAX));
    long long tile_base, n_tiles;
    tile_range(N, tile, lc, tile_base, n_tiles);
    if (n_tiles <= 0) return 0;
    if (lc.samp_hi < 0) profile_mark(BPMF_KERNEL_BP_BEAM, 0, stream);
    enqueue(tile_base, n_tiles);
    BPMF_LAUNCH_CHECK();
    if (lc.samp_hi < 0) profile_mark(BPMF_KERNEL_BP_BEAM, 1, stream);
    return 0;
}

template <int V>
using IntC = std::integral_constant<int, V>;

// f(oob, reduce) with both codes as IntC: the one place where they become template arguments
template <typename F>
int with_oob_reduce(int oob, int reduce, F f)
{
    if (reduce == BPMF_BP_REDUCE_MAX)
        return oob == BPMF_BP_STRICT ? f(IntC<BPMF_BP_STRICT>{}, IntC<BPMF_BP_REDUCE_MAX>{})
                                     : f(IntC<BPMF_BP_FLEXIBLE>{}, IntC<BPMF_BP_REDUCE_MAX>{});
    return oob == BPMF_BP_STRICT ? f(IntC<BPMF_BP_STRICT>{}, IntC<BPMF_BP_REDUCE_NONE>{})
                                 : f(IntC<BPMF_BP_FLEXIBLE>{}, IntC<BPMF_BP_REDUCE_NONE>{});
}

// The general kernel `k` of a plan (bp_general_kernel: the schedule's choice) over lc's samples.
int dispatch_beam(const bpmf_bp_plan* pl, const BpKernel& k, const float* U, size_t N, int oob, int reduce,
                  const BpLaunch& lc, hipStream_t stream, float* beam, int32_t* arg)
{
    const BpPlanShape& sh = pl->shape;
    return with_oob_reduce(oob, reduce, [&](auto oob_c, auto reduce_c) -> int {
        constexpr int OOB = decltype(oob_c)::value, REDUCE = decltype(reduce_c)::value;
        // a batch of series (lc.n_events > 1, reduce="max") runs the BATCH instantiation of the same kernel
        auto batched = [&](auto launch) -> int {
            if constexpr (REDUCE == BPMF_BP_REDUCE_MAX)
                if (lc.n_events > 1) return launch(std::true_type{});
            return launch(std::false_type{});
        };
        auto wps2 = [&](auto wpb_c, auto nsv_c, auto b64_c) -> int { return batched([&](auto batch_c) -> int {
            constexpr int WPB = decltype(wpb_c)::value;
            auto kern = bp_beam_wps2_kernel<WPB, decltype(nsv_c)::value, OOB, REDUCE, decltype(b64_c)::value,
                                            decltype(batch_c)::value>;
            return launch_general(kern, k.lds_bytes, k.tile, N, lc, stream, [&](long long tile_base, long long n_tiles) {
                // x: a multiple of 8 (XCD-aware tile order), y: group ranges
                kern<<<dim3((unsigned)((n_tiles + 7) / 8 * 8), (unsigned)lc.n_split, (unsigned)lc.n_events), dim3(64 * WPB),
                       k.lds_bytes, stream>>>(
                    U, (long long)N, pl->d_groups, sh.n_groups, (const int4*)pl->d_chunks, pl->d_hdr2, pl->d_recs,
                    sh.id_offset, beam, arg, tile_base, n_tiles, lc.split_stride, lc.best0, lc.u_estride, lc.out_estride);
            });
        }); };
        auto wps = [&](auto ntv_c) -> int { return batched([&](auto batch_c) -> int {
            auto kern = bp_beam_wps_kernel<8, decltype(ntv_c)::value, OOB, REDUCE, decltype(batch_c)::value>;
            return launch_general(kern, k.lds_bytes, k.tile, N, lc, stream, [&](long long tile_base, long long n_tiles) {
                kern<<<dim3((unsigned)n_tiles, 1, (unsigned)lc.n_events), dim3(BP_THREADS), k.lds_bytes, stream>>>(
                    U, (long long)N, pl->d_groups, sh.n_groups, (const int4*)pl->d_chunks, (const int4*)pl->d_srcs,
                    (const int4*)pl->d_termsv, sh.id_offset, beam, arg, tile_base, lc.best0, lc.u_estride, lc.out_estride);
            });
        }); };
        auto readlane = [&](auto tpt_c, auto nblk_c) -> int { return batched([&](auto batch_c) -> int {
            auto kern = bp_beam_kernel<decltype(tpt_c)::value, 4, decltype(nblk_c)::value, OOB, REDUCE, decltype(batch_c)::value>;
            return launch_general(kern, k.lds_bytes, k.tile, N, lc, stream, [&](long long tile_base, long long n_tiles) {
                kern<<<dim3((unsigned)n_tiles, 1, (unsigned)lc.n_events), dim3(BP_THREADS), k.lds_bytes, stream>>>(
                    U, (long long)N, pl->d_groups, sh.n_groups, (const int4*)pl->d_chunks, (const int*)pl->d_srcs,
                    pl->d_off, pl->d_beta, sh.NT, sh.id_offset, beam, arg, tile_base, lc.best0, lc.u_estride,
                    lc.out_estride);
            });
        }); };
        // <= 16 stations: 16 waves with 8-byte gathers or 12 with 4-byte gathers
        auto wps2_upto16 = [&](auto nsv_c) -> int {
            if (k.wpb == 16 && k.b64) return wps2(IntC<16>{}, nsv_c, std::true_type{});
            if (k.wpb == 12 && !k.b64) return wps2(IntC<12>{}, nsv_c, std::false_type{});
            return -1;
        };
        int rc = -1;            // (stays -1: a kernel that is not compiled)
        if (k.family == BP_FAMILY_WPS2) {
            switch (k.nsv) {
                case 4: rc = wps2_upto16(IntC<4>{}); break;
                case 8: rc = wps2_upto16(IntC<8>{}); break;
                case 12: rc = wps2_upto16(IntC<12>{}); break;
                case 16: rc = wps2_upto16(IntC<16>{}); break;
                case 32: if (k.wpb == 16 && !k.b64) rc = wps2(IntC<16>{}, IntC<32>{}, std::false_type{}); break;
                default: break;
            }
        } else if (k.family == BP_FAMILY_WPS) {
            switch (k.ntv) {
                case 8: rc = wps(IntC<8>{}); break;
                case 16: rc = wps(IntC<16>{}); break;
                case 24: rc = wps(IntC<24>{}); break;
                case 32: rc = wps(IntC<32>{}); break;
                default: break;
            }
        } else if (k.family == BP_FAMILY_READLANE && (k.tpt == 1 || k.tpt == 2)) {
            const bool t1 = k.tpt == 1;
            switch (k.nblk) {
                case 1: rc = t1 ? readlane(IntC<1>{}, IntC<1>{}) : readlane(IntC<2>{}, IntC<1>{}); break;
                case 2: rc = t1 ? readlane(IntC<1>{}, IntC<2>{}) : readlane(IntC<2>{}, IntC<2>{}); break;
                case 4: rc = t1 ? readlane(IntC<1>{}, IntC<4>{}) : readlane(IntC<2>{}, IntC<4>{}); break;
                default: break;
            }
        }
        return rc;
    });
}

// prestack of the samples [t_lo, t_hi)
int launch_prestack(const float* d_features, const float* d_w_phases, size_t N, size_t C, int S, int P, float* U,
                    long long t_lo, long long t_hi, hipStream_t stream)
{
    if (t_hi <= t_lo) return 0;
    const unsigned nb = (unsigned)((t_hi - t_lo + 255) / 256);
    if (P <= 4) {
        bp_prestack_kernel<4><<<dim3(nb, (unsigned)S), dim3(256), 0, stream>>>(d_features, d_w_phases, (long long)N,
                                                                               (int)C, P, U, t_lo, t_hi);
    } else {
        bp_prestack_any_kernel<<<dim3(nb, (unsigned)(S * P)), dim3(256), 0, stream>>>(d_features, d_w_phases, (long long)N,
                                                                                     (int)C, P, U, t_lo, t_hi);
    }
    BPMF_LAUNCH_CHECK();
    return 0;
}

// The day of features of a host-pointer call, arriving in pieces (bpmf_bp_run below): need(samp_end, stream)
// returns once the work enqueued on `stream` behind it may read features and prestack of the samples
// [0, samp_end) -- it uploads the missing pieces on the copy stream (the host thread is inside the runtime's
// pageable-memory staging meanwhile; the device computes what was enqueued before) and enqueues their
// prestack on `stream` behind the piece's event.
struct BpFeed {
    virtual int need(long long samp_end, hipStream_t stream) = 0;
    virtual ~BpFeed() {}
};

// What every reduce="max" launch sequence does around its beam kernels: the kernels write `sch.rows` partial
// (beam, arg) rows per series behind the prestack -- or, with one row, straight into the outputs --, one merge
// launch folds them (interior samples [lo_s, hi_s) hold all the rows, the samples around them those of the edge
// kernel; `n_series` series with their sets of rows one behind the other), then `finish(beam, arg)`.
// launch(pbeam, parg, merge) enqueues the kernels.
template <typename Launch, typename Finish>
int with_partial_rows(const BpSchedule& sch, void* d_workspace, size_t N, size_t n_series, float* beam, int32_t* arg,
                      hipStream_t stream, Launch launch, Finish finish)
{
    const bool merge = sch.rows > 1;
    float* pbeam = merge ? (float*)((char*)d_workspace + sch.o_pbeam) : beam;
    int32_t* parg = merge ? (int32_t*)((char*)d_workspace + sch.o_parg) : arg;
    if (int rc = launch(pbeam, parg, merge)) return rc;
    if (merge) {
        bp_merge_splits_kernel<<<dim3((unsigned)((N + 255) / 256), (unsigned)n_series), dim3(256), 0, stream>>>(
            pbeam, parg, sch.rows, sch.n_split_edge, sch.lo_s, sch.hi_s, N, beam, arg, (size_t)sch.rows * N);
        BPMF_LAUNCH_CHECK();
    }
    return finish(beam, arg);
}

// bpmf_bp_run_dev, and a host-pointer call's run on the device: `feed` (not null: the day of features is still
// arriving, see BpFeed) and `defer_finish` (option bp.compat_first_computed: samples without any computed beam
// keep -inf; bpmf_bp_run_multi finishes them after the merge of all devices' shares)
int bp_run_dev(const bpmf_bp_plan* pl, const float* d_features, const float* d_w_phases, size_t N, size_t C,
               int out_of_bounds, int reduce, void* d_workspace, size_t workspace_bytes, hipStream_t stream,
               float* d_beam_out, int32_t* d_arg_out, BpFeed* feed, bool defer_finish)
{
    if (!pl || !d_features || !d_w_phases || !d_workspace || !d_beam_out || N == 0 || C == 0) {
        set_error("bpmf_bp_run_dev: bad argument");
        return -1;
    }
    if ((out_of_bounds != BPMF_BP_STRICT && out_of_bounds != BPMF_BP_FLEXIBLE) ||
        (reduce != BPMF_BP_REDUCE_MAX && reduce != BPMF_BP_REDUCE_NONE)) {
        set_error("bpmf_bp_run_dev: unknown out_of_bounds/reduce code");
        return -1;
    }
    if (reduce == BPMF_BP_REDUCE_MAX && !d_arg_out) {
        set_error("bpmf_bp_run_dev: reduce=max needs an arg-max output");
        return -1;
    }
    if (N > 0x7fffffffull) {
        set_error("bpmf_bp_run_dev: N exceeds the int32 index range");
        return -1;
    }
    const BpPlanShape& sh = pl->shape;
    // option bp.split is read ONCE: the size check and every launch below follow this schedule
    const BpSchedule sch = bp_schedule(sh, N, reduce, (int)option(OPT_BP_SPLIT), 0);
    if (workspace_bytes < sch.total) {
        set_error("bpmf_bp_run_dev: workspace too small (%zu < %zu)", workspace_bytes, sch.total);
        return -1;
    }
    // option debug.poison_output (tests): a sample that no kernel writes comes back as NaN / -1 instead of
    // whatever the caller's buffer held
    if (reduce == BPMF_BP_REDUCE_MAX && option(OPT_DEBUG_POISON_OUTPUT) != 0) {
        BPMF_HIP_CHECK(hipMemsetAsync(d_beam_out, 0xFF, N * sizeof(float), stream));
        BPMF_HIP_CHECK(hipMemsetAsync(d_arg_out, 0xFF, N * sizeof(int32_t), stream));
    }
    float* U = (float*)((char*)d_workspace + sch.o_prestack);
    const int P = (int)sh.P, S = (int)sh.S;
    // A host-pointer call may stream its day of features in while the kernels run (BpFeed, bpmf_bp_run):
    // the feed uploads AND prestacks piece by piece; only the interior-tile path below consumes it in
    // pieces, every other path asks for the whole series first.
    // option bp.host_piece_samples: samples of the first piece (default 131 072 = one round of the chip at tile
    // 512; the tests shrink it), 0 = the whole day in front of the first kernel
    const long long piece0 = (long long)align_up((size_t)option(OPT_BP_HOST_PIECE_SAMPLES), 1024);
    const bool feed_pieces = feed && sch.path == BP_PATH_INTERIOR && piece0 > 0;
    if (feed && !feed_pieces)
        if (int rc = feed->need((long long)N, stream)) return rc;
    if (!feed)
        if (int rc = launch_prestack(d_features, d_w_phases, N, C, S, P, U, 0, (long long)N, stream)) return rc;
    const bool first_computed = reduce == BPMF_BP_REDUCE_MAX && option(OPT_BP_COMPAT_FIRST_COMPUTED) != 0;
    const float best0 = first_computed ? -INFINITY : 0.0f;      // (BpLaunch::best0)
    auto finish = [&](float* beam, int32_t* arg) -> int {
        if (first_computed && !defer_finish) {
            bp_finish_first_computed_kernel<<<dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream>>>(
                beam, arg, N, sh.id_offset);
            BPMF_LAUNCH_CHECK();
        }
        return 0;
    };
    if (sch.path == BP_PATH_DIRECT) {
        // no LDS plan: global-memory gathers, ranges of sources per tile
        profile_mark(BPMF_KERNEL_BP_BEAM, 0, stream);
        const int rc = with_partial_rows(sch, d_workspace, N, 1, d_beam_out, d_arg_out, stream,
                                         [&](float* pbeam, int32_t* parg, bool) -> int {
            return launch_beam_direct(pl, U, N, out_of_bounds, reduce, stream, pbeam, parg, sch.n_split, (long long)N, best0);
        }, finish);
        profile_mark(BPMF_KERNEL_BP_BEAM, 1, stream);
        return rc;
    }
    if (sch.path == BP_PATH_GENERAL)    // the general kernels over the whole series
        return with_partial_rows(sch, d_workspace, N, 1, d_beam_out, d_arg_out, stream,
                                 [&](float* pbeam, int32_t* parg, bool merge) -> int {
            return dispatch_beam(pl, sch.kernel, U, N, out_of_bounds, reduce,
                                 BpLaunch{0, -1, sch.n_split, merge ? (long long)N : 0, best0}, stream, pbeam, parg);
        }, finish);
    // The interior samples [lo_s, hi_s) run the class kernels of bp_fast.hip, the tiles at the ends of the day the
    // general kernel over all sources (bp_schedule)
    const int n_split = sch.n_split;
    const long long lo_s = sch.lo_s, hi_s = sch.hi_s;
    std::lock_guard<std::mutex> enqueue_lock(pl->enqueue_mutex);
    profile_mark(BPMF_KERNEL_BP_BEAM, 0, stream);
    const int rc_all = with_partial_rows(sch, d_workspace, N, 1, d_beam_out, d_arg_out, stream,
                                         [&](float* pbeam, int32_t* parg, bool merge) -> int {
        int rc = 0;
        const bool have_edge = lo_s > 0 || hi_s < (long long)N;
        hipStream_t es = stream;          // edge tiles: on the side stream, beside the interior kernels
        if (have_edge && pl->side_stream && !feed_pieces) {
            BPMF_HIP_CHECK(hipEventRecord(pl->ev_fork, stream));
            BPMF_HIP_CHECK(hipStreamWaitEvent(pl->side_stream, pl->ev_fork, 0));
            es = pl->side_stream;
        }
        auto edge = [&](long long from, long long to) {
            if (to > from && !rc)
                rc = dispatch_beam(pl, sch.kernel, U, N, out_of_bounds, reduce,
                                   BpLaunch{from, to, sch.n_split_edge, merge ? (long long)N : 0, best0}, es, pbeam, parg);
        };
        auto run_edges = [&]() {
            edge(0, lo_s);
            edge(hi_s, (long long)N);
        };
        // (a day arriving in pieces: the edge tiles need both ends of the series -- they are forked to the side
        // stream in front of the LAST interior piece, once everything has been asked for, and run beside it)
        bool edges_done = false;
        auto edges_of_a_fed_day = [&]() -> int {
            edges_done = true;
            if (int r = feed->need((long long)N, stream)) return r;
            if (have_edge && pl->side_stream) {
                BPMF_HIP_CHECK(hipEventRecord(pl->ev_fork, stream));
                BPMF_HIP_CHECK(hipStreamWaitEvent(pl->side_stream, pl->ev_fork, 0));
                es = pl->side_stream;
            }
            run_edges();
            if (!rc && es != stream) BPMF_HIP_CHECK(hipEventRecord(pl->ev_join, es));
            return rc;
        };
        if (!feed_pieces) {
            run_edges();
            if (!rc && es != stream) BPMF_HIP_CHECK(hipEventRecord(pl->ev_join, es));
        }
        // The interior tiles: one launch per class -- or, while the day is still arriving from the host
        // (feed_pieces), one launch per class and PIECE of the range, each behind the piece of features it
        // reads.  A piece is a whole number of rounds of the chip (256 workgroups of 512 samples, one per CU):
        // 1, 2, then 4 rounds -- the first kernels start after 1 % of the upload, and a launch boundary costs
        // no partly filled round.
        long long a = lo_s;
        long long piece = piece0;
        while (a < hi_s && !rc) {
            long long b = hi_s;
            if (feed_pieces) {
                b = std::min(hi_s, a + piece);
                if (hi_s - b < piece0) b = hi_s;          // no sliver at the end
                piece = std::min<long long>(piece * 2, 4 * piece0);
                if (b == hi_s) rc = edges_of_a_fed_day();
                else rc = feed->need(std::min<long long>((long long)N, b + std::max(sh.tmax_all, 0) + 8 + 1024), stream);
            }
            for (int c = 0; c < sh.n_classes && !rc; ++c) {
                const BpFastClass& fc = pl->cls[c];
                rc = launch_beam_fast(fc, sh.id_offset, U, N, a / fc.tile, b / fc.tile, stream,
                                      pbeam + (size_t)c * n_split * N, parg + (size_t)c * n_split * N, n_split,
                                      merge ? (long long)N : 0, best0);
            }
            a = b;
        }
        if (feed_pieces && !rc && !edges_done) rc = edges_of_a_fed_day();     // (no interior tile at all)
        if (!rc && es != stream) BPMF_HIP_CHECK(hipStreamWaitEvent(stream, pl->ev_join, 0));
        return rc;
    }, finish);
    profile_mark(BPMF_KERNEL_BP_BEAM, 1, stream);
    return rc_all;
}

}  // namespace

// ---- a batch of short series (event relocation, bp_relocate.hip) ----
// reduce="max" of E series: event e reads the prestack U + e S P N and writes beam / arg + e N.  Always the general
// kernel over every tile (series this short have next to no interior tiles), the build's conventions (running
// maximum from (0, first id)).  A plan without LDS windows runs its events one after the other on the stream and
// folds each through the same rows.
int bpmf::bp_max_batch(const bpmf_bp_plan* pl, const BpSchedule& sch, void* d_workspace, size_t N, size_t E,
                       int out_of_bounds, hipStream_t stream, float* beam, int32_t* arg)
{
    const float* U = (const float*)((char*)d_workspace + sch.o_prestack);
    const size_t u_estride = pl->shape.S * pl->shape.P * N;
    auto finish = [](float*, int32_t*) -> int { return 0; };
    if (sch.path == BP_PATH_DIRECT) {
        for (size_t e = 0; e < E; ++e) {
            if (int rc = with_partial_rows(sch, d_workspace, N, 1, beam + e * N, arg + e * N, stream,
                                           [&](float* pbeam, int32_t* parg, bool) -> int {
                    return launch_beam_direct(pl, U + e * u_estride, N, out_of_bounds, BPMF_BP_REDUCE_MAX, stream, pbeam,
                                              parg, sch.n_split, (long long)N, 0.0f);
                }, finish))
                return rc;
        }
        return 0;
    }
    return with_partial_rows(sch, d_workspace, N, E, beam, arg, stream, [&](float* pbeam, int32_t* parg, bool merge) -> int {
        BpLaunch lc{0, -1, sch.n_split, merge ? (long long)N : 0, 0.0f};
        lc.n_events = (int)E;
        lc.u_estride = (long long)u_estride;
        lc.out_estride = (long long)(merge ? (size_t)sch.rows * N : N);
        return dispatch_beam(pl, sch.kernel, U, N, out_of_bounds, BPMF_BP_REDUCE_MAX, lc, stream, pbeam, parg);
    }, finish);
}

extern "C" int bpmf_bp_run_dev(const bpmf_bp_plan* pl, const float* d_features,
                               const float* d_w_phases, size_t N, size_t C, int out_of_bounds,
                               int reduce, void* d_workspace, size_t workspace_bytes,
                               bpmf_stream_t stream, float* d_beam_out, int32_t* d_arg_out)
{
    return bp_run_dev(pl, d_features, d_w_phases, N, C, out_of_bounds, reduce, d_workspace, workspace_bytes,
                      (hipStream_t)stream, d_beam_out, d_arg_out, nullptr, false);
}

namespace {
// the plans bpmf_bp_run keeps (bp_plan_cache.h); never destroyed: at process exit the runtime may be gone already
BpPlanCache& plan_cache()
{
    static BpPlanCache* c = new BpPlanCache(
        [](void* pl) { bpmf_bp_plan_destroy((bpmf_bp_plan*)pl); },
        [] { int n = 0; return device_counts(&n, nullptr) == hipSuccess ? n : 0; });
    return *c;
}

// The day of features of a host-pointer call, uploaded IN PIECES on the copy stream while the kernels of the pieces
// that have arrived run (bp_run_dev asks for the samples it is about to read) -- the upload of a whole day in front
// of the first kernel cost cfg3 a third of its time (201.7 ms end to end against 150.6 resident, round-4 bench;
// BPMF makes exactly this call, template_search.py:549-558).
struct HostFeed : BpFeed {
    HostCall& hc; DayFeed& day; const float* host; float* d_feat; const float* d_wp; float* U;
    size_t N, C; int S, P; long long have = 0;
    HostFeed(HostCall& hc_, DayFeed& day_, const float* host_, float* d_feat_, const float* d_wp_, float* U_, size_t N_,
             size_t C_, size_t S_, size_t P_)
        : hc(hc_), day(day_), host(host_), d_feat(d_feat_), d_wp(d_wp_), U(U_), N(N_), C(C_), S((int)S_), P((int)P_) {}
    int need(long long samp_end, hipStream_t stream) override
    {
        samp_end = std::min<long long>((samp_end + 1023) / 1024 * 1024, (long long)N);
        if (samp_end <= have) return 0;
        day.arrive(d_feat, host, (size_t)S * C, N, (size_t)have, (size_t)samp_end, stream);
        if (!hc.ok()) return hc.rc;
        const int rc = launch_prestack(d_feat, d_wp, N, C, S, P, U, have, samp_end, stream);
        if (have == 0) t_call_stats.first_kernel_ms = host_now_ms() - hc.t0;      // the first kernels follow
        have = samp_end;
        return rc;
    }
};

int bp_run_call(const float* features, const int32_t* moveouts, const float* w_phases, const float* w_sources, size_t N,
                size_t K, size_t S, size_t C, size_t P, int out_of_bounds, int reduce, int device, float* beam_out,
                int32_t* arg_out, bool defer_finish, FanoutScope& fan)
{
    if (!features || !moveouts || !w_phases || !w_sources || !beam_out) {
        set_error("bpmf_bp_run: null pointer");
        return -1;
    }
    HostCall hc("bpmf_bp_run", device, fan);
    if (!hc.ok()) return hc.rc;
    DeviceContext* ctx = hc.ctx;
    BpPlanCache::Ticket ticket;
    bpmf_bp_plan* pl = (bpmf_bp_plan*)plan_cache().take(device, K, S, P, moveouts, w_sources, option_generation(), &ticket);
    if (!pl)
        if (int rc = bpmf_bp_plan_create(moveouts, w_sources, K, S, P, device, 0, &pl)) return rc;
    t_call_stats.plan_ms = host_now_ms() - hc.t0;
    hc.also_drain = pl->side_stream;
    const size_t b_f = S * C * N * sizeof(float), b_wp = S * C * P * sizeof(float),
                 b_ws = bpmf_bp_workspace_bytes(pl, N, C),
                 b_beam = (reduce == BPMF_BP_REDUCE_MAX ? N : K * N) * sizeof(float),
                 b_arg = N * sizeof(int32_t);
    const size_t o_f = hc.add(b_f), o_wp = hc.add(b_wp), o_ws = hc.add(b_ws), o_beam = hc.add(b_beam), o_arg = hc.add(b_arg);
    hipStream_t stream = ctx->s_run;
    hipError_t e = hipSuccess;
    if (char* base = hc.reserve(std::min<size_t>((size_t)64 << 20, std::max<size_t>(b_f, 4096)))) {
        // The day of features: a peer of a multi-device call copies it from the first device, everybody else feeds it
        // from the host while the kernels run.  The weights go through the pinned pieces as well.
        DayFeed day(hc, "H2D features");
        const bool from_peer = day.from_peer(base + o_f, b_f, stream);
        if (hc.ok() && (e = staged_upload_rows(ctx, (float*)(base + o_wp), w_phases, 1, b_wp / 4, 0, b_wp / 4, stream)) != hipSuccess)
            hc.fail(e, "H2D weights_phases");
        if (hc.ok() && reduce == BPMF_BP_REDUCE_NONE && (e = hipMemsetAsync(base + o_beam, 0, b_beam, stream)) != hipSuccess)
            hc.fail(e, "memset");
        if (hc.ok()) {
            HostFeed host_feed(hc, day, features, (float*)(base + o_f), (const float*)(base + o_wp), (float*)(base + o_ws), N, C, S, P);
            if (from_peer) t_call_stats.first_kernel_ms = host_now_ms() - hc.t0;
            hc.note(bp_run_dev(pl, (const float*)(base + o_f), (const float*)(base + o_wp), N, C, out_of_bounds, reduce,
                               base + o_ws, b_ws, stream, (float*)(base + o_beam), (int32_t*)(base + o_arg),
                               from_peer ? nullptr : &host_feed, defer_finish));
        }
        // The results' way back, through the pinned pieces (staged_download: the runtime's pageable path page-locks a
        // destination it has not seen before, and a result array is a new allocation on every call)
        hc.wait_since = host_now_ms();
        if (hc.ok() && (e = staged_download(ctx, beam_out, base + o_beam, b_beam, stream)) != hipSuccess) hc.fail(e, "D2H beam");
        if (hc.ok() && reduce == BPMF_BP_REDUCE_MAX && arg_out &&
            (e = staged_download(ctx, arg_out, base + o_arg, b_arg, stream)) != hipSuccess) hc.fail(e, "D2H argmax");
    }
    hc.finish();        // (the plan's streams are drained: it may go back to the cache, or be destroyed)
    plan_cache().give_back(ticket, pl, moveouts, w_sources);
    return hc.rc;
}
}  // namespace

int bpmf::bp_run_host(const float* features, const int32_t* moveouts, const float* w_phases,
                      const float* w_sources, size_t N, size_t K, size_t S, size_t C, size_t P, int out_of_bounds,
                      int reduce, int device, float* beam_out, int32_t* arg_out, bool defer_finish, FanoutScope& fan)
{
    return guarded("bpmf_bp_run", [&] {
        return bp_run_call(features, moveouts, w_phases, w_sources, N, K, S, C, P, out_of_bounds, reduce, device,
                           beam_out, arg_out, defer_finish, fan);
    });
}

extern "C" int bpmf_bp_run(const float* features, const int32_t* moveouts, const float* w_phases,
                           const float* w_sources, size_t N, size_t K, size_t S, size_t C, size_t P,
                           int out_of_bounds, int reduce, int device, float* beam_out,
                           int32_t* arg_out)
{
    FanoutScope nobody;
    return bp_run_host(features, moveouts, w_phases, w_sources, N, K, S, C, P, out_of_bounds, reduce, device,
                       beam_out, arg_out, false, nobody);
}

extern "C" int bpmf_bp_pack_max_dev(const float* d_beam, const int32_t* d_arg, size_t N,
                                    int as_signed, bpmf_stream_t stream, uint64_t* d_packed)
{
    if (!d_beam || !d_arg || !d_packed) { set_error("bpmf_bp_pack_max_dev: null pointer"); return -1; }
    if (N == 0) return 0;
    bp_pack_kernel<<<dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(
        d_beam, d_arg, N, as_signed ? 0x8000000000000000ull : 0ull, (unsigned long long*)d_packed);
    BPMF_LAUNCH_CHECK();
    return 0;
}

extern "C" int bpmf_bp_unpack_max_dev(const uint64_t* d_packed, size_t N, int as_signed,
                                      bpmf_stream_t stream, float* d_beam, int32_t* d_arg)
{
    if (!d_beam || !d_arg || !d_packed) { set_error("bpmf_bp_unpack_max_dev: null pointer"); return -1; }
    if (N == 0) return 0;
    bp_unpack_kernel<<<dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(
        (const unsigned long long*)d_packed, N, as_signed ? 0x8000000000000000ull : 0ull, d_beam,
        d_arg);
    BPMF_LAUNCH_CHECK();
    return 0;
}
