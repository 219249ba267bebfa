// NumPy's float32 sums on the device, shared by templates.hip and picker.hip: np.sum / np.mean / np.std of a row of at
// most 8192 float32 staged in LDS, bit for bit.  pairwise_sum is NumPy's: under 8 elements a running sum from 0; up to
// 128 elements eight strided running sums combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) plus the tail; above 128 a
// split at n/2 rounded down to a multiple of 8.  The shape of that tree depends on the length alone: the host lists its
// leaves (offset, length, depth) once -- at most 128 -- and passes the list to the kernel by value.  One workgroup of
// TP_THREADS threads works on one row: each (leaf, accumulator j) is one thread's at most 16 sequential adds out of
// LDS; one thread per leaf adds the eight partial sums and the tail; thread 0 folds the leaves with a stack (equal
// depths combine), which is the recursion.
#pragma once
#include "common.h"
#include <cmath>

namespace bpmf {

constexpr int TP_THREADS = 256;
constexpr int TP_MAX_SAMPLES = 8192;               // NumPy sums longer rows in buffers of 8192: another tree
constexpr int TP_MAX_LEAVES = 128;
constexpr int TP_MAX_DEPTH = 15;

// The leaves of NumPy's pairwise sum over n elements, in order: offset (bits 0-13), length (14-21), depth (22-27).
struct LeafTable {
    int n;
    uint32_t leaf[TP_MAX_LEAVES];
};

inline bool list_leaves(int offset, int n, int depth, LeafTable& t)
{
    if (n <= 128) {
        if (t.n >= TP_MAX_LEAVES || depth > TP_MAX_DEPTH) return false;
        t.leaf[t.n++] = (uint32_t)offset | ((uint32_t)n << 14) | ((uint32_t)depth << 22);
        return true;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    return list_leaves(offset, n2, depth + 1, t) && list_leaves(offset + n2, n - n2, depth + 1, t);
}

struct SumScratch {
    float part[TP_MAX_LEAVES * 8];
    float leaf_sum[TP_MAX_LEAVES];
    float stack_value[TP_MAX_DEPTH + 1];
    int stack_depth[TP_MAX_DEPTH + 1];
    float total;
};

// np.sum of the float32 row x (in LDS, complete) whose leaves `tab` lists; every thread of the block gets the sum.
__device__ inline float block_pairwise_sum(const float* x, const LeafTable& tab, SumScratch& s, int tid)
{
    const int n_leaves = tab.n;
    for (int it = tid; it < n_leaves * 8; it += TP_THREADS) {
        const uint32_t w = tab.leaf[it >> 3];
        const int j = it & 7, off = w & 0x3fff, len = (w >> 14) & 0xff;
        float r = 0.0f;
        if (len < 8) {                                             // the whole row: a running sum from 0
            if (j == 0)
                for (int i = 0; i < len; ++i) r = __fadd_rn(r, x[off + i]);
        } else {
            r = x[off + j];
            for (int i = 8; i < len - (len & 7); i += 8) r = __fadd_rn(r, x[off + i + j]);
        }
        s.part[it] = r;
    }
    __syncthreads();
    if (tid < n_leaves) {
        const uint32_t w = tab.leaf[tid];
        const int off = w & 0x3fff, len = (w >> 14) & 0xff;
        const float* r = s.part + 8 * tid;
        float res = r[0];
        if (len >= 8) {
            res = __fadd_rn(__fadd_rn(__fadd_rn(r[0], r[1]), __fadd_rn(r[2], r[3])),
                            __fadd_rn(__fadd_rn(r[4], r[5]), __fadd_rn(r[6], r[7])));
            for (int i = len - (len & 7); i < len; ++i) res = __fadd_rn(res, x[off + i]);
        }
        s.leaf_sum[tid] = res;
    }
    __syncthreads();
    if (tid == 0) {
        int sp = 0;
        for (int i = 0; i < n_leaves; ++i) {
            float v = s.leaf_sum[i];
            int d = (tab.leaf[i] >> 22) & 0x3f;
            while (sp > 0 && s.stack_depth[sp - 1] == d) {         // sum(left half) + sum(right half)
                --sp;
                v = __fadd_rn(s.stack_value[sp], v);
                --d;
            }
            s.stack_value[sp] = v;
            s.stack_depth[sp] = d;
            ++sp;
        }
        s.total = __fadd_rn(0.0f, s.stack_value[0]);               // np.add.reduce starts from its identity: -0.0 -> +0.0
    }
    __syncthreads();
    const float total = s.total;
    __syncthreads();                                               // (the next sum writes the scratch again)
    return total;
}

// np.std of the row of `len` float32 in LDS; the row is replaced by its squared deviations.  `mean_out`: np.mean.
__device__ inline float block_std(float* x, int len, const LeafTable& tab, SumScratch& s, int tid,
                                  float* mean_out = nullptr)
{
    const float count = (float)len;
    const float mean = __fdiv_rn(block_pairwise_sum(x, tab, s, tid), count);
    if (mean_out) *mean_out = mean;
    for (int l = tid; l < len; l += TP_THREADS) {
        const float d = __fsub_rn(x[l], mean);
        x[l] = __fmul_rn(d, d);
    }
    __syncthreads();
    // (sqrtf: the correctly rounded square root, v_sqrt_f32 plus a next-up / next-down fix-up by fma.  __fsqrt_rn
    // compiles to the bare v_sqrt_f32, which is one ulp off NumPy's about once in fifteen windows.)
    return sqrtf(__fdiv_rn(block_pairwise_sum(x, tab, s, tid), count));
}

// data[i] inside the day, +0.0 outside; the address is clamped, so the load is never predicated (n >= 1)
__device__ __forceinline__ float clipped_sample(const float* __restrict__ x, long long i, long long n)
{
    const long long ic = i < 0 ? 0 : (i >= n ? n - 1 : i);
    const float v = x[ic];
    return ic == i ? v : 0.0f;
}

}  // namespace bpmf
