// NumPy's float32 sums of a row staged in LDS, by one workgroup, bit for bit: np.sum / np.mean / np.std of at most
// NP_CHUNK float32 -- one pairwise tree.  The order of the additions is np_order.h's, the single definition; what is
// here is its block layout, shared by templates.hip and picker.hip.  The shape of the tree depends on the length
// alone: the host lists its leaves once (list_leaves: np_walk) and passes the list to the kernel by value.  One
// workgroup of TP_THREADS threads works on one row: each (leaf, accumulator j) is one thread's at most 16 sequential
// adds out of LDS; one thread per leaf adds the eight partial sums and the tail; thread 0 folds the leaves (NpFold, on
// SumScratch's LDS array).
#pragma once
#include "common.h"
#include "np_order.h"
#include <cmath>

namespace bpmf {

constexpr int TP_THREADS = 256;

// The leaves of the tree over n elements, in order: offset (bits 0-13), length (14-21), depth (22-27).
struct LeafTable {
    int n;
    uint32_t leaf[NP_MAX_LEAVES];
};

inline bool list_leaves(int n, LeafTable& t)           // 1 <= n <= NP_CHUNK
{
    t.n = 0;
    np_walk(n, [&](const NpLeaf& l) {
        if (t.n < NP_MAX_LEAVES) t.leaf[t.n] = (uint32_t)l.off | ((uint32_t)l.len << 14) | ((uint32_t)l.depth << 22);
        ++t.n;
    });
    return t.n <= NP_MAX_LEAVES;
}

struct SumScratch {
    float part[NP_MAX_LEAVES * 8];
    float leaf_sum[NP_MAX_LEAVES];
    float fold_value[NP_MAX_DEPTH + 1];
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
        NpFold<float> fold{s.fold_value, 0};
        for (int i = 0; i < n_leaves; ++i) fold.push(s.leaf_sum[i], (tab.leaf[i] >> 22) & 0x3f);
        s.total = __fadd_rn(0.0f, s.fold_value[0]);               // np.add.reduce starts from its identity: -0.0 -> +0.0
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

}  // namespace bpmf
