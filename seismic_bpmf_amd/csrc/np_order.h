// The order in which NumPy's add.reduce adds a contiguous row of float32 or float64 (numpy/core/src/umath/
// loops_utils.h.src: pairwise_sum, and the ufunc buffer of 8192 elements) -- the single definition in csrc/; every
// "bit for bit NumPy" sum of the library is built from these one-thread primitives:
//   - a row longer than NP_CHUNK elements is summed in pieces of NP_CHUNK, the piece sums added in order;
//   - a piece is a binary tree: a range longer than NP_LEAF splits at np_split(n), n/2 rounded down to a multiple of 8,
//     and its value is sum(left) + sum(right);
//   - a leaf of 8 .. NP_LEAF elements is eight strided running sums combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)),
//     then the tail one by one; under 8 elements it is a running sum from 0.
// What a caller does with a tree's value -- start a chain at it or at 0, which decides the sign of a zero -- is the
// caller's: nothing here adds an identity except np_sum, which is np.add.reduce itself.
// Nothing but <cstdint> is needed, so a host compiler compiles the same text (tests/np_order_check.cpp).  The bodies
// switch contraction off themselves: a functor's product is never fused into the sums.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define NP_ORDER_FN __host__ __device__ inline
#else
#define NP_ORDER_FN inline
#endif

namespace bpmf {

constexpr int NP_LEAF = 128;                           // longest range that is summed without a split
constexpr int NP_CHUNK = 8192;                         // NumPy's buffer: the longest range that is one tree
constexpr int NP_MAX_DEPTH = 15;                       // of a leaf below its chunk's root; bounds for 1 .. NP_CHUNK,
constexpr int NP_MAX_LEAVES = 128;                     // both far from reached (tests/test_np_order.py)

NP_ORDER_FN int np_split(int n)
{
    const int n2 = n / 2;
    return n2 - n2 % 8;
}

// one leaf (n <= NP_LEAF) over f(off) .. f(off + n - 1)
template <typename T, typename F>
NP_ORDER_FN T np_leaf_sum(const F& f, int off, int n)
{
#pragma clang fp contract(off)
    if (n < 8) {
        T res = (T)0;
        for (int i = 0; i < n; ++i) res = res + f(off + i);
        return res;
    }
    T r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = f(off + j);
    int i = 8;
    for (; i < n - (n & 7); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = r[j] + f(off + i + j);
    }
    T res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res = res + f(off + i);
    return res;
}

// the leaf [off, off + len) that holds position p of a chunk of n elements (0 <= p < n <= NP_CHUNK), and its depth
// below the chunk's root
struct NpLeaf {
    int off, len, depth;
};
NP_ORDER_FN NpLeaf np_leaf_of(int n, int p)
{
    NpLeaf l{0, n, 0};
    while (l.len > NP_LEAF) {
        const int n2 = np_split(l.len);
        if (p < l.off + n2) l.len = n2;
        else { l.off += n2; l.len -= n2; }
        ++l.depth;
    }
    return l;
}

// The leaves of a chunk of n <= NP_CHUNK elements in order, visit(NpLeaf) for each: the leaf of 0, then the leaf of the
// position behind it, and so on -- a descent from the root per leaf instead of a stack.
template <typename V>
NP_ORDER_FN void np_walk(int n, const V& visit)
{
    for (int p = 0; p < n;) {
        const NpLeaf l = np_leaf_of(n, p);
        visit(l);
        p = l.off + l.len;
    }
}

// The tree above the leaves: push their values in order, each with its depth.  A value waits at its depth for its
// right sibling; when that comes they combine as left + right one level up.  After the last leaf value[0] is the
// tree's.  `value`: NP_MAX_DEPTH + 1 entries of the caller's, private or LDS.
template <typename T>
struct NpFold {
    T* value;
    uint32_t waiting;                                  // bit d: value[d] holds a left half; starts at 0
    NP_ORDER_FN void push(T v, int d)
    {
#pragma clang fp contract(off)
        for (; waiting >> d & 1u; --d) {
            v = value[d] + v;
            waiting ^= 1u << d;
        }
        value[d] = v;
        waiting |= 1u << d;
    }
};

// the tree's value for the one chunk f(off) .. f(off + n - 1), n <= NP_CHUNK, and nothing else (n == 0: (T)0)
template <typename T, typename F>
NP_ORDER_FN T np_chunk_sum(const F& f, int off, int n)
{
    T value[NP_MAX_DEPTH + 1];
    value[0] = (T)0;
    NpFold<T> fold{value, 0};
    np_walk(n, [&](const NpLeaf& l) { fold.push(np_leaf_sum<T>(f, off + l.off, l.len), l.depth); });
    return value[0];
}

// np.sum over f(0) .. f(n - 1): the chunks in order, from the identity
template <typename T, typename F>
NP_ORDER_FN T np_sum(const F& f, int n)
{
#pragma clang fp contract(off)
    T total = (T)0;
    for (int piece = 0; piece < n; piece += NP_CHUNK)
        total = total + np_chunk_sum<T>(f, piece, n - piece < NP_CHUNK ? n - piece : NP_CHUNK);
    return total;
}

}  // namespace bpmf
