// Host check of csrc/np_order.h, driven by tests/test_np_order.py.
//   np_order_check FILE   FILE: records of (int32 m, m float32).  Per record one line "m <bits of np_sum<float>(x)>
//                         <bits of np_sum<double>(i * (double) x[i])>", in hexadecimal.
// Then, for every chunk length 1 .. NP_CHUNK: the leaves of the walk tile the chunk in order, np_leaf_of finds each from
// its first and from its last element, there are at most NP_MAX_LEAVES, none is deeper than NP_MAX_DEPTH and the fold
// of their lengths ends with the chunk's alone.  The last line is "walk ok <most leaves> <greatest depth>"; a violation is reported and the exit status is 1.
#include "np_order.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace bpmf;

static bool check_walk(int n, int& most_leaves, int& deepest)
{
    int value[32];                                         // (a fold of the leaves' lengths: the tree's value is n)
    NpFold<int> fold{value, 0};
    int at = 0, leaves = 0;
    bool ok = true;
    np_walk(n, [&](const NpLeaf& l) {
        const NpLeaf first = np_leaf_of(n, l.off), last = np_leaf_of(n, l.off + l.len - 1);
        auto same = [&](const NpLeaf& o) { return o.off == l.off && o.len == l.len && o.depth == l.depth; };
        if (l.off != at || l.len < 1 || l.len > NP_LEAF || !same(first) || !same(last) || l.depth > NP_MAX_DEPTH) {
            std::printf("walk of %d: leaf %d is (%d, %d, depth %d), expected at %d; from its last element (%d, %d, depth "
                        "%d)\n", n, leaves, l.off, l.len, l.depth, at, last.off, last.len, last.depth);
            ok = false;
        }
        if (l.depth <= NP_MAX_DEPTH) fold.push(l.len, l.depth);
        at += l.len > 0 ? l.len : 1;
        ++leaves;
        if (l.depth > deepest) deepest = l.depth;
    });
    if (at != n || leaves > NP_MAX_LEAVES || fold.waiting != 1u || value[0] != n) {
        std::printf("walk of %d: %d leaves cover %d elements, the fold ends waiting at %x with %d\n", n, leaves, at,
                    (unsigned)fold.waiting, value[0]);
        ok = false;
    }
    if (leaves > most_leaves) most_leaves = leaves;
    return ok;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t m;
    std::vector<float> x;
    while (std::fread(&m, sizeof m, 1, f) == 1) {
        x.resize((size_t)m);
        if (m < 0 || std::fread(x.data(), sizeof(float), (size_t)m, f) != (size_t)m) return 2;
        const float* p = x.data();
        const float s32 = np_sum<float>([=](int i) { return p[i]; }, m);
        const double s64 = np_sum<double>([=](int i) { return (double)i * (double)p[i]; }, m);
        uint32_t b32;
        uint64_t b64;
        std::memcpy(&b32, &s32, sizeof b32);
        std::memcpy(&b64, &s64, sizeof b64);
        std::printf("%d %08x %016llx\n", (int)m, (unsigned)b32, (unsigned long long)b64);
    }
    std::fclose(f);
    int most_leaves = 0, deepest = 0;
    for (int n = 1; n <= NP_CHUNK; ++n)
        if (!check_walk(n, most_leaves, deepest)) return 1;
    std::printf("walk ok %d %d\n", most_leaves, deepest);
    return 0;
}
