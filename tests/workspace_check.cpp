// csrc/workspace.h alone: one layout, measured on a null base and placed on a real one.  A stand-alone host
// program (tests/test_workspace_layout.py builds it, with the sanitizers where the compiler has them, and runs
// it); it includes nothing of the library but that header.  Exit status 0 and a last line "ok ..." when every
// check holds; the first failed check is printed and the status is 1.
#include "workspace.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using bpmf::Carver;

namespace {

struct Region {
    const char* name;
    char* at;
    size_t offset, payload, align;   // offset before the take, the bytes asked for, the alignment of the END
};

struct Pair { float a; int b; int c; };   // 12 bytes: a count of them is no multiple of 8

// An inner layout, carved from the address of a nested region of the outer one.
size_t inner(void* base, size_t n, std::vector<Region>* out)
{
    Carver c(base);
    size_t o = c.offset();
    char* p = (char*)c.take<double>(n);
    if (out) out->push_back({"inner.double", p, o, n * 8, 256});
    o = c.offset();
    p = (char*)c.take<unsigned char>(n + 1);
    if (out) out->push_back({"inner.byte", p, o, n + 1, 256});
    return c.bytes();
}

// Every feature once: default and explicit alignment, extra bytes, a skip, a nested region, counts of 0 and 1.
// `mark` receives offset() in the middle, as row_carve's zero_bytes does.
size_t layout(void* base, size_t n, std::vector<Region>& out, std::vector<Region>& nested, size_t* mark, size_t* skip_at)
{
    Carver c(base);
    auto note = [&](const char* name, void* p, size_t o, size_t payload, size_t align) {
        out.push_back({name, (char*)p, o, payload, align});
    };
    size_t o = c.offset();
    note("double", c.take<double>(n), o, n * 8, 256);
    o = c.offset();
    note("pair", c.take<Pair>(n), o, n * sizeof(Pair), 256);
    *mark = c.offset();
    *skip_at = c.offset();
    c.skip(256);
    o = c.offset();
    note("float+64", c.take<float>(n, 64), o, n * 4 + 64, 256);
    o = c.offset();
    note("empty", c.take<int>(0), o, 0, 256);
    o = c.offset();
    note("one", c.take<char>(1), o, 1, 256);
    o = c.offset();
    const size_t inner_bytes = inner(nullptr, n, nullptr);
    void* in = c.nest(inner_bytes);
    note("nested", in, o, inner_bytes, 256);
    const size_t again = inner(in, n, &nested);
    if (again != inner_bytes) { std::printf("FAIL inner layout: %zu bytes measured, %zu placed\n", inner_bytes, again); std::exit(1); }
    o = c.offset();
    note("int/16", c.take<int>(n, 0, 16), o, n * 4, 16);
    o = c.offset();
    note("word/16", c.nest(16, 16), o, 16, 16);
    o = c.offset();
    note("short/1", c.take<short>(n, 0, 1), o, n * 2, 1);
    if (c.offset() != c.bytes()) { std::printf("FAIL offset() != bytes() at the end\n"); std::exit(1); }
    return c.bytes();
}

#define CHECK(cond, ...)                                                                                               \
    do {                                                                                                               \
        if (!(cond)) { std::printf("FAIL n=%zu %s: ", n, #cond); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } \
    } while (0)

int check(size_t n)
{
    std::vector<Region> m, mn, p, pn;
    size_t mark_m = 0, mark_p = 0, skip_m = 0, skip_p = 0;
    const size_t measured = layout(nullptr, n, m, mn, &mark_m, &skip_m);
    // measuring returns only null pointers
    for (const Region& r : m) CHECK(r.at == nullptr, "%s", r.name);
    for (const Region& r : mn) CHECK(r.at == nullptr, "%s", r.name);

    // a base aligned to 256 and exactly `measured` bytes behind it: AddressSanitizer guards both ends
    void* raw = nullptr;
    CHECK(posix_memalign(&raw, 256, measured) == 0, "posix_memalign");
    char* base = (char*)raw;
    const size_t placed = layout(base, n, p, pn, &mark_p, &skip_p);
    CHECK(placed == measured, "%zu placed, %zu measured", placed, measured);
    CHECK(mark_p == mark_m && skip_p == skip_m, "marks differ");
    CHECK(p.size() == m.size() && pn.size() == mn.size(), "region counts differ");

    size_t at = 0, start_align = 256;
    for (size_t i = 0; i < p.size(); ++i) {
        const Region &a = p[i], &b = m[i];
        CHECK(a.offset == b.offset && a.payload == b.payload, "%s: measured at %zu, placed at %zu", a.name, b.offset, a.offset);
        // a region starts where the one before it ended (behind the skip: 256 bytes later): no overlap, no gap
        CHECK(a.offset == at, "%s: at %zu, the region before it ends at %zu", a.name, a.offset, at);
        CHECK(a.at == base + a.offset, "%s: address", a.name);
        // every start is aligned to the coarsest alignment asked for so far
        CHECK((uintptr_t)a.at % start_align == 0, "%s: start not on %zu", a.name, start_align);
        std::memset(a.at, 0x5a, a.payload);                      // the payload lies inside the allocation
        // the advance: the payload (count * sizeof(T) + extra_bytes) rounded up to the alignment asked for
        at += (a.payload + a.align - 1) / a.align * a.align;
        start_align = a.align < start_align ? a.align : start_align;
        if (i == 1) {
            CHECK(mark_p == at && skip_p == at, "offset() behind two regions: %zu, they end at %zu", mark_p, at);
            at += 256;
        }
    }
    CHECK(at == placed, "the last region ends at %zu, bytes() is %zu", at, placed);
    // the inner layout lies inside its nested region, from its first byte
    const Region& host = p[5];
    CHECK(std::strcmp(host.name, "nested") == 0, "order");
    CHECK(pn[0].at == host.at && pn[0].offset == 0, "inner layout does not start at the nested region");
    CHECK(pn[1].at + pn[1].payload <= host.at + host.payload, "inner layout leaves the nested region");
    CHECK(pn[1].at >= pn[0].at + pn[0].payload, "inner regions overlap");
    std::free(raw);
    return 0;
}

}  // namespace

int main()
{
    if (bpmf::align_up(0, 256) != 0 || bpmf::align_up(1, 256) != 256 || bpmf::align_up(256, 256) != 256 ||
        bpmf::align_up(257, 256) != 512 || bpmf::align_up(17, 16) != 32 || bpmf::align_up(5, 1) != 5) {
        std::printf("FAIL align_up\n");
        return 1;
    }
    const size_t counts[] = {0, 1, 2, 3, 21, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000, 4097};
    for (size_t n : counts)
        if (check(n)) return 1;
    std::printf("ok %zu layouts\n", sizeof(counts) / sizeof(counts[0]));
    return 0;
}
