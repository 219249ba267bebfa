// Host check of csrc/day_rows.h, driven by tests/test_day_rows.py.
//   day_rows_check FILE   FILE: int64 S, C, N, n; the day, S C N float32; then records of three int64 (item, has_start,
//                         start).  The starts of a call are one array indexed by the window, so a record's start is
//                         placed at its window's index of an otherwise zero array (has_start = 0: no array at all).
// Per record one line "item win c s trace start inside" and the bits of the n clipped samples of the row, in
// hexadecimal.  Then the refusals of day_rows_refused: per case "refused <0|1> <text>"; the last two with a null pointer.
#include "day_rows.h"

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace bpmf;

static char g_text[512];

static void keep_text(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_text, sizeof g_text, fmt, ap);
    va_end(ap);
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t head[4];
    if (std::fread(head, sizeof head, 1, f) != 1) return 2;
    const int S = (int)head[0], C = (int)head[1], n = (int)head[3];
    const long long N = head[2];
    std::vector<float> day((size_t)S * C * N);
    if (std::fread(day.data(), sizeof(float), day.size(), f) != day.size()) return 2;
    int64_t rec[3];
    while (std::fread(rec, sizeof rec, 1, f) == 1) {
        const unsigned item = (unsigned)rec[0];
        std::vector<long long> starts((size_t)(item / C) + 1, 0);
        starts.back() = rec[2];
        const DayRow r = day_row(S, C, N, rec[1] ? starts.data() : nullptr, item);
        std::printf("%u %d %d %d %lld %lld %d", item, r.win, r.c, r.s, r.trace, r.start,
                    day_window_inside(r.start, n, N) ? 1 : 0);
        for (int i = 0; i < n; ++i) {
            const float v = clipped_sample(day.data() + r.trace, r.start + i, N);
            uint32_t bits;
            std::memcpy(&bits, &v, sizeof bits);
            std::printf(" %08x", (unsigned)bits);
        }
        std::printf("\n");
    }
    std::fclose(f);

    const size_t most = 0x7fffffffull, limit = (size_t)DAY_INDEX_LIMIT;
    const struct { bool whole; size_t S, C, N, windows; bool null_pointer; } cases[] = {
        {false, 3, 2, 50, 7},          {true, 3, 2, 50, 7},          {true, 3, 2, 50, 6},
        {false, 0, 2, 50, 6},          {false, 3, 0, 50, 6},         {false, 3, 2, 0, 6},
        {false, 3, 2, limit, 6},       {false, 3, 2, limit + 1, 6},  {false, 3, 2, 50, most / 2},
        {false, 3, 2, 50, most / 2 + 1}, {false, most / 2 + 1, 2, 50, 6}, {true, most / 2 + 1, 2, 50, most / 2 + 1},
        {false, most / 2, 2, 50, 6},   {true, 3, 2, 50, 0},          {true, 0, 0, 0, 0},
        {false, 3, 2, 50, 6, true},    {true, 0, 0, 0, 0, true},
    };
    for (const auto& k : cases) {
        g_text[0] = 0;
        const bool refused = day_rows_refused("entry", k.whole, k.null_pointer, k.S, k.C, k.N, k.windows, keep_text);
        std::printf("refused %d %s\n", refused ? 1 : 0, g_text);
    }
    return 0;
}
