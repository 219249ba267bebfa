// Host-only check of the backprojection planner under sanitizers: bp_plan_host + bp_schedule (csrc/bp_plan.hip) on
// the kinds of tables tests/test_bp_launch_info.py uses and on seeded random tables (K <= 200, S <= 70, P <= 3,
// signed moveouts, zero weights), under the option sets that reach every planner branch; the invariants of the
// schedule are asserted on every call.  Needs no GPU and loads nothing into another process.  From the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/bp_plan_host_check.hip \
//         seismic_bpmf_amd/csrc/bp_plan.hip seismic_bpmf_amd/csrc/util.hip -o /tmp/bp_plan_host_check \
//     && /tmp/bp_plan_host_check
#include "../seismic_bpmf_amd/csrc/bp_plan.h"

#include <cstdlib>
#include <random>
#include <vector>

using namespace bpmf;

namespace {

long g_plans = 0, g_schedules = 0;

#define REQUIRE(cond)                                                                        \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, what);     \
            abort();                                                                         \
        }                                                                                    \
    } while (0)

struct Table {
    size_t K, S, P;
    std::vector<int32_t> mv;
    std::vector<float> ws;
};

// `used` weighted stations per source (capped by S; every `none_every`-th source has none), moveouts in [lo, hi]
Table make_table(std::mt19937& rng, size_t K, size_t S, size_t P, int used_lo, int used_hi, int lo, int hi, int none_every)
{
    Table t{K, S, P, std::vector<int32_t>(K * S * P), std::vector<float>(K * S, 0.0f)};
    std::uniform_int_distribution<int> tau(lo, hi), n_used(used_lo, used_hi), station(0, (int)S - 1), w(1, 4);
    for (auto& v : t.mv) v = tau(rng);
    for (size_t k = 0; k < K; ++k) {
        if (none_every && k % (size_t)none_every == 1) continue;
        const int n = std::min<int>(n_used(rng), (int)S);
        for (int placed = 0; placed < n;) {
            float& x = t.ws[k * S + (size_t)station(rng)];
            if (x == 0.0f) { x = 0.25f * (float)w(rng); ++placed; }
        }
    }
    return t;
}

void check_schedule(const BpPlanShape& sh, size_t N, int reduce, int forced, size_t n_events, const char* what)
{
    const BpSchedule s = bp_schedule(sh, N, reduce, forced, n_events);
    ++g_schedules;
    const long long n = (long long)N;
    REQUIRE(0 <= s.lo_s && s.lo_s <= s.hi_s && s.hi_s <= n);
    REQUIRE(s.lo_s == s.hi_s || (s.lo_s % 1024 == 0 && s.hi_s % 1024 == 0));
    REQUIRE(s.path == BP_PATH_INTERIOR || (s.lo_s == 0 && s.hi_s == 0));
    REQUIRE((s.path == BP_PATH_DIRECT) == sh.direct);
    REQUIRE(s.path != BP_PATH_INTERIOR || (sh.fast && reduce == BPMF_BP_REDUCE_MAX && n_events == 0));
    if (s.hi_s > s.lo_s) REQUIRE(s.lo_s + sh.tmin_all >= 0 && s.hi_s - 1 + sh.tmax_all + 8 < n);
    for (int c = 0; c < sh.n_classes; ++c) REQUIRE(s.lo_s == s.hi_s || (s.lo_s % sh.cls[c].tile == 0 && s.hi_s % sh.cls[c].tile == 0));
    REQUIRE(s.rows >= 1 && s.n_split >= 1 && s.n_split_edge >= 1 && s.n_split_edge <= s.n_split);
    REQUIRE(s.kernel.tile > 0 && (s.kernel.family != BP_FAMILY_NONE) == !sh.direct);
    REQUIRE(s.kernel.lds_bytes <= BP_LDS_MAX);
    const size_t E = n_events ? n_events : 1, sets = s.path == BP_PATH_DIRECT ? 1 : E;
    const size_t prestack = E * sh.S * sh.P * N * sizeof(float);
    REQUIRE(s.o_prestack == 0 && prestack <= s.o_pbeam && s.o_pbeam % 256 == 0 && s.o_pbeam - prestack < 256);
    if (s.rows > 1) {
        REQUIRE(s.o_pbeam + sets * s.rows * N * 4 <= s.o_parg && s.o_parg + sets * s.rows * N * 4 <= s.total);
    } else {
        REQUIRE(s.o_parg == s.o_pbeam && s.o_pbeam <= s.total);
    }
    if (n_events == 0) {     // one size for both reduce codes
        const int other = reduce == BPMF_BP_REDUCE_MAX ? BPMF_BP_REDUCE_NONE : BPMF_BP_REDUCE_MAX;
        REQUIRE(bp_schedule(sh, N, other, forced, 0).total == s.total);
    }
}

void check_table(const Table& t, const char* what)
{
    REQUIRE(bp_plan_refusal(t.mv.data(), t.ws.data(), t.K, t.S, t.P) == nullptr);
    const BpPlanHost h = bp_plan_host(t.mv.data(), t.ws.data(), t.K, t.S, t.P, 1000);
    ++g_plans;
    const BpPlanShape& sh = h.shape;
    REQUIRE(sh.K == t.K && sh.S == t.S && sh.P == t.P && sh.id_offset == 1000);
    if (sh.direct) {
        REQUIRE(sh.direct_reason != BP_LDS_PLAN && h.dhdr.size() == t.K && h.dfirst.size() == t.K + 1 && !h.dterms.empty());
        REQUIRE(!sh.fast && sh.n_classes == 0 && sh.n_groups == 0);
    } else {
        const PlanHost& ph = h.general();
        REQUIRE(sh.direct_reason == BP_LDS_PLAN && ph.srcs.size() == t.K && (int)ph.groups.size() == sh.n_groups);
        REQUIRE(ph.off.size() == t.K * (size_t)sh.NT && ph.beta.size() == ph.off.size() && sh.lds_bytes <= BP_LDS_MAX);
        REQUIRE(!sh.nsv || (h.recs.size() == t.K * (size_t)(sh.nsv / 2) && h.hdr2.size() == t.K));
        REQUIRE(!sh.ntv || h.termsv.size() == t.K * (size_t)sh.ntv);
        REQUIRE(sh.fast == (sh.n_classes > 0) && (!sh.fast || (int)h.classes.size() == sh.n_classes));
        size_t in_classes = 0;
        for (int c = 0; c < sh.n_classes; ++c) {
            const BpClassShape& cs = sh.cls[c];
            REQUIRE((cs.tile == 512 || cs.tile == 256 || cs.tile == 128) && cs.n_pass >= 1 && cs.n_groups >= cs.n_pass);
            REQUIRE(cs.n_groups % cs.n_pass == 0 && cs.lds_bytes <= BP_LDS_MAX && (int)h.classes[c].fh.fg.size() == cs.n_groups);
            in_classes += cs.n_sources;
        }
        REQUIRE(!sh.fast || in_classes <= t.K);
    }
    static const size_t Ns[] = {1, 307, 700, 1023, 1024, 1025, 2048, 3000, 3073, 5000, 512 * 1023 + 1, 512 * 1024};
    for (size_t N : Ns)
        for (int forced : {-1, 0, 3, 100000}) {
            check_schedule(sh, N, BPMF_BP_REDUCE_MAX, forced, 0, what);
            check_schedule(sh, N, BPMF_BP_REDUCE_NONE, forced, 0, what);
            for (size_t E : {(size_t)1, (size_t)7, (size_t)300}) check_schedule(sh, N, BPMF_BP_REDUCE_MAX, forced, E, what);
        }
}

struct OptionSet { const char* name[3]; long value[3]; };

}  // namespace

int main()
{
    static const OptionSet sets[] = {
        {{nullptr}, {0}}, {{"bp.dual"}, {0}}, {{"bp.fast"}, {0}}, {{"bp.tpt"}, {1}}, {{"bp.direct"}, {1}},
        {{"bp.max_group", "bp.lds_kb"}, {4, 24}}, {{"bp.fast_tile"}, {256}}, {{"bp.fast_tile", "bp.halves"}, {128, 0}},
        {{"bp.reorder", "bp.fast_uniform"}, {0, 0}}, {{"bp.compat_strict_upper_only", "bp.compat_range_all_stations"}, {1, 1}},
    };
    char what[160];
    for (const OptionSet& os : sets) {
        for (int i = 0; i < 3 && os.name[i]; ++i)
            if (bpmf_set_option(os.name[i], os.value[i]) != 0) { fprintf(stderr, "option %s: %s\n", os.name[i], bpmf_last_error()); return 1; }
        std::mt19937 rng(12345);
        // the kinds of tables of tests/test_bp_launch_info.py
        struct Kind { size_t K, S, P; int used, lo, hi, none_every; };
        static const Kind kinds[] = {
            {24, 8, 2, 8, 0, 300, 0}, {24, 8, 2, 8, -100, 200, 0}, {24, 8, 2, 8, -1500, 200, 0}, {24, 8, 2, 8, -3000, -20, 0},
            {40, 8, 2, 8, 0, 300, 0}, {40, 24, 2, 20, 0, 300, 0}, {40, 44, 2, 40, 0, 300, 0}, {300, 4, 2, 3, 0, 300, 0},
            {12, 4, 2, 3, 0, 40, 0}, {12, 8, 2, 7, 0, 40, 0}, {12, 12, 2, 11, 0, 40, 0}, {12, 16, 2, 15, 0, 40, 0},
            {12, 21, 2, 20, 0, 40, 0}, {12, 44, 2, 40, 0, 40, 0}, {30, 18, 2, 16, 0, 8, 5}, {30, 18, 2, 17, 0, 8, 5},
            {12, 8, 1, 8, 0, 40, 0}, {12, 33, 1, 33, 0, 40, 0}, {12, 65, 1, 65, 0, 40, 0}, {12, 129, 1, 129, 0, 40, 0},
            {12, 8, 3, 2, 0, 40, 0}, {12, 11, 3, 11, 0, 40, 0}, {12, 22, 3, 22, 0, 40, 0}, {12, 43, 3, 43, 0, 40, 0},
            {10, 70, 3, 45, 0, 4, 0}, {10, 70, 3, 70, 0, 4, 0}, {10, 90, 3, 90, 0, 20, 0}, {1, 1, 1, 1, 0, 0, 0}, {3, 2, 2, 0, -5, 5, 0},
        };
        for (const Kind& k : kinds) {
            snprintf(what, sizeof(what), "options %s..., table K=%zu S=%zu P=%zu used=%d moveouts %d..%d", os.name[0] ? os.name[0] : "default",
                     k.K, k.S, k.P, k.used, k.lo, k.hi);
            check_table(make_table(rng, k.K, k.S, k.P, k.used, k.used, k.lo, k.hi, k.none_every), what);
        }
        // seeded random tables
        const int n_random = os.name[0] ? 40 : 300;
        for (int i = 0; i < n_random; ++i) {
            std::mt19937 r(1000 + i);
            const size_t K = 1 + r() % 200, S = 1 + r() % 70, P = 1 + r() % 3;
            const int spread = (int[]){0, 5, 60, 400, 3000, 40000}[r() % 6], centre = (int[]){0, 0, 1, -1, -2}[r() % 5] * spread;
            const int lo = centre - (centre > 0 ? 0 : spread), hi = centre + (centre < 0 ? -9 * (spread > 9) : spread);
            const int used_hi = 1 + (int)(r() % S), used_lo = (int)(r() % (unsigned)(used_hi + 1));
            snprintf(what, sizeof(what), "options %s..., random table %d: K=%zu S=%zu P=%zu used %d..%d moveouts %d..%d",
                     os.name[0] ? os.name[0] : "default", i, K, S, P, used_lo, used_hi, std::min(lo, hi), std::max(lo, hi));
            check_table(make_table(r, K, S, P, used_lo, used_hi, std::min(lo, hi), std::max(lo, hi), (int)(r() % 4) * 3), what);
        }
        for (int i = 0; i < 3 && os.name[i]; ++i) {
            long v = 0, dflt = 0;
            bpmf_get_option(os.name[i], &v, &dflt);
            bpmf_set_option(os.name[i], dflt);
        }
    }
    printf("bp_plan_host_check: %ld plans, %ld schedules, all invariants hold\n", g_plans, g_schedules);
    return 0;
}
