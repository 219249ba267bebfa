// Host-only check of the plan cache of bpmf_bp_run (csrc/bp_plan_cache.hip) under sanitizers: fake plans (counted
// allocations) on small tables (K <= 64, S <= 8, P <= 2) through a sequence that reaches a hit, a miss, equal keys with
// different tables, the return into the reserved slot, growth to capacity, LRU eviction on one device while another
// device's plans stay, a cache full of other devices' plans, and a change of the option generation.  Every fake plan
// is destroyed exactly once or still held.  Needs no GPU and loads nothing into another process.  From the repository
// root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/bp_plan_cache_host_check.hip \
//         seismic_bpmf_amd/csrc/bp_plan_cache.hip -o /tmp/bp_plan_cache_host_check \
//     && /tmp/bp_plan_cache_host_check
#include "../seismic_bpmf_amd/csrc/bp_plan_cache.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

using bpmf::BpPlanCache;

namespace {

#define REQUIRE(cond)                                                                 \
    do {                                                                              \
        if (!(cond)) {                                                                \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond);         \
            abort();                                                                  \
        }                                                                             \
    } while (0)

struct FakePlan { long id; };
long g_created = 0, g_destroyed = 0;
std::set<long> g_live;
int g_devices = 2;

void* make_plan()
{
    FakePlan* p = new FakePlan{g_created++};
    g_live.insert(p->id);
    return p;
}
void destroy_plan(void* plan)
{
    FakePlan* p = (FakePlan*)plan;
    REQUIRE(g_live.erase(p->id) == 1);        // exactly once
    ++g_destroyed;
    delete p;
}
int device_count() { return g_devices; }

struct Table {
    size_t K, S, P;
    std::vector<int32_t> mv;
    std::vector<float> ws;
};
Table make_table(size_t K, size_t S, size_t P, int seed)
{
    Table t{K, S, P, std::vector<int32_t>(K * S * P), std::vector<float>(K * S)};
    for (size_t i = 0; i < t.mv.size(); ++i) t.mv[i] = (int32_t)((i * 37 + (size_t)seed * 101) % 211) - 50;
    for (size_t i = 0; i < t.ws.size(); ++i) t.ws[i] = (float)((i + (size_t)seed) % 5) * 0.25f;
    return t;
}

struct Taken { bool hit; long id; BpPlanCache::Ticket ticket; void* plan; };
// the first half of a call: the cached plan or a new one
Taken take(BpPlanCache& c, int device, const Table& t, uint64_t generation)
{
    Taken r;
    r.plan = c.take(device, t.K, t.S, t.P, t.mv.data(), t.ws.data(), generation, &r.ticket);
    r.hit = r.plan != nullptr;
    REQUIRE(r.hit == (r.ticket.slot >= 0));
    if (!r.plan) r.plan = make_plan();
    r.id = ((FakePlan*)r.plan)->id;
    return r;
}
void give_back(BpPlanCache& c, const Taken& r, const Table& t) { c.give_back(r.ticket, r.plan, t.mv.data(), t.ws.data()); }
// a whole call
Taken call(BpPlanCache& c, int device, const Table& t, uint64_t generation)
{
    const Taken r = take(c, device, t, generation);
    give_back(c, r, t);
    return r;
}
void check_counts(const BpPlanCache& c, size_t held)
{
    REQUIRE(c.held() == held);
    REQUIRE((size_t)(g_created - g_destroyed) == held && g_live.size() == held);
}

}  // namespace

int main()
{
    {
        BpPlanCache cache(destroy_plan, device_count);
        REQUIRE(cache.capacity() == 4);                       // max(4, 2 x 2 devices)
        // 4096 bytes of moveouts: the size from which the key samples one word in 64
        const Table A = make_table(64, 8, 2, 1), B = make_table(5, 3, 1, 2);
        REQUIRE(A.mv.size() * sizeof(int32_t) == 4096);

        // a miss, then hits; the plan comes back into the slot that stayed reserved for it
        const Taken a0 = call(cache, 0, A, 1);
        REQUIRE(!a0.hit);
        check_counts(cache, 1);
        for (int i = 0; i < 2; ++i) {
            const Taken a = take(cache, 0, A, 1);
            REQUIRE(a.hit && a.id == a0.id && a.ticket.slot == 0);
            REQUIRE(cache.held() == 0);                       // taken out while in use
            give_back(cache, a, A);
            check_counts(cache, 1);
        }
        // the same tables on another device: a miss
        const Taken d1 = call(cache, 1, A, 1);
        REQUIRE(!d1.hit);
        check_counts(cache, 2);

        // equal keys, different tables (a word the sampled key does not read): a miss while the tables are kept
        Table A2 = A;
        A2.mv[5] += 1;
        const Taken a2 = call(cache, 0, A2, 1);
        REQUIRE(a2.ticket.key == a0.ticket.key && a2.ticket.key2 == a0.ticket.key2);
        REQUIRE(!a2.hit && a2.id != a0.id);
        check_counts(cache, 3);
        REQUIRE(call(cache, 0, A2, 1).id == a2.id && call(cache, 0, A, 1).id == a0.id);      // each finds its own

        // another option generation: a miss; the cache is at its capacity now
        const Taken g2 = call(cache, 0, A, 2);
        REQUIRE(!g2.hit && g2.ticket.key != a0.ticket.key);
        check_counts(cache, 4);
        REQUIRE(call(cache, 0, A, 1).id == a0.id && g_destroyed == 0);

        // full: a new plan of device 0 takes the slot of device 0's least recently used plan (A2, then generation 2);
        // device 1's plan stays
        const Taken b0 = call(cache, 0, B, 1);
        REQUIRE(!b0.hit && g_destroyed == 1 && !g_live.count(a2.id));
        check_counts(cache, 4);
        REQUIRE(call(cache, 1, A, 1).id == d1.id && call(cache, 0, A, 1).id == a0.id);
        REQUIRE(!call(cache, 0, A2, 1).hit && g_destroyed == 2 && !g_live.count(g2.id));
        REQUIRE(call(cache, 0, B, 1).id == b0.id);
        check_counts(cache, 4);

        // a cache full of other devices' plans: the plan is destroyed, not cached
        for (int i = 0; i < 2; ++i) {
            const Taken x = call(cache, 2, B, 1);
            REQUIRE(!x.hit && !g_live.count(x.id) && g_destroyed == 3 + i);
            check_counts(cache, 4);
        }

        // a slot reserved for a plan in use is not handed to somebody else's plan
        {
            const Taken a = take(cache, 0, A, 1);
            REQUIRE(a.hit && a.id == a0.id && cache.held() == 3);
            const Taken b1 = call(cache, 1, B, 1);            // (device 1's only plan goes instead)
            REQUIRE(!b1.hit && g_destroyed == 5 && !g_live.count(d1.id) && cache.held() == 3);
            give_back(cache, a, A);
            check_counts(cache, 4);
            REQUIRE(call(cache, 0, A, 1).id == a0.id && call(cache, 1, B, 1).id == b1.id);
        }

        // more devices: the cache grows to the new capacity without destroying anything, then evicts again
        g_devices = 4;
        REQUIRE(cache.capacity() == 8);
        long first = -1;
        for (int i = 0; i < 4; ++i) {
            const Taken t = call(cache, 3, make_table(1 + (size_t)i, 2, 2, 3), 1);
            REQUIRE(!t.hit && g_destroyed == 5);
            if (i == 0) first = t.id;
            check_counts(cache, 5 + (size_t)i);
        }
        REQUIRE(!call(cache, 3, make_table(7, 2, 2, 3), 1).hit && g_destroyed == 6 && !g_live.count(first));
        check_counts(cache, 8);
        g_devices = 0;                                        // (no device visible counts as one)
        REQUIRE(cache.capacity() == 4);
    }
    // the cache is gone and has destroyed what it held
    REQUIRE(g_created == g_destroyed && g_live.empty());
    printf("bp_plan_cache_host_check: %ld fake plans, each destroyed exactly once\n", g_created);
    return 0;
}
