// The plans bpmf_bp_run keeps from one call to the next, keyed by (device, shapes, both tables, option generation).
// BPMF calls beamform once per day with the same moveout table and source weights (template_search.py:549-558);
// building the plan costs 0.04 s for 50 000 sources but 3 s for a million, so the last plans are kept.
//
// A hit compares the tables themselves (host copies are kept while they are small; above 1 GiB a second,
// independent 64-bit hash stands in).  A plan is TAKEN OUT while a call uses it and its slot stays reserved for it;
// give_back() returns it there, or finds a place for a new plan: a free slot, a new slot while there are fewer than
// max(4, 2 x devices) -- one per visible device and one spare each, so that a process driving every GPU of a node
// keeps all of its plans from one day to the next -- or the slot of the least recently used plan OF THE SAME DEVICE
// (that device's calls are serialised by its context mutex, which the caller holds, so nobody can be about to take
// it); a cache filled by other devices' plans is left alone and the plan is destroyed.
//
// The cache sees a plan as an opaque pointer and a destroy function and makes no HIP call: it links and runs
// without a device (tools/bp_plan_cache_host_check.hip).
#pragma once
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>

namespace bpmf {

class BpPlanCache {
public:
    using Destroy = void (*)(void* plan);
    using DeviceCount = int (*)();              // visible devices (the capacity follows it; < 1 counts as 1)
    static constexpr size_t KEEP_BYTES = (size_t)1 << 30;      // tables up to this size are kept and compared

    // what take() found out about the call's tables, for give_back()
    struct Ticket {
        uint64_t key = 0, key2 = 0;
        size_t K = 0, S = 0, P = 0;
        int device = 0;
        int slot = -1;                          // the reserved slot of a hit; -1 after a miss
    };

    BpPlanCache(Destroy destroy, DeviceCount device_count) : destroy_(destroy), device_count_(device_count) {}
    ~BpPlanCache();                             // destroys the plans it holds
    BpPlanCache(const BpPlanCache&) = delete;
    BpPlanCache& operator=(const BpPlanCache&) = delete;

    // The plan of these tables on `device`, taken out of its slot (nullptr: none, the caller builds one).  The
    // option generation is part of the key: a plan is built under the options of its creation, and a changed
    // option must not leave a plan of the previous settings in use.
    void* take(int device, size_t K, size_t S, size_t P, const int32_t* moveouts, const float* w_sources,
               uint64_t option_generation, Ticket* ticket);
    // The second half: `plan` (taken or newly built for the tables of `ticket`) goes back or is destroyed.
    void give_back(const Ticket& ticket, void* plan, const int32_t* moveouts, const float* w_sources);

    size_t held() const;                        // plans in the cache right now
    size_t capacity() const;

private:
    struct Entry {
        uint64_t key = 0, key2 = 0;
        size_t K = 0, S = 0, P = 0;
        int device = 0;
        std::vector<int32_t> mv;                // empty: table too large to keep, (key, key2) decide
        std::vector<float> ws;
        void* plan = nullptr;
        bool reserved = false;                  // its plan is in use by a call and comes back into this slot
        uint64_t stamp = 0;                     // last use (eviction = least recently used)
    };
    Destroy destroy_;
    DeviceCount device_count_;
    mutable std::mutex mutex_;
    std::vector<Entry> entries_;                // never shrinks: a ticket's slot index stays valid
    uint64_t clock_ = 0;
};

}  // namespace bpmf
