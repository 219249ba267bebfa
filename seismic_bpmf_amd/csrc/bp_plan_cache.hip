// The plan cache of bpmf_bp_run: see bp_plan_cache.h.  Host code only, no HIP call.
#include "bp_plan_cache.h"

#include <algorithm>
#include <cstring>

namespace bpmf {
namespace {
// 64-bit multiply-xorshift over the bytes of a table, 8 at a time (not cryptographic: a cache key)
uint64_t hash_words(const void* p, size_t bytes, uint64_t seed)
{
    const unsigned char* b = (const unsigned char*)p;
    uint64_t h = seed ^ (bytes * 0x9e3779b97f4a7c15ull);
    size_t i = 0;
    for (; i + 8 <= bytes; i += 8) {
        uint64_t w;
        memcpy(&w, b + i, 8);
        h = (h ^ w) * 0xff51afd7ed558ccdull;
        h ^= h >> 32;
    }
    uint64_t w = 0;
    if (i < bytes) memcpy(&w, b + i, bytes - i);
    h = (h ^ w) * 0xc4ceb9fe1a85ec53ull;
    return h ^ (h >> 29);
}
// Tables small enough to be kept are COMPARED on a hit: their keys only pre-select, and hash one 8-byte word in 64
// -- 24 MB of hashing per cfg3 call were 4 ms of a 160 ms call; larger tables are hashed in full, twice.
uint64_t table_hash(const void* p, size_t bytes, uint64_t seed, bool sampled)
{
    if (!sampled || bytes < 4096) return hash_words(p, bytes, seed);
    uint64_t h = seed ^ bytes;
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i + 8 <= bytes; i += 512) {
        uint64_t w8;
        memcpy(&w8, b + i, 8);
        h = (h ^ w8) * 0xff51afd7ed558ccdull;
        h ^= h >> 32;
    }
    return h ^ hash_words(b + bytes - 64, 64, seed);
}
}  // namespace

BpPlanCache::~BpPlanCache()
{
    for (Entry& e : entries_)
        if (e.plan) destroy_(e.plan);
}

size_t BpPlanCache::capacity() const
{
    return (size_t)std::max(4, 2 * std::max(1, device_count_()));
}

size_t BpPlanCache::held() const
{
    std::lock_guard<std::mutex> g(mutex_);
    size_t n = 0;
    for (const Entry& e : entries_) n += e.plan != nullptr;
    return n;
}

void* BpPlanCache::take(int device, size_t K, size_t S, size_t P, const int32_t* moveouts, const float* w_sources,
                        uint64_t option_generation, Ticket* t)
{
    const size_t b_mv = K * S * P * sizeof(int32_t), b_ws = K * S * sizeof(float);
    const bool keep = b_mv + b_ws <= KEEP_BYTES;
    *t = Ticket();
    t->K = K; t->S = S; t->P = P; t->device = device;
    t->key = table_hash(moveouts, b_mv, 0x9e3779b97f4a7c15ull ^ (K * 31 + S * 7 + P), keep) ^
             table_hash(w_sources, b_ws, 0xc2b2ae3d27d4eb4full, keep) ^ (option_generation * 0xd6e8feb86659fd93ull);
    t->key2 = keep ? t->key * 0x9e3779b97f4a7c15ull
                   : hash_words(moveouts, b_mv, 0x165667b19e3779f9ull) + hash_words(w_sources, b_ws, 0x27d4eb2f165667c5ull);
    std::lock_guard<std::mutex> g(mutex_);
    for (size_t i = 0; i < entries_.size(); ++i) {
        Entry& e = entries_[i];
        if (!e.plan || e.key != t->key || e.key2 != t->key2 || e.K != K || e.S != S || e.P != P || e.device != device)
            continue;
        if (!e.mv.empty() && (memcmp(e.mv.data(), moveouts, b_mv) != 0 || memcmp(e.ws.data(), w_sources, b_ws) != 0))
            continue;
        void* plan = e.plan;
        e.plan = nullptr;
        e.reserved = true;
        t->slot = (int)i;
        return plan;
    }
    return nullptr;
}

void BpPlanCache::give_back(const Ticket& t, void* plan, const int32_t* moveouts, const float* w_sources)
{
    std::lock_guard<std::mutex> g(mutex_);
    if (t.slot >= 0) {                          // the slot this plan came from still holds its tables
        Entry& e = entries_[(size_t)t.slot];
        e.plan = plan;
        e.reserved = false;
        e.stamp = ++clock_;
        return;
    }
    Entry* slot = nullptr;
    for (Entry& e : entries_)
        if (!e.plan && !e.reserved) { slot = &e; break; }
    if (!slot && entries_.size() < capacity()) {
        entries_.emplace_back();
        slot = &entries_.back();
    }
    if (!slot) {
        for (Entry& e : entries_)
            if (e.plan && e.device == t.device && (!slot || e.stamp < slot->stamp)) slot = &e;
        if (!slot) {
            destroy_(plan);
            return;
        }
        destroy_(slot->plan);
    }
    slot->key = t.key; slot->key2 = t.key2;
    slot->K = t.K; slot->S = t.S; slot->P = t.P;
    slot->device = t.device;
    slot->plan = plan;
    slot->stamp = ++clock_;
    if (t.K * t.S * t.P * sizeof(int32_t) + t.K * t.S * sizeof(float) <= KEEP_BYTES) {
        slot->mv.assign(moveouts, moveouts + t.K * t.S * t.P);
        slot->ws.assign(w_sources, w_sources + t.K * t.S);
    } else {
        slot->mv.clear(); slot->mv.shrink_to_fit();
        slot->ws.clear(); slot->ws.shrink_to_fit();
    }
}

}  // namespace bpmf
