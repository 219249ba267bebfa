// Backprojection, the host side of a plan (no kernel, no HIP call, no device): the LDS plan of the general
// kernels and of the station-count classes of bp_fast.hip for one moveout table (bp_plan_host), and the schedule
// of one run on such a plan (bp_schedule): path, general kernel, group ranges per tile, interior range, layout of
// the workspace.  bp.hip uploads the one (bp_plan_upload) and launches along the other; bpmf_bp_launch_info shows
// both without a device.
#include "bp_plan.h"

#include <algorithm>
#include <cstring>
#include <exception>
#include <vector>

using namespace bpmf;

// ----------------------------------------------------------------------- plan ---
namespace {

// Processing order: recursive median bisection of the sources on the moveout column with
// the largest spread (a kd-tree walk), so that consecutive sources have similar moveouts
// on every station and a group's LDS windows stay short.
void bisect_order(const int32_t* mv, size_t SP, std::vector<int>& idx, size_t lo, size_t hi,
                  size_t leaf)
{
    if (hi - lo <= leaf) return;
    size_t best_col = 0;
    long long best_range = -1;
    for (size_t c = 0; c < SP; ++c) {
        int mn = mv[(size_t)idx[lo] * SP + c], mx = mn;
        for (size_t i = lo + 1; i < hi; ++i) {
            const int v = mv[(size_t)idx[i] * SP + c];
            mn = std::min(mn, v);
            mx = std::max(mx, v);
        }
        if ((long long)mx - mn > best_range) { best_range = (long long)mx - mn; best_col = c; }
    }
    if (best_range <= 0) return;
    const size_t mid = lo + (hi - lo) / 2;
    std::nth_element(idx.begin() + lo, idx.begin() + mid, idx.begin() + hi, [&](int a, int b) {
        const int va = mv[(size_t)a * SP + best_col], vb = mv[(size_t)b * SP + best_col];
        return va < vb || (va == vb && a < b);
    });
    bisect_order(mv, SP, idx, lo, mid, leaf);
    bisect_order(mv, SP, idx, mid, hi, leaf);
}

// Extreme moveouts of one source for the strict bound test and the number of its used (station, phase)
// terms: over the WEIGHTED stations (the build's convention, oracle/bpmf_oracle.c:bp_cpu), or -- option
// bp.compat_range_all_stations -- over all stations of a source that has at least one weighted station.
int source_tau_range(const int32_t* mv, const float* ws, size_t k, size_t S, size_t P, bool all_stations,
                     long long& lo, long long& hi)
{
    int n = 0;
    bool seen = false;
    lo = hi = 0;
    for (size_t s = 0; s < S; ++s) {
        const bool used = ws[k * S + s] != 0.0f;
        if (used) n += (int)P;
        else if (!all_stations) continue;
        for (size_t p = 0; p < P; ++p) {
            const long long tau = mv[(k * S + s) * P + p];
            if (!seen || tau < lo) lo = tau;
            if (!seen || tau > hi) hi = tau;
            seen = true;
        }
    }
    if (n == 0) lo = hi = 0;
    return n;
}

// Greedy grouping of consecutive sources (in processing order): a group is closed when the
// next source would push the LDS need (zero slab + sum over used rows of tile + moveout
// spread) past the soft budget.  Returns false if one source alone exceeds `hard_floats`.
// dual: every window is staged twice, the second copy shifted by one sample, both at even
// offsets; a term whose offset into the window is odd reads the shifted copy, so that ALL emitted
// offsets are even (8-byte aligned pairs for the ds_read_b64 kernel).
// `order_in`: the sources of this plan in processing order (all of them, or one station-count class).
bool build_plan(const int32_t* mv, const float* ws, const std::vector<int>& order_in, size_t S, size_t P,
                bool all_stations, int tile, int chunk, size_t soft_floats, const size_t hard_floats, int max_group,
                int32_t id_offset, bool dual, PlanHost& ph)
{
    // a window is staged in 16-byte lanes: its length is rounded up to a multiple of 4 floats
    // (the extra samples are real data or zero fill, never addressed by a term)
    auto row_len = [&](int spread) -> size_t { return ((size_t)tile + (size_t)spread + 3) & ~(size_t)3; };
    auto row_cost = [&](int spread) -> size_t { return dual ? 2 * row_len(spread) : row_len(spread); };
    const size_t SP = S * P;
    std::vector<int> order = order_in;
    const size_t K = order.size();
    // the zero slab: one tile of the generic kernels, a fixed 512 floats in front of the
    // descriptor slab of the dual plans (bp_fast.hip, any tile)
    const size_t zero_slab = dual ? (size_t)BPF_ZERO_SLAB : (size_t)tile;

    size_t max_terms = 1;
    ph.srcs.resize(K);
    auto src_of = [&](size_t k) {
        long long lo = 0, hi = 0;
        const int n = source_tau_range(mv, ws, k, S, P, all_stations, lo, hi);
        max_terms = std::max(max_terms, (size_t)n);
        return BpSource{(int)((long long)k + id_offset), (int)lo, (int)hi,
                        (n + chunk - 1) / chunk * chunk};
    };
    for (size_t q = 0; q < K; ++q) ph.srcs[q] = src_of((size_t)order[q]);
    const int NT = (int)((max_terms + chunk - 1) / chunk * chunk);
    ph.NT = NT;
    // A source's own windows (terms x tile + the zero slab) must leave room for the moveout
    // spread of a useful group.  When they do not even fit the soft budget with 16 samples of
    // spread per row (dense station weights), use the whole LDS (one workgroup per CU) instead of
    // degenerating to one source per group.  (Measured on cfg3 geometry, 10 / 15 / 20 used
    // stations: 0.35 / 0.64 / 0.91 s.)
    // dual plans (bp_fast.hip) keep 4 KB behind the zero slab for the next group's window descriptors
    // (16 bytes per window; a group has at most 2 S P windows)
    const size_t slab_extra = dual ? (size_t)4 * std::min<size_t>(BPF_DESC_MAX, (2 * S * P + 63) / 64 * 64) : 0;
    const size_t base_need = zero_slab + slab_extra + max_terms * row_cost(0);
    // More than 16 stations (P = 2: 32 terms): the packed kernel runs one 16-wave workgroup per CU.
    if (base_need + max_terms * (row_cost(16) - row_cost(0)) > soft_floats || (P == 2 && max_terms > 32))
        soft_floats = hard_floats;
    ph.off.assign(K * (size_t)NT, 0);       // padded terms read the zero slab at offset 0
    ph.beta.assign(K * (size_t)NT, 0.0f);

    std::vector<int> gmin(SP), gmax(SP), base(SP);
    std::vector<char> used(SP);
    struct RowUpdate { size_t row; int lo, hi; };
    std::vector<RowUpdate> upd;
    upd.reserve(SP);
    size_t first = 0;
    while (first < K) {
        std::fill(used.begin(), used.end(), 0);
        size_t need = zero_slab + slab_extra, q = first;  // the zero slab (+ the descriptor slab)
        for (; q < K && (int)(q - first) < max_group; ++q) {
            const size_t k = (size_t)order[q];
            size_t need2 = need;
            upd.clear();
            for (size_t s = 0; s < S; ++s) {
                if (ws[k * S + s] == 0.0f) continue;
                for (size_t p = 0; p < P; ++p) {
                    const size_t r = s * P + p;
                    const int tau = mv[(k * S + s) * P + p];
                    int lo = tau, hi = tau;
                    if (used[r]) {
                        lo = std::min(lo, gmin[r]);
                        hi = std::max(hi, gmax[r]);
                        need2 += row_cost(hi - lo) - row_cost(gmax[r] - gmin[r]);
                    } else {
                        need2 += row_cost(0);
                    }
                    upd.push_back(RowUpdate{r, lo, hi});
                }
            }
            const size_t limit = (q == first) ? hard_floats : soft_floats;
            if (need2 > limit) {
                if (q == first) return false;
                break;
            }
            for (const RowUpdate& u : upd) {
                used[u.row] = 1;
                gmin[u.row] = u.lo;
                gmax[u.row] = u.hi;
            }
            need = need2;
        }
        // close group [first, q): lay the windows out after the zero slab, cut them in chunks
        BpGroup g{(int)first, (int)(q - first), (int)ph.chunks.size(), 0};
        size_t o = zero_slab + slab_extra;
        for (size_t r = 0; r < SP; ++r) {
            base[r] = -1;
            if (!used[r]) continue;
            const int len = (int)row_len(gmax[r] - gmin[r]);
            base[r] = (int)o;
            for (int x0 = 0; x0 < len; x0 += BP_THREADS)
                ph.chunks.push_back(BpChunk{(int)r, gmin[r] + x0, (int)o + x0,
                                            std::min(BP_THREADS, len - x0)});
            if (dual) {  // the copy shifted by one sample, right behind (both bases multiples of 4)
                for (int x0 = 0; x0 < len; x0 += BP_THREADS)
                    ph.chunks.push_back(BpChunk{(int)r, gmin[r] + 1 + x0, (int)o + len + x0,
                                                std::min(BP_THREADS, len - x0)});
            }
            o += row_cost(gmax[r] - gmin[r]);
        }
        g.n_chunk = (int)ph.chunks.size() - g.first_chunk;
        ph.lds_floats = std::max(ph.lds_floats, o);
        if (dual) {  // ascending ids inside the group (see GLOCAL in bp_beam_wps2_kernel)
            std::sort(order.begin() + first, order.begin() + q);
            for (size_t qq = first; qq < q; ++qq) ph.srcs[qq] = src_of((size_t)order[qq]);
        }
        for (size_t qq = first; qq < q; ++qq) {
            const size_t k = (size_t)order[qq];
            size_t j = 0;
            for (size_t s = 0; s < S; ++s) {
                if (ws[k * S + s] == 0.0f) continue;
                for (size_t p = 0; p < P; ++p, ++j) {
                    const size_t r = s * P + p;
                    const int rel = mv[(k * S + s) * P + p] - gmin[r];
                    if (dual && (rel & 1))
                        ph.off[qq * NT + j] = base[r] + (int)row_len(gmax[r] - gmin[r]) + rel - 1;
                    else
                        ph.off[qq * NT + j] = base[r] + rel;
                    ph.beta[qq * NT + j] = ws[k * S + s];
                }
            }
        }
        ph.groups.push_back(g);
        first = q;
    }
    return true;
}

// Multi-residency plan (bp_fast.hip, HALVES): dual windows at `tile`, groups of at most `max_group`
// sources, the weighted stations of every source dealt to residencies of `per` stations each (in
// station order: the first `per`, the next `per`, ...); a group is closed when any residency's windows
// would exceed `hard_floats` of LDS.  Every group becomes ph.n_pass consecutive entries of ph.groups
// (same sources, the chunks of one residency each); ph.off holds the offsets of a source's terms inside
// the residency they belong to.
bool build_plan_halves(const int32_t* mv, const float* ws, const std::vector<int>& order_in, size_t S, size_t P,
                       bool all_stations, int tile, int chunk, const size_t hard_floats, int max_group, int32_t id_offset,
                       int per, int n_pass, int slots, PlanHost& ph)
{
    auto row_len = [&](int spread) -> size_t { return ((size_t)tile + (size_t)spread + 3) & ~(size_t)3; };
    auto row_cost = [&](int spread) -> size_t { return 2 * row_len(spread); };
    const size_t SP = S * P;
    std::vector<int> order = order_in;
    const size_t K = order.size();
    const size_t zero_slab = (size_t)BPF_ZERO_SLAB;
    const size_t slab_extra = (size_t)4 * std::min<size_t>(BPF_DESC_MAX, (2 * S * P + 63) / 64 * 64);
    size_t max_terms = 1;
    ph = PlanHost();
    ph.n_pass = n_pass;
    ph.per = per;
    ph.slots = slots;
    ph.srcs.resize(K);
    auto src_of = [&](size_t k) {
        long long lo = 0, hi = 0;
        const int n = source_tau_range(mv, ws, k, S, P, all_stations, lo, hi);
        max_terms = std::max(max_terms, (size_t)n);
        return BpSource{(int)((long long)k + id_offset), (int)lo, (int)hi, (n + chunk - 1) / chunk * chunk};
    };
    for (size_t q = 0; q < K; ++q) ph.srcs[q] = src_of((size_t)order[q]);
    if (max_terms > (size_t)per * n_pass * P) return false;
    const int NT = (int)((max_terms + chunk - 1) / chunk * chunk);
    ph.NT = NT;
    ph.off.assign(K * (size_t)NT, 0);
    ph.beta.assign(K * (size_t)NT, 0.0f);
    std::vector<std::vector<int>> gmin(n_pass, std::vector<int>(SP)), gmax(n_pass, std::vector<int>(SP)),
        base(n_pass, std::vector<int>(SP));
    std::vector<std::vector<char>> used(n_pass, std::vector<char>(SP));
    struct RowUpdate { int h; size_t row; int lo, hi; };
    std::vector<RowUpdate> upd;
    std::vector<size_t> need(n_pass), need2(n_pass);
    size_t first = 0;
    while (first < K) {
        for (int h = 0; h < n_pass; ++h) {
            std::fill(used[h].begin(), used[h].end(), 0);
            need[h] = zero_slab + slab_extra;
        }
        size_t q = first;
        for (; q < K && (int)(q - first) < max_group; ++q) {
            const size_t k = (size_t)order[q];
            need2 = need;
            upd.clear();
            int ord = 0;
            for (size_t s = 0; s < S; ++s) {
                if (ws[k * S + s] == 0.0f) continue;
                const int h = ord / per;
                ++ord;
                for (size_t p = 0; p < P; ++p) {
                    const size_t r = s * P + p;
                    const int tau = mv[(k * S + s) * P + p];
                    int lo = tau, hi = tau;
                    if (used[h][r]) {
                        lo = std::min(lo, gmin[h][r]);
                        hi = std::max(hi, gmax[h][r]);
                        need2[h] += row_cost(hi - lo) - row_cost(gmax[h][r] - gmin[h][r]);
                    } else {
                        need2[h] += row_cost(0);
                    }
                    upd.push_back(RowUpdate{h, r, lo, hi});
                    // (a row may appear in several residencies of a GROUP -- different sources count a
                    // station differently -- but only once per residency)
                }
            }
            bool fits = true;
            for (int h = 0; h < n_pass; ++h) fits = fits && need2[h] <= hard_floats;
            if (!fits) {
                if (q == first) return false;
                break;
            }
            for (const RowUpdate& u : upd) {
                used[u.h][u.row] = 1;
                gmin[u.h][u.row] = u.lo;
                gmax[u.h][u.row] = u.hi;
            }
            need = need2;
        }
        std::sort(order.begin() + first, order.begin() + q);          // ascending ids inside the group
        for (size_t qq = first; qq < q; ++qq) ph.srcs[qq] = src_of((size_t)order[qq]);
        for (int h = 0; h < n_pass; ++h) {
            BpGroup g{(int)first, (int)(q - first), (int)ph.chunks.size(), 0};
            size_t o = zero_slab + slab_extra;
            for (size_t r = 0; r < SP; ++r) {
                base[h][r] = -1;
                if (!used[h][r]) continue;
                const int len = (int)row_len(gmax[h][r] - gmin[h][r]);
                base[h][r] = (int)o;
                for (int x0 = 0; x0 < len; x0 += BP_THREADS)
                    ph.chunks.push_back(BpChunk{(int)r, gmin[h][r] + x0, (int)o + x0, std::min(BP_THREADS, len - x0)});
                for (int x0 = 0; x0 < len; x0 += BP_THREADS)
                    ph.chunks.push_back(BpChunk{(int)r, gmin[h][r] + 1 + x0, (int)o + len + x0, std::min(BP_THREADS, len - x0)});
                o += row_cost(gmax[h][r] - gmin[h][r]);
            }
            g.n_chunk = (int)ph.chunks.size() - g.first_chunk;
            ph.lds_floats = std::max(ph.lds_floats, o);
            ph.groups.push_back(g);
        }
        for (size_t qq = first; qq < q; ++qq) {
            const size_t k = (size_t)order[qq];
            size_t j = 0;
            int ord = 0;
            for (size_t s = 0; s < S; ++s) {
                if (ws[k * S + s] == 0.0f) continue;
                const int h = ord / per;
                ++ord;
                for (size_t p = 0; p < P; ++p, ++j) {
                    const size_t r = s * P + p;
                    const int rel = mv[(k * S + s) * P + p] - gmin[h][r];
                    ph.off[qq * NT + j] = (rel & 1) ? base[h][r] + (int)row_len(gmax[h][r] - gmin[h][r]) + rel - 1
                                                    : base[h][r] + rel;
                    ph.beta[qq * NT + j] = ws[k * S + s];
                }
            }
        }
        first = q;
    }
    return true;
}

// ---- interior-tile fast path: host-side tables of one station-count class (bp_fast.hip) ----
// A source of `n` (even-padded) stations as `nparts` records of `tp` stations for the kernel of
// this tile: the smallest padded total + 2 per part, then the fewest parts.  Part sizes the kernels instantiate:
// tile 512: 4..16 even, one part; tile 256: 6..16 even; tile 128: 8, 12, 16, 20, 24.
bool fast_parts(int n, int tile, int& tp, int& nparts)
{
    static const int t512[] = {4, 6, 8, 10, 12, 14, 16}, t256[] = {6, 8, 10, 12, 14, 16}, t128[] = {8, 12, 16, 20, 24};
    const int* opts = tile == 512 ? t512 : (tile == 256 ? t256 : t128);
    const int n_opts = tile == 512 ? 7 : (tile == 256 ? 6 : 5);
    // A part boundary costs about as much as two stations at tiles 512 / 256 (header, refill
    // pipeline restart).  At tile 128 a unit is a whole quad of the record and the distance between
    // the request of a quad and its first use is (quads per part - 3) units: short parts stall on
    // the record loads (5 parts of 8 stations: 0.26 of the gather rate at cfg5's share) -- prefer
    // the longest parts.
    const int part_cost = tile == 128 ? 8 : 2;
    int best_total = 1 << 30;
    tp = 0;
    nparts = 0;
    for (int i = 0; i < n_opts; ++i) {
        const int k = std::max(1, (n + opts[i] - 1) / opts[i]);
        if (tile == 512 && k > 1) continue;
        if (k > 16) continue;
        const int total = k * opts[i] + part_cost * k;
        if (total < best_total || (total == best_total && k < nparts)) {
            best_total = total;
            tp = opts[i];
            nparts = k;
        }
    }
    return tp != 0;
}

// Relative time per time sample of the interior kernel on this plan: every group pays one staging
// round (two barriers, the window copies: ~6000 cycles measured at cfg3), every source its gathers
// (64 lanes x 8 bytes per ds_read_b64 at ~0.7 x 256 B/clk/CU, a little less on the small tiles,
// whose units carry more address arithmetic per byte), all of it amortised over `tile` samples.
double plan_cost(const PlanHost& ph, int tile)
{
    const double eff = tile == 512 ? 0.70 : (tile == 256 ? 0.66 : 0.40);   // (tile 128: measured 0.35 at 40 stations, VALU-bound)
    double cycles = 0.0;
    for (const BpGroup& g : ph.groups) {
        double terms = 0.0;
        for (int q = g.first_src; q < g.first_src + g.n_src; ++q) terms += ph.srcs[q].nterm;
        // an entry of a multi-residency plan is one residency: `per` stations of every source (padded
        // records), and a short group is padded to 16 x BPF_HALVES_SLOTS sources; ~8800 cycles between the
        // gathers of two entries were measured there (cfg5's share, 40 stations)
        if (ph.n_pass > 1) terms = 2.0 * ph.per * 16 * ph.slots;
        cycles += (ph.n_pass > 1 ? 8800.0 : 6000.0) + terms * (double)tile * 4.0 / (256.0 * eff);   // 4 gathered bytes per term and sample
    }
    return cycles / tile;
}

bool build_fast_host(const PlanHost& ph, int tile, bool allow_uniform, FastHost& fh)
{
    const int NT = ph.NT;
    fh = FastHost();
    fh.uniform = allow_uniform;
    int tp_max = 4;
    const size_t K = ph.srcs.size();
    std::vector<int> tp_of(K, 0), np_of(K, 0);
    for (size_t q = 0; q < K; ++q) {
        const BpSource& sr = ph.srcs[q];
        if (sr.nterm <= 0) continue;
        ++fh.n_sources;
        int tp, np;
        if (!fast_parts(sr.nterm / 2, tile, tp, np)) return false;
        tp_of[q] = tp;
        np_of[q] = np;
        tp_max = std::max(tp_max, tp);
        fh.max_sta = std::max(fh.max_sta, sr.nterm / 2);
        float w0 = 0.0f;
        for (int j = 0; j < NT; j += 2) {
            const float b = ph.beta[q * NT + j];
            if (b == 0.0f) continue;
            if (w0 == 0.0f) w0 = b;
            else if (b != w0) fh.uniform = false;
        }
    }
    if (fh.n_sources == 0) return false;
    const int rec_dw = (2 + 2 * tp_max + 3) / 4 * 4;
    fh.rec_dw = rec_dw;
    std::vector<int> members;
    for (const BpGroup& g : ph.groups) {
        // the group's staging chunks (pieces of <= 256 floats), merged back into whole windows
        BpFastGroup f{(int)fh.fr.size(), 0, (int)fh.fw.size(), 0};
        for (int c = g.first_chunk; c < g.first_chunk + g.n_chunk; ++c) {
            const BpChunk& ck = ph.chunks[c];
            if ((int)fh.fw.size() > f.first_win && fh.fw.back().row == ck.row &&
                fh.fw.back().gofs + fh.fw.back().len == ck.gofs && fh.fw.back().dst + fh.fw.back().len == ck.dst)
                fh.fw.back().len += ck.n;
            else
                fh.fw.push_back(BpWindow{ck.row, ck.gofs, ck.dst, ck.n});
        }
        f.n_win = (int)fh.fw.size() - f.first_win;
        if (f.n_win > BPF_DESC_MAX) return false;       // > 256 windows in a group: general kernel
        // runs of equal (tp, nparts), ascending id inside a run (the plan lists a group's sources by
        // ascending id); at most 16 x 16 combinations, most groups have one or two
        for (int np = 1; np <= 16; ++np) {
            for (int tp = 4; tp <= 24; tp += 2) {
                members.clear();
                for (int q = g.first_src; q < g.first_src + g.n_src; ++q)
                    if (tp_of[q] == tp && np_of[q] == np) members.push_back(q);
                if (members.empty()) continue;
                const size_t first_rec = fh.rec.size() / rec_dw;
                const size_t rounds = (members.size() + 15) / 16;
                fh.rec.resize(fh.rec.size() + rounds * np * 16 * rec_dw, 0);
                fh.fr.push_back(BpRun{(int)first_rec, (int)members.size(), tp, np});
                ++f.n_run;
                for (size_t m = 0; m < members.size(); ++m) {
                    const int q = members[m];
                    float w0 = 0.0f;
                    for (int j = 0; j < NT && w0 == 0.0f; j += 2) w0 = ph.beta[(size_t)q * NT + j];
                    for (int part = 0; part < np; ++part) {
                        const size_t r0 = (first_rec + ((m / 16) * np + part) * 16 + m % 16) * rec_dw;
                        fh.rec[r0] = ph.srcs[q].id;
                        fh.rec[r0 + 1] = fh.uniform ? __builtin_bit_cast(int, w0) : 0;
                        for (int i = 0; i < tp; ++i) {
                            const int st = part * tp + i;
                            const bool real = 2 * st + 1 < NT;  // beyond the term table: the zero slab, weight 0
                            const int oP = real ? ph.off[(size_t)q * NT + 2 * st] : 0;
                            const int oS = real ? ph.off[(size_t)q * NT + 2 * st + 1] : 0;
                            if (fh.uniform) {                   // LDS byte addresses of the two windows
                                fh.rec[r0 + 2 + 2 * i] = oP * 4;
                                fh.rec[r0 + 3 + 2 * i] = oS * 4;
                            } else {                            // {offs_P | offs_S << 16, weight}
                                fh.rec[r0 + 2 + 2 * i] = (int)((unsigned)oP | ((unsigned)oS << 16));
                                fh.rec[r0 + 3 + 2 * i] = real ? __builtin_bit_cast(int, ph.beta[(size_t)q * NT + 2 * st]) : 0;
                            }
                        }
                    }
                }
            }
        }
        fh.fg.push_back(f);
    }
    fh.rec.resize(fh.rec.size() + (size_t)17 * rec_dw, 0);        // one round of records (+ 1: whole s_load_dwordx8): the prefetch past the last part
    fh.fw.resize(fh.fw.size() + BPF_DESC_MAX, BpWindow{0, 0, 0, 0});   // the descriptor prefetch past the last group
    return true;
}

// Tables of a multi-residency class (build_plan_halves): per group ph.n_pass BpFastGroup entries, each
// with ONE run that lists all the group's sources (ascending id: wave w owns sources w, w + 16, ... in
// every residency -- the slots of the kernel's `carry` registers) as exactly two records of ph.per / 2
// stations.
bool build_fast_host_halves(const PlanHost& ph, FastHost& fh, bool allow_uniform)
{
    const int NT = ph.NT;
    fh = FastHost();
    fh.uniform = allow_uniform;
    const size_t K = ph.srcs.size();
    for (size_t q = 0; q < K; ++q) {
        const BpSource& sr = ph.srcs[q];
        if (sr.nterm <= 0) return false;                  // (sources without stations are not in this class)
        ++fh.n_sources;
        fh.max_sta = std::max(fh.max_sta, sr.nterm / 2);
        float w0 = 0.0f;
        for (int j = 0; j < NT; j += 2) {
            const float b = ph.beta[q * NT + j];
            if (b == 0.0f) continue;
            if (w0 == 0.0f) w0 = b;
            else if (b != w0) fh.uniform = false;
        }
    }
    const int tp = ph.per / 2, np = 2, WPB = 16, full = WPB * ph.slots;
    if ((tp != 6 && tp != 8 && tp != 10) || fh.n_sources == 0) return false;
    const int rec_dw = (2 + 2 * tp + 3) / 4 * 4;
    fh.rec_dw = rec_dw;
    for (size_t gi = 0; gi < ph.groups.size(); ++gi) {
        const BpGroup& g = ph.groups[gi];
        const int h = (int)(gi % (size_t)ph.n_pass);
        if (g.n_src > full) return false;
        const int flags = (h > 0 ? BPF_GROUP_LOAD : 0) | (h + 1 < ph.n_pass ? BPF_GROUP_STORE : 0);
        BpFastGroup f{(int)fh.fr.size(), 1 | flags, (int)fh.fw.size(), 0};
        for (int c = g.first_chunk; c < g.first_chunk + g.n_chunk; ++c) {
            const BpChunk& ck = ph.chunks[c];
            if ((int)fh.fw.size() > f.first_win && fh.fw.back().row == ck.row &&
                fh.fw.back().gofs + fh.fw.back().len == ck.gofs && fh.fw.back().dst + fh.fw.back().len == ck.dst)
                fh.fw.back().len += ck.n;
            else
                fh.fw.push_back(BpWindow{ck.row, ck.gofs, ck.dst, ck.n});
        }
        f.n_win = (int)fh.fw.size() - f.first_win;
        if (f.n_win > BPF_DESC_MAX) return false;
        const size_t first_rec = fh.rec.size() / rec_dw;
        // every wave walks exactly ph.slots sources (the kernel's slots are straight-line code):
        // a short group is padded with records of weight 0 at LDS offset 0 and id -1 (never a maximum)
        const size_t n = (size_t)g.n_src, rounds = (size_t)ph.slots;
        fh.rec.resize(fh.rec.size() + rounds * np * WPB * rec_dw, 0);
        fh.fr.push_back(BpRun{(int)first_rec, full, tp, np});
        for (size_t m = n; m < (size_t)full; ++m)
            for (int part = 0; part < np; ++part) fh.rec[(first_rec + ((m / WPB) * np + part) * WPB + m % WPB) * rec_dw] = -1;
        for (size_t m = 0; m < n; ++m) {
            const int q = g.first_src + (int)m;
            const int st_lo = h * ph.per, st_hi = std::min((h + 1) * ph.per, ph.srcs[q].nterm / 2);
            float w0 = 0.0f;
            for (int j = 0; j < NT && w0 == 0.0f; j += 2) w0 = ph.beta[(size_t)q * NT + j];
            for (int part = 0; part < np; ++part) {
                const size_t r0 = (first_rec + ((m / WPB) * np + part) * WPB + m % WPB) * rec_dw;
                fh.rec[r0] = ph.srcs[q].id;
                fh.rec[r0 + 1] = fh.uniform ? __builtin_bit_cast(int, w0) : 0;
                for (int i = 0; i < tp; ++i) {
                    const int st = st_lo + part * tp + i;
                    const bool real = st < st_hi && 2 * st + 1 < NT;    // beyond this residency: the zero slab, weight 0
                    const int oP = real ? ph.off[(size_t)q * NT + 2 * st] : 0;
                    const int oS = real ? ph.off[(size_t)q * NT + 2 * st + 1] : 0;
                    if (fh.uniform) {
                        fh.rec[r0 + 2 + 2 * i] = oP * 4;
                        fh.rec[r0 + 3 + 2 * i] = oS * 4;
                    } else {
                        fh.rec[r0 + 2 + 2 * i] = (int)((unsigned)oP | ((unsigned)oS << 16));
                        fh.rec[r0 + 3 + 2 * i] = real ? __builtin_bit_cast(int, ph.beta[(size_t)q * NT + 2 * st]) : 0;
                    }
                }
            }
        }
        fh.fg.push_back(f);
    }
    // one round of records behind the last one (the look-ahead past a wave's last part), and one more
    // record: the kernel fetches a record in whole s_load_dwordx8 (24 dwords where rec_dw is 20)
    fh.rec.resize(fh.rec.size() + (size_t)17 * rec_dw, 0);
    fh.fw.resize(fh.fw.size() + BPF_DESC_MAX, BpWindow{0, 0, 0, 0});
    return true;
}

}  // namespace

const char* bpmf::bp_plan_refusal(const int32_t* moveouts, const float* w_sources, size_t K, size_t S, size_t P)
{
    if (!moveouts || !w_sources || K == 0 || S == 0 || P == 0) return "bad argument";
    if (K > 0x7fffffffull || K * S * P > 0x7fffffffffull) return "grid too large";
    return nullptr;
}

BpPlanHost bpmf::bp_plan_host(const int32_t* moveouts, const float* w_sources, size_t K, size_t S, size_t P,
                              int32_t source_id_offset)
{
    // options (defaults chosen on MI355X)
    const size_t soft_kb = (size_t)std::max(8, (int)option(OPT_BP_LDS_KB));
    const int max_group = std::max(1, (int)option(OPT_BP_MAX_GROUP));
    const int tpt_first = (int)option(OPT_BP_TPT);
    const bool reorder = option(OPT_BP_REORDER) != 0;
    const bool verbose = option(OPT_BP_VERBOSE) != 0;
    const bool opt_dual = option(OPT_BP_DUAL) != 0, opt_fast = option(OPT_BP_FAST) != 0;
    const bool opt_uniform = option(OPT_BP_FAST_UNIFORM) != 0, opt_halves = option(OPT_BP_HALVES) != 0;
    const int forced_tile = (int)option(OPT_BP_FAST_TILE);
    const bool opt_direct = option(OPT_BP_DIRECT) != 0;
    const bool upper_only = option(OPT_BP_COMPAT_STRICT_UPPER_ONLY) != 0;
    const bool all_stations = option(OPT_BP_COMPAT_RANGE_ALL_STATIONS) != 0;
    const int chunk = 4;  // terms gathered side by side by the generic kernel (8 measured equal)
    const size_t hard = BP_LDS_MAX / sizeof(float);
    const size_t soft = std::min(hard, soft_kb * 1024 / sizeof(float));
    const size_t SP = S * P;

    BpPlanHost out;
    BpPlanShape& sh = out.shape;
    sh.K = K; sh.S = S; sh.P = P;
    sh.id_offset = source_id_offset;

    // weighted stations per source, extreme used moveouts of the grid
    std::vector<int> nsta(K, 0);
    int max_sta = 0, tmin_all = 0, tmax_all = 0;
    bool any_src = false;
    for (size_t k = 0; k < K; ++k) {
        long long lo = 0, hi = 0;
        const int n = source_tau_range(moveouts, w_sources, k, S, P, all_stations, lo, hi) / (int)P;
        if (n > 0) {
            if (!any_src || lo < tmin_all) tmin_all = (int)lo;
            if (!any_src || hi > tmax_all) tmax_all = (int)hi;
            any_src = true;
        }
        nsta[k] = n;
        max_sta = std::max(max_sta, n);
    }
    sh.tmin_all = tmin_all;
    sh.tmax_all = tmax_all;
    // option bp.compat_strict_upper_only: "strict" tests t + tau_max < N only and a used term in front of
    // sample 0 contributes nothing.  With every used moveout >= 0 (BPMF's tables: moveouts relative to the
    // first arrival, template_search.py:212-214) that IS the default; a table with a negative used moveout
    // takes the global-memory kernel of bp_direct.hip, the one that tests every term.
    const bool upper_only_direct = upper_only && any_src && tmin_all < 0;
    // processing order of the whole grid (kd-tree walk); a class keeps its members in this order
    std::vector<int> order(K);
    for (size_t k = 0; k < K; ++k) order[k] = (int)k;
    if (reorder) bisect_order(moveouts, SP, order, 0, K, 16);

    // ---- Two-phase grids: the ds_read_b64 kernel on dual windows (bp_fast.hip).  The sources are
    // sorted into classes by their number of weighted stations -- <= 16, 17..32, 33..64 -- and
    // every class gets the largest tile (512 / 256 / 128 samples) at which the dual windows of its
    // groups fit the LDS with the lowest modelled cost; one 17-station source no longer moves a
    // whole grid off the fast path, and dense 20- or 40-station weights run it on the small tiles.
    std::vector<ClassHost>& classes = out.classes;
    const bool want_dual = P == 2 && opt_dual && tpt_first == 2;
    if (want_dual && any_src && max_sta <= 64) {
        static const int bound[4] = {0, 16, 32, 64};
        static const int cand[3][3] = {{512, 256, 128}, {256, 128, 0}, {128, 0, 0}};
        bool ok = true;
        std::vector<int> members;
        for (int c = 0; c < 3 && ok; ++c) {
            members.clear();
            for (size_t q = 0; q < K; ++q) {
                const int n = nsta[order[q]];
                // sources without any station ride along with the first class when the whole grid is
                // one class (they are skipped by the kernels; the shared plan must list every source)
                if ((n > bound[c] && n <= bound[c + 1]) || (c == 0 && n == 0 && max_sta <= 16))
                    members.push_back(order[q]);
            }
            if (members.empty()) continue;
            ClassHost best;
            double best_cost = 0.0;
            for (int i = 0; i < 3 && cand[c][i]; ++i) {
                if (forced_tile && cand[c][i] != forced_tile) continue;
                ClassHost ch;
                ch.tile = cand[c][i];
                if (!build_plan(moveouts, w_sources, members, S, P, all_stations, ch.tile, chunk, hard, hard, max_group,
                                source_id_offset, true, ch.ph))
                    continue;
                const double cost = plan_cost(ch.ph, ch.tile);
                if (verbose)
                    fprintf(stderr, "[bpmf] bp class %d (%zu sources, %d..%d stations) tile %d: %zu groups, cost %.1f\n",
                            c, members.size(), bound[c] + 1, bound[c + 1], ch.tile, ch.ph.groups.size(), cost);
                if (!best.tile || cost < best_cost) {
                    best = std::move(ch);
                    best_cost = cost;
                }
                // groups of hundreds of sources: a smaller tile cannot win
                if ((double)members.size() / (double)best.ph.groups.size() >= 256.0 && best.tile == cand[c][i]) break;
            }
            // 33-64 stations: two LDS residencies per group at tile 256 (the station halves of every
            // source, partial beams carried in registers) against one at tile 128
            if (c == 2 && (!forced_tile || forced_tile == 256) && opt_halves) {
                ClassHost ch;
                ch.tile = 256;
                ch.halves = true;
                // 2-4 residencies of at most 20 stations, every source as two records of 6 / 8 / 10 stations in
                // each of them
                int cmax = 0;
                for (int m : members) cmax = std::max(cmax, nsta[m]);
                const int n_pass = std::max(2, (cmax + 19) / 20);
                const int tp_h = std::max(6, (((cmax + n_pass - 1) / n_pass + 1) / 2 + 1) / 2 * 2), per = 2 * tp_h;
                const int slots = BPF_HALVES_SLOTS;
                if (tp_h <= 10 &&
                    build_plan_halves(moveouts, w_sources, members, S, P, all_stations, 256, chunk, hard,
                                      std::min(max_group, 16 * slots), source_id_offset, per, n_pass, slots, ch.ph) &&
                    build_fast_host_halves(ch.ph, ch.fh, opt_uniform)) {
                    const double cost = plan_cost(ch.ph, 256);
                    if (verbose)
                        fprintf(stderr, "[bpmf] bp class %d, %d residencies of %d stations at tile 256: %zu entries, cost %.1f\n",
                                c, n_pass, per, ch.ph.groups.size(), cost);
                    if (!best.tile || cost < best_cost || forced_tile == 256) {
                        best = std::move(ch);
                        best_cost = cost;
                    }
                }
            }
            if (!best.tile || (!best.halves && !build_fast_host(best.ph, best.tile, opt_uniform, best.fh))) {
                ok = false;
                break;
            }
            classes.push_back(std::move(best));
        }
        if (!ok) classes.clear();
    }
    // A single class at tile 512 that lists every source doubles as the plan of the general kernels
    // (their 8-byte-gather flavour): edge tiles and reduce="none" then gather 8 bytes too, and the
    // grid is planned once.  Otherwise the general kernels get their own single-window plan.
    const bool share = classes.size() == 1 && classes[0].tile == 512 && classes[0].ph.srcs.size() == K;
    const bool use_fast = !classes.empty() && opt_fast;
    if (!share && !use_fast) classes.clear();

    int tpt = 0;
    if (share) {
        tpt = 2;
    } else {
        for (int cnd = tpt_first; cnd >= 1 && !tpt; --cnd) {   // tile 256 x bp.tpt, then 256
            out.own = PlanHost();
            if (build_plan(moveouts, w_sources, order, S, P, all_stations, BP_THREADS * cnd, chunk, soft, hard,
                           max_group, source_id_offset, false, out.own))
                tpt = cnd;
        }
    }
    out.general_is_class0 = share;
    const PlanHost& ph = out.general();
    sh.direct_reason = !tpt ? BP_DIRECT_WINDOWS
                            : (ph.NT > 256 ? BP_DIRECT_TERMS
                                           : (opt_direct ? BP_DIRECT_OPTION : (upper_only_direct ? BP_DIRECT_UPPER_ONLY : BP_LDS_PLAN)));
    if (sh.direct_reason != BP_LDS_PLAN) {
        // No LDS plan: one source's station-phase windows do not fit at the smallest tile, or a source has
        // more than 256 (station, phase) terms (or option bp.direct asks for it: the tests).  The grid runs
        // bp_direct.hip on compact term lists in the oracle's order.
        out.dhdr.resize(K);
        out.dfirst.assign(K + 1, 0);
        for (size_t k = 0; k < K; ++k) {
            long long lo = 0, hi = 0;
            const int any = source_tau_range(moveouts, w_sources, k, S, P, all_stations, lo, hi) > 0 ? 1 : 0;
            out.dfirst[k] = (long long)out.dterms.size();
            for (size_t s = 0; s < S; ++s) {
                const float b = w_sources[k * S + s];
                if (b == 0.0f) continue;
                for (size_t p = 0; p < P; ++p)
                    out.dterms.push_back(make_int4((int)(s * P + p), moveouts[(k * S + s) * P + p], __builtin_bit_cast(int, b), 0));
            }
            // (strict-upper-only: the lower test always passes; the kernel drops a term in front of sample 0)
            out.dhdr[k] = make_int4(any, upper_only ? 0 : (int)lo, (int)hi, 0);
        }
        out.dfirst[K] = (long long)out.dterms.size();
        if (verbose) {
            static const char* const why[] = {"", "windows exceed the LDS", "> 256 terms per source", "bp.direct",
                                              "bp.compat_strict_upper_only, a negative used moveout"};
            fprintf(stderr, "[bpmf] bp plan: K=%zu, no LDS plan (%s): global-memory gathers over %zu terms\n", K,
                    why[sh.direct_reason], out.dterms.size());
        }
        if (out.dterms.empty()) out.dterms.push_back(make_int4(0, 0, 0, 0));
        sh.direct = true;
        sh.tpt = 4;
        sh.NT = (int)std::min<size_t>(SP, 0x7fffffff);
        classes.clear();
        out.own = PlanHost();
        out.general_is_class0 = false;
        return out;
    }
    sh.tpt = tpt;
    sh.NT = ph.NT;
    sh.n_groups = (int)ph.groups.size();
    sh.lds_bytes = ph.lds_floats * sizeof(float);
    sh.dual = share;
    if (verbose)
        fprintf(stderr, "[bpmf] bp plan: K=%zu groups=%d (mean %.1f src) tile=%d NT=%d chunk=%d lds=%zu B dual=%d classes=%zu\n",
                K, sh.n_groups, (double)K / (double)ph.groups.size(), BP_THREADS * tpt, sh.NT, chunk, sh.lds_bytes,
                (int)sh.dual, classes.size());
    // packed per-station records for the two-phase kernel
    if (P == 2 && ph.NT <= 64) {
        const int nsta_max = ph.NT / 2;   // NT is a multiple of 4
        const int opts[5] = {4, 8, 12, 16, 32};
        for (int o = 0; o < 5 && !sh.nsv; ++o)
            if (nsta_max <= opts[o]) sh.nsv = opts[o];
    }
    if (sh.nsv) {
        out.recs.assign(K * (size_t)(sh.nsv / 2), make_int4(0, 0, 0, 0));
        out.hdr2.resize(K);
        for (size_t q = 0; q < K; ++q) {
            int* r = (int*)&out.recs[q * (sh.nsv / 2)];
            const int nterm = ph.srcs[q].nterm;  // padded to the chunk (4): pairs of terms = stations
            int nst = 0;
            for (int j = 0; j + 1 < nterm; j += 2) {
                const unsigned o0 = (unsigned)ph.off[q * ph.NT + j], o1 = (unsigned)ph.off[q * ph.NT + j + 1];
                r[2 * nst] = (int)(o0 | (o1 << 16));
                r[2 * nst + 1] = __builtin_bit_cast(int, ph.beta[q * ph.NT + j]);
                ++nst;
            }
            out.hdr2[q] = make_int4(ph.srcs[q].id, ph.srcs[q].tmin, ph.srcs[q].tmax, (nst + 1) / 2 * 2);
        }
    }
    // the per-term table of bp_beam_wps_kernel (tile 512 without packed records, <= 32 terms per
    // source): {byte offset, weight} pairs padded to ntv per source
    if (tpt == 2 && !sh.nsv && ph.NT <= 32) {
        sh.ntv = (ph.NT + 7) / 8 * 8;
        out.termsv.assign(K * (size_t)sh.ntv, BpTermV{0, 0.0f});
        for (size_t q = 0; q < K; ++q)
            for (int j = 0; j < ph.NT; ++j)
                out.termsv[q * sh.ntv + j] = BpTermV{ph.off[q * ph.NT + j] * 4, ph.beta[q * ph.NT + j]};
    }
    // interior-tile classes
    if (use_fast) {
        for (size_t c = 0; c < classes.size(); ++c) {
            const ClassHost& ch = classes[c];
            BpClassShape& cs = sh.cls[sh.n_classes++];
            cs.tile = ch.tile;
            cs.halves = ch.halves;
            cs.n_pass = ch.halves ? ch.ph.n_pass : 1;
            cs.n_groups = (int)ch.fh.fg.size();
            cs.lds_bytes = ch.ph.lds_floats * sizeof(float);
            cs.n_sources = ch.fh.n_sources;
            cs.max_stations = ch.fh.max_sta;
            if (verbose)
                fprintf(stderr, "[bpmf] bp fast class %zu: tile %d, %zu sources (<= %d stations), %d groups, %zu runs, uniform=%d, rec=%d dwords\n",
                        c, cs.tile, cs.n_sources, cs.max_stations, cs.n_groups, ch.fh.fr.size(), (int)ch.fh.uniform, ch.fh.rec_dw);
        }
        sh.fast = sh.n_classes > 0;
        sh.fast_shares_generic = share;
    }
    return out;
}

// ------------------------------------------------------------------- schedule ---
// The general kernel of a plan: packed per-station records (P = 2, tile 512), else the per-term table (<= 32
// terms per source, tile 512), else the readlane kernel (any plan, tile 256 x tpt).
BpKernel bpmf::bp_general_kernel(const BpPlanShape& sh)
{
    BpKernel k;
    k.waves_per_cu = 8;
    k.gather_bytes = sh.dual ? 8 : 4;
    if (sh.direct) {                // no LDS plan: global-memory gathers (bp_direct.hip)
        k.tile = BPD_TILE;
        return k;
    }
    if (sh.tpt == 2 && sh.nsv) {
        // Packed records of <= 16 stations keep a source's metadata in SGPRs: 16 waves per workgroup with
        // the 8-byte gathers of a dual plan, 12 (2 workgroups, 24 waves per CU) with 4-byte gathers, which
        // need >= 4 waves/SIMD to reach the LDS rate.  32 stations: one 16-wave workgroup per CU, the
        // records gathered in two parts.
        k.family = BP_FAMILY_WPS2;
        k.nsv = sh.nsv;
        k.b64 = sh.nsv <= 16 && sh.dual;
        k.wpb = sh.nsv > 16 || sh.dual ? 16 : 12;
        k.tile = 512;
        k.lds_bytes = std::max(sh.lds_bytes, (size_t)2 * k.wpb * 512 * sizeof(float));
        k.waves_per_cu = k.wpb == 16 ? 16 : 24;
    } else if (sh.tpt == 2 && sh.ntv) {
        k.family = BP_FAMILY_WPS;
        k.ntv = sh.ntv;
        k.tile = 512;
        // the end-of-kernel merge needs 2 * 4 * tile floats of LDS
        k.lds_bytes = std::max(sh.lds_bytes, (size_t)8 * 512 * sizeof(float));
    } else {
        k.family = BP_FAMILY_READLANE;
        k.tpt = sh.tpt == 1 ? 1 : 2;
        k.nblk = sh.NT <= 64 ? 1 : (sh.NT <= 128 ? 2 : 4);      // blocks of 64 terms per source
        k.tile = BP_THREADS * k.tpt;
        k.lds_bytes = sh.lds_bytes;
    }
    return k;
}

// source ranges per tile of reduce="max" on a plan without LDS windows: enough workgroups for ~4 rounds over the chip
int bpmf::direct_split_count(const BpPlanShape& sh, size_t N)
{
    const long long tiles = (long long)((N + BPD_TILE - 1) / BPD_TILE);
    long long want = tiles >= 1024 ? 1 : (1024 + tiles - 1) / tiles;
    return (int)std::max<long long>(1, std::min<long long>({want, (long long)sh.K, 256}));
}

namespace {
// Group ranges per tile (gridDim.y of the beam kernels).  A workgroup owns a 512-sample tile and one
// workgroup fills a CU, so a series of fewer than ~128 tiles -- the reference's event relocation
// beamforms 1 500-3 000 samples over the whole grid (BPMF/dataset.py:2174-2216) -- leaves most of the
// 256 CUs idle (and up to ~1000 tiles the last round of workgroups runs half empty): the groups of the
// plan are then dealt to 1024 / tiles workgroups per tile.
// option bp.split: 0/1 = off, n = force n ranges (tests), -1 = automatic.  Only the P = 2 packed kernels take it.
// `n_events`: series of N samples computed by one launch (a batch of events fills the chip with its events' tiles)
long long split_wanted(size_t N, int forced, size_t n_events)
{
    const long long n_tiles = (long long)((N + 511) / 512) * (long long)n_events;
    // enough workgroups for ~4 rounds over the 256 CUs (a split costs one merge pass and nothing else:
    // the ranges stage disjoint windows), none from 1024 tiles (N >= 524 288) on
    long long want = n_tiles >= 1024 ? 1 : (1024 + n_tiles - 1) / n_tiles;
    if (forced >= 0) want = forced < 1 ? 1 : forced;
    return want;
}
}  // namespace

BpSchedule bpmf::bp_schedule(const BpPlanShape& sh, size_t N, int reduce, int forced_split, size_t n_events)
{
    BpSchedule s;
    s.kernel = bp_general_kernel(sh);
    const bool is_max = reduce == BPMF_BP_REDUCE_MAX;
    const size_t E = std::max<size_t>(n_events, 1);
    size_t row_sets = E;    // sets of `rows` partial rows in the workspace
    size_t ws_rows = 1;     // rows a set is sized for
    if (sh.direct) {
        // ranges of sources per tile folded by the merge kernel; a batch runs its events one after the other
        // through the same rows
        s.path = BP_PATH_DIRECT;
        const int n = direct_split_count(sh, N);
        s.n_split = s.n_split_edge = s.rows = is_max ? n : 1;
        ws_rows = (size_t)n;
        row_sets = 1;
    } else {
        const bool can_split = sh.tpt == 2 && sh.nsv && sh.n_groups >= 2;   // (the packed kernels)
        // the general kernels alone (reduce="none", plans without interior classes, batches: their group ranges
        // count the tiles of the WHOLE batch -- a few hundred events fill the chip without any split)
        const int n_general =
            can_split ? (int)std::max<long long>(1, std::min<long long>(split_wanted(N, forced_split, E), sh.n_groups)) : 1;
        // reduce="max" on a plan with interior classes: group ranges per tile of every class kernel, and of
        // the general kernel on the edge tiles (1 when that kernel cannot split)
        long long want = split_wanted(N, forced_split, 1);
        for (int c = 0; c < sh.n_classes; ++c)
            want = std::min<long long>(want, sh.cls[c].n_groups / sh.cls[c].n_pass);   // (groups of sources, not entries)
        if (can_split) want = std::min<long long>(want, sh.n_groups);
        const int n_fast = (int)std::max<long long>(1, want);
        const bool run = n_events == 0;
        if (run && sh.fast && is_max) {
            // Samples on which no source can leave the trace -- t + tmin_all >= 0 and t + tmax_all (+ the
            // staging slack of 8 samples) < N, rounded to multiples of 1024 (whole tiles of every kernel) --
            // run the interior kernel of bp_fast.hip, once per station-count class, which is the same for
            // strict and flexible; the few tiles at the ends of the day run the general kernel over all
            // sources.  Several classes, or several group ranges per tile on a short series, write
            // partial rows behind the prestack, folded by one merge launch (value, then lowest id).
            s.path = BP_PATH_INTERIOR;
            s.n_split = n_fast;
            s.n_split_edge = can_split ? n_fast : 1;
            s.rows = n_fast * sh.n_classes;
            long long lo_s = sh.tmin_all < 0 ? ((long long)(-(long long)sh.tmin_all) + 1023) / 1024 * 1024 : 0;
            long long hi_s = ((long long)N - sh.tmax_all - 8) / 1024 * 1024;
            if ((long long)N - sh.tmax_all - 8 < 0) hi_s = 0;
            // The interior range ends at a WHOLE tile of every kernel inside the series.  (Rounds 2-3 clamped it
            // to N: when every used moveout is negative -- tmax_all < -8 -- N - tmax_all - 8 exceeds N, the clamp
            // left a bound that is no multiple of the tile, the interior launch stopped at the last whole tile
            // below it and the edge launch, starting AT the bound, was empty: the samples of the last partial
            // tile were never written.  Found by the 150 000-case session of round 4, seeds 15831 and 17025 of
            // test_bp_random_shapes_signed_moveouts; pinned by test_bp_all_used_moveouts_negative.)
            hi_s = std::min(hi_s, (long long)N / 1024 * 1024);
            lo_s = std::min(lo_s, (long long)N);
            s.lo_s = lo_s;
            s.hi_s = std::max(lo_s, hi_s);
        } else {
            // the general kernels over the whole series; reduce="max" of several group ranges goes through
            // partial rows and one merge launch
            s.path = BP_PATH_GENERAL;
            s.n_split = s.n_split_edge = n_general;
            s.rows = is_max ? n_general : 1;
        }
        // (a run's workspace is sized for the larger of the general and the interior rows, whatever `reduce` is:
        // bpmf_bp_workspace_bytes does not know it)
        ws_rows = run ? std::max<size_t>((size_t)n_general, sh.fast ? (size_t)n_fast * (size_t)sh.n_classes : 0)
                      : (size_t)s.rows;
    }
    // the prestacked traces (of every event) + the partial maxima: beam rows, then arg rows (not aligned again)
    s.o_prestack = 0;
    s.o_pbeam = align_up(E * sh.S * sh.P * N * sizeof(float), 256);
    s.o_parg = s.o_pbeam + (s.rows > 1 ? row_sets * (size_t)s.rows * N * sizeof(float) : 0);
    s.total = s.o_pbeam + (ws_rows > 1 ? align_up(row_sets * ws_rows * N * (sizeof(float) + sizeof(int32_t)), 256) : 0);
    return s;
}

// ------------------------------------------------------------------ diagnostics ---
namespace {
void plan_stats(const BpPlanShape& sh, bpmf_bp_plan_stats* out)
{
    const BpKernel k = bp_general_kernel(sh);
    memset(out, 0, sizeof(*out));
    out->tile = k.tile;
    out->gather_bytes = k.gather_bytes;
    out->waves_per_cu = k.waves_per_cu;
    if (sh.direct) return;
    out->n_groups = sh.n_groups;
    out->lds_bytes = (int32_t)sh.lds_bytes;
    out->stations_max = sh.nsv;
    // reduce="max": the interior tiles run the classes of bp_fast.hip (8-byte gathers, 16 waves per CU);
    // tile / n_groups then describe the class that holds most sources
    out->n_classes = sh.n_classes;
    int big = 0;
    for (int c = 0; c < sh.n_classes; ++c) {
        out->class_tile[c] = sh.cls[c].tile;
        out->class_sources[c] = (int32_t)sh.cls[c].n_sources;
        out->class_groups[c] = sh.cls[c].n_groups;
        out->class_stations_max[c] = sh.cls[c].max_stations;
        if (sh.cls[c].n_sources > sh.cls[big].n_sources) big = c;
    }
    if (sh.fast) {
        out->tile = sh.cls[big].tile;
        out->n_groups = sh.cls[big].n_groups;
        out->lds_bytes = (int32_t)sh.cls[big].lds_bytes;
        out->gather_bytes = 8;
        out->waves_per_cu = 16;
    }
}
}  // namespace

extern "C" int bpmf_bp_plan_info(const bpmf_bp_plan* pl, bpmf_bp_plan_stats* out)
{
    if (!pl || !out) {
        set_error("bpmf_bp_plan_info: bad argument");
        return -1;
    }
    plan_stats(pl->shape, out);
    return 0;
}

// The plan and the schedule of a run of these tables under the current options, as
// out[BPMF_BP_LAUNCH_INFO_FIELDS] (include/bpmf_hip.h)
extern "C" int bpmf_bp_launch_info(const int32_t* moveouts, const float* w_sources, size_t K, size_t S, size_t P,
                                   size_t N, int reduce, size_t n_events, int64_t* out)
{
    if (!out) {
        set_error("bpmf_bp_launch_info: null pointer");
        return -1;
    }
    if (const char* why = bp_plan_refusal(moveouts, w_sources, K, S, P)) {
        set_error("bpmf_bp_launch_info: %s", why);
        return -1;
    }
    if (N == 0 || N > 0x7fffffffull || (reduce != BPMF_BP_REDUCE_MAX && reduce != BPMF_BP_REDUCE_NONE) ||
        (n_events > 0 && reduce != BPMF_BP_REDUCE_MAX)) {
        set_error("bpmf_bp_launch_info: bad N / reduce / n_events");
        return -1;
    }
    try {
        const BpPlanShape sh = bp_plan_host(moveouts, w_sources, K, S, P, 0).shape;
        const BpSchedule s = bp_schedule(sh, N, reduce, (int)option(OPT_BP_SPLIT), n_events);
        bpmf_bp_plan_stats st;
        plan_stats(sh, &st);
        int64_t* o = out;
        for (int64_t v : {(int64_t)sh.K, (int64_t)sh.S, (int64_t)sh.P, (int64_t)sh.tpt, (int64_t)sh.NT, (int64_t)sh.nsv,
                          (int64_t)sh.ntv, (int64_t)sh.dual, (int64_t)sh.n_groups, (int64_t)sh.lds_bytes,
                          (int64_t)sh.direct_reason, (int64_t)sh.fast, (int64_t)sh.fast_shares_generic,
                          (int64_t)sh.n_classes})
            *o++ = v;
        for (int c = 0; c < BPF_MAX_CLASSES; ++c)
            for (int64_t v : {(int64_t)sh.cls[c].tile, (int64_t)sh.cls[c].halves, (int64_t)sh.cls[c].n_pass,
                              (int64_t)sh.cls[c].n_groups, (int64_t)sh.cls[c].lds_bytes, (int64_t)sh.cls[c].n_sources,
                              (int64_t)sh.cls[c].max_stations})
                *o++ = v;
        const BpKernel& k = s.kernel;
        for (int64_t v : {(int64_t)sh.tmin_all, (int64_t)sh.tmax_all, (int64_t)sh.id_offset,
                          (int64_t)s.path, (int64_t)k.family, (int64_t)k.wpb, (int64_t)k.nsv, (int64_t)k.b64, (int64_t)k.ntv,
                          (int64_t)k.tpt, (int64_t)k.nblk, (int64_t)k.tile, (int64_t)k.lds_bytes, (int64_t)k.waves_per_cu,
                          (int64_t)k.gather_bytes, (int64_t)s.n_split, (int64_t)s.n_split_edge, (int64_t)s.rows,
                          (int64_t)s.lo_s, (int64_t)s.hi_s, (int64_t)s.o_prestack, (int64_t)s.o_pbeam, (int64_t)s.o_parg,
                          (int64_t)s.total,
                          (int64_t)st.n_groups, (int64_t)st.tile, (int64_t)st.lds_bytes, (int64_t)st.gather_bytes,
                          (int64_t)st.stations_max, (int64_t)st.waves_per_cu, (int64_t)st.n_classes})
            *o++ = v;
        for (const int32_t* a : {st.class_tile, st.class_sources, st.class_groups, st.class_stations_max})
            for (int c = 0; c < 3; ++c) *o++ = a[c];
        static_assert(BPMF_BP_LAUNCH_INFO_FIELDS == 14 + 7 * BPF_MAX_CLASSES + 31 + 12, "fields of bpmf_bp_launch_info");
    } catch (const std::exception& e) {     // (std::bad_alloc of the planning must not cross the C boundary)
        set_error("bpmf_bp_launch_info: exception: %s", e.what());
        return -3;
    }
    return 0;
}
