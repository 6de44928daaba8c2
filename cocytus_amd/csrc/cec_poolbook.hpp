// cec_poolbook.hpp -- the recovery pool's host state, which touches no device: the Book
// (the one request record, the slot allocator with id reuse, the flush queue, the checks
// of replies, residuals and solve lists, the plan and the commit of a flush, the pieces of
// an update), the stream slots of a flush and the key of a flush pattern.  Plain C++ (no
// HIP), included by cec_pool.inc and, as shipped, by tests/drain_c/pool_book_main.cpp,
// which runs it under ASan + UBSan against a per-unit model.
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <vector>

namespace poolbook {

constexpr int kMaxK = 16, kMaxM = 8;  // CEC_MAX_K, CEC_MAX_M (asserted in cec_pool.inc)
constexpr int kStreams = 48;          // kMaxStreams
constexpr int kInputs = 16;           // kPatN
constexpr int kOutputs = 4;           // kPatL
constexpr uint32_t kUnit = 4096;      // kTile
// A fused flush pattern's outputs are R' if anything is folded and the n rebuilt shards.  One
// launch holds kOutputs, so the flush's own launch solves n <= 3; more are solved behind it.
constexpr int kFusedLosses = kOutputs - 1;

// A recovery mask names k lids (mask_ok): the data lids that answer and as many parities
// as data lids are lost.
inline uint32_t data_lids(int k, uint32_t mask) { return mask & ((1u << k) - 1); }
inline uint32_t parity_lids(int k, uint32_t mask) { return mask & ~((1u << k) - 1); }
inline int n_lost(int k, uint32_t mask) { return __builtin_popcount(parity_lids(k, mask)); }
// The parities whose residuals the leader `self` must be given: the mask's others.
inline uint32_t needed(int k, int self, uint32_t mask) { return parity_lids(k, mask) & ~(1u << self); }

// The one request record.
struct Req {
    bool used = false;
    uint32_t mask = 0;
    int ub = 0, nunits = 0, slot = 0;
    bool touched = false;        // first touch done or queued
    bool touch_pending = false;  // the first touch happens at the next flush
    uint32_t contributed = 0;    // data lids applied or queued
    uint32_t queued = 0;         // data lids queued for the next flush
    uint32_t given = 0;          // parity lids whose residual was given (static: never folded into)
    bool enqueued = false;       // in queued_ids: a reply or a residual came since the last flush
    bool solved = false;         // rebuilt by a solve, and R has not changed since
    bool solved_host = false;    // ... into the host planes (the _host solves)
};

enum Refusal {
    kAccepted = 0,
    kNotLive,     // residual: no such request
    kNotParity,   // the lid is no parity of the request's mask
    kSelf,        // the pool's own parity: its residual is R
    kTwice,       // that parity's residual was given before
    kSingleLoss,  // a single-loss request takes none
    kPairTwice,   // batch (replies too): a (request, lid) pair listed twice
    kNoReply,     // reply: no such request, no bytes, or the peer is no data lid of its mask
    kApplied,     // reply: that peer contributed before (recovery.c:75)
    kIncomplete,  // solve list: no such request, or a data lid of its mask has not replied
    kListedTwice,
    kNotReady,    // ... complete, but not every other participating parity's residual given
    kNoOutput,    // ... a lost lid has no output arena
    kBadArgs,     // begin: units or mask (k lids, none at or above k + m, names self)
    kTooLarge,    // begin: more units than the buffer
    kNoRun,       // begin: no free contiguous run
};

// An entry of a batch whose (a, b) pair is listed again, or -1.
inline int repeated_pair(const int *a, const int *b, int n) {
    std::vector<std::array<int, 3>> v(n > 0 ? n : 0);
    for (int i = 0; i < n; ++i) v[i] = {a[i], b[i], i};
    std::sort(v.begin(), v.end());
    for (int i = 1; i < n; ++i)
        if (v[i][0] == v[i - 1][0] && v[i][1] == v[i - 1][1]) return v[i - 1][2];
    return -1;
}

// What a flush does with queued_ids[x]: fold its replies, or make the first touch of a request
// whose mask names no data lid (kFold), fold and solve in the same launch (kFused: ready, at
// most kFusedLosses), or nothing (a residual came, and the request is not ready or the pass
// does not solve).  `later`: ready with more losses, solved behind the
// launch.  `planes`: the host output planes a to_host pass writes.
enum Action : char { kNothing, kFold, kFused };
struct Plan {
    std::vector<char> action;
    std::vector<int> later;
    int planes = 0;
};

struct Span {  // a touched request's arena range; max_end: the running maximum of the ends
    uint64_t base, end, max_end;
    int id;
};
struct Piece {  // of update `upd`, inside request `id`
    int id;
    uint64_t r_off, d_off;  // in R; in the update's buffer
    uint32_t len;
    int upd;
};

struct Book {
    int k = 0, m = 0, self = 0;
    std::vector<Req> reqs;
    std::vector<int> free_ids;    // ended request ids, reused LIFO
    std::vector<int> slot_owner;  // -1 free
    int cursor = 0;               // next-fit start: O(1) amortised begin for unit-sized requests
    // The ids with something for the next flush, each at most once (Req::enqueued).  A flush
    // clears queue and marks; a request that ends while marked is taken out, so an id reused
    // by the next begin -- which starts unmarked, or enters once itself (a mask without data
    // lids) -- cannot enter twice.
    std::vector<int> queued_ids;

    Book() = default;
    Book(int k_, int m_, int self_, int capacity_units) : k(k_), m(m_), self(self_), slot_owner(capacity_units, -1) {}
    int capacity() const { return static_cast<int>(slot_owner.size()); }
    // The one liveness test.
    const Req *find(int id) const {
        return id >= 0 && id < static_cast<int>(reqs.size()) && reqs[id].used ? &reqs[id] : nullptr;
    }
    int active() const { return std::count_if(reqs.begin(), reqs.end(), [](const Req &r) { return r.used; }); }
    // The lost data lids of a mask (ascending: C[] / data[], memcached.c:7911-7922), as many as its parities.
    uint32_t lost_lids(uint32_t mask) const { return ~mask & ((1u << k) - 1); }
    int n_lost(uint32_t mask) const { return poolbook::n_lost(k, mask); }
    // check_recovery_1st_completeness: every data lid of the mask applied or queued.
    bool complete(int id) const {
        const Req *r = find(id);
        return r && (r->contributed & data_lids(k, r->mask)) == data_lids(k, r->mask);
    }
    // ... and every other participating parity's residual given.  A single loss needs none:
    // ready == complete.
    // With k <= m a mask may name no data lid: k parities rebuild all k shards.  Such a request
    // is complete from the start (ready at once for k = 1), and its residual is R = P[range],
    // the first-touch copy of recovery.c:79-82 with no fold behind it.  No reply will ever
    // bring that copy about, so begin queues it: the next flush of any kind makes it (and
    // solves in the same launch, if it solves and the request is ready), and every reader of R
    // -- solve, residual, the pieces of an update -- flushes first.  Until then R[slot] holds
    // what the slots' previous owner left, and check_solve refuses the request.
    bool ready(int id) const {
        const Req *r = find(id);
        return complete(id) && (r->given & needed(k, self, r->mask)) == needed(k, self, r->mask);
    }

    // A request of units [unit_begin, unit_end]: its id, or -Refusal.  Next fit from the
    // cursor, wrapping once: requests end roughly in begin order, so the free units are
    // usually right at the cursor.
    int begin(uint32_t mask, int unit_begin, int unit_end) {
        if (unit_begin < 0 || unit_end < unit_begin || !(mask & (1u << self)) || (mask >> (k + m)) != 0 ||
            __builtin_popcount(mask) != k)
            return -kBadArgs;
        const int cap = capacity();
        if (unit_end - unit_begin >= cap) return -kTooLarge;
        const int n = unit_end - unit_begin + 1;
        int slot = -1;
        for (int step = 0, run = 0, s = cursor; step < cap + n; ++step, ++s) {
            if (s == cap) {
                s = 0;
                run = 0;  // a run may not wrap around the end of the buffer
            }
            run = slot_owner[s] < 0 ? run + 1 : 0;
            if (run == n) {
                slot = s - n + 1;
                break;
            }
        }
        if (slot < 0) return -kNoRun;
        cursor = (slot + n) % cap;
        if (free_ids.empty()) free_ids.push_back(static_cast<int>(reqs.size())), reqs.emplace_back();  // a new id
        const int id = free_ids.back();
        free_ids.pop_back();
        reqs[id] = Req{true, mask, unit_begin, n, slot};
        std::fill_n(slot_owner.begin() + slot, n, id);
        if (!data_lids(k, mask)) {  // no reply to wait for: the first touch goes into the next flush (ready, above)
            reqs[id].touched = reqs[id].touch_pending = true;
            enqueue(id);
        }
        return id;
    }
    // Still in the queue with nothing to fold (a residual came since the last flush, or the
    // first touch of a mask without data lids is still to be made): taken out.  (A reply still
    // queued -- find(id)->queued -- is the caller's to flush first.)
    void end(int id) {
        Req &r = reqs[id];
        if (r.enqueued) queued_ids.erase(std::remove(queued_ids.begin(), queued_ids.end(), id), queued_ids.end());
        std::fill_n(slot_owner.begin() + r.slot, r.nunits, -1);
        r.used = r.enqueued = false;
        free_ids.push_back(id);
    }

    // Every entry of a batch checked before any is noted; *bad = the first refused entry.
    template <class Check>
    Refusal check_batch(const int *ids, const int *lids, int n, int *bad, Check one) const {
        for (*bad = 0; *bad < n; ++*bad)
            if (Refusal why = one(*bad)) return why;
        *bad = repeated_pair(ids, lids, n);
        return *bad < 0 ? kAccepted : kPairTwice;
    }
    Refusal check_reply(int id, int peer, const void *units) const {
        const Req *r = find(id);
        if (!r || !units || peer < 0 || peer >= k || !(r->mask & (1u << peer))) return kNoReply;
        return r->contributed & (1u << peer) ? kApplied : kAccepted;
    }
    Refusal check_replies(const int *ids, const int *peers, const void *const *units, int n, int *bad) const {
        return check_batch(ids, peers, n, bad, [&](int i) { return check_reply(ids[i], peers[i], units[i]); });
    }
    Refusal check_residual(int id, int lid) const {
        const Req *r = find(id);
        if (!r) return kNotLive;
        if (n_lost(r->mask) < 2) return kSingleLoss;  // (its one parity is the pool's own)
        if (lid == self) return kSelf;
        if (lid < k || lid >= k + m || !(r->mask & (1u << lid))) return kNotParity;
        return r->given & (1u << lid) ? kTwice : kAccepted;
    }
    Refusal check_residuals(const int *ids, const int *lids, int n, int *bad) const {
        return check_batch(ids, lids, n, bad, [&](int i) { return check_residual(ids[i], lids[i]); });
    }
    // Something for the next flush: a reply to fold, or a residual that may have made it ready.
    void enqueue(int id) {
        if (!reqs[id].enqueued) queued_ids.push_back(id);
        reqs[id].enqueued = true;
    }
    void note_reply(int id, int peer) {  // (checked; its bytes are in the peer's staging)
        Req &r = reqs[id];
        if (!r.touched) r.touched = r.touch_pending = true;
        r.contributed |= 1u << peer;
        r.queued |= 1u << peer;
        enqueue(id);
    }
    void note_residual(int id, int lid) {
        reqs[id].given |= 1u << lid;
        enqueue(id);
    }

    // The plan of a flush that solves (`solves`) into the host planes (`to_host`) or into the
    // arenas of the data lids in `arenas`.  A lost lid's arena not given: folded only.
    Plan plan_flush(bool solves, bool to_host, uint32_t arenas) const {
        Plan pl;
        pl.action.assign(queued_ids.size(), kNothing);
        for (size_t x = 0; x < queued_ids.size(); ++x) {
            const int id = queued_ids[x];
            const Req &r = reqs[id];
            if (r.queued || r.touch_pending) pl.action[x] = kFold;
            if (!solves || !ready(id) || (!to_host && (lost_lids(r.mask) & ~arenas))) continue;
            if (const int n = n_lost(r.mask); n > kFusedLosses) {
                pl.later.push_back(id);
            } else {
                pl.action[x] = kFused;
                if (to_host) pl.planes = std::max(pl.planes, n);
            }
        }
        return pl;
    }
    // The flush's launch done: the queue emptied, the fused requests solved.  Returns those.
    int commit_flush(const Plan &pl, bool to_host) {
        int n_solved = 0;
        for (size_t x = 0; x < queued_ids.size(); ++x) {
            Req &r = reqs[queued_ids[x]];
            r.queued = 0;
            r.touch_pending = r.enqueued = false;
            if (pl.action[x] == kFused) r.solved = true, r.solved_host = to_host, ++n_solved;
        }
        queued_ids.clear();
        return n_solved;
    }
    // R[slot] holds the request's residual: touched, and the first touch flushed.
    bool holds_residual(int id) const {
        const Req *r = find(id);
        return r && r->touched && !r->touch_pending;
    }
    // A solve list: live and complete with R in place (the caller flushes first, so a queued
    // first touch is made by then), listed once, ready, outputs there; *bad = the refused entry.
    Refusal check_solve(const int *ids, int n, bool to_host, uint32_t arenas, int *bad) const {
        std::vector<char> listed(reqs.size(), 0);
        for (*bad = 0; *bad < n; ++*bad) {
            const int id = ids[*bad];
            if (!complete(id) || !holds_residual(id)) return kIncomplete;
            if (listed[id]++) return kListedTwice;
            if (!ready(id)) return kNotReady;
            if (!to_host && (lost_lids(reqs[id].mask) & ~arenas)) return kNoOutput;
        }
        return kAccepted;
    }
    void mark_solved(const std::vector<int> &ids, bool to_host) {
        for (int id : ids) reqs[id].solved = true, reqs[id].solved_host = to_host;
    }

    // The touched requests by arena range (they may overlap in the pool's API; the server's do not).
    std::vector<Span> touched_spans() const {
        std::vector<Span> spans;
        for (int id = 0; id < static_cast<int>(reqs.size()); ++id) {
            const Req &r = reqs[id];
            if (!r.used || !r.touched) continue;
            const uint64_t base = static_cast<uint64_t>(r.ub) * kUnit;
            spans.push_back({base, base + static_cast<uint64_t>(r.nunits) * kUnit, 0, id});
        }
        std::sort(spans.begin(), spans.end(), [](const Span &a, const Span &b) { return a.base < b.base; });
        for (size_t i = 0; i < spans.size(); ++i) spans[i].max_end = std::max(spans[i].end, i ? spans[i - 1].max_end : 0);
        return spans;
    }
    // recovery_try_update_unit (recovery.c:99-131) for update `upd` = [addr, addr + len) of data
    // lid `peer`: its pieces inside touched requests the peer has not contributed to, appended
    // to `out`; their R moves on, so they are no longer solved.  No test of the mask: recovery.c:
    // 116-120 folds a lost lid's diffs too (a substitute forwards them under that lid, memcached.c:
    // 7700, :7758), which keeps R equal to the lost shard's live bytes.  Returns the units folded.
    int pieces(const std::vector<Span> &spans, uint64_t addr, uint32_t len, int peer, int upd, std::vector<Piece> &out) {
        const uint64_t a = addr, b = addr + len;
        int units = 0;
        const auto starts_past = [](uint64_t v, const Span &s) { return v <= s.base; };
        size_t x = std::upper_bound(spans.begin(), spans.end(), b, starts_past) - spans.begin();
        while (x-- > 0 && spans[x].max_end > a) {
            Req &r = reqs[spans[x].id];
            const uint64_t lo = std::max(a, spans[x].base), hi = std::min(b, spans[x].end);
            if ((r.contributed & (1u << peer)) || lo >= hi) continue;
            out.push_back({spans[x].id, static_cast<uint64_t>(r.slot) * kUnit + (lo - spans[x].base), lo - a,
                           static_cast<uint32_t>(hi - lo), upd});
            units += static_cast<int>((hi - 1) / kUnit - lo / kUnit + 1);
            r.solved = r.solved_host = false;
        }
        return units;
    }
};

// The stream slots of a flush.  Its patterns outlive the call (the pool's table is append-
// only) with the slots baked in, so a slot is a function of (k, m) alone:
//
//   0            P, this parity's arena
//   1            R, the residuals
//   2 .. 2+k     Q_j, data lid j's reply staging
//   2+k .. 2+2k  a flush_solve: the arena of data lid j; a flush_solve_host: host output
//                plane x in slot 2+k+x (x-th lost lid, x < n <= min(k, m)).  One flush has
//                arenas or host planes, never both, so they share the slots; the pattern
//                key carries to_host.
//   2+2k .. +m   G_p, the staging of parity k+p's given residuals (the own parity's slot
//                stays empty)
//
// 2 + 2k + m = 42 at k = 16, m = 8, within the kernels' 48.
struct FlushSlots {
    int k, m;
    int parity() const { return 0; }
    int residual() const { return 1; }
    int reply(int j) const { return 2 + j; }
    int out(int j) const { return 2 + k + j; }
    int given(int parity_lid) const { return 2 + 2 * k + (parity_lid - k); }
    int count() const { return 2 + 2 * k + m; }
};
static_assert(2 + 2 * kMaxK + kMaxM <= kStreams, "a flush's streams at k = 16, m = 8");

// The inputs of a fused flush pattern: P or R, the queued replies (at most the k - n data
// lids of the mask), the n - 1 given residuals: at most k <= kInputs.
inline int flush_inputs(int queued_replies, int n) { return 1 + queued_replies + (n - 1); }
static_assert(1 + (kMaxK - 1) + (1 - 1) <= kInputs && 1 + (kMaxK - kMaxM) + (kMaxM - 1) <= kInputs, "k inputs");

// The key of a flush pattern: the queued data lids and the first touch decide the fold;
// a request solved in the same launch adds its whole mask (which lids are lost AND which
// parities' residuals come in, with their inverse) and where the shards go.  Requests not
// solved share one pattern per (queued, touch) whatever their mask.
// At most 2^k * 2 fold-only patterns, and per mask of <= 3 losses 2^(k-n) * 2 * 2
// (queued subsets of its k - n data lids, +1 for the residual-only pattern; touch; to_host).
inline uint64_t flush_key(uint32_t queued, bool touch, bool solved, uint32_t mask, bool to_host) {
    return static_cast<uint64_t>(queued & 0xFFFFu) | (touch ? 1ull << 16 : 0) |
           (solved ? (1ull << 17) | (to_host ? 1ull << 18 : 0) | (static_cast<uint64_t>(mask) << 32) : 0);
}

// The launches of an explicit solve of requests losing up to n_max shards.
inline int solve_launches(int n_max) { return (n_max + kOutputs - 1) / kOutputs; }

}  // namespace poolbook
