// The recovery pool's host bookkeeping (cocytus_amd/csrc/cec_poolbook.hpp, the shipped
// header): the flush's slot layout and pattern keys, readiness and the all-or-nothing check
// of a residual batch against brute force over random requests, and poolbook::Book -- the
// pool's whole state machine -- over random schedules against a model that keeps the
// reference's per-unit state, masks that name no data lid (k <= m) among them: such a request
// holds R = P from begin, and no plan or accepted solve list may name a request that holds no
// residual.  Built with ASan + UBSan by tests/test_pool_losses_abi.py; prints "ok".
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <tuple>
#include <vector>

#include "cec_poolbook.hpp"

using namespace poolbook;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            return 1;                                                     \
        }                                                                 \
    } while (0)
#define TRY(call)             \
    do {                      \
        if (call) return 1;   \
    } while (0)

static std::mt19937 rng(0xC0C7);
static int rnd(int lo, int hi) { return lo + static_cast<int>(rng() % static_cast<unsigned>(hi - lo + 1)); }

// A random recovery mask of RS(k, m) that names `self`: n <= max_lost lost data lids, n parities.
static uint32_t random_mask(int k, int m, int self, int *n_out, int max_lost) {
    const int n = rnd(1, max_lost);
    std::vector<int> d(k), p;
    for (int j = 0; j < k; ++j) d[j] = j;
    for (int q = k; q < k + m; ++q)
        if (q != self) p.push_back(q);
    std::shuffle(d.begin(), d.end(), rng);
    std::shuffle(p.begin(), p.end(), rng);
    uint32_t mask = 1u << self;
    for (int i = n; i < k; ++i) mask |= 1u << d[i];  // the first n are lost
    for (int i = 0; i < n - 1; ++i) mask |= 1u << p[i];
    *n_out = n;
    return mask;
}

static int slots() {
    for (int k = 1; k <= kMaxK; ++k)
        for (int m = 1; m <= kMaxM; ++m) {
            const FlushSlots at{k, m};
            std::set<int> seen = {at.parity(), at.residual()};
            for (int j = 0; j < k; ++j) seen.insert(at.reply(j));
            for (int j = 0; j < k; ++j) seen.insert(at.out(j));
            for (int q = k; q < k + m; ++q) seen.insert(at.given(q));
            CHECK(static_cast<int>(seen.size()) == at.count());  // no two streams share a slot
            CHECK(*seen.begin() == 0 && *seen.rbegin() == at.count() - 1 && at.count() <= kStreams);
            // host planes (x < n <= min(k, m)) fit the arenas' slots
            CHECK(at.out(std::min(k, m) - 1) < at.given(k));
            for (int n = 1; n <= std::min(k, m); ++n) {
                CHECK(flush_inputs(k - n, n) == k && flush_inputs(k - n, n) <= kInputs);
                CHECK((n <= kFusedLosses) == (1 + n <= kOutputs));
                CHECK(solve_launches(n) == (n + 3) / 4);
            }
        }
    CHECK((FlushSlots{16, 8}.count()) == 42);
    return 0;
}

// Requests in any state (written into the book's records directly: k <= m masks that name no
// data lid among them): complete, ready and the residual checks against brute force.
static int readiness_and_batches() {
    for (int round = 0; round < 4000; ++round) {
        const int k = rnd(1, kMaxK), m = rnd(1, kMaxM), self = rnd(k, k + m - 1);
        const int nreq = rnd(1, 12);
        Book book(k, m, self, nreq);
        std::vector<Req> &reqs = book.reqs;
        reqs.resize(nreq);
        std::vector<int> nl(nreq);
        for (int i = 0; i < nreq; ++i) {
            Req &r = reqs[i];
            r.used = rnd(0, 9) != 0;
            r.mask = random_mask(k, m, self, &nl[i], std::min(k, m));
            CHECK(__builtin_popcount(r.mask) == k && n_lost(k, r.mask) == nl[i]);
            CHECK(__builtin_popcount(book.lost_lids(r.mask)) == nl[i] && !(book.lost_lids(r.mask) & r.mask));
            CHECK(__builtin_popcount(needed(k, self, r.mask)) == nl[i] - 1 && !(needed(k, self, r.mask) & (1u << self)));
            r.contributed = rnd(0, 2) ? data_lids(k, r.mask) : data_lids(k, r.mask) & rng();
            r.given = rnd(0, 2) ? needed(k, self, r.mask) & rng() : needed(k, self, r.mask);
            // brute force
            bool comp = r.used, rdy = r.used;
            for (int j = 0; j < k; ++j)
                if ((r.mask >> j & 1) && !(r.contributed >> j & 1)) comp = rdy = false;
            for (int q = k; q < k + m; ++q)
                if (q != self && (r.mask >> q & 1) && !(r.given >> q & 1)) rdy = false;
            CHECK(book.complete(i) == comp && book.ready(i) == rdy);
            if (nl[i] == 1) CHECK(book.ready(i) == book.complete(i));
        }
        auto req_of = [&](int id) { return id >= 0 && id < nreq && reqs[id].used ? reqs[id] : Req{}; };
        // a batch: mostly valid entries, sometimes one bad one or a repeated pair
        const int n = rnd(0, 10);
        std::vector<int> ids(n), lids(n);
        for (int i = 0; i < n; ++i) {
            ids[i] = rnd(0, 19) ? rnd(0, nreq - 1) : rnd(-2, nreq + 2);
            const Req r = req_of(ids[i]);
            std::vector<int> open;
            for (int q = k; q < k + m; ++q)
                if (q != self && (r.mask >> q & 1) && !(r.given >> q & 1)) open.push_back(q);
            lids[i] = !open.empty() && rnd(0, 19) ? open[rnd(0, static_cast<int>(open.size()) - 1)] : rnd(-1, k + m);
        }
        // brute force: the first entry that a one-by-one check refuses, else the first
        // entry whose pair appears again
        Refusal want = kAccepted;
        int want_bad = -1;
        for (int i = 0; i < n && want == kAccepted; ++i) {
            const Req r = req_of(ids[i]);
            Refusal why = kAccepted;
            if (!r.used) why = kNotLive;
            else if (n_lost(k, r.mask) < 2) why = kSingleLoss;
            else if (lids[i] == self) why = kSelf;
            else if (lids[i] < k || lids[i] >= k + m || !(r.mask >> lids[i] & 1)) why = kNotParity;
            else if (r.given >> lids[i] & 1) why = kTwice;
            CHECK(book.check_residual(ids[i], lids[i]) == why);
            if (why) want = why, want_bad = i;
        }
        if (want == kAccepted) {
            std::map<std::pair<int, int>, int> first;
            for (int i = 0; i < n; ++i) {
                auto ins = first.emplace(std::make_pair(ids[i], lids[i]), i);
                if (!ins.second) {
                    want = kPairTwice;
                    break;
                }
            }
        }
        int bad = -1;
        const std::vector<Req> before = reqs;
        const Refusal got = book.check_residuals(ids.data(), lids.data(), n, &bad);
        CHECK(got == want);
        if (want != kAccepted && want != kPairTwice) CHECK(bad == want_bad);
        if (want == kPairTwice) {
            CHECK(bad >= 0 && bad < n);
            int again = 0;
            for (int i = 0; i < n; ++i) again += ids[i] == ids[bad] && lids[i] == lids[bad];
            CHECK(again >= 2);
        }
        for (int i = 0; i < nreq; ++i)  // the check changes nothing
            CHECK(reqs[i].given == before[i].given && reqs[i].contributed == before[i].contributed);
    }
    return 0;
}

static int keys() {
    // distinct (queued, touch, solved ? (mask, to_host) : -) give distinct keys; unsolved
    // requests share a key whatever their mask
    std::map<uint64_t, std::vector<uint32_t>> seen;
    for (int round = 0; round < 20000; ++round) {
        const uint32_t queued = rng() & 0xFFFF, mask = rng();
        const bool touch = rng() & 1, solved = rng() & 1, to_host = rng() & 1;
        const std::vector<uint32_t> what = {queued, touch, solved, solved ? mask : 0u, solved ? to_host : 0u};
        auto ins = seen.emplace(flush_key(queued, touch, solved, mask, to_host), what);
        CHECK(ins.first->second == what);
    }
    CHECK(flush_key(5, true, false, 0x1234, true) == flush_key(5, true, false, 0x4321, false));
    CHECK(flush_key(5, true, true, 0x1234, true) != flush_key(5, true, true, 0x1234, false));
    CHECK(flush_key(5, true, true, 0x1234, true) != flush_key(5, true, true, 0x1235, true));
    return 0;
}

// The flush queue over a reused id: add_residual; end; begin; add_peer.  The id enters once.
static int queue_reuse() {
    Book b(3, 2, 3, 4);
    const uint32_t dbl = 0b11100;  // {D2, P0, P1}
    const int id = b.begin(dbl, 7, 7);
    CHECK(id == 0 && b.check_residual(id, 4) == kAccepted);
    b.note_residual(id, 4);
    CHECK(b.queued_ids == std::vector<int>{0});
    b.end(id);
    CHECK(b.queued_ids.empty() && !b.find(id) && b.active() == 0);
    CHECK(b.begin(dbl, 9, 9) == id && !b.find(id)->enqueued);
    b.note_reply(id, 2);
    b.note_residual(id, 4);
    CHECK(b.queued_ids == std::vector<int>{0} && b.ready(id));
    return 0;
}

// Masks that name no data lid, step by step.  RS(1,1): the one mask {P0}, ready at begin and
// solved by the next solving flush, in its launch.  RS(2,2) {P0, P1} led by P0: folded (R = P)
// by a pass that comes before P1's residual, solved by the pass after it; and with the
// residual first, both in one launch under a key of its own.
static int no_data_lids() {
    {
        Book b(1, 1, 1, 4);
        const int id = b.begin(0b10, 5, 5);
        CHECK(id == 0 && b.complete(id) && b.ready(id) && !b.holds_residual(id));
        CHECK(b.find(id)->touched && b.find(id)->touch_pending && b.queued_ids == std::vector<int>{0});
        int bad = -1;
        CHECK(b.check_solve(&id, 1, true, 0, &bad) == kIncomplete && bad == 0);  // (the pool flushes first)
        CHECK(b.check_residual(id, 1) == kSingleLoss);
        Plan pl = b.plan_flush(true, true, 0);
        CHECK(pl.action == std::vector<char>{kFused} && pl.later.empty() && pl.planes == 1);
        CHECK(b.commit_flush(pl, true) == 1 && b.queued_ids.empty());
        CHECK(b.find(id)->solved && b.find(id)->solved_host && b.holds_residual(id) && !b.find(id)->touch_pending);
        // the lost lid's diff moves R on; the explicit solve is accepted now
        std::vector<Piece> pieces;
        CHECK(b.pieces(b.touched_spans(), 5 * kUnit + 7, 100, 0, 0, pieces) == 1 && pieces.size() == 1);
        CHECK(pieces[0].id == id && pieces[0].r_off == b.find(id)->slot * kUnit + 7 && pieces[0].len == 100);
        CHECK(!b.find(id)->solved && b.ready(id));
        CHECK(b.check_solve(&id, 1, true, 0, &bad) == kAccepted);
        // a pass that does not solve makes the first touch alone; ended while it is owed: out of the queue
        const int two = b.begin(0b10, 9, 10);
        pl = b.plan_flush(false, false, 0);
        CHECK(pl.action == std::vector<char>{kFold});
        CHECK(b.commit_flush(pl, false) == 0 && b.holds_residual(two) && !b.find(two)->solved);
        const int three = b.begin(0b10, 0, 0);
        CHECK(b.queued_ids == std::vector<int>{three});
        b.end(three);
        CHECK(b.queued_ids.empty() && b.begin(0b10, 1, 1) == three && b.queued_ids == std::vector<int>{three});
    }
    for (int residual_first = 0; residual_first < 2; ++residual_first) {
        Book b(2, 2, 2, 4);
        const uint32_t mask = 0b1100;
        const int id = b.begin(mask, 3, 4);
        CHECK(id == 0 && b.complete(id) && !b.ready(id) && b.queued_ids == std::vector<int>{0});
        CHECK(b.lost_lids(mask) == 0b11 && b.n_lost(mask) == 2 && needed(2, 2, mask) == 0b1000);
        Plan pl;
        if (!residual_first) {
            pl = b.plan_flush(true, false, 0b11);
            CHECK(pl.action == std::vector<char>{kFold});  // not ready: R = P alone
            CHECK(b.commit_flush(pl, false) == 0 && b.holds_residual(id) && !b.find(id)->solved);
        }
        CHECK(b.check_residual(id, 3) == kAccepted && b.check_residual(id, 2) == kSelf);
        b.note_residual(id, 3);
        CHECK(b.ready(id) && b.queued_ids == std::vector<int>{0});
        const bool touch = b.find(id)->touch_pending;
        CHECK(touch == static_cast<bool>(residual_first));
        pl = b.plan_flush(true, false, 0b01);  // shard 1 has no arena: not solved
        CHECK(pl.action == std::vector<char>{touch ? kFold : kNothing});
        pl = b.plan_flush(true, false, 0b11);
        CHECK(pl.action == std::vector<char>{kFused} && pl.later.empty());
        CHECK(flush_key(0, touch, true, mask, false) != flush_key(0, !touch, true, mask, false));
        CHECK(b.commit_flush(pl, false) == 1 && b.find(id)->solved && b.holds_residual(id));
    }
    return 0;
}

static bool bit(uint32_t v, int j) { return j >= 0 && j < 32 && (v >> j & 1); }
static auto fields(const Req &r) {
    return std::make_tuple(r.used, r.mask, r.ub, r.nunits, r.slot, r.touched, r.touch_pending, r.contributed, r.queued,
                           r.given, r.enqueued, r.solved, r.solved_host);
}
static bool same(const Book &a, const Book &b) {
    if (a.reqs.size() != b.reqs.size()) return false;
    for (size_t i = 0; i < a.reqs.size(); ++i)
        if (fields(a.reqs[i]) != fields(b.reqs[i])) return false;
    return a.free_ids == b.free_ids && a.slot_owner == b.slot_owner && a.cursor == b.cursor &&
           a.queued_ids == b.queued_ids;
}

// One random schedule of a Book against the model below, which is written from what the pool
// promises and not from the book: the reference's state per unit (recovery.c:61-131: in a
// request, touched, the lids that contributed), here per slot of R with the arena unit the
// slot stands for, a plain occupancy array, and per request what came since the last flush.
// The steps call the book as cec_pool.inc does (a flush ahead of a solve, of update pieces
// and of the end of a request with a reply queued).
struct Schedule {
    int k, m, self, cap;
    Book b;
    std::vector<int> occ, unit;  // per slot: the owner (-1 free), its arena unit
    std::vector<char> touched;   // per slot
    std::vector<uint32_t> fed;   // per slot: the data lids that contributed
    struct R {
        bool live = false;
        uint32_t mask = 0;
        int ub = 0, n = 0, slot = 0;
        uint32_t replied = 0;  // data lids replied since the last flush
        bool news = false;     // a reply or a residual since the last flush
        int touches = 0;       // first touches flushed
        uint32_t given = 0;
        bool solved = false, host = false;
    };
    std::vector<R> reqs;
    std::vector<int> free_ids;

    bool live(int id) const { return id >= 0 && id < static_cast<int>(reqs.size()) && reqs[id].live; }
    // A mask that names no data lid (k <= m): the request holds R = P from begin, so its units
    // are touched from then on; the copy itself is owed to the next flush, as a first reply's is.
    bool no_data(int id) const { return (reqs[id].mask & ((1u << k) - 1)) == 0; }
    bool touch_owed(int id) const { return reqs[id].touches == 0 && (reqs[id].replied || no_data(id)); }
    // Every unit of the request holds a residual (P, or P and replies), queued or made ...
    bool holds(int id) const {
        if (!live(id)) return false;
        for (int s = reqs[id].slot; s < reqs[id].slot + reqs[id].n; ++s)
            if (!touched[s]) return false;
        return true;
    }
    // ... and made: a flush has written it to the slots.
    bool in_place(int id) const { return holds(id) && reqs[id].touches == 1; }
    bool complete(int id) const {
        if (!live(id)) return false;
        for (int s = reqs[id].slot; s < reqs[id].slot + reqs[id].n; ++s)
            for (int j = 0; j < k; ++j)
                if (bit(reqs[id].mask, j) && !bit(fed[s], j)) return false;
        return true;
    }
    bool ready(int id) const {
        if (!complete(id)) return false;
        for (int q = k; q < k + m; ++q)
            if (q != self && bit(reqs[id].mask, q) && !bit(reqs[id].given, q)) return false;
        return true;
    }
    std::vector<int> lost(int id) const {
        std::vector<int> l;
        for (int j = 0; j < k; ++j)
            if (!bit(reqs[id].mask, j)) l.push_back(j);
        return l;
    }
    bool has_outputs(int id, bool to_host, uint32_t arenas) const {
        for (int j : lost(id))
            if (!to_host && !bit(arenas, j)) return false;
        return true;
    }
    std::vector<int> live_ids() const {
        std::vector<int> v;
        for (int id = 0; id < static_cast<int>(reqs.size()); ++id)
            if (reqs[id].live) v.push_back(id);
        return v;
    }
    int some_id() const {  // mostly live
        const std::vector<int> v = live_ids();
        return v.empty() || !rnd(0, 11) ? rnd(-1, static_cast<int>(reqs.size()) + 1) : v[rnd(0, static_cast<int>(v.size()) - 1)];
    }

    int invariants() const {
        int n_live = 0;
        std::vector<int> owner(cap, -1);
        for (int id = 0; id < static_cast<int>(reqs.size()); ++id) {
            const R &r = reqs[id];
            const Req *q = b.find(id);
            CHECK((q != nullptr) == r.live);
            if (!r.live) continue;
            ++n_live;
            CHECK(q->mask == r.mask && q->ub == r.ub && q->nunits == r.n && q->slot == r.slot);
            CHECK(r.slot >= 0 && r.n >= 1 && r.slot + r.n <= cap);  // contiguous, inside the buffer
            for (int s = r.slot; s < r.slot + r.n; ++s) {
                CHECK(owner[s] < 0);  // no slot has two owners
                owner[s] = id;
                CHECK(unit[s] == r.ub + (s - r.slot));
                CHECK(q->touched == static_cast<bool>(touched[s]) && q->contributed == fed[s]);
            }
            CHECK(q->given == r.given && q->queued == r.replied);
            CHECK(b.complete(id) == complete(id) && b.ready(id) == ready(id));
            CHECK(b.n_lost(r.mask) == static_cast<int>(lost(id).size()));
            uint32_t l = 0;
            for (int j : lost(id)) l |= 1u << j;
            CHECK(b.lost_lids(r.mask) == l);
            CHECK(q->solved == r.solved && (!r.solved || q->solved_host == r.host));
            CHECK(q->enqueued == r.news);
            CHECK(q->touch_pending == touch_owed(id) && b.holds_residual(id) == in_place(id));
            CHECK(!complete(id) || holds(id));  // nothing complete without a residual
        }
        CHECK(b.find(-1) == nullptr && b.find(static_cast<int>(reqs.size())) == nullptr);
        CHECK(owner == occ && owner == b.slot_owner && b.active() == n_live && b.capacity() == cap);
        // the queue: each id at most once, exactly the live ids with news
        std::set<int> in(b.queued_ids.begin(), b.queued_ids.end());
        CHECK(in.size() == b.queued_ids.size());
        for (int id = 0; id < static_cast<int>(reqs.size()); ++id) CHECK(in.count(id) == (reqs[id].live && reqs[id].news));
        CHECK(in.empty() || (*in.begin() >= 0 && *in.rbegin() < static_cast<int>(reqs.size())));
        return 0;
    }

    int begin() {
        int nl;
        // 1 .. min(k, m) losses: with k <= m, masks that name no data lid among them
        uint32_t mask = random_mask(k, m, self, &nl, std::min(k, m));
        int ub = rnd(0, 40), n = rnd(1, 5);
        const Book before = b;
        if (!rnd(0, 14)) {  // refused arguments
            switch (rnd(0, 3)) {
            case 0: ub = -1 - rnd(0, 3); break;
            case 1: n = -rnd(0, 2); break;
            case 2: mask ^= 1u << self; break;  // (popcount k - 1, and not naming self)
            default: mask = (mask & (mask - 1)) | 1u << (k + m + rnd(0, 3)); break;  // (k lids, one past k + m)
            }
            CHECK(b.begin(mask, ub, ub + n - 1) == -kBadArgs && same(b, before));
            return 0;
        }
        bool fits = false;  // a free run of n that does not wrap, by scanning
        for (int s = 0; s + n <= cap && !fits; ++s) {
            fits = true;
            for (int t = s; t < s + n; ++t) fits &= occ[t] < 0;
        }
        const int id = b.begin(mask, ub, ub + n - 1);
        if (n > cap || !fits) {
            CHECK(id == (n > cap ? -kTooLarge : -kNoRun) && same(b, before));
            return 0;
        }
        int want = static_cast<int>(reqs.size());  // ids are reused last in, first out
        if (!free_ids.empty()) {
            want = free_ids.back();
            free_ids.pop_back();
        } else {
            reqs.emplace_back();
        }
        CHECK(id == want);
        R r;
        r.live = true, r.mask = mask, r.ub = ub, r.n = n;
        reqs[id] = r;
        // in the queue at once, once, exactly if its first touch waits for no reply
        reqs[id].news = no_data(id);
        CHECK(std::count(b.queued_ids.begin(), b.queued_ids.end(), id) == (no_data(id) ? 1 : 0));
        const Req *q = b.find(id);
        CHECK(q && q->slot >= 0 && q->slot + n <= cap);
        reqs[id].slot = q->slot;
        for (int s = q->slot; s < q->slot + n; ++s) {
            CHECK(occ[s] < 0);
            occ[s] = id, unit[s] = ub + (s - q->slot), touched[s] = no_data(id), fed[s] = 0;
        }
        return 0;
    }

    // Replies (reply = true: lids are data peers) or residuals: mostly acceptable entries,
    // some bad, some repeated; all refused, or all noted.
    int batch(bool reply) {
        const int n = rnd(0, 9) ? rnd(1, 6) : 0;
        std::vector<int> ids(n), lids(n);
        std::vector<const void *> units(n, &cap);
        std::set<std::pair<int, int>> picked;
        for (int i = 0; i < n; ++i) {
            ids[i] = some_id();
            std::vector<int> open;
            if (live(ids[i]))
                for (int j = reply ? 0 : k; j < (reply ? k : k + m); ++j)
                    if (j != self && bit(reqs[ids[i]].mask, j) && !bit(reply ? fed[reqs[ids[i]].slot] : reqs[ids[i]].given, j) &&
                        !picked.count({ids[i], j}))
                        open.push_back(j);
            lids[i] = !open.empty() && rnd(0, 19) ? open[rnd(0, static_cast<int>(open.size()) - 1)] : rnd(-1, k + m);
            if (i && !rnd(0, 24)) ids[i] = ids[i - 1], lids[i] = lids[i - 1];  // a pair again
            if (reply && !rnd(0, 39)) units[i] = nullptr;
            picked.insert({ids[i], lids[i]});
        }
        Refusal want = kAccepted;
        int want_bad = -1;
        for (int i = 0; i < n && !want; ++i) {
            const int id = ids[i], lid = lids[i];
            if (reply) {
                if (!live(id) || !units[i] || lid < 0 || lid >= k || !bit(reqs[id].mask, lid)) want = kNoReply;
                else if (bit(fed[reqs[id].slot], lid)) want = kApplied;
            } else {
                if (!live(id)) want = kNotLive;
                else if (lost(id).size() < 2) want = kSingleLoss;
                else if (lid == self) want = kSelf;
                else if (lid < k || lid >= k + m || !bit(reqs[id].mask, lid)) want = kNotParity;
                else if (bit(reqs[id].given, lid)) want = kTwice;
            }
            if (want) want_bad = i;
        }
        if (!want && static_cast<int>(picked.size()) < n) want = kPairTwice;
        const Book before = b;
        int bad = -1;
        Refusal got;
        if (n == 1 && rnd(0, 1))  // the single forms
            got = reply ? b.check_reply(ids[0], lids[0], units[0]) : b.check_residual(ids[0], lids[0]), bad = want ? 0 : -1;
        else
            got = reply ? b.check_replies(ids.data(), lids.data(), units.data(), n, &bad)
                        : b.check_residuals(ids.data(), lids.data(), n, &bad);
        CHECK(got == want && same(b, before));  // a refused batch changes nothing
        if (want == kPairTwice) {
            int again = 0;
            CHECK(bad >= 0 && bad < n);
            for (int i = 0; i < n; ++i) again += ids[i] == ids[bad] && lids[i] == lids[bad];
            CHECK(again >= 2);
        } else if (want) {
            CHECK(bad == want_bad);  // the first bad entry
        }
        if (want) return 0;
        for (int i = 0; i < n; ++i) {
            R &r = reqs[ids[i]];
            r.news = true;
            if (reply) {
                b.note_reply(ids[i], lids[i]);
                r.replied |= 1u << lids[i];
                for (int s = r.slot; s < r.slot + r.n; ++s) touched[s] = 1, fed[s] |= 1u << lids[i];
            } else {
                b.note_residual(ids[i], lids[i]);
                r.given |= 1u << lids[i];
            }
        }
        return 0;
    }

    int flush(bool solves, bool to_host, uint32_t arenas) {
        Plan pl = b.plan_flush(solves, to_host, arenas);
        const std::vector<int> queue = b.queued_ids;
        CHECK(pl.action.size() == queue.size());
        std::vector<int> later;
        int planes = 0, fused = 0;
        for (size_t x = 0; x < queue.size(); ++x) {
            const R &r = reqs[queue[x]];
            const Req &q = *b.find(queue[x]);
            // folds exactly the lids replied since the last flush; the first touch once
            // (a mask without data lids owes its first touch without one)
            CHECK(q.queued == r.replied && q.touch_pending == touch_owed(queue[x]));
            const bool solve = solves && ready(queue[x]) && has_outputs(queue[x], to_host, arenas);
            const int n = static_cast<int>(lost(queue[x]).size());
            const Action want = solve && n <= 3 ? kFused : r.replied || touch_owed(queue[x]) ? kFold : kNothing;
            CHECK(pl.action[x] == want);
            // solved by this pass: from a residual in place, or one this very launch makes
            if (solve) CHECK(holds(queue[x]) && (in_place(queue[x]) || (touch_owed(queue[x]) && want != kNothing)));
            if (solve && n >= 4) later.push_back(queue[x]);
            if (want == kFused) ++fused;
            if (want == kFused && to_host) planes = std::max(planes, n);
        }
        CHECK(pl.later == later && pl.planes == planes);
        if (!rnd(0, 9)) {  // the launch failed: nothing committed, the book as it was
            TRY(invariants());
            pl = b.plan_flush(solves, to_host, arenas);
        }
        CHECK(b.commit_flush(pl, to_host) == fused && b.queued_ids.empty());
        b.mark_solved(pl.later, to_host);  // (pool_solve_run behind the launch)
        for (size_t x = 0; x < queue.size(); ++x) {
            R &r = reqs[queue[x]];
            if (touch_owed(queue[x])) ++r.touches;
            r.replied = 0;
            r.news = false;
            if (pl.action[x] == kFused || std::count(later.begin(), later.end(), queue[x])) r.solved = true, r.host = to_host;
        }
        return 0;
    }

    int solve() {
        TRY(flush(false, false, 0));
        const bool to_host = rnd(0, 1);
        const uint32_t arenas = to_host ? 0 : rnd(0, 3) ? (1u << k) - 1 : rng() & ((1u << k) - 1);
        const int n = rnd(0, 5);
        std::vector<int> ids(n);
        for (int &id : ids) id = some_id();
        Refusal want = kAccepted;
        int want_bad = n;
        std::set<int> listed;
        for (int x = 0; x < n && !want; ++x) {
            if (!complete(ids[x])) want = kIncomplete;  // (or no such request)
            else if (!listed.insert(ids[x]).second) want = kListedTwice;
            else if (!ready(ids[x])) want = kNotReady;
            else if (!has_outputs(ids[x], to_host, arenas)) want = kNoOutput;
            if (want) want_bad = x;
        }
        const Book before = b;
        int bad = -1;
        CHECK(b.check_solve(ids.data(), n, to_host, arenas, &bad) == want && bad == want_bad && same(b, before));
        if (want) return 0;
        for (int id : ids) CHECK(in_place(id));  // no accepted list reads slots that hold no residual
        b.mark_solved(ids, to_host);
        for (int id : ids) reqs[id].solved = true, reqs[id].host = to_host;
        return 0;
    }

    // The pieces of an update: the model's units with touched && !contributed(peer), cut at
    // request and update boundaries.
    int update() {
        TRY(flush(false, false, 0));
        const std::vector<Span> spans = b.touched_spans();
        const int n_upd = rnd(1, 3);
        for (int u = 0; u < n_upd; ++u) {
            const int peer = rnd(0, k - 1);
            const uint64_t addr = static_cast<uint64_t>(rnd(0, 44)) * kUnit + (rnd(0, 2) ? 0 : rnd(0, 4095));
            const uint32_t len = rnd(0, 3) ? rnd(1, 3 * 4096) : rnd(0, 1) ? 0 : rnd(1, 12) * kUnit;
            std::set<std::tuple<int, uint64_t, uint64_t, uint32_t>> want, got;
            int want_units = 0;
            for (int id : live_ids()) {
                R &r = reqs[id];
                uint64_t lo = 0, hi = 0;  // the request's units are adjacent: their pieces are one
                for (int s = r.slot; s < r.slot + r.n; ++s) {
                    if (!touched[s] || bit(fed[s], peer)) continue;
                    const uint64_t ua = static_cast<uint64_t>(unit[s]) * kUnit, ub = ua + kUnit;
                    const uint64_t a = std::max(ua, addr), e = std::min<uint64_t>(ub, addr + len);
                    if (a >= e) continue;
                    ++want_units;
                    if (lo == hi) lo = a;
                    hi = e;
                }
                if (lo == hi) continue;
                const uint64_t base = static_cast<uint64_t>(r.ub) * kUnit;
                want.insert({id, static_cast<uint64_t>(r.slot) * kUnit + (lo - base), lo - addr, static_cast<uint32_t>(hi - lo)});
                r.solved = false;  // R moved on
            }
            std::vector<Piece> pieces;
            const int units = b.pieces(spans, addr, len, peer, u, pieces);
            for (const Piece &pc : pieces) {
                CHECK(pc.upd == u);
                CHECK(got.insert({pc.id, pc.r_off, pc.d_off, pc.len}).second);
            }
            CHECK(got == want && units == want_units);
        }
        return 0;
    }

    int end() {
        const int id = some_id();
        if (!live(id)) {
            CHECK(!b.find(id));
            return 0;
        }
        if (b.find(id)->queued) TRY(flush(false, false, 0));  // a reply still queued: folded first
        b.end(id);
        R &r = reqs[id];
        for (int s = r.slot; s < r.slot + r.n; ++s) occ[s] = -1;
        r = R{};
        free_ids.push_back(id);
        return 0;
    }

    int run(int steps) {
        b = Book(k, m, self, cap);
        occ.assign(cap, -1), unit.assign(cap, 0), touched.assign(cap, 0), fed.assign(cap, 0);
        for (int step = 0; step < steps; ++step) {
            const int op = rnd(0, 99);
            if (op < 20) TRY(begin());
            else if (op < 45) TRY(batch(true));
            else if (op < 60) TRY(batch(false));
            else if (op < 65) TRY(flush(false, false, 0));
            else if (op < 71) TRY(flush(true, false, rnd(0, 1) ? (1u << k) - 1 : rng() & ((1u << k) - 1)));
            else if (op < 76) TRY(flush(true, true, 0));
            else if (op < 83) TRY(solve());
            else if (op < 90) TRY(update());
            else TRY(end());
            TRY(invariants());
        }
        return 0;
    }
};

static int schedules() {
    for (int round = 0; round < 2000; ++round) {
        rng.seed(0xB00C0000u + round);
        Schedule s;
        s.k = rnd(1, kMaxK), s.m = rnd(1, kMaxM), s.self = rnd(s.k, s.k + s.m - 1), s.cap = rnd(1, 24);
        if (s.run(rnd(200, 400))) {
            std::printf("schedule %d: RS(%d,%d), self %d, capacity %d\n", round, s.k, s.m, s.self, s.cap);
            return 1;
        }
    }
    return 0;
}

int main() {
    if (slots() || readiness_and_batches() || keys() || queue_reuse() || no_data_lids() || schedules()) return 1;
    std::printf("ok\n");
    return 0;
}
