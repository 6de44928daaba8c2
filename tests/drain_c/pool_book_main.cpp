// The recovery pool's host bookkeeping (cocytus_amd/csrc/cec_poolbook.hpp, the shipped
// header): readiness, the all-or-nothing check of a residual batch, the flush's slot layout
// and pattern keys, against brute force over random requests.  Built with ASan + UBSan by
// tests/test_pool_losses_abi.py; prints "ok".
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
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

static std::mt19937 rng(0xC0C7);
static int rnd(int lo, int hi) { return lo + static_cast<int>(rng() % static_cast<unsigned>(hi - lo + 1)); }

// A random recovery mask of RS(k, m) that names `self`: n lost data lids, n parities.
static uint32_t random_mask(int k, int m, int self, int *n_out) {
    const int n = rnd(1, std::min(k, m));
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

static int readiness_and_batches() {
    for (int round = 0; round < 4000; ++round) {
        const int k = rnd(1, kMaxK), m = rnd(1, kMaxM), self = rnd(k, k + m - 1);
        const int nreq = rnd(1, 12);
        std::vector<Req> reqs(nreq);
        std::vector<int> nl(nreq);
        for (int i = 0; i < nreq; ++i) {
            Req &r = reqs[i];
            r.live = rnd(0, 9) != 0;
            r.mask = random_mask(k, m, self, &nl[i]);
            CHECK(__builtin_popcount(r.mask) == k && n_lost(k, r.mask) == nl[i]);
            CHECK(__builtin_popcount(needed(k, self, r.mask)) == nl[i] - 1 && !(needed(k, self, r.mask) & (1u << self)));
            r.contributed = rnd(0, 2) ? data_lids(k, r.mask) : data_lids(k, r.mask) & rng();
            r.given = rnd(0, 2) ? needed(k, self, r.mask) & rng() : needed(k, self, r.mask);
            // brute force
            bool comp = r.live, rdy = r.live;
            for (int j = 0; j < k; ++j)
                if ((r.mask >> j & 1) && !(r.contributed >> j & 1)) comp = rdy = false;
            for (int q = k; q < k + m; ++q)
                if (q != self && (r.mask >> q & 1) && !(r.given >> q & 1)) rdy = false;
            CHECK(complete(k, r) == comp && ready(k, self, r) == rdy);
            if (nl[i] == 1) CHECK(ready(k, self, r) == complete(k, r));
        }
        auto req_of = [&](int id) { return id >= 0 && id < nreq ? reqs[id] : Req{}; };
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
            if (!r.live) why = kNotLive;
            else if (n_lost(k, r.mask) < 2) why = kSingleLoss;
            else if (lids[i] == self) why = kSelf;
            else if (lids[i] < k || lids[i] >= k + m || !(r.mask >> lids[i] & 1)) why = kNotParity;
            else if (r.given >> lids[i] & 1) why = kTwice;
            CHECK(check_residual(k, m, self, r, lids[i]) == why);
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
        const Refusal got = check_residuals(k, m, self, ids.data(), lids.data(), n, req_of, &bad);
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

// The flush queue over reused ids: requests begin (ids reused last in, first out, the mark
// cleared as begin does), are queued by replies and residuals, end while queued or not, and
// are flushed.  The queue must hold each live queued id exactly once and no ended one --
// the case of add_residual; end; begin; add_peer among them, stated first.
static int queue() {
    {
        std::vector<int> q;
        bool mark = false;
        enqueue(q, mark, 7);  // add_residual
        dequeue(q, mark, 7);  // end
        CHECK(q.empty() && !mark);
        mark = false;         // begin reuses id 7
        enqueue(q, mark, 7);  // add_peer
        enqueue(q, mark, 7);
        CHECK(q.size() == 1 && q[0] == 7 && mark);
    }
    for (int round = 0; round < 2000; ++round) {
        const int cap = rnd(1, 12);
        std::vector<char> used(cap, 0);
        bool marks[12] = {};
        std::vector<int> free_ids, q;
        int next = 0;
        for (int step = 0; step < 200; ++step) {
            const int op = rnd(0, 9);
            if (op < 3) {  // begin
                int id;
                if (!free_ids.empty()) {
                    id = free_ids.back();
                    free_ids.pop_back();
                } else if (next < cap) {
                    id = next++;
                } else {
                    continue;
                }
                used[id] = 1;
                marks[id] = false;  // r = Req{}
            } else if (op < 7) {  // a reply or a residual
                const int id = rnd(0, cap - 1);
                if (used[id]) enqueue(q, marks[id], id);
            } else if (op < 9) {  // end
                const int id = rnd(0, cap - 1);
                if (!used[id]) continue;
                dequeue(q, marks[id], id);
                used[id] = 0;
                free_ids.push_back(id);
            } else {  // flush
                for (int id : q) marks[id] = false;
                q.clear();
            }
            std::set<int> in(q.begin(), q.end());
            CHECK(in.size() == q.size() && static_cast<int>(q.size()) <= cap);  // each id once
            for (int id = 0; id < cap; ++id) CHECK((in.count(id) == 1) == (used[id] && marks[id]));
        }
    }
    return 0;
}

int main() {
    if (slots() || readiness_and_batches() || keys() || queue()) return 1;
    std::printf("ok\n");
    return 0;
}
