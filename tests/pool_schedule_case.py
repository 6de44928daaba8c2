"""Random schedules of the recovery pool against a per-unit model.

cec_recovery_pool is the most stateful device component of the library: one object holds many
requests of different masks and loss counts, and its first touches, folds, fused and deferred
solves, host planes, given residuals, diffs and its append-only pattern table all share the same
4 KiB residual slots.  This file holds what a random schedule of pool calls needs on the CPU:

  Model      what the pool must do, call by call, written from include/cocytus_ec.h and the
             reference's per-unit rules (recovery.c:61-131, memcached.c:7842-7922).  numpy
             only: nothing of cocytus_amd, of oracle/ or of poolbook::Book is read; the coding
             matrix is a parameter.  Its arithmetic is recovery_case.residual_of / solve_lost
             and kernel_matrix_case.MUL.
  Generator  draws each step from the model's state and its own seeded generator alone, so a
             dry run without a GPU is step for step the GPU run.
  schedule   the loop of both: tests/test_pool_schedule_case.py runs it dry (model tie-down,
             coverage counters), tests/test_gpu_pool_schedules.py runs it with a pool.

THE MODEL'S STATE.  Per live request (named by the generator's own handle; the runner maps
handles to the ids begin returns): mask and unit range; R, None until the first touch has been
flushed; contributed, queued, touch_pending; the replies still queued; the given residuals;
enqueued; solved, solved_host; the last solved bytes per lost lid.  Besides: the queue, the
stripe set (k data and m parity arenas, consistent at every step), of which P = the leader's
parity arena is what the pool reads, and the two output slabs (device, pinned) in the sentinel.

THE RULES, each with the line of include/cocytus_ec.h that states it:

  * A plain flush empties the queue.  A request it makes ready is not solved by a later
    flush_solve; only an explicit solve does that.           (cec_recovery_pool_flush)
  * flush_solve solves only requests that are queued and ready and whose lost lids all have an
    arena in `out`; a request with a NULL arena is folded only.  (cec_recovery_pool_flush_solve)
  * Three or fewer losses are solved in the fold's own launch, four or more behind it.
                                                              (cec_recovery_pool_flush_solve)
  * fold_update(s), solve, residual, and end of a request with a queued reply all flush first.
    (cec_recovery_pool_fold_update, _fold_updates, _solve, _residual, _end)
  * A diff folds into every touched live request it meets whose `contributed` lacks that lid,
    lost lids included.  It clears `solved`; the request stays ready and out of the queue;
    overlapping requests each take the diff.                 (cec_recovery_pool_fold_update)
  * Given residuals never move.                              (cec_recovery_pool_add_residual)
  * A mask with no data lid is touched and queued from begin.
    (A MASK THAT NAMES NO DATA LID, pool)
  * output(rid, x) is None unless the last solve of rid was a _host one and `solved` still
    holds.                                                   (cec_recovery_pool_output)
  * residual of a live request that holds none (its mask names data lids, no reply ever
    queued) is CEC_EINVAL: nothing copied, nothing flushed.  (cec_recovery_pool_residual)
  * The first touch and every fold read P at the flush, so the caller folds a diff BEFORE it
    applies it to P.                                         (A MASK THAT NAMES NO DATA LID, pool)

The flush's return value: the requests solved for a pass that solves, else the requests with a
reply queued.  The key of a flush pattern, counted for the coverage of the table's growth, is
(queued, touch, fused, mask if fused, to_host if fused) as cec_poolbook.hpp's flush_key packs
it; the table starts again when a flush finds the engine changed.

PLACEMENT.  The model knows nothing of where the pool puts a request.  begin is predicted only
where every placement agrees: with L live requests and F free units an n-unit request fits
under any placement if F >= (L + 1)(n - 1) + 1 (L requests cut the free units into at most
L + 1 runs; if each held at most n - 1 units there would be at most (L + 1)(n - 1) free), and
cannot fit if F < n or n > capacity (CEC_EFULL, nothing changed).  The generator draws nothing
in between.

RACES THE GENERATOR AVOIDS.  Two live requests may cover the same arena units.  Solved into
arenas by one call, both would write the same bytes of a lost lid's arena, in no defined
order; the generator never lists two such requests in one arena solve and turns a flush_solve
that would solve two into a flush_solve_host (whose planes are slot-addressed).
"""
from __future__ import annotations

import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import recovery_case as rc  # noqa: E402
from kernel_matrix_case import MUL, SENT, TILE as U  # noqa: E402

CAP = 24                 # the pool's capacity in units
ARENA_UNITS = 32
ARENA = ARENA_UNITS * U
EINVAL, EFULL = -1, -7   # cec_status
FUSED_MAX = 3            # kFusedLosses: one launch holds R' and three shards

# (k, m) -> the leader, the seeds and the schedule length.  The length is the smallest multiple
# of 100 steps at which every coverage condition of tests/test_pool_schedule_case.py holds
# for every seed listed.  The seeds are the first two, counting from 1, whose schedules meet
# them within 400 steps (coverage_gaps below says what a seed lacks); a change to the generator
# or to the conditions means choosing them again, never dropping a condition.
CODES = {
    (3, 2): dict(leader=4, seeds=(2, 4), steps=400),      # highest parity
    (6, 4): dict(leader=6, seeds=(2, 4), steps=400),      # lowest parity
    (3, 4): dict(leader=3, seeds=(5, 8), steps=300),      # lowest parity
    (10, 8): dict(leader=17, seeds=(24, 30), steps=400),  # highest parity
}


def bits(x: int) -> list:
    return [j for j in range(32) if (x >> j) & 1]


class Req:
    def __init__(self, h, mask, ub, n):
        self.h, self.mask, self.ub, self.n = h, mask, ub, n
        self.R = None
        self.touched = self.touch_pending = False
        self.contributed = self.queued = 0
        self.Q = {}        # queued replies {data lid: bytes}
        self.given = {}    # {parity lid: bytes}, static
        self.enqueued = self.solved = self.solved_host = False
        self.out = {}      # the last solved bytes {lost lid: bytes}
        # for the tie-down and the coverage counters only
        self.input_seen = self.dirty = False
        self.ever_arena = self.ever_host = False
        self.lost_diff_after_solve = False

    @property
    def span(self):
        return slice(self.ub * U, (self.ub + self.n) * U)

    def row(self):
        return dict(h=self.h, mask=hex(self.mask), units=[self.ub, self.ub + self.n - 1],
                    holds_R=self.R is not None, touched=self.touched, touch_pending=self.touch_pending,
                    contributed=bits(self.contributed), queued=bits(self.queued), given=sorted(self.given),
                    enqueued=self.enqueued, solved=self.solved, solved_host=self.solved_host)


class Outcome:
    """What one step must do: its return value, the bytes to hand to the pool (replies,
    residuals, diffs, in the step's order), the bytes a read returns, and the ranges of P
    the test applies afterwards.  (The outputs and the flags are read off the model.)"""

    def __init__(self):
        self.ret = None
        self.payload = []
        self.read = None
        self.p_ranges = []


class Model:
    def __init__(self, k, m, mat, leader, seed):
        self.k, self.m, self.mat, self.leader = k, m, [int(v) for v in mat], leader
        rng = np.random.default_rng([0x9005, k, m, seed])
        self.D = rng.integers(0, 256, (k, ARENA), dtype=np.uint8)
        self.PAR = np.stack(rc.encode(self.mat, k, m, list(self.D)))
        self.out = {"dev": np.full((k, ARENA), SENT, np.uint8), "pin": np.full((k, ARENA), SENT, np.uint8)}
        self.reqs: dict = {}
        self.queue: list = []
        self.engine = 0            # toggled by the engine step; the runner maps 0 to its starting engine
        self.table_engine = None
        self.keys: set = set()
        self.ev = collections.Counter()
        self.tie = []              # (step, handle, losses, equal) of every solve of a clean request
        self.step_no = -1
        self.ended_masks: list = []  # masks ended since the last begin

    # ---------------------------------------------------------------- state
    @property
    def P(self):
        return self.PAR[self.leader - self.k]

    def coef(self, lid):
        return self.mat[self.leader * self.k + lid]

    def used(self):
        return sum(r.n for r in self.reqs.values())

    def free(self):
        return CAP - self.used()

    def fits(self, n):
        return self.free() >= (len(self.reqs) + 1) * (n - 1) + 1

    def data_lids(self, r):
        return r.mask & ((1 << self.k) - 1)

    def lost(self, r):
        return rc.lost_of(self.k, r.mask)

    def pars(self, r):
        return rc.pars_of(self.k, self.m, r.mask)

    def complete(self, r):
        return r.contributed == self.data_lids(r)

    def ready(self, r):
        return self.complete(r) and all(q in r.given for q in self.pars(r) if q != self.leader)

    def output(self, r, x):
        lost = self.lost(r)
        return r.out[lost[x]] if r.solved and r.solved_host and x < len(lost) else None

    def table(self):
        return [r.row() for r in self.reqs.values()]

    # ---------------------------------------------------------------- the pool's passes
    def _enqueue(self, r):
        if not r.enqueued:
            self.queue.append(r.h)
        r.enqueued = True

    def _solve(self, r, to_host, slab):
        res = {q: (r.R if q == self.leader else r.given[q]) for q in self.pars(r)}
        r.out = rc.solve_lost(self.mat, self.k, self.m, r.mask, res)
        n = len(r.out)
        if not to_host:
            for j, v in r.out.items():
                self.out[slab][j, r.span] = v
        if to_host and r.ever_arena:
            self.ev["host_after_arena"] += 1
        if not to_host and r.ever_host:
            self.ev["arena_after_host"] += 1
        if r.lost_diff_after_solve:
            self.ev["resolved_after_lost_diff"] += 1
            r.lost_diff_after_solve = False
        r.ever_host |= to_host
        r.ever_arena |= not to_host
        r.solved, r.solved_host = True, to_host
        if not self.data_lids(r):
            self.ev["no_data_solved"] += 1
        if not r.dirty:
            ok = all(np.array_equal(v, self.D[j, r.span]) for j, v in r.out.items())
            self.tie.append((self.step_no, r.h, n, ok))

    def _flush(self, solves=False, to_host=False, slab=None, none_lid=None):
        if not self.queue:
            return 0
        if self.table_engine != self.engine:
            self.table_engine = self.engine
            self.keys = set()
        folded = n_solved = 0
        kinds = set()
        for h in self.queue:
            r = self.reqs[h]
            folds = bool(r.queued or r.touch_pending)
            n = len(self.lost(r))
            can = solves and self.ready(r) and (to_host or none_lid not in self.lost(r))
            fused = can and n <= FUSED_MAX
            if solves and self.ready(r) and not can:
                self.ev["null_arena_folded_only"] += 1
            if folds or fused:
                self.keys.add((r.queued, r.touch_pending, fused, r.mask if fused else 0, bool(to_host and fused)))
                self.ev["max_keys"] = max(self.ev["max_keys"], len(self.keys))
            if folds:
                base = self.P[r.span] if r.touch_pending else r.R
                r.R = rc.residual_of(self.mat, self.k, self.leader, base, {j: r.Q[j] for j in bits(r.queued)})
                kinds.add("touch" if r.touch_pending else "fold")
            folded += bool(r.queued)
            r.queued, r.Q = 0, {}
            r.touch_pending = r.enqueued = False
            if can:
                self._solve(r, to_host, slab)
                n_solved += 1
                self.ev[f"fused_{n}" if fused else "deferred"] += 1
                kinds.add("fused" if fused else "deferred")
        self.queue = []
        if len(kinds) == 4:
            self.ev["flush_of_all_four"] += 1
        return n_solved if solves else folded

    def _fold(self, peer, addr, diff):
        """One diff into R (the flush done); returns the units folded."""
        a, b = addr, addr + len(diff)
        units, takers = 0, []
        for r in self.reqs.values():
            base = r.ub * U
            lo, hi = max(a, base), min(b, base + r.n * U)
            if not r.touched or lo >= hi or (r.contributed >> peer) & 1:
                continue
            r.R[lo - base:hi - base] ^= MUL[self.coef(peer)][diff[lo - a:hi - a]]
            units += (hi - 1) // U - lo // U + 1
            if peer in self.lost(r) and r.solved:
                r.lost_diff_after_solve = True
            r.solved = r.solved_host = False
            if any(lo < h2 and l2 < hi for _h, l2, h2 in takers):
                self.ev["overlapping_both_take"] += 1
            takers.append((r.h, lo, hi))
        return units, takers

    def _set(self, peer, addr, diff):
        """The SET itself: the data shard and every parity arena move on (P with them: the
        test applies the diff to the leader's arena after the fold, as the pool's caller)."""
        a, b = addr, addr + len(diff)
        self.D[peer, a:b] ^= diff
        for p in range(self.m):
            self.PAR[p, a:b] ^= MUL[self.mat[(self.k + p) * self.k + peer]][diff]
        for r in self.reqs.values():
            if r.input_seen and a < (r.ub + r.n) * U and r.ub * U < b:
                r.dirty = True

    @staticmethod
    def diff_bytes(u):
        return np.random.default_rng([0xD1FF, u["dseed"]]).integers(0, 256, u["len"], dtype=np.uint8)

    # ---------------------------------------------------------------- one step
    def apply(self, step, step_no=-1) -> Outcome:
        self.step_no = step_no
        o = Outcome()
        op = step["op"]
        if op == "begin":
            n = step["ue"] - step["ub"] + 1
            if step["expect"] == "full":
                assert n > CAP or self.free() < n, step
                o.ret = EFULL
                self.ev["full_probe"] += 1
            else:
                assert self.fits(n) and step["ue"] < ARENA_UNITS, step
                if self.ended_masks and self.free() < CAP / 2 and any(x != step["mask"] for x in self.ended_masks):
                    self.ev["reuse_other_mask"] += 1
                self.ended_masks = []
                r = self.reqs[step["h"]] = Req(step["h"], step["mask"], step["ub"], n)
                if not self.data_lids(r):  # touched and queued from begin
                    r.touched = r.touch_pending = r.input_seen = True
                    self._enqueue(r)
                o.ret = "id"
        elif op == "replies":
            for h, j, _way in step["items"]:
                r = self.reqs[h]
                assert (r.mask >> j) & 1 and j < self.k and not (r.contributed >> j) & 1, step
                r.Q[j] = self.D[j, r.span].copy()
                o.payload.append(r.Q[j])
                if not r.touched:
                    r.touched = r.touch_pending = True
                r.contributed |= 1 << j
                r.queued |= 1 << j
                r.input_seen = True
                self._enqueue(r)
        elif op == "residuals":
            for h, q, _way in step["items"]:
                r = self.reqs[h]
                assert q in self.pars(r) and q != self.leader and q not in r.given and len(self.lost(r)) >= 2, step
                r.given[q] = rc.residual_of(self.mat, self.k, q, self.PAR[q - self.k, r.span],
                                            {j: self.D[j, r.span] for j in bits(self.data_lids(r))})
                o.payload.append(r.given[q])
                r.input_seen = True
                self._enqueue(r)
        elif op == "flush":
            o.ret = self._flush()
        elif op == "flush_solve":
            o.ret = self._flush(True, False, step["slab"], step["none_lid"])
        elif op == "flush_solve_host":
            o.ret = self._flush(True, True)
        elif op in ("solve", "solve_host"):
            self._flush()
            rs = [self.reqs[h] for h in step["hs"]]
            if all(self.ready(r) for r in rs):
                assert step["bad"] is None and len(set(step["hs"])) == len(rs), step
                if len({len(self.lost(r)) for r in rs}) >= 2:
                    self.ev["mixed_solve_list"] += 1
                for r in rs:
                    self._solve(r, op == "solve_host", step.get("slab"))
                self.ev["explicit_solve"] += 1
                o.ret = 0
            else:
                assert step["bad"] is not None, step
                self.ev["solve_refused"] += 1
                o.ret = EINVAL
        elif op == "fold_update":
            self._flush()
            diff = self.diff_bytes(step)
            o.payload.append(diff)
            o.ret, _ = self._fold(step["peer"], step["addr"], diff)
            self._set(step["peer"], step["addr"], diff)
            o.p_ranges.append((step["addr"], step["len"]))
            self.ev["fold_units"] += o.ret
        elif op == "fold_updates":
            self._flush()
            o.ret, met = [], []
            for u in step["ups"]:
                diff = self.diff_bytes(u)
                o.payload.append(diff)
                units, takers = self._fold(u["peer"], u["addr"], diff)
                o.ret.append(units)
                met.append(takers)
            # two updates' pieces meeting in one request's R go to separate waves
            if any(h1 == h2 and l1 < e2 and l2 < e1 for x in range(len(met)) for y in range(x)
                   for h1, l1, e1 in met[x] for h2, l2, e2 in met[y]):
                self.ev["two_waves"] += 1
            for u, diff in zip(step["ups"], o.payload):
                self._set(u["peer"], u["addr"], diff)
                o.p_ranges.append((u["addr"], u["len"]))
            self.ev["fold_units"] += sum(o.ret)
        elif op == "residual":
            r = self.reqs[step["h"]]
            if not r.touched:
                o.ret = EINVAL
                self.ev["residual_refused"] += 1
            else:
                self._flush()
                o.ret, o.read = 0, r.R.copy()
        elif op == "end":
            r = self.reqs[step["h"]]
            if r.queued:
                self.ev["end_reply_queued"] += 1
                self._flush()
            elif r.enqueued and not r.touch_pending:
                self.ev["end_residual_queued"] += 1
            if r.enqueued:
                self.queue.remove(r.h)
            self.ended_masks.append(r.mask)
            del self.reqs[r.h]
        elif op == "engine":
            self.engine ^= 1
            if self.reqs:
                self.ev["engine_switch_live"] += 1
        else:
            raise ValueError(op)
        return o


class Generator:
    """The next step, from the model's state and a seeded generator alone."""

    def __init__(self, model: Model, seed: int):
        self.M = model
        self.rng = np.random.default_rng([0x5C4ED, model.k, model.m, seed])
        self.next_h = 0
        self.next_dseed = 0

    # small helpers over the generator
    def ri(self, lo, hi):  # inclusive
        return int(self.rng.integers(lo, hi + 1))

    def chance(self, p):
        return bool(self.rng.random() < p)

    def pick(self, xs):
        return xs[self.ri(0, len(xs) - 1)]

    def some(self, xs, n):
        return [xs[i] for i in sorted(self.rng.permutation(len(xs))[:n].tolist())]

    def stream(self):
        return self.ri(0, 2)  # None and two streams of the runner's

    # ---------------------------------------------------------------- candidates
    def pending_replies(self):
        M = self.M
        return {r.h: [j for j in bits(M.data_lids(r) & ~r.contributed)] for r in M.reqs.values()
                if M.data_lids(r) & ~r.contributed}

    def pending_residuals(self):
        M = self.M
        out = {}
        for r in M.reqs.values():
            need = [q for q in M.pars(r) if q != M.leader and q not in r.given]
            if need and len(M.lost(r)) >= 2:
                out[r.h] = need
        return out

    def conflict(self, a, b):
        """Both solved into arenas by one call would write the same bytes."""
        M = self.M
        return a.ub < b.ub + b.n and b.ub < a.ub + a.n and set(M.lost(a)) & set(M.lost(b))

    def mask(self):
        M = self.M
        k, m = M.k, M.m
        top = min(k, m)
        n = self.ri(1, min(top, FUSED_MAX)) if self.chance(0.5) else self.ri(1, top)  # fused and deferred alike
        lost = self.some(list(range(k)), n)
        others = [p for p in range(k, k + m) if p != M.leader]
        pars = sorted([M.leader] + self.some(others, n - 1))
        return rc.mask_of(k, lost, pars)

    def update(self):
        M = self.M
        ln = self.ri(1, 64) if self.chance(0.3) else self.ri(1, 9000)
        touched = [r for r in M.reqs.values() if r.touched]
        if touched and self.chance(0.7):
            r = self.pick(touched)
            addr = r.ub * U + self.ri(-ln + 1, r.n * U - 1)
        else:
            addr = self.ri(0, ARENA - ln)
        addr = min(max(addr, 0), ARENA - ln)
        if self.chance(0.5):
            addr &= ~15
        if touched and self.chance(0.5):  # a lid some touched request has lost or not yet heard from
            r = self.pick(touched)
            peer = self.pick([j for j in range(M.k) if not (r.contributed >> j) & 1])
        else:
            peer = self.ri(0, M.k - 1)
        self.next_dseed += 1
        return dict(peer=peer, addr=addr, len=ln, dseed=self.next_dseed, boff=self.ri(0, 15))

    # ---------------------------------------------------------------- the draw
    def next(self) -> dict:
        M = self.M
        live = list(M.reqs.values())
        used = M.used()
        rep, res = self.pending_replies(), self.pending_residuals()
        ready = [r for r in live if M.ready(r)]
        w = {
            "begin": 10 if used < 10 else 5 if used < 16 else 2,
            "probe": 0.4,
            "replies": 10 if rep else 0,
            "residuals": 6 if res else 0,
            "flush": 1.5 if M.queue else 0.2,
            "flush_solve": 4 if M.queue else 0.2,
            "flush_solve_host": 3 if M.queue else 0.2,
            "solve": 2.5 if ready else 0,
            "solve_host": 2.5 if ready else 0,
            "fold_update": 3,
            "fold_updates": 2,
            "residual": 1.5 if live else 0,
            "end": (1 + 8 * used / CAP) if live else 0,
            "engine": 0.2,
        }
        names = list(w)
        p = np.array([w[n] for n in names], float)
        op = names[int(self.rng.choice(len(names), p=p / p.sum()))]
        return getattr(self, "g_" + op)(live, ready, rep, res)

    def g_begin(self, live, *_):
        M = self.M
        n = self.ri(1, 3)
        while not M.fits(n):
            n -= 1
            if n == 0:  # no unit free
                return self.g_probe(live)
        if live and self.chance(0.35):  # over a live request's units
            r = self.pick(live)
            ub = self.ri(r.ub - n + 1, r.ub + r.n - 1)
        else:
            ub = self.ri(0, ARENA_UNITS - n)
        ub = min(max(ub, 0), ARENA_UNITS - n)
        self.next_h += 1
        return dict(op="begin", h=self.next_h, mask=self.mask(), ub=ub, ue=ub + n - 1, expect="ok")

    def g_probe(self, live, *_):
        M = self.M
        if M.free() < 3 and self.chance(0.7):
            n = self.ri(M.free() + 1, 3)  # F < n
        else:
            n = self.ri(CAP + 1, ARENA_UNITS)  # n > capacity
        ub = self.ri(0, ARENA_UNITS - n)
        return dict(op="begin", h=0, mask=self.mask(), ub=ub, ue=ub + n - 1, expect="full")

    def _items(self, pending, ways):
        """(handle, lid, way) of one call: most of one request's, often some of another's."""
        items = []
        hs = self.some(list(pending), min(len(pending), self.pick([1, 1, 2, 3])))
        for h in hs:
            lids = pending[h]
            take = len(lids) if self.chance(0.4) else self.ri(1, len(lids))
            items += [[h, j, self.pick(ways)] for j in self.some(lids, take)]
        order = self.rng.permutation(len(items)).tolist()
        return [items[i] for i in order]

    def g_replies(self, live, ready, rep, res):
        items = self._items(rep, ["pageable", "device", "staging"])
        return dict(op="replies", items=items, batch=len(items) > 1 or self.chance(0.5))

    def g_residuals(self, live, ready, rep, res):
        items = self._items(res, ["pageable", "device", "staging"])
        return dict(op="residuals", items=items, batch=len(items) > 1 or self.chance(0.5))

    def g_flush(self, *_):
        return dict(op="flush", stream=self.stream())

    def g_flush_solve(self, *_):
        M = self.M
        none_lid = None
        if self.chance(0.25):  # one arena NULL: often a lid that a request about to be solved has lost
            hit = sorted({j for h in M.queue if M.ready(M.reqs[h]) for j in M.lost(M.reqs[h])})
            none_lid = self.pick(hit) if hit and self.chance(0.7) else self.ri(0, M.k - 1)
        would = [M.reqs[h] for h in M.queue if M.ready(M.reqs[h]) and none_lid not in M.lost(M.reqs[h])]
        if any(self.conflict(a, b) for x, a in enumerate(would) for b in would[:x]):
            return self.g_flush_solve_host()
        return dict(op="flush_solve", slab=self.pick(["dev", "pin"]), none_lid=none_lid, stream=self.stream())

    def g_flush_solve_host(self, *_):
        return dict(op="flush_solve_host", stream=self.stream())

    def _solve_list(self, ready, arenas):
        M = self.M
        want = self.some(ready, self.ri(1, min(5, len(ready))))
        hs = []
        for r in want:
            if not arenas or not any(self.conflict(r, M.reqs[h]) for h in hs):
                hs.append(r.h)
        order = self.rng.permutation(len(hs)).tolist()
        hs = [hs[i] for i in order]
        bad = None
        unready = [r.h for r in M.reqs.values() if not M.ready(r)]
        if unready and self.chance(0.15):  # a request that is not ready, slipped in: nothing solved
            bad = self.pick(unready)
            hs.insert(self.ri(0, len(hs)), bad)
        return hs, bad

    def g_solve(self, live, ready, *_):
        hs, bad = self._solve_list(ready, True)
        return dict(op="solve", hs=hs, bad=bad, slab=self.pick(["dev", "pin"]), stream=self.stream())

    def g_solve_host(self, live, ready, *_):
        hs, bad = self._solve_list(ready, False)
        return dict(op="solve_host", hs=hs, bad=bad, stream=self.stream())

    def g_fold_update(self, *_):
        return dict(op="fold_update", way=self.pick(["pageable", "device"]), stream=self.stream(), **self.update())

    def g_fold_updates(self, *_):
        ups = []
        for _x in range(self.ri(1, 12)):
            u = self.update()
            if ups and self.chance(0.4):  # over the one before
                prev = ups[-1]
                u["addr"] = min(max(prev["addr"] + self.ri(-u["len"] + 1, prev["len"] - 1), 0), ARENA - u["len"])
            ups.append(u)
        return dict(op="fold_updates", ups=ups, stream=self.stream())

    def g_residual(self, live, *_):
        bare = [r for r in live if not r.touched]  # holds no residual: refused
        r = self.pick(bare) if bare and self.chance(0.2) else self.pick(live)
        return dict(op="residual", h=r.h, way=self.pick(["host", "device"]), stream=self.stream())

    def g_end(self, live, *_):
        solved = [r for r in live if r.solved]
        queued = [r for r in live if r.enqueued]  # a reply, a residual or its first touch still queued
        r = (self.pick(queued) if queued and self.chance(0.2) else
             self.pick(solved) if solved and self.chance(0.6) else self.pick(live))
        return dict(op="end", h=r.h)

    def g_engine(self, *_):
        return dict(op="engine")


def schedule(k, m, mat, seed, n_steps=None, on_step=None, on_start=None):
    """Run CODES[(k, m)]'s schedule of `seed`: on_start(model) before the first step, then
    on_step(i, step, outcome, model) after the model has taken step i (the GPU runner drives
    the pool there).  Returns (model, steps)."""
    cfg = CODES[(k, m)]
    model = Model(k, m, mat, cfg["leader"], seed)
    gen = Generator(model, seed)
    if on_start:
        on_start(model)
    steps = []
    for i in range(cfg["steps"] if n_steps is None else n_steps):
        step = gen.next()
        steps.append(step)
        out = model.apply(step, i)
        if on_step:
            on_step(i, step, out, model)
    return model, steps


def finish(model: Model, on_step, first_index: int) -> None:
    """The end of a run with a pool: read the residual of every live request that holds one,
    then end them all.  (Not part of the schedule: the coverage is counted before it.)"""
    tail = [dict(op="residual", h=r.h, way="host", stream=0) for r in model.reqs.values() if r.touched]
    tail += [dict(op="end", h=h) for h in model.reqs]
    for i, step in enumerate(tail, first_index):
        on_step(i, step, model.apply(step, i), model)


def coverage_gaps(model: Model) -> list:
    """The coverage conditions a finished dry run has NOT met (none: the schedule does enough)."""
    k, m, ev = model.k, model.m, model.ev
    top = min(k, m)
    need = {f"fused_{n}": 1 for n in range(1, min(FUSED_MAX, top) + 1)}
    if top >= 4:
        need["deferred"] = 1
    if k <= m:
        need["no_data_solved"] = 1
    need.update(mixed_solve_list=1, host_after_arena=1, arena_after_host=1, reuse_other_mask=1,
                resolved_after_lost_diff=1, overlapping_both_take=1, end_reply_queued=1, end_residual_queued=1,
                full_probe=1, engine_switch_live=1, two_waves=1, residual_refused=1, solve_refused=1,
                null_arena_folded_only=1, max_keys=17)  # more than 16 keys between two resets of the table: it outgrows its first blob
    gaps = [name for name, least in need.items() if ev[name] < least]
    clean = {n for _s, _h, n, _ok in model.tie}
    gaps += [f"clean_solve_of_{n}_losses" for n in range(1, top + 1) if n not in clean]
    return gaps
