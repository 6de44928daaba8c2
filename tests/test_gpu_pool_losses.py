"""GPU: the recovery pool at every loss count, against the reference of tests/recovery_case.py.

A pool leads a request that loses n >= 2 data lids once the other n - 1 participating
parities' residuals have been given (add_residual / add_residuals / parity_staging): the
explicit solves take ceil(n / 4) launches, and a flush that makes a request ready solves it
in its own launch up to three losses, behind it past three.  RS(3,2), RS(6,4), RS(10,8) on
both engines; requests of 1 and 3 units that start neither at unit 0 nor at slot 0 (a
one-unit filler request holds slot 0) in a pool of 16 units.

Every comparison is bit-exact.  Output arenas lie in the 0xA5 sentinel and are compared
whole, so bytes outside a request's units must come back unchanged; pageable residuals
carry PAD sentinel bytes either side; the parity arena and the peers' units are checked
unwritten at the end.  Launch counts are deltas of ec.last_launch()["seq"].

Launch counts of the fused passes: a flush_solve that folds and makes ready takes 1 launch
for n <= 3 and 1 + ceil(n / 4) for n >= 4.  Where the residuals arrive alone in a later
pass there is nothing to fold, so that pass has no fold launch: 1 launch for n <= 3 (the
solve) and ceil(n / 4) for n >= 4; with the pass that folded the last reply (1 launch) that
is 1 + ceil(n / 4) for the request, as in the first order.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_matrix_case as kc  # noqa: E402
import recovery_case as rc  # noqa: E402

pytestmark = pytest.mark.gpu

SENT, U = kc.SENT, kc.TILE
PAD = 128
CAP = 16
ARENA_UNITS = 8
ARENA = ARENA_UNITS * U
FILLER = (0, 0)              # holds slot 0
RANGES = [(2, 2), (4, 6)]    # slots 1 and 2-4
CODES = [(3, 2), (6, 4), (10, 8)]
WAYS = ["pageable", "device", "in_place"]


def ceil_div(a, b):
    return -(-a // b)


@pytest.fixture(params=[pytest.param(kc.PERM, id="perm"), pytest.param(kc.LDS, id="lds")])
def engine(request, gpu):
    torch, ec = gpu
    default = ec.get_engine()
    ec.set_engine(request.param)
    yield request.param
    ec.set_engine(default)


def seq_now(ec):
    return ec.last_launch()["seq"]


def span(r):
    return slice(r[0] * U, (r[1] + 1) * U)


_CASES: dict = {}


class Case:
    """One code's matrix, seeded shards and parities over ARENA bytes, computed once and
    never written again; residuals and solved shards per (mask, range) are cached on it."""

    def __init__(self, ec, k, m):
        self.k, self.m = k, m
        self.mat = ec.coding_matrix(k, m)
        rng = np.random.default_rng(0x9001 + 100 * k + m)
        self.data = rng.integers(0, 256, (k, ARENA), dtype=np.uint8)
        self.parity = np.stack(rc.encode(self.mat, k, m, list(self.data)))
        self.data.setflags(write=False)
        self.parity.setflags(write=False)
        self._res: dict = {}

    def residuals(self, mask, r):
        """{participating parity: its full residual over range r}; solve_lost of them is
        asserted equal to the data once."""
        key = (mask, r)
        if key not in self._res:
            k, m = self.k, self.m
            peers = {j: self.data[j, span(r)] for j in rc.surviving_of(k, mask)}
            res = {p: rc.residual_of(self.mat, k, p, self.parity[p - k, span(r)], peers) for p in rc.pars_of(k, m, mask)}
            for j, v in rc.solve_lost(self.mat, k, m, mask, res).items():
                assert np.array_equal(v, self.data[j, span(r)]), (k, m, hex(mask), j)
            self._res[key] = res
        return self._res[key]


def case_of(ec, k, m) -> Case:
    if (k, m) not in _CASES:
        _CASES[(k, m)] = Case(ec, k, m)
    return _CASES[(k, m)]


class Rig:
    """A pool of `leader` over the case's parity arena with the filler request in slot 0,
    the k output arenas in the sentinel, and the bookkeeping of the guards."""

    def __init__(self, torch, ec, C: Case, leader):
        self.torch, self.ec, self.C, self.leader = torch, ec, C, leader
        self.parity_dev = torch.from_numpy(C.parity[leader - C.k].copy()).cuda()
        self.pool = ec.RecoveryPool(C.k, C.m, C.mat, leader, self.parity_dev, capacity_units=CAP)
        filler_mask = rc.mask_of(C.k, [0], [leader])
        self.filler = self.pool.begin(filler_mask, *FILLER)
        self.slab = torch.full((C.k, ARENA), SENT, dtype=torch.uint8, device="cuda")
        self.arenas = [self.slab[j] for j in range(C.k)]
        self.units = [C.data[j].copy() for j in range(C.k)]  # the peers' bytes as sent (pageable)
        self.guards = []
        self.ways = set()

    def close(self):
        C = self.C
        assert np.array_equal(self.parity_dev.cpu().numpy(), C.parity[self.leader - C.k]), "parity arena written"
        for j in range(C.k):
            assert np.array_equal(self.units[j], C.data[j]), f"units of shard {j} written"
        for buf, want in self.guards:
            whole = buf.cpu().numpy() if hasattr(buf, "cpu") else buf
            assert np.array_equal(whole, want), "a given residual's buffer was written"
        self.pool.end(self.filler)
        assert self.pool.active == 0
        self.pool.destroy()

    def begin(self, mask, ranges=RANGES):
        rids = [self.pool.begin(mask, *r) for r in ranges]
        return rids

    def replies(self, rids, lids, ranges=RANGES):
        ids, peers, bufs = [], [], []
        for rid, r in zip(rids, ranges):
            for j in lids:
                ids.append(rid)
                peers.append(j)
                bufs.append(self.units[j][span(r)])
        if ids:
            self.pool.add_peers(ids, peers, bufs)

    def give(self, rids, mask, way, ranges=RANGES, batch=True):
        """The other participating parities' residuals, `way` one of WAYS."""
        C = self.C
        self.ways.add(way)
        ids, lids, bufs = [], [], []
        for rid, r in zip(rids, ranges):
            res = C.residuals(mask, r)
            for q in rc.pars_of(C.k, C.m, mask):
                if q == self.leader:
                    continue
                n = len(res[q])
                if way == "in_place":
                    addr, view = self.pool.parity_staging(rid, q)
                    assert len(view) == n
                    view[:] = res[q]
                    buf = addr
                else:
                    host = np.full(n + 2 * PAD, SENT, np.uint8)
                    host[PAD:PAD + n] = res[q]
                    whole = self.torch.from_numpy(host.copy()).cuda() if way == "device" else host
                    self.guards.append((whole, host.copy()))
                    buf = whole[PAD:PAD + n]
                ids.append(rid)
                lids.append(q)
                bufs.append(buf)
        if batch:
            if ids:
                self.pool.add_residuals(ids, lids, bufs)
        else:
            for i, q, b in zip(ids, lids, bufs):
                self.pool.add_residual(i, q, b)

    def check_arenas(self, mask, what, ranges=RANGES, want=None):
        """The whole slab: the lost lids' units of the ranges rebuilt, every other byte the
        sentinel; then the slab is reset."""
        C = self.C
        exp = np.full((C.k, ARENA), SENT, np.uint8)
        for r in ranges:
            for j in rc.lost_of(C.k, mask):
                exp[j, span(r)] = C.data[j, span(r)] if want is None else want[r][j]
        self.torch.cuda.synchronize()
        got = self.slab.cpu().numpy()
        if not np.array_equal(got, exp):
            row, p = np.argwhere(got != exp)[0]
            raise AssertionError(f"{what}: arena {row} byte {p}: got {got[row, p]:#x} want {exp[row, p]:#x} "
                                 f"({int((got != exp).sum())} bytes wrong)")
        self.slab.fill_(SENT)

    def check_planes(self, rids, mask, what, ranges=RANGES, want=None):
        C = self.C
        lost = rc.lost_of(C.k, mask)
        for rid, r in zip(rids, ranges):
            for x, j in enumerate(lost):  # ascending lost lids
                got = self.pool.output(rid, x)
                assert got is not None and len(got) == (r[1] - r[0] + 1) * U, (what, rid, x)
                exp = C.data[j, span(r)] if want is None else want[r][j]
                assert np.array_equal(got, exp), f"{what}: plane {x} (shard {j}) of request {rid}"
            assert self.pool.output(rid, len(lost)) is None, what
            assert np.array_equal(self.pool.output(rid), self.pool.output(rid, 0))

    def end(self, rids):
        for rid in rids:
            self.pool.end(rid)


def what_of(C, mask, leader, extra=""):
    return (f"RS({C.k},{C.m}) mask {mask:#x} lost {rc.lost_of(C.k, mask)} parities {rc.pars_of(C.k, C.m, mask)} "
            f"leader {leader} {extra}")


def leaders_and_masks(k, m):
    return [(mask, leader) for mask in rc.loss_sets(k, m) for leader in rc.pars_of(k, m, mask)]


# ------------------------------------------------------------------ 1. explicit solve
@pytest.mark.parametrize("k,m", CODES)
def test_pool_explicit_solve_every_loss_count(gpu, engine, k, m):
    """Every mask of loss_sets, each participating parity leading in turn, to the arenas and
    to the host planes; residuals pageable, device and in place in turn.  A complete request
    is ready only once the residuals are in; ceil(n / 4) launches behind the flush."""
    torch, ec = gpu
    C = case_of(ec, k, m)
    rigs: dict = {}
    turn = 0
    seen_n, ways_used = set(), set()
    for mask, leader in leaders_and_masks(k, m):
        if leader not in rigs:
            rigs[leader] = Rig(torch, ec, C, leader)
        rig, pool = rigs[leader], rigs[leader].pool
        n = len(rc.lost_of(k, mask))
        seen_n.add(n)
        for to_host in (False, True):
            way = WAYS[turn % 3]
            turn += 1
            if n >= 2:
                ways_used.add(way)
            what = what_of(C, mask, leader, f"{'host' if to_host else 'arena'} {way}")
            rids = rig.begin(mask)
            rig.replies(rids, rc.surviving_of(k, mask))
            assert all(pool.complete(r) for r in rids) and all(pool.ready(r) == (n == 1) for r in rids), what
            assert pool.flush() == len(rids), what
            rig.give(rids, mask, way, batch=turn % 2 == 0)
            assert all(pool.ready(r) and not pool.solved(r) for r in rids), what
            seq0 = seq_now(ec)
            if to_host:
                pool.solve_host(rids)
            else:
                pool.solve(rids, rig.arenas)
            assert seq_now(ec) == seq0 + ceil_div(n, 4), what
            assert all(pool.solved(r) for r in rids), what
            if to_host:
                rig.check_planes(rids, mask, what)
                rig.check_arenas(mask, what, ranges=[])  # no arena byte written
            else:
                assert pool.output(rids[0]) is None, what
                rig.check_arenas(mask, what)
            rig.end(rids)
    assert seen_n == set(range(1, min(m, k - 1) + 1))
    assert ways_used == set(WAYS)
    for rig in rigs.values():
        rig.close()


# ------------------------------------------------------------------ 2. fused
@pytest.mark.parametrize("k,m", CODES)
def test_pool_flush_solves_what_it_makes_ready(gpu, engine, k, m):
    """Order A: the residuals, then the last reply, one flush_solve / flush_solve_host: 1
    launch for n <= 3, 1 + ceil(n / 4) for n >= 4.  Order B: every reply folded by a first
    pass (1 launch, which solves single losses only), the residuals alone in a later pass:
    1 launch for n <= 3, ceil(n / 4) for n >= 4 (nothing to fold: see the module docstring)."""
    torch, ec = gpu
    C = case_of(ec, k, m)
    rigs: dict = {}
    turn = 0
    for mask, leader in leaders_and_masks(k, m):
        if leader not in rigs:
            rigs[leader] = Rig(torch, ec, C, leader)
        rig, pool = rigs[leader], rigs[leader].pool
        n, surv = len(rc.lost_of(k, mask)), rc.surviving_of(k, mask)
        for order in ("A", "B"):
            to_host = turn % 2 == 1
            way = WAYS[turn % 3]
            turn += 1
            what = what_of(C, mask, leader, f"order {order} {'host' if to_host else 'arena'} {way}")
            flush_solve = (lambda: pool.flush_solve_host()) if to_host else (lambda: pool.flush_solve(rig.arenas))
            rids = rig.begin(mask)
            if order == "A":
                rig.replies(rids, surv[:-1])
                if len(surv) > 1:  # (else the first touch happens in the fused launch)
                    assert pool.flush() == len(rids), what
                rig.give(rids, mask, way)
                assert not any(pool.ready(r) for r in rids), what
                rig.replies(rids, surv[-1:])
                assert all(pool.ready(r) for r in rids), what
                seq0 = seq_now(ec)
                assert flush_solve() == len(rids), what
                assert seq_now(ec) == seq0 + (1 if n <= 3 else 1 + ceil_div(n, 4)), what
            else:
                rig.replies(rids, surv)
                seq0 = seq_now(ec)
                assert flush_solve() == (len(rids) if n == 1 else 0), what
                assert seq_now(ec) == seq0 + 1, what
                assert all(pool.solved(r) == (n == 1) for r in rids), what
                if n > 1:
                    rig.give(rids, mask, way)
                    seq0 = seq_now(ec)
                    assert flush_solve() == len(rids), what
                    assert seq_now(ec) == seq0 + (1 if n <= 3 else ceil_div(n, 4)), what
            assert all(pool.solved(r) for r in rids), what
            if to_host:
                rig.check_planes(rids, mask, what)
                rig.check_arenas(mask, what, ranges=[])
            else:
                rig.check_arenas(mask, what)
            # the residual the pass left is the full one (the fused launch wrote R' too)
            for rid, r in zip(rids, RANGES):
                res = np.zeros((r[1] - r[0] + 1) * U, np.uint8)
                pool.residual(rid, res)
                assert np.array_equal(res, C.residuals(mask, r)[leader]), what
            rig.end(rids)
    for rig in rigs.values():
        rig.close()


# ------------------------------------------------------------------ 3. a mixed pass
def test_pool_mixed_pass_solves_exactly_the_ready(gpu, engine):
    """RS(6,4), twelve one-unit requests led by P0 over all four loss counts in one pass:
    ready (R), complete but missing a residual (C), incomplete (I).  One flush_solve_host
    solves exactly the ready ones, in one launch while no ready one loses four; the four-loss
    requests, their residuals completed in a later pass, take ceil(4 / 4) = 1 more."""
    torch, ec = gpu
    k, m = 6, 4
    C = case_of(ec, k, m)
    leader = k
    rig = Rig(torch, ec, C, leader)
    pool = rig.pool
    states = {1: "RRI", 2: "RCI", 3: "RCI", 4: "CCI"}
    reqs = []  # (rid, mask, range, state)
    unit = 1
    for n, sts in states.items():
        masks = [mk for mk in rc.masks_of(k, m, n) if (mk >> leader) & 1]
        for i, st in enumerate(sts):
            mask = masks[(5 * i + n) % len(masks)]
            r = (unit % ARENA_UNITS, unit % ARENA_UNITS)
            unit += 1
            reqs.append((pool.begin(mask, *r), mask, r, st))
    assert {n: sum(1 for q in reqs if len(rc.lost_of(k, q[1])) == n) for n in states} == {1: 3, 2: 3, 3: 3, 4: 3}
    assert len(reqs) == 12 and sum(q[3] == "R" for q in reqs) == 4
    held = []  # the residual a C request still misses
    for rid, mask, r, st in reqs:
        surv = rc.surviving_of(k, mask)
        rig.replies([rid], surv if st != "I" else surv[:-1], ranges=[r])
        others = [q for q in rc.pars_of(k, m, mask) if q != leader]
        give = others if st != "C" else others[:-1]
        for q in give:
            pool.add_residual(rid, q, C.residuals(mask, r)[q].copy())
        if st == "C":
            held.append((rid, others[-1], C.residuals(mask, r)[others[-1]].copy()))
        assert pool.complete(rid) == (st != "I") and pool.ready(rid) == (st == "R"), (rid, st)
    seq0 = seq_now(ec)
    assert pool.flush_solve_host() == 4
    assert seq_now(ec) == seq0 + 1
    for rid, mask, r, st in reqs:
        assert pool.solved(rid) == (st == "R"), (rid, hex(mask), st)
        if st == "R":
            rig.check_planes([rid], mask, f"mixed pass {mask:#x}", ranges=[r])
        else:
            assert pool.output(rid) is None
    # the later pass: the missing residuals alone; two of them complete four-loss requests
    pool.add_residuals([h[0] for h in held], [h[1] for h in held], [h[2] for h in held])
    seq0 = seq_now(ec)
    assert pool.flush_solve_host() == len(held) == 4
    assert seq_now(ec) == seq0 + 1 + 1  # n <= 3 in the pass's launch, n = 4 in ceil(4 / 4) behind it
    for rid, mask, r, st in reqs:
        assert pool.solved(rid) == (st != "I")
        if st == "C":
            rig.check_planes([rid], mask, f"later pass {mask:#x}", ranges=[r])
    rig.check_arenas(0, "mixed pass", ranges=[])
    rig.end([q[0] for q in reqs])
    rig.close()


# ------------------------------------------------------------------ 4. the widest layouts
@pytest.mark.parametrize("n", [8, 3])
def test_pool_rs16_8_first_touch_in_the_flush(gpu, engine, n):
    """RS(16,8), one unit, every reply and residual queued before the one flush_solve, so the
    first touch happens in it.  8 lost: the fold (P and 8 replies) and two solve launches (R
    and 7 residuals in, 8 shards out), 3 launches, the slot layout at its widest (42 slots).
    3 lost: P, 13 replies and 2 residuals are 16 inputs, the edge of a pattern, with R' and
    the 3 shards its 4 outputs: one launch."""
    torch, ec = gpu
    k, m = 16, 8
    C = case_of(ec, k, m)
    leader = k + 2
    pars = list(range(k, k + m)) if n == 8 else [k, leader, k + m - 1]
    mask = rc.mask_of(k, list(range(1, 2 * n, 2)), pars)
    rig = Rig(torch, ec, C, leader)
    r = [(3, 3)]
    rids = rig.begin(mask, ranges=r)
    rig.replies(rids, rc.surviving_of(k, mask), ranges=r)
    rig.give(rids, mask, "in_place", ranges=r)
    assert rig.pool.ready(rids[0])
    seq0 = seq_now(ec)
    assert rig.pool.flush_solve(rig.arenas) == 1
    rec = ec.last_launch()
    assert rec["seq"] == seq0 + (3 if n == 8 else 1), rec
    if n == 3:
        assert (rec["nt"], rec["lt"]) == (16, 4), rec
    rig.check_arenas(mask, f"RS(16,8) {n} lost", ranges=r)
    # and to the host planes, by an explicit solve: ceil(n / 4) launches
    seq0 = seq_now(ec)
    rig.pool.solve_host(rids)
    assert seq_now(ec) == seq0 + ceil_div(n, 4)
    rig.check_planes(rids, mask, f"RS(16,8) {n} lost, host", ranges=r)
    rig.end(rids)
    rig.close()


# ------------------------------------------------------------------ 5. a fold after the solve
@pytest.mark.parametrize("k,m", [(3, 2), (6, 4)])
def test_pool_fold_after_solve_clears_solved(gpu, engine, k, m):
    """A lost lid's diff folded after the solve (recovery.c:116-120): solved clears, the
    request stays ready, and a second solve equals solve_lost over the moved R and the
    unchanged given residuals."""
    torch, ec = gpu
    C = case_of(ec, k, m)
    mask = rc.loss_sets(k, m)[2]  # two lost, the lowest lids and parities
    leader = rc.pars_of(k, m, mask)[1]
    lost = rc.lost_of(k, mask)
    assert len(lost) == 2
    rig = Rig(torch, ec, C, leader)
    pool = rig.pool
    rids = rig.begin(mask)
    rig.replies(rids, rc.surviving_of(k, mask))
    rig.give(rids, mask, "pageable")
    assert pool.flush_solve_host() == 2
    rig.check_planes(rids, mask, "before the fold")
    # 5000 bytes of lost lid lost[1] from the middle of unit 4: units 4 and 5 of the second request
    diff = np.random.default_rng(77).integers(0, 256, 5000, dtype=np.uint8)
    addr = 4 * U + 1000
    assert pool.fold_update(lost[1], addr, diff.copy()) == 2
    assert pool.solved(rids[0]) and not pool.solved(rids[1]) and pool.ready(rids[1])
    assert pool.output(rids[1]) is None
    moved = C.residuals(mask, RANGES[1])[leader].copy()
    o = addr - RANGES[1][0] * U
    moved[o:o + len(diff)] ^= kc.MUL[int(C.mat[leader * k + lost[1]])][diff]
    res = dict(C.residuals(mask, RANGES[1]))
    res[leader] = moved
    want = {RANGES[1]: rc.solve_lost(C.mat, k, m, mask, res)}
    seq0 = seq_now(ec)
    pool.solve_host([rids[1]])
    assert seq_now(ec) == seq0 + 1 and pool.solved(rids[1])
    rig.check_planes([rids[1]], mask, "after the fold", ranges=[RANGES[1]], want=want)
    pool.solve([rids[1]], rig.arenas)
    rig.check_arenas(mask, "after the fold, arenas", ranges=[RANGES[1]], want=want)
    rig.end(rids)
    rig.close()


# ------------------------------------------------------------------ 6. refusals
def test_pool_residual_refusals(gpu, engine):
    """Each CEC_EINVAL of add_residual(s); a refused batch queues nothing (ready stays false
    and the following flush solves nothing); solve of a complete, not-ready request is refused
    and leaves solved false; a single-loss pass beside it is unaffected."""
    torch, ec = gpu
    k, m = 6, 4
    C = case_of(ec, k, m)
    leader = k + 1
    rig = Rig(torch, ec, C, leader)
    pool = rig.pool
    mask = rc.mask_of(k, [0, 3, 4], [k, leader, k + 3])  # parities 6, 7, 9; 8 is left out
    single = rc.mask_of(k, [2], [leader])
    r3, r1 = (2, 2), (4, 6)
    rid = pool.begin(mask, *r3)
    sid = pool.begin(single, *r1)
    res = C.residuals(mask, r3)
    good = lambda q: res[q].copy()  # noqa: E731

    def refused(fn):
        with pytest.raises(ec.CecError) as ei:
            fn()
        assert ei.value.code == ec.CEC_EINVAL

    refused(lambda: pool.add_residual(99, k, good(k)))                   # not live
    refused(lambda: pool.add_residual(rid, k + 2, good(k)))              # parity 8 is not in the mask
    refused(lambda: pool.add_residual(rid, 1, good(k)))                  # a data lid
    refused(lambda: pool.add_residual(rid, leader, good(k)))             # lid_self
    refused(lambda: pool.add_residual(sid, k, np.zeros(3 * U, np.uint8)))  # a single loss takes none
    for bad_rid, bad_lid in ((rid, leader), (rid, k + 2), (rid, 1), (sid, k), (99, k)):
        with pytest.raises(ec.CecError) as ei:  # no staging where add_residual would take nothing
            pool.parity_staging(bad_rid, bad_lid)
        assert ei.value.code == ec.CEC_EINVAL, (bad_rid, bad_lid)
    pool.add_residual(rid, k, good(k))
    refused(lambda: pool.add_residual(rid, k, good(k)))                  # given twice
    # batches: a bad entry last, and a pair twice; nothing of either is queued
    refused(lambda: pool.add_residuals([rid, rid], [k + 3, k + 2], [good(k + 3), good(k + 3)]))
    refused(lambda: pool.add_residuals([rid, rid], [k + 3, k + 3], [good(k + 3), good(k + 3)]))
    rig.replies([rid], rc.surviving_of(k, mask), ranges=[r3])
    rig.replies([sid], rc.surviving_of(k, single), ranges=[r1])
    assert pool.complete(rid) and not pool.ready(rid) and pool.ready(sid)
    seq0 = seq_now(ec)
    assert pool.flush_solve(rig.arenas) == 1  # the single loss beside it, in the one launch
    assert seq_now(ec) == seq0 + 1
    assert pool.solved(sid) and not pool.solved(rid)
    rig.check_arenas(single, "single loss beside a refused batch", ranges=[r1])
    refused(lambda: pool.solve([rid], rig.arenas))                       # complete, not ready
    refused(lambda: pool.solve_host([rid]))
    assert not pool.solved(rid)
    rig.check_arenas(mask, "refused solve", ranges=[])
    pool.add_residuals([rid], [k + 3], [good(k + 3)])
    assert pool.ready(rid)
    seq0 = seq_now(ec)
    assert pool.flush_solve(rig.arenas) == 1  # the last residual alone put it into this flush
    assert seq_now(ec) == seq0 + 1 and pool.solved(rid)
    rig.check_arenas(mask, "after the last residual", ranges=[r3])
    rig.end([rid, sid])
    rig.close()


# ------------------------------------------------------------------ 7. a request ended while queued
@pytest.mark.parametrize("solve", [True, False], ids=["flush_solve", "flush"])
def test_pool_request_ended_with_only_a_residual_queued(gpu, engine, solve):
    """add_residual queues a request whose replies were folded earlier; end before the next
    flush (a cancelled recovery) must take it out of the queue.  The next begin reuses the id:
    were it still queued, its first reply would queue it a second time, and the flush would
    append its tiles twice and count it twice.  Asserted: the reused id, the flush's returned
    count, its one launch over exactly the request's 3 tiles, and the rebuilt bytes."""
    torch, ec = gpu
    k, m = 6, 4
    C = case_of(ec, k, m)
    leader = k
    rig = Rig(torch, ec, C, leader)
    pool = rig.pool
    double = rc.mask_of(k, [1, 4], [leader, k + 2])
    single = rc.mask_of(k, [3], [leader])
    r = (4, 6)
    rid = pool.begin(double, *r)
    rig.replies([rid], rc.surviving_of(k, double), ranges=[r])
    assert pool.flush() == 1
    pool.add_residual(rid, k + 2, C.residuals(double, r)[k + 2].copy())
    assert pool.ready(rid)
    pool.end(rid)  # queued by the residual alone
    again = pool.begin(single, *r)
    assert again == rid  # ids are reused last in, first out
    rig.replies([again], rc.surviving_of(k, single), ranges=[r])
    seq0 = seq_now(ec)
    if solve:
        assert pool.flush_solve(rig.arenas) == 1
    else:
        assert pool.flush() == 1
    rec = ec.last_launch()
    assert rec["seq"] == seq0 + 1 and rec["n_tiles"] == 3, rec
    if solve:
        assert pool.solved(again)
        rig.check_arenas(single, "the reused id", ranges=[r])
    else:
        assert pool.flush() == 0  # nothing left in the queue
        pool.solve([again], rig.arenas)
        assert ec.last_launch()["n_tiles"] == 3
        rig.check_arenas(single, "the reused id, explicit solve", ranges=[r])
    rig.end([again])
    rig.close()
