"""GPU: recovery when the mask names no data lid, against tests/recovery_case.py.

With k <= m a valid recovery mask can name k parities and nothing else: every data shard is
lost.  No peer replies, so nothing brings the first touch about; the residual of such a
request is R = P[range] from the start (the first-touch copy of recovery.c:79-82 with no
fold behind it), and the k parities' residuals rebuild all k shards.  The other recovery
tests stop at min(m, k - 1) losses; these run the masks they leave out.

* stateless ops (cec_residual + cec_solve, cec_decode) over plan C: every mask of RS(1,2),
  RS(2,2), RS(2,3), RS(3,4) and RS(4,8) (494 masks, 70 of them without a data lid, four
  outputs), the 56 no-data masks of RS(5,8) (five outputs: two launches) and 0xFF00 of
  RS(8,8); all 34 masks of RS(3,4) in one decode launch;
* sessions of RS(1,2), RS(2,2), RS(3,4), RS(5,8), RS(8,8): the residual after create is P,
  the solve rebuilds every shard, finish is refused, diffs fold in before and after the
  first read; the masks of RS(2,2) and RS(3,4) that do name data lids run two-step and fused;
* the pool, same codes: explicit solves, fused flushes, a pass mixed with an ordinary
  request, residual() on a parity that does not lead, updates before the first flush, after
  a flush and after a solve.

Conventions of tests/test_gpu_recovery_losses.py and tests/test_gpu_pool_losses.py, whose
helpers are used: both engines, bit-exact, 0xA5 sentinels and whole-buffer compares, the
parity arena checked unwritten where the test did not write it, launch counts as deltas of
ec.last_launch()["seq"].  Ahead of every no-data session a decoy session of the same byte
size takes a pageable peer and is destroyed; ahead of every no-data pool request decoys
take every free slot, a reply each, are flushed and ended: a residual that is merely what
the buffer's last owner left shows.

Launches: a session's first touch is one launch in create.  The pool makes it in the next
flush of any kind: a flush_solve with the residuals in is 1 launch for n <= 3 and
1 + ceil(n / 4) past that; an explicit solve that still finds the first touch queued is
1 + ceil(n / 4), after a flush ceil(n / 4).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_matrix_case as kc  # noqa: E402
import recovery_case as rc  # noqa: E402
import test_gpu_pool_losses as pl  # noqa: E402
import test_gpu_recovery_losses as rl  # noqa: E402

pytestmark = pytest.mark.gpu

SENT, U, ROW = kc.SENT, kc.TILE, kc.ROW
UB, UE, LO, HI, NB = rl.UB, rl.UE, rl.LO, rl.HI, rl.NB
RANGES, WAYS, span = pl.RANGES, pl.WAYS, pl.span
CODES = [(1, 2), (2, 2), (3, 4), (5, 8), (8, 8)]
ceil_div, seq_now, dev = rl.ceil_div, rl.seq_now, rl.dev


@pytest.fixture(params=[pytest.param(kc.PERM, id="perm"), pytest.param(kc.LDS, id="lds")])
def engine(request, gpu):
    torch, ec = gpu
    default = ec.get_engine()
    ec.set_engine(request.param)
    yield request.param
    ec.set_engine(default)


def nd_sets(k, m):
    """The no-data masks the sessions and the pool run: of the lowest and of the highest k
    parities (RS(1,2): both its masks; k == m: the one there is)."""
    sets = [s for s in rc.session_sets(k, m) if not rc.surviving_of(k, s)]
    assert sets and set(sets) <= set(rc.no_data_masks(k, m)) and len(sets) == (1 if k == m else 2)
    return sets


def refused(ec, fn):
    with pytest.raises(ec.CecError) as ei:
        fn()
    assert ei.value.code == ec.CEC_EINVAL


# ------------------------------------------------------------------ stateless ops
EVERY = {(1, 2): 2, (2, 2): 5, (2, 3): 9, (3, 4): 34, (4, 8): 494}
STATELESS = list(EVERY) + [(5, 8), (8, 8)]


def stateless_masks(k, m):
    if (k, m) in EVERY:
        masks = rc.all_masks(k, m)
        assert len(masks) == EVERY[(k, m)]
    else:
        masks = rc.no_data_masks(k, m)
        assert len(masks) == {(5, 8): 56, (8, 8): 1}[(k, m)]
        assert (k, m) != (8, 8) or masks == [0xFF00]
    no_data = [mk for mk in masks if not rc.surviving_of(k, mk)]
    assert len(no_data) == {(1, 2): 2, (2, 2): 1, (2, 3): 3, (3, 4): 4, (4, 8): 70, (5, 8): 56, (8, 8): 1}[(k, m)]
    return masks


@pytest.mark.parametrize("k,m", STATELESS)
def test_residual_solve_masks_without_data_lids(gpu, oracle, engine, k, m):
    """Each participating parity's cec_residual (n launches), then one cec_solve
    (ceil(n / 4): n = 4, 5 and 8 all-parity inputs among them), over plan C.  With no data lid
    named the residual is a copy of P.  Rows: k + m arenas, m residuals, k outputs; the rows a
    mask does not name are XORed with 0xFF first, so reading one shows."""
    torch, ec = gpu
    C = rl.code_case(ec, oracle, k, m)
    base = np.full((2 * k + 2 * m, ROW), SENT, np.uint8)
    base[:k], base[k:k + m] = C.data, C.parity
    seen = set()
    with ec.Plan(rl.EXT_C) as plan:
        for mask in stateless_masks(k, m):
            lost, pars = rc.lost_of(k, mask), rc.pars_of(k, m, mask)
            n = len(lost)
            seen.add((n, n == k))
            res, sol = C.plan_ref(mask)
            if n == k:
                for p in pars:
                    assert np.array_equal(res[p], C.parity[p - k, rl.IDX_C])
            host0 = base.copy()
            host0[np.ix_(rl.unnamed_rows(k, m, mask), rl.IDX_C)] ^= 0xFF
            exp = host0.copy()
            for p in pars:
                exp[m + p, rl.IDX_C] = res[p]
            for j in lost:
                exp[k + 2 * m + j, rl.IDX_C] = sol[j]
            slab = dev(torch, host0)
            rows = [slab[r] for r in range(len(host0))]
            seq0 = seq_now(ec)
            for p in pars:
                ec.residual(k, m, C.mat, p, mask, rows[:k + m], rows[m + p], plan)
            assert seq_now(ec) == seq0 + n, hex(mask)
            ec.solve(k, m, C.mat, mask, [rows[m + lid] if lid in pars else None for lid in range(k + m)],
                     [rows[k + 2 * m + j] if j in lost else None for j in range(k)], plan)
            assert seq_now(ec) == seq0 + n + ceil_div(n, 4), (hex(mask), n)
            torch.cuda.synchronize()
            rl.assert_slab(slab.cpu().numpy(), exp, f"RS({k},{m}) mask {mask:#x} residual + solve")
    assert (k, True) in seen


@pytest.mark.parametrize("k,m", STATELESS)
def test_decode_masks_without_data_lids(gpu, oracle, engine, k, m):
    """cec_decode of one mask per launch over plan C, ceil(n / 4) launches.  Rows: k + m
    arenas, k outputs."""
    torch, ec = gpu
    C = rl.code_case(ec, oracle, k, m)
    base = np.full((2 * k + m, ROW), SENT, np.uint8)
    base[:k], base[k:k + m] = C.data, C.parity
    with ec.Plan(rl.EXT_C) as plan:
        for mask in stateless_masks(k, m):
            lost = rc.lost_of(k, mask)
            C.plan_ref(mask)  # (solve_lost of the residuals gives these bytes back: asserted there)
            host0 = base.copy()
            host0[np.ix_(rl.unnamed_rows(k, m, mask), rl.IDX_C)] ^= 0xFF
            exp = host0.copy()
            for j in lost:
                exp[k + m + j, rl.IDX_C] = C.data[j, rl.IDX_C]
            slab = dev(torch, host0)
            rows = [slab[r] for r in range(len(host0))]
            seq0 = seq_now(ec)
            ec.decode(k, m, C.mat, [mask], rows[:k + m], rows[k + m:], plan)
            assert seq_now(ec) == seq0 + ceil_div(len(lost), 4), hex(mask)
            torch.cuda.synchronize()
            rl.assert_slab(slab.cpu().numpy(), exp, f"RS({k},{m}) mask {mask:#x} decode")


def test_decode_all_masks_of_rs34_in_one_launch(gpu, oracle, engine):
    """RS(3,4): all 34 masks, the four of three parities and no data lid among them, dealt
    over 34 extents of 48 bytes at 16-byte-aligned offsets: one launch."""
    torch, ec = gpu
    k, m = 3, 4
    mat = ec.coding_matrix(k, m)
    assert mat == oracle.big_vandermonde(k + m, k)
    masks = rc.all_masks(k, m)
    assert len(masks) == 34 and sum(not rc.surviving_of(k, mk) for mk in masks) == 4
    ext = [(16 + 64 * e, 16 + 64 * e, 48, e) for e in range(len(masks))]
    row = ext[-1][0] + 48 + 16
    row += -row % 128
    rng = np.random.default_rng(0xA34 + engine)
    data = rng.integers(0, 256, (k, row), dtype=np.uint8)
    host0 = np.full((2 * k + m, row), SENT, np.uint8)
    host0[:k] = data
    host0[k:k + m] = np.stack(rc.encode(mat, k, m, list(data)))
    for (off, _, n, e) in ext:
        host0[rl.unnamed_rows(k, m, masks[e]), off:off + n] ^= 0xFF
    exp = host0.copy()
    for (off, _, n, e) in ext:
        for j in rc.lost_of(k, masks[e]):
            exp[k + m + j, off:off + n] = data[j, off:off + n]
    slab = dev(torch, host0)
    rows = [slab[r] for r in range(len(host0))]
    seq0 = seq_now(ec)
    with ec.Plan(ext) as plan:
        ec.decode(k, m, mat, masks, rows[:k + m], rows[k + m:], plan)
        rec = ec.last_launch()
        torch.cuda.synchronize()
    assert rec["seq"] == seq0 + 1 and rec["engine"] == engine, rec
    rl.assert_slab(slab.cpu().numpy(), exp, "RS(3,4) 34 masks in one launch")


# ------------------------------------------------------------------ sessions
_JUNK: dict = {}


def decoy_session(torch, ec):
    """A session of the same byte size (RS(2,2), D0 lost, led by P0) takes its one peer from
    pageable memory and is destroyed: the residual and the staging buffer it hands back to
    the cache hold bytes that are neither any case's parity nor zero."""
    if not _JUNK:
        rng = np.random.default_rng(0xDEC0)
        _JUNK["parity"] = dev(torch, rng.integers(0, 256, rl.SESSION_ARENA, dtype=np.uint8))
        _JUNK["units"] = rng.integers(1, 256, NB, dtype=np.uint8)
        _JUNK["mat"] = ec.coding_matrix(2, 2)
    with ec.Recovery(2, 2, _JUNK["mat"], 2, 0b0110, UB, UE, _JUNK["parity"]) as d:
        assert d.nbytes == NB
        d.add_peer(1, _JUNK["units"])
        assert d.complete


def run_no_data(S, mask, leader, pageable):
    """create (the first touch: one launch), the residual read back, finish refused, solve."""
    C, ec, torch = S.C, S.ec, S.torch
    k, m = C.k, C.m
    lost, pars = rc.lost_of(k, mask), rc.pars_of(k, m, mask)
    n = len(lost)
    assert lost == list(range(k)) and n == k
    full = C.full_residuals(mask)  # (solve_lost of them is the data: asserted there)
    for p in pars:
        assert np.array_equal(full[p], C.sparity[p - k, LO:HI])
    what = rl.what_of(C, mask, leader, "no data lid, " + ("pageable" if pageable else "device"))
    decoy_session(torch, ec)
    seq0 = seq_now(ec)
    with ec.Recovery(k, m, C.mat, leader, mask, UB, UE, S.pdev[leader - k]) as rec:
        created = seq_now(ec) - seq0
        assert rec.nbytes == NB and rec.complete, what
        assert np.array_equal(S.residual(rec), full[leader]), f"{what}: the residual after create is not P"
        peers = {q: rl.Guarded(torch, NB, full[q], device=not pageable) for q in pars if q != leader}
        pr = {q: g.view for q, g in peers.items()}
        outs = S.outputs(lost, device=not pageable)
        ov = {j: g.view for j, g in outs.items()}
        # finish takes a data peer of the mask: there is none
        seq1 = seq_now(ec)
        for peer in range(k):
            refused(ec, lambda: rec.finish(peer, S.units[peer].view, pr, ov))
        assert seq_now(ec) == seq1, what
        for j, g in outs.items():
            assert (g.bytes(what) == SENT).all(), f"{what}: a refused finish wrote shard {j}"
        rec.solve(pr, ov)
        took = seq_now(ec) - seq1
        torch.cuda.synchronize()
        S.check_outputs(outs, what)
        for q, g in peers.items():
            assert np.array_equal(g.bytes(what), full[q]), f"{what}: residual of {q} written"
        assert np.array_equal(S.residual(rec), full[leader]), f"{what}: solve changed the residual"
        assert created == 1, what
        if not pageable:
            assert took == ceil_div(n, 4), what


@pytest.mark.parametrize("k,m", CODES)
def test_sessions_without_data_lids(gpu, oracle, engine, k, m):
    """Every participating parity leads in turn, device and pageable buffers: the residual
    after create equals P[range], cec_recovery_solve rebuilds all k shards in ceil(k / 4)
    launches, cec_recovery_finish is refused (CEC_EINVAL, no launch, outputs untouched)."""
    torch, ec = gpu
    S = rl.Sessions(torch, ec, rl.code_case(ec, oracle, k, m))
    for mask in nd_sets(k, m):
        for leader in rc.pars_of(k, m, mask):
            run_no_data(S, mask, leader, pageable=False)
            run_no_data(S, mask, leader, pageable=True)
    S.check_inputs()


def run_no_data_updates(S, mask, leader, pageable):
    """Two writes to lost shards reach the parity while the session is open: one before the
    residual is first read, one after.  Each is applied to the parity arena (a copy of this
    test's own) and folded; the residual stays the live parity bytes and the solve returns
    the new data."""
    C, ec, torch = S.C, S.ec, S.torch
    k, m = C.k, C.m
    lost, pars = rc.lost_of(k, mask), rc.pars_of(k, m, mask)
    what = rl.what_of(C, mask, leader, "no data lid, updates")
    arena = dev(torch, C.sparity[leader - k])
    live = C.sparity[leader - k].copy()
    data = C.sdata.copy()
    second = np.ascontiguousarray(C.diff[::-1][:3000])
    updates = [(0, rl.DIFF_ADDR, C.diff, 2), (k - 1, LO + 8, second, 1)]  # units 3 and 4; unit 2

    def write(lid, addr, diff):
        data[lid, addr:addr + len(diff)] ^= diff
        live[addr:addr + len(diff)] ^= kc.MUL[C.coef(leader, lid)][diff]
        arena[addr:addr + len(diff)] = torch.from_numpy(live[addr:addr + len(diff)].copy()).cuda()

    decoy_session(torch, ec)
    with ec.Recovery(k, m, C.mat, leader, mask, UB, UE, arena) as rec:
        for i, (lid, addr, diff, units) in enumerate(updates):
            write(lid, addr, diff)
            assert rec.fold_update(lid, addr, diff.copy() if pageable else dev(torch, diff)) == units, (what, i)
            assert rec.complete
            got = S.residual(rec)  # (the first read comes after the first update)
            assert np.array_equal(got, live[LO:HI]), f"{what}: the residual after update {i} is not the live parity"
        new_parity = rc.encode(C.mat, k, m, list(data))
        assert np.array_equal(new_parity[leader - k], live) and np.array_equal(arena.cpu().numpy(), live)
        peers = {q: rl.Guarded(torch, NB, new_parity[q - k][LO:HI], device=not pageable) for q in pars if q != leader}
        outs = S.outputs(lost, device=not pageable)
        rec.solve({q: g.view for q, g in peers.items()}, {j: g.view for j, g in outs.items()})
        torch.cuda.synchronize()
        S.check_outputs(outs, what, data=data)
    assert np.array_equal(arena.cpu().numpy(), live), f"{what}: parity arena written"


@pytest.mark.parametrize("k,m", CODES)
def test_sessions_without_data_lids_fold_updates(gpu, oracle, engine, k, m):
    """A diff of a lost lid applied to the parity arena and folded, before the first read of
    the residual and after it; device and pageable diffs."""
    torch, ec = gpu
    S = rl.Sessions(torch, ec, rl.code_case(ec, oracle, k, m))
    for mask in nd_sets(k, m):
        for i, leader in enumerate(rc.pars_of(k, m, mask)):
            run_no_data_updates(S, mask, leader, pageable=i % 2 == 1)
    S.check_inputs()


@pytest.mark.parametrize("k,m", [(2, 2), (3, 4)])
def test_sessions_k_le_m_masks_that_name_data_lids(gpu, oracle, engine, k, m):
    """The other masks of codes with k <= m, as the k > m codes run them: two-step (ascending
    on device buffers, descending on pageable ones) and cec_recovery_finish, every
    participating parity leading.  RS(2,2): its four single losses; RS(3,4): one and two lost."""
    torch, ec = gpu
    S = rl.Sessions(torch, ec, rl.code_case(ec, oracle, k, m))
    masks = rc.masks_of(2, 2, 1) if (k, m) == (2, 2) else rc.loss_sets(k, m)
    assert len(masks) == 4 and all(rc.surviving_of(k, mk) for mk in masks)
    for mask in masks:
        rl.run_two_step(S, mask, descending=False, pageable=False)
        rl.run_two_step(S, mask, descending=True, pageable=True)
        for leader in rc.pars_of(k, m, mask):
            rl.run_finish(S, mask, leader, engine)
    S.check_inputs()


# ------------------------------------------------------------------ the pool
DECOY_UNITS = (0, 1, 3, 7)  # no unit of RANGES: a slot left with another unit's parity shows too


class Rig(pl.Rig):
    """pl.Rig, and the decoys.  With k = 1 the filler's own mask names no data lid: its first
    touch is flushed here, so that no later pass finds it queued and solves it."""

    def __init__(self, torch, ec, C, leader):
        super().__init__(torch, ec, C, leader)
        assert not set(DECOY_UNITS) & {u for r in RANGES for u in range(r[0], r[1] + 1)}
        if C.k == 1:
            assert self.pool.flush() == 0

    def dirty(self):
        """Fifteen one-unit decoys take every slot but the filler's.  Each loses D0, takes D1's
        reply (R = P ^ c * D1 after the flush) and is ended.  k = 1 has no such mask: its
        decoys hold the parity of other units."""
        C, pool = self.C, self.pool
        mask = rc.mask_of(C.k, [0], [self.leader])
        ranges = [(DECOY_UNITS[i % 4],) * 2 for i in range(pl.CAP - 1)]
        rids = self.begin(mask, ranges=ranges)
        if C.k >= 2:
            self.replies(rids, [1], ranges=ranges)
            assert pool.flush() == len(rids)
        else:
            assert pool.flush() == 0
        self.end(rids)
        assert pool.active == 1

    def begin_no_data(self, mask, what):
        n = len(rc.lost_of(self.C.k, mask))
        self.dirty()
        rids = self.begin(mask)
        self.states(rids, n == 1, False, what + ": after begin")
        return rids

    def states(self, rids, ready, solved, what):
        """complete from the start, whatever else."""
        pool = self.pool
        for r in rids:
            assert (pool.complete(r), pool.ready(r), pool.solved(r)) == (True, ready, solved), (what, r)

    def check_residuals(self, rids, what, parity=None):
        """pool.residual of each request: the parity's bytes over its range."""
        parity = self.C.parity[self.leader - self.C.k] if parity is None else parity
        for rid, r in zip(rids, RANGES):
            got = np.full((r[1] - r[0] + 1) * U, SENT, np.uint8)
            self.pool.residual(rid, got)
            assert np.array_equal(got, parity[span(r)]), f"{what}: the residual of request {rid} is not P"

    def check_rebuilt(self, rids, mask, to_host, what, **kw):
        if to_host:
            self.check_planes(rids, mask, what, **kw)
            self.check_arenas(mask, what, ranges=[])  # no arena byte written
        else:
            assert self.pool.output(rids[0]) is None, what
            self.check_arenas(mask, what, **kw)


def pool_cases(k, m):
    return [(mask, leader) for mask in nd_sets(k, m) for leader in rc.pars_of(k, m, mask)]


@pytest.mark.parametrize("k,m", CODES)
def test_pool_explicit_solve_without_data_lids(gpu, engine, k, m):
    """solve into the arenas and solve_host into the planes, each participating parity
    leading in turn, the residuals given in the three ways.  With the first touch still
    queued the solve is the flush's launch and ceil(n / 4); after a flush (which folds no
    reply: it returns 0) ceil(n / 4) alone."""
    torch, ec = gpu
    C = pl.case_of(ec, k, m)
    n = k
    rigs: dict = {}
    turn = 0
    for mask, leader in pool_cases(k, m):
        if leader not in rigs:
            rigs[leader] = Rig(torch, ec, C, leader)
        rig, pool = rigs[leader], rigs[leader].pool
        for to_host in (False, True):
            way, flush_first = WAYS[turn % 3], turn // 2 % 2 == 1
            turn += 1
            what = pl.what_of(C, mask, leader, f"{'host' if to_host else 'arena'} {way} flush_first={flush_first}")
            rids = rig.begin_no_data(mask, what)
            rig.give(rids, mask, way, batch=turn % 2 == 0)
            rig.states(rids, True, False, what + ": residuals given")
            if flush_first:
                seq0 = seq_now(ec)
                assert pool.flush() == 0, what
                assert seq_now(ec) == seq0 + 1, what
                rig.states(rids, True, False, what + ": flushed")
            seq0 = seq_now(ec)
            if to_host:
                pool.solve_host(rids)
            else:
                pool.solve(rids, rig.arenas)
            took = seq_now(ec) - seq0
            rig.states(rids, True, True, what + ": solved")
            rig.check_rebuilt(rids, mask, to_host, what)
            rig.check_residuals(rids, what)
            assert took == (0 if flush_first else 1) + ceil_div(n, 4), what
            rig.end(rids)
    assert n == 1 or set().union(*(rig.ways for rig in rigs.values())) == set(WAYS)
    for rig in rigs.values():
        rig.close()


@pytest.mark.parametrize("k,m", CODES)
def test_pool_flush_solves_without_data_lids(gpu, engine, k, m):
    """Order A: the residuals arrive in the pass that makes the first touch: one flush_solve /
    flush_solve_host, 1 launch for n <= 3 (RS(1,2): the first pass after begin), the fold's
    and ceil(n / 4) behind it for RS(5,8) and RS(8,8).  Order B (n >= 2): a plain flush makes
    the first touch, the residuals come alone in a later pass: 1 launch for n <= 3,
    ceil(n / 4) past that."""
    torch, ec = gpu
    C = pl.case_of(ec, k, m)
    n = k
    rigs: dict = {}
    turn = 0
    for mask, leader in pool_cases(k, m):
        if leader not in rigs:
            rigs[leader] = Rig(torch, ec, C, leader)
        rig, pool = rigs[leader], rigs[leader].pool
        for order in ("A", "B") if n >= 2 else ("A", "A"):
            to_host, way = turn % 2 == 1, WAYS[turn % 3]
            turn += 1
            what = pl.what_of(C, mask, leader, f"order {order} {'host' if to_host else 'arena'} {way}")
            flush_solve = (lambda: pool.flush_solve_host()) if to_host else (lambda: pool.flush_solve(rig.arenas))
            rids = rig.begin_no_data(mask, what)
            if order == "B":
                seq0 = seq_now(ec)
                assert pool.flush() == 0 and seq_now(ec) == seq0 + 1, what
                rig.states(rids, False, False, what + ": flushed")
            rig.give(rids, mask, way)
            rig.states(rids, True, False, what + ": residuals given")
            seq0 = seq_now(ec)
            solved = flush_solve()
            took = seq_now(ec) - seq0
            rig.states(rids, True, True, what + ": after the pass")
            rig.check_rebuilt(rids, mask, to_host, what)
            rig.check_residuals(rids, what)
            assert solved == len(rids), what
            assert took == (1 if n <= 3 else ceil_div(n, 4) + (order == "A")), what
            rig.end(rids)
    for rig in rigs.values():
        rig.close()


@pytest.mark.parametrize("k,m", [c for c in CODES if c[0] >= 2])
def test_pool_pass_mixes_no_data_and_ordinary_request(gpu, engine, k, m):
    """One flush_solve over a no-data request (units 4-6, its residuals just given) and a
    single-loss request completed by its replies in the same pass (unit 2): two pattern keys
    in one launch, both rebuilt; past three losses the no-data request is solved behind it."""
    torch, ec = gpu
    C = pl.case_of(ec, k, m)
    n = k
    mask = nd_sets(k, m)[-1]
    leader = rc.pars_of(k, m, mask)[-1]
    ordinary = rc.mask_of(k, [0], [leader])
    rig = Rig(torch, ec, C, leader)
    pool = rig.pool
    for to_host in (False, True):
        what = pl.what_of(C, mask, leader, f"mixed with {ordinary:#x}, {'host' if to_host else 'arena'}")
        rig.dirty()
        nd, od = pool.begin(mask, *RANGES[1]), pool.begin(ordinary, *RANGES[0])
        rig.replies([od], rc.surviving_of(k, ordinary), ranges=RANGES[:1])
        rig.give([nd], mask, "device" if to_host else "in_place", ranges=RANGES[1:])
        assert pool.ready(nd) and pool.ready(od) and not pool.solved(nd) and not pool.solved(od), what
        seq0 = seq_now(ec)
        solved = pool.flush_solve_host() if to_host else pool.flush_solve(rig.arenas)
        took = seq_now(ec) - seq0
        assert pool.solved(nd) and pool.solved(od), what
        if to_host:
            rig.check_planes([nd], mask, what, ranges=RANGES[1:])
            rig.check_planes([od], ordinary, what, ranges=RANGES[:1])
            rig.check_arenas(mask, what, ranges=[])
        else:
            exp = np.full((k, pl.ARENA), SENT, np.uint8)
            exp[:, span(RANGES[1])] = C.data[:, span(RANGES[1])]
            exp[0, span(RANGES[0])] = C.data[0, span(RANGES[0])]
            torch.cuda.synchronize()
            rl.assert_slab(rig.slab.cpu().numpy(), exp, what)
            rig.slab.fill_(SENT)
        assert solved == 2, what
        assert took == (1 if n <= 3 else 1 + ceil_div(n, 4)), what
        rig.end([nd, od])
    rig.close()


@pytest.mark.parametrize("k,m", CODES)
def test_pool_residual_of_a_parity_that_does_not_lead(gpu, engine, k, m):
    """A participating parity that only ships its residual: begin, then pool.residual.  The
    bytes are P's over the range; one launch (the flush that makes the first touch) for the
    two requests, none for the second read."""
    torch, ec = gpu
    C = pl.case_of(ec, k, m)
    rigs: dict = {}
    for mask, parity in pool_cases(k, m):
        if parity not in rigs:
            rigs[parity] = Rig(torch, ec, C, parity)
        rig = rigs[parity]
        what = pl.what_of(C, mask, parity, "residual alone")
        rids = rig.begin_no_data(mask, what)
        seq0 = seq_now(ec)
        rig.check_residuals(rids, what)
        assert seq_now(ec) == seq0 + 1, what
        rig.states(rids, k == 1, False, what + ": after residual")
        rig.end(rids)
    for rig in rigs.values():
        rig.close()


@pytest.mark.parametrize("k,m", CODES)
def test_pool_updates_without_data_lids(gpu, engine, k, m):
    """Writes to lost shards while the requests are open, each folded (fold_update /
    fold_updates) and then applied to the parity arena by the test, as the pool's caller
    does: before the first flush, after a flush and after a solve.  The residual stays the
    live parity bytes; a solve with the other parities' live residuals returns the new data;
    a fold after the solve clears solved, and the second solve is solve_lost over the moved
    residual and the given ones, which stay as given (for k = 1: the new data)."""
    torch, ec = gpu
    C = pl.case_of(ec, k, m)
    n = k
    mask = nd_sets(k, m)[0]
    pars = rc.pars_of(k, m, mask)
    leader = pars[len(pars) // 2]
    rig = Rig(torch, ec, C, leader)
    pool = rig.pool
    what = pl.what_of(C, mask, leader, "updates")
    coef = lambda lid: int(C.mat[leader * k + lid])  # noqa: E731
    rng = np.random.default_rng(0x0DD + 10 * k + m)
    live = C.parity[leader - k].copy()
    data = C.data.copy()

    def write(lid, addr, diff):
        """(after the fold: the pool's first touch reads the arena at the flush ahead of it)"""
        data[lid, addr:addr + len(diff)] ^= diff
        live[addr:addr + len(diff)] ^= kc.MUL[coef(lid)][diff]
        rig.parity_dev[addr:addr + len(diff)] = torch.from_numpy(live[addr:addr + len(diff)].copy()).cuda()

    rids = rig.begin_no_data(mask, what)
    # before the first flush: 5000 bytes of D0 from the middle of unit 4 (units 4 and 5)
    d1, a1 = rng.integers(0, 256, 5000, dtype=np.uint8), 4 * U + 1000
    seq0 = seq_now(ec)
    assert pool.fold_update(0, a1, d1.copy()) == 2, what
    assert seq_now(ec) == seq0 + 2, what  # the flush that makes the first touch, and the fold
    write(0, a1, d1)
    rig.states(rids, n == 1, False, what + ": first update")
    rig.check_residuals(rids, what + ": first update", parity=live)
    # after a flush: the last shard, the whole of unit 2 and the head of unit 4, one window
    d2, a2 = rng.integers(0, 256, U, dtype=np.uint8), 2 * U
    d3, a3 = rng.integers(0, 256, 100, dtype=np.uint8), 4 * U
    assert pool.fold_updates([(d2.copy(), a2, k - 1), (d3.copy(), a3, k - 1)]) == [1, 1], what
    write(k - 1, a2, d2)
    write(k - 1, a3, d3)
    rig.check_residuals(rids, what + ": second update", parity=live)
    # the other parities' residuals as they are now, and the solve
    new_parity = rc.encode(C.mat, k, m, list(data))
    assert np.array_equal(new_parity[leader - k], live)
    others = [q for q in pars if q != leader]
    given = {r: {q: new_parity[q - k][span(r)].copy() for q in others} for r in RANGES}
    if others:
        pool.add_residuals([rid for rid in rids for _ in others], others * len(rids),
                           [given[r][q] for r in RANGES for q in others])
    rig.states(rids, True, False, what + ": residuals given")
    seq0 = seq_now(ec)
    pool.solve_host(rids)
    assert seq_now(ec) == seq0 + ceil_div(n, 4), what
    rig.states(rids, True, True, what + ": solved")
    rig.check_planes(rids, mask, what, want={r: {j: data[j, span(r)] for j in range(k)} for r in RANGES})
    # after the solve: D0 again, inside unit 5 (the second request)
    d4, a4 = rng.integers(0, 256, 2000, dtype=np.uint8), 5 * U + 100
    assert pool.fold_update(0, a4, d4.copy()) == 1, what
    write(0, a4, d4)
    rig.states(rids[:1], True, True, what + ": third update, the request it misses")
    rig.states(rids[1:], True, False, what + ": third update")
    assert pool.output(rids[1]) is None, what
    rig.check_residuals(rids, what + ": third update", parity=live)
    res = dict(given[RANGES[1]])
    res[leader] = live[span(RANGES[1])]
    want = {RANGES[1]: rc.solve_lost(C.mat, k, m, mask, res)}
    if n == 1:
        assert np.array_equal(want[RANGES[1]][0], data[0, span(RANGES[1])])
    seq0 = seq_now(ec)
    pool.solve_host(rids[1:])
    assert seq_now(ec) == seq0 + ceil_div(n, 4), what
    rig.states(rids, True, True, what + ": solved again")
    rig.check_planes(rids[1:], mask, what + ": second solve", ranges=RANGES[1:], want=want)
    pool.solve(rids[1:], rig.arenas)
    rig.check_arenas(mask, what + ": second solve, arenas", ranges=RANGES[1:], want=want)
    rig.end(rids)
    rig.parity_dev.copy_(torch.from_numpy(C.parity[leader - k].copy()).cuda())  # as close() expects it
    for j in range(k):  # (the rig's copies of the peers' bytes: none was sent)
        assert np.array_equal(rig.units[j], C.data[j])
    rig.close()
