"""GPU: the launch record of every op that launches over a window of its own tile buffer.

A plan launch walks the plan's tiles and a region launch an implicit range; the drainer, the
recovery pool and the host batch instead build a tile list per call in a buffer of their
own and launch over a window of it.  The parity tests compare the bytes of those ops; these
also read cec_last_launch after each, so that a window which loses its tile count, its
full-line-tile count (the input of the workgroup split) or its kernel choice fails here.

Each op runs RS(3,2) over two tiny inputs in a 32 KiB arena:

* ALIGNED: three whole 4 KiB units at 4 KiB offsets (every base on a 128-B line);
* RAGGED: pieces of 100, 4095 and 4097 bytes at 16-B aligned offsets off the 128-B lines.

The pool's flush and solve work on whole units only, so their second case keeps the units
and moves the rebuilt shard's arena 16 bytes off the line instead.

The expected record is worked out here, not read from a run: tiles are cut at the 4 KiB
boundaries of the offset the kernel addresses the written stream with (tiles_of /
append_tiles), a launch splits each tile over four workgroups when at least three quarters
of its tiles are full tiles on a line and every base is line-aligned (split_shift_for), the
grid is one workgroup per tile part, and under the automatic store policy a launch this
small stores write-through.  Bytes are compared with the oracle as in test_gpu_parity.py.

Not reached: cec_drainer_apply's staged path (pack threads, two uploads per round) takes
over above 1 MiB of packed diffs or 8192 tiles, which no input of this size comes near.
tests/test_gpu_drainer_paths.py runs it on both sides of each of those two limits, with the
round cutting of the pack and in-place paths, batches that mix staged and pageable diffs,
and arena offsets around 2^32; test_drainer_matches_sequential_loop covers its bytes on
random batches.
"""
from __future__ import annotations

import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, M, U, LINE = 3, 2, 4096, 128
ARENA = 8 * U
ALIGNED = [(1 * U, U), (2 * U, U), (4 * U, U)]
RAGGED = [(16, 100), (U + 48, 4095), (3 * U + 16, 4097)]
INPUTS = [pytest.param(ALIGNED, id="aligned"), pytest.param(RAGGED, id="ragged")]
LEADER = K  # P0: the parity that drains, leads the recoveries and owns the pools


def cut(off: int, n: int) -> list[tuple[int, int]]:
    """The tiles of one extent: pieces that end on the 4 KiB boundaries of `off`."""
    out = []
    while n:
        step = min(U - off % U, n)
        out.append((off, step))
        off, n = off + step, n - step
    return out


def check_record(ec, extents, bases, kind, nt, lt, acc):
    """The thread's last launch against the record its tile window must produce.
    extents: (offset of the written stream, length) of each piece; bases: every stream
    base of the launch the test chose (the ops' own staging is allocated page-aligned)."""
    tiles = [t for off, n in extents for t in cut(off, n)]
    full = sum(1 for off, n in tiles if n == U and off % LINE == 0)
    forced = os.environ.get("CEC_SPLIT_SHIFT")
    if forced:
        split = min(2, max(0, int(forced)))
    else:
        split = 2 if full * 4 >= len(tiles) * 3 and all(b % LINE == 0 for b in bases) else 0
    policy, wt_max = ec.store_policy()
    wt = policy == "wt" or (policy == "auto" and len(tiles) * U * (nt + lt) <= wt_max)
    rec = ec.last_launch()
    got = {f: rec[f] for f in ("kind", "nt", "lt", "acc", "split_shift", "n_tiles", "grid")}
    got["wt"] = bool(rec["flags"] & ec.CEC_LAUNCH_WRITE_THROUGH)
    assert got == dict(kind=kind, nt=nt, lt=lt, acc=acc, split_shift=split, n_tiles=len(tiles),
                       grid=len(tiles) << split, wt=wt)


@pytest.fixture(scope="module")
def code(gpu, oracle):
    """RS(3,2), three data shards of one arena each and their parities (host, read only)."""
    torch, ec = gpu
    mat = ec.coding_matrix(K, M)
    data = [oracle.splitmix_bytes(0x1A0C4000 + j, ARENA) for j in range(K)]
    parity = oracle.encode(mat, K, M, data)
    for a in data + parity:
        a.setflags(write=False)
    return mat, data, parity


def coef(mat, lid):
    return mat[LEADER * K + lid]


def dev_arena(torch, init: np.ndarray | None, shift: int = 0):
    """A device arena whose base sits `shift` bytes past a 128-B line."""
    t = torch.zeros(ARENA + LINE, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % LINE == 0
    t = t[shift:shift + ARENA]
    if init is not None:
        t.copy_(torch.from_numpy(init.copy()))
    return t


def diffs_for(oracle, extents, seed):
    return [oracle.splitmix_bytes(seed + i, n) for i, (_, n) in enumerate(extents)]


# ------------------------------------------------------------------ cec_drainer_apply
@pytest.mark.parametrize("path", ["in_place", "small"])
@pytest.mark.parametrize("extents", INPUTS)
def test_drainer_apply(gpu, oracle, code, extents, path):
    """One overlap-free window: one launch of the narrow 1 x 1 XOR kernel over its tiles,
    from diffs received in the drainer's staging (in place) and from pageable buffers (the
    small mapped path, which ends with the signal-kernel wait: cec_last_sync moves)."""
    torch, ec = gpu
    mat, _, parity = code
    diffs = diffs_for(oracle, extents, 0xD1F0)
    want = parity[0].copy()
    for i, ((addr, n), diff) in enumerate(zip(extents, diffs)):
        v = want[addr:addr + n].copy()
        oracle.parity_apply(mat, K, LEADER, i % K, diff, v)
        want[addr:addr + n] = v
    arena = dev_arena(torch, parity[0])
    with ec.Drainer(K, M, mat, LEADER, staging_bytes=1 << 20) as d:
        if path == "in_place":
            base, view = d.staging()
            ups, so = [], 0
            for i, ((addr, n), diff) in enumerate(zip(extents, diffs)):
                view[so:so + n] = diff
                ups.append((base + so, addr, i % K, n))
                so = (so + n + 15) & ~15
        else:
            ups = [(diff, addr, i % K) for i, ((addr, _), diff) in enumerate(zip(extents, diffs))]
        syncs = ec.last_sync()["seq"]
        assert d.apply(ups, arena) == 1
        assert ec.last_sync()["seq"] - syncs == (1 if path == "small" else 0)
    check_record(ec, extents, [arena.data_ptr()], ec.CEC_KERNEL_NARROW, 1, 1, ec.CEC_ACC_ALL)
    assert np.array_equal(arena.cpu().numpy(), want)


# ------------------------------------------------------------------ recovery pool
def lost_d0_mask(ec):
    return ec.recovery_mask(K, M, LEADER, [0, 1, 1, 1, 1])


UNIT_RANGES = [(1, 2), (4, 4)]  # ALIGNED as requests: slots 0-1 and 2 of the pool


@pytest.mark.parametrize("op", ["flush_solve", "solve"])
@pytest.mark.parametrize("shift", [pytest.param(0, id="aligned"), pytest.param(16, id="base_off_line")])
def test_pool_flush_solve_and_solve(gpu, oracle, code, op, shift):
    """D0 rebuilt from P0, D1 and D2 over ALIGNED's units.  flush_solve: one launch of the
    exact 3 x 2 kernel (R = P ^ c1 D1 ^ c2 D2 and out = inv R in one pass); solve after a
    plain flush: the narrow 1 x 1 write kernel (only D0's pattern of the k is used)."""
    torch, ec = gpu
    mat, data, parity = code
    p0 = dev_arena(torch, parity[0])
    out0 = dev_arena(torch, None, shift)
    with ec.RecoveryPool(K, M, mat, LEADER, p0, capacity_units=8) as pool:
        rids = [pool.begin(lost_d0_mask(ec), ub, ue) for ub, ue in UNIT_RANGES]
        for rid, (ub, ue) in zip(rids, UNIT_RANGES):
            for peer in (1, 2):
                pool.add_peer(rid, peer, data[peer][ub * U:(ue + 1) * U].copy())
        if op == "flush_solve":
            assert pool.flush_solve([out0, None, None]) == len(rids)
            bases, shape = [p0.data_ptr(), out0.data_ptr()], (ec.CEC_KERNEL_EXACT, 3, 2, ec.CEC_ACC_NONE)
        else:
            assert pool.flush() == len(rids)
            pool.solve(rids, [out0, None, None])
            bases, shape = [out0.data_ptr()], (ec.CEC_KERNEL_NARROW, 1, 1, ec.CEC_ACC_NONE)
        check_record(ec, ALIGNED, bases, *shape)
        assert all(pool.solved(rid) for rid in rids)
    want = np.zeros(ARENA, np.uint8)
    for off, n in ALIGNED:
        want[off:off + n] = data[0][off:off + n]
    assert np.array_equal(out0.cpu().numpy(), want)


def touched_pool(ec, pool, data, ranges):
    """Requests over `ranges` with D1's reply queued: touched, D2 and D0 not yet fed."""
    rids = [pool.begin(lost_d0_mask(ec), ub, ue) for ub, ue in ranges]
    for rid, (ub, ue) in zip(rids, ranges):
        pool.add_peer(rid, 1, data[1][ub * U:(ue + 1) * U].copy())
    return rids


def residual_after(oracle, mat, data, parity, ranges, folds):
    """R of each request: P ^ c1 D1 (first touch and D1's reply), then each fold
    (lid, addr, diff) as R ^= c_lid * diff, in arena coordinates."""
    r = parity[0].copy()
    oracle.region_multiply(data[1].copy(), coef(mat, 1), r, 1)
    for lid, addr, diff in folds:
        oracle.region_multiply(diff.copy(), coef(mat, lid), r[addr:addr + diff.size], 1)
    return [r[ub * U:(ue + 1) * U] for ub, ue in ranges]


def pool_residuals(pool, rids, ranges):
    out = []
    for rid, (ub, ue) in zip(rids, ranges):
        out.append(np.zeros((ue - ub + 1) * U, np.uint8))
        pool.residual(rid, out[-1])
    return out


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


def r_offset(ranges, addr):
    """Where the pool's residual buffer holds arena byte `addr`: requests take their slots
    in begin order from slot 0."""
    slot = 0
    for ub, ue in ranges:
        if ub * U <= addr < (ue + 1) * U:
            return slot * U + addr - ub * U
        slot += ue - ub + 1
    raise AssertionError(addr)


@pytest.mark.parametrize("case", ["aligned", "ragged"])
def test_pool_fold_update(gpu, oracle, code, case):
    """One SET diff per call (a pageable diff, through the pool's mapped staging): the
    queued reply is flushed first, then one launch of the narrow 1 x 1 XOR kernel over the
    diff's tiles in R.  ALIGNED: one diff over its two adjacent units; RAGGED: one call
    per piece."""
    torch, ec = gpu
    mat, data, parity = code
    ranges, pieces = (UNIT_RANGES, [(U, 2 * U)]) if case == "aligned" else ([(0, 4)], RAGGED)
    diffs = diffs_for(oracle, pieces, 0xF01D)
    p0 = dev_arena(torch, parity[0])
    with ec.RecoveryPool(K, M, mat, LEADER, p0, capacity_units=8) as pool:
        rids = touched_pool(ec, pool, data, ranges)
        for (addr, n), diff in zip(pieces, diffs):
            assert pool.fold_update(2, addr, diff) == (addr + n - 1) // U - addr // U + 1
            check_record(ec, [(r_offset(ranges, addr), n)], [], ec.CEC_KERNEL_NARROW, 1, 1, ec.CEC_ACC_ALL)
        got = pool_residuals(pool, rids, ranges)
    folds = [(2, addr, diff) for (addr, _), diff in zip(pieces, diffs)]
    assert same(got, residual_after(oracle, mat, data, parity, ranges, folds))


@pytest.mark.parametrize("case", ["aligned", "ragged"])
def test_pool_fold_updates(gpu, oracle, code, case):
    """A drain window in one call: its pieces do not meet in R, so one wave -- one launch of
    the narrow 1 x 1 XOR kernel over all their tiles (lids 2 and lost 0: two of the k
    patterns used, one shape)."""
    torch, ec = gpu
    mat, data, parity = code
    ranges, pieces = (UNIT_RANGES, ALIGNED) if case == "aligned" else ([(0, 4)], RAGGED)
    diffs = diffs_for(oracle, pieces, 0xF02D)
    lids = [2, 0, 2]
    p0 = dev_arena(torch, parity[0])
    with ec.RecoveryPool(K, M, mat, LEADER, p0, capacity_units=8) as pool:
        rids = touched_pool(ec, pool, data, ranges)
        seq = ec.last_launch()["seq"]
        units = pool.fold_updates([(diff, addr, lid) for (addr, _), diff, lid in zip(pieces, diffs, lids)])
        assert units == [(addr + n - 1) // U - addr // U + 1 for addr, n in pieces]
        assert ec.last_launch()["seq"] - seq == 2  # the flush of D1's replies, then one wave
        check_record(ec, [(r_offset(ranges, addr), n) for addr, n in pieces], [], ec.CEC_KERNEL_NARROW, 1, 1,
                     ec.CEC_ACC_ALL)
        got = pool_residuals(pool, rids, ranges)
    folds = [(lid, addr, diff) for (addr, _), diff, lid in zip(pieces, diffs, lids)]
    assert same(got, residual_after(oracle, mat, data, parity, ranges, folds))


# ------------------------------------------------------------------ cec_region_multiply_batch
@pytest.mark.parametrize("extents", INPUTS)
def test_region_multiply_batch(gpu, oracle, extents):
    """dst ^= c * src over a page-aligned host heap, three coefficients (three patterns, one
    shape): one round, one wave, one launch of the narrow 1 x 1 XOR kernel.  The kernel
    addresses the staged destinations: disjoint pieces are packed in address order, each
    at the next staging offset with its address's phase within 16 bytes."""
    torch, ec = gpu
    raw = np.zeros(2 * ARENA + U, np.uint8)
    skip = -raw.ctypes.data % U
    heap = raw[skip:skip + 2 * ARENA]
    heap[:] = oracle.splitmix_bytes(0xBA7C, heap.size)
    jobs = [(ARENA + off, off, n, c) for (off, n), c in zip(extents, (245, 244, 7))]
    want = heap.copy()
    for s, d, n, c in jobs:
        oracle.region_multiply(want[s:s + n].copy(), c, want[d:d + n], 1)
    b = heap.ctypes.data
    assert ec.region_multiply_batch([(b + s, b + d, None, n, c, 1) for s, d, n, c in jobs]) == (1, 1)
    staged, cur = [], 0
    for _, d, n, _ in sorted(jobs, key=lambda j: j[1]):
        cur += (b + d - cur) & 15
        staged.append((cur, n))
        cur += n
    check_record(ec, staged, [], ec.CEC_KERNEL_NARROW, 1, 1, ec.CEC_ACC_ALL)
    assert np.array_equal(heap, want)
