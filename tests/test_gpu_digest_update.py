"""GPU: cec_digest_apply_diffs keeps a live digest array equal to cec_digest_region of the
arena, through the op itself and through all three paths of the drainer; the self-check and
the cross-process check over live arrays find what they should.

Expected bytes come from the numpy model of tests/digest_update_case.py (its identity is
pinned on the CPU in tests/test_digest_update.py), never from the library.  One arena of
LEN = 8 * 4096 - 19 bytes (a ragged last unit, 8 units) and the extents of that file.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import digest_case as dc  # noqa: E402
import digest_update_case as uc  # noqa: E402

LEN, N_UNITS, TILE = uc.LEN, uc.N_UNITS, uc.TILE
ROWS = uc.packed(uc.EXTENTS)
RNG_SEED = 0xD16E57


def dev(torch, a, shift=0):
    """A device copy of host bytes; `shift`: its base moved by that many bytes."""
    t = torch.empty(a.size + shift + 64, dtype=torch.uint8, device="cuda")
    t[shift:shift + a.size].copy_(torch.from_numpy(a))
    return t[shift:shift + a.size]


def plan_of(ec, rows):
    return ec.Plan([(off, so, n, j) for off, so, n, j in rows])


def live_of(gpu, arena):
    """Fresh guarded digests of one device arena: cec_digest_region."""
    torch, ec = gpu
    bufs = dc.DigestBuffers(torch, 1, N_UNITS)
    ec.digest_region([arena], bufs.views, LEN)
    return bufs


def host_digests(bufs) -> np.ndarray:
    return bufs.host(0).reshape(N_UNITS, dc.DIGEST_BYTES)


def row_of(mat, k, lid):
    return [mat[lid * k + j] for j in range(k)]


def random_case(rows, seed=0):
    rng = np.random.default_rng(RNG_SEED + seed)
    arena = rng.integers(0, 256, LEN, dtype=np.uint8)
    diffs = rng.integers(0, 256, max(so + n for _, so, n, _ in rows) + 16, dtype=np.uint8)
    return arena, diffs


def expect_update_record(ec, n_tiles):
    rec = ec.last_launch()
    assert (rec["kind"], rec["nt"], rec["lt"], rec["acc"], rec["engine"]) == (
        ec.CEC_KERNEL_DIGEST_UPDATE, 1, 0, ec.CEC_ACC_ALL, ec.CEC_ENGINE_PERM), rec
    assert (rec["split_shift"], rec["flags"], rec["n_tiles"], rec["grid"], rec["lds_bytes"]) == (
        0, 0, n_tiles, (n_tiles + 3) // 4, 0), rec
    assert ec.last_engine() == ec.CEC_ENGINE_PERM


@pytest.mark.gpu
@pytest.mark.parametrize("k,m,lid,shift", [(3, 2, 4, 0), (3, 2, 3, 0), (3, 2, 1, 0), (3, 2, 4, 1), (6, 3, 8, 0)],
                         ids=["rs32-lid4", "rs32-lid3", "rs32-data1", "rs32-lid4-diffs+1", "rs63-lid8"])
def test_bytes(gpu, k, m, lid, shift):
    """live = digest_region(arena); the diffs go into the arena (apply_diffs; for the data lid
    the XOR of its own extents) and into live (digest_apply_diffs): live equals
    digest_region(arena) and the model, byte for byte; units the plan does not touch, the
    guards and the diffs are unchanged; the launch record is as specified."""
    torch, ec = gpu
    mat = ec.coding_matrix(k, m)
    if (k, m) == (3, 2):
        assert row_of(mat, k, 4) == [1, 245, 244] and row_of(mat, k, 3) == [1, 1, 1]
    row = row_of(mat, k, lid)
    if lid < k:
        assert row == uc.identity_row(k, lid)
    rows = [(off, so, n, i % k if k > 3 else j) for i, (off, so, n, j) in enumerate(ROWS)]
    assert {j for _, _, _, j in rows} == set(range(k))
    arena0, diffs = random_case(rows, seed=lid)
    after = uc.apply_to_arena(arena0, diffs, rows, row)
    want = uc.fold_into_digests(uc.region_digests(arena0), diffs, rows, row)
    assert np.array_equal(want, uc.region_digests(after))

    d_diffs = dev(torch, diffs, shift)
    arena = dev(torch, arena0)
    live = live_of(gpu, arena)
    torch.cuda.synchronize()
    before = host_digests(live).copy()
    assert np.array_equal(before, uc.region_digests(arena0))
    engine = ec.get_engine()
    ec.set_engine(ec.CEC_ENGINE_LDS)  # (PERM arithmetic whatever the setting)
    try:
        with plan_of(ec, rows) as plan:
            assert plan.num_tiles == uc.N_TILES
            if lid >= k:
                ec.apply_diffs(k, m, mat, lid, d_diffs, arena, plan)
            else:
                arena.copy_(torch.from_numpy(after))
            seq = ec.last_launch()["seq"]
            ec.digest_apply_diffs(k, m, mat, lid, d_diffs, live.views[0], N_UNITS, plan)
            torch.cuda.synchronize()
            assert ec.last_launch()["seq"] == seq + 1
            expect_update_record(ec, uc.N_TILES)
    finally:
        ec.set_engine(engine)
    assert np.array_equal(arena.cpu().numpy(), after)
    got = host_digests(live)
    assert np.array_equal(got, want)
    assert np.array_equal(got, host_digests(live_of(gpu, arena)))
    touched = {off // TILE for off, _, _, j in uc.tiles_of(rows) if row[j]}
    for u in set(range(N_UNITS)) - touched:
        assert np.array_equal(got[u], before[u]), u
    if lid < k:
        assert touched < set(range(N_UNITS))  # the other shards' extents left their units alone
    assert live.guards_intact()
    assert np.array_equal(d_diffs.cpu().numpy(), diffs)


@pytest.mark.gpu
def test_overlap_and_repeat(gpu):
    """A plan with two extents on the same bytes is accepted (apply_diffs refuses it) and folds
    both; the same plan a second time restores the original digests."""
    torch, ec = gpu
    k, m, lid = 3, 2, 4
    mat = ec.coding_matrix(k, m)
    row = row_of(mat, k, lid)
    rows = uc.packed([(TILE + 48, 300, 1), (TILE + 48, 300, 2), (100, 5000, 0), (7 * TILE + 16, TILE - 35, 2)])
    arena0, diffs = random_case(rows, seed=77)
    base = uc.region_digests(arena0)
    want = uc.fold_into_digests(base, diffs, rows, row)
    assert np.array_equal(want, uc.region_digests(uc.apply_to_arena(arena0, diffs, rows, row)))
    arena, d_diffs = dev(torch, arena0), dev(torch, diffs)
    live = live_of(gpu, arena)
    with plan_of(ec, rows) as plan:
        with pytest.raises(ec.CecError) as ei:
            ec.apply_diffs(k, m, mat, lid, d_diffs, arena, plan)
        assert ei.value.code == ec.CEC_EOVERLAP
        ec.digest_apply_diffs(k, m, mat, lid, d_diffs, live.views[0], N_UNITS, plan)
        torch.cuda.synchronize()
        expect_update_record(ec, 5)
        assert np.array_equal(host_digests(live), want)
        ec.digest_apply_diffs(k, m, mat, lid, d_diffs, live.views[0], N_UNITS, plan)
        torch.cuda.synchronize()
        assert np.array_equal(host_digests(live), base)
    assert live.guards_intact()


def pieces(extents, sizes):
    """The extents cut into disjoint updates of at most sizes[i] bytes each."""
    out = []
    for (off, n, j), step in zip(extents, sizes):
        out += [(off + o, min(step, n - o), j) for o in range(0, n, step)]
    return out


# 38 disjoint updates drawn from the extents, then one more on top of each of two of them:
# 40 updates, two overlapping pairs, two overlap waves
SMALL_WINDOW = pieces(uc.EXTENTS, [256, 256, 16, 1, 512, 1000, 77, 1, 1016, 2, 407]) + [
    (300, 100, 2), (TILE + 700, 64, 0)]
# 48 updates of 4 KiB (the drainer below has 64 KiB of staging per half)
WINDOW_4K = [((i * 3) % 7 * TILE + (16 * i if i % 4 == 0 else 0), TILE, i % 3) for i in range(48)]
# above the small window (1 MiB packed): 17 rounds of 64 KiB through that drainer
PIPELINED = [((i * 5) % 7 * TILE + (3 if i % 9 == 0 else 0), TILE, i % 3) for i in range(272)]


def drain(gpu, updates, staging_bytes, in_place, seed):
    """The updates through an attached and a detached drainer over copies of one parity arena.
    Returns (rounds of the attached apply, i.e. its launches minus the detached one's)."""
    torch, ec = gpu
    k, m, lid = 3, 2, 4
    mat = ec.coding_matrix(k, m)
    row = row_of(mat, k, lid)
    rng = np.random.default_rng(RNG_SEED + seed)
    parity0 = rng.integers(0, 256, LEN, dtype=np.uint8)
    bufs = [rng.integers(0, 256, n, dtype=np.uint8) for _, n, _ in updates]
    want = parity0.copy()
    for (off, n, j), b in zip(updates, bufs):
        want[off:off + n] ^= uc.mul(row[j], b)
    launches = {}
    parity = {}
    for attached in (False, True):
        arena = dev(torch, parity0)
        parity[attached] = arena
        live = live_of(gpu, arena)
        torch.cuda.synchronize()
        with ec.Drainer(k, m, mat, lid, staging_bytes=staging_bytes) as d:
            if attached:
                d.set_digests(live.views[0], N_UNITS)
            if in_place:
                base, view = d.staging()
                ups, so = [], 0
                for (off, n, j), b in zip(updates, bufs):
                    view[so:so + n] = b  # "received" into the staging
                    ups.append((base + so, off, j, n))
                    so = (so + n + 15) & ~15
            else:
                ups = [(b, off, j) for (off, n, j), b in zip(updates, bufs)]
            launches[attached] = d.apply(ups, arena)
            torch.cuda.synchronize()
            if attached:
                rec = ec.last_launch()  # the round's last launch is its digest update
                assert (rec["kind"], rec["nt"], rec["lt"], rec["acc"]) == (
                    ec.CEC_KERNEL_DIGEST_UPDATE, 1, 0, ec.CEC_ACC_ALL), rec
                got = host_digests(live).copy()
                assert np.array_equal(got, uc.region_digests(want))
                assert np.array_equal(got, host_digests(live_of(gpu, arena)))
                assert live.guards_intact()
                # detached again: a further apply changes the parity, not the digests
                d.set_digests(None)
                assert d.apply(ups, arena) == launches[False]
                torch.cuda.synchronize()
                assert np.array_equal(host_digests(live), got)
                assert np.array_equal(arena.cpu().numpy(), parity0)  # (applied twice)
            else:
                assert np.array_equal(arena.cpu().numpy(), want)
    assert torch.equal(parity[False], dev(torch, want))
    return launches[True] - launches[False], launches[False]


@pytest.mark.gpu
def test_drainer_small_window(gpu):
    assert len(SMALL_WINDOW) == 40
    rounds, detached = drain(gpu, SMALL_WINDOW, 1 << 20, in_place=False, seed=1)
    assert (rounds, detached) == (1, 2)  # two overlap waves, one digest launch over both


@pytest.mark.gpu
def test_drainer_in_place_staging(gpu):
    rounds, detached = drain(gpu, SMALL_WINDOW, 1 << 20, in_place=True, seed=2)
    assert (rounds, detached) == (1, 2)


@pytest.mark.gpu
def test_drainer_64k_staging_48_updates(gpu):
    """48 updates of 4 KiB through a drainer with 64 KiB of staging: 192 KiB packed is within
    the drainer's small window (1 MiB), which has its own staging, so this is ONE round."""
    rounds, _ = drain(gpu, WINDOW_4K, 64 << 10, in_place=False, seed=3)
    assert rounds == 1


@pytest.mark.gpu
def test_drainer_pipelined_rounds(gpu):
    """272 updates of 4 KiB (above the small window) through 64 KiB halves: 16 updates per
    round, 17 pipelined rounds, one digest launch behind each round's fold launches."""
    rounds, _ = drain(gpu, PIPELINED, 64 << 10, in_place=False, seed=4)
    assert rounds == 17


@pytest.mark.gpu
def test_self_check(gpu):
    """verify_region(live, fresh) is clean; one flipped byte in unit 3 and one in the ragged
    unit 7 come back as exactly those units, their lengths, lid UNLOCATED."""
    torch, ec = gpu
    arena0, _ = random_case(ROWS, seed=5)
    arena = dev(torch, arena0)
    live = live_of(gpu, arena)
    with ec.Scrub(N_UNITS) as report:
        report.verify_region(live.views[0], live_of(gpu, arena).views[0], LEN)
        assert report.wait() == 0 and report.findings() == []
        rec = ec.last_launch()
        assert (rec["kind"], rec["nt"], rec["lt"]) == (ec.CEC_KERNEL_DIGEST_CHECK, 4, 1), rec
        for pos in (TILE * 3 + 15, LEN - 1):
            arena[pos:pos + 1] ^= 0x40
        fresh = live_of(gpu, arena)
        report.verify_region(live.views[0], fresh.views[0], LEN)
        assert report.wait() == 2
        assert [(f["tile"], f["off"], f["len"], f["lid"]) for f in report.findings()] == [
            (3, 3 * TILE, TILE, ec.CEC_SCRUB_UNLOCATED), (7, 7 * TILE, TILE - 19, ec.CEC_SCRUB_UNLOCATED)]
        assert live.guards_intact() and fresh.guards_intact()


@pytest.mark.gpu
def test_cross_process_check_over_live_arrays(gpu):
    """The live arrays of all five shards of an RS(3,2) group, each kept current through
    digest_apply_diffs over one batch of SETs, pass run_digests_region with 0 findings; a diff
    withheld from parity 4's arena and digests is reported as that unit, lid 4."""
    torch, ec = gpu
    k, m = 3, 2
    mat = ec.coding_matrix(k, m)
    rng = np.random.default_rng(RNG_SEED + 6)
    host = [rng.integers(0, 256, LEN, dtype=np.uint8) for _ in range(k)]
    for p in range(m):
        par = np.zeros(LEN, dtype=np.uint8)
        for j in range(k):
            par ^= uc.mul(mat[(k + p) * k + j], host[j])
        host.append(par)
    arenas = [dev(torch, h) for h in host]
    lives = [live_of(gpu, a) for a in arenas]
    diffs = rng.integers(0, 256, uc.staging_bytes(uc.EXTENTS) + 1024, dtype=np.uint8)
    d_diffs = dev(torch, diffs)

    def batch(rows, lids):
        """One batch of SETs as the shards `lids` see it: arena and live digests both."""
        with plan_of(ec, rows) as plan:
            for lid in lids:
                if lid >= k:
                    ec.apply_diffs(k, m, mat, lid, d_diffs, arenas[lid], plan)
                else:  # the data shard's own values change by their diffs
                    h = uc.apply_to_arena(arenas[lid].cpu().numpy(), diffs, rows, uc.identity_row(k, lid))
                    arenas[lid].copy_(torch.from_numpy(h))
                ec.digest_apply_diffs(k, m, mat, lid, d_diffs, lives[lid].views[0], N_UNITS, plan)
            torch.cuda.synchronize()

    views = [b.views[0] for b in lives]
    with ec.Scrub(N_UNITS) as report:
        batch(ROWS, range(k + m))
        report.run_digests_region(k, m, mat, views[:k], views[k:], LEN)
        assert report.wait() == 0 and report.findings() == []
        for lid in range(k + m):  # every shard's own check passes as well
            report.verify_region(views[lid], live_of(gpu, arenas[lid]).views[0], LEN)
            assert report.wait() == 0, lid
        batch([(3 * TILE + 32, 0, 512, 0)], [0, 1, 2, 3])  # parity 4 never sees this diff
        report.verify_region(views[4], live_of(gpu, arenas[4]).views[0], LEN)
        assert report.wait() == 0  # parity 4 agrees with itself: only the group can tell
        report.run_digests_region(k, m, mat, views[:k], views[k:], LEN)
        assert report.wait() == 1
        assert [(f["tile"], f["off"], f["len"], f["lid"]) for f in report.findings()] == [(3, 3 * TILE, TILE, 4)]
    assert all(b.guards_intact() for b in lives)


@pytest.mark.gpu
def test_refusals_and_failure(gpu):
    """Misaligned digests, a NULL argument, pattern 3 with k = 3, an extent ending at
    n_units * 4096 + 1 and a drainer update beyond n_units: CEC_EINVAL, nothing launched,
    nothing written.  An injected launch failure: CEC_EHIP, digests untouched, the next call works."""
    torch, ec = gpu
    k, m, lid = 3, 2, 4
    mat = ec.coding_matrix(k, m)
    arena0, diffs = random_case(ROWS, seed=8)
    arena, d_diffs = dev(torch, arena0), dev(torch, diffs)
    live = live_of(gpu, arena)
    torch.cuda.synchronize()
    raws = [r.clone() for r in live.raw]
    v = live.views[0]

    def einval(call, word):
        with pytest.raises(ec.CecError) as ei:
            call()
        assert ei.value.code == ec.CEC_EINVAL and word in str(ei.value), str(ei.value)

    with plan_of(ec, ROWS) as plan, ec.Plan([(0, 0, 64, 3)]) as pat3, \
            ec.Plan([(0, 0, 16, 0), (N_UNITS * TILE - 15, 16, 16, 1)]) as beyond, ec.Plan([]) as empty:
        seq = ec.last_launch()["seq"]
        einval(lambda: ec.digest_apply_diffs(k, m, mat, lid, d_diffs, live.raw[0][dc.GUARD + 8:], N_UNITS, plan),
               "aligned")
        einval(lambda: ec.digest_apply_diffs(k, m, mat, lid, None, v, N_UNITS, plan), "NULL")
        einval(lambda: ec.digest_apply_diffs(k, m, mat, lid, d_diffs, None, N_UNITS, plan), "NULL")
        einval(lambda: ec.digest_apply_diffs(k, m, mat, k + m, d_diffs, v, N_UNITS, plan), "lid_self")
        einval(lambda: ec.digest_apply_diffs(k, m, mat, lid, d_diffs, v, N_UNITS, pat3), "source shard 3")
        einval(lambda: ec.digest_apply_diffs(k, m, mat, lid, d_diffs, v, N_UNITS, beyond), "extent 1 ends at")
        einval(lambda: ec.digest_apply_diffs(k, m, mat, lid, d_diffs, v, N_UNITS - 1, plan), "extent 10 ends at")
        ec.digest_apply_diffs(k, m, mat, lid, d_diffs, v, N_UNITS, empty)  # nothing to do
        with ec.Drainer(k, m, mat, lid, staging_bytes=1 << 20) as d:
            einval(lambda: d.set_digests(live.raw[0][dc.GUARD + 8:], N_UNITS), "aligned")
            d.set_digests(v, N_UNITS)
            ups = ec.host_updates([(diffs[:256], 0, 0), (diffs[256:272], N_UNITS * TILE - 15, 1)])
            assert ec.lib().cec_drainer_validate(d._h, ups, 2) == ec.CEC_EINVAL
            einval(lambda: d.apply(ups, arena), "update 1 ends at")
            d.set_digests(None)
            assert ec.lib().cec_drainer_validate(d._h, ups, 2) == ec.CEC_OK  # (detached: as before)
        assert ec.last_launch()["seq"] == seq
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(live.raw, raws))
        assert np.array_equal(arena.cpu().numpy(), arena0)

        ec.fail_launch(0)
        with pytest.raises(ec.CecError) as ei:
            ec.digest_apply_diffs(k, m, mat, lid, d_diffs, v, N_UNITS, plan)
        assert ei.value.code == ec.CEC_EHIP
        torch.cuda.synchronize()
        assert ec.last_launch()["seq"] == seq
        assert all(torch.equal(a, b) for a, b in zip(live.raw, raws))
        ec.digest_apply_diffs(k, m, mat, lid, d_diffs, v, N_UNITS, plan)  # the hook has disarmed
        torch.cuda.synchronize()
        want = uc.fold_into_digests(uc.region_digests(arena0), diffs, ROWS, row_of(mat, k, lid))
        assert np.array_equal(host_digests(live), want)
        assert live.guards_intact()
