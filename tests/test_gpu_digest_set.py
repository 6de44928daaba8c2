"""GPU: cec_digest_set and cec_diff_update_digests keep the live digests of every arena of a
group equal to cec_digest_region of that arena through the SET path, and leave the arenas
with cec_diff_update's bytes.

Expected bytes come from the numpy model of tests/digest_set_case.py (pinned on the CPU in
tests/test_digest_set.py), never from the library: the arenas from the SET itself, the digests
from region_digests of the arenas after it, cross-checked there against the positioned fold of
new ^ old.  One arena length, uc.LEN (8 units, a ragged last one), and the 14 disjoint tiles of
uc.EXTENTS: four values in one unit, a full aligned unit, three units from mid-unit, unaligned
starts, a single last byte, two bytes across a boundary, a value that ends at LEN.
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import digest_case as dc  # noqa: E402
import digest_set_case as sc  # noqa: E402
import digest_update_case as uc  # noqa: E402

LEN, N_UNITS, TILE = uc.LEN, uc.N_UNITS, uc.TILE


def dev(torch, a, shift=0):
    """A device copy of host bytes; `shift`: its base moved by that many bytes."""
    t = torch.empty(a.size + shift + 64, dtype=torch.uint8, device="cuda")
    t[shift:shift + a.size].copy_(torch.from_numpy(a))
    return t[shift:shift + a.size]


def plan_of(ec, rows):
    return ec.Plan([(off, so, n, j) for off, so, n, j in rows])


def host(t) -> np.ndarray:
    return t.cpu().numpy()


def units(bufs, i) -> np.ndarray:
    return bufs.host(i).reshape(N_UNITS, dc.DIGEST_BYTES)


def diff_update_launches(m_live: int, install: bool) -> int:
    """cec_diff_update's launches: a pattern holds four outputs (the live parities, then the
    install), so one launch for up to four and one more per further four."""
    return (m_live + int(install) + 3) // 4


@functools.lru_cache(maxsize=None)
def case(k, m, install, lost=()):
    """The host side of one case, computed once: matrix, rows, the group before, the arenas
    and the digests (data lids, then parities) after.  Tests only read these arrays."""
    from cocytus_amd import ec

    mat = ec.coding_matrix(k, m)
    if (k, m) == (3, 2):
        assert mat == sc.RS32
    rows = sc.rows_for(k)
    data, parity, staging = sc.random_group(k, m, mat, rows, seed=16 * k + m)
    d_after, p_after = sc.set_model(mat, k, m, data, parity, staging, rows, install, lost)
    want = sc.digests_after(mat, k, m, data, parity, staging, rows, install, lost)
    before = [uc.region_digests(a) for a in data + parity]
    return mat, rows, data, parity, staging, d_after + p_after, want, before


class Group:
    """The device side: arenas, staging, and guarded live digests based with digest_region."""

    def __init__(self, gpu, k, m, data, parity, staging, shift_arena=0, shift_staging=0):
        torch, ec = gpu
        self.k, self.m = k, m
        self.arenas = [dev(torch, a, shift_arena) for a in data + parity]
        self.staging = dev(torch, staging, shift_staging)
        self.live = dc.DigestBuffers(torch, k + m, N_UNITS)
        ec.digest_region(self.arenas, self.live.views, LEN)
        torch.cuda.synchronize()

    @property
    def data(self):
        return self.arenas[:self.k]

    @property
    def parity(self):
        return self.arenas[self.k:]

    @property
    def data_digests(self):
        return self.live.views[:self.k]

    @property
    def parity_digests(self):
        return self.live.views[self.k:]

    def digests(self):
        return [units(self.live, i) for i in range(self.k + self.m)]


def expect_set_record(ec, n_tiles):
    rec = ec.last_launch()
    assert (rec["kind"], rec["nt"], rec["lt"], rec["acc"], rec["engine"]) == (
        7, 2, 0, ec.CEC_ACC_ALL, ec.CEC_ENGINE_PERM), rec
    assert rec["kind"] == ec.CEC_KERNEL_DIGEST_SET
    assert (rec["split_shift"], rec["flags"], rec["n_tiles"], rec["grid"], rec["lds_bytes"]) == (
        0, 0, n_tiles, (n_tiles + 3) // 4, 0), rec
    assert ec.last_engine() == ec.CEC_ENGINE_PERM


BYTES_CASES = [(k, m, install, 0, 0) for k, m in ((3, 2), (6, 3), (11, 8)) for install in (True, False)] + [
    (3, 2, True, 0, 1), (3, 2, True, 1, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ["perm", "lds"])
@pytest.mark.parametrize("k,m,install,shift_arena,shift_staging", BYTES_CASES,
                         ids=["rs%d%d-%s%s%s" % (k, m, "install" if i else "keep", "-arenas+1" * sa, "-staging+1" * ss)
                              for k, m, i, sa, ss in BYTES_CASES])
def test_bytes(gpu, k, m, install, shift_arena, shift_staging, engine):
    """After diff_update_digests every arena equals the model and cec_diff_update on a copy,
    every live array equals the model and a fresh digest_region of its arena; units no tile of
    that lid touches, the guards and the staging are unchanged; without install the data
    digests are bit-identical to before; the launches are the digest launch plus
    cec_diff_update's own (2 in all for m + install <= 4); both engines give these bytes."""
    torch, ec = gpu
    mat, rows, data, parity, staging, after, want, before = case(k, m, install)
    assert {j for _, _, _, j in rows} == set(range(k))
    g = Group(gpu, k, m, data, parity, staging, shift_arena, shift_staging)
    copy = [dev(torch, a, shift_arena) for a in data + parity]
    for lid in range(k + m):
        assert np.array_equal(g.digests()[lid], before[lid]), lid
    saved = ec.get_engine()
    ec.set_engine(ec.CEC_ENGINE_LDS if engine == "lds" else ec.CEC_ENGINE_PERM)
    try:
        with plan_of(ec, rows) as plan:
            assert plan.num_tiles == uc.N_TILES
            seq = ec.last_launch()["seq"]
            ec.diff_update_digests(k, m, mat, g.data, g.staging, g.parity, install, g.data_digests,
                                   g.parity_digests, N_UNITS, plan)
            torch.cuda.synchronize()
            assert ec.last_launch()["seq"] == seq + 1 + diff_update_launches(m, install)
            if m + int(install) <= 4:
                assert ec.last_launch()["seq"] == seq + 2
            assert ec.last_launch()["kind"] in (ec.CEC_KERNEL_EXACT, ec.CEC_KERNEL_GENERIC)
            ec.diff_update(k, m, mat, copy[:k], g.staging, copy[k:], install, plan)
            torch.cuda.synchronize()
    finally:
        ec.set_engine(saved)
    got = g.digests()
    fresh = dc.DigestBuffers(torch, k + m, N_UNITS)
    ec.digest_region(g.arenas, fresh.views, LEN)
    torch.cuda.synchronize()
    tiles = uc.tiles_of(rows)
    for lid in range(k + m):
        assert np.array_equal(host(g.arenas[lid]), after[lid]), lid
        assert torch.equal(g.arenas[lid], copy[lid]), lid
        assert np.array_equal(got[lid], want[lid]), lid
        assert np.array_equal(got[lid], units(fresh, lid)), lid
        touched = {off // TILE for off, _, _, j in tiles if lid >= k or (install and j == lid)}
        for u in set(range(N_UNITS)) - touched:
            assert np.array_equal(got[lid][u], before[lid][u]), (lid, u)
        if lid < k:
            assert touched < set(range(N_UNITS)) or k == 1
            if not install:
                assert np.array_equal(got[lid], before[lid]), lid
    assert g.live.guards_intact() and fresh.guards_intact()
    assert np.array_equal(host(g.staging), staging)


@pytest.mark.gpu
def test_lost_parity(gpu):
    """parity[1] = None on RS(3,2): that arena and its digest array are untouched (its digest
    pointer may be None as well), the others are right."""
    torch, ec = gpu
    k, m = 3, 2
    mat, rows, data, parity, staging, after, want, before = case(k, m, True, (1,))
    g = Group(gpu, k, m, data, parity, staging)
    raw1 = g.live.raw[k + 1].clone()
    with plan_of(ec, rows) as plan:
        seq = ec.last_launch()["seq"]
        ec.diff_update_digests(k, m, mat, g.data, g.staging, [g.parity[0], None], True, g.data_digests,
                               [g.parity_digests[0], None], N_UNITS, plan)
        torch.cuda.synchronize()
        assert ec.last_launch()["seq"] == seq + 2
    got = g.digests()
    for lid in range(k + m):
        assert np.array_equal(host(g.arenas[lid]), after[lid]), lid
        assert np.array_equal(got[lid], want[lid]), lid
    assert np.array_equal(host(g.arenas[k + 1]), parity[1]) and np.array_equal(got[k + 1], before[k + 1])
    assert torch.equal(g.live.raw[k + 1], raw1)
    assert g.live.guards_intact()


@pytest.mark.gpu
def test_primitive(gpu):
    """digest_set alone: the arenas are unchanged, the digests equal the model of the installed
    batch, the launch record is kind 7, 2 x 0, ACC_ALL, PERM, no split, no flags, grid
    (14 + 3) // 4, no LDS; a second call restores the digests; None entries and a None array
    are skipped and leave their arrays untouched."""
    torch, ec = gpu
    k, m = 3, 2
    mat, rows, data, parity, staging, after, want, before = case(k, m, True)
    g = Group(gpu, k, m, data, parity, staging)
    raws = [r.clone() for r in g.live.raw]
    saved = ec.get_engine()
    ec.set_engine(ec.CEC_ENGINE_LDS)  # (PERM arithmetic whatever the setting)
    try:
        with plan_of(ec, rows) as plan, ec.Plan([]) as empty:
            seq = ec.last_launch()["seq"]
            ec.digest_set(k, m, mat, g.data, g.staging, g.data_digests, g.parity_digests, N_UNITS, plan)
            torch.cuda.synchronize()
            assert ec.last_launch()["seq"] == seq + 1
            expect_set_record(ec, uc.N_TILES)
            assert (uc.N_TILES + 3) // 4 == 4
            for lid in range(k + m):
                assert np.array_equal(host(g.arenas[lid]), (data + parity)[lid]), lid
                assert np.array_equal(g.digests()[lid], want[lid]), lid
            assert np.array_equal(host(g.staging), staging)
            ec.digest_set(k, m, mat, g.data, g.staging, g.data_digests, g.parity_digests, N_UNITS, plan)
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(g.live.raw, raws))  # restored

            # data lid 1 and parity 0 not kept: only the others move
            ec.digest_set(k, m, mat, g.data, g.staging, [g.data_digests[0], None, g.data_digests[2]],
                          [None, g.parity_digests[1]], N_UNITS, plan)
            torch.cuda.synchronize()
            expect_set_record(ec, uc.N_TILES)
            for lid in range(k + m):
                kept = lid not in (1, k)
                assert np.array_equal(g.digests()[lid], want[lid] if kept else before[lid]), lid
                if not kept:
                    assert torch.equal(g.live.raw[lid], raws[lid])
            # no data digests at all: the parity side of the same batch, which restores parity 1
            ec.digest_set(k, m, mat, g.data, g.staging, None, [None, g.parity_digests[1]], N_UNITS, plan)
            torch.cuda.synchronize()
            for lid in range(k + m):
                assert np.array_equal(g.digests()[lid], want[lid] if lid in (0, 2) else before[lid]), lid
            # nothing kept: a launch that reads nothing and writes nothing
            ec.digest_set(k, m, mat, g.data, g.staging, None, None, N_UNITS, plan)
            seq = ec.last_launch()["seq"]
            ec.digest_set(k, m, mat, g.data, g.staging, g.data_digests, g.parity_digests, N_UNITS, empty)
            assert ec.last_launch()["seq"] == seq  # an empty plan launches nothing
            torch.cuda.synchronize()
            for lid in range(k + m):
                assert np.array_equal(g.digests()[lid], want[lid] if lid in (0, 2) else before[lid]), lid
    finally:
        ec.set_engine(saved)
    assert g.live.guards_intact()


@pytest.mark.gpu
def test_refusals(gpu):
    """Every CEC_EINVAL of the primitive, the strict NULLs of the composite, and CEC_EOVERLAP for
    two extents on the same bytes: the status with a message that names the offender, and
    seq, arenas and digests unchanged."""
    torch, ec = gpu
    k, m = 3, 2
    mat, rows, data, parity, staging, after, want, before = case(k, m, True)
    g = Group(gpu, k, m, data, parity, staging)
    raws = [r.clone() for r in g.live.raw]
    dd, pd = g.data_digests, g.parity_digests
    odd = g.live.raw[0][dc.GUARD + 8:]  # a digest array that is not 16-byte aligned
    assert odd.data_ptr() % 16 == 8

    def refused(call, word, code=None):
        with pytest.raises(ec.CecError) as ei:
            call()
        assert ei.value.code == (ec.CEC_EINVAL if code is None else code), str(ei.value)
        assert word in str(ei.value), str(ei.value)

    class NoPlan:
        handle = None

    with plan_of(ec, rows) as plan, ec.Plan([(0, 0, 64, 3)]) as pat3, \
            ec.Plan([(0, 0, 16, 0), (N_UNITS * TILE - 15, 16, 16, 1)]) as beyond, \
            ec.Plan([(TILE + 48, 0, 300, 1), (TILE + 48, 304, 300, 2)]) as overlap:
        seq = ec.last_launch()["seq"]

        def prim(k_=k, m_=m, mat_=mat, data_=g.data, st=g.staging, dd_=dd, pd_=pd, n=N_UNITS, plan_=plan):
            return lambda: ec.digest_set(k_, m_, mat_, data_, st, dd_, pd_, n, plan_)

        def comp(data_=g.data, st=g.staging, par=g.parity, install=True, dd_=dd, pd_=pd, n=N_UNITS, plan_=plan,
                 k_=k):
            return lambda: ec.diff_update_digests(k_, m, mat, data_, st, par, install, dd_, pd_, n, plan_)

        refused(prim(k_=0), "unsupported code")
        refused(prim(m_=9), "unsupported code")
        refused(prim(mat_=mat[:-1] + [256]), "outside GF(2^8)")
        refused(prim(data_=None), "NULL")
        refused(prim(st=None), "NULL")
        refused(prim(plan_=NoPlan()), "NULL")
        refused(prim(data_=[g.data[0], None, g.data[2]]), "data[1] is NULL")
        refused(prim(dd_=[dd[0], odd, dd[2]]), "data_digests[1] is not 16-byte aligned")
        refused(prim(pd_=[pd[0], odd]), "parity_digests[1] is not 16-byte aligned")
        refused(prim(plan_=pat3), "source shard 3")
        refused(prim(n=2 ** 52 + 1), "no unit count")
        refused(prim(plan_=beyond), "extent 1 ends at")
        refused(prim(n=N_UNITS - 1), "extent 10 ends at")
        refused(prim(plan_=overlap), "overlap", ec.CEC_EOVERLAP)
        if torch.cuda.device_count() > 1:  # (a plan of another device: only where there is one)
            torch.cuda.set_device(1)
            try:
                refused(prim(), "device")
                refused(comp(), "device")
            finally:
                torch.cuda.set_device(0)

        # the composite: the primitive's refusals ...
        refused(comp(k_=17), "unsupported code")
        refused(comp(data_=None), "NULL")
        refused(comp(st=None), "NULL")
        refused(comp(par=None), "NULL")
        refused(comp(plan_=NoPlan()), "NULL")
        refused(comp(data_=[g.data[0], None, g.data[2]]), "data[1] is NULL")
        refused(comp(dd_=[dd[0], odd, dd[2]]), "data_digests[1] is not 16-byte aligned")
        refused(comp(pd_=[odd, pd[1]]), "parity_digests[0] is not 16-byte aligned")
        refused(comp(plan_=pat3), "source shard 3")
        refused(comp(n=2 ** 52 + 1), "no unit count")
        refused(comp(plan_=beyond), "extent 1 ends at")
        refused(comp(n=N_UNITS - 1), "extent 10 ends at")
        refused(comp(plan_=overlap), "overlap", ec.CEC_EOVERLAP)
        # ... and its strict NULLs: every arena it writes has its digests kept
        refused(comp(dd_=None), "data_digests is NULL")
        refused(comp(dd_=[dd[0], dd[1], None]), "data_digests[2] is NULL")
        refused(comp(pd_=None), "parity_digests[0] is NULL")
        refused(comp(pd_=[pd[0], None]), "parity_digests[1] is NULL")
        refused(comp(par=[None, g.parity[1]], pd_=[pd[0], None]), "parity_digests[1] is NULL")

        assert ec.last_launch()["seq"] == seq
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(g.live.raw, raws))
        for lid in range(k + m):
            assert np.array_equal(host(g.arenas[lid]), (data + parity)[lid]), lid

        # without install the data digests are not needed, nor a lost parity's: accepted
        ec.diff_update_digests(k, m, mat, g.data, g.staging, [g.parity[0], None], False, None, [pd[0], None],
                               N_UNITS, plan)
        torch.cuda.synchronize()
        assert ec.last_launch()["seq"] == seq + 2
    assert g.live.guards_intact()


@pytest.mark.gpu
def test_failed_launches(gpu):
    """An injected failure of the second launch: CEC_EHIP, every arena and every digest as before
    the call (the digest launch ran twice), the last launch record is kind 7.  An injected
    failure of the first: CEC_EHIP, nothing launched.  Then the op works."""
    torch, ec = gpu
    k, m = 3, 2
    mat, rows, data, parity, staging, after, want, before = case(k, m, True)
    g = Group(gpu, k, m, data, parity, staging)
    raws = [r.clone() for r in g.live.raw]

    def unchanged():
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(g.live.raw, raws))
        for lid in range(k + m):
            assert np.array_equal(host(g.arenas[lid]), (data + parity)[lid]), lid

    def call(plan):
        ec.diff_update_digests(k, m, mat, g.data, g.staging, g.parity, True, g.data_digests, g.parity_digests,
                               N_UNITS, plan)

    with plan_of(ec, rows) as plan:
        seq = ec.last_launch()["seq"]
        ec.fail_launch(1)
        try:
            with pytest.raises(ec.CecError) as ei:
                call(plan)
        finally:
            ec.fail_launch(-1)
        assert ei.value.code == ec.CEC_EHIP and "as before the call" in str(ei.value), str(ei.value)
        assert ec.last_launch()["seq"] == seq + 2  # the digest launch and the one that undid it
        expect_set_record(ec, uc.N_TILES)
        unchanged()

        ec.fail_launch(0)
        try:
            with pytest.raises(ec.CecError) as ei:
                call(plan)
        finally:
            ec.fail_launch(-1)
        assert ei.value.code == ec.CEC_EHIP
        assert ec.last_launch()["seq"] == seq + 2
        unchanged()

        ec.fail_launch(0)
        try:
            with pytest.raises(ec.CecError) as ei:
                ec.digest_set(k, m, mat, g.data, g.staging, g.data_digests, g.parity_digests, N_UNITS, plan)
        finally:
            ec.fail_launch(-1)
        assert ei.value.code == ec.CEC_EHIP
        assert ec.last_launch()["seq"] == seq + 2
        unchanged()

        call(plan)
        torch.cuda.synchronize()
        assert ec.last_launch()["seq"] == seq + 4
    for lid in range(k + m):
        assert np.array_equal(host(g.arenas[lid]), after[lid]), lid
        assert np.array_equal(g.digests()[lid], want[lid]), lid
    assert g.live.guards_intact()


def batch_rows(seed):
    """A SET batch of its own for the end-to-end run: 16-byte aligned values of 16..4096 bytes,
    one per unit, sources in rotation."""
    rng = np.random.default_rng(0xE2E + seed)
    ext = []
    for u in range(N_UNITS):
        if rng.integers(0, 4) == 0:
            continue
        at = int(rng.integers(0, 128)) * 16
        n = int(rng.integers(1, (TILE - at) // 16 + 1)) * 16
        n = min(n, LEN - (u * TILE + at))
        ext.append((u * TILE + at, n, (u + seed) % 3))
    return uc.packed(ext)


@pytest.mark.gpu
def test_end_to_end(gpu):
    """The five live arrays of an encoded RS(3,2) group, three SET batches through
    diff_update_digests: the group check over the live arrays flags 0 units and every arena
    agrees with its live array.  A fourth batch through plain diff_update, a SET that bypassed
    the digests: verify_region flags exactly the touched units of each written arena."""
    torch, ec = gpu
    k, m = 3, 2
    mat = ec.coding_matrix(k, m)
    data, parity, _ = sc.random_group(k, m, mat, sc.rows_for(k), seed=99, consistent=True)
    g = Group(gpu, k, m, data, parity, np.zeros(16, dtype=np.uint8))
    model_d, model_p = data, parity

    def fresh_of(lid):
        b = dc.DigestBuffers(torch, 1, N_UNITS)
        ec.digest_region([g.arenas[lid]], b.views, LEN)
        return b

    with ec.Scrub(N_UNITS) as report:
        for seed in (1, 2, 3, 4):
            rows = batch_rows(seed)
            rng = np.random.default_rng(0xBA7C4 + seed)
            staging = rng.integers(0, 256, max(so + n for _, so, n, _ in rows) + 16, dtype=np.uint8)
            d_staging = dev(torch, staging)
            model_d, model_p = sc.set_model(mat, k, m, model_d, model_p, staging, rows, True)
            with plan_of(ec, rows) as plan:
                if seed < 4:
                    ec.diff_update_digests(k, m, mat, g.data, d_staging, g.parity, True, g.data_digests,
                                           g.parity_digests, N_UNITS, plan)
                else:
                    ec.diff_update(k, m, mat, g.data, d_staging, g.parity, True, plan)
                torch.cuda.synchronize()
            for lid in range(k + m):
                assert np.array_equal(host(g.arenas[lid]), (model_d + model_p)[lid]), (seed, lid)
            if seed < 4:
                report.run_digests_region(k, m, mat, g.data_digests, g.parity_digests, LEN)
                assert report.wait() == 0 and report.findings() == [], seed
                for lid in range(k + m):
                    report.verify_region(g.live.views[lid], fresh_of(lid).views[0], LEN)
                    assert report.wait() == 0, (seed, lid)
                    assert np.array_equal(units(g.live, lid), uc.region_digests((model_d + model_p)[lid]))
        # the fourth batch went past the digests: each arena's self-check names its stale units
        tiles = uc.tiles_of(rows)
        assert tiles
        for lid in range(k + m):
            touched = sorted({off // TILE for off, _, _, j in tiles if lid >= k or j == lid})
            report.verify_region(g.live.views[lid], fresh_of(lid).views[0], LEN)
            assert report.wait() == len(touched), lid
            assert [f["tile"] for f in report.findings()] == touched, lid
        assert {off // TILE for off, _, _, _ in tiles}  # (the parities have stale units)
    assert g.live.guards_intact()
