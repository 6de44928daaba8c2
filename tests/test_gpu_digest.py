"""GPU: cec_digest writes the model's bytes, and cec_scrub_digests finds on the digests
exactly what cec_scrub finds on the arenas.

The expected digests come from the numpy model of tests/digest_case.py (pinned against the
oracle in tests/test_digest.py); the arena groups, the ragged and full extents and the
one-finding check are tests/scrub_case.py's.  Every test leaves the module's groups as it
found them.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import digest_case as dc  # noqa: E402

CODES = [(3, 2), (4, 2), (6, 3), (10, 4), (5, 1), (12, 8)]
MIXED = dc.RAGGED + dc.FULL
MIXED_TILES = dc.tiles_of(MIXED)
FULL_TILES = dc.tiles_of(dc.FULL)
WAVES_SHIFT = min(2, max(0, int(os.environ.get("CEC_DIGEST_WAVES_SHIFT") or 2)))  # work items per workgroup, log2

_groups = {}


def group(gpu, oracle, k, m):
    torch, ec = gpu
    if (k, m) not in _groups:
        _groups[k, m] = dc.Group(torch, ec, oracle, k, m)
    return _groups[k, m]


def plan_of(ec, extents):
    return ec.Plan([(o, 0, n, 0) for o, n in extents])


def check_capacity(k, lt):
    return (4 if k <= 4 else 8 if k <= 8 else 16), (1 if lt <= 1 else 2 if lt <= 2 else 4)


def digest_all(gpu, g, plan, n_tiles):
    """Fresh digest arrays of every arena of the group over the plan."""
    torch, ec = gpu
    bufs = dc.DigestBuffers(torch, g.k + g.m, n_tiles)
    ec.digest(g.arenas, bufs.views, plan)
    return bufs


def check(g, report, bufs, plan):
    report.run_digests(g.k, g.m, g.mat, bufs.views[:g.k], bufs.views[g.k:], plan)
    return report.wait()


def expect_digest_record(ec, n, n_tiles):
    rec = ec.last_launch()
    assert (rec["kind"], rec["nt"], rec["lt"], rec["acc"], rec["engine"]) == (
        ec.CEC_KERNEL_DIGEST, n, 0, ec.CEC_ACC_NONE, ec.CEC_ENGINE_PERM), rec
    per_wg = 1 << WAVES_SHIFT
    assert (rec["split_shift"], rec["flags"], rec["n_tiles"], rec["grid"], rec["lds_bytes"]) == (
        0, 0, n_tiles, (n_tiles * n + per_wg - 1) // per_wg, 0), rec
    assert ec.last_engine() == ec.CEC_ENGINE_PERM


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", CODES)
def test_bytes_equal_the_model(gpu, oracle, k, m):
    """Every tile of the mixed and of the full plan, one arena alone and the whole group in
    one launch: the model's bytes, guards untouched, the slab untouched, the launch record
    as specified; a second run into a dirtied buffer writes the same bytes."""
    torch, ec = gpu
    g = group(gpu, oracle, k, m)
    before = g.slab.clone()
    host = [a.cpu().numpy() for a in g.arenas]
    engine = ec.get_engine()
    ec.set_engine(ec.CEC_ENGINE_LDS)  # (PERM arithmetic whatever the setting)
    try:
        for extents, tiles in ((MIXED, MIXED_TILES), (dc.FULL, FULL_TILES)):
            want = [dc.digests_of(h, tiles) for h in host]
            with plan_of(ec, extents) as plan:
                for lids in ([k + m - 1], list(range(k + m))):
                    bufs = dc.DigestBuffers(torch, len(lids), len(tiles))
                    seq = ec.last_launch()["seq"]
                    ec.digest([g.arenas[i] for i in lids], bufs.views, plan)
                    torch.cuda.synchronize()
                    assert ec.last_launch()["seq"] == seq + 1
                    expect_digest_record(ec, len(lids), len(tiles))
                    for i, lid in enumerate(lids):
                        assert np.array_equal(bufs.host(i), want[lid]), (lid, len(tiles))
                    for v in bufs.views:
                        v.fill_(0x3C)
                    ec.digest([g.arenas[i] for i in lids], bufs.views, plan)
                    torch.cuda.synchronize()
                    for i, lid in enumerate(lids):
                        assert np.array_equal(bufs.host(i), want[lid]), (lid, "second run")
                    assert bufs.guards_intact()
    finally:
        ec.set_engine(engine)
    assert torch.equal(g.slab, before)


@pytest.mark.gpu
def test_region_tail_and_misaligned_bases(gpu, oracle):
    """The region [0, 8192 + 33) (a short last tile), and a group whose bases are moved by
    one byte (the gather path on full tiles too): the model's bytes."""
    torch, ec = gpu
    g = group(gpu, oracle, 3, 2)
    length = 8192 + 33
    tiles = dc.region_tiles(length)
    assert tiles[-1] == (8192, 33)
    bufs = dc.DigestBuffers(torch, 5, len(tiles))
    ec.digest_region(g.arenas, bufs.views, length)
    torch.cuda.synchronize()
    expect_digest_record(ec, 5, 3)
    for i, a in enumerate(g.arenas):
        assert np.array_equal(bufs.host(i), dc.digests_of(a.cpu().numpy(), tiles)), i
    assert bufs.guards_intact()
    seq = ec.last_launch()["seq"]
    ec.digest_region(g.arenas, bufs.views, 0)  # nothing to do, nothing launched
    with ec.Plan([]) as empty:
        ec.digest(g.arenas, bufs.views, empty)
    assert ec.last_launch()["seq"] == seq

    s = dc.Group(torch, ec, oracle, 3, 2, shift=1, seed=9)
    before = s.slab.clone()
    with plan_of(ec, MIXED) as plan:
        bufs = digest_all(gpu, s, plan, len(MIXED_TILES))
        torch.cuda.synchronize()
        for i, a in enumerate(s.arenas):
            assert np.array_equal(bufs.host(i), dc.digests_of(a.cpu().numpy(), MIXED_TILES)), i
        assert bufs.guards_intact()
    assert torch.equal(s.slab, before)


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", CODES)
def test_clean_group_is_clean(gpu, oracle, k, m):
    """run_digests over a clean group's digests: 0, no findings; one check launch per four
    parities, recorded as the digest check with its capacities."""
    torch, ec = gpu
    g = group(gpu, oracle, k, m)
    with ec.Scrub(len(MIXED_TILES)) as report:
        for extents, tiles in ((MIXED, MIXED_TILES), (dc.FULL, FULL_TILES)):
            with plan_of(ec, extents) as plan:
                bufs = digest_all(gpu, g, plan, len(tiles))
                seq = ec.last_launch()["seq"]
                assert check(g, report, bufs, plan) == 0
                assert report.findings() == []
                rec = ec.last_launch()
                assert rec["seq"] - seq == (m + 3) // 4  # (12,8): two launches of 4 parities
                assert (rec["kind"], rec["acc"], rec["engine"]) == (
                    ec.CEC_KERNEL_DIGEST_CHECK, ec.CEC_ACC_ALL, ec.CEC_ENGINE_PERM), rec
                assert (rec["nt"], rec["lt"]) == check_capacity(k, min(4, m - 4 * ((m - 1) // 4))), rec
                assert (rec["split_shift"], rec["flags"], rec["n_tiles"], rec["grid"]) == (0, 0, len(tiles), 1), rec
                assert ec.last_engine() == ec.CEC_ENGINE_PERM


def flips_agree(gpu, g, report, plan, tiles, cases, lids):
    """One flip at a time: digest + run_digests gives exactly one finding, the tile and lid
    that were hit, equal field for field to cec_scrub's on the arenas."""
    torch, ec = gpu
    for t, b in cases:
        off, n = tiles[t]
        for lid in lids:
            v = g.flip(lid, off + b)
            bufs = digest_all(gpu, g, plan, len(tiles))
            assert check(g, report, bufs, plan) == 1, (t, b, lid)
            found = report.findings()
            dc.expect_one(ec, g, found, t, off, n, lid)
            assert g.scrub(report, plan) == 1
            assert report.findings() == found, (t, b, lid)
            g.flip(lid, off + b, v)
    bufs = digest_all(gpu, g, plan, len(tiles))
    assert check(g, report, bufs, plan) == 0 and report.findings() == []


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", CODES)
def test_one_flipped_byte_each_lid_each_position(gpu, oracle, k, m):
    """Byte 0, 15, 16, 1023, 1024 and 4095 of a full tile and the last valid byte of every
    ragged tile, in every lid."""
    torch, ec = gpu
    g = group(gpu, oracle, k, m)
    with ec.Scrub(len(MIXED_TILES)) as report, plan_of(ec, MIXED) as plan:
        full_t = len(MIXED_TILES) - 2
        cases = [(t, n - 1) for t, (_, n) in enumerate(MIXED_TILES) if n < dc.TILE]
        cases += [(full_t, b) for b in dc.FULL_POSITIONS]
        flips_agree(gpu, g, report, plan, MIXED_TILES, cases, range(k + m))


@pytest.mark.gpu
def test_bytes_outside_every_extent_are_not_read(gpu, oracle):
    """The byte right after (16, 1) and the byte before (8385, 33), in every lid: the digests
    do not change and 0 units are flagged."""
    torch, ec = gpu
    g = group(gpu, oracle, 3, 2)
    with ec.Scrub(len(MIXED_TILES)) as report, plan_of(ec, MIXED) as plan:
        clean = digest_all(gpu, g, plan, len(MIXED_TILES))
        for pos in (17, 8384):
            for lid in range(5):
                v = g.flip(lid, pos)
                bufs = digest_all(gpu, g, plan, len(MIXED_TILES))
                assert torch.equal(bufs.views[lid], clean.views[lid]), (pos, lid)
                assert check(g, report, bufs, plan) == 0, (pos, lid)
                g.flip(lid, pos, v)


@pytest.mark.gpu
def test_distributed_form(gpu, oracle):
    """Each arena digested alone (n = 1) by its own cec_digest_region call on its own stream,
    the digests taken to host memory and back into fresh device buffers, then the check:
    two flips in different units and lids come back as cec_scrub_region reports them."""
    torch, ec = gpu
    k, m = 3, 2
    g = group(gpu, oracle, k, m)
    length = 4 * dc.TILE + 77
    hits = [(0, 1 * dc.TILE + 100), (k, length - 1)]
    vals = [g.flip(lid, pos) for lid, pos in hits]
    torch.cuda.synchronize()
    try:
        streams = [torch.cuda.Stream() for _ in range(k + m)]
        bufs = dc.DigestBuffers(torch, k + m, 5)
        torch.cuda.synchronize()
        for i, s in enumerate(streams):
            ec.digest_region([g.arenas[i]], [bufs.views[i]], length, stream=s)
            expect_digest_record(ec, 1, 5)
        shipped = []
        for i, s in enumerate(streams):
            s.synchronize()
            shipped.append(bufs.host(i).copy())
        fresh = [torch.from_numpy(h).cuda() for h in shipped]
        with ec.Scrub(8) as report:
            report.run_digests_region(k, m, g.mat, fresh[:k], fresh[k:], length)
            assert report.wait() == 2
            found = report.findings()
            assert [(f["tile"], f["off"], f["len"], f["lid"]) for f in found] == [
                (1, dc.TILE, dc.TILE, 0), (4, 4 * dc.TILE, 77, k)], found
            report.run_region(k, m, g.mat, g.data, g.parity, length)
            assert report.wait() == 2
            assert report.findings() == found
    finally:
        for (lid, pos), v in zip(hits, vals):
            g.flip(lid, pos, v)
        torch.cuda.synchronize()


@pytest.mark.gpu
def test_two_chunks_and_the_documented_limit(gpu, oracle):
    """Equal values in one column of two chunks of a tile, (0, 255) and (63, 64): flagged and
    located as the arena scrub does.  The (1, 2, 3) * v pattern in chunks 1, 2, 3: the digest
    check returns 0 while cec_scrub on the arenas returns 1 (the header's LIMIT)."""
    torch, ec = gpu
    k, m, lid, t = 3, 2, 1, 5
    g = group(gpu, oracle, k, m)
    off = FULL_TILES[t][0]
    with ec.Scrub(len(FULL_TILES)) as report, plan_of(ec, dc.FULL) as plan:
        for i, j in ((0, 255), (63, 64)):
            for c in (i, j):
                g.flip(lid, off + 16 * c + 5, 0x6B)
            bufs = digest_all(gpu, g, plan, len(FULL_TILES))
            assert check(g, report, bufs, plan) == 1, (i, j)
            found = report.findings()
            dc.expect_one(ec, g, found, t, off, dc.TILE, lid)
            assert g.scrub(report, plan) == 1 and report.findings() == found
            for c in (i, j):
                g.flip(lid, off + 16 * c + 5, 0x6B)
        for c in (1, 2, 3):
            g.flip(lid, off + 16 * c + 9, int(dc.MUL[c][0x37]))
        bufs = digest_all(gpu, g, plan, len(FULL_TILES))
        assert check(g, report, bufs, plan) == 0
        assert g.scrub(report, plan) == 1
        dc.expect_one(ec, g, report.findings(), t, off, dc.TILE, lid)
        for c in (1, 2, 3):
            g.flip(lid, off + 16 * c + 9, int(dc.MUL[c][0x37]))
        assert g.scrub(report, plan) == 0


@pytest.mark.gpu
def test_repair_after_a_digest_run(gpu, oracle):
    """A data-lid tile (ragged) and a parity-lid tile located from the digests: repair puts
    the original bytes back; digest and check again: 0."""
    torch, ec = gpu
    k, m = 3, 2
    g = group(gpu, oracle, k, m)
    before = g.slab.clone()
    hits = {4: 0, 15: k + 1}  # tile -> lid
    for t, lid in hits.items():
        off, n = MIXED_TILES[t]
        for b in {0, n // 2, n - 1}:
            g.flip(lid, off + b)
    with ec.Scrub(len(MIXED_TILES)) as report, plan_of(ec, MIXED) as plan:
        bufs = digest_all(gpu, g, plan, len(MIXED_TILES))
        assert check(g, report, bufs, plan) == 2
        assert {f["tile"]: f["lid"] for f in report.findings()} == hits
        assert report.repair(k, m, g.mat, g.data, g.parity) == 0
        torch.cuda.synchronize()
        assert torch.equal(g.slab, before)
        bufs = digest_all(gpu, g, plan, len(MIXED_TILES))
        assert check(g, report, bufs, plan) == 0


@pytest.mark.gpu
def test_refusals_and_failure(gpu, oracle):
    """More units than the report holds, a NULL parity digest, a plan with a pattern index and
    a misaligned digest array are refused with nothing launched; an injected launch failure
    leaves the report invalid until the next good run, and a failed cec_digest writes nothing."""
    torch, ec = gpu
    k, m = 3, 2
    g = group(gpu, oracle, k, m)
    n_tiles = len(MIXED_TILES)
    with plan_of(ec, MIXED) as plan, ec.Scrub(n_tiles) as report:
        bufs = digest_all(gpu, g, plan, n_tiles)
        assert check(g, report, bufs, plan) == 0
        seq = ec.last_launch()["seq"]
        with ec.Scrub(4) as small:
            with pytest.raises(ec.CecError) as ei:
                small.run_digests(k, m, g.mat, bufs.views[:k], bufs.views[k:], plan)
            assert ei.value.code == ec.CEC_EINVAL and "report holds" in str(ei.value)
        with pytest.raises(ec.CecError) as ei:
            report.run_digests(k, m, g.mat, bufs.views[:k], [bufs.views[k], None], plan)
        assert ei.value.code == ec.CEC_EINVAL and "NULL" in str(ei.value)
        with pytest.raises(ec.CecError) as ei:
            report.run_digests(k, m, g.mat, [bufs.raw[0][8:]] + bufs.views[1:k], bufs.views[k:], plan)
        assert ei.value.code == ec.CEC_EINVAL and "aligned" in str(ei.value)
        with ec.Plan([(0, 0, 4096, 1)]) as patterned:
            with pytest.raises(ec.CecError) as ei:
                report.run_digests(k, m, g.mat, bufs.views[:k], bufs.views[k:], patterned)
            assert ei.value.code == ec.CEC_EINVAL and "pattern" in str(ei.value)
            with pytest.raises(ec.CecError) as ei:
                ec.digest(g.arenas, bufs.views, patterned)
            assert ei.value.code == ec.CEC_EINVAL and "pattern" in str(ei.value)
        with pytest.raises(ec.CecError) as ei:
            ec.digest(g.arenas[:1], [bufs.raw[0][8:]], plan)
        assert ei.value.code == ec.CEC_EINVAL and "aligned" in str(ei.value)
        assert ec.last_launch()["seq"] == seq  # nothing launched
        assert report.wait() == 0              # (refused before the report was touched)

        ec.fail_launch(0)
        with pytest.raises(ec.CecError) as ei:
            report.run_digests(k, m, g.mat, bufs.views[:k], bufs.views[k:], plan)
        assert ei.value.code == ec.CEC_EHIP
        for call in (report.wait, report.findings):
            with pytest.raises(ec.CecError) as ei:
                call()
            assert ei.value.code == ec.CEC_EINVAL
        assert check(g, report, bufs, plan) == 0  # a successful run afterwards works

        dirty = dc.DigestBuffers(torch, k + m, n_tiles, fill=0x77)
        ec.fail_launch(0)
        with pytest.raises(ec.CecError) as ei:
            ec.digest(g.arenas, dirty.views, plan)
        assert ei.value.code == ec.CEC_EHIP
        torch.cuda.synchronize()
        assert all(bool((r == 0x77).all()) for r in dirty.raw)  # nothing written
        ec.digest(g.arenas, dirty.views, plan)                  # the hook has disarmed
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(dirty.views, bufs.views))
