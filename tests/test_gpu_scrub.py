"""GPU: cec_scrub finds exactly the corruption that was injected, and nothing else.

An arena group is random data with the oracle's parity (tests/scrub_case.py).  A clean
group scrubs to 0 with every byte of the slab unchanged; a flipped byte comes back as one
finding with the right tile, offset, length, lid and syndromes; cec_scrub_repair puts the
original bytes back.  One plan mixes the kernel-matrix file's ragged extents with 8 full
line-aligned tiles (one 256-lane workgroup per tile), a second holds full aligned tiles
only (four one-wave workgroups per tile): both split shifts are asserted from the launch
record.  The CPU side (classifier model, refusals without a device) is tests/test_scrub.py.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scrub_case as sc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = [(3, 2), (4, 2), (6, 3), (10, 4), (5, 1), (12, 8)]
EXACT = {(3, 2), (4, 2), (6, 3)}
MIXED = sc.RAGGED + sc.FULL
MIXED_TILES = sc.tiles_of(MIXED)
FULL_TILES = sc.tiles_of(sc.FULL)

_groups = {}


def group(gpu, oracle, k, m):
    """One arena group per code for the whole module; every test leaves it as it found it."""
    torch, ec = gpu
    if (k, m) not in _groups:
        _groups[k, m] = sc.Group(torch, ec, oracle, k, m)
    return _groups[k, m]


def plan_of(ec, extents):
    return ec.Plan([(o, 0, n, 0) for o, n in extents])


def capacity(k, m):
    if (k, m) in EXACT:
        return k, m
    lt = min(m, 4)
    return (4 if k <= 4 else 8 if k <= 8 else 16), (1 if lt <= 1 else 2 if lt <= 2 else 4)


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", CODES)
def test_clean_group_is_clean_and_untouched(gpu, oracle, k, m):
    """The oracle's parity, then cec_encode's own, scrub to 0 on both plans (split shift 0
    and 2) with every byte of the slab (data, parity, the bytes around them) unchanged;
    the launch record names the scrub kernel, PERM whatever the engine setting."""
    torch, ec = gpu
    g = group(gpu, oracle, k, m)
    before = g.slab.clone()
    engine = ec.get_engine()
    ec.set_engine(ec.CEC_ENGINE_LDS)
    try:
        with ec.Scrub(len(MIXED_TILES)) as report:
            for extents, tiles, shift in ((MIXED, MIXED_TILES, 0), (sc.FULL, FULL_TILES, 2)):
                with plan_of(ec, extents) as plan:
                    for encode_first in (False, True):
                        if encode_first:
                            ec.encode(k, m, g.mat, g.data, g.parity, plan)
                        seq = ec.last_launch()["seq"]
                        assert g.scrub(report, plan) == 0
                        assert report.findings() == []
                        rec = ec.last_launch()
                        assert rec["seq"] - seq == (m + 3) // 4  # (12,8): two launches of 4 parities
                        assert (rec["kind"], rec["acc"], rec["engine"]) == (
                            ec.CEC_KERNEL_SCRUB, ec.CEC_ACC_ALL, ec.CEC_ENGINE_PERM), rec
                        assert (rec["nt"], rec["lt"]) == capacity(k, m), rec
                        assert (rec["split_shift"], rec["n_tiles"], rec["grid"], rec["flags"]) == (
                            shift, len(tiles), len(tiles) << shift, 0), rec
                        assert ec.last_engine() == ec.CEC_ENGINE_PERM
                        assert torch.equal(g.slab, before)
    finally:
        ec.set_engine(engine)


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", CODES)
def test_one_flipped_byte_each_lid_each_position(gpu, oracle, k, m):
    """Byte 0, 15, 16, 1023, 1024 and 4095 of a full tile under both splits, and the last
    valid byte of every ragged tile: exactly one finding, the tile and lid that were hit.
    The report is reused throughout; m = 1 detects and says UNLOCATED."""
    torch, ec = gpu
    g = group(gpu, oracle, k, m)
    with ec.Scrub(len(MIXED_TILES)) as report:
        with plan_of(ec, MIXED) as plan:
            full_t = len(MIXED_TILES) - 2
            cases = [(t, n - 1) for t, (_, n) in enumerate(MIXED_TILES) if n < sc.TILE]
            cases += [(full_t, b) for b in sc.FULL_POSITIONS]
            sc.check_single_flips(ec, g, report, plan, MIXED_TILES, cases, range(k + m))
            assert ec.last_launch()["split_shift"] == 0
        with plan_of(ec, sc.FULL) as plan:
            sc.check_single_flips(ec, g, report, plan, FULL_TILES, [(5, b) for b in sc.FULL_POSITIONS],
                                  range(k + m))
            assert ec.last_launch()["split_shift"] == 2


@pytest.mark.gpu
def test_bytes_outside_every_extent_are_not_read(gpu, oracle):
    """The byte right after (16, 1) and the byte before (8385, 33), in every lid: 0 flagged."""
    torch, ec = gpu
    g = group(gpu, oracle, 3, 2)
    with ec.Scrub(len(MIXED_TILES)) as report, plan_of(ec, MIXED) as plan:
        for pos in (17, 8384):
            for lid in range(5):
                v = g.flip(lid, pos)
                assert g.scrub(report, plan) == 0, (pos, lid)
                g.flip(lid, pos, v)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [1, 7])
def test_misaligned_bases(gpu, oracle, shift):
    """Every arena base moved by 1 or 7 bytes (the byte-gather path for every tile): clean,
    blind to the bytes outside the extents, and the same findings on a subset."""
    torch, ec = gpu
    g = sc.Group(torch, ec, oracle, 3, 2, shift=shift, seed=shift)
    before = g.slab.clone()
    with ec.Scrub(len(MIXED_TILES)) as report, plan_of(ec, MIXED) as plan:
        assert g.scrub(report, plan) == 0
        assert ec.last_launch()["split_shift"] == 0
        for pos in (17, 8384):
            v = g.flip(1, pos)
            assert g.scrub(report, plan) == 0, pos
            g.flip(1, pos, v)
        cases = [(t, n - 1) for t, (_, n) in enumerate(MIXED_TILES) if n < sc.TILE]
        cases += [(len(MIXED_TILES) - 1, b) for b in (0, 1023, 1024, 4095)]
        sc.check_single_flips(ec, g, report, plan, MIXED_TILES, cases, (0, 2, 3, 4))
    assert torch.equal(g.slab, before)


@pytest.mark.gpu
def test_many_corrupt_tiles(gpu, oracle):
    """64 full tiles, every third one corrupted in rotating lids over 1-300 bytes, one tile
    with two data lids hit at different bytes, one with both parities hit: the counter is
    exact, the findings ascend, every lid is right, the two-lid tiles are UNLOCATED."""
    torch, ec = gpu
    k, m, n_tiles = 3, 2, 64
    g = sc.Group(torch, ec, oracle, k, m, size=n_tiles * sc.TILE, seed=4)
    rng = np.random.default_rng(64)
    want = {}
    for t in range(0, n_tiles, 3):
        lid = (t // 3) % (k + m)
        nbytes = int(rng.integers(1, 301))
        at = np.sort(rng.choice(sc.TILE, nbytes, replace=False)) + t * sc.TILE
        x = torch.from_numpy(rng.integers(1, 256, nbytes, dtype=np.uint8)).cuda()
        g.arenas[lid][torch.from_numpy(at).cuda()] ^= x
        want[t] = lid
    g.flip(0, 1 * sc.TILE + 5)
    g.flip(2, 1 * sc.TILE + 3000)
    g.flip(3, 2 * sc.TILE + 100)
    g.flip(4, 2 * sc.TILE + 101)
    want[1] = want[2] = ec.CEC_SCRUB_UNLOCATED
    with ec.Scrub(n_tiles) as report, plan_of(ec, [(0, n_tiles * sc.TILE)]) as plan:
        assert g.scrub(report, plan) == len(want)
        assert ec.last_launch()["split_shift"] == 2
        found = report.findings()
        assert [f["tile"] for f in found] == sorted(want)
        assert {f["tile"]: f["lid"] for f in found} == want
        assert all((f["off"], f["len"]) == (f["tile"] * sc.TILE, sc.TILE) for f in found)
        assert len(report.findings(cap=5)) == 5
        # the implicit region over the same bytes: the same findings
        report.run_region(k, m, g.mat, g.data, g.parity, n_tiles * sc.TILE)
        assert report.wait() == len(want)
        assert {f["tile"]: f["lid"] for f in report.findings()} == want


@pytest.mark.gpu
def test_implicit_region_tail(gpu, oracle):
    """len = 3 * 4096 + 77: a flip in the tail's last byte is found (tile 3, 77 bytes), a
    flip at byte len is not."""
    torch, ec = gpu
    k, m, n = 3, 2, 3 * sc.TILE + 77
    g = group(gpu, oracle, k, m)  # (the oracle's parity covers [0, n) as well)
    with ec.Scrub(4) as report:
        report.run_region(k, m, g.mat, g.data, g.parity, n)
        assert report.wait() == 0
        assert ec.last_launch()["n_tiles"] == 4
        for lid in range(k + m):
            v = g.flip(lid, n - 1)
            report.run_region(k, m, g.mat, g.data, g.parity, n)
            assert report.wait() == 1
            sc.expect_one(ec, g, report.findings(), 3, 3 * sc.TILE, 77, lid)
            g.flip(lid, n - 1, v)
            v = g.flip(lid, n)
            report.run_region(k, m, g.mat, g.data, g.parity, n)
            assert report.wait() == 0, lid
            g.flip(lid, n, v)
        with pytest.raises(ec.CecError) as ei:  # 5 tiles into a report of 4
            report.run_region(k, m, g.mat, g.data, g.parity, 4 * sc.TILE + 1)
        assert ei.value.code == ec.CEC_EINVAL


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(3, 2), (6, 3)])
def test_repair(gpu, oracle, k, m):
    """Data-lid tiles (ragged ones among them), parity-lid tiles and one two-lid tile:
    repair leaves 1 finding alone, every byte of the slab but that tile's two flipped
    bytes equals the original, and a second scrub flags exactly that tile."""
    torch, ec = gpu
    g = group(gpu, oracle, k, m)
    before = g.slab.clone()
    hits = {0: 0, 4: k - 1, 7: 1, 9: k, 11: k + m - 1, 12: 0, 15: k + 1, 18: 2}  # tile -> lid
    for t, lid in hits.items():
        off, n = MIXED_TILES[t]
        for b in {0, n // 2, n - 1}:
            g.flip(lid, off + b)
    two = 13
    off2 = MIXED_TILES[two][0]
    va, vb = g.flip(0, off2 + 9), g.flip(1, off2 + 2000)
    with ec.Scrub(len(MIXED_TILES)) as report, plan_of(ec, MIXED) as plan:
        assert g.scrub(report, plan) == len(hits) + 1
        assert {f["tile"]: f["lid"] for f in report.findings()} == {**hits, two: ec.CEC_SCRUB_UNLOCATED}
        assert report.repair(k, m, g.mat, g.data, g.parity) == 1
        assert g.scrub(report, plan) == 1
        (f,) = report.findings()
        assert (f["tile"], f["lid"]) == (two, ec.CEC_SCRUB_UNLOCATED)
        g.flip(0, off2 + 9, va)
        g.flip(1, off2 + 2000, vb)
        assert torch.equal(g.slab, before)
        assert g.scrub(report, plan) == 0
        assert report.repair(k, m, g.mat, g.data, g.parity) == 0  # nothing to do


@pytest.mark.gpu
def test_refusals_and_failure(gpu, oracle):
    """An injected launch failure leaves the report invalid until the next good run; a run
    too large for the report, a plan with a pattern index and a NULL parity are refused
    with nothing launched; release_stream, then stream destroy, then report destroy."""
    torch, ec = gpu
    k, m = 3, 2
    g = group(gpu, oracle, k, m)
    L = ec.lib()
    with plan_of(ec, MIXED) as plan:
        report = ec.Scrub(len(MIXED_TILES))
        ec.fail_launch(0)
        with pytest.raises(ec.CecError) as ei:
            report.run(k, m, g.mat, g.data, g.parity, plan)
        assert ei.value.code == ec.CEC_EHIP
        for call in (report.wait, report.findings, lambda: report.repair(k, m, g.mat, g.data, g.parity)):
            with pytest.raises(ec.CecError) as ei:
                call()
            assert ei.value.code == ec.CEC_EINVAL
        assert g.scrub(report, plan) == 0  # a successful run afterwards works

        seq = ec.last_launch()["seq"]
        with ec.Scrub(4) as small:
            with pytest.raises(ec.CecError) as ei:
                small.run(k, m, g.mat, g.data, g.parity, plan)
            assert ei.value.code == ec.CEC_EINVAL and "report holds" in str(ei.value)
        with ec.Plan([(0, 0, 4096, 1)]) as patterned:
            with pytest.raises(ec.CecError) as ei:
                report.run(k, m, g.mat, g.data, g.parity, patterned)
            assert ei.value.code == ec.CEC_EINVAL and "pattern" in str(ei.value)
        with pytest.raises(ec.CecError) as ei:
            report.run(k, m, g.mat, g.data, [g.parity[0], None], plan)
        assert ei.value.code == ec.CEC_EINVAL
        assert ec.last_launch()["seq"] == seq  # nothing launched
        assert report.wait() == 0              # (refused before the report was touched)

        stream = ctypes.c_void_p()
        assert L.cec_stream_create(ctypes.byref(stream)) == ec.CEC_OK
        torch.cuda.synchronize()
        v = g.flip(k, 16)
        torch.cuda.synchronize()
        report.run(k, m, g.mat, g.data, g.parity, plan, stream=stream.value)
        assert report.wait() == 1
        sc.expect_one(ec, g, report.findings(), 0, 16, 1, k)
        g.flip(k, 16, v)
        report.release_stream(stream.value)
        plan.release_stream(stream.value)
        assert L.cec_stream_destroy(stream) == ec.CEC_OK
        report.destroy()


@pytest.mark.gpu
def test_scrub_under_pinned_environment(gpu):
    """CEC_STORE_POLICY=wt changes nothing (the scrub has no stores) and CEC_SPLIT_SHIFT=1,
    the split the automatic rule never picks, finds the same tiles: one child process."""
    e = {x: v for x, v in os.environ.items() if x not in ("CEC_STORE_POLICY", "CEC_WT_MAX_BYTES", "CEC_SPLIT_SHIFT")}
    e.update(CEC_STORE_POLICY="wt", CEC_SPLIT_SHIFT="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "scrub_case.py")], env=e,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]
