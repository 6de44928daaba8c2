"""Shared pieces of tests/test_gpu_scrub.py, and its child-process case.

Run as a child by test_gpu_scrub.py::test_scrub_under_pinned_environment with
CEC_STORE_POLICY=wt and CEC_SPLIT_SHIFT=1 set (the library reads both once per process):
the scrub has no stores, so the store policy changes nothing, and the split the automatic
rule never picks finds the same tiles.  Prints "OK" on success; any mismatch raises.

Expected values are the injected corruption itself and oracle.encode: an arena group is
random data with the oracle's parity, and a flipped byte must come back as one finding
with that tile, that lid.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TILE = 4096
# the kernel-matrix file's ragged extents, then 8 full line-aligned tiles
RAGGED = [(16, 1), (48, 15), (80, 16), (112, 17), (160, 4095), (4272, 4097), (8385, 33), (8439, 4098)]
FULL0 = 16384
FULL = [(FULL0 + i * TILE, TILE) for i in range(8)]
SIZE = FULL0 + 8 * TILE + 64
FULL_POSITIONS = (0, 15, 16, 1023, 1024, 4095)  # chunk, wave / part and tile boundaries


def tiles_of(extents):
    """The tile list cec_plan_create builds: pieces that end on 4 KiB arena boundaries."""
    out = []
    for off, n in extents:
        o = 0
        while o < n:
            step = min(TILE - (off + o) % TILE, n - o)
            out.append((off + o, step))
            o += step
    return out


class Group:
    """k + m arenas in one slab at the odd 4 KiB stride: random bytes everywhere, the
    oracle's parity over [0, size).  `shift`: every base moved by that many bytes."""

    def __init__(self, torch, ec, oracle, k, m, size=SIZE, shift=0, seed=1):
        self.torch, self.ec, self.k, self.m, self.size = torch, ec, k, m, size
        self.mat = oracle.big_vandermonde(k + m, k)
        assert self.mat == ec.coding_matrix(k, m)
        rng = np.random.default_rng(seed + 1000 * k + m)
        views = ec.arena_tensors(k + m, size + shift + 64)
        self.slab = views[0]._base
        self.slab.copy_(torch.from_numpy(rng.integers(0, 256, self.slab.numel(), dtype=np.uint8)))
        host = [rng.integers(0, 256, size, dtype=np.uint8) for _ in range(k)]
        host += oracle.encode(self.mat, k, m, host)
        self.arenas = [v[shift:] for v in views]
        for a, h in zip(self.arenas, host):
            a[:size].copy_(torch.from_numpy(h))
        torch.cuda.synchronize()
        self.data, self.parity = self.arenas[:k], self.arenas[k:]

    def flip(self, lid, pos, v=None):
        """XOR a non-zero value into one byte; returns it (flip again to restore)."""
        v = v or 1 + (pos * 7 + lid * 13) % 255
        self.arenas[lid][pos:pos + 1] ^= v
        return v

    def scrub(self, report, plan):
        report.run(self.k, self.m, self.mat, self.data, self.parity, plan)
        return report.wait()


def expect_one(ec, g, found, tile, off, n, lid):
    """Exactly one finding: that tile, that lid (UNLOCATED when m = 1), its syndromes, and
    for a data lid every other data lid ruled out."""
    assert len(found) == 1, found
    f = found[0]
    assert (f["tile"], f["off"], f["len"]) == (tile, off, n), (f, tile, off, n)
    assert f["syndromes"] == ((1 << g.m) - 1 if lid < g.k else 1 << (lid - g.k)), (f, lid)
    assert f["lid"] == (lid if g.m >= 2 else ec.CEC_SCRUB_UNLOCATED), (f, lid)
    if lid < g.k:
        assert f["ruled_out"] == (((1 << g.k) - 1) & ~(1 << lid) if g.m >= 2 else 0), (f, lid)


def check_single_flips(ec, g, report, plan, tiles, cases, lids):
    """cases: (tile index, byte within the tile).  One flip at a time, each lid in turn,
    the report reused; a run after the byte is restored returns 0."""
    for t, b in cases:
        off, n = tiles[t]
        for lid in lids:
            v = g.flip(lid, off + b)
            assert g.scrub(report, plan) == 1, (t, b, lid)
            expect_one(ec, g, report.findings(), t, off, n, lid)
            g.flip(lid, off + b, v)
    assert g.scrub(report, plan) == 0 and report.findings() == []


def main() -> None:
    import torch

    torch.cuda.set_device(0)
    torch.empty(1, device="cuda")
    from cocytus_amd import ec
    from oracle import pyoracle

    assert ec.device_check() == ec.CEC_OK, ec.lib().cec_last_error()
    assert ec.store_policy()[0] == "wt" and os.environ.get("CEC_SPLIT_SHIFT") == "1"
    for k, m in ((3, 2), (10, 4)):
        g = Group(torch, ec, pyoracle, k, m)
        before = g.slab.clone()
        mixed = RAGGED + FULL
        tiles = tiles_of(mixed)
        with ec.Plan([(o, 0, n, 0) for o, n in mixed]) as plan, ec.Scrub(len(tiles)) as report:
            assert g.scrub(report, plan) == 0
            rec = ec.last_launch()
            assert (rec["kind"], rec["split_shift"], rec["flags"]) == (ec.CEC_KERNEL_SCRUB, 1, 0), rec
            assert rec["grid"] == 2 * len(tiles), rec
            full_t = len(tiles) - 3
            cases = [(t, n - 1) for t, (_, n) in enumerate(tiles) if n < TILE]
            cases += [(full_t, b) for b in (0, 2047, 2048, 4095)]  # the two parts' boundary
            check_single_flips(ec, g, report, plan, tiles, cases, range(k + m))
        assert torch.equal(g.slab, before)
    print("OK")


if __name__ == "__main__":
    main()
