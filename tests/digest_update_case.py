"""Shared pieces of tests/test_digest_update.py and tests/test_gpu_digest_update.py.

The positioned model of cec_digest_apply_diffs, written with tests/digest_case.py's own field
arithmetic (it calls neither the library nor the oracle): a plan tile never crosses a 4 KiB
arena boundary, and for every tile

    digests[off >> 12] ^= c * digest(a 4 KiB unit, zero but for the tile's diff bytes at off & 4095)

The arena of the GPU file and its extents (off, len, j = source data lid) are here too, with
src_off packed at 16-byte steps.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import digest_case as dc  # noqa: E402

TILE = dc.TILE
N_UNITS = 8
LEN = N_UNITS * TILE - 19  # a ragged last unit

EXTENTS = [
    (0, 256, 0), (256, 256, 1), (512, 16, 2), (1024, 1, 0),  # four values in one unit
    (4096, 4096, 1),                                         # a full aligned unit
    (12192, 8288, 2),                                        # three units: from mid-unit to a boundary
    (5 * TILE + 3, 77, 0),                                   # unaligned start, odd length
    (5 * TILE + 4095, 1, 1),                                 # the last byte of a unit
    (6 * TILE + 16, 4064, 2),
    (7 * TILE - 1, 2, 1),                                    # two bytes across a boundary
    (7 * TILE + 16, TILE - 35, 0),                           # ends at LEN
]
N_TILES = 14


def packed(extents):
    """[(off, src_off, len, j)]: src_off packed at 16-byte steps in extent order."""
    out, so = [], 0
    for off, n, j in extents:
        out.append((off, so, n, j))
        so += (n + 15) & ~15
    return out


def staging_bytes(extents) -> int:
    return sum((n + 15) & ~15 for _, n, _ in extents)


def tiles_of(rows):
    """The tile list cec_plan_create builds from (off, src_off, len, j) rows."""
    out = []
    for off, so, n, j in rows:
        o = 0
        while o < n:
            step = min(TILE - (off + o) % TILE, n - o)
            out.append((off + o, so + o, step, j))
            o += step
    return out


def mul(c: int, x) -> np.ndarray:
    return dc.MUL[c][np.asarray(x, dtype=np.uint8)]


def region_digests(arena) -> np.ndarray:
    """cec_digest_region of a host arena: (units, 32)."""
    return dc.digests_of(arena, dc.region_tiles(arena.size)).reshape(-1, dc.DIGEST_BYTES)


def apply_to_arena(arena, diffs, rows, coef) -> np.ndarray:
    """arena[off ..] ^= coef[j] * diffs[src_off ..] for every row, in order."""
    out = arena.copy()
    for off, so, n, j in rows:
        out[off:off + n] ^= mul(coef[j], diffs[so:so + n])
    return out


def fold_into_digests(live, diffs, rows, coef) -> np.ndarray:
    """The positioned model: live (units, 32) after the rows' tiles are folded in."""
    out = live.copy()
    for off, so, n, j in tiles_of(rows):
        if coef[j] == 0:
            continue
        unit = np.zeros(TILE, dtype=np.uint8)
        at = off % TILE
        unit[at:at + n] = diffs[so:so + n]
        out[off // TILE] ^= mul(coef[j], dc.digest(unit))
    return out


def identity_row(k: int, lid: int):
    return [int(j == lid) for j in range(k)]
