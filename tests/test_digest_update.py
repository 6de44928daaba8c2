"""CPU: the positioned model behind cec_digest_apply_diffs, and the new bindings.

The model (tests/digest_update_case.py) folds c * digest(diff placed at off & 4095) per tile
into the region digests of an arena; that must equal the region digests of the arena after
the diffs were applied to it -- for the GPU file's extents, every row of RS(3,2) a shard can
hold, overlapping extents and a repeated plan.  No GPU, no library arithmetic.
"""
from __future__ import annotations

import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import digest_update_case as uc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("cec_digest_apply_diffs", "cec_drainer_set_digests", "cec_digest_verify_region")


def test_the_extents_are_what_the_gpu_file_says():
    rows = uc.packed(uc.EXTENTS)
    tiles = uc.tiles_of(rows)
    assert len(tiles) == uc.N_TILES
    assert all(off // uc.TILE == (off + n - 1) // uc.TILE for off, _, n, _ in tiles)
    spans = sorted((off, off + n) for off, n, _ in uc.EXTENTS)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))  # disjoint
    assert spans[-1][1] == uc.LEN
    assert all(so % 16 == 0 for _, so, _, _ in rows)
    # every unit is touched by some extent; a single source lid leaves units alone (j = 1: 2, 3, 4)
    assert {off // uc.TILE for off, _, _, _ in tiles} == set(range(uc.N_UNITS))
    assert {off // uc.TILE for off, _, _, j in tiles if j == 1} == {0, 1, 5, 6, 7}


@pytest.mark.parametrize("row", [[1, 245, 244], [1, 1, 1], [0, 1, 0], [1, 0, 0]])
def test_positioned_fold_equals_the_digest_of_the_updated_arena(row):
    rng = np.random.default_rng(17)
    arena = rng.integers(0, 256, uc.LEN, dtype=np.uint8)
    rows = uc.packed(uc.EXTENTS)
    diffs = rng.integers(0, 256, uc.staging_bytes(uc.EXTENTS), dtype=np.uint8)
    live = uc.region_digests(arena)
    after = uc.apply_to_arena(arena, diffs, rows, row)
    folded = uc.fold_into_digests(live, diffs, rows, row)
    assert np.array_equal(folded, uc.region_digests(after))
    touched = {off // uc.TILE for off, _, _, j in uc.tiles_of(rows) if row[j]}
    for u in set(range(uc.N_UNITS)) - touched:
        assert np.array_equal(folded[u], live[u]), u


def test_overlap_and_repeat():
    """Two extents on the same bytes fold twice (XOR commutes); the same plan twice restores."""
    row = [1, 245, 244]
    rng = np.random.default_rng(18)
    arena = rng.integers(0, 256, uc.LEN, dtype=np.uint8)
    rows = uc.packed([(4096 + 48, 300, 1), (4096 + 48, 300, 2), (100, 5000, 0)])
    diffs = rng.integers(0, 256, uc.staging_bytes([(o, n, j) for o, _, n, j in rows]), dtype=np.uint8)
    live = uc.region_digests(arena)
    once = uc.fold_into_digests(live, diffs, rows, row)
    assert np.array_equal(once, uc.region_digests(uc.apply_to_arena(arena, diffs, rows, row)))
    assert np.array_equal(uc.fold_into_digests(once, diffs, rows, row), live)


def test_header_declares_and_library_resolves_the_new_functions():
    from cocytus_amd import build, ec

    build.build(verbose=False)
    src = open(os.path.join(ROOT, "include", "cocytus_ec.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = ec.lib()
    for name in NEW_FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in ec._SIGS and getattr(L, name).restype is ec._i, name
    assert re.search(r"CEC_KERNEL_DIGEST_UPDATE\s*=\s*6\b", src)
    assert ec.CEC_KERNEL_DIGEST_UPDATE == 6
    assert "Out of scope: keeping digests current" not in open(os.path.join(ROOT, "include", "cocytus_ec.h")).read()
