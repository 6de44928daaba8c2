"""Shared pieces of tests/test_digest_set.py and tests/test_gpu_digest_set.py.

The numpy model of a SET batch over all k + m arenas of a group (it calls neither the library
nor the oracle): for every row (off, src_off, n, j)

    d = staging[src_off : src_off + n] ^ data[j][off : off + n]          (new ^ old)
    parity[p][off : off + n] ^= MATRIX(k + p, j) * d     for every parity p that is not lost
    data[j][off : off + n] = staging[src_off : src_off + n]              if installed

and the digests the SET path must leave: region_digests of each arena after the batch, which
tests/digest_update_case.py's positioned fold reaches from the digests before it with the
diffs d placed at the rows' src_off (identity row for a data lid, the matrix row for a parity).
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import digest_update_case as uc  # noqa: E402


RS32 = [1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 1, 1, 1, 245, 244]  # the RS(3,2) matrix of ec.coding_matrix(3, 2)


def rows_for(k: int, rows=None):
    """uc.EXTENTS packed; for k > 3 row i names source lid i % k."""
    rows = uc.packed(uc.EXTENTS) if rows is None else rows
    return [(off, so, n, i % k if k > 3 else j) for i, (off, so, n, j) in enumerate(rows)]


def row_of(mat, k: int, lid: int):
    return [int(mat[lid * k + j]) for j in range(k)]


def encode(mat, k: int, m: int, data):
    out = []
    for p in range(m):
        par = np.zeros_like(data[0])
        for j in range(k):
            par ^= uc.mul(mat[(k + p) * k + j], data[j])
        out.append(par)
    return out


def random_group(k: int, m: int, mat, rows, seed: int, consistent: bool = False):
    """(data, parity, staging) host arrays of uc.LEN bytes per arena; parity random unless
    `consistent` (the SET path never reads it, and random bytes show a stray write)."""
    rng = np.random.default_rng(0x5E7D16 + seed)
    data = [rng.integers(0, 256, uc.LEN, dtype=np.uint8) for _ in range(k)]
    parity = encode(mat, k, m, data) if consistent else [rng.integers(0, 256, uc.LEN, dtype=np.uint8)
                                                         for _ in range(m)]
    staging = rng.integers(0, 256, max(so + n for _, so, n, _ in rows) + 16, dtype=np.uint8)
    return data, parity, staging


def diffs_of(data, staging, rows) -> np.ndarray:
    """new ^ old of every row at its src_off (zero elsewhere)."""
    d = np.zeros_like(staging)
    for off, so, n, j in rows:
        d[so:so + n] = staging[so:so + n] ^ data[j][off:off + n]
    return d


def set_model(mat, k: int, m: int, data, parity, staging, rows, install: bool, lost=()):
    """(data after, parity after) of the batch; `lost`: parities that are skipped."""
    d_after = [a.copy() for a in data]
    p_after = [a.copy() for a in parity]
    for off, so, n, j in rows:
        new = staging[so:so + n]
        diff = new ^ data[j][off:off + n]
        for p in range(m):
            if p not in lost:
                p_after[p][off:off + n] ^= uc.mul(mat[(k + p) * k + j], diff)
        if install:
            d_after[j][off:off + n] = new
    return d_after, p_after


def digests_after(mat, k: int, m: int, data, parity, staging, rows, install: bool, lost=()):
    """The digests (units, 32) of every arena after the batch, data lids then parities: from
    the model's arenas, cross-checked against the positioned fold of new ^ old."""
    d_after, p_after = set_model(mat, k, m, data, parity, staging, rows, install, lost)
    diffs = diffs_of(data, staging, rows)
    out = []
    for lid, (before, after) in enumerate(zip(data + parity, d_after + p_after)):
        want = uc.region_digests(after)
        if lid < k:
            row = uc.identity_row(k, lid) if install else [0] * k
        else:
            row = [0] * k if lid - k in lost else row_of(mat, k, lid)
        assert np.array_equal(uc.fold_into_digests(uc.region_digests(before), diffs, rows, row), want), lid
        out.append(want)
    return out
