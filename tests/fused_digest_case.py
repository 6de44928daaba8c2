"""Shared pieces of tests/test_fused_digest.py and tests/test_gpu_fused_digest.py.

The case generator and the model of the digest-emitting ops (cec_encode_digests,
cec_encode_region_digests, cec_decode_digests): arena bytes from the oracle
(oracle/pyoracle.py: encode, decode), digests from the word model of tests/digest_case.py
(digest, per 4 KiB unit of the arena, the last one zero-padded).  Nothing here calls the
library.
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import digest_case as dc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TILE = dc.TILE
DIGEST_BYTES = dc.DIGEST_BYTES

# Arena lengths: 1, 4 and 5 units (one workgroup of four waves exactly, and one with three idle
# waves), and 9 units whose last is ragged: one chunk, half a unit and a bit, one byte short.
LENGTHS = [TILE, 4 * TILE, 5 * TILE, 8 * TILE + 16, 8 * TILE + 2064, 8 * TILE + 4095]
LENGTH_IDS = ["1u", "4u", "5u", "8u+16", "8u+2064", "8u+4095"]


def n_units(length: int) -> int:
    return (length + TILE - 1) // TILE


def unit_span(u: int, length: int):
    """Bytes [lo, hi) of unit u of an arena of `length` bytes."""
    return u * TILE, min((u + 1) * TILE, length)


def scattered_units(length: int) -> list[int]:
    """A non-contiguous choice of units that keeps the first and the (possibly ragged) last."""
    n = n_units(length)
    return [u for u in range(n) if u not in (1, n - 2)] if n >= 4 else list(range(n))


def unit_extents(units, length: int, pattern=lambda u: 0):
    """One extent (off, src_off, len, pattern) per unit."""
    return [(unit_span(u, length)[0], 0, unit_span(u, length)[1] - unit_span(u, length)[0], pattern(u)) for u in units]


def matrix(k: int, m: int) -> list[int]:
    from oracle import pyoracle

    return pyoracle.big_vandermonde(k + m, k)


@functools.lru_cache(maxsize=None)
def data_arenas(k: int, length: int, seed: int = 0):
    """k data arenas of `length` random bytes.  Cached: read only."""
    from oracle import pyoracle

    return tuple(pyoracle.splitmix_bytes(0xF05ED000 + 64 * seed + j, length) for j in range(k))


def unit_digests(arena: np.ndarray) -> np.ndarray:
    """(units, 32): the digest of every 4 KiB unit of the arena, as cec_digest_region lays them."""
    return dc.digests_of(arena, dc.region_tiles(arena.size)).reshape(-1, DIGEST_BYTES)


@functools.lru_cache(maxsize=None)
def encode_case(k: int, m: int, length: int):
    """(matrix, data, parity, digests of data + parity) of one group.  Cached: read only."""
    from oracle import pyoracle

    mat = matrix(k, m)
    data = data_arenas(k, length, seed=k + m)
    parity = tuple(pyoracle.encode(mat, k, m, list(data)))
    return mat, data, parity, tuple(unit_digests(a) for a in data + parity)


def mask_of(k: int, m: int, lost, pars) -> int:
    """The recovery mask that loses the data lids `lost` and solves with the parities `pars`."""
    assert len(lost) == len(pars)
    mask = 0
    for j in range(k):
        if j not in lost:
            mask |= 1 << j
    for p in pars:
        mask |= 1 << (k + p)
    return mask


def lost_of(k: int, mask: int) -> list[int]:
    return [j for j in range(k) if not (mask >> j) & 1]


def rotating_masks(k: int, m: int, n_lost: int) -> list[int]:
    """k masks: mask q loses data lids q, q + 1, .. (mod k) and takes parities q, q + 1, .. (mod m)."""
    return [mask_of(k, m, sorted((q + i) % k for i in range(n_lost)), sorted((q + i) % m for i in range(n_lost)))
            for q in range(k)]


def decode_unit(mat, k, m, mask, arenas, lo, hi) -> dict:
    """{lost lid: bytes [lo, hi) rebuilt by the oracle} from the slices of the mask's arenas."""
    from oracle import pyoracle

    part = [np.ascontiguousarray(a[lo:hi]) if (mask >> lid) & 1 else None for lid, a in enumerate(arenas)]
    out = pyoracle.decode(mat, k, m, mask, part)
    assert out is not None
    return dict(zip(lost_of(k, mask), out))


def decode_model(mat, k, m, masks, arenas, rows, length):
    """The bytes and unit digests cec_decode_digests leaves: {lid: {unit: (bytes, digest)}} over
    the plan's rows (off, src_off, len, mask index), every row whole units."""
    got: dict = {}
    for off, _, n, q in rows:
        assert off % TILE == 0
        for lo in range(off, off + n, TILE):
            hi = min(lo + TILE, off + n)
            for lid, b in decode_unit(mat, k, m, masks[q], arenas, lo, hi).items():
                got.setdefault(lid, {})[lo // TILE] = (b, dc.digest(b))
    return got
