"""Shared pieces of tests/test_digest.py and tests/test_gpu_digest.py.

The numpy model of the unit digest (include/cocytus_ec.h, "THE DIGEST"), written from its
definition with its own bit-serial field arithmetic: it calls neither the library nor the
oracle.  A tile of len = 1..4096 bytes is padded with zeros to 4096 and read as 256 chunks
of 16 bytes; per byte column D0 = XOR_i c_i, D1 = sum_i w_i * c_i with w_i the field element
of byte value i; digest = D0 || D1 (32 bytes).

The arena groups, extents and the one-finding check are tests/scrub_case.py's.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from scrub_case import FULL, FULL_POSITIONS, RAGGED, TILE, Group, expect_one, tiles_of  # noqa: E402,F401

DIGEST_BYTES = 32
CHUNK = 16
CHUNKS = TILE // CHUNK
POLY = 0x11D


def gf_mul_bits(a, b: int):
    """a * b in GF(2^8) mod 0x11D, shift-and-add; a: uint8 array (or scalar), b: 0..255."""
    a = np.asarray(a, dtype=np.uint16)
    out = np.zeros_like(a)
    for bit in range(8):
        if (b >> bit) & 1:
            out ^= a
        a = a << 1
        a = np.where(a & 0x100, a ^ POLY, a).astype(np.uint16)
    return out.astype(np.uint8)


# MUL[w] = the 256-entry product row of weight w
MUL = np.stack([gf_mul_bits(np.arange(256), w) for w in range(256)])


def digest(tile) -> np.ndarray:
    """The 32-byte digest of one tile (uint8 array of 1..4096 bytes)."""
    tile = np.asarray(tile, dtype=np.uint8)
    assert 1 <= tile.size <= TILE
    c = np.zeros(TILE, dtype=np.uint8)
    c[:tile.size] = tile
    c = c.reshape(CHUNKS, CHUNK)
    d0 = np.bitwise_xor.reduce(c, axis=0)
    d1 = np.bitwise_xor.reduce(MUL[np.arange(CHUNKS)[:, None], c], axis=0)
    return np.concatenate([d0, d1])


def digests_of(arena, tiles) -> np.ndarray:
    """The digest array of one arena (host uint8 array) over a tile list [(off, len)]."""
    out = np.empty((len(tiles), DIGEST_BYTES), dtype=np.uint8)
    for t, (off, n) in enumerate(tiles):
        out[t] = digest(arena[off:off + n])
    return out.reshape(-1)


def region_tiles(length: int):
    """The implicit 4 KiB tiling of [0, length)."""
    return [(o, min(TILE, length - o)) for o in range(0, length, TILE)]


GUARD = 64


class DigestBuffers:
    """One digest array per arena with GUARD bytes on both sides, all filled with `fill`."""

    def __init__(self, torch, n_arenas: int, n_tiles: int, fill: int = 0xA5):
        self.torch, self.fill, self.nbytes = torch, fill, n_tiles * DIGEST_BYTES
        self.raw = [torch.full((2 * GUARD + self.nbytes,), fill, dtype=torch.uint8, device="cuda")
                    for _ in range(n_arenas)]
        self.views = [r[GUARD:GUARD + self.nbytes] for r in self.raw]

    def host(self, i: int) -> np.ndarray:
        return self.views[i].cpu().numpy()

    def guards_intact(self) -> bool:
        return all(bool((r[:GUARD] == self.fill).all()) and bool((r[GUARD + self.nbytes:] == self.fill).all())
                   for r in self.raw)
