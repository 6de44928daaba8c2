"""cec_drainer_apply at its boundaries: the batches, the sequential model and the path predictor.

A plain module (no GPU, nothing of the library): tests/test_drain_case.py asserts on the CPU
that every batch built here sits where it claims, tests/test_gpu_drainer_paths.py runs them.

The model is the drain loop itself, one update after the other in list order:

    parity[addr : addr + len] ^= MUL[MATRIX(lid_self, src_lid)][buf]

with kernel_matrix_case.MUL, the bit-serial GF(2^8) table.  The caller passes the row of the
coding matrix (ec.coding_matrix(k, m)[lid_self * k : lid_self * k + k]); for RS(3,2) the two
parity rows are RS32_ROWS, which the GPU test pins against the library's matrix.

The predictor restates, from the documentation of cocytus_amd/csrc/cec_drain.inc, which of its
paths a batch takes, how the path cuts the batch into rounds, and how many kernel launches
that makes.  Its constants mirror that file (each names where it lives); expected counts are
worked out here and never read from a run.
"""
from __future__ import annotations

import heapq
import os
import sys
from typing import NamedTuple, Optional, Sequence

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_matrix_case import MUL  # noqa: E402

TILE = 4096                  # kTile: tiles are cut at the 4 KiB boundaries of addr (append_tiles, cec_launchplan.hpp)
SMALL_BYTES = 1 << 20        # kDrainSmallBytes (cec_drain.inc): the small window, 16-byte padded diffs
SMALL_TILES = 8192           # kDrainSmallTiles (cec_drain.inc)
ROUND_BYTES = 16 << 20       # kRoundBytes (cec_drain.inc): the pack path's pipelining granularity
TILE_SLACK = 1024            # cec_drainer_create: tile_half = half / 16 + 1024

K, M = 3, 2
RS32_ROWS = {3: [1, 1, 1], 4: [1, 245, 244]}  # MATRIX(lid_self, 0..2) of RS(3,2), lid_self = P0, P1


class Update(NamedTuple):
    addr: int
    length: int
    src_lid: int
    stage: Optional[int]  # offset in the drainer's staging area where the diff lies; None: pageable memory


class Case(NamedTuple):
    name: str
    staging_bytes: int
    arena: int            # bytes of the parity arena
    updates: list
    origin: int = 0       # case H: the first arena byte that is initialised and compared
    seed: str = ""        # seeds the random bytes in place of the name (two cases over one input)


def in_staging(case: Case) -> list:
    return [u.stage is not None for u in case.updates]


# ------------------------------------------------------------------ the model
def diff_bytes(case: Case, seed: int = 0) -> list:
    """The diff of every update: slices of one random block (seeded by the case's name)."""
    rng = np.random.default_rng([seed] + [ord(c) for c in case.seed or case.name])
    blob = rng.integers(0, 256, sum(u.length for u in case.updates) + 1, dtype=np.uint8)
    out, at = [], 0
    for u in case.updates:
        out.append(blob[at:at + u.length])
        at += u.length
    return out


def model(arena0: np.ndarray, updates: Sequence[Update], bufs, row, origin: int = 0) -> np.ndarray:
    """The sequential loop over `updates`; arena0[0] is arena byte `origin`."""
    out = arena0.copy()
    for u, b in zip(updates, bufs):
        if u.length:
            assert len(b) == u.length
            out[u.addr - origin:u.addr - origin + u.length] ^= MUL[int(row[u.src_lid])][b]
    return out


# ------------------------------------------------------------------ the predictor
def pad16(n: int) -> int:
    return (n + 15) & ~15


def half_of(staging_bytes: int) -> int:
    """cec_drainer_create: half = staging_bytes rounded up to 16; the staging area is 2 x half."""
    return pad16(staging_bytes)


def tile_half_of(staging_bytes: int) -> int:
    """cec_drainer_create: tile_half = half / 16 + 1024."""
    return half_of(staging_bytes) // 16 + TILE_SLACK


def tiles_of(addr: int, n: int) -> int:
    """tiles_of (cec_launchplan.hpp): pieces of [addr, addr + n) that end on 4 KiB boundaries of addr."""
    return (addr % TILE + n + TILE - 1) // TILE if n else 0


def waves_of(updates: Sequence[Update]) -> list:
    """overlap_waves (cec_hostplan.hpp): all 0 when no two non-empty updates overlap; else the
    greedy colouring in (addr, index) order -- the lowest wave none of whose members is still
    open; an empty update takes a wave and gives it back at once."""
    n = len(updates)
    by_addr = sorted(range(n), key=lambda i: (updates[i].addr, i))
    end, overlap = 0, False
    for i in by_addr:
        u = updates[i]
        if not u.length:
            continue
        if u.addr < end:
            overlap = True
            break
        end = max(end, u.addr + u.length)
    wave = [0] * n
    if not overlap:
        return wave
    open_, free, nw = [], [], 0
    for i in by_addr:
        u = updates[i]
        while open_ and open_[0][0] <= u.addr:
            free.append(heapq.heappop(open_)[1])
        if free:
            w = min(free)
            free.remove(w)
        else:
            w, nw = nw, nw + 1
        wave[i] = w
        if u.length:
            heapq.heappush(open_, (u.addr + u.length, w))
        else:
            free.append(w)
    return wave


def apply_order(wave: Sequence[int]) -> list:
    """The stable sort of the list order by wave."""
    return sorted(range(len(wave)), key=lambda i: wave[i])


class Prediction(NamedTuple):
    path: str                 # "none" | "in_place" | "small" | "pack" | "mixed"
    rounds: Optional[list]    # update indices of each round, in apply order (None: mixed)
    launches: Optional[int]   # kernel launches of the call (None: mixed, only >= 1 is promised)


def _launches(updates, wave, rounds, digests: bool) -> int:
    """One fold launch per wave that has a tile in the round (drainer_fold), and with digests
    attached one digest launch per round that has a tile."""
    total = 0
    for r in rounds:
        live = {wave[i] for i in r if updates[i].length}
        total += len(live) + (1 if digests and live else 0)
    return total


def predict(updates: Sequence[Update], staging_bytes: int, staged: Sequence[bool], digests: bool = False) -> Prediction:
    """What cec_drainer_apply does with the batch (cec_drain.inc):

    * in place: every non-empty update lies in the staging area -- rounds of at most
      2 * tile_half tiles (a round's first update always fits);
    * else small: at most SMALL_BYTES of 16-byte padded diffs and at most SMALL_TILES tiles --
      one round;
    * else, with a non-empty update in the staging area: mixed (two parts; launches >= 1);
    * else pack: rounds of at most round_cap = min(half, ROUND_BYTES) padded bytes and at
      most tile_half tiles (a round's first update always fits).
    """
    n = len(updates)
    if n == 0:
        return Prediction("none", [], 0)
    half, tile_half = half_of(staging_bytes), tile_half_of(staging_bytes)
    wave = waves_of(updates)
    order = apply_order(wave)
    if all(s for u, s in zip(updates, staged) if u.length):
        cap, rounds = 2 * tile_half, []
        for i in order:
            t = tiles_of(updates[i].addr, updates[i].length)
            if not rounds or (used and used + t > cap):
                rounds.append([])
                used = 0
            rounds[-1].append(i)
            used += t
        return Prediction("in_place", rounds, _launches(updates, wave, rounds, digests))
    nbytes = sum(pad16(u.length) for u in updates)
    ntiles = sum(tiles_of(u.addr, u.length) for u in updates)
    if nbytes <= SMALL_BYTES and ntiles <= SMALL_TILES:
        return Prediction("small", [order], _launches(updates, wave, [order], digests))
    if any(s and u.length for u, s in zip(updates, staged)):
        return Prediction("mixed", None, None)
    round_cap, rounds = min(half, max(ROUND_BYTES, TILE)), []
    for i in order:
        need, t = pad16(updates[i].length), tiles_of(updates[i].addr, updates[i].length)
        if not rounds or (rounds[-1] and (so + need > round_cap or used + t > tile_half)):
            rounds.append([])
            so = used = 0
        rounds[-1].append(i)
        so, used = so + need, used + t
    return Prediction("pack", rounds, _launches(updates, wave, rounds, digests))


def predict_case(case: Case, digests: bool = False) -> Prediction:
    return predict(case.updates, case.staging_bytes, in_staging(case), digests)


def packed_bytes(case: Case) -> int:
    return sum(pad16(u.length) for u in case.updates)


def total_tiles(case: Case) -> int:
    return sum(tiles_of(u.addr, u.length) for u in case.updates)


# ------------------------------------------------------------------ the batches
def case_a(extra: bool) -> Case:
    """256 pageable updates of 4 KiB at distinct units: exactly SMALL_BYTES; `extra`: one
    more of 16 bytes, the first batch that is 16 bytes too large for the small window."""
    ups = [Update(TILE * ((i * 37) % 256), TILE, i % K, None) for i in range(256)]
    if extra:
        ups.append(Update(256 * TILE + 48, 16, 1, None))
    return Case("A+16" if extra else "A", 1 << 20, 258 * TILE, ups)


def straddlers(n: int) -> list:
    """n two-byte updates over the 4 KiB boundaries 1..n: two tiles each."""
    return [Update(TILE * (i + 1) - 1, 2, i % K, None) for i in range(n)]


def case_b(extra: bool) -> Case:
    """4096 straddlers: exactly SMALL_TILES tiles (64 KiB packed); `extra`: a one-byte
    update more, tile 8193."""
    ups = straddlers(4096)
    if extra:
        ups.append(Update(5, 1, 2, None))
    return Case("B+1" if extra else "B", 64 << 10, 4098 * TILE, ups)


def case_c() -> Case:
    """5200 straddlers through 64 KiB halves (tile_half = 5120): 81.25 KiB packed would be two
    rounds by bytes; the tile limit cuts after 2560 updates."""
    return Case("C", 64 << 10, 5202 * TILE, straddlers(5200))


def case_d() -> Case:
    """8192 one-byte updates at consecutive bytes of an 8 KiB staging area (every source but
    each 16th unaligned; the last ends on the area's last byte): 2 * tile_half = 2560 tiles
    per round of the in-place path."""
    ups = [Update(16 * i + i % 3, 1, i % K, i) for i in range(8192)]
    return Case("D", TILE, 16 * 8192 + 3, ups)


def case_e() -> Case:
    """D, but the last 100 updates go to the addresses of the first 100: a second wave, and
    the first wave is cut by three round boundaries."""
    ups = list(case_d().updates)
    for i in range(8092, 8192):
        ups[i] = ups[i]._replace(addr=ups[i - 8092].addr)
    return Case("E", TILE, 16 * 8192 + 3, ups)


F_EXTENTS = [(16, 100), (TILE + 48, 4095), (3 * TILE + 16, 4097)]


def case_f() -> Case:
    """Three ragged updates that lie in the second half of a 2 x 1 MiB staging area only, the
    middle one at an odd offset."""
    half = 1 << 20
    at = [half + 48, half + 2 * TILE + 5, 2 * half - 4097]  # (the last ends on the area's last byte)
    ups = [Update(addr, n, i % K, so) for i, ((addr, n), so) in enumerate(zip(F_EXTENTS, at))]
    return Case("F", half, 8 * TILE, ups)


def _mixed(name: str, n_total: int, pageable: Sequence[int], overlaps: dict) -> Case:
    """n_total updates of 4 KiB at units 0.., those at the `pageable` indices in pageable
    memory and the others at consecutive 4 KiB slots of the staging area from offset 0;
    overlaps: {index: the earlier index whose address it takes}."""
    ups, so = [], 0
    for i in range(n_total):
        addr = TILE * overlaps.get(i, i)
        if i in pageable:
            ups.append(Update(addr, TILE, i % K, None))
        else:
            ups.append(Update(addr, TILE, i % K, so))
            so += TILE
    return Case(name, 1 << 20, (n_total + 1) * TILE, ups)


def case_g1() -> Case:
    """One pageable update first, then 300 in the staging area: above the small window."""
    return _mixed("G1", 301, [0], {})


def case_g2() -> Case:
    """Pageable updates at indices 0, 150 and 299; updates 200..239 (in the staging area) go to
    the addresses of updates 0..39, the first of them onto the pageable update 0: two waves."""
    return _mixed("G2", 301, [0, 150, 299], {i: i - 200 for i in range(200, 240)})


def case_g3() -> Case:
    """One pageable update and 20 in the staging area: within the small window."""
    return _mixed("G3", 21, [0], {})


def case_g5() -> Case:
    """A mixed batch whose part outside the staging area is itself above the small window, and
    holds one diff larger than it: a pageable update of 1 MiB + 5000 bytes at arena byte 3,
    260 pageable ones of 4 KiB, 20 in the staging area; three overlaps, one per kind."""
    big = (1 << 20) + 5000
    first = (3 + big + TILE - 1) // TILE  # the first unit behind the large update
    ups = [Update(3, big, 0, None)]
    ups += [Update(TILE * (first + i), TILE, i % K, None) for i in range(260)]
    ups += [Update(TILE * (first + 260 + i), TILE, i % K, TILE * i + 16) for i in range(20)]
    ups[100] = ups[100]._replace(addr=ups[50].addr)       # pageable onto pageable
    ups[265] = ups[265]._replace(addr=ups[7].addr + 16)   # staged onto two pageable ones
    ups[200] = ups[200]._replace(addr=ups[270].addr)      # pageable onto staged
    return Case("G5", 2 << 20, TILE * (first + 281), ups)


H_MID = 1 << 32
H_WINDOW = 64 << 10
H_GUARD = TILE


def case_h(n: int, staged: bool) -> Case:
    """n ragged updates inside [2^32 - 64 KiB, 2^32 + 64 KiB) of an arena of 2^32 + 1 MiB bytes:
    one straddles 2^32, one is the two bytes around it, one starts on it (three waves); the
    others lie below and above those, disjoint, every third at an odd address."""
    lo, hi = H_MID - H_WINDOW, H_MID + H_WINDOW
    spans = [(H_MID - 1000, 3000), (H_MID - 1, 2), (H_MID, 500)]
    below, above = (n - 3) // 2, n - 3 - (n - 3) // 2
    for start, end, count in ((lo, H_MID - 1000, below), (H_MID + 2000, hi, above)):
        slot = (end - start) // count
        assert slot > 17
        for j in range(count):
            spans.append((start + j * slot + (j * 5 % 17 if j % 3 == 0 else 16), 1 + (j * 977) % (slot - 17)))
    ups, so = [], 0
    for i, (addr, ln) in enumerate(spans):
        ups.append(Update(addr, ln, i % K, so + i % 2 if staged else None))
        so += pad16(ln + 1)
    return Case(f"H{n}{'s' if staged else 'p'}", 1 << 20, H_MID + (1 << 20), ups, origin=lo - H_GUARD)


def case_i_empty(staged: bool) -> Case:
    """Five updates of length 0: buf NULL, or a pointer into the staging area."""
    ups = [Update(TILE * i + 7, 0, i % K, 16 * i if staged else None) for i in range(5)]
    return Case("I0s" if staged else "I0", 1 << 20, 8 * TILE, ups)


def case_i_leading_empty(with_empty: bool) -> Case:
    """Six pageable ragged updates, three of them overlapping in a chain (two waves);
    `with_empty`: an empty one first."""
    ups = [Update(16 + 700 * i + (3 if i == 4 else 0), 900 if i in (1, 2) else 600, i % K, None) for i in range(6)]
    if with_empty:
        ups.insert(0, Update(100, 0, 0, None))
    return Case("I1e" if with_empty else "I1", 1 << 20, 8 * TILE, ups, seed="I1")
