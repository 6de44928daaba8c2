"""Shared pieces of tests/test_scrub.py, tests/test_gpu_scrub.py and
tests/test_gpu_scrub_words.py (the word model, its classifier, the codes, scenarios and
kernel list of the word tests: second half of this file), and the child-process case of
tests/test_gpu_scrub.py.

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


# ------------------------------------------------------------------ the word model
# The report word of one tile, from its definition in include/cocytus_ec.h: bits [0, 8) the
# parities whose syndrome is non-zero, bits [8, 24) the data lids ruled out as the single
# corrupt shard (lid j where ratio[q][j] * S_p0 != S_q in some byte, within one launch of up
# to four parities).  `mul` is a 256 x 256 product table, `div` a division function: the
# oracle's in tests/test_scrub.py, the bit-serial table of tests/digest_case.py on the GPU.
GROUP = 4  # parities per launch
UNLOCATED = -1


def table_div(mul):
    """a / b from a product table alone."""
    inv = [0] + [int(np.nonzero(mul[b] == 1)[0][0]) for b in range(1, 256)]
    return lambda a, b: int(mul[a][inv[b]])


def syndromes(mul, mat, k, m, data, parity):
    out = []
    for p in range(m):
        s = parity[p].copy()
        for j in range(k):
            s ^= mul[mat[(k + p) * k + j]][data[j]]
        out.append(s)
    return out


def kernel_word(mul, div, mat, k, m, data, parity) -> int:
    S = syndromes(mul, mat, k, m, data, parity)
    word = 0
    for p in range(m):
        word |= int(S[p].any()) << p
    for p0 in range(0, m, GROUP):
        lt = min(GROUP, m - p0)
        for j in range(k):
            for q in range(1, lt):
                ratio = div(mat[(k + p0 + q) * k + j], mat[(k + p0) * k + j])
                if (mul[ratio][S[p0]] != S[p0 + q]).any():
                    word |= 1 << (8 + j)
    return word


def classify(word: int, k: int, m: int, mat) -> int:
    """cec_scrub_classify's rule as the header states it: exactly one syndrome bit p (m >= 2)
    is parity lid k + p; the syndrome bits of every parity whose coefficient for j is
    non-zero, with j the only data lid not ruled out, is j; anything else is UNLOCATED."""
    syn, ruled = word & 0xFF, (word >> 8) & 0xFFFF
    assert syn and not syn >> m, hex(word)
    if m < 2:
        return UNLOCATED
    if syn & (syn - 1) == 0:
        return k + syn.bit_length() - 1
    left = [j for j in range(k) if not (ruled >> j) & 1]
    if len(left) != 1:
        return UNLOCATED
    reached = sum(int(mat[(k + p) * k + left[0]] != 0) << p for p in range(m))
    return left[0] if syn == reached else UNLOCATED


# ------------------------------------------------------------------ every kernel, every word
# The codes of tests/test_gpu_scrub_words.py and the kernel their LAST launch runs (one
# launch per four parities; nt / lt of ec.last_launch()).  Together the last launches are
# all nine capacity rungs of scrub_kernel and of digest_check_kernel, most of them both as
# a first group (syn_shift 0) and as a second one (syn_shift 4), with every n_out from 1 to
# 4 under capacity 4 (m = 3 and m = 7).
WORD_CODES = [(2, 2), (3, 1), (3, 3), (4, 5), (3, 6), (4, 7), (7, 2), (8, 5), (5, 6), (6, 7), (9, 1), (16, 2),
              (16, 5), (13, 6), (11, 7), (16, 8)]
WORD_LAST = [(4, 2), (4, 1), (4, 4), (4, 1), (4, 2), (4, 4), (8, 2), (8, 1), (8, 2), (8, 4), (16, 1), (16, 2),
             (16, 1), (16, 2), (16, 4), (16, 4)]
EXACT_CODES = [(3, 2), (4, 2), (6, 3)]  # scrub_kernel<k, m, exact>; the digest check has none
KIND_SCRUB, KIND_DIGEST_CHECK = 3, 5    # cec_launch_record::kind


def last_capacity(k: int, m: int) -> tuple:
    """(nt, lt) of the capacity kernel the last launch of a run over RS(k, m) takes."""
    lt = m - GROUP * ((m - 1) // GROUP)
    return (4 if k <= 4 else 8 if k <= 8 else 16), (1 if lt <= 1 else 2 if lt <= 2 else 4)


def all_instantiations() -> set:
    """What launch_scrub and launch_digest_check compile, as (kind, nt, lt, exact): 12 + 9.
    The launch record does not say whether a 4 x 2 scrub ran the exact kernel or the
    capacity one: `exact` is launch_scrub's rule (the launch holds every parity of one of
    EXACT_CODES), which scrub_inst applies to the code that was run."""
    s = {(KIND_SCRUB, k, m, True) for k, m in EXACT_CODES}
    for kind in (KIND_SCRUB, KIND_DIGEST_CHECK):
        s |= {(kind, nt, lt, False) for nt in (4, 8, 16) for lt in (1, 2, 4)}
    return s


UNREACHABLE_SCRUB = {}  # (kind, nt, lt, exact) -> why no public call lands on it: none so far


def scrub_inst(rec: dict, k: int, m: int) -> tuple:
    return (rec["kind"], rec["nt"], rec["lt"], rec["kind"] == KIND_SCRUB and (k, m) in EXACT_CODES)


# One arena group per code carries every scenario at once, each on a tile of its own, and one
# scrub run per plan checks them all: WORD_M is RAGGED's 11 tiles and then 32 full
# line-aligned tiles (fewer than three quarters of the tiles are full: split shift 0, four
# waves in one workgroup), WORD_F the whole of [0, WORD_END) as 36 full tiles (split shift
# 2: four one-wave workgroups per tile, so "counted once" goes through device atomics
# between workgroups; its first four tiles hold all the ragged tiles' corruption together).
WORD_N_FULL = 32
WORD_END = FULL0 + WORD_N_FULL * TILE
WORD_SIZE = WORD_END + 64
WORD_M = RAGGED + [(FULL0 + i * TILE, TILE) for i in range(WORD_N_FULL)]
WORD_F = [(0, WORD_END)]
SPREAD = (0, 15, 16, 1023, 1024, 2048, 4095)  # every wave or part, both edges of a wave


class Scenario:
    """Corruption of one tile of WORD_M: `hits` are (lid, arena position, XOR value), all
    inside the tile [off, off + len).  `lid`: the verdict the scenario's own construction
    demands (None: the model alone decides).  The digest check must report such a tile
    exactly as cec_scrub does when its hits lie within two 16-byte chunks (`two_chunks`,
    the header's GUARANTEE)."""

    def __init__(self, name, off, n, hits, lid=None):
        self.name, self.off, self.len, self.hits, self.lid = name, off, n, hits, lid
        assert all(off <= pos < off + n and 1 <= v <= 255 for _, pos, v in hits), name
        self.two_chunks = len({(pos - off) // 16 for _, pos, _ in hits}) <= 2


def scenarios(k: int, m: int, alias: bool = True):
    """(scenarios, outside) of RS(k, m): one scenario per second full tile of WORD_M (a clean
    tile between any two) and one per ragged tile; `outside` are hits on the bytes right
    before and right after every ragged tile that belong to no tile of WORD_M, in a data
    and a parity lid: they must change nothing.  Values are non-zero, from a seeded
    generator, but for the two fixed cases."""
    rng = np.random.default_rng(7000 + 100 * k + m)
    located = (lambda lid: lid) if m >= 2 else (lambda lid: UNLOCATED)
    out = []

    def val():
        return int(rng.integers(1, 256))

    def full(name, hits, lid=None):
        off = FULL0 + 2 * sum(s.len == TILE and s.off >= FULL0 for s in out) * TILE
        assert off + TILE <= WORD_END, name
        out.append(Scenario(name, off, TILE, [(l, off + b, v) for l, b, v in hits], lid))

    # 1. one data lid, spread over the tile
    for j in (range(k) if k <= 4 else sorted({0, 7, 8, 15, k - 1} & set(range(k)))):
        full(f"1: data lid {j}", [(j, b, val()) for b in SPREAD], located(j))
    # 2. one parity lid, spread: the first, the last of the first launch, the first of the
    #    second launch (a tile flagged by the second launch only), the last
    for p in sorted({0, min(m, GROUP) - 1, m - 1} | ({GROUP} if m > GROUP else set())):
        full(f"2: parity {p}", [(k + p, b, val()) for b in SPREAD], located(k + p))
    # 3. two data lids at different bytes, in different waves
    full("3: two data lids, two waves", [(0, 5, val()), (k - 1, 3000, val())])
    # 4. two data lids at the same byte (at (13,6) these two values cancel in parity 3)
    full("4: two data lids, one byte", [(0, 1500, 5), (1, 1500, 9)])
    # 5. a data lid and a parity of the first launch, at different bytes
    full("5: data lid and a first-launch parity", [(1, 100, val()), (k + min(1, m - 1), 2100, val())])
    if m > GROUP:
        # 6. a data lid and the first parity of the second launch: with m = 5 that parity is
        #    alone in its launch and rules out nothing, so the verdict is the data lid
        full("6: data lid and a second-launch parity", [(k - 1, 700, val()), (k + GROUP, 3500, val())],
             k - 1 if m == GROUP + 1 else UNLOCATED)
        # 7. one parity of each launch
        full("7: a parity of each launch", [(k, 40, val()), (k + m - 1, 4000, val())], UNLOCATED)
    # 9. about 300 random bytes in one data lid
    at = np.sort(rng.choice(TILE, 300, replace=False))
    full("9: 300 bytes of one data lid", [(k // 2, int(b), val()) for b in at], located(k // 2))
    if alias and (k, m) == (7, 2):
        # the header's "improbably, a wrong lid", pinned: errors 89 in lid 0 and 110 in lid 1
        # at one byte have exactly the syndromes of error 0x37 in lid 2 (the only such pair)
        full("alias: two data lids that look like a third", [(0, 2222, 89), (1, 2222, 110)], 2)
    # 8. every ragged tile: its last valid byte, the lids in rotation
    tiles = tiles_of(RAGGED)
    edge = [0, k, k - 1, k + m - 1, k // 2, k + m // 2]
    for t, (off, n) in enumerate(tiles):
        lid = edge[t % len(edge)]
        out.append(Scenario(f"8: ragged tile {t}", off, n, [(lid, off + n - 1, val())], located(lid)))
    every = tiles_of(WORD_M)
    outside = [(lid, pos, val()) for t, (off, n) in enumerate(tiles) for pos in (off - 1, off + n)
               if not any(o <= pos < o + length for o, length in every) for lid in (t % k, k + t % m)]
    assert outside and all(0 <= pos < FULL0 for _, pos, _ in outside)
    hit = [h[:2] for s in out for h in s.hits] + [h[:2] for h in outside]
    assert len(set(hit)) == len(hit)  # no byte is hit twice
    return out, outside


def model_words(mul, div, mat, k, m, host, tiles, view=lambda a, off, n: a[off:off + n]):
    """The model's word of every tile, from the host copies of the k + m arenas (`view`
    picks what the kernel reads of one arena for one tile)."""
    return [kernel_word(mul, div, mat, k, m, [view(host[j], off, n) for j in range(k)],
                        [view(host[k + p], off, n) for p in range(m)]) for off, n in tiles]


def expected_findings(words, tiles, k, m, mat):
    """cec_scrub_findings' list for the model's words: the flagged tiles, ascending."""
    return [{"tile": t, "off": off, "len": n, "syndromes": w & 0xFF, "ruled_out": (w >> 8) & 0xFFFF,
             "lid": classify(w, k, m, mat)} for t, ((off, n), w) in enumerate(zip(tiles, words)) if w & 0xFF]


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
