"""CPU: the host side of cec_scrub -- the classifier, the condition it rests on, refusals.

The kernel reports one word per flagged tile: bits [0, 8) the parities whose syndrome is
non-zero, bits [8, 24) the data lids ruled out as the single corrupt shard (lid j is ruled
out where ratio[q][j] * S_p0 != S_q in some byte, within one launch of up to four
parities).  `kernel_word` (tests/scrub_case.py) is a numpy model of that word, here over
the oracle's matrix and products; cec_scrub_classify must turn it into the injected lid.
The GPU tests check that the kernels produce these words: tests/test_gpu_scrub.py for
single flips, tests/test_gpu_scrub_words.py word for word on every compiled scrub and
digest-check kernel.  The last three tests here are that file's CPU side: the list of
compiled kernels, the scenarios it injects, and scrub_case.classify, the mirror of
cec_scrub_classify it takes its expected lids from.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import digest_case as dc  # noqa: E402
import scrub_case as sc  # noqa: E402
from scrub_case import GROUP, kernel_word  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = [(3, 2), (4, 2), (6, 3), (10, 4), (5, 1), (12, 8)] + sc.WORD_CODES


@pytest.fixture(scope="module")
def ec():
    from cocytus_amd import ec

    ec.lib()
    return ec


@pytest.fixture(scope="module")
def mul(oracle):
    """256 x 256 product table of the oracle."""
    return np.array([[oracle.gf_mul(a, b) for b in range(256)] for a in range(256)], dtype=np.uint8)


def stripe(oracle, mat, k, m, n=256, seed=5):
    rng = np.random.default_rng(seed + 100 * k + m)
    data = [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(k)]
    return data, oracle.encode(mat, k, m, data)


@pytest.mark.parametrize("k,m", CODES)
def test_classifier_locates_every_single_lid(ec, oracle, mul, k, m):
    """One corrupt lid, one byte or many: the classifier names it (m >= 2) or says
    UNLOCATED (m = 1); the clean stripe's word has no syndrome bit."""
    mat = oracle.big_vandermonde(k + m, k)
    data, parity = stripe(oracle, mat, k, m)
    assert kernel_word(mul, oracle.gf_div, mat, k, m, data, parity) == 0
    rng = np.random.default_rng(k * 31 + m)
    for lid in range(k + m):
        for nbytes in (1, 37):
            d = [x.copy() for x in data]
            p = [x.copy() for x in parity]
            tgt = d[lid] if lid < k else p[lid - k]
            at = rng.choice(len(tgt), nbytes, replace=False)
            tgt[at] ^= rng.integers(1, 256, nbytes, dtype=np.uint8)
            word = kernel_word(mul, oracle.gf_div, mat, k, m, d, p)
            assert word & 0xFF == ((1 << m) - 1 if lid < k else 1 << (lid - k)), (lid, hex(word))
            want = lid if m >= 2 else ec.CEC_SCRUB_UNLOCATED
            assert ec.scrub_classify(word, k, m, mat) == want, (lid, nbytes, hex(word))


@pytest.mark.parametrize("k,m", [c for c in CODES if c[1] >= 2])
def test_classifier_refuses_two_corrupt_lids(ec, oracle, mul, k, m):
    """Two data lids hit at different bytes, and two parities: UNLOCATED."""
    mat = oracle.big_vandermonde(k + m, k)
    data, parity = stripe(oracle, mat, k, m)
    for a in range(k):
        for b in range(a + 1, k):
            d = [x.copy() for x in data]
            d[a][3] ^= 0x5A
            d[b][200] ^= 0x11
            word = kernel_word(mul, oracle.gf_div, mat, k, m, d, parity)
            assert ec.scrub_classify(word, k, m, mat) == ec.CEC_SCRUB_UNLOCATED, (a, b, hex(word))
    for a in range(m):
        for b in range(a + 1, m):
            p = [x.copy() for x in parity]
            p[a][7] ^= 0x80
            p[b][100] ^= 0x01
            word = kernel_word(mul, oracle.gf_div, mat, k, m, data, p)
            assert ec.scrub_classify(word, k, m, mat) == ec.CEC_SCRUB_UNLOCATED, (a, b, hex(word))


def test_classifier_refuses_a_word_without_syndrome(ec, oracle):
    mat = oracle.big_vandermonde(5, 3)
    for word in (0, 0x0700, 0b100):  # nothing; rule-outs only; a parity the code does not have
        with pytest.raises(ec.CecError) as ei:
            ec.scrub_classify(word, 3, 2, mat)
        assert ei.value.code == ec.CEC_EINVAL and "syndrome" in str(ei.value)
    with pytest.raises(ec.CecError) as ei:
        ec.scrub_classify(1, 17, 2, [1] * 19 * 17)
    assert ei.value.code == ec.CEC_EINVAL


@pytest.mark.parametrize("k,m", CODES)
def test_ratio_distinctness(oracle, k, m):
    """The condition the location rests on (the MDS property): within every launch group of
    two or more parities, ratio[q][j] differs between any two data lids, and every parity
    coefficient is non-zero."""
    mat = oracle.big_vandermonde(k + m, k)
    assert all(mat[(k + p) * k + j] != 0 for p in range(m) for j in range(k))
    for p0 in range(0, m, GROUP):
        for q in range(1, min(GROUP, m - p0)):
            ratios = [oracle.gf_div(mat[(k + p0 + q) * k + j], mat[(k + p0) * k + j]) for j in range(k)]
            assert len(set(ratios)) == k, (p0, q, ratios)


CHILD = r"""
import ctypes, sys
sys.path.insert(0, %r)
from cocytus_amd import ec
L = ec.lib()
h = ctypes.c_void_p()
rc = L.cec_scrub_create(ctypes.byref(h), 16)
assert rc == ec.CEC_ENODEV and not h, rc
mat = ec.coding_matrix(3, 2)
rc = L.cec_scrub_region(None, 3, 2, ec._int_array(mat), ec._ptr_array([0x1000] * 3), ec._ptr_array([0x2000] * 2),
                        0, None)
assert rc == ec.CEC_EINVAL, rc   # no report can exist without a device
try:
    ec.Scrub(16)
except ec.CecError as e:
    assert e.code == ec.CEC_ENODEV
    print("ENODEV")
"""


def test_scrub_without_gpu_is_enodev():
    """In a child process with the device hidden: no report, CEC_ENODEV, nothing computed."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ENODEV", r.stdout[-2000:] + r.stderr[-2000:]


def test_bad_arguments_refused_before_the_device(ec):
    """Refusals that need no device: they come back CEC_EINVAL (not CEC_ENODEV) on any
    machine.  (A plan cannot exist without a device: its refusals are in the GPU tests.)"""
    L = ec.lib()
    mat = ec._int_array(ec.coding_matrix(3, 2))
    data, parity = ec._ptr_array([0x1000] * 3), ec._ptr_array([0x2000] * 2)

    def err():
        return L.cec_last_error().decode()

    assert L.cec_scrub_region(None, 3, 2, mat, data, ec._ptr_array([0x2000, 0]), 4096, None) == ec.CEC_EINVAL
    assert "parity[1] is NULL" in err()
    assert L.cec_scrub_region(None, 3, 2, mat, ec._ptr_array([0x1000, 0, 0x1000]), parity, 4096, None) == ec.CEC_EINVAL
    assert "data[1] is NULL" in err()
    for k, m in ((0, 2), (17, 2), (3, 0), (3, 9)):
        big = ec._int_array([1] * 32 * 32)
        assert L.cec_scrub_region(None, k, m, big, data, parity, 4096, None) == ec.CEC_EINVAL
        assert "unsupported code" in err()
    assert L.cec_scrub(None, 3, 2, mat, data, parity, None, None) == ec.CEC_EINVAL
    assert "plan is NULL" in err()
    h = ctypes.c_void_p()
    for n in (0, 0xFFFFFFFF // 256 + 1):
        assert L.cec_scrub_create(ctypes.byref(h), n) == ec.CEC_EINVAL and not h
        assert "max_tiles" in err()
    assert L.cec_scrub_wait(None) == ec.CEC_EINVAL
    assert L.cec_scrub_findings(None, None, 0) == ec.CEC_EINVAL


# ------------------------------------------------------------------ the CPU side of test_gpu_scrub_words.py
def test_instantiation_list():
    """12 + 9 compiled scrub and digest-check kernels; the last launches of WORD_CODES are
    the table the issue of that file states, and between them every capacity rung."""
    compiled = sc.all_instantiations()
    assert len([i for i in compiled if i[0] == sc.KIND_SCRUB]) == 12
    assert len([i for i in compiled if i[0] == sc.KIND_DIGEST_CHECK]) == 9
    assert not set(sc.UNREACHABLE_SCRUB) - compiled
    assert [sc.last_capacity(k, m) for k, m in sc.WORD_CODES] == sc.WORD_LAST
    assert set(sc.WORD_LAST) == {(nt, lt) for nt in (4, 8, 16) for lt in (1, 2, 4)}
    # most rungs both as a first and as a second launch; every n_out under capacity 4
    assert {min(4, m - p0) for k, m in sc.WORD_CODES if k <= 4 for p0 in range(0, m, 4)} == {1, 2, 3, 4}
    assert {(k, m) for k, m in sc.WORD_CODES if k == 16} >= {(16, 2), (16, 8)}  # all 16 rule-out bits, 24 slots
    assert not set(sc.WORD_CODES) & set(sc.EXACT_CODES)
    # the split rule the two plans rely on: fewer / all of the tiles are full line tiles
    m_tiles, f_tiles = sc.tiles_of(sc.WORD_M), sc.tiles_of(sc.WORD_F)
    line = [t for t in m_tiles if t[1] == sc.TILE and t[0] % 128 == 0]
    assert (len(m_tiles), len(line)) == (11 + sc.WORD_N_FULL, sc.WORD_N_FULL) and 4 * len(line) < 3 * len(m_tiles)
    assert all(t == (i * sc.TILE, sc.TILE) for i, t in enumerate(f_tiles)) and len(f_tiles) == sc.WORD_END // sc.TILE


def word_stripe(oracle, k, m):
    mat = oracle.big_vandermonde(k + m, k)
    rng = np.random.default_rng(11 + 100 * k + m)
    host = [rng.integers(0, 256, sc.WORD_SIZE, dtype=np.uint8) for _ in range(k)]
    return mat, host + oracle.encode(mat, k, m, host)


@pytest.mark.parametrize("k,m", sc.WORD_CODES + sc.EXACT_CODES)
def test_scenarios_and_classifier_mirror(ec, oracle, mul, k, m):
    """The scenarios of the GPU word tests through the model: a clean group and the bytes
    outside the ragged tiles give no word; every scenario's tile, and no other, is flagged
    with the verdict its construction demands (scenario 6: the data lid with m = 5,
    UNLOCATED with m >= 6); scrub_case.classify equals cec_scrub_classify on every word
    the scenarios produce, over the arenas and over the digests, on both plans."""
    mat, host = word_stripe(oracle, k, m)
    div = oracle.gf_div
    assert np.array_equal(mul, dc.MUL) and all(sc.table_div(dc.MUL)(a, 29) == div(a, 29) for a in range(256))
    scen, outside = sc.scenarios(k, m)
    m_tiles, f_tiles = sc.tiles_of(sc.WORD_M), sc.tiles_of(sc.WORD_F)
    assert not any(sc.model_words(mul, div, mat, k, m, host, m_tiles))
    for lid, pos, v in outside:
        host[lid][pos] ^= v
    assert not any(sc.model_words(mul, div, mat, k, m, host, m_tiles))
    for s in scen:
        for lid, pos, v in s.hits:
            host[lid][pos] ^= v
    by_off = {s.off: s for s in scen}
    assert len(by_off) == len(scen) == len({(s.off, s.len) for s in scen} & set(m_tiles))
    digest = lambda a, off, n: dc.digest(a[off:off + n])  # noqa: E731
    n_words = 0
    for tiles in (m_tiles, f_tiles):
        words = sc.model_words(mul, div, mat, k, m, host, tiles)
        dwords = sc.model_words(mul, div, mat, k, m, host, tiles, view=digest)
        for (off, n), w, dw in zip(tiles, words, dwords):
            s = by_off.get(off) if (off, n) in m_tiles else None
            if off >= sc.FULL0 or tiles is m_tiles:
                assert bool(w & 0xFF) == (s is not None), (off, hex(w))  # clean tiles in between
            for x in (w, dw):
                if x & 0xFF:
                    assert sc.classify(x, k, m, mat) == ec.scrub_classify(x, k, m, mat), hex(x)
                    n_words += 1
            if s is not None:
                if s.lid is not None:
                    assert sc.classify(w, k, m, mat) == s.lid, (s.name, hex(w))
                if s.two_chunks:
                    assert dw == w, (s.name, hex(w), hex(dw))  # the header's GUARANTEE
                # a located lid is the one that was hit (so the repair test may expect its
                # original bytes back), but for the alias and for scenario 6's lone parity
                got = sc.classify(w, k, m, mat)
                if got != sc.UNLOCATED and not s.name.startswith("alias"):
                    lone = {k + 4} if s.name.startswith("6") and m == 5 else set()
                    assert {h[0] for h in s.hits} - lone == {got}, (s.name, got)
    assert n_words >= 2 * len(scen)
    six = [s for s in scen if s.name.startswith("6")]
    assert len(six) == (m > 4) and all(s.lid == (k - 1 if m == 5 else sc.UNLOCATED) for s in six)


def test_the_two_fixed_cases(oracle, mul):
    """(13,6): errors 5 and 9 in lids 0 and 1 at one byte cancel in parity 3, so five of the
    six syndromes are set and the tile is UNLOCATED.  (7,2): errors 89 in lid 0 and 110 in
    lid 1 at one byte have the syndromes of error 0x37 in lid 2, and are reported as lid 2
    -- the header's "improbably, a wrong lid"; no other pair of values in lids 0 and 1 is
    taken for lid 2."""
    k, m = 13, 6
    mat, host = word_stripe(oracle, k, m)
    (s,) = [s for s in sc.scenarios(k, m)[0] if s.name.startswith("4")]
    assert [(lid, v) for lid, _, v in s.hits] == [(0, 5), (1, 9)]
    assert oracle.gf_mul(mat[(k + 3) * k], 5) == oracle.gf_mul(mat[(k + 3) * k + 1], 9)
    for lid, pos, v in s.hits:
        host[lid][pos] ^= v
    (w,) = sc.model_words(mul, oracle.gf_div, mat, k, m, host, [(s.off, s.len)])
    assert w & 0xFF == 0b110111 and sc.classify(w, k, m, mat) == sc.UNLOCATED, hex(w)

    k, m = 7, 2
    mat, host = word_stripe(oracle, k, m)
    (s,) = [s for s in sc.scenarios(k, m)[0] if s.name.startswith("alias")]
    tile = [(s.off, s.len)]
    third = [h.copy() for h in host]
    third[2][s.hits[0][1]] ^= 0x37
    for lid, pos, v in s.hits:
        host[lid][pos] ^= v
    view = lambda a, off, n: a[off:off + n]  # noqa: E731
    S = [sc.syndromes(mul, mat, k, m, [view(h[j], *tile[0]) for j in range(k)],
                      [view(h[k + p], *tile[0]) for p in range(m)]) for h in (host, third)]
    assert all(np.array_equal(a, b) for a, b in zip(*S)) and all(a.any() for a in S[0])
    (w,) = sc.model_words(mul, oracle.gf_div, mat, k, m, host, tile)
    assert sc.classify(w, k, m, mat) == 2 and s.lid == 2
    c = [[mat[(k + p) * k + j] for j in range(3)] for p in range(m)]
    pairs = [(a, b) for a in range(1, 256) for b in range(1, 256)
             if oracle.gf_mul(oracle.gf_mul(c[0][0], a) ^ oracle.gf_mul(c[0][1], b), c[1][2]) ==
             oracle.gf_mul(oracle.gf_mul(c[1][0], a) ^ oracle.gf_mul(c[1][1], b), c[0][2])]
    assert (89, 110) in pairs
