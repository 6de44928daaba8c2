"""CPU: the host side of cec_scrub -- the classifier, the condition it rests on, refusals.

The kernel reports one word per flagged tile: bits [0, 8) the parities whose syndrome is
non-zero, bits [8, 24) the data lids ruled out as the single corrupt shard (lid j is ruled
out where ratio[q][j] * S_p0 != S_q in some byte, within one launch of up to four
parities).  `kernel_word` below is a numpy model of that word built from the oracle's
matrix and products; cec_scrub_classify must turn it into the injected lid.  The GPU tests
(tests/test_gpu_scrub.py) check that the kernel produces these words.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = [(3, 2), (4, 2), (6, 3), (10, 4), (5, 1), (12, 8)]
GROUP = 4  # parities per launch


@pytest.fixture(scope="module")
def ec():
    from cocytus_amd import ec

    ec.lib()
    return ec


@pytest.fixture(scope="module")
def mul(oracle):
    """256 x 256 product table of the oracle."""
    return np.array([[oracle.gf_mul(a, b) for b in range(256)] for a in range(256)], dtype=np.uint8)


def syndromes(mul, mat, k, m, data, parity):
    out = []
    for p in range(m):
        s = parity[p].copy()
        for j in range(k):
            s ^= mul[mat[(k + p) * k + j]][data[j]]
        out.append(s)
    return out


def kernel_word(oracle, mul, mat, k, m, data, parity) -> int:
    S = syndromes(mul, mat, k, m, data, parity)
    word = 0
    for p in range(m):
        word |= int(S[p].any()) << p
    for p0 in range(0, m, GROUP):
        lt = min(GROUP, m - p0)
        for j in range(k):
            for q in range(1, lt):
                ratio = oracle.gf_div(mat[(k + p0 + q) * k + j], mat[(k + p0) * k + j])
                if (mul[ratio][S[p0]] != S[p0 + q]).any():
                    word |= 1 << (8 + j)
    return word


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
    assert kernel_word(oracle, mul, mat, k, m, data, parity) == 0
    rng = np.random.default_rng(k * 31 + m)
    for lid in range(k + m):
        for nbytes in (1, 37):
            d = [x.copy() for x in data]
            p = [x.copy() for x in parity]
            tgt = d[lid] if lid < k else p[lid - k]
            at = rng.choice(len(tgt), nbytes, replace=False)
            tgt[at] ^= rng.integers(1, 256, nbytes, dtype=np.uint8)
            word = kernel_word(oracle, mul, mat, k, m, d, p)
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
            word = kernel_word(oracle, mul, mat, k, m, d, parity)
            assert ec.scrub_classify(word, k, m, mat) == ec.CEC_SCRUB_UNLOCATED, (a, b, hex(word))
    for a in range(m):
        for b in range(a + 1, m):
            p = [x.copy() for x in parity]
            p[a][7] ^= 0x80
            p[b][100] ^= 0x01
            word = kernel_word(oracle, mul, mat, k, m, data, p)
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
