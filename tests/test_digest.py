"""CPU: the unit digest's definition (the numpy model of tests/digest_case.py) against the
oracle, its guarantee and its documented limit, and the host-side refusals of cec_digest /
cec_scrub_digests.

The model is written from the header's definition with its own shift-and-add field
arithmetic.  The GPU tests (tests/test_gpu_digest.py) check that the kernel produces the
model's bytes; here the model itself is pinned: it commutes with the oracle's encode, it is
linear, it sees every one- and two-chunk corruption, and it misses the (1, 2, 3) * v pattern
the header names as its limit.
"""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import digest_case as dc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = [(3, 2), (4, 2), (6, 3), (10, 4), (5, 1), (12, 8)]
LENGTHS = [1, 15, 16, 17, 4095, 4096]


@pytest.fixture(scope="module")
def ec():
    from cocytus_amd import ec

    ec.lib()
    return ec


def test_model_field_is_the_oracles(oracle):
    """The model's own multiplication table equals the oracle's on a sample of rows."""
    for a in (0, 1, 2, 3, 0x1D, 0x40, 0x80, 0xFF):
        assert [int(x) for x in dc.MUL[a]] == [oracle.gf_mul(a, b) for b in range(256)]


@pytest.mark.parametrize("k,m", CODES)
def test_digest_commutes_with_encode(oracle, k, m):
    """digest(parity_p) = sum_j MATRIX(k+p, j) * digest(data_j): the digests of the oracle's
    parity equal the oracle's encode of the data digests, for every tile length."""
    mat = oracle.big_vandermonde(k + m, k)
    rng = np.random.default_rng(100 * k + m)
    for n in LENGTHS:
        data = [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(k)]
        parity = oracle.encode(mat, k, m, data)
        want = oracle.encode(mat, k, m, [dc.digest(d) for d in data])
        for p in range(m):
            assert np.array_equal(dc.digest(parity[p]), want[p]), (n, p)


def test_digest_is_linear():
    """digest(a ^ b) = digest(a) ^ digest(b), digest(c * a) = c * digest(a); a short tile
    digests as the same bytes padded with zeros."""
    rng = np.random.default_rng(7)
    for n in LENGTHS:
        a = rng.integers(0, 256, n, dtype=np.uint8)
        b = rng.integers(0, 256, n, dtype=np.uint8)
        assert np.array_equal(dc.digest(a ^ b), dc.digest(a) ^ dc.digest(b))
        for c in (0, 1, 2, 0x53, 0xFF):
            assert np.array_equal(dc.digest(dc.MUL[c][a]), dc.MUL[c][dc.digest(a)]), (n, c)
        padded = np.zeros(dc.TILE, dtype=np.uint8)
        padded[:n] = a
        assert np.array_equal(dc.digest(a), dc.digest(padded))


def test_every_single_byte_change_changes_the_digest():
    """All 4096 positions, one value: by linearity the change of the digest is the digest
    of the error alone, and it is never zero."""
    for pos in range(dc.TILE):
        e = np.zeros(dc.TILE, dtype=np.uint8)
        e[pos] = 0x5A
        d = dc.digest(e)
        assert d.any(), pos
        # D0 carries the value in the byte's column, D1 the value times the chunk's weight
        assert d[pos % 16] == 0x5A and d[16 + pos % 16] == dc.MUL[pos // 16][0x5A]


def test_every_pair_of_chunks_with_equal_error_is_caught():
    """Equal errors in two chunks of one column cancel in D0; the distinct weights keep D1
    non-zero.  (0, 255) is the pair weights 2^i would miss."""
    rng = np.random.default_rng(11)
    pairs = [(0, 255), (1, 254), (63, 64), (0, 64)]
    while len(pairs) < 504:
        i, j = (int(x) for x in rng.integers(0, dc.CHUNKS, 2))
        if i != j:
            pairs.append((i, j))
    for i, j in pairs:
        col, v = int(rng.integers(0, 16)), int(rng.integers(1, 256))
        e = np.zeros(dc.TILE, dtype=np.uint8)
        e[16 * i + col] = e[16 * j + col] = v
        d = dc.digest(e)
        assert not d[:16].any() and d[16 + col] == dc.MUL[i ^ j][v] != 0, (i, j)


def test_two_chunks_with_any_errors_are_caught():
    """Distance 3 per column: two chunks with unrelated non-zero errors change the digest."""
    rng = np.random.default_rng(12)
    for _ in range(300):
        i, j = (int(x) for x in rng.choice(dc.CHUNKS, 2, replace=False))
        e = np.zeros(dc.TILE, dtype=np.uint8)
        e[16 * i:16 * i + 16] = rng.integers(0, 256, 16, dtype=np.uint8)
        e[16 * j:16 * j + 16] = rng.integers(0, 256, 16, dtype=np.uint8)
        if e.any():
            assert dc.digest(e).any(), (i, j)


def test_the_documented_limit():
    """Errors (1, 2, 3) * v in chunks 1, 2, 3 of one column are in the null space: 1 ^ 2 ^ 3
    = 0 and 1*1 ^ 2*2 ^ 3*3 = 1 ^ 4 ^ 5 = 0."""
    for v in (1, 0x37, 0xFF):
        for col in (0, 9, 15):
            e = np.zeros(dc.TILE, dtype=np.uint8)
            for i in (1, 2, 3):
                e[16 * i + col] = dc.MUL[i][v]
            assert e.any() and not dc.digest(e).any()


def test_constants(ec):
    assert ec.DIGEST_BYTES == 32 == dc.DIGEST_BYTES
    assert (ec.CEC_KERNEL_DIGEST, ec.CEC_KERNEL_DIGEST_CHECK) == (4, 5)


def test_bad_arguments_refused_before_the_device(ec):
    """Refusals that need no device come back CEC_EINVAL (not CEC_ENODEV) with a message on
    any machine."""
    L = ec.lib()
    mat = ec._int_array(ec.coding_matrix(3, 2))

    def err():
        return L.cec_last_error().decode()

    one = ec._ptr_array([0x1000])
    assert L.cec_digest_region(1, None, one, 4096, None) == ec.CEC_EINVAL and "NULL" in err()
    assert L.cec_digest_region(1, one, None, 4096, None) == ec.CEC_EINVAL and "NULL" in err()
    for n in (0, 25, -1):
        many = ec._ptr_array([0x1000] * 25)
        assert L.cec_digest_region(n, many, many, 4096, None) == ec.CEC_EINVAL
        assert "outside [1, 24]" in err()
    assert L.cec_digest_region(2, ec._ptr_array([0x1000, 0]), ec._ptr_array([0x2000] * 2), 4096, None) == ec.CEC_EINVAL
    assert "arenas[1] is NULL" in err()
    assert L.cec_digest_region(2, ec._ptr_array([0x1000] * 2), ec._ptr_array([0x2000, 0]), 4096, None) == ec.CEC_EINVAL
    assert "digests[1] is NULL" in err()
    assert L.cec_digest_region(1, one, ec._ptr_array([0x2008]), 4096, None) == ec.CEC_EINVAL
    assert "16-byte aligned" in err()
    assert L.cec_digest(1, one, one, None, None) == ec.CEC_EINVAL and "plan is NULL" in err()

    data, parity = ec._ptr_array([0x1000] * 3), ec._ptr_array([0x2000] * 2)
    assert L.cec_scrub_digests_region(None, 3, 2, mat, None, parity, 4096, None) == ec.CEC_EINVAL
    assert "NULL digest array" in err()
    assert L.cec_scrub_digests_region(None, 3, 2, mat, data, None, 4096, None) == ec.CEC_EINVAL
    assert L.cec_scrub_digests_region(None, 3, 2, mat, data, ec._ptr_array([0x2000, 0]), 4096, None) == ec.CEC_EINVAL
    assert "parity digests[1] is NULL" in err()
    assert L.cec_scrub_digests_region(None, 3, 2, mat, ec._ptr_array([0x1000, 0, 0x1000]), parity, 4096,
                                      None) == ec.CEC_EINVAL
    assert "data digests[1] is NULL" in err()
    for k, m in ((0, 2), (17, 2), (3, 0), (3, 9)):
        big = ec._int_array([1] * 32 * 32)
        assert L.cec_scrub_digests_region(None, k, m, big, data, parity, 4096, None) == ec.CEC_EINVAL
        assert "unsupported code" in err()
    assert L.cec_scrub_digests(None, 3, 2, mat, data, parity, None, None) == ec.CEC_EINVAL
    assert "plan is NULL" in err()


CHILD = r"""
import sys
sys.path.insert(0, %r)
from cocytus_amd import ec
L = ec.lib()
mat = ec._int_array(ec.coding_matrix(3, 2))
one = ec._ptr_array([0x1000])
assert L.cec_digest_region(0, one, one, 4096, None) == ec.CEC_EINVAL     # arguments first
rc = L.cec_digest_region(1, one, ec._ptr_array([0x2000]), 4096, None)
assert rc == ec.CEC_ENODEV, rc
assert L.cec_digest_region(1, one, ec._ptr_array([0x2000]), 0, None) == ec.CEC_ENODEV
data, parity = ec._ptr_array([0x1000] * 3), ec._ptr_array([0x2000] * 2)
rc = L.cec_scrub_digests_region(None, 3, 2, mat, data, parity, 4096, None)
assert rc == ec.CEC_ENODEV, rc      # (no report can exist without a device)
try:
    ec.digest_region([0x1000], [0x2000], 4096)
except ec.CecError as e:
    assert e.code == ec.CEC_ENODEV
    print("ENODEV")
"""


def test_digest_without_gpu_is_enodev():
    """In a child process with the device hidden: good arguments are CEC_ENODEV, nothing is
    computed (there is no CPU fallback)."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ENODEV", r.stdout[-2000:] + r.stderr[-2000:]
