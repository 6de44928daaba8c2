"""CPU: the recovery reference of tests/recovery_case.py, tied down before the GPU is
compared with it (tests/test_gpu_recovery_losses.py).

For every mask: encode with the bit-serial table, form each participating parity's residual
from the surviving shards, and solve -- the lost shards come back bit-exact.  No mask is
skipped: a singular submatrix of the coding matrix fails the test with the mask named.
On the golden RS(3,2) / RS(4,2) masks the reference agrees with the oracle's decode.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import recovery_case as rc  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N = 257  # bytes per shard: every byte value, and one more


def check_mask(mat, k, m, mask, data, parity):
    lost, pars, surv = rc.lost_of(k, mask), rc.pars_of(k, m, mask), rc.surviving_of(k, mask)
    assert len(lost) == len(pars) >= 1 and len(lost) + len(surv) == k
    res = {p: rc.residual_of(mat, k, p, parity[p - k], {j: data[j] for j in surv}) for p in pars}
    # the residual is what the lost shards alone contribute to the parity
    for p in pars:
        assert np.array_equal(res[p], rc.residual_of(mat, k, p, np.zeros(N, np.uint8), {j: data[j] for j in lost}))
    try:
        out = rc.solve_lost(mat, k, m, mask, res)
    except rc.SingularError as e:
        pytest.fail(f"RS({k},{m}) mask {mask:#x} (lost {lost}, parities {pars}): {e}")
    assert sorted(out) == lost
    for j in lost:
        assert np.array_equal(out[j], data[j]), (k, m, hex(mask), j)


def code_case(oracle, k, m):
    mat = oracle.big_vandermonde(k + m, k)
    assert mat is not None and len(mat) == (k + m) * k
    rng = np.random.default_rng(0x5EC0 + 100 * k + m)
    data = [rng.integers(0, 256, N, dtype=np.uint8) for _ in range(k)]
    data[0][:256] = np.arange(256, dtype=np.uint8)
    parity = rc.encode(mat, k, m, data)
    for p, want in enumerate(oracle.encode(mat, k, m, data)):  # the two encodes agree
        assert np.array_equal(parity[p], want), p
    return mat, data, parity


def test_mask_lists():
    """masks_of counts C(k, n) * C(m, n) distinct recovery masks; RS(6,4) has 209 in all."""
    for k, m in ((3, 2), (6, 4), (10, 8)):
        for n in range(1, min(k, m) + 1):
            masks = rc.masks_of(k, m, n)
            assert len(masks) == len(set(masks)) == math.comb(k, n) * math.comb(m, n)
            for mask in masks:
                assert bin(mask).count("1") == k and mask < 1 << (k + m)
                assert len(rc.lost_of(k, mask)) == len(rc.pars_of(k, m, mask)) == n
            assert masks == rc.masks_of(k, m, n)  # a fixed order
    assert len(rc.all_masks(6, 4)) == 209
    assert len(rc.all_masks(3, 2)) == 9


def test_loss_sets():
    """Two masks per loss count 1..min(m, k - 1): the lowest lids and the highest."""
    assert rc.loss_sets(3, 2) == [0b01110, 0b10011, 0b11100, 0b11001]
    for k, m in ((3, 2), (6, 4), (10, 8), (5, 4)):
        sets = rc.loss_sets(k, m)
        top = min(m, k - 1)
        assert len(sets) == len(set(sets)) == 2 * top
        for i, mask in enumerate(sets):
            n = i // 2 + 1
            lost, pars = rc.lost_of(k, mask), rc.pars_of(k, m, mask)
            want = (list(range(n)), list(range(k, k + n))) if i % 2 == 0 else \
                (list(range(k - n, k)), list(range(k + m - n, k + m)))
            assert (lost, pars) == want
            assert k - n >= 1 and mask in rc.masks_of(k, m, n)


def test_no_data_masks_and_session_sets():
    """no_data_masks: the C(m, k) masks of k parities and no data lid, in masks_of's order,
    none where k > m.  session_sets: two masks per loss count up to n = k, the last two (one
    if k == m) no-data masks; below n = k it is loss_sets."""
    for k, m in ((1, 1), (1, 2), (2, 2), (2, 3), (3, 4), (4, 8), (5, 8), (8, 8)):
        nd = rc.no_data_masks(k, m)
        assert len(nd) == len(set(nd)) == math.comb(m, k) and nd == rc.no_data_masks(k, m)
        for mask in nd:
            assert mask & ((1 << k) - 1) == 0 and bin(mask).count("1") == k and mask < 1 << (k + m)
            assert rc.lost_of(k, mask) == list(range(k)) and rc.surviving_of(k, mask) == []
        assert nd == sorted(nd, key=lambda mk: rc.pars_of(k, m, mk))  # lexicographic parity sets
        assert [mk for mk in rc.all_masks(k, m) if not rc.surviving_of(k, mk)] == nd
        sets = rc.session_sets(k, m)
        assert len(sets) == len(set(sets)) == 2 * k - (k == m)
        assert sorted({len(rc.lost_of(k, s)) for s in sets}) == list(range(1, k + 1))
        assert [s for s in sets if len(rc.lost_of(k, s)) < k] == rc.loss_sets(k, m)
        assert [s for s in sets if len(rc.lost_of(k, s)) == k] == ([nd[0]] if k == m else [nd[0], nd[-1]])
    assert rc.no_data_masks(2, 2) == [0b1100] and rc.no_data_masks(8, 8) == [0xFF00]
    assert rc.no_data_masks(1, 2) == [0b010, 0b100]
    assert rc.no_data_masks(3, 2) == [] and rc.no_data_masks(6, 4) == []
    assert len(rc.no_data_masks(4, 8)) == 70 and len(rc.no_data_masks(5, 8)) == 56
    assert rc.session_sets(2, 2) == [0b0110, 0b1001, 0b1100]


EVERY_MASK = {(3, 2): 9, (6, 4): 209, (1, 2): 2, (2, 2): 5, (2, 3): 9, (3, 4): 34, (4, 8): 494}


@pytest.mark.parametrize("k,m", list(EVERY_MASK))
def test_every_mask_solves(oracle, k, m):
    """Every mask of RS(3,2) (9) and RS(6,4) (209), and of the k <= m codes RS(1,2) (2),
    RS(2,2) (5), RS(2,3) (9), RS(3,4) (34) and RS(4,8) (494), whose masks of k losses name no
    data lid: solve_lost returns the data."""
    mat, data, parity = code_case(oracle, k, m)
    masks = rc.all_masks(k, m)
    assert len(masks) == EVERY_MASK[(k, m)]
    if k <= m:
        assert set(rc.no_data_masks(k, m)) <= set(masks) and rc.no_data_masks(k, m)
    for mask in masks:
        check_mask(mat, k, m, mask, data, parity)


def test_loss_sets_and_the_no_data_mask_solve_rs88(oracle):
    """RS(8,8): loss_sets (one to seven lost) and 0xFF00, all eight shards from the eight
    parities alone."""
    k, m = 8, 8
    mat, data, parity = code_case(oracle, k, m)
    sets = rc.loss_sets(k, m) + [0xFF00]
    assert len(sets) == 15 and rc.no_data_masks(k, m) == [0xFF00] and sets == rc.session_sets(k, m)
    for mask in sets:
        check_mask(mat, k, m, mask, data, parity)


def test_loss_sets_solve_rs108(oracle):
    """RS(10,8): one to eight shards lost, the lowest and the highest lids of each count."""
    k, m = 10, 8
    mat, data, parity = code_case(oracle, k, m)
    sets = rc.loss_sets(k, m)
    assert len(sets) == 16 and max(len(rc.lost_of(k, s)) for s in sets) == 8
    for mask in sets:
        check_mask(mat, k, m, mask, data, parity)


@pytest.mark.parametrize("name,k,m", [("decode_rs32.npz", 3, 2), ("decode_rs42.npz", 4, 2)])
def test_agrees_with_oracle_decode_on_golden_masks(oracle, name, k, m):
    """On the committed golden decode masks: residual_of + solve_lost == the oracle's decode
    == the fixture's rebuilt bytes."""
    z = np.load(os.path.join(GOLDEN, name))
    mat = [int(v) for v in z["matrix"]]
    assert mat == oracle.big_vandermonde(k + m, k)
    arenas = [z[f"arena{i}"] for i in range(k + m)]
    assert len(z["masks"])
    for mask in (int(x) for x in z["masks"]):
        lost, pars, surv = rc.lost_of(k, mask), rc.pars_of(k, m, mask), rc.surviving_of(k, mask)
        assert lost, hex(mask)
        ref = oracle.decode(mat, k, m, mask, [a if (mask >> i) & 1 else None for i, a in enumerate(arenas)])
        res = {p: rc.residual_of(mat, k, p, arenas[p], {j: arenas[j] for j in surv}) for p in pars}
        out = rc.solve_lost(mat, k, m, mask, res)
        for x, j in enumerate(lost):
            assert np.array_equal(out[j], ref[x]), (hex(mask), j)
            assert np.array_equal(out[j], z[f"mask{mask}_lost{j}"]), (hex(mask), j)


def test_singular_system_raises():
    """Two equal parity rows: every double loss is singular, and says so; a single loss of
    a column with a zero coefficient likewise."""
    k, m = 3, 2
    mat = [1, 0, 0, 0, 1, 0, 0, 0, 1, 7, 9, 0, 7, 9, 0]
    res = {3: np.zeros(8, np.uint8), 4: np.zeros(8, np.uint8)}
    with pytest.raises(rc.SingularError):
        rc.solve_lost(mat, k, m, rc.mask_of(k, (0, 1), (3, 4)), res)
    with pytest.raises(rc.SingularError):
        rc.solve_lost(mat, k, m, rc.mask_of(k, (2,), (3,)), res)
    out = rc.solve_lost(mat, k, m, rc.mask_of(k, (1,), (4,)), {4: np.full(8, 9, np.uint8)})
    assert np.array_equal(out[1], np.ones(8, np.uint8))
    with pytest.raises(ValueError):
        rc.solve_lost(mat, k, m, 0b00111 | 1 << 3, res)  # four lids named: not a recovery mask
