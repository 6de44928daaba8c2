"""An independent reference for recovery at every loss count.

The recovery ops (cec_residual / cec_solve, cec_decode, the cec_recovery sessions) rebuild
n lost data shards from n participating parities' residuals:

    residual of parity p   R_p = P_p ^ sum_{j surviving} M[p][j] * D_j
                               = sum_{l lost} M[p][l] * D_l
    the lost shards        the solution of the n x n system M[pars][lost] * D_lost = R

The reference here solves that system by Gauss-Jordan elimination on the residuals' byte
columns themselves (no inverse matrix is formed), with the bit-serial product table of
tests/kernel_matrix_case.py: nothing of oracle/, of the library's tables or of its matrix
inversion is read.  tests/test_recovery_case.py ties it down on the CPU; the GPU tests of
tests/test_gpu_recovery_losses.py compare with it bit for bit.
"""
from __future__ import annotations

import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_matrix_case import MUL, gf_inv  # noqa: E402


class SingularError(ValueError):
    """The n x n submatrix M[pars][lost] of a mask has no inverse."""


def lost_of(k: int, mask: int) -> list:
    """The data lids the mask does not name, ascending."""
    return [j for j in range(k) if not (mask >> j) & 1]


def surviving_of(k: int, mask: int) -> list:
    return [j for j in range(k) if (mask >> j) & 1]


def pars_of(k: int, m: int, mask: int) -> list:
    """The participating parity lids of the mask, ascending."""
    return [p for p in range(k, k + m) if (mask >> p) & 1]


def mask_of(k: int, lost, pars) -> int:
    """The recovery mask that loses the data lids `lost` and names the parities `pars`."""
    assert len(lost) == len(pars) and all(0 <= j < k for j in lost) and all(p >= k for p in pars)
    return sum(1 << j for j in range(k) if j not in lost) | sum(1 << p for p in pars)


def encode(mat, k: int, m: int, data) -> list:
    """parity[p] = sum_j M[k + p][j] * data[j] with the bit-serial table."""
    par = []
    for p in range(m):
        acc = np.zeros(len(data[0]), np.uint8)
        for j in range(k):
            acc ^= MUL[int(mat[(k + p) * k + j])][data[j]]
        par.append(acc)
    return par


def residual_of(mat, k: int, lid_self: int, parity_bytes, peers: dict) -> np.ndarray:
    """P ^ sum_j MUL[M[self][j]][D_j] over the peers given ({data lid: bytes})."""
    r = np.array(parity_bytes, np.uint8, copy=True)
    for j, d in peers.items():
        assert 0 <= j < k, j
        r ^= MUL[int(mat[lid_self * k + j])][d]
    return r


def solve_lost(mat, k: int, m: int, mask: int, residuals: dict) -> dict:
    """{lost lid: bytes} from {participating parity lid: residual}: Gauss-Jordan over GF(2^8)
    on the system M[pars][lost] * D_lost = R, the row operations applied to the residuals'
    bytes.  Raises SingularError if the submatrix is singular."""
    lost, pars = lost_of(k, mask), pars_of(k, m, mask)
    n = len(lost)
    if bin(mask).count("1") != k or len(pars) != n or mask >> (k + m):
        raise ValueError(f"mask {mask:#x} is not a recovery mask of RS({k},{m})")
    a = [[int(mat[p * k + l]) for l in lost] for p in pars]
    rows = [np.array(residuals[p], np.uint8, copy=True) for p in pars]
    for col in range(n):
        piv = next((r for r in range(col, n) if a[r][col]), None)
        if piv is None:
            raise SingularError(f"RS({k},{m}) mask {mask:#x}: M[{pars}][{lost}] is singular")
        a[col], a[piv] = a[piv], a[col]
        rows[col], rows[piv] = rows[piv], rows[col]
        inv = gf_inv(a[col][col])
        a[col] = [int(MUL[inv][v]) for v in a[col]]
        rows[col] = MUL[inv][rows[col]]
        for r in range(n):
            f = a[r][col]
            if r == col or not f:
                continue
            a[r] = [v ^ int(MUL[f][w]) for v, w in zip(a[r], a[col])]
            rows[r] = rows[r] ^ MUL[f][rows[col]]
    assert a == [[int(r == c) for c in range(n)] for r in range(n)]
    return {lost[c]: rows[c] for c in range(n)}


def masks_of(k: int, m: int, n: int) -> list:
    """Every mask with n data lids lost and n parities participating, in a fixed order:
    the lost sets in lexicographic order, the parity sets likewise within each."""
    return [mask_of(k, lost, pars) for lost in itertools.combinations(range(k), n)
            for pars in itertools.combinations(range(k, k + m), n)]


def all_masks(k: int, m: int) -> list:
    """masks_of for every loss count 1..min(k, m)."""
    return [mask for n in range(1, min(k, m) + 1) for mask in masks_of(k, m, n)]


def no_data_masks(k: int, m: int) -> list:
    """The C(m, k) masks that name no data lid (k <= m; none otherwise): every data shard
    lost, k parities rebuild them.  The parity sets in lexicographic order, as masks_of(k, m,
    k) lists them."""
    return masks_of(k, m, k) if k <= m else []


def session_sets(k: int, m: int) -> list:
    """loss_sets carried on to n = min(k, m) for the codes with k <= m: for each n the lowest
    n data lids lost with the lowest n parities, and the highest n with the highest n.  At
    n = k both lose every data lid: the no-data masks of the lowest and of the highest k
    parities (one mask if k == m)."""
    assert k <= m, (k, m)
    out = []
    for n in range(1, k + 1):
        for mask in (mask_of(k, range(n), range(k, k + n)),
                     mask_of(k, range(k - n, k), range(k + m - n, k + m))):
            if mask not in out:
                out.append(mask)
    return out


def loss_sets(k: int, m: int) -> list:
    """The deterministic subset the session tests run: for each n in 1..min(m, k - 1) the
    lowest n data lids lost with the lowest n parities, and the highest n with the highest n.
    k - n >= 1 always; wherever k - n >= 2 a session is touched before its last peer."""
    out = []
    for n in range(1, min(m, k - 1) + 1):
        for mask in (mask_of(k, range(n), range(k, k + n)),
                     mask_of(k, range(k - n, k), range(k + m - n, k + m))):
            if mask not in out:
                out.append(mask)
    return out
