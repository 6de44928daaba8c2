"""One launch under a write-through tail, against the oracle, in a child process.

The body of tests/test_gpu_store_tail.py.  The library reads CEC_WT_MAX_BYTES,
CEC_WT_TAIL_BYTES, CEC_STORE_POLICY and CEC_SPLIT_SHIFT once per process, so every case
runs as

    python tests/store_tail_case.py [--engine lds] CASE EXPECT [CASE EXPECT ...]

under the environment the test pins, and prints "OK".  CASE names the op and its plan (see
CASES); EXPECT is what the launch record must say of the last launch:

    nt          no write-through bit, no tail bit, wt_from = CEC_NO_WT_TAIL
    wt          the write-through bit, no tail bit, wt_from = CEC_NO_WT_TAIL
    tail:<g>    the tail bit and wt_from = g, no write-through bit
    tail:-<n>   the same, g = (work items of the launch) - n

Every arena is a row of one slab with the sentinel 0xA5 wherever no input lies; after the
op the WHOLE slab is compared byte for byte with what oracle/pyoracle.py computes, so every
output byte is checked and every byte around every extent must be unchanged.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import pyoracle  # noqa: E402

SENT = 0xA5
TILE = 4096
NARROW, EXACT, GENERIC = 0, 1, 2
PERM, LDS = 0, 1
WRITE_THROUGH, WT_TAIL = 2, 4
NO_TAIL = 2**64 - 1


def full_tiles(n):
    """n full tiles on 4 KiB offsets, a guard tile before and after."""
    return [((i + 1) * TILE, TILE) for i in range(n)], (n + 2) * TILE


def ragged():
    """1, 15, 17, 4095, 4096 and 4098 bytes at offsets that are no multiple of 16."""
    ext, o = [], 4099
    for n in (1, 15, 17, 4095, 4096, 4098):
        ext.append((o, n))
        o += n + 4096 + 21  # (keeps every offset odd or 5 mod 16; a guard gap after each)
    assert all(e[0] % 16 for e in ext)
    return ext, (o + 127) // 128 * 128


def slab_of(rng, n_rows, arena, random_rows):
    host = np.full((n_rows, arena), SENT, np.uint8)
    for r in random_rows:
        host[r] = rng.integers(0, 256, arena, dtype=np.uint8)
    return host


def run_encode(ec, rng, dev, k, m, ext, arena):
    mat = ec.coding_matrix(k, m)
    host = slab_of(rng, k + m, arena, range(k))
    exp = host.copy()
    par = pyoracle.encode(mat, k, m, [host[j].copy() for j in range(k)])
    for o, n in ext:
        for p in range(m):
            exp[k + p, o:o + n] = par[p][o:o + n]
    slab = dev(host)
    with ec.Plan([(o, 0, n, 0) for o, n in ext]) as plan:
        ec.encode(k, m, mat, [slab[j] for j in range(k)], [slab[k + p] for p in range(m)], plan)
        rec = ec.last_launch()
    return slab, exp, rec


def run_decode(ec, rng, dev, ext, arena):
    """The rotating single-shard decode: 6 masks, extent e rebuilt under mask e % 6."""
    k, m = 3, 2
    mat = ec.coding_matrix(k, m)
    host = slab_of(rng, k + m + k, arena, range(k))
    par = pyoracle.encode(mat, k, m, [host[j].copy() for j in range(k)])
    for p in range(m):
        host[k + p] = par[p]
    masks = [ec.recovery_mask(k, m, k + p, [int(i != j) for i in range(k + m)]) for p in range(m) for j in range(k)]
    assert masks == [pyoracle.recovery_mask(k, m, k + p, [int(i != j) for i in range(k + m)])
                     for p in range(m) for j in range(k)]
    exp = host.copy()
    for e, (o, n) in enumerate(ext):
        mk = masks[e % len(masks)]
        (lost,) = [j for j in range(k) if not (mk >> j) & 1]
        (got,) = pyoracle.decode(mat, k, m, mk, [host[i, o:o + n].copy() for i in range(k + m)])
        assert np.array_equal(got, host[lost, o:o + n])
        exp[k + m + lost, o:o + n] = got
    slab = dev(host)
    with ec.Plan([(o, 0, n, e % len(masks)) for e, (o, n) in enumerate(ext)]) as plan:
        ec.decode(k, m, mat, masks, [slab[i] for i in range(k + m)], [slab[k + m + j] for j in range(k)], plan)
        rec = ec.last_launch()
    return slab, exp, rec


def run_diff_update(ec, rng, dev, ext, arena):
    """cec_diff_update with install: parities read-modify-write, the data shard overwritten."""
    k, m = 3, 2
    mat = ec.coding_matrix(k, m)
    host = slab_of(rng, k + m + 1, arena, range(k + m + 1))
    exp = host.copy()
    for e, (o, n) in enumerate(ext):
        j = e % k
        new = host[k + m, o:o + n].copy()
        pv = [host[k + p, o:o + n].copy() for p in range(m)]
        pyoracle.diff_update(mat, k, m, j, host[j, o:o + n].copy(), new, pv, True)
        for p in range(m):
            exp[k + p, o:o + n] = pv[p]
        exp[j, o:o + n] = new
    slab = dev(host)
    with ec.Plan([(o, o, n, e % k) for e, (o, n) in enumerate(ext)]) as plan:
        ec.diff_update(k, m, mat, [slab[j] for j in range(k)], slab[k + m], [slab[k + p] for p in range(m)], True, plan)
        rec = ec.last_launch()
    return slab, exp, rec


def run_region_multiply(ec, rng, dev, nbytes):
    host = slab_of(rng, 2, nbytes + 2 * TILE, [0])
    exp = host.copy()
    dst = exp[1, TILE:TILE + nbytes].copy()
    pyoracle.region_multiply(host[0, TILE:TILE + nbytes].copy(), 0x53, dst, 0)
    exp[1, TILE:TILE + nbytes] = dst
    slab = dev(host)
    ec.region_multiply(slab[0][TILE:], 0x53, nbytes, slab[1][TILE:], 0)
    return slab, exp, ec.last_launch()


# name -> (kind, nt, lt, runner)
CASES = {
    "encode9": (EXACT, 3, 2, lambda ec, rng, dev: run_encode(ec, rng, dev, 3, 2, *full_tiles(9))),
    "ragged": (EXACT, 3, 2, lambda ec, rng, dev: run_encode(ec, rng, dev, 3, 2, *ragged())),
    "decode13": (EXACT, 3, 1, lambda ec, rng, dev: run_decode(ec, rng, dev, *full_tiles(13))),
    "diff9": (EXACT, 2, 3, lambda ec, rng, dev: run_diff_update(ec, rng, dev, *full_tiles(9))),
    "rs53": (EXACT, 5, 3, lambda ec, rng, dev: run_encode(ec, rng, dev, 5, 3, *full_tiles(9))),
    "rs92": (GENERIC, 16, 2, lambda ec, rng, dev: run_encode(ec, rng, dev, 9, 2, *full_tiles(9))),
    "narrow": (NARROW, 1, 1, lambda ec, rng, dev: run_region_multiply(ec, rng, dev, 3 * TILE)),
}


def check(torch, ec, dev, lds, name, expect):
    kind, nt, lt, run = CASES[name]
    seq0 = ec.last_launch()["seq"]
    slab, exp, rec = run(ec, np.random.default_rng(0xC0C7), dev)
    torch.cuda.synchronize()
    print("record", rec, flush=True)
    assert rec["seq"] == seq0 + 1, rec
    assert (rec["kind"], rec["nt"], rec["lt"]) == (kind, nt, lt), rec
    assert rec["engine"] == (LDS if lds else PERM), rec
    assert rec["grid"] == rec["n_tiles"] << rec["split_shift"], rec
    forced = os.environ.get("CEC_SPLIT_SHIFT")
    if forced is not None:
        assert rec["split_shift"] == int(forced), rec
    bits = rec["flags"] & (WRITE_THROUGH | WT_TAIL)
    if expect.startswith("tail:"):
        g = int(expect[5:])
        if g < 0:
            g += rec["grid"]
        assert bits == WT_TAIL and rec["wt_from"] == g and 0 < g < rec["grid"], (expect, g, rec)
    else:
        assert bits == {"nt": 0, "wt": WRITE_THROUGH}[expect] and rec["wt_from"] == NO_TAIL, (expect, rec)
    got = slab.cpu().numpy()
    if not np.array_equal(got, exp):
        r, p = np.argwhere(got != exp)[0]
        raise AssertionError(f"{name}: row {r} byte {p}: got {got[r, p]:#x} want {exp[r, p]:#x} "
                             f"({int((got != exp).sum())} wrong)")


def main(argv):
    import torch

    torch.cuda.set_device(0)
    torch.empty(1, device="cuda")
    from cocytus_amd import ec

    lds = argv[:2] == ["--engine", "lds"]
    pairs = argv[2:] if lds else argv
    assert pairs and len(pairs) % 2 == 0, argv
    ec.set_engine(LDS if lds else PERM)

    def dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        assert t.data_ptr() % 128 == 0 and a.shape[1] % 128 == 0
        return t

    for name, expect in zip(pairs[::2], pairs[1::2]):
        check(torch, ec, dev, lds, name, expect)
    print("OK")


if __name__ == "__main__":
    main(sys.argv[1:])
