#!/usr/bin/env python3
"""The idle recoverer's pass at RS(3,2) with D0 and D1 both lost, led by P0 on a recovery pool.

85 single-unit requests over one 1 MiB range.  The passes are timed by the wall clock in one
process and interleaved after warm-ups; replies and residuals are received in place (written
into the pool's stagings before the clock starts), begin / end are outside the clock:

  pooled       85 data replies (add_peers) + 85 residuals of P1 (add_residuals) + one
               flush_solve_host: the double loss solved in the pass's one launch
  per_request  (a) the path the server glue took before the pool led multi-loss requests,
               through the public API: add_peers + flush, 85 x cec_recovery_pool_residual, one
               cec_region_multiply_batch of 4 jobs per request (inv x C over host buffers)
  reference    (b) the reference's one-thread chain through oracle/: per request
               recovery_recover_units (recovery.c:61-96) of D2's reply, then the bottom half's
               inversion and n x n multiplies (memcached.c:7907-7922).  Two forms: one pair of
               calls per request (as the server runs it; each call carries about a microsecond
               of Python binding) and the same bytes as one 85-unit range in one pair of calls
               (no per-request cost at all: the lower bound)
  single_loss  the pass the pool always solved (D0 lost: 170 replies + one flush_solve_host)
  pcie_floor   the bytes the pooled pass moves (replies and residuals up, two planes down)
               over this link's raw pinned copy rates, measured in the same process

Every pass's rebuilt bytes are compared with the data.

--ab PARENT_LIB: the check that the pooled and the single-loss pass kept their time.  Child
processes of this tool with --pool-only (those two passes alone), alternating between this
build and PARENT_LIB (CEC_LIB_PATH), each under its own time limit; reported per pass and
build: the median of the children's medians and their range, the run-to-run spread the
comparison is read against (single_loss_ab, pooled_ab).

One JSON line.

    python tools/pool_losses_bench.py [--iters 30] [--ab path/to/parent/libcocytus_ec.so] \
        >> profiles/pool_losses_bench.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(us):
    q = statistics.quantiles(us, n=4)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "spread_us": round(q[2] - q[0], 2)}


def pcie_raw(torch, nbytes=256 << 20, reps=4):
    """Raw pinned H2D / D2H copy rates of this GPU's link (GB/s), as bench.py takes them."""
    x = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    y = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    y.copy_(x, non_blocking=True)
    torch.cuda.synchronize()
    rates = []
    for a, b in ((y, x), (x, y)):
        t1 = time.perf_counter()
        for _ in range(reps):
            a.copy_(b, non_blocking=True)
        torch.cuda.synchronize()
        rates.append(reps * nbytes / (time.perf_counter() - t1) / 1e9)
    return rates[0], rates[1]


AB_PASSES = ("single_loss", "pooled")


def ab_pool_passes(parent_lib: str, rounds: int, iters: int, limit_s: int) -> dict:
    """Alternating child processes: this build, the parent build, ... each --pool-only."""
    meds = {name: {"this": [], "parent": []} for name in AB_PASSES}
    for _ in range(rounds):
        for which in ("this", "parent"):
            env = dict(os.environ)
            env.pop("CEC_LIB_PATH", None)
            if which == "parent":
                env["CEC_LIB_PATH"] = os.path.abspath(parent_lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--pool-only", "--iters", str(iters)],
                               env=env, capture_output=True, text=True, timeout=limit_s, check=True)
            line = json.loads(r.stdout.strip().splitlines()[-1])
            for name in AB_PASSES:
                meds[name][which].append(line[name]["median_us"])
    res = {}
    for name in AB_PASSES:
        out = {w: {"median_of_medians_us": round(statistics.median(v), 2), "min_us": min(v), "max_us": max(v),
                   "children": v} for w, v in meds[name].items()}
        out["this_minus_parent_us"] = round(out["this"]["median_of_medians_us"] - out["parent"]["median_of_medians_us"], 2)
        out["run_to_run_spread_us"] = round(max(max(v) - min(v) for v in meds[name].values()), 2)
        out["within_spread"] = abs(out["this_minus_parent_us"]) <= out["run_to_run_spread_us"]
        # the merge criterion: this build's median inside the parent's own min-max
        out["this_within_parent_range"] = out["parent"]["min_us"] <= out["this"]["median_of_medians_us"] <= out["parent"]["max_us"]
        res[name + "_ab"] = out
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--single-only", action="store_true")
    ap.add_argument("--pool-only", action="store_true", help="the pooled and the single-loss pass alone")
    ap.add_argument("--ab", metavar="PARENT_LIB")
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--ab-limit", type=int, default=120, help="seconds per child process")
    args = ap.parse_args()

    import numpy as np
    import torch

    torch.cuda.set_device(0)
    torch.empty(1, device="cuda")
    from cocytus_amd import ec

    k, m, U, NREQ, UNITS = 3, 2, 4096, 85, 256
    P0, P1 = k, k + 1
    mat = ec.coding_matrix(k, m)
    rng = np.random.default_rng(0xC0C7D0)
    data = rng.integers(0, 256, (k, UNITS * U), dtype=np.uint8)
    dd = [torch.from_numpy(d).cuda() for d in data]
    pd = [torch.empty(UNITS * U, dtype=torch.uint8, device="cuda") for _ in range(m)]
    ec.encode_region(k, m, mat, dd, pd, UNITS * U)
    torch.cuda.synchronize()
    parity = [p.cpu().numpy() for p in pd]
    double, single = 0b11100, 0b01110  # {D2, P0, P1}; {D1, D2, P0}
    # P1's residual over the range with D2 in (what P1 ships to the leader)
    mul = np.zeros((256, 256), np.uint8)
    for c in {int(v) for v in mat}:
        mul[c] = [ec.lib().galois_single_multiply(c, v, 8) for v in range(256)]
    res1 = parity[1] ^ mul[int(mat[P1 * k + 2])][data[2]]
    rc_inv, inv = ec.jerasure_invert_matrix([int(mat[P0 * k]), int(mat[P0 * k + 1]),
                                             int(mat[P1 * k]), int(mat[P1 * k + 1])], 2, 8)
    assert rc_inv == 0
    out = {"tool": "pool_losses_bench", "code": [k, m], "requests": NREQ, "iters": args.iters,
           "library": ec.LIB_PATH if os.environ.get("CEC_LIB_PATH") else os.path.basename(ec.LIB_PATH),
           "kernel_code_id": ec.kernel_code_id()}
    cself = np.zeros((NREQ, U), np.uint8)
    own = np.zeros((NREQ, 2, U), np.uint8)
    SPOT = (0, 41, NREQ - 1)

    with ec.RecoveryPool(k, m, mat, P0, pd[0], capacity_units=128) as pool:
        def begin(mask, peers, with_residual):
            rids = [pool.begin(mask, u, u) for u in range(NREQ)]
            ids, lids, ptrs = [], [], []
            for u, rid in enumerate(rids):
                for j in peers:
                    addr, view = pool.staging(rid, j)
                    view[:] = data[j, u * U:(u + 1) * U]
                    ids.append(rid), lids.append(j), ptrs.append(addr)
            replies = ec.pool_replies(ids, lids, ptrs)
            residuals = None
            if with_residual:
                ptrs = []
                for u, rid in enumerate(rids):
                    addr, view = pool.parity_staging(rid, P1)
                    view[:] = res1[u * U:(u + 1) * U]
                    ptrs.append(addr)
                residuals = ec.pool_replies(rids, [P1] * NREQ, ptrs)
            return rids, replies, residuals

        def end(rids):
            for rid in rids:
                pool.end(rid)

        def pooled():
            rids, replies, residuals = begin(double, [2], True)
            t0 = time.perf_counter()
            pool.add_peers(replies)
            pool.add_residuals(residuals)
            solved = pool.flush_solve_host()
            t = (time.perf_counter() - t0) * 1e6
            assert solved == NREQ
            for u in SPOT:
                for x in (0, 1):
                    assert np.array_equal(pool.output(rids[u], x), data[x, u * U:(u + 1) * U]), (u, x)
            end(rids)
            return t

        def per_request():
            rids, replies, _ = begin(double, [2], False)
            b_res, b_c, b_o = res1.ctypes.data, cself.ctypes.data, own.ctypes.data
            t0 = time.perf_counter()
            pool.add_peers(replies)
            pool.flush()
            jobs = []
            for u, rid in enumerate(rids):
                pool.residual(rid, cself[u])
                for x in (0, 1):
                    dst = b_o + (u * 2 + x) * U
                    jobs.append((b_c + u * U, dst, None, U, inv[x * 2], 0))
                    jobs.append((b_res + u * U, dst, None, U, inv[x * 2 + 1], 1))
            ec.region_multiply_batch(jobs)
            t = (time.perf_counter() - t0) * 1e6
            for u in SPOT:
                for x in (0, 1):
                    assert np.array_equal(own[u, x], data[x, u * U:(u + 1) * U]), (u, x)
            end(rids)
            return t

        def single_loss():
            rids, replies, _ = begin(single, [1, 2], False)
            t0 = time.perf_counter()
            pool.add_peers(replies)
            solved = pool.flush_solve_host()
            t = (time.perf_counter() - t0) * 1e6
            assert solved == NREQ
            for u in SPOT:
                assert np.array_equal(pool.output(rids[u]), data[0, u * U:(u + 1) * U]), u
            end(rids)
            return t

        pool_only = args.single_only or args.pool_only
        passes = {"pooled": pooled, "single_loss": single_loss} if args.pool_only else {"single_loss": single_loss}
        if not pool_only:
            from oracle import pyoracle

            p0u = [parity[0][u * U:(u + 1) * U].copy() for u in range(NREQ)]
            d2u = [data[2][u * U:(u + 1) * U].copy() for u in range(NREQ)]
            r1u = [res1[u * U:(u + 1) * U].copy() for u in range(NREQ)]
            unit_res = [np.empty(U, np.uint8) for _ in range(NREQ)]
            p0r, d2r, r1r = (np.ascontiguousarray(a[:NREQ * U]) for a in (parity[0], data[2], res1))
            range_res = np.empty(NREQ * U, np.uint8)

            def reference_per_request():
                t0 = time.perf_counter()
                outs = []
                for u in range(NREQ):
                    pyoracle.recover_units(mat, k, P0, 2, p0u[u], d2u[u], unit_res[u], [0])
                    outs.append(pyoracle.bottom_half(mat, k, m, double, [unit_res[u], r1u[u]]))
                t = (time.perf_counter() - t0) * 1e6
                for u in SPOT:
                    for x in (0, 1):
                        assert np.array_equal(outs[u][x], data[x, u * U:(u + 1) * U]), (u, x)
                return t

            def reference_one_range():
                t0 = time.perf_counter()
                pyoracle.recover_units(mat, k, P0, 2, p0r, d2r, range_res, [0])
                outs = pyoracle.bottom_half(mat, k, m, double, [range_res, r1r])
                t = (time.perf_counter() - t0) * 1e6
                for x in (0, 1):
                    assert np.array_equal(outs[x], data[x, :NREQ * U]), x
                return t

            passes = {"pooled": pooled, "per_request": per_request, "reference_per_request": reference_per_request,
                      "reference_one_range": reference_one_range, "single_loss": single_loss}
        for _ in range(args.warmup):
            for fn in passes.values():
                fn()
        us = {name: [] for name in passes}
        for _ in range(args.iters):
            for name, fn in passes.items():
                us[name].append(fn())
        for name in passes:
            out[name] = stats(us[name])
        if not pool_only:
            med = {name: out[name]["median_us"] for name in passes}
            out["per_request_over_pooled_median"] = round(med["per_request"] / med["pooled"], 2)
            out["reference_per_request_over_pooled_median"] = round(med["reference_per_request"] / med["pooled"], 2)
            out["reference_one_range_over_pooled_median"] = round(med["reference_one_range"] / med["pooled"], 2)
            out["pooled_over_single_loss_median"] = round(med["pooled"] / med["single_loss"], 2)
    if not (args.single_only or args.pool_only):
        h2d, d2h = pcie_raw(torch)
        up, down = 2 * NREQ * U, 2 * NREQ * U  # replies + residuals read in place; two planes written
        floor = max(up / (h2d * 1e9), down / (d2h * 1e9)) * 1e6
        out["pcie_floor"] = {"h2d_bytes": up, "d2h_bytes": down, "GBps_raw": {"h2d": round(h2d, 1), "d2h": round(d2h, 1)},
                             "floor_us": round(floor, 2), "floor_over_pooled": round(floor / out["pooled"]["median_us"], 3)}
    if args.ab:
        out.update(ab_pool_passes(args.ab, args.ab_rounds, args.iters, args.ab_limit))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
