#!/usr/bin/env python3
"""cec_digest_set and cec_diff_update_digests on the benchmark's SET shape.

RS(3,2), all five arenas on one device, 65,536 SETs of 4 KiB (256 MiB of staging), seeded
bytes, sources in rotation; everything compared is taken in one process and the same run,
alternating, after warm-ups, with HIP events.  After every op that writes, the live digests
of all five arenas are compared with cec_digest_region of the arenas (outside the timing).

  a. cec_digest_set alone (all five arrays kept) beside cec_digest_region of two arenas in one
     launch: the existing kernel over the same 512 MiB.
  b. cec_diff_update_digests beside cec_diff_update alone, interleaved, fresh staging bytes
     before every op (the plain op is followed by a re-base, untimed).
  c. the new op beside the only alternative the library had: cec_set_diff into a diff buffer
     as large as the batch, one cec_digest_apply_diffs per digest array (three data lids, two
     parities), then cec_diff_update.
  d. the small window: 16 SETs of 4 KiB, with and without digests: events, and the wall clock
     of call + stream synchronize.

--mode a|b|c|d|all selects the parts (a counter pass profiles one at a time).  One JSON line.

    python tools/set_digest_bench.py [--iters 20] >> profiles/set_digest_bench.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(us):
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2)}


def ratio(a, b):
    return round(statistics.median(a) / statistics.median(b), 4)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--stripes", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--small-iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mode", default="all", choices=["a", "b", "c", "d", "all"])
    args = ap.parse_args()
    if args.iters % 2:
        ap.error("--iters must be even (an even number of cec_digest_set calls restores the digests)")

    import torch

    torch.cuda.set_device(0)
    torch.empty(1, device="cuda")
    from cocytus_amd import ec

    k, m, n, B = 3, 2, 4096, args.stripes
    mat = ec.coding_matrix(k, m)
    stream = torch.cuda.current_stream()
    g = torch.Generator(device="cuda").manual_seed(0xC0C70009)
    arenas = ec.arena_tensors(k + m, B * n)
    for a in arenas[:k]:
        a.random_(0, 256, generator=g)
    data, parity = arenas[:k], arenas[k:]
    ec.encode_region(k, m, mat, data, parity, B * n, stream)
    staging = torch.empty(B * n, dtype=torch.uint8, device="cuda")
    staging.random_(0, 256, generator=g)
    live = [torch.zeros(B * ec.DIGEST_BYTES, dtype=torch.uint8, device="cuda") for _ in range(k + m)]
    fresh = [torch.zeros(B * ec.DIGEST_BYTES, dtype=torch.uint8, device="cuda") for _ in range(k + m)]
    scratch2 = [torch.zeros(B * ec.DIGEST_BYTES, dtype=torch.uint8, device="cuda") for _ in range(2)]
    full = ec.Plan([(s * n, s * n, n, s % k) for s in range(B)])
    few = ec.Plan([(((s * 2654435761) % B) * n, s * n, n, s % k) for s in range(16)])
    out = {"tool": "set_digest_bench", "code": [k, m], "stripes": B, "value_bytes": n, "iters": args.iters,
           "mode": args.mode, "library": os.path.basename(ec.LIB_PATH), "kernel_code_id": ec.kernel_code_id()}
    checks = 0

    def rebase():
        ec.digest_region(arenas, live, B * n, stream)

    def check(what):
        nonlocal checks
        ec.digest_region(arenas, fresh, B * n, stream)
        torch.cuda.synchronize()
        for lid in range(k + m):
            assert torch.equal(live[lid], fresh[lid]), f"{what}: live digests of lid {lid} differ from digest_region"
        checks += 1

    def timed(fn):
        a, b = ec.Event(), ec.Event()
        a.record(stream)
        fn()
        b.record(stream)
        return a.elapsed_ms(b) * 1e3

    def new_values():
        staging.random_(0, 256, generator=g)

    def with_digests(plan=full):
        ec.diff_update_digests(k, m, mat, data, staging, parity, True, live[:k], live[k:], B, plan, stream)

    def plain(plan=full):
        ec.diff_update(k, m, mat, data, staging, parity, True, plan, stream)

    rebase()
    check("base")

    if args.mode in ("a", "all"):
        def region2():
            ec.digest_region(arenas[:2], scratch2, B * n, stream)

        def dset():
            ec.digest_set(k, m, mat, data, staging, live[:k], live[k:], B, full, stream)

        for _ in range(args.warmup):
            region2()
            dset()
            dset()
        reg_us, set_us = [], []
        for _ in range(args.iters):  # (an even number of calls: live ends where it began)
            reg_us.append(timed(region2))
            set_us.append(timed(dset))
        rec = ec.last_launch()
        check("a: an even number of cec_digest_set calls")
        out["a_digest_set_alone"] = {
            "bytes_read": 2 * B * n, "atomic_bytes": (1 + m) * B * ec.DIGEST_BYTES,
            "digest_region_2_arenas": stats(reg_us), "digest_set": stats(set_us),
            "set_over_region_median": ratio(set_us, reg_us), "launch": rec}

    if args.mode in ("b", "all"):
        for _ in range(args.warmup):
            new_values()
            with_digests()
            new_values()
            plain()
        rebase()
        check("b: warm-up")
        dig_us, plain_us = [], []
        for _ in range(args.iters):
            new_values()
            plain_us.append(timed(plain))
            rec_plain = ec.last_launch()
            rebase()  # (the plain op went past the digests)
            new_values()
            dig_us.append(timed(with_digests))
            check("b: cec_diff_update_digests")
        md, mp = statistics.median(dig_us), statistics.median(plain_us)
        out["b_set_op"] = {
            "bytes_read_per_tile_units": {"diff_update": 7, "diff_update_digests": 9},
            "diff_update": stats(plain_us), "diff_update_digests": stats(dig_us),
            "digests_over_plain_median": round(md / mp, 4), "added_median_us": round(md - mp, 2),
            "launch_diff_update": rec_plain}

    if args.mode in ("c", "all"):
        diff = torch.empty(B * n, dtype=torch.uint8, device="cuda")

        def alternative():
            ec.set_diff(k, data, staging, diff, full, stream)
            for lid in range(k + m):
                ec.digest_apply_diffs(k, m, mat, lid, diff, live[lid], B, full, stream)
            plain()

        seq = ec.last_launch()["seq"]
        new_values()
        alternative()
        alt_launches = ec.last_launch()["seq"] - seq
        check("c: the alternative")
        for _ in range(args.warmup):
            new_values()
            alternative()
            new_values()
            with_digests()
        alt_us, dig_us = [], []
        for _ in range(args.iters):
            new_values()
            alt_us.append(timed(alternative))
            check("c: set_diff + apply_diffs x 5 + diff_update")
            new_values()
            dig_us.append(timed(with_digests))
            check("c: cec_diff_update_digests")
        out["c_against_existing_ops"] = {
            "alternative": stats(alt_us), "alternative_launches": alt_launches, "scratch_bytes": B * n,
            "diff_update_digests": stats(dig_us), "new_over_alternative_median": ratio(dig_us, alt_us)}
        del diff

    if args.mode in ("d", "all"):
        def wall(fn):
            t0 = time.perf_counter()
            fn()
            ec.stream_synchronize(stream)
            return (time.perf_counter() - t0) * 1e6

        for _ in range(10):
            with_digests(few)
            plain(few)
        ev = {"plain": [], "digests": []}
        wl = {"plain": [], "digests": []}
        for i in range(args.small_iters):
            for key, fn in (("plain", lambda: plain(few)), ("digests", lambda: with_digests(few))):
                if i % 2:
                    ev[key].append(timed(fn))
                else:
                    wl[key].append(wall(fn))
        # (staging is unchanged here, so after the first install every op is a fixed point)
        rebase()
        with_digests(few)
        check("d: the small window")
        out["d_small_window_16"] = {
            "events": {key: stats(v) for key, v in ev.items()},
            "wall_call_plus_sync": {key: stats(v) for key, v in wl.items()},
            "added_median_us_events": round(statistics.median(ev["digests"]) - statistics.median(ev["plain"]), 2),
            "added_median_us_wall": round(statistics.median(wl["digests"]) - statistics.median(wl["plain"]), 2)}

    out["live_equals_digest_region_checks"] = checks
    print(json.dumps(out))


if __name__ == "__main__":
    main()
