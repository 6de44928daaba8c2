#!/usr/bin/env python3
"""cec_digest and cec_scrub_digests against cec_scrub on bench.py's metric shape, in one process.

RS(3,2), 65,536 values of 4 KiB, arenas at the odd 4 KiB stride, seeded bytes (the arenas,
seed and event timing of tools/scrub_bench.py).  After 3 warm-ups of each, 20 launches of
each of four ops are timed with HIP events, alternating:
  * cec_scrub over the 5 arenas                (reads 1,342,177,280 bytes)
  * cec_digest of the 5 arenas in one launch   (reads the same bytes, writes 1/128 of them)
  * cec_digest of one arena                    (the distributed case: 268,435,456 bytes)
  * cec_scrub_digests over the 5 digest arrays (reads 10,485,760 bytes)
then one-tile runs of both new ops (their fixed parts), and 20 rounds with one corrupt unit
per 1,024: the digest path must flag and locate exactly what the arena scrub does.
Prints one JSON line; fractions of 8 TB/s are "by events" (event intervals
include the launch gap).  Run tools/hbm_mix beside it for the box's plain read ceilings.

    python tools/digest_bench.py [--stripes 65536] [--iters 20] >> profiles/digest_bench.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 8.0e12


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--stripes", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch

    torch.cuda.set_device(0)
    torch.empty(1, device="cuda")
    from cocytus_amd import ec

    k, m, n, B = 3, 2, 4096, args.stripes
    mat = ec.coding_matrix(k, m)
    g = torch.Generator(device="cuda").manual_seed(0xC0C70007)
    arenas = ec.arena_tensors(k + m, B * n)
    data, parity = arenas[:k], arenas[k:]
    for t in data:
        t.random_(0, 256, generator=g)
    plan = ec.Plan([(s * n, 0, n, 0) for s in range(B)])
    report = ec.Scrub(B)
    stream = torch.cuda.current_stream()
    ec.encode(k, m, mat, data, parity, plan, stream)
    digests = [torch.zeros(B * ec.DIGEST_BYTES, dtype=torch.uint8, device="cuda") for _ in range(k + m)]
    nbytes = (k + m) * B * n

    def scrub():
        report.run(k, m, mat, data, parity, plan, stream)

    def digest5():
        ec.digest(arenas, digests, plan, stream)

    def digest1():
        ec.digest(arenas[:1], digests[:1], plan, stream)

    def check():
        report.run_digests(k, m, mat, digests[:k], digests[k:], plan, stream)

    def timed(fn):
        a, b = ec.Event(), ec.Event()
        a.record(stream)
        fn()
        b.record(stream)
        return a.elapsed_ms(b) * 1e3

    for _ in range(args.warmup):
        scrub()
        digest5()
        digest1()
        check()
    assert report.wait() == 0, "the encode's own parity does not check clean by digests"
    check_rec = ec.last_launch()
    digest5()
    digest_rec = ec.last_launch()
    scrub_us, d5_us, d1_us, chk_us = [], [], [], []
    for _ in range(args.iters):
        scrub_us.append(timed(scrub))
        assert report.wait() == 0
        d5_us.append(timed(digest5))
        d1_us.append(timed(digest1))
        chk_us.append(timed(check))
        assert report.wait() == 0
    # the fixed parts: the same ops over one tile
    with ec.Plan([(0, 0, n, 0)]) as one:
        d_tiny = [timed(lambda: ec.digest(arenas[:1], digests[:1], one, stream)) for _ in range(args.iters)]
        c_tiny = [timed(lambda: report.run_digests(k, m, mat, digests[:k], digests[k:], one, stream))
                  for _ in range(args.iters)]
        assert report.wait() == 0
    # one corrupt unit per 1,024, lids in rotation: both paths must say the same
    hit = list(range(0, B, 1024))
    for i, t in enumerate(hit):
        arenas[i % (k + m)][t * n + 17 * (i % 200)] ^= 0x5A
    torch.cuda.synchronize()
    scrub()
    flagged = report.wait()
    by_arenas = report.findings()
    rare_d5, rare_chk = [], []
    for _ in range(args.iters):
        rare_d5.append(timed(digest5))
        rare_chk.append(timed(check))
    flagged_d = report.wait()
    by_digests = report.findings()
    located = sum(f["lid"] == i % (k + m) for i, f in enumerate(by_digests))
    assert flagged == flagged_d == len(hit) and located == len(hit), (flagged, flagged_d, located, len(hit))
    assert by_digests == by_arenas, "the digest path and the arena scrub disagree"

    def stats(us, nb):
        med = statistics.median(us)
        return {"median_us": round(med, 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
                "gbps_by_events": round(nb / med / 1e3, 1),
                "fraction_of_8TBps_by_events": round(nb / (med * 1e-6) / PEAK, 4)}

    dig_bytes = (k + m) * B * ec.DIGEST_BYTES
    out = {"tool": "digest_bench", "code": [k, m], "stripes": B, "value_bytes": n, "iters": args.iters,
           "waves_shift": int(os.environ.get("CEC_DIGEST_WAVES_SHIFT") or 2),
           "bytes_read": {"scrub": nbytes, "digest_5": nbytes, "digest_1": B * n, "scrub_digests": dig_bytes},
           "scrub_clean": stats(scrub_us, nbytes), "digest_5": stats(d5_us, nbytes),
           "digest_1": stats(d1_us, B * n), "scrub_digests": stats(chk_us, dig_bytes),
           "digest_5_over_scrub_median": round(statistics.median(d5_us) / statistics.median(scrub_us), 4),
           "digest_one_tile_us": {"median": round(statistics.median(d_tiny), 2), "min": round(min(d_tiny), 2)},
           "scrub_digests_one_unit_us": {"median": round(statistics.median(c_tiny), 2), "min": round(min(c_tiny), 2)},
           "digest_5_1_in_1024_corrupt": stats(rare_d5, nbytes),
           "scrub_digests_1_in_1024_corrupt": stats(rare_chk, dig_bytes),
           "flagged": flagged_d, "located": located, "same_findings_as_scrub": True,
           "digest_launch": digest_rec, "check_launch": check_rec, "kernel_code_id": ec.kernel_code_id()}
    report.destroy()
    plan.destroy()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
