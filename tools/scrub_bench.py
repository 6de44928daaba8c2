#!/usr/bin/env python3
"""cec_scrub against cec_encode on bench.py's metric shapes, in one process.

RS(3,2), 65,536 values of 4 KiB, arenas at the odd 4 KiB stride, seeded bytes.  After 3
warm-ups of each, 20 launches of cec_encode and 20 of cec_scrub are timed with HIP events,
alternating; then 20 scrub launches over one tile (the op's fixed part: clear, launch,
counter copy-back) and 20 with one corrupt tile per 1,024 (the rare path's cost).
Both ops stream (3 + 2) x 65,536 x 4 KiB = 1,342,177,280 bytes per launch, the encode as 3
reads : 2 writes, the scrub as reads only.  Prints one JSON line; the
fractions of 8 TB/s are "by events" (event intervals include the launch gap).

    python tools/scrub_bench.py [--stripes 65536] [--iters 20] >> profiles/scrub_bench.jsonl
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
    nbytes = (k + m) * B * n

    def encode():
        ec.encode(k, m, mat, data, parity, plan, stream)

    def scrub():
        report.run(k, m, mat, data, parity, plan, stream)

    def timed(fn):
        a, b = ec.Event(), ec.Event()
        a.record(stream)
        fn()
        b.record(stream)
        return a.elapsed_ms(b) * 1e3

    for _ in range(args.warmup):
        encode()
        scrub()
    assert report.wait() == 0, "the encode's own parity does not scrub clean"
    rec = ec.last_launch()
    enc_us, scrub_us = [], []
    for _ in range(args.iters):
        enc_us.append(timed(encode))
        scrub_us.append(timed(scrub))
    assert report.wait() == 0
    # the op's fixed part (clear, launch, counter copy-back): the same op over one tile
    with ec.Plan([(0, 0, n, 0)]) as one:
        tiny_us = [timed(lambda: report.run(k, m, mat, data, parity, one, stream)) for _ in range(args.iters)]
        assert report.wait() == 0
    # the rare path: one corrupt tile per 1,024, lids in rotation
    hit = list(range(0, B, 1024))
    for i, t in enumerate(hit):
        arenas[i % (k + m)][t * n + 17 * (i % 200)] ^= 0x5A
    torch.cuda.synchronize()
    rare_us = [timed(scrub) for _ in range(args.iters)]
    flagged = report.wait()
    located = sum(f["lid"] == i % (k + m) for i, f in enumerate(report.findings()))
    assert flagged == len(hit) and located == len(hit), (flagged, located, len(hit))

    def stats(us):
        med = statistics.median(us)
        return {"median_us": round(med, 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
                "gbps_by_events": round(nbytes / med / 1e3, 1),
                "fraction_of_8TBps_by_events": round(nbytes / (med * 1e-6) / PEAK, 4)}

    out = {"tool": "scrub_bench", "code": [k, m], "stripes": B, "value_bytes": n, "iters": args.iters,
           "bytes_per_launch": {"encode": nbytes, "scrub": nbytes},
           "encode": stats(enc_us), "scrub_clean": stats(scrub_us), "scrub_1_in_1024_corrupt": stats(rare_us),
           "scrub_one_tile_us": {"median": round(statistics.median(tiny_us), 2), "min": round(min(tiny_us), 2)},
           "scrub_over_encode_median": round(statistics.median(scrub_us) / statistics.median(enc_us), 4),
           "flagged": flagged, "located": located, "scrub_launch": rec,
           "kernel_code_id": ec.kernel_code_id()}
    report.destroy()
    plan.destroy()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
