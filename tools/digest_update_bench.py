#!/usr/bin/env python3
"""cec_digest_apply_diffs and the drainer with live digests, on tools/digest_bench.py's shape.

RS(3,2), parity lid 4, 65,536 diffs of 4 KiB (256 MiB), seeded bytes; everything compared is
taken in one process and the same run, alternating, after warm-ups.

  1. kernel, HIP events: cec_digest_apply_diffs over the 65,536 full units beside
     cec_digest_region of one arena of the same size (the same 256 MiB read; the update adds
     2 MiB of atomic bytes), and the contended case, 1,048,576 diffs of 256 B (sixteen per
     unit).  Checked: live == digest_region(arena) once the same diffs are in the arena.
  2. drain, wall clock: cec_drainer_apply of the 65,536 pageable diffs into an HBM arena,
     digests attached against detached, interleaved; live == digest_region(parity) after.
  3. small window, wall clock: 16 diffs of 4 KiB, attached against detached (the fixed cost
     of the extra launch).

--detached-only runs 2 and 3 without digests and nothing else, so that an earlier build
(CEC_LIB_PATH) can be timed in a process of its own on the same box.  One JSON line.

    python tools/digest_update_bench.py [--iters 20] >> profiles/digest_update_bench.jsonl
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--stripes", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--drain-iters", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--detached-only", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch

    torch.cuda.set_device(0)
    torch.empty(1, device="cuda")
    from cocytus_amd import ec

    k, m, lid, n, B = 3, 2, 4, 4096, args.stripes
    mat = ec.coding_matrix(k, m)
    stream = torch.cuda.current_stream()
    g = torch.Generator(device="cuda").manual_seed(0xC0C70008)
    arena = ec.arena_tensors(1, B * n)[0]
    arena.random_(0, 256, generator=g)
    out = {"tool": "digest_update_bench", "code": [k, m], "lid_self": lid, "stripes": B, "value_bytes": n,
           "iters": args.iters, "drain_iters": args.drain_iters, "library": os.path.basename(ec.LIB_PATH),
           "kernel_code_id": ec.kernel_code_id()}

    def fresh_digests():
        d = torch.zeros(B * ec.DIGEST_BYTES, dtype=torch.uint8, device="cuda")
        ec.digest_region([arena], [d], B * n, stream)
        return d

    def timed(fn):
        a, b = ec.Event(), ec.Event()
        a.record(stream)
        fn()
        b.record(stream)
        return a.elapsed_ms(b) * 1e3

    if not args.detached_only:
        diffs = torch.empty(B * n, dtype=torch.uint8, device="cuda")
        diffs.random_(0, 256, generator=g)
        live, scratch = fresh_digests(), fresh_digests()
        full = ec.Plan([(s * n, s * n, n, s % k) for s in range(B)])
        small = ec.Plan(ec.extents_array((s * 256, s * 256, 256, s % k) for s in range(B * 16)))

        def region():
            ec.digest_region([arena], [scratch], B * n, stream)

        def update(plan):
            ec.digest_apply_diffs(k, m, mat, lid, diffs, live, B, plan, stream)

        for _ in range(args.warmup):
            region()
            update(full)
            update(small)
        update(full)
        rec = ec.last_launch()
        update(small)
        rec_small = ec.last_launch()
        reg_us, full_us, small_us = [], [], []
        for _ in range(args.iters):  # (an even number of updates per plan: live ends where it began)
            reg_us.append(timed(region))
            full_us.append(timed(lambda: update(full)))
            small_us.append(timed(lambda: update(small)))
        if (args.warmup + 1 + args.iters) % 2:
            update(full)
            update(small)
        torch.cuda.synchronize()
        assert torch.equal(live, scratch), "an even number of updates did not restore the digests"
        for plan in (full, small):  # the diffs into the arena and into live: live == digest_region(arena)
            ec.apply_diffs(k, m, mat, lid, diffs, arena, plan, stream)
            update(plan)
            region()
            torch.cuda.synchronize()
            assert torch.equal(live, scratch), "live digests differ from digest_region of the updated arena"
        out["kernel"] = {
            "bytes_read": B * n, "atomic_bytes": B * ec.DIGEST_BYTES,
            "digest_region_1": stats(reg_us), "apply_diffs_full_units": stats(full_us),
            "apply_diffs_256B_x16_per_unit": stats(small_us),
            "full_over_region_median": round(statistics.median(full_us) / statistics.median(reg_us), 4),
            "contended_over_region_median": round(statistics.median(small_us) / statistics.median(reg_us), 4),
            "launch_full": rec, "launch_256B": rec_small, "live_equals_digest_region": True}
        full.destroy()
        small.destroy()
        del diffs

    # ---- the drain: pageable diffs, addresses shuffled over the arena
    rng = np.random.default_rng(0xC0C70008)
    host = rng.integers(0, 256, B * n, dtype=np.uint8)
    src = rng.integers(0, k, B)
    addrs = rng.permutation(B).astype(np.uint64) * n
    ups = ec.host_updates([(host[i * n:(i + 1) * n], int(addrs[i]), int(src[i])) for i in range(B)])
    few = ec.host_updates([(host[i * n:(i + 1) * n], int(addrs[i]), int(src[i])) for i in range(16)])
    modes = ["detached"] if args.detached_only else ["detached", "attached"]
    live = None if args.detached_only else fresh_digests()
    torch.cuda.synchronize()
    with ec.Drainer(k, m, mat, lid, staging_bytes=64 << 20) as d:
        def apply(mode, window):
            if live is not None:
                d.set_digests(live if mode == "attached" else None, B)
            t0 = time.perf_counter()
            launches = d.apply(window, arena)
            return (time.perf_counter() - t0) * 1e6, launches

        for window, key, iters in ((ups, "drain_65536", args.drain_iters), (few, "small_window_16", args.iters * 5)):
            for mode in modes:
                for _ in range(2):
                    apply(mode, window)
            us = {mode: [] for mode in modes}
            launches = {}
            for _ in range(iters):
                for mode in modes:
                    t, launches[mode] = apply(mode, window)
                    us[mode].append(t)
            out[key] = {mode: dict(stats(us[mode]), launches=launches[mode]) for mode in modes}
            if "attached" in us:
                md, ma = statistics.median(us["detached"]), statistics.median(us["attached"])
                out[key]["attached_minus_detached_median_us"] = round(ma - md, 2)
                out[key]["attached_over_detached_median"] = round(ma / md, 4)
        if live is not None:
            # detached applies moved the parity but not the digests: re-base, then one attached apply
            d.set_digests(None)
            live = fresh_digests()
            d.set_digests(live, B)
            d.apply(ups, arena)
            want = fresh_digests()
            torch.cuda.synchronize()
            assert torch.equal(live, want), "the drainer's live digests differ from digest_region(parity)"
            out["drain_live_equals_digest_region"] = True
    print(json.dumps(out))


if __name__ == "__main__":
    main()
