#!/usr/bin/env python3
"""The digest-emitting encode and decode beside the unfused sequences they replace.

RS(3,2), all five arenas on one device, 65,536 units of 4 KiB per arena, seeded bytes;
everything compared is taken in one process and the same run, alternating, after warm-ups,
with HIP events.  After every fused op the arrays it kept are compared with cec_digest_region
of the arenas (outside the timing).

  a. basing a group: cec_encode_region_digests (3 arena reads, 2 writes) beside
     cec_encode_region + cec_digest_region over the k data arenas + cec_encode_region over the
     digest arrays (6 reads, 2 writes).  By byte counts the fused form moves 5/8.
  b. rebuilding a lost shard, masks rotating per unit: cec_decode_digests (3 reads, 1 write)
     beside cec_decode + cec_digest of the rebuilt units (4 reads, 1 write): 4/5.

--mode a|b|all selects the parts (a counter pass profiles one at a time).  One JSON line.

    python tools/fused_digest_bench.py [--iters 20] >> profiles/fused_digest_bench.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(us):
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2)}


def ratio(a, b):
    return round(statistics.median(a) / statistics.median(b), 4)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--units", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mode", default="all", choices=["a", "b", "all"])
    args = ap.parse_args()

    import torch

    torch.cuda.set_device(0)
    torch.empty(1, device="cuda")
    from cocytus_amd import ec

    k, m, n, B = 3, 2, 4096, args.units
    mat = ec.coding_matrix(k, m)
    stream = torch.cuda.current_stream()
    g = torch.Generator(device="cuda").manual_seed(0xC0C7000A)
    arenas = ec.arena_tensors(k + m, B * n)
    for a in arenas[:k]:
        a.random_(0, 256, generator=g)
    data, parity = arenas[:k], arenas[k:]

    def digest_arrays(count):
        return [torch.zeros(B * ec.DIGEST_BYTES, dtype=torch.uint8, device="cuda") for _ in range(count)]

    live, fresh = digest_arrays(k + m), digest_arrays(k + m)
    out = {"tool": "fused_digest_bench", "code": [k, m], "units": B, "unit_bytes": n, "iters": args.iters,
           "mode": args.mode, "library": os.path.basename(ec.LIB_PATH), "kernel_code_id": ec.kernel_code_id()}
    checks = 0

    def timed(fn):
        a, b = ec.Event(), ec.Event()
        a.record(stream)
        fn()
        b.record(stream)
        return a.elapsed_ms(b) * 1e3

    def clear(ts):
        for t in ts:
            t.zero_()

    if args.mode in ("a", "all"):
        def fused():
            ec.encode_region_digests(k, m, mat, data, parity, live[:k], live[k:], B * n, stream)

        def unfused():
            ec.encode_region(k, m, mat, data, parity, B * n, stream)
            ec.digest_region(data, live[:k], B * n, stream)
            ec.encode_region(k, m, mat, live[:k], live[k:], B * ec.DIGEST_BYTES, stream)

        def check(what):
            nonlocal checks
            ec.digest_region(arenas, fresh, B * n, stream)
            torch.cuda.synchronize()
            for lid in range(k + m):
                assert torch.equal(live[lid], fresh[lid]), f"{what}: digests of lid {lid} differ from digest_region"
            checks += 1

        for _ in range(args.warmup):
            fused()
            unfused()
        seq = ec.last_launch()["seq"]
        unfused()
        unfused_launches = ec.last_launch()["seq"] - seq
        fused_us, unfused_us = [], []
        for _ in range(args.iters):
            clear(live + parity)
            unfused_us.append(timed(unfused))
            check("a: the unfused sequence")
            clear(live + parity)
            fused_us.append(timed(fused))
            rec = ec.last_launch()
            check("a: cec_encode_region_digests")
        out["a_base_a_group"] = {
            "arena_streams": {"unfused": 2 * k + m, "fused": k + m},
            "unfused": stats(unfused_us), "unfused_launches": unfused_launches, "fused": stats(fused_us),
            "fused_over_unfused_median": ratio(fused_us, unfused_us), "by_byte_counts": round((k + m) / (2 * k + m), 4),
            "launch": rec}

    if args.mode in ("b", "all"):
        ec.encode_region(k, m, mat, data, parity, B * n, stream)
        masks = [ec.recovery_mask(k, m, k + p, [int(i != j) for i in range(k + m)]) for p in range(m) for j in range(k)]
        rebuilt = ec.arena_tensors(k, B * n)
        emitted, ref = digest_arrays(k), digest_arrays(k)
        plan = ec.Plan([(s * n, 0, n, s % len(masks)) for s in range(B)])
        # the units each data lid is rebuilt in: cec_digest of those, tile t of lid j's plan
        units_of = [[s for s in range(B) if not (masks[s % len(masks)] >> j) & 1] for j in range(k)]
        per_lid = [ec.Plan([(s * n, 0, n, 0) for s in units_of[j]]) for j in range(k)]
        unit_idx = [torch.tensor(u, device="cuda") for u in units_of]
        compact = [torch.zeros(len(units_of[j]) * ec.DIGEST_BYTES, dtype=torch.uint8, device="cuda") for j in range(k)]

        def fused():
            ec.decode_digests(k, m, mat, masks, arenas, rebuilt, emitted, B * n, plan, stream)

        def unfused():
            ec.decode(k, m, mat, masks, arenas, rebuilt, plan, stream)
            for j in range(k):
                ec.digest(rebuilt[j:j + 1], compact[j:j + 1], per_lid[j], stream)

        def check(what):
            nonlocal checks
            ec.digest_region(rebuilt, ref, B * n, stream)
            torch.cuda.synchronize()
            for j in range(k):
                lost = torch.tensor([not (masks[s % len(masks)] >> j) & 1 for s in range(len(masks))], device="cuda")
                rows = lost.repeat(B // len(masks) + 1)[:B]
                got, want = emitted[j].view(B, ec.DIGEST_BYTES)[rows], ref[j].view(B, ec.DIGEST_BYTES)[rows]
                assert torch.equal(got, want), f"{what}: emitted digests of lid {j} differ from digest_region"
            for s in (0, 1, B - 1):
                j = [x for x in range(k) if not (masks[s % len(masks)] >> x) & 1][0]
                assert torch.equal(rebuilt[j][s * n:(s + 1) * n], data[j][s * n:(s + 1) * n]), f"{what}: unit {s}"
            checks += 1

        for _ in range(args.warmup):
            fused()
            unfused()
        seq = ec.last_launch()["seq"]
        unfused()
        unfused_launches = ec.last_launch()["seq"] - seq
        fused_us, unfused_us = [], []
        for _ in range(args.iters):
            clear(rebuilt + compact)
            unfused_us.append(timed(unfused))
            ec.digest_region(rebuilt, ref, B * n, stream)
            torch.cuda.synchronize()
            for j in range(k):  # (cec_digest's tile t of lid j's plan is unit units_of[j][t])
                assert torch.equal(compact[j].view(-1, ec.DIGEST_BYTES), ref[j].view(B, ec.DIGEST_BYTES)[unit_idx[j]]), \
                    f"b: cec_digest of lid {j} differs from digest_region"
            clear(rebuilt + emitted)
            fused_us.append(timed(fused))
            rec = ec.last_launch()
            check("b: cec_decode_digests")
        out["b_rebuild_a_shard"] = {
            "arena_streams": {"unfused": k + 2, "fused": k + 1}, "masks": len(masks),
            "unfused": stats(unfused_us), "unfused_launches": unfused_launches, "fused": stats(fused_us),
            "fused_over_unfused_median": ratio(fused_us, unfused_us), "by_byte_counts": round((k + 1) / (k + 2), 4),
            "launch": rec}
        plan.destroy()
        for p_ in per_lid:
            p_.destroy()

    out["digests_equal_digest_region_checks"] = checks
    print(json.dumps(out))


if __name__ == "__main__":
    main()
