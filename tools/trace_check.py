#!/usr/bin/env python3
"""Check a bench line's roofline against rocprofv3's kernel trace of the SAME run.

    python tools/trace_check.py <rocprof -d dir> <bench line .jsonl> [out.json]

The bench command (`python bench.py`, plain or `--full`) is run under
`rocprofv3 --kernel-trace --stats`.  The line's `roofline.launch_ms` / `decode_roofline.
launch_ms` are the average HIP-event times of its timed whole-batch encode / decode
launches; here the same launches are picked out of the trace -- for each op, the first
(warmup + steps) dispatches of its kernel (encode: combine_kernel<K, M, engine>, the
rotating single-shard decode: combine_kernel<K, 1, engine>, the engine the line says
ran) with the whole batch's grid (256 work-items per 4 KiB tile), in start order (the
metric's workload runs first; later whole-batch dispatches of that kernel belong to other
workloads), the last `steps` of them timed -- and their average duration is compared with
the line's.  The trace may be gzip'd (run_kernel_trace.csv.gz).

Per op it also prints, over the same timed dispatches, `duration_us` (median and range) and
`gap_before_next_us`: the start of the next dispatch in the trace minus this dispatch's
end, i.e. what the launch boundary behind this kernel costs.  Only gaps to another
whole-batch dispatch of the metric's workload count (the last timed decode is followed by
the host's synchronize and the verification, not by a dependent launch), so an op may have
one gap fewer than durations.  `duration_plus_gap_us` is their sum per dispatch.
Under `--full` the strong-scaling shares appear as `shares[<tiles>]` with the same three
figures, and each op gets `fixed_us`: twice the half batch's median minus the whole
batch's, the per-launch cost that does not scale with the bytes streamed.
"""
from __future__ import annotations

import csv
import glob
import gzip
import json
import os
import statistics
import sys


def main(prof_dir, line_path, out_path=None):
    line = json.loads([ln for ln in open(line_path) if ln.startswith("{")][-1])
    traces = glob.glob(os.path.join(prof_dir, "**", "run_kernel_trace.csv*"), recursive=True)
    stats = glob.glob(os.path.join(prof_dir, "**", "run_kernel_stats.csv"), recursive=True)
    assert traces, f"no run_kernel_trace.csv under {prof_dir}"
    opener = gzip.open if traces[0].endswith(".gz") else open
    with opener(traces[0], "rt") as f:
        rows = list(csv.DictReader(f))
    # the warmups the bench actually ran (it runs at least one even under --warmup 0)
    steps, warm = line["steps"], line.get("warmup_run", max(1, line["warmup"]))
    k, m = line["config"]["k"], line["config"]["m"]
    tiles = line["config"]["stripes_per_gpu"] * line["config"]["value_bytes"] // 4096
    whole = tiles * 256  # one 4 KiB tile = 256 lanes (in 1, 2 or 4 workgroups): the whole batch
    ran = line["config"]["engine"]  # "... (ran: encode PERM, decode PERM, ..."

    def engine_of(op):
        return "LdsEngine" if f"{op} LDS" in ran else "PermEngine"

    def grid(r):
        return int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)

    # encode: combine_kernel<K, M, ...>; decode (one lost shard): combine_kernel<K, 1, ...>
    def spread(v):
        return {"n": len(v), "median": round(statistics.median(v), 3), "min": round(min(v), 3),
                "max": round(max(v), 3)} if v else {"n": 0}

    # every dispatch in start order: the successor of a dispatch, whatever kernel it is
    order = sorted(rows, key=lambda r: int(r["Start_Timestamp"]))
    succ = {id(r): order[i + 1] for i, r in enumerate(order[:-1])}
    batches = {}

    out = {"command": f"python bench.py{' --full' if line.get('full') else ''} under rocprofv3 --kernel-trace --stats",
           "whole_batch_grid_work_items": whole, "tiles": tiles, "line_value": line["value"],
           "line_kernel_code_id": line["roofline"].get("kernel_code_id"),
           "stats_csv": os.path.relpath(stats[0], prof_dir) if stats else None}
    for op, outs, rl in (("encode", m, line["roofline"]), ("decode", 1, line["decode_roofline"])):
        eng = engine_of(op)
        sig = f"combine_kernel<{k}, {outs}, cec::{eng}"
        disp = sorted((r for r in rows if sig in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
        # the metric's workload runs first: its warm + steps whole-batch dispatches; later
        # ones of the same kernel and grid belong to other workloads
        batch = [r for r in disp if grid(r) == whole][: warm + steps]
        timed = batch[warm:]
        batches[op] = batch
        durs = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in timed]
        avg = sum(durs) / len(durs)
        ev = rl["launch_ms"]
        nbytes = rl["algorithmic_bytes_per_launch"]
        out[op] = {
            "kernel": timed[0]["Kernel_Name"], "dispatches_timed": len(durs), "warmup_dispatches_skipped": warm,
            "trace_avg_ms": round(avg, 5), "trace_median_ms": round(statistics.median(durs), 5),
            "line_event_avg_ms": ev, "event_over_trace": round(ev / avg, 4),
            "trace_frac_of_8TBps": round(nbytes / (avg * 1e-3) / 8e12, 4), "line_frac": rl["frac"],
        }
    # launch boundaries: gaps between consecutive whole-batch dispatches of the workload
    def boundaries(batches, into):
        mine = {id(r) for b in batches.values() for r in b}
        for op, batch in batches.items():
            timed = batch[warm:]
            durs = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in timed]
            pairs = [(d, (int(succ[id(r)]["Start_Timestamp"]) - int(r["End_Timestamp"])) / 1e3)
                     for r, d in zip(timed, durs) if id(r) in succ and id(succ[id(r)]) in mine]
            into.setdefault(op, {}).update(duration_us=spread(durs), gap_before_next_us=spread([g for _, g in pairs]),
                                           duration_plus_gap_us=spread([d + g for d, g in pairs]))

    boundaries(batches, out)
    # --full: the strong-scaling shares (1/2, 1/4, 1/8 of the batch, same kernels, same
    # warmup and steps) give the same figures at smaller sizes, and with the half batch the
    # part of duration + gap that does not scale with the bytes:
    # fixed_us = 2 * median(half) - median(whole).
    for div in (2, 4, 8):
        part = {}
        for op, outs in (("encode", m), ("decode", 1)):
            sig = f"combine_kernel<{k}, {outs}, cec::{engine_of(op)}"
            disp = sorted((r for r in rows if sig in r["Kernel_Name"] and grid(r) * div == whole),
                          key=lambda r: int(r["Start_Timestamp"]))[: warm + steps]
            if len(disp) == warm + steps:
                part[op] = disp
        if len(part) == 2:
            boundaries(part, out.setdefault("shares", {}).setdefault(str(tiles // div), {}))
    half = out.get("shares", {}).get(str(tiles // 2))
    if half:
        for op in ("encode", "decode"):
            out[op]["fixed_us"] = {
                key: round(2 * half[op][key]["median"] - out[op][key]["median"], 3)
                for key in ("duration_us", "duration_plus_gap_us")}
    # (round-5 keys, for the records that quote them)
    out.update({x: out["encode"][x] for x in ("kernel", "dispatches_timed", "warmup_dispatches_skipped",
                                               "trace_avg_ms", "trace_median_ms", "line_event_avg_ms",
                                               "event_over_trace", "trace_frac_of_8TBps", "line_frac")})
    print(json.dumps(out, indent=1))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main(*sys.argv[1:])
