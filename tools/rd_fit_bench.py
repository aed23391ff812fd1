#!/usr/bin/env python3
"""Encoding a set to one byte budget on one GPU: encode_rd_fit against encode_rd_streams on the same batch (256 streams of
64 to 448 frames, the total the sum of the per-stream budgets a rate gives), each timed to the call's return after a warm-up,
alternately; the byte totals and the summed sqErr of both.  --streams-only: encode_rd_streams alone (with DCS_HIP_LIB naming
a build from before there was encode_rd_fit, the same batch on that build).  --rocprof: per-kernel times of one fit call from
`rocprofv3 --kernel-trace --stats`, in a run of their own, and the allocator kernels' share of them.  Prints one JSON line."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dcsexplorer_amd as D                     # noqa: E402

RATE = 64000
ALLOCATOR = ("encRdCurveKernel", "enc93RdCurveKernel", "encFitHullKernel", "encFitSortKernel", "encFitWalkKernel")


def signals(n_streams, seed):
    """tones over noise with a slow envelope, a different mix, level and length per stream; every eighth near silence"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_streams):
        t = np.arange(int(rng.integers(64, 449)) * 240) / 31250.0
        x = sum(rng.uniform(0.05, 0.3) * np.sin(2 * np.pi * rng.uniform(60, 9000) * t + rng.uniform(0, 6)) for _ in range(4))
        x = x * (0.55 + 0.45 * np.sin(2 * np.pi * rng.uniform(0.2, 3.0) * t)) + rng.normal(0, rng.uniform(0.001, 0.08), t.size)
        x *= 0.002 if i % 8 == 7 else rng.uniform(0.2, 1.0)
        out.append(np.clip(np.rint(x * 30000.0), -32768, 32767).astype(np.int16))
    return out


def budgets(pcm):
    return [18 + (RATE * ((len(x) + 239) // 240) * 240 // 31250) // 8 for x in pcm]


def rocprof():
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "fit", "--",
               sys.executable, os.path.abspath(__file__), "--fit-only"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return dict(error="rocprofv3 exit %d" % r.returncode, stderr=r.stderr[-800:])
        kernels = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                short = row.get("Name", "").replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].split("::")[-1]
                k = kernels.setdefault(short, dict(calls=0, total_ms=0.0))
                k["calls"] += int(row["Calls"])
                k["total_ms"] = round(k["total_ms"] + float(row["TotalDurationNs"]) / 1e6, 3)
        total = sum(k["total_ms"] for k in kernels.values())
        alloc = sum(k["total_ms"] for n, k in kernels.items() if n in ALLOCATOR)
        return dict(kernels=kernels, all_kernels_ms=round(total, 3), allocator_kernels_ms=round(alloc, 3),
                    allocator_share=round(alloc / total, 4) if total else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--fit-only", action="store_true", help="(the profiled run) one encode_rd_fit call of the batch")
    ap.add_argument("--streams-only", action="store_true")
    a = ap.parse_args()
    if a.rocprof:
        print(json.dumps(dict(rocprof=rocprof())))
        return
    pcm = signals(a.streams, 0xF17B)
    bud = budgets(pcm)
    total = sum(bud)
    ctx = D.Context(0)
    if a.fit_only:
        ctx.encode_rd_fit(pcm, total)
        ctx.close()
        return
    have_fit = not a.streams_only and hasattr(ctx.L, "dcs_encode_rd_fit")
    per = ctx.encode_rd_streams(pcm, None, bud)                     # warm-up, and the results
    fit = ctx.encode_rd_fit(pcm, total) if have_fit else None
    tp, tf = [], []
    for _ in range(a.iters):
        t0 = time.perf_counter()
        ctx.encode_rd_streams(pcm, None, bud)
        tp.append(time.perf_counter() - t0)
        if have_fit:
            t0 = time.perf_counter()
            ctx.encode_rd_fit(pcm, total)
            tf.append(time.perf_counter() - t0)
    ctx.close()
    res = dict(build_id=D.build_id(), streams=a.streams, frames=sum((len(x) + 239) // 240 for x in pcm), rate=RATE, total_bytes=total,
               streams_ms=round(float(np.median(tp)) * 1e3, 1), streams_rounds_ms=[round(v * 1e3, 1) for v in tp],
               streams_bytes=sum(len(s) for s in per[0]), streams_sq_err=int(sum(int(v) for v in per[2]["sqErr"])))
    if have_fit:
        res.update(fit_ms=round(float(np.median(tf)) * 1e3, 1), fit_rounds_ms=[round(v * 1e3, 1) for v in tf],
                   fit_bytes=sum(len(s) for s in fit[0]), fit_sq_err=int(fit[3]["sqErr"]), fit_steps=int(fit[3]["nSteps"]),
                   fit_steps_taken=int(fit[3]["stepsTaken"]),
                   sq_err_ratio=round(int(fit[3]["sqErr"]) / max(int(sum(int(v) for v in per[2]["sqErr"])), 1), 4))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
