#!/usr/bin/env python3
"""Encoder throughput on one GPU (dcs_encode_streams, host buffers in and out, timed to the call's return, which
synchronises the device): frames per second and the real-time factor (seconds of 31 250 Hz audio per second) for
256 streams x 256 frames and for one stream of 65 535 frames (the format's longest), in the reference's wildcard layout
(three layouts searched).  --version 9301 / 9302: the OS93 encoder (dcs_encode93_streams) in its wildcard (0x9302: Type 0
and Type 1; 0x9301: Type 0).  --version 9301 --type 1 / -1: the OS93a Type-1 encoder (dcs_encode93a_streams), alone or
in its wildcard beside Type 0.  --rd: the rate-distortion 1994+ encoder (dcs_encode_rd_streams, every layout, each stream held
to the bytes dcs_encode_streams gave it) against dcs_encode_streams in the same run and against encode_fit over the six
rates of tests/sweep_ref.py, which is what it replaces for a budget: medians of alternating rounds.  --rd --version 9301 / 9302:
the rate-distortion OS93 Type-0 encoder (dcs_encode93_rd_streams) against dcs_encode93_streams' Type 0 and encode93a_fit /
encode_fit in the same way.  --rocprof: per-kernel times from `rocprofv3 --kernel-trace --stats`, in a run of their own.
Prints one JSON line."""
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


def signal(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 31250.0
    x = 0.3 * np.sin(2 * np.pi * 220.0 * (1 + seed % 7) * t) + 0.1 * np.sin(2 * np.pi * 3100.0 * t) + 0.05 * rng.standard_normal(n)
    return np.clip(np.rint(x * 32767), -32768, 32767).astype(np.int16)


def measure(encode, pcm, iters):
    encode(pcm)                                 # warm-up: buffers, code objects
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        streams = encode(pcm)[0]
        times.append(time.perf_counter() - t0)
    frames = sum((len(x) + 239) // 240 for x in pcm)
    med = float(np.median(times))
    return dict(streams=len(pcm), frames=frames, iters=iters, median_ms=round(med * 1e3, 3), min_ms=round(min(times) * 1e3, 3),
                frames_per_s=round(frames / med), realtime_factor=round(frames * 240 / 31250.0 / med, 1),
                bytes_out=sum(len(s) for s in streams))


def rocprof(iters, version, typ):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "enc", "--", sys.executable, os.path.abspath(__file__),
               "--iters", str(iters), "--version", version] + (["--type", str(typ)] if typ is not None else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return dict(error="rocprofv3 exit %d" % r.returncode, stderr=r.stderr[-800:])
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Name", "")
                if "enc" in name:
                    short = name.replace("(anonymous namespace)::", "").split("(")[0].split("::")[-1]
                    out[short] = dict(calls=int(row["Calls"]), total_ms=round(float(row["TotalDurationNs"]) / 1e6, 3),
                                      avg_us=round(float(row["AverageNs"]) / 1e3, 1))
        return out


RATES = (256000, 192000, 128000, 96000, 64000, 48000)


def rd_rounds(ctx, D, pcm, rounds, with_fit, version="9400"):
    """alternating rounds of encode_streams, encode_rd_streams within its bytes, and encode_fit over RATES within their sum
    (version 9301 / 9302: encode93_streams' Type 0, encode93_rd_streams, and encode93a_fit / encode_fit on Type-0 sets)"""
    if version == "9400":
        budgets = [len(s) for s in ctx.encode_streams(pcm)[0]]
        sets = [D.encode_params(None, targetBitRate=r) for r in RATES]
        calls = dict(encode_streams=lambda: ctx.encode_streams(pcm), encode_rd_streams=lambda: ctx.encode_rd_streams(pcm, None, budgets))
        fit = ctx.encode_fit
    else:
        os_ = D.OS93A if version == "9301" else D.OS93B
        budgets = [len(s) for s in ctx.encode93_streams(pcm, os_, D.FMT_93_T0)[0]]
        sets = [D.encode93_params(os_, D.FMT_93_T0, targetBitRate=r) for r in RATES]
        calls = dict(encode_streams=lambda: ctx.encode93_streams(pcm, os_, D.FMT_93_T0),
                     encode_rd_streams=lambda: ctx.encode93_rd_streams(pcm, os_, budgets))
        fit = ctx.encode93a_fit if version == "9301" else ctx.encode_fit
    if with_fit:
        calls["encode_fit"] = lambda: fit(pcm, sets, sum(budgets))
    times = {k: [] for k in calls}
    out = {}
    for k, f in calls.items():
        out[k] = f()                            # warm-up: buffers, code objects
    for _ in range(rounds):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t0)
    frames = sum((len(x) + 239) // 240 for x in pcm)
    res = dict(streams=len(pcm), frames=frames, rounds=rounds)
    for k in calls:
        med = float(np.median(times[k]))
        res[k] = dict(median_ms=round(med * 1e3, 3), min_ms=round(min(times[k]) * 1e3, 3), max_ms=round(max(times[k]) * 1e3, 3),
                      frames_per_s=round(frames / med), bytes_out=sum(len(s) for s in out[k][0]))
    info = out["encode_rd_streams"][2]
    res["encode_rd_streams"].update(fits=int(info["fits"].sum()), sq_err=int(info["sqErr"].astype(object).sum()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--version", choices=["9400", "9301", "9302"], default="9400")
    ap.add_argument("--type", type=int, choices=[-1, 1], default=None, help="with --version 9301: dcs_encode93a_streams, Type 1 or the wildcard")
    ap.add_argument("--rd", action="store_true", help="dcs_encode_rd_streams against encode_streams and encode_fit, alternating rounds")
    ap.add_argument("--streams", type=int, default=256, help="with --rd: streams of 256 frames in the batch")
    a = ap.parse_args()
    if a.rd:
        import dcsexplorer_amd as D
        ctx = D.Context(0)
        res = dict(build_id=D.build_id(), version=a.version,
                   batch=rd_rounds(ctx, D, [signal(256 * 240, k) for k in range(a.streams)], a.iters, True, a.version),
                   # (encode_fit measures, and a measured stream has 65 534 frames at the most: the long stream goes without it)
                   stream_65535=rd_rounds(ctx, D, [signal(65535 * 240, 999)], max(2, a.iters // 3), False, a.version))
        ctx.close()
        print(json.dumps(res))
        return
    if a.type is not None and a.version != "9301":
        ap.error("--type goes with --version 9301")
    if a.rocprof:
        print(json.dumps(dict(version=a.version, kernels=rocprof(3, a.version, a.type))))
        return
    import dcsexplorer_amd as D
    ctx = D.Context(0)
    if a.version == "9400":
        encode = ctx.encode_streams
    elif a.type is not None:
        encode = lambda pcm: ctx.encode93a_streams(pcm, D.FMT_93A_T1 if a.type == 1 else None)        # noqa: E731
    else:
        os_ = D.OS93A if a.version == "9301" else D.OS93B
        encode = lambda pcm: ctx.encode93_streams(pcm, os_)        # noqa: E731
    batch = [signal(256 * 240, k) for k in range(256)]
    res = dict(batch_256x256=measure(encode, batch, a.iters), stream_65535=measure(encode, [signal(65535 * 240, 999)], max(2, a.iters // 3)))
    if a.version != "9400":
        res = dict(version=a.version, **res)
    if a.type is not None:
        res = dict(type=a.type, build_id=D.build_id(), **res)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
