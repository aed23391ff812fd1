#!/usr/bin/env python3
"""Sweeping encoder parameters on one GPU: dcs_encode_sweep with DCS_SWEEP_MEASURE (every stream encoded with every set,
decoded and compared with its source in one call, the PCM resident in HBM) against the composition it replaces, built from
the one-set entry points only (encode_streams once per set -> decode_streams with extra_frames = 1 -> the sums in numpy),
and the sweep without the measurement against the encode_streams calls alone.  Six bit rates, wildcard layout, for 256
streams x 1 000 frames and for 4 streams x 20 000 frames; the two paths timed alternately in one process after a warm-up,
each to the call's return; bytes and sums compared.  --version 9301 --type 1: dcs_encode93a_sweep, OS93a Type-1 sets at the
six rates and one maximumQuantizationError (one search per stream-frame serves all six), against one encode93a_streams call
per set, for 256 streams x 256 frames.  --rocprof: per-kernel times of the measuring sweep from `rocprofv3 --kernel-trace
--stats`, in a run of their own.  Prints one JSON line."""
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

RATES = (256000, 192000, 128000, 96000, 64000, 48000)
SHAPES = {"batch_256x1000": (256, 1000), "long_4x20000": (4, 20000)}
SHAPES_93A = {"batch_256x256": (256, 256)}
TYPE1 = False                   # --version 9301 --type 1
KEYS = ("sumSrcSq", "sumDecSq", "sumCross", "peakErr")


def signals(n_streams, n_frames, seed):
    """16-bit valued tones over noise with a slow envelope, a different mix per stream"""
    rng = np.random.default_rng(seed)
    t = np.arange(n_frames * 240) / 31250.0
    out = []
    for _ in range(n_streams):
        x = sum(rng.uniform(0.05, 0.3) * np.sin(2 * np.pi * rng.uniform(60, 9000) * t + rng.uniform(0, 6)) for _ in range(4))
        x = x * (0.55 + 0.45 * np.sin(2 * np.pi * rng.uniform(0.2, 3.0) * t)) + rng.normal(0, rng.uniform(0.001, 0.08), t.size)
        out.append(np.clip(np.rint(x * 30000.0), -32768, 32767).astype(np.int16))
    return out


def sweep(ctx, pcm, sets, measure):
    streams, res = (ctx.encode93a_sweep if TYPE1 else ctx.encode_sweep)(pcm, sets, measure=measure)[:2]
    return streams, [tuple(int(r[k]) for k in KEYS) for r in res] if measure else None


def composed(ctx, pcm, sets, measure):
    """one encode_streams (encode93a_streams) call per set; measuring: each set's streams decoded with one extra frame, and
    numpy's sums"""
    n, k = len(pcm), len(sets)
    streams, sums = [None] * (n * k), [None] * (n * k)
    q = [x.astype(np.int64) for x in pcm] if measure else None
    for r, rate in enumerate(RATES):
        enc, info = ctx.encode93a_streams(pcm, D.FMT_93A_T1, targetBitRate=rate)[:2] if TYPE1 else ctx.encode_streams(pcm, None, targetBitRate=rate)
        for i, s in enumerate(enc):
            streams[i * k + r] = s
        if not measure:
            continue
        items = [(D.OS93A if TYPE1 else D.OS95 if inf["formatSubType"] == 3 else D.OS94, s, 255, 255) for s, inf in zip(enc, info)]
        dec, err, first = ctx.decode_streams(items, extra_frames=1)
        if err.any():
            raise RuntimeError("decode error in an encoded stream")
        flat = dec.reshape(-1)
        for i in range(n):
            d = flat[int(first[i]) * 240 + 16:int(first[i]) * 240 + 16 + len(q[i])].astype(np.int64)
            sums[i * k + r] = (int(np.dot(q[i], q[i])), int(np.dot(d, d)), int(np.dot(d, q[i])), int(np.abs(d - q[i]).max()))
    return streams, sums if measure else None


def timed(ctx, pcm, sets, measure, iters):
    a, b = sweep(ctx, pcm, sets, measure), composed(ctx, pcm, sets, measure)       # warm-up, and the results compared
    ts, tc = [], []
    for _ in range(iters):
        for fn, t in ((sweep, ts), (composed, tc)):
            t0 = time.perf_counter()
            fn(ctx, pcm, sets, measure)
            t.append(time.perf_counter() - t0)
    ms, mc = float(np.median(ts)), float(np.median(tc))
    return dict(sweep_ms=round(ms * 1e3, 1), composed_ms=round(mc * 1e3, 1), ratio=round(mc / ms, 3),
                sweep_rounds_ms=[round(v * 1e3, 1) for v in ts], composed_rounds_ms=[round(v * 1e3, 1) for v in tc],
                bytes_equal=a[0] == b[0], sums_equal=a[1] == b[1], bytes_out=sum(len(s) for s in a[0]))


def rocprof():
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "sw", "--",
               sys.executable, os.path.abspath(__file__), "--sweep-only"] + (["--version", "9301", "--type", "1"] if TYPE1 else [])
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
        return dict(kernels=kernels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--sweep-only", action="store_true", help="(the profiled run) one measuring sweep of the 256 x 1 000 batch")
    ap.add_argument("--version", choices=["9400", "9301"], default="9400")
    ap.add_argument("--type", type=int, choices=[1], default=None, help="with --version 9301: dcs_encode93a_sweep over OS93a Type-1 sets")
    a = ap.parse_args()
    if (a.version == "9301") != (a.type == 1):
        ap.error("--version 9301 and --type 1 go together")
    global TYPE1
    TYPE1 = a.type == 1
    if a.rocprof:
        print(json.dumps(dict(rocprof=rocprof())))
        return
    sets = [D.encode93a_params(D.FMT_93A_T1, targetBitRate=r) if TYPE1 else D.encode_params(None, targetBitRate=r) for r in RATES]
    ctx = D.Context(0)
    if a.sweep_only:
        sweep(ctx, signals(256, 256 if TYPE1 else 1000, 0x5EE0), sets, True)
        ctx.close()
        return
    res = {}
    for name, (n, frames) in (SHAPES_93A if TYPE1 else SHAPES).items():
        pcm = signals(n, frames, 0x5EE0)
        res[name] = dict(job_frames=n * frames * len(sets), measured=timed(ctx, pcm, sets, True, a.iters),
                         bytes_only=timed(ctx, pcm, sets, False, a.iters))
    ctx.close()
    print(json.dumps(dict(build_id=D.build_id(), results=res, all_equal=all(v[m]["bytes_equal"] and v[m]["sums_equal"] for v in res.values()
                                                     for m in ("measured", "bytes_only")))))


if __name__ == "__main__":
    main()
