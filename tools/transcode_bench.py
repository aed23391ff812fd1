#!/usr/bin/env python3
"""Transcoding throughput on one GPU: dcs_transcode_streams (decode and re-encode with the PCM resident in HBM) against the
host composition it replaces (dcs_decode_streams with extraFrames = 1 -> int16 to float on the host -> dcs_encode_streams /
dcs_encode93_streams), timed alternately in one process after a warm-up, each to the call's return.  Every source family
(OS94 Type 1, OS93b Type 1, OS93a Type 1) into every target family (0x9400, 0x9302, 0x9301) in the target's wildcard layout,
DCS_TRANSCODE_REENCODE_ALL (so a source of the target's own family is re-encoded too), for 256 streams x 1 000 frames and
for one stream of 65 534 frames (65 535 out).  Reports source frames per second of both paths, their ratio, and whether
their bytes are equal.  --rocprof: per-kernel times and the host<->device copies of the fused path from `rocprofv3
--kernel-trace --memory-copy-trace --stats`, in a run of their own.  Prints one JSON line."""
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
from dcsexplorer_amd.api import _check, _ptr    # noqa: E402

SOURCES = {"94": (D.FMT_94_T1_S0, D.OS94), "93b": (D.FMT_93B_T1, D.OS93B), "93a": (D.FMT_93A_T1, D.OS93A)}
TARGETS = {"9400": 0x9400, "9302": 0x9302, "9301": 0x9301}


def sources(fam, n_streams, n_frames, seed):
    fmt, os_ = SOURCES[fam]
    return [D.synth_stream(fmt, n_frames, seed + k, nbands=18 if fmt == D.FMT_93A_T1 else 16) for k in range(n_streams)], os_


def fused(ctx, streams, os_, version):
    return ctx.transcode_streams(streams, [os_] * len(streams), version, reencode_all=True)[0]


def composed(ctx, streams, os_, version):
    """the host composition: decode down, convert on the host, encode up"""
    L = ctx.L
    refs = (D.api.StreamRef * len(streams))()
    keep = [np.frombuffer(s, np.uint8) for s in streams]
    total = 0
    for k, s in enumerate(streams):
        refs[k].data, refs[k].len, refs[k].os = keep[k].ctypes.data, len(s), os_
        refs[k].volume, refs[k].level, refs[k].channelVolume = 0x67, 0xFF, 0xFF
        total += ((s[0] << 8) | s[1]) + 1
    pcm = np.empty((total, 240), np.int16)
    first = np.empty(len(streams) + 1, np.uint32)
    err = np.empty(total, np.uint32)
    _check(L.dcs_decode_streams(ctx.h, refs, len(streams), 1, _ptr(pcm), total, _ptr(first), _ptr(err)), ctx.h)
    if err.any():
        raise RuntimeError("decode error in a source")
    x = pcm.reshape(-1).astype(np.float32) / np.float32(32768.0)
    parts = [x[first[k] * 240:first[k + 1] * 240] for k in range(len(streams))]
    if version == 0x9400:
        return ctx.encode_streams(parts)[0]
    return ctx.encode93_streams(parts, D.OS93A if version == 0x9301 else D.OS93B)[0]


def measure(ctx, streams, os_, version, iters):
    frames = sum((s[0] << 8) | s[1] for s in streams)
    a, b = fused(ctx, streams, os_, version), composed(ctx, streams, os_, version)      # warm-up, and the bytes compared
    tf, tc = [], []
    for _ in range(iters):
        for fn, t in ((fused, tf), (composed, tc)):
            t0 = time.perf_counter()
            fn(ctx, streams, os_, version)
            t.append(time.perf_counter() - t0)
    mf, mc = float(np.median(tf)), float(np.median(tc))
    return dict(frames=frames, fused_ms=round(mf * 1e3, 2), host_ms=round(mc * 1e3, 2), fused_fps=round(frames / mf),
                host_fps=round(frames / mc), speedup=round(mc / mf, 3), bit_exact=a == b, bytes_out=sum(len(s) for s in a))


def rocprof():
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "tc", "--",
               sys.executable, os.path.abspath(__file__), "--fused-only"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return dict(error="rocprofv3 exit %d" % r.returncode, stderr=r.stderr[-800:])
        kernels, copies = {}, []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                short = row.get("Name", "").replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].split("::")[-1]
                k = kernels.setdefault(short, dict(calls=0, total_ms=0.0))
                k["calls"] += int(row["Calls"])
                k["total_ms"] = round(k["total_ms"] + float(row["TotalDurationNs"]) / 1e6, 3)
        # the runtime's copies by direction: count, total and longest duration (and bytes where the trace has them); a
        # PCM-sized copy (256 000 frames x 480 B = 123 MB) would take milliseconds
        for path in glob.glob(os.path.join(d, "**", "*memory_copy_trace.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                size = next((int(v) for key, v in row.items() if key and ("size" in key.lower() or "bytes" in key.lower()) and v), None)
                kind = row.get("Direction") or row.get("Kind") or "?"
                dur = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6 if "End_Timestamp" in row else None
                copies.append((kind, dur, size))
        by = {}
        for kind, dur, size in copies:
            c = by.setdefault(kind, dict(count=0, total_ms=0.0, longest_ms=0.0, largest_bytes=None))
            c["count"] += 1
            if dur is not None:
                c["total_ms"] = round(c["total_ms"] + dur, 3)
                c["longest_ms"] = round(max(c["longest_ms"], dur), 3)
            if size is not None:
                c["largest_bytes"] = max(c["largest_bytes"] or 0, size)
        return dict(kernels=kernels, copies=by)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--fused-only", action="store_true", help="(the profiled run) one pass of the fused path over the batches")
    a = ap.parse_args()
    if a.rocprof:
        print(json.dumps(dict(rocprof=rocprof())))
        return
    ctx = D.Context(0)
    if a.fused_only:
        for fam in SOURCES:
            streams, os_ = sources(fam, 256, 1000, 0x7B00)
            for version in TARGETS.values():
                fused(ctx, streams, os_, version)
        ctx.close()
        return
    res = {}
    for fam in SOURCES:
        batch, os_ = sources(fam, 256, 1000, 0x7B00)
        long_, _ = sources(fam, 1, 65534, 0x7C00)
        for name, version in TARGETS.items():
            res["%s->%s" % (fam, name)] = dict(batch_256x1000=measure(ctx, batch, os_, version, a.iters),
                                              stream_65534=measure(ctx, long_, os_, version, max(2, a.iters - 1)))
    ctx.close()
    ratios = [v[k]["speedup"] for v in res.values() for k in v]
    print(json.dumps(dict(results=res, all_bit_exact=all(v[k]["bit_exact"] for v in res.values() for k in v),
                          speedup_min=min(ratios), speedup_max=max(ratios))))


if __name__ == "__main__":
    main()
