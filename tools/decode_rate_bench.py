#!/usr/bin/env python3
"""Decoding at an output rate on one GPU: dcs_decode_streams_at at 48 000 and at 44 100 Hz (the decoded PCM converted where
it lies in HBM; the converted samples and the error words come down) against dcs_decode_streams (the 31 250 Hz PCM and the
error words come down), for the realistic_65536 and survey3_65536 stream lists and for ragged_65536, a list of this tool's
own (256 seeded synthetic 1994+ streams of 1, 3, 5 .. 511 frames, 65 536 frames in all: every stream has a length of its
own, where the other two lists have one length between them and so no count walk at all).  Each C call is timed alone into
buffers made beforehand: the median of --iters alternating rounds after a warm-up round.  Per list: the median milliseconds of
each call, the bytes each brings over the link, and how many distinct stream lengths the list has (each is one count walk).

--trace: where a call's time goes.  A child process with DCS_RATE_TRACE set runs each list at 48 000 Hz --iters times
after a warm-up call; the library's own stderr lines (index and plan on the host, batch made and queued, the converter's
walks, convolution and waits, the download into the caller's buffer) are read back and their medians reported.  --rocprof:
the kernels' times (the decode kernel, rsWalkKernel where the table is walked on a device lane, rsConvolveKernel) from
`rocprofv3 --kernel-trace --stats`, a run of its own.  --flac: dcs_decode_streams_flac_at (the converted samples leave the
device as FLAC) against dcs_decode_streams_at at both rates, without and with the MD5: the median milliseconds of each call,
the bytes each brings over the link, the compression ratio (converted PCM bytes / FLAC bytes) and the kinds of subframe
written.  Prints one JSON line."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dcsexplorer_amd as D                     # noqa: E402
from dcsexplorer_amd import workloads           # noqa: E402
from dcsexplorer_amd.api import FLAC_WRITE_INFO_DTYPE, RATE_INFO_DTYPE, _check, _ptr, _resample_out_bound, _stream_refs   # noqa: E402

LISTS = ("realistic_65536", "survey3_65536", "ragged_65536")
RATES = (48000, 44100)


def median_ms(fns, iters):
    """the functions timed in turn, `iters` rounds after one warm-up round -> their median milliseconds"""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(iters):
        for fn, t in zip(fns, ts):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
    return [round(float(np.median(t)) * 1e3, 2) for t in ts]


def ragged():
    return [(D.OS94, D.synth_stream(D.FMT_94_T0 + k % 3, 1 + 2 * k, seed=0x4A66 + k), 255, 0x64) for k in range(256)]


def streams_of(name):
    return ragged() if name == "ragged_65536" else workloads.WORKLOADS[name]()


def calls_of(ctx, name):
    """the two C calls on one list, into buffers made once (np.empty: no host pass over them) -> (down_pcm, down_at, facts)"""
    streams = streams_of(name)
    refs, keep = _stream_refs(streams)
    n = len(streams)
    frames = [(int(k[0]) << 8) | int(k[1]) for k in keep]
    total = sum(frames)
    pcm, err, first = np.empty((total, 240), np.int16), np.empty(total, np.uint32), np.empty(n + 1, np.uint32)
    cap = sum(_resample_out_bound(f * 240, max(RATES), False) for f in frames)
    out, offs, info = np.empty(cap, np.int16), np.empty(n + 1, np.uint64), np.empty(n, RATE_INFO_DTYPE)
    converted, clipped = {}, {}

    def down_pcm():
        _check(ctx.L.dcs_decode_streams(ctx.h, refs, n, 0, _ptr(pcm), total, _ptr(first), _ptr(err)), ctx.h)

    def down_at(rate):
        _check(ctx.L.dcs_decode_streams_at(ctx.h, refs, n, 0, rate, None, 0, _ptr(out), cap, _ptr(offs), _ptr(info), _ptr(err)), ctx.h)
        converted[rate], clipped[rate] = int(offs[n]), int(info["nClipped"].sum())

    facts = dict(frames=total, streams=n, distinct_lengths=len(set(frames)), longest_frames=max(frames),
                 pcm_link_bytes=pcm.nbytes + err.nbytes)
    return down_pcm, down_at, facts, converted, clipped, err.nbytes, (refs, keep)


def measure_list(ctx, name, iters):
    down_pcm, down_at, res, converted, clipped, err_bytes, _keep = calls_of(ctx, name)
    ms = median_ms([down_pcm] + [lambda r=r: down_at(r) for r in RATES], iters)
    res["decode_streams_ms"] = ms[0]
    for r, m in zip(RATES, ms[1:]):
        res["decode_streams_at_%d_ms" % r] = m
        res["at_%d_link_bytes" % r] = 2 * converted[r] + err_bytes
        res["at_%d_clipped" % r] = clipped[r]
    return res


def measure_list_flac(ctx, name, iters):
    """--flac: dcs_decode_streams_flac_at (the converted samples written as FLAC where they lie in HBM; FLAC bytes, the two
    per-stream tables and the error words come down) against dcs_decode_streams_at (the converted samples come down), per
    rate: the C calls alone into buffers made once, timed in alternating rounds"""
    streams = streams_of(name)
    refs, keep = _stream_refs(streams)
    n = len(streams)
    frames = [(int(k[0]) << 8) | int(k[1]) for k in keep]
    total = sum(frames)
    err = np.empty(total, np.uint32)
    bounds = [_resample_out_bound(f * 240, max(RATES), False) for f in frames]
    cap, flac_cap = sum(bounds), sum(D.flac_write_bound(b) for b in bounds)
    out, offs, info = np.empty(cap, np.int16), np.empty(n + 1, np.uint64), np.empty(n, RATE_INFO_DTYPE)
    flac, flac_offs, flac_info = np.empty(flac_cap, np.uint8), np.empty(n + 1, np.uint64), np.empty(n, FLAC_WRITE_INFO_DTYPE)
    seen = {}

    def down_at(rate):
        _check(ctx.L.dcs_decode_streams_at(ctx.h, refs, n, 0, rate, None, 0, _ptr(out), cap, _ptr(offs), _ptr(info), _ptr(err)), ctx.h)
        seen[rate, "samples"] = int(offs[n])

    def down_flac_at(rate, flags):
        _check(ctx.L.dcs_decode_streams_flac_at(ctx.h, refs, n, 0, rate, None, flags, _ptr(flac), flac_cap, _ptr(flac_offs), _ptr(flac_info),
                                                _ptr(info), _ptr(err)), ctx.h)
        seen[rate, "flac"] = int(flac_offs[n])
        seen[rate, "kinds"] = {k: int(flac_info[k].sum()) for k in ("nConstant", "nVerbatim", "nFixed")}

    fns = [f for r in RATES for f in (lambda r=r: down_at(r), lambda r=r: down_flac_at(r, 0), lambda r=r: down_flac_at(r, D.FLAC_MD5))]
    ms = median_ms(fns, iters)
    res = dict(frames=total, streams=n, distinct_lengths=len(set(frames)), longest_frames=max(frames))
    for i, r in enumerate(RATES):
        res["decode_streams_at_%d_ms" % r], res["decode_streams_flac_at_%d_ms" % r], res["decode_streams_flac_at_%d_md5_ms" % r] = ms[3 * i:3 * i + 3]
        res["at_%d_link_bytes" % r] = 2 * seen[r, "samples"] + err.nbytes
        res["flac_at_%d_link_bytes" % r] = (seen[r, "flac"] + 15) // 16 * 16 + 8 * (n + 2) + FLAC_WRITE_INFO_DTYPE.itemsize * n + err.nbytes
        res["flac_at_%d_ratio" % r] = round(2 * seen[r, "samples"] / seen[r, "flac"], 4)
        res["flac_at_%d_kinds" % r] = seen[r, "kinds"]
    del keep
    return res


def rocprof():
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "dr", "--",
               sys.executable, os.path.abspath(__file__), "--once"]
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


TRACE_FIELDS = (("index_and_plan_ms", r"index and plan ([0-9.]+) ms"), ("batch_made_and_queued_ms", r"batch made and queued ([0-9.]+) ms"),
                ("walks_convolution_waits_ms", r"walks, convolution and waits ([0-9.]+) ms"), ("download_ms", r"download ([0-9.]+) ms"))


def trace(iters):
    """the library's own account of a call at 48 000 Hz, per list: medians over `iters` calls after a warm-up call"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--trace-child", "--iters", str(iters)], capture_output=True, text=True,
                       timeout=900, env=dict(os.environ, DCS_RATE_TRACE="1"))
    if r.returncode != 0:
        return dict(error="exit %d" % r.returncode, stderr=r.stderr[-800:])
    res, name = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("list "):
            name = line.split()[1]
            res[name] = {k: [] for k, _ in TRACE_FIELDS}
        for k, pat in TRACE_FIELDS:
            m = re.search(pat, line)
            if m and name:
                res[name][k].append(float(m.group(1)))
    return {n: {k: round(float(np.median(v[1:])), 3) for k, v in f.items() if len(v) > 1} for n, f in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--flac", action="store_true", help="decode_streams_flac_at against decode_streams_at, per list and rate")
    ap.add_argument("--once", action="store_true", help="(the profiled run) one decode_streams_at of each list at 48 000 Hz")
    ap.add_argument("--trace-child", action="store_true", help="(the traced run) iters + 1 calls of each list at 48 000 Hz")
    a = ap.parse_args()
    if a.rocprof:
        print(json.dumps(dict(rocprof=rocprof())))
        return
    if a.trace:
        print(json.dumps(dict(trace_48000=trace(a.iters))))
        return
    workloads.register_recordings(np.load(os.path.join(ROOT, "tests", "golden", "encoder_golden.npz")))
    ctx = D.Context(0)
    if a.once or a.trace_child:
        for name in LISTS:
            down_at, keep = calls_of(ctx, name)[1::5]
            sys.stderr.write("list %s\n" % name)
            sys.stderr.flush()
            for _ in range(a.iters + 1 if a.trace_child else 1):
                down_at(48000)
            del keep
        ctx.close()
        return
    res = {name: (measure_list_flac if a.flac else measure_list)(ctx, name, a.iters) for name in LISTS}
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
