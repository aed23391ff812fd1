#!/usr/bin/env python3
"""FLAC output on one GPU: dcs_decode_streams_flac (the decoded PCM written as FLAC where it lies in HBM; FLAC bytes and error
words come down) against dcs_decode_streams (PCM and error words come down), timed alternately in one process after a
warm-up, each to the call's return, with and without DCS_FLAC_MD5.  For the realistic_65536 and survey3_65536 stream lists:
the median time of each, the bytes each brings over the link and the compression ratio (PCM bytes / FLAC bytes).  For a list
of low-level audio-like PCM (256 x 256 frames of seeded sines and small noise; synthetic DCS streams may decode to
near-noise) and for one stream of 65 535 frames: dcs_flac_write_streams' time (which includes the PCM's upload) and ratio,
with and without the MD5 -- the difference is W4's cost, one lane walking one stream.  --rocprof: W1-W4's kernel times beside
the decode kernel's, from `rocprofv3 --kernel-trace --stats` in a run of their own.  --pipeline: the same two stream lists through
dcs_pipeline with all three stages on the device, FLAC out (with and without the MD5) against PCM out at the same depth, in
alternating rounds after a warm-up: milliseconds per list sustained over --lists lists a side, and what each brings over the link
per list.  Prints one JSON line."""
import argparse
import csv
import ctypes
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
from dcsexplorer_amd import workloads           # noqa: E402
from dcsexplorer_amd.api import FLAC_WRITE_INFO_DTYPE, PipelineFlacResult, PipelineResult, _check, _ptr, _stream_refs   # noqa: E402

LISTS = ("realistic_65536", "survey3_65536")


def audio_like(n_streams, n_frames, seed=0xA0D10):
    r = np.random.default_rng(seed)
    t = np.arange(n_frames * 240)
    out = []
    for _ in range(n_streams):
        x = sum(a * np.sin(t * (2 * np.pi * f / 31250) + p) for a, f, p in zip(r.uniform(50, 1500, 3), r.uniform(60, 4000, 3), r.uniform(0, 6, 3)))
        out.append(np.rint(x + r.normal(0, 4, t.size)).astype(np.int16))
    return out


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


def kinds_of(info):
    return {k: int(info[k].sum()) for k in ("nConstant", "nVerbatim", "nFixed")}


def measure_list(ctx, name, iters):
    """both sides are the C call alone, into buffers made once before the clock starts (np.empty: no host pass over them)"""
    streams = workloads.WORKLOADS[name]()
    refs, keep = _stream_refs(streams)
    n = len(streams)
    frames = [(int(k[0]) << 8) | int(k[1]) for k in keep]
    total = sum(frames)
    pcm, err, first = np.empty((total, 240), np.int16), np.empty(total, np.uint32), np.empty(n + 1, np.uint32)
    cap = sum(D.flac_write_bound(f * 240) for f in frames)
    out, offs, info = np.empty(cap, np.uint8), np.empty(n + 1, np.uint64), np.empty(n, FLAC_WRITE_INFO_DTYPE)

    def down_pcm():
        _check(ctx.L.dcs_decode_streams(ctx.h, refs, n, 0, _ptr(pcm), total, _ptr(first), _ptr(err)), ctx.h)

    def down_flac(flags):
        _check(ctx.L.dcs_decode_streams_flac(ctx.h, refs, n, 0, flags, _ptr(out), cap, _ptr(offs), _ptr(info), _ptr(err)), ctx.h)

    ms = median_ms([down_pcm, lambda: down_flac(0), lambda: down_flac(D.FLAC_MD5)], iters)
    flac_bytes = int(offs[n])
    return dict(frames=total, pcm_link_bytes=pcm.nbytes + err.nbytes, flac_link_bytes=flac_bytes + err.nbytes,
                ratio=round(pcm.nbytes / flac_bytes, 4), kinds=kinds_of(info), decode_streams_ms=ms[0],
                decode_streams_flac_ms=ms[1], decode_streams_flac_md5_ms=ms[2])


def measure_pcm(ctx, pcm_list, iters):
    n = len(pcm_list)
    pcm = np.concatenate(pcm_list)
    soffs = np.concatenate(([0], np.cumsum([p.size for p in pcm_list]))).astype(np.uint64)
    cap = sum(D.flac_write_bound(p.size) for p in pcm_list)
    out, offs, info = np.empty(cap, np.uint8), np.empty(n + 1, np.uint64), np.empty(n, FLAC_WRITE_INFO_DTYPE)

    def write(flags):
        _check(ctx.L.dcs_flac_write_streams(ctx.h, _ptr(pcm), _ptr(soffs), n, 31250, flags, _ptr(out), cap, _ptr(offs), _ptr(info)), ctx.h)

    ms = median_ms([lambda: write(0), lambda: write(D.FLAC_MD5)], iters)
    return dict(samples=int(pcm.size), flac_bytes=int(offs[n]), ratio=round(pcm.nbytes / int(offs[n]), 4), kinds=kinds_of(info),
                write_ms=ms[0], write_md5_ms=ms[1], md5_ms=round(ms[1] - ms[0], 2))


def measure_pipeline(ctx, name, depth, lists, rounds):
    """the C calls alone on both sides (collect hands out pointers into pinned memory; nothing is copied out of it)"""
    streams = workloads.WORKLOADS[name]()
    refs, keep = _stream_refs(streams)
    n = len(streams)
    frames = sum((int(k[0]) << 8) | int(k[1]) for k in keep)
    L = ctx.L
    sides = dict(pcm=dict(flac=False, md5=False), flac=dict(flac=True, md5=False), flac_md5=dict(flac=True, md5=True))
    flac_bytes, other_path = {}, {side: 0 for side in sides}

    def run(side, count):
        pipe = ctx.pipeline(depth, index_on_device=True, pack_on_device=True, plan_on_device=True, **sides[side])
        res = PipelineFlacResult() if sides[side]["flac"] else PipelineResult()
        collect = L.dcs_pipeline_collect_flac if sides[side]["flac"] else L.dcs_pipeline_collect

        def collect_one():
            _check(collect(pipe.h, ctypes.byref(res)), ctx.h)
            other_path[side] += res.path != 7           # (a list the device planner handed back to the host's)
            if sides[side]["flac"]:
                flac_bytes[side] = int(ctypes.cast(res.flacOffsets, ctypes.POINTER(ctypes.c_uint64))[n])

        def lists_through(k_lists):
            done = 0
            for k in range(k_lists):
                _check(L.dcs_pipeline_submit(pipe.h, refs, n, 0), ctx.h)      # (blocks while `depth` lists are in flight)
                if k >= depth - 1:
                    collect_one()
                    done += 1
            while done < k_lists:
                collect_one()
                done += 1

        lists_through(2 * depth)                        # warm: the context's buffer cache, every stream's first copies
        t0 = time.perf_counter()
        lists_through(count)
        ms = (time.perf_counter() - t0) * 1e3 / count
        pipe.close()
        return ms

    per_round = max(depth, (lists + rounds - 1) // rounds)
    ms = {side: [] for side in sides}
    for _ in range(rounds):
        for side in sides:
            ms[side].append(run(side, per_round))
    err_bytes, table_bytes = 4 * frames, 8 * (n + 2) + FLAC_WRITE_INFO_DTYPE.itemsize * n
    out = dict(frames=frames, streams=n, depth=depth, lists_per_side=per_round * rounds, rounds=rounds)
    for side in sides:
        link = 480 * frames + err_bytes if side == "pcm" else (flac_bytes[side] + 15) // 16 * 16 + table_bytes + err_bytes
        out[side] = dict(ms_per_list=round(float(np.median(ms[side])), 4), rounds_ms=[round(m, 4) for m in ms[side]], link_bytes_per_list=link,
                         lists_not_on_device_path=other_path[side])
    out["link_ratio"] = round(out["pcm"]["link_bytes_per_list"] / out["flac"]["link_bytes_per_list"], 4)
    return out


def rocprof():
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "fw", "--",
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--pipeline", action="store_true", help="FLAC pipeline against PCM pipeline, sustained")
    ap.add_argument("--depth", type=int, default=32, help="(--pipeline) lists in flight, the same for both sides")
    ap.add_argument("--lists", type=int, default=240, help="(--pipeline) lists timed per side, at least")
    ap.add_argument("--rounds", type=int, default=3, help="(--pipeline) alternating rounds the lists are spread over")
    ap.add_argument("--once", action="store_true", help="(the profiled run) one decode_streams_flac of each list and one long stream")
    a = ap.parse_args()
    if a.rocprof:
        print(json.dumps(dict(rocprof=rocprof())))
        return
    workloads.register_recordings(np.load(os.path.join(ROOT, "tests", "golden", "encoder_golden.npz")))
    ctx = D.Context(0)
    if a.once:
        for name in LISTS:
            ctx.decode_streams_flac(workloads.WORKLOADS[name](), md5=True)
        ctx.flac_write_streams(audio_like(1, 65535), md5=True)
        ctx.close()
        return
    if a.pipeline:
        res = {name: measure_pipeline(ctx, name, a.depth, max(a.lists, 200), a.rounds) for name in LISTS}
        ctx.close()
        print(json.dumps(res))
        return
    res = {name: measure_list(ctx, name, a.iters) for name in LISTS}
    res["audio_like_256x256"] = measure_pcm(ctx, audio_like(256, 256), a.iters)
    res["one_stream_65535"] = measure_pcm(ctx, audio_like(1, 65535), a.iters)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
