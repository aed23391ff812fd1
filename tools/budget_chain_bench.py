#!/usr/bin/env python3
"""Budgets from any source on one GPU: encode_files_budget in the shared form on a seeded list of 256 WAV files (16-bit mono,
44.1 kHz, 64 to 448 frames once converted) and, behind them, 16 DCSa containers of OS93b streams of 64 to 448 frames (searched
under the 1994+ target: the join kernel's share), against the composition it replaces on the same build: wav_decode ->
resample_streams, decode_streams for the containers -> (the floats on the host) -> encode_rd_fit.  Three rounds after a
warm-up, the two paths alternating, each timed to the call's return; median and range, the bytes each path sends over the link, and whether both wrote the same
streams.  --rocprof: per-kernel times of one encode_files_budget call from `rocprofv3 --kernel-trace --stats`, in a run of
their own.  Prints one JSON line."""
import argparse
import csv
import glob
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dcsexplorer_amd as D                     # noqa: E402

RATE = 64000
FILE_RATE = 44100


def wav(x):
    """a 16-bit mono RIFF/WAVE file of the int16 samples x"""
    data = np.asarray(x, "<i2").tobytes()
    fmt = struct.pack("<HHIIHH", 1, 1, FILE_RATE, FILE_RATE * 2, 2, 16)
    return b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + len(data)) + b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt \
        + b"data" + struct.pack("<I", len(data)) + data


def files(n, seed):
    """tones over noise with a slow envelope, a different mix, level and length per file; every eighth near silence"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        frames = int(rng.integers(64, 449))
        t = np.arange(frames * 240 * FILE_RATE // 31250 - 64) / float(FILE_RATE)
        x = sum(rng.uniform(0.05, 0.3) * np.sin(2 * np.pi * rng.uniform(60, 9000) * t + rng.uniform(0, 6)) for _ in range(4))
        x = x * (0.55 + 0.45 * np.sin(2 * np.pi * rng.uniform(0.2, 3.0) * t)) + rng.normal(0, rng.uniform(0.001, 0.08), t.size)
        x *= 0.002 if i % 8 == 7 else rng.uniform(0.2, 0.9)
        out.append(wav(np.clip(np.rint(x * 30000.0), -32768, 32767).astype(np.int16)))
    return out


def containers(n, seed):
    """DCSa containers of synthetic OS93b Type-1 streams"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        s = D.synth_stream(D.FMT_93B_T1, int(rng.integers(64, 449)), seed=seed + i)
        out.append(D.dcsa_header(D.OS93B, len(s)) + s)
    return out


def composed(ctx, fs, cons, total):
    """the composition, and the bytes it sends over the link"""
    mono = ctx.wav_decode(fs)
    floats = ctx.resample_streams(mono, FILE_RATE)
    pcm = []
    for c in cons:
        os_, s = D.dcsa_parse(c)
        pcm.append(ctx.decode_streams([(os_, s, 0x67, 0xFF)], extra_frames=1)[0].ravel().astype(np.float32) / np.float32(32768))
    res = ctx.encode_rd_fit(floats + pcm, total)
    link = sum(len(f) for f in fs + cons) + 2 * 4 * sum(len(m) for m in mono) + 2 * 4 * sum(len(x) for x in floats) \
        + (2 + 4) * sum(len(x) for x in pcm) + sum(len(s) for s in res[0])
    return res, link, floats


def rocprof(n):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "chain", "--",
               sys.executable, os.path.abspath(__file__), "--one-call", "--files", str(n[0]), "--containers", str(n[1])]
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
        front = sum(k["total_ms"] for name, k in kernels.items() if name.startswith(("wav", "rs", "lv", "flac", "encJoin")))
        return dict(kernels=kernels, all_kernels_ms=round(total, 3), front_of_encoder_ms=round(front, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--containers", type=int, default=16)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--one-call", action="store_true", help="(the profiled run) one encode_files_budget call of the list")
    a = ap.parse_args()
    if a.rocprof:
        print(json.dumps(dict(rocprof=rocprof((a.files, a.containers)))))
        return
    fs = files(a.files, 0xB0D6E7)
    cons = containers(a.containers, 0xC0)
    ctx = D.Context(0)
    frames = [int(n) // 240 + (1 if int(n) % 240 else 0) for n in ctx.encode_files(fs)[1]["nSamples"]]
    frames += [((c[36] << 8) | c[37]) + 1 for c in cons]
    total = sum(18 + (RATE * f * 240 // 31250) // 8 for f in frames)
    if a.one_call:
        ctx.encode_files_budget(fs + cons, total=total)
        ctx.close()
        return
    one = ctx.encode_files_budget(fs + cons, total=total)                  # warm-up, and the results
    (two, link_two, _) = composed(ctx, fs, cons, total)
    t_one, t_two = [], []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        ctx.encode_files_budget(fs + cons, total=total)
        t_one.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        composed(ctx, fs, cons, total)
        t_two.append(time.perf_counter() - t0)
    ctx.close()
    ms = lambda v: round(v * 1e3, 1)
    print(json.dumps(dict(
        build_id=D.build_id(), files=a.files, containers=a.containers, frames=sum(frames), rate=RATE, total_bytes=total, rounds=a.rounds,
        one_call_ms=ms(float(np.median(t_one))), one_call_range_ms=[ms(min(t_one)), ms(max(t_one))],
        composed_ms=ms(float(np.median(t_two))), composed_range_ms=[ms(min(t_two)), ms(max(t_two))],
        one_call_link_bytes=sum(len(f) for f in fs + cons) + sum(len(s) for s in one[0]), composed_link_bytes=link_two,
        same_streams=one[0] == two[0], same_record=one[-1].tobytes() == two[3].tobytes(),
        used_bytes=int(one[-1]["usedBytes"]), sq_err=int(one[-1]["sqErr"]),
        measured="one_call_ms, composed_ms and their ranges (wall clock to each call's return, this run); the link bytes are counted "
                 "from the arrays' sizes, not measured")))


if __name__ == "__main__":
    main()
