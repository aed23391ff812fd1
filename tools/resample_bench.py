#!/usr/bin/env python3
"""Resampling throughput on one GPU: dcs_resample_streams (stage, walk, convolve; the input up, the 31 250 Hz samples down)
and dcs_encode_streams_at (the same, then the encoder on the resampled signal where it lies), against dcs_encode_streams on
PCM resampled beforehand (the encoder alone, its 31 250 Hz input uploaded).  Two workloads: 256 streams x 10 s at 44.1 kHz,
and one stream of 65 000 frames (15.6 M output samples, 22 M input samples at 44.1 kHz).  Each path is timed to the
call's return, median of --iters after a warm-up call; the default filter table.  Reports output samples per second and
checks that encode_streams_at's bytes are encode_streams' bytes on the pre-resampled PCM.  Also times the position walk
alone on the host (dcs_resample_count over the list, one thread), against which the device walk's share of rocprof can be set.  Prints one JSON line.
Per-kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/resample_bench.py --iters 1`."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dcsexplorer_amd as D                     # noqa: E402


def workload(name, rng):
    if name == "256x10s":
        n = 441000
        t = np.arange(n) / 44100.0
        return [(0.25 * np.sin(2 * np.pi * (220 + 7 * k) * t) + 0.05 * rng.uniform(-1, 1, n)).astype(np.float32) for k in range(256)]
    n = int(65000 * 240 / (31250.0 / 44100)) - 2000
    t = np.arange(n) / 44100.0
    return [(0.3 * np.sin(2 * np.pi * 440 * t) + 0.05 * rng.uniform(-1, 1, n)).astype(np.float32)]


def timed(fn, iters):
    fn()
    ts = []
    for _ in range(iters):
        t = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--workloads", default="256x10s,1x65000f")
    a = ap.parse_args()
    ctx = D.Context(0)
    rng = np.random.default_rng(7)
    res = {}
    for w in a.workloads.split(","):
        pcm = workload(w, rng)
        t_rs, y = timed(lambda: ctx.resample_streams(pcm, 44100), a.iters)
        n_out = sum(len(v) for v in y)
        t_at, enc_at = timed(lambda: ctx.encode_streams_at(pcm, 44100)[0], a.iters)
        t_enc, enc = timed(lambda: ctx.encode_streams(y)[0], a.iters)
        # the same position walk on the host, one stream after another (dcs_resample_count)
        t_host, counts = timed(lambda: [D.resample_count(len(v), 44100) for v in pcm], a.iters)
        assert sum(counts) == n_out
        res[w] = dict(streams=len(pcm), in_samples=int(sum(len(v) for v in pcm)), out_samples=int(n_out),
                      resample_s=t_rs, resample_out_per_s=n_out / t_rs, encode_at_s=t_at, encode_at_out_per_s=n_out / t_at,
                      encode_preresampled_s=t_enc, encode_preresampled_out_per_s=n_out / t_enc, bytes_equal=enc_at == enc,
                      host_walk_s=t_host, host_walk_ns_per_out=1e9 * t_host / n_out)
    ctx.close()
    print(json.dumps(dict(tool="resample_bench", results=res)))


if __name__ == "__main__":
    sys.exit(main())
