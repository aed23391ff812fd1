#!/usr/bin/env python3
"""dcs_encode_files throughput on one GPU, against the host composition it replaces: the WAV files read on the host
(wav_parse + tests/wav_ref.py's conversion and downmix), then dcs_encode_streams_at on the float PCM.  Workloads:
256 x 10 s 16-bit stereo 44.1 kHz (each walk on a device lane), one 180 s 16-bit stereo 44.1 kHz file (the walk on the
host), 256 x 10 s IMA ADPCM mono 22.05 kHz (its composition decodes with dcs_wav_decode, because the numpy ADPCM restatement
is a Python loop).  Each path is timed to the call's return, median of --iters after a warm-up call, the two paths
alternating; both must give the same bytes.  Prints one JSON line.  Per-kernel times: run this under
`rocprofv3 --kernel-trace --stats -- python tools/encode_files_bench.py --iters 1`.

--flac: what reading FLAC costs.  The same audio as a FLAC file and as a 16-bit WAV file through encode_files: the 1 s
44.1 kHz stereo shape of tests/flac_cases.py (4 096-sample frames, LPC orders 8 and 6, left/side and mid/side) repeated to
--flac-seconds, the file replicated over --flac-files counts (1, 16, 256).  Wall time per call for each, median of --iters;
both must give the same bytes.  The WAV run is the yardstick; the difference is the cost of F1, F2, F3 and the index.  Under
`rocprofv3 --kernel-trace --stats -- python tools/encode_files_bench.py --flac --flac-files 256 --iters 1` the three kernels
stand beside the resample and encode kernels.

--level fit|gain: what the level stage costs.  The files of each workload through encode_files without a level and with one
that scales every file (fit: DCS_LEVEL_FIT to --ceiling, below the files' peaks; gain: DCS_LEVEL_GAIN of 0.5), the two calls
alternating, median and range of --iters each; beside them a device-to-device copy of the resampled floats (the stage reads
and writes them once), timed in the same run.  With a library from before the stage (DCS_HIP_LIB) only the call without a
level runs: the same command on two builds compares their unlevelled paths."""
import argparse
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dcsexplorer_amd as D                     # noqa: E402
import wav_cases as W                           # noqa: E402
import wav_ref as R                             # noqa: E402


def stereo16(seconds, rate, seed):
    n = seconds * rate
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    lr = np.stack([0.3 * np.sin(2 * np.pi * (220 + seed) * t), 0.3 * np.sin(2 * np.pi * (330 + seed) * t)], axis=1)
    v = np.round((lr + 0.05 * rng.uniform(-1, 1, lr.shape)).reshape(-1) * 32767).astype("<i2")
    return W.riff([W.fmt_chunk(1, 2, rate, 16), W.chunk("data", v.tobytes())])


def ima_mono(seconds, rate, seed, block_align=1024):
    """IMA ADPCM blocks with seeded headers and small nibbles (codes 0, 1, 8, 9: the step index settles at 0)"""
    rng = np.random.default_rng(seed)
    per = 2 * (block_align - 4)
    nb = -(-seconds * rate // (per + 1))
    nib = rng.choice(np.array([0, 1, 8, 9], np.uint8), size=(nb, per))
    body = (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8)
    hdr = np.zeros((nb, 4), np.uint8)
    hdr[:, 0:2] = np.frombuffer(struct.pack("<h", 0) * nb, np.uint8).reshape(nb, 2)
    data = np.concatenate([hdr, body], axis=1).tobytes()
    fact = W.chunk("fact", struct.pack("<I", seconds * rate))
    return W.riff([W.fmt_chunk(0x11, 1, rate, 4, block_align=block_align, size=20), fact, W.chunk("data", data)])


def workload(name):
    if name == "256x10s_s16_stereo_44k":
        return [stereo16(10, 44100, k) for k in range(256)]
    if name == "1x180s_s16_stereo_44k":
        return [W.long_wav()]
    return [ima_mono(10, 22050, k) for k in range(256)]


def flac_and_wav(seconds):
    """-> (FLAC file, WAV file) of the same integers: flac_cases' realistic second, its frames renumbered and repeated"""
    import flac_cases as F
    import flac_ref as FR
    second = dict(F.cases())["realistic_44100_stereo"]
    ints = F.integers()["realistic_44100_stereo"][0]
    _, frames = FR.index(second)
    out = []
    for c in range(seconds):
        for j, f in enumerate(frames):
            body = second[f["offset"] + f["headerLength"]:f["offset"] + f["length"] - 2]
            fr = F.frame_header(c * len(frames) + j, f["blockSize"], f["channelAssignment"]) + body
            out.append(fr + struct.pack(">H", F.crc16(fr)))
    info = F.streaminfo(frames[-1]["blockSize"], frames[0]["blockSize"], 44100, 2, 16, 44100 * seconds)
    flac = b"fLaC" + F.metadata_block(0, info, True) + b"".join(out)
    return flac, W.wav("s16", 2, 44100, np.tile(ints, seconds))


def flac_mode(ctx, a):
    flac, wav = flac_and_wav(a.flac_seconds)
    res = dict(seconds=a.flac_seconds, flac_mb=len(flac) / 1e6, wav_mb=len(wav) / 1e6, frames=D.flac_parse(flac)["nFrames"], counts={})
    for n in [int(x) for x in a.flac_files.split(",")]:
        ff, ww = [flac] * n, [wav] * n
        out_f, info = ctx.encode_files(ff)
        out_w, _ = ctx.encode_files(ww)
        tf, tw = [], []
        for _ in range(a.iters):
            t = time.perf_counter(); ctx.encode_files(ff); tf.append(time.perf_counter() - t)
            t = time.perf_counter(); ctx.encode_files(ww); tw.append(time.perf_counter() - t)
        res["counts"][n] = dict(f1_lanes=n * res["frames"], flac_s=float(np.median(tf)), wav_s=float(np.median(tw)),
                                flac_minus_wav_s=float(np.median(tf) - np.median(tw)), bytes_equal=out_f == out_w,
                                out_samples=int(info["nSamples"].sum()))
    return res


def d2d_copy_s(n_floats, iters):
    """median seconds of one device-to-device copy of n_floats float32 values"""
    import torch
    a = torch.zeros(n_floats, dtype=torch.float32, device="cuda")
    b = torch.empty_like(a)
    b.copy_(a)
    torch.cuda.synchronize()
    ts = []
    for _ in range(max(iters, 5)):
        t = time.perf_counter(); b.copy_(a); torch.cuda.synchronize(); ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def level_mode(ctx, a):
    have = hasattr(ctx.L, "dcs_encode_files_level")
    level = D.Level(D.LEVEL_FIT, ceiling=a.ceiling) if a.level == "fit" else D.Level(D.LEVEL_GAIN, gain=0.5)
    res = {}
    for w in a.workloads.split(","):
        files = workload(w)
        out, info = ctx.encode_files(files)
        row = dict(files=len(files), out_samples=int(info["nSamples"].sum()))
        if have:
            out_l, _, li = ctx.encode_files(files, level=level)
            row.update(scaled=int((li["gain"] != 1).sum()), peak_in_max=float(li["peakIn"].max()), peak_out_max=float(li["peakOut"].max()))
        tp, tl = [], []
        for _ in range(a.iters):
            t = time.perf_counter(); ctx.encode_files(files); tp.append(time.perf_counter() - t)
            if have:
                t = time.perf_counter(); ctx.encode_files(files, level=level); tl.append(time.perf_counter() - t)
        row.update(plain_s=float(np.median(tp)), plain_min_s=min(tp), plain_max_s=max(tp))
        if have:
            row.update(level_s=float(np.median(tl)), level_min_s=min(tl), level_max_s=max(tl),
                       level_minus_plain_s=float(np.median(tl) - np.median(tp)))
        row["d2d_copy_s"] = d2d_copy_s(row["out_samples"], a.iters)
        res[w] = row
    return res


def host_composition(ctx, files):
    mono, rates = [], []
    if R.parse(files[0])[1].get("sampleFormat") == R.IMA:
        mono = ctx.wav_decode(files)
        rates = [D.wav_parse(f)["rate"] for f in files]
    else:
        for f in files:
            st, m, d = R.decode(f)
            mono.append(m)
            rates.append(d["rate"])
    return ctx.encode_streams_at(mono, rates)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--workloads", default="256x10s_s16_stereo_44k,1x180s_s16_stereo_44k,256x10s_ima_mono_22k")
    ap.add_argument("--flac", action="store_true")
    ap.add_argument("--flac-seconds", type=int, default=60)
    ap.add_argument("--flac-files", default="1,16,256")
    ap.add_argument("--level", choices=["fit", "gain"])
    ap.add_argument("--ceiling", type=float, default=0.25)
    a = ap.parse_args()
    ctx = D.Context(0)
    if a.level:
        res = level_mode(ctx, a)
        ctx.close()
        print(json.dumps(dict(tool="encode_files_bench", mode="level", level=a.level, lib=os.path.basename(D.lib_path()), results=res)))
        return 0
    if a.flac:
        res = flac_mode(ctx, a)
        ctx.close()
        print(json.dumps(dict(tool="encode_files_bench", mode="flac", results=res)))
        return 0
    res = {}
    for w in a.workloads.split(","):
        files = workload(w)
        fused = lambda: ctx.encode_files(files)                          # noqa: E731
        host = lambda: host_composition(ctx, files)                      # noqa: E731
        out, info = fused()
        want = host()
        tf, th = [], []
        for _ in range(a.iters):
            t = time.perf_counter(); out, info = fused(); tf.append(time.perf_counter() - t)
            t = time.perf_counter(); want = host(); th.append(time.perf_counter() - t)
        n_out = int(info["nSamples"].sum())
        res[w] = dict(files=len(files), mb_in=sum(len(f) for f in files) / 1e6, out_samples=n_out,
                      walk=sorted(set(int(x) for x in info["walk"])), encode_files_s=float(np.median(tf)),
                      host_composition_s=float(np.median(th)), speedup=float(np.median(th) / np.median(tf)),
                      encode_files_out_per_s=n_out / float(np.median(tf)), bytes_equal=out == want)
    ctx.close()
    print(json.dumps(dict(tool="encode_files_bench", results=res)))


if __name__ == "__main__":
    sys.exit(main())
