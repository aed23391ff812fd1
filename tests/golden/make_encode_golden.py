#!/usr/bin/env python3
"""Generates tests/golden/encode_golden.npz + encode_golden.json: PCM in, the reference ENCODER's stream bytes out
(DCSEncoder::OpenStream(31250) / WriteStream(float) / CloseStream through encoder/enc_pcm_driver.cpp), for the 1994+
format in every fixed layout and the wildcard, over a sweep of CompressionParams and a set of edge signals.

Build container only.  The encoder is the checker `make -C oracle encref` builds from where it lies under /root/reference
(oracle/_ref/dcs_encref: g++ -O2, encoder/enc_shim.h, the pass-through resampler encoder/enc_resample_stub.c), and
its second build with -fsanitize=bounds,shift,float-cast-overflow (oracle/_ref/dcs_encref_san) screens every case:
a case with a bounds or float-cast report is DROPPED (the reference's bytes then depend on its binary layout); shift
reports are kept -- the 1 << bitsPerBand of CompressStream runs as x86 shl, which masks the count, and the library
defines that rule ("Encoding").  Outputs are data and travel to the GPU box.

npz keys: <signal>/pcm per input signal (int16 where every sample is a 16-bit value, which the test divides by 32768,
else float32), and <case>/stream (uint8) for the cases whose stream is at most KEEP_BYTES long.  json: per case the
params, the variant asked for, the reference's winner, the stream's length, header and sha256 -- the bytes of every stream are
pinned by the digest, the small ones are also kept whole (the fixture stays a few hundred kB)."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.join(ROOT, "tests", "golden", "encoder")
FMTS = {"wild": (-1, -1), "T0s0": (0, 0), "T0s3": (0, 3), "T1s0": (1, 0), "T1s3": (1, 3)}
KEEP_BYTES = 4096
DEFAULTS = dict(powerBandCutoff=0.97, targetBitRate=128000, minimumDynamicRange=10 / 32768, maximumQuantizationError=10 / 32768)


def build(sanitize):
    """the reference encoder (sanitize=False) or its UBSan build, as oracle/Makefile's `encref` target makes them"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "encref"])
    exe = os.path.join(ROOT, "oracle", "_ref", "dcs_encref_san" if sanitize else "dcs_encref")
    if not os.path.exists(exe):
        raise RuntimeError("%s was not built (the reference encoder sources are missing)" % exe)
    return exe


def recording(variant, n_frames=128):
    """the shape of encoder/enc_driver.cpp's signal (rising tone over harmonics, tremolo chord, noise burst, near
    silence, decaying low note), 16-bit valued"""
    n = n_frames * 240
    i = np.arange(n, dtype=np.float64)
    t, u = i / 31250.0, i / n
    pitch = 1.0 + 0.19 * variant
    rng = np.random.default_rng(0xE4C0DE + variant)
    noise = rng.uniform(-1, 1, n)
    rich = sum(np.sin(2 * np.pi * 173.0 * pitch * h * t + 0.7 * h) / h for h in range(1, 25))
    v = np.where(u < 0.25, 0.40 * np.sin(2 * np.pi * pitch * (200.0 + 3800.0 * u * 4) * t) + 0.18 * rich + 0.16 * noise,
        np.where(u < 0.50, (0.30 * np.sin(2 * np.pi * 440.0 * pitch * t) + 0.25 * np.sin(2 * np.pi * 1320.0 * pitch * t) + 0.15 * rich)
                 * (0.6 + 0.4 * np.sin(2 * np.pi * 6.0 * t)) + 0.14 * noise,
        np.where(u < 0.65, 0.40 * noise,
        np.where(u < 0.75, 0.0008 * noise,
                 0.70 * np.exp(-(u - 0.75) * 12.0) * (np.sin(2 * np.pi * 110.0 * pitch * t) + 0.4 * rich) + 0.10 * noise))))
    return np.clip(np.rint(v * 30000.0), -32768, 32767).astype(np.int16)


def edge_signals():
    rng = np.random.default_rng(0xED6E)
    i16 = lambda a: np.clip(np.rint(a * 32768.0), -32768, 32767).astype(np.int16)      # noqa: E731
    t = np.arange(30000) / 31250.0
    return {
        "len1": i16(rng.uniform(-0.5, 0.5, 1)),
        "len239": i16(rng.uniform(-0.5, 0.5, 239)),
        "len240": i16(rng.uniform(-0.5, 0.5, 240)),
        "len241": i16(rng.uniform(-0.5, 0.5, 241)),
        "silence": np.zeros(2400, np.int16),
        "dc": np.full(4800, 8192, np.int16),
        "square": np.where((np.arange(9600) // 150) & 1, 1.0, -1.0).astype(np.float32),
        "noise_fs": rng.uniform(-1.0, 1.0, 9600).astype(np.float32),
        "sine40": i16(0.5 * np.sin(2 * np.pi * 40.0 * t)),
        "near_silent": i16(rng.integers(-6, 7, 12000) / 32768.0),
        "float_tones": (0.3 * np.sin(2 * np.pi * 523.25 * t[:14400]) + 0.2 * np.sin(2 * np.pi * 3001.7 * t[:14400])
                        + 0.05 * rng.standard_normal(14400)).astype(np.float32),
    }


def cases():
    """(name, signal key, fmt key, params)"""
    out = []
    for v in range(4):
        for fk in FMTS:
            out.append(("rec%d-%s" % (v, fk), "rec%d" % v, fk, {}))
    for rate in (16000, 32000, 64000, 256000):
        for fk in ("wild", "T1s3", "T0s0"):
            out.append(("rec1-rate%d-%s" % (rate // 1000, fk), "rec1", fk, dict(targetBitRate=rate)))
    for cut in (0.9, 1.0):
        for fk in ("wild", "T1s0"):
            out.append(("rec2-cut%s-%s" % (cut, fk), "rec2", fk, dict(powerBandCutoff=cut)))
    out.append(("rec3-mindr0-wild", "rec3", "wild", dict(minimumDynamicRange=0.0)))
    out.append(("rec3-mindr0-T1s3", "rec3", "T1s3", dict(minimumDynamicRange=0.0)))
    out.append(("rec0-maxqe4-wild", "rec0", "wild", dict(maximumQuantizationError=4 / 32768)))
    out.append(("rec0-maxqe4-T0s3", "rec0", "T0s3", dict(maximumQuantizationError=4 / 32768)))
    for key in edge_signals():
        for fk in ("wild", "T0s0", "T1s0", "T1s3"):
            out.append(("%s-%s" % (key, fk), key, fk, {}))
    out.append(("near_silent-mindr0-wild", "near_silent", "wild", dict(minimumDynamicRange=0.0)))
    out.append(("sine40-rate8-T1s3", "sine40", "T1s3", dict(targetBitRate=8000)))
    return out


def run(exe, pcm, fk, p, tmp):
    src, dst = os.path.join(tmp, "in.f32"), os.path.join(tmp, "out.bin")
    x = (pcm.astype(np.float32) / np.float32(32768.0)) if pcm.dtype == np.int16 else pcm.astype(np.float32)
    x.astype("<f4").tofile(src)
    typ, sub = FMTS[fk]
    argv = [exe, src, dst, "9400", str(typ), str(sub), float(np.float32(p["powerBandCutoff"])).hex(), str(p["targetBitRate"]),
            float(np.float32(p["minimumDynamicRange"])).hex(), float(np.float32(p["maximumQuantizationError"])).hex()]
    r = subprocess.run(argv, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s: %s" % (argv, r.stderr))
    return open(dst, "rb").read(), r.stderr


def main():
    signals = {"rec%d" % v: recording(v) for v in range(4)}
    signals.update(edge_signals())
    arrays, meta, dropped = {}, [], []
    with tempfile.TemporaryDirectory() as tmp:
        exe, san = build(False), build(True)
        for name, key, fk, over in cases():
            p = dict(DEFAULTS, **over)
            _, report = run(san, signals[key], fk, p, tmp)
            kinds = sorted({("shift" if "shift" in l else "bounds" if "out of bounds" in l or "index" in l else "float-cast")
                            for l in report.splitlines() if "runtime error" in l})
            if any(k != "shift" for k in kinds):
                dropped.append((name, kinds))
                continue
            stream, _ = run(exe, signals[key], fk, p, tmp)
            sizes = {}
            for k in ("T0s0", "T0s3", "T1s0", "T1s3"):
                if fk == "wild" or fk == k:
                    sizes[k] = len(run(exe, signals[key], k, p, tmp)[0])
            winner = min(sizes, key=lambda k: (sizes[k], list(sizes).index(k)))     # first strictly smallest
            if len(stream) <= KEEP_BYTES:
                arrays[name + "/stream"] = np.frombuffer(stream, dtype=np.uint8)
            if key + "/pcm" not in arrays:
                arrays[key + "/pcm"] = signals[key]
            meta.append(dict(name=name, signal=key, fmt=fk, params={k: float(np.float32(v)) if k != "targetBitRate" else int(v)
                                                                      for k, v in p.items()},
                             winner=[FMTS[winner][0], FMTS[winner][1]], nFrames=(stream[0] << 8) | stream[1], bytes=len(stream),
                             sha256=hashlib.sha256(stream).hexdigest(), header=stream[2:18].hex(),
                             ubsan=kinds))
            print(name, len(stream), "bytes", winner, kinds)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "encode_golden.npz"), **arrays)
    with open(os.path.join(ROOT, "tests", "golden", "encode_golden.json"), "w") as f:
        json.dump(dict(cases=meta, dropped=[dict(name=n, ubsan=k) for n, k in dropped]), f, indent=1)
    print("%d cases, %d dropped: %s" % (len(meta), len(dropped), dropped))


if __name__ == "__main__":
    sys.exit(main())
