#!/usr/bin/env python3
"""Generates tests/golden/encode93_golden.npz + encode93_golden.json: the reference ENCODER's OS93 streams
(formatVersion 0x9301 / 0x9302, CompressFrame93b) for the inputs of encode_golden.npz, through the same driver
(encoder/enc_pcm_driver.cpp) and the same builds as make_encode_golden.py (`make -C oracle encref`): g++ -O2, and a second time with
-fsanitize=bounds,shift,float-cast-overflow to screen every case (a bounds or float-cast report drops the case; shift
reports are kept, the library's masked-shift rule covers them).

Build container only.  The inputs are read from encode_golden.npz, so the fixture holds streams only; a signal missing
there is an error.  One case encodes the longest stream the format allows (recording(1, 65535) of make_encode_golden.py,
recomputed by the test), and keeps its length, header and sha256 only.

Per case: the version and type asked for, the params, the reference's winner (the first strictly smallest of the types
tried), the stream's length, header and sha256, the UBSan report kinds, and `rules`: how often the library's Keep +15
rule (tests/enc93_ref.py) fired in the layouts tried -- a case where it fires cannot equal the reference's bytes, and none
does; tests/test_encode93_host.py pins the rule on its own."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_encode_golden as G         # noqa: E402
import enc93_ref as R                  # noqa: E402

FMTS = {"b-wild": (0x9302, -1), "b-T0": (0x9302, 0), "b-T1": (0x9302, 1), "a-T0": (0x9301, 0), "a-wild": (0x9301, -1)}
KEEP_BYTES = 4096
LONG = ("long65535", 1, 65535)         # (signal name, recording variant, frames)


def cases():
    """(name, signal key, fmt key, params)"""
    sigs = ["rec%d" % v for v in range(4)] + list(G.edge_signals())
    out = [("%s-%s" % (s, fk), s, fk, {}) for s in sigs for fk in FMTS]
    for rate in (8000, 16000, 32000, 64000, 256000):
        for fk in ("b-wild", "b-T1", "a-T0"):
            out.append(("rec1-rate%d-%s" % (rate // 1000, fk), "rec1", fk, dict(targetBitRate=rate)))
    for cut in (0.0, 0.9, 1.0):
        for fk in ("b-wild", "b-T1"):
            out.append(("rec2-cut%s-%s" % (cut, fk), "rec2", fk, dict(powerBandCutoff=cut)))
    for fk in ("b-wild", "b-T1", "a-T0"):
        out.append(("rec0-maxqe3-%s" % fk, "rec0", fk, dict(maximumQuantizationError=3 / 32768)))
    out.append(("noise_fs-maxqe1-b-wild", "noise_fs", "b-wild", dict(maximumQuantizationError=1 / 32768)))
    out.append(("sine40-rate8-b-T1", "sine40", "b-T1", dict(targetBitRate=8000)))
    out.append(("%s-b-wild" % LONG[0], LONG[0], "b-wild", {}))
    return out


def run(exe, x, version, typ, p, tmp):
    src, dst = os.path.join(tmp, "in.f32"), os.path.join(tmp, "out.bin")
    x.astype("<f4").tofile(src)
    argv = [exe, src, dst, "%x" % version, str(typ), "-1", float(np.float32(p["powerBandCutoff"])).hex(), str(p["targetBitRate"]),
            float(np.float32(p["minimumDynamicRange"])).hex(), float(np.float32(p["maximumQuantizationError"])).hex()]
    r = subprocess.run(argv, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s: %s" % (argv, r.stderr))
    return open(dst, "rb").read(), r.stderr


def main():
    src = np.load(os.path.join(HERE, "encode_golden.npz"))
    arrays, meta, dropped = {}, [], []

    def signal(key):
        if key == LONG[0]:
            return G.recording(LONG[1], LONG[2])
        if key + "/pcm" not in src.files:
            raise KeyError("signal %r is not in encode_golden.npz" % key)
        return src[key + "/pcm"]

    with tempfile.TemporaryDirectory() as tmp:
        exe, san = G.build(False), G.build(True)
        for name, key, fk, over in cases():
            p = dict(G.DEFAULTS, **over)
            version, typ = FMTS[fk]
            pcm = signal(key)
            x = (pcm.astype(np.float32) / np.float32(32768.0)) if pcm.dtype == np.int16 else pcm.astype(np.float32)
            _, report = run(san, x, version, typ, p, tmp)
            kinds = sorted({("shift" if "shift" in l else "bounds" if "out of bounds" in l or "index" in l else "float-cast")
                            for l in report.splitlines() if "runtime error" in l})
            if any(k != "shift" for k in kinds):
                dropped.append((name, kinds))
                continue
            stream, _ = run(exe, x, version, typ, p, tmp)
            sizes = {t: len(run(exe, x, version, t, p, tmp)[0]) for t in R.layouts(version, typ)}
            winner = min(sizes, key=lambda t: (sizes[t], list(sizes).index(t)))        # first strictly smallest
            fired = 0
            if key != LONG[0]:
                fired = R.encode(pcm, version, typ, **p)[3]
            if len(stream) <= KEEP_BYTES:
                arrays[name + "/stream"] = np.frombuffer(stream, dtype=np.uint8)
            meta.append(dict(name=name, signal=key, version=version, type=typ,
                             params={k: float(np.float32(v)) if k != "targetBitRate" else int(v) for k, v in p.items()},
                             winner=winner, nFrames=(stream[0] << 8) | stream[1], bytes=len(stream),
                             sha256=hashlib.sha256(stream).hexdigest(), header=stream[2:18].hex(), ubsan=kinds, rules=fired))
            print(name, len(stream), "bytes, winner", winner, kinds, "rule fired" if fired else "")
    np.savez_compressed(os.path.join(HERE, "encode93_golden.npz"), **arrays)
    with open(os.path.join(HERE, "encode93_golden.json"), "w") as f:
        json.dump(dict(long=dict(signal=LONG[0], recording=LONG[1], frames=LONG[2]), cases=meta,
                       dropped=[dict(name=n, ubsan=k) for n, k in dropped]), f, indent=1)
    print("%d cases, %d dropped: %s; the Keep +15 rule fired in %d" % (len(meta), len(dropped), dropped,
                                                                       sum(c["rules"] > 0 for c in meta)))


if __name__ == "__main__":
    sys.exit(main())
