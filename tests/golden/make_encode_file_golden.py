#!/usr/bin/env python3
"""Generates dcs_encode_files' fixtures from the reference's own code (build container only; outputs are data):
  encode_file_golden.{json,npz}  every case of tests/wav_cases.py (cases(), the 180 s file with its sha256 only, then
                                 float_edge_cases()) run through the
                                 reference's DCSEncoder::EncodeFile (encode_file/ef_driver.cpp), linked with the vendored
                                 libnyquist and libsamplerate: NyquistIO::Load's result (its float bits for the short cases,
                                 the sha256 of all of them, or its exception text) and EncodeFile's stream or error text
libnyquist is built with its own CMake (-G Ninja, LIBNYQUIST_BUILD_EXAMPLE=OFF, whose example target has no sources) and
linked whole.  libsamplerate's best-quality slot holds the library's default table, as in make_resample_golden.py, so the
fixture bytes are what dcs_encode_files writes with a NULL filter.  Every case is also run in a build with
-fsanitize=bounds,shift,float-cast-overflow (the encoder's sources, libsamplerate and the driver), as make_encode_golden.py
screens its cases; the reports are recorded per case, and a case whose run crashes is recorded as such.  Everything is
compiled into a temporary directory.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import wav_cases as W                   # noqa: E402
from oracle import flacref                      # noqa: E402  (libnyquist's build: one recipe)
import make_resample_golden as MR       # noqa: E402  (stand_in: the best-quality slot)

HERE = os.path.join(ROOT, "tests", "golden")
REF = "/root/reference"
NQ = os.path.join(REF, "libnyquist")
LSR = os.path.join(REF, "libsamplerate", "src")
KEEP_VALUES = 1200          # cases with at most this many values keep Load's float bits; all keep the sha256
KEEP_STREAM = 4096          # streams up to this many bytes are kept whole
VERSIONS = ((0x9400, -1, -1), (0x9302, -1, -1))


def build(tmp, nq_lib, coeffs, inc, extra=()):
    tag = "san" if extra else "plain"
    d = os.path.join(tmp, tag)
    os.makedirs(d, exist_ok=True)
    open(os.path.join(d, "high_qual_coeffs.h"), "w").write(MR.stand_in(coeffs, inc))
    objs = []
    for src in ("samplerate.c", "src_sinc.c", "src_linear.c", "src_zoh.c"):
        o = os.path.join(d, src + ".o")
        subprocess.check_call(["gcc", "-O2", "-w", "-I" + d, "-I" + LSR, "-c", os.path.join(LSR, src), "-o", o] + list(extra))
        objs.append(o)
    exe = os.path.join(d, "ef_driver")
    enc = os.path.join(REF, "DCSEncoder")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-w", "-include", os.path.join(HERE, "encoder", "enc_shim.h"),
                           "-I" + enc, "-I" + LSR, "-I" + os.path.join(NQ, "include"), "-o", exe,
                           os.path.join(HERE, "encode_file", "ef_driver.cpp"), os.path.join(enc, "DCSEncoder.cpp"),
                           os.path.join(enc, "DCSEncodeFile.cpp"), os.path.join(REF, "DCSDecoder", "DCSDecoder.cpp"),
                           os.path.join(REF, "DCSDecoder", "DCSDecoderNative.cpp")] + objs + list(extra)
                          + ["-Wl,--whole-archive", nq_lib, "-Wl,--no-whole-archive", "-lpthread", "-lm"])
    return exe


def run(exe, path, tmp, fv, typ, sub):
    st, f32 = os.path.join(tmp, "out.stream"), os.path.join(tmp, "out.f32")
    for p in (st, f32):
        if os.path.exists(p):
            os.remove(p)
    r = subprocess.run([exe, path, st, f32, "%x" % fv, str(typ), str(sub)], capture_output=True, text=True, errors="replace",
                       timeout=600)
    res = dict(rc=r.returncode, load=None, encode=None)
    for line in r.stdout.splitlines():
        if line.startswith("load "):
            res["load"] = line[5:].replace(path, "case.wav")
        elif line.startswith("encode "):
            res["encode"] = line[7:].replace(path, "case.wav")
    res["values"] = open(f32, "rb").read() if os.path.exists(f32) else None
    res["stream"] = open(st, "rb").read() if os.path.exists(st) else None
    res["ubsan"] = sorted({("shift" if "shift" in l else "bounds" if "out of bounds" in l or "index" in l else "float-cast")
                           for l in r.stderr.splitlines() if "runtime error" in l})
    return res


def main():
    import dcsexplorer_amd as D
    coeffs, inc = D.resample_filter_default()
    # (the float-edge cases come last, so the entries before them keep their places and their bytes)
    cases = W.cases() + [("long_180s_s16_stereo_44100", W.long_wav())] + W.float_edge_cases()
    meta, arrays = [], {}
    with tempfile.TemporaryDirectory() as tmp:
        nq_lib = flacref.build_libnyquist(NQ, os.path.join(tmp, "nq"))
        plain = build(tmp, nq_lib, coeffs, inc)
        san = build(tmp, nq_lib, coeffs, inc, extra=["-fsanitize=bounds,shift,float-cast-overflow"])
        for name, data in cases:
            path = os.path.join(tmp, "case.wav")           # NyquistIO picks its decoder by the extension
            open(path, "wb").write(data)
            entry = dict(name=name, file_sha256=hashlib.sha256(data).hexdigest(), runs=[])
            for fv, typ, sub in VERSIONS:
                if fv != 0x9400 and name.startswith("long_"):
                    continue
                s = run(san, path, tmp, fv, typ, sub)
                p = run(plain, path, tmp, fv, typ, sub)
                rec = dict(version=fv, type=typ, subType=sub, rc=p["rc"], load=p["load"], encode=p["encode"], ubsan=s["ubsan"],
                           san_rc=s["rc"])
                if p["stream"] is not None:
                    rec["bytes"] = len(p["stream"])
                    rec["sha256"] = hashlib.sha256(p["stream"]).hexdigest()
                    if len(p["stream"]) <= KEEP_STREAM:
                        arrays["%s/%x/stream" % (name, fv)] = np.frombuffer(p["stream"], np.uint8)
                if fv == 0x9400 and p["values"] is not None:
                    entry["n_values"] = len(p["values"]) // 4
                    entry["values_sha256"] = hashlib.sha256(p["values"]).hexdigest()
                    if entry["n_values"] <= KEEP_VALUES:
                        arrays[name + "/values"] = np.frombuffer(p["values"], "<f4")
                entry["runs"].append(rec)
            meta.append(entry)
            print(name, [(r["load"], r["encode"], r["ubsan"], r["rc"]) for r in entry["runs"]][0])
    np.savez_compressed(os.path.join(HERE, "encode_file_golden.npz"), **arrays)
    json.dump(dict(cases=meta, keep_values=KEEP_VALUES, keep_stream=KEEP_STREAM), open(os.path.join(HERE, "encode_file_golden.json"), "w"),
              indent=0)


if __name__ == "__main__":
    sys.exit(main())
