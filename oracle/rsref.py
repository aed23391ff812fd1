#!/usr/bin/env python3
"""Builds libsamplerate, UNMODIFIED and where it lies under the reference tree, as checker binaries (test infrastructure):

  oracle/_ref/dcs_rsref_default, dcs_rsref_long, dcs_rsref_big   tests/golden/resample/rs_driver.c over the converter, the
                                  best-quality slot holding the library's default table, the long table of
                                  tests/golden/resample_filters.npz, and big_table() of the default one
  oracle/_ref/dcs_encrate_ref, dcs_encrate_ref_san               tests/golden/resample/enc_rate_driver.cpp: the reference
                                  DCSEncoder over the real converter (default table); the second with
                                  -fsanitize=bounds,shift,float-cast-overflow (host code)
  oracle/_ref/dcs_rsout_default, dcs_rsout_long, dcs_rsout_big   tests/golden/resample/out_rate_driver.c over the converter: int16
                                  at 31 250 Hz to an output rate between libsamplerate's own int16 conversions; the default
                                  table, the long table of tests/golden/decode_rate_golden.npz (on which the flush cap
                                  binds) and big_table() of the default one

The vendored libsamplerate lacks high_qual_coeffs.h, so every build gets a stand-in of ours, generated beside its object
files (never committed), that puts a table of our choice in the best-quality slot; the fastest and medium slots are the
vendored tables.  The tables come from resample_filters.npz, not from the built library, so this needs no libdcs_hip.so.
tests/golden/make_resample_golden.py builds its converters with build_lsr() too: one recipe.

  python3 oracle/rsref.py <reference root> <output directory>
"""
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BINARIES = ("dcs_rsref_default", "dcs_rsref_long", "dcs_rsref_big", "dcs_encrate_ref", "dcs_encrate_ref_san",
            "dcs_rsout_default", "dcs_rsout_long", "dcs_rsout_big")
SANITIZE = "-fsanitize=bounds,shift,float-cast-overflow"
BIG_FACTOR = 4


def vendored(lsr, name):
    """a vendored table: (float32 coefficients, increment), read from its header as data"""
    text = open(os.path.join(lsr, name)).read()
    inc = int(re.search(r"increment\s*:\s*(\d+)", text).group(1))
    body = text[text.index("=", text.index("coeffs [")):]        # "= { increment, { c0, c1, ... } }"
    body = body[body.index("{", body.index("{") + 1) + 1:body.index("}")]
    vals = [float(v) for v in re.findall(r"[-+]?\d*\.\d+(?:[eE][-+]?\d+)?|[-+]?\d+[eE][-+]?\d+", body)]
    return np.array(vals, np.float32), inc


def big_table(coeffs, inc):
    """a table BIG_FACTOR times as dense as `coeffs`: big[4 i + j] = f32(c[i] + j / 4 * (c[i + 1] - c[i])) in f64, then the
    two closing zeros of libsamplerate's layout.  Only + - * / on IEEE doubles, so the bits are the same on every machine."""
    c = np.asarray(coeffs, np.float32).astype(np.float64)
    half = len(c) - 2
    j = np.arange(BIG_FACTOR, dtype=np.float64) / BIG_FACTOR
    body = (c[:half, None] + j[None, :] * (c[1:half + 1] - c[:half])[:, None]).astype(np.float32).reshape(-1)
    return np.concatenate([body, np.zeros(2, np.float32)]), inc * BIG_FACTOR


def stand_in(coeffs, inc):
    """high_qual_coeffs.h of ours: the best-quality slot holds `coeffs`"""
    vals = ",\n".join(float(v).hex() for v in coeffs.astype(np.float64))
    return ("static const struct slow_high_qual_coeffs_s\n{\tint increment ;\n\tcoeff_t coeffs [%d] ;\n} slow_high_qual_coeffs =\n"
            "{\t%d,\n{\n%s\n}\n} ;\n" % (len(coeffs), inc, vals))


def build_lsr(tmp, name, coeffs, inc, driver, cxx=False, extra=(), ref="/root/reference", exe=None):
    """compile the vendored converter in tmp/name with `coeffs` in its best-quality slot and link it with `driver`
    (cxx: with the reference DCSEncoder as well) -> the program's path (tmp/name/drv unless `exe` names another)"""
    lsr = os.path.join(ref, "libsamplerate", "src")
    d = os.path.join(tmp, name)
    os.makedirs(d, exist_ok=True)
    open(os.path.join(d, "high_qual_coeffs.h"), "w").write(stand_in(coeffs, inc))
    objs = []
    for src in ("samplerate.c", "src_sinc.c", "src_linear.c", "src_zoh.c"):
        o = os.path.join(d, src + ".o")
        subprocess.check_call(["gcc", "-O2", "-w", "-I" + d, "-I" + lsr, "-c", os.path.join(lsr, src), "-o", o] + list(extra))
        objs.append(o)
    exe = exe or os.path.join(d, "drv")
    if cxx:
        enc = os.path.join(GOLDEN, "encoder")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-w", "-include", os.path.join(enc, "enc_shim.h"),
                               "-I" + os.path.join(ref, "DCSEncoder"), "-I" + lsr, "-o", exe, driver,
                               os.path.join(ref, "DCSEncoder", "DCSEncoder.cpp"), os.path.join(ref, "DCSDecoder", "DCSDecoder.cpp"),
                               os.path.join(ref, "DCSDecoder", "DCSDecoderNative.cpp")] + objs + list(extra) + ["-lpthread", "-lm"])
    else:
        subprocess.check_call(["gcc", "-O2", "-w", "-I" + lsr, "-o", exe, driver] + objs + ["-lm"])
    return exe


def npz_table(name):
    f = np.load(os.path.join(GOLDEN, "resample_filters.npz"))
    return f[name + "/coeffs"], int(f[name + "/increment"])


def out_long_table():
    """the long table of the output-rate fixtures: 400 input samples a side, so that the flush cap binds from 44.1 kHz up"""
    f = np.load(os.path.join(GOLDEN, "decode_rate_golden.npz"))
    return f["long/coeffs"], int(f["long/increment"])


def main(argv):
    if len(argv) != 3:
        sys.stderr.write(__doc__)
        return 2
    ref, out = argv[1], os.path.abspath(argv[2])
    work = os.path.join(out, "rsref_build")
    default = npz_table("default")
    rs = os.path.join(GOLDEN, "resample", "rs_driver.c")
    enc = os.path.join(GOLDEN, "resample", "enc_rate_driver.cpp")
    rsout = os.path.join(GOLDEN, "resample", "out_rate_driver.c")
    jobs = [("default", default, rs, False, ()), ("long", npz_table("long"), rs, False, ()), ("big", big_table(*default), rs, False, ()),
            ("enc", default, enc, True, ()), ("encsan", default, enc, True, (SANITIZE,)),
            ("out_default", default, rsout, False, ()), ("out_long", out_long_table(), rsout, False, ()),
            ("out_big", big_table(*default), rsout, False, ())]
    assert len(jobs) == len(BINARIES)
    for (name, table, driver, cxx, extra), exe in zip(jobs, BINARIES):
        build_lsr(work, name, table[0], table[1], driver, cxx=cxx, extra=list(extra), ref=ref, exe=os.path.join(out, exe))
    print("built oracle/_ref/%s from %s/libsamplerate" % (", ".join(BINARIES), ref))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
