#!/usr/bin/env python3
"""Build-container tool: the numeric constants of the 1994+ ENCODER that the decode side does not already carry,
re-emitted as dcsexplorer_amd/csrc/dcs_enc_tables.h (bit patterns, so the library depends on no host libm or decimal
parser).  Runs only where /root/reference is mounted; its output is committed.  No reference code is copied: these
are numbers of the format and of the reference encoder's analysis transform.

Provenance (file:line in /root/reference/DCSEncoder/DCSEncoder.cpp):
    PI :37   bandSampleNorm94 :63-66   scalingFactors :78-142   bandShare :887
    windowFunc :1008-1011   twiddleCoefficients :1134-1151   DualFFT coefficients :1392-1406 (computed, see below)

What is DERIVED instead of extracted, and checked equal to the reference's literal here:
    scalingFactors[j] == kScaleMant[j & 3] >> (15 - (j >> 2))          (dcs_tables.h, the decoder's mantissas)
    xlat02/35/6F      == the decoder's kXlatB* with the two bytes swapped (width << 8 | scale adjust)
    preAdjMap0/3      == kPreAdjSub0/3;  bandSampleCounts94 == kBandCount94
    the 1994+ frame-header and sample codebooks are the inverses of the decode trees (the encoder goldens pin them)
The twiddles are NOT the decoder's kFftCoef / 32768: e.g. -0.0245361f is not -804/32768 in float, so they are extracted.

The 896 DualFFT coefficients are what the reference computes at run time: theta = -2*PI*(float)j/(float)m in float
arithmetic, then cosf(theta), sinf(theta).  They are evaluated here with the C library's own cosf/sinf (ctypes) -- the
same functions the reference's build calls -- and emitted as bit patterns."""
import ctypes
import ctypes.util
import os
import re
import struct
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/DCSEncoder/DCSEncoder.cpp"
F32 = np.float32


def strip_comments(s):
    s = re.sub(r'//[^\n]*', '', s)
    return re.sub(r'/\*.*?\*/', '', s, flags=re.S)


def body(src, name):
    m = re.search(r'\b' + re.escape(name) + r'\s*\[[^\]]*\]\s*=\s*\{(.*?)\};', src, re.S)
    return m.group(1)


def f32_of_decimal(text):
    """the float a C float literal denotes: the correctly rounded binary32 of the decimal (checked against numpy's
    double-then-float path, which could double-round)"""
    v = F32(float(text))
    exact = Fraction(text)
    lo, hi = np.nextafter(v, F32(-np.inf)), np.nextafter(v, F32(np.inf))
    for w in (lo, hi):
        assert abs(Fraction(float(w)) - exact) >= abs(Fraction(float(v)) - exact), text
    return v


def bits(v):
    return struct.unpack("<I", struct.pack("<f", float(v)))[0]


def dcs_table(name):
    src = open(os.path.join(ROOT, "dcsexplorer_amd", "csrc", "dcs_tables.h")).read()
    return [int(t, 0) for t in re.findall(r'0x[0-9a-fA-F]+|\d+', body(src, name))]


def main():
    src = strip_comments(open(REF).read())
    pi = f32_of_decimal(re.search(r'PI\s*=\s*([0-9.]+)f', src).group(1))
    window = [f32_of_decimal(t) for t in re.findall(r'-?\d+\.\d+', body(src, "windowFunc"))]
    twiddle = [f32_of_decimal(t) for t in re.findall(r'-?\d+\.\d+', body(src, "twiddleCoefficients"))]
    share = [int(t) for t in re.findall(r'\d+', body(src, "bandShare"))]
    norm = [F32(int(a)) / F32(int(b)) for a, b in re.findall(r'(\d+)\.0f/(\d+)', body(src, "bandSampleNorm94"))]
    scale = [int(t) for t in re.findall(r'\d+', body(src, "scalingFactors"))]
    assert len(window) == 16 and len(twiddle) == 128 and len(share) == 16 and len(norm) == 16 and len(scale) == 64

    # derived from the decode side, checked equal to the literal
    mant = dcs_table("kScaleMant")
    assert scale == [mant[j & 3] >> (15 - (j >> 2)) for j in range(64)]
    for enc, dec in (("xlat02", "kXlatB02"), ("xlat35", "kXlatB35"), ("xlat6F", "kXlatB6F")):
        lit = [int(t, 0) for t in re.findall(r'0x[0-9a-fA-F]+', body(src, enc))]
        assert lit == [((v & 0xFF) << 8) | (v >> 8) for v in dcs_table(dec)], enc
    assert [int(t) for t in re.findall(r'\d+', body(src, "preAdjMap0"))] == dcs_table("kPreAdjSub0")
    assert [int(t) for t in re.findall(r'\d+', body(src, "preAdjMap3"))] == dcs_table("kPreAdjSub3")
    assert [int(t) for t in re.findall(r'\d+', body(src, "bandSampleCounts94"))] == dcs_table("kBandCount94")
    der = [F32(v if v < 0x8000 else v - 0x10000) / F32(32768) for v in dcs_table("kFftCoef")]
    assert not all(any(bits(d) == bits(t) for d in der) for t in twiddle)     # (why the twiddles are extracted)

    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.cosf.restype = libm.sinf.restype = ctypes.c_float
    libm.cosf.argtypes = libm.sinf.argtypes = [ctypes.c_float]
    coeff = []
    for s in range(1, 8):
        m = 1 << s
        for _k in range(0, 128, m):
            for j in range(m // 2):
                theta = F32(-2) * pi * F32(j) / F32(m)
                coeff += [F32(libm.cosf(float(theta))), F32(libm.sinf(float(theta)))]
    assert len(coeff) == 896

    def arr(name, ctype, vals, per, fmt):
        lines = ["static const %s %s[%d] = {" % (ctype, name, len(vals))]
        for i in range(0, len(vals), per):
            lines.append("    " + ", ".join(fmt(v) for v in vals[i:i + per]) + ",")
        return "\n".join(lines) + "\n};\n"

    hx = lambda v: "0x%08xu" % bits(v)            # noqa: E731
    out = ["// GENERATED by tools/extract_enc_tables.py -- do not edit.",
           "// Numeric constants of the 1994+ encoder's analysis transform and rate model, as float bit patterns",
           "// (see the tool for provenance and for what is derived from dcs_tables.h instead).",
           "#pragma once", "#include <stdint.h>", "",
           "// window over the first and last 16 input samples of a frame",
           arr("kEncWindowBits", "uint32_t", window, 8, hx),
           "// twiddle (cos, sin) pairs of the post-FFT fold",
           arr("kEncTwiddleBits", "uint32_t", twiddle, 8, hx),
           "// DualFFT coefficients: (cosf, sinf)(-2*PI*j/m) for stage s = 1..7, m = 2^s, k = 0..127 step m, j < m/2",
           arr("kEncFftBits", "uint32_t", coeff, 8, hx),
           "// per-band RMS normalisation 16/n of the stream statistics",
           arr("kEncBandNormBits", "uint32_t", norm, 8, hx),
           "// rate model: relative bit share per band",
           arr("kEncBandShare", "uint8_t", share, 16, str)]
    open(os.path.join(ROOT, "dcsexplorer_amd", "csrc", "dcs_enc_tables.h"), "w").write("\n".join(out))
    print("dcs_enc_tables.h: window 16, twiddle 128, fft 896, norm 16, share 16")


if __name__ == "__main__":
    main()
