#!/usr/bin/env python3
"""OS93a Type 1 beside the layouts the reference can write, on the committed recordings (tests/golden/encoder_golden.npz)
at the default parameters: bytes of 0x9301 Type 1 (dcs_encode93a_streams), 0x9301 Type 0 and 0x9302 Type 1
(dcs_encode93_streams), and the waveform SNR of the first two after decoding each on the GPU for nFrames + 1 frames at
volume, mixing level and channel volume 0xFF -- the sweep's measure (INTEGRATION.md "Sweeping"): q = clamp(rint(x * 32768)),
d = decoded[k + 16], exact integer sums; beside the plain SNR the gain sumCross / sumSrcSq and the SNR with that gain
taken out, since every OS93a decode comes out inverted.  Type 0's sums are also taken from dcs_encode_sweep itself and
must agree.
--rates: the same at other bit rates, so that the two can be compared at equal bytes.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sums(ctx, D, os_, stream, x):
    pcm, err, _ = ctx.decode_streams([(os_, stream, 255, 0xFF)], extra_frames=1)
    assert not err.any()
    d = pcm.reshape(-1).astype(np.int64)[16:16 + len(x)]
    q = np.clip(np.rint(x.astype(np.float64) * 32768), -32768, 32767).astype(np.int64)
    return int((q * q).sum()), int((d * d).sum()), int((q * d).sum())


def snr(s):
    src, dec, cross = s
    e = src + dec - 2 * cross
    return None if e == 0 or src == 0 else round(10 * np.log10(src / e), 2)


def gain_snr(s):
    """the least-squares gain of the decode against the source (sumCross / sumSrcSq; OS93a decodes inverted: it is negative),
    and the SNR once that gain is taken out"""
    src, dec, cross = s
    if src == 0 or dec * src == cross * cross:
        return None, None
    return round(cross / src, 4), round(10 * np.log10(cross * cross / (src * dec - cross * cross)), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rates", type=int, nargs="*", default=[128000])
    a = ap.parse_args()
    import dcsexplorer_amd as D
    rec = np.load(os.path.join(ROOT, "tests", "golden", "encoder_golden.npz"))
    pcm, seen = [], set()
    for k in sorted(k for k in rec.files if k.endswith("/pcm")):
        x = np.ascontiguousarray(rec[k]).reshape(-1)
        if x.tobytes() not in seen:
            seen.add(x.tobytes())
            pcm.append((x.astype(np.float32) / np.float32(32768)) if x.dtype == np.int16 else x.astype(np.float32))
    ctx = D.Context(0)
    out = dict(build_id=D.build_id(), recordings=len(pcm), frames=[(len(x) + 239) // 240 for x in pcm], rates={})
    for rate in a.rates:
        t1, _, infa = ctx.encode93a_streams(pcm, D.FMT_93A_T1, targetBitRate=rate)
        t0, _ = ctx.encode93_streams(pcm, D.OS93A, D.FMT_93_T0, targetBitRate=rate)
        b1, _ = ctx.encode93_streams(pcm, D.OS93B, D.FMT_93B_T1, targetBitRate=rate)
        wild, winfo, _ = ctx.encode93a_streams(pcm, None, targetBitRate=rate)
        _, res = ctx.encode_sweep(pcm, [D.encode93_params(D.OS93A, D.FMT_93_T0, targetBitRate=rate)], None, measure=True, streams=False)
        rows = []
        for k, x in enumerate(pcm):
            s1, s0 = sums(ctx, D, D.OS93A, t1[k], x), sums(ctx, D, D.OS93A, t0[k], x)
            same = bool(res[k]["measured"]) and (int(res[k]["sumSrcSq"]), int(res[k]["sumDecSq"]), int(res[k]["sumCross"])) == s0
            rows.append(dict(t1_bytes=len(t1[k]), t0_bytes=len(t0[k]), b_t1_bytes=len(b1[k]), wildcard_bytes=len(wild[k]),
                             wildcard_type=int(winfo[k]["formatType"]), t1_snr_db=snr(s1), t0_snr_db=snr(s0),
                             t1_gain_snr=gain_snr(s1), t0_gain_snr=gain_snr(s0), t0_sums_equal_sweep=same,
                             t1_fits=int(infa[k]["frameBits"]) <= int(infa[k]["budgetBits"])))
        out["rates"][str(rate)] = rows
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
