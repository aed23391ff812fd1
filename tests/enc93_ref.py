"""numpy restatement of the OS93 encoder (test infrastructure, like enc_ref.py: not part of the product).

The analysis transform is enc_ref's (the same for every format).  What this adds, in float32 and in the reference's order
(DCSEncoder.cpp: Frame::Frame :2535-2565, CloseStream :717-850, CompressStream :859-999, FindBestBandEncoding :1502-1617,
CompressFrame93b :2053-2470):
  * statistics over 16 bands of 16 samples, f[0..255], with every band norm 1.0;
  * the header: no Type-1 scale adjust, no sub-type bits, 0x80 in byte 0 for Type 1; the rate model's share norm over
    the layout's own band counts (Type 1: 15, then 16 x 15);
  * the band loop: the sub-type 0 search over codes 1..15, the delta codes of sub-types 1 and 2 on the scaled integers,
    the carried prvSample / prvDelta, the 1-bit repeat of a zero band, and (Type 1) the band-type codes carried from
    frame to frame, updated only when a delta is written.

The one rule where the library departs from the reference ("Encoding"): the reference's "Keep" codebook
has no code for delta +15, so a sub-type-1 candidate whose delta falls outside the chosen codebook (-15..+14 for Keep,
-16..+15 for Invert) is not eligible; the band keeps its sub-type-0 code.  encode() reports whether it fired.

The walk works from per-band records that do not depend on the incoming prvSample / prvDelta (the search's two codes, the
bit lengths of the deltas inside the band, the first two and last two scaled values), as the library's kernels do; the
records are checked against the direct computation of GetDeltaBandCode by tests/test_encode93_host.py.
"""
import re

import numpy as np

import enc_ref as E

F32 = np.float32
DEFAULTS = dict(E.DEFAULTS)

STAT_FIRST = np.arange(16) * 16                                 # Frame::Frame: bandSampleCounts93 for every OS93 stream
COUNT = {0: np.full(16, 16), 1: np.array([15] + [16] * 15)}     # bandSampleCounts93 / bandSampleCounts93b_Type1
FIRST = {t: np.concatenate([[0], np.cumsum(c)[:-1]]) for t, c in COUNT.items()}


def _vlc93():
    """the Keep / Invert band-type codebooks, [invert][delta + 16] -> (code, length): the inverse of the decoder's
    kVlc93BandType (leaf < 0x1E: Keep, delta = leaf - 0x0F; else Invert, delta = leaf - 0x2E)"""
    code, length = np.zeros((2, 32), np.int64), np.zeros((2, 32), np.int64)
    for c, n, v in re.findall(r'\{0x([0-9a-f]+),\s*(\d+),\s*(-?\d+)\}', E._D["kVlc93BandType"]):
        v = int(v)
        inv = 1 if v >= 0x1E else 0
        d = v - (0x2E if inv else 0x0F)
        code[inv, d + 16], length[inv, d + 16] = int(c, 16), int(n)
    return code, length


BT_CODE, BT_LEN = _vlc93()


def frame_stats(f):
    """per frame and band (16 x 16): power (serial in sample order), lo, hi"""
    F = f.shape[0]
    power, lo, hi = np.zeros((F, 16), F32), np.zeros((F, 16), F32), np.zeros((F, 16), F32)
    for b in range(16):
        s0 = STAT_FIRST[b]
        p = f[:, s0] * f[:, s0]
        l, h = f[:, s0].copy(), f[:, s0].copy()
        for j in range(1, 16):
            s = f[:, s0 + j]
            p = p + s * s
            l, h = np.minimum(l, s), np.maximum(h, s)
        power[:, b], lo[:, b], hi[:, b] = p, l, h
    return power, lo, hi


def header(power_sum, rlo, rhi, typ, p=DEFAULTS):
    """CloseStream's bandsToKeep and CompressStream's OS93 header -> (16 header bytes, bandsToKeep, bitsPerBand[16])"""
    rms = np.sqrt(power_sum.astype(F32) * F32(1)).astype(F32)
    total = F32(0)
    for i in range(16):
        total = F32(total + rms[i])
    keep = 16
    if total != F32(0):
        norm, below = F32(1) / total, F32(0)
        for i in range(16):
            below = F32(below + F32(rms[i] * norm))
            if below >= F32(p["powerBandCutoff"]):
                keep = i
                break
    bits_per_frame = F32(F32(p["targetBitRate"]) / F32(F32(31250) / F32(240)))
    share_norm = F32(0)
    for i in range(keep):
        share_norm = F32(share_norm + F32(E.BAND_SHARE[i] * COUNT[typ][i]))
    bits = np.zeros(16, np.int64)
    hdr = np.full(16, 0xFF, np.int64)
    for b in range(keep):
        bits[b] = int(F32(F32(E.BAND_SHARE[b]) / share_norm) * bits_per_frame)
        lo_, hi_ = max(F32(rlo[b] * F32(-32768)), F32(0)), max(F32(rhi[b] * F32(32768)), F32(0))
        fs = hi_ if hi_ > lo_ else lo_
        div = 1 << (int(bits[b]) & 31)
        div = div - (1 << 32) if div >= 1 << 31 else div
        target = int(np.ceil(F32(fs / F32(div)))) if fs != 0 else 1
        hdr[b] = max(int(np.count_nonzero(E.SCALE < target)) - 1, 0)
    if typ != 0:
        hdr[0] |= 0x80
    return hdr.astype(np.uint8), keep, bits


def scaled(f, typ, band, hscale):
    """roundf(f * 32768 / scale) of the band's samples, every frame: [F, n]"""
    sf = F32(E.SCALE[hscale])
    s0 = FIRST[typ][band]
    return E.round_away(f[:, s0:s0 + COUNT[typ][band]] * F32(32768) / sf)


def search(f, typ, band, hscale, p=DEFAULTS):
    """FindBestBandEncoding of sub-type 0 for every frame: (best code over 1..15, best code over 1..14)"""
    codes = np.arange(1, 16)
    w = codes + (1 if typ == 0 else 0)
    ref = 1 << (w - 1)
    mask = 0xFFFF >> (16 - w)
    sf = F32(E.SCALE[hscale])
    s0, n = FIRST[typ][band], COUNT[typ][band]
    orig = f[:, s0:s0 + n][:, None, :]
    sc = E.round_away(orig * F32(32768) / sf)
    stored = (sc + ref[None, :, None]) & mask[None, :, None]
    rec = (stored - ref[None, :, None]).astype(F32) * sf / F32(32768)
    qe = rec - orig
    err = np.zeros(qe.shape[:2], F32)
    for j in range(n):
        err = err + qe[:, :, j] * qe[:, :, j]
    mqe = F32(p["maximumQuantizationError"])
    passed = err <= F32(mqe * mqe) * F32(n)
    out = []
    for allowed in (np.ones(15, bool), codes != 15):
        ok = passed & allowed[None, :]
        narrow = np.where(ok, w[None, :], 99).min(axis=1)
        cand = allowed[None, :] & ((narrow[:, None] == 99) | (w[None, :] == narrow[:, None]))
        out.append(codes[np.argmin(np.where(cand, err, np.inf), axis=1)])
    return out


def bitlen(x):
    return np.array([int(v).bit_length() for v in np.ravel(x)], np.int64).reshape(np.shape(x))


def records(f, hdr, keep, typ, p=DEFAULTS):
    """per band (list over bands < keep): the scaled integers [F, n] and the walk's per-frame record
    (best, best without 15, bit length of max |buf1[i]| i >= 1, of max |buf2[i]| i >= 2)"""
    out = []
    for b in range(keep):
        hs = int(hdr[b]) & 0x3F
        s = scaled(f, typ, b, hs)
        best, best15 = search(f, typ, b, hs, p)
        d1 = np.diff(s, axis=1)
        d2 = np.diff(d1, axis=1)
        out.append(dict(s=s, best=best, best15=best15, L1=bitlen(np.abs(d1).max(axis=1)), L2=bitlen(np.abs(d2).max(axis=1))))
    return out


def delta_code(L, typ):
    """GetDeltaBandCode from the bit length of max |delta|"""
    return 0 if L == 0 else L + (1 if typ == 1 else 0)


def walk(recs, keep, typ, F):
    """CompressFrame93b's band loop, frame after frame -> per (frame, band): code, sub-type, repeat flag, the 0-bit flag
    (last band's code was 0), the old band-type code (Type 1), the incoming prvSample / prvDelta; and how often the
    Keep +15 rule fired"""
    shape = (F, 16)
    code, sub, rep, flag, old_, P_, D_ = (np.zeros(shape, np.int64) for _ in range(7))
    btc = [0] * 16
    fired = 0
    for t in range(F):
        last_code, last_sub, P, D = -1, (0 if typ == 1 else 2), 0, 0
        for b in range(keep):
            r = recs[b]
            s = r["s"][t]
            s0, s1, sl, dl = int(s[0]), int(s[1]), int(s[-1]), int(s[-1] - s[-2])
            old = btc[b] if typ == 1 else 0
            c0 = int(r["best15"][t] if (typ == 1 and last_sub == 0 and old == 0) else r["best"][t])
            c1 = delta_code(max(abs(s0 - P).bit_length(), int(r["L1"][t])), typ)
            c2 = delta_code(max(abs(s0 - P - D).bit_length(), abs(s1 - 2 * s0 + P).bit_length(), int(r["L2"][t])), typ)
            c, sb = c0, 0
            if c1 < c or (c1 == c and last_sub == 1):
                if typ == 1 and last_sub == 1 and c1 - old > 14:
                    fired += 1                          # no Keep code for the delta: the sub-type-0 code stays
                else:
                    c, sb = c1, 1
            if typ == 0 and c2 < c:
                c, sb = c2, 2
            code[t, b], sub[t, b], old_[t, b], P_[t, b], D_[t, b] = c, sb, old, P, D
            flag[t, b] = last_code == 0
            if last_code == 0 and c == 0 and last_sub == sb:
                rep[t, b] = 1
                P, D = sl, dl
            else:
                if typ == 1:
                    btc[b] = c
                if c == 0:
                    P, D = (0, 0) if sb == 0 else (P, 0) if sb == 1 else (P, D)
                else:
                    P, D = sl, dl
            last_code, last_sub = c, sb
    return dict(code=code, sub=sub, rep=rep, flag=flag, old=old_, P=P_, D=D_), fired


def emit(recs, w, keep, typ, F):
    """the frames' bit stream as (value, length) pairs in stream order"""
    cols_v, cols_n = [], []
    for b in range(keep):
        code, sb, rep, flag = w["code"][:, b], w["sub"][:, b], w["rep"][:, b], w["flag"][:, b]
        prev_sub = w["sub"][:, b - 1] if b else np.full(F, 0 if typ == 1 else 2)
        # the repeat bit, or the 0 bit after a zero band
        cols_v.append(np.where(rep == 1, 1, 0))
        cols_n.append(np.where((rep == 1) | (flag == 1), 1, 0))
        if typ == 0:
            dbit = (sb == (prev_sub + 1) % 3).astype(np.int64)
            v = np.where(sb == prev_sub, code, (1 << 5) | (dbit << 4) | code)
            n = np.where(sb == prev_sub, 5, 6)
        else:
            inv = (sb != prev_sub).astype(np.int64)
            v, n = BT_CODE[inv, code - w["old"][:, b] + 16], BT_LEN[inv, code - w["old"][:, b] + 16]
        cols_v.append(v)
        cols_n.append(np.where(rep == 1, 0, n))
        s = recs[b]["s"]
        P, D = w["P"][:, b][:, None], w["D"][:, b][:, None]
        buf1 = np.hstack([s[:, :1] - P, np.diff(s, axis=1)])
        buf2 = np.hstack([s[:, :1] - P - D, s[:, 1:2] - 2 * s[:, :1] + P, np.diff(s, n=2, axis=1)])
        buf = np.where(sb[:, None] == 0, s, np.where(sb[:, None] == 1, buf1, buf2))
        nbits = code + (1 if typ == 0 else 0)
        live = (rep == 0) & (code != 0)
        vals = buf & ((1 << nbits) - 1)[:, None]
        lens = np.where(live, nbits, 0)[:, None] + 0 * vals
        for j in range(s.shape[1]):
            cols_v.append(vals[:, j])
            cols_n.append(lens[:, j])
    if not cols_v:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.stack(cols_v, 1).ravel(), np.stack(cols_n, 1).ravel()


def analyse_stream(x):
    f = E.analyse(E.frames_of(x))
    power, lo, hi = frame_stats(f)
    return f, E.stream_stats(power, lo, hi)


def encode_layout(an, typ, p=DEFAULTS):
    """-> (stream bytes, bandsToKeep, times the Keep +15 rule fired)"""
    f, (ps, rlo, rhi) = an
    hdr, keep, _ = header(ps, rlo, rhi, typ, p)
    F = f.shape[0]
    recs = records(f, hdr, keep, typ, p)
    w, fired = walk(recs, keep, typ, F)
    body = E.pack_bits(*emit(recs, w, keep, typ, F))
    return bytes([F >> 8, F & 0xFF]) + hdr.tobytes() + body, keep, fired


def layouts(version, typ):
    """the types CloseStream tries for formatVersion `version` and streamFormatType `typ`, in its order"""
    if version not in (0x9301, 0x9302) or typ not in (-1, 0, 1):
        raise ValueError("not an OS93 encoding: version %#x, type %r" % (version, typ))
    if version == 0x9301 and typ == 1:
        raise ValueError("OS93a Type 1 is not encodable (CompressFrame93a)")
    if version == 0x9301:
        return [0]
    return [0, 1] if typ == -1 else [typ]


def encode(pcm, version=0x9302, typ=-1, **params):
    """-> (stream bytes, type written, bandsToKeep, times the Keep +15 rule fired in the layouts tried)"""
    p = dict(DEFAULTS, **params)
    x = E.to_float(pcm)
    if len(x) == 0 or (len(x) + 239) // 240 > 65535:
        raise ValueError("empty stream or more than 65 535 frames")
    an = analyse_stream(x)
    best, fired = None, 0
    for t in layouts(version, typ):
        s, keep, k = encode_layout(an, t, p)
        fired += k
        if best is None or len(s) < len(best[0]):
            best = (s, t, keep)
    return best + (fired,)


def bound(n_samples):
    """the longest stream n_samples samples can encode to, either layout (0 = not encodable)"""
    nf = (n_samples + 239) // 240
    if nf == 0 or nf > 65535:
        return 0
    t0 = 16 * (1 + 2 + 4 + 16 * 16)
    t1 = 16 * (1 + 30) + 15 * 15 + 15 * 16 * 15
    return 18 + (nf * max(t0, t1) + 7) // 8
