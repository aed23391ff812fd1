"""numpy restatement of the 1994+ encoder (test infrastructure, like graph_ref.py: not part of the product).

Float32 throughout, every operation in the reference encoder's order (DCSEncoder.cpp: TransformFrame :1001-1069,
DFTAlgorithmOrig :1218-1358, DualFFT :1360-1500, Frame::Frame :2535-2571, CloseStream :717-850, CompressStream
:859-960, CompressFrame94 :1623-2050), vectorised across frames and candidate codes, with every sum kept serial.
numpy's float32 arithmetic is IEEE single without contraction, which is what the reference's x86-64 build does.

The three rules the library defines where the reference is undefined or wrong ("Encoding"):
  * 1 << bitsPerBand with bitsPerBand > 31 is 1 << (bitsPerBand & 31), as the reference's x86 shl computes it;
  * a Type-1 candidate code whose scale index exceeds 0x3f is not eligible;
  * int16 input is x / 32768 (the reference's int16 overload skips slots); empty input and > 65 535 frames are errors.
"""
import math
import os
import re

import numpy as np

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "dcsexplorer_amd", "csrc")

VARIANTS = [(0, 0), (0, 3), (1, 0), (1, 3)]       # the reference's wildcard order (CloseStream :790)
DEFAULTS = dict(powerBandCutoff=0.97, targetBitRate=128000, minimumDynamicRange=10 / 32768, maximumQuantizationError=10 / 32768)


def _arrays(path):
    src = open(path).read()
    out = {}
    for m in re.finditer(r'static const \w+ (\w+)\[\d+\] = \{(.*?)\};', src, re.S):
        out[m.group(1)] = m.group(2)
    return out


def _ints(text):
    return [int(t, 0) for t in re.findall(r'0x[0-9a-fA-F]+|-?\d+', text)]


def _f32bits(text):
    return np.array([int(t, 16) for t in re.findall(r'0x([0-9a-fA-F]+)u', text)], dtype=np.uint32).view(np.float32)


_D = _arrays(os.path.join(CSRC, "dcs_tables.h"))
_E = _arrays(os.path.join(CSRC, "dcs_enc_tables.h"))
WINDOW = _f32bits(_E["kEncWindowBits"])
TWIDDLE = _f32bits(_E["kEncTwiddleBits"])
FFT = _f32bits(_E["kEncFftBits"])
BAND_NORM = _f32bits(_E["kEncBandNormBits"])
BAND_SHARE = np.array(_ints(_E["kEncBandShare"]))
BAND_COUNT = np.array(_ints(_D["kBandCount94"]))
BAND_FIRST = np.concatenate([[0], np.cumsum(BAND_COUNT)[:-1]])
_MANT = _ints(_D["kScaleMant"])
SCALE = np.array([_MANT[j & 3] >> (15 - (j >> 2)) for j in range(64)], dtype=np.int64)
PREADJ = {0: np.array(_ints(_D["kPreAdjSub0"])), 3: np.array(_ints(_D["kPreAdjSub3"]))}
XLAT = [np.array(_ints(_D[n])) for n in ("kXlatB02", "kXlatB35", "kXlatB6F")]       # decode layout: adjust << 8 | width


def _vlc(name):
    trip = re.findall(r'\{0x([0-9a-f]+),\s*(\d+),\s*(-?\d+)\}', _D[name])
    return [(int(c, 16), int(n), int(v)) for c, n, v in trip]


# encode codebooks: the inverses of the decode trees
HDR_CODE = np.zeros(31, np.int64)
HDR_LEN = np.zeros(31, np.int64)
for _c, _n, _v in _vlc("kVlc94BandTypeDelta"):
    HDR_CODE[_v + 16], HDR_LEN[_v + 16] = _c, _n
SMP_CODE, SMP_LEN, DZ_CODE, DZ_LEN = {}, {}, {}, {}
for _w in range(1, 7):
    SMP_CODE[_w], SMP_LEN[_w] = np.zeros(1 << _w, np.int64), np.zeros(1 << _w, np.int64)
    for _c, _n, _v in _vlc("kVlc94Sample%d" % _w):
        if _v & 0x80:
            DZ_CODE[_w], DZ_LEN[_w] = _c, _n
        else:
            SMP_CODE[_w][_v], SMP_LEN[_w][_v] = _c, _n


def _bitrev7(i):
    return int("{:07b}".format(i)[::-1], 2)


BITREV = np.array([_bitrev7(i) for i in range(128)])


def round_away(v):
    """roundf: halves away from zero"""
    t = np.trunc(v)
    return (t + np.where(np.abs(v - t) >= F32(0.5), np.sign(v), F32(0))).astype(np.int64)


def frames_of(x):
    """frame k = x[240k-16 .. 240k+240), zero before the start and after the end; ceil(n/240) frames"""
    n = len(x)
    nf = (n + 239) // 240
    pad = np.zeros(16 + nf * 240 + 16, F32)
    pad[16:16 + n] = x
    return pad[np.arange(nf)[:, None] * 240 + np.arange(256)[None, :]]


def analyse(fr):
    """[F,256] input frames -> [F,256] DCS frame samples (the reference's frame.f)"""
    F = fr.shape[0]
    x = fr.astype(F32).copy()
    for i in range(16):
        x[:, i] *= WINDOW[i]
        x[:, 255 - i] *= WINDOW[i]
    buf = np.zeros((F, 258), F32)
    buf[:, BITREV * 2] = x[:, 0::2]
    buf[:, BITREV * 2 + 1] = x[:, 1::2]
    for s in range(1, 7):
        m = 1 << s
        kk, jj = np.meshgrid(np.arange(0, 128, m), np.arange(m // 2), indexing="ij")
        kk, jj = kk.ravel(), jj.ravel()
        ci = (s - 1) * 128 + 2 * ((kk // m) * (m // 2) + jj)
        c, sn = FFT[ci], FFT[ci + 1]
        t, u = (kk + jj + m // 2) * 2, (kk + jj) * 2
        ar, ai, ur, ui = buf[:, t], buf[:, t + 1], buf[:, u], buf[:, u + 1]
        tr = ar * c - ai * sn
        ti = ar * sn + ai * c
        buf[:, u], buf[:, u + 1] = tr + ur, ti + ui
        buf[:, t], buf[:, t + 1] = ur - tr, ui - ti
    j = np.arange(1, 64)
    ci = 896 - 126 + 2 * (j - 1)
    c, sn = FFT[ci], FFT[ci + 1]
    t = 128 + 2 * j
    ar, ai = buf[:, t].copy(), buf[:, t + 1].copy()
    buf[:, t] = ar * c - ai * sn
    buf[:, t + 1] = ar * sn + ai * c
    buf[:, :256] *= F32(1 / 64)
    f = buf
    half = F32(2)
    f[:, 1] = (f[:, 0] + f[:, 0x80]) / half
    f[:, 0x81] = f[:, 1]
    f[:, 0x100] = f[:, 1]
    f[:, 0x101] = f[:, 1]
    p0 = np.arange(64) * 2
    p1 = 0x80 + p0
    x0, y0, x1, y1 = f[:, p0], f[:, p0 + 1], f[:, p1], f[:, p1 + 1]
    f[:, p0], f[:, p0 + 1], f[:, p1], f[:, p1 + 1] = (x0 + x1) / half, (y0 + y1) / half, (x0 - x1) / half, (y0 - y1) / half
    p1 = 0x100 - p0
    x0, y0, x1, y1 = f[:, p0], f[:, p0 + 1], f[:, p1], f[:, p1 + 1]
    xs, ys = (x0 - x1) / half, (y0 + y1) / half
    c, sn = TWIDDLE[p0], TWIDDLE[p0 + 1]
    f[:, p0], f[:, p0 + 1] = (x0 + x1) / half, (y0 - y1) / half
    f[:, p1], f[:, p1 + 1] = xs * sn - ys * c, xs * c + ys * sn
    x0, y0, x1, y1 = -f[:, p0], -f[:, p0 + 1], -f[:, p1], -f[:, p1 + 1]
    f[:, p0], f[:, p0 + 1], f[:, p1], f[:, p1 + 1] = (x0 + x1) / half, (y0 + y1) / half, (x0 - x1) / half, (y0 - y1) / half
    f[:, 0x80] = -f[:, 0x80]
    f[:, 0x81] = -f[:, 0x81]
    f[:, 129:256:2] = -f[:, 129:256:2]
    f[:, 1] = f[:, 0]
    return f[:, 1:257].copy()


def frame_stats(f):
    """per frame and band: power (serial in sample order), lo, hi"""
    F = f.shape[0]
    power, lo, hi = np.zeros((F, 16), F32), np.zeros((F, 16), F32), np.zeros((F, 16), F32)
    for b in range(16):
        s0 = BAND_FIRST[b]
        p = f[:, s0] * f[:, s0]
        l, h = f[:, s0].copy(), f[:, s0].copy()
        for j in range(1, BAND_COUNT[b]):
            s = f[:, s0 + j]
            p = p + s * s
            l, h = np.minimum(l, s), np.maximum(h, s)
        power[:, b], lo[:, b], hi[:, b] = p, l, h
    return power, lo, hi


def stream_stats(power, lo, hi):
    """powerSum in frame order, and the range over the stream"""
    return np.add.accumulate(power, axis=0, dtype=F32)[-1], lo.min(axis=0), hi.max(axis=0)


def header(power_sum, rlo, rhi, typ, sub, p=DEFAULTS):
    """CloseStream's bandsToKeep and CompressStream's header -> (16 header bytes, bandsToKeep, bitsPerBand[16])"""
    rms = np.sqrt(power_sum.astype(F32) * BAND_NORM).astype(F32)
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
        share_norm = F32(share_norm + F32(BAND_SHARE[i] * BAND_COUNT[i]))
    bits = np.zeros(16, np.int64)
    hdr = np.full(16, 0xFF, np.int64)
    for b in range(keep):
        bits[b] = int(F32(F32(BAND_SHARE[b]) / share_norm) * bits_per_frame)
        lo_, hi_ = max(F32(rlo[b] * F32(-32768)), F32(0)), max(F32(rhi[b] * F32(32768)), F32(0))
        fs = hi_ if hi_ > lo_ else lo_
        div = 1 << (int(bits[b]) & 31)
        div = div - (1 << 32) if div >= 1 << 31 else div
        target = int(math.ceil(F32(fs / F32(div)))) if fs != 0 else 1
        hdr[b] = max(int(np.count_nonzero(SCALE < target)) - 1, 0)
        if typ == 1:
            adj = (0x0D if b < 3 else 0x17) + (1 if sub == 0 else 3)
            hdr[b] = hdr[b] - adj if hdr[b] > adj else 0
    if typ != 0:
        hdr[0] |= 0x80
    hdr[1] |= (sub & 2) << 6
    hdr[2] |= (sub & 1) << 7
    return hdr.astype(np.uint8), keep, bits


def interpret(typ, band, codes, hscale, pre):
    """band-type codes (array) -> (bit width, scale index, reference value)"""
    codes = np.asarray(codes)
    if typ == 0:
        w, sc = codes, np.full(codes.shape, hscale)
    else:
        e = XLAT[0 if band < 3 else 1 if band < 6 else 2][codes]
        w, sc = e & 0xFF, hscale + (e >> 8) + (pre if band < 3 else 0)
    ref = np.where((w >= 1) & (w <= 6), 1 << np.maximum(w - 1, 0), 0)
    return np.where(codes == 0, 0, w), np.where(codes == 0, 0, sc), np.where(codes == 0, 0, ref)


def search(f, typ, band, hscale, pre, p=DEFAULTS):
    """FindBestBandEncoding for every frame at one pre-adjust: (best code over 1..15, best code over 1..14)"""
    codes = np.arange(1, 16)
    w, sc, _ = interpret(typ, band, codes, hscale, pre)
    ref = 1 << (w - 1)              # the search biases every width to mid-range, even the raw ones (:1534)
    elig = sc <= 0x3F
    sf = SCALE[np.minimum(sc, 63)].astype(F32)
    mask = 0xFFFF >> (16 - w)
    orig = f[:, BAND_FIRST[band]:BAND_FIRST[band] + BAND_COUNT[band]][:, None, :]
    scaled = round_away(orig * F32(32768) / sf[None, :, None])
    stored = (scaled + ref[None, :, None]) & mask[None, :, None]
    rec = (stored - ref[None, :, None]).astype(F32) * sf[None, :, None] / F32(32768)
    qe = rec - orig
    err = np.zeros(qe.shape[:2], F32)
    for j in range(qe.shape[2]):
        err = err + qe[:, :, j] * qe[:, :, j]
    mqe = F32(p["maximumQuantizationError"])
    passed = err <= F32(mqe * mqe) * F32(BAND_COUNT[band])
    out = []
    for allowed in (elig, elig & (codes != 15)):
        ok = passed & allowed[None, :]
        narrow = np.where(ok, w[None, :], 99).min(axis=1)
        cand = allowed[None, :] & ((narrow[:, None] == 99) | (w[None, :] == narrow[:, None]))
        out.append(codes[np.argmin(np.where(cand, err, np.inf), axis=1)])
    return out


def choose_codes(f, lo, hi, hdr, keep, typ, sub, p=DEFAULTS):
    """the band-type codes of every frame (the frame-to-frame walk of CompressFrame94)"""
    F = f.shape[0]
    codes = np.zeros((F, 16), np.int64)
    zero = (hi - lo) < F32(p["minimumDynamicRange"])
    pmap = PREADJ[0 if sub == 0 else 3]
    best = {}
    for b in range(keep):
        pres = sorted(set(pmap.tolist())) if (typ == 1 and b < 3) else [0]
        for pre in pres:
            best[b, pre] = search(f, typ, b, int(hdr[b]) & 0x3F, pre, p)
    old = np.zeros(16, np.int64)
    for t in range(F):
        for b in range(keep):
            pre = pmap[old[b]] if (typ == 1 and b < 3) else 0
            a, n15 = best[b, pre]
            new = 0 if zero[t, b] else (n15[t] if old[b] == 0 else a[t])
            codes[t, b] = new
        old = codes[t]
    return codes


def emit(f, codes, hdr, keep, typ, sub):
    """the frames' bit stream as (value, length) pairs in stream order"""
    F = f.shape[0]
    prev = np.vstack([np.zeros((1, 16), np.int64), codes[:-1]])
    cols_v, cols_n = [], []
    for b in range(keep):
        d = codes[:, b] - prev[:, b] + 16
        cols_v.append(HDR_CODE[d])
        cols_n.append(HDR_LEN[d])
    pmap = PREADJ[0 if sub == 0 else 3]
    for b in range(keep):
        pre = pmap[prev[:, b]] if (typ == 1 and b < 3) else np.zeros(F, np.int64)
        w, sc, ref = interpret(typ, b, codes[:, b], int(hdr[b]) & 0x3F, pre)
        sf = SCALE[np.minimum(sc, 63)].astype(F32)
        n = BAND_COUNT[b]
        stg = round_away(f[:, BAND_FIRST[b]:BAND_FIRST[b] + n] * F32(32768) / sf[:, None])
        mask = (0xFFFF >> (16 - w))[:, None]
        idx = (stg + ref[:, None]) & mask
        vals, lens = idx.copy(), np.where(w[:, None] > 0, w[:, None], 0) + 0 * idx
        cb = (w >= 1) & (w <= 6)
        z = stg == 0
        run = np.zeros_like(stg)
        for j in range(n):
            run[:, j] = np.where(z[:, j], (run[:, j - 1] + 1) if j else 1, 0)
        nxt = np.hstack([z[:, 1:], np.zeros((F, 1), bool)])
        dz = z & ((run % 2) == 1) & nxt & cb[:, None]
        skip = z & ((run % 2) == 0) & cb[:, None]
        for wi in range(1, 7):
            sel = w == wi
            if sel.any():
                vals[sel] = SMP_CODE[wi][idx[sel]]
                lens[sel] = SMP_LEN[wi][idx[sel]]
                dsel = dz & sel[:, None]
                vals[dsel], lens[dsel] = DZ_CODE[wi], DZ_LEN[wi]
        lens[skip] = 0
        for j in range(n):
            cols_v.append(vals[:, j])
            cols_n.append(lens[:, j])
    if not cols_v:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.stack(cols_v, 1).ravel(), np.stack(cols_n, 1).ravel()


def pack_bits(vals, lens):
    """MSB-first, zero-padded to a byte"""
    keep = lens > 0
    vals, lens = vals[keep], lens[keep]
    total = int(lens.sum())
    if total == 0:
        return b""
    start = np.cumsum(lens) - lens
    owner = np.repeat(np.arange(len(lens)), lens)
    k = np.arange(total) - start[owner]
    bit = (vals[owner] >> (lens[owner] - 1 - k)) & 1
    return np.packbits(bit.astype(np.uint8)).tobytes()


def to_float(pcm):
    pcm = np.asarray(pcm)
    return pcm.astype(F32) / F32(32768) if pcm.dtype == np.int16 else pcm.astype(F32)


def analyse_stream(x):
    f = analyse(frames_of(x))
    power, lo, hi = frame_stats(f)
    return f, lo, hi, stream_stats(power, lo, hi)


def encode_variant(an, typ, sub, p=DEFAULTS):
    f, lo, hi, (ps, rlo, rhi) = an
    hdr, keep, _ = header(ps, rlo, rhi, typ, sub, p)
    codes = choose_codes(f, lo, hi, hdr, keep, typ, sub, p)
    body = pack_bits(*emit(f, codes, hdr, keep, typ, sub))
    F = f.shape[0]
    return bytes([F >> 8, F & 0xFF]) + hdr.tobytes() + body, keep


def encode(pcm, fmt=(-1, -1), **params):
    """-> (stream bytes, (type, sub-type) written, bandsToKeep).  fmt = (type, sub-type), -1 = wildcard"""
    p = dict(DEFAULTS, **params)
    x = to_float(pcm)
    if len(x) == 0 or (len(x) + 239) // 240 > 65535:
        raise ValueError("empty stream or more than 65 535 frames")
    an = analyse_stream(x)
    best = None
    sizes = {}
    for typ, sub in VARIANTS:
        if fmt[0] not in (-1, typ) or fmt[1] not in (-1, sub):
            continue
        key = (typ, 0 if typ == 0 else sub)
        if key not in sizes:
            sizes[key] = encode_variant(an, typ, sub, p)
        s, keep = sizes[key]
        if typ == 0 and sub == 3:
            s = s[:3] + bytes([s[3] | 0x80, s[4] | 0x80]) + s[5:]
        if best is None or len(s) < len(best[0]):
            best = (s, (typ, sub), keep)
    return best
