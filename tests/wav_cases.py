"""Seeded WAV files for dcs_encode_files / dcs_wav_parse tests: every case is a recipe (name -> bytes), so no WAV bytes are
committed.  The writer builds RIFF files chunk by chunk, so a case can carry extra chunks, odd sizes and the traps of
libnyquist's ScanForChunk."""
import hashlib
import struct

import numpy as np

GUID_TAIL = bytes([0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71])
IMA_STEP = [7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118,
            130, 143, 157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060,
            1166, 1282, 1411, 1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484,
            7132, 7845, 8630, 9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767]


def chunk(code, payload, pad=True):
    b = code.encode() + struct.pack("<I", len(payload)) + payload
    return b + (b"\0" if pad and len(payload) % 2 else b"")


def fmt_chunk(code, channels, rate, bits, block_align=None, size=16, sub=None):
    ba = block_align if block_align is not None else channels * max(bits, 8) // 8
    body = struct.pack("<HHIIHH", code, channels, rate, rate * ba, ba, bits)
    if size >= 18:
        body += struct.pack("<H", size - 18)
    if size >= 40:
        sub_code = sub if sub is not None else 1
        body += struct.pack("<HI", bits, 3 if channels == 2 else 4) + struct.pack("<I", sub_code) + GUID_TAIL[2:]
    body = body.ljust(size, b"\0")
    return chunk("fmt ", body)


def riff(chunks, size_delta=0, head=b"RIFF"):
    body = b"WAVE" + b"".join(chunks)
    return head + struct.pack("<I", len(body) + size_delta) + body


def pcm_payload(fmt, values):
    v = np.asarray(values)
    if fmt == "u8":
        return v.astype(np.uint8).tobytes()
    if fmt == "s16":
        return v.astype("<i2").tobytes()
    if fmt == "s24":
        x = v.astype(np.int64) & 0xFFFFFF
        return np.stack([(x & 0xFF), (x >> 8) & 0xFF, (x >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes()
    if fmt == "s32":
        return v.astype("<i4").tobytes()
    if fmt == "f32":
        return v.astype("<f4").tobytes()
    if fmt == "f64":
        return v.astype("<f8").tobytes()
    raise ValueError(fmt)


BITS = {"u8": 8, "s16": 16, "s24": 24, "s32": 32, "f32": 32, "f64": 64}


def signal(fmt, n, seed, scale=0.6):
    """n values of a seeded tone plus noise, in the format's own integer or float range"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = scale * (0.7 * np.sin(2 * np.pi * t * (0.003 + 0.01 * rng.random())) + 0.3 * (rng.random(n) * 2 - 1))
    if fmt == "u8":
        return np.clip(np.round(x * 127 + 128), 0, 255).astype(np.int64)
    if fmt in ("f32", "f64"):
        return x
    full = {"s16": 32767, "s24": 8388607, "s32": 2147483647}[fmt]
    return np.round(x * full).astype(np.int64)


def wav(fmt, channels, rate, values, fmt_size=16, extensible=None, extra_before=(), extra_after=()):
    code = 3 if fmt in ("f32", "f64") else 1
    if extensible is not None:
        code, fmt_size = 0xFFFE, 40
    fc = fmt_chunk(code, channels, rate, BITS[fmt], size=fmt_size, sub=extensible)
    return riff([fc, *extra_before, chunk("data", pcm_payload(fmt, values)), *extra_after])


# ------------------------------------------------------------------------------------------------------ IMA ADPCM writer

def ima_encode(values, channels, block_align, seed):
    """int16 values (interleaved) -> IMA ADPCM blocks with headers; the encoder is a plain greedy one (the decode is what is
    tested).  Step indices start from a seeded value."""
    rng = np.random.default_rng(seed)
    words = (block_align - 4 * channels) // (4 * channels)
    per_block = 8 * words                        # values per channel after the header sample
    v = np.asarray(values, np.int64).reshape(-1, channels)
    nb = max(1, -(-len(v) // (per_block + 1)))
    out = bytearray()
    for b in range(nb):
        seg = v[b * (per_block + 1):(b + 1) * (per_block + 1)]
        hdr = bytearray()
        nib = []
        for c in range(channels):
            col = seg[:, c] if len(seg) else np.zeros(1, np.int64)
            p, s = int(col[0]), int(rng.integers(0, 89))
            hdr += struct.pack("<hBB", p, s, 0)
            codes = []
            for k in range(per_block):
                target = int(col[1 + k]) if 1 + k < len(col) else p
                step = IMA_STEP[s]
                d = target - p
                n = 8 if d < 0 else 0
                d = abs(d)
                if d >= step: n |= 4; d -= step
                if d >= step >> 1: n |= 2; d -= step >> 1
                if d >= step >> 2: n |= 1
                diff = step >> 3
                if n & 4: diff += step
                if n & 2: diff += step >> 1
                if n & 1: diff += step >> 2
                if n & 8: diff = -diff
                p = ((p + diff + 32768) & 0xFFFF) - 32768
                s = min(88, max(0, s + [-1, -1, -1, -1, 2, 4, 6, 8][n & 7]))
                codes.append(n)
            nib.append(codes)
        body = bytearray()
        for w in range(words):
            for c in range(channels):
                cs = nib[c][8 * w:8 * w + 8]
                body += bytes(cs[2 * j] | (cs[2 * j + 1] << 4) for j in range(4))
        out += hdr + body
    return bytes(out), nb


def ima_wav(channels, rate, n_frames, block_align, seed, fact=None, partial=0, extra=(), patch=None):
    vals = signal("s16", n_frames * channels, seed, 0.5)
    data, nb = ima_encode(vals, channels, block_align, seed)
    data = bytearray(data + bytes(range(partial)))
    if patch:
        patch(data)
    samples = fact if fact is not None else n_frames
    chunks = [fmt_chunk(0x11, channels, rate, 4, block_align=block_align, size=20)]
    if fact is not False:
        chunks.append(chunk("fact", struct.pack("<I", samples)))
    chunks += [*extra, chunk("data", bytes(data))]
    return riff(chunks)


# ----------------------------------------------------------------------------------------------------------- the cases

def cases():
    """-> list of (name, bytes); the order and the bytes are fixed by the seeds"""
    out = []
    rates = [8000, 22050, 31250, 44100, 48000]
    seed = 100
    for fmt in ("u8", "s16", "s24", "s32", "f32", "f64"):
        for ch in (1, 2):
            for rate in rates:
                seed += 1
                n = (777 + 13 * seed) * ch + (1 if ch == 2 and seed % 3 == 0 else 0)     # odd counts: an unpaired value
                out.append(("%s_%dch_%d" % (fmt, ch, rate), wav(fmt, ch, rate, signal(fmt, n, seed))))
    out.append(("s16_fmt18", wav("s16", 2, 44100, signal("s16", 2000, 1), fmt_size=18)))
    out.append(("s16_fmt40_plain", wav("s16", 1, 22050, signal("s16", 1501, 2), fmt_size=40)))
    out.append(("ext_pcm_s16", wav("s16", 2, 48000, signal("s16", 3000, 3), extensible=1)))
    out.append(("ext_pcm_s24", wav("s24", 1, 44100, signal("s24", 2001, 4), extensible=1)))
    out.append(("ext_pcm_s32", wav("s32", 2, 44100, signal("s32", 2002, 5), extensible=1)))
    out.append(("ext_float_f32", wav("f32", 2, 44100, signal("f32", 2400, 6), extensible=3)))
    out.append(("ext_float_f64", wav("f64", 1, 22050, signal("f64", 1999, 7), extensible=3)))
    lst = chunk("LIST", b"INFOISFT" + struct.pack("<I", 5) + b"test\0", pad=True)
    out.append(("extra_chunks", wav("s16", 2, 44100, signal("s16", 2500, 8),
                                    extra_before=[lst, chunk("fact", struct.pack("<I", 1250)), chunk("bext", bytes(602))])))
    out.append(("odd_chunk_pad", wav("s16", 1, 31250, signal("s16", 1800, 9), extra_before=[chunk("junk", b"abc")],
                                     extra_after=[chunk("cue ", b"12345")])))
    # ScanForChunk's trap: "data" inside a LIST payload comes first, so libnyquist takes it as the data chunk
    trap = chunk("LIST", b"INFO" + b"data" + struct.pack("<I", 64) + bytes(range(64)))
    out.append(("scan_trap_data_in_list", wav("s16", 1, 22050, signal("s16", 1200, 10), extra_before=[trap])))
    # full-scale negative samples
    fs16 = signal("s16", 4000, 11)
    fs16[100:140] = -32768
    out.append(("fullscale_s16_31250", wav("s16", 1, 31250, fs16)))
    fs8 = signal("u8", 4000, 12)
    fs8[200:220] = 0
    out.append(("fullscale_u8_31250", wav("u8", 1, 31250, fs8)))
    # IMA ADPCM: 256 .. 2048-byte blocks, mono and stereo, a trailing partial block
    for ba, ch, rate, nf in ((256, 1, 22050, 3000), (512, 2, 22050, 2600), (1024, 1, 44100, 5000), (2048, 2, 8000, 4100)):
        out.append(("ima_%d_%dch" % (ba, ch), ima_wav(ch, rate, nf, ba, seed=ba + ch)))
    out.append(("ima_partial_block", ima_wav(1, 22050, 2000, 256, seed=77, partial=100)))
    out.append(("ima_fact_short", ima_wav(1, 22050, 2000, 256, seed=78, fact=1500)))
    out.append(("ima_fact_long", ima_wav(2, 22050, 1000, 512, seed=79, fact=1200)))
    # refused files
    small = riff([fmt_chunk(1, 1, 8000, 16), chunk("data", bytes(12))])
    out.append(("err_size_63", small[:63]))
    f64b = riff([fmt_chunk(1, 1, 8000, 16), chunk("data", bytes(20))])
    out.append(("size_64", f64b))
    out.append(("err_riff_size", riff([fmt_chunk(1, 1, 8000, 16), chunk("data", bytes(200))], size_delta=2)))
    out.append(("err_rifx", riff([fmt_chunk(1, 1, 8000, 16), chunk("data", bytes(200))], head=b"RIFX")))
    out.append(("err_mulaw", riff([fmt_chunk(7, 1, 8000, 8), chunk("data", bytes(200))])))
    out.append(("err_3ch", riff([fmt_chunk(1, 3, 8000, 16), chunk("data", bytes(300))])))
    out.append(("err_bits12", riff([fmt_chunk(1, 1, 8000, 12, block_align=2), chunk("data", bytes(200))])))
    out.append(("err_int64", riff([fmt_chunk(1, 1, 8000, 64), chunk("data", bytes(200))])))
    out.append(("err_ext_other", riff([fmt_chunk(0xFFFE, 1, 8000, 16, size=40, sub=2), chunk("data", bytes(200))])))
    out.append(("err_blockalign0", riff([fmt_chunk(1, 1, 8000, 16, block_align=0), chunk("data", bytes(200))])))
    out.append(("err_data_past_end", riff([fmt_chunk(1, 1, 8000, 16), b"data" + struct.pack("<I", 400) + bytes(200)])))
    out.append(("err_fmt_at_end", riff([chunk("data", bytes(200)), b"fmt " + struct.pack("<I", 16) + bytes(8)])))
    out.append(("err_no_data", riff([fmt_chunk(1, 1, 8000, 16), chunk("junk", bytes(200))])))
    out.append(("enc_err_rate_low", wav("s16", 1, 3000, signal("s16", 400, 13))))
    out.append(("err_ima_reserved", ima_wav(1, 22050, 1000, 256, seed=80, patch=lambda d: d.__setitem__(256 + 3, 1))))
    out.append(("err_ima_no_fact", ima_wav(1, 22050, 1000, 256, seed=81, fact=False)))
    out.append(("err_ima_step89", ima_wav(1, 22050, 1000, 256, seed=82, patch=lambda d: d.__setitem__(2, 89))))
    out.append(("err_ima_overflow", ima_wav(1, 22050, 3000, 256, seed=83, fact=100)))
    return out


# ------------------------------------------------------------------------------------------------- float files' edges

F32_TINY, F32_NORM_MIN, F32_MAX = 2.0 ** -149, 2.0 ** -126, float(np.finfo(np.float32).max)
ONE_UP, ONE_DOWN = float(np.nextafter(np.float32(1), np.float32(2))), float(np.nextafter(np.float32(1), np.float32(0)))


def _quiet(n, seed):
    return signal("f32", n, seed, 0.3).astype(np.float32).astype(np.float64)


def _isolated(n, seed, vals):
    """a quiet tone with single samples of `vals`, 40 apart"""
    x = _quiet(n, seed)
    for k, v in enumerate(vals * 3):
        x[100 + 40 * k] = v
    return x


def float_edge_cases():
    """-> list of (name, bytes): f32 and f64 files, plain and EXTENSIBLE, mono and stereo, at the edges of the float formats.
    A second list beside cases(), which stays as it is.  1 000 values each."""
    rng = np.random.default_rng(0xF10A7)
    n = 1000
    out = []
    sub = rng.integers(-(1 << 23) + 1, 1 << 23, n).astype(np.float64) * F32_TINY            # every f32 subnormal magnitude
    sub[::7] = -0.0
    sub[3::11] = 0.0
    out.append(("fe_f32_subnormal_1ch", wav("f32", 1, 44100, sub)))
    out.append(("fe_f32_subnormal_2ch", wav("f32", 2, 22050, np.append(sub, -F32_TINY))))    # half a frame at the end: not counted
    out.append(("fe_f32_negzero_2ch", wav("f32", 2, 48000, np.full(n, -0.0))))
    # f64 values that are no f32: they round into the subnormal range (ties and near-ties of 2^-149 among them), or to +-0
    to_sub = rng.choice([-1.0, 1.0], n) * np.exp(rng.uniform(np.log(F32_TINY / 2), np.log(F32_NORM_MIN), n))
    to_sub[:8] = np.array([0.5, 1.5, 2.5, 0.5 + 2.0 ** -30, 0.5 - 2.0 ** -30, 1.5 - 2.0 ** -30, 2.0 ** 23 - 0.5, 2.0 ** 23 - 0.25]) * F32_TINY
    out.append(("fe_f64_to_subnormal_1ch", wav("f64", 1, 44100, to_sub)))
    out.append(("fe_f64_to_subnormal_2ch", wav("f64", 2, 8000, -to_sub)))
    out.append(("fe_f64_to_zero_2ch", wav("f64", 2, 44100, rng.choice([-1.0, 1.0], n) * rng.uniform(1e-47, 6e-46, n))))
    mixed = np.where(rng.random(n) < 0.5, sub, rng.uniform(-0.25, 0.25, n).astype(np.float32))
    out.append(("fe_f32_mixed_1ch", wav("f32", 1, 31250, mixed)))
    out.append(("fe_f64_mixed_2ch", wav("f64", 2, 31250, np.where(rng.random(n) < 0.5, to_sub, rng.uniform(-0.25, 0.25, n)))))
    # f64 values a hair either side of the midpoint of two neighbouring f32 values, and on it (ties to even)
    g = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    up = np.nextafter(g, np.float32(1)).astype(np.float64)
    mid = (g.astype(np.float64) + up) / 2
    ties = mid + rng.choice([-1.0, 0.0, 1.0], n) * np.abs(mid) * 2.0 ** -50
    out.append(("fe_f64_near_ties_1ch", wav("f64", 1, 22050, ties)))
    out.append(("fe_f64_near_ties_2ch", wav("f64", 2, 44100, ties[::-1].copy())))
    # at and around +-1: single samples in a quiet tone, then whole files
    out.append(("fe_f32_at_one_1ch", wav("f32", 1, 31250, _isolated(n, 21, [1.0, -1.0, ONE_DOWN, -ONE_DOWN]))))
    out.append(("fe_f64_rounds_to_one_1ch", wav("f64", 1, 44100, _isolated(n, 22, [1.0 + 2.0 ** -25, -1.0 - 2.0 ** -25, 1.0 - 2.0 ** -26]))))
    out.append(("fe_f32_above_one_1ch", wav("f32", 1, 31250, _isolated(n, 23, [ONE_UP, -ONE_UP]))))
    out.append(("fe_f32_dc_one_1ch", wav("f32", 1, 31250, np.full(n, 1.0))))
    out.append(("fe_f32_dc_above_one_1ch", wav("f32", 1, 31250, np.full(n, ONE_UP))))
    out.append(("fe_f64_dc_above_one_2ch", wav("f64", 2, 31250, np.full(n, -(1.0 + 2.0 ** -23)))))
    # f64 values that round to exactly FLT_MAX, and ones that overflow f32
    half_ulp = 2.0 ** 103
    out.append(("fe_f64_to_fltmax_1ch", wav("f64", 1, 44100, _isolated(n, 24, [F32_MAX + 0.99 * half_ulp, -F32_MAX - 0.5 * half_ulp,
                                                                                 F32_MAX - 0.99 * half_ulp]))))
    out.append(("fe_f64_overflow_1ch", wav("f64", 1, 44100, _isolated(n, 25, [F32_MAX + half_ulp, -1e300, 3.5e38]))))
    # not finite: a NaN, infinities, and finite pairs whose sum is not
    out.append(("fe_f32_nan_1ch", wav("f32", 1, 44100, _isolated(n, 26, [np.nan]))))
    out.append(("fe_f32_inf_2ch", wav("f32", 2, 44100, _isolated(n, 27, [np.inf, -np.inf]))))
    out.append(("fe_f64_inf_1ch", wav("f64", 1, 48000, _isolated(n, 28, [-np.inf]))))
    pair = _quiet(n, 29)
    pair[200:202] = F32_MAX
    pair[300:302] = [-F32_MAX, -3e38]
    out.append(("fe_f32_pair_overflow_2ch", wav("f32", 2, 44100, pair)))
    out.append(("fe_f32_fltmax_1ch", wav("f32", 1, 44100, _isolated(n, 30, [F32_MAX, -F32_MAX]))))
    # EXTENSIBLE float (rule 10: the library reads float where libnyquist reads integers)
    out.append(("fe_ext_f32_subnormal_2ch", wav("f32", 2, 44100, sub, extensible=3)))
    out.append(("fe_ext_f64_to_subnormal_1ch", wav("f64", 1, 22050, to_sub, extensible=3)))
    out.append(("fe_ext_f32_inf_1ch", wav("f32", 1, 44100, _isolated(n, 31, [np.inf]), extensible=3)))
    return out


def ima_wrap_wav():
    """one ADPCM block whose predictor overflows int16 at once: 32700 + 61 436 wraps to 28 600 (a clamp gives 32 767)"""
    data = struct.pack("<hBB", 32700, 88, 0) + bytes([0x77] * 4) * 63
    return riff([fmt_chunk(0x11, 1, 22050, 4, block_align=256, size=20), chunk("fact", struct.pack("<I", 504)), chunk("data", data)])


def ima_huge_fact_wav():
    """one 256-byte ADPCM block with fact = 0xFFFFFFF0: 4 294 967 280 values, more than the walk indexes"""
    vals = signal("s16", 600, 5, 0.5)
    data, _ = ima_encode(vals, 1, 256, 5)
    return riff([fmt_chunk(0x11, 1, 22050, 4, block_align=256, size=20), chunk("fact", struct.pack("<I", 0xFFFFFFF0)),
                 chunk("data", data[:256])])


def long_wav(seconds=180, rate=44100, seed=0x180):
    """the long file: 16-bit stereo, `seconds` at `rate`, a seeded tone at -6 dB plus noise"""
    n = seconds * rate
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    left = 0.35 * np.sin(2 * np.pi * 440.0 * t / rate) + 0.1 * (rng.random(n) * 2 - 1)
    right = 0.35 * np.sin(2 * np.pi * 523.25 * t / rate) + 0.1 * (rng.random(n) * 2 - 1)
    v = np.round(np.stack([left, right], axis=1).reshape(-1) * 32767).astype("<i2")
    return riff([fmt_chunk(1, 2, rate, 16), chunk("data", v.tobytes())])


def sha256(b):
    return hashlib.sha256(b).hexdigest()
