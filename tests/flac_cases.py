"""Seeded FLAC files for dcs_flac_parse / dcs_flac_decode / dcs_encode_files tests: every case is a recipe (name -> bytes), so
no FLAC bytes are committed.  The writer works from the decoder's side: it chooses warm-ups, coefficients and small residuals,
runs the predictor recurrence, and retries while a sample leaves its depth, so every stream is valid by construction and uses
exactly the subframe type, order, precision, shift, Rice parameters, partition order and escapes the case asks for (an
encoder would choose them itself).  cases() are files the reference loads; refused_cases() hold one file per clause of
INTEGRATION.md "Encoding files" rules 20-25."""
import functools
import struct

import numpy as np

INVALID_ARG, BAD_STREAM = -1, -6
RATE_CODES = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}
FIXED_TAPS = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}


# ------------------------------------------------------------------------------------------------------------ bit level

class BitWriter:
    def __init__(self):
        self.buf, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, k):
        if k == 0:
            return
        self.acc = (self.acc << k) | (int(v) & ((1 << k) - 1))
        self.n += k
        while self.n >= 8:
            self.n -= 8
            self.buf.append((self.acc >> self.n) & 0xFF)
        self.acc &= (1 << self.n) - 1

    def unary(self, q):
        while q >= 32:
            self.put(0, 32)
            q -= 32
        self.put(1, q + 1)

    def align(self, fill=0):
        if self.n:
            self.put(fill, 8 - self.n)

    def bytes(self):
        assert self.n == 0
        return bytes(self.buf)


def _table(poly, width):
    top, mask = 1 << (width - 1), (1 << width) - 1
    t = []
    for i in range(256):
        c = i << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        t.append(c)
    return t


CRC8_TABLE, CRC16_TABLE = _table(0x07, 8), _table(0x8005, 16)


def crc8(data):
    c = 0
    for b in data:
        c = CRC8_TABLE[c ^ b]
    return c


def crc16(data, c=0):
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ CRC16_TABLE[(c >> 8) ^ b]
    return c


def utf8(v):
    """FLAC's extended UTF-8 coding of a frame or sample number (up to 36 bits)"""
    if v < 0x80:
        return bytes([v])
    n = 2
    while v >= 1 << (5 * n + 1):
        n += 1
    out = [((0xFF << (8 - n)) & 0xFF) | (v >> (6 * (n - 1)))]
    for i in range(n - 2, -1, -1):
        out.append(0x80 | ((v >> (6 * i)) & 0x3F))
    return bytes(out)


# ------------------------------------------------------------------------------------------------------------ subframes

def S(t, order=0, prec=0, shift=0, method=0, po=0, k=3, wasted=0, amp=None, values=None, exact=None):
    """a subframe recipe: t in const / verbatim / fixed / lpc; k: one Rice parameter for every partition or a list with one
    entry per partition, an entry being a parameter or ('esc', raw width); values: the samples themselves (verbatim / const);
    exact: (warm-ups, LPC coefficients, residuals) of a fixed or LPC subframe as the caller chose them, in the subframe's own
    depth (after the wasted bits are taken off) -- residuals of any size, nothing drawn, nothing capped at 6 << k; the writer
    still runs the recurrence and asserts that every sample stays inside its depth"""
    return dict(t=t, order=order, prec=prec, shift=shift, method=method, po=po, k=k, wasted=wasted, amp=amp, values=values,
                exact=exact)


def _coefs(rng, order, prec, shift):
    lo, hi = -(1 << (prec - 1)), (1 << (prec - 1)) - 1
    if shift == 0 or prec == 1:
        c = [0] * order                                     # integer taps must sum to at most 1: one tap of -1
        c[int(rng.integers(order))] = -1
        return c
    c = rng.integers(lo, hi + 1, order).astype(np.int64)
    total = int(np.abs(c).sum())
    limit = int(0.9 * (1 << shift))
    if total > limit:
        c = c * limit // total
    return [int(x) for x in c]


def _partition_counts(bs, order, po):
    per = bs >> po
    return [per - (order if p == 0 else 0) for p in range(1 << po)]


def make_subframe(rng, bs, bits, spec):
    """-> (write(bitwriter), samples as the decoder restores them, before the channel assignment is undone)"""
    w = spec["wasted"]
    eff = bits - w
    lo, hi = -(1 << (eff - 1)), (1 << (eff - 1)) - 1
    t = spec["t"]
    if t in ("const", "verbatim"):
        n = 1 if t == "const" else bs
        if spec["values"] is not None:
            v = [int(x) for x in spec["values"]]
            assert len(v) == n and all(lo <= (x >> w) <= hi and (x >> w) << w == x for x in v)
            v = [x >> w for x in v]
        else:
            a = spec["amp"] if spec["amp"] is not None else int(0.45 * hi)
            v = [int(x) for x in rng.integers(-a, a + 1, n)]

        def write(bw):
            bw.put((0 if t == "const" else 1) << 1 | (1 if w else 0), 8)
            if w:
                bw.unary(w - 1)
            for x in v:
                bw.put(x, eff)
        full = v * bs if t == "const" else v
        return write, [x << w for x in full]
    order, method, po = spec["order"], spec["method"], spec["po"]
    plen = 5 if method else 4
    counts = _partition_counts(bs, order, po)
    assert (bs >> po) << po == bs and counts[0] >= 0
    ks = spec["k"] if isinstance(spec["k"], list) else [spec["k"]] * len(counts)
    assert len(ks) == len(counts)
    amp0 = spec["amp"] if spec["amp"] is not None else max(1, hi >> 6)
    for attempt in range(40 if spec.get("exact") is None else 0):
        amp = max(1, amp0 >> attempt)
        if t == "lpc":
            prec, shift = spec["prec"], spec["shift"]
            coefs = _coefs(rng, order, prec, shift)
        else:
            prec, shift, coefs = 0, 0, FIXED_TAPS[order]
        warm = [int(x) for x in rng.integers(-amp * 4, amp * 4 + 1, order)]
        res = []
        for c, k in zip(counts, ks):
            if isinstance(k, tuple):
                width = k[1]
                a = 0 if width == 0 else min(amp, (1 << (width - 1)) - 1)
                part = rng.integers(-a - (1 if width else 0), a + 1, c)
                if 0 < width <= 18 and c:
                    part[0] = -(1 << (width - 1))           # the raw field's most negative value
            else:
                a = min(amp, 6 << k)
                part = rng.integers(-a, a + 1, c)
            res += [int(x) for x in part]
        data = list(warm)
        ok = all(lo <= x <= hi for x in data)
        for r in res:
            s = 0
            for j in range(order):
                s += coefs[j] * data[-1 - j]
            v = r + (s >> shift)
            if not lo <= v <= hi:
                ok = False
                break
            data.append(v)
        if ok:
            break
    else:
        if spec.get("exact") is None:
            raise AssertionError("no stable signal for %r" % (spec,))
        prec, shift = (spec["prec"], spec["shift"]) if t == "lpc" else (0, 0)
        warm, coefs, res = ([int(x) for x in part] for part in spec["exact"])
        coefs = coefs if t == "lpc" else FIXED_TAPS[order]
        assert len(warm) == len(coefs) == order and len(res) == sum(counts)
        assert t != "lpc" or all(-(1 << (prec - 1)) <= c < 1 << (prec - 1) for c in coefs)
        i = 0
        for c, k in zip(counts, ks):                       # (an escape's residuals must fit its raw width)
            if isinstance(k, tuple):
                assert all(-(1 << k[1]) <= 2 * r < 1 << k[1] for r in res[i:i + c]), (k, res[i:i + c])
            i += c
        data = list(warm)
        for r in res:
            data.append(r + (sum(coefs[j] * data[-1 - j] for j in range(order)) >> shift))
        assert all(lo <= x <= hi for x in data), "an exact recipe leaves its depth"

    def write(bw):
        code = 8 + order if t == "fixed" else 32 + order - 1
        bw.put(code << 1 | (1 if w else 0), 8)
        if w:
            bw.unary(w - 1)
        for x in warm:
            bw.put(x, eff)
        if t == "lpc":
            bw.put(prec - 1, 4)
            bw.put(shift, 5)
            for c in coefs:
                bw.put(c, prec)
        bw.put(method, 2)
        bw.put(po, 4)
        i = 0
        for c, k in zip(counts, ks):
            if isinstance(k, tuple):
                bw.put((1 << plen) - 1, plen)
                bw.put(k[1], 5)
                for r in res[i:i + c]:
                    bw.put(r, k[1])
            else:
                bw.put(k, plen)
                for r in res[i:i + c]:
                    u = (r << 1) if r >= 0 else ((-r) << 1) - 1
                    bw.unary(u >> k)
                    bw.put(u, k)
            i += c
    return write, [x << w for x in data]


# --------------------------------------------------------------------------------------------------------------- frames

def block_size_code(bs, explicit=None):
    if explicit is not None:
        return explicit
    if bs == 192:
        return 1
    for n in range(4):
        if bs == 576 << n:
            return 2 + n
    for n in range(8):
        if bs == 256 << n:
            return 8 + n
    return 6 if bs <= 256 else 7


def frame_header(number, bs, assign, variable=False, bs_code=None, rate_code=0, size_code=0):
    code = block_size_code(bs, bs_code)
    h = bytearray([0xFF, 0xF8 | (1 if variable else 0), code << 4 | rate_code, assign << 4 | size_code << 1])
    h += utf8(number)
    if code == 6:
        h.append(bs - 1)
    elif code == 7:
        h += struct.pack(">H", bs - 1)
    if rate_code == 12:
        h.append(44)
    elif rate_code == 13:
        h += struct.pack(">H", 44100)
    elif rate_code == 14:
        h += struct.pack(">H", 4410)
    h.append(crc8(h))
    return bytes(h)


def undo_assignment(assign, a, b):
    if assign == 8:
        return a, [x - y for x, y in zip(a, b)]
    if assign == 9:
        return [x + y for x, y in zip(a, b)], b
    if assign == 10:
        left, right = [], []
        for m, s in zip(a, b):
            m = (m << 1) | (s & 1)
            left.append((m + s) >> 1)
            right.append((m - s) >> 1)
        return left, right
    return a, b


def make_frame(rng, number, bs, bits, channels, assign, subs, **hdr):
    """-> (frame bytes, per-channel decoded integers).  subs: one recipe per channel"""
    for attempt in range(60):
        bw = BitWriter()
        chans = []
        for ch in range(channels):
            side = (assign == 8 and ch == 1) or (assign == 9 and ch == 0) or (assign == 10 and ch == 1)
            write, data = make_subframe(rng, bs, bits + (1 if side else 0), subs[ch])
            write(bw)
            chans.append(data)
        if channels == 2:
            chans = list(undo_assignment(assign, chans[0], chans[1]))
        lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        if all(lo <= x <= hi for c in chans for x in c):
            break
    else:
        raise AssertionError("no frame whose channels fit their depth")
    bw.align()
    body = frame_header(number, bs, assign, **hdr) + bw.bytes()
    return body + struct.pack(">H", crc16(body)), chans


def metadata_block(kind, payload, last=False):
    return bytes([(0x80 if last else 0) | kind]) + struct.pack(">I", len(payload))[1:] + payload


def streaminfo(min_bs, max_bs, rate, channels, bits, total):
    v = (rate << 44) | ((channels - 1) << 41) | ((bits - 1) << 36) | total
    return struct.pack(">HH", min_bs, max_bs) + bytes(6) + v.to_bytes(8, "big") + bytes(16)


def flac_file(rate, channels, bits, frames, total=None, extra=(), prefix=b"", trailer=b""):
    """frames: [(bytes, chans)].  -> (file bytes, interleaved decoded integers)"""
    sizes = [len(c[0]) for _, c in frames]
    n = sum(sizes)
    total = n if total is None else total
    blocks = [(0, streaminfo(min(sizes[:-1] or sizes), max(sizes), rate, channels, bits, total))] + list(extra)
    meta = b"".join(metadata_block(k, p, i == len(blocks) - 1) for i, (k, p) in enumerate(blocks))
    inter = []
    for _, chans in frames:
        for i in range(len(chans[0])):
            for c in chans:
                inter.append(c[i])
    return prefix + b"fLaC" + meta + b"".join(b for b, _ in frames) + trailer, inter


def simple(seed, rate, channels, bits, specs, variable=False, total=None, extra=(), prefix=b"", trailer=b"", **hdr):
    """specs: [(block size, assignment code, [recipe per channel], header options)] -> (file bytes, interleaved integers)"""
    rng = np.random.default_rng(seed)
    frames, sample = [], 0
    for k, spec in enumerate(specs):
        bs, assign, subs = spec[:3]
        opts = dict(hdr)
        opts.update(spec[3] if len(spec) > 3 else {})
        frames.append(make_frame(rng, sample if variable else k, bs, bits, channels, assign, subs, variable=variable, **opts))
        sample += bs
    return flac_file(rate, channels, bits, frames, total, extra, prefix, trailer)


# ---------------------------------------------------------------------------------------------------------------- cases

def _assign_specs(bs):
    lpc = S("lpc", order=4, prec=12, shift=11, k=4)
    fx = S("fixed", order=2, k=3, po=1)
    return [(bs, 1, [lpc, fx]), (bs, 8, [lpc, fx]), (bs, 9, [fx, lpc]), (bs, 10, [lpc, S("fixed", order=1, k=2)]),
            (bs, 10, [S("verbatim"), S("verbatim", amp=9)]), (bs, 8, [S("const"), S("const", amp=5)])]


def _sync_trap():
    """the next frame's own header bytes planted in verbatim data: a candidate start with a good CRC-8 and the expected
    number, which only the CRC-16 of the span tells from the real one"""
    rng = np.random.default_rng(77)
    fake = frame_header(1, 32, 0)
    fake += b"\0" * (len(fake) % 2)
    planted = [int(x) for x in np.frombuffer(fake, ">i2")]
    vals = [int(x) for x in rng.integers(-900, 900, 32)]
    vals[5:5 + len(planted)] = planted
    vals[20] = -8                                            # FF F8 again, with no header behind it
    frames = [make_frame(rng, 0, 32, 16, 1, 0, [S("verbatim", values=vals)]),
              make_frame(rng, 1, 32, 16, 1, 0, [S("fixed", order=2, k=4)]),
              make_frame(rng, 2, 32, 16, 1, 0, [S("lpc", order=3, prec=10, shift=9, k=4)])]
    return flac_file(22050, 1, 16, frames)


def _realistic():
    specs = []
    left = 44100
    while left > 0:
        bs = min(4096, left)
        specs.append((bs, 10 if len(specs) % 2 else 8, [S("lpc", order=8, prec=12, shift=11, method=0, po=3 if bs == 4096 else 0, k=7,
                                                          amp=300),
                                                        S("lpc", order=6, prec=12, shift=11, po=2 if bs == 4096 else 0, k=5, amp=60)]))
        left -= bs
    return simple(4410, 44100, 2, 16, specs)


def _block_sizes():
    sizes = [192, 576, 1152, 2304, 4608, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768]
    specs = [(bs, 0, [S("fixed", order=0, k=10 + i % 3, amp=6000)]) for i, bs in enumerate(sizes)]
    specs += [(100, 0, [S("fixed", order=3, k=4)]), (300, 0, [S("fixed", order=1, k=3)], dict(bs_code=7)),
              (256, 0, [S("fixed", order=1, k=3)], dict(bs_code=6)), (1, 0, [S("verbatim")])]
    return simple(55, 32000, 1, 16, specs, variable=True)


@functools.lru_cache(maxsize=None)
def _built():
    """[(name, file bytes, interleaved decoded integers, (rate, channels, bits))]"""
    out = []

    def add(name, rate, channels, bits, built):
        out.append((name, built[0], np.asarray(built[1], np.int64), (rate, channels, bits)))

    add("types_s16_mono", 8000, 1, 16, simple(1, 8000, 1, 16, [
        (32, 0, [S("const")]), (32, 0, [S("verbatim")]), (32, 0, [S("fixed", order=0, k=5)]), (32, 0, [S("fixed", order=1, k=4)]),
        (32, 0, [S("fixed", order=2, k=3)]), (32, 0, [S("fixed", order=3, k=2, po=1)]), (32, 0, [S("fixed", order=4, k=2, po=2)]),
        (32, 0, [S("lpc", order=1, prec=8, shift=7, k=4)])]))
    add("lpc_orders_s16_mono", 16000, 1, 16, simple(2, 16000, 1, 16, [
        (48, 0, [S("lpc", order=1, prec=1, shift=0, k=3)]), (48, 0, [S("lpc", order=2, prec=12, shift=14, k=3)]),
        (48, 0, [S("lpc", order=8, prec=15, shift=14, k=4)]), (48, 0, [S("lpc", order=12, prec=12, shift=0, k=2)]),
        (48, 0, [S("lpc", order=32, prec=15, shift=14, k=3)]), (48, 0, [S("lpc", order=32, prec=15, shift=0, k=3)]),
        (48, 0, [S("lpc", order=8, prec=1, shift=14, k=3)]), (48, 0, [S("lpc", order=12, prec=12, shift=14, k=5, po=2)])]))
    esc = lambda w: ("esc", w)
    add("rice_s24_mono", 24000, 1, 24, simple(3, 24000, 1, 24, [
        (64, 0, [S("fixed", order=1, method=0, k=0)]), (64, 0, [S("fixed", order=2, method=0, k=14, po=1, amp=20000)]),
        (64, 0, [S("fixed", order=0, method=1, k=0)]), (64, 0, [S("lpc", order=2, prec=9, shift=8, method=1, k=30, po=2)]),
        (64, 0, [S("fixed", order=1, method=0, k=esc(0))]), (64, 0, [S("fixed", order=2, method=0, k=esc(9))]),
        (64, 0, [S("fixed", order=0, method=1, k=esc(0))]), (64, 0, [S("fixed", order=1, method=1, k=esc(17), amp=40000)]),
        (64, 0, [S("fixed", order=1, method=0, po=6, k=[(i * 5) % 15 for i in range(64)])]),
        (64, 0, [S("fixed", order=0, method=1, po=6, k=[(i * 7) % 31 for i in range(64)])]),
        (64, 0, [S("lpc", order=4, prec=10, shift=9, method=1, po=3, k=[2, esc(6), 0, esc(0), 30, 5, esc(24), 1], amp=3000)])]))
    add("wasted_s16_stereo", 22050, 2, 16, simple(4, 22050, 2, 16, [
        (32, 1, [S("lpc", order=2, prec=8, shift=7, k=3, wasted=3), S("fixed", order=1, k=3)]),
        (32, 1, [S("fixed", order=2, k=2, wasted=2), S("lpc", order=3, prec=9, shift=8, k=2, wasted=5)]),
        (32, 1, [S("verbatim", wasted=1), S("const", wasted=9)]),
        (32, 10, [S("fixed", order=1, k=3, wasted=2), S("fixed", order=1, k=2, wasted=1)]),
        (32, 8, [S("verbatim", wasted=4), S("verbatim", wasted=11, amp=3)])]))
    add("assign_s8_stereo", 11025, 2, 8, simple(5, 11025, 2, 8, _assign_specs(24), size_code=1, rate_code=0))
    add("assign_s16_stereo", 48000, 2, 16, simple(6, 48000, 2, 16, _assign_specs(40), size_code=4, rate_code=10))
    add("assign_s24_stereo", 96000, 2, 24, simple(7, 96000, 2, 24, _assign_specs(16), size_code=6, rate_code=11))
    add("block_sizes_variable_mono", 32000, 1, 16, _block_sizes())
    add("fixed_short_last_mono", 12000, 1, 16, simple(8, 12000, 1, 16, [(16, 0, [S("fixed", order=2, k=3)])] * 5 + [(1, 0, [S("verbatim")])]))
    add("rate_codes_mono", 44100, 1, 16, simple(9, 44100, 1, 16, [(16, 0, [S("fixed", order=1, k=3)], dict(rate_code=c)) for c in range(1, 15)]))
    add("frames_300_mono", 31250, 1, 16, simple(10, 31250, 1, 16, [(16, 0, [S("fixed", order=i % 5, k=3)]) for i in range(300)]))
    add("one_frame_65535_s8", 8000, 1, 8, simple(11, 8000, 1, 8, [(65535, 0, [S("lpc", order=2, prec=8, shift=7, k=2, amp=3)])]))
    add("realistic_44100_stereo", 44100, 2, 16, _realistic())
    add("stereo_odd_total", 31250, 2, 16, simple(12, 31250, 2, 16, [(16, 8, [S("fixed", order=1, k=3), S("fixed", order=0, k=2)])] * 2
                                                 + [(1, 1, [S("verbatim"), S("const")])]))
    picture = bytes(np.random.default_rng(13).integers(0, 256, 70000, dtype=np.uint8))
    add("metadata_blocks_mono", 8000, 1, 16, simple(13, 8000, 1, 16, [(32, 0, [S("fixed", order=2, k=3)])] * 3, extra=[
        (1, bytes(40)), (3, bytes(18 * 3)), (4, struct.pack("<I", 4) + b"test" + struct.pack("<I", 0)), (6, picture),
        (2, b"abcd" + bytes(12)), (1, b"")]))
    add("id3v2_prefix_mono", 8000, 1, 16, simple(14, 8000, 1, 16, [(32, 0, [S("lpc", order=2, prec=7, shift=6, k=3)])] * 2,
                                                 prefix=b"ID3\x03\x00\x00" + bytes([0, 0, 1, 5]) + bytes(133)))
    add("sync_trap_mono", 22050, 1, 16, _sync_trap())
    short = simple(15, 8000, 1, 16, [(32, 0, [S("fixed", order=1, k=3)])] * 2, total=100)
    add("total_larger_zero_tail", 8000, 1, 16, (short[0], short[1] + [0] * 36))
    two = [(32, 0, [S("fixed", order=1, k=3)])] * 2
    add("trailing_zeros", 8000, 1, 16, simple(16, 8000, 1, 16, two, trailer=bytes(128)))
    add("trailing_id3v1", 8000, 1, 16, simple(17, 8000, 1, 16, two, trailer=b"TAG" + bytes(125)))
    add("trailing_random", 8000, 1, 16, simple(18, 8000, 1, 16, two,
                                               trailer=bytes(np.random.default_rng(18).integers(0, 0xF0, 200, dtype=np.uint8))))
    fs16 = [-32768, 32767, -32768, 0] * 60
    add("fullscale_s16_31250", 31250, 1, 16, simple(19, 31250, 1, 16, [(240, 0, [S("verbatim", values=fs16)])]))
    fs8 = [-128, 127, -128, 0] * 60
    add("fullscale_s8_31250", 31250, 1, 8, simple(20, 31250, 1, 8, [(240, 0, [S("verbatim", values=fs8)])]))
    return out


def cases():
    """[(name, FLAC file bytes)]: files the reference loads"""
    return [(n, b) for n, b, _, _ in _built()]


def integers():
    """{name: (interleaved decoded integers, (rate, channels, bits))} of cases(): what the writer ran the recurrence to"""
    return {n: (v, fmt) for n, _, v, fmt in _built()}


# -------------------------------------------------------------------------------------------------------------- refusals

def _reframe(body):
    """a frame from hand-made bytes: header + payload, with a correct CRC-16"""
    return body + struct.pack(">H", crc16(body))


def _raw_subframe_frame(number, bs, put):
    bw = BitWriter()
    put(bw)
    bw.align()
    return _reframe(frame_header(number, bs, 0) + bw.bytes())


def _good(rng, number, bs=32, bits=16, channels=1, assign=0, **hdr):
    sub = [S("fixed", order=1, k=3)] * channels
    return make_frame(rng, number, bs, bits, channels, assign, sub, **hdr)[0]


def _file(frames, rate=8000, channels=1, bits=16, total=None, bs=32, trailer=b""):
    total = bs * len(frames) if total is None else total
    return b"fLaC" + metadata_block(0, streaminfo(bs, bs, rate, channels, bits, total), True) + b"".join(frames) + trailer


@functools.lru_cache(maxsize=None)
def refused_cases():
    """[(name, bytes, status, where, rule)]: where = 'host' when dcs_flac_parse refuses the file, 'device' when a kernel does
    (dcs_flac_parse accepts it), 'plan' when only dcs_encode_files(_plan) does (the resampler's rate range)"""
    rng = np.random.default_rng(99)
    g = lambda k, **kw: _good(rng, k, **kw)
    out = []
    ok3 = [g(0), g(1), g(2)]
    out.append(("r20_ogg_flac", b"OggS" + bytes(24) + b"\x7fFLAC" + _file(ok3), INVALID_ARG, "host", 20))
    out.append(("r20_junk_before_marker", b"junk" + _file(ok3), INVALID_ARG, "host", 20))
    out.append(("r20_id3_length_misses_marker", b"ID3\x03\x00\x00" + bytes([0, 0, 0, 9]) + bytes(10) + _file(ok3), INVALID_ARG, "host", 20))
    for bits in (12, 20):
        fr = [make_frame(rng, k, 32, bits, 1, 0, [S("fixed", order=1, k=3)])[0] for k in range(2)]
        out.append(("r21_bits%d" % bits, _file(fr, bits=bits), INVALID_ARG, "host", 21))
    fr = [make_frame(rng, k, 32, 16, 3, 2, [S("fixed", order=1, k=3)] * 3)[0] for k in range(2)]
    out.append(("r21_3ch", _file(fr, channels=3), INVALID_ARG, "host", 21))
    out.append(("r21_frame_depth_differs", _file([g(0), make_frame(rng, 1, 32, 8, 1, 0, [S("fixed", order=1, k=2)], size_code=1)[0], g(2)]),
                BAD_STREAM, "host", 21))
    out.append(("r21_frame_channels_differ", _file([g(0), g(1, channels=2, assign=1), g(2)]), BAD_STREAM, "host", 21))
    out.append(("r22_total_zero", _file(ok3, total=0), BAD_STREAM, "host", 22))
    out.append(("r22_total_smaller", _file(ok3, total=50), BAD_STREAM, "host", 22))
    out.append(("r22_further_frame", _file(ok3, total=64), BAD_STREAM, "host", 22))
    flip = bytearray(ok3[1])
    flip[-1] ^= 0x40
    out.append(("r23_crc16_flipped", _file([ok3[0], bytes(flip), ok3[2]]), BAD_STREAM, "host", 23))
    flip = bytearray(ok3[2])
    flip[-2] ^= 0x01
    out.append(("r23_crc16_flipped_last", _file([ok3[0], ok3[1], bytes(flip)]), BAD_STREAM, "host", 23))
    flip = bytearray(ok3[1])
    flip[5] ^= 0x10                                          # the header's CRC-8
    out.append(("r23_crc8_flipped", _file([ok3[0], bytes(flip), ok3[2]]), BAD_STREAM, "host", 23))
    out.append(("r23_lost_sync", _file([ok3[0], b"\x12\x34\x56", ok3[1], ok3[2]]), BAD_STREAM, "host", 23))
    # (libFLAC does not compare frame numbers; the index does, and the span it then gives frame 0 fails F1's length check)
    out.append(("r23_wrong_frame_number", _file([ok3[0], g(2), g(3)]), BAD_STREAM, "device", 23))

    def reserved(bw):
        bw.put(2 << 1, 8)
        for _ in range(32):
            bw.put(5, 16)

    def first_bit(bw):
        bw.put(0x80 | 1 << 1, 8)
        for _ in range(32):
            bw.put(5, 16)

    def precision(bw):
        bw.put((32 + 1) << 1, 8)
        bw.put(3, 16)
        bw.put(4, 16)
        bw.put(15, 4)
        bw.put(5, 5)
        for _ in range(40):
            bw.put(0x5A, 8)

    def neg_shift(bw):
        bw.put(32 << 1, 8)                                   # LPC order 1
        bw.put(3, 16)
        bw.put(7, 4)                                         # precision 8
        bw.put(-2, 5)
        bw.put(1, 8)
        bw.put(0, 2)
        bw.put(0, 4)
        bw.put(2, 4)
        for _ in range(31):
            bw.unary(0)
            bw.put(1, 2)

    def depth(bw):
        bw.put(8 << 1, 8)                                    # FIXED order 0: the residual is the sample
        bw.put(0, 2)
        bw.put(0, 4)
        bw.put(14, 4)
        for i in range(32):
            bw.unary(5 if i == 7 else 0)                    # 5 << 14 | 1 = 81 921 -> -40 961, outside 16 bits
            bw.put(1, 14)

    def bad_partition(bw):                                   # order 3 does not divide a block of 20
        bw.put(8 << 1, 8)
        bw.put(0, 2)
        bw.put(3, 4)
        for p in range(8):
            bw.put(2, 4)
            for _ in range(2):
                bw.unary(0)
                bw.put(1, 2)

    def overrun(bw):                                         # a unary run that never ends inside the frame
        bw.put(8 << 1, 8)
        bw.put(0, 2)
        bw.put(0, 4)
        bw.put(0, 4)
        for _ in range(40):
            bw.put(0, 8)

    for name, put, bs in (("r23_reserved_subframe_type", reserved, 32), ("r23_first_bit_nonzero", first_bit, 32),
                          ("r23_lpc_precision_1111", precision, 32), ("r23_negative_lpc_shift", neg_shift, 32),
                          ("r23_sample_outside_depth", depth, 32), ("r23_partition_order_does_not_divide", bad_partition, 20),
                          ("r23_unary_overrun", overrun, 32)):
        mid = _raw_subframe_frame(1, bs, put)
        if bs == 32:
            out.append((name, _file([ok3[0], mid, ok3[2]]), BAD_STREAM, "device", 23))
            out.append((name + "_last", _file([ok3[0], g(1), _raw_subframe_frame(2, bs, put)]), BAD_STREAM,
                        "device" if put is depth else "host", 23))
        else:
            frames = [make_frame(rng, 0, 20, 16, 1, 0, [S("fixed", order=1, k=3)])[0], mid,
                      make_frame(rng, 2, 20, 16, 1, 0, [S("fixed", order=1, k=3)])[0]]
            out.append((name, _file(frames, bs=20), BAD_STREAM, "device", 23))
    body = ok3[1][:-2]
    out.append(("r23_length_mismatch", _file([ok3[0], _reframe(body + b"\0"), ok3[2]]), BAD_STREAM, "device", 23))

    def padded(bw):
        bw.put(8 << 1, 8)
        bw.put(0, 2)
        bw.put(0, 4)
        bw.put(1, 4)
        for _ in range(32):
            bw.unary(0)
            bw.put(1, 1)
        bw.put(1, 1)                                         # 83 bits: the padding starts with a 1
    out.append(("r23_padding_nonzero", _file([ok3[0], _raw_subframe_frame(1, 32, padded), ok3[2]]), BAD_STREAM, "device", 23))
    out.append(("r24_short_stream_trailing_zeros", _file(ok3, total=200, trailer=bytes(64)), BAD_STREAM, "device", 24))
    out.append(("r24_short_stream_trailing_junk", _file(ok3, total=200, trailer=b"\x01\x02\x03\x04\x05\x06\x07"), BAD_STREAM, "host", 24))
    out.append(("rate_2000_below_range", _file(ok3, rate=2000), INVALID_ARG, "plan", 0))
    return out
