"""Plain Python / numpy restatement of the FLAC reader as dcs_flac_parse / dcs_flac_index / dcs_flac_decode define it: the
metadata chain and the frame index (candidate starts confirmed by CRC-16), the walk of a frame's subframes (F1), the predictor
restore (F2), the channel assignment, the cut to the stream's width and libnyquist's conversion (F3), and EncodeFile's
downmix.  It decodes what libFLAC 1.3.1 decodes (stream_decoder.c) and converts as FlacDecoder.cpp / Common.cpp do, with the
library's numbered rules 20-24 ("Encoding files") where the reference crashes or gives silence."""
import functools

import numpy as np

from flac_cases import crc8, crc16

OK, INVALID_ARG, BAD_STREAM = 0, -1, -6
S16, S24, S8 = 1, 2, 7
FIXED_TAPS = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}


class Refused(Exception):
    def __init__(self, status, why):
        Exception.__init__(self, why)
        self.status = status


class BitReader:
    """MSB first over b[pos:end]; a read past the end raises Refused"""
    def __init__(self, b, pos, end):
        self.b, self.pos, self.end, self.acc, self.n, self.used = b, pos, end, 0, 0, 0

    def get(self, k):
        if k == 0:
            return 0
        while self.n < k:
            if self.pos >= self.end:
                raise Refused(BAD_STREAM, "a read past the frame's end")
            self.acc = (self.acc << 8) | self.b[self.pos]
            self.pos += 1
            self.n += 8
        self.n -= k
        v = (self.acc >> self.n) & ((1 << k) - 1)
        self.acc &= (1 << self.n) - 1
        self.used += k
        return v

    def signed(self, k):
        v = self.get(k)
        return v - (1 << k) if k and v >> (k - 1) else v

    def unary(self):
        q = 0
        while self.get(1) == 0:
            q += 1
        return q


def skip_id3(b):
    """skip_id3v2_tag_: 3 bytes of version and flags, four 7-bit size bytes -> the offset where fLaC must stand"""
    if b[:3] == b"ID3" and len(b) >= 14:
        return 10 + ((b[6] & 0x7F) << 21 | (b[7] & 0x7F) << 14 | (b[8] & 0x7F) << 7 | (b[9] & 0x7F))
    return 0


def candidates(b, start):
    """every 0xFF from start on, then the end of the file"""
    q = b.find(b"\xff", start)
    while q >= 0:
        yield q
        q = b.find(b"\xff", q + 1)
    yield len(b)


def header(b, pos, stream_bits):
    """read_frame_header_ -> dict or None"""
    if pos + 6 > len(b) or b[pos] != 0xFF or (b[pos + 1] & 0xFE) != 0xF8 or b[pos + 3] & 1:
        return None
    blocking = b[pos + 1] & 1
    bs_code, sr_code, ch, ss_code = b[pos + 2] >> 4, b[pos + 2] & 15, b[pos + 3] >> 4, (b[pos + 3] >> 1) & 7
    if bs_code == 0 or sr_code == 15 or ch > 10 or ss_code in (3, 7):
        return None
    q = pos + 4
    lead = b[q]
    q += 1
    if lead < 0x80:
        v, extra = lead, 0
    else:
        extra = 0
        while extra < 7 and lead & (0x40 >> extra):
            extra += 1
        if extra == 0 or extra > (6 if blocking else 5) or (lead == 0xFF):
            return None
        v = lead & ((0x3F >> extra))
    tail = {6: 1, 7: 2}.get(bs_code, 0) + {12: 1, 13: 2, 14: 2}.get(sr_code, 0)
    if q + extra + tail + 1 > len(b):
        return None
    for _ in range(extra):
        if b[q] & 0xC0 != 0x80:
            return None
        v = v << 6 | (b[q] & 0x3F)
        q += 1
    if bs_code == 1:
        bs = 192
    elif bs_code <= 5:
        bs = 576 << (bs_code - 2)
    elif bs_code == 6:
        bs = b[q] + 1
        q += 1
    elif bs_code == 7:
        bs = (b[q] << 8 | b[q + 1]) + 1
        q += 2
    else:
        bs = 256 << (bs_code - 8)
    q += {12: 1, 13: 2, 14: 2}.get(sr_code, 0)
    if crc8(b[pos:q]) != b[q]:
        return None
    return dict(blockSize=bs, headerLength=q + 1 - pos, channelAssignment=ch, channels=ch + 1 if ch < 8 else 2,
                bitsPerSample=[stream_bits, 8, 12, 0, 16, 20, 24, 0][ss_code], blockingStrategy=blocking, number=v)


def walk(b, pos, end, h):
    """F1: the subframes of the frame whose header h starts at pos, read up to `end` (the CRC-16 excluded)
    -> (subframes [dict(type, order, shift, wasted, bits, qlp, data)], bytes consumed after the header, padding bits)"""
    br = BitReader(b, pos + h["headerLength"], end)
    bs, assign = h["blockSize"], h["channelAssignment"]
    subs = []
    for ch in range(h["channels"]):
        side = (assign == 8 and ch == 1) or (assign == 9 and ch == 0) or (assign == 10 and ch == 1)
        bits = h["bitsPerSample"] + (1 if side else 0)
        head = br.get(8)
        if head & 0x80:
            raise Refused(BAD_STREAM, "a nonzero first subframe bit")
        wasted = 0
        if head & 1:
            wasted = br.unary() + 1
            if wasted >= bits:
                raise Refused(BAD_STREAM, "more wasted bits than bits")
            bits -= wasted
        t = (head >> 1) & 0x3F
        sub = dict(order=0, shift=0, wasted=wasted, bits=bits, qlp=[])
        if t == 0:
            sub["type"] = "const"
            sub["data"] = [br.signed(bits)] * bs
        elif t == 1:
            sub["type"] = "verbatim"
            sub["data"] = [br.signed(bits) for _ in range(bs)]
        elif 8 <= t <= 12 or t >= 32:
            lpc = t >= 32
            order = (t & 31) + 1 if lpc else t & 7
            if order > bs:
                raise Refused(BAD_STREAM, "a predictor order above the block size")
            data = [br.signed(bits) for _ in range(order)]
            if lpc:
                prec = br.get(4)
                if prec == 15:
                    raise Refused(BAD_STREAM, "LPC precision 1111")
                shift = br.signed(5)
                if shift < 0:
                    raise Refused(BAD_STREAM, "a negative LPC shift")
                qlp = [br.signed(prec + 1) for _ in range(order)]
            else:
                shift, qlp = 0, FIXED_TAPS[order]
            method = br.get(2)
            if method > 1:
                raise Refused(BAD_STREAM, "a reserved residual coding method")
            plen = 5 if method else 4
            po = br.get(4)
            per = bs >> po
            if per << po != bs or per < order:
                raise Refused(BAD_STREAM, "a partition order that does not fit the block")
            for p in range(1 << po):
                count = per - (order if p == 0 else 0)
                k = br.get(plen)
                if k == (1 << plen) - 1:
                    w = br.get(5)
                    data += [br.signed(w) for _ in range(count)]
                else:
                    for _ in range(count):
                        u = (br.unary() << k) | br.get(k)
                        data.append((u >> 1) ^ -(u & 1))
            sub.update(type="lpc" if lpc else "fixed", order=order, shift=shift, qlp=list(qlp), data=data)
        else:
            raise Refused(BAD_STREAM, "a reserved subframe type")
        subs.append(sub)
    pad = -br.used & 7
    if br.get(pad) != 0:
        raise Refused(BAD_STREAM, "nonzero padding")
    return subs, br.used // 8


def restore(sub):
    """F2: the recurrence over warm-ups and residuals; every restored sample must fit the subframe's depth (rule 23)"""
    order, shift, qlp, d = sub["order"], sub["shift"], sub["qlp"], sub["data"]
    lo, hi = -(1 << (sub["bits"] - 1)), (1 << (sub["bits"] - 1)) - 1
    out = list(d[:order])
    for r in d[order:]:
        s = 0
        for j in range(order):
            s += qlp[j] * out[-1 - j]
        v = r + (s >> shift)
        if not lo <= v <= hi:
            raise Refused(BAD_STREAM, "a restored sample outside its subframe's depth")
        out.append(v)
    return [x << sub["wasted"] for x in out]


@functools.lru_cache(maxsize=None)
def _read(b):
    """-> (info dict, frames [dict]); raises Refused"""
    d = {}
    if len(b) >= 1 << 32:
        raise Refused(INVALID_ARG, "4 GiB or more")
    pos = skip_id3(b)
    if b[pos:pos + 4] != b"fLaC":
        raise Refused(INVALID_ARG, "no fLaC marker")
    pos += 4
    last, first = False, True
    while not last:
        if pos + 4 > len(b):
            raise Refused(BAD_STREAM, "metadata past the end")
        last, kind, size = b[pos] >> 7, b[pos] & 0x7F, int.from_bytes(b[pos + 1:pos + 4], "big")
        pos += 4
        if pos + size > len(b):
            raise Refused(BAD_STREAM, "metadata past the end")
        if first:
            if kind != 0 or size != 34:
                raise Refused(BAD_STREAM, "STREAMINFO is not first")
            v = int.from_bytes(b[pos + 10:pos + 18], "big")
            d.update(minBlockSize=int.from_bytes(b[pos:pos + 2], "big"), maxBlockSize=int.from_bytes(b[pos + 2:pos + 4], "big"),
                     rate=v >> 44, channels=((v >> 41) & 7) + 1, bitDepth=((v >> 36) & 31) + 1, totalSamples=v & ((1 << 36) - 1))
            first = False
        pos += size
    d["firstFrameOffset"] = pos
    if d["bitDepth"] not in (8, 16, 24):
        raise Refused(INVALID_ARG, "bit depth")
    d["sampleFormat"] = {8: S8, 16: S16, 24: S24}[d["bitDepth"]]
    if d["channels"] not in (1, 2):
        raise Refused(INVALID_ARG, "channels")
    total = d["totalSamples"]
    if total == 0:
        raise Refused(BAD_STREAM, "total_samples 0")
    d["nValues"] = total * d["channels"]
    frames, sample = [], 0
    expected = lambda h, k, s: h["number"] == (s if h["blockingStrategy"] else k)
    while sample < total and pos < len(b):
        k = len(frames)
        h = header(b, pos, d["bitDepth"])
        if h is None:
            raise Refused(BAD_STREAM, "frame %d: lost sync" % k)
        if not expected(h, k, sample):
            raise Refused(BAD_STREAM, "frame %d: number" % k)
        if h["channels"] != d["channels"] or h["bitsPerSample"] != d["bitDepth"]:
            raise Refused(BAD_STREAM, "frame %d: differs from STREAMINFO" % k)
        bs = h["blockSize"]
        if sample + bs > total:
            raise Refused(BAD_STREAM, "frame %d: more samples than STREAMINFO says" % k)
        end = 0
        if sample + bs == total:
            _, used = walk(b, pos, len(b), h)               # the last frame libFLAC decodes ends where its subframes end
            end = pos + h["headerLength"] + used + 2
            if end > len(b) or crc16(b[pos:end]) != 0:
                raise Refused(BAD_STREAM, "frame %d: CRC-16" % k)
            more = header(b, end, d["bitDepth"])
            if more is not None and expected(more, k + 1, sample + bs):
                raise Refused(BAD_STREAM, "frame %d: more samples than STREAMINFO says" % (k + 1))
        else:
            crc, done = crc16(b[pos:pos + h["headerLength"]]), pos + h["headerLength"]
            for q in candidates(b, done + 2):                 # a false sync inside the frame fails the CRC-16 and is passed over
                if q < len(b):
                    nxt = header(b, q, d["bitDepth"])
                    if nxt is None or not expected(nxt, k + 1, sample + bs):
                        continue
                crc, done = crc16(b[done:q], crc), q
                if crc == 0:
                    end = q
                    break
            if end == 0:
                raise Refused(BAD_STREAM, "frame %d: no candidate confirms its CRC-16" % k)
        frames.append(dict(offset=pos, length=end - pos, blockSize=bs, firstSample=sample, channelAssignment=h["channelAssignment"],
                           bitsPerSample=h["bitsPerSample"], blockingStrategy=h["blockingStrategy"], headerLength=h["headerLength"]))
        sample += bs
        pos = end
    if not frames:
        raise Refused(BAD_STREAM, "no frames")
    d["nFrames"] = len(frames)
    return d, frames


def parse(b):
    """-> (status, dict of the DcsFlacInfo fields that apply)"""
    try:
        return OK, dict(_read(bytes(b))[0])
    except Refused as e:
        return e.status, dict(reason=str(e))


def index(b):
    """-> (status, [dict of the DcsFlacFrame fields])"""
    try:
        return OK, _read(bytes(b))[1]
    except Refused as e:
        return e.status, []


def cut(x, bits):
    """the memcpy of the low bits / 8 bytes of an int32, sign-extended"""
    x = np.asarray(x, np.int64) & ((1 << bits) - 1)
    return np.where(x >> (bits - 1), x - (1 << bits), x)


def to_float(x, bits):
    """ConvertToFloat32 for PCM_S8, PCM_16, PCM_24"""
    x = np.asarray(x, np.int64).astype(np.float32)
    if bits == 8:
        return x * (np.float32(1) / np.float32(127))
    return x / np.float32(32767 if bits == 16 else 8388608)


@functools.lru_cache(maxsize=None)
def _integers(b):
    d, frames = _read(b)
    C, bits = d["channels"], d["bitDepth"]
    out = np.zeros(d["nValues"], np.int64)                  # (samples no frame supplies stay 0)
    for f in frames:
        h = header(b, f["offset"], bits)
        subs, used = walk(b, f["offset"], f["offset"] + f["length"] - 2, h)
        if h["headerLength"] + used + 2 != f["length"]:
            raise Refused(BAD_STREAM, "a frame's parsed length differs from its indexed length")
        ch = [restore(s) for s in subs]
        if C == 2:
            a, s = ch
            assign = f["channelAssignment"]
            if assign == 8:
                ch = [a, [x - y for x, y in zip(a, s)]]
            elif assign == 9:
                ch = [[x + y for x, y in zip(a, s)], s]
            elif assign == 10:
                m = [(x << 1) | (y & 1) for x, y in zip(a, s)]
                ch = [[(x + y) >> 1 for x, y in zip(m, s)], [(x - y) >> 1 for x, y in zip(m, s)]]
        base = f["firstSample"] * C
        for c in range(C):
            out[base + c:base + f["blockSize"] * C:C] = ch[c]
    out = cut(out, bits)
    out.setflags(write=False)
    return out


def integers(b):
    """-> (status, the interleaved integers as libnyquist's write callback keeps them, info)"""
    try:
        return OK, _integers(bytes(b)), _read(bytes(b))[0]
    except Refused as e:
        return e.status, None, dict(reason=str(e))


def values(b):
    """NyquistIO::Load's floats (interleaved)"""
    st, x, d = integers(b)
    return to_float(x, d["bitDepth"])


def downmix(v, channels):
    """EncodeFile: (L + R) / 2.0f"""
    v = np.asarray(v, np.float32)
    return v if channels == 1 else (v[0::2] + v[1::2]) / np.float32(2)


def decode(b):
    """-> (status, mono float32 or None, info): dcs_flac_decode"""
    st, x, d = integers(b)
    if st != OK:
        return st, None, d
    return OK, downmix(to_float(x, d["bitDepth"]), d["channels"]), d
