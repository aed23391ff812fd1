// dcs_flac.hip.h -- native FLAC files for dcs_encode_files, read as the reference reads them: NyquistIO::Load picks
// FlacDecoder (FlacDecoder.cpp), which runs libFLAC 1.3.1 (stream_decoder.c), copies the low 1, 2 or 3 bytes of every decoded
// int32 and converts them with ConvertToFloat32 (Common.cpp: PCM_S8, PCM_16, PCM_24).  The FLAC reader only: included in
// dcs_encode.hip after dcs_wav.hip.h, whose WavFile and conversion helpers (wavScale, wavMean) it uses, and before
// dcs_encode_files.hip.h, whose driver (wavStageOnDevice, planFiles, encodeFiles) calls into this file; it shares that
// translation unit's floating-point contract.
//
//   F1 walk     flacWalkKernel     one lane per frame: the frame's subframes, serially, through a 64-bit bit window refilled
//                                  by dword loads (MSB first): headers, warm-ups, LPC parameters, Rice and escape coded
//                                  residuals.  Residuals and warm-ups go planar into an int32 staging buffer at
//                                  [first sample x channels + channel x block size + i], one descriptor per subframe beside
//                                  them.  Every read is bounded by the frame's bit length; the bits consumed, padded to a byte,
//                                  plus the CRC-16 must be the indexed length
//   F2 restore  flacRestoreKernel  one lane per (frame, channel): the predictor recurrence in place over the planar buffer,
//                                  64-bit sums, the order-many history and the taps in per-lane LDS columns; a sample outside
//                                  its subframe's depth flags the file; then the shift by the wasted bits
//   F3 mix      flacMixKernel      one workgroup strip per frame, one thread per sample: the channel assignment undone, the
//                                  value cut to the stream's width as the reference's memcpy cuts it, W1's conversion and
//                                  stereo mean, into the staged mono buffer at [first sample + i]
//
// The host reads the metadata and indexes the frames (flacParse): a frame ends where the next header with the expected number
// starts and the CRC-16 of the span is zero, so only the frame bytes go up and F1's lanes start independently.  The frame
// that completes STREAMINFO's sample count has no successor to look for; the host walks that one frame with F1's own
// routine (flacWalkFrame is host and device code) to find its end, as libFLAC stops there too and ignores what follows.
#pragma once

namespace {

enum { kFlacConstant = 0, kFlacVerbatim = 1, kFlacFixed = 2, kFlacLpc = 3 };
enum { kFlacErrParse = 1, kFlacErrLength = 2, kFlacErrDepth = 3, kFlacErrShift = 4 };      // (the smallest code of a frame is kept)

// what F1 leaves F2 for one subframe
struct FlacSub
{
    int32_t type;           // kFlac*; -1: the frame did not parse, F2 leaves it alone
    int32_t order, shift, wasted;
    int32_t bits;           // the effective depth: the frame's, + 1 for a side channel, - wasted
    int32_t reserved[3];
    int32_t qlp[32];
};

// one frame on the device
struct FlacFrameDev
{
    uint64_t byteOff;       // the frame's first byte in the uploaded blob
    uint64_t stageOff;      // its first int32 in the staging buffer: the file's base + first sample x channels
    uint64_t monoPos;       // its first mono sample in the staged buffer
    uint32_t length, hdrLen, blockSize;
    uint32_t file, frame;   // the file's index in the call's group, the frame's in the file
    int32_t assign, bps, channels, sampleFormat;
};

// The bit window: `n` valid bits at the top of `win`, zeros below them; `left` bits of the frame not yet consumed.  A read
// past the frame's end sets `bad` and gives zeros, and a load never starts at or beyond `end`.
struct FlacBits
{
    const uint8_t *p, *end;
    uint64_t win;
    int32_t n;
    int64_t left;
    bool bad;

    __host__ __device__ static uint32_t load32(const uint8_t *q, const uint8_t *end)
    {
#if defined(__HIP_DEVICE_COMPILE__)
        // (q is dword aligned; the dword may end up to 3 bytes past `end`, inside the blob's padding)
        return q < end ? __builtin_bswap32(*reinterpret_cast<const uint32_t *>(q)) : 0u;
#else
        uint32_t v = 0;
        for (int i = 0 ; i < 4 ; ++i)
            v = v << 8 | (q + i < end ? q[i] : 0u);
        return v;
#endif
    }
    __host__ __device__ void refill()
    {
        while (n <= 32)
        {
            win |= static_cast<uint64_t>(load32(p, end)) << (32 - n);
            n += 32;
            p += 4;
        }
    }
    __host__ __device__ void init(const uint8_t *first, const uint8_t *last)
    {
        int32_t skip = 0;
#if defined(__HIP_DEVICE_COMPILE__)
        skip = static_cast<int32_t>(reinterpret_cast<uintptr_t>(first) & 3u);
#endif
        p = first - skip;
        end = last;
        win = 0;
        n = 0;
        left = (last - first) * 8;
        bad = false;
        refill();
        win <<= 8 * skip;
        n -= 8 * skip;
    }
    __host__ __device__ uint32_t get(int32_t k)                 // 0 <= k <= 32
    {
        if (k > left)
        {
            bad = true;
            left = 0;
            return 0;
        }
        if (k == 0)
            return 0;
        refill();
        const uint32_t v = static_cast<uint32_t>(win >> (64 - k));
        win <<= k;
        n -= k;
        left -= k;
        return v;
    }
    __host__ __device__ int32_t getSigned(int32_t k)
    {
        if (k == 0)
            return 0;
        const uint32_t v = get(k);
        return static_cast<int32_t>(v << (32 - k)) >> (32 - k);
    }
    __host__ __device__ uint32_t unary()                        // zeros before the next 1, which is consumed
    {
        uint32_t count = 0;
        for (;;)
        {
            refill();
            if (win == 0)
            {
                count += static_cast<uint32_t>(n);
                left -= n;
                n = 0;
                if (left >= 0)
                    continue;
            }
            else
            {
                const int32_t z = __builtin_clzll(win);
                count += static_cast<uint32_t>(z);
                win = z == 63 ? 0 : win << (z + 1);             // (the run's one in the window's last bit: no shift by 64)
                n -= z + 1;
                left -= z + 1;
                if (left >= 0)
                    return count;
            }
            bad = true;
            left = 0;
            return 0;
        }
    }
};

// FLAC__fixed_restore_signal's formulas as taps (1; 2 -1; 3 -3 1; 4 -6 4 -1), four signed bytes an order
__host__ __device__ inline int32_t flacFixedTap(int32_t order, int32_t j)
{
    const uint32_t packed = order == 1 ? 0x00000001u : order == 2 ? 0x0000FF02u : order == 3 ? 0x0001FD03u : 0xFF04FA04u;
    return static_cast<int8_t>(packed >> (8 * j));
}

// read_subframe_* and read_residual_partitioned_rice_ (stream_decoder.c) for one frame after its header.  stage (null: only
// the length is wanted) takes warm-ups and residuals at [ch x blockSize + i], subs one descriptor per channel.  Returns 0 or
// a kFlacErr*; br.left is what the frame has left after the padding to a byte.
__host__ __device__ inline uint32_t flacWalkFrame(FlacBits &br, uint32_t bs, int32_t channels, int32_t assign, int32_t bps,
                                                  int32_t *stage, FlacSub *subs)
{
    for (int32_t ch = 0 ; ch < channels ; ++ch)
    {
        const bool side = (assign == 8 && ch == 1) || (assign == 9 && ch == 0) || (assign == 10 && ch == 1);
        int32_t bits = bps + (side ? 1 : 0);
        const uint32_t head = br.get(8);
        if (head & 0x80)
            return kFlacErrParse;
        int32_t wasted = 0;
        if (head & 1)
        {
            wasted = static_cast<int32_t>(br.unary()) + 1;
            if (br.bad || wasted >= bits)
                return kFlacErrParse;
            bits -= wasted;
        }
        const uint32_t t = (head >> 1) & 0x3F;
        int32_t type, order = 0;
        if (t == 0) type = kFlacConstant;
        else if (t == 1) type = kFlacVerbatim;
        else if (t >= 8 && t <= 12) { type = kFlacFixed; order = static_cast<int32_t>(t & 7); }
        else if (t >= 32) { type = kFlacLpc; order = static_cast<int32_t>(t & 31) + 1; }
        else return kFlacErrParse;
        if (static_cast<uint32_t>(order) > bs)
            return kFlacErrParse;
        int32_t *out = stage != nullptr ? stage + static_cast<uint64_t>(ch) * bs : nullptr;
        FlacSub *sub = subs != nullptr ? subs + ch : nullptr;
        int32_t shift = 0;
        if (type == kFlacConstant)
        {
            const int32_t v = br.getSigned(bits);
            if (out != nullptr)
                for (uint32_t i = 0 ; i < bs ; ++i)
                    out[i] = v;
        }
        else if (type == kFlacVerbatim)
        {
            for (uint32_t i = 0 ; i < bs && !br.bad ; ++i)
            {
                const int32_t v = br.getSigned(bits);
                if (out != nullptr)
                    out[i] = v;
            }
        }
        else
        {
            for (int32_t i = 0 ; i < order ; ++i)
            {
                const int32_t v = br.getSigned(bits);
                if (out != nullptr)
                    out[i] = v;
            }
            if (type == kFlacLpc)
            {
                const int32_t prec = static_cast<int32_t>(br.get(4));
                if (prec == 15)
                    return kFlacErrParse;
                shift = br.getSigned(5);
                if (shift < 0)
                    return kFlacErrShift;
                for (int32_t j = 0 ; j < order ; ++j)
                {
                    const int32_t c = br.getSigned(prec + 1);
                    if (sub != nullptr)
                        sub->qlp[j] = c;
                }
            }
            else if (sub != nullptr)
                for (int32_t j = 0 ; j < order ; ++j)
                    sub->qlp[j] = flacFixedTap(order, j);
            const uint32_t method = br.get(2);
            if (method > 1)
                return kFlacErrParse;
            const int32_t plen = method ? 5 : 4, esc = (1 << plen) - 1;
            const uint32_t po = br.get(4);
            const uint32_t per = bs >> po;
            if ((per << po) != bs || per < static_cast<uint32_t>(order))
                return kFlacErrParse;
            uint32_t i = static_cast<uint32_t>(order);
            for (uint32_t part = 0 ; part < (1u << po) && !br.bad ; ++part)
            {
                const uint32_t count = per - (part == 0 ? static_cast<uint32_t>(order) : 0u);
                const int32_t k = static_cast<int32_t>(br.get(plen));
                if (k == esc)
                {
                    const int32_t w = static_cast<int32_t>(br.get(5));
                    for (uint32_t c = 0 ; c < count && !br.bad ; ++c, ++i)
                    {
                        const int32_t v = br.getSigned(w);
                        if (out != nullptr && i < bs)
                            out[i] = v;
                    }
                }
                else
                    for (uint32_t c = 0 ; c < count && !br.bad ; ++c, ++i)
                    {
                        const uint32_t q = br.unary();
                        const uint32_t u = (q << k) | br.get(k);
                        const int32_t v = static_cast<int32_t>(u >> 1) ^ -static_cast<int32_t>(u & 1);
                        if (out != nullptr && i < bs)
                            out[i] = v;
                    }
            }
        }
        if (br.bad)
            return kFlacErrParse;
        if (sub != nullptr)
        {
            sub->type = type;
            sub->order = order;
            sub->shift = shift;
            sub->wasted = wasted;
            sub->bits = bits;
        }
    }
    const int32_t pad = static_cast<int32_t>(br.left & 7);
    if (br.get(pad) != 0)
        return kFlacErrLength;
    return 0;
}

// ------------------------------------------------------------------------------------------------------------- kernels

// F1
__global__ __launch_bounds__(64) void flacWalkKernel(const uint8_t *__restrict__ blob, const FlacFrameDev *__restrict__ frames,
                                                     uint32_t nFrames, int32_t *__restrict__ stage, FlacSub *__restrict__ subs,
                                                     uint32_t *__restrict__ err)
{
    for (uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x ; lane < nFrames ; lane += gridDim.x * blockDim.x)
    {
        const FlacFrameDev fr = frames[lane];
        const uint8_t *first = blob + fr.byteOff;
        FlacBits br;
        br.init(first + fr.hdrLen, first + fr.length - 2);
        uint32_t code = flacWalkFrame(br, fr.blockSize, fr.channels, fr.assign, fr.bps, stage + fr.stageOff, subs + 2 * uint64_t(lane));
        if (code == 0 && br.left != 0)
            code = kFlacErrLength;
        if (code != 0)
        {
            subs[2 * uint64_t(lane)].type = -1;
            subs[2 * uint64_t(lane) + 1].type = -1;
            atomicMin(&err[fr.file], fr.frame << 4 | code);
        }
    }
}

// F2: FLAC__lpc_restore_signal (and FLAC__fixed_restore_signal as taps with shift 0): data[i] = residual[i] + (sum >> shift).
// With every restored sample inside its depth the 64-bit sum equals the 32-bit one of libFLAC's narrow routines, which it
// picks only where bits + precision + log2(order) <= 32.
// (one channel of one frame; hist and taps are the lane's columns of 32 words, `stride` words apart)
__host__ __device__ inline bool flacRestoreChannel(int32_t *d, uint32_t bs, const FlacSub &sub, int32_t *hist, int32_t *taps,
                                                   uint32_t stride)
{
    const int32_t order = sub.order, shift = sub.shift, wasted = sub.wasted;
    const int64_t lo = -(int64_t(1) << (sub.bits - 1)), hi = (int64_t(1) << (sub.bits - 1)) - 1;
    for (int32_t j = 0 ; j < order ; ++j)
    {
        taps[j * stride] = sub.qlp[j];
        hist[j * stride] = d[j];
        d[j] = static_cast<int32_t>(static_cast<uint32_t>(d[j]) << wasted);
    }
    bool bad = false;
    for (uint32_t i = static_cast<uint32_t>(order) ; i < bs ; ++i)
    {
        int64_t sum = 0;
        for (int32_t j = 0 ; j < order ; ++j)
            sum += int64_t(taps[j * stride]) * hist[((i - 1 - static_cast<uint32_t>(j)) & 31) * stride];
        const int64_t v = int64_t(d[i]) + (sum >> shift);
        bad |= v < lo || v > hi;
        hist[(i & 31) * stride] = static_cast<int32_t>(v);
        d[i] = static_cast<int32_t>(static_cast<uint32_t>(v) << wasted);
    }
    return bad;
}

__global__ __launch_bounds__(64) void flacRestoreKernel(const FlacFrameDev *__restrict__ frames, uint32_t nFrames,
                                                        int32_t *__restrict__ stage, const FlacSub *__restrict__ subs,
                                                        uint32_t *__restrict__ err)
{
    __shared__ int32_t hist[32][64], taps[32][64];
    const uint32_t t = threadIdx.x;
    for (uint64_t lane = blockIdx.x * uint64_t(blockDim.x) + t ; lane < 2 * uint64_t(nFrames) ; lane += uint64_t(gridDim.x) * blockDim.x)
    {
        const FlacFrameDev &fr = frames[lane >> 1];
        const int32_t ch = static_cast<int32_t>(lane & 1);
        const FlacSub &sub = subs[lane];
        if (ch >= fr.channels || sub.type < 0)
            continue;
        const bool bad = flacRestoreChannel(stage + fr.stageOff + uint64_t(ch) * fr.blockSize, fr.blockSize, sub, &hist[0][t], &taps[0][t], 64);
        if (bad)
            atomicMin(&err[fr.file], fr.frame << 4 | kFlacErrDepth);
    }
}

// the low 1, 2 or 3 bytes of a decoded int32, sign-extended: what the reference's memcpy keeps
template <int F>
__host__ __device__ inline int32_t flacCut(int32_t x)
{
    if constexpr (F == DCS_WAV_S8)
        return static_cast<int8_t>(x);
    else if constexpr (F == DCS_WAV_S16)
        return static_cast<int16_t>(x);
    else
        return static_cast<int32_t>(static_cast<uint32_t>(x) << 8) >> 8;
}

// left/side, right/side and mid/side undone (stream_decoder.c, read_frame_); unsigned, so that corrupt data may wrap
__host__ __device__ inline void flacUndoAssignment(int32_t assign, int32_t &a, int32_t &b)
{
    const uint32_t ua = static_cast<uint32_t>(a), ub = static_cast<uint32_t>(b);
    if (assign == 8)
        b = static_cast<int32_t>(ua - ub);
    else if (assign == 9)
        a = static_cast<int32_t>(ua + ub);
    else if (assign == 10)
    {
        const uint32_t m = ua << 1 | (ub & 1);
        a = static_cast<int32_t>(m + ub) >> 1;
        b = static_cast<int32_t>(m - ub) >> 1;
    }
}

template <int F>
__device__ inline void flacMixFrame(const FlacFrameDev &fr, const int32_t *__restrict__ s, float *__restrict__ mono)
{
    const uint32_t bs = fr.blockSize;
    for (uint32_t i = threadIdx.x ; i < bs ; i += blockDim.x)
    {
        int32_t a = s[i];
        float x;
        if (fr.channels == 2)
        {
            int32_t b = s[bs + i];
            flacUndoAssignment(fr.assign, a, b);
            x = wavMean(wavScale<F>(flacCut<F>(a)), wavScale<F>(flacCut<F>(b)));
        }
        else
            x = wavScale<F>(flacCut<F>(a));
        mono[fr.monoPos + i] = x;
    }
}

// F3
__global__ __launch_bounds__(256) void flacMixKernel(const FlacFrameDev *__restrict__ frames, uint32_t nFrames,
                                                     const int32_t *__restrict__ stage, float *__restrict__ mono)
{
    for (uint32_t fi = blockIdx.x ; fi < nFrames ; fi += gridDim.x)
    {
        const FlacFrameDev &fr = frames[fi];
        const int32_t *s = stage + fr.stageOff;
        if (fr.sampleFormat == DCS_WAV_S8)
            flacMixFrame<DCS_WAV_S8>(fr, s, mono);
        else if (fr.sampleFormat == DCS_WAV_S16)
            flacMixFrame<DCS_WAV_S16>(fr, s, mono);
        else
            flacMixFrame<DCS_WAV_S24>(fr, s, mono);
    }
}

// ----------------------------------------------------------------------------------------------------------- host side

DcsStatus flacRefuse(DcsFlacInfo *w, DcsStatus st, const std::string &why)
{
    snprintf(w->reason, sizeof(w->reason), "%s", why.c_str());
    return st;
}

uint8_t flacCrc8(const uint8_t *p, uint64_t n)               // poly 0x07, init 0
{
    uint32_t c = 0;
    for (uint64_t i = 0 ; i < n ; ++i)
    {
        c ^= p[i];
        for (int b = 0 ; b < 8 ; ++b)
            c = (c & 0x80) ? ((c << 1) ^ 0x07) & 0xFF : (c << 1) & 0xFF;
    }
    return static_cast<uint8_t>(c);
}

const uint16_t *flacCrc16Table()                            // poly 0x8005, init 0, MSB first
{
    static const std::vector<uint16_t> table = [] {
        std::vector<uint16_t> t(256);
        for (uint32_t i = 0 ; i < 256 ; ++i)
        {
            uint32_t c = i << 8;
            for (int b = 0 ; b < 8 ; ++b)
                c = (c & 0x8000) ? ((c << 1) ^ 0x8005) & 0xFFFF : (c << 1) & 0xFFFF;
            t[i] = static_cast<uint16_t>(c);
        }
        return t;
    }();
    return table.data();
}

inline uint16_t flacCrc16(uint16_t c, const uint8_t *p, uint64_t n)
{
    const uint16_t *t = flacCrc16Table();
    for (uint64_t i = 0 ; i < n ; ++i)
        c = static_cast<uint16_t>((c << 8) ^ t[(c >> 8) ^ p[i]]);
    return c;
}

struct FlacHeader
{
    uint32_t blockSize, hdrLen;
    int32_t assign, bps, blocking, channels;
    uint64_t number;
};

// read_frame_header_ (stream_decoder.c): false where libFLAC would not take the bytes at pos for a frame header
bool flacHeader(const uint8_t *f, uint64_t len, uint64_t pos, int32_t streamBps, FlacHeader &h)
{
    if (pos + 6 > len)
        return false;
    const uint8_t *p = f + pos;
    if (p[0] != 0xFF || (p[1] & 0xFE) != 0xF8 || (p[3] & 1) != 0)
        return false;
    h.blocking = p[1] & 1;
    const int32_t bsCode = p[2] >> 4, srCode = p[2] & 15, ch = p[3] >> 4, ssCode = (p[3] >> 1) & 7;
    if (bsCode == 0 || srCode == 15 || ch > 10 || ssCode == 3 || ssCode == 7)
        return false;
    const uint64_t room = len - pos;
    uint64_t q = 4;
    const uint8_t lead = p[q++];
    int32_t extra;
    uint64_t v;
    if (!(lead & 0x80)) { v = lead; extra = 0; }
    else if ((lead & 0xE0) == 0xC0) { v = lead & 0x1F; extra = 1; }
    else if ((lead & 0xF0) == 0xE0) { v = lead & 0x0F; extra = 2; }
    else if ((lead & 0xF8) == 0xF0) { v = lead & 0x07; extra = 3; }
    else if ((lead & 0xFC) == 0xF8) { v = lead & 0x03; extra = 4; }
    else if ((lead & 0xFE) == 0xFC) { v = lead & 0x01; extra = 5; }
    else if (lead == 0xFE && h.blocking) { v = 0; extra = 6; }
    else return false;
    const int32_t tail = (bsCode == 6 ? 1 : bsCode == 7 ? 2 : 0) + (srCode == 12 ? 1 : srCode >= 13 ? 2 : 0);
    if (q + static_cast<uint64_t>(extra + tail) + 1 > room)
        return false;
    for (int32_t i = 0 ; i < extra ; ++i)
    {
        const uint8_t c = p[q++];
        if ((c & 0xC0) != 0x80)
            return false;
        v = v << 6 | (c & 0x3F);
    }
    h.number = v;
    if (bsCode == 1) h.blockSize = 192;
    else if (bsCode <= 5) h.blockSize = 576u << (bsCode - 2);
    else if (bsCode == 6) h.blockSize = uint32_t(p[q++]) + 1;
    else if (bsCode == 7) { h.blockSize = (uint32_t(p[q]) << 8 | p[q + 1]) + 1; q += 2; }
    else h.blockSize = 256u << (bsCode - 8);
    q += srCode == 12 ? 1 : srCode >= 13 ? 2 : 0;
    if (flacCrc8(p, q) != p[q])
        return false;
    h.hdrLen = static_cast<uint32_t>(q + 1);
    h.assign = ch;
    h.channels = ch < 8 ? ch + 1 : 2;
    const int32_t depth[8] = { streamBps, 8, 12, 0, 16, 20, 24, 0 };
    h.bps = depth[ssCode];
    return true;
}

bool isFlacFile(const uint8_t *f, uint64_t len)
{
    if (len >= 4 && memcmp(f, "fLaC", 4) == 0)
        return true;
    if (len < 14 || memcmp(f, "ID3", 3) != 0)
        return false;
    // skip_id3v2_tag_ (stream_decoder.c): 3 bytes of version and flags, four 7-bit size bytes
    const uint64_t skip = 10 + (uint64_t(f[6] & 0x7F) << 21 | uint64_t(f[7] & 0x7F) << 14 | uint64_t(f[8] & 0x7F) << 7 | uint64_t(f[9] & 0x7F));
    return skip + 4 <= len && memcmp(f + skip, "fLaC", 4) == 0;
}

// One file's metadata and frame index, with rules 20-24 of INTEGRATION.md "Encoding files".  frames may be null.
DcsStatus flacParse(const uint8_t *f, uint64_t len, DcsFlacInfo *w, std::vector<DcsFlacFrame> *frames)
{
    memset(w, 0, sizeof(*w));
    if (frames != nullptr)
        frames->clear();
    if (len >= (uint64_t(1) << 32))
        return flacRefuse(w, DCS_ERR_INVALID_ARG, "4 GiB or more");
    if (!isFlacFile(f, len))
        return flacRefuse(w, DCS_ERR_INVALID_ARG, "no fLaC marker at the start or after one ID3v2 tag (Ogg FLAC is not read)");
    uint64_t pos = f[0] == 'I' ? 10 + (uint64_t(f[6] & 0x7F) << 21 | uint64_t(f[7] & 0x7F) << 14 | uint64_t(f[8] & 0x7F) << 7 | uint64_t(f[9] & 0x7F)) : 0;
    pos += 4;
    bool last = false, first = true;
    while (!last)
    {
        if (pos + 4 > len)
            return flacRefuse(w, DCS_ERR_BAD_STREAM, "the metadata chain runs past the end of the file");
        last = (f[pos] & 0x80) != 0;
        const int32_t type = f[pos] & 0x7F;
        const uint64_t size = uint64_t(f[pos + 1]) << 16 | uint64_t(f[pos + 2]) << 8 | f[pos + 3];
        pos += 4;
        if (pos + size > len)
            return flacRefuse(w, DCS_ERR_BAD_STREAM, "a metadata block runs past the end of the file");
        if (first)
        {
            if (type != 0 || size != 34)
                return flacRefuse(w, DCS_ERR_BAD_STREAM, "the first metadata block is not a 34-byte STREAMINFO");
            const uint8_t *s = f + pos;
            w->minBlockSize = uint32_t(s[0]) << 8 | s[1];
            w->maxBlockSize = uint32_t(s[2]) << 8 | s[3];
            w->rate = uint32_t(s[10]) << 12 | uint32_t(s[11]) << 4 | s[12] >> 4;
            w->channels = ((s[12] >> 1) & 7) + 1;
            w->bitDepth = (((s[12] & 1) << 4) | (s[13] >> 4)) + 1;
            w->totalSamples = uint64_t(s[13] & 15) << 32 | uint64_t(s[14]) << 24 | uint64_t(s[15]) << 16 | uint64_t(s[16]) << 8 | s[17];
            first = false;
        }
        pos += size;
    }
    w->firstFrameOffset = pos;
    if (w->bitDepth != 8 && w->bitDepth != 16 && w->bitDepth != 24)
        return flacRefuse(w, DCS_ERR_INVALID_ARG, "a bit depth other than 8, 16 or 24 (libnyquist reads it as silence)");
    w->sampleFormat = w->bitDepth == 8 ? DCS_WAV_S8 : w->bitDepth == 16 ? DCS_WAV_S16 : DCS_WAV_S24;
    if (w->channels != 1 && w->channels != 2)
        return flacRefuse(w, DCS_ERR_INVALID_ARG, "channel count other than 1 or 2");
    if (w->totalSamples == 0)
        return flacRefuse(w, DCS_ERR_BAD_STREAM, "STREAMINFO gives no total sample count (the reference overruns its buffer)");
    w->nValues = w->totalSamples * static_cast<uint64_t>(w->channels);
    // the frame index
    uint64_t sample = 0;
    uint32_t k = 0;
    const auto at = [&](const char *what) { return "frame " + std::to_string(k) + ": " + what; };
    while (sample < w->totalSamples)
    {
        if (pos == len)
            break;                                          // fewer samples than STREAMINFO says: a zero tail, as in the reference
        FlacHeader h;
        if (!flacHeader(f, len, pos, w->bitDepth, h))
            return flacRefuse(w, DCS_ERR_BAD_STREAM, at("lost sync (no valid frame header where the frame should start)"));
        if (h.number != (h.blocking ? sample : k))
            return flacRefuse(w, DCS_ERR_BAD_STREAM, at("its frame or sample number is not the next one"));
        if (h.channels != w->channels || h.bps != w->bitDepth)
            return flacRefuse(w, DCS_ERR_BAD_STREAM, at("its channel count or sample size differs from STREAMINFO's"));
        if (sample + h.blockSize > w->totalSamples)
            return flacRefuse(w, DCS_ERR_BAD_STREAM, at("the frames hold more samples than STREAMINFO says (the reference overruns its buffer)"));
        uint64_t end = 0;
        if (sample + h.blockSize == w->totalSamples)
        {
            // the last frame libFLAC decodes: its end is where its subframes end
            FlacBits br;
            br.init(f + pos + h.hdrLen, f + len);
            const int64_t total = br.left;
            const uint32_t code = flacWalkFrame(br, h.blockSize, h.channels, h.assign, h.bps, nullptr, nullptr);
            if (code != 0)
                return flacRefuse(w, DCS_ERR_BAD_STREAM, at(code == kFlacErrShift ? "a negative LPC shift" : "its subframes do not parse"));
            end = pos + h.hdrLen + static_cast<uint64_t>(total - br.left) / 8 + 2;
            if (end > len || flacCrc16(0, f + pos, end - pos) != 0)
                return flacRefuse(w, DCS_ERR_BAD_STREAM, at("CRC-16 mismatch"));
            FlacHeader more;
            if (flacHeader(f, len, end, w->bitDepth, more) && more.number == (more.blocking ? sample + h.blockSize : k + 1))
            {
                ++k;
                return flacRefuse(w, DCS_ERR_BAD_STREAM, at("the frames hold more samples than STREAMINFO says (the reference overruns its buffer)"));
            }
        }
        else
        {
            // a candidate start confirms this frame when the CRC-16 of the span up to it is zero
            uint16_t crc = flacCrc16(0, f + pos, h.hdrLen);
            uint64_t done = pos + h.hdrLen;
            for (uint64_t q = pos + h.hdrLen + 2 ; end == 0 && q <= len ; ++q)
            {
                FlacHeader next;
                if (q < len && !(f[q] == 0xFF && flacHeader(f, len, q, w->bitDepth, next)
                                 && next.number == (next.blocking ? sample + h.blockSize : k + 1)))
                    continue;
                crc = flacCrc16(crc, f + done, q - done);
                done = q;
                if (crc == 0)
                    end = q;
            }
            if (end == 0)
                return flacRefuse(w, DCS_ERR_BAD_STREAM, at("no following frame or end of file confirms its CRC-16"));
        }
        if (frames != nullptr)
            frames->push_back(DcsFlacFrame{ pos, static_cast<uint32_t>(end - pos), h.blockSize, sample, h.assign, h.bps, h.blocking,
                                            static_cast<int32_t>(h.hdrLen) });
        sample += h.blockSize;
        pos = end;
        ++k;
    }
    if (k == 0)
        return flacRefuse(w, DCS_ERR_BAD_STREAM, "no frames");
    w->nFrames = k;
    return DCS_OK;
}

const char *flacErrText(uint32_t code)
{
    switch (code)
    {
        case kFlacErrLength: return "its parsed length differs from its indexed length, or its padding is not zero";
        case kFlacErrDepth: return "a restored sample lies outside its subframe's depth";
        case kFlacErrShift: return "a negative LPC shift";
        default: return "its subframes do not parse (reserved type, nonzero first bit, invalid precision or partition order, or a read past its end)";
    }
}

std::string stageWhy(uint32_t bad)
{
    if (!(bad & 0x80000000u))
        return "a sample (or a stereo pair's mean) is not finite";
    return "frame " + std::to_string((bad & 0x7FFFFFFFu) >> 4) + ": " + flacErrText(bad & 15u);
}

// A FLAC file among the files of a call: its record and frame index; both null for a WAV file.  Its DcsWavInfo is flacAsWav's.
struct FlacSource
{
    const DcsFlacInfo *info;
    const std::vector<DcsFlacFrame> *frames;
};

// The FLAC files of a call's group on the device: frame bytes up, F1, F2, F3 into dMono (zeroed first where no frame writes).
// errOut[k] (one word per file of the group, 0xFFFFFFFF = none) is copied back on the stream; the caller synchronises.
DcsStatus flacStage(DcsCtx *ctx, CacheArena &held, hipStream_t st, const uint8_t *const *bytes, const FlacSource *flac, uint32_t n,
                    const std::vector<WavFile> &wf, float *dMono, std::vector<uint32_t> &errOut)
{
    std::vector<FlacFrameDev> fr;
    std::vector<uint64_t> blobOff(n, 0);
    uint64_t blobBytes = 0, nStage = 0;
    for (uint32_t k = 0 ; k < n ; ++k)
    {
        if (flac[k].info == nullptr)
            continue;
        const DcsFlacInfo &w = *flac[k].info;
        const std::vector<DcsFlacFrame> &ff = *flac[k].frames;
        blobOff[k] = blobBytes;
        const uint64_t span = ff.back().offset + ff.back().length - ff.front().offset;
        blobBytes += (span + 255) & ~uint64_t(255);
        for (uint32_t i = 0 ; i < ff.size() ; ++i)
        {
            FlacFrameDev d{};
            d.byteOff = blobOff[k] + (ff[i].offset - ff.front().offset);
            d.stageOff = nStage + ff[i].firstSample * static_cast<uint64_t>(w.channels);
            d.monoPos = wf[k].monoOff + ff[i].firstSample;
            d.length = ff[i].length;
            d.hdrLen = static_cast<uint32_t>(ff[i].headerLength);
            d.blockSize = ff[i].blockSize;
            d.file = k;
            d.frame = i < (1u << 27) ? i : (1u << 27) - 1;
            d.assign = ff[i].channelAssignment;
            d.bps = ff[i].bitsPerSample;
            d.channels = w.channels;
            d.sampleFormat = w.sampleFormat;
            fr.push_back(d);
        }
        nStage += w.nValues;
    }
    errOut.assign(n, 0xFFFFFFFFu);
    if (fr.size() >= (uint64_t(1) << 31))
    {
        dcsCtxSetError(ctx, "2^31 FLAC frames or more in one call");
        return DCS_ERR_INVALID_ARG;
    }
    const uint32_t nFrames = static_cast<uint32_t>(fr.size());
    uint8_t *dBlob;
    FlacFrameDev *dFrames;
    int32_t *dStage;
    FlacSub *dSubs;
    uint32_t *dErr;
    ENCCHK(held.alloc(&dBlob, blobBytes + 256));            // (a lane's last dword may end 3 bytes past its frame)
    ENCCHK(held.alloc(&dFrames, nFrames));
    ENCCHK(held.alloc(&dStage, nStage));
    ENCCHK(held.alloc(&dSubs, 2 * uint64_t(nFrames)));
    ENCCHK(held.alloc(&dErr, n));
    for (uint32_t k = 0 ; k < n ; ++k)
    {
        if (flac[k].info == nullptr)
            continue;
        const std::vector<DcsFlacFrame> &ff = *flac[k].frames;
        ENCCHK(hipMemcpyAsync(dBlob + blobOff[k], bytes[k] + ff.front().offset, ff.back().offset + ff.back().length - ff.front().offset,
                              hipMemcpyHostToDevice, st));
        // the samples no frame supplies stay zero, as in the reference's zero-filled vector
        ENCCHK(hipMemsetAsync(dMono + wf[k].monoOff, 0, sizeof(float) * wf[k].nMono, st));
    }
    ENCCHK(hipMemcpyAsync(dFrames, fr.data(), sizeof(FlacFrameDev) * nFrames, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemsetAsync(dErr, 0xFF, sizeof(uint32_t) * n, st));
    const uint32_t walkBlocks = (nFrames + 63) / 64, restoreBlocks = static_cast<uint32_t>((2 * uint64_t(nFrames) + 63) / 64);
    hipLaunchKernelGGL(flacWalkKernel, dim3(walkBlocks), dim3(64), 0, st, dBlob, dFrames, nFrames, dStage, dSubs, dErr);
    hipLaunchKernelGGL(flacRestoreKernel, dim3(restoreBlocks), dim3(64), 0, st, dFrames, nFrames, dStage, dSubs, dErr);
    hipLaunchKernelGGL(flacMixKernel, dim3(nFrames < (1u << 20) ? nFrames : (1u << 20)), dim3(256), 0, st, dFrames, nFrames, dStage, dMono);
    ENCCHK(hipGetLastError());
    ENCCHK(hipMemcpyAsync(errOut.data(), dErr, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, st));
    return DCS_OK;
}

// the reader's record of a FLAC file as the shared driver's DcsWavInfo: what the downmix, the length limits and the bound read
DcsWavInfo flacAsWav(const DcsFlacInfo &w)
{
    DcsWavInfo v{};
    v.formatCode = w.sampleFormat;
    v.sampleFormat = w.sampleFormat;
    v.bitDepth = w.bitDepth;
    v.channels = w.channels;
    v.rate = w.rate;
    v.nValues = w.nValues;
    return v;
}

}  // namespace

extern "C" DcsStatus dcs_flac_parse(const uint8_t *file, size_t len, DcsFlacInfo *info)
{
    if (info == nullptr || (file == nullptr && len != 0))
        return DCS_ERR_INVALID_ARG;
    return encGuard([&] {
        DcsFlacInfo w;
        const DcsStatus st = flacParse(file, file == nullptr ? 0 : len, &w, nullptr);
        w.status = st;
        *info = w;
        return st;
    });
}

extern "C" DcsStatus dcs_flac_index(const uint8_t *file, size_t len, DcsFlacFrame *frames, uint32_t cap, uint32_t *nFrames)
{
    if (nFrames == nullptr || (file == nullptr && len != 0))
        return DCS_ERR_INVALID_ARG;
    return encGuard([&]() -> DcsStatus {
        DcsFlacInfo w;
        std::vector<DcsFlacFrame> ff;
        const DcsStatus st = flacParse(file, file == nullptr ? 0 : len, &w, &ff);
        *nFrames = static_cast<uint32_t>(ff.size());
        if (st != DCS_OK)
            return st;
        if (frames == nullptr || cap < ff.size())
            return DCS_ERR_CAPACITY;
        memcpy(frames, ff.data(), sizeof(DcsFlacFrame) * ff.size());
        return DCS_OK;
    });
}
