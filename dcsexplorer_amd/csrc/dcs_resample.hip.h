// dcs_resample.hip.h -- the reference's input resampler on the GPU: libsamplerate's sinc converter, mono, at the fixed
// ratio 31250 / rate (DCSEncoder::OpenStream, DCSEncoder.cpp:165-185; src_sinc.c:280-424 sinc_mono_vari_process and
// calc_output_single; common.h:147-155 fmod_one), and EncodeFile's stereo downmix (DCSEncodeFile.cpp:81-102).  Included at
// the end of dcs_encode.hip after dcs_level.hip.h: it shares that translation unit's floating-point contract (no
// contraction, f64 and f32 rounded at every step, denormals kept) and hands its output to the encoder's driver where it
// lies.  The way from the converted signal to the encoder (the level stage, the gate, the hand-over) is stated once, in
// rsEncodeConverted, for the streams of this file and the files of dcs_encode_files.hip.h.
//
//   R1 stage    rsStageKernel     one thread per mono sample: (L + R) / 2.0f for stereo, a copy for mono; a non-finite value
//                                 flags its stream
//   R2 walk     rsWalkKernel      one lane per stream: the serial position chain (input_index += 1 / ratio, fmod_one), the
//                                 end rule and the 512-sample cap of the end-of-input flush; per output the integer input
//                                 position and start_filter_index, per stream the count
//   R3 convolve rsConvolveKernel  one thread per output: the left half, the right half, each summed in f64 in the reference's
//                                 order, scaled and rounded to f32; the stream's peak |y|
//
// Each output's value depends only on the whole input and the output's position.  How many outputs there are depends on the
// reference's calls as well: the end-of-input call runs once with a 512-float buffer (CloseStream, DCSEncoder.cpp:717-721),
// and the end rule is an f64 sum in the converter's buffer indices, so the walk replays the buffer's bookkeeping (rsWalk).
//
// The same converter runs the other way behind the decoder (the end of this file): int16 at 31 250 Hz to int16 at an output
// rate, ratio outRate / 31250.0, with R3's int16 instantiation and one walk-record table for the whole call.
#pragma once

namespace {

const int kRsFlushCap = 512;            // CloseStream's one end-of-input call: WriteStream's outbuf[512]
const uint32_t kRsMinRate = 4000, kRsMaxRate = 384000;

// what the walk needs of one stream, fixed before it runs (src_sinc.c:359-405)
struct RsStream
{
    uint64_t inOff;         // first mono sample in the staged buffer
    uint64_t nIn;           // mono samples
    uint64_t slotOff;       // first slot of its walk records ...
    uint64_t nSlots;        // ... and their number (rsSlots)
    uint64_t outOff;        // first output sample (set after the walk)
    double step;            // 1.0 / ratio
    double terminate;       // 1.0 / ratio + 1e-20
    double floatInc;        // increment * min(ratio, 1)
    int64_t half;           // half_filter_chan_len
    int32_t increment;      // lrint(floatInc * 4096)
    int32_t bLen;           // the converter's buffer length (sinc_set_converter)
    int32_t passThrough;    // rate 31 250 without DCS_RESAMPLE_AT_UNITY: the samples as they are
    int32_t hostWalk;       // walked by the host pool, not by a device lane (rsHostRoute; dcs_encode_files only)
};

__host__ __device__ inline double rsFmodOne(double x)
{
    const double res = x - rint(x);
    return res < 0.0 ? res + 1.0 : res;
}

// The position chain of sinc_mono_vari_process (src_sinc.c:342-413) over the reference encoder's calls: 16 samples per
// src_process, a 512-float output buffer, then one zero-length end-of-input call (WriteStream / CloseStream,
// DCSEncoder.cpp:650-721).  sink(k, pos, start_filter_index) per output, with pos the absolute input position; returns the
// count.  The converter's buffer is restated in its own indices (prepare_data's loads and moves, src_sinc.c:1156-1226):
// the end rule compares b_current + input_index + terminate with b_real_end there, and that f64 sum rounds by the size of
// b_current, so absolute positions would keep an extra sample at the end of some whole-second streams.  Indices are 32-bit
// (f64 <-> i32 are single instructions on the device; streams are shorter than 2^31 samples, rsCheck).
template <class Sink>
__host__ __device__ inline uint64_t rsWalk(const RsStream &s, Sink sink)
{
    if (s.passThrough)
    {
        for (uint64_t k = 0 ; k < s.nIn ; ++k)
            sink(k, static_cast<int64_t>(k), 0);
        return s.nIn;
    }
    const int32_t n = static_cast<int32_t>(s.nIn), half = static_cast<int32_t>(s.half), bLen = s.bLen;
    int32_t bCur = 0, bEnd = 0, bRealEnd = -1, fed = 0, pos = 0;
    double idx = 0.0;
    uint64_t k = 0;
    // (bEnd - bCur + bLen) % bLen and (bCur + adv) % bLen for operands in (-bLen, 2 bLen): a compare instead of a division
    auto inHand = [&]() { const int32_t d = bEnd - bCur; return d < 0 ? d + bLen : d >= bLen ? d - bLen : d; };
    auto advance = [&]() {
        const double rem = rsFmodOne(idx);
        const int32_t adv = static_cast<int32_t>(rint(idx - rem));
        bCur += adv;
        bCur = bCur >= bLen ? bCur - bLen : bCur;
        pos += adv;
        idx = rem;
    };
    while (bRealEnd < 0)
    {
        const int32_t inCount = n - fed < 16 ? n - fed : 16;
        const bool eof = inCount == 0;
        fed += inCount;
        int32_t inUsed = 0, outGen = 0;
        advance();                                          // the call's opening fmod_one (no move: idx is in [0, 1))
        while (outGen < kRsFlushCap)
        {
            if (inHand() <= half)
            {
                if (bRealEnd < 0)                           // prepare_data
                {
                    int32_t len;
                    if (bCur == 0)
                    {
                        len = bLen - 2 * half;
                        bCur = bEnd = half;
                    }
                    else if (bEnd + half + 1 < bLen)
                        len = bLen - bCur - half > 0 ? bLen - bCur - half : 0;
                    else
                    {
                        len = bEnd - bCur;
                        bCur = half;
                        bEnd = half + len;
                        len = bLen - bCur - half > 0 ? bLen - bCur - half : 0;
                    }
                    len = inCount - inUsed < len ? inCount - inUsed : len;
                    bEnd += len;
                    inUsed += len;
                    if (inUsed == inCount && bEnd - bCur < 2 * half && eof)
                    {
                        if (bLen - bEnd < half + 5)
                        {
                            len = bEnd - bCur;
                            bCur = half;
                            bEnd = half + len;
                        }
                        bRealEnd = bEnd;
                        len = bEnd + half + 5 > bLen ? bLen - bEnd : half + 5;
                        bEnd += len;
                    }
                }
                if (inHand() <= half)
                    break;
            }
            if (bRealEnd >= 0 && static_cast<double>(bCur) + idx + s.terminate > static_cast<double>(bRealEnd))
                break;
            sink(k, pos, static_cast<int32_t>(rint(idx * s.floatInc * 4096.0)));
            ++k;
            ++outGen;
            idx += s.step;
            advance();
        }
    }
    return k;
}

// walk records the stream may fill (none for a pass-through): the end rule keeps pos + 1 / ratio <= n, so k <= n * ratio;
// the margin covers the chain's rounding
uint64_t rsSlots(const RsStream &s)
{
    return s.passThrough ? 0 : static_cast<uint64_t>(static_cast<double>(s.nIn) / s.step) + 4;
}

bool rsFilterValid(const DcsResampleFilter *f)
{
    if (f == nullptr || f->coeffs == nullptr || f->increment < 1 || f->increment > (1 << 18) || f->nCoeffs < 3)
        return false;
    // sinc_set_converter's check (src_sinc.c:229-234), and what keeps int_to_fp (coeff_half_len) and the first tap's
    // coeff_count in range: a half length below 2^19 and at least one input sample wide
    const int32_t half = f->nCoeffs - 2;
    int32_t count = half, bits = 0;
    for (bits = 0 ; (int32_t(1) << bits) < count ; bits++)
        count |= int32_t(1) << bits;
    if (bits + 12 - 1 >= 32 || half >= (1 << 19) || half < f->increment)
        return false;
    for (int32_t i = 0 ; i < f->nCoeffs ; ++i)
        if (!isfinite(f->coeffs[i]))
            return false;
    return true;
}

// the fixed quantities of one stream of nIn mono samples converted at ratio = to / from, the two rates as the caller's
// contract divides them: 31250.0 / rate in front of the encoders, outRate / 31250.0 behind the decoder (one f64 division)
RsStream rsStreamOf(uint64_t nIn, double to, double from, bool passThrough, const DcsResampleFilter &f)
{
    RsStream s{};
    s.nIn = nIn;
    s.passThrough = passThrough;
    const double ratio = to / from;
    double count = (f.nCoeffs - 2 + 2.0) / f.increment;
    if (ratio < 1.0)
        count /= ratio;
    s.half = static_cast<int64_t>(lrint(count)) + 1;
    s.step = 1.0 / ratio;
    s.terminate = 1.0 / ratio + 1e-20;
    s.floatInc = f.increment * (ratio < 1.0 ? ratio : 1.0);
    s.increment = static_cast<int32_t>(lrint(s.floatInc * 4096.0));
    // src_sinc.c:215-217: lrint(2.5 * coeff_half_len / index_inc * SRC_MAX_RATIO), at least 4096, times the channels (1)
    const int32_t bLen = static_cast<int32_t>(lrint(2.5 * (f.nCoeffs - 2) / (f.increment * 1.0) * 256));
    s.bLen = bLen > 4096 ? bLen : 4096;
    return s;
}

// ... of mono samples nIn at `rate`, for the encoders
RsStream rsStreamOf(uint64_t nIn, uint32_t rate, const DcsResampleFilter &f, uint32_t flags)
{
    return rsStreamOf(nIn, 31250.0, static_cast<double>(rate), rate == 31250 && (flags & DCS_RESAMPLE_AT_UNITY) == 0, f);
}

uint64_t rsMonoLength(uint64_t nValues, int32_t channels) { return channels == 2 ? (nValues + 1) / 2 : nValues; }

// R1: blockIdx.y strides over the streams, the x dimension over a stream's mono samples
__global__ __launch_bounds__(256) void rsStageKernel(const float *__restrict__ in, const uint64_t *__restrict__ inOffsets,
                                                     const int32_t *__restrict__ channels, const RsStream *__restrict__ streams,
                                                     uint32_t nStreams, float *__restrict__ mono, uint32_t *__restrict__ bad)
{
    for (uint32_t si = blockIdx.y ; si < nStreams ; si += gridDim.y)
    {
        const RsStream &s = streams[si];
        const uint64_t base = inOffsets[si] - inOffsets[0], nValues = inOffsets[si + 1] - inOffsets[si];
        const bool stereo = channels[si] == 2;
        bool isBad = false;
        for (uint64_t j = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x ; j < s.nIn ; j += uint64_t(gridDim.x) * blockDim.x)
        {
            float x;
            if (stereo && 2 * j + 1 < nValues)
                x = (in[base + 2 * j] + in[base + 2 * j + 1]) / 2.0f;
            else
                x = in[base + (stereo ? 2 * j : j)];
            if (!isfinite(x))
                isBad = true;
            mono[s.inOff + j] = x;
        }
        if (isBad)
            atomicOr(&bad[si], 1u);
    }
}

// R2: one lane per stream; out-of-range lanes do nothing
__global__ __launch_bounds__(64) void rsWalkKernel(const RsStream *__restrict__ streams, uint32_t nStreams, int2 *__restrict__ slots,
                                                   uint64_t *__restrict__ counts)
{
    const uint32_t si = blockIdx.x * blockDim.x + threadIdx.x;
    if (si >= nStreams)
        return;
    const RsStream s = streams[si];
    if (s.hostWalk)
        return;
    if (s.passThrough)
    {
        counts[si] = s.nIn;
        return;
    }
    int2 *dst = slots + s.slotOff;
    // (rsSlots bounds the count; the guard keeps a stream that broke the bound inside its own records, and the host refuses it)
    const uint64_t count = rsWalk(s, [&](uint64_t k, int64_t pos, int32_t sfi) {
        if (k < s.nSlots)
            dst[k] = make_int2(static_cast<int32_t>(pos), sfi);
    });
    counts[si] = count;
}

// One output of calc_output_single (src_sinc.c:280-333): coefficient i + fraction * (coefficient i+1 - i), the difference a
// float subtraction, each half summed in f64 in the loop's order, then left + right.  x: the stream's mono samples, zero
// outside [0, n): floats, or a decoder's int16, which enter as src_short_to_float_array makes them (samplerate.c:486-495),
// (float)(s / 32768.0), exact for every int16 and so formed in registers.
__device__ inline float rsSample(const float *__restrict__ x, int64_t d) { return x[d]; }
__device__ inline float rsSample(const int16_t *__restrict__ x, int64_t d) { return static_cast<float>(x[d] / 32768.0); }

template <class T>
__device__ inline double rsOutput(const float *__restrict__ c, int32_t maxFilterIndex, int32_t increment, int32_t sfi,
                                  const T *__restrict__ x, int64_t n, int64_t pos)
{
    int32_t fi = sfi;
    int32_t cc = (maxFilterIndex - fi) / increment;
    fi = fi + cc * increment;
    int64_t d = pos - cc;
    double left = 0.0;
    do
    {
        const double fraction = static_cast<double>(fi & 4095) * (1.0 / 4096.0);
        const int32_t indx = fi >> 12;
        const float c0 = c[indx], c1 = c[indx + 1];
        const double icoeff = static_cast<double>(c0) + fraction * static_cast<double>(c1 - c0);
        const float v = (d >= 0 && d < n) ? rsSample(x, d) : 0.0f;
        left += icoeff * static_cast<double>(v);
        fi -= increment;
        ++d;
    } while (fi >= 0);

    fi = increment - sfi;
    cc = (maxFilterIndex - fi) / increment;
    fi = fi + cc * increment;
    d = pos + 1 + cc;
    double right = 0.0;
    do
    {
        const double fraction = static_cast<double>(fi & 4095) * (1.0 / 4096.0);
        const int32_t indx = fi >> 12;
        const float c0 = c[indx], c1 = c[indx + 1];
        const double icoeff = static_cast<double>(c0) + fraction * static_cast<double>(c1 - c0);
        const float v = (d >= 0 && d < n) ? rsSample(x, d) : 0.0f;
        right += icoeff * static_cast<double>(v);
        fi -= increment;
        --d;
    } while (fi > 0);
    return left + right;
}

// src_float_to_short_array as a build without CPU_CLIPS_* compiles it (samplerate.c:497-516): the float times 2^31 in f64,
// the two ends clamped (and counted), else lrint and an arithmetic shift by 16.  The shift floors: -0.3 of a step is -1,
// +0.7 of a step is 0.  That is libsamplerate's rounding and stays as it is.  (|v| < 2^31 where lrint runs: 32 bits hold it.)
__device__ inline int16_t rsToShort(float y, uint32_t &clipped)
{
    const double v = static_cast<double>(y) * 2147483648.0;
    if (v >= 2147483647.0)
    {
        ++clipped;
        return 32767;
    }
    if (v <= -2147483648.0)
    {
        ++clipped;
        return -32768;
    }
    return static_cast<int16_t>(static_cast<int32_t>(rint(v)) >> 16);
}

// R3: blockIdx.y strides over the streams, x over a stream's outputs.  LDS: the table is copied to LDS once per block
// (tables up to kRsLdsMaxCoeffs); otherwise it is read through the caches.  T = float: the encoders' side, floats in and
// out.  T = int16_t: the decoder's side (rsConvertPcm16), int16 read where the decoder left it, quantised by rsToShort and
// stored as int16; `clipped` then counts each stream's clamped outputs, and a pass-through copies the samples.
const int32_t kRsLdsMaxCoeffs = 16384;          // 64 KiB
template <bool LDS, class T>
__global__ __launch_bounds__(256) void rsConvolveKernel(const float *__restrict__ coeffs, int32_t nCoeffs, int32_t tableInc,
                                                        const RsStream *__restrict__ streams, uint32_t nStreams,
                                                        const uint64_t *__restrict__ counts, const int2 *__restrict__ slots,
                                                        const T *__restrict__ mono, T *__restrict__ out,
                                                        uint32_t *__restrict__ peak, unsigned long long *__restrict__ clipped)
{
    extern __shared__ float ldsCoeffs[];
    const float *c = coeffs;
    if constexpr (LDS)
    {
        for (int32_t i = threadIdx.x ; i < nCoeffs ; i += blockDim.x)
            ldsCoeffs[i] = coeffs[i];
        __syncthreads();
        c = ldsCoeffs;
    }
    const int32_t maxFilterIndex = (nCoeffs - 2) << 12;
    for (uint32_t si = blockIdx.y ; si < nStreams ; si += gridDim.y)
    {
        const RsStream &s = streams[si];
        const uint64_t count = counts[si];
        const T *x = mono + s.inOff;
        const int64_t n = static_cast<int64_t>(s.nIn);
        uint32_t top = 0, nClipped = 0;
        for (uint64_t k = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x ; k < count ; k += uint64_t(gridDim.x) * blockDim.x)
        {
            float y;
            if (s.passThrough)
                y = rsSample(x, static_cast<int64_t>(k));
            else
            {
                const int2 r = slots[s.slotOff + k];
                y = static_cast<float>((s.floatInc / tableInc) * rsOutput(c, maxFilterIndex, s.increment, r.y, x, n, r.x));
            }
            if constexpr (std::is_same<T, float>::value)
                out[s.outOff + k] = y;
            else
                out[s.outOff + k] = s.passThrough ? x[k] : rsToShort(y, nClipped);
            const uint32_t b = __float_as_uint(fabsf(y));
            top = b > top ? b : top;
        }
        if (top != 0)
            atomicMax(&peak[si], top);
        if (nClipped != 0)
            atomicAdd(&clipped[si], static_cast<unsigned long long>(nClipped));
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------- host side

namespace {

// The library's own table (dcs_resample_filter_default), in libsamplerate's layout: coeffs[i] = h(i / 128) for a
// Kaiser-windowed sinc h(t) = fc sinc(fc t) w(t / 48), fc = 0.91 of the input Nyquist, beta = 11, zero from t = 48 on.
// Computed once in f64 and rounded to f32.
const int32_t kRsDefaultIncrement = 128, kRsDefaultHalfWidth = 48;
const double kRsDefaultCutoff = 0.91, kRsDefaultBeta = 11.0;

double rsBesselI0(double x)
{
    double sum = 1.0, term = 1.0;
    for (int k = 1 ; k < 200 ; ++k)
    {
        const double q = x / (2.0 * k);
        term *= q * q;
        sum += term;
        if (term < sum * 1e-18)
            break;
    }
    return sum;
}

const std::vector<float> &rsDefaultTable()
{
    static const std::vector<float> table = [] {
        const int32_t half = kRsDefaultIncrement * kRsDefaultHalfWidth;
        std::vector<float> c(static_cast<size_t>(half) + 2, 0.0f);
        const double i0b = rsBesselI0(kRsDefaultBeta), pi = 3.14159265358979323846;
        for (int32_t i = 0 ; i < half ; ++i)
        {
            const double t = static_cast<double>(i) / kRsDefaultIncrement, x = kRsDefaultCutoff * t;
            const double sinc = i == 0 ? 1.0 : sin(pi * x) / (pi * x);
            const double r = t / kRsDefaultHalfWidth;
            const double w = rsBesselI0(kRsDefaultBeta * sqrt(1.0 - r * r)) / i0b;
            c[static_cast<size_t>(i)] = static_cast<float>(kRsDefaultCutoff * sinc * w);
        }
        return c;
    }();
    return table;
}

DcsResampleFilter rsDefaultFilter()
{
    const std::vector<float> &t = rsDefaultTable();
    return DcsResampleFilter{ t.data(), static_cast<int32_t>(t.size()), kRsDefaultIncrement };
}

// the checks every entry point shares: the filter (null = the default), flags, rate, channels; why = the message
DcsStatus rsCheck(uint32_t n, const uint64_t *sampleOffsets, const uint32_t *rates, const int32_t *channels,
                  const DcsResampleFilter *filter, uint32_t flags, DcsResampleFilter &f, std::string &why)
{
    if ((flags & ~DCS_RESAMPLE_AT_UNITY) != 0)
    {
        why = "unknown flags";
        return DCS_ERR_INVALID_ARG;
    }
    f = filter != nullptr ? *filter : rsDefaultFilter();
    if (!rsFilterValid(&f))
    {
        why = "filter: not a valid libsamplerate table (increment >= 1, increment <= nCoeffs - 2 < 2^19, finite coefficients)";
        return DCS_ERR_INVALID_ARG;
    }
    for (uint32_t i = 0 ; i < n ; ++i)
    {
        const std::string name = "stream " + std::to_string(i);
        if (rates[i] < kRsMinRate || rates[i] > kRsMaxRate)
        {
            why = name + ": rate " + std::to_string(rates[i]) + " Hz is outside 4 000 .. 384 000";
            return DCS_ERR_INVALID_ARG;
        }
        const int32_t ch = channels != nullptr ? channels[i] : 1;
        if (ch != 1 && ch != 2)
        {
            why = name + ": " + std::to_string(ch) + " channels (1 or 2)";
            return DCS_ERR_INVALID_ARG;
        }
        if (sampleOffsets[i + 1] <= sampleOffsets[i])
        {
            why = name + ": empty";
            return DCS_ERR_INVALID_ARG;
        }
        if (rsMonoLength(sampleOffsets[i + 1] - sampleOffsets[i], ch) >= (uint64_t(1) << 31))
        {
            why = name + ": 2^31 samples or more";
            return DCS_ERR_INVALID_ARG;
        }
    }
    return DCS_OK;
}

// what the converter produced: the outputs on the device (stream i = [offsets[i], offsets[i + 1]), offsets[n] in all) and
// the bits of each stream's largest |y|
struct RsConverted
{
    float *d = nullptr;
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> peak;
    uint64_t room = 0;                      // (in) floats the buffer is to hold behind the last stream, for the caller to fill
};

// how a message names stream i of a call: "<unit> label[i]" (label null: i)
std::string rsName(const char *unit, const uint32_t *label, uint32_t i)
{
    return std::string(unit) + " " + std::to_string(label != nullptr ? label[i] : i);
}

// Walk the files' position chains on the host rather than on device lanes where one or a few long ones dominate the list:
// a file whose walk makes more than kRsHostWalkMin outputs and at least 1 / kRsHostWalkShare of the list's.  A device lane
// takes about 263 ns an output, the host about 5 ns, so such a file is walked about 50 times faster
// on the host while the device walks the rest; a batch of comparable files stays on the device lanes, which walk in parallel.
const uint64_t kRsHostWalkMin = 65536;
const uint64_t kRsHostWalkShare = 4;
void rsHostRoute(std::vector<RsStream> &hs)
{
    uint64_t total = 0;
    for (const RsStream &s : hs)
        total += s.passThrough ? 0 : rsSlots(s);
    for (RsStream &s : hs)
    {
        const uint64_t est = s.passThrough ? 0 : rsSlots(s);
        s.hostWalk = est > kRsHostWalkMin && est * kRsHostWalkShare >= total;
    }
}

// After staging: the walk (device lanes, and the host pool for streams marked hostWalk, at the same time), the counts back,
// the convolution.  hs[i].inOff locates stream i in dMono; dBad (optional) holds R1's flags.  Messages name stream i as
// "<unit> label[i]" (rsName).  On DCS_OK `c` is filled; the buffers belong to `held`.
DcsStatus rsWalkConvolve(DcsCtx *ctx, std::vector<RsStream> &hs, const float *dMono, const uint32_t *dBad, const DcsResampleFilter &f,
                         const uint32_t *label, const char *unit, CacheArena &held, RsConverted &c)
{
    const uint32_t n = static_cast<uint32_t>(hs.size());
    std::vector<uint64_t> &outOffsets = c.offsets;
    outOffsets.assign(static_cast<size_t>(n) + 1, 0);
    std::vector<uint64_t> counts(n);
    std::vector<uint32_t> bad(n);
    uint64_t nSlots = 0;
    std::vector<uint32_t> onHost;
    for (uint32_t i = 0 ; i < n ; ++i)
    {
        hs[i].slotOff = nSlots;
        hs[i].nSlots = rsSlots(hs[i]);
        nSlots += hs[i].nSlots;
        if (hs[i].hostWalk)
            onHost.push_back(i);
    }
    auto name = [&](uint32_t i) { return rsName(unit, label, i); };
    const hipStream_t st = dcsCtxStream(ctx);
    float *dCoeffs, *dRes;
    uint64_t *dCounts;
    RsStream *dStr;
    uint32_t *dPeak;
    int2 *dSlots;
    ENCCHK(held.alloc(&dCoeffs, f.nCoeffs));
    ENCCHK(held.alloc(&dCounts, n));
    ENCCHK(held.alloc(&dStr, n));
    ENCCHK(held.alloc(&dPeak, n));
    ENCCHK(held.alloc(&dSlots, nSlots ? nSlots : 1));
    ENCCHK(hipMemcpyAsync(dCoeffs, f.coeffs, sizeof(float) * f.nCoeffs, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(dStr, hs.data(), sizeof(RsStream) * n, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemsetAsync(dPeak, 0, sizeof(uint32_t) * n, st));
    hipLaunchKernelGGL(rsWalkKernel, dim3((n + 63) / 64), dim3(64), 0, st, dStr, n, dSlots, dCounts);
    ENCCHK(hipGetLastError());
    // the host pool walks its streams while the lanes walk theirs (dcs_host_threads, at most one thread a stream)
    std::vector<std::vector<int2>> hostRec(onHost.size());
    if (!onHost.empty())
    {
        std::atomic<size_t> next{0};
        auto worker = [&]() {
            for (size_t j = next++ ; j < onHost.size() ; j = next++)
            {
                const RsStream &s = hs[onHost[j]];
                std::vector<int2> &rec = hostRec[j];
                rec.reserve(s.nSlots);
                counts[onHost[j]] = rsWalk(s, [&](uint64_t k, int64_t pos, int32_t sfi) {
                    if (k < s.nSlots)
                        rec.push_back(make_int2(static_cast<int32_t>(pos), sfi));
                });
            }
        };
        int nThreads = dcs_host_threads();
        nThreads = nThreads < 1 ? 1 : nThreads > static_cast<int>(onHost.size()) ? static_cast<int>(onHost.size()) : nThreads;
        std::vector<std::thread> pool;
        for (int t = 1 ; t < nThreads ; ++t)
            pool.emplace_back(worker);
        worker();
        for (std::thread &t : pool)
            t.join();
    }
    std::vector<uint64_t> devCounts(n);
    ENCCHK(hipMemcpyAsync(devCounts.data(), dCounts, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, st));
    if (dBad != nullptr)
        ENCCHK(hipMemcpyAsync(bad.data(), dBad, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, st));
    ENCCHK(hipStreamSynchronize(st));
    for (uint32_t i = 0 ; i < n ; ++i)
        if (!hs[i].hostWalk)
            counts[i] = devCounts[i];
    for (uint32_t i = 0 ; i < n ; ++i)
        if (bad[i])
        {
            dcsCtxSetError(ctx, (name(i) + ": an input sample (or a stereo pair's mean) is not finite").c_str());
            return DCS_ERR_BAD_STREAM;
        }
    for (uint32_t i = 0 ; i < n ; ++i)
        if (!hs[i].passThrough && counts[i] > hs[i].nSlots)
        {
            // a defect of this library, not of the input: the walk made more outputs than rsSlots allows (nothing is truncated)
            dcsCtxSetError(ctx, (name(i) + ": internal error: the resampler's walk made " + std::to_string(counts[i])
                                 + " outputs, more than its bound " + std::to_string(hs[i].nSlots)).c_str());
            return DCS_ERR_HIP;
        }
    if (!onHost.empty())
    {
        for (size_t j = 0 ; j < onHost.size() ; ++j)
            if (!hostRec[j].empty())
                ENCCHK(hipMemcpyAsync(dSlots + hs[onHost[j]].slotOff, hostRec[j].data(), sizeof(int2) * hostRec[j].size(),
                                      hipMemcpyHostToDevice, st));
        ENCCHK(hipMemcpyAsync(dCounts, counts.data(), sizeof(uint64_t) * n, hipMemcpyHostToDevice, st));
    }
    uint64_t maxCount = 0;
    for (uint32_t i = 0 ; i < n ; ++i)
    {
        hs[i].outOff = outOffsets[i];
        outOffsets[i + 1] = outOffsets[i] + counts[i];
        maxCount = counts[i] > maxCount ? counts[i] : maxCount;
    }
    ENCCHK(held.alloc(&dRes, outOffsets[n] + c.room ? outOffsets[n] + c.room : 1));
    ENCCHK(hipMemcpyAsync(dStr, hs.data(), sizeof(RsStream) * n, hipMemcpyHostToDevice, st));
    // about 4 096 blocks in all: each block of the LDS variant copies the table once and then strides over its outputs
    const dim3 grid = streamGrid(n, maxCount, 4096, 0);
    if (f.nCoeffs <= kRsLdsMaxCoeffs)
        hipLaunchKernelGGL((rsConvolveKernel<true, float>), grid, dim3(256), sizeof(float) * f.nCoeffs, st, dCoeffs, f.nCoeffs,
                           f.increment, dStr, n, dCounts, dSlots, dMono, dRes, dPeak, static_cast<unsigned long long *>(nullptr));
    else
        hipLaunchKernelGGL((rsConvolveKernel<false, float>), grid, dim3(256), 0, st, dCoeffs, f.nCoeffs, f.increment, dStr, n,
                           dCounts, dSlots, dMono, dRes, dPeak, static_cast<unsigned long long *>(nullptr));
    ENCCHK(hipGetLastError());
    c.peak.assign(n, 0);
    ENCCHK(hipMemcpyAsync(c.peak.data(), dPeak, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, st));
    ENCCHK(hipStreamSynchronize(st));
    c.d = dRes;
    return DCS_OK;
}

// The converter on the device for float input: stage (R1), then rsWalkConvolve, every stream on the device lanes.
DcsStatus resampleOnDevice(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t n, const uint32_t *rates,
                           const int32_t *channels, const DcsResampleFilter &f, uint32_t flags, CacheArena &held, RsConverted &c)
{
    std::vector<RsStream> hs(n);
    std::vector<int32_t> ch(n);
    uint64_t nMono = 0, maxMono = 0;
    for (uint32_t i = 0 ; i < n ; ++i)
    {
        ch[i] = channels != nullptr ? channels[i] : 1;
        const uint64_t m = rsMonoLength(sampleOffsets[i + 1] - sampleOffsets[i], ch[i]);
        hs[i] = rsStreamOf(m, rates[i], f, flags);
        hs[i].inOff = nMono;
        nMono += m;
        maxMono = m > maxMono ? m : maxMono;
    }
    const uint64_t nValues = sampleOffsets[n] - sampleOffsets[0];
    const hipStream_t st = dcsCtxStream(ctx);
    float *dIn, *dMono;
    uint64_t *dInOff;
    int32_t *dCh;
    RsStream *dStr;
    uint32_t *dBad;
    ENCCHK(hipSetDevice(dcsCtxDevice(ctx)));
    ENCCHK(held.alloc(&dIn, nValues));
    ENCCHK(held.alloc(&dMono, nMono));
    ENCCHK(held.alloc(&dInOff, size_t(n) + 1));
    ENCCHK(held.alloc(&dCh, n));
    ENCCHK(held.alloc(&dStr, n));
    ENCCHK(held.alloc(&dBad, n));
    ENCCHK(hipMemcpyAsync(dIn, pcm + sampleOffsets[0], sizeof(float) * nValues, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(dInOff, sampleOffsets, sizeof(uint64_t) * (n + 1), hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(dCh, ch.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(dStr, hs.data(), sizeof(RsStream) * n, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemsetAsync(dBad, 0, sizeof(uint32_t) * n, st));
    hipLaunchKernelGGL(rsStageKernel, streamGrid(n, maxMono, 0, 1024), dim3(256), 0, st, dIn, dInOff, dCh, dStr, n, dMono, dBad);
    ENCCHK(hipGetLastError());
    return rsWalkConvolve(ctx, hs, dMono, dBad, f, nullptr, "stream", held, c);
}

// The gate in front of the encoder: per stream and in stream order, first the length the encoder can take, then the range
// of what it would read (the levelled peak where the call has a level).  bound[i]: the largest |x| stream i may hold (null:
// 1); rangeFormat: the caller's message for the range, a format of the stream's name (%s), the peak and the bound (%.9g).
DcsStatus rsGate(DcsCtx *ctx, const RsConverted &c, const LevelStage &lv, const uint32_t *label, const char *unit, const float *bound,
                 const char *rangeFormat)
{
    for (uint32_t i = 0 ; i + 1 < c.offsets.size() ; ++i)
    {
        const std::string name = rsName(unit, label, i);
        const uint64_t m = c.offsets[i + 1] - c.offsets[i];
        if (m == 0 || (m + 239) / 240 > 65535)
        {
            dcsCtxSetError(ctx, (name + (m == 0 ? ": resamples to no samples" : ": resamples to more than 65 535 frames")).c_str());
            return DCS_ERR_INVALID_ARG;
        }
        const float top = lv.top(i, c.peak), b = bound != nullptr ? bound[i] : 1.0f;
        if (!(top <= b))                    // |y| beyond the bound, or not a number
        {
            char text[192];
            snprintf(text, sizeof(text), rangeFormat, name.c_str(), static_cast<double>(top), static_cast<double>(b));
            dcsCtxSetError(ctx, text);
            return DCS_ERR_BAD_STREAM;
        }
    }
    return DCS_OK;
}

// From the converted signal on the device to the encoder, for streams (dcs_encode_streams_at_level) and files
// (encodeFiles): plan the level from the peaks, gate, scale (queued, no wait), encode where the floats lie, collect the
// clamp's counts, publish the records to levelOut.  Nothing is published where the gate refuses.  publishEarly: the
// records go to levelOut as soon as the gate has passed, so they stand where the encoder then refuses (its
// DCS_ERR_CAPACITY); without it they are written only once everything has succeeded.  `encode` (or null: encodeStreams
// with params, os93 and `to`) takes the EncInput in the encoder's place: the budget calls' way to a searched EncJobs.
using RsEncode = std::function<DcsStatus(EncInput &in)>;
DcsStatus rsEncodeConverted(DcsCtx *ctx, CacheArena &held, const RsConverted &c, LevelStage &lv, const uint32_t *label, const char *unit,
                            const float *bound, const char *rangeFormat, bool publishEarly, DcsLevelInfo *levelOut,
                            const DcsEncodeParams *params, bool os93, const EncOutput &to, const RsEncode *encode = nullptr)
{
    lv.plan(c.peak);
    ENCTRY(rsGate(ctx, c, lv, label, unit, bound, rangeFormat));
    if (publishEarly)
        lv.publish(levelOut);
    ENCTRY(lv.scale(held, c.d, c.offsets.data()));
    EncInput in;
    in.sampleOffsets = c.offsets.data();
    in.nStreams = static_cast<uint32_t>(c.peak.size());
    in.devFloat = c.d;
    in.label = label;
    in.bound = bound;
    ENCTRY(encode != nullptr ? (*encode)(in) : encodeStreams(ctx, in, params, os93, to));
    return lv.finish(levelOut);
}

}  // namespace

extern "C" DcsStatus dcs_resample_filter_default(DcsResampleFilter *filter)
{
    if (filter == nullptr)
        return DCS_ERR_INVALID_ARG;
    return encGuard([&] {
        *filter = rsDefaultFilter();
        return DCS_OK;
    });
}

extern "C" DcsStatus dcs_resample_count(uint64_t nValues, uint32_t rate, int32_t channels, const DcsResampleFilter *filter,
                                        uint32_t flags, uint64_t *countOut)
{
    if (countOut == nullptr)
        return DCS_ERR_INVALID_ARG;
    return encGuard([&] {
        const uint64_t offs[2] = { 0, nValues };
        DcsResampleFilter f;
        std::string why;
        const DcsStatus st = rsCheck(1, offs, &rate, &channels, filter, flags, f, why);
        if (st == DCS_OK)
            *countOut = rsWalk(rsStreamOf(rsMonoLength(nValues, channels), rate, f, flags), [](uint64_t, int64_t, int32_t) {});
        return st;
    });
}

extern "C" DcsStatus dcs_resample_streams(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams,
                                          const uint32_t *rates, const int32_t *channels, const DcsResampleFilter *filter,
                                          uint32_t flags, float *out, size_t outCap, uint64_t *outOffsets)
{
    return dcs_resample_streams_level(ctx, pcm, sampleOffsets, nStreams, rates, channels, filter, flags, out, outCap, outOffsets,
                                      nullptr, 0, nullptr);
}

extern "C" DcsStatus dcs_resample_streams_level(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams,
                                                const uint32_t *rates, const int32_t *channels, const DcsResampleFilter *filter,
                                                uint32_t flags, float *out, size_t outCap, uint64_t *outOffsets,
                                                const DcsLevel *levels, uint32_t nLevels, DcsLevelInfo *levelInfo)
{
    return encGuard([&]() -> DcsStatus {
        if (ctx == nullptr || sampleOffsets == nullptr || outOffsets == nullptr || (nStreams != 0 && (pcm == nullptr || rates == nullptr)))
            return DCS_ERR_INVALID_ARG;
        DcsResampleFilter f;
        std::string why;
        const DcsStatus status = rsCheck(nStreams, sampleOffsets, rates, channels, filter, flags, f, why);
        if (status != DCS_OK)
        {
            dcsCtxSetError(ctx, why.c_str());
            return status;
        }
        LevelStage lv{ ctx, levels, nLevels };
        ENCTRY(lv.check(nStreams, "stream"));
        outOffsets[0] = 0;
        if (nStreams == 0)
            return DCS_OK;
        CacheArena held(ctx);
        RsConverted c;
        ENCTRY(resampleOnDevice(ctx, pcm, sampleOffsets, nStreams, rates, channels, f, flags, held, c));
        memcpy(outOffsets, c.offsets.data(), sizeof(uint64_t) * c.offsets.size());
        // (the offsets stand, and with publishEarly the records, where DCS_ERR_CAPACITY then says the buffer is too small)
        return lvToHost(lv, held, c.d, outOffsets, c.peak, "the resampled signal is not finite", true, out, outCap, levelInfo);
    });
}

extern "C" DcsStatus dcs_encode_streams_at(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams,
                                           const uint32_t *rates, const int32_t *channels, const DcsResampleFilter *filter,
                                           uint32_t flags, const DcsEncodeParams *params, uint8_t *out, size_t outCap,
                                           uint64_t *outOffsets, DcsEncodeInfo *info)
{
    return dcs_encode_streams_at_level(ctx, pcm, sampleOffsets, nStreams, rates, channels, filter, flags, params, out, outCap, outOffsets,
                                       info, nullptr, 0, nullptr);
}

namespace {

// dcs_encode_streams_at_level (budget null) and dcs_encode_streams_at_budget: the argument checks, the converter, and
// rsEncodeConverted with the reference-equal encoder or the searched one behind it
DcsStatus encodeStreamsAt(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams,
                          const uint32_t *rates, const int32_t *channels, const DcsResampleFilter *filter,
                          uint32_t flags, const DcsEncodeParams *params, const DcsBudget *budget, uint8_t *out, size_t outCap,
                          uint64_t *outOffsets, DcsEncodeInfo *info, DcsEncodeRdInfo *infoRd,
                          const DcsLevel *levels, uint32_t nLevels, DcsLevelInfo *levelInfo)
{
    if (ctx == nullptr || sampleOffsets == nullptr || outOffsets == nullptr || (nStreams != 0 && (pcm == nullptr || rates == nullptr)))
        return DCS_ERR_INVALID_ARG;
    const bool os93 = budgetOs93(params);
    if (budget != nullptr)
    {
        const auto say = [&](const char *why) { dcsCtxSetError(ctx, why); };
        if (!searchedParams("dcs_encode_streams_at_budget", params, os93, say) || !budgetValid("dcs_encode_streams_at_budget", budget, say))
            return DCS_ERR_INVALID_ARG;
    }
    else if (!paramsValid(params, os93))
    {
        if (const char *type1 = whyOs93aType1(params, os93))
            dcsCtxSetError(ctx, type1);
        return DCS_ERR_INVALID_ARG;
    }
    DcsResampleFilter f;
    std::string why;
    const DcsStatus status = rsCheck(nStreams, sampleOffsets, rates, channels, filter, flags, f, why);
    if (status != DCS_OK)
    {
        dcsCtxSetError(ctx, why.c_str());
        return status;
    }
    LevelStage lv{ ctx, levels, nLevels };
    ENCTRY(lv.check(nStreams, "stream"));
    if (nStreams == 0)
    {
        outOffsets[0] = 0;
        return DCS_OK;
    }
    CacheArena held(ctx);
    RsConverted c;
    ENCTRY(resampleOnDevice(ctx, pcm, sampleOffsets, nStreams, rates, channels, f, flags, held, c));
    // (the budget call: every stream a searched job, its record the caller's own)
    const RsEncode searched = [&](EncInput &in) -> DcsStatus {
        BudgetUnits u;
        for (uint32_t i = 0 ; i < nStreams ; ++i)
            u.search(i);
        std::vector<DcsEncodeInfo> enc;
        const DcsStatus st = encodeBudgeted(ctx, in, u, params, os93, *budget, out, outCap, outOffsets, enc, infoRd);
        if (info != nullptr && (st == DCS_OK || st == DCS_ERR_CAPACITY))
            memcpy(info, enc.data(), sizeof(DcsEncodeInfo) * nStreams);
        return st;
    };
    return rsEncodeConverted(ctx, held, c, lv, nullptr, "stream", nullptr,
                             "%s: the resampled signal peaks at |x| = %.9g, outside [-1, 1] (attenuate the input)", true, levelInfo,
                             params, os93, EncOutput{ out, outCap, outOffsets, info, nullptr }, budget != nullptr ? &searched : nullptr);
}

}  // namespace

extern "C" DcsStatus dcs_encode_streams_at_level(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams,
                                                 const uint32_t *rates, const int32_t *channels, const DcsResampleFilter *filter,
                                                 uint32_t flags, const DcsEncodeParams *params, uint8_t *out, size_t outCap,
                                                 uint64_t *outOffsets, DcsEncodeInfo *info,
                                                 const DcsLevel *levels, uint32_t nLevels, DcsLevelInfo *levelInfo)
{
    return encGuard([&]() -> DcsStatus {
        return encodeStreamsAt(ctx, pcm, sampleOffsets, nStreams, rates, channels, filter, flags, params, nullptr, out, outCap, outOffsets,
                               info, nullptr, levels, nLevels, levelInfo);
    });
}

extern "C" DcsStatus dcs_encode_streams_at_budget(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams,
                                                  const uint32_t *rates, const int32_t *channels, const DcsResampleFilter *filter,
                                                  uint32_t flags, const DcsEncodeParams *params, const DcsBudget *budget, uint8_t *out,
                                                  size_t outCap, uint64_t *outOffsets, DcsEncodeInfo *info, DcsEncodeRdInfo *infoRd,
                                                  const DcsLevel *levels, uint32_t nLevels, DcsLevelInfo *levelInfo)
{
    return encGuard([&]() -> DcsStatus {
        if (budget == nullptr)
            return DCS_ERR_INVALID_ARG;
        return encodeStreamsAt(ctx, pcm, sampleOffsets, nStreams, rates, channels, filter, flags, params, budget, out, outCap, outOffsets,
                               info, infoRd, levels, nLevels, levelInfo);
    });
}

// ------------------------------------------------------------------ the other direction: 31 250 Hz int16 to an output rate
//
// dcs_resample_out_streams and the decode calls of dcs_decode_rate.hip.h: the same converter at ratio outRate / 31250.0,
// int16 in (rsSample) and int16 out (rsToShort), one rate per call.  Output k's walk record (pos, start_filter_index)
// depends on k and the ratio alone -- the chain is idx += step; advance(), the call-opening advance() does nothing to an
// idx already in [0, 1), and a stream's length decides only where the end rule and the flush cap stop it -- so a call
// keeps ONE record table, the longest stream's walk, of which every stream reads a prefix (slotOff 0), and walks each
// distinct length once more without a sink for its count.

namespace {

const uint32_t kRsOutMinRate = 4000, kRsOutMaxRate = 65535;     // the upper end: what a FLAC frame header can say

// the checks the output-rate entry points share, before any device work (sampleOffsets null: the rate, table and flags alone)
DcsStatus rsOutCheck(uint32_t n, const uint64_t *sampleOffsets, uint32_t outRate, const DcsResampleFilter *filter, uint32_t flags,
                     DcsResampleFilter &f, std::string &why)
{
    if ((flags & ~DCS_RESAMPLE_AT_UNITY) != 0)
    {
        why = "unknown flags";
        return DCS_ERR_INVALID_ARG;
    }
    if (outRate < kRsOutMinRate || outRate > kRsOutMaxRate)
    {
        why = "output rate " + std::to_string(outRate) + " Hz is outside 4 000 .. 65 535";
        return DCS_ERR_INVALID_ARG;
    }
    f = filter != nullptr ? *filter : rsDefaultFilter();
    if (!rsFilterValid(&f))
    {
        why = "filter: not a valid libsamplerate table (increment >= 1, increment <= nCoeffs - 2 < 2^19, finite coefficients)";
        return DCS_ERR_INVALID_ARG;
    }
    for (uint32_t i = 0 ; sampleOffsets != nullptr && i < n ; ++i)
    {
        if (sampleOffsets[i + 1] <= sampleOffsets[i])
        {
            why = "stream " + std::to_string(i) + ": empty";
            return DCS_ERR_INVALID_ARG;
        }
        if (sampleOffsets[i + 1] - sampleOffsets[i] >= (uint64_t(1) << 31))
        {
            why = "stream " + std::to_string(i) + ": 2^31 samples or more";
            return DCS_ERR_INVALID_ARG;
        }
    }
    return DCS_OK;
}

RsStream rsOutStreamOf(uint64_t nIn, uint32_t outRate, const DcsResampleFilter &f, uint32_t flags)
{
    return rsStreamOf(nIn, static_cast<double>(outRate), 31250.0, outRate == 31250 && (flags & DCS_RESAMPLE_AT_UNITY) == 0, f);
}

// what the converter produced on the device: int16 samples, stream i = [offsets[i], offsets[i + 1])
struct RsConverted16
{
    int16_t *d = nullptr;
    std::vector<uint64_t> offsets;
    std::vector<DcsRateInfo> info;
};

// The walks of one call whose streams hs all convert at one ratio: the shared record table (*dSlots, the longest stream's
// walk) and counts[i].  The table is walked where rsHostRoute puts a stream of its length that is a list of its own: on
// one device lane, or above kRsHostWalkMin outputs on the host.  Every other distinct length is walked without a sink on
// the host pool, at the same time: device lanes, one a length, took 42.5 ms for 255 lengths of up to 511 frames, and the
// call 56.6 ms where it takes 22.8 ms with the pool (profiles/decode_rate_bench.txt).  One wait.
DcsStatus rsOutWalks(DcsCtx *ctx, const std::vector<RsStream> &hs, CacheArena &held, int2 **dSlots, std::vector<uint64_t> &counts)
{
    const hipStream_t st = dcsCtxStream(ctx);
    const uint32_t n = static_cast<uint32_t>(hs.size());
    // the distinct lengths, falling; the first one's walk is the table
    std::vector<uint64_t> lengths(n);
    for (uint32_t i = 0 ; i < n ; ++i)
        lengths[i] = hs[i].nIn;
    std::sort(lengths.begin(), lengths.end(), std::greater<uint64_t>());
    lengths.erase(std::unique(lengths.begin(), lengths.end()), lengths.end());
    const uint32_t nLen = static_cast<uint32_t>(lengths.size());
    std::vector<RsStream> table(1, hs[0]);
    table[0].nIn = lengths[0];
    table[0].inOff = table[0].slotOff = 0;
    table[0].nSlots = rsSlots(table[0]);
    rsHostRoute(table);
    const RsStream &tb = table[0];
    ENCCHK(held.alloc(dSlots, tb.nSlots));
    std::vector<uint64_t> lenCounts(nLen, 0);
    if (!tb.hostWalk)
    {
        RsStream *dWalk = nullptr;
        uint64_t *dCount = nullptr;
        ENCCHK(held.alloc(&dWalk, 1));
        ENCCHK(held.alloc(&dCount, 1));
        ENCCHK(hipMemcpyAsync(dWalk, &tb, sizeof(RsStream), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(rsWalkKernel, dim3(1), dim3(64), 0, st, dWalk, 1u, *dSlots, dCount);
        ENCCHK(hipGetLastError());
        ENCCHK(hipMemcpyAsync(&lenCounts[0], dCount, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    }
    // the host pool meanwhile (dcs_host_threads, at most one thread a walk), the longest first
    std::vector<int2> rec;                                          // the table's records, where the host walks it
    const uint32_t firstOnHost = tb.hostWalk ? 0 : 1;
    if (firstOnHost < nLen)
    {
        std::atomic<uint32_t> next{firstOnHost};
        auto worker = [&]() {
            for (uint32_t j = next++ ; j < nLen ; j = next++)
            {
                if (j == 0)
                {
                    rec.reserve(tb.nSlots);
                    lenCounts[0] = rsWalk(tb, [&](uint64_t k, int64_t pos, int32_t sfi) {
                        if (k < tb.nSlots)
                            rec.push_back(make_int2(static_cast<int32_t>(pos), sfi));
                    });
                    continue;
                }
                RsStream s = tb;
                s.nIn = lengths[j];
                lenCounts[j] = rsWalk(s, [](uint64_t, int64_t, int32_t) {});
            }
        };
        int nThreads = dcs_host_threads();
        const int nWalks = static_cast<int>(nLen - firstOnHost);
        nThreads = nThreads < 1 ? 1 : nThreads > nWalks ? nWalks : nThreads;
        std::vector<std::thread> pool;
        for (int t = 1 ; t < nThreads ; ++t)
            pool.emplace_back(worker);
        worker();
        for (std::thread &t : pool)
            t.join();
    }
    if (!rec.empty())
        ENCCHK(hipMemcpyAsync(*dSlots, rec.data(), sizeof(int2) * rec.size(), hipMemcpyHostToDevice, st));
    ENCCHK(hipStreamSynchronize(st));
    for (uint32_t j = 0 ; j < nLen ; ++j)
        if (lenCounts[j] > tb.nSlots || lenCounts[j] > lenCounts[0])
        {
            // a defect of this library, not of the input: a walk left the table every stream reads a prefix of
            dcsCtxSetError(ctx, ("internal error: the resampler's walk of " + std::to_string(lengths[j]) + " samples made "
                                 + std::to_string(lenCounts[j]) + " outputs; the table holds " + std::to_string(lenCounts[0])
                                 + " and may hold " + std::to_string(tb.nSlots)).c_str());
            return DCS_ERR_HIP;
        }
    for (uint32_t i = 0 ; i < n ; ++i)
        counts[i] = lenCounts[std::lower_bound(lengths.begin(), lengths.end(), hs[i].nIn, std::greater<uint64_t>()) - lengths.begin()];
    return DCS_OK;
}

// The converter on int16 PCM resident on the device (stream i = dPcm[sampleOffsets[i] .. sampleOffsets[i + 1]), offsets on
// the host), queued on the context's stream behind whatever produces dPcm there.  It waits twice: for the counts
// (rsOutWalks; not for a pass-through), then for the peaks and clip counts.  On DCS_OK `c` is filled; the buffers belong
// to `held`.
DcsStatus rsConvertPcm16(DcsCtx *ctx, const int16_t *dPcm, const uint64_t *sampleOffsets, uint32_t n, uint32_t outRate,
                         const DcsResampleFilter &f, uint32_t flags, CacheArena &held, RsConverted16 &c)
{
    const hipStream_t st = dcsCtxStream(ctx);
    std::vector<RsStream> hs(n);
    std::vector<uint64_t> counts(n);
    for (uint32_t i = 0 ; i < n ; ++i)
    {
        hs[i] = rsOutStreamOf(sampleOffsets[i + 1] - sampleOffsets[i], outRate, f, flags);
        hs[i].inOff = sampleOffsets[i];
        counts[i] = hs[i].nIn;
    }
    ENCCHK(hipSetDevice(dcsCtxDevice(ctx)));
    int2 *dSlots = nullptr;
    if (!hs[0].passThrough)
        ENCTRY(rsOutWalks(ctx, hs, held, &dSlots, counts));
    c.offsets.assign(static_cast<size_t>(n) + 1, 0);
    uint64_t maxCount = 0;
    for (uint32_t i = 0 ; i < n ; ++i)
    {
        hs[i].outOff = c.offsets[i];
        c.offsets[i + 1] = c.offsets[i] + counts[i];
        maxCount = counts[i] > maxCount ? counts[i] : maxCount;
    }
    float *dCoeffs;
    uint64_t *dCounts;
    RsStream *dStr;
    uint32_t *dPeak;
    unsigned long long *dClipped;
    int16_t *dOut;
    ENCCHK(held.alloc(&dCoeffs, f.nCoeffs));
    ENCCHK(held.alloc(&dCounts, n));
    ENCCHK(held.alloc(&dStr, n));
    ENCCHK(held.alloc(&dPeak, n));
    ENCCHK(held.alloc(&dClipped, n));
    ENCCHK(held.alloc(&dOut, c.offsets[n] ? c.offsets[n] : 1));
    ENCCHK(hipMemcpyAsync(dCoeffs, f.coeffs, sizeof(float) * f.nCoeffs, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(dCounts, counts.data(), sizeof(uint64_t) * n, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(dStr, hs.data(), sizeof(RsStream) * n, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemsetAsync(dPeak, 0, sizeof(uint32_t) * n, st));
    ENCCHK(hipMemsetAsync(dClipped, 0, sizeof(unsigned long long) * n, st));
    // about 4 096 blocks in all, as the float side
    const dim3 grid = streamGrid(n, maxCount, 4096, 0);
    if (f.nCoeffs <= kRsLdsMaxCoeffs)
        hipLaunchKernelGGL((rsConvolveKernel<true, int16_t>), grid, dim3(256), sizeof(float) * f.nCoeffs, st, dCoeffs, f.nCoeffs,
                           f.increment, dStr, n, dCounts, dSlots, dPcm, dOut, dPeak, dClipped);
    else
        hipLaunchKernelGGL((rsConvolveKernel<false, int16_t>), grid, dim3(256), 0, st, dCoeffs, f.nCoeffs, f.increment, dStr, n,
                           dCounts, dSlots, dPcm, dOut, dPeak, dClipped);
    ENCCHK(hipGetLastError());
    std::vector<uint32_t> peak(n);
    std::vector<unsigned long long> clipped(n);
    ENCCHK(hipMemcpyAsync(peak.data(), dPeak, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, st));
    ENCCHK(hipMemcpyAsync(clipped.data(), dClipped, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, st));
    ENCCHK(hipStreamSynchronize(st));
    c.info.assign(n, DcsRateInfo{});
    for (uint32_t i = 0 ; i < n ; ++i)
    {
        c.info[i].nIn = hs[i].nIn;
        c.info[i].nOut = counts[i];
        c.info[i].nClipped = clipped[i];
        memcpy(&c.info[i].peak, &peak[i], sizeof(float));
    }
    c.d = dOut;
    return DCS_OK;
}

}  // namespace

// The converter on a decode batch's PCM where it lies (dcs_decode_streams_at, dcs_decode_rate.hip.h) and the body of
// dcs_resample_out_streams: convert, fill outOffsets and info, then bring the samples down if they fit.  The PCM has to
// stay until this returns.
DcsStatus dcsRateFromDevice(DcsCtx *ctx, const int16_t *dPcm, const uint64_t *sampleOffsets, uint32_t n, uint32_t outRate,
                            const DcsResampleFilter *filter, uint32_t flags, int16_t *out, size_t outCapSamples, uint64_t *outOffsets,
                            DcsRateInfo *info)
{
    return encGuard([&]() -> DcsStatus {
        if (ctx == nullptr || sampleOffsets == nullptr || outOffsets == nullptr)
            return DCS_ERR_INVALID_ARG;
        DcsResampleFilter f;
        std::string why;
        const DcsStatus status = rsOutCheck(n, sampleOffsets, outRate, filter, flags, f, why);
        if (status != DCS_OK)
        {
            dcsCtxSetError(ctx, why.c_str());
            return status;
        }
        outOffsets[0] = 0;
        if (n == 0)
            return DCS_OK;
        // (DCS_RATE_TRACE: where a call's time goes, on stderr; the first figure includes the wait for whatever made dPcm)
        static const bool trace = getenv("DCS_RATE_TRACE") != nullptr;
        const auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        const double t0 = trace ? now() : 0;
        CacheArena held(ctx);
        RsConverted16 c;
        ENCTRY(rsConvertPcm16(ctx, dPcm, sampleOffsets, n, outRate, f, flags, held, c));
        memcpy(outOffsets, c.offsets.data(), sizeof(uint64_t) * c.offsets.size());
        if (info != nullptr)
            memcpy(info, c.info.data(), sizeof(DcsRateInfo) * n);
        if (out == nullptr || outCapSamples < c.offsets[n])
            return DCS_ERR_CAPACITY;
        const double t1 = trace ? now() : 0;
        ENCCHK(hipMemcpyAsync(out, c.d, sizeof(int16_t) * c.offsets[n], hipMemcpyDeviceToHost, held.stream()));
        ENCCHK(hipStreamSynchronize(held.stream()));
        if (trace)
            fprintf(stderr, "rate convert: walks, convolution and waits %.3f ms, download %.3f ms (%llu bytes)\n", t1 - t0, now() - t1,
                    static_cast<unsigned long long>(sizeof(int16_t) * c.offsets[n]));
        return DCS_OK;
    });
}

// the output-rate entry points' argument check on its own, for a caller that has device work of its own to do first
// (sampleOffsets null: the rate, the table and the flags alone)
DcsStatus dcsRateCheck(DcsCtx *ctx, const uint64_t *sampleOffsets, uint32_t n, uint32_t outRate, const DcsResampleFilter *filter,
                       uint32_t flags)
{
    return encGuard([&]() -> DcsStatus {
        DcsResampleFilter f;
        std::string why;
        const DcsStatus status = rsOutCheck(n, sampleOffsets, outRate, filter, flags, f, why);
        if (status != DCS_OK)
            dcsCtxSetError(ctx, why.c_str());
        return status;
    });
}

extern "C" DcsStatus dcs_resample_out_count(uint64_t nSamples, uint32_t outRate, const DcsResampleFilter *filter, uint32_t flags,
                                            uint64_t *countOut)
{
    if (countOut == nullptr)
        return DCS_ERR_INVALID_ARG;
    return encGuard([&] {
        const uint64_t offs[2] = { 0, nSamples };
        DcsResampleFilter f;
        std::string why;
        const DcsStatus st = rsOutCheck(1, offs, outRate, filter, flags, f, why);
        if (st == DCS_OK)
            *countOut = rsWalk(rsOutStreamOf(nSamples, outRate, f, flags), [](uint64_t, int64_t, int32_t) {});
        return st;
    });
}

// host only, for tests: the walk records (pos, start_filter_index) of a stream of nSamples at outRate, at most cap of them
// into pos[] and sfi[]; *countOut = the walk's count
extern "C" DcsStatus dcs_resample_out_walk(uint64_t nSamples, uint32_t outRate, const DcsResampleFilter *filter, uint32_t flags,
                                           int64_t *pos, int32_t *sfi, uint64_t cap, uint64_t *countOut)
{
    if (countOut == nullptr || (cap != 0 && (pos == nullptr || sfi == nullptr)))
        return DCS_ERR_INVALID_ARG;
    return encGuard([&] {
        const uint64_t offs[2] = { 0, nSamples };
        DcsResampleFilter f;
        std::string why;
        const DcsStatus st = rsOutCheck(1, offs, outRate, filter, flags, f, why);
        if (st == DCS_OK)
            *countOut = rsWalk(rsOutStreamOf(nSamples, outRate, f, flags), [&](uint64_t k, int64_t p, int32_t s) {
                if (k < cap)
                {
                    pos[k] = p;
                    sfi[k] = s;
                }
            });
        return st;
    });
}

extern "C" DcsStatus dcs_resample_out_streams(DcsCtx *ctx, const int16_t *pcm, const uint64_t *sampleOffsets, uint32_t nStreams,
                                              uint32_t outRate, const DcsResampleFilter *filter, uint32_t flags, int16_t *out,
                                              size_t outCapSamples, uint64_t *outOffsets, DcsRateInfo *info)
{
    return encGuard([&]() -> DcsStatus {
        if (ctx == nullptr || sampleOffsets == nullptr || outOffsets == nullptr || (nStreams != 0 && pcm == nullptr))
            return DCS_ERR_INVALID_ARG;
        DcsResampleFilter f;
        std::string why;
        const DcsStatus status = rsOutCheck(nStreams, sampleOffsets, outRate, filter, flags, f, why);
        if (status != DCS_OK)
        {
            dcsCtxSetError(ctx, why.c_str());
            return status;
        }
        if (nStreams == 0)
        {
            outOffsets[0] = 0;
            return DCS_OK;
        }
        // the streams as they lie in the caller's array, gaps between them included
        const uint64_t lo = sampleOffsets[0], hi = sampleOffsets[nStreams];
        std::vector<uint64_t> offs(static_cast<size_t>(nStreams) + 1);
        for (uint32_t k = 0 ; k <= nStreams ; ++k)
            offs[k] = sampleOffsets[k] - lo;
        ENCCHK(hipSetDevice(dcsCtxDevice(ctx)));
        CacheArena held(ctx);
        int16_t *dPcm = nullptr;
        ENCCHK(held.alloc(&dPcm, hi - lo));
        ENCCHK(hipMemcpyAsync(dPcm, pcm + lo, sizeof(int16_t) * (hi - lo), hipMemcpyHostToDevice, held.stream()));
        return dcsRateFromDevice(ctx, dPcm, offs.data(), nStreams, outRate, filter, flags, out, outCapSamples, outOffsets, info);
    });
}
