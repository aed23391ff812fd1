// dcs_encode.hip -- the DCS encoder on the GPU: PCM at 31 250 Hz in, streams byte-identical to the reference's
// DCSEncoder out (DCSEncoder.cpp: TransformFrame :1001-1069, DFTAlgorithmOrig :1218-1358, DualFFT :1360-1500,
// Frame::Frame :2535-2571, CloseStream :717-850, CompressStream :859-960, CompressFrame94 :1623-2050, CompressFrame93b
// :2053-2470, BitWriter :2573-2704), for the 1994+ format and for OS93 (0x9301 / 0x9302).
//
// A translation unit of its own because of the floating-point contract below: the reference is plain x86-64 code that
// rounds every multiply and add separately, and byte-exact streams need the same here, in device AND host code.  The
// decoder's kernels keep the library's default contraction.  Division stays a real, correctly rounded division (hipcc's
// default for f32), f32 denormals stay on, and every sum that the reference accumulates serially is accumulated serially in
// its order: parallelism goes across frames, bands, candidate codes and streams, never inside one sum.
//
//   E1 encAnalyseKernel   one wavefront per frame: window, bit-reversed load, 6 radix-2 stages, the odd-coefficient pass,
//                         the folds, the twiddle, the sign fix (each stage element-parallel over LDS); per-band power / lo / hi
//   E2 encStreamKernel    one wavefront per stream: powerSum in frame order and the range
//      encHeaderKernel    one wavefront per job: the header of each layout
//   E3 encSearchKernel    one thread per (frame, band, layout, pre-adjust): the 15 candidate codes' error sums, the best code
//                         with and without code 15 (the only things the previous frame's code can change)
//   E4 encChainKernel     one lane per (stream, layout, band): the walk over frames through those per-frame choices
//   E5 encBitsKernel / encSizeKernel / encHeadKernel / encPackKernel: bits per band and frame, stream sizes, the winner,
//                         frame bit offsets, and the bits themselves OR-ed into a zeroed buffer of big-endian words
//
// OS93 shares E1, E2 and the E5 size / head / swap steps (with the OS93 tables: 16 bands of 16 for the statistics, band
// norms 1.0, the layouts' own counts in the rate model) and replaces E3-E5a and the pack:
//   O3 enc93SearchKernel  one thread per (frame, band, layout): the scaled integers, the sub-type 0 search, and what the
//                         band's delta codes need that does not depend on the previous band (Enc93Rec)
//   O4 enc93WalkKernel    CompressFrame93b's band loop: Type 0 one lane per frame (no state crosses frames), Type 1 one lane
//                         per stream, frame after frame (the band-type codes carried from frame to frame)
//   O5 enc93PackKernel    one lane per (frame, band): the band's flag and type bits, then its samples
//
// OS93a Type 1, the pair-table layout no reference encoder writes, shares E1 and the swap and has an algorithm and kernels
// (A1-A5) of its own, dcs_encode93a.hip.h: a third family of the one driver, chosen per job by its set's type, so that one
// call (dcs_encode93a_sweep) may hold Type-0 jobs on the O stages and Type-1 jobs on the A stages.
//
// The rate-distortion 1994+ encoder (dcs_encode_rd_streams) is a fourth family, R1-R6 in dcs_encode_rd.hip.h: it shares E1,
// the swap and the driver, writes the 1994+ format from a trellis search of its own and holds each job to a byte budget; a
// call of it has jobs of this family only.
//
// The rate-distortion OS93 Type-0 encoder (dcs_encode93_rd_streams) is a fifth family, S1-S8 in dcs_encode93_rd.hip.h, under the
// same rules: E1, the swap and the driver are shared, the trellis runs over the bands of a frame, a call has jobs of this family only.
//
// E1 and encStreamKernel run per stream and do not read the parameters, and neither does A1's search; A1's walk reads one
// of them, maximumQuantizationError, and runs once per distinct value.  Everything behind them runs per JOB, a stream
// encoded with one parameter set (EncJob, EncSet): its rows in the per-frame buffers are the job's own, the spectrum it reads
// is its stream's.  dcs_encode_streams and its kin are one job per stream with one set; dcs_encode_sweep and
// dcs_encode93a_sweep are any list of jobs, and with DCS_SWEEP_MEASURE decode every job's stream where the pack step left it
// and reduce the round trip's error (encMeasureKernel).
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <stdio.h>
#include <algorithm>
#include <functional>
#include <atomic>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>
#include "../../include/dcs_hip.h"
#include "dcs_tables.h"
#include "dcs_enc_tables.h"
#include "dcs_cache.h"

int dcsCtxDevice(DcsCtx *ctx);
hipStream_t dcsCtxStream(DcsCtx *ctx);
void dcsCtxSetError(DcsCtx *ctx, const char *text);

namespace {

// Everything the encoder looks up, in one block that is built on the host (from dcs_tables.h and dcs_enc_tables.h) and
// copied to the device per call.  One instance per format family: count / first / bandNorm are the statistics' bands
// (Frame::Frame, CloseStream), shareCount[type] the bands the rate model weighs (CompressStream :866-868).
struct EncTabs
{
    float window[16], twiddle[128], fft[896], bandNorm[16];
    int32_t share[16], count[16], first[16], scale[64];
    int32_t os93;                      // OS93: no Type-1 scale adjust, no sub-type bits in the header
    int32_t shareCount[2][16];
    uint8_t preAdj[2][16];             // sub-type 0, sub-type 3
    uint8_t xw[3][16], xa[3][16];      // Type 1 band-type code -> bit width / scale adjust, for bands 0-2, 3-5, 6-15
    uint32_t hdrCode[31];              // frame-header band-type delta codes, index delta + 16
    uint8_t hdrLen[31];
    uint16_t smpCode[7][64];           // sample codebooks 1..6, index = stored value
    uint8_t smpLen[7][64];
    uint16_t dzCode[7];                // the codebooks' two-zeros code
    uint8_t dzLen[7];
    uint32_t btCode[2][32];            // OS93 Type 1 band-type delta codes, [Invert][delta + 16] (Keep: -15..14, Invert: -16..15)
    uint8_t btLen[2][32];
};

float fromBits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }

EncTabs buildTabs(bool os93)
{
    EncTabs t;
    memset(&t, 0, sizeof(t));
    t.os93 = os93;
    for (int i = 0 ; i < 16 ; ++i) t.window[i] = fromBits(kEncWindowBits[i]);
    for (int i = 0 ; i < 128 ; ++i) t.twiddle[i] = fromBits(kEncTwiddleBits[i]);
    for (int i = 0 ; i < 896 ; ++i) t.fft[i] = fromBits(kEncFftBits[i]);
    for (int b = 0, first = 0 ; b < 16 ; ++b)
    {
        t.bandNorm[b] = os93 ? 1.0f : fromBits(kEncBandNormBits[b]);
        t.share[b] = kEncBandShare[b];
        t.count[b] = os93 ? 16 : kBandCount94[b];
        t.first[b] = first;
        first += t.count[b];
        t.shareCount[0][b] = t.count[b];
        t.shareCount[1][b] = os93 && b == 0 ? 15 : t.count[b];       // OS93b Type 1: 15 samples in band 0
    }
    // the scaling factors are the decoder's mantissas at the code's octave (tools/extract_enc_tables.py checks this equal
    // to the reference's table)
    for (int j = 0 ; j < 64 ; ++j) t.scale[j] = kScaleMant[j & 3] >> (15 - (j >> 2));
    for (int i = 0 ; i < 16 ; ++i)
    {
        t.preAdj[0][i] = kPreAdjSub0[i];
        t.preAdj[1][i] = kPreAdjSub3[i];
        const uint16_t *x[3] = { kXlatB02, kXlatB35, kXlatB6F };
        for (int k = 0 ; k < 3 ; ++k) { t.xw[k][i] = x[k][i] & 0xFF; t.xa[k][i] = x[k][i] >> 8; }
    }
    // encode codebooks = the inverses of the decode trees
    for (const DcsVlc &v : kVlc94BandTypeDelta) { t.hdrCode[v.val + 16] = v.code; t.hdrLen[v.val + 16] = v.len; }
    const DcsVlc *books[7] = { nullptr, kVlc94Sample1, kVlc94Sample2, kVlc94Sample3, kVlc94Sample4, kVlc94Sample5, kVlc94Sample6 };
    for (int w = 1 ; w <= 6 ; ++w)
        for (int i = 0 ; i < (1 << w) + 1 ; ++i)
        {
            const DcsVlc &v = books[w][i];
            if (v.val & 0x80) { t.dzCode[w] = static_cast<uint16_t>(v.code); t.dzLen[w] = v.len; }
            else { t.smpCode[w][v.val] = static_cast<uint16_t>(v.code); t.smpLen[w][v.val] = v.len; }
        }
    // the decoder's leaf: < 0x1E keeps the band sub-type (delta = leaf - 0x0F), else inverts it (delta = leaf - 0x2E)
    for (const DcsVlc &v : kVlc93BandType)
    {
        const int inv = v.val >= 0x1E ? 1 : 0;
        const int d = v.val - (inv ? 0x2E : 0x0F);
        t.btCode[inv][d + 16] = v.code;
        t.btLen[inv][d + 16] = v.len;
    }
    return t;
}

const EncTabs &encTabs() { static const EncTabs t = buildTabs(false); return t; }
const EncTabs &encTabs93() { static const EncTabs t = buildTabs(true); return t; }

// CloseStream's band cutoff and CompressStream's header (the rate model), for one layout of either family.  The reference computes
// 1 << bitsPerBand[band] with counts above 31 at its default settings (few bands kept); its x86 build masks the count,
// and that is the rule here, written out.
__host__ __device__ void encHeader(const EncTabs &T, const float *ps, const float *lo, const float *hi, float cutoff, int rate,
                                   int typ, int sub, uint8_t *hdr, int *keepOut, int *bits)
{
    float rms[16], total = 0.0f;
    for (int i = 0 ; i < 16 ; ++i)
    {
        rms[i] = sqrtf(ps[i] * T.bandNorm[i]);
        total += rms[i];
    }
    const float powerNorm = 1.0f / total;
    int keep = 16;
    if (total != 0.0f)
    {
        float below = 0.0f;
        for (int i = 0 ; i < 16 ; ++i)
        {
            below += rms[i] * powerNorm;
            if (below >= cutoff) { keep = i; break; }
        }
    }
    const float framesPerSecond = 31250.0f / 240.0f;
    const float bitsPerFrame = static_cast<float>(rate) / framesPerSecond;
    float shareNorm = 0.0f;
    for (int i = 0 ; i < keep ; ++i)
        shareNorm += static_cast<float>(T.share[i] * T.shareCount[typ][i]);
    for (int b = 0 ; b < 16 ; ++b) { hdr[b] = 0xFF; bits[b] = 0; }
    for (int b = 0 ; b < keep ; ++b)
    {
        bits[b] = static_cast<int>(static_cast<float>(T.share[b]) / shareNorm * bitsPerFrame);
        float l = lo[b] * -32768.0f, h = hi[b] * 32768.0f;
        if (l < 0) l = 0;
        if (h < 0) h = 0;
        const float fullScale = h > l ? h : l;
        const int divider = static_cast<int>(1u << (bits[b] & 31));       // x86 shl semantics; 1u << 31 reads as INT32_MIN
        const int target = fullScale != 0 ? static_cast<int>(ceilf(fullScale / static_cast<float>(divider))) : 1;
        int code = 0;
        for (int j = 0 ; j < 64 ; ++j)
        {
            if (T.scale[j] < target) code = j;
            else break;
        }
        if (typ == 1 && !T.os93)
        {
            const int adjust = (b < 3 ? 0x0d : 0x17) + (sub == 0 ? 1 : 3);
            code = code > adjust ? code - adjust : 0;
        }
        hdr[b] = static_cast<uint8_t>(code);
    }
    if (typ != 0) hdr[0] |= 0x80;
    if (!T.os93)
    {
        hdr[1] |= static_cast<uint8_t>((sub & 2) << 6);
        hdr[2] |= static_cast<uint8_t>((sub & 1) << 7);
    }
    *keepOut = keep;
}

// a band-type code -> bit width and scale index (CompressFrame94's InterpretBandTypeCode, :1669-1760)
__device__ inline void encInterpret(const EncTabs &T, int typ, int band, int code, int hscale, int pre, int *w, int *sc)
{
    if (code == 0) { *w = 0; *sc = 0; return; }
    if (typ == 0) { *w = code; *sc = hscale; return; }
    const int k = band < 3 ? 0 : band < 6 ? 1 : 2;
    *w = T.xw[k][code];
    *sc = hscale + T.xa[k][code] + (band < 3 ? pre : 0);
}

// FindBestResult over codes 1..15 and over 1..14: the narrowest passing width, then the smallest error among the codes of
// that width (of all codes when none passes), the first on a tie -> best | bestWithout15 << 4
__device__ inline uint8_t encPick(const float *err, const int *width, const bool *elig, const bool *pass)
{
    int best[2];
#pragma unroll
    for (int set = 0 ; set < 2 ; ++set)
    {
        const int last = set == 0 ? 15 : 14;
        int narrow = -1;
        for (int c = 1 ; c <= last ; ++c)
            if (elig[c - 1] && pass[c - 1] && (narrow == -1 || width[c - 1] < narrow))
                narrow = width[c - 1];
        float minErr = -1.0f;
        int b = 0;
        for (int c = 1 ; c <= last ; ++c)
            if (elig[c - 1] && (narrow == -1 || width[c - 1] == narrow) && (minErr < 0 || err[c - 1] < minErr))
            {
                b = c;
                minErr = err[c - 1];
            }
        best[set] = b;
    }
    return static_cast<uint8_t>(best[0] | (best[1] << 4));
}

// FindBestBandEncoding + FindBestResult (:1502-1621) over codes 1..15 at one pre-adjust; returns best | bestWithout15 << 4.
// A code whose scale index exceeds 0x3f is not eligible (the reference reads past its table there).
__device__ uint8_t encSearch(const EncTabs &T, const float *smp, int n, int typ, int band, int hscale, int pre, float errMax)
{
    float err[15];
    int width[15];
    bool elig[15], pass[15];
#pragma unroll
    for (int c = 1 ; c <= 15 ; ++c)
    {
        int w, sc;
        encInterpret(T, typ, band, c, hscale, pre, &w, &sc);
        width[c - 1] = w;
        elig[c - 1] = sc <= 0x3f;
        err[c - 1] = 0.0f;
        pass[c - 1] = false;
        if (!elig[c - 1])
            continue;
        const float scaleFactor = static_cast<float>(T.scale[sc]);
        const int refVal = 1 << (w - 1);                   // (the search biases every width, raw ones too: :1534)
        const int mask = 0xFFFF >> (16 - w);
        float sum = 0.0f;
        for (int i = 0 ; i < n ; ++i)
        {
            const float orig = smp[i];
            const int scaled = static_cast<int>(roundf(orig * 32768.0f / scaleFactor));
            const int stored = (scaled + refVal) & mask;
            const float reconstructed = (static_cast<float>(stored - refVal) * scaleFactor) / 32768.0f;
            const float q = reconstructed - orig;
            sum += q * q;
        }
        err[c - 1] = sum;
        pass[c - 1] = sum <= errMax;
    }
    return encPick(err, width, elig, pass);
}

// MSB-first bits into big-endian words (byte-swapped at the end); frames and streams share boundary words, hence the OR
__device__ inline void encPut(uint32_t *W, uint64_t pos, uint32_t val, int len)
{
    const uint64_t wi = pos >> 5;
    const int end = static_cast<int>(pos & 31) + len;
    if (end <= 32)
        atomicOr(&W[wi], val << (32 - end));
    else
    {
        atomicOr(&W[wi], val >> (end - 32));
        atomicOr(&W[wi + 1], val << (64 - end));
    }
}

// one band's samples (CompressFrame94 :1996-2045): returns their bit count, and writes them when W != nullptr
__device__ uint32_t encBandSamples(const EncTabs &T, const float *smp, int n, int w, int sc, uint32_t *W, uint64_t pos)
{
    if (w == 0)
        return 0;
    const float scaleFactor = static_cast<float>(T.scale[sc]);
    const int mask = 0xFFFF >> (16 - w);
    const bool book = w <= 6;
    const int refVal = book ? 1 << (w - 1) : 0;
    uint32_t bits = 0;
    for (int i = 0 ; i < n ; ++i)
    {
        const int s = static_cast<int>(roundf(smp[i] * 32768.0f / scaleFactor));
        uint32_t code;
        int len;
        if (book && s == 0 && i + 1 < n && static_cast<int>(roundf(smp[i + 1] * 32768.0f / scaleFactor)) == 0)
        {
            code = T.dzCode[w];
            len = T.dzLen[w];
            ++i;
        }
        else
        {
            const int v = (s + refVal) & mask;
            code = book ? T.smpCode[w][v] : static_cast<uint32_t>(v);
            len = book ? T.smpLen[w][v] : w;
        }
        if (W != nullptr)
            encPut(W, pos + bits, code, len);
        bits += static_cast<uint32_t>(len);
    }
    return bits;
}

// errFrame: the decoder's error word of the stream's first frame (int16 input from a decode batch; 0 for float input)
struct EncStream { uint64_t sampleOff; uint32_t nSamples, firstFrame, nFrames, errFrame; float bound; };   // bound: largest |x|

// A job: stream `stream` encoded with parameter set `set`.  Its nFrames rows in the per-job-frame buffers (best, codes, bits,
// frame offsets) start at firstFrame; row k reads frame specFirst + k of E1's output (specFirst = its stream's firstFrame).
struct EncJob { uint32_t stream, set, firstFrame, nFrames, specFirst; };

// what the kernels read of a DcsEncodeParams: vmask = the layouts to compute, cmask = CloseStream's candidates (EncRun::buildSets)
struct EncSet { float cutoff, minDR, maxQE; int32_t rate; uint32_t vmask, cmask; };

// the frame of E1's output that row f of the per-job-frame buffers reads
__device__ inline uint32_t encSpecFrame(const EncJob &j, uint32_t f) { return j.specFirst + (f - j.firstFrame); }

// layouts computed: v0 = Type 0 (sub-types 0 and 3 differ only in two header bits), v1 = Type 1 sub-type 0, v2 = Type 1
// sub-type 3.  Search slots per (frame, band): 0 = v0; 1, 2 = v1 at pre-adjust 0, 1; 3..7 = v2 at pre-adjust 0..4.
__device__ inline int encSlot(const EncTabs &T, int v, int band, int old)
{
    if (v == 0) return 0;
    return (v == 1 ? 1 : 3) + (band < 3 ? T.preAdj[v - 1][old] : 0);
}

__device__ inline int encPre(const EncTabs &T, int v, int band, int old)
{
    return (v != 0 && band < 3) ? T.preAdj[v - 1][old] : 0;
}

__device__ inline int rev7(int i) { return static_cast<int>(__builtin_bitreverse32(static_cast<uint32_t>(i)) >> 25); }

// E1: one wavefront per frame, four frames per block.  S = float: the caller's samples, |x| <= 1 checked.  S = int16_t: a
// decode batch's resident PCM, x / 32768 (a power of two: exact, the same value as the float path's x / 32768.0f); frame
// k of the stream reads decoded frames k - 1 and k, and lane 0 ORs decoded frame k's error word into the stream's flag.
template <typename S>
__global__ __launch_bounds__(256) void encAnalyseKernel(const EncTabs *__restrict__ Tp, const S *__restrict__ pcm,
    const EncStream *__restrict__ streams, const uint32_t *__restrict__ frameStream, uint32_t F, float *__restrict__ spec,
    float *__restrict__ pw, float *__restrict__ flo, float *__restrict__ fhi, uint32_t *__restrict__ bad,
    const uint32_t *__restrict__ err)
{
    constexpr bool kPcm16 = std::is_same<S, int16_t>::value;
    const EncTabs &T = *Tp;
    __shared__ float lds[4][260];
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
    const uint32_t f = blockIdx.x * 4 + wv;
    const bool live = f < F;
    float *b = lds[wv];
    if (live)
    {
        const uint32_t si = frameStream[f];
        const EncStream s = streams[si];
        const int64_t base = static_cast<int64_t>(f - s.firstFrame) * 240 - 16;
        bool isBad = false;
        for (int q = 0 ; q < 4 ; ++q)
        {
            const int i = l + 64 * q;
            const int64_t idx = base + i;
            const S raw = (idx >= 0 && idx < static_cast<int64_t>(s.nSamples)) ? pcm[s.sampleOff + static_cast<uint64_t>(idx)] : S(0);
            float x;
            if constexpr (kPcm16)
                x = static_cast<float>(raw) * (1.0f / 32768.0f);
            else
            {
                x = raw;
                if (!(fabsf(x) <= s.bound))
                    isBad = true;
            }
            if (i < 16) x *= T.window[i];
            else if (i >= 240) x *= T.window[255 - i];
            b[(rev7(i >> 1) << 1) | (i & 1)] = x;
        }
        if constexpr (kPcm16)
            if (l == 0 && err[s.errFrame + (f - s.firstFrame)] != 0)
                isBad = true;
        if (isBad)
            atomicOr(&bad[si], 1u);
    }
    __syncthreads();
    for (int st = 1 ; st <= 6 ; ++st)
    {
        if (live)
        {
            const int half = 1 << (st - 1);
            const int j = l & (half - 1), k = (l >> (st - 1)) * 2 * half;
            const float c = T.fft[(st - 1) * 128 + 2 * l], sn = T.fft[(st - 1) * 128 + 2 * l + 1];
            const int t = (k + j + half) * 2, u = (k + j) * 2;
            const float ar = b[t], ai = b[t + 1], ur = b[u], ui = b[u + 1];
            const float tr = ar * c - ai * sn;
            const float ti = ar * sn + ai * c;
            b[u] = tr + ur;
            b[u + 1] = ti + ui;
            b[t] = ur - tr;
            b[t + 1] = ui - ti;
        }
        __syncthreads();
    }
    if (live && l >= 1)
    {
        const float c = T.fft[896 - 126 + 2 * (l - 1)], sn = T.fft[896 - 126 + 2 * (l - 1) + 1];
        const int t = 128 + l * 2;
        const float ar = b[t], ai = b[t + 1];
        b[t] = ar * c - ai * sn;
        b[t + 1] = ar * sn + ai * c;
    }
    __syncthreads();
    if (live)
        for (int q = 0 ; q < 4 ; ++q)
            b[l + 64 * q] *= (1 / 64.0f);
    __syncthreads();
    if (live && l == 0)
    {
        b[0x1] = (b[0x0] + b[0x80]) / 2.0f;
        b[0x81] = b[0x1];
        b[0x100] = b[0x1];
        b[0x101] = b[0x1];
    }
    __syncthreads();
    if (live)        // even/odd folding
    {
        const int p0 = 2 * l, p1 = 0x80 + 2 * l;
        const float x0 = b[p0], y0 = b[p0 + 1], x1 = b[p1], y1 = b[p1 + 1];
        b[p0] = (x0 + x1) / 2.0f;
        b[p0 + 1] = (y0 + y1) / 2.0f;
        b[p1] = (x0 - x1) / 2.0f;
        b[p1 + 1] = (y0 - y1) / 2.0f;
    }
    __syncthreads();
    if (live)        // twiddling
    {
        const int p0 = 2 * l, p1 = 0x100 - 2 * l;
        const float x0 = b[p0], y0 = b[p0 + 1], x1 = b[p1], y1 = b[p1 + 1];
        const float xsum = (x0 - x1) / 2.0f;
        const float ysum = (y0 + y1) / 2.0f;
        const float costh = T.twiddle[2 * l], sinth = T.twiddle[2 * l + 1];
        b[p0] = (x0 + x1) / 2.0f;
        b[p0 + 1] = (y0 - y1) / 2.0f;
        b[p1] = xsum * sinth - ysum * costh;
        b[p1 + 1] = xsum * costh + ysum * sinth;
    }
    __syncthreads();
    if (live)        // high/low folding
    {
        const int p0 = 2 * l, p1 = 0x100 - 2 * l;
        const float x0 = -b[p0], y0 = -b[p0 + 1], x1 = -b[p1], y1 = -b[p1 + 1];
        b[p0] = (x0 + x1) / 2.0f;
        b[p0 + 1] = (y0 + y1) / 2.0f;
        b[p1] = (x0 - x1) / 2.0f;
        b[p1 + 1] = (y0 - y1) / 2.0f;
    }
    __syncthreads();
    if (live && l == 0)
    {
        b[0x80] = -b[0x80];
        b[0x81] = -b[0x81];
    }
    __syncthreads();
    if (live)
        b[129 + 2 * l] = -b[129 + 2 * l];
    __syncthreads();
    if (live && l == 0)
        b[1] = b[0];
    __syncthreads();
    if (!live)
        return;
    // the frame is b[1 .. 256]
    for (int q = 0 ; q < 4 ; ++q)
        spec[static_cast<size_t>(f) * 256 + l + 64 * q] = b[1 + l + 64 * q];
    if (l < 16)
    {
        const float *p = b + 1 + T.first[l];
        float lo = p[0], hi = lo, power = lo * lo;
        for (int j = 1 ; j < T.count[l] ; ++j)
        {
            const float s = p[j];
            power += s * s;
            if (s < lo) lo = s;
            if (s > hi) hi = s;
        }
        pw[static_cast<size_t>(f) * 16 + l] = power;
        flo[static_cast<size_t>(f) * 16 + l] = lo;
        fhi[static_cast<size_t>(f) * 16 + l] = hi;
    }
}

// E2: one wavefront per stream: sums[stream][0 / 1 / 2][band] = powerSum in frame order, the lowest and the highest sample
__global__ __launch_bounds__(64) void encStreamKernel(const EncStream *__restrict__ streams, const float *__restrict__ pw,
    const float *__restrict__ flo, const float *__restrict__ fhi, float *__restrict__ sums)
{
    const EncStream s = streams[blockIdx.x];
    const int l = threadIdx.x;
    if (l < 16)
    {
        float ps = 0.0f, lo = 0.0f, hi = 0.0f;
        constexpr int U = 16;
        for (uint32_t j0 = 0 ; j0 < s.nFrames ; j0 += U)
        {
            float p[U], a[U], c[U];
#pragma unroll
            for (int u = 0 ; u < U ; ++u)
            {
                const uint32_t j = j0 + u < s.nFrames ? j0 + u : s.nFrames - 1;
                const size_t idx = static_cast<size_t>(s.firstFrame + j) * 16 + l;
                p[u] = pw[idx]; a[u] = flo[idx]; c[u] = fhi[idx];
            }
#pragma unroll
            for (int u = 0 ; u < U ; ++u)
            {
                if (j0 + u >= s.nFrames) break;
                ps += p[u];                                   // powerSum in frame order
                if (j0 + u == 0 || a[u] < lo) lo = a[u];
                if (j0 + u == 0 || c[u] > hi) hi = c[u];
            }
        }
        float *o = sums + static_cast<size_t>(blockIdx.x) * 48 + l;
        o[0] = ps; o[16] = lo; o[32] = hi;
    }
}

// E2, the header half: one wavefront per job, one lane per layout
__global__ __launch_bounds__(64) void encHeaderKernel(const EncTabs *__restrict__ Tp, const EncJob *__restrict__ jobs,
    const EncSet *__restrict__ sets, const float *__restrict__ sums, uint8_t *__restrict__ hdrOut, int32_t *__restrict__ keepOut)
{
    __shared__ float sSum[48];
    const EncJob j = jobs[blockIdx.x];
    const EncSet p = sets[j.set];
    const int l = threadIdx.x;
    if (l < 48)
        sSum[l] = sums[static_cast<size_t>(j.stream) * 48 + l];
    __syncthreads();
    if (l < 3 && ((p.vmask >> l) & 1))
    {
        uint8_t hdr[16];
        int bits[16], keep;
        encHeader(*Tp, sSum, sSum + 16, sSum + 32, p.cutoff, p.rate, l == 0 ? 0 : 1, l == 2 ? 3 : 0, hdr, &keep, bits);
        for (int b = 0 ; b < 16 ; ++b)
            hdrOut[(static_cast<size_t>(blockIdx.x) * 3 + l) * 16 + b] = hdr[b];
        keepOut[blockIdx.x] = keep;                         // (the same for every layout)
    }
}

// E3: one block per job-frame, one thread per (band, slot)
__global__ __launch_bounds__(128) void encSearchKernel(const EncTabs *__restrict__ Tp, const float *__restrict__ spec,
    const float *__restrict__ flo, const float *__restrict__ fhi, const uint32_t *__restrict__ frameJob,
    const EncJob *__restrict__ jobs, const EncSet *__restrict__ sets, const uint8_t *__restrict__ hdr,
    const int32_t *__restrict__ keepArr, uint8_t *__restrict__ best)
{
    const EncTabs &T = *Tp;
    __shared__ float smp[256];
    const uint32_t f = blockIdx.x;
    const int t = threadIdx.x;
    const uint32_t ji = frameJob[f];
    const EncJob job = jobs[ji];
    const uint32_t sf = encSpecFrame(job, f);
    smp[t] = spec[static_cast<size_t>(sf) * 256 + t];
    smp[t + 128] = spec[static_cast<size_t>(sf) * 256 + 128 + t];
    __syncthreads();
    const int band = t >> 3, slot = t & 7;
    if (band >= keepArr[ji])
        return;
    const EncSet p = sets[job.set];
    const int v = slot == 0 ? 0 : slot < 3 ? 1 : 2;
    const int pre = slot == 0 ? 0 : slot < 3 ? slot - 1 : slot - 3;
    if (!((p.vmask >> v) & 1) || (band >= 3 && pre != 0))
        return;
    const size_t sb = static_cast<size_t>(sf) * 16 + band;
    uint8_t out = 0;
    if (!(fhi[sb] - flo[sb] < p.minDR))
    {
        const int n = T.count[band];
        const float errMax = (p.maxQE * p.maxQE) * static_cast<float>(n);
        out = encSearch(T, smp + T.first[band], n, v == 0 ? 0 : 1, band, hdr[(static_cast<size_t>(ji) * 3 + v) * 16 + band] & 0x3f, pre, errMax);
    }
    best[(static_cast<size_t>(f) * 16 + band) * 8 + slot] = out;
}

// E4: one block per job, one lane per (layout, band): the band-type codes, frame after frame
__global__ __launch_bounds__(64) void encChainKernel(const EncTabs *__restrict__ Tp, const EncJob *__restrict__ jobs,
    const EncSet *__restrict__ sets, const int32_t *__restrict__ keepArr, uint32_t F, const uint64_t *__restrict__ best,
    uint8_t *__restrict__ codes)
{
    const EncTabs &T = *Tp;
    const EncJob s = jobs[blockIdx.x];
    const uint32_t vmask = sets[s.set].vmask;
    const int v = threadIdx.x >> 4, band = threadIdx.x & 15;
    if (v >= 3 || !((vmask >> v) & 1) || band >= keepArr[blockIdx.x])
        return;
    int old = 0;
    constexpr int U = 16;
    for (uint32_t j0 = 0 ; j0 < s.nFrames ; j0 += U)
    {
        uint64_t row[U];
#pragma unroll
        for (int u = 0 ; u < U ; ++u)
        {
            const uint32_t j = j0 + u < s.nFrames ? j0 + u : s.nFrames - 1;
            row[u] = best[static_cast<size_t>(s.firstFrame + j) * 16 + band];
        }
#pragma unroll
        for (int u = 0 ; u < U ; ++u)
        {
            if (j0 + u >= s.nFrames) break;
            const int b = static_cast<int>((row[u] >> (8 * encSlot(T, v, band, old))) & 0xFF);
            const int nw = old == 0 ? b >> 4 : b & 15;        // old == 0: code 15 is out of reach (delta > 14)
            codes[(static_cast<size_t>(v) * F + s.firstFrame + j0 + u) * 16 + band] = static_cast<uint8_t>(nw);
            old = nw;
        }
    }
}

// E5a: one block per job-frame, one lane per (layout, band): header-code and sample bits
__global__ __launch_bounds__(64) void encBitsKernel(const EncTabs *__restrict__ Tp, const float *__restrict__ spec,
    const uint32_t *__restrict__ frameJob, const EncJob *__restrict__ jobs, const EncSet *__restrict__ sets,
    const uint8_t *__restrict__ hdr, const int32_t *__restrict__ keepArr, uint32_t F, const uint8_t *__restrict__ codes,
    uint8_t *__restrict__ hdrBits, uint16_t *__restrict__ smpBits, uint32_t *__restrict__ frameBits)
{
    const EncTabs &T = *Tp;
    __shared__ float smp[256];
    __shared__ uint32_t fb[3][16];
    const uint32_t f = blockIdx.x;
    const int l = threadIdx.x;
    const uint32_t si = frameJob[f];
    const EncJob job = jobs[si];
    const uint32_t sf = encSpecFrame(job, f), vmask = sets[job.set].vmask;
    for (int q = 0 ; q < 4 ; ++q)
        smp[l + 64 * q] = spec[static_cast<size_t>(sf) * 256 + l + 64 * q];
    __syncthreads();
    const int v = l >> 4, band = l & 15;
    uint32_t hb = 0, sb = 0;
    if (v < 3 && ((vmask >> v) & 1) && band < keepArr[si])
    {
        const size_t at = (static_cast<size_t>(v) * F + f) * 16 + band;
        const int code = codes[at];
        const int old = f == job.firstFrame ? 0 : codes[at - 16];
        hb = T.hdrLen[code - old + 16];
        int w, sc;
        encInterpret(T, v == 0 ? 0 : 1, band, code, hdr[(static_cast<size_t>(si) * 3 + v) * 16 + band] & 0x3f, encPre(T, v, band, old), &w, &sc);
        sb = encBandSamples(T, smp + T.first[band], T.count[band], w, sc, nullptr, 0);
        hdrBits[at] = static_cast<uint8_t>(hb);
        smpBits[at] = static_cast<uint16_t>(sb);
    }
    if (v < 3)
        fb[v][band] = hb + sb;
    __syncthreads();
    if (l < 3)
    {
        uint32_t sum = 0;
        for (int b = 0 ; b < 16 ; ++b)
            sum += fb[l][b];
        frameBits[static_cast<size_t>(l) * F + f] = sum;
    }
}

// E5b: one block per job: sizes of the layouts, the winner (the first strictly smallest, CloseStream :805), and the
// exclusive scan of the winner's frame bits
__global__ __launch_bounds__(256) void encSizeKernel(const EncJob *__restrict__ jobs, const EncSet *__restrict__ sets, uint32_t F,
    const uint32_t *__restrict__ frameBits, int32_t *__restrict__ winOut, uint64_t *__restrict__ sizeOut, uint32_t *__restrict__ frameOff)
{
    __shared__ uint64_t red[3][256];
    __shared__ uint32_t scan[256];
    __shared__ int sWin;
    __shared__ uint32_t carry;
    const EncJob s = jobs[blockIdx.x];
    const uint32_t cmask = sets[s.set].cmask;
    const int t = threadIdx.x;
    uint64_t tot[3] = { 0, 0, 0 };
    for (uint32_t j = t ; j < s.nFrames ; j += 256)
        for (int v = 0 ; v < 3 ; ++v)
            tot[v] += frameBits[static_cast<size_t>(v) * F + s.firstFrame + j];
    for (int v = 0 ; v < 3 ; ++v)
        red[v][t] = tot[v];
    __syncthreads();
    for (int w = 128 ; w > 0 ; w >>= 1)
    {
        if (t < w)
            for (int v = 0 ; v < 3 ; ++v)
                red[v][t] += red[v][t + w];
        __syncthreads();
    }
    if (t == 0)
    {
        int win = -1;
        uint64_t bestSize = 0;
        for (int c = 0 ; c < 4 ; ++c)           // (0,0), (0,3), (1,0), (1,3)
        {
            if (!((cmask >> c) & 1))
                continue;
            const int v = c < 2 ? 0 : c - 1;
            const uint64_t size = 18 + (red[v][0] + 7) / 8;
            if (win < 0 || size < bestSize) { win = c; bestSize = size; }
        }
        winOut[blockIdx.x] = win;
        sizeOut[blockIdx.x] = bestSize;
        sWin = win < 2 ? 0 : win - 1;
        carry = 0;
    }
    __syncthreads();
    const int v = sWin;
    for (uint32_t j0 = 0 ; j0 < s.nFrames ; j0 += 256)
    {
        const uint32_t j = j0 + t;
        const uint32_t x = j < s.nFrames ? frameBits[static_cast<size_t>(v) * F + s.firstFrame + j] : 0;
        scan[t] = x;
        __syncthreads();
        for (int w = 1 ; w < 256 ; w <<= 1)
        {
            const uint32_t y = t >= w ? scan[t - w] : 0;
            __syncthreads();
            scan[t] += y;
            __syncthreads();
        }
        if (j < s.nFrames)
            frameOff[s.firstFrame + j] = carry + scan[t] - x;
        __syncthreads();
        if (t == 255)
            carry += scan[255];
        __syncthreads();
    }
}

// E5c: the 2-byte frame count and the 16-byte header of each job's winner
__global__ __launch_bounds__(64) void encHeadKernel(const EncJob *__restrict__ jobs, const uint8_t *__restrict__ hdr,
    const int32_t *__restrict__ win, const uint64_t *__restrict__ outOff, uint32_t *__restrict__ W)
{
    const uint32_t si = blockIdx.x;
    const int k = threadIdx.x;
    if (k >= 18)
        return;
    const int c = win[si], v = c < 2 ? 0 : c - 1;
    if (c < 0)
        return;                                 // no layout of this family is the job's (cmask 0): an OS93a Type-1 job
    const uint32_t nF = jobs[si].nFrames;
    uint32_t byte;
    if (k < 2)
        byte = k == 0 ? nF >> 8 : nF & 0xFF;
    else
    {
        byte = hdr[(static_cast<size_t>(si) * 3 + v) * 16 + k - 2];
        if (c == 1 && (k == 3 || k == 4))       // Type 0 sub-type 3: the sub-type bits of header bytes 1 and 2
            byte |= 0x80;
    }
    encPut(W, outOff[si] * 8 + k * 8, byte, 8);
}

// E5d: four job-frames per block, one lane per band: the winner's header codes and samples
__global__ __launch_bounds__(64) void encPackKernel(const EncTabs *__restrict__ Tp, const float *__restrict__ spec,
    const uint32_t *__restrict__ frameJob, const EncJob *__restrict__ jobs, const uint8_t *__restrict__ hdr,
    const int32_t *__restrict__ keepArr, const int32_t *__restrict__ win, uint32_t F, const uint8_t *__restrict__ codes,
    const uint8_t *__restrict__ hdrBits, const uint16_t *__restrict__ smpBits, const uint32_t *__restrict__ frameOff,
    const uint64_t *__restrict__ outOff, uint32_t *__restrict__ W)
{
    const EncTabs &T = *Tp;
    __shared__ float smp[4][256];
    const int l = threadIdx.x;
    for (int q = 0 ; q < 16 ; ++q)
    {
        const int idx = l + 64 * q;
        const uint32_t ff = blockIdx.x * 4 + (idx >> 8);
        smp[idx >> 8][idx & 255] = ff < F ? spec[static_cast<size_t>(encSpecFrame(jobs[frameJob[ff]], ff)) * 256 + (idx & 255)] : 0.0f;
    }
    __syncthreads();
    const uint32_t f = blockIdx.x * 4 + (l >> 4);
    const int band = l & 15;
    if (f >= F)
        return;
    const uint32_t si = frameJob[f];
    const int keep = keepArr[si];
    if (band >= keep)
        return;
    const int c = win[si], v = c < 2 ? 0 : c - 1;
    const size_t row = (static_cast<size_t>(v) * F + f) * 16;
    uint32_t hOff = 0, hAll = 0, sOff = 0;
    for (int b = 0 ; b < keep ; ++b)
    {
        hAll += hdrBits[row + b];
        if (b < band)
        {
            hOff += hdrBits[row + b];
            sOff += smpBits[row + b];
        }
    }
    const uint64_t base = (outOff[si] + 18) * 8 + frameOff[f];
    const int code = codes[row + band];
    const int old = f == jobs[si].firstFrame ? 0 : codes[row - 16 + band];
    encPut(W, base + hOff, T.hdrCode[code - old + 16], T.hdrLen[code - old + 16]);
    int w, sc;
    encInterpret(T, v == 0 ? 0 : 1, band, code, hdr[(static_cast<size_t>(si) * 3 + v) * 16 + band] & 0x3f, encPre(T, v, band, old), &w, &sc);
    encBandSamples(T, smp[l >> 4] + T.first[band], T.count[band], w, sc, W, base + hAll + sOff);
}

__global__ __launch_bounds__(256) void encSwapKernel(uint32_t *W, size_t n)
{
    const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n)
        W[i] = __builtin_bswap32(W[i]);
}

// ---------------------------------------------------------------------------------------------------- OS93 (CompressFrame93b)

// a band of an OS93 layout: 16 bands of 16 samples over f[0..255]; Type 1 has 15 in band 0 and ends at f[254] (:2144)
__device__ inline void enc93Band(int typ, int band, int *first, int *n)
{
    *n = typ == 1 && band == 0 ? 15 : 16;
    *first = band * 16 - (typ == 1 && band > 0 ? 1 : 0);
}

// what the band loop needs of one (frame, band, layout) that does not depend on the bands before it: the sub-type 0
// code (pick = best | best without 15 << 4), the bit lengths of max |buf1[i]| for i >= 1 and of max |buf2[i]| for i >= 2
// (<< 8, << 16), and the scaled integers the incoming prvSample / prvDelta meet: the first two and the last sample and delta
struct Enc93Rec { int32_t s0, s1, sLast, dLast; uint32_t pick; };

// the band loop's output per (layout, frame, band): the flag and type-code bits (value, length), the incoming prvSample /
// prvDelta, and meta = flag/type length | code << 8 | band sub-type << 12 | sample bits << 16
struct Enc93Band { uint32_t hdr; int32_t P, D; uint32_t meta; };

__device__ inline uint32_t bitLen(uint32_t x) { return x ? 32u - static_cast<uint32_t>(__builtin_clz(x)) : 0u; }

__device__ inline uint32_t absI(int x) { return x < 0 ? 0u - static_cast<uint32_t>(x) : static_cast<uint32_t>(x); }

// O3: four job-frames per block, one thread per (frame, band, layout)
__global__ __launch_bounds__(128) void enc93SearchKernel(const EncTabs *__restrict__ Tp, const float *__restrict__ spec,
    const uint32_t *__restrict__ frameJob, const EncJob *__restrict__ jobs, const EncSet *__restrict__ sets,
    const uint8_t *__restrict__ hdr, const int32_t *__restrict__ keepArr, uint32_t F, Enc93Rec *__restrict__ rec)
{
    const EncTabs &T = *Tp;
    __shared__ float smp[4][256];
    const int t = threadIdx.x;
    for (int q = 0 ; q < 8 ; ++q)
    {
        const int idx = t + 128 * q;
        const uint32_t ff = blockIdx.x * 4 + (idx >> 8);
        smp[idx >> 8][idx & 255] = ff < F ? spec[static_cast<size_t>(encSpecFrame(jobs[frameJob[ff]], ff)) * 256 + (idx & 255)] : 0.0f;
    }
    __syncthreads();
    const uint32_t f = blockIdx.x * 4 + (t >> 5);
    const int v = (t >> 4) & 1, band = t & 15;
    if (f >= F)
        return;
    const uint32_t si = frameJob[f];
    const EncSet p = sets[jobs[si].set];
    if (!((p.vmask >> v) & 1) || band >= keepArr[si])
        return;
    int first, n;
    enc93Band(v, band, &first, &n);
    const float *x = smp[t >> 5] + first;
    const float scaleFactor = static_cast<float>(T.scale[hdr[(static_cast<size_t>(si) * 3 + v) * 16 + band] & 0x3f]);
    // FindBestBandEncoding: every code shares the band's scale, so each sample is scaled once; each code's error sum
    // stays serial in sample order
    float err[15];
    int width[15];
    bool elig[15], pass[15];
#pragma unroll
    for (int c = 1 ; c <= 15 ; ++c)
    {
        err[c - 1] = 0.0f;
        width[c - 1] = c + (v == 0 ? 1 : 0);
        elig[c - 1] = true;
    }
    int s0 = 0, s1 = 0, prv = 0, prvD = 0;
    uint32_t m1 = 0, m2 = 0;
    for (int i = 0 ; i < n ; ++i)
    {
        const float orig = x[i];
        const int s = static_cast<int>(roundf(orig * 32768.0f / scaleFactor));
#pragma unroll
        for (int c = 1 ; c <= 15 ; ++c)
        {
            const int w = width[c - 1];
            const int refVal = 1 << (w - 1);
            const int stored = (s + refVal) & (0xFFFF >> (16 - w));
            const float reconstructed = (static_cast<float>(stored - refVal) * scaleFactor) / 32768.0f;
            const float q = reconstructed - orig;
            err[c - 1] += q * q;
        }
        if (i == 0) s0 = s;
        if (i == 1) s1 = s;
        if (i >= 1)
        {
            const int d = s - prv;
            m1 = max(m1, absI(d));
            if (i >= 2) m2 = max(m2, absI(d - prvD));
            prvD = d;
        }
        prv = s;
    }
    const float errMax = (p.maxQE * p.maxQE) * static_cast<float>(n);
#pragma unroll
    for (int c = 0 ; c < 15 ; ++c)
        pass[c] = err[c] <= errMax;
    rec[(static_cast<size_t>(v) * F + f) * 16 + band] = Enc93Rec{ s0, s1, prv, prvD, encPick(err, width, elig, pass) | (bitLen(m1) << 8) | (bitLen(m2) << 16) };
}

// GetDeltaBandCode from the bit length of max |delta|: bit width = length + 1, code = width - 1 in Type 0, = width in Type 1
__device__ inline int enc93DeltaCode(int typ, uint32_t len) { return len == 0 ? 0 : static_cast<int>(len) + typ; }

// one frame of CompressFrame93b's band loop (:2196-2466); btc = the band-type codes carried from frame to frame (Type 1),
// btCode / btLen = EncTabs' Keep / Invert codebooks, copied to LDS (a global load per band would put a memory latency on
// every step of the Type-1 walk)
template <int TYP>
__device__ inline uint32_t enc93Frame(const uint32_t (*btCode)[32], const uint8_t (*btLen)[32], int keep, const Enc93Rec (&r)[16],
                                      int (&btc)[16], Enc93Band *out)
{
    int lastCode = -1, lastSub = TYP == 1 ? 0 : 2, P = 0, D = 0;
    uint32_t bits = 0;
#pragma unroll
    for (int b = 0 ; b < 16 ; ++b)
    {
        if (b >= keep)
            continue;                           // (not break: the loop stays fully unrolled, r[] and btc[] in registers)
        const Enc93Rec &x = r[b];
        const int old = TYP == 1 ? btc[b] : 0;
        // the sub-type 0 search leaves out code 15 when it is out of the Keep codebook's reach (delta > 14)
        const int c0 = (TYP == 1 && lastSub == 0 && old == 0) ? static_cast<int>((x.pick >> 4) & 15) : static_cast<int>(x.pick & 15);
        const int c1 = enc93DeltaCode(TYP, max(bitLen(absI(x.s0 - P)), (x.pick >> 8) & 0xFF));
        int code = c0, sub = 0;
        // a sub-type 1 candidate the chosen codebook cannot express is not eligible (Keep has no +15 code)
        if ((c1 < code || (c1 == code && lastSub == 1)) && !(TYP == 1 && lastSub == 1 && c1 - old > 14))
        {
            code = c1;
            sub = 1;
        }
        if (TYP == 0)
        {
            const int c2 = enc93DeltaCode(0, max(max(bitLen(absI(x.s0 - P - D)), bitLen(absI(x.s1 - 2 * x.s0 + P))), x.pick >> 16));
            if (c2 < code)
            {
                code = c2;
                sub = 2;
            }
        }
        uint32_t hv, hl, sb = 0;
        const int inP = P, inD = D;
        if (lastCode == 0 && code == 0 && lastSub == sub)
        {
            hv = 1;                             // repeat the zero band; prvSample / prvDelta follow the scaled samples
            hl = 1;
            P = x.sLast;
            D = x.dLast;
        }
        else
        {
            if (TYP == 0)
            {
                const bool keepSub = sub == lastSub;
                hv = keepSub ? static_cast<uint32_t>(code) : (2u | (sub == (lastSub + 1) % 3 ? 1u : 0u)) << 4 | static_cast<uint32_t>(code);
                hl = keepSub ? 5 : 6;
            }
            else
            {
                const int inv = sub != lastSub ? 1 : 0;
                hv = btCode[inv][code - old + 16];
                hl = btLen[inv][code - old + 16];
                btc[b] = code;
            }
            hl += lastCode == 0 ? 1 : 0;          // the 0 bit: not a repeat
            if (code == 0)
            {
                if (sub == 0) { P = 0; D = 0; }
                else if (sub == 1) D = 0;
            }
            else
            {
                sb = static_cast<uint32_t>((b == 0 && TYP == 1 ? 15 : 16) * (code + (TYP == 0 ? 1 : 0)));
                P = x.sLast;
                D = x.dLast;
            }
        }
        out[b] = Enc93Band{ hv, inP, inD, hl | static_cast<uint32_t>(code) << 8 | static_cast<uint32_t>(sub) << 12 | sb << 16 };
        bits += hl + sb;
        lastCode = code;
        lastSub = sub;
    }
    return bits;
}

template <int TYP>
__device__ inline void enc93Load(const Enc93Rec *__restrict__ rec, size_t row, int keep, Enc93Rec (&r)[16])
{
#pragma unroll
    for (int b = 0 ; b < 16 ; ++b)
        if (b < keep)
            r[b] = rec[row + b];
}

// O4: Type 0 (TYP 0): one lane per job-frame.  Type 1: one lane per job that computes Type 1, frame after frame, the next frame's records loaded
// while the current one is walked.  Writes each band's Enc93Band and each frame's bit count.
template <int TYP>
__global__ __launch_bounds__(64) void enc93WalkKernel(const EncTabs *__restrict__ Tp, const EncJob *__restrict__ jobs,
    const EncSet *__restrict__ sets, const uint32_t *__restrict__ frameJob, const int32_t *__restrict__ keepArr, uint32_t F, uint32_t nUnits,
    const Enc93Rec *__restrict__ rec, Enc93Band *__restrict__ out, uint32_t *__restrict__ frameBits)
{
    __shared__ uint32_t btCode[2][32];
    __shared__ uint8_t btLen[2][32];
    btCode[threadIdx.x >> 5][threadIdx.x & 31] = Tp->btCode[threadIdx.x >> 5][threadIdx.x & 31];
    btLen[threadIdx.x >> 5][threadIdx.x & 31] = Tp->btLen[threadIdx.x >> 5][threadIdx.x & 31];
    __syncthreads();
    const uint32_t u = blockIdx.x * 64 + threadIdx.x;
    if (u >= nUnits)
        return;
    Enc93Rec r[16];
    int btc[16];
#pragma unroll
    for (int b = 0 ; b < 16 ; ++b)
        btc[b] = 0;
    if (TYP == 0)
    {
        const uint32_t ji = frameJob[u];
        if (!(sets[jobs[ji].set].vmask & 1))
            return;
        const int keep = keepArr[ji];
        enc93Load<TYP>(rec, static_cast<size_t>(u) * 16, keep, r);
        frameBits[u] = enc93Frame<TYP>(btCode, btLen, keep, r, btc, out + static_cast<size_t>(u) * 16);
        return;
    }
    const EncJob s = jobs[u];
    if (!(sets[s.set].vmask & 2))
        return;
    const int keep = keepArr[u];
    const size_t base = static_cast<size_t>(F) * 16;          // layout 1's rows
    enc93Load<TYP>(rec, base + static_cast<size_t>(s.firstFrame) * 16, keep, r);
    for (uint32_t j = 0 ; j < s.nFrames ; ++j)
    {
        const uint32_t f = s.firstFrame + j;
        Enc93Rec nx[16];
        enc93Load<TYP>(rec, base + static_cast<size_t>(j + 1 < s.nFrames ? f + 1 : f) * 16, keep, nx);
        frameBits[F + f] = enc93Frame<TYP>(btCode, btLen, keep, r, btc, out + base + static_cast<size_t>(f) * 16);
#pragma unroll
        for (int b = 0 ; b < 16 ; ++b)
            r[b] = nx[b];
    }
}

// O5: four job-frames per block, one lane per band: the winner's flag and type bits, then the samples of its band sub-type
__global__ __launch_bounds__(64) void enc93PackKernel(const EncTabs *__restrict__ Tp, const float *__restrict__ spec,
    const uint32_t *__restrict__ frameJob, const EncJob *__restrict__ jobs, const uint8_t *__restrict__ hdr, const int32_t *__restrict__ keepArr,
    const int32_t *__restrict__ win, uint32_t F, const Enc93Band *__restrict__ bands, const uint32_t *__restrict__ frameOff,
    const uint64_t *__restrict__ outOff, uint32_t *__restrict__ W)
{
    const EncTabs &T = *Tp;
    __shared__ float smp[4][256];
    const int l = threadIdx.x;
    for (int q = 0 ; q < 16 ; ++q)
    {
        const int idx = l + 64 * q;
        const uint32_t ff = blockIdx.x * 4 + (idx >> 8);
        smp[idx >> 8][idx & 255] = ff < F ? spec[static_cast<size_t>(encSpecFrame(jobs[frameJob[ff]], ff)) * 256 + (idx & 255)] : 0.0f;
    }
    __syncthreads();
    const uint32_t f = blockIdx.x * 4 + (l >> 4);
    const int band = l & 15;
    if (f >= F)
        return;
    const uint32_t si = frameJob[f];
    if (win[si] < 0 || band >= keepArr[si])                     // (win < 0: an OS93a Type-1 job, packed by enc93aPackKernel)
        return;
    const int v = win[si] < 2 ? 0 : 1;                          // (0,0) -> Type 0, (1,0) -> Type 1
    const size_t row = (static_cast<size_t>(v) * F + f) * 16;
    uint64_t pos = (outOff[si] + 18) * 8 + frameOff[f];
    for (int b = 0 ; b < band ; ++b)
    {
        const uint32_t m = bands[row + b].meta;
        pos += (m & 0xFF) + (m >> 16);
    }
    const Enc93Band x = bands[row + band];
    encPut(W, pos, x.hdr, static_cast<int>(x.meta & 0xFF));
    if ((x.meta >> 16) == 0)
        return;
    pos += x.meta & 0xFF;
    int first, n;
    enc93Band(v, band, &first, &n);
    const float scaleFactor = static_cast<float>(T.scale[hdr[(static_cast<size_t>(si) * 3 + v) * 16 + band] & 0x3f]);
    const int sub = static_cast<int>((x.meta >> 12) & 3);
    const int nBits = static_cast<int>((x.meta >> 8) & 15) + (v == 0 ? 1 : 0);
    const uint32_t mask = (1u << nBits) - 1;
    int prv = x.P, prvD = x.D;
    for (int i = 0 ; i < n ; ++i)
    {
        const int s = static_cast<int>(roundf(smp[l >> 4][first + i] * 32768.0f / scaleFactor));
        const int val = sub == 0 ? s : sub == 1 ? s - prv : s - prv - prvD;
        prvD = s - prv;
        prv = s;
        encPut(W, pos + static_cast<uint64_t>(i) * nBits, static_cast<uint32_t>(val) & mask, nBits);
    }
}

bool paramsValid(const DcsEncodeParams *p, bool os93)
{
    if (p == nullptr || p->streamFormatType < -1 || p->streamFormatType > 1 || p->targetBitRate < 1 || p->targetBitRate > 100000000
        || !isfinite(p->powerBandCutoff) || !isfinite(p->minimumDynamicRange) || !isfinite(p->maximumQuantizationError))
        return false;
    if (!os93)
        return p->formatVersion == 0x9400
            && (p->streamFormatSubType == -1 || p->streamFormatSubType == 0 || p->streamFormatSubType == 3);
    // OS93 has no sub-types: CloseStream forces 0 (:777-782); OS93a Type 1 has no encoder (CompressFrame93a :2485-2531)
    return (p->formatVersion == 0x9301 || p->formatVersion == 0x9302) && p->streamFormatSubType >= -1 && p->streamFormatSubType <= 3
        && !(p->formatVersion == 0x9301 && p->streamFormatType == 1);
}

// the message for a set that paramsValid refuses because it asks for OS93a Type 1 (null: it was refused for another reason)
const char *whyOs93aType1(const DcsEncodeParams *p, bool os93)
{
    return os93 && p != nullptr && p->formatVersion == 0x9301 && p->streamFormatType == 1
        ? "OS93a Type 1 streams cannot be encoded (the reference has no encoder for them); ask for Type 0" : nullptr;
}

const uint32_t kMaxBitsPerFrame = 16 * 23 + 255 * 15;      // every band at its longest header code and widest samples
// OS93, every band at its longest flag and type code and widest samples: Type 1 (1 + 30 bits, 15-bit samples, 15 in
// band 0) = 4 321 bits, more than Type 0 (1 + 2 + 4 bits, 16 x 16-bit samples) = 4 208
const uint32_t kMaxBitsPerFrame93 = 16 * (1 + 30) + (15 + 15 * 16) * 15;

size_t boundOf(uint64_t nSamples, uint32_t bitsPerFrame)
{
    const uint64_t nFrames = (nSamples + 239) / 240;
    if (nFrames == 0 || nFrames > 65535)
        return 0;
    return static_cast<size_t>(18 + (nFrames * bitsPerFrame + 7) / 8);
}

}  // namespace

extern "C" DcsStatus dcs_encode_params_default(DcsEncodeParams *p)
{
    if (p == nullptr)
        return DCS_ERR_INVALID_ARG;
    *p = DcsEncodeParams{ 0x9400, 0, 1, 3, 0.97f, 128000, 10.0f / 32768.0f, 10.0f / 32768.0f };
    return DCS_OK;
}

extern "C" size_t dcs_encode_bound(uint64_t nSamples)
{
    return boundOf(nSamples, kMaxBitsPerFrame);
}

extern "C" size_t dcs_encode93_bound(uint64_t nSamples)
{
    return boundOf(nSamples, kMaxBitsPerFrame93);
}

extern "C" DcsStatus dcs_encode_header(const float *powerSum, const float *lo, const float *hi, const DcsEncodeParams *params,
                                       int formatType, int formatSubType, uint8_t *headerOut, int32_t *bandsToKeepOut, int32_t *bitsPerBandOut)
{
    if (powerSum == nullptr || lo == nullptr || hi == nullptr || headerOut == nullptr || !paramsValid(params, false)
        || (formatType != 0 && formatType != 1) || (formatSubType != 0 && formatSubType != 3))
        return DCS_ERR_INVALID_ARG;
    int bits[16], keep;
    encHeader(encTabs(), powerSum, lo, hi, params->powerBandCutoff, params->targetBitRate, formatType, formatSubType, headerOut, &keep, bits);
    if (bandsToKeepOut != nullptr) *bandsToKeepOut = keep;
    if (bitsPerBandOut != nullptr)
        for (int b = 0 ; b < 16 ; ++b) bitsPerBandOut[b] = bits[b];
    return DCS_OK;
}

extern "C" DcsStatus dcs_encode93_header(const float *powerSum, const float *lo, const float *hi, const DcsEncodeParams *params,
                                         int formatType, uint8_t *headerOut, int32_t *bandsToKeepOut, int32_t *bitsPerBandOut)
{
    if (powerSum == nullptr || lo == nullptr || hi == nullptr || headerOut == nullptr || !paramsValid(params, true)
        || (formatType != 0 && formatType != 1) || (params->formatVersion == 0x9301 && formatType == 1))
        return DCS_ERR_INVALID_ARG;
    int bits[16], keep;
    encHeader(encTabs93(), powerSum, lo, hi, params->powerBandCutoff, params->targetBitRate, formatType, 0, headerOut, &keep, bits);
    if (bandsToKeepOut != nullptr) *bandsToKeepOut = keep;
    if (bitsPerBandOut != nullptr)
        for (int b = 0 ; b < 16 ; ++b) bitsPerBandOut[b] = bits[b];
    return DCS_OK;
}

#define ENCCHK(call)                                                                                 \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            char buf_[256];                                                                          \
            snprintf(buf_, sizeof(buf_), "%s failed: %s", #call, hipGetErrorString(e_));             \
            dcsCtxSetError(ctx, buf_);                                                               \
            return DCS_ERR_HIP;                                                                      \
        }                                                                                            \
    } while (0)

// ------------------------------------------------------------------------ measuring a job's round trip (dcs_sweep.hip.h)

// what the encoder knows of a stream it has sized, enough for the device path's stream table (dcs_sweep.hip.h)
// (head: the third byte of an OS93a Type-1 stream, 1 pp bbbbb; not read of any other)
struct DcsSweepStream { uint32_t nFrames, nBytes; int32_t os, formatType, formatSubType, bandsToKeep; uint32_t head; };
struct DcsSweepDecode;
DcsStatus dcsSweepLayout(const DcsSweepStream *s, uint32_t n, uint64_t *offs, size_t *blobLen, size_t *blobBytes);
DcsStatus dcsSweepDecodeStart(DcsCtx *ctx, const DcsSweepStream *s, uint32_t n, const uint64_t *offs, const uint8_t *dBlob, size_t blobLen,
                              const uint8_t *hostBlob, DcsSweepDecode **out, const int16_t **dPcm, const uint32_t **dErr,
                              const volatile uint32_t **planFlag, const uint32_t **firstFrame);
void dcsSweepDecodeRelease(DcsSweepDecode *d);

namespace {

// the sums of one job (DcsSweepResult's, as the kernel adds them up), and the OR of its frames' decode error words
struct EncMeasure { unsigned long long srcSq, decSq, cross; int32_t peak; uint32_t err; };

const uint32_t kMeasureFrames = 32;         // frames of a job per block of encMeasureKernel
const uint32_t kNotDecoded = 0xFFFFFFFFu;   // firstDec of a job whose stream was not decoded

__device__ inline long long waveSum(long long v)
{
    for (int o = 32 ; o > 0 ; o >>= 1)
        v += __shfl_down(v, o);
    return v;
}

// M1: block (j, y) compares samples [y * 7 680, (y + 1) * 7 680) of job j's source, q = clamp(rint(x * 32768)), with the
// decoded stream 16 samples on (the decoder's overlap; it was decoded for nFrames + 1 frames, so the last 16 exist), and
// ORs the error words of decoded frames [y * 32, (y + 1) * 32).  All sums are integers: any order of adding is exact.
__global__ __launch_bounds__(256) void encMeasureKernel(const float *__restrict__ pcm, const EncStream *__restrict__ streams,
    const EncJob *__restrict__ jobs, const uint32_t *__restrict__ firstDec, const int16_t *__restrict__ dec,
    const uint32_t *__restrict__ decErr, EncMeasure *__restrict__ res)
{
    const EncJob j = jobs[blockIdx.x];
    const EncStream s = streams[j.stream];
    const uint32_t t = threadIdx.x;
    const uint32_t fr = blockIdx.y * kMeasureFrames + t;
    if (firstDec[blockIdx.x] == kNotDecoded)
        return;
    if (t < kMeasureFrames && fr <= j.nFrames && decErr[firstDec[blockIdx.x] + fr] != 0)
        atomicOr(&res[blockIdx.x].err, 1u);
    const uint32_t k0 = blockIdx.y * kMeasureFrames * 240;
    if (k0 >= s.nSamples)
        return;
    const uint32_t k1 = min(k0 + kMeasureFrames * 240, s.nSamples);
    const float *x = pcm + s.sampleOff;
    const int16_t *d = dec + static_cast<size_t>(firstDec[blockIdx.x]) * 240 + 16;
    long long a = 0, b = 0, c = 0;
    int peak = 0;
    for (uint32_t k = k0 + t ; k < k1 ; k += 256)
    {
        int q = static_cast<int>(rintf(x[k] * 32768.0f));
        q = q > 32767 ? 32767 : q < -32768 ? -32768 : q;
        const int y = d[k];
        a += static_cast<long long>(q * q);
        b += static_cast<long long>(y * y);
        c += static_cast<long long>(y * q);
        const int e = y > q ? y - q : q - y;
        peak = e > peak ? e : peak;
    }
    a = waveSum(a); b = waveSum(b); c = waveSum(c);
    for (int o = 32 ; o > 0 ; o >>= 1)
        peak = max(peak, __shfl_down(peak, o));
    if ((t & 63) == 0)
    {
        EncMeasure &r = res[blockIdx.x];
        atomicAdd(&r.srcSq, static_cast<unsigned long long>(a));
        atomicAdd(&r.decSq, static_cast<unsigned long long>(b));
        atomicAdd(&r.cross, static_cast<unsigned long long>(c));      // (two's complement: the signed sum)
        atomicMax(&r.peak, peak);
    }
}

}  // namespace

// ------------------------------------------- OS93a Type 1, the pair-table layout: tables and kernels (dcs_encode93a.hip.h)
// (here: behind every kernel above that is no template, so that those keep their order in the code object, and in front of
// EncRun, which launches these; see the note above EncRun::analyse for the templates)

#include "dcs_encode93a.hip.h"
#include "dcs_encode_rd.h"
#include "dcs_encode93_rd.h"

namespace {

// Where the driver reads its samples: the caller's float PCM on the host (dcs_encode_streams, dcs_encode93_streams), a
// decode batch's int16 PCM and error words, resident on the device (dcs_transcode_streams, dcs_transcode.hip.h), or the
// resampler's float output, resident on the device (dcs_encode_streams_at, dcs_resample.hip.h)
struct EncInput
{
    const uint64_t *sampleOffsets = nullptr;    // stream i = samples [sampleOffsets[i], sampleOffsets[i + 1]) of the one that is set:
    uint32_t nStreams = 0;
    const float *hostPcm = nullptr;
    const float *devFloat = nullptr;
    const int16_t *devPcm = nullptr;        // sampleOffsets[i] a multiple of 240 ...
    const uint32_t *devErr = nullptr;       // ... and its frames' error words at sampleOffsets[i] / 240
    const uint32_t *label = nullptr;        // the number a message gives stream i (null: i)
    const float *bound = nullptr;           // the largest |x| stream i may hold (null: 1; dcs_encode_files, INTEGRATION rule 12)
    const volatile uint32_t *planFlag = nullptr;    // a word the device writes before the PCM is final: not 0 = the PCM is not to be used
    bool unusable = false;                  // (out) planFlag was set: DCS_ERR_BAD_STREAM, and nothing was written
};

// the jobs of a call: job j = (stream list[j].stream, set list[j].paramSet), every set of the one encoder `os93` names.
// A set that asks for (0x9301, Type 1) puts its jobs into the A family (dcs_encode93a.hip.h); only dcs_encode93a_streams
// and dcs_encode93a_sweep let one in.
struct EncJobs
{
    const DcsEncodeParams *sets;
    uint32_t nSets;
    const DcsSweepJob *list;
    uint32_t n;
    bool os93;
    bool rd = false;                        // the R family (dcs_encode_rd.hip.h): every set 0x9400, every job searched to a budget
    const uint32_t *budgetBytes = nullptr;  // rd, rd93: per job, the most bytes its stream may have (null: the sets' targetBitRate)
    bool rd93 = false;                      // the S family (dcs_encode93_rd.hip.h): every set OS93 Type 0, every job searched to a budget
    const struct EncFit *fit = nullptr;     // rd, rd93: the jobs share one budget (dcs_encode_rd_fit.hip.h); budgetBytes is then null
};

// what dcs_encode_rd_fit and dcs_encode93_rd_fit ask of the driver: all jobs' streams together at most totalBytes, job j at
// most capBytes[j] (null: no caps); *info (or null) takes the allocator's record
struct EncFit { uint64_t totalBytes; const uint32_t *capBytes; DcsEncodeRdFitInfo *info; };

// after the sizes are known: the host memory that takes the `total` bytes (stream i at outOffsets[i]), or null for DCS_ERR_CAPACITY
using EncPlace = std::function<uint8_t *(const uint64_t *outOffsets, uint64_t total)>;

// where a call's streams and what is known of them go
struct EncOutput
{
    uint8_t *out = nullptr;                 // the caller's buffer of outCap bytes, where `place` is not given
    size_t outCap = 0;
    uint64_t *outOffsets = nullptr;         // nJobs + 1
    DcsEncodeInfo *info = nullptr;          // nJobs, or null
    const EncPlace *place = nullptr;
    DcsEncode93aInfo *info93a = nullptr;    // nJobs, or null: the Type-1 candidate of a job of the A family, zeros of any other
    DcsEncodeRdInfo *infoRd = nullptr;      // nJobs, or null: what the R family's search chose
};

// what dcs_encode_sweep asks of the driver beyond a list of jobs
struct EncSweep
{
    DcsSweepResult *results = nullptr;
    bool measure = false;
    bool sizesOnly = false;                 // out == NULL && outCap == 0: nothing is packed for the host
};

// most job-frames a group may hold (0: what the memory takes); dcs_encode_sweep_group_frames
std::atomic<uint64_t> gGroupFrames{ 0 };

const int kCandType[4] = { 0, 0, 1, 1 }, kCandSub[4] = { 0, 3, 0, 3 };     // candidates in CloseStream's order (0,0), (0,3), (1,0), (1,3)

#define HIPTRY(call)                                                                                 \
    do {                                                                                             \
        const hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess)                                                                        \
            return e_;                                                                               \
    } while (0)
#define ENCTRY(call)                                                                                 \
    do {                                                                                             \
        const DcsStatus s_ = (call);                                                                 \
        if (s_ != DCS_OK)                                                                            \
            return s_;                                                                               \
    } while (0)

// a decode queued by dcsSweepDecodeStart, released (which waits for the stream) on every way out of its scope
struct SweepDecodeGuard
{
    DcsSweepDecode *d = nullptr;
    ~SweepDecodeGuard() { dcsSweepDecodeRelease(d); }
};

// The one host driver behind every encode, as an object that lives for one call.  A job is (stream, parameter set);
// dcs_encode_streams and its kin are one job per stream with one set.  run() strings the steps together, each a member
// function below, in this order:
//   checkStreams   the streams' lengths, before anything is written; then the empty call's zeros, before any HIP call
//   buildSets      the parameter sets as the kernels read them, and which layouts any of them asks for
//   allocCall      the buffers that live as long as the call (CallBufs)
//   allocGroups    the jobs in groups, runs of the job list whose per-job-frame buffers (GroupBufs, sized for the largest
//                  group) fit the memory: makeGroups + allocGroup, one group unless a cap is set or an allocation fails
//   analyse        upload, E1 and the sums of E2, once per stream; where the call has jobs of the A family, A1: the search
//                  once per stream-frame and its walk once per distinct maximumQuantizationError (buildSets: setQ, rowOf)
//   runGroup       per group: the header half of E2, the families' band stages (O or E on the jobs whose set has a layout
//                  of theirs, A2 on the Type-1 jobs) and the sizes, and a wait, after which win, keep and size of its jobs
//                  are on the host.  After the first group's wait, checkInput: planFlag, then bad[]
//   fitAllot       (a fit call only, dcs_encode_rd_fit.hip.h) once every group has run and left its jobs' candidates in the call's
//                  curve table: the allocator over all jobs; the allotments become the jobs' budgets and sizes.  Each group
//                  then chooses again before it is packed: fitRechoose where it is still resident (a call of one group runs
//                  its trellises once), runGroup where it is not; fitReport checks the sizes and writes info and infoRd
//   placeOutput    once every size is known: outOffsets, info, results, and the memory the bytes go to (the capacity check)
//   packGroup      per group again (one that is no longer resident is first computed again by runGroup): layout, header,
//                  pack (for the Type-1 jobs A3, A4, their head and A5) and swap into the group's blob on the device; then
//                  one of
//   deliverGroup   the blob to its place in the output, or with sweep.measure
//   measureGroup   the group's streams decoded where the pack step left them and compared with their sources (M1), the
//                  blob staged on the host when the decode or the output needs it there (stageBlob)
// Three lifetimes of device memory: `call`, `group` (emptied when an allocation attempt fails) and `blob` (taken anew for
// every group).  The destructor waits for the stream once and gives back blob, group, call, in that order.
class EncRun
{
public:
    EncRun(DcsCtx *ctx, EncInput &in, const EncJobs &jobs, const EncOutput &to, const EncSweep &sweep)
        : ctx(ctx), st(dcsCtxStream(ctx)), in(in), jobs(jobs), to(to), sweep(sweep), dev(in.devPcm != nullptr),
          devF(in.devFloat != nullptr), call(ctx), group(ctx), blob(ctx) {}
    ~EncRun()
    {
        if (!call.empty())
            call.wait();
        blob.clear();
        group.clear();
        call.clear();
    }
    DcsStatus run();

private:
    DcsStatus checkStreams();
    void buildSets();
    DcsStatus allocCall();
    void makeGroups(uint64_t limit);
    hipError_t allocGroup();
    DcsStatus allocGroups();
    DcsStatus analyse();
    DcsStatus runGroup(uint32_t g);
    DcsStatus checkInput();
    DcsStatus placeOutput();
    DcsStatus layoutGroup(uint32_t g, size_t *nWords);
    DcsStatus packGroup(uint32_t g);
    DcsStatus deliverGroup(uint32_t g);
    DcsStatus stageBlob();
    void selectDecodes(uint32_t n);
    DcsStatus decodeAndCompare(uint32_t n, bool onHost, bool *unusable);
    DcsStatus reportGroup(uint32_t g);
    DcsStatus measureGroup(uint32_t g);
    // the R family's share of allocCall, allocGroup, analyse, runGroup and packGroup (defined behind dcs_encode_rd.hip.h)
    DcsStatus rdAllocCall();
    hipError_t rdAllocGroup();
    DcsStatus rdAnalyse();
    DcsStatus rdRunGroup(uint32_t j0, uint32_t n);
    DcsStatus rdPackGroup(uint32_t n, uint32_t JF);
    // the S family's share of the same steps (defined behind dcs_encode93_rd.hip.h)
    DcsStatus rd93AllocCall();
    hipError_t rd93AllocGroup();
    DcsStatus rd93Analyse();
    DcsStatus rd93RunGroup(uint32_t j0, uint32_t n, uint32_t JF);
    DcsStatus rd93PackGroup(uint32_t n, uint32_t JF);
    void budgetsRd();
    void sizesRd(uint32_t j0, uint32_t n);
    void writeInfo(uint32_t j);
    // a fit call's own steps (defined behind dcs_encode_rd_fit.hip.h)
    DcsStatus fitAllocCall();
    DcsStatus fitCurves(uint32_t j0, uint32_t n);
    DcsStatus fitAllot();
    DcsStatus fitRechoose(uint32_t g);
    DcsStatus fitReport(uint32_t g);
    void fitRecord();
    std::string name(uint32_t i) const { return "stream " + std::to_string(in.label ? in.label[i] : i); }

    // ---- fixed by the arguments
    DcsCtx *const ctx;
    const hipStream_t st;
    EncInput &in;
    const EncJobs jobs;
    const EncOutput to;
    const EncSweep sweep;
    const bool dev, devF;                       // the input is a decode batch's int16 PCM / float PCM on the device
    std::vector<EncStream> hs;                  // (checkStreams)
    std::vector<uint32_t> frameStream;
    uint32_t F = 0;                             // frames of all streams
    std::vector<EncSet> hsets;                  // (buildSets)
    uint32_t anyV = 0;                          // the layouts any set asks for: bit 0 Type 0, bit 1 (1, 0), bit 2 (1, 3);
                                                // 0: every job is of the A family, and no O or E stage is launched
    uint64_t allFrames = 0, largest = 0;        // job-frames of all jobs, of the largest job
    // the A family (OS93a Type 1): the distinct maximumQuantizationError values of its sets, each set's index among them
    // (kA93None: a set of the O family), and per (q, stream) that a job names its row of A1's totals (kA93None: none does)
    std::vector<float> qs;
    std::vector<uint32_t> setQ, rowOf;
    uint32_t nRows = 0;
    std::vector<unsigned long long> floorE;     // [q][18] (analyse; the source of an asynchronous upload)
    // the R family: E_b per set, and per job its budget in frame bits (-1: nothing fits) and what R3 chose
    std::vector<unsigned long long> floorRd;    // [set][16]
    std::vector<long long> budgetRd;
    std::vector<EncRdChoice> choiceRd;
    // the S family: E_b per set (floorRd, one value a set: every band has sixteen samples), budgetRd, and what S5 chose
    std::vector<Enc93RdChoice> choiceRd93;
    // a fit call: the allotments in bytes (empty until fitAllot has run) and the allocator's record
    std::vector<uint32_t> allot;
    DcsEncodeRdFitInfo fitRec{};

    // ---- device buffers of the call: valid from allocCall to the end
    struct CallBufs
    {
        EncTabs *dT;
        float *dPcm = nullptr;                  // the host's PCM uploaded (null where the input is on the device)
        EncStream *dStr;
        EncSet *dSets;
        uint32_t *dFS;                          // frame -> stream
        float *dSpec, *dPw, *dLo, *dHi;         // E1's output per frame
        uint32_t *dBad;                         // per stream: a sample E1 refused
        float *dSums;                           // E2's sums per stream
        struct                                  // the A family only (A1)
        {
            Enc93aTabs *dA = nullptr;
            unsigned long long *dFloorE = nullptr;      // [q][18]
            uint32_t *dSetQ = nullptr, *dRowOf = nullptr;
            Enc93aTot *dTot = nullptr;          // [row][candidate]
        } a93;
        struct                                  // the R family only (R1)
        {
            EncRdTabs *dR = nullptr;
            unsigned long long *dItems = nullptr;       // [stream-frame][band][width][scale code]
            uint32_t *dPeak = nullptr;          // [stream][band]
            unsigned long long *dD0 = nullptr, *dFloor = nullptr;   // [stream][band], [set][band]
        } rd;
        struct                                  // the S family only (S1)
        {
            EncRdTabs *dR = nullptr;
            unsigned long long *dItems = nullptr;       // [stream-frame][band][scale code][option]
            Enc93RdRec *dRecs = nullptr;        // [stream-frame][band][scale code]
            unsigned long long *dD0 = nullptr, *dFloor = nullptr;   // [stream][band], [set]
        } r93;
        struct                                  // a fit call only (F1-F4)
        {
            unsigned long long *dCurveSize = nullptr, *dCurveD = nullptr;   // [job][kFitMaxPoints]: every job's candidates
            unsigned long long *dOff = nullptr; // [job + 1]
            uint32_t *dCap = nullptr, *dAllot = nullptr;
            DcsEncodeRdFitInfo *dFit = nullptr;
        } fit;
    } cb;
    CacheArena call;

    // ---- device buffers of a group, sized for the largest one: valid from allocGroups to the end, their CONTENT that of
    // the resident group (runGroup), dOutOff of the group packed last
    struct GroupBufs
    {
        EncJob *dJobs;
        uint32_t *dFJ;                          // job-frame -> job of the group
        uint8_t *dHdr;
        int32_t *dKeep, *dWin;
        uint64_t *dSize, *dOutOff;
        uint32_t *dFrameBits, *dFrameOff;
        struct { Enc93Rec *dRec = nullptr; Enc93Band *dBand = nullptr; } o93;                       // OS93 only (O3-O5)
        struct { uint8_t *dBest = nullptr, *dCodes = nullptr, *dHdrBits = nullptr; uint16_t *dSmpBits = nullptr; } v94;   // 1994+ only (E3-E5)
        struct { Enc93aChoice *dChoice = nullptr; Enc93aRec *dRec = nullptr; } a93;                 // OS93a Type 1 only (A2-A5)
        struct { EncMeasure *dMeas = nullptr; uint32_t *dFirstDec = nullptr; } m;                   // sweep.measure only (M1)
        struct                                                                                      // the R family only (R2-R6)
        {
            EncRdTot *dTot = nullptr;           // [job][layout][band][window index][lambda]
            EncRdChoice *dChoice = nullptr;
            long long *dBudget = nullptr;
            uint8_t *dSurv = nullptr, *dEnd = nullptr, *dCodes = nullptr;   // [job-frame][band][state], [job][band], [job-frame][band]
            uint32_t *dBits = nullptr;          // [job-frame]
        } rd;
        struct                                                                                      // the S family only (S2-S8)
        {
            unsigned long long *dProxyJ = nullptr;      // [job][band][scale code][lambda]
            uint32_t *dProxyB = nullptr;
            Enc93RdHead *dHead = nullptr;       // [job][lambda]
            Enc93RdTot *dTot = nullptr;         // [job][lambda]
            Enc93RdChoice *dChoice = nullptr;
            long long *dBudget = nullptr;
            uint8_t *dCodes = nullptr;          // [job-frame][band]: the band's state
            uint32_t *dBits = nullptr;          // [job-frame]
        } r93;
    } gb;
    CacheArena group;

    // ---- the groups, and what is known of every job once its group has run
    std::vector<uint32_t> groupFirst;           // group g = jobs [groupFirst[g], groupFirst[g + 1])
    uint64_t groupFrames = 0;                   // the largest group's job-frames ...
    uint32_t groupJobs = 0;                     // ... and the most jobs in a group
    uint32_t resident = ~0u, residentFrames = 0;    // the group whose rows the group buffers hold, and its job-frames
    std::vector<EncJob> hj;                     // the resident group's jobs ...
    std::vector<uint32_t> frameJob;             // ... and rows
    std::vector<int32_t> win, keep;             // per job (runGroup)
    std::vector<uint64_t> size;
    std::vector<Enc93aChoice> choiceA;          // per job of the A family (runGroup)
    std::vector<uint32_t> bad;                  // per stream, on the host after the first group's wait
    uint8_t *dst = nullptr;                     // where the bytes go (placeOutput); null: nowhere

    // ---- the packed group: valid from packGroup to the next one
    CacheArena blob;
    uint32_t *dW = nullptr;                     // the blob, big-endian after the swap
    size_t blobLen = 0;
    std::vector<uint64_t> offs;                 // job k of the group at blob byte offs[k]
    std::vector<DcsSweepStream> ss;             // (sweep.measure) what the decoder is told of each
    std::vector<uint8_t> stage;                 // the blob on the host ...
    bool staged = false;                        // ... once stageBlob has run for this group

    // ---- measureGroup's own
    std::vector<uint32_t> sel, firstDec;        // the jobs of the group that are decoded; per job its first decoded frame
    std::vector<DcsSweepStream> selS;
    std::vector<uint64_t> selOff;
    uint32_t mostFrames = 0;                    // of the selected jobs: the longest ...
    uint64_t selFrames = 0;                     // ... and all of them
    std::vector<EncMeasure> meas;
};

DcsStatus EncRun::checkStreams()
{
    hs.resize(in.nStreams);
    for (uint32_t i = 0 ; i < in.nStreams ; ++i)
    {
        const uint64_t *so = in.sampleOffsets;
        if (so[i + 1] <= so[i])
        {
            dcsCtxSetError(ctx, (name(i) + ": empty").c_str());
            return DCS_ERR_INVALID_ARG;
        }
        const uint64_t n = so[i + 1] - so[i];
        const uint64_t nF = (n + 239) / 240;
        if (nF > 65535)
        {
            dcsCtxSetError(ctx, (name(i) + ": more than 65 535 frames").c_str());
            return DCS_ERR_INVALID_ARG;
        }
        if (sweep.measure && nF == 65535)
        {
            dcsCtxSetError(ctx, (name(i) + ": 65 535 frames; measured with the extra frame its decode would need 65 536, more than the frame count holds").c_str());
            return DCS_ERR_INVALID_ARG;
        }
        hs[i] = EncStream{ so[i] - so[0], static_cast<uint32_t>(n), F, static_cast<uint32_t>(nF),
                           dev ? static_cast<uint32_t>(so[i] / 240) : 0u, in.bound != nullptr ? in.bound[i] : 1.0f };
        frameStream.insert(frameStream.end(), static_cast<size_t>(nF), i);
        F += static_cast<uint32_t>(nF);
    }
    return DCS_OK;
}

void EncRun::buildSets()
{
    hsets.resize(jobs.nSets);
    for (uint32_t k = 0 ; k < jobs.nSets ; ++k)
    {
        const DcsEncodeParams &p = jobs.sets[k];
        const int typ = p.streamFormatType, sub = jobs.os93 ? 0 : p.streamFormatSubType;
        uint32_t cmask = 0;
        for (int c = 0 ; c < 4 ; ++c)
            if ((typ < 0 || typ == kCandType[c]) && (sub < 0 || sub == kCandSub[c])
                && !(jobs.os93 && p.formatVersion == 0x9301 && kCandType[c] == 1))
                cmask |= 1u << c;
        const uint32_t vmask = ((cmask & 3) ? 1u : 0u) | ((cmask & 4) ? 2u : 0u) | ((cmask & 8) ? 4u : 0u);
        hsets[k] = EncSet{ p.powerBandCutoff, p.minimumDynamicRange, p.maximumQuantizationError, p.targetBitRate, vmask, cmask };
        if (!jobs.rd && !jobs.rd93)
            anyV |= vmask;                      // (a set of the R or S family: no E or O stage touches its jobs)
    }
    // the A family's sets (cmask 0 above: no O stage touches their jobs) by their distinct maximumQuantizationError
    setQ.assign(jobs.nSets, kA93None);
    for (uint32_t k = 0 ; jobs.os93 && k < jobs.nSets ; ++k)
        if (isType1Of93a(jobs.sets[k]))
        {
            const float q = jobs.sets[k].maximumQuantizationError;
            const size_t at = std::find(qs.begin(), qs.end(), q) - qs.begin();
            if (at == qs.size())
                qs.push_back(q);
            setQ[k] = static_cast<uint32_t>(at);
        }
    rowOf.assign(qs.size() * in.nStreams, kA93None);
    for (uint32_t j = 0 ; j < jobs.n ; ++j)
    {
        const DcsSweepJob &job = jobs.list[j];
        const uint64_t nF = hs[job.stream].nFrames;
        allFrames += nF;
        largest = nF > largest ? nF : largest;
        if (setQ[job.paramSet] != kA93None)
        {
            uint32_t &row = rowOf[static_cast<size_t>(setQ[job.paramSet]) * in.nStreams + job.stream];
            if (row == kA93None)
                row = nRows++;
        }
    }
}

DcsStatus EncRun::allocCall()
{
    const uint32_t nStreams = in.nStreams;
    ENCCHK(call.alloc(&cb.dT, 1));
    if (!dev && !devF)
        ENCCHK(call.alloc(&cb.dPcm, in.sampleOffsets[nStreams] - in.sampleOffsets[0]));
    ENCCHK(call.alloc(&cb.dStr, nStreams));
    ENCCHK(call.alloc(&cb.dSets, jobs.nSets));
    ENCCHK(call.alloc(&cb.dFS, F));
    ENCCHK(call.alloc(&cb.dSpec, size_t(256) * F));
    ENCCHK(call.alloc(&cb.dPw, size_t(16) * F));
    ENCCHK(call.alloc(&cb.dLo, size_t(16) * F));
    ENCCHK(call.alloc(&cb.dHi, size_t(16) * F));
    ENCCHK(call.alloc(&cb.dBad, nStreams));
    ENCCHK(call.alloc(&cb.dSums, size_t(48) * nStreams));
    if (!qs.empty())
    {
        ENCCHK(call.alloc(&cb.a93.dA, 1));
        ENCCHK(call.alloc(&cb.a93.dFloorE, 18 * qs.size()));
        ENCCHK(call.alloc(&cb.a93.dSetQ, jobs.nSets));
        ENCCHK(call.alloc(&cb.a93.dRowOf, rowOf.size()));
        ENCCHK(call.alloc(&cb.a93.dTot, size_t(kA93Cand) * nRows));
    }
    if (jobs.rd)
        ENCTRY(rdAllocCall());
    if (jobs.rd93)
        ENCTRY(rd93AllocCall());
    if (jobs.fit != nullptr)
        ENCTRY(fitAllocCall());
    return DCS_OK;
}

// the groups: runs of the job list of at most `limit` job-frames, a job never split
void EncRun::makeGroups(uint64_t limit)
{
    groupFirst.assign(1, 0);
    groupFrames = 0; groupJobs = 0;
    uint64_t inGroup = 0;
    for (uint32_t j = 0 ; j < jobs.n ; ++j)
    {
        const uint64_t nF = hs[jobs.list[j].stream].nFrames;
        if ((inGroup != 0 && inGroup + nF > limit) || inGroup + nF > 0xFFFFFFFFull)
        {
            groupFirst.push_back(j);
            inGroup = 0;
        }
        inGroup += nF;
        groupFrames = inGroup > groupFrames ? inGroup : groupFrames;
        groupJobs = std::max(groupJobs, j + 1 - groupFirst.back());
    }
    groupFirst.push_back(jobs.n);
}

// every buffer of a group, sized for the largest one; the first failure is returned, for allocGroups to judge
hipError_t EncRun::allocGroup()
{
    const size_t JF = static_cast<size_t>(groupFrames), NJ = groupJobs;
    HIPTRY(group.alloc(&gb.dJobs, NJ));
    HIPTRY(group.alloc(&gb.dFJ, JF));
    HIPTRY(group.alloc(&gb.dHdr, 48 * NJ));
    HIPTRY(group.alloc(&gb.dKeep, NJ));
    HIPTRY(group.alloc(&gb.dWin, NJ));
    HIPTRY(group.alloc(&gb.dSize, NJ));
    HIPTRY(group.alloc(&gb.dOutOff, NJ));
    if (anyV != 0)
        HIPTRY(group.alloc(&gb.dFrameBits, 3 * JF));
    HIPTRY(group.alloc(&gb.dFrameOff, JF));
    if (anyV != 0 && jobs.os93)
    {
        HIPTRY(group.alloc(&gb.o93.dRec, 32 * JF));
        HIPTRY(group.alloc(&gb.o93.dBand, 32 * JF));
    }
    if (anyV != 0 && !jobs.os93)
    {
        HIPTRY(group.alloc(&gb.v94.dBest, 128 * JF));
        HIPTRY(group.alloc(&gb.v94.dCodes, 48 * JF));
        HIPTRY(group.alloc(&gb.v94.dHdrBits, 48 * JF));
        HIPTRY(group.alloc(&gb.v94.dSmpBits, 48 * JF));
    }
    if (!qs.empty())
    {
        HIPTRY(group.alloc(&gb.a93.dChoice, NJ));
        HIPTRY(group.alloc(&gb.a93.dRec, JF));
    }
    if (sweep.measure)
    {
        HIPTRY(group.alloc(&gb.m.dMeas, NJ));
        HIPTRY(group.alloc(&gb.m.dFirstDec, NJ));
    }
    if (jobs.rd)
        HIPTRY(rdAllocGroup());
    if (jobs.rd93)
        HIPTRY(rd93AllocGroup());
    return hipSuccess;
}

// all jobs in one group when that can be had (or the cap that is set); half the job-frames each time the memory runs out
DcsStatus EncRun::allocGroups()
{
    uint64_t limit = gGroupFrames.load() != 0 ? std::max<uint64_t>(gGroupFrames.load(), largest) : allFrames;
    for (;;)
    {
        makeGroups(limit);
        const hipError_t e = allocGroup();
        if (e == hipSuccess)
            return DCS_OK;
        group.clear();
        if (e != hipErrorOutOfMemory || groupFrames <= largest)
            ENCCHK(e);
        limit = std::max<uint64_t>(largest, groupFrames / 2);
    }
}

// E2's header half to the sizes for group g, and a wait: win, keep and size of its jobs are on the host after it
DcsStatus EncRun::runGroup(uint32_t g)
{
    const uint32_t j0 = groupFirst[g], n = groupFirst[g + 1] - j0;
    hj.resize(n);
    frameJob.clear();
    uint32_t JF = 0;
    for (uint32_t k = 0 ; k < n ; ++k)
    {
        const DcsSweepJob &job = jobs.list[j0 + k];
        const EncStream &s = hs[job.stream];
        hj[k] = EncJob{ job.stream, job.paramSet, JF, s.nFrames, s.firstFrame };
        frameJob.insert(frameJob.end(), s.nFrames, k);
        JF += s.nFrames;
    }
    ENCCHK(hipMemcpyAsync(gb.dJobs, hj.data(), sizeof(EncJob) * n, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(gb.dFJ, frameJob.data(), sizeof(uint32_t) * JF, hipMemcpyHostToDevice, st));
    if (anyV != 0)
    {
        ENCCHK(hipMemsetAsync(gb.dFrameBits, 0, sizeof(uint32_t) * 3 * JF, st));
        hipLaunchKernelGGL(encHeaderKernel, dim3(n), dim3(64), 0, st, cb.dT, gb.dJobs, cb.dSets, cb.dSums, gb.dHdr, gb.dKeep);
    }
    if (anyV != 0 && jobs.os93)
    {
        hipLaunchKernelGGL(enc93SearchKernel, dim3((JF + 3) / 4), dim3(128), 0, st, cb.dT, cb.dSpec, gb.dFJ, gb.dJobs, cb.dSets, gb.dHdr,
                           gb.dKeep, JF, gb.o93.dRec);
        if (anyV & 1)
            hipLaunchKernelGGL(enc93WalkKernel<0>, dim3((JF + 63) / 64), dim3(64), 0, st, cb.dT, gb.dJobs, cb.dSets, gb.dFJ, gb.dKeep, JF, JF,
                               gb.o93.dRec, gb.o93.dBand, gb.dFrameBits);
        if (anyV & 2)
            hipLaunchKernelGGL(enc93WalkKernel<1>, dim3((n + 63) / 64), dim3(64), 0, st, cb.dT, gb.dJobs, cb.dSets, gb.dFJ, gb.dKeep, JF, n,
                               gb.o93.dRec, gb.o93.dBand, gb.dFrameBits);
    }
    if (anyV != 0 && !jobs.os93)
    {
        ENCCHK(hipMemsetAsync(gb.v94.dBest, 0, size_t(128) * JF, st));
        ENCCHK(hipMemsetAsync(gb.v94.dCodes, 0, size_t(48) * JF, st));
        hipLaunchKernelGGL(encSearchKernel, dim3(JF), dim3(128), 0, st, cb.dT, cb.dSpec, cb.dLo, cb.dHi, gb.dFJ, gb.dJobs, cb.dSets, gb.dHdr,
                           gb.dKeep, gb.v94.dBest);
        hipLaunchKernelGGL(encChainKernel, dim3(n), dim3(64), 0, st, cb.dT, gb.dJobs, cb.dSets, gb.dKeep, JF,
                           reinterpret_cast<const uint64_t *>(gb.v94.dBest), gb.v94.dCodes);
        hipLaunchKernelGGL(encBitsKernel, dim3(JF), dim3(64), 0, st, cb.dT, cb.dSpec, gb.dFJ, gb.dJobs, cb.dSets, gb.dHdr, gb.dKeep, JF,
                           gb.v94.dCodes, gb.v94.dHdrBits, gb.v94.dSmpBits, gb.dFrameBits);
    }
    // (a job of the A family has no layout here, cmask 0: encSizeKernel leaves its win at -1, which the head and pack
    // kernels of this family pass over)
    if (anyV != 0)
        hipLaunchKernelGGL(encSizeKernel, dim3(n), dim3(256), 0, st, gb.dJobs, cb.dSets, JF, gb.dFrameBits, gb.dWin, gb.dSize, gb.dFrameOff);
    if (!qs.empty())
        hipLaunchKernelGGL(enc93aChooseKernel, dim3(n), dim3(256), 0, st, cb.a93.dTot, cb.a93.dRowOf, in.nStreams, gb.dJobs, cb.dSets,
                           cb.a93.dSetQ, gb.a93.dChoice);
    if (jobs.rd)
        ENCTRY(rdRunGroup(j0, n));
    if (jobs.rd93)
        ENCTRY(rd93RunGroup(j0, n, JF));
    if (jobs.fit != nullptr && allot.empty())
        ENCTRY(fitCurves(j0, n));
    ENCCHK(hipGetLastError());
    if (anyV != 0)
    {
        ENCCHK(hipMemcpyAsync(win.data() + j0, gb.dWin, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        ENCCHK(hipMemcpyAsync(keep.data() + j0, gb.dKeep, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        ENCCHK(hipMemcpyAsync(size.data() + j0, gb.dSize, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, st));
    }
    if (!qs.empty())
        ENCCHK(hipMemcpyAsync(choiceA.data() + j0, gb.a93.dChoice, sizeof(Enc93aChoice) * n, hipMemcpyDeviceToHost, st));
    ENCCHK(hipStreamSynchronize(st));
    // a Type-1 job: the candidate (1, 0) of CloseStream's list, its header's band count, 3 header bytes and the frames' bits
    for (uint32_t k = 0 ; k < n ; ++k)
        if (setQ[hj[k].set] != kA93None)
        {
            win[j0 + k] = 2;
            keep[j0 + k] = choiceA[j0 + k].numBands;
            size[j0 + k] = 3 + (choiceA[j0 + k].frameBits + 7) / 8;
        }
    sizesRd(j0, n);
    resident = g;
    residentFrames = JF;
    return DCS_OK;
}

// win, keep and size of n jobs from job j0 from what the R or the S family chose for them
void EncRun::sizesRd(uint32_t j0, uint32_t n)
{
    // a job of the R family: the candidate of CloseStream's list it chose, its header's band count, 18 bytes and the frames' bits
    for (uint32_t k = 0 ; jobs.rd && k < n ; ++k)
    {
        win[j0 + k] = choiceRd[j0 + k].variant;
        keep[j0 + k] = choiceRd[j0 + k].numBands;
        size[j0 + k] = 18 + (choiceRd[j0 + k].frameBits + 7) / 8;
    }
    // a job of the S family: Type 0, its header's band count, 18 bytes and the frames' bits
    for (uint32_t k = 0 ; jobs.rd93 && k < n ; ++k)
    {
        win[j0 + k] = 0;
        keep[j0 + k] = choiceRd93[j0 + k].numBands;
        size[j0 + k] = 18 + (choiceRd93[j0 + k].frameBits + 7) / 8;
    }
}

// Upload, E1 and encStreamKernel; bad[] is on its way to the host, there after the first group's wait; then A1 for the
// streams that jobs of the A family name.  (The step before runGroup, written after it: the kernel templates are
// instantiated in the order the source first launches them, and the device code object keeps the order it had.  The A
// family's two, enc93aFrameKernel<false> here and <true> in packGroup, follow E1's and precede the resampler's.)
DcsStatus EncRun::analyse()
{
    const uint32_t nStreams = in.nStreams;
    const uint64_t first = in.sampleOffsets[0], nSamples = in.sampleOffsets[nStreams] - first;
    const EncTabs &tabs = jobs.os93 ? encTabs93() : encTabs();
    bad.resize(nStreams);
    ENCCHK(hipMemcpyAsync(cb.dT, &tabs, sizeof(EncTabs), hipMemcpyHostToDevice, st));
    if (!dev && !devF)
        ENCCHK(hipMemcpyAsync(cb.dPcm, in.hostPcm + first, sizeof(float) * nSamples, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(cb.dStr, hs.data(), sizeof(EncStream) * nStreams, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(cb.dSets, hsets.data(), sizeof(EncSet) * jobs.nSets, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(cb.dFS, frameStream.data(), sizeof(uint32_t) * F, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemsetAsync(cb.dBad, 0, sizeof(uint32_t) * nStreams, st));
    if (dev)
        hipLaunchKernelGGL(encAnalyseKernel<int16_t>, dim3((F + 3) / 4), dim3(256), 0, st, cb.dT, in.devPcm + first, cb.dStr, cb.dFS, F,
                           cb.dSpec, cb.dPw, cb.dLo, cb.dHi, cb.dBad, in.devErr);
    else
        hipLaunchKernelGGL(encAnalyseKernel<float>, dim3((F + 3) / 4), dim3(256), 0, st, cb.dT, devF ? in.devFloat + first : cb.dPcm,
                           cb.dStr, cb.dFS, F, cb.dSpec, cb.dPw, cb.dLo, cb.dHi, cb.dBad, static_cast<const uint32_t *>(nullptr));
    if (anyV != 0)
        hipLaunchKernelGGL(encStreamKernel, dim3(nStreams), dim3(64), 0, st, cb.dStr, cb.dPw, cb.dLo, cb.dHi, cb.dSums);
    ENCCHK(hipMemcpyAsync(bad.data(), cb.dBad, sizeof(uint32_t) * nStreams, hipMemcpyDeviceToHost, st));
    if (jobs.rd)
        return rdAnalyse();
    if (jobs.rd93)
        return rd93Analyse();
    if (qs.empty())
        return DCS_OK;
    // A1: one search per stream-frame; kA93QPerLaunch of the distinct q to a launch
    const uint32_t nQ = static_cast<uint32_t>(qs.size());
    floorE.resize(size_t(18) * nQ);
    for (uint32_t k = 0 ; k < nQ ; ++k)
        floorE93a(qs[k], floorE.data() + size_t(18) * k);
    ENCCHK(hipMemcpyAsync(cb.a93.dA, &encTabs93a(), sizeof(Enc93aTabs), hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(cb.a93.dFloorE, floorE.data(), sizeof(unsigned long long) * floorE.size(), hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(cb.a93.dSetQ, setQ.data(), sizeof(uint32_t) * jobs.nSets, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(cb.a93.dRowOf, rowOf.data(), sizeof(uint32_t) * rowOf.size(), hipMemcpyHostToDevice, st));
    ENCCHK(hipMemsetAsync(cb.a93.dTot, 0, sizeof(Enc93aTot) * kA93Cand * nRows, st));
    for (uint32_t q0 = 0 ; q0 < nQ ; q0 += kA93QPerLaunch)
        hipLaunchKernelGGL(enc93aFrameKernel<false>, dim3(F), dim3(256), 0, st, cb.a93.dA, cb.a93.dFloorE, cb.dSpec, cb.dFS, cb.a93.dRowOf,
                           nStreams, q0, std::min(kA93QPerLaunch, nQ - q0), cb.a93.dTot, static_cast<const EncJob *>(nullptr),
                           static_cast<const uint32_t *>(nullptr), static_cast<const Enc93aChoice *>(nullptr), static_cast<Enc93aRec *>(nullptr));
    return DCS_OK;
}

// what the first wait brings: was the input usable at all (planFlag), then did E1 refuse a sample (bad[])
DcsStatus EncRun::checkInput()
{
    if (in.planFlag != nullptr && *in.planFlag != 0)
    {
        in.unusable = true;
        return DCS_ERR_BAD_STREAM;
    }
    for (uint32_t i = 0 ; i < in.nStreams ; ++i)
        if (bad[i])
        {
            dcsCtxSetError(ctx, (name(i) + (dev ? ": the decoder reports an error in a frame (DCS_FRAME_STOP / DCS_FRAME_FATAL)"
                                                : in.bound != nullptr ? ": a sample is not finite or beyond its format's full scale"
                                                : ": a sample is not finite or |x| > 1")).c_str());
            return DCS_ERR_BAD_STREAM;
        }
    return DCS_OK;
}

// info, info93a, infoRd and the sweep's result of job j, from what its group's run left on the host
void EncRun::writeInfo(uint32_t j)
{
    const DcsEncodeInfo e{ kCandType[win[j]], kCandSub[win[j]], static_cast<int32_t>(hs[jobs.list[j].stream].nFrames),
                           static_cast<int32_t>(size[j]), keep[j] };
    if (to.info != nullptr)
        to.info[j] = e;
    if (to.info93a != nullptr)
    {
        const DcsEncodeParams &p = jobs.sets[jobs.list[j].paramSet];
        const Enc93aChoice &c = choiceA[j];
        const uint64_t budget = static_cast<uint64_t>(p.targetBitRate) * static_cast<uint64_t>(e.nFrames) * 240ull / 31250ull;
        to.info93a[j] = setQ[jobs.list[j].paramSet] == kA93None ? DcsEncode93aInfo{}
                        : DcsEncode93aInfo{ c.selector, c.ladderIndex, c.numBands, 0, c.frameBits, budget, c.sumD };
    }
    if (to.infoRd != nullptr && jobs.rd93)
    {
        const Enc93RdChoice &c = choiceRd93[j];
        to.infoRd[j] = DcsEncodeRdInfo{ 0, 0, c.ladderIndex, c.numBands, c.frameBits,
                                        static_cast<uint64_t>(std::max<long long>(budgetRd[j], 0)), c.sumD, c.fits, 0 };
    }
    else if (to.infoRd != nullptr)
    {
        const EncRdChoice &c = choiceRd[j];
        to.infoRd[j] = DcsEncodeRdInfo{ kCandType[c.variant], kCandSub[c.variant], c.ladderIndex, c.numBands, c.frameBits,
                                        static_cast<uint64_t>(std::max<long long>(budgetRd[j], 0)), c.sumD, c.fits, 0 };
    }
    if (sweep.results != nullptr)
    {
        memset(&sweep.results[j], 0, sizeof(DcsSweepResult));       // (its padding too: records compare as bytes)
        sweep.results[j].enc = e;
    }
}

// every size is known: outOffsets, info and results, then dst (null with DCS_OK: a sweep that asked for sizes only).  (A fit
// call knows the sizes, its allotments, before its groups have chosen: fitReport writes their info.)
DcsStatus EncRun::placeOutput()
{
    uint64_t *outOffsets = to.outOffsets;
    for (uint32_t j = 0 ; j < jobs.n ; ++j)
    {
        outOffsets[j + 1] = outOffsets[j] + size[j];
        if (jobs.fit == nullptr)
            writeInfo(j);
    }
    if (sweep.sizesOnly)
        return DCS_OK;
    const uint64_t total = outOffsets[jobs.n];
    dst = to.place != nullptr && *to.place ? (*to.place)(outOffsets, total) : (to.out != nullptr && to.outCap >= total ? to.out : nullptr);
    return dst != nullptr ? DCS_OK : DCS_ERR_CAPACITY;
}

// Where the jobs of group g lie in its blob, and the blob's size in words.  For the output: as in the output.  For a
// decode: where the device path's stream layout wants them (each stream on a 4-byte boundary, the blob's zeroed tail).
DcsStatus EncRun::layoutGroup(uint32_t g, size_t *nWords)
{
    const uint32_t j0 = groupFirst[g], n = groupFirst[g + 1] - j0;
    offs.resize(n);
    if (!sweep.measure)
    {
        for (uint32_t k = 0 ; k < n ; ++k)
            offs[k] = to.outOffsets[j0 + k] - to.outOffsets[j0];
        blobLen = static_cast<size_t>(to.outOffsets[j0 + n] - to.outOffsets[j0]);
        *nWords = (blobLen + 3) / 4 + 1;
        return DCS_OK;
    }
    ss.resize(n);
    for (uint32_t k = 0 ; k < n ; ++k)
    {
        const int c = win[j0 + k];
        const uint16_t ver = jobs.sets[hj[k].set].formatVersion;
        const bool a93 = setQ[hj[k].set] != kA93None;
        ss[k] = DcsSweepStream{ hj[k].nFrames, static_cast<uint32_t>(size[j0 + k]),
                                ver == 0x9301 ? DCS_OS93A : ver == 0x9302 ? DCS_OS93B : kCandSub[c] == 3 ? DCS_OS95 : DCS_OS94, kCandType[c],
                                jobs.os93 ? 0 : kCandSub[c], keep[j0 + k],
                                a93 ? 0x80u | static_cast<uint32_t>(choiceA[j0 + k].selector) << 5 | static_cast<uint32_t>(keep[j0 + k]) : 0u };
    }
    size_t blobBytes;
    ENCTRY(dcsSweepLayout(ss.data(), n, offs.data(), &blobLen, &blobBytes));
    *nWords = blobBytes / 4;
    return DCS_OK;
}

// header, pack and swap of the resident group g into a blob of its own
DcsStatus EncRun::packGroup(uint32_t g)
{
    const uint32_t n = groupFirst[g + 1] - groupFirst[g], JF = residentFrames;
    size_t nWords;
    ENCTRY(layoutGroup(g, &nWords));
    blob.clear();
    staged = false;
    ENCCHK(blob.alloc(&dW, nWords));
    ENCCHK(hipMemsetAsync(dW, 0, sizeof(uint32_t) * nWords, st));
    ENCCHK(hipMemcpyAsync(gb.dOutOff, offs.data(), sizeof(uint64_t) * n, hipMemcpyHostToDevice, st));
    if (anyV != 0)
        hipLaunchKernelGGL(encHeadKernel, dim3(n), dim3(64), 0, st, gb.dJobs, gb.dHdr, gb.dWin, gb.dOutOff, dW);
    if (anyV != 0 && jobs.os93)
        hipLaunchKernelGGL(enc93PackKernel, dim3((JF + 3) / 4), dim3(64), 0, st, cb.dT, cb.dSpec, gb.dFJ, gb.dJobs, gb.dHdr, gb.dKeep, gb.dWin,
                           JF, gb.o93.dBand, gb.dFrameOff, gb.dOutOff, dW);
    if (anyV != 0 && !jobs.os93)
        hipLaunchKernelGGL(encPackKernel, dim3((JF + 3) / 4), dim3(64), 0, st, cb.dT, cb.dSpec, gb.dFJ, gb.dJobs, gb.dHdr, gb.dKeep, gb.dWin,
                           JF, gb.v94.dCodes, gb.v94.dHdrBits, gb.v94.dSmpBits, gb.dFrameOff, gb.dOutOff, dW);
    if (!qs.empty())
    {
        // the Type-1 jobs: each job-frame's choices (A3), the frames' offsets (A4), the 3-byte headers and the pack (A5)
        hipLaunchKernelGGL(enc93aFrameKernel<true>, dim3(JF), dim3(256), 0, st, cb.a93.dA, cb.a93.dFloorE, cb.dSpec, gb.dFJ,
                           static_cast<const uint32_t *>(nullptr), 0u, 0u, 0u, static_cast<Enc93aTot *>(nullptr), gb.dJobs, cb.a93.dSetQ,
                           gb.a93.dChoice, gb.a93.dRec);
        hipLaunchKernelGGL(enc93aOffsetKernel, dim3(n), dim3(256), 0, st, gb.dJobs, cb.a93.dSetQ, gb.a93.dRec, gb.dFrameOff);
        hipLaunchKernelGGL(enc93aHeadKernel, dim3((n + 63) / 64), dim3(64), 0, st, gb.dJobs, cb.a93.dSetQ, gb.a93.dChoice, gb.dOutOff, n, dW);
        hipLaunchKernelGGL(enc93aPackKernel, dim3(JF), dim3(128), 0, st, cb.a93.dA, cb.dSpec, gb.dFJ, gb.dJobs, cb.a93.dSetQ, gb.a93.dChoice,
                           gb.a93.dRec, gb.dFrameOff, gb.dOutOff, dW);
    }
    if (jobs.rd)
        ENCTRY(rdPackGroup(n, JF));
    if (jobs.rd93)
        ENCTRY(rd93PackGroup(n, JF));
    hipLaunchKernelGGL(encSwapKernel, dim3(static_cast<unsigned>((nWords + 255) / 256)), dim3(256), 0, st, dW, nWords);
    ENCCHK(hipGetLastError());
    return DCS_OK;
}

// the packed group g to its place in the output, and a wait
DcsStatus EncRun::deliverGroup(uint32_t g)
{
    ENCCHK(hipMemcpyAsync(dst + to.outOffsets[groupFirst[g]], dW, blobLen, hipMemcpyDeviceToHost, st));
    ENCCHK(hipStreamSynchronize(st));
    return DCS_OK;
}

// the packed group's blob to `stage`, queued once per group; the caller waits
DcsStatus EncRun::stageBlob()
{
    if (staged)
        return DCS_OK;
    stage.resize(blobLen);
    ENCCHK(hipMemcpyAsync(stage.data(), dW, blobLen, hipMemcpyDeviceToHost, st));
    staged = true;
    return DCS_OK;
}

// The jobs of the packed group (n of them) whose streams are decoded.  One kind is left out: an OS93a Type-0 stream with
// no band kept.  Its header is sixteen 0xFF bytes, the first of which carries the type bit, so every decoder reads it as
// OS93a Type 1 with 31 bands; its record stays measured = 0.  (A Type-1 stream's header says what it is: always decoded.)
void EncRun::selectDecodes(uint32_t n)
{
    sel.clear(); selS.clear(); selOff.clear();
    mostFrames = 0;
    selFrames = 0;
    for (uint32_t k = 0 ; k < n ; ++k)
        if (!(ss[k].os == DCS_OS93A && ss[k].formatType == 0 && ss[k].bandsToKeep == 0))
        {
            sel.push_back(k); selS.push_back(ss[k]); selOff.push_back(offs[k]);
            mostFrames = std::max(mostFrames, hj[k].nFrames);
            selFrames += hj[k].nFrames;
        }
}

// One attempt: the selected streams decoded, on the device path from the bytes where they lie or (onHost) as a host-planned
// batch from the staged blob, then M1 and a wait, after which meas[] is on the host, and so is the blob where the output
// wants it.  *unusable: the device planner gave the list up (its flag); the sums are then not to be used.
DcsStatus EncRun::decodeAndCompare(uint32_t n, bool onHost, bool *unusable)
{
    if (onHost && !staged)
    {
        ENCTRY(stageBlob());
        ENCCHK(hipStreamSynchronize(st));
    }
    SweepDecodeGuard dec;
    const int16_t *decPcm = nullptr;
    const uint32_t *decErr = nullptr, *firstFrame = nullptr;
    const volatile uint32_t *flag = nullptr;
    const uint32_t nSel = static_cast<uint32_t>(sel.size());
    ENCTRY(dcsSweepDecodeStart(ctx, selS.data(), nSel, selOff.data(), reinterpret_cast<const uint8_t *>(dW), blobLen,
                               onHost ? stage.data() : nullptr, &dec.d, &decPcm, &decErr, &flag, &firstFrame));
    for (uint32_t i = 0 ; i < nSel ; ++i)
        firstDec[sel[i]] = firstFrame[i];
    ENCCHK(hipMemcpyAsync(gb.m.dFirstDec, firstDec.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemsetAsync(gb.m.dMeas, 0, sizeof(EncMeasure) * n, st));
    hipLaunchKernelGGL(encMeasureKernel, dim3(n, (mostFrames + 1 + kMeasureFrames - 1) / kMeasureFrames), dim3(256), 0, st,
                       cb.dPcm, cb.dStr, gb.dJobs, gb.m.dFirstDec, decPcm, decErr, gb.m.dMeas);
    ENCCHK(hipGetLastError());
    ENCCHK(hipMemcpyAsync(meas.data(), gb.m.dMeas, sizeof(EncMeasure) * n, hipMemcpyDeviceToHost, st));
    if (dst != nullptr)
        ENCTRY(stageBlob());
    ENCCHK(hipStreamSynchronize(st));
    *unusable = flag != nullptr && *flag != 0;
    return DCS_OK;
}

// meas[] to the results of group g's jobs, and their bytes from `stage` to the output
DcsStatus EncRun::reportGroup(uint32_t g)
{
    const uint32_t j0 = groupFirst[g], n = groupFirst[g + 1] - j0;
    for (uint32_t k = 0 ; k < n ; ++k)
    {
        const uint32_t j = j0 + k;
        if (meas[k].err != 0)
        {
            dcsCtxSetError(ctx, ("job " + std::to_string(j) + " (" + name(hj[k].stream) + ", set " + std::to_string(hj[k].set)
                                 + "): the decoder reports an error in a frame of the stream just encoded").c_str());
            return DCS_ERR_HIP;
        }
        DcsSweepResult &r = sweep.results[j];
        if (dst != nullptr)
            memcpy(dst + to.outOffsets[j], stage.data() + offs[k], size[j]);
        if (firstDec[k] == kNotDecoded)
            continue;
        r.measured = 1;
        r.peakErr = meas[k].peak;
        r.nCompared = hs[hj[k].stream].nSamples;
        r.sumSrcSq = static_cast<int64_t>(meas[k].srcSq);
        r.sumDecSq = static_cast<int64_t>(meas[k].decSq);
        r.sumCross = static_cast<int64_t>(meas[k].cross);
    }
    return DCS_OK;
}

// The packed group g decoded and compared with its sources.  The decode, as transcoding runs it (dcs_transcode.hip.h): the
// device path on the bytes where they lie; the host-planned batch, for which the bytes are read back, where the device
// planner cannot serve the list (a second attempt) or one long stream dominates it (the only one: the device index walk is
// one wavefront per stream, serial over its frames).
DcsStatus EncRun::measureGroup(uint32_t g)
{
    const uint32_t n = groupFirst[g + 1] - groupFirst[g];
    selectDecodes(n);
    const bool walkOnHost = mostFrames > 2048 && uint64_t(mostFrames) * 64 > selFrames;
    meas.assign(n, EncMeasure{});
    firstDec.assign(n, kNotDecoded);
    if (sel.empty() && dst != nullptr)
    {
        ENCTRY(stageBlob());
        ENCCHK(hipStreamSynchronize(st));
    }
    for (int attempt = walkOnHost ? 1 : 0 ; attempt < 2 && !sel.empty() ; ++attempt)
    {
        bool unusable = false;
        ENCTRY(decodeAndCompare(n, attempt == 1, &unusable));
        if (!unusable)
            break;
    }
    return reportGroup(g);
}

DcsStatus EncRun::run()
{
    ENCTRY(checkStreams());
    to.outOffsets[0] = 0;
    if (in.nStreams == 0 || jobs.n == 0)
    {
        for (uint32_t j = 0 ; j < jobs.n ; ++j)
            to.outOffsets[j + 1] = 0;
        return DCS_OK;
    }
    buildSets();
    win.resize(jobs.n); keep.resize(jobs.n); size.resize(jobs.n); choiceA.resize(jobs.n);
    if (jobs.rd)
        choiceRd.resize(jobs.n);
    if (jobs.rd93)
        choiceRd93.resize(jobs.n);
    ENCCHK(hipSetDevice(dcsCtxDevice(ctx)));
    ENCTRY(allocCall());
    ENCTRY(allocGroups());
    ENCTRY(analyse());
    const uint32_t nGroups = static_cast<uint32_t>(groupFirst.size()) - 1;
    for (uint32_t g = 0 ; g < nGroups ; ++g)
    {
        ENCTRY(runGroup(g));
        if (g == 0)
            ENCTRY(checkInput());
    }
    if (jobs.fit != nullptr)
        ENCTRY(fitAllot());
    ENCTRY(placeOutput());
    if (dst == nullptr && !sweep.measure)
        return DCS_OK;
    for (uint32_t g = 0 ; g < nGroups ; ++g)
    {
        if (jobs.fit != nullptr)
        {
            ENCTRY(nGroups == 1 ? fitRechoose(g) : runGroup(g));
            ENCTRY(fitReport(g));
        }
        else if (resident != g)
            ENCTRY(runGroup(g));
        ENCTRY(packGroup(g));
        ENCTRY(sweep.measure ? measureGroup(g) : deliverGroup(g));
    }
    if (jobs.fit != nullptr)
        fitRecord();
    return DCS_OK;
}

// the entry points that encode every stream with one parameter set: job i = (stream i, set 0)
DcsStatus encodeStreams(DcsCtx *ctx, EncInput &in, const DcsEncodeParams *params, bool os93, const EncOutput &to)
{
    const bool dev = in.devPcm != nullptr, devF = in.devFloat != nullptr;
    if (ctx == nullptr || in.sampleOffsets == nullptr || to.outOffsets == nullptr
        || (in.nStreams != 0 && in.hostPcm == nullptr && !dev && !devF) || (dev && in.devErr == nullptr))
        return DCS_ERR_INVALID_ARG;
    if (!paramsValid(params, os93))
    {
        if (const char *why = whyOs93aType1(params, os93))
            dcsCtxSetError(ctx, why);
        return DCS_ERR_INVALID_ARG;
    }
    std::vector<DcsSweepJob> list(in.nStreams);
    for (uint32_t i = 0 ; i < in.nStreams ; ++i)
        list[i] = DcsSweepJob{ i, 0 };
    return EncRun(ctx, in, EncJobs{ params, 1, list.data(), in.nStreams, os93 }, to, EncSweep()).run();
}

// dcs_encode_streams and dcs_encode93_streams
DcsStatus encodeHostPcm(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams, const DcsEncodeParams *params,
                        bool os93, const EncOutput &to)
{
    EncInput in;
    in.sampleOffsets = sampleOffsets;
    in.nStreams = nStreams;
    in.hostPcm = pcm;
    return encodeStreams(ctx, in, params, os93, to);
}

}  // namespace

extern "C" DcsStatus dcs_encode_streams(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams,
                                        const DcsEncodeParams *params, uint8_t *out, size_t outCap, uint64_t *outOffsets,
                                        DcsEncodeInfo *info)
{
    return encodeHostPcm(ctx, pcm, sampleOffsets, nStreams, params, false, EncOutput{ out, outCap, outOffsets, info, nullptr });
}

extern "C" DcsStatus dcs_encode93_streams(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams,
                                          const DcsEncodeParams *params, uint8_t *out, size_t outCap, uint64_t *outOffsets,
                                          DcsEncodeInfo *info)
{
    return encodeHostPcm(ctx, pcm, sampleOffsets, nStreams, params, true, EncOutput{ out, outCap, outOffsets, info, nullptr });
}

// ------------------------------------------------------------------------------------------------------- sweeping and fitting

extern "C" void dcs_encode_sweep_group_frames(uint64_t maxJobFrames)
{
    gGroupFrames.store(maxJobFrames);
}

namespace {

// what dcs_encode_sweep and dcs_encode93a_sweep refuse before they look at a set
bool sweepArgsValid(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams, const DcsEncodeParams *sets,
                    uint32_t nSets, uint32_t flags, const DcsSweepResult *results, const uint8_t *out, size_t outCap, const uint64_t *outOffsets)
{
    return !(ctx == nullptr || sampleOffsets == nullptr || outOffsets == nullptr || sets == nullptr || nSets == 0 || (nStreams != 0 && pcm == nullptr)
             || (flags & ~DCS_SWEEP_MEASURE) != 0 || ((flags & DCS_SWEEP_MEASURE) != 0 && results == nullptr) || (out == nullptr && outCap != 0));
}

// ... and what they do once their sets are checked: the job list (null: every pair, stream-major), then the driver on the
// caller's PCM
DcsStatus sweepHostPcm(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams, EncJobs js, uint32_t flags,
                       DcsSweepResult *results, const EncOutput &to)
{
    const uint32_t nSets = js.nSets;
    std::vector<DcsSweepJob> all;
    if (js.list == nullptr)
    {
        if (static_cast<uint64_t>(nStreams) * nSets > 0xFFFFFFFFull)
            return DCS_ERR_INVALID_ARG;
        js.n = nStreams * nSets;
        all.resize(js.n);
        for (uint32_t j = 0 ; j < js.n ; ++j)
            all[j] = DcsSweepJob{ j / nSets, j % nSets };
        js.list = all.data();
    }
    for (uint32_t j = 0 ; j < js.n ; ++j)
        if (js.list[j].stream >= nStreams || js.list[j].paramSet >= nSets)
        {
            dcsCtxSetError(ctx, ("job " + std::to_string(j) + ": names stream " + std::to_string(js.list[j].stream) + " of " + std::to_string(nStreams)
                                 + ", set " + std::to_string(js.list[j].paramSet) + " of " + std::to_string(nSets)).c_str());
            return DCS_ERR_INVALID_ARG;
        }
    EncInput in;
    in.sampleOffsets = sampleOffsets;
    in.nStreams = nStreams;
    in.hostPcm = pcm;
    EncSweep sweep;
    sweep.results = results;
    sweep.measure = (flags & DCS_SWEEP_MEASURE) != 0;
    sweep.sizesOnly = to.out == nullptr;
    return EncRun(ctx, in, js, to, sweep).run();
}

}  // namespace

extern "C" DcsStatus dcs_encode_sweep(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams,
                                      const DcsEncodeParams *sets, uint32_t nSets, const DcsSweepJob *jobs, uint32_t nJobs,
                                      uint32_t flags, DcsSweepResult *results, uint8_t *out, size_t outCap, uint64_t *outOffsets)
{
    if (!sweepArgsValid(ctx, pcm, sampleOffsets, nStreams, sets, nSets, flags, results, out, outCap, outOffsets))
        return DCS_ERR_INVALID_ARG;
    const bool os93 = sets[0].formatVersion != 0x9400;
    for (uint32_t k = 0 ; k < nSets ; ++k)
    {
        if (sets[k].formatVersion != sets[0].formatVersion)
        {
            dcsCtxSetError(ctx, ("set " + std::to_string(k) + ": the sets of one call belong to one encoder (all formatVersion 0x9400, all 0x9301 or all 0x9302)").c_str());
            return DCS_ERR_INVALID_ARG;
        }
        if (!paramsValid(&sets[k], os93))
        {
            const char *why = whyOs93aType1(&sets[k], os93);
            dcsCtxSetError(ctx, why != nullptr ? why : ("set " + std::to_string(k) + ": not a valid DcsEncodeParams").c_str());
            return DCS_ERR_INVALID_ARG;
        }
    }
    return sweepHostPcm(ctx, pcm, sampleOffsets, nStreams, EncJobs{ sets, nSets, jobs, nJobs, os93 }, flags, results,
                        EncOutput{ out, outCap, outOffsets, nullptr, nullptr });
}

// ------------------------------------------------------------------------------------------ OS93a, Type 0 and Type 1

extern "C" size_t dcs_encode93a_bound(uint64_t nSamples)
{
    return std::max(boundOf(nSamples, kMaxBitsPerFrame93), boundOf(nSamples, kA93MaxFrameBits));
}

extern "C" DcsStatus dcs_encode93a_sweep(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams,
                                         const DcsEncodeParams *sets, uint32_t nSets, const DcsSweepJob *jobs, uint32_t nJobs,
                                         uint32_t flags, DcsSweepResult *results, DcsEncode93aInfo *info93a,
                                         uint8_t *out, size_t outCap, uint64_t *outOffsets)
{
    if (!sweepArgsValid(ctx, pcm, sampleOffsets, nStreams, sets, nSets, flags, results, out, outCap, outOffsets))
        return DCS_ERR_INVALID_ARG;
    for (uint32_t k = 0 ; k < nSets ; ++k)
    {
        const std::string set = "set " + std::to_string(k);
        if (sets[k].formatVersion != 0x9301)
        {
            dcsCtxSetError(ctx, (set + ": dcs_encode93a_sweep takes OS93a sets only (formatVersion 0x9301)").c_str());
            return DCS_ERR_INVALID_ARG;
        }
        if (!paramsValid93a(&sets[k]))
        {
            dcsCtxSetError(ctx, (set + ": not a valid DcsEncodeParams").c_str());
            return DCS_ERR_INVALID_ARG;
        }
        if (sets[k].streamFormatType < 0)
        {
            dcsCtxSetError(ctx, (set + ": streamFormatType -1; a sweep lists Type 0 and Type 1 as sets of their own and reports both").c_str());
            return DCS_ERR_INVALID_ARG;
        }
    }
    return sweepHostPcm(ctx, pcm, sampleOffsets, nStreams, EncJobs{ sets, nSets, jobs, nJobs, true }, flags, results,
                        EncOutput{ out, outCap, outOffsets, nullptr, nullptr, info93a });
}

namespace {

// Type 1 of every stream: one job per stream through the one driver
DcsStatus encode93aType1(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams, const DcsEncodeParams *params,
                         const EncOutput &to)
{
    DcsEncodeParams p1 = *params;
    p1.streamFormatType = 1;
    EncInput in;
    in.sampleOffsets = sampleOffsets;
    in.nStreams = nStreams;
    in.hostPcm = pcm;
    std::vector<DcsSweepJob> list(nStreams);
    for (uint32_t i = 0 ; i < nStreams ; ++i)
        list[i] = DcsSweepJob{ i, 0 };
    return EncRun(ctx, in, EncJobs{ &p1, 1, list.data(), nStreams, true }, to, EncSweep()).run();
}

}  // namespace

extern "C" DcsStatus dcs_encode93a_streams(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams,
                                           const DcsEncodeParams *params, uint8_t *out, size_t outCap, uint64_t *outOffsets,
                                           DcsEncodeInfo *info, DcsEncode93aInfo *info93a)
{
    if (ctx == nullptr || sampleOffsets == nullptr || outOffsets == nullptr || (nStreams != 0 && pcm == nullptr) || !paramsValid93a(params))
        return DCS_ERR_INVALID_ARG;
    if (info93a != nullptr)
        memset(info93a, 0, sizeof(DcsEncode93aInfo) * nStreams);
    if (params->streamFormatType == 0)
        return encodeHostPcm(ctx, pcm, sampleOffsets, nStreams, params, true, EncOutput{ out, outCap, outOffsets, info, nullptr });
    if (params->streamFormatType == 1)
        return encode93aType1(ctx, pcm, sampleOffsets, nStreams, params, EncOutput{ out, outCap, outOffsets, info, nullptr, info93a });

    // the wildcard: both types into buffers of their own, then per stream the first strictly smallest, Type 0 first (CloseStream :805)
    DcsEncodeParams p0 = *params;
    p0.streamFormatType = 0;
    std::vector<uint64_t> off0(nStreams + 1), off1(nStreams + 1);
    std::vector<DcsEncodeInfo> inf0(nStreams), inf1(nStreams);
    size_t cap0 = 0, cap1 = 0;
    for (uint32_t i = 0 ; i < nStreams ; ++i)
    {
        const uint64_t n = sampleOffsets[i + 1] > sampleOffsets[i] ? sampleOffsets[i + 1] - sampleOffsets[i] : 0;
        cap0 += boundOf(n, kMaxBitsPerFrame93);
        cap1 += boundOf(n, kA93MaxFrameBits);
    }
    std::vector<uint8_t> buf0(cap0 + 1), buf1(cap1 + 1);
    ENCTRY(encodeHostPcm(ctx, pcm, sampleOffsets, nStreams, &p0, true, EncOutput{ buf0.data(), buf0.size(), off0.data(), inf0.data(), nullptr }));
    ENCTRY(encode93aType1(ctx, pcm, sampleOffsets, nStreams, params, EncOutput{ buf1.data(), buf1.size(), off1.data(), inf1.data(), nullptr, info93a }));
    outOffsets[0] = 0;
    for (uint32_t i = 0 ; i < nStreams ; ++i)
    {
        const bool one = off1[i + 1] - off1[i] < off0[i + 1] - off0[i];
        outOffsets[i + 1] = outOffsets[i] + (one ? off1[i + 1] - off1[i] : off0[i + 1] - off0[i]);
        if (info != nullptr)
            info[i] = one ? inf1[i] : inf0[i];
    }
    if (nStreams == 0)
        return DCS_OK;
    if (out == nullptr || outCap < outOffsets[nStreams])
        return DCS_ERR_CAPACITY;
    for (uint32_t i = 0 ; i < nStreams ; ++i)
    {
        const uint64_t n = outOffsets[i + 1] - outOffsets[i];
        const bool one = off1[i + 1] - off1[i] < off0[i + 1] - off0[i];
        memcpy(out + outOffsets[i], one ? buf1.data() + off1[i] : buf0.data() + off0[i], n);
    }
    return DCS_OK;
}

extern "C" DcsStatus dcs_encode_fit(const uint64_t *nBytes, const uint64_t *sqErr, uint32_t nStreams, uint32_t nSets, uint64_t budget,
                                    int32_t *choiceOut, uint64_t *totalOut)
{
    if (nBytes == nullptr || sqErr == nullptr || nStreams == 0 || nSets == 0 || choiceOut == nullptr || totalOut == nullptr)
        return DCS_ERR_INVALID_ARG;
    auto at = [nSets](const uint64_t *t, uint32_t i, uint32_t r) { return t[static_cast<size_t>(i) * nSets + r]; };
    // the first set, in the caller's order of preference, that fits as a whole
    uint32_t r = nSets, smallest = 0;
    uint64_t total = 0, smallestTotal = 0;
    for (uint32_t c = 0 ; c < nSets && r == nSets ; ++c)
    {
        uint64_t sum = 0;
        for (uint32_t i = 0 ; i < nStreams ; ++i)
            sum += at(nBytes, i, c);
        if (c == 0 || sum < smallestTotal) { smallest = c; smallestTotal = sum; }
        if (sum <= budget) { r = c; total = sum; }
    }
    if (r == nSets)
    {
        for (uint32_t i = 0 ; i < nStreams ; ++i)
            choiceOut[i] = static_cast<int32_t>(smallest);
        *totalOut = smallestTotal;
        return DCS_ERR_CAPACITY;
    }
    // the streams by descending error at r (ties: ascending index), each moved once to the first more preferred set that
    // lowers its error and still fits
    std::vector<uint32_t> order(nStreams);
    for (uint32_t i = 0 ; i < nStreams ; ++i)
    {
        order[i] = i;
        choiceOut[i] = static_cast<int32_t>(r);
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return at(sqErr, a, r) > at(sqErr, b, r); });
    for (uint32_t i : order)
        for (uint32_t c = 0 ; c < r ; ++c)
            if (at(sqErr, i, c) < at(sqErr, i, r) && total - at(nBytes, i, r) + at(nBytes, i, c) <= budget)
            {
                total = total - at(nBytes, i, r) + at(nBytes, i, c);
                choiceOut[i] = static_cast<int32_t>(c);
                break;
            }
    *totalOut = total;
    return DCS_OK;
}

// ----------------------------------------------------------------------------------------- transcoding (dcs_transcode.hip.h)

namespace {

uint16_t sourceVersion(int32_t os) { return os == DCS_OS93A ? 0x9301 : os == DCS_OS93B ? 0x9302 : 0x9400; }

}  // namespace

// EncodeDCSFile's rule (DCSEncoder.cpp:498-517): a source is copied when its version is the target's, or when both are OS93
// and the source is Type 0; every other source is decoded for nFrames + 1 frames and encoded again.  why = the reason of a
// failure, for dcs_last_error.
DcsStatus dcsTranscodePlan(const DcsStreamRef *src, uint32_t nStreams, const DcsEncodeParams *target, uint32_t flags,
                           int32_t *actionOut, uint64_t *boundOut, std::string &why)
{
    if ((nStreams != 0 && src == nullptr) || target == nullptr || (flags & ~DCS_TRANSCODE_REENCODE_ALL) != 0)
        return DCS_ERR_INVALID_ARG;
    const bool os93 = target->formatVersion != 0x9400;
    if (!paramsValid(target, os93))
    {
        char text[96];
        snprintf(text, sizeof(text), "target: not a valid DcsEncodeParams for formatVersion 0x%x", target->formatVersion);
        const char *type1 = whyOs93aType1(target, os93);
        why = type1 != nullptr ? type1 : text;
        return DCS_ERR_INVALID_ARG;
    }
    for (uint32_t i = 0 ; i < nStreams ; ++i)
    {
        const DcsStreamRef &s = src[i];
        const std::string name = "stream " + std::to_string(i);
        if (s.data == nullptr || s.os < DCS_OS93A || s.os > DCS_OS95)
        {
            why = name + ": no data, or not a DcsOsVersion";
            return DCS_ERR_INVALID_ARG;
        }
        if (s.len < 3)
        {
            why = name + ": shorter than 3 bytes (no type bit)";
            return DCS_ERR_BAD_STREAM;
        }
        const uint16_t v = sourceVersion(s.os);
        const uint32_t nFrames = (static_cast<uint32_t>(s.data[0]) << 8) | s.data[1];
        const bool copy = (flags & DCS_TRANSCODE_REENCODE_ALL) == 0
                          && (v == target->formatVersion || (os93 && v != 0x9400 && (s.data[2] & 0x80) == 0));
        if (!copy && nFrames == 0)
        {
            why = name + ": zero frames";
            return DCS_ERR_BAD_STREAM;
        }
        if (!copy && nFrames + 1 > 65535)
        {
            why = name + ": 65 535 frames; re-encoded with the extra frame it would need 65 536, more than the frame count holds";
            return DCS_ERR_INVALID_ARG;
        }
        if (actionOut != nullptr)
            actionOut[i] = copy ? DCS_TRANSCODE_COPIED : DCS_TRANSCODE_REENCODED;
        if (boundOut != nullptr)
            boundOut[i] = copy ? static_cast<uint64_t>(s.len) : boundOf(static_cast<uint64_t>(nFrames + 1) * 240, os93 ? kMaxBitsPerFrame93 : kMaxBitsPerFrame);
    }
    return DCS_OK;
}

// The re-encodes of dcs_transcode_streams: encodeStreams on a decode batch's resident PCM (stream k from sample
// sampleOffsets[k]) and error words.  label[k] = the source's index, for messages.  *unusable: planFlag was set after the
// first wait (nothing written).  place: as EncPlace.
DcsStatus dcsEncodeFromDevice(DcsCtx *ctx, const int16_t *dPcm, const uint32_t *dErr, const volatile uint32_t *planFlag,
                              const uint64_t *sampleOffsets, const uint32_t *label, uint32_t nStreams, const DcsEncodeParams *target,
                              bool *unusable, uint64_t *encOffsets, DcsEncodeInfo *info, const EncPlace &place)
{
    EncInput in;
    in.sampleOffsets = sampleOffsets;
    in.nStreams = nStreams;
    in.devPcm = dPcm;
    in.devErr = dErr;
    in.label = label;
    in.planFlag = planFlag;
    const DcsStatus st = encodeStreams(ctx, in, target, target->formatVersion != 0x9400, EncOutput{ nullptr, 0, encOffsets, info, &place });
    *unusable = in.unusable;
    return st;
}

// The chain in front of the encoder, each header using only those before it.

// -------------------------------------------------------------------- level control (dcs_level.hip.h)

#include "dcs_level.hip.h"

// ------------------------------------------------------------------------------- resampling (dcs_resample.hip.h)

#include "dcs_resample.hip.h"

// ------------------------------------------------------------------------------------ the WAV reader (dcs_wav.hip.h)

#include "dcs_wav.hip.h"

// ---------------------------------------------------------------------------------- the FLAC reader (dcs_flac.hip.h)

#include "dcs_flac.hip.h"

// ------------------------------------------------------------------------------ the FLAC writer (dcs_flac_write.hip.h)

#include "dcs_flac_write.hip.h"

// ------------------------------------------------------------------------ encoding files (dcs_encode_files.hip.h)

#include "dcs_encode_files.hip.h"

// ------------------------------------------------- the rate-distortion 1994+ encoder: kernels and driver (dcs_encode_rd.hip.h)
// (behind every other kernel of the unit, templates included: those keep their place in the code object)

#include "dcs_encode_rd.hip.h"

namespace {

DcsStatus EncRun::rdAllocCall()
{
    ENCCHK(call.alloc(&cb.rd.dR, 1));
    ENCCHK(call.alloc(&cb.rd.dItems, size_t(kRdItemsPerFrame) * F));
    ENCCHK(call.alloc(&cb.rd.dPeak, size_t(16) * in.nStreams));
    ENCCHK(call.alloc(&cb.rd.dD0, size_t(16) * in.nStreams));
    ENCCHK(call.alloc(&cb.rd.dFloor, size_t(16) * jobs.nSets));
    return DCS_OK;
}

hipError_t EncRun::rdAllocGroup()
{
    const size_t JF = static_cast<size_t>(groupFrames), NJ = groupJobs;
    HIPTRY(group.alloc(&gb.rd.dTot, size_t(kRdRowsPerJob) * NJ));
    HIPTRY(group.alloc(&gb.rd.dChoice, NJ));
    HIPTRY(group.alloc(&gb.rd.dBudget, NJ));
    HIPTRY(group.alloc(&gb.rd.dSurv, 256 * JF));
    HIPTRY(group.alloc(&gb.rd.dEnd, 16 * NJ));
    HIPTRY(group.alloc(&gb.rd.dCodes, 16 * JF));
    HIPTRY(group.alloc(&gb.rd.dBits, JF));
    return hipSuccess;
}

// the budgets of all jobs, in frame bits (-1: nothing fits)
void EncRun::budgetsRd()
{
    budgetRd.resize(jobs.n);
    for (uint32_t j = 0 ; j < jobs.n ; ++j)
    {
        const uint64_t nF = hs[jobs.list[j].stream].nFrames;
        if (jobs.budgetBytes == nullptr)
            budgetRd[j] = static_cast<long long>(static_cast<uint64_t>(jobs.sets[jobs.list[j].paramSet].targetBitRate) * nF * 240ull / 31250ull);
        else
            budgetRd[j] = jobs.budgetBytes[j] >= 18 ? (static_cast<long long>(jobs.budgetBytes[j]) - 18) * 8 : -1;
    }
}

// R1 over every stream-frame; the budgets
DcsStatus EncRun::rdAnalyse()
{
    floorRd.resize(size_t(16) * jobs.nSets);
    for (uint32_t k = 0 ; k < jobs.nSets ; ++k)
        floorERd(jobs.sets[k].maximumQuantizationError, floorRd.data() + size_t(16) * k);
    budgetsRd();
    ENCCHK(hipMemcpyAsync(cb.rd.dR, &encTabsRd(), sizeof(EncRdTabs), hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(cb.rd.dFloor, floorRd.data(), sizeof(unsigned long long) * floorRd.size(), hipMemcpyHostToDevice, st));
    ENCCHK(hipMemsetAsync(cb.rd.dPeak, 0, sizeof(uint32_t) * 16 * in.nStreams, st));
    ENCCHK(hipMemsetAsync(cb.rd.dD0, 0, sizeof(unsigned long long) * 16 * in.nStreams, st));
    hipLaunchKernelGGL(encRdItemKernel, dim3(F), dim3(256), 0, st, cb.dT, cb.rd.dR, cb.dSpec, cb.dFS, cb.rd.dItems, cb.rd.dPeak, cb.rd.dD0);
    return DCS_OK;
}

// R2 and R3 for the n jobs of a group from job j0; the choices are on the host after runGroup's wait
DcsStatus EncRun::rdRunGroup(uint32_t j0, uint32_t n)
{
    ENCCHK(hipMemcpyAsync(gb.rd.dBudget, budgetRd.data() + j0, sizeof(long long) * n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(encRdTrellisKernel<false>, dim3(kRdRowsPerJob / 16 * n), dim3(256), 0, st, cb.dT, cb.rd.dR, cb.rd.dItems, cb.rd.dPeak,
                       cb.rd.dFloor, gb.dJobs, cb.dSets, gb.rd.dTot, static_cast<const EncRdChoice *>(nullptr),
                       static_cast<uint8_t *>(nullptr), static_cast<uint8_t *>(nullptr));
    hipLaunchKernelGGL(encRdChooseKernel, dim3(n), dim3(256), 0, st, gb.rd.dTot, cb.rd.dD0, gb.dJobs, cb.dSets, gb.rd.dBudget, gb.rd.dChoice);
    ENCCHK(hipMemcpyAsync(choiceRd.data() + j0, gb.rd.dChoice, sizeof(EncRdChoice) * n, hipMemcpyDeviceToHost, st));
    return DCS_OK;
}

// R4 to R6 for the resident group: the chosen chains with their survivors, the frames' bits and offsets, header and pack
DcsStatus EncRun::rdPackGroup(uint32_t n, uint32_t JF)
{
    ENCCHK(hipMemsetAsync(gb.rd.dCodes, 0, size_t(16) * JF, st));
    hipLaunchKernelGGL(encRdTrellisKernel<true>, dim3(n), dim3(256), 0, st, cb.dT, cb.rd.dR, cb.rd.dItems, cb.rd.dPeak, cb.rd.dFloor,
                       gb.dJobs, cb.dSets, static_cast<EncRdTot *>(nullptr), gb.rd.dChoice, gb.rd.dSurv, gb.rd.dEnd);
    hipLaunchKernelGGL(encRdBackKernel, dim3((16 * n + 63) / 64), dim3(64), 0, st, gb.dJobs, gb.rd.dChoice, gb.rd.dSurv, gb.rd.dEnd, n,
                       gb.rd.dCodes);
    hipLaunchKernelGGL(encRdBitsKernel, dim3((JF + 63) / 64), dim3(64), 0, st, cb.dT, cb.rd.dItems, cb.rd.dPeak, gb.dFJ, gb.dJobs,
                       gb.rd.dChoice, gb.rd.dCodes, JF, gb.rd.dBits);
    hipLaunchKernelGGL(encRdOffsetKernel, dim3(n), dim3(256), 0, st, gb.dJobs, gb.rd.dBits, gb.dFrameOff);
    hipLaunchKernelGGL(encRdHeadKernel, dim3((n + 63) / 64), dim3(64), 0, st, cb.dT, cb.rd.dPeak, gb.dJobs, gb.rd.dChoice, gb.dOutOff, n, dW);
    hipLaunchKernelGGL(encRdPackKernel, dim3(JF), dim3(64), 0, st, cb.dT, cb.rd.dR, cb.dSpec, cb.rd.dItems, cb.rd.dPeak, gb.dFJ, gb.dJobs,
                       gb.rd.dChoice, gb.rd.dCodes, gb.dFrameOff, gb.dOutOff, dW);
    return DCS_OK;
}

}  // namespace

extern "C" size_t dcs_encode_rd_bound(uint64_t nSamples)
{
    return boundOf(nSamples, rdMaxFrameBits());
}

extern "C" DcsStatus dcs_encode_rd_streams(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams,
                                           const DcsEncodeParams *params, const uint32_t *budgetBytes, uint8_t *out, uint64_t outCap,
                                           uint64_t *outOffsets, DcsEncodeInfo *info, DcsEncodeRdInfo *infoRd)
{
    if (ctx == nullptr || sampleOffsets == nullptr || outOffsets == nullptr || (nStreams != 0 && pcm == nullptr))
        return DCS_ERR_INVALID_ARG;
    if (!paramsValidRd(params))
    {
        dcsCtxSetError(ctx, "dcs_encode_rd_streams: formatVersion 0x9400, streamFormatType 0, 1 or -1, streamFormatSubType 0, 3 or -1, "
                            "targetBitRate 1..100 000 000 and finite parameters");
        return DCS_ERR_INVALID_ARG;
    }
    EncInput in;
    in.sampleOffsets = sampleOffsets;
    in.nStreams = nStreams;
    in.hostPcm = pcm;
    std::vector<DcsSweepJob> list(nStreams);
    for (uint32_t i = 0 ; i < nStreams ; ++i)
        list[i] = DcsSweepJob{ i, 0 };
    EncJobs js{ params, 1, list.data(), nStreams, false };
    js.rd = true;
    js.budgetBytes = budgetBytes;
    EncOutput to{ out, static_cast<size_t>(outCap), outOffsets, info, nullptr, nullptr };
    to.infoRd = infoRd;
    return EncRun(ctx, in, js, to, EncSweep()).run();
}

// ------------------------------------------ the rate-distortion OS93 Type-0 encoder: kernels and driver (dcs_encode93_rd.hip.h)
// (behind every other kernel of the unit once more)

#include "dcs_encode93_rd.hip.h"

namespace {

DcsStatus EncRun::rd93AllocCall()
{
    ENCCHK(call.alloc(&cb.r93.dR, 1));
    ENCCHK(call.alloc(&cb.r93.dItems, size_t(kRd93ItemsPerFrame) * F));
    ENCCHK(call.alloc(&cb.r93.dRecs, size_t(kRd93RecsPerFrame) * F));
    ENCCHK(call.alloc(&cb.r93.dD0, size_t(16) * in.nStreams));
    ENCCHK(call.alloc(&cb.r93.dFloor, jobs.nSets));
    return DCS_OK;
}

hipError_t EncRun::rd93AllocGroup()
{
    const size_t JF = static_cast<size_t>(groupFrames), NJ = groupJobs;
    HIPTRY(group.alloc(&gb.r93.dProxyJ, size_t(kRd93ProxyPerJob) * NJ));
    HIPTRY(group.alloc(&gb.r93.dProxyB, size_t(kRd93ProxyPerJob) * NJ));
    HIPTRY(group.alloc(&gb.r93.dHead, size_t(kRdKL) * NJ));
    HIPTRY(group.alloc(&gb.r93.dTot, size_t(kRdKL) * NJ));
    HIPTRY(group.alloc(&gb.r93.dChoice, NJ));
    HIPTRY(group.alloc(&gb.r93.dBudget, NJ));
    HIPTRY(group.alloc(&gb.r93.dCodes, 16 * JF));
    HIPTRY(group.alloc(&gb.r93.dBits, JF));
    return hipSuccess;
}

// S1 over every stream-frame; the budgets
DcsStatus EncRun::rd93Analyse()
{
    const uint16_t version = jobs.sets[0].formatVersion;        // (one per call: dcs_encode93_rd_streams has one set)
    floorRd.resize(jobs.nSets);
    for (uint32_t k = 0 ; k < jobs.nSets ; ++k)
        floorRd[k] = floorE93Rd(jobs.sets[k].maximumQuantizationError);
    budgetsRd();
    ENCCHK(hipMemcpyAsync(cb.r93.dR, &encTabs93Rd(version), sizeof(EncRdTabs), hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(cb.r93.dFloor, floorRd.data(), sizeof(unsigned long long) * floorRd.size(), hipMemcpyHostToDevice, st));
    ENCCHK(hipMemsetAsync(cb.r93.dD0, 0, sizeof(unsigned long long) * 16 * in.nStreams, st));
    hipLaunchKernelGGL(enc93RdItemKernel, dim3(F), dim3(256), 0, st, cb.dT, cb.r93.dR, rd93M0(version), cb.dSpec, cb.dFS, cb.r93.dItems,
                       cb.r93.dRecs, cb.r93.dD0);
    return DCS_OK;
}

// S2 to S5 for the n jobs (JF job-frames) of a group from job j0; the choices are on the host after runGroup's wait
DcsStatus EncRun::rd93RunGroup(uint32_t j0, uint32_t n, uint32_t JF)
{
    const uint32_t chunks = (JF + kRd93ChunkFrames - 1) / kRd93ChunkFrames;
    ENCCHK(hipMemcpyAsync(gb.r93.dBudget, budgetRd.data() + j0, sizeof(long long) * n, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemsetAsync(gb.r93.dProxyJ, 0, sizeof(unsigned long long) * kRd93ProxyPerJob * n, st));
    ENCCHK(hipMemsetAsync(gb.r93.dProxyB, 0, sizeof(uint32_t) * kRd93ProxyPerJob * n, st));
    ENCCHK(hipMemsetAsync(gb.r93.dTot, 0, sizeof(Enc93RdTot) * kRdKL * n, st));
    hipLaunchKernelGGL(enc93RdProxyKernel, dim3(kRd93ProxyPerJob / 256, chunks), dim3(256), 0, st, cb.r93.dR, cb.r93.dItems, cb.r93.dFloor,
                       gb.dFJ, gb.dJobs, JF, gb.r93.dProxyJ, gb.r93.dProxyB);
    hipLaunchKernelGGL(enc93RdHeaderKernel, dim3(n), dim3(64), 0, st, gb.r93.dProxyJ, gb.r93.dProxyB, cb.r93.dD0, gb.dJobs, gb.r93.dHead);
    hipLaunchKernelGGL(enc93RdTrellisKernel<false>, dim3(chunks, kRdKL), dim3(256), 0, st, cb.r93.dR, cb.r93.dItems, cb.r93.dRecs,
                       cb.r93.dFloor, gb.dFJ, gb.dJobs, JF, gb.r93.dHead, static_cast<const Enc93RdChoice *>(nullptr), gb.r93.dTot,
                       static_cast<uint8_t *>(nullptr), static_cast<uint32_t *>(nullptr));
    hipLaunchKernelGGL(enc93RdChooseKernel, dim3((n + 63) / 64), dim3(64), 0, st, gb.r93.dTot, gb.r93.dHead, cb.r93.dD0, gb.dJobs,
                       gb.r93.dBudget, n, gb.r93.dChoice);
    ENCCHK(hipMemcpyAsync(choiceRd93.data() + j0, gb.r93.dChoice, sizeof(Enc93RdChoice) * n, hipMemcpyDeviceToHost, st));
    return DCS_OK;
}

// S6 to S8 for the resident group: the chosen lambda's trellises with their paths, the frames' offsets, header and pack
DcsStatus EncRun::rd93PackGroup(uint32_t n, uint32_t JF)
{
    const uint32_t chunks = (JF + kRd93ChunkFrames - 1) / kRd93ChunkFrames;
    const uint32_t m0 = rd93M0(jobs.sets[0].formatVersion);
    hipLaunchKernelGGL(enc93RdTrellisKernel<true>, dim3(chunks), dim3(256), 0, st, cb.r93.dR, cb.r93.dItems, cb.r93.dRecs, cb.r93.dFloor,
                       gb.dFJ, gb.dJobs, JF, static_cast<const Enc93RdHead *>(nullptr), gb.r93.dChoice, static_cast<Enc93RdTot *>(nullptr),
                       gb.r93.dCodes, gb.r93.dBits);
    hipLaunchKernelGGL(encRdOffsetKernel, dim3(n), dim3(256), 0, st, gb.dJobs, gb.r93.dBits, gb.dFrameOff);
    hipLaunchKernelGGL(enc93RdHeadKernel, dim3((n + 63) / 64), dim3(64), 0, st, gb.dJobs, gb.r93.dChoice, gb.dOutOff, n, dW);
    hipLaunchKernelGGL(enc93RdPackKernel, dim3(JF), dim3(64), 0, st, cb.dT, cb.r93.dR, m0, cb.dSpec, cb.r93.dRecs, gb.dFJ, gb.dJobs,
                       gb.r93.dChoice, gb.r93.dCodes, gb.dFrameOff, gb.dOutOff, dW);
    return DCS_OK;
}

}  // namespace

extern "C" size_t dcs_encode93_rd_bound(uint64_t nSamples)
{
    return boundOf(nSamples, kRd93MaxFrameBits);
}

extern "C" DcsStatus dcs_encode93_rd_streams(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams,
                                             const DcsEncodeParams *params, const uint32_t *budgetBytes, uint8_t *out, uint64_t outCap,
                                             uint64_t *outOffsets, DcsEncodeInfo *info, DcsEncodeRdInfo *infoRd)
{
    if (ctx == nullptr || sampleOffsets == nullptr || outOffsets == nullptr || (nStreams != 0 && pcm == nullptr))
        return DCS_ERR_INVALID_ARG;
    if (!paramsValid93Rd(params))
    {
        dcsCtxSetError(ctx, "dcs_encode93_rd_streams: formatVersion 0x9301 or 0x9302, streamFormatType 0 or -1 (OS93 Type 0; Type 1 is "
                            "not searched), targetBitRate 1..100 000 000 and finite parameters");
        return DCS_ERR_INVALID_ARG;
    }
    EncInput in;
    in.sampleOffsets = sampleOffsets;
    in.nStreams = nStreams;
    in.hostPcm = pcm;
    std::vector<DcsSweepJob> list(nStreams);
    for (uint32_t i = 0 ; i < nStreams ; ++i)
        list[i] = DcsSweepJob{ i, 0 };
    EncJobs js{ params, 1, list.data(), nStreams, true };
    js.rd93 = true;
    js.budgetBytes = budgetBytes;
    EncOutput to{ out, static_cast<size_t>(outCap), outOffsets, info, nullptr, nullptr };
    to.infoRd = infoRd;
    return EncRun(ctx, in, js, to, EncSweep()).run();
}

// ------------------------------------------------------- a set of streams to one byte budget: kernels and driver (dcs_encode_rd_fit.hip.h)
// (behind every other kernel of the unit once more)

#include "dcs_encode_rd_fit.hip.h"

namespace {

DcsStatus EncRun::fitAllocCall()
{
    ENCCHK(call.alloc(&cb.fit.dCurveSize, size_t(kFitMaxPoints) * jobs.n));
    ENCCHK(call.alloc(&cb.fit.dCurveD, size_t(kFitMaxPoints) * jobs.n));
    ENCCHK(call.alloc(&cb.fit.dOff, size_t(jobs.n) + 1));
    if (jobs.fit->capBytes != nullptr)
        ENCCHK(call.alloc(&cb.fit.dCap, jobs.n));
    ENCCHK(call.alloc(&cb.fit.dAllot, jobs.n));
    ENCCHK(call.alloc(&cb.fit.dFit, 1));
    return DCS_OK;
}

// F1 behind R2 or S4 of the resident group (n jobs from job j0): its jobs' candidates into the call's curve table
DcsStatus EncRun::fitCurves(uint32_t j0, uint32_t n)
{
    unsigned long long *dSize = cb.fit.dCurveSize + size_t(kFitMaxPoints) * j0, *dD = cb.fit.dCurveD + size_t(kFitMaxPoints) * j0;
    if (jobs.rd)
        hipLaunchKernelGGL(encRdCurveKernel, dim3(n), dim3(256), 0, st, gb.rd.dTot, cb.rd.dD0, gb.dJobs, cb.dSets, dSize, dD);
    else
        hipLaunchKernelGGL(enc93RdCurveKernel, dim3((n * kFitMaxPoints + 63) / 64), dim3(64), 0, st, gb.r93.dTot, gb.r93.dHead, cb.r93.dD0,
                           gb.dJobs, n, dSize, dD);
    return DCS_OK;
}

// F2 to F4 over all jobs, and a wait: the allotments and the record are on the host after it, the curves never.  A job's
// budget is its allotment, or its cap where even its smallest candidate is beyond that (a pinned job: fits = 0).
DcsStatus EncRun::fitAllot()
{
    const EncFit &fit = *jobs.fit;
    std::vector<unsigned long long> off(size_t(jobs.n) + 1);
    for (uint32_t j = 0 ; j <= jobs.n ; ++j)
        off[j] = static_cast<unsigned long long>(kFitMaxPoints) * j;
    ENCCHK(hipMemcpyAsync(cb.fit.dOff, off.data(), sizeof(unsigned long long) * off.size(), hipMemcpyHostToDevice, st));
    if (fit.capBytes != nullptr)
        ENCCHK(hipMemcpyAsync(cb.fit.dCap, fit.capBytes, sizeof(uint32_t) * jobs.n, hipMemcpyHostToDevice, st));
    ENCTRY(fitAllotDevice(ctx, call, cb.fit.dCurveSize, cb.fit.dCurveD, cb.fit.dOff, jobs.n, size_t(kFitMaxPoints) * jobs.n, fit.totalBytes,
                          cb.fit.dCap, cb.fit.dAllot, cb.fit.dFit));
    allot.resize(jobs.n);
    ENCCHK(hipMemcpyAsync(allot.data(), cb.fit.dAllot, sizeof(uint32_t) * jobs.n, hipMemcpyDeviceToHost, st));
    ENCCHK(hipMemcpyAsync(&fitRec, cb.fit.dFit, sizeof(fitRec), hipMemcpyDeviceToHost, st));
    ENCCHK(hipStreamSynchronize(st));
    for (uint32_t j = 0 ; j < jobs.n ; ++j)
    {
        const uint32_t b = fit.capBytes != nullptr ? std::min(allot[j], fit.capBytes[j]) : allot[j];
        budgetRd[j] = b >= 18 ? (static_cast<long long>(b) - 18) * 8 : -1;
        size[j] = allot[j];
    }
    if (fit.info != nullptr)
        *fit.info = fitRec;
    return DCS_OK;
}

// R3 or S5 again for group g, still resident, with the allotments as budgets; the choices are on the host after the wait
DcsStatus EncRun::fitRechoose(uint32_t g)
{
    const uint32_t j0 = groupFirst[g], n = groupFirst[g + 1] - j0;
    if (jobs.rd)
    {
        ENCCHK(hipMemcpyAsync(gb.rd.dBudget, budgetRd.data() + j0, sizeof(long long) * n, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(encRdChooseKernel, dim3(n), dim3(256), 0, st, gb.rd.dTot, cb.rd.dD0, gb.dJobs, cb.dSets, gb.rd.dBudget, gb.rd.dChoice);
        ENCCHK(hipMemcpyAsync(choiceRd.data() + j0, gb.rd.dChoice, sizeof(EncRdChoice) * n, hipMemcpyDeviceToHost, st));
    }
    else
    {
        ENCCHK(hipMemcpyAsync(gb.r93.dBudget, budgetRd.data() + j0, sizeof(long long) * n, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(enc93RdChooseKernel, dim3((n + 63) / 64), dim3(64), 0, st, gb.r93.dTot, gb.r93.dHead, cb.r93.dD0, gb.dJobs,
                           gb.r93.dBudget, n, gb.r93.dChoice);
        ENCCHK(hipMemcpyAsync(choiceRd93.data() + j0, gb.r93.dChoice, sizeof(Enc93RdChoice) * n, hipMemcpyDeviceToHost, st));
    }
    ENCCHK(hipGetLastError());
    ENCCHK(hipStreamSynchronize(st));
    sizesRd(j0, n);
    return DCS_OK;
}

// group g has chosen with its allotments: every stream is as long as its allotment (a hull vertex is a candidate's size),
// on which the output offsets already rest; then its jobs' info and infoRd
DcsStatus EncRun::fitReport(uint32_t g)
{
    for (uint32_t j = groupFirst[g] ; j < groupFirst[g + 1] ; ++j)
    {
        if (size[j] != allot[j])
        {
            dcsCtxSetError(ctx, ("job " + std::to_string(j) + ": chose " + std::to_string(size[j]) + " bytes for an allotment of "
                                 + std::to_string(allot[j])).c_str());
            return DCS_ERR_HIP;
        }
        writeInfo(j);
    }
    return DCS_OK;
}

// the record once every stream is written: sqErr is the sum of what the streams' records say
void EncRun::fitRecord()
{
    fitRec.sqErr = 0;
    for (uint32_t j = 0 ; j < jobs.n ; ++j)
        fitRec.sqErr += jobs.rd ? choiceRd[j].sumD : choiceRd93[j].sumD;
    if (jobs.fit->info != nullptr)
        *jobs.fit->info = fitRec;
}

// dcs_encode_rd_fit and dcs_encode93_rd_fit behind their parameter checks
DcsStatus encodeRdFit(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams, const DcsEncodeParams *params,
                      bool os93, const EncFit &fit, const EncOutput &to)
{
    if (fit.info != nullptr)
    {
        *fit.info = DcsEncodeRdFitInfo{};
        fit.info->totalBytes = fit.totalBytes;
        fit.info->fits = 1;
    }
    EncInput in;
    in.sampleOffsets = sampleOffsets;
    in.nStreams = nStreams;
    in.hostPcm = pcm;
    std::vector<DcsSweepJob> list(nStreams);
    for (uint32_t i = 0 ; i < nStreams ; ++i)
        list[i] = DcsSweepJob{ i, 0 };
    EncJobs js{ params, 1, list.data(), nStreams, os93 };
    js.rd = !os93;
    js.rd93 = os93;
    js.fit = &fit;
    return EncRun(ctx, in, js, to, EncSweep()).run();
}

}  // namespace

extern "C" DcsStatus dcs_encode_rd_fit(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams,
                                       const DcsEncodeParams *params, uint64_t totalBytes, const uint32_t *capBytes, uint8_t *out,
                                       uint64_t outCap, uint64_t *outOffsets, DcsEncodeInfo *info, DcsEncodeRdInfo *infoRd,
                                       DcsEncodeRdFitInfo *fit)
{
    if (ctx == nullptr || sampleOffsets == nullptr || outOffsets == nullptr || (nStreams != 0 && pcm == nullptr))
        return DCS_ERR_INVALID_ARG;
    if (!paramsValidRd(params))
    {
        dcsCtxSetError(ctx, "dcs_encode_rd_fit: formatVersion 0x9400, streamFormatType 0, 1 or -1, streamFormatSubType 0, 3 or -1, "
                            "targetBitRate 1..100 000 000 and finite parameters");
        return DCS_ERR_INVALID_ARG;
    }
    EncOutput to{ out, static_cast<size_t>(outCap), outOffsets, info, nullptr, nullptr };
    to.infoRd = infoRd;
    return encodeRdFit(ctx, pcm, sampleOffsets, nStreams, params, false, EncFit{ totalBytes, capBytes, fit }, to);
}

extern "C" DcsStatus dcs_encode93_rd_fit(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams,
                                         const DcsEncodeParams *params, uint64_t totalBytes, const uint32_t *capBytes, uint8_t *out,
                                         uint64_t outCap, uint64_t *outOffsets, DcsEncodeInfo *info, DcsEncodeRdInfo *infoRd,
                                         DcsEncodeRdFitInfo *fit)
{
    if (ctx == nullptr || sampleOffsets == nullptr || outOffsets == nullptr || (nStreams != 0 && pcm == nullptr))
        return DCS_ERR_INVALID_ARG;
    if (!paramsValid93Rd(params))
    {
        dcsCtxSetError(ctx, "dcs_encode93_rd_fit: formatVersion 0x9301 or 0x9302, streamFormatType 0 or -1 (OS93 Type 0; Type 1 is "
                            "not searched), targetBitRate 1..100 000 000 and finite parameters");
        return DCS_ERR_INVALID_ARG;
    }
    EncOutput to{ out, static_cast<size_t>(outCap), outOffsets, info, nullptr, nullptr };
    to.infoRd = infoRd;
    return encodeRdFit(ctx, pcm, sampleOffsets, nStreams, params, true, EncFit{ totalBytes, capBytes, fit }, to);
}

extern "C" DcsStatus dcs_encode_rd_allot(DcsCtx *ctx, const uint64_t *sizeBytes, const uint64_t *sqErr, const uint64_t *curveOffsets,
                                         uint32_t nJobs, uint64_t totalBytes, const uint32_t *capBytes, uint32_t *allotOut,
                                         DcsEncodeRdFitInfo *fit)
{
    if (fit == nullptr || curveOffsets == nullptr || (nJobs != 0 && (sizeBytes == nullptr || sqErr == nullptr || allotOut == nullptr)))
        return DCS_ERR_INVALID_ARG;
    const char *why = nullptr;
    for (uint32_t j = 0 ; j < nJobs && why == nullptr ; ++j)
        if (curveOffsets[j + 1] <= curveOffsets[j] || curveOffsets[j + 1] - curveOffsets[j] > kFitMaxPoints)
            why = "dcs_encode_rd_allot: a job has 1 to 168 candidates";
    const uint64_t first = curveOffsets[0], N = why == nullptr ? curveOffsets[nJobs] - first : 0;
    for (uint64_t i = 0 ; i < N && why == nullptr ; ++i)
        if (sizeBytes[first + i] > 0xFFFFFFFFull || sqErr[first + i] >= kFitMaxD)
            why = "dcs_encode_rd_allot: sizes are below 2^32 and errors below 2^62";
    if (why != nullptr)
    {
        if (ctx != nullptr)
            dcsCtxSetError(ctx, why);
        return DCS_ERR_INVALID_ARG;
    }
    if (ctx == nullptr || nJobs == 0)
    {
        fitAllotHost(sizeBytes, sqErr, curveOffsets, nJobs, totalBytes, capBytes, allotOut, fit);
        return DCS_OK;
    }
    ENCCHK(hipSetDevice(dcsCtxDevice(ctx)));
    const hipStream_t st = dcsCtxStream(ctx);
    CacheArena arena(ctx);
    std::vector<unsigned long long> off(size_t(nJobs) + 1);
    for (uint32_t j = 0 ; j <= nJobs ; ++j)
        off[j] = curveOffsets[j] - first;
    unsigned long long *dSize, *dD, *dOff;
    uint32_t *dCap = nullptr, *dAllot;
    DcsEncodeRdFitInfo *dFit;
    ENCCHK(arena.alloc(&dSize, N));
    ENCCHK(arena.alloc(&dD, N));
    ENCCHK(arena.alloc(&dOff, off.size()));
    if (capBytes != nullptr)
        ENCCHK(arena.alloc(&dCap, nJobs));
    ENCCHK(arena.alloc(&dAllot, nJobs));
    ENCCHK(arena.alloc(&dFit, 1));
    ENCCHK(hipMemcpyAsync(dSize, sizeBytes + first, sizeof(uint64_t) * N, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(dD, sqErr + first, sizeof(uint64_t) * N, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(dOff, off.data(), sizeof(unsigned long long) * off.size(), hipMemcpyHostToDevice, st));
    if (capBytes != nullptr)
        ENCCHK(hipMemcpyAsync(dCap, capBytes, sizeof(uint32_t) * nJobs, hipMemcpyHostToDevice, st));
    const DcsStatus s = fitAllotDevice(ctx, arena, dSize, dD, dOff, nJobs, static_cast<size_t>(N), totalBytes, dCap, dAllot, dFit);
    if (s != DCS_OK)
        return s;
    ENCCHK(hipMemcpyAsync(allotOut, dAllot, sizeof(uint32_t) * nJobs, hipMemcpyDeviceToHost, st));
    ENCCHK(hipMemcpyAsync(fit, dFit, sizeof(*fit), hipMemcpyDeviceToHost, st));
    ENCCHK(hipStreamSynchronize(st));
    return DCS_OK;
}
