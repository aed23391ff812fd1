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
// the driver, which launches these)

#include "dcs_encode93a.hip.h"
#include "dcs_encode_rd.h"
#include "dcs_encode93_rd.h"

// ------------------------------------------------- the host driver: families O, E and A, and EncRun (dcs_encode_run.hip.h)

#include "dcs_encode_run.hip.h"

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
    EncOneSet one(pcm, sampleOffsets, nStreams);
    return EncRun(ctx, one.in, one.jobs(&p1, true), to, EncSweep()).run();
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

// the sources of either plan, behind the check of the target: `version` the target's, bitsPerFrame its encoder's most
DcsStatus transcodePlanSources(const DcsStreamRef *src, uint32_t nStreams, uint16_t version, uint32_t flags, const DcsBudget *budget,
                               uint32_t bitsPerFrame, int32_t *actionOut, uint64_t *boundOut, std::string &why)
{
    const bool os93 = version != 0x9400;
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
        bool copy = (flags & DCS_TRANSCODE_REENCODE_ALL) == 0
                          && (v == version || (os93 && v != 0x9400 && (s.data[2] & 0x80) == 0));
        if (copy && budget != nullptr)
            copy = budgetCopies(*budget, i, s.len);
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
            boundOut[i] = copy ? static_cast<uint64_t>(s.len) : boundOf(static_cast<uint64_t>(nFrames + 1) * 240, bitsPerFrame);
    }
    return DCS_OK;
}

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
    return transcodePlanSources(src, nStreams, target->formatVersion, flags, nullptr, os93 ? kMaxBitsPerFrame93 : kMaxBitsPerFrame,
                                actionOut, boundOut, why);
}

// The same for dcs_transcode_streams_budget: a target of a searched family, and a source that would be copied is searched
// all the same where it does not keep to its own bound (budgetCopies)
DcsStatus dcsTranscodePlanBudget(const DcsStreamRef *src, uint32_t nStreams, const DcsEncodeParams *target, uint32_t flags,
                                 const DcsBudget *budget, int32_t *actionOut, uint64_t *boundOut, std::string &why)
{
    if ((nStreams != 0 && src == nullptr) || target == nullptr || (flags & ~DCS_TRANSCODE_REENCODE_ALL) != 0)
        return DCS_ERR_INVALID_ARG;
    const bool os93 = budgetOs93(target);
    const auto say = [&](const char *text) { why = text; };
    if (!searchedParams("dcs_transcode_streams_budget", target, os93, say) || !budgetValid("dcs_transcode_streams_budget", budget, say))
        return DCS_ERR_INVALID_ARG;
    return transcodePlanSources(src, nStreams, target->formatVersion, flags, budget, os93 ? kRd93MaxFrameBits : rdMaxFrameBits(),
                                actionOut, boundOut, why);
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

// the decode of transcoding, which the budget calls run their searches on (defined in the runtime's unit)
#include "dcs_transcode_decoded.h"

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

// ------------------------------------------------ existing streams to a budget (dcs_encode_budget.hip.h; no kernel)

#include "dcs_encode_budget.hip.h"

// ----------------------------------------- the rate-distortion 1994+ encoder: kernels (dcs_encode_rd.hip.h) and the R family
// (behind every other kernel of the unit, templates included: those keep their place in the code object)

#include "dcs_encode_rd.hip.h"

namespace {

bool EncRdFamily::select()
{
    choice.resize(jobs.n);
    return selectSearch(false);
}

DcsStatus EncRdFamily::allocCall()
{
    ENCCHK(s.call.alloc(&dR, 1));
    ENCCHK(s.call.alloc(&dItems, size_t(kRdItemsPerFrame) * s.F));
    ENCCHK(s.call.alloc(&dPeak, size_t(16) * in.nStreams));
    ENCCHK(s.call.alloc(&dD0, size_t(16) * in.nStreams));
    ENCCHK(s.call.alloc(&dFloor, size_t(16) * jobs.nSets));
    return DCS_OK;
}

hipError_t EncRdFamily::allocGroup()
{
    const size_t JF = static_cast<size_t>(s.groupFrames), NJ = s.groupJobs;
    HIPTRY(s.group.alloc(&dTot, size_t(kRdRowsPerJob) * NJ));
    HIPTRY(s.group.alloc(&dChoice, NJ));
    HIPTRY(s.group.alloc(&dBudget, NJ));
    HIPTRY(s.group.alloc(&dSurv, 256 * JF));
    HIPTRY(s.group.alloc(&dEnd, 16 * NJ));
    HIPTRY(s.group.alloc(&dCodes, 16 * JF));
    HIPTRY(s.group.alloc(&dBits, JF));
    return hipSuccess;
}

// R1 over every stream-frame; the budgets
DcsStatus EncRdFamily::analyse()
{
    floorRd.resize(size_t(16) * jobs.nSets);
    for (uint32_t k = 0 ; k < jobs.nSets ; ++k)
        floorERd(jobs.sets[k].maximumQuantizationError, floorRd.data() + size_t(16) * k);
    budgets();
    ENCCHK(hipMemcpyAsync(dR, &encTabsRd(), sizeof(EncRdTabs), hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(dFloor, floorRd.data(), sizeof(unsigned long long) * floorRd.size(), hipMemcpyHostToDevice, st));
    ENCCHK(hipMemsetAsync(dPeak, 0, sizeof(uint32_t) * 16 * in.nStreams, st));
    ENCCHK(hipMemsetAsync(dD0, 0, sizeof(unsigned long long) * 16 * in.nStreams, st));
    hipLaunchKernelGGL(encRdItemKernel, dim3(s.F), dim3(256), 0, st, cb.dT, dR, cb.dSpec, cb.dFS, dItems, dPeak, dD0);
    return DCS_OK;
}

// R2 and R3 for the n jobs of a group from job j0; the choices are on the host after the group's wait
DcsStatus EncRdFamily::runGroup(uint32_t j0, uint32_t n, uint32_t)
{
    ENCTRY(uploadBudgets(j0, n));
    hipLaunchKernelGGL(encRdTrellisKernel<false>, dim3(kRdRowsPerJob / 16 * n), dim3(256), 0, st, cb.dT, dR, dItems, dPeak,
                       dFloor, gb.dJobs, cb.dSets, dTot, static_cast<const EncRdChoice *>(nullptr),
                       static_cast<uint8_t *>(nullptr), static_cast<uint8_t *>(nullptr));
    launchChoose(n);
    return fetchChoice(j0, n);
}

void EncRdFamily::launchChoose(uint32_t n)
{
    hipLaunchKernelGGL(encRdChooseKernel, dim3(n), dim3(256), 0, st, dTot, dD0, gb.dJobs, cb.dSets, dBudget, dChoice);
}

DcsStatus EncRdFamily::fetchChoice(uint32_t j0, uint32_t n)
{
    ENCCHK(hipMemcpyAsync(choice.data() + j0, dChoice, sizeof(EncRdChoice) * n, hipMemcpyDeviceToHost, st));
    return DCS_OK;
}

// a job of the R family: the candidate of CloseStream's list it chose, its header's band count, 18 bytes and the frames' bits
void EncRdFamily::sizeJobs(uint32_t j0, uint32_t n)
{
    for (uint32_t j = j0 ; j < j0 + n ; ++j)
    {
        s.win[j] = choice[j].variant;
        s.keep[j] = choice[j].numBands;
        s.size[j] = 18 + (choice[j].frameBits + 7) / 8;
    }
}

// R4 to R6 for the resident group: the chosen chains with their survivors, the frames' bits and offsets, header and pack
DcsStatus EncRdFamily::packGroup(uint32_t n, uint32_t JF)
{
    ENCCHK(hipMemsetAsync(dCodes, 0, size_t(16) * JF, st));
    hipLaunchKernelGGL(encRdTrellisKernel<true>, dim3(n), dim3(256), 0, st, cb.dT, dR, dItems, dPeak, dFloor,
                       gb.dJobs, cb.dSets, static_cast<EncRdTot *>(nullptr), dChoice, dSurv, dEnd);
    hipLaunchKernelGGL(encRdBackKernel, dim3((16 * n + 63) / 64), dim3(64), 0, st, gb.dJobs, dChoice, dSurv, dEnd, n, dCodes);
    hipLaunchKernelGGL(encRdBitsKernel, dim3((JF + 63) / 64), dim3(64), 0, st, cb.dT, dItems, dPeak, gb.dFJ, gb.dJobs,
                       dChoice, dCodes, JF, dBits);
    hipLaunchKernelGGL(encRdOffsetKernel, dim3(n), dim3(256), 0, st, gb.dJobs, dBits, gb.dFrameOff);
    hipLaunchKernelGGL(encRdHeadKernel, dim3((n + 63) / 64), dim3(64), 0, st, cb.dT, dPeak, gb.dJobs, dChoice, gb.dOutOff, n, s.dW);
    hipLaunchKernelGGL(encRdPackKernel, dim3(JF), dim3(64), 0, st, cb.dT, dR, cb.dSpec, dItems, dPeak, gb.dFJ, gb.dJobs,
                       dChoice, dCodes, gb.dFrameOff, gb.dOutOff, s.dW);
    return DCS_OK;
}

void EncRdFamily::writeInfo(uint32_t j)
{
    const EncRdChoice &c = choice[j];
    if (to.infoRd != nullptr)
        to.infoRd[j] = DcsEncodeRdInfo{ kCandType[c.variant], kCandSub[c.variant], c.ladderIndex, c.numBands, c.frameBits,
                                        static_cast<uint64_t>(std::max<long long>(budgetRd[j], 0)), c.sumD, c.fits, 0 };
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
    return encodeSearched(ctx, "dcs_encode_rd_streams", pcm, sampleOffsets, nStreams, params, false, budgetBytes, nullptr, out, outCap,
                          outOffsets, info, infoRd);
}

// --------------------------------- the rate-distortion OS93 Type-0 encoder: kernels (dcs_encode93_rd.hip.h) and the S family
// (behind every other kernel of the unit once more)

#include "dcs_encode93_rd.hip.h"

namespace {

bool Enc93RdFamily::select()
{
    choice.resize(jobs.n);
    return selectSearch(true);
}

DcsStatus Enc93RdFamily::allocCall()
{
    ENCCHK(s.call.alloc(&dR, 1));
    ENCCHK(s.call.alloc(&dItems, size_t(kRd93ItemsPerFrame) * s.F));
    ENCCHK(s.call.alloc(&dRecs, size_t(kRd93RecsPerFrame) * s.F));
    ENCCHK(s.call.alloc(&dD0, size_t(16) * in.nStreams));
    ENCCHK(s.call.alloc(&dFloor, jobs.nSets));
    return DCS_OK;
}

hipError_t Enc93RdFamily::allocGroup()
{
    const size_t JF = static_cast<size_t>(s.groupFrames), NJ = s.groupJobs;
    HIPTRY(s.group.alloc(&dProxyJ, size_t(kRd93ProxyPerJob) * NJ));
    HIPTRY(s.group.alloc(&dProxyB, size_t(kRd93ProxyPerJob) * NJ));
    HIPTRY(s.group.alloc(&dHead, size_t(kRdKL) * NJ));
    HIPTRY(s.group.alloc(&dTot, size_t(kRdKL) * NJ));
    HIPTRY(s.group.alloc(&dChoice, NJ));
    HIPTRY(s.group.alloc(&dBudget, NJ));
    HIPTRY(s.group.alloc(&dCodes, 16 * JF));
    HIPTRY(s.group.alloc(&dBits, JF));
    return hipSuccess;
}

// S1 over every stream-frame; the budgets
DcsStatus Enc93RdFamily::analyse()
{
    const uint16_t version = jobs.sets[0].formatVersion;        // (one per call: dcs_encode93_rd_streams has one set)
    floorRd.resize(jobs.nSets);
    for (uint32_t k = 0 ; k < jobs.nSets ; ++k)
        floorRd[k] = floorE93Rd(jobs.sets[k].maximumQuantizationError);
    budgets();
    ENCCHK(hipMemcpyAsync(dR, &encTabs93Rd(version), sizeof(EncRdTabs), hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(dFloor, floorRd.data(), sizeof(unsigned long long) * floorRd.size(), hipMemcpyHostToDevice, st));
    ENCCHK(hipMemsetAsync(dD0, 0, sizeof(unsigned long long) * 16 * in.nStreams, st));
    hipLaunchKernelGGL(enc93RdItemKernel, dim3(s.F), dim3(256), 0, st, cb.dT, dR, rd93M0(version), cb.dSpec, cb.dFS, dItems, dRecs, dD0);
    return DCS_OK;
}

// S2 to S5 for the n jobs (JF job-frames) of a group from job j0; the choices are on the host after the group's wait
DcsStatus Enc93RdFamily::runGroup(uint32_t j0, uint32_t n, uint32_t JF)
{
    const uint32_t chunks = (JF + kRd93ChunkFrames - 1) / kRd93ChunkFrames;
    ENCTRY(uploadBudgets(j0, n));
    ENCCHK(hipMemsetAsync(dProxyJ, 0, sizeof(unsigned long long) * kRd93ProxyPerJob * n, st));
    ENCCHK(hipMemsetAsync(dProxyB, 0, sizeof(uint32_t) * kRd93ProxyPerJob * n, st));
    ENCCHK(hipMemsetAsync(dTot, 0, sizeof(Enc93RdTot) * kRdKL * n, st));
    hipLaunchKernelGGL(enc93RdProxyKernel, dim3(kRd93ProxyPerJob / 256, chunks), dim3(256), 0, st, dR, dItems, dFloor,
                       gb.dFJ, gb.dJobs, JF, dProxyJ, dProxyB);
    hipLaunchKernelGGL(enc93RdHeaderKernel, dim3(n), dim3(64), 0, st, dProxyJ, dProxyB, dD0, gb.dJobs, dHead);
    hipLaunchKernelGGL(enc93RdTrellisKernel<false>, dim3(chunks, kRdKL), dim3(256), 0, st, dR, dItems, dRecs,
                       dFloor, gb.dFJ, gb.dJobs, JF, dHead, static_cast<const Enc93RdChoice *>(nullptr), dTot,
                       static_cast<uint8_t *>(nullptr), static_cast<uint32_t *>(nullptr));
    launchChoose(n);
    return fetchChoice(j0, n);
}

void Enc93RdFamily::launchChoose(uint32_t n)
{
    hipLaunchKernelGGL(enc93RdChooseKernel, dim3((n + 63) / 64), dim3(64), 0, st, dTot, dHead, dD0, gb.dJobs, dBudget, n, dChoice);
}

DcsStatus Enc93RdFamily::fetchChoice(uint32_t j0, uint32_t n)
{
    ENCCHK(hipMemcpyAsync(choice.data() + j0, dChoice, sizeof(Enc93RdChoice) * n, hipMemcpyDeviceToHost, st));
    return DCS_OK;
}

// a job of the S family: Type 0, its header's band count, 18 bytes and the frames' bits
void Enc93RdFamily::sizeJobs(uint32_t j0, uint32_t n)
{
    for (uint32_t j = j0 ; j < j0 + n ; ++j)
    {
        s.win[j] = 0;
        s.keep[j] = choice[j].numBands;
        s.size[j] = 18 + (choice[j].frameBits + 7) / 8;
    }
}

// S6 to S8 for the resident group: the chosen lambda's trellises with their paths, the frames' offsets, header and pack
DcsStatus Enc93RdFamily::packGroup(uint32_t n, uint32_t JF)
{
    const uint32_t chunks = (JF + kRd93ChunkFrames - 1) / kRd93ChunkFrames;
    const uint32_t m0 = rd93M0(jobs.sets[0].formatVersion);
    hipLaunchKernelGGL(enc93RdTrellisKernel<true>, dim3(chunks), dim3(256), 0, st, dR, dItems, dRecs, dFloor,
                       gb.dFJ, gb.dJobs, JF, static_cast<const Enc93RdHead *>(nullptr), dChoice, static_cast<Enc93RdTot *>(nullptr),
                       dCodes, dBits);
    hipLaunchKernelGGL(encRdOffsetKernel, dim3(n), dim3(256), 0, st, gb.dJobs, dBits, gb.dFrameOff);
    hipLaunchKernelGGL(enc93RdHeadKernel, dim3((n + 63) / 64), dim3(64), 0, st, gb.dJobs, dChoice, gb.dOutOff, n, s.dW);
    hipLaunchKernelGGL(enc93RdPackKernel, dim3(JF), dim3(64), 0, st, cb.dT, dR, m0, cb.dSpec, dRecs, gb.dFJ, gb.dJobs,
                       dChoice, dCodes, gb.dFrameOff, gb.dOutOff, s.dW);
    return DCS_OK;
}

void Enc93RdFamily::writeInfo(uint32_t j)
{
    const Enc93RdChoice &c = choice[j];
    if (to.infoRd != nullptr)
        to.infoRd[j] = DcsEncodeRdInfo{ 0, 0, c.ladderIndex, c.numBands, c.frameBits,
                                        static_cast<uint64_t>(std::max<long long>(budgetRd[j], 0)), c.sumD, c.fits, 0 };
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
    return encodeSearched(ctx, "dcs_encode93_rd_streams", pcm, sampleOffsets, nStreams, params, true, budgetBytes, nullptr, out, outCap,
                          outOffsets, info, infoRd);
}

// --------------------------------------- a set of streams to one byte budget: kernels (dcs_encode_rd_fit.hip.h) and EncFitRun
// (behind every other kernel of the unit once more)

#include "dcs_encode_rd_fit.hip.h"

namespace {

DcsStatus EncFitRun::allocCall()
{
    ENCCHK(s.call.alloc(&dCurveSize, size_t(kFitMaxPoints) * jobs.n));
    ENCCHK(s.call.alloc(&dCurveD, size_t(kFitMaxPoints) * jobs.n));
    ENCCHK(s.call.alloc(&dOff, size_t(jobs.n) + 1));
    if (jobs.fit->capBytes != nullptr)
        ENCCHK(s.call.alloc(&dCap, jobs.n));
    ENCCHK(s.call.alloc(&dAllot, jobs.n));
    ENCCHK(s.call.alloc(&dFit, 1));
    return DCS_OK;
}

// F1 behind R2 or S4 of the resident group (n jobs from job j0): its jobs' candidates into the call's curve table
void EncRdFamily::launchCurves(uint32_t n, unsigned long long *dSize, unsigned long long *dD)
{
    hipLaunchKernelGGL(encRdCurveKernel, dim3(n), dim3(256), 0, st, dTot, dD0, gb.dJobs, cb.dSets, dSize, dD);
}

void Enc93RdFamily::launchCurves(uint32_t n, unsigned long long *dSize, unsigned long long *dD)
{
    hipLaunchKernelGGL(enc93RdCurveKernel, dim3((n * kFitMaxPoints + 63) / 64), dim3(64), 0, st, dTot, dHead, dD0, gb.dJobs, n, dSize, dD);
}

void EncFitRun::launchCurves(uint32_t j0, uint32_t n)
{
    s.searched->launchCurves(n, dCurveSize + size_t(kFitMaxPoints) * j0, dCurveD + size_t(kFitMaxPoints) * j0);
}

// F2 to F4 over all jobs, and a wait: the allotments and the record are on the host after it, the curves never.  A job's
// budget is its allotment, or its cap where even its smallest candidate is beyond that (a pinned job: fits = 0).
DcsStatus EncFitRun::allot()
{
    const EncFit &fit = *jobs.fit;
    std::vector<unsigned long long> off(size_t(jobs.n) + 1);
    for (uint32_t j = 0 ; j <= jobs.n ; ++j)
        off[j] = static_cast<unsigned long long>(kFitMaxPoints) * j;
    ENCCHK(hipMemcpyAsync(dOff, off.data(), sizeof(unsigned long long) * off.size(), hipMemcpyHostToDevice, st));
    if (fit.capBytes != nullptr)
        ENCCHK(hipMemcpyAsync(dCap, fit.capBytes, sizeof(uint32_t) * jobs.n, hipMemcpyHostToDevice, st));
    ENCTRY(fitAllotDevice(ctx, s.call, dCurveSize, dCurveD, dOff, jobs.n, size_t(kFitMaxPoints) * jobs.n, fit.totalBytes, dCap, dAllot, dFit));
    allotBytes.resize(jobs.n);
    ENCCHK(hipMemcpyAsync(allotBytes.data(), dAllot, sizeof(uint32_t) * jobs.n, hipMemcpyDeviceToHost, st));
    ENCCHK(hipMemcpyAsync(&rec, dFit, sizeof(rec), hipMemcpyDeviceToHost, st));
    ENCCHK(hipStreamSynchronize(st));
    for (uint32_t j = 0 ; j < jobs.n ; ++j)
    {
        const uint32_t b = fit.capBytes != nullptr ? std::min(allotBytes[j], fit.capBytes[j]) : allotBytes[j];
        s.searched->budgetRd[j] = b >= 18 ? (static_cast<long long>(b) - 18) * 8 : -1;
        s.size[j] = allotBytes[j];
    }
    if (fit.info != nullptr)
        *fit.info = rec;
    allotted = true;
    return DCS_OK;
}

// R3 or S5 again for group g, still resident, with the allotments as budgets; the choices are on the host after the wait
DcsStatus EncFitRun::rechoose(uint32_t g)
{
    const uint32_t j0 = s.groupFirst[g], n = s.groupFirst[g + 1] - j0;
    ENCTRY(s.searched->chooseAgain(j0, n));
    ENCCHK(hipGetLastError());
    ENCCHK(hipStreamSynchronize(st));
    s.searched->sizeJobs(j0, n);
    return DCS_OK;
}

// job j's group has chosen with its allotments: its stream is as long as its allotment (a hull vertex is a candidate's
// size), on which the output offsets already rest
DcsStatus EncFitRun::report(uint32_t j)
{
    if (s.size[j] != allotBytes[j])
    {
        dcsCtxSetError(ctx, ("job " + std::to_string(j) + ": chose " + std::to_string(s.size[j]) + " bytes for an allotment of "
                             + std::to_string(allotBytes[j])).c_str());
        return DCS_ERR_HIP;
    }
    return DCS_OK;
}

// the record once every stream is written: sqErr is the sum of what the streams' records say
void EncFitRun::record()
{
    rec.sqErr = 0;
    for (uint32_t j = 0 ; j < jobs.n ; ++j)
        rec.sqErr += s.searched->sumD(j);
    if (jobs.fit->info != nullptr)
        *jobs.fit->info = rec;
}

}  // namespace

extern "C" DcsStatus dcs_encode_rd_fit(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams,
                                       const DcsEncodeParams *params, uint64_t totalBytes, const uint32_t *capBytes, uint8_t *out,
                                       uint64_t outCap, uint64_t *outOffsets, DcsEncodeInfo *info, DcsEncodeRdInfo *infoRd,
                                       DcsEncodeRdFitInfo *fit)
{
    const EncFit f{ totalBytes, capBytes, fit };
    return encodeSearched(ctx, "dcs_encode_rd_fit", pcm, sampleOffsets, nStreams, params, false, nullptr, &f, out, outCap, outOffsets,
                          info, infoRd);
}

extern "C" DcsStatus dcs_encode93_rd_fit(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams,
                                         const DcsEncodeParams *params, uint64_t totalBytes, const uint32_t *capBytes, uint8_t *out,
                                         uint64_t outCap, uint64_t *outOffsets, DcsEncodeInfo *info, DcsEncodeRdInfo *infoRd,
                                         DcsEncodeRdFitInfo *fit)
{
    const EncFit f{ totalBytes, capBytes, fit };
    return encodeSearched(ctx, "dcs_encode93_rd_fit", pcm, sampleOffsets, nStreams, params, true, nullptr, &f, out, outCap, outOffsets,
                          info, infoRd);
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

// ------------------------------------------ the join of dcs_encode_files_budget's one input (dcs_encode_join.hip.h)
// (behind every other kernel of the unit once more)

#include "dcs_encode_join.hip.h"
