// dcs_encode.hip -- the 1994+ DCS encoder on the GPU: PCM at 31 250 Hz in, streams byte-identical to the reference's
// DCSEncoder out (DCSEncoder.cpp: TransformFrame :1001-1069, DFTAlgorithmOrig :1218-1358, DualFFT :1360-1500,
// Frame::Frame :2535-2571, CloseStream :717-850, CompressStream :859-960, CompressFrame94 :1623-2050, BitWriter :2573-2704).
//
// A translation unit of its own because of the floating-point contract below: the reference is plain x86-64 code that
// rounds every multiply and add separately, and byte-exact streams need the same here, in device AND host code.  The
// decoder's kernels keep the library's default contraction.  Division stays a real, correctly rounded division (hipcc's
// default for f32), f32 denormals stay on, and every sum that the reference accumulates serially is accumulated serially in
// its order: parallelism goes across frames, bands, candidate codes and streams, never inside one sum.
//
//   E1 encAnalyseKernel   one wavefront per frame: window, bit-reversed load, 6 radix-2 stages, the odd-coefficient pass,
//                         the folds, the twiddle, the sign fix (each stage element-parallel over LDS); per-band power / lo / hi
//   E2 encStreamKernel    one wavefront per stream: powerSum in frame order and the range, then the header of each layout
//   E3 encSearchKernel    one thread per (frame, band, layout, pre-adjust): the 15 candidate codes' error sums, the best code
//                         with and without code 15 (the only things the previous frame's code can change)
//   E4 encChainKernel     one lane per (stream, layout, band): the walk over frames through those per-frame choices
//   E5 encBitsKernel / encSizeKernel / encHeadKernel / encPackKernel: bits per band and frame, stream sizes, the winner,
//                         frame bit offsets, and the bits themselves OR-ed into a zeroed buffer of big-endian words
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <stdio.h>
#include <string>
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
// copied to the device per call.
struct EncTabs
{
    float window[16], twiddle[128], fft[896], bandNorm[16];
    int32_t share[16], count[16], first[16], scale[64];
    uint8_t preAdj[2][16];             // sub-type 0, sub-type 3
    uint8_t xw[3][16], xa[3][16];      // Type 1 band-type code -> bit width / scale adjust, for bands 0-2, 3-5, 6-15
    uint32_t hdrCode[31];              // frame-header band-type delta codes, index delta + 16
    uint8_t hdrLen[31];
    uint16_t smpCode[7][64];           // sample codebooks 1..6, index = stored value
    uint8_t smpLen[7][64];
    uint16_t dzCode[7];                // the codebooks' two-zeros code
    uint8_t dzLen[7];
};

float fromBits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }

EncTabs buildTabs()
{
    EncTabs t;
    memset(&t, 0, sizeof(t));
    for (int i = 0 ; i < 16 ; ++i) t.window[i] = fromBits(kEncWindowBits[i]);
    for (int i = 0 ; i < 128 ; ++i) t.twiddle[i] = fromBits(kEncTwiddleBits[i]);
    for (int i = 0 ; i < 896 ; ++i) t.fft[i] = fromBits(kEncFftBits[i]);
    for (int b = 0, first = 0 ; b < 16 ; ++b)
    {
        t.bandNorm[b] = fromBits(kEncBandNormBits[b]);
        t.share[b] = kEncBandShare[b];
        t.count[b] = kBandCount94[b];
        t.first[b] = first;
        first += kBandCount94[b];
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
    return t;
}

const EncTabs &encTabs() { static const EncTabs t = buildTabs(); return t; }

// CloseStream's band cutoff and CompressStream's header (the rate model), for one layout.  The reference computes
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
        shareNorm += static_cast<float>(T.share[i] * T.count[i]);
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
        if (typ == 1)
        {
            const int adjust = (b < 3 ? 0x0d : 0x17) + (sub == 0 ? 1 : 3);
            code = code > adjust ? code - adjust : 0;
        }
        hdr[b] = static_cast<uint8_t>(code);
    }
    if (typ != 0) hdr[0] |= 0x80;
    hdr[1] |= static_cast<uint8_t>((sub & 2) << 6);
    hdr[2] |= static_cast<uint8_t>((sub & 1) << 7);
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

struct EncStream { uint64_t sampleOff; uint32_t nSamples, firstFrame, nFrames, pad; };

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

// E1: one wavefront per frame, four frames per block
__global__ __launch_bounds__(256) void encAnalyseKernel(const EncTabs *__restrict__ Tp, const float *__restrict__ pcm,
    const EncStream *__restrict__ streams, const uint32_t *__restrict__ frameStream, uint32_t F, float *__restrict__ spec,
    float *__restrict__ pw, float *__restrict__ flo, float *__restrict__ fhi, uint32_t *__restrict__ bad)
{
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
            float x = (idx >= 0 && idx < static_cast<int64_t>(s.nSamples)) ? pcm[s.sampleOff + static_cast<uint64_t>(idx)] : 0.0f;
            if (!(fabsf(x) <= 1.0f))
                isBad = true;
            if (i < 16) x *= T.window[i];
            else if (i >= 240) x *= T.window[255 - i];
            b[(rev7(i >> 1) << 1) | (i & 1)] = x;
        }
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

// E2: one wavefront per stream
__global__ __launch_bounds__(64) void encStreamKernel(const EncTabs *__restrict__ Tp, const EncStream *__restrict__ streams,
    const float *__restrict__ pw, const float *__restrict__ flo, const float *__restrict__ fhi, float cutoff, int rate,
    uint32_t vmask, uint8_t *__restrict__ hdrOut, int32_t *__restrict__ keepOut)
{
    __shared__ float sPs[16], sLo[16], sHi[16];
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
        sPs[l] = ps; sLo[l] = lo; sHi[l] = hi;
    }
    __syncthreads();
    if (l < 3 && ((vmask >> l) & 1))
    {
        uint8_t hdr[16];
        int bits[16], keep;
        encHeader(*Tp, sPs, sLo, sHi, cutoff, rate, l == 0 ? 0 : 1, l == 2 ? 3 : 0, hdr, &keep, bits);
        for (int b = 0 ; b < 16 ; ++b)
            hdrOut[(static_cast<size_t>(blockIdx.x) * 3 + l) * 16 + b] = hdr[b];
        keepOut[blockIdx.x] = keep;                         // (the same for every layout)
    }
}

// E3: one block per frame, one thread per (band, slot)
__global__ __launch_bounds__(128) void encSearchKernel(const EncTabs *__restrict__ Tp, const float *__restrict__ spec,
    const float *__restrict__ flo, const float *__restrict__ fhi, const uint32_t *__restrict__ frameStream,
    const uint8_t *__restrict__ hdr, const int32_t *__restrict__ keepArr, uint32_t vmask, float minDR, float maxQE,
    uint8_t *__restrict__ best)
{
    const EncTabs &T = *Tp;
    __shared__ float smp[256];
    const uint32_t f = blockIdx.x;
    const int t = threadIdx.x;
    smp[t] = spec[static_cast<size_t>(f) * 256 + t];
    smp[t + 128] = spec[static_cast<size_t>(f) * 256 + 128 + t];
    __syncthreads();
    const int band = t >> 3, slot = t & 7;
    const uint32_t si = frameStream[f];
    if (band >= keepArr[si])
        return;
    const int v = slot == 0 ? 0 : slot < 3 ? 1 : 2;
    const int pre = slot == 0 ? 0 : slot < 3 ? slot - 1 : slot - 3;
    if (!((vmask >> v) & 1) || (band >= 3 && pre != 0))
        return;
    const size_t fb = static_cast<size_t>(f) * 16 + band;
    uint8_t out = 0;
    if (!(fhi[fb] - flo[fb] < minDR))
    {
        const int n = T.count[band];
        const float errMax = (maxQE * maxQE) * static_cast<float>(n);
        out = encSearch(T, smp + T.first[band], n, v == 0 ? 0 : 1, band, hdr[(static_cast<size_t>(si) * 3 + v) * 16 + band] & 0x3f, pre, errMax);
    }
    best[fb * 8 + slot] = out;
}

// E4: one block per stream, one lane per (layout, band): the band-type codes, frame after frame
__global__ __launch_bounds__(64) void encChainKernel(const EncTabs *__restrict__ Tp, const EncStream *__restrict__ streams,
    const int32_t *__restrict__ keepArr, uint32_t vmask, uint32_t F, const uint64_t *__restrict__ best, uint8_t *__restrict__ codes)
{
    const EncTabs &T = *Tp;
    const EncStream s = streams[blockIdx.x];
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

// E5a: one block per frame, one lane per (layout, band): header-code and sample bits
__global__ __launch_bounds__(64) void encBitsKernel(const EncTabs *__restrict__ Tp, const float *__restrict__ spec,
    const EncStream *__restrict__ streams, const uint32_t *__restrict__ frameStream, const uint8_t *__restrict__ hdr,
    const int32_t *__restrict__ keepArr, uint32_t vmask, uint32_t F, const uint8_t *__restrict__ codes,
    uint8_t *__restrict__ hdrBits, uint16_t *__restrict__ smpBits, uint32_t *__restrict__ frameBits)
{
    const EncTabs &T = *Tp;
    __shared__ float smp[256];
    __shared__ uint32_t fb[3][16];
    const uint32_t f = blockIdx.x;
    const int l = threadIdx.x;
    for (int q = 0 ; q < 4 ; ++q)
        smp[l + 64 * q] = spec[static_cast<size_t>(f) * 256 + l + 64 * q];
    __syncthreads();
    const int v = l >> 4, band = l & 15;
    const uint32_t si = frameStream[f];
    uint32_t hb = 0, sb = 0;
    if (v < 3 && ((vmask >> v) & 1) && band < keepArr[si])
    {
        const size_t at = (static_cast<size_t>(v) * F + f) * 16 + band;
        const int code = codes[at];
        const int old = f == streams[si].firstFrame ? 0 : codes[at - 16];
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

// E5b: one block per stream: sizes of the layouts, the winner (the first strictly smallest, CloseStream :805), and the
// exclusive scan of the winner's frame bits
__global__ __launch_bounds__(256) void encSizeKernel(const EncStream *__restrict__ streams, uint32_t F, uint32_t cmask,
    const uint32_t *__restrict__ frameBits, int32_t *__restrict__ winOut, uint64_t *__restrict__ sizeOut, uint32_t *__restrict__ frameOff)
{
    __shared__ uint64_t red[3][256];
    __shared__ uint32_t scan[256];
    __shared__ int sWin;
    __shared__ uint32_t carry;
    const EncStream s = streams[blockIdx.x];
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

// E5c: the 2-byte frame count and the 16-byte header of each stream's winner
__global__ __launch_bounds__(64) void encHeadKernel(const EncStream *__restrict__ streams, const uint8_t *__restrict__ hdr,
    const int32_t *__restrict__ win, const uint64_t *__restrict__ outOff, uint32_t *__restrict__ W)
{
    const uint32_t si = blockIdx.x;
    const int k = threadIdx.x;
    if (k >= 18)
        return;
    const int c = win[si], v = c < 2 ? 0 : c - 1;
    const uint32_t nF = streams[si].nFrames;
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

// E5d: four frames per block, one lane per band: the winner's header codes and samples
__global__ __launch_bounds__(64) void encPackKernel(const EncTabs *__restrict__ Tp, const float *__restrict__ spec,
    const EncStream *__restrict__ streams, const uint32_t *__restrict__ frameStream, const uint8_t *__restrict__ hdr,
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
        smp[idx >> 8][idx & 255] = ff < F ? spec[static_cast<size_t>(ff) * 256 + (idx & 255)] : 0.0f;
    }
    __syncthreads();
    const uint32_t f = blockIdx.x * 4 + (l >> 4);
    const int band = l & 15;
    if (f >= F)
        return;
    const uint32_t si = frameStream[f];
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
    const int old = f == streams[si].firstFrame ? 0 : codes[row - 16 + band];
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

bool paramsValid(const DcsEncodeParams *p)
{
    return p != nullptr && p->formatVersion == 0x9400 && p->streamFormatType >= -1 && p->streamFormatType <= 1
        && (p->streamFormatSubType == -1 || p->streamFormatSubType == 0 || p->streamFormatSubType == 3)
        && p->targetBitRate >= 1 && p->targetBitRate <= 100000000 && isfinite(p->powerBandCutoff)
        && isfinite(p->minimumDynamicRange) && isfinite(p->maximumQuantizationError);
}

const uint32_t kMaxBitsPerFrame = 16 * 23 + 255 * 15;      // every band at its longest header code and widest samples

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
    const uint64_t nFrames = (nSamples + 239) / 240;
    if (nFrames == 0 || nFrames > 65535)
        return 0;
    return static_cast<size_t>(18 + (nFrames * kMaxBitsPerFrame + 7) / 8);
}

extern "C" DcsStatus dcs_encode_header(const float *powerSum, const float *lo, const float *hi, const DcsEncodeParams *params,
                                       int formatType, int formatSubType, uint8_t *headerOut, int32_t *bandsToKeepOut, int32_t *bitsPerBandOut)
{
    if (powerSum == nullptr || lo == nullptr || hi == nullptr || headerOut == nullptr || !paramsValid(params)
        || (formatType != 0 && formatType != 1) || (formatSubType != 0 && formatSubType != 3))
        return DCS_ERR_INVALID_ARG;
    int bits[16], keep;
    encHeader(encTabs(), powerSum, lo, hi, params->powerBandCutoff, params->targetBitRate, formatType, formatSubType, headerOut, &keep, bits);
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

extern "C" DcsStatus dcs_encode_streams(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams,
                                        const DcsEncodeParams *params, uint8_t *out, size_t outCap, uint64_t *outOffsets,
                                        DcsEncodeInfo *info)
{
    if (ctx == nullptr || sampleOffsets == nullptr || outOffsets == nullptr || !paramsValid(params) || (nStreams != 0 && pcm == nullptr))
        return DCS_ERR_INVALID_ARG;
    std::vector<EncStream> hs(nStreams);
    std::vector<uint32_t> frameStream;
    uint32_t F = 0;
    for (uint32_t i = 0 ; i < nStreams ; ++i)
    {
        if (sampleOffsets[i + 1] <= sampleOffsets[i])
        {
            dcsCtxSetError(ctx, ("stream " + std::to_string(i) + ": empty").c_str());
            return DCS_ERR_INVALID_ARG;
        }
        const uint64_t n = sampleOffsets[i + 1] - sampleOffsets[i];
        const uint64_t nF = (n + 239) / 240;
        if (nF > 65535)
        {
            dcsCtxSetError(ctx, ("stream " + std::to_string(i) + ": more than 65 535 frames").c_str());
            return DCS_ERR_INVALID_ARG;
        }
        hs[i] = EncStream{ sampleOffsets[i] - sampleOffsets[0], static_cast<uint32_t>(n), F, static_cast<uint32_t>(nF), 0 };
        frameStream.insert(frameStream.end(), static_cast<size_t>(nF), i);
        F += static_cast<uint32_t>(nF);
    }
    if (nStreams == 0)
    {
        outOffsets[0] = 0;
        return DCS_OK;
    }
    const int typ = params->streamFormatType, sub = params->streamFormatSubType;
    uint32_t cmask = 0;                 // candidates in CloseStream's order (0,0), (0,3), (1,0), (1,3)
    const int ct[4] = { 0, 0, 1, 1 }, cs[4] = { 0, 3, 0, 3 };
    for (int c = 0 ; c < 4 ; ++c)
        if ((typ < 0 || typ == ct[c]) && (sub < 0 || sub == cs[c]))
            cmask |= 1u << c;
    const uint32_t vmask = ((cmask & 3) ? 1u : 0u) | ((cmask & 4) ? 2u : 0u) | ((cmask & 8) ? 4u : 0u);
    const uint64_t nSamples = sampleOffsets[nStreams] - sampleOffsets[0];

    const hipStream_t st = dcsCtxStream(ctx);
    std::vector<CacheBuf> held;
    auto alloc = [&](void **p, size_t bytes) -> hipError_t {
        held.emplace_back();
        const hipError_t e = held.back().alloc(ctx, false, (bytes + 255) & ~size_t(255));
        *p = held.back().as();
        return e;
    };
    EncTabs *dT; float *dPcm, *dSpec, *dPw, *dLo, *dHi; EncStream *dStr; uint32_t *dFS, *dBad, *dFrameBits, *dFrameOff, *dW;
    uint8_t *dHdr, *dBest, *dCodes, *dHdrBits; uint16_t *dSmpBits; int32_t *dKeep, *dWin; uint64_t *dSize, *dOutOff;
    std::vector<int32_t> win(nStreams), keep(nStreams);
    std::vector<uint64_t> size(nStreams);
    std::vector<uint32_t> bad(nStreams);
    DcsStatus status = [&]() -> DcsStatus {
        ENCCHK(hipSetDevice(dcsCtxDevice(ctx)));
        ENCCHK(alloc(reinterpret_cast<void **>(&dT), sizeof(EncTabs)));
        ENCCHK(alloc(reinterpret_cast<void **>(&dPcm), sizeof(float) * nSamples));
        ENCCHK(alloc(reinterpret_cast<void **>(&dStr), sizeof(EncStream) * nStreams));
        ENCCHK(alloc(reinterpret_cast<void **>(&dFS), sizeof(uint32_t) * F));
        ENCCHK(alloc(reinterpret_cast<void **>(&dSpec), sizeof(float) * 256 * F));
        ENCCHK(alloc(reinterpret_cast<void **>(&dPw), sizeof(float) * 16 * F));
        ENCCHK(alloc(reinterpret_cast<void **>(&dLo), sizeof(float) * 16 * F));
        ENCCHK(alloc(reinterpret_cast<void **>(&dHi), sizeof(float) * 16 * F));
        ENCCHK(alloc(reinterpret_cast<void **>(&dBad), sizeof(uint32_t) * nStreams));
        ENCCHK(alloc(reinterpret_cast<void **>(&dHdr), 48 * size_t(nStreams)));
        ENCCHK(alloc(reinterpret_cast<void **>(&dKeep), sizeof(int32_t) * nStreams));
        ENCCHK(alloc(reinterpret_cast<void **>(&dBest), size_t(128) * F));
        ENCCHK(alloc(reinterpret_cast<void **>(&dCodes), size_t(48) * F));
        ENCCHK(alloc(reinterpret_cast<void **>(&dHdrBits), size_t(48) * F));
        ENCCHK(alloc(reinterpret_cast<void **>(&dSmpBits), sizeof(uint16_t) * 48 * F));
        ENCCHK(alloc(reinterpret_cast<void **>(&dFrameBits), sizeof(uint32_t) * 3 * F));
        ENCCHK(alloc(reinterpret_cast<void **>(&dFrameOff), sizeof(uint32_t) * F));
        ENCCHK(alloc(reinterpret_cast<void **>(&dWin), sizeof(int32_t) * nStreams));
        ENCCHK(alloc(reinterpret_cast<void **>(&dSize), sizeof(uint64_t) * nStreams));
        ENCCHK(alloc(reinterpret_cast<void **>(&dOutOff), sizeof(uint64_t) * nStreams));
        ENCCHK(hipMemcpyAsync(dT, &encTabs(), sizeof(EncTabs), hipMemcpyHostToDevice, st));
        ENCCHK(hipMemcpyAsync(dPcm, pcm + sampleOffsets[0], sizeof(float) * nSamples, hipMemcpyHostToDevice, st));
        ENCCHK(hipMemcpyAsync(dStr, hs.data(), sizeof(EncStream) * nStreams, hipMemcpyHostToDevice, st));
        ENCCHK(hipMemcpyAsync(dFS, frameStream.data(), sizeof(uint32_t) * F, hipMemcpyHostToDevice, st));
        ENCCHK(hipMemsetAsync(dBad, 0, sizeof(uint32_t) * nStreams, st));
        ENCCHK(hipMemsetAsync(dBest, 0, size_t(128) * F, st));
        ENCCHK(hipMemsetAsync(dCodes, 0, size_t(48) * F, st));
        ENCCHK(hipMemsetAsync(dFrameBits, 0, sizeof(uint32_t) * 3 * F, st));
        hipLaunchKernelGGL(encAnalyseKernel, dim3((F + 3) / 4), dim3(256), 0, st, dT, dPcm, dStr, dFS, F, dSpec, dPw, dLo, dHi, dBad);
        hipLaunchKernelGGL(encStreamKernel, dim3(nStreams), dim3(64), 0, st, dT, dStr, dPw, dLo, dHi, params->powerBandCutoff,
                           params->targetBitRate, vmask, dHdr, dKeep);
        hipLaunchKernelGGL(encSearchKernel, dim3(F), dim3(128), 0, st, dT, dSpec, dLo, dHi, dFS, dHdr, dKeep, vmask,
                           params->minimumDynamicRange, params->maximumQuantizationError, dBest);
        hipLaunchKernelGGL(encChainKernel, dim3(nStreams), dim3(64), 0, st, dT, dStr, dKeep, vmask, F,
                           reinterpret_cast<const uint64_t *>(dBest), dCodes);
        hipLaunchKernelGGL(encBitsKernel, dim3(F), dim3(64), 0, st, dT, dSpec, dStr, dFS, dHdr, dKeep, vmask, F, dCodes, dHdrBits, dSmpBits, dFrameBits);
        hipLaunchKernelGGL(encSizeKernel, dim3(nStreams), dim3(256), 0, st, dStr, F, cmask, dFrameBits, dWin, dSize, dFrameOff);
        ENCCHK(hipGetLastError());
        ENCCHK(hipMemcpyAsync(bad.data(), dBad, sizeof(uint32_t) * nStreams, hipMemcpyDeviceToHost, st));
        ENCCHK(hipMemcpyAsync(win.data(), dWin, sizeof(int32_t) * nStreams, hipMemcpyDeviceToHost, st));
        ENCCHK(hipMemcpyAsync(keep.data(), dKeep, sizeof(int32_t) * nStreams, hipMemcpyDeviceToHost, st));
        ENCCHK(hipMemcpyAsync(size.data(), dSize, sizeof(uint64_t) * nStreams, hipMemcpyDeviceToHost, st));
        ENCCHK(hipStreamSynchronize(st));
        for (uint32_t i = 0 ; i < nStreams ; ++i)
            if (bad[i])
            {
                dcsCtxSetError(ctx, ("stream " + std::to_string(i) + ": a sample is not finite or |x| > 1").c_str());
                return DCS_ERR_BAD_STREAM;
            }
        outOffsets[0] = 0;
        for (uint32_t i = 0 ; i < nStreams ; ++i)
            outOffsets[i + 1] = outOffsets[i] + size[i];
        if (info != nullptr)
            for (uint32_t i = 0 ; i < nStreams ; ++i)
                info[i] = DcsEncodeInfo{ ct[win[i]], cs[win[i]], static_cast<int32_t>(hs[i].nFrames), static_cast<int32_t>(size[i]), keep[i] };
        const uint64_t total = outOffsets[nStreams];
        if (out == nullptr || outCap < total)
            return DCS_ERR_CAPACITY;
        const size_t nWords = static_cast<size_t>((total + 3) / 4) + 1;
        ENCCHK(alloc(reinterpret_cast<void **>(&dW), sizeof(uint32_t) * nWords));
        ENCCHK(hipMemsetAsync(dW, 0, sizeof(uint32_t) * nWords, st));
        ENCCHK(hipMemcpyAsync(dOutOff, outOffsets, sizeof(uint64_t) * nStreams, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(encHeadKernel, dim3(nStreams), dim3(64), 0, st, dStr, dHdr, dWin, dOutOff, dW);
        hipLaunchKernelGGL(encPackKernel, dim3((F + 3) / 4), dim3(64), 0, st, dT, dSpec, dStr, dFS, dHdr, dKeep, dWin, F, dCodes,
                           dHdrBits, dSmpBits, dFrameOff, dOutOff, dW);
        hipLaunchKernelGGL(encSwapKernel, dim3(static_cast<unsigned>((nWords + 255) / 256)), dim3(256), 0, st, dW, nWords);
        ENCCHK(hipGetLastError());
        ENCCHK(hipMemcpyAsync(out, dW, total, hipMemcpyDeviceToHost, st));
        ENCCHK(hipStreamSynchronize(st));
        return DCS_OK;
    }();
    (void)hipStreamSynchronize(st);
    for (CacheBuf &h : held)
        h.release();
    return status;
}
