// dcs_encode93a.hip.h -- the OS93a Type-1 (pair-table) encoder, included by dcs_encode.hip.
//
// The reference has no encoder for this layout (CompressFrame93a, DCSEncoder.cpp:2485-2527), so the algorithm is this
// project's own; what is fixed from outside is the decoder (DecoderImpl93a::DecompressFrame, DCSDecoderNative.cpp:2831-3032,
// unpack93a in dcs_kernels.hip.h).  A frame is 127 coefficient pairs in 18 bands; a coded band has a width w = 1..9, a
// quarter-octave scale code s and one index per pair into the 2^w points of kPair93a.  After one f32 multiply and one
// roundf per coefficient (the targets) every decision is an integer one, restated in tests/enc93a_ref.py.
//
//   E1  encAnalyseKernel  the OS93 front end, unchanged (its spectrum is all that is read of it)
//   A1  enc93aFrameKernel<false>  a block per frame: targets and pair table in LDS; the search D(band, w, s) = sum over the
//                         band's pairs of the squared distance to the nearest point, a lane per (w, s, pair) with the points
//                         in a serial loop (a wavefront shares w, so the table read is one broadcast and nothing is reduced
//                         across lanes); then the walk, a lane per (codebook pp, lambda of the ladder), over the D table in
//                         LDS; per-stream totals by integer atomics
//   A2  enc93aChooseKernel  a block per stream: the candidate within the budget with the least error
//   A3  enc93aFrameKernel<true>  the chosen candidate's search and walk again, each frame's choices to a 40-byte record
//   A4  enc93aOffsetKernel  a block per stream: the frames' bit offsets
//   A5  enc93aPackKernel  a block per frame: prefix and delta codes, each pair's nearest point again, OR-ed into zeroed
//                         big-endian words; encSwapKernel turns them into bytes
//
// Nothing per frame is kept between A1 and A3 but E1's spectrum: 1 264 device bytes per frame (spectrum 1 024, E1's band
// statistics 192, frame -> stream 4, record 40, offset 4), so one call holds its whole batch and a 65 535-frame stream
// takes 83 MB.

namespace {

constexpr int kA93NS = 4;                  // scale codes searched per (band, width)
constexpr int kA93KL = 64;                 // the ladder's entries
constexpr int kA93Cand = 4 * kA93KL;       // candidates per frame: (pp, lambda)
constexpr int kA93SMin = 4, kA93SMax = 0x39, kA93Prv0 = 0x1A;
constexpr uint32_t kA93M0 = 0xFFFE;        // OS93a's mixing multiplier at mixing level 0xFF
constexpr float kA93K = 32768.0f;          // spec 1.0 = frame-buffer 32768 at kA93M0
constexpr uint32_t kA93MaxFrameBits = 18 * (4 + 8) + 127 * 9;

struct Enc93aTabs
{
    uint32_t pair[1024];                   // kPair93a as words: point j of width w at (1 << w) + j, first value in the low half
    uint64_t ladder[kA93KL];
    uint64_t floorE[18];                   // E_b of this call's maximumQuantizationError
    int32_t sfs[64], pmax[10];
    uint8_t inputs[18], first[18], bandOf[127];
    uint8_t pfxLen[4][10], pfxCode[4][10], wmax[4];
    uint8_t dlLen[54], dlCode[54];
};

// per (stream, candidate): sums over the stream's frames
struct Enc93aTot { unsigned long long bits, sumD; uint32_t hist[20]; };       // hist[L + 1] = frames whose last coded band is L

struct Enc93aRec { uint8_t w[18], s[18]; int8_t last; uint8_t pad; uint16_t bits; };
static_assert(sizeof(Enc93aRec) == 40, "Enc93aRec");

inline int a93Sfs(int s)
{
    uint32_t sf = 0x8000;
    for (int i = 0 ; i < (s & 3) ; ++i)
        sf = (sf * 0x9838u) >> 15;
    sf <<= (s >> 2);
    sf = ((sf >> 16) * kA93M0) >> 15;
    return static_cast<int16_t>(sf & 0xFFFF);
}

Enc93aTabs buildTabs93a(float maxQE)
{
    Enc93aTabs t;
    memset(&t, 0, sizeof(t));
    for (int i = 0 ; i < 1024 ; ++i)
        t.pair[i] = static_cast<uint32_t>(kPair93a[2 * i]) | (static_cast<uint32_t>(kPair93a[2 * i + 1]) << 16);
    t.ladder[0] = 0;
    for (int k = 1 ; k < kA93KL - 1 ; ++k)
        t.ladder[k] = static_cast<uint64_t>(2 + (k & 1)) << (k >> 1);
    t.ladder[kA93KL - 1] = 1ull << 40;
    const double q = static_cast<double>(maxQE);
    for (int b = 0, first = 0 ; b < 18 ; ++b)
    {
        t.inputs[b] = kInputsPerBand93a[b];
        t.first[b] = static_cast<uint8_t>(first);
        for (int i = 0 ; i < t.inputs[b] ; ++i)
            t.bandOf[first + i] = static_cast<uint8_t>(b);
        first += t.inputs[b];
        t.floorE[b] = static_cast<uint64_t>(floor(((1073741824.0 * q) * q) * static_cast<double>(2 * t.inputs[b])));
    }
    for (int s = 0 ; s < 64 ; ++s)
        t.sfs[s] = a93Sfs(s);
    for (int w = 1 ; w <= 9 ; ++w)
        for (int i = 2 << w ; i < 4 << w ; ++i)
        {
            const int v = static_cast<int16_t>(kPair93a[i]);
            t.pmax[w] = std::max(t.pmax[w], v < 0 ? -v : v);
        }
    for (int pp = 0 ; pp < 4 ; ++pp)
        for (int i = 0 ; i < 16 ; ++i)
        {
            const int e = kBandBits93a[pp * 16 + i], n = e >> 8, w = e & 0xFF;
            if (w != 0xFF && t.pfxLen[pp][w] == 0)
            {
                t.pfxLen[pp][w] = static_cast<uint8_t>(n);
                t.pfxCode[pp][w] = static_cast<uint8_t>(i >> (4 - n));
                t.wmax[pp] = std::max<uint8_t>(t.wmax[pp], static_cast<uint8_t>(w));
            }
        }
    for (int i = 0 ; i < 16 ; ++i)
    {
        const int e = kScaleCb93a[i], n = (e >> 8) & 0xF, v = e & 0xFF;
        if (v != 0xFF)
        {
            if (t.dlLen[v] == 0) { t.dlLen[v] = static_cast<uint8_t>(n); t.dlCode[v] = static_cast<uint8_t>(i >> (4 - n)); }
            continue;
        }
        for (int j = 0 ; j < 16 ; ++j)
        {
            const int e2 = kScaleCb93a[((e >> 12) << 4) + j], n2 = (e2 >> 8) & 0xF, v2 = e2 & 0xFF;
            if (t.dlLen[v2] == 0) { t.dlLen[v2] = static_cast<uint8_t>(n2); t.dlCode[v2] = static_cast<uint8_t>(((i << 4) | j) >> (8 - n2)); }
        }
    }
    return t;
}

// what a block keeps of the tables and of its frame
struct Enc93aLds
{
    uint32_t pair[1024];
    unsigned long long D[18][9][kA93NS], D0[18], floorE[18];
    int32_t t[256], sfs[64], pmax[10];
    uint8_t s0[18][9];
    uint8_t inputs[18], first[18], bandOf[127], pfxLen[4][10], wmax[4], dlLen[54];
    uint8_t chW[18], chS[18];
};

// MultiplyRoundAdd on a zero accumulator (roundHi in dcs_kernels.hip.h): the frame-buffer word of p = point * scale
__device__ __forceinline__ int a93Recon(int p)
{
    uint32_t mr = (static_cast<uint32_t>(p) << 1) + 0x8000u;
    if ((p & 0x7FFF) == 0x4000)
        mr &= ~0x10000u;
    return static_cast<int>(mr) >> 16;
}

__device__ __forceinline__ unsigned long long a93Dist(uint32_t word, int sf, int t0, int t1)
{
    const int d0 = t0 - a93Recon(__mul24(static_cast<int16_t>(word & 0xFFFFu), sf));
    const int d1 = t1 - a93Recon(__mul24(static_cast<int>(word) >> 16, sf));
    // (|d| < 2^16: the square fits 32 bits unsigned, not signed)
    return static_cast<unsigned long long>(static_cast<uint32_t>(d0) * static_cast<uint32_t>(d0)) + static_cast<uint32_t>(d1) * static_cast<uint32_t>(d1);
}

// the codebook value that takes the carried prv to scale code s at width w, or -1 (scaleCode = prv + value - 1 + 2w,
// minus 0x36 above 0x39; value 0..0x35)
__device__ __forceinline__ int a93Delta(int prv, int w, int s)
{
    int v = s - (prv + 2 * w - 1);
    if (v < 0)
        v += 54;
    return (v < 0 || v > 53) ? -1 : v;
}

// The target of frame-buffer word i from E1's frame (spec = the reference's frame.f, 256 floats).  The OS93 Type-0 decoder
// writes frame.f[k] to word k + 1 and then moves word 1 into word 0 (DecoderImpl93::DecompressFrame's DC step, dcFixup in
// dcs_kernels.hip.h), so its frame buffer is word 0 = f[0], word 1 = 0, word i = f[i - 1]; this decoder writes words
// 0..253 as they come, so these are the values it has to be given.
__device__ __forceinline__ int a93Target(const float *frame, int i)
{
    if (i == 1)
        return 0;
    const float r = roundf(frame[i == 0 ? 0 : i - 1] * kA93K);
    return static_cast<int>(fminf(fmaxf(r, -32768.0f), 32767.0f));
}

struct Enc93aWalk { int last; uint32_t through; unsigned long long sumD; };

// one candidate's walk over the frame's D table; chW / chS (LDS, or null): the choices
__device__ inline Enc93aWalk a93Walk(const Enc93aLds &S, int pp, unsigned long long lam, uint8_t *chW, uint8_t *chS)
{
    int prv = kA93Prv0;
    Enc93aWalk o = { -1, 0, 0 };
    uint32_t bits = 0;
    const int wmax = S.wmax[pp];
    for (int b = 0 ; b < 18 ; ++b)
    {
        const int n = S.inputs[b];
        const unsigned long long eb = S.floorE[b];
        uint32_t bb = S.pfxLen[pp][0];
        unsigned long long bd = S.D0[b], bc = (bd > eb ? bd : eb) + lam * bb;
        int bw = 0, bs = 0;
        for (int w = 1 ; w <= wmax ; ++w)
        {
            const int s0 = S.s0[b][w - 1];
            const uint32_t fixed = S.pfxLen[pp][w] + static_cast<uint32_t>(n * w);
            for (int k = 0 ; k < kA93NS ; ++k)
            {
                const int v = a93Delta(prv, w, s0 + k);
                if (v < 0)
                    continue;
                const uint32_t nb = fixed + S.dlLen[v];
                const unsigned long long d = S.D[b][w - 1][k];
                const unsigned long long cost = (d > eb ? d : eb) + lam * nb;
                if (cost < bc || (cost == bc && nb < bb))
                {
                    bc = cost; bb = nb; bd = d; bw = w; bs = s0 + k;
                }
            }
        }
        bits += bb;
        o.sumD += bd;
        if (bw != 0)
        {
            prv = bs - 2 * bw;
            o.last = b;
            o.through = bits;
        }
        if (chW != nullptr)
        {
            chW[b] = static_cast<uint8_t>(bw);
            chS[b] = static_cast<uint8_t>(bs);
        }
    }
    return o;
}

// what A2 leaves per stream
struct Enc93aChoice { int32_t selector, ladderIndex, numBands, fits; unsigned long long frameBits, sumD; };

// A1 (PACK = false) and A3 (PACK = true): a block per frame
template <bool PACK>
__global__ __launch_bounds__(256) void enc93aFrameKernel(const Enc93aTabs *__restrict__ Tp, const float *__restrict__ spec,
    const uint32_t *__restrict__ frameStream, Enc93aTot *__restrict__ tot, const Enc93aChoice *__restrict__ choice,
    Enc93aRec *__restrict__ rec)
{
    const Enc93aTabs &T = *Tp;
    __shared__ Enc93aLds S;
    const int tid = threadIdx.x;
    const uint32_t f = blockIdx.x, si = frameStream[f];
    int ppOnly = 0, wLimit = 9;
    Enc93aChoice ch = {};
    if (PACK)
    {
        ch = choice[si];
        ppOnly = ch.selector;
        wLimit = T.wmax[ppOnly];
    }
    for (int i = tid ; i < 1024 ; i += 256)
        S.pair[i] = T.pair[i];
    S.t[tid] = tid < 254 ? a93Target(spec + static_cast<size_t>(f) * 256, tid) : 0;
    for (int i = tid ; i < 18 * 9 * kA93NS ; i += 256)
        (&S.D[0][0][0])[i] = 0;
    if (tid < 64) S.sfs[tid] = T.sfs[tid];
    if (tid < 10) S.pmax[tid] = T.pmax[tid];
    if (tid < 18) { S.inputs[tid] = T.inputs[tid]; S.first[tid] = T.first[tid]; S.floorE[tid] = T.floorE[tid]; }
    if (tid < 127) S.bandOf[tid] = T.bandOf[tid];
    if (tid < 40) (&S.pfxLen[0][0])[tid] = (&T.pfxLen[0][0])[tid];
    if (tid < 4) S.wmax[tid] = T.wmax[tid];
    if (tid < 54) S.dlLen[tid] = T.dlLen[tid];
    __syncthreads();

    // per band: the energy D(b, 0); per (band, width): where the window of scale codes starts
    if (tid < 18)
    {
        unsigned long long e = 0;
        for (int i = 2 * S.first[tid] ; i < 2 * (S.first[tid] + S.inputs[tid]) ; ++i)
            e += static_cast<unsigned long long>(static_cast<uint32_t>(S.t[i] * S.t[i]));
        S.D0[tid] = e;
    }
    if (tid < 18 * 9)
    {
        const int b = tid / 9, w = 1 + tid % 9;
        int peak = 0;
        for (int i = 2 * S.first[b] ; i < 2 * (S.first[b] + S.inputs[b]) ; ++i)
            peak = max(peak, abs(S.t[i]));
        int hi = kA93SMin;
        for (int s = kA93SMin ; s <= kA93SMax ; ++s)
            hi += ((S.pmax[w] * S.sfs[s]) >> 15) < peak ? 1 : 0;
        hi = min(hi, kA93SMax);
        S.s0[b][w - 1] = static_cast<uint8_t>(max(kA93SMin, hi - (kA93NS - 1)));
    }
    __syncthreads();

    // the search: item = (w, k, pair), w-major, so that the lanes of a wavefront share w
    const int nItems = wLimit * kA93NS * 127;
    for (int idx = tid ; idx < nItems ; idx += 256)
    {
        const int w = 1 + idx / (kA93NS * 127), r = idx % (kA93NS * 127), k = r / 127, pr = r % 127;
        const int b = S.bandOf[pr];
        const int sf = S.sfs[S.s0[b][w - 1] + k];
        const int t0 = S.t[2 * pr], t1 = S.t[2 * pr + 1];
        const uint32_t *pts = S.pair + (1 << w);
        unsigned long long best = a93Dist(pts[0], sf, t0, t1);
        for (int j = 1 ; j < (1 << w) ; ++j)
        {
            const unsigned long long d = a93Dist(pts[j], sf, t0, t1);
            best = d < best ? d : best;
        }
        atomicAdd(&S.D[b][w - 1][k], best);
    }
    __syncthreads();

    if (!PACK)
    {
        const int pp = tid >> 6;
        const Enc93aWalk o = a93Walk(S, pp, T.ladder[tid & 63], nullptr, nullptr);
        Enc93aTot *p = tot + static_cast<size_t>(si) * kA93Cand + tid;
        atomicAdd(&p->bits, static_cast<unsigned long long>(o.through));
        atomicAdd(&p->sumD, o.sumD);
        atomicAdd(&p->hist[o.last + 1], 1u);
    }
    else if (tid == 0)
    {
        const Enc93aWalk o = a93Walk(S, ppOnly, T.ladder[ch.ladderIndex], S.chW, S.chS);
        Enc93aRec r;
        for (int b = 0 ; b < 18 ; ++b) { r.w[b] = S.chW[b]; r.s[b] = S.chS[b]; }
        r.last = static_cast<int8_t>(o.last);
        r.pad = 0;
        r.bits = static_cast<uint16_t>(o.through + (o.last + 1 < ch.numBands ? 4u : 0u));
        rec[f] = r;
    }
}

// A2: a block per stream, a thread per candidate; thread 0 picks
__global__ __launch_bounds__(256) void enc93aChooseKernel(const Enc93aTot *__restrict__ tot, const unsigned long long *__restrict__ budget,
    Enc93aChoice *__restrict__ choice)
{
    __shared__ unsigned long long sBits[kA93Cand], sD[kA93Cand];
    __shared__ int sBands[kA93Cand];
    const int c = threadIdx.x;
    const Enc93aTot &t = tot[static_cast<size_t>(blockIdx.x) * kA93Cand + c];      // (read in place: a copy indexed by a loop would live in scratch)
    int numBands = 1;
    for (int i = 1 ; i < 19 ; ++i)
        if (t.hist[i] != 0)
            numBands = i;
    unsigned long long term = 0;
    for (int i = 0 ; i < numBands ; ++i)
        term += t.hist[i];
    sBits[c] = t.bits + 4 * term;
    sD[c] = t.sumD;
    sBands[c] = numBands;
    __syncthreads();
    if (c != 0)
        return;
    const unsigned long long cap = budget[blockIdx.x];
    int best = -1, least = 0;
    for (int k = 0 ; k < kA93Cand ; ++k)
    {
        if (sBits[k] < sBits[least])
            least = k;
        if (sBits[k] <= cap && (best < 0 || sD[k] < sD[best] || (sD[k] == sD[best] && sBits[k] < sBits[best])))
            best = k;
    }
    const int win = best >= 0 ? best : least;
    choice[blockIdx.x] = Enc93aChoice{ win / kA93KL, win % kA93KL, sBands[win], best >= 0 ? 1 : 0, sBits[win], sD[win] };
}

// A4: a block per stream: the exclusive scan of its frames' bits
__global__ __launch_bounds__(256) void enc93aOffsetKernel(const EncStream *__restrict__ streams, const Enc93aRec *__restrict__ rec,
    uint32_t *__restrict__ frameOff)
{
    __shared__ uint32_t scan[256];
    __shared__ uint32_t carry;
    const EncStream s = streams[blockIdx.x];
    const int t = threadIdx.x;
    if (t == 0)
        carry = 0;
    __syncthreads();
    for (uint32_t j0 = 0 ; j0 < s.nFrames ; j0 += 256)
    {
        const uint32_t j = j0 + t;
        const uint32_t x = j < s.nFrames ? rec[s.firstFrame + j].bits : 0;
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

// the frame count and the header byte 1 pp bbbbb
__global__ __launch_bounds__(64) void enc93aHeadKernel(const EncStream *__restrict__ streams, const Enc93aChoice *__restrict__ choice,
    const uint64_t *__restrict__ outOff, uint32_t n, uint32_t *__restrict__ W)
{
    const uint32_t si = blockIdx.x * 64 + threadIdx.x;
    if (si >= n)
        return;
    const uint32_t nF = streams[si].nFrames;
    const Enc93aChoice c = choice[si];
    encPut(W, outOff[si] * 8, (nF << 8) | 0x80u | (static_cast<uint32_t>(c.selector) << 5) | static_cast<uint32_t>(c.numBands), 24);
}

// A5: a block per frame.  Lane 0 walks the bands for their bit positions and writes the prefix and delta codes; then a
// lane per pair finds its nearest point again (the lowest index of a tie: the loop runs upwards and replaces on less only)
__global__ __launch_bounds__(128) void enc93aPackKernel(const Enc93aTabs *__restrict__ Tp, const float *__restrict__ spec,
    const uint32_t *__restrict__ frameStream, const Enc93aChoice *__restrict__ choice, const Enc93aRec *__restrict__ rec,
    const uint32_t *__restrict__ frameOff, const uint64_t *__restrict__ outOff, uint32_t *__restrict__ W)
{
    const Enc93aTabs &T = *Tp;
    __shared__ uint32_t pair[1024];
    __shared__ uint32_t idxPos[18];
    __shared__ Enc93aRec sr;
    const int tid = threadIdx.x;
    const uint32_t f = blockIdx.x, si = frameStream[f];
    for (int i = tid ; i < 1024 ; i += 128)
        pair[i] = T.pair[i];
    if (tid == 0)
        sr = rec[f];
    __syncthreads();
    const Enc93aChoice ch = choice[si];
    const uint64_t base = (outOff[si] + 3) * 8 + frameOff[f];
    if (tid == 0)
    {
        const int pp = ch.selector;
        int prv = kA93Prv0;
        uint32_t pos = 0;
        for (int b = 0 ; b <= sr.last ; ++b)
        {
            const int w = sr.w[b], s = sr.s[b];
            encPut(W, base + pos, T.pfxCode[pp][w], T.pfxLen[pp][w]);
            pos += T.pfxLen[pp][w];
            if (w == 0)
                continue;
            const int v = a93Delta(prv, w, s);
            encPut(W, base + pos, T.dlCode[v], T.dlLen[v]);
            pos += T.dlLen[v];
            prv = s - 2 * w;
            idxPos[b] = pos;
            pos += static_cast<uint32_t>(T.inputs[b]) * static_cast<uint32_t>(w);
        }
        if (sr.last + 1 < ch.numBands)
            encPut(W, base + pos, 2u, 4);           // the terminator, 0010 in all four codebooks
    }
    __syncthreads();
    if (tid >= 127)
        return;
    const int b = T.bandOf[tid];
    if (b > sr.last || sr.w[b] == 0)
        return;
    const int w = sr.w[b], sf = T.sfs[sr.s[b]];
    const int t0 = a93Target(spec + static_cast<size_t>(f) * 256, 2 * tid), t1 = a93Target(spec + static_cast<size_t>(f) * 256, 2 * tid + 1);
    const uint32_t *pts = pair + (1 << w);
    unsigned long long best = a93Dist(pts[0], sf, t0, t1);
    uint32_t at = 0;
    for (int j = 1 ; j < (1 << w) ; ++j)
    {
        const unsigned long long d = a93Dist(pts[j], sf, t0, t1);
        if (d < best) { best = d; at = static_cast<uint32_t>(j); }
    }
    encPut(W, base + idxPos[b] + static_cast<uint32_t>(tid - T.first[b]) * static_cast<uint32_t>(w), at, w);
}

bool paramsValid93a(const DcsEncodeParams *p)
{
    return p != nullptr && p->formatVersion == 0x9301 && p->streamFormatType >= -1 && p->streamFormatType <= 1
        && p->streamFormatSubType >= -1 && p->streamFormatSubType <= 3 && p->targetBitRate >= 1 && p->targetBitRate <= 100000000
        && isfinite(p->powerBandCutoff) && isfinite(p->minimumDynamicRange) && isfinite(p->maximumQuantizationError);
}

// Type 1 of every stream: the driver of one call.  Its steps, in order: the streams' lengths; the call's buffers; upload,
// E1, A1, A2 and a wait (the choices and E1's flags are on the host); sizes, outOffsets, info and the capacity check; A3-A5,
// the swap, the download and a wait.
DcsStatus encode93aType1(DcsCtx *ctx, const float *pcm, const uint64_t *so, uint32_t nStreams, const DcsEncodeParams *params,
                         uint8_t *out, size_t outCap, uint64_t *outOffsets, DcsEncodeInfo *info, DcsEncode93aInfo *info93a)
{
    const hipStream_t st = dcsCtxStream(ctx);
    std::vector<EncStream> hs(nStreams);
    std::vector<uint32_t> frameStream;
    std::vector<unsigned long long> budget(nStreams);
    uint32_t F = 0;
    for (uint32_t i = 0 ; i < nStreams ; ++i)
    {
        if (so[i + 1] <= so[i])
        {
            dcsCtxSetError(ctx, ("stream " + std::to_string(i) + ": empty").c_str());
            return DCS_ERR_INVALID_ARG;
        }
        const uint64_t n = so[i + 1] - so[i], nF = (n + 239) / 240;
        if (nF > 65535)
        {
            dcsCtxSetError(ctx, ("stream " + std::to_string(i) + ": more than 65 535 frames").c_str());
            return DCS_ERR_INVALID_ARG;
        }
        hs[i] = EncStream{ so[i] - so[0], static_cast<uint32_t>(n), F, static_cast<uint32_t>(nF), 0u, 1.0f };
        frameStream.insert(frameStream.end(), static_cast<size_t>(nF), i);
        budget[i] = static_cast<unsigned long long>(params->targetBitRate) * nF * 240ull / 31250ull;
        F += static_cast<uint32_t>(nF);
    }
    outOffsets[0] = 0;
    if (nStreams == 0)
        return DCS_OK;
    ENCCHK(hipSetDevice(dcsCtxDevice(ctx)));

    CacheArena call(ctx), blob(ctx);
    EncTabs *dT; Enc93aTabs *dA; float *dPcm, *dSpec, *dPw, *dLo, *dHi; EncStream *dStr; uint32_t *dFS, *dBad, *dFrameOff;
    Enc93aTot *dTot; Enc93aChoice *dChoice; Enc93aRec *dRec; unsigned long long *dBudget; uint64_t *dOutOff;
    const uint64_t nSamples = so[nStreams] - so[0];
    ENCCHK(call.alloc(&dT, 1));
    ENCCHK(call.alloc(&dA, 1));
    ENCCHK(call.alloc(&dPcm, nSamples));
    ENCCHK(call.alloc(&dStr, nStreams));
    ENCCHK(call.alloc(&dFS, F));
    ENCCHK(call.alloc(&dSpec, size_t(256) * F));
    ENCCHK(call.alloc(&dPw, size_t(16) * F));
    ENCCHK(call.alloc(&dLo, size_t(16) * F));
    ENCCHK(call.alloc(&dHi, size_t(16) * F));
    ENCCHK(call.alloc(&dBad, nStreams));
    ENCCHK(call.alloc(&dTot, size_t(kA93Cand) * nStreams));
    ENCCHK(call.alloc(&dChoice, nStreams));
    ENCCHK(call.alloc(&dBudget, nStreams));
    ENCCHK(call.alloc(&dOutOff, nStreams));
    ENCCHK(call.alloc(&dRec, F));
    ENCCHK(call.alloc(&dFrameOff, F));

    const Enc93aTabs tabs = buildTabs93a(params->maximumQuantizationError);
    std::vector<uint32_t> bad(nStreams);
    std::vector<Enc93aChoice> choice(nStreams);
    ENCCHK(hipMemcpyAsync(dT, &encTabs93(), sizeof(EncTabs), hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(dA, &tabs, sizeof(Enc93aTabs), hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(dPcm, pcm + so[0], sizeof(float) * nSamples, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(dStr, hs.data(), sizeof(EncStream) * nStreams, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(dFS, frameStream.data(), sizeof(uint32_t) * F, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(dBudget, budget.data(), sizeof(unsigned long long) * nStreams, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemsetAsync(dBad, 0, sizeof(uint32_t) * nStreams, st));
    ENCCHK(hipMemsetAsync(dTot, 0, sizeof(Enc93aTot) * kA93Cand * nStreams, st));
    hipLaunchKernelGGL(encAnalyseKernel<float>, dim3((F + 3) / 4), dim3(256), 0, st, dT, dPcm, dStr, dFS, F, dSpec, dPw, dLo, dHi, dBad,
                       static_cast<const uint32_t *>(nullptr));
    hipLaunchKernelGGL(enc93aFrameKernel<false>, dim3(F), dim3(256), 0, st, dA, dSpec, dFS, dTot, static_cast<const Enc93aChoice *>(nullptr),
                       static_cast<Enc93aRec *>(nullptr));
    hipLaunchKernelGGL(enc93aChooseKernel, dim3(nStreams), dim3(256), 0, st, dTot, dBudget, dChoice);
    ENCCHK(hipGetLastError());
    ENCCHK(hipMemcpyAsync(bad.data(), dBad, sizeof(uint32_t) * nStreams, hipMemcpyDeviceToHost, st));
    ENCCHK(hipMemcpyAsync(choice.data(), dChoice, sizeof(Enc93aChoice) * nStreams, hipMemcpyDeviceToHost, st));
    ENCCHK(hipStreamSynchronize(st));
    for (uint32_t i = 0 ; i < nStreams ; ++i)
        if (bad[i])
        {
            dcsCtxSetError(ctx, ("stream " + std::to_string(i) + ": a sample is not finite or |x| > 1").c_str());
            return DCS_ERR_BAD_STREAM;
        }

    for (uint32_t i = 0 ; i < nStreams ; ++i)
    {
        const Enc93aChoice &c = choice[i];
        const uint64_t size = 3 + (c.frameBits + 7) / 8;
        outOffsets[i + 1] = outOffsets[i] + size;
        if (info != nullptr)
            info[i] = DcsEncodeInfo{ 1, 0, static_cast<int32_t>(hs[i].nFrames), static_cast<int32_t>(size), c.numBands };
        if (info93a != nullptr)
            info93a[i] = DcsEncode93aInfo{ c.selector, c.ladderIndex, c.numBands, 0, c.frameBits, budget[i], c.sumD };
    }
    const uint64_t total = outOffsets[nStreams];
    if (out == nullptr || outCap < total)
        return DCS_ERR_CAPACITY;

    uint32_t *dW;
    const size_t nWords = static_cast<size_t>(total / 4 + 2);
    ENCCHK(blob.alloc(&dW, nWords));
    ENCCHK(hipMemsetAsync(dW, 0, sizeof(uint32_t) * nWords, st));
    ENCCHK(hipMemcpyAsync(dOutOff, outOffsets, sizeof(uint64_t) * nStreams, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(enc93aFrameKernel<true>, dim3(F), dim3(256), 0, st, dA, dSpec, dFS, static_cast<Enc93aTot *>(nullptr), dChoice, dRec);
    hipLaunchKernelGGL(enc93aOffsetKernel, dim3(nStreams), dim3(256), 0, st, dStr, dRec, dFrameOff);
    hipLaunchKernelGGL(enc93aHeadKernel, dim3((nStreams + 63) / 64), dim3(64), 0, st, dStr, dChoice, dOutOff, nStreams, dW);
    hipLaunchKernelGGL(enc93aPackKernel, dim3(F), dim3(128), 0, st, dA, dSpec, dFS, dChoice, dRec, dFrameOff, dOutOff, dW);
    hipLaunchKernelGGL(encSwapKernel, dim3(static_cast<unsigned>((nWords + 255) / 256)), dim3(256), 0, st, dW, nWords);
    ENCCHK(hipGetLastError());
    ENCCHK(hipMemcpyAsync(out, dW, total, hipMemcpyDeviceToHost, st));
    ENCCHK(hipStreamSynchronize(st));
    return DCS_OK;
}

}  // namespace

extern "C" size_t dcs_encode93a_bound(uint64_t nSamples)
{
    return std::max(boundOf(nSamples, kMaxBitsPerFrame93), boundOf(nSamples, kA93MaxFrameBits));
}

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
        return encode93aType1(ctx, pcm, sampleOffsets, nStreams, params, out, outCap, outOffsets, info, info93a);

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
    ENCTRY(encode93aType1(ctx, pcm, sampleOffsets, nStreams, params, buf1.data(), buf1.size(), off1.data(), inf1.data(), info93a));
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
