// dcs_encode93a.hip.h -- the OS93a Type-1 (pair-table) encoder, included by dcs_encode.hip.
//
// The reference has no encoder for this layout (CompressFrame93a, DCSEncoder.cpp:2485-2527), so the algorithm is this
// project's own; what is fixed from outside is the decoder (DecoderImpl93a::DecompressFrame, DCSDecoderNative.cpp:2831-3032,
// unpack93a in dcs_kernels.hip.h).  A frame is 127 coefficient pairs in 18 bands; a coded band has a width w = 1..9, a
// quarter-octave scale code s and one index per pair into the 2^w points of kPair93a.  After one f32 multiply and one
// roundf per coefficient (the targets) every decision is an integer one, restated in tests/enc93a_ref.py.
//
// These are the kernels of a family of EncRun's (Enc93aFamily, dcs_encode_run.hip.h), beside the OS93 (O3-O5) and the 1994+ (E3-E5) stages: a
// job whose set asks for (0x9301, Type 1) runs them, a job of the same call whose set asks for Type 0 runs the O stages.
//
//   E1  encAnalyseKernel  the OS93 front end, unchanged (its spectrum is all that is read of it), once per stream
//   A1  enc93aFrameKernel<false>  once per STREAM-frame, whatever the jobs: targets and pair table in LDS; the search
//                         D(band, w, s) = sum over the band's pairs of the squared distance to the nearest point, a lane per
//                         (w, s, pair) with the points in a serial loop (a wavefront shares w, so the table read is one
//                         broadcast and nothing is reduced across lanes).  Neither targetBitRate nor
//                         maximumQuantizationError is read by it.  Then the walk, a lane per (codebook pp, lambda of the
//                         ladder), over the D table in LDS, once for every distinct maximumQuantizationError q under which a
//                         job names the stream (E_b of q: the floorE table); totals per (q, stream, candidate) by integer
//                         atomics, at row rowOf[q][stream] of the totals table.  A launch walks at most kA93QPerLaunch
//                         values of q; a call with more of them launches again, and a block whose stream none of the
//                         launch's q concerns leaves before the search
//   A2  enc93aChooseKernel  a block per job: within its own budget, the candidate of its (q, stream) row with the least error
//   A3  enc93aFrameKernel<true>  per job-frame: the job's chosen candidate's search and walk again under its q, the frame's
//                         choices to a 40-byte record
//   A4  enc93aOffsetKernel  a block per job: the frames' bit offsets
//   A5  enc93aPackKernel  a block per job-frame: prefix and delta codes, each pair's nearest point again, OR-ed into zeroed
//                         big-endian words; encSwapKernel turns them into bytes
//
// Nothing per frame is kept between A1 and A3 but E1's spectrum (no D table in HBM): per stream-frame 1 220 device bytes
// (spectrum 1 024, E1's band statistics 192, frame -> stream 4), per job-frame of the resident group 48 (record 40, offset
// 4, job-frame -> job 4; the O stages' rows beside them where Type-0 jobs share the call), and 24 KB of totals per
// (stream, distinct q).

namespace {

constexpr int kA93NS = 4;                  // scale codes searched per (band, width)
constexpr int kA93KL = 64;                 // the ladder's entries
constexpr int kA93Cand = 4 * kA93KL;       // candidates per frame: (pp, lambda)
constexpr int kA93SMin = 4, kA93SMax = 0x39, kA93Prv0 = 0x1A;
constexpr uint32_t kA93M0 = 0xFFFE;        // OS93a's mixing multiplier at mixing level 0xFF
constexpr float kA93K = 32768.0f;          // spec 1.0 = frame-buffer 32768 at kA93M0
constexpr uint32_t kA93MaxFrameBits = 18 * (4 + 8) + 127 * 9;
constexpr uint32_t kA93QPerLaunch = 8;     // distinct maximumQuantizationError values one launch of A1 walks
constexpr uint32_t kA93None = 0xFFFFFFFFu; // setQ: a set of the O family; rowOf: no job names this stream under this q

struct Enc93aTabs
{
    uint32_t pair[1024];                   // kPair93a as words: point j of width w at (1 << w) + j, first value in the low half
    uint64_t ladder[kA93KL];
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

// E_b of one maximumQuantizationError: a row of the floorE table, which has one per distinct value of the call.  It
// saturates at 2^40, compared in double before the cast (q is any finite float: the unbounded value passes 2^64 from
// q = 24 771).  Every D is below 2^38, so from 2^38 on max(D, E_b) = E_b for every option of the band and the walk picks the
// fewest bits, whatever E_b is; and a cost stays below 2^40 + 2^40 * 264 < 2^50.
constexpr unsigned long long kA93FloorMax = 1ull << 40;

void floorE93a(float maxQE, unsigned long long *row)
{
    const double q = static_cast<double>(maxQE);
    for (int b = 0 ; b < 18 ; ++b)
    {
        const double e = floor(((1073741824.0 * q) * q) * static_cast<double>(2 * kInputsPerBand93a[b]));
        row[b] = e >= static_cast<double>(kA93FloorMax) ? kA93FloorMax : static_cast<unsigned long long>(e);
    }
}

Enc93aTabs buildTabs93a()
{
    Enc93aTabs t;
    memset(&t, 0, sizeof(t));
    for (int i = 0 ; i < 1024 ; ++i)
        t.pair[i] = static_cast<uint32_t>(kPair93a[2 * i]) | (static_cast<uint32_t>(kPair93a[2 * i + 1]) << 16);
    t.ladder[0] = 0;
    for (int k = 1 ; k < kA93KL - 1 ; ++k)
        t.ladder[k] = static_cast<uint64_t>(2 + (k & 1)) << (k >> 1);
    t.ladder[kA93KL - 1] = 1ull << 40;
    for (int b = 0, first = 0 ; b < 18 ; ++b)
    {
        t.inputs[b] = kInputsPerBand93a[b];
        t.first[b] = static_cast<uint8_t>(first);
        for (int i = 0 ; i < t.inputs[b] ; ++i)
            t.bandOf[first + i] = static_cast<uint8_t>(b);
        first += t.inputs[b];
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

const Enc93aTabs &encTabs93a() { static const Enc93aTabs t = buildTabs93a(); return t; }

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

// what A2 leaves per job
struct Enc93aChoice { int32_t selector, ladderIndex, numBands, fits; unsigned long long frameBits, sumD; };

// A1 (PACK = false), a block per stream-frame: owner = frame -> stream; the walks of q0 .. q0 + nQ - 1 (nQ at most
// kA93QPerLaunch) into the rows rowOf[q * nStreams + stream] of tot.  A3 (PACK = true), a block per job-frame of the
// resident group: owner = job-frame -> job; the job's choice under the q of its set (setQ), to rec.
template <bool PACK>
__global__ __launch_bounds__(256) void enc93aFrameKernel(const Enc93aTabs *__restrict__ Tp, const unsigned long long *__restrict__ floorE,
    const float *__restrict__ spec, const uint32_t *__restrict__ owner, const uint32_t *__restrict__ rowOf, uint32_t nStreams, uint32_t q0,
    uint32_t nQ, Enc93aTot *__restrict__ tot, const EncJob *__restrict__ jobs, const uint32_t *__restrict__ setQ,
    const Enc93aChoice *__restrict__ choice, Enc93aRec *__restrict__ rec)
{
    const Enc93aTabs &T = *Tp;
    __shared__ Enc93aLds S;
    const int tid = threadIdx.x;
    const uint32_t f = blockIdx.x, own = owner[f];
    uint32_t sf = f;
    int ppOnly = 0, wLimit = 9;
    Enc93aChoice ch = {};
    if (PACK)
    {
        const EncJob job = jobs[own];
        const uint32_t q = setQ[job.set];
        if (q == kA93None)
            return;                             // a job of the O family
        sf = encSpecFrame(job, f);
        ch = choice[own];
        ppOnly = ch.selector;
        wLimit = T.wmax[ppOnly];
        if (tid < 18) S.floorE[tid] = floorE[static_cast<size_t>(q) * 18 + tid];
    }
    else
    {
        bool named = false;
        for (uint32_t k = 0 ; k < nQ ; ++k)
            named = named || rowOf[static_cast<size_t>(q0 + k) * nStreams + own] != kA93None;
        if (!named)
            return;                             // (the whole block: own is the block's)
    }
    for (int i = tid ; i < 1024 ; i += 256)
        S.pair[i] = T.pair[i];
    S.t[tid] = tid < 254 ? a93Target(spec + static_cast<size_t>(sf) * 256, tid) : 0;
    for (int i = tid ; i < 18 * 9 * kA93NS ; i += 256)
        (&S.D[0][0][0])[i] = 0;
    if (tid < 64) S.sfs[tid] = T.sfs[tid];
    if (tid < 10) S.pmax[tid] = T.pmax[tid];
    if (tid < 18) { S.inputs[tid] = T.inputs[tid]; S.first[tid] = T.first[tid]; }
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
        const int sfac = S.sfs[S.s0[b][w - 1] + k];
        const int t0 = S.t[2 * pr], t1 = S.t[2 * pr + 1];
        const uint32_t *pts = S.pair + (1 << w);
        unsigned long long best = a93Dist(pts[0], sfac, t0, t1);
        for (int j = 1 ; j < (1 << w) ; ++j)
        {
            const unsigned long long d = a93Dist(pts[j], sfac, t0, t1);
            best = d < best ? d : best;
        }
        atomicAdd(&S.D[b][w - 1][k], best);
    }
    __syncthreads();

    if (!PACK)
    {
        // the D table is walked once per q of the launch that a job names the stream under; only E_b changes between them
        const int pp = tid >> 6;
        const unsigned long long lam = T.ladder[tid & 63];
        for (uint32_t k = 0 ; k < nQ ; ++k)
        {
            const uint32_t row = rowOf[static_cast<size_t>(q0 + k) * nStreams + own];
            if (row == kA93None)
                continue;
            if (tid < 18) S.floorE[tid] = floorE[static_cast<size_t>(q0 + k) * 18 + tid];
            __syncthreads();
            const Enc93aWalk o = a93Walk(S, pp, lam, nullptr, nullptr);
            Enc93aTot *p = tot + static_cast<size_t>(row) * kA93Cand + tid;
            atomicAdd(&p->bits, static_cast<unsigned long long>(o.through));
            atomicAdd(&p->sumD, o.sumD);
            atomicAdd(&p->hist[o.last + 1], 1u);
            __syncthreads();
        }
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

// A2: a block per job of the resident group, a thread per candidate of its (q, stream) row; thread 0 picks within the
// job's budget, floor(targetBitRate * nFrames * 240 / 31250) bits
__global__ __launch_bounds__(256) void enc93aChooseKernel(const Enc93aTot *__restrict__ tot, const uint32_t *__restrict__ rowOf,
    uint32_t nStreams, const EncJob *__restrict__ jobs, const EncSet *__restrict__ sets, const uint32_t *__restrict__ setQ,
    Enc93aChoice *__restrict__ choice)
{
    __shared__ unsigned long long sBits[kA93Cand], sD[kA93Cand];
    __shared__ int sBands[kA93Cand];
    const int c = threadIdx.x;
    const EncJob job = jobs[blockIdx.x];
    const uint32_t q = setQ[job.set];
    if (q == kA93None)
        return;
    const uint32_t row = rowOf[static_cast<size_t>(q) * nStreams + job.stream];
    const Enc93aTot &t = tot[static_cast<size_t>(row) * kA93Cand + c];      // (read in place: a copy indexed by a loop would live in scratch)
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
    const unsigned long long cap = static_cast<unsigned long long>(sets[job.set].rate) * job.nFrames * 240ull / 31250ull;
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

// A4: a block per job: the exclusive scan of its frames' bits
__global__ __launch_bounds__(256) void enc93aOffsetKernel(const EncJob *__restrict__ jobs, const uint32_t *__restrict__ setQ,
    const Enc93aRec *__restrict__ rec, uint32_t *__restrict__ frameOff)
{
    __shared__ uint32_t scan[256];
    __shared__ uint32_t carry;
    const EncJob s = jobs[blockIdx.x];
    if (setQ[s.set] == kA93None)
        return;
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

// the frame count and the header byte 1 pp bbbbb of each Type-1 job of the group
__global__ __launch_bounds__(64) void enc93aHeadKernel(const EncJob *__restrict__ jobs, const uint32_t *__restrict__ setQ,
    const Enc93aChoice *__restrict__ choice, const uint64_t *__restrict__ outOff, uint32_t n, uint32_t *__restrict__ W)
{
    const uint32_t si = blockIdx.x * 64 + threadIdx.x;
    if (si >= n || setQ[jobs[si].set] == kA93None)
        return;
    const uint32_t nF = jobs[si].nFrames;
    const Enc93aChoice c = choice[si];
    encPut(W, outOff[si] * 8, (nF << 8) | 0x80u | (static_cast<uint32_t>(c.selector) << 5) | static_cast<uint32_t>(c.numBands), 24);
}

// A5: a block per job-frame.  Lane 0 walks the bands for their bit positions and writes the prefix and delta codes; then a
// lane per pair finds its nearest point again (the lowest index of a tie: the loop runs upwards and replaces on less only)
__global__ __launch_bounds__(128) void enc93aPackKernel(const Enc93aTabs *__restrict__ Tp, const float *__restrict__ spec,
    const uint32_t *__restrict__ frameJob, const EncJob *__restrict__ jobs, const uint32_t *__restrict__ setQ,
    const Enc93aChoice *__restrict__ choice, const Enc93aRec *__restrict__ rec, const uint32_t *__restrict__ frameOff,
    const uint64_t *__restrict__ outOff, uint32_t *__restrict__ W)
{
    const Enc93aTabs &T = *Tp;
    __shared__ uint32_t pair[1024];
    __shared__ uint32_t idxPos[18];
    __shared__ Enc93aRec sr;
    const int tid = threadIdx.x;
    const uint32_t f = blockIdx.x, si = frameJob[f];
    const EncJob job = jobs[si];
    if (setQ[job.set] == kA93None)
        return;
    const float *frame = spec + static_cast<size_t>(encSpecFrame(job, f)) * 256;
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
    const int t0 = a93Target(frame, 2 * tid), t1 = a93Target(frame, 2 * tid + 1);
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

// a set of the A family: EncRun runs the kernels above on its jobs, the O stages on every other job of an OS93 call
inline bool isType1Of93a(const DcsEncodeParams &p) { return p.formatVersion == 0x9301 && p.streamFormatType == 1; }

}  // namespace
