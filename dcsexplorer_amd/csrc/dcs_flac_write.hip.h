// dcs_flac_write.hip.h -- native FLAC written on the device: int16 PCM in HBM in, one FLAC stream per PCM stream out
// (INTEGRATION.md "Writing FLAC" has the format rules; tests/flac_write_ref.py restates them).  Included in dcs_encode.hip
// behind the FLAC reader; integer arithmetic only, so that unit's floating-point contract does not touch it.
//
// Mono, 16 bits, fixed block size 4096.  A stream of whole DCS frames (dcs_flac_write_streams, dcs_decode_streams_flac, the
// pipeline) has blocks that are multiples of 16 samples, at least 16: the hot path, every block of a decode at 31 250 Hz and
// all but the last block of any stream.  A stream of any length from 1 sample on (dcs_flac_write_samples,
// dcs_decode_streams_flac_at: a converter's output) ends in a block of 1 .. 4096 samples; W1 and W3 take such a block on a
// side of their own, chosen by a branch on the block's length that every lane of the workgroup takes alike, and a block of
// whole 16s runs what it always ran.  The finest partitions of a block of n samples are 2^P, P = min(4, trailing zero bits
// of n) (rules 9 to 11).
//   W1 fwChooseKernel   one workgroup per block: the samples into LDS, the five fixed predictors' |residual| sums, the
//                       2^P x 15 table of exact Rice bit counts of the best order (16 x 15 for whole 16s), its merges for
//                       partition orders P..0, and the block's record (FwRec): CONSTANT, VERBATIM or FIXED with order,
//                       partition order, parameters
//   W2 fwPlaceKernel    one wavefront per stream: the frames' byte offsets behind the stream's 42 header bytes (a scan of
//                       the records' frame sizes), the stream's size, smallest and largest frame and kind counts (FwSum)
//   W3 fwWriteKernel    one workgroup per block: the frame assembled in zeroed LDS as big-endian dwords (each lane ORs in
//                       only a code's one and low bits, the unary zeros are the buffer's), both CRCs from per-lane parts
//                       moved to their place by powers of x (a CRC is linear), and the copy out, dwords where aligned
//   W4 fwMd5Kernel      DCS_FLAC_MD5 only: one lane per stream walks its samples in 64-byte blocks (the chain is serial), any
//                       number of samples, odd ones included
// Nothing comes back to the host between them.  Three more kernels stand where the host's size-then-place step would:
//      fwBaseKernel     one workgroup: the exclusive scan of the streams' sizes (rounds of 256 with a carried total: a scan in
//                       each wavefront, the wavefronts' totals through LDS, as W2's within a stream), which is W3's dBase and,
//                       with FwSum and the block table, the result table as the ABI lays it out (outOffsets, DcsFlacWriteInfo)
//                       and the total in a word of its own
//      fwHeadKernel     the 42 bytes in front of each stream ("fLaC" and STREAMINFO, from FwSum and W4's digests), one lane
//                       per byte: stream bases fall at every alignment, and a lane stores nothing but its own byte
//      fwDownKernel     16-byte copies in a grid-stride loop whose length is read from a word on the DEVICE: the FLAC bytes go
//                       to pinned host memory without the host knowing, when it queues the copy, how many there are
// dcsFlacWriteQueue (dcs_flac_held.h) is the one statement of the order they are queued in; the output in HBM and its pinned
// staging are sized by a bound the host knows beforehand (fwBound: every block VERBATIM).
#pragma once
#include "dcs_flac_held.h"

namespace {

constexpr uint32_t kFwBlock = 4096;
constexpr uint32_t kFwThreads = 256;
constexpr uint32_t kFwHeadBytes = 42;                                   // "fLaC", a metadata block header, STREAMINFO
constexpr uint32_t kFwMaxFrame = 16 + 1 + 2 * kFwBlock + 2;             // dcs_flac_write_bound's bytes per block
constexpr uint32_t kFwBufDw = (kFwMaxFrame + 3) / 4 + 2;                // the frame in LDS, and room for a straddling write
enum : uint32_t { FW_CONSTANT = 0, FW_VERBATIM = 1, FW_FIXED = 2 };

struct FwRec { uint32_t frameBytes; uint8_t kind, order, p, pad; uint8_t k[16]; };
struct FwSum { uint64_t bytes; uint32_t nConstant, nVerbatim, nFixed, minFrame, maxFrame, pad; };
static_assert(sizeof(FwRec) == 24 && sizeof(FwSum) == 32, "records as the host reads them");

// bytes of the frame header: sync and codes (4), the frame number, the block size where it is spelled out, the rate (2), CRC-8
__host__ __device__ inline uint32_t fwNumberBytes(uint32_t v)
{
    uint32_t n = 1;
    if (v >= 0x80)
        for (n = 2 ; (v >> (5 * n + 1)) != 0 ; ++n) {}
    return n;
}
__host__ __device__ inline uint32_t fwHeaderBytes(uint32_t number, uint32_t n)
{
    return 4 + fwNumberBytes(number) + (n == kFwBlock ? 0u : n <= 256 ? 1u : 2u) + 2 + 1;
}

// the largest k with blockFirst[k] <= b (blockFirst has nStreams + 1 entries, strictly rising: every stream has a block)
__device__ inline uint32_t fwStreamOf(const uint32_t *blockFirst, uint32_t nStreams, uint32_t b)
{
    uint32_t lo = 0, hi = nStreams;
    while (hi - lo > 1)
    {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (blockFirst[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}

// block b: its stream, its number in the stream, its first sample in pcm and its length
struct FwBlock { uint32_t stream, number, n; uint64_t first; };
__device__ inline FwBlock fwBlockOf(const uint64_t *offs, const uint32_t *blockFirst, uint32_t nStreams, uint32_t b)
{
    FwBlock w;
    w.stream = fwStreamOf(blockFirst, nStreams, b);
    w.number = b - blockFirst[w.stream];
    const uint64_t len = offs[w.stream + 1] - offs[w.stream], done = static_cast<uint64_t>(w.number) * kFwBlock;
    w.first = offs[w.stream] + done;
    w.n = len - done < kFwBlock ? static_cast<uint32_t>(len - done) : kFwBlock;
    return w;
}

// the fixed predictor's residual of order O at sample i >= O: a plain finite difference
template <int O> __device__ inline int32_t fwResidual(const int32_t *s, uint32_t i)
{
    if (O == 0) return s[i];
    if (O == 1) return s[i] - s[i - 1];
    if (O == 2) return s[i] - 2 * s[i - 1] + s[i - 2];
    if (O == 3) return s[i] - 3 * s[i - 1] + 3 * s[i - 2] - s[i - 3];
    return s[i] - 4 * s[i - 1] + 6 * s[i - 2] - 4 * s[i - 3] + s[i - 4];
}
__device__ inline int32_t fwResidualOf(uint32_t order, const int32_t *s, uint32_t i)
{
    switch (order)
    {
    case 0: return fwResidual<0>(s, i);
    case 1: return fwResidual<1>(s, i);
    case 2: return fwResidual<2>(s, i);
    case 3: return fwResidual<3>(s, i);
    default: return fwResidual<4>(s, i);
    }
}
__device__ inline uint32_t fwZigzag(int32_t e) { return e >= 0 ? static_cast<uint32_t>(e) << 1 : (static_cast<uint32_t>(-e) << 1) - 1; }

__device__ inline void fwLoadBlock(int32_t *s, const int16_t *pcm, const FwBlock &w)
{
    for (uint32_t i = threadIdx.x ; i < w.n ; i += kFwThreads)
        s[i] = pcm[w.first + i];
}

// ------------------------------------------------------------------------------------------------------------ W1
// the first of the 2^q nodes of partition order q in W1's tables: 0, 16, 24, 28, 30 for q = 4 .. 0
__device__ inline uint32_t fwNodeBase(uint32_t q) { return 32u - (2u << q); }

// W1 from the finest partitions' B rows on (they stand at the nodes of partition order P; the caller's barrier is behind
// them): the merges, each node's best parameter, the partition order and the block's record.  kWhole: the block is a
// multiple of 16 samples, P is 4, and the loops have the fixed bounds they always had; else P < 4 is the block's own.
template <bool kWhole> __device__ inline void fwChooseFrom(unsigned long long (*B)[15], unsigned long long *nodeBits, uint32_t *nodeK, uint32_t blockP,
                                                          uint32_t n, uint32_t order, uint32_t head, FwRec *out)
{
    const uint32_t t = threadIdx.x, P = kWhole ? 4u : blockP, finest = fwNodeBase(P);
    // partitions of the lower orders are sums of pairs
    for (uint32_t from = finest, to = finest + (1u << P), count = (1u << P) / 2 ; count >= 1 ; from = to, to += count, count >>= 1)
    {
        if (t < count * 15)
        {
            const uint32_t m = t / 15, k = t % 15;
            B[to + m][k] = B[from + 2 * m][k] + B[from + 2 * m + 1][k];
        }
        __syncthreads();
    }
    if (t >= finest && t < 31)
    {
        unsigned long long best = B[t][0];
        uint32_t bestK = 0;
        for (uint32_t k = 1 ; k < 15 ; ++k)
            if (B[t][k] < best) { best = B[t][k]; bestK = k; }           // (ties: the lowest parameter)
        nodeBits[t] = best;
        nodeK[t] = bestK;
    }
    __syncthreads();
    if (t == 0)
    {
        // a partition order is a candidate only where a partition is longer than the warm-up, (n >> q) > order, as the format
        // asks: the first partition then holds a residual.  Order 0 always is one (the predictor's order is below n: 0 for
        // n <= 4).  The orders above P do not divide n.
        unsigned long long total = 0;
        uint32_t p = 0, base = 0;
        bool any = false;
        for (uint32_t q = P, from = finest ; ; from += 1u << q, --q)
        {
            if ((n >> q) > order)
            {
                unsigned long long sum = 4ull << q;
                for (uint32_t j = 0 ; j < (1u << q) ; ++j)
                    sum += nodeBits[from + j];
                if (!any || sum <= total) { total = sum; p = q; base = from; }  // (ties: the lowest partition order)
                any = true;
            }
            if (q == 0)
                break;
        }
        FwRec r = {};
        if (6 + total >= 16ull * (n - order))
        {
            r.kind = FW_VERBATIM;
            r.frameBytes = head + 1 + 2 * n + 2;
        }
        else
        {
            r.kind = FW_FIXED;
            r.order = static_cast<uint8_t>(order);
            r.p = static_cast<uint8_t>(p);
            const uint32_t bits = 8 + 16 * order + 6 + static_cast<uint32_t>(total);
            r.frameBytes = head + (bits + 7) / 8 + 2;
        }
        *out = r;
        // (the parameters go straight to the record: indexing the local copy would put it in scratch)
        for (uint32_t j = 0 ; r.kind == FW_FIXED && j < (1u << p) ; ++j)
            out->k[j] = static_cast<uint8_t>(nodeK[base + j]);
    }
}

__global__ __launch_bounds__(kFwThreads) void fwChooseKernel(const int16_t *pcm, const uint64_t *offs, const uint32_t *blockFirst,
                                                             uint32_t nStreams, uint32_t nBlocks, FwRec *rec)
{
    __shared__ int32_t s[kFwBlock];
    __shared__ uint32_t part[kFwThreads / 64][6];
    __shared__ unsigned long long B[31][15];            // nodes 0..15: partition order 4; 16..23: 3; 24..27: 2; 28, 29: 1; 30: 0
    __shared__ uint32_t halfSum[kFwThreads / 32][15];   // a block that is no multiple of 16: the half wavefronts' shift sums
    __shared__ unsigned long long nodeBits[31];
    __shared__ uint32_t nodeK[31];
    __shared__ uint32_t chosen[2];                      // differs, order
    const uint32_t b = blockIdx.x, t = threadIdx.x;
    if (b >= nBlocks)
        return;
    const FwBlock w = fwBlockOf(offs, blockFirst, nStreams, b);
    const uint32_t n = w.n;
    fwLoadBlock(s, pcm, w);
    __syncthreads();

    // the five orders' sums over i = 4 .. n-1 (a lane adds at most 16 residuals below 2^20), and whether any sample differs
    uint32_t acc[6] = { 0, 0, 0, 0, 0, 0 };
    for (uint32_t i = t ; i < n ; i += kFwThreads)
    {
        acc[5] |= s[i] != s[0] ? 1u : 0u;
        if (i >= 4)
        {
            const int32_t e0 = fwResidual<0>(s, i), e1 = fwResidual<1>(s, i), e2 = fwResidual<2>(s, i), e3 = fwResidual<3>(s, i),
                          e4 = fwResidual<4>(s, i);
            acc[0] += e0 < 0 ? -e0 : e0; acc[1] += e1 < 0 ? -e1 : e1; acc[2] += e2 < 0 ? -e2 : e2;
            acc[3] += e3 < 0 ? -e3 : e3; acc[4] += e4 < 0 ? -e4 : e4;
        }
    }
#pragma unroll
    for (int q = 0 ; q < 6 ; ++q)
        for (int d = 32 ; d >= 1 ; d >>= 1)
            acc[q] += __shfl_xor(acc[q], d, 64);        // (64 lanes x 2^24 fits; the differs word only has to stay non-zero)
    if ((t & 63) == 0)
        for (int q = 0 ; q < 6 ; ++q)
            part[t >> 6][q] = acc[q];
    __syncthreads();
    if (t == 0)
    {
        unsigned long long best = 0;
        uint32_t order = 0, differs = 0;
        for (uint32_t o = 0 ; o < 5 ; ++o)
        {
            unsigned long long sum = 0;
            for (uint32_t v = 0 ; v < kFwThreads / 64 ; ++v)
                sum += part[v][o];
            if (o == 0 || sum < best) { best = sum; order = o; }         // (ties: the lowest order)
        }
        for (uint32_t v = 0 ; v < kFwThreads / 64 ; ++v)
            differs |= part[v][5];
        chosen[0] = differs;
        chosen[1] = order;
    }
    __syncthreads();
    const uint32_t order = chosen[1];
    const uint32_t head = fwHeaderBytes(w.number, n);
    if (chosen[0] == 0)
    {
        if (t == 0)
        {
            FwRec r = {};
            r.kind = FW_CONSTANT;
            r.frameBytes = head + 1 + 2 + 2;
            rec[b] = r;
        }
        return;
    }

    // The finest partitions: 2^P of n >> P samples, P = min(4, trailing zero bits of n).  Their B rows stand at the nodes
    // of partition order P (fwNodeBase), so that a block of whole 16s, P = 4, fills nodes 0..15 as it always did.
    const uint32_t P = (n & 15) == 0 ? 4u : static_cast<uint32_t>(__builtin_ctz(n)), finest = fwNodeBase(P);
    // B[j][k] of the 16 finest partitions: lane group j = t / 16 walks partition j, 15 shift-adds a residual.  The branch is
    // on the block's length alone: every lane of the workgroup takes the same side.
    if (P == 4)
    {
        const uint32_t size = n / 16, j = t >> 4;
        uint32_t sum[15];
#pragma unroll
        for (int k = 0 ; k < 15 ; ++k)
            sum[k] = 0;
        for (uint32_t i = j * size + (t & 15) ; i < (j + 1) * size ; i += 16)
            if (i >= order)
            {
                const uint32_t u = fwZigzag(fwResidualOf(order, s, i));
#pragma unroll
                for (int k = 0 ; k < 15 ; ++k)
                    sum[k] += u >> k;
            }
#pragma unroll
        for (int k = 0 ; k < 15 ; ++k)
            for (int d = 8 ; d >= 1 ; d >>= 1)
                sum[k] += __shfl_xor(sum[k], d, 64);    // (256 residuals below 2^21)
        if ((t & 15) == 0)
        {
            // the partition's residuals: its samples from `order` on (none at all where a short block's partition lies in the warm-up)
            const uint32_t last = (j + 1) * size;
            const uint32_t count = last <= order ? 0u : last - order < size ? last - order : size;
#pragma unroll
            for (int k = 0 ; k < 15 ; ++k)
                B[j][k] = static_cast<unsigned long long>(sum[k]) + static_cast<unsigned long long>(k + 1) * count;
        }
    }
    else
    {
        // a block that is no multiple of 16 (a stream's last one): 2^P partitions, P < 4, and 256 >> P lanes to a partition,
        // which is 32 or more, so every half wavefront lies in one partition.  The half wavefronts' sums meet in LDS.
        const uint32_t size = n >> P, group = kFwThreads >> P, j = t / group;
        uint32_t sum[15];
#pragma unroll
        for (int k = 0 ; k < 15 ; ++k)
            sum[k] = 0;
        for (uint32_t i = j * size + (t & (group - 1)) ; i < (j + 1) * size ; i += group)
            if (i >= order)
            {
                const uint32_t u = fwZigzag(fwResidualOf(order, s, i));
#pragma unroll
                for (int k = 0 ; k < 15 ; ++k)
                    sum[k] += u >> k;
            }
#pragma unroll
        for (int k = 0 ; k < 15 ; ++k)
            for (int d = 16 ; d >= 1 ; d >>= 1)
                sum[k] += __shfl_xor(sum[k], d, 64);    // (32 lanes x 16 residuals below 2^21)
        if ((t & 31) == 0)
#pragma unroll
            for (int k = 0 ; k < 15 ; ++k)
                halfSum[t >> 5][k] = sum[k];
        __syncthreads();
        if (t < (15u << P))
        {
            const uint32_t m = t / 15, k = t % 15, halves = (kFwThreads / 32) >> P, last = (m + 1) * size;
            const uint32_t count = last <= order ? 0u : last - order < size ? last - order : size;
            unsigned long long bits = static_cast<unsigned long long>(k + 1) * count;
            for (uint32_t h = 0 ; h < halves ; ++h)
                bits += halfSum[m * halves + h][k];
            B[finest + m][k] = bits;
        }
    }
    __syncthreads();
    if (P == 4)
        fwChooseFrom<true>(B, nodeBits, nodeK, P, n, order, head, &rec[b]);
    else
        fwChooseFrom<false>(B, nodeBits, nodeK, P, n, order, head, &rec[b]);
}

// ------------------------------------------------------------------------------------------------------------ W2
__global__ __launch_bounds__(kFwThreads) void fwPlaceKernel(const uint32_t *blockFirst, uint32_t nStreams, const FwRec *rec,
                                                            unsigned long long *rel, FwSum *sums)
{
    const uint32_t k = blockIdx.x * (kFwThreads / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= nStreams)
        return;
    const uint32_t first = blockFirst[k], nb = blockFirst[k + 1] - first;
    unsigned long long running = kFwHeadBytes;
    uint32_t kinds[3] = { 0, 0, 0 }, lo = 0xFFFFFFFFu, hi = 0;
    for (uint32_t base = 0 ; base < nb ; base += 64)
    {
        const uint32_t idx = base + lane;
        uint32_t size = 0;
        if (idx < nb)
        {
            const FwRec r = rec[first + idx];
            size = r.frameBytes;
            kinds[0] += r.kind == FW_CONSTANT; kinds[1] += r.kind == FW_VERBATIM; kinds[2] += r.kind == FW_FIXED;
            lo = size < lo ? size : lo;
            hi = size > hi ? size : hi;
        }
        uint32_t incl = size;
        for (int d = 1 ; d < 64 ; d <<= 1)
        {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= static_cast<uint32_t>(d))
                incl += up;
        }
        if (idx < nb)
            rel[first + idx] = running + (incl - size);
        running += __shfl(incl, 63, 64);
    }
    for (int d = 32 ; d >= 1 ; d >>= 1)
    {
        for (int q = 0 ; q < 3 ; ++q)
            kinds[q] += __shfl_xor(kinds[q], d, 64);
        const uint32_t l2 = __shfl_xor(lo, d, 64), h2 = __shfl_xor(hi, d, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if (lane == 0)
        sums[k] = FwSum{ running, kinds[0], kinds[1], kinds[2], lo, hi, 0 };
}

// ------------------------------------------------------------------------------------------------------------ W3
// `len` bits (1..32) of val at bit `pos` of the frame, most significant bit first, into big-endian dwords
__device__ inline void fwPut(uint32_t *buf, uint32_t pos, uint32_t val, uint32_t len)
{
    const uint32_t dw = pos >> 5, off = pos & 31;
    if (dw + 1 >= kFwBufDw)
        return;
    const unsigned long long v = static_cast<unsigned long long>(val) << (64 - off - len);
    const uint32_t hi = static_cast<uint32_t>(v >> 32), lo = static_cast<uint32_t>(v);
    if (hi != 0) atomicOr(&buf[dw], hi);
    if (lo != 0) atomicOr(&buf[dw + 1], lo);
}
__device__ inline uint32_t fwByte(const uint32_t *buf, uint32_t j) { return (buf[j >> 2] >> (24 - 8 * (j & 3))) & 0xFF; }

// a * b modulo the CRC-16's polynomial x^16 + x^15 + x^2 + 1, polynomials over GF(2) in 16 bits
__device__ inline uint32_t fwMul16(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
    for (int i = 15 ; i >= 0 ; --i)
    {
        r = ((r << 1) ^ ((r & 0x8000) ? 0x8005u : 0u)) & 0xFFFF;
        if ((b >> i) & 1)
            r ^= a;
    }
    return r;
}
// x^(8 m) modulo that polynomial: what moves a CRC past m bytes that follow
__device__ inline uint32_t fwShift16(uint32_t m)
{
    uint32_t r = 1, g = 0x0100;
    for ( ; m != 0 ; m >>= 1, g = fwMul16(g, g))
        if (m & 1)
            r = fwMul16(r, g);
    return r;
}
// one byte through the CRC-8 (polynomial 0x07)
__device__ inline uint32_t fwCrc8Step(uint32_t c)
{
    for (int i = 0 ; i < 8 ; ++i)
        c = ((c << 1) ^ ((c & 0x80) ? 0x07u : 0u)) & 0xFF;
    return c;
}

// the residual code of sample i of a FIXED block: what goes in front of it (10 bits: coding method 00, the partition order
// and the first parameter; 4 bits: a later partition's parameter), its parameter, quotient and low part
struct FwCode { uint32_t pre, k, q, low; };
__device__ inline FwCode fwCodeOf(const FwRec &r, const uint32_t *params, const int32_t *s, uint32_t n, uint32_t i)
{
    const uint32_t size = n >> r.p, j = i / size;
    FwCode c;
    c.k = params[j];
    c.pre = i == r.order ? 10u : i == j * size ? 4u : 0u;
    const uint32_t u = fwZigzag(fwResidualOf(r.order, s, i));
    c.q = u >> c.k;
    c.low = (1u << c.k) | (u & ((1u << c.k) - 1));
    return c;
}

// Lane t of a FIXED block codes samples 16 t .. 16 t + 15.  kWhole: the block is a multiple of 16 samples and the lane has
// all 16; else the lane stops at n (the last lane of a block of any other length would code samples that are not there).
template <bool kWhole> __device__ inline uint32_t fwLaneBits(const FwRec &r, const uint32_t *params, const int32_t *s, uint32_t n, uint32_t t)
{
    const uint32_t end = kWhole || 16 * t + 16 < n ? 16 * t + 16 : n;
    uint32_t bits = 0;
    for (uint32_t i = 16 * t ; i < end ; ++i)
    {
        if (i < r.order)
            bits += 16;
        else
        {
            const FwCode c = fwCodeOf(r, params, s, n, i);
            bits += c.pre + c.q + 1 + c.k;
        }
    }
    return bits;
}
// ... and writes them from bit `pos` of the frame on
template <bool kWhole> __device__ inline void fwLanePut(uint32_t *buf, uint32_t pos, const FwRec &r, const uint32_t *params, const int32_t *s,
                                                        uint32_t n, uint32_t t)
{
    const uint32_t end = kWhole || 16 * t + 16 < n ? 16 * t + 16 : n;
    for (uint32_t i = 16 * t ; i < end ; ++i)
    {
        if (i < r.order)
        {
            if ((s[i] & 0xFFFF) != 0)
                fwPut(buf, pos, s[i] & 0xFFFF, 16);
            pos += 16;
        }
        else
        {
            const FwCode c = fwCodeOf(r, params, s, n, i);
            if (c.pre == 10)
            {
                if (r.p != 0) fwPut(buf, pos, r.p, 6);
                if (c.k != 0) fwPut(buf, pos + 6, c.k, 4);
            }
            else if (c.pre == 4 && c.k != 0)
                fwPut(buf, pos, c.k, 4);
            fwPut(buf, pos + c.pre + c.q, c.low, c.k + 1);
            pos += c.pre + c.q + 1 + c.k;
        }
    }
}

__global__ __launch_bounds__(kFwThreads) void fwWriteKernel(const int16_t *pcm, const uint64_t *offs, const uint32_t *blockFirst,
                                                            uint32_t nStreams, uint32_t nBlocks, const FwRec *rec,
                                                            const unsigned long long *rel, const unsigned long long *streamBase,
                                                            uint32_t rate, uint8_t *out)
{
    __shared__ int32_t s[kFwBlock];
    __shared__ uint32_t buf[kFwBufDw];
    __shared__ uint32_t tab16[256];
    __shared__ uint32_t params[16];
    __shared__ uint32_t waveSum[kFwThreads / 64];
    const uint32_t b = blockIdx.x, t = threadIdx.x;
    if (b >= nBlocks)
        return;
    const FwBlock w = fwBlockOf(offs, blockFirst, nStreams, b);
    const uint32_t n = w.n;
    const FwRec r = rec[b];
    const uint32_t fb = r.frameBytes, head = fwHeaderBytes(w.number, n);
    // (a record that does not fit the buffer cannot come from W1; nothing is written for one)
    if (fb > kFwMaxFrame || fb < head + 3)
        return;
    fwLoadBlock(s, pcm, w);
    for (uint32_t i = t ; i < kFwBufDw ; i += kFwThreads)
        buf[i] = 0;
    {
        uint32_t c = t << 8;
        for (int i = 0 ; i < 8 ; ++i)
            c = ((c << 1) ^ ((c & 0x8000) ? 0x8005u : 0u)) & 0xFFFF;
        tab16[t] = c;
    }
    if (t < 16)
        params[t] = rec[b].k[t];
    __syncthreads();

    // the frame header but for its CRC-8, and the subframe header
    if (t == 0)
    {
        const uint32_t code = n == kFwBlock ? 0xCu : n <= 256 ? 0x6u : 0x7u;
        fwPut(buf, 0, 0xFFF80008u | (((code << 4) | 0xD) << 8), 32);
        uint32_t pos = 32;
        const uint32_t nb = fwNumberBytes(w.number);
        if (nb == 1)
            fwPut(buf, pos, w.number, 8);
        else
        {
            fwPut(buf, pos, ((0xFFu << (8 - nb)) & 0xFF) | (w.number >> (6 * (nb - 1))), 8);
            for (uint32_t i = 1 ; i < nb ; ++i)
                fwPut(buf, pos + 8 * i, 0x80 | ((w.number >> (6 * (nb - 1 - i))) & 0x3F), 8);
        }
        pos += 8 * nb;
        if (code == 0x6) { fwPut(buf, pos, n - 1, 8); pos += 8; }
        if (code == 0x7) { fwPut(buf, pos, n - 1, 16); pos += 16; }
        fwPut(buf, pos, rate, 16);
        const uint32_t sub = r.kind == FW_CONSTANT ? 0x00u : r.kind == FW_VERBATIM ? 0x02u : 0x10u | (static_cast<uint32_t>(r.order) << 1);
        if (sub != 0)
            fwPut(buf, 8 * head, sub, 8);
        if (r.kind == FW_CONSTANT && (s[0] & 0xFFFF) != 0)
            fwPut(buf, 8 * head + 8, s[0] & 0xFFFF, 16);
    }
    const uint32_t body = 8 * head + 8;                 // the first bit behind the subframe header
    if (r.kind == FW_VERBATIM)
    {
        for (uint32_t i = t ; i < n ; i += kFwThreads)
            if ((s[i] & 0xFFFF) != 0)
                fwPut(buf, body + 16 * i, s[i] & 0xFFFF, 16);
    }
    // FIXED: the bits of this lane's 16 samples.  A block of whole 16s takes the loops of exactly 16; any other length (a
    // stream's last block) the ones bounded by n.  The branch is on the block's length: the same side in every lane.
    const bool whole = (n & 15) == 0;
    uint32_t mine = 0;
    if (r.kind == FW_FIXED && 16 * t < n)
        mine = whole ? fwLaneBits<true>(r, params, s, n, t) : fwLaneBits<false>(r, params, s, n, t);
    // an exclusive scan of the lanes' bit counts: inside each wavefront, then over the wavefronts
    uint32_t incl = mine;
    for (int d = 1 ; d < 64 ; d <<= 1)
    {
        const uint32_t up = __shfl_up(incl, d, 64);
        if ((t & 63) >= static_cast<uint32_t>(d))
            incl += up;
    }
    if ((t & 63) == 63)
        waveSum[t >> 6] = incl;
    __syncthreads();                                    // (also: the header bytes are in place)
    if (r.kind == FW_FIXED && 16 * t < n)
    {
        uint32_t pos = body + incl - mine;
        for (uint32_t v = 0 ; v < (t >> 6) ; ++v)
            pos += waveSum[v];
        if (whole)
            fwLanePut<true>(buf, pos, r, params, s, n, t);
        else
            fwLanePut<false>(buf, pos, r, params, s, n, t);
    }
    // CRC-8 of the header: lane i takes byte i past the bytes that follow it
    if (t < 64)
    {
        uint32_t c = 0;
        if (t < head - 1)
        {
            c = fwCrc8Step(fwByte(buf, t));
            for (uint32_t m = t + 1 ; m < head - 1 ; ++m)
                c = fwCrc8Step(c);
        }
        for (int d = 8 ; d >= 1 ; d >>= 1)
            c ^= __shfl_xor(c, d, 64);
        if (t == 0 && c != 0)
            fwPut(buf, 8 * (head - 1), c, 8);
    }
    __syncthreads();

    // CRC-16 of the frame but for its last two bytes: 256 parts of `each` bytes, zero bytes in front of the first part
    // (they leave a CRC that starts from 0 as it is), part t moved past the each * (255 - t) bytes behind it
    {
        const uint32_t len = fb - 2, each = (len + kFwThreads - 1) / kFwThreads, pad = each * kFwThreads - len;
        uint32_t c = 0;
        for (uint32_t j = 0 ; j < each ; ++j)
        {
            const uint32_t at = t * each + j;
            if (at >= pad)
                c = ((c << 8) & 0xFFFF) ^ tab16[(c >> 8) ^ fwByte(buf, at - pad)];
        }
        c = fwMul16(c, fwShift16(each * (kFwThreads - 1 - t)));
        for (int d = 32 ; d >= 1 ; d >>= 1)
            c ^= __shfl_xor(c, d, 64);
        __syncthreads();                                // (waveSum is read above by every lane that needs it)
        if ((t & 63) == 0)
            waveSum[t >> 6] = c;
        __syncthreads();
        if (t == 0)
        {
            uint32_t crc = 0;
            for (uint32_t v = 0 ; v < kFwThreads / 64 ; ++v)
                crc ^= waveSum[v];
            if (crc != 0)
                fwPut(buf, 8 * len, crc, 16);
        }
        __syncthreads();
    }

    // out: bytes up to the first aligned dword, dwords, the bytes that are left
    uint8_t *dst = out + streamBase[w.stream] + rel[b];
    const uint32_t mis = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(dst) & 3);
    const uint32_t lead = ((4 - mis) & 3) < fb ? ((4 - mis) & 3) : fb;
    const uint32_t nDw = (fb - lead) / 4, tail = fb - lead - 4 * nDw;
    if (t < lead)
        dst[t] = static_cast<uint8_t>(fwByte(buf, t));
    uint32_t *dst32 = reinterpret_cast<uint32_t *>(dst + lead);
    for (uint32_t d = t ; d < nDw ; d += kFwThreads)
    {
        const uint32_t j = lead + 4 * d, sh = 8 * (j & 3);
        const uint32_t w0 = buf[j >> 2], w1 = buf[(j >> 2) + 1];
        const uint32_t be = sh == 0 ? w0 : (w0 << sh) | (w1 >> (32 - sh));
        dst32[d] = __builtin_bswap32(be);
    }
    if (t < tail)
        dst[lead + 4 * nDw + t] = static_cast<uint8_t>(fwByte(buf, lead + 4 * nDw + t));
}

// ------------------------------------------------------------------------------------------------------------ W4
__device__ inline uint32_t fwRotl(uint32_t x, int c) { return (x << c) | (x >> (32 - c)); }
__device__ inline void fwMd5Block(uint32_t (&h)[4], const uint32_t (&M)[16])
{
    constexpr uint32_t K[64] = {
        0xd76aa478, 0xe8c7b756, 0x242070db, 0xc1bdceee, 0xf57c0faf, 0x4787c62a, 0xa8304613, 0xfd469501, 0x698098d8, 0x8b44f7af, 0xffff5bb1,
        0x895cd7be, 0x6b901122, 0xfd987193, 0xa679438e, 0x49b40821, 0xf61e2562, 0xc040b340, 0x265e5a51, 0xe9b6c7aa, 0xd62f105d, 0x02441453,
        0xd8a1e681, 0xe7d3fbc8, 0x21e1cde6, 0xc33707d6, 0xf4d50d87, 0x455a14ed, 0xa9e3e905, 0xfcefa3f8, 0x676f02d9, 0x8d2a4c8a, 0xfffa3942,
        0x8771f681, 0x6d9d6122, 0xfde5380c, 0xa4beea44, 0x4bdecfa9, 0xf6bb4b60, 0xbebfbc70, 0x289b7ec6, 0xeaa127fa, 0xd4ef3085, 0x04881d05,
        0xd9d4d039, 0xe6db99e5, 0x1fa27cf8, 0xc4ac5665, 0xf4292244, 0x432aff97, 0xab9423a7, 0xfc93a039, 0x655b59c3, 0x8f0ccc92, 0xffeff47d,
        0x85845dd1, 0x6fa87e4f, 0xfe2ce6e0, 0xa3014314, 0x4e0811a1, 0xf7537e82, 0xbd3af235, 0x2ad7d2bb, 0xeb86d391 };
    constexpr int S[4][4] = { { 7, 12, 17, 22 }, { 5, 9, 14, 20 }, { 4, 11, 16, 23 }, { 6, 10, 15, 21 } };
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3];
#pragma unroll
    for (int i = 0 ; i < 64 ; ++i)
    {
        const int round = i >> 4;
        const uint32_t f = round == 0 ? (b & c) | (~b & d) : round == 1 ? (d & b) | (~d & c) : round == 2 ? b ^ c ^ d : c ^ (b | ~d);
        const int g = round == 0 ? i : round == 1 ? (5 * i + 1) & 15 : round == 2 ? (3 * i + 5) & 15 : (7 * i) & 15;
        const uint32_t sum = a + f + K[i] + M[g];
        a = d; d = c; c = b;
        b = b + fwRotl(sum, S[round][i & 3]);
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d;
}

// the MD5 of each stream's samples as little-endian int16: 16 bytes a stream.  Any number of samples: `rest`, what lies behind
// the last whole 64-byte block, may be odd (a word of the padding block then holds one sample and the 0x80 byte), and from
// 28 samples on the length goes into a block of its own.  A stream may start at an odd sample: the reads are 16-bit.
__global__ __launch_bounds__(64) void fwMd5Kernel(const int16_t *pcm, const uint64_t *offs, uint32_t nStreams, uint32_t *digest)
{
    const uint32_t k = blockIdx.x * 64 + threadIdx.x;
    if (k >= nStreams)
        return;
    const uint16_t *p = reinterpret_cast<const uint16_t *>(pcm) + offs[k];
    const uint64_t nSamples = offs[k + 1] - offs[k], full = nSamples / 32;
    const uint32_t rest = static_cast<uint32_t>(nSamples % 32);         // samples behind the last whole 64-byte block
    uint32_t h[4] = { 0x67452301, 0xefcdab89, 0x98badcfe, 0x10325476 };
    uint32_t M[16];
    for (uint64_t blk = 0 ; blk < full ; ++blk, p += 32)
    {
#pragma unroll
        for (int wd = 0 ; wd < 16 ; ++wd)
            M[wd] = static_cast<uint32_t>(p[2 * wd]) | (static_cast<uint32_t>(p[2 * wd + 1]) << 16);
        fwMd5Block(h, M);
    }
    // the padding: a 0x80 byte, zeros, the length in bits in the last eight bytes of a block
#pragma unroll
    for (int wd = 0 ; wd < 16 ; ++wd)
    {
        const uint32_t at = 2 * wd;
        M[wd] = at + 1 < rest ? static_cast<uint32_t>(p[at]) | (static_cast<uint32_t>(p[at + 1]) << 16)
              : at < rest     ? static_cast<uint32_t>(p[at]) | 0x800000u
              : at == rest    ? 0x80u : 0u;
    }
    const uint64_t bits = nSamples * 16;
    if (rest > 27)                                      // (no room for the length behind the 0x80 byte)
    {
        fwMd5Block(h, M);
#pragma unroll
        for (int wd = 0 ; wd < 16 ; ++wd)
            M[wd] = 0;
    }
    M[14] = static_cast<uint32_t>(bits);
    M[15] = static_cast<uint32_t>(bits >> 32);
    fwMd5Block(h, M);
    for (int i = 0 ; i < 4 ; ++i)
        digest[4 * k + i] = h[i];
}

// ------------------------------------------------------------------------------------------------------------ base
// byte i of the 42 in front of a stream: "fLaC", the header of STREAMINFO as the last metadata block, STREAMINFO
__host__ __device__ inline uint32_t fwHeadByte(uint32_t i, uint32_t rate, uint64_t nSamples, uint32_t minFrame, uint32_t maxFrame,
                                               const uint32_t *digest)
{
    if (i < 4) return i == 0 ? 'f' : i == 1 ? 'L' : i == 2 ? 'a' : 'C';
    if (i < 8) return i == 4 ? 0x80u : i == 7 ? 34u : 0u;
    if (i < 12) return (i & 1) == 0 ? kFwBlock >> 8 : kFwBlock & 0xFF;
    if (i < 15) return (minFrame >> (16 - 8 * (i - 12))) & 0xFF;
    if (i < 18) return (maxFrame >> (16 - 8 * (i - 15))) & 0xFF;
    if (i < 26)
    {
        const uint64_t v = (static_cast<uint64_t>(rate) << 44) | (0ull << 41) | (15ull << 36) | nSamples;
        return static_cast<uint32_t>(v >> (56 - 8 * (i - 18))) & 0xFF;
    }
    // (the digest's words are little-endian)
    return digest != nullptr ? (digest[(i - 26) >> 2] >> (8 * ((i - 26) & 3))) & 0xFF : 0u;
}

__global__ __launch_bounds__(kFwThreads) void fwBaseKernel(const FwSum *sums, const uint64_t *offs, const uint32_t *blockFirst, uint32_t nStreams,
                                                           unsigned long long *base, uint64_t *outOffsets, uint64_t *total,
                                                           DcsFlacWriteInfo *info)
{
    __shared__ unsigned long long waveTotal[kFwThreads / 64];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned long long carry = 0;
    for (uint32_t first = 0 ; first < nStreams ; first += kFwThreads)   // (the same rounds for every lane: the barriers below)
    {
        const uint32_t k = first + t;
        FwSum s = {};
        if (k < nStreams)
            s = sums[k];
        unsigned long long incl = s.bytes;
        for (int d = 1 ; d < 64 ; d <<= 1)
        {
            const unsigned long long up = __shfl_up(incl, d, 64);
            if (lane >= static_cast<uint32_t>(d))
                incl += up;
        }
        if (lane == 63)
            waveTotal[wave] = incl;
        __syncthreads();
        unsigned long long before = carry;
        for (uint32_t v = 0 ; v < kFwThreads / 64 ; ++v)
        {
            if (v < wave)
                before += waveTotal[v];
            carry += waveTotal[v];
        }
        if (k < nStreams)
        {
            const unsigned long long at = before + incl - s.bytes;
            base[k] = at;
            outOffsets[k] = at;
            info[k] = DcsFlacWriteInfo{ offs[k + 1] - offs[k], s.bytes, blockFirst[k + 1] - blockFirst[k], s.nConstant, s.nVerbatim, s.nFixed,
                                        s.minFrame, s.maxFrame };
        }
        __syncthreads();                                // (waveTotal is the next round's)
    }
    if (t == 0)
    {
        outOffsets[nStreams] = carry;
        *total = carry;
    }
}

// ------------------------------------------------------------------------------------------------------------ head
__global__ __launch_bounds__(kFwThreads) void fwHeadKernel(const FwSum *sums, const uint64_t *offs, const unsigned long long *base,
                                                           const uint32_t *digest, uint32_t nStreams, uint32_t rate, uint8_t *out)
{
    const uint64_t at = static_cast<uint64_t>(blockIdx.x) * kFwThreads + threadIdx.x;
    const uint64_t k = at / kFwHeadBytes;
    if (k >= nStreams)
        return;
    const uint32_t i = static_cast<uint32_t>(at - k * kFwHeadBytes);
    out[base[k] + i] = static_cast<uint8_t>(fwHeadByte(i, rate, offs[k + 1] - offs[k], sums[k].minFrame, sums[k].maxFrame,
                                                       digest != nullptr ? digest + 4 * k : nullptr));
}

// ------------------------------------------------------------------------------------------------------------ down
// *count bytes (null: all of cap16 x 16), rounded up to 16 and never more than cap16 x 16, from src to dst: both 16-byte aligned,
// both at least cap16 x 16 bytes long
__global__ __launch_bounds__(kFwThreads) void fwDownKernel(uint4 *dst, const uint4 *src, const uint64_t *count, uint64_t cap16)
{
    uint64_t n16 = cap16;
    if (count != nullptr)
    {
        const uint64_t want = (*count + 15) / 16;
        n16 = want < cap16 ? want : cap16;
    }
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kFwThreads;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kFwThreads + threadIdx.x ; i < n16 ; i += stride)
        dst[i] = src[i];
}

// ------------------------------------------------------------------------------------------------------------ host
// what the writer's calls check before any device work; *bad = the stream at fault.  kFlacWriteAnyLength (dcs_flac_held.h; no
// caller's flag: the entry points that take whole frames only refuse it as an unknown flag before they come here) lifts
// the rule that a stream is whole frames of 240 samples: dcs_flac_write_samples and dcs_decode_streams_flac_at.
DcsStatus fwCheck(const uint64_t *offs, uint32_t n, uint32_t rate, uint32_t flags, uint32_t *bad, std::string &why)
{
    *bad = 0;
    const bool anyLength = (flags & kFlacWriteAnyLength) != 0;
    if (offs == nullptr) { why = "no sample offsets"; return DCS_ERR_INVALID_ARG; }
    if ((flags & ~(DCS_FLAC_MD5 | kFlacWriteAnyLength)) != 0) { why = "unknown flag"; return DCS_ERR_INVALID_ARG; }
    if (rate < 1 || rate > 65535) { why = "rate " + std::to_string(rate) + " outside 1..65535"; return DCS_ERR_INVALID_ARG; }
    uint64_t blocks = 0;
    for (uint32_t k = 0 ; k < n ; ++k)
    {
        *bad = k;
        if (offs[k + 1] < offs[k]) { why = "stream " + std::to_string(k) + ": offsets fall"; return DCS_ERR_INVALID_ARG; }
        const uint64_t len = offs[k + 1] - offs[k];
        if (len == 0 && anyLength) { why = "stream " + std::to_string(k) + ": no samples"; return DCS_ERR_INVALID_ARG; }
        if (len == 0 || (!anyLength && len % DCS_FRAME_SAMPLES != 0))
        {
            why = "stream " + std::to_string(k) + ": " + std::to_string(len) + " samples are not whole frames of 240";
            return DCS_ERR_INVALID_ARG;
        }
        if (len >= (1ull << 36)) { why = "stream " + std::to_string(k) + ": 2^36 samples or more"; return DCS_ERR_INVALID_ARG; }
        blocks += (len + kFwBlock - 1) / kFwBlock;
    }
    *bad = 0;
    if (blocks > 0x7FFFFFFFull) { why = "more than 2^31 - 1 blocks in one call"; return DCS_ERR_INVALID_ARG; }
    return DCS_OK;
}

// ... on a caller's flags, of which kFlacWriteAnyLength is none: whole frames only, or with anyLength any length from 1 on
DcsStatus fwCheckCall(const uint64_t *offs, uint32_t n, uint32_t rate, uint32_t flags, bool anyLength, uint32_t *bad, std::string &why)
{
    *bad = 0;
    if ((flags & ~DCS_FLAC_MD5) != 0) { why = "unknown flag"; return DCS_ERR_INVALID_ARG; }
    return fwCheck(offs, n, rate, flags | (anyLength ? kFlacWriteAnyLength : 0u), bad, why);
}

// what the streams of a call can come to at most: 42 bytes a stream, and every block VERBATIM behind the longest frame header
// (16 + 1 + 2 n + 2 for a block of n samples; W1 writes a block so where FIXED would not make it smaller)
uint64_t fwBound(const uint64_t *offs, uint32_t n, uint32_t nBlocks)
{
    return static_cast<uint64_t>(kFwHeadBytes) * n + 19ull * nBlocks + 2 * (offs[n] - offs[0]);
}

hipError_t fwCopy16(hipStream_t stream, void *dst, const void *src, const uint64_t *count, uint64_t capBytes, unsigned blockCap)
{
    const uint64_t cap16 = capBytes / 16;
    if (cap16 == 0)
        return hipSuccess;
    if (((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15u) != 0)
        return hipErrorInvalidValue;
    const unsigned blocks = static_cast<unsigned>(std::min<uint64_t>((cap16 + kFwThreads - 1) / kFwThreads, std::max(1u, blockCap)));
    hipLaunchKernelGGL(fwDownKernel, dim3(blocks), dim3(kFwThreads), 0, stream, static_cast<uint4 *>(dst), static_cast<const uint4 *>(src), count, cap16);
    return hipGetLastError();
}

}  // namespace

extern "C" uint64_t dcs_flac_write_bound(uint64_t nSamples)
{
    return kFwHeadBytes + ((nSamples + kFwBlock - 1) / kFwBlock) * static_cast<uint64_t>(kFwMaxFrame);
}

extern "C" DcsStatus dcs_flac_write_check(const uint64_t *sampleOffsets, uint32_t nStreams, uint32_t rate, uint32_t flags, uint32_t *badStream)
{
    uint32_t bad = 0;
    std::string why;
    const DcsStatus st = fwCheckCall(sampleOffsets, nStreams, rate, flags, false, &bad, why);
    if (badStream != nullptr)
        *badStream = bad;
    return st;
}

extern "C" DcsStatus dcs_flac_write_samples_check(const uint64_t *sampleOffsets, uint32_t nStreams, uint32_t rate, uint32_t flags,
                                                  uint32_t *badStream)
{
    uint32_t bad = 0;
    std::string why;
    const DcsStatus st = fwCheckCall(sampleOffsets, nStreams, rate, flags, true, &bad, why);
    if (badStream != nullptr)
        *badStream = bad;
    return st;
}

// dcs_index.cpp: the host pool
void dcsHostPoolRun(uint32_t n, int threads, const std::function<void(uint32_t)> &fn);
bool dcsIndexPoolBusy();

// the one copy from pinned staging into the caller's (pageable) buffer: megabytes of it go in parts on the host pool's threads,
// since one thread moves them slower than the link brought them down
static void fwCopyOut(uint8_t *dst, const uint8_t *src, size_t bytes)
{
    constexpr size_t kPart = size_t(1) << 20;
    const uint32_t parts = static_cast<uint32_t>((bytes + kPart - 1) / kPart);
    const int threads = std::min<int>({ static_cast<int>(parts / 2), dcs_host_threads(), 8 });
    if (threads < 2 || dcsIndexPoolBusy())
    {
        memcpy(dst, src, bytes);
        return;
    }
    dcsHostPoolRun(parts, threads, [&](uint32_t k) {
        const size_t from = static_cast<size_t>(k) * kPart;
        memcpy(dst + from, src + from, std::min(kPart, bytes - from));
    });
}

DcsStatus dcsFlacWriteQueue(DcsCtx *ctx, hipStream_t stream, const int16_t *dPcm, const uint64_t *sampleOffsets, uint32_t n, uint32_t rate,
                            uint32_t flags, FlacHeld &held, unsigned downBlocks)
{
    if (ctx == nullptr || n == 0)
        return DCS_ERR_INVALID_ARG;
    uint32_t bad = 0;
    std::string why;
    const DcsStatus checked = fwCheck(sampleOffsets, n, rate, flags, &bad, why);
    if (checked != DCS_OK)
    {
        dcsCtxSetError(ctx, why.c_str());
        return checked;
    }
    const bool md5 = (flags & DCS_FLAC_MD5) != 0;
    auto blocksOf = [&](uint32_t k) { return static_cast<uint32_t>((sampleOffsets[k + 1] - sampleOffsets[k] + kFwBlock - 1) / kFwBlock); };
    uint32_t nBlocks = 0;
    for (uint32_t k = 0 ; k < n ; ++k)
        nBlocks += blocksOf(k);

    // the device's working memory, every part on a 256-byte boundary: what goes up first, the table that comes down last
    size_t need = 0;
    auto part = [&](size_t bytes) { const size_t at = need; need += (bytes + 255) & ~size_t(255); return at; };
    const size_t nn = static_cast<size_t>(n);
    const size_t offsAt = part(sizeof(uint64_t) * (nn + 1) + sizeof(uint32_t) * (nn + 1)), firstAt = offsAt + sizeof(uint64_t) * (nn + 1);
    const size_t upBytes = need;
    const size_t recAt = part(sizeof(FwRec) * nBlocks), relAt = part(sizeof(unsigned long long) * nBlocks), sumsAt = part(sizeof(FwSum) * nn),
                 baseAt = part(sizeof(unsigned long long) * nn), digestAt = part(sizeof(uint32_t) * 4 * nn);
    const size_t tableAt = part(FlacHeld::tableBytes(n)), tableBytes = need - tableAt;
    held.n = n;
    held.bound = fwBound(sampleOffsets, n, nBlocks);
    const size_t outBytes = (static_cast<size_t>(held.bound) + 255) & ~size_t(255);
    ENCCHK(held.dWork.alloc(ctx, false, need));
    ENCCHK(held.dOut.alloc(ctx, false, outBytes));
    ENCCHK(held.hUp.alloc(ctx, true, upBytes));
    ENCCHK(held.hTable.alloc(ctx, true, tableBytes));
    ENCCHK(held.hOut.alloc(ctx, true, outBytes));

    uint8_t *dWork = held.dWork.as<uint8_t>(), *dOut = held.dOut.as<uint8_t>();
    uint64_t *hOffs = held.hUp.as<uint64_t>();
    uint32_t *hFirst = reinterpret_cast<uint32_t *>(held.hUp.as<uint8_t>() + firstAt);
    memcpy(hOffs, sampleOffsets, sizeof(uint64_t) * (nn + 1));
    hFirst[0] = 0;
    for (uint32_t k = 0 ; k < n ; ++k)
        hFirst[k + 1] = hFirst[k] + blocksOf(k);
    const uint64_t *dOffs = reinterpret_cast<const uint64_t *>(dWork + offsAt);
    const uint32_t *dBlockFirst = reinterpret_cast<const uint32_t *>(dWork + firstAt);
    FwRec *dRec = reinterpret_cast<FwRec *>(dWork + recAt);
    unsigned long long *dRel = reinterpret_cast<unsigned long long *>(dWork + relAt), *dBase = reinterpret_cast<unsigned long long *>(dWork + baseAt);
    FwSum *dSums = reinterpret_cast<FwSum *>(dWork + sumsAt);
    uint32_t *dDigest = md5 ? reinterpret_cast<uint32_t *>(dWork + digestAt) : nullptr;
    uint64_t *dOutOffsets = reinterpret_cast<uint64_t *>(dWork + tableAt), *dTotal = dOutOffsets + nn + 1;
    DcsFlacWriteInfo *dInfo = reinterpret_cast<DcsFlacWriteInfo *>(dOutOffsets + nn + 2);

    ENCCHK(fwCopy16(stream, dWork + offsAt, hOffs, nullptr, upBytes, 64));
    hipLaunchKernelGGL(fwChooseKernel, dim3(nBlocks), dim3(kFwThreads), 0, stream, dPcm, dOffs, dBlockFirst, n, nBlocks, dRec);
    ENCCHK(hipGetLastError());
    hipLaunchKernelGGL(fwPlaceKernel, dim3((n + kFwThreads / 64 - 1) / (kFwThreads / 64)), dim3(kFwThreads), 0, stream, dBlockFirst, n,
                       dRec, dRel, dSums);
    ENCCHK(hipGetLastError());
    hipLaunchKernelGGL(fwBaseKernel, dim3(1), dim3(kFwThreads), 0, stream, dSums, dOffs, dBlockFirst, n, dBase, dOutOffsets, dTotal, dInfo);
    ENCCHK(hipGetLastError());
    if (md5)
    {
        hipLaunchKernelGGL(fwMd5Kernel, dim3((n + 63) / 64), dim3(64), 0, stream, dPcm, dOffs, n, dDigest);
        ENCCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(fwHeadKernel, dim3(static_cast<uint32_t>((nn * kFwHeadBytes + kFwThreads - 1) / kFwThreads)), dim3(kFwThreads), 0, stream,
                       dSums, dOffs, dBase, dDigest, n, rate, dOut);
    ENCCHK(hipGetLastError());
    hipLaunchKernelGGL(fwWriteKernel, dim3(nBlocks), dim3(kFwThreads), 0, stream, dPcm, dOffs, dBlockFirst, n, nBlocks, dRec, dRel, dBase,
                       rate, dOut);
    ENCCHK(hipGetLastError());
    ENCCHK(fwCopy16(stream, held.hTable.as(), dWork + tableAt, nullptr, tableBytes, 64));
    ENCCHK(fwCopy16(stream, held.hOut.as(), dOut, dTotal, outBytes, downBlocks));
    return DCS_OK;
}

// The writer on PCM that lies in HBM (stream k = dPcm[sampleOffsets[k] .. sampleOffsets[k + 1]), offsets on the host): the body of
// dcs_flac_write_streams, and what dcs_decode_streams_flac (dcs_decode_flac.hip.h) hands a batch's PCM to.  Everything is
// queued on the context's stream and waited for once; the PCM has to stay until this returns.
DcsStatus dcsFlacWriteFromDevice(DcsCtx *ctx, const int16_t *dPcm, const uint64_t *sampleOffsets, uint32_t n, uint32_t rate,
                                 uint32_t flags, uint8_t *out, size_t outCap, uint64_t *outOffsets, DcsFlacWriteInfo *info)
{
    if (ctx == nullptr || outOffsets == nullptr)
        return DCS_ERR_INVALID_ARG;
    uint32_t bad = 0;
    std::string why;
    const DcsStatus checked = fwCheck(sampleOffsets, n, rate, flags, &bad, why);
    if (checked != DCS_OK)
    {
        dcsCtxSetError(ctx, why.c_str());
        return checked;
    }
    outOffsets[0] = 0;
    if (n == 0)
        return DCS_OK;
    ENCCHK(hipSetDevice(dcsCtxDevice(ctx)));
    hipStream_t stream = dcsCtxStream(ctx);
    FlacHeld held;
    // (DCS_FLAC_TRACE: where a call's time goes, on stderr)
    static const bool trace = getenv("DCS_FLAC_TRACE") != nullptr;
    const auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = trace ? now() : 0;
    const DcsStatus queued = dcsFlacWriteQueue(ctx, stream, dPcm, sampleOffsets, n, rate, flags, held, 1024);
    const double t1 = trace ? now() : 0;
    const hipError_t waited = hipStreamSynchronize(stream);         // (also for a run that failed half queued: its buffers go back)
    const double t2 = trace ? now() : 0;
    if (queued != DCS_OK)
        return queued;
    ENCCHK(waited);
    memcpy(outOffsets, held.offsets(), sizeof(uint64_t) * (static_cast<size_t>(n) + 1));
    if (info != nullptr)
        memcpy(info, held.info(), sizeof(DcsFlacWriteInfo) * n);
    const uint64_t total = held.total();
    if (out == nullptr || outCap < total)
        return DCS_ERR_CAPACITY;
    fwCopyOut(out, held.bytes(), total);
    if (trace)
        fprintf(stderr, "flac write: queue %.3f ms, wait %.3f ms, copy out %.3f ms (%llu bytes)\n", t1 - t0, t2 - t1, now() - t2,
                static_cast<unsigned long long>(total));
    return DCS_OK;
}

// dcs_flac_write_streams (whole frames only) and dcs_flac_write_samples (anyLength) on PCM in host memory
static DcsStatus fwWriteHostPcm(DcsCtx *ctx, const int16_t *pcm, const uint64_t *sampleOffsets, uint32_t nStreams, uint32_t rate,
                                uint32_t flags, bool anyLength, uint8_t *out, size_t outCap, uint64_t *outOffsets, DcsFlacWriteInfo *info)
{
    return encGuard([&]() -> DcsStatus {
        if (ctx == nullptr || outOffsets == nullptr || (nStreams != 0 && pcm == nullptr))
            return DCS_ERR_INVALID_ARG;
        uint32_t bad = 0;
        std::string why;
        const DcsStatus checked = fwCheckCall(sampleOffsets, nStreams, rate, flags, anyLength, &bad, why);
        if (checked != DCS_OK)
        {
            dcsCtxSetError(ctx, why.c_str());
            return checked;
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
        return dcsFlacWriteFromDevice(ctx, dPcm, offs.data(), nStreams, rate, flags | (anyLength ? kFlacWriteAnyLength : 0u), out, outCap,
                                      outOffsets, info);
    });
}

extern "C" DcsStatus dcs_flac_write_streams(DcsCtx *ctx, const int16_t *pcm, const uint64_t *sampleOffsets, uint32_t nStreams,
                                            uint32_t rate, uint32_t flags, uint8_t *out, size_t outCap, uint64_t *outOffsets,
                                            DcsFlacWriteInfo *info)
{
    return fwWriteHostPcm(ctx, pcm, sampleOffsets, nStreams, rate, flags, false, out, outCap, outOffsets, info);
}

extern "C" DcsStatus dcs_flac_write_samples(DcsCtx *ctx, const int16_t *pcm, const uint64_t *sampleOffsets, uint32_t nStreams,
                                            uint32_t rate, uint32_t flags, uint8_t *out, size_t outCap, uint64_t *outOffsets,
                                            DcsFlacWriteInfo *info)
{
    return fwWriteHostPcm(ctx, pcm, sampleOffsets, nStreams, rate, flags, true, out, outCap, outOffsets, info);
}

// The chain behind dcs_decode_streams_flac_at (dcs_decode_flac_rate.hip.h): a decode batch's PCM where it lies, through the
// output-rate converter (rsConvertPcm16, dcs_resample.hip.h) and from there, still in HBM, through the writer at outRate.
// The converted samples belong to `held` until the writer has returned; neither they nor the 31 250 Hz PCM come down.
// flags: DCS_RESAMPLE_AT_UNITY for the converter, flacFlags: DCS_FLAC_MD5 for the writer.  rateInfo and info are optional;
// rateInfo is filled as soon as the converter is through, whatever the writer then says.
DcsStatus dcsFlacRateFromDevice(DcsCtx *ctx, const int16_t *dPcm, const uint64_t *sampleOffsets, uint32_t n, uint32_t outRate,
                                const DcsResampleFilter *filter, uint32_t flags, uint32_t flacFlags, uint8_t *out, size_t outCap,
                                uint64_t *outOffsets, DcsFlacWriteInfo *info, DcsRateInfo *rateInfo)
{
    return encGuard([&]() -> DcsStatus {
        if (ctx == nullptr || sampleOffsets == nullptr || outOffsets == nullptr || n == 0 || (flacFlags & ~DCS_FLAC_MD5) != 0)
            return DCS_ERR_INVALID_ARG;
        DcsResampleFilter f;
        std::string why;
        const DcsStatus status = rsOutCheck(n, sampleOffsets, outRate, filter, flags, f, why);
        if (status != DCS_OK)
        {
            dcsCtxSetError(ctx, why.c_str());
            return status;
        }
        CacheArena held(ctx);
        RsConverted16 c;
        ENCTRY(rsConvertPcm16(ctx, dPcm, sampleOffsets, n, outRate, f, flags, held, c));
        if (rateInfo != nullptr)
            memcpy(rateInfo, c.info.data(), sizeof(DcsRateInfo) * n);
        return dcsFlacWriteFromDevice(ctx, c.d, c.offsets.data(), n, outRate, flacFlags | kFlacWriteAnyLength, out, outCap, outOffsets, info);
    });
}
