// dcs_level.hip.h -- level control between the converter and the encoder: a gain per stream, chosen by the caller
// (DCS_LEVEL_GAIN) or from the stream's peak (DCS_LEVEL_FIT, DCS_LEVEL_NORMALIZE), and an optional clamp (DCS_LEVEL_CLIP).
// The reference has no such stage: it encodes whatever the converter gives, overshoot included; this library refuses what
// leaves the encoder's range (INTEGRATION.md rules 3, 12, 19) and here lets the caller say what should happen instead
// (rules 26-33).  Included at the end of dcs_encode.hip, the first of the headers of the chain in front of the encoder
// (dcs_resample.hip.h, dcs_wav.hip.h, dcs_flac.hip.h and dcs_encode_files.hip.h follow and use it): it shares that
// translation unit's floating-point contract (no contraction, f32 rounded at every step, denormals kept), which makes y * g
// one multiply with one rounding on the device as in a numpy restatement.
//
//   L0 peak   lvPeakKernel    the largest |y| of each stream as bits (dcs_level_streams only: the converter's R3 already
//                             gives the peak of what it writes, the pass-through included)
//   L1 scale  lvScaleKernel   y = y * g in place, then the clamp and its count; a stream with g == 1 and no clamp is left alone
//
// Everything between is host arithmetic on one float per stream: lvFitGain and LevelStage::plan.  Rounding is monotone, so
// the peak after the multiply is (float)(P * g) and needs no second reduction.  LevelStage is the stage of one call, the
// one object every driver of the chain runs it through.
#pragma once
#include <float.h>

namespace {

float fromBitsU(uint32_t b) { float x; memcpy(&x, &b, 4); return x; }

// The one guard at the C boundary of the chain's headers: a host allocation that fails is DCS_ERR_NO_MEMORY, and no
// exception leaves the C interface
template <class Body>
DcsStatus encGuard(Body body)
{
    try { return body(); }
    catch (const std::bad_alloc &) { return DCS_ERR_NO_MEMORY; }
}

// The grid of a streaming launch of 256-thread blocks: y strides over the n streams (n >= 1), x over the `items` of the
// longest one, at least one block a stream and at most blocksPerStream, or, where blocksInAll is given, as many as make
// about blocksInAll in the whole grid
dim3 streamGrid(uint32_t n, uint64_t items, uint64_t blocksInAll, uint64_t blocksPerStream)
{
    const unsigned gy = n < 65535 ? n : 65535;
    const uint64_t want = (items + 255) / 256, most = blocksInAll != 0 ? (blocksInAll + gy - 1) / gy : blocksPerStream;
    return dim3(static_cast<unsigned>(want < 1 ? 1 : want < most ? want : most), gy);
}

// the correctly rounded c / P, stepped towards 0 until (float)(P * g) <= c (P > 0, 0 < c <= 1)
__host__ __device__ inline float lvFitGain(float P, float c)
{
    float g = c / P;
    if (isinf(g))
        g = FLT_MAX;
    while (P * g > c)
        g = nextafterf(g, 0.0f);
    return g;
}

// why a DcsLevel is refused, or null
const char *lvWhyInvalid(const DcsLevel &l)
{
    if (l.mode != DCS_LEVEL_GAIN && l.mode != DCS_LEVEL_FIT && l.mode != DCS_LEVEL_NORMALIZE)
        return "level: unknown mode (DCS_LEVEL_GAIN, DCS_LEVEL_FIT or DCS_LEVEL_NORMALIZE)";
    if ((l.flags & ~DCS_LEVEL_CLIP) != 0)
        return "level: unknown flags";
    if (l.mode == DCS_LEVEL_GAIN && !(isfinite(l.gain) && l.gain > 0.0f))
        return "level: gain must be finite and greater than 0";
    if (!(l.ceiling > 0.0f && l.ceiling <= 1.0f))
        return "level: ceiling must be greater than 0 and at most 1";
    return nullptr;
}

// one stream's record from its peak (finite, >= 0) and a valid level; nClipped is the device's to count
DcsLevelInfo lvInfoOf(float P, const DcsLevel &l)
{
    float g = 1.0f;
    if (l.mode == DCS_LEVEL_GAIN)
        g = l.gain;
    else if (l.mode == DCS_LEVEL_FIT ? P > l.ceiling : P != 0.0f)
        g = lvFitGain(P, l.ceiling);
    float after = P * g;
    if ((l.flags & DCS_LEVEL_CLIP) != 0 && after > l.ceiling)
        after = l.ceiling;
    return DcsLevelInfo{ P, g, after, l.mode, 0 };
}

DcsStatus lvCheckLevels(DcsCtx *ctx, const DcsLevel *levels, uint32_t nLevels, uint32_t n, const char *unit)
{
    if (levels == nullptr || (nLevels != 1 && nLevels != n))
    {
        dcsCtxSetError(ctx, (std::string("levels: one DcsLevel, or one per ") + unit).c_str());
        return DCS_ERR_INVALID_ARG;
    }
    for (uint32_t i = 0 ; i < nLevels ; ++i)
        if (const char *why = lvWhyInvalid(levels[i]))
        {
            dcsCtxSetError(ctx, (std::string(unit) + " " + std::to_string(i) + ": " + why).c_str());
            return DCS_ERR_INVALID_ARG;
        }
    return DCS_OK;
}

// what L1 reads of one stream
struct LvStream
{
    uint64_t off, n;        // its samples in the buffer
    float gain;
    float clip;             // the ceiling its products are clamped to; 0: no clamp
};

// L0: blockIdx.y strides over the streams, x over a stream's samples
__global__ __launch_bounds__(256) void lvPeakKernel(const float *__restrict__ buf, const LvStream *__restrict__ streams, uint32_t nStreams,
                                                    uint32_t *__restrict__ peak)
{
    for (uint32_t si = blockIdx.y ; si < nStreams ; si += gridDim.y)
    {
        const LvStream s = streams[si];
        const float *p = buf + s.off;
        uint32_t top = 0;
        for (uint64_t k = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x ; k < s.n ; k += uint64_t(gridDim.x) * blockDim.x)
        {
            const uint32_t b = __float_as_uint(fabsf(p[k]));
            top = b > top ? b : top;
        }
        if (top != 0)
            atomicMax(&peak[si], top);
    }
}

__device__ inline float lvSample(float y, float g, float c, uint32_t &nClipped)
{
    y = y * g;
    if (c != 0.0f && fabsf(y) > c)
    {
        y = copysignf(c, y);
        ++nClipped;
    }
    return y;
}

// L1: blockIdx.y strides over the streams, x over a stream's samples, four at a time between the first and the last
// 16-byte boundary inside the stream (a stream starts wherever the one before it ended); the up to three samples before
// and after are the first threads' of the stream's first block
__global__ __launch_bounds__(256) void lvScaleKernel(float *__restrict__ buf, const LvStream *__restrict__ streams, uint32_t nStreams,
                                                     unsigned long long *__restrict__ nClipped)
{
    const uint64_t tid = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x, nThreads = uint64_t(gridDim.x) * blockDim.x;
    for (uint32_t si = blockIdx.y ; si < nStreams ; si += gridDim.y)
    {
        const LvStream s = streams[si];
        if (s.gain == 1.0f && s.clip == 0.0f)
            continue;
        float *p = buf + s.off;
        uint64_t head = (4 - ((reinterpret_cast<uintptr_t>(p) >> 2) & 3)) & 3;
        head = head < s.n ? head : s.n;
        const uint64_t nVec = (s.n - head) / 4, tail = head + 4 * nVec;
        float4 *v = reinterpret_cast<float4 *>(p + head);
        uint32_t clipped = 0;
        for (uint64_t k = tid ; k < nVec ; k += nThreads)
        {
            float4 q = v[k];
            q.x = lvSample(q.x, s.gain, s.clip, clipped);
            q.y = lvSample(q.y, s.gain, s.clip, clipped);
            q.z = lvSample(q.z, s.gain, s.clip, clipped);
            q.w = lvSample(q.w, s.gain, s.clip, clipped);
            v[k] = q;
        }
        if (tid < head + (s.n - tail))
        {
            const uint64_t k = tid < head ? tid : tail + (tid - head);
            p[k] = lvSample(p[k], s.gain, s.clip, clipped);
        }
        if (clipped != 0)
            atomicAdd(&nClipped[si], static_cast<unsigned long long>(clipped));
    }
}

// The level stage of one call.  levels == null && nLevels == 0: the call has none, and every step below does nothing.
// `which` (encodeFiles): stream i of the call's group is the caller's unit which[i], whose level it takes and whose record
// it fills; null: i itself.
struct LevelStage
{
    DcsCtx *ctx;
    const DcsLevel *levels;
    uint32_t nLevels;
    const uint32_t *which = nullptr;
    std::vector<DcsLevelInfo> li = {};              // one record per stream, from plan() on
    unsigned long long *dClipped = nullptr;         // the clamp's counts per stream on the device, or null where no stream clamps

    bool on() const { return levels != nullptr || nLevels != 0; }
    const DcsLevel &of(uint32_t i) const { return levels[nLevels == 1 ? 0 : which != nullptr ? which[i] : i]; }

    // the levels of a call of n units, before anything runs
    DcsStatus check(uint32_t n, const char *unit) const { return on() ? lvCheckLevels(ctx, levels, nLevels, n, unit) : DCS_OK; }

    // The records from the streams' peaks' bits (rsWalkConvolve's, lvPeakKernel's).  A peak that is not finite gives the
    // neutral record with that peak in and out: every caller refuses it by the check it makes of peakOut (finite, rsGate).
    void plan(const std::vector<uint32_t> &peak)
    {
        li.resize(on() ? peak.size() : 0);
        for (uint32_t i = 0 ; i < li.size() ; ++i)
        {
            const float P = fromBitsU(peak[i]);
            li[i] = isfinite(P) ? lvInfoOf(P, of(i)) : DcsLevelInfo{ P, 1.0f, P, of(i).mode, 0 };
        }
    }

    // the largest |x| whoever reads stream i next will see
    float top(uint32_t i, const std::vector<uint32_t> &peak) const { return on() ? li[i].peakOut : fromBitsU(peak[i]); }

    // the refusal of the entry points that hand floats back: a levelled peak that is not finite; `phrase` says what it means
    // where the peak was not finite to begin with
    DcsStatus finite(const char *phrase) const
    {
        for (uint32_t i = 0 ; i < li.size() ; ++i)
            if (!isfinite(li[i].peakOut))
            {
                dcsCtxSetError(ctx, ("stream " + std::to_string(i) + ": "
                                     + (isfinite(li[i].peakIn) ? "the levelled signal is not finite (the gain overflows)" : phrase)).c_str());
                return DCS_ERR_BAD_STREAM;
            }
        return DCS_OK;
    }

    // L1 on the streams of dBuf (stream i = [offsets[i], offsets[i + 1])) with the gains of li; nothing is launched where
    // every stream keeps its samples.  No wait: the launch is ordered before whatever reads dBuf next on the context's stream.
    DcsStatus scale(CacheArena &held, float *dBuf, const uint64_t *offsets)
    {
        const uint32_t n = static_cast<uint32_t>(li.size());
        std::vector<LvStream> hs(n);
        bool any = false, anyClip = false;
        uint64_t maxN = 0;
        for (uint32_t i = 0 ; i < n ; ++i)
        {
            const DcsLevel &l = of(i);
            // FIT and NORMALIZE end at or below the ceiling, and a stream of no samples has nothing to clamp
            const bool clip = (l.flags & DCS_LEVEL_CLIP) != 0 && l.mode == DCS_LEVEL_GAIN && offsets[i + 1] > offsets[i];
            hs[i] = LvStream{ offsets[i], offsets[i + 1] - offsets[i], li[i].gain, clip ? l.ceiling : 0.0f };
            any = any || clip || li[i].gain != 1.0f;
            anyClip = anyClip || clip;
            maxN = hs[i].n > maxN ? hs[i].n : maxN;
        }
        if (!any || maxN == 0)
            return DCS_OK;
        const hipStream_t st = dcsCtxStream(ctx);
        LvStream *dStr;
        ENCCHK(held.alloc(&dStr, n));
        ENCCHK(hipMemcpyAsync(dStr, hs.data(), sizeof(LvStream) * n, hipMemcpyHostToDevice, st));
        if (anyClip)
        {
            ENCCHK(held.alloc(&dClipped, n));
            ENCCHK(hipMemsetAsync(dClipped, 0, sizeof(unsigned long long) * n, st));
        }
        // about 2 048 blocks in all, each thread four samples a step
        hipLaunchKernelGGL(lvScaleKernel, streamGrid(n, maxN / 4, 2048, 0), dim3(256), 0, st, dBuf, dStr, n, dClipped);
        ENCCHK(hipGetLastError());
        return DCS_OK;
    }

    // the records as they stand into the caller's array (null: nowhere)
    void publish(DcsLevelInfo *to) const
    {
        for (uint32_t i = 0 ; to != nullptr && i < li.size() ; ++i)
            to[which != nullptr ? which[i] : i] = li[i];
    }

    // after the last reader of the scaled signal is queued: the clamp's counts into li (one small copy and a wait, only where
    // a stream clamps), then publish
    DcsStatus finish(DcsLevelInfo *to)
    {
        if (dClipped != nullptr)
        {
            const hipStream_t st = dcsCtxStream(ctx);
            std::vector<unsigned long long> c(li.size());
            ENCCHK(hipMemcpyAsync(c.data(), dClipped, sizeof(unsigned long long) * c.size(), hipMemcpyDeviceToHost, st));
            ENCCHK(hipStreamSynchronize(st));
            for (size_t i = 0 ; i < c.size() ; ++i)
                li[i].nClipped = c[i];
        }
        publish(to);
        return DCS_OK;
    }
};

// From floats on the device to the caller's buffer, for the entry points that hand floats back (dcs_resample_streams_level,
// dcs_level_streams): plan the level from the peaks, refuse what is not finite (`phrase`: what a peak that was not finite
// to begin with means), look at the capacity, scale, copy down, collect the clamp's counts, publish.  publishEarly: the
// records (no clamp counted yet) stand before the capacity is looked at, so DCS_ERR_CAPACITY tells the caller what the
// level would do; nothing is published where the signal is refused.
DcsStatus lvToHost(LevelStage &lv, CacheArena &held, float *dBuf, const uint64_t *offsets, const std::vector<uint32_t> &peak,
                   const char *phrase, bool publishEarly, float *out, size_t outCap, DcsLevelInfo *levelInfo)
{
    DcsCtx *ctx = lv.ctx;
    lv.plan(peak);
    ENCTRY(lv.finite(phrase));
    if (publishEarly)
        lv.publish(levelInfo);
    const uint64_t total = offsets[peak.size()] - offsets[0];
    if (out == nullptr || outCap < total)
        return DCS_ERR_CAPACITY;
    ENCTRY(lv.scale(held, dBuf, offsets));
    ENCCHK(hipMemcpyAsync(out, dBuf, sizeof(float) * total, hipMemcpyDeviceToHost, held.stream()));
    ENCCHK(hipStreamSynchronize(held.stream()));
    return lv.finish(levelInfo);
}

}  // namespace

extern "C" DcsStatus dcs_level_gain(float peak, const DcsLevel *level, float bound, float *gainOut, float *peakOut)
{
    if (level == nullptr || gainOut == nullptr || peakOut == nullptr || lvWhyInvalid(*level) != nullptr || !(isfinite(peak) && peak >= 0.0f)
        || !(bound > 0.0f))
        return DCS_ERR_INVALID_ARG;
    const DcsLevelInfo li = lvInfoOf(peak, *level);
    *gainOut = li.gain;
    *peakOut = li.peakOut;
    return li.peakOut <= bound ? DCS_OK : DCS_ERR_BAD_STREAM;
}

extern "C" DcsStatus dcs_level_streams(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams,
                                       const DcsLevel *levels, uint32_t nLevels, float *out, size_t outCap, uint64_t *outOffsets,
                                       DcsLevelInfo *levelInfo)
{
    return encGuard([&]() -> DcsStatus {
        if (ctx == nullptr || sampleOffsets == nullptr || outOffsets == nullptr)
            return DCS_ERR_INVALID_ARG;
        for (uint32_t i = 0 ; i < nStreams ; ++i)
            if (sampleOffsets[i + 1] < sampleOffsets[i])
                return DCS_ERR_INVALID_ARG;
        const uint64_t total = nStreams != 0 ? sampleOffsets[nStreams] - sampleOffsets[0] : 0;
        if (total != 0 && pcm == nullptr)
            return DCS_ERR_INVALID_ARG;
        ENCTRY(lvCheckLevels(ctx, levels, nLevels, nStreams, "stream"));        // (here the levels are not optional)
        for (uint32_t i = 0 ; i <= nStreams ; ++i)
            outOffsets[i] = nStreams != 0 ? sampleOffsets[i] - sampleOffsets[0] : 0;
        // the capacity is known before anything runs, and is refused before anything runs: no record is published then,
        // and a sample that is not finite goes unseen
        if (total != 0 && (out == nullptr || outCap < total))
            return DCS_ERR_CAPACITY;
        LevelStage lv{ ctx, levels, nLevels };
        std::vector<uint32_t> peak(nStreams, 0);
        if (total == 0)
        {
            lv.plan(peak);
            return lv.finish(levelInfo);
        }
        CacheArena held(ctx);
        const hipStream_t st = dcsCtxStream(ctx);
        std::vector<LvStream> hs(nStreams);
        uint64_t maxN = 0;
        for (uint32_t i = 0 ; i < nStreams ; ++i)
        {
            hs[i] = LvStream{ outOffsets[i], outOffsets[i + 1] - outOffsets[i], 1.0f, 0.0f };
            maxN = hs[i].n > maxN ? hs[i].n : maxN;
        }
        float *dBuf;
        LvStream *dStr;
        uint32_t *dPeak;
        ENCCHK(hipSetDevice(dcsCtxDevice(ctx)));
        ENCCHK(held.alloc(&dBuf, total));
        ENCCHK(held.alloc(&dStr, nStreams));
        ENCCHK(held.alloc(&dPeak, nStreams));
        ENCCHK(hipMemcpyAsync(dBuf, pcm + sampleOffsets[0], sizeof(float) * total, hipMemcpyHostToDevice, st));
        ENCCHK(hipMemcpyAsync(dStr, hs.data(), sizeof(LvStream) * nStreams, hipMemcpyHostToDevice, st));
        ENCCHK(hipMemsetAsync(dPeak, 0, sizeof(uint32_t) * nStreams, st));
        hipLaunchKernelGGL(lvPeakKernel, streamGrid(nStreams, maxN, 2048, 0), dim3(256), 0, st, dBuf, dStr, nStreams, dPeak);
        ENCCHK(hipGetLastError());
        ENCCHK(hipMemcpyAsync(peak.data(), dPeak, sizeof(uint32_t) * nStreams, hipMemcpyDeviceToHost, st));
        ENCCHK(hipStreamSynchronize(st));
        return lvToHost(lv, held, dBuf, outOffsets, peak, "a sample is not finite", false, out, outCap, levelInfo);
    });
}
