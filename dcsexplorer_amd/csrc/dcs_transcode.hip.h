// dcs_transcode.hip.h -- dcs_transcode_streams: DCS streams of any family into one target family, the reference's
// DCSEncoder::EncodeDCSFile (DCSEncoder.cpp:402-587).  Included at the end of dcs_runtime.hip, behind dcs_device_path.hip.h
// (it uses the runtime's batch internals and the device path's stream layout).
//
// A source whose format fits the target is copied; every other one is decoded as the reference's recipe plays it (a fresh
// decoder, nFrames + 1 frames: dcs_decode_streams with extraFrames = 1) and encoded again.  The decode is the device path
// (upload, dcsIndexWaveKernel, the device planner and packer, dcsDecodeKernel), the host-planned batch where the device
// planner cannot serve the list or one long source dominates it; the encoder's analysis kernel (E1, dcs_encode.hip) reads the batch's int16 PCM and error
// words where they lie.  Nothing PCM-sized crosses PCIe: the stream bytes go up, the encoded bytes come down.
#pragma once

#include <functional>

#include "dcs_transcode_decoded.h"

// dcs_encode.hip
DcsStatus dcsTranscodePlan(const DcsStreamRef *src, uint32_t nStreams, const DcsEncodeParams *target, uint32_t flags,
                           int32_t *actionOut, uint64_t *boundOut, std::string &why);
DcsStatus dcsEncodeFromDevice(DcsCtx *ctx, const int16_t *dPcm, const uint32_t *dErr, const volatile uint32_t *planFlag,
                              const uint64_t *sampleOffsets, const uint32_t *label, uint32_t nStreams, const DcsEncodeParams *target,
                              bool *unusable, uint64_t *encOffsets, DcsEncodeInfo *info,
                              const std::function<uint8_t *(const uint64_t *, uint64_t)> &place);

// The re-encoded sources decoded with one extra frame: PCM and error words resident in `batch`, stream k from frame
// firstJob[k].  The batch owns them; release() waits for the context's stream, so whatever reads them has finished.
struct TranscodeDecode
{
    DcsCtx *ctx = nullptr;
    std::vector<uint8_t> blob;              // (the sources of the asynchronous uploads live until release)
    std::vector<DcsStreamLoc> locs;
    DcsBuiltStreams built;
    CacheBuf dBlob, dRec, dInfo, dLocs;
    DcsBatch *batch = nullptr;
    std::vector<uint32_t> firstJob;
    void release()
    {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        if (batch) dcs_batch_destroy(batch);
        batch = nullptr;
        for (CacheBuf *c : { &dBlob, &dRec, &dInfo, &dLocs })       // (in this order: the cache evicts what came back first)
            c->release();
    }
};

// the device path, queued on the context's stream and not waited for: whether the device planner served the list is its
// flag word (batchPlanFlag) after the next wait
static DcsStatus transcodeDecodeOnDevice(DcsCtx *ctx, const DcsStreamRef *refs, uint32_t n, TranscodeDecode &d)
{
    std::vector<DcsStreamLoc> &locs = d.locs;
    std::vector<uint64_t> firstRecord;
    size_t blobLen = 0;
    uint64_t totalRec = 0;
    DcsStatus st = layoutStreams(refs, n, locs, firstRecord, &blobLen, &totalRec);
    if (st != DCS_OK)
        return st;
    DcsPlanTable table;
    st = planTableFor(refs, n, 1, locs.data(), firstRecord.data(), totalRec, table, d.firstJob);
    if (st != DCS_OK)
        return st;
    d.blob.assign(deviceBlobBytes(blobLen), 0);
    for (uint32_t k = 0 ; k < n ; ++k)
        memcpy(d.blob.data() + locs[k].off, refs[k].data, locs[k].len);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, d.dBlob.alloc(ctx, false, d.blob.size()));
    HIPCHK(ctx, d.dRec.alloc(ctx, false, sizeof(DcsFrameIndex) * (totalRec ? totalRec : 1)));
    HIPCHK(ctx, d.dInfo.alloc(ctx, false, sizeof(DcsStreamInfo) * n));
    HIPCHK(ctx, d.dLocs.alloc(ctx, false, sizeof(DcsStreamLoc) * n));
    HIPCHK(ctx, hipMemcpyAsync(d.dBlob.as(), d.blob.data(), d.blob.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d.dLocs.as(), locs.data(), d.dLocs.bytes(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(d.dRec.as(), 0, d.dRec.bytes(), ctx->stream));
    HIPCHK(ctx, launchIndexWave(ctx->stream, reinterpret_cast<uintptr_t>(d.dBlob.as()), d.dLocs.as<const DcsStreamLoc>(), n, ctx->dTables,
                                d.dRec.as<DcsFrameIndex>(), d.dInfo.as<DcsStreamInfo>(), nullptr));
    BatchOptions o(ctx);
    o.xcdRanges = pipeXcdRanges();
    st = createBatchPlannedOnDevice(ctx, o, table, 1, static_cast<uint32_t>(totalRec), d.dRec.as<const DcsFrameIndex>(),
                                    d.dInfo.as<const DcsStreamInfo>(), d.dBlob.as<const uint8_t>(), blobLen, &d.batch);
    return st != DCS_OK ? st : dcs_batch_run(d.batch, nullptr);
}

// the host-planned batch (dcs_decode_streams' way for a list the device planner cannot serve)
static DcsStatus transcodeDecodeOnHost(DcsCtx *ctx, const DcsStreamRef *refs, uint32_t n, TranscodeDecode &d)
{
    DcsStatus st = dcsBuildStreams(refs, n, 1, d.built, false, false);
    if (st != DCS_OK)
        return st;
    d.firstJob = d.built.firstJob;
    BatchOptions o(ctx);
    st = createBatch(ctx, o, d.built.blob.data(), d.built.blob.size(), d.built.srcs.data(), nullptr, static_cast<uint32_t>(d.built.srcs.size()),
                     d.built.jobs.data(), static_cast<uint32_t>(d.built.jobs.size()), nullptr, 0, &d.batch);
    return st != DCS_OK ? st : dcs_batch_run(d.batch, nullptr);
}

// a source longer than this that has less than 1/64 of the list's frames beside it is walked on the host (see below)
static const uint64_t kTranscodeHostWalkFrames = 2048;

// dcs_transcode_decoded.h states what this is, for this unit and the encoder's
DcsStatus dcsTranscodeDecoded(DcsCtx *ctx, const DcsStreamRef *refs, uint32_t nRe, const TranscodeEncode &encode)
{
    // The device index walk is one wavefront per stream, serial over its frames (about 7.6 us a frame on MI355X): a list
    // that one long source dominates is walked faster by the host pool, and then planned on the host as well.
    uint64_t total = 0, longest = 0;
    for (uint32_t k = 0 ; k < nRe ; ++k)
    {
        const uint64_t n = (static_cast<uint64_t>(refs[k].data[0]) << 8) | refs[k].data[1];
        total += n;
        longest = n > longest ? n : longest;
    }
    const bool walkOnHost = longest > kTranscodeHostWalkFrames && longest * 64 > total;
    DcsStatus st = DCS_OK;
    for (int attempt = walkOnHost ? 1 : 0 ; attempt < 2 ; ++attempt)
    {
        TranscodeDecode d;
        d.ctx = ctx;
        st = attempt == 0 ? transcodeDecodeOnDevice(ctx, refs, nRe, d) : transcodeDecodeOnHost(ctx, refs, nRe, d);
        bool unusable = false;
        if (st == DCS_OK)
        {
            std::vector<uint64_t> sampleOffsets(static_cast<size_t>(nRe) + 1);
            for (uint32_t k = 0 ; k <= nRe ; ++k)
                sampleOffsets[k] = static_cast<uint64_t>(d.firstJob[k]) * DCS_FRAME_SAMPLES;
            st = encode(d.batch->dPcm.as<const int16_t>(), d.batch->dErr,
                        attempt == 0 ? d.batch->hStage.as<const volatile uint32_t>() : nullptr, sampleOffsets.data(), &unusable);
        }
        d.release();
        if (!unusable)
            break;
    }
    return st;
}

DcsEncodeInfo dcsTranscodeCopyInfo(const DcsStreamRef &s)
{
    const uint8_t *p = s.data;
    const bool is94 = s.os == DCS_OS94 || s.os == DCS_OS95;
    const int sub = is94 ? (s.len > 3 ? (p[3] >> 7) << 1 : 0) | (s.len > 4 ? p[4] >> 7 : 0) : 0;
    return DcsEncodeInfo{ p[2] >> 7, sub, static_cast<int32_t>((static_cast<uint32_t>(p[0]) << 8) | p[1]), static_cast<int32_t>(s.len), -1 };
}

extern "C" DcsStatus dcs_transcode_plan(const DcsStreamRef *src, uint32_t nStreams, const DcsEncodeParams *target, uint32_t flags,
                                        int32_t *actionOut, uint64_t *boundOut)
{
    std::string why;
    return dcsTranscodePlan(src, nStreams, target, flags, actionOut, boundOut, why);
}

extern "C" DcsStatus dcs_transcode_streams(DcsCtx *ctx, const DcsStreamRef *src, uint32_t nStreams, const DcsEncodeParams *target,
                                           uint32_t flags, uint8_t *out, size_t outCap, uint64_t *outOffsets, DcsTranscodeInfo *info)
{
    if (ctx == nullptr || outOffsets == nullptr)
        return DCS_ERR_INVALID_ARG;
    std::vector<int32_t> action(nStreams);
    std::vector<uint64_t> bound(nStreams);
    std::string why;
    DcsStatus st = dcsTranscodePlan(src, nStreams, target, flags, action.data(), bound.data(), why);
    if (st != DCS_OK)
    {
        if (!why.empty())
            setError(ctx, why);
        return st;
    }
    // the re-encoded sources, in input order
    std::vector<DcsStreamRef> refs;
    std::vector<uint32_t> label;
    for (uint32_t i = 0 ; i < nStreams ; ++i)
        if (action[i] == DCS_TRANSCODE_REENCODED)
        {
            refs.push_back(src[i]);
            label.push_back(i);
        }
    const uint32_t nRe = static_cast<uint32_t>(refs.size());
    std::vector<DcsEncodeInfo> encInfo(nRe);
    std::vector<uint64_t> encOffsets(static_cast<size_t>(nRe) + 1, 0);
    std::vector<uint8_t> encoded;
    // the final layout, once the re-encodes' sizes are known: copies and re-encodes in input order
    auto layout = [&](const uint64_t *encOffs) -> uint64_t {
        outOffsets[0] = 0;
        for (uint32_t i = 0, r = 0 ; i < nStreams ; ++i)
        {
            const uint64_t size = action[i] == DCS_TRANSCODE_COPIED ? src[i].len : encOffs[r + 1] - encOffs[r];
            r += action[i] == DCS_TRANSCODE_REENCODED ? 1 : 0;
            outOffsets[i + 1] = outOffsets[i] + size;
        }
        return outOffsets[nStreams];
    };
    if (nRe == 0)
    {
        if (layout(encOffsets.data()) > outCap || (nStreams != 0 && out == nullptr))
            st = DCS_ERR_CAPACITY;
    }
    else
    {
        st = dcsTranscodeDecoded(ctx, refs.data(), nRe, [&](const int16_t *dPcm, const uint32_t *dErr, const volatile uint32_t *planFlag,
                                                            const uint64_t *sampleOffsets, bool *unusable) {
            return dcsEncodeFromDevice(ctx, dPcm, dErr, planFlag, sampleOffsets, label.data(), nRe, target, unusable, encOffsets.data(),
                                       encInfo.data(), [&](const uint64_t *encOffs, uint64_t total) -> uint8_t * {
                                           if (layout(encOffs) > outCap || out == nullptr)
                                               return nullptr;
                                           encoded.resize(total);
                                           return encoded.data();
                                       });
        });
        if (st != DCS_OK && st != DCS_ERR_CAPACITY)
            return st;
    }
    if (info != nullptr)
        for (uint32_t i = 0, r = 0 ; i < nStreams ; ++i)
        {
            const uint8_t *p = src[i].data;
            DcsTranscodeInfo &t = info[i];
            t.action = action[i];
            t.srcFrames = static_cast<int32_t>((static_cast<uint32_t>(p[0]) << 8) | p[1]);
            if (action[i] == DCS_TRANSCODE_REENCODED)
                t.enc = encInfo[r++];
            else
                t.enc = dcsTranscodeCopyInfo(src[i]);
        }
    if (st != DCS_OK)
        return st;
    for (uint32_t i = 0, r = 0 ; i < nStreams ; ++i)
        if (action[i] == DCS_TRANSCODE_COPIED)
            memcpy(out + outOffsets[i], src[i].data, src[i].len);
        else
        {
            memcpy(out + outOffsets[i], encoded.data() + encOffsets[r], encOffsets[r + 1] - encOffsets[r]);
            ++r;
        }
    return DCS_OK;
}
