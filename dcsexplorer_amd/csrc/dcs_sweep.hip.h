// dcs_sweep.hip.h -- the decode half of DCS_SWEEP_MEASURE (dcs_encode_sweep and dcs_encode93a_sweep, dcs_encode.hip): the streams the encoder has
// just packed, decoded with one extra frame where they lie in HBM.  Included at the end of dcs_runtime.hip, behind
// dcs_transcode.hip.h, whose two ways of queueing a decode these are: the device path (dcsIndexWaveKernel, the device
// planner and packer, dcsDecodeKernel) on a blob that is already resident, and the host-planned batch on the same bytes
// read back, for a list the device planner cannot serve.  Volume, mixing level and channel volume are 0xFF, the decoder's
// unity setting.
#pragma once

// what the encoder knows of a stream it has sized (dcs_encode.hip declares the same); head: the third byte of an OS93a
// Type-1 stream, 1 pp bbbbb, not read of any other
struct DcsSweepStream { uint32_t nFrames, nBytes; int32_t os, formatType, formatSubType, bandsToKeep; uint32_t head; };

// an OS93a Type-1 stream: a 3-byte header (the frame count and `head`) and at least one byte of frames; every other layout
// has the frame count and 16 header bytes
static bool sweepIs93aType1(const DcsSweepStream &s) { return s.os == DCS_OS93A && s.formatType == 1; }
static uint32_t sweepMinBytes(const DcsSweepStream &s) { return sweepIs93aType1(s) ? 4 : 18; }

struct DcsSweepDecode
{
    TranscodeDecode d;
    std::vector<uint8_t> heads;
    std::vector<DcsStreamRef> refs;
};

// The stream table reads five bytes of a stream on the host (layoutStreams, planTableFor): the frame count, the type bit
// and the 1994+ sub-type bits.  The encoder knows them before the bytes exist anywhere but in HBM: heads = those five
// bytes per stream, refs = streams of nBytes bytes that begin with them.  The header byte of a band that is not kept is
// 0xFF, top bit included: a stream that keeps fewer than 1 / 2 / 3 bands has the bit of header byte 0 / 1 / 2 set whatever
// its layout, and every decoder reads it so (encHeader, dcs_encode.hip).  An OS93a Type-1 stream has no such bytes: its
// third byte is its whole header and is given as it is; of it the stream table reads the top bit, which makes the stream
// OS93a Type 1 with a 1-byte header (planTableFor), and nothing of bytes 3 and 4, which are frame data.
static void sweepRefs(const DcsSweepStream *s, uint32_t n, std::vector<uint8_t> &heads, std::vector<DcsStreamRef> &refs)
{
    heads.assign(static_cast<size_t>(n) * 8, 0);
    refs.resize(n);
    for (uint32_t k = 0 ; k < n ; ++k)
    {
        uint8_t *h = heads.data() + static_cast<size_t>(k) * 8;
        h[0] = static_cast<uint8_t>(s[k].nFrames >> 8);
        h[1] = static_cast<uint8_t>(s[k].nFrames & 0xFF);
        if (sweepIs93aType1(s[k]))
            h[2] = static_cast<uint8_t>(s[k].head);
        else
        {
            h[2] = (s[k].formatType != 0 || s[k].bandsToKeep < 1) ? 0x80 : 0;
            h[3] = ((s[k].formatSubType & 2) != 0 || s[k].bandsToKeep < 2) ? 0x80 : 0;
            h[4] = ((s[k].formatSubType & 1) != 0 || s[k].bandsToKeep < 3) ? 0x80 : 0;
        }
        refs[k] = DcsStreamRef{ h, s[k].nBytes, s[k].os, 0xFF, 0xFF, 0xFF };
    }
}

// where layoutStreams puts the streams (offs[k]), the blob's length and the bytes its device copy takes (zeroed tail included)
DcsStatus dcsSweepLayout(const DcsSweepStream *s, uint32_t n, uint64_t *offs, size_t *blobLen, size_t *blobBytes)
{
    std::vector<uint8_t> heads;
    std::vector<DcsStreamRef> refs;
    std::vector<DcsStreamLoc> locs;
    std::vector<uint64_t> firstRecord;
    uint64_t totalRec = 0;
    sweepRefs(s, n, heads, refs);
    const DcsStatus st = layoutStreams(refs.data(), n, locs, firstRecord, blobLen, &totalRec);
    if (st != DCS_OK)
        return st;
    for (uint32_t k = 0 ; k < n ; ++k)
    {
        if (locs[k].len != s[k].nBytes)
            return DCS_ERR_INVALID_ARG;
        offs[k] = locs[k].off;
    }
    *blobBytes = deviceBlobBytes(*blobLen);
    return DCS_OK;
}

// Queue the decode of the n streams at dBlob + offs[k] on the context's stream, nFrames + 1 frames each, and do not wait.
// hostBlob == NULL: the device path on dBlob (blobLen bytes and deviceBlobBytes' zeroed tail); *planFlag is then the device
// planner's word, to be read after the next wait: not 0 = the PCM is not to be used.  hostBlob = the same bytes on the
// host: the host-planned batch, *planFlag NULL.  *dPcm / *dErr: the batch's PCM and error words, stream k from frame
// (*firstFrame)[k]; they live until dcsSweepDecodeRelease, which waits for the stream.
DcsStatus dcsSweepDecodeStart(DcsCtx *ctx, const DcsSweepStream *s, uint32_t n, const uint64_t *offs, const uint8_t *dBlob, size_t blobLen,
                              const uint8_t *hostBlob, DcsSweepDecode **out, const int16_t **dPcm, const uint32_t **dErr,
                              const volatile uint32_t **planFlag, const uint32_t **firstFrame)
{
    *out = nullptr;
    DcsSweepDecode *w = new (std::nothrow) DcsSweepDecode;
    if (w == nullptr)
        return DCS_ERR_NO_MEMORY;
    *out = w;
    TranscodeDecode &d = w->d;
    d.ctx = ctx;
    sweepRefs(s, n, w->heads, w->refs);
    DcsStatus st;
    if (hostBlob != nullptr)
    {
        for (uint32_t k = 0 ; k < n ; ++k)
            w->refs[k].data = hostBlob + offs[k];
        st = transcodeDecodeOnHost(ctx, w->refs.data(), n, d);
    }
    else
        st = [&]() -> DcsStatus {
            // (any subset of the streams dcsSweepLayout placed, where it placed them)
            std::vector<uint64_t> firstRecord(n);
            uint64_t totalRec = 0;
            d.locs.resize(n);
            for (uint32_t k = 0 ; k < n ; ++k)
            {
                if (s[k].nFrames == 0 || s[k].nBytes < sweepMinBytes(s[k]) || offs[k] + s[k].nBytes > blobLen)
                    return DCS_ERR_INVALID_ARG;
                d.locs[k].off = offs[k]; d.locs[k].len = s[k].nBytes; d.locs[k].os = s[k].os; d.locs[k].firstRecord = totalRec;
                firstRecord[k] = totalRec;
                totalRec += s[k].nFrames;
            }
            DcsPlanTable table;
            DcsStatus ls = planTableFor(w->refs.data(), n, 1, d.locs.data(), firstRecord.data(), totalRec, table, d.firstJob);
            if (ls != DCS_OK)
                return ls;
            HIPCHK(ctx, hipSetDevice(ctx->device));
            HIPCHK(ctx, d.dRec.alloc(ctx, false, sizeof(DcsFrameIndex) * (totalRec ? totalRec : 1)));
            HIPCHK(ctx, d.dInfo.alloc(ctx, false, sizeof(DcsStreamInfo) * n));
            HIPCHK(ctx, d.dLocs.alloc(ctx, false, sizeof(DcsStreamLoc) * n));
            HIPCHK(ctx, hipMemcpyAsync(d.dLocs.as(), d.locs.data(), d.dLocs.bytes(), hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(ctx, hipMemsetAsync(d.dRec.as(), 0, d.dRec.bytes(), ctx->stream));
            HIPCHK(ctx, launchIndexWave(ctx->stream, reinterpret_cast<uintptr_t>(dBlob), d.dLocs.as<const DcsStreamLoc>(), n, ctx->dTables,
                                        d.dRec.as<DcsFrameIndex>(), d.dInfo.as<DcsStreamInfo>(), nullptr));
            BatchOptions o(ctx);
            o.xcdRanges = pipeXcdRanges();
            ls = createBatchPlannedOnDevice(ctx, o, table, 1, static_cast<uint32_t>(totalRec), d.dRec.as<const DcsFrameIndex>(),
                                            d.dInfo.as<const DcsStreamInfo>(), dBlob, blobLen, &d.batch);
            return ls != DCS_OK ? ls : dcs_batch_run(d.batch, nullptr);
        }();
    if (st != DCS_OK)
        return st;
    *dPcm = d.batch->dPcm.as<const int16_t>();
    *dErr = d.batch->dErr;
    *planFlag = hostBlob == nullptr ? d.batch->hStage.as<const volatile uint32_t>() : nullptr;
    *firstFrame = d.firstJob.data();
    return DCS_OK;
}

void dcsSweepDecodeRelease(DcsSweepDecode *w)
{
    if (w == nullptr)
        return;
    w->d.release();
    delete w;
}
