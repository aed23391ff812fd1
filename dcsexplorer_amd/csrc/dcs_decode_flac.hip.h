// dcs_decode_flac.hip.h -- dcs_decode_streams_flac: streams decoded as dcs_decode_streams (or, with DCS_FLAC_SEQUENCE, as
// dcs_decode_stream_sequence) decodes them, the batch's PCM handed to the FLAC writer (dcs_flac_write.hip.h, in
// dcs_encode.hip's unit) where it lies in HBM, as dcs_transcode_streams hands it to the encoder.  Included at the end of
// dcs_runtime.hip.  The FLAC bytes and the error words come down; the PCM does not.
#pragma once
#include "dcs_flac_held.h"

// dcs_flac_write.hip.h (dcsFlacWriteQueue, which a pipeline's lists go through, is declared in dcs_flac_held.h)
DcsStatus dcsFlacWriteFromDevice(DcsCtx *ctx, const int16_t *dPcm, const uint64_t *sampleOffsets, uint32_t n, uint32_t rate,
                                 uint32_t flags, uint8_t *out, size_t outCap, uint64_t *outOffsets, DcsFlacWriteInfo *info);

extern "C" DcsStatus dcs_decode_streams_flac(DcsCtx *ctx, const DcsStreamRef *streams, uint32_t nStreams, uint32_t extraFrames,
                                             uint32_t flags, uint8_t *out, size_t outCap, uint64_t *outOffsets,
                                             DcsFlacWriteInfo *info, uint32_t *errOut)
{
    if (ctx == nullptr || streams == nullptr || nStreams == 0 || outOffsets == nullptr || (flags & ~(DCS_FLAC_MD5 | DCS_FLAC_SEQUENCE)) != 0)
        return DCS_ERR_INVALID_ARG;
    const bool sequence = (flags & DCS_FLAC_SEQUENCE) != 0;
    if (sequence)
    {
        if (extraFrames < 2)
            return DCS_ERR_INVALID_ARG;
        for (uint32_t k = 1 ; k < nStreams ; ++k)
            if (streams[k].os != streams[0].os || streams[k].volume != streams[0].volume || streams[k].channelVolume != streams[0].channelVolume)
                return DCS_ERR_INVALID_ARG;
    }
    // the host-planned batch on the context's stream; the writer's kernels queue behind its launch
    TranscodeDecode d;
    d.ctx = ctx;
    DcsStatus st = dcsBuildStreams(streams, nStreams, extraFrames, d.built, false, sequence);
    if (st == DCS_OK)
    {
        BatchOptions o(ctx);
        st = createBatch(ctx, o, d.built.blob.data(), d.built.blob.size(), d.built.srcs.data(), static_cast<uint32_t>(d.built.srcs.size()),
                         d.built.jobs.data(), static_cast<uint32_t>(d.built.jobs.size()), nullptr, 0, &d.batch);
    }
    if (st == DCS_OK)
        st = dcs_batch_run(d.batch, nullptr);
    if (st == DCS_OK)
    {
        std::vector<uint64_t> sampleOffsets;
        dcsFlacSampleOffsets(d.built.firstJob.data(), nStreams, sampleOffsets);
        st = dcsFlacWriteFromDevice(ctx, d.batch->dPcm.as<const int16_t>(), sampleOffsets.data(), nStreams, 31250, flags & DCS_FLAC_MD5,
                                    out, outCap, outOffsets, info);
        // (the writer has waited for the stream: the error words are final)
        if ((st == DCS_OK || st == DCS_ERR_CAPACITY) && errOut != nullptr
            && hipMemcpy(errOut, d.batch->dErr, sizeof(uint32_t) * d.batch->nJobs, hipMemcpyDeviceToHost) != hipSuccess)
        {
            setError(ctx, "dcs_decode_streams_flac: the error words' copy failed");
            st = DCS_ERR_HIP;
        }
    }
    d.release();
    return st;
}
