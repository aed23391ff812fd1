// dcs_decode_flac.hip.h -- dcs_decode_streams_flac: streams decoded as dcs_decode_streams (or, with DCS_FLAC_SEQUENCE, as
// dcs_decode_stream_sequence) decodes them, the batch's PCM handed to the FLAC writer (dcs_flac_write.hip.h, in
// dcs_encode.hip's unit) where it lies in HBM, as dcs_transcode_streams hands it to the encoder.  Included at the end of
// dcs_runtime.hip.  The FLAC bytes and the error words come down; the PCM does not.
#pragma once
#include "dcs_flac_held.h"

// dcs_flac_write.hip.h (dcsFlacWriteQueue, which a pipeline's lists go through, is declared in dcs_flac_held.h)
DcsStatus dcsFlacWriteFromDevice(DcsCtx *ctx, const int16_t *dPcm, const uint64_t *sampleOffsets, uint32_t n, uint32_t rate,
                                 uint32_t flags, uint8_t *out, size_t outCap, uint64_t *outOffsets, DcsFlacWriteInfo *info);

// What dcs_decode_streams_flac, dcs_decode_streams_at (dcs_decode_rate.hip.h) and dcs_decode_streams_flac_at
// (dcs_decode_flac_rate.hip.h) share: the list decoded as
// dcs_decode_streams decodes it (sequence: as dcs_decode_stream_sequence does, under its argument rules) by the
// host-planned batch on the context's stream, and the batch's PCM handed to `consume` where it lies in HBM, stream k =
// dPcm[sampleOffsets[k] .. sampleOffsets[k + 1]).  `check` sees the sample offsets before any device work and may refuse
// the list.  `consume` queues behind the decode and waits for the stream, so the error words are final when it returns;
// they are copied to errOut (optional) after DCS_OK and after DCS_ERR_CAPACITY.  Refusals are named in dcs_last_error as
// "<call>: ...".
template <class Check, class Consume>
static DcsStatus decodeListThen(DcsCtx *ctx, const char *call, const DcsStreamRef *streams, uint32_t nStreams, uint32_t extraFrames,
                                bool sequence, uint32_t *errOut, Check check, Consume consume)
{
    const auto refuse = [&](const std::string &why) {
        setError(ctx, (std::string(call) + ": " + why).c_str());
        return DCS_ERR_INVALID_ARG;
    };
    if (streams == nullptr || nStreams == 0)
        return refuse("no streams");
    if (sequence)
    {
        if (extraFrames < 2)
            return refuse("a sequence takes at least 2 extra frames");
        for (uint32_t k = 1 ; k < nStreams ; ++k)
            if (streams[k].os != streams[0].os || streams[k].volume != streams[0].volume || streams[k].channelVolume != streams[0].channelVolume)
                return refuse("stream " + std::to_string(k) + ": a sequence's streams share one OS version, volume and channel volume");
    }
    // the host-planned batch on the context's stream; the consumer's kernels queue behind its launch
    TranscodeDecode d;
    d.ctx = ctx;
    DcsStatus st = dcsBuildStreams(streams, nStreams, extraFrames, d.built, false, sequence);
    std::vector<uint64_t> sampleOffsets;
    if (st == DCS_OK)
    {
        dcsFlacSampleOffsets(d.built.firstJob.data(), nStreams, sampleOffsets);
        st = check(sampleOffsets.data());
    }
    if (st == DCS_OK)
    {
        BatchOptions o(ctx);
        st = createBatch(ctx, o, d.built.blob.data(), d.built.blob.size(), d.built.srcs.data(), nullptr, static_cast<uint32_t>(d.built.srcs.size()),
                         d.built.jobs.data(), static_cast<uint32_t>(d.built.jobs.size()), nullptr, 0, &d.batch);
    }
    if (st == DCS_OK)
        st = dcs_batch_run(d.batch, nullptr);
    if (st == DCS_OK)
    {
        st = consume(d.batch->dPcm.as<const int16_t>(), sampleOffsets.data());
        if ((st == DCS_OK || st == DCS_ERR_CAPACITY) && errOut != nullptr
            && hipMemcpy(errOut, d.batch->dErr, sizeof(uint32_t) * d.batch->nJobs, hipMemcpyDeviceToHost) != hipSuccess)
        {
            setError(ctx, (std::string(call) + ": the error words' copy failed").c_str());
            st = DCS_ERR_HIP;
        }
    }
    d.release();
    return st;
}

extern "C" DcsStatus dcs_decode_streams_flac(DcsCtx *ctx, const DcsStreamRef *streams, uint32_t nStreams, uint32_t extraFrames,
                                             uint32_t flags, uint8_t *out, size_t outCap, uint64_t *outOffsets,
                                             DcsFlacWriteInfo *info, uint32_t *errOut)
{
    if (ctx == nullptr || outOffsets == nullptr || (flags & ~(DCS_FLAC_MD5 | DCS_FLAC_SEQUENCE)) != 0)
        return DCS_ERR_INVALID_ARG;
    return decodeListThen(ctx, "dcs_decode_streams_flac", streams, nStreams, extraFrames, (flags & DCS_FLAC_SEQUENCE) != 0, errOut,
                          [](const uint64_t *) { return DCS_OK; },
                          [&](const int16_t *dPcm, const uint64_t *sampleOffsets) {
                              return dcsFlacWriteFromDevice(ctx, dPcm, sampleOffsets, nStreams, 31250, flags & DCS_FLAC_MD5, out, outCap,
                                                            outOffsets, info);
                          });
}
