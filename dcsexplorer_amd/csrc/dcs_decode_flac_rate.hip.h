// dcs_decode_flac_rate.hip.h -- dcs_decode_streams_flac_at: streams decoded as dcs_decode_streams (or, with
// DCS_FLAC_SEQUENCE, as dcs_decode_stream_sequence) decodes them, the batch's PCM handed where it lies in HBM to the
// output-rate converter and its output, still in HBM, to the FLAC writer (dcsFlacRateFromDevice, dcs_flac_write.hip.h, in
// dcs_encode.hip's unit: the converter's bit equality rests on that unit's floating-point contract).  Included at the end
// of dcs_runtime.hip behind dcs_decode_flac.hip.h and dcs_decode_rate.hip.h.  The FLAC bytes, the converter's per-stream
// figures and the error words come down; neither the 31 250 Hz PCM nor the converted samples do.
#pragma once

// dcs_flac_write.hip.h
DcsStatus dcsFlacRateFromDevice(DcsCtx *ctx, const int16_t *dPcm, const uint64_t *sampleOffsets, uint32_t n, uint32_t outRate,
                                const DcsResampleFilter *filter, uint32_t flags, uint32_t flacFlags, uint8_t *out, size_t outCap,
                                uint64_t *outOffsets, DcsFlacWriteInfo *info, DcsRateInfo *rateInfo);

extern "C" DcsStatus dcs_decode_streams_flac_at(DcsCtx *ctx, const DcsStreamRef *streams, uint32_t nStreams, uint32_t extraFrames,
                                                uint32_t outRate, const DcsResampleFilter *filter, uint32_t flags, uint8_t *out,
                                                size_t outCap, uint64_t *outOffsets, DcsFlacWriteInfo *info, DcsRateInfo *rateInfo,
                                                uint32_t *errOut)
{
    if (ctx == nullptr)
        return DCS_ERR_INVALID_ARG;
    if (outOffsets == nullptr)
    {
        setError(ctx, "dcs_decode_streams_flac_at: outOffsets is null");
        return DCS_ERR_INVALID_ARG;
    }
    if ((flags & ~(DCS_FLAC_MD5 | DCS_FLAC_SEQUENCE | DCS_FLAC_AT_UNITY)) != 0)
    {
        setError(ctx, "dcs_decode_streams_flac_at: unknown flags");
        return DCS_ERR_INVALID_ARG;
    }
    // the rate, the table and the converter's flag are dcs_decode_streams_at's to judge (dcsRateCheck), first without the
    // streams, then on their lengths before the decode is queued; the writer judges the converted lengths (fwCheck)
    const uint32_t rsFlags = (flags & DCS_FLAC_AT_UNITY) != 0 ? DCS_RESAMPLE_AT_UNITY : 0u;
    const DcsStatus checked = dcsRateCheck(ctx, nullptr, 0, outRate, filter, rsFlags);
    if (checked != DCS_OK)
        return checked;
    return decodeListThen(ctx, "dcs_decode_streams_flac_at", streams, nStreams, extraFrames, (flags & DCS_FLAC_SEQUENCE) != 0, errOut,
                          [&](const uint64_t *sampleOffsets) { return dcsRateCheck(ctx, sampleOffsets, nStreams, outRate, filter, rsFlags); },
                          [&](const int16_t *dPcm, const uint64_t *sampleOffsets) {
                              return dcsFlacRateFromDevice(ctx, dPcm, sampleOffsets, nStreams, outRate, filter, rsFlags, flags & DCS_FLAC_MD5,
                                                           out, outCap, outOffsets, info, rateInfo);
                          });
}
