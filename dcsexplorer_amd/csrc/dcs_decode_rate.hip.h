// dcs_decode_rate.hip.h -- dcs_decode_streams_at: streams decoded as dcs_decode_streams (or, with DCS_OUT_SEQUENCE, as
// dcs_decode_stream_sequence) decodes them, the batch's PCM handed to the output-rate converter (dcs_resample.hip.h, in
// dcs_encode.hip's unit, whose floating-point contract the converter's bit equality rests on) where it lies in HBM, as
// dcs_transcode_streams hands it to the encoder.  Included at the end of dcs_runtime.hip.  The converted samples and the
// error words come down; the 31 250 Hz PCM does not.
#pragma once

// dcs_resample.hip.h
DcsStatus dcsRateCheck(DcsCtx *ctx, const uint64_t *sampleOffsets, uint32_t n, uint32_t outRate, const DcsResampleFilter *filter, uint32_t flags);
DcsStatus dcsRateFromDevice(DcsCtx *ctx, const int16_t *dPcm, const uint64_t *sampleOffsets, uint32_t n, uint32_t outRate,
                            const DcsResampleFilter *filter, uint32_t flags, int16_t *out, size_t outCapSamples, uint64_t *outOffsets,
                            DcsRateInfo *info);

extern "C" DcsStatus dcs_decode_streams_at(DcsCtx *ctx, const DcsStreamRef *streams, uint32_t nStreams, uint32_t extraFrames,
                                           uint32_t outRate, const DcsResampleFilter *filter, uint32_t flags, int16_t *out,
                                           size_t outCapSamples, uint64_t *outOffsets, DcsRateInfo *info, uint32_t *errOut)
{
    if (ctx == nullptr)
        return DCS_ERR_INVALID_ARG;
    if (outOffsets == nullptr)
    {
        setError(ctx, "dcs_decode_streams_at: outOffsets is null");
        return DCS_ERR_INVALID_ARG;
    }
    if ((flags & ~(DCS_RESAMPLE_AT_UNITY | DCS_OUT_SEQUENCE)) != 0)
    {
        setError(ctx, "dcs_decode_streams_at: unknown flags");
        return DCS_ERR_INVALID_ARG;
    }
    const uint32_t rsFlags = flags & DCS_RESAMPLE_AT_UNITY;
    const DcsStatus checked = dcsRateCheck(ctx, nullptr, 0, outRate, filter, rsFlags);
    if (checked != DCS_OK)
        return checked;
    // (DCS_RATE_TRACE: where a call's time goes, on stderr; the converter adds its own line, dcsRateFromDevice)
    static const bool trace = getenv("DCS_RATE_TRACE") != nullptr;
    const auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = trace ? now() : 0;
    double tBuilt = 0, tQueued = 0;
    const DcsStatus st = decodeListThen(ctx, "dcs_decode_streams_at", streams, nStreams, extraFrames, (flags & DCS_OUT_SEQUENCE) != 0, errOut,
                          // (a stream that decodes to no samples is refused here, before the decode is queued)
                          [&](const uint64_t *sampleOffsets) {
                              tBuilt = trace ? now() : 0;
                              return dcsRateCheck(ctx, sampleOffsets, nStreams, outRate, filter, rsFlags);
                          },
                          [&](const int16_t *dPcm, const uint64_t *sampleOffsets) {
                              tQueued = trace ? now() : 0;
                              return dcsRateFromDevice(ctx, dPcm, sampleOffsets, nStreams, outRate, filter, rsFlags, out, outCapSamples,
                                                       outOffsets, info);
                          });
    if (trace && st == DCS_OK)
        fprintf(stderr, "decode at rate: index and plan %.3f ms, batch made and queued %.3f ms, the rest %.3f ms\n", tBuilt - t0,
                tQueued - tBuilt, now() - tQueued);
    return st;
}
