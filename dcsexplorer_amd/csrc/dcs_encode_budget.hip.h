// dcs_encode_budget.hip.h -- dcs_transcode_plan_budget and dcs_transcode_streams_budget: existing streams
// searched to a budget.  Included by dcs_encode.hip behind the chain in front of the encoder; no kernel is defined here.
// The two other budget calls stand with the calls they extend: dcs_encode_streams_at_budget in dcs_resample.hip.h,
// dcs_encode_files_budget in dcs_encode_files.hip.h.  What the three share is encodeBudgeted (dcs_encode_run.hip.h).

extern "C" DcsStatus dcs_transcode_plan_budget(const DcsStreamRef *src, uint32_t nStreams, const DcsEncodeParams *target, uint32_t flags,
                                               const DcsBudget *budget, int32_t *actionOut, uint64_t *boundOut)
{
    return encGuard([&] {
        std::string why;
        return dcsTranscodePlanBudget(src, nStreams, target, flags, budget, actionOut, boundOut, why);
    });
}

// dcs_transcode_streams with the searched family behind the decode: the plan under the budget's copy rule, the searched
// sources decoded, and one encodeBudgeted on the batch's int16 PCM (E1's int16 instantiation, as dcsEncodeFromDevice)
extern "C" DcsStatus dcs_transcode_streams_budget(DcsCtx *ctx, const DcsStreamRef *src, uint32_t nStreams, const DcsEncodeParams *target,
                                                  uint32_t flags, const DcsBudget *budget, uint8_t *out, size_t outCap,
                                                  uint64_t *outOffsets, DcsTranscodeInfo *info, DcsEncodeRdInfo *infoRd)
{
    return encGuard([&]() -> DcsStatus {
        if (ctx == nullptr || outOffsets == nullptr)
            return DCS_ERR_INVALID_ARG;
        std::vector<int32_t> action(nStreams);
        std::string why;
        DcsStatus st = dcsTranscodePlanBudget(src, nStreams, target, flags, budget, action.data(), nullptr, why);
        if (st != DCS_OK)
        {
            if (!why.empty())
                dcsCtxSetError(ctx, why.c_str());
            return st;
        }
        BudgetUnits u;
        std::vector<DcsStreamRef> refs;
        std::vector<uint32_t> label;
        for (uint32_t i = 0 ; i < nStreams ; ++i)
            if (action[i] == DCS_TRANSCODE_REENCODED)
            {
                u.search(static_cast<uint32_t>(refs.size()));
                refs.push_back(src[i]);
                label.push_back(i);
            }
            else
                u.keep(src[i].data, src[i].len);
        const uint32_t nRe = static_cast<uint32_t>(refs.size());
        const bool os93 = budgetOs93(target);
        std::vector<DcsEncodeInfo> enc;
        EncInput none;
        if (nRe == 0)
            st = encodeBudgeted(ctx, none, u, target, os93, *budget, out, outCap, outOffsets, enc, infoRd);
        else
            st = dcsTranscodeDecoded(ctx, refs.data(), nRe, [&](const int16_t *dPcm, const uint32_t *dErr, const volatile uint32_t *planFlag,
                                                                const uint64_t *sampleOffsets, bool *unusable) {
                EncInput in;
                in.sampleOffsets = sampleOffsets;
                in.nStreams = nRe;
                in.devPcm = dPcm;
                in.devErr = dErr;
                in.label = label.data();
                in.planFlag = planFlag;
                const DcsStatus s = encodeBudgeted(ctx, in, u, target, os93, *budget, out, outCap, outOffsets, enc, infoRd);
                *unusable = in.unusable;
                return s;
            });
        if (st != DCS_OK && st != DCS_ERR_CAPACITY)
            return st;
        for (uint32_t i = 0 ; info != nullptr && i < nStreams ; ++i)
        {
            info[i].action = action[i];
            info[i].srcFrames = static_cast<int32_t>((static_cast<uint32_t>(src[i].data[0]) << 8) | src[i].data[1]);
            info[i].enc = action[i] == DCS_TRANSCODE_REENCODED ? enc[i] : dcsTranscodeCopyInfo(src[i]);
        }
        return st;
    });
}
