// dcs_transcode_decoded.h -- what the runtime's unit (dcs_transcode.hip.h defines it) gives the encoder's unit
// (dcs_encode.hip, the budget calls) of transcoding's decode: one statement of the types, read by both units.
#pragma once

#include <functional>

#include "../../include/dcs_hip.h"

// Sources decoded as dcs_transcode_streams decodes the ones it re-encodes -- one extra frame; the device walk or the host
// walk by its rule; again on the host's way where the device planner's flag was set -- and `encode` run on the batch's
// resident PCM and error words: stream k from sample sampleOffsets[k]; planFlag the device planner's word, null on the
// host's way; *unusable = the flag was set and nothing was written.  The batch is released when `encode` has returned.
using TranscodeEncode = std::function<DcsStatus(const int16_t *dPcm, const uint32_t *dErr, const volatile uint32_t *planFlag,
                                                const uint64_t *sampleOffsets, bool *unusable)>;
DcsStatus dcsTranscodeDecoded(DcsCtx *ctx, const DcsStreamRef *refs, uint32_t n, const TranscodeEncode &encode);

// what a copied source's record says: the type bit, the 1994+ sub-type bits (header bytes 1 and 2), no cutoff known
DcsEncodeInfo dcsTranscodeCopyInfo(const DcsStreamRef &s);
