// dcs_encode_join.hip.h -- J1: the decoded int16 PCM of the DCSa containers that dcs_encode_files_budget
// searches, gathered as floats into the arena that holds the converter's output, so that a mixed file list is ONE input of
// ONE EncRun (one curve table, one allocation).  Included by dcs_encode.hip behind every other kernel of the unit: the
// kernels the code object has keep their order.
#pragma once

namespace {

// one joined stream: nSamples samples (whole frames) from sample srcOff of the decode batch's PCM, whose error words lie
// from frame srcOff / 240, to the arena from float dstOff
struct EncJoinStream { uint64_t srcOff, dstOff; uint32_t nSamples, nFrames; };

// J1: one block strides over one stream.  Lane i of a step reads sample base + i (16 bits, a wavefront 128 contiguous bytes)
// and writes float base + i (32 bits, 256 contiguous bytes): x * (1 / 32768), the value E1's int16 instantiation forms, so
// the search reads what it reads in dcs_transcode_streams_budget.  The frames' error words are ORed into streamErr[stream],
// which the driver reads beside E1's bad[] (EncInput::devStreamErr).  No LDS, no scratch.
__global__ __launch_bounds__(256) void encJoinPcmKernel(const int16_t *__restrict__ pcm, const uint32_t *__restrict__ err,
    const EncJoinStream *__restrict__ streams, float *__restrict__ arena, uint32_t *__restrict__ streamErr)
{
    const EncJoinStream s = streams[blockIdx.x];
    const int16_t *src = pcm + s.srcOff;
    float *dst = arena + s.dstOff;
    for (uint32_t i = threadIdx.x ; i < s.nSamples ; i += 256)
        dst[i] = static_cast<float>(src[i]) * (1.0f / 32768.0f);
    const uint32_t *e = err + s.srcOff / 240;
    uint32_t any = 0;
    for (uint32_t f = threadIdx.x ; f < s.nFrames ; f += 256)
        any |= e[f];
    if (any != 0)
        atomicOr(&streamErr[blockIdx.x], any);
}

// J1 queued on the context's stream, behind the decode that wrote dPcm and in front of whatever reads the arena next; no wait
DcsStatus encJoinPcm(DcsCtx *ctx, CacheArena &held, const int16_t *dPcm, const uint32_t *dErr, const uint64_t *srcOffsets, uint32_t n,
                     float *arena, const uint64_t *dstOffsets, uint32_t *dStreamErr)
{
    std::vector<EncJoinStream> hs(n);
    for (uint32_t k = 0 ; k < n ; ++k)
    {
        const uint64_t m = srcOffsets[k + 1] - srcOffsets[k];
        if (m % 240 != 0 || srcOffsets[k] % 240 != 0 || m > 65535ull * 240 || dstOffsets[k + 1] - dstOffsets[k] != m)
        {
            dcsCtxSetError(ctx, "internal error: a joined stream is not whole frames, or its place in the arena is not its length");
            return DCS_ERR_HIP;
        }
        hs[k] = EncJoinStream{ srcOffsets[k], dstOffsets[k], static_cast<uint32_t>(m), static_cast<uint32_t>(m / 240) };
    }
    const hipStream_t st = held.stream();
    EncJoinStream *dStr;
    ENCCHK(held.alloc(&dStr, n));
    // (pageable memory: the copy has left hs when the call returns)
    ENCCHK(hipMemcpyAsync(dStr, hs.data(), sizeof(EncJoinStream) * n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(encJoinPcmKernel, dim3(n), dim3(256), 0, st, dPcm, dErr, dStr, arena, dStreamErr);
    ENCCHK(hipGetLastError());
    return DCS_OK;
}

}  // namespace
