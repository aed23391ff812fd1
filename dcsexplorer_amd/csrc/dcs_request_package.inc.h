// dcs_request_package.inc.h -- the loads of one chunk's package, as the first instructions of dcsDecodeKernel (dcs_kernels.hip.h)
// and again in front of a wavefront's second chunk; included as text like dcs_decode_chunk.inc.h, and for the same reason.
// In scope: chunk (uint32_t), valid (bool: a padding wavefront reads package 0), and the registers the package lands in.
        const uint8_t *pkg = a.packages + (valid ? static_cast<size_t>(chunk) * (offPool + static_cast<uint32_t>(imgDw) * 4u) : 0);
        static_assert(sizeof(DcsSlot) == 32 && offsetof(DcsSlot, runStartDw) == 16 && offsetof(DcsSlot, nextJob) == 24 && DCS_PKG_SLOT_BYTES == 80, "DcsSlot / package layout");
        phead0 = reinterpret_cast<const uint4 *>(pkg)[min(lane, kHeadVec - 1)];
        if (kHeadLoads > 1)
            phead1 = reinterpret_cast<const uint4 *>(pkg)[min(lane + 64, kHeadVec - 1)];
        if (split4)
        {
            // (4-byte records, lane l's at l x 4: one dword -- ADVICE r5: an 8-byte load there was 4-byte aligned on odd lanes and
            // read past the split area on the last one; a uniform branch, the layout word comes with the kernel's arguments)
            const uint32_t raw = *reinterpret_cast<const uint32_t *>(pkg + dcsPkgOffSplit(FPW) + static_cast<uint32_t>(lane) * 4u);
            psplit = make_uint2(raw & 0xFFFFu, raw & 0xFFFF0000u);
        }
        else
            psplit = *reinterpret_cast<const uint2 *>(pkg + dcsPkgOffSplit(FPW) + static_cast<uint32_t>(lane) * 8u);
#pragma unroll
        for (int t = 0 ; t < kPoolPieces ; ++t)
        {
            // (unconditional: a predicated load would make the compiler wait for every load above before the tables
            // are even requested; lanes past the image re-read its last 16 bytes and store nothing)
            const int i = min(lane * 4 + 256 * t, imgDw - 4);
            pimg[t] = *reinterpret_cast<const uint4 *>(pkg + offPool + i * 4);
        }
