// dcs_decode_chunk.inc.h -- the body of dcsDecodeKernel (dcs_kernels.hip.h) for ONE chunk, from its package in registers to its
// PCM in memory.  Not a header of its own: the kernel includes it once per chunk a wavefront decodes, as straight-line code, with
//   PASS  (constexpr int)       0, or 1 for a wavefront's second chunk
//   chunk (const uint32_t)      the chunk
//   kPace (constexpr PaceSchedule), stamp (const Stamper)
// in scope, next to everything the kernel's prologue has set up.  (Text included twice rather than a lambda called twice: with the
// body in a function of its own, even one inlined at its only call, the one-chunk kernels came out of the compiler with other
// code than before -- other register allocation, some thirty more packed adds in the transforms.)
    DCS_STAMP(1);

    // hand the package head to the lanes: through this wavefront's bit pool (filled with the image right after)
    struct { uint32_t job; uint32_t prevSlot, flags, nSrc, shiftXform; uint32_t firstSrc, prevJob, poolOff, bpl; } slot;
    uint32_t exportNext;                                // where the chunk's tail for another chunk is due (a scalar: see below)
    uint4 pd0, pd1, phdr;
    uint2 pd2;
    // (8 frames per wavefront: this lane plans bands q and q + 8 of its slot's frame, see below.  Their header and band-type bytes
    // are read as bytes where the head lies in LDS anyway -- picking them out of the eight registers by a band number that is
    // the lane's costs a dozen selects)
    uint32_t planHdr0 = 0, planHdr1 = 0, planType0 = 0, planType1 = 0;
    {
        uint4 *scratch = reinterpret_cast<uint4 *>(L.pool());
        static_assert(kHeadVec * 16 <= poolDwords(FPW) * 4, "the package head fits in the bit pool");
        if (lane < kHeadVec)
            scratch[lane] = phead0;
        if (kHeadLoads > 1 && lane + 64 < kHeadVec)
            scratch[lane + 64] = phead1;
        waveSync();
        const uint4 *sp5 = scratch + 5 * s;             // (dcs_common.h: five pieces per slot)
        const uint4 s0 = sp5[0];
        pd0 = sp5[1]; pd1 = sp5[2];
        const uint4 d2v = sp5[3];
        pd2 = make_uint2(d2v.x, d2v.y);
        phdr = sp5[4];
        if constexpr (bandPlanInLds(FPW))
        {
            // (DcsFrameIndex.bandType: bytes 4..19 of a slot's third and fourth pieces; the stream header: its fifth piece)
            const unsigned char *bytes = reinterpret_cast<const unsigned char *>(sp5) + q;
            planType0 = bytes[36]; planType1 = bytes[44];
            planHdr0 = bytes[64]; planHdr1 = bytes[72];
        }
        waveSync();
        slot.job = s0.x;
        slot.prevSlot = s0.y & 0xFFu; slot.flags = (s0.y >> 8) & 0xFFu; slot.nSrc = (s0.y >> 16) & 0xFFu; slot.shiftXform = s0.y >> 24;
        slot.firstSrc = s0.z; slot.prevJob = s0.w;
        slot.poolOff = d2v.z & 0xFFFFu;
        slot.bpl = (d2v.z >> 16) & 0xFFu;
        // (DCS_SLOT_EXPORT: the job whose first samples this frame's tail overlaps into.  A chunk has at most one such frame, its
        // last one, so this is the same for every lane: taken into a scalar register here, no vector register lives through phase 1)
        const unsigned long long exportSlots = __ballot(lane < FPW && !(slot.flags & DCS_SLOT_EMPTY) && (slot.flags & DCS_SLOT_EXPORT) != 0);
        exportNext = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(d2v.w), exportSlots != 0 ? static_cast<int>(__builtin_ctzll(exportSlots)) : 0));
    }

    // ---- the band plan of the first-source round (planBand94, unpack94): two records per lane, lane (s, q)'s at lane and
    // lane + 64 of the [16][FPW] array.  Skipped where no frame of the chunk starts with a 1994+ source (a uniform branch).
    if constexpr (bandPlanInLds(FPW))
    {
        const int fmt0 = static_cast<int>((pd0.z >> 16) & 0xFFu);
        if (__any(!(slot.flags & DCS_SLOT_EMPTY) && slot.nSrc != 0 && fmt0 >= DCS_FMT_94_T0))
        {
            uint2 *plan = reinterpret_cast<uint2 *>(L.plan());
            const uint2 *tmpl = reinterpret_cast<const uint2 *>(smem + planTableOffset(FPW));
            const bool type1 = fmt0 != DCS_FMT_94_T0;
            const uint32_t keyLim = type1 ? 16u : 17u;
            const uint32_t cls0 = !type1 ? DCS_B94_TYPE0 : q < 3 ? 0u : q < 6 ? 17u : 34u, cls1 = type1 ? 34u : DCS_B94_TYPE0;
            const uint32_t pre = (type1 && q < 3) ? (pd2.y >> (4 * q)) & 15u : 0u;
            plan[lane] = planBand94(L.tables(), tmpl, planHdr0, planType0, cls0, keyLim, q < 2 ? 7u + q : 16u, pre);
            plan[lane + 64] = planBand94(L.tables(), tmpl, planHdr1, planType1, cls1, keyLim, q == 7 ? 32u : 16u, 0u);
        }
    }

    // the lane's transform constants for the chunk's first frame (the whole chunk, normally): requested now, needed in
    // phase 2.  (Requesting them with the first loads of the kernel, which a batch flag could allow when every job runs
    // the same transform, makes that first round trip longer: 4 % slower on the 4 096-frame batch.)
    // (a wavefront's second chunk keeps the first one's while the family stays the same)
    // (SOLE, an even-deal kernel: every job of the batch runs the 1994+ transform -- createBatch sets DCS_BATCH_EVEN_DEAL for no
    // other -- so the constants are the wavefront's, requested with its first chunk)
    if constexpr (SOLE)
    {
        if (PASS == 0)
            loadLaneConsts(a.tables, lane, DCS_XFORM_94, C);
    }
    else
    {
        const int firstXform = __builtin_amdgcn_readfirstlane(static_cast<int>(slot.shiftXform >> 4)) == DCS_XFORM_94 ? DCS_XFORM_94 : DCS_XFORM_93;
        if (PASS == 0 || firstXform != constsXform)
        {
            constsXform = firstXform;
            loadLaneConsts(a.tables, lane, constsXform, C);
        }
    }
    // the bit pool of round 0: a straight copy of the package's image
#pragma unroll
    for (int t = 0 ; t < kPoolPieces ; ++t)
    {
        const int i = lane * 4 + 256 * t;
        const bool in = i < imgDw;                  // (behind the image the pool is zero, as it was when the image had the pool's length)
        if (i < poolDwords(FPW))
            ldsWrite4(L.pool() + i, in ? pimg[t].x : 0u, in ? pimg[t].y : 0u, in ? pimg[t].z : 0u, in ? pimg[t].w : 0u);
    }

    // ---- job of this lane's slot ---------------------------------------------------------------------------
    const bool live = !(slot.flags & DCS_SLOT_EMPTY);
    struct { uint32_t firstSrc; int nSrc; int volShift; int xform; uint32_t prev; } job;
    job.firstSrc = slot.firstSrc; job.nSrc = slot.nSrc; job.volShift = slot.shiftXform & 15;
    job.xform = slot.shiftXform >> 4; job.prev = slot.prevJob;

    // ---- phase 1: unpack, one round per source index -------------------------------------------------
    uint32_t err = 0;
    {
        uint32_t *pool = L.pool();
        const DcsLdsTables *T = L.tables();
        uint16_t *row = L.row(s);
        const uint32_t *blobW = reinterpret_cast<const uint32_t *>(a.blob);
        const uint32_t blobWords = static_cast<uint32_t>((a.blobLen + 3) >> 2);
        const int myNSrc = live ? job.nSrc : 0;

        // one unpack round = the r-th source of every frame of the chunk.  R0 (the first source, in most batches the
        // only one): the planner has put into the slot record where the compressed bytes, the stream header and
        // the lane's split record lie, so all of it is requested in ONE memory round trip together with the
        // descriptor; for further sources (multi-channel mixes) the addresses follow from the descriptor.
        auto unpackRound = [&](auto r0tag, const int r)
        {
            constexpr bool R0 = decltype(r0tag)::value;
            const bool has = r < myNSrc;
            // the descriptor: identical addresses within a slot's sub-lanes
            const uint4 *sdp = reinterpret_cast<const uint4 *>(&a.srcs[has ? job.firstSrc + r : 0]);
            uint4 d0 = make_uint4(0, 0, 0, 0), d1 = d0;
            uint2 d2 = make_uint2(0, 0);
            uint2 sp = make_uint2(0, 0);
            const int bplSlot = slot.bpl;
            if (R0)
            {
                // (SOLE: taken as they are.  Both packers write a slot without a source -- a padding slot, a silent job -- as zeros
                // in all of these, dcsPkgSlotEntry and dcsLaneSplit in dcs_package.h; only hdrLen below wants something else)
                if constexpr (SOLE) { d0 = pd0; d1 = pd1; d2 = pd2; sp = psplit; }
                else if (has) { d0 = pd0; d1 = pd1; d2 = pd2; sp = psplit; }
            }
            else if (has) { d0 = sdp[0]; d1 = sdp[1]; d2 = *reinterpret_cast<const uint2 *>(sdp + 2); }
            // DcsSrcDesc: [0] streamOff lo, [1] streamOff hi, [2] mixMul | format<<16 | hdrLen<<24,
            // idx at byte 12: [3] bitOff, [4] nBits | hdrBits<<16, [5..8] bandType, [9] preAdj | nBands<<16 | flags<<24,
            // [10..39] split[15], two dwords each
            const uint64_t streamOff = static_cast<uint64_t>(d0.x) | (static_cast<uint64_t>(d0.y) << 32);
            const uint32_t mixMul = d0.z & 0xFFFFu;
            const int format = static_cast<int>((d0.z >> 16) & 0xFFu);
            const int hdrLen = has ? static_cast<int>(d0.z >> 24) : 16;
            const uint32_t bitOff = d0.w;
            const uint32_t nBits = d1.x & 0xFFFFu, hdrBits = d1.x >> 16;
            const int nBands = static_cast<int>((d2.y >> 16) & 0xFFu);
            const uint32_t flags = d2.y >> 24;
            const bool serial = R0 ? bplSlot == 0 : ((flags & DCS_IDX_SERIAL) != 0 || SUB == 1);

            Quarter Q;
            Q.t0 = d1.y; Q.t1 = d1.z; Q.t2 = d1.w; Q.t3 = d2.x;
            Q.preAdj = d2.y & 0xFFFFu;

            const uint64_t bitPos = (streamOff + 2 + static_cast<uint64_t>(hdrLen)) * 8 + bitOff;
            // ---- stage the compressed bytes into the bit pool, byte-swapped so that bit 31 of a dword is the next
            // stream bit.  All loads are issued before the first store, so their latencies overlap.
            uint32_t off;                                                   // pool dword of this lane's frame
            bool fits;
            if (R0)
            {
                // (the pool was filled from the package's image)
                off = min(static_cast<uint32_t>(slot.poolOff), static_cast<uint32_t>(poolDwords(FPW) - 1));
                fits = true;
            }
            else
            {
                // further sources: one coalesced run of dwords per slot, positions from a prefix sum over the slots
                const uint32_t startDw = static_cast<uint32_t>(bitPos >> 5);
                const uint32_t nDw = (has && q == 0) ? dcsPoolDwords(streamOff, static_cast<uint32_t>(hdrLen), bitOff, nBits) : 0u;
                uint32_t incl = nDw;
#pragma unroll
                for (int d = 1 ; d < 64 ; d <<= 1)
                {
                    const uint32_t up = __shfl_up(incl, d);
                    if (lane >= d) incl += up;
                }
                const uint32_t offMine = incl - nDw;
                off = __shfl(offMine, s);                                   // from the slot's q = 0 lane
                const uint32_t nDwSlot = __shfl(nDw, s);
                fits = off + nDwSlot <= static_cast<uint32_t>(poolDwords(FPW));
                constexpr int kStageUnroll = FPW < 8 ? FPW : 8;
                for (int t0 = 0 ; t0 < FPW ; t0 += kStageUnroll)
                {
                    uint32_t v[kStageUnroll], dst[kStageUnroll];
                    bool any64 = false;
#pragma unroll
                    for (int u = 0 ; u < kStageUnroll ; ++u)
                    {
                        const uint32_t n = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(nDw), t0 + u));
                        const uint32_t st = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(startDw), t0 + u));
                        const uint32_t o = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(offMine), t0 + u));
                        const bool room = o + n <= static_cast<uint32_t>(poolDwords(FPW));
                        const uint32_t w = st + static_cast<uint32_t>(lane);
                        const bool mine = room && static_cast<uint32_t>(lane) < n;
                        v[u] = (mine && w < blobWords) ? blobW[w] : 0u;
                        dst[u] = mine ? o + static_cast<uint32_t>(lane) : 0xFFFFFFFFu;
                        any64 = any64 || (room && n > 64);
                    }
#pragma unroll
                    for (int u = 0 ; u < kStageUnroll ; ++u)
                        if (dst[u] != 0xFFFFFFFFu)
                            pool[dst[u]] = __builtin_bswap32(v[u]);
                    if (any64)
                    {
                        // frames longer than 256 bytes: the rest, slot by slot
                        for (int u = 0 ; u < kStageUnroll ; ++u)
                        {
                            const uint32_t n = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(nDw), t0 + u));
                            const uint32_t st = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(startDw), t0 + u));
                            const uint32_t o = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(offMine), t0 + u));
                            if (o + n > static_cast<uint32_t>(poolDwords(FPW)))
                                continue;
                            for (uint32_t i = static_cast<uint32_t>(lane) + 64 ; i < n ; i += 64)
                            {
                                const uint32_t w = st + i;
                                pool[o + i] = w < blobWords ? __builtin_bswap32(blobW[w]) : 0u;
                            }
                        }
                    }
                }
            }

            if (R0) DCS_STAMP(2);
            // the stream header: 16 bytes at streamOff + 2 (round 0: from the package, aligned and masked there)
            if (R0)
            {
                if constexpr (SOLE) { Q.h0 = phdr.x; Q.h1 = phdr.y; Q.h2 = phdr.z; Q.h3 = phdr.w; }      // (zeros, as above)
                else { Q.h0 = has ? phdr.x : 0u; Q.h1 = has ? phdr.y : 0u; Q.h2 = has ? phdr.z : 0u; Q.h3 = has ? phdr.w : 0u; }
            }
            else
            {
                const uint32_t hw = static_cast<uint32_t>((streamOff + 2) >> 2);
                const uint32_t sh = static_cast<uint32_t>((streamOff + 2) & 3);
                uint32_t hdrW[5];
#pragma unroll
                for (int i = 0 ; i < 5 ; ++i)
                    hdrW[i] = (has && hw + i < blobWords) ? blobW[hw + i] : 0u;
                Q.h0 = __builtin_amdgcn_alignbyte(hdrW[1], hdrW[0], sh);
                Q.h1 = __builtin_amdgcn_alignbyte(hdrW[2], hdrW[1], sh);
                Q.h2 = __builtin_amdgcn_alignbyte(hdrW[3], hdrW[2], sh);
                Q.h3 = __builtin_amdgcn_alignbyte(hdrW[4], hdrW[3], sh);
                if (hdrLen == 1)
                {
                    Q.h0 &= 0xFFu; Q.h1 = Q.h2 = Q.h3 = 0;
                }
            }
            waveSync();

            if (R0) DCS_STAMP(3);
            // ---- which part of the frame this lane unpacks, and from which decoder state ----------------
            const bool ok = has && fits && unpacker;
            if (has && !fits && q == 0)
                err |= DCS_FRAME_FATAL | DCS_FRAME_STOP;            // cannot happen with the library's planner
            if (has && q == 0)
                err |= flags >> 4;                                  // errors the index pass met before band 0 (:1771-1773)
            uint32_t relBits = hdrBits;                             // band 0 starts behind the 1994+ frame header
            Q.bandBase = 0;
            Q.outIdx = 1;
            Q.prv = 0; Q.prvDelta = 0;
            Q.subType = (format == DCS_FMT_93B_T1) ? 0 : 2;
            Q.reuse = false; Q.first = true;
            Q.midEnd = Q.midStart = Q.midStraddle = false;
            Q.endIdx = 0;
            // (the batch's packages carry the even deal, dcs_package.h: first source, eight lanes per frame)
            constexpr bool evenDeal = R0 && SUB == 8 && EVEN;
            if (serial)
                Q.nb = (q == 0) ? nBands : 0;
            else
            {
                const int nb16 = min(nBands, 16);
                if (R0)
                {
                    // the packer dealt the bands out (dcsLaneFirstBand): this lane's first
                    // band comes with its split record, its last one is where the next lane of the frame starts
                    const bool f93a = format == DCS_FMT_93A_T1;
                    const int nbEnd = f93a ? min(nBands, 18) : nb16;
                    const int myBase = (sp.x & 0x8000u) ? nbEnd
                                     : static_cast<int>(sp.y >> 28) + ((f93a && (sp.y & (DCS_SPLIT_BASE16 << 16)) != 0) ? 16 : 0);
                    const int nextBase = __shfl(myBase, lane + FPW);
                    Q.bandBase = myBase;
                    Q.nb = max((q == SUB - 1 ? nbEnd : nextBase) - myBase, 0);
                    if (SUB == 16)
                    {
                        // the frame's last lane may hold the second half of band 15; the lane before it then stops there
                        const bool mid = format >= DCS_FMT_94_T0 && q == SUB - 1 && myBase == 15 && (sp.y & (DCS_SPLIT_MID15 << 16)) != 0;
                        const bool nextMid = __shfl(static_cast<int>(mid), lane + FPW) != 0;
                        Q.midStart = mid;
                        Q.midStraddle = mid && (sp.y & (DCS_MID15_STRADDLE << 16)) != 0;
                        Q.midEnd = q == SUB - 2 && nextMid;
                        if (Q.midEnd)
                            Q.nb = 16 - myBase;
                    }
                    if constexpr (evenDeal)
                    {
                        // the even deal: a lane may start with the second half of a band (its record says so), and then the lane
                        // before it stops there -- at the output index the record names, a sample later behind a straddling code
                        const bool mid = format >= DCS_FMT_94_T0 && !(sp.x & 0x8000u) && (sp.y & (DCS_SPLIT_MID15 << 16)) != 0;
                        const bool nextMid = __shfl(static_cast<int>(mid), lane + FPW) != 0 && q != SUB - 1;
                        const int nextIdx = __shfl(static_cast<int>((sp.y >> 16) & 0x1FFu), lane + FPW);
                        Q.midStart = mid;
                        Q.midStraddle = mid && (sp.y & (DCS_MID15_STRADDLE << 16)) != 0;
                        Q.midEnd = nextMid;
                        Q.endIdx = nextIdx;
                        if (nextMid)
                            Q.nb = min(nextBase + 1, nbEnd) - myBase;
                    }
                }
                else
                {
                    // further sources of a frame: the deal worked out here, bpl = ceil(nBands / SUB) (OS93a Type 1: bands in
                    // order, the tail handled below)
                    const int bpl = max((nb16 + SUB - 1) / SUB, 1);
                    if (format == DCS_FMT_93A_T1)
                    {
                        Q.bandBase = min(q * bpl, nb16);
                        Q.nb = min(max(nb16 - Q.bandBase, 0), bpl);
                    }
                    else
                    {
                        Q.bandBase = dcsLaneFirstBand(format, q, bpl, nb16);
                        Q.nb = (q == SUB - 1 ? nb16 : dcsLaneFirstBand(format, q + 1, bpl, nb16)) - Q.bandBase;
                    }
                }
                if (q != 0 && Q.nb != 0)
                {
                    if (!R0)
                        sp = reinterpret_cast<const uint2 *>(sdp)[5 + Q.bandBase - 1];
                    const uint32_t sp0 = sp.x, sp1 = sp.y;
                    relBits = sp0 & 0x7FFFu;
                    Q.prv = sp0 >> 16;
                    Q.prvDelta = sp1 & 0xFFFFu;
                    const uint32_t st = sp1 >> 16;
                    Q.outIdx = static_cast<int>(st & 0x1FFu);
                    Q.subType = static_cast<int>((st >> 9) & 3u);
                    Q.reuse = (st & 0x800u) != 0;
                    Q.first = false;
                }
            }
            const uint32_t inPool = static_cast<uint32_t>(bitPos & 31) + relBits;
            const uint32_t *brAt = pool + (ok ? off + (inPool >> 5) : 0u);
            const int brBit = static_cast<int>(inPool & 31);

            if (R0) DCS_STAMP(12);
            // every lane enters the unpackers (their symbol loops are wave-convergent); lanes without a
            // source of that family are masked off inside
            const bool is94 = ok && format >= DCS_FMT_94_T0;
            // OS93a Type 1: up to 18 bands, the lane that holds band 15 also takes 16 and 17; a lane whose split
            // record says the frame ended earlier has nothing to do
            const bool is93a = ok && format == DCS_FMT_93A_T1 && Q.nb != 0 && !(Q.bandBase != 0 && Q.reuse);
            const bool is93 = ok && format < DCS_FMT_93A_T1;
            if (__any(is94))
            {
                BR94 br;
                br.init(brAt, brBit);
                // (first source, 8 lanes per frame: the bands' set-up comes from the plan; the record of this lane's first band)
                const uint32_t planAt = (R0 && bandPlanInLds(FPW))
                    ? static_cast<uint32_t>(reinterpret_cast<uintptr_t>((LdsBytePtr)L.plan())) + static_cast<uint32_t>(Q.bandBase * FPW + s) * kPlanRecBytes
                    : 0u;
                err |= unpack94<R0, BR94, SUB, evenDeal>(T, row, br, Q, format, mixMul, is94, stamp, planAt);
            }
            // (SOLE, an even-deal kernel: every source of the batch is a 1994+ frame, createBatch sets DCS_BATCH_EVEN_DEAL for no
            // other; no 1993-family code.  The even-deal kernels of batches with a second source keep it: every cut of it tried
            // sent one of them to scratch memory, profiles/NOTES.md 57)
            if constexpr (!SOLE)
            {
            BR93 br;
            br.init(brAt, brBit);
            if (__any(is93))
                err |= unpack93<R0, BR93>(T, row, br, Q, format, mixMul, is93, stamp);
            if (is93a)
            {
                // Round 0: the packer dealt all eighteen bands out (dcsLaneFirstBand), a lane walks [bandBase, bandBase + nb).
                // Further sources of a frame (the deal made above, bands 0..15 in order): with 16 lanes per frame bands 16
                // and 17 go to the lanes of bands 0 and 1, the two shortest (their split records travel in the frame record's
                // bandType bytes, dcs_scan.h); with fewer lanes per frame the lane that holds band 15 takes them as well.
                constexpr bool kSpreadTail = SUB == 16 && !R0;
                const int end = Q.bandBase + Q.nb;
                const int end2 = (!R0 && SUB != 16 && end >= 16 && nBands > 16) ? nBands : end;
                const int prv0 = Q.bandBase == 0 ? 0x1A : sx16(Q.prv), out0 = Q.bandBase == 0 ? 0 : Q.outIdx;
                const int hb0 = static_cast<int>(Q.h0 & 0xFFu);
                if (pairTableInLds(FPW))
                    err |= unpack93a<R0, BR93>(T, row, br, hb0, mixMul, reinterpret_cast<const uint16_t *>(smem + ldsBytes(FPW) - 4096),
                                         Q.bandBase, end2, prv0, out0);
                else
                    err |= unpack93a<R0, BR93>(T, row, br, hb0, mixMul, a.tables->pair93a, Q.bandBase, end2, prv0, out0);
                if (kSpreadTail && pairTableInLds(FPW) && q < 2 && 16 + q < nBands)
                {
                    const uint32_t r0 = q == 0 ? Q.t0 : Q.t2, r1 = q == 0 ? Q.t1 : Q.t3;       // DcsSplit of band 16 + q
                    if (!((r1 >> 16) & 0x800u))                                                   // (the frame had not ended)
                    {
                        const uint32_t inPool2 = static_cast<uint32_t>(bitPos & 31) + (r0 & 0xFFFFu);
                        BR93 br2;
                        br2.init(pool + off + (inPool2 >> 5), static_cast<int>(inPool2 & 31));
                        err |= unpack93a<R0, BR93>(T, row, br2, hb0, mixMul, reinterpret_cast<const uint16_t *>(smem + ldsBytes(FPW) - 4096),
                                             16 + q, 17 + q, sx16(r0 >> 16), static_cast<int>((r1 >> 16) & 0x1FFu));
                    }
                }
            }
            }
            waveSync();
        };

        {
            if (__any(myNSrc > 0))
                unpackRound(std::true_type{}, 0);
            // (SOLE: no job of the batch has a second source, and the rounds of further sources are not instantiated)
            if constexpr (!SOLE)
                for (int r = 1 ; __any(r < myNSrc) ; ++r)
                    unpackRound(std::false_type{}, r);
        }

        DCS_STAMP(4);
        // a frame's error bits = OR over its sub-lanes
        if (__any(err != 0))            // (rare: skip the exchange when no lane of the wavefront has anything to report)
        {
#pragma unroll
            for (int m = FPW ; m < 64 ; m <<= 1)
                err |= __shfl_xor(err, m);
        }
        if (live && q == 0)
        {
            if constexpr (!SOLE)
                if (job.xform == DCS_XFORM_93)
                    dcMagnitude93(row);
            if (!(slot.flags & DCS_SLOT_HALO) && a.err != nullptr)
                a.err[slot.job] = err;
        }
    }
    waveSync();

    DCS_STAMP(5);
    // ---- phase 2: transform passes (8 frames x 8 lanes, or 4 frames x 16 lanes), overlap, emit ------------
    uint32_t *tails = reinterpret_cast<uint32_t *>(L.tails());         // [slot][8] dwords = 16 samples
#ifdef DCS_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    DCS_STAMP(7);
#endif
    const int nSlots = __popcll(__ballot(live && lane < FPW));          // padding slots are trailing
    const int slotJob = static_cast<int>(slot.job);
    const int slotWord = static_cast<int>(slot.flags | (slot.prevSlot << 8) | (static_cast<uint32_t>(job.volShift) << 16));
    const int jobXform = job.xform, jobPrev = static_cast<int>(job.prev);


    // (SOLE, an even-deal kernel: eight slots at most, all of them 1994+ transforms, are ONE pass of eight frames: the loop's body
    // as straight-line code, no run lengths and no look at the jobs' transforms.  A chunk without a live slot -- the planner makes
    // none -- would run it with no lane group active and store nothing.)
    constexpr bool kOnePass = SOLE;
    static_assert(!kOnePass || (EVEN && FPW == 8), "the even deal: 8 frames per wavefront, one transform pass of 8");
    const unsigned long long slots94 = kOnePass ? 0ull : __ballot(live && lane < FPW && jobXform == DCS_XFORM_94);
    const bool oneXform = kOnePass || slots94 == 0 || slots94 == __ballot(live && lane < FPW);
    for (int s0 = 0 ; kOnePass || s0 < nSlots ; )
    {
        // a pass takes the run of slots from s0 on that want the same transform (8 frames at most for 1994+, 4 for 1993)
        const int xf = kOnePass ? DCS_XFORM_94 : __builtin_amdgcn_readlane(jobXform, s0);
        const int G = (xf == DCS_XFORM_94) ? 8 : 4;
#ifndef DCS_RUN_BALLOT_MIN_FPW
#define DCS_RUN_BALLOT_MIN_FPW 8
#endif
        int n = 1;
        if constexpr (kOnePass)
            n = nSlots;
        else if constexpr (FPW >= DCS_RUN_BALLOT_MIN_FPW)
        {
            // the run length as a count of trailing zeros over a ballot
            const unsigned long long sameXf = (xf == DCS_XFORM_94) ? slots94 : ~slots94;
            n = min(min(static_cast<int>(__builtin_ctzll(~(sameXf >> s0))), G), nSlots - s0);
        }
        else if (oneXform)
            n = min(G, nSlots - s0);            // the usual case: every frame of the chunk wants the same transform
        else
        {
            // (with 4 slots the loop is as short and measured faster)
            while (n < G && s0 + n < nSlots && __builtin_amdgcn_readlane(jobXform, s0 + n) == xf)
                ++n;
        }

        if constexpr (!kOnePass)
            if (xf != constsXform)
            {
                constsXform = xf;                       // a chunk that mixes decoders of both families
                loadLaneConsts(a.tables, lane, constsXform, C);
            }
        const int lpfShift = (xf == DCS_XFORM_94) ? 3 : 4;
        const int g = lane >> lpfShift;
        const bool active = g < n;
        const int mySlot = s0 + (active ? g : 0);
        const int myWord = __shfl(slotWord, mySlot);
        const int myFlags = myWord & 0xFF, myPrevSlot = (myWord >> 8) & 0xFF, myShift = myWord >> 16;
        const uint32_t myJob = static_cast<uint32_t>(__shfl(slotJob, mySlot));
        const uint32_t myPrevJob = static_cast<uint32_t>(__shfl(jobPrev, mySlot));
        const int lr = (xf == DCS_XFORM_94) ? bitrevN(lane & 7, 3) : bitrevN(lane & 15, 4);   // the output sample (pair) this lane overlaps

        // a tail handed in by the caller (DCS_PREV_EXT, streaming use): requested before the transform, so that the
        // overlap below never waits for memory
        uint32_t extTail = 0;
        if (__any(active && (myFlags & DCS_SLOT_EXT_TAIL) != 0))
        {
            if (active && (myFlags & DCS_SLOT_EXT_TAIL) != 0 && a.tailsIn != nullptr)
            {
                const size_t k = static_cast<size_t>(myPrevJob & 0x7FFFFFFFu);
                extTail = (xf == DCS_XFORM_94) ? reinterpret_cast<const uint32_t *>(a.tailsIn)[k * 8 + lr]
                                               : static_cast<uint32_t>(static_cast<uint16_t>(a.tailsIn[k * 16 + lr]));
            }
        }

        // lane groups beyond the pass's frames run the same instruction stream on a dummy row (the bit
        // pool is dead in phase 2) and store nothing
        PassLane P;
        P.rowC = active ? reinterpret_cast<uint32_t *>(L.row(mySlot)) : L.pool();
#ifdef DCS_STAMPS_XFORM
        P.stamp = stamp;
#endif
        P.l = lane & ((1 << lpfShift) - 1);
        P.shiftPair = static_cast<uint32_t>(myShift) * 0x00010001u;
        P.paced = paced && kPace.steps && s0 + n >= nSlots;            // (the chunk's last pass)

        uint32_t x[16];
        BflyRegs R;
        R.k8000 = 0x8000u; R.k10000 = 0x10000u; R.watch = 0xFFFFu;
        R.k4000 = 0x4000u; R.watchB = 0x7FFF7FFFu;
        asm volatile("" : "+v"(R.k8000), "+v"(R.k10000), "+v"(R.k4000));    // keep them in vector registers (VOP3 takes no literal operand)
        if constexpr (kOnePass)     // (the batch's rows hold its first sources' bands and nothing else: the short pre-pass)
            transform94x8<kPace.levels, true>(P, W, C, R, x, 16u - ((a.flags >> DCS_BATCH_BANDS_SHIFT) & DCS_BATCH_BANDS_MASK));
        else if (xf == DCS_XFORM_94)
            transform94x8<kPace.levels>(P, W, C, R, x);
        else
            transform93x4<kPace.levels>(P, W, C, R, x);
        if (s0 == 0) DCS_STAMP(14);

        // tail for the successor = output samples 240..255 (:569-575, :805-812): register 15 of every lane.  Lane
        // groups without a frame write to a spare row of the tail array.
        {
            const int ts = active ? mySlot : FPW;
            if (xf == DCS_XFORM_94)
                tails[ts * 8 + lr] = x[15];
            else
                reinterpret_cast<uint16_t *>(tails)[ts * 16 + lr] = static_cast<uint16_t>(x[15]);
        }
        waveSync();

        if (s0 == 0) DCS_STAMP(15);
        const bool emit = active && !(myFlags & DCS_SLOT_HALO);
        const bool hasPrev = myPrevSlot != DCS_NO_PREV_SLOT;
        // Where the successor or the predecessor lies in another chunk, the frame goes to the rendezvous (see the top of this file):
        // its tail for a successor elsewhere (DCS_SLOT_EXPORT), its own first sample (pair), NOT overlapped, for a tail from
        // elsewhere (DCS_SLOT_IMPORT; such a frame leaves its first 16 samples to whoever arrives second).  The exchanges are issued
        // half way through the PCM stores -- the registers their results take have just come free, and the other half of the stores
        // covers their way to memory and back -- and looked at behind the last store.
        const bool exporter = active && (myFlags & DCS_SLOT_EXPORT) != 0;
        const bool deferred = active && (myFlags & DCS_SLOT_IMPORT) != 0;
#ifndef DCS_RDV_SPLIT_FPW4
#define DCS_RDV_SPLIT_FPW4 12
#endif
        // (stores issued in front of the exchanges: with 4 frames per wavefront -- sixteen lanes unpack a frame, the longest-lived
        // register set -- the exchanges' results only fit behind twelve of them)
        constexpr int kSplit = FPW == 4 ? DCS_RDV_SPLIT_FPW4 : 8;
        // (the lane's output position once more, opaque to the compiler: with 4 frames per wavefront every pass runs the same transform,
        // and the addresses behind the transform, hoisted out of the pass loop as 64-bit pairs, cost the transform its registers)
        int lrA = lr;
        if (FPW == 4)
            asm volatile("" : "+v"(lrA));
        unsigned long long metAsProducer = 0, metAsConsumer = 0;
        auto rendezvous = [&](uint32_t mine0, uint32_t tailOut)
        {
            if (exporter)
                metAsProducer = __hip_atomic_exchange(a.handoff + static_cast<size_t>(chunk) * 16 + lrA, handoffWord(a.epoch, 0u, tailOut),
                                                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (deferred)
                metAsConsumer = __hip_atomic_exchange(a.handoff + static_cast<size_t>(myPrevJob) * 16 + lrA, handoffWord(a.epoch, 1u, mine0),
                                                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        };
        // (The PCM of every kernel but the two of single-source even-deal batches leaves as 15 two- resp. four-byte stores per lane.
        // Putting a frame's samples in order in its dead tile row first and storing 16 bytes per lane as plain stores was measured
        // three times: 5 % slower twice before the even deal, and 0.43 us = 1.6 % slower on dcsDecodeKernel<8, 2, true, true> over
        // survey3_65536, profiles/NOTES.md 59 -- the extra LDS round trip is on the critical path and the narrow stores are not.
        // What pays is the same path with WRITE-THROUGH stores, below.  Swapping registers r and r + 8 with lane l ^ 8 by DPP and
        // storing sample PAIRS, 8 stores instead of 15 for a 1993 frame: no difference.)
        if (kOnePass || xf == DCS_XFORM_94)
        {
            // overlap-add on sample pair m = bitrev3(l) (register 0) (:538-555)
            uint32_t tailPair = tails[(hasPrev ? myPrevSlot : mySlot) * 8 + lr];
            tailPair = hasPrev ? tailPair : extTail;
            const uint32_t mixed = packC(overlapMix(reC(x[0]), C.k[DCS_K94_OVLA] & 0xFFFFu, reC(tailPair), C.k[DCS_K94_OVLB] & 0xFFFFu),
                                         overlapMix(imC(x[0]), C.k[DCS_K94_OVLA] >> 16, imC(tailPair), C.k[DCS_K94_OVLB] >> 16));
            x[0] = deferred ? x[0] : mixed;                             // (a deferred frame keeps the raw pair for the rendezvous)
            uint32_t *out = reinterpret_cast<uint32_t *>(a.pcm) + static_cast<size_t>(myJob) * (DCS_FRAME_SAMPLES / 2) + lrA;
            if constexpr (SOLE)
            {
                // The kernels of single-source even-deal batches write their PCM THROUGH the L2 (storePcm16, dcs_kernels.hip.h):
                // plain stores keep their lines in the XCD's L2 until the write-back at the end of the kernel, which whatever
                // follows the launch waits for -- 31.5 MB per launch of the headline workload, half of it from the launch's last
                // microseconds.  A write-through store costs per instruction, not per byte, so the samples go out 16 bytes at a
                // time: every lane puts its pairs in order into the frame's dead tile row (lane groups without a frame: into the
                // dead bit pool), lane 0 of the group the frame's job and flags behind them (dwords 130 and 131 of the row's 132),
                // and the chunk's 8 x 30 16-byte pieces leave in four rounds, piece g = lane + 64 t of frame g / 30.  Nothing is
                // stored for a padding slot or a frame without a slot (g / 30 >= nSlots), for a halo slot, and for pieces 0 and 1
                // -- samples 0..15 -- of a frame whose tail comes from another chunk: those belong to the rendezvous, which keeps
                // its 4-byte stores, as do the tails and the error words.  The exchanges are issued between the LDS writes and the
                // wide stores.  (The wide stores are inline assembly, outside the compiler's count of memory operations in
                // flight: memory operations complete in order, so a wait it places can only wait for more; and the rows are not
                // read again.)  27.12 -> 25.32 us on survey3_65536, profiles/NOTES.md 59.
                uint32_t *rowO = P.rowC + lrA;
                if (!deferred)
                    rowO[0] = x[0];
#pragma unroll
                for (int r = 1 ; r < 15 ; ++r)
                    rowO[8 * bitrevN(r, 4)] = x[r];                     // pair 8*bitrev4(r) + bitrev3(l)
                if (P.l == 0)
                    *reinterpret_cast<uint2 *>(P.rowC + 130) = make_uint2(myJob, static_cast<uint32_t>(myFlags));
                waveSync();
                rendezvous(x[0], x[15]);
                U32x4 piece[4];
                char *dst[4];
                bool put[4];
#pragma unroll
                for (int t = 0 ; t < 4 ; ++t)
                {
                    const int g = lane + 64 * t;
                    const int f = min((g * 2185) >> 16, FPW - 1), p = g - 30 * f;       // (g / 30 for g < 240; lanes beyond: no store)
                    const uint32_t *rowF = reinterpret_cast<const uint32_t *>(L.row(f));
                    const uint2 jf = *reinterpret_cast<const uint2 *>(rowF + 130);
                    const uint4 v = ldsRead4(rowF + 4 * (p & 31));
                    piece[t] = U32x4{ v.x, v.y, v.z, v.w };
                    put[t] = g < 240 && f < nSlots && !(jf.y & DCS_SLOT_HALO) && !((jf.y & DCS_SLOT_IMPORT) != 0 && p < 2);
                    dst[t] = reinterpret_cast<char *>(a.pcm) + static_cast<size_t>(jf.x) * (DCS_FRAME_SAMPLES * 2) + p * 16;
                }
#pragma unroll
                for (int t = 0 ; t < 4 ; ++t)
                    if (put[t])
                        storePcm16(dst[t], piece[t]);
                if (emit && a.tailsOut != nullptr && (myFlags & DCS_SLOT_KEEP_TAIL))
                    reinterpret_cast<uint32_t *>(a.tailsOut)[static_cast<size_t>(myJob) * 8 + lrA] = x[15];
            }
            else
            {
                if (emit)
                {
                    if (!deferred)
                        out[0] = x[0];
#pragma unroll
                    for (int r = 1 ; r < kSplit ; ++r)
                        out[8 * bitrevN(r, 4)] = x[r];                  // pair 8*bitrev4(r) + bitrev3(l)
                }
                rendezvous(x[0], x[15]);
                if (emit)
                {
#pragma unroll
                    for (int r = kSplit ; r < 15 ; ++r)
                        out[8 * bitrevN(r, 4)] = x[r];
                    if (a.tailsOut != nullptr && (myFlags & DCS_SLOT_KEEP_TAIL))
                        reinterpret_cast<uint32_t *>(a.tailsOut)[static_cast<size_t>(myJob) * 8 + lrA] = x[15];
                }
            }
            // the second to arrive finishes the consumer's first sample pair
            if (deferred && handoffMeets(metAsConsumer, a.epoch, 0u))
            {
                const uint32_t theirTail = static_cast<uint32_t>(metAsConsumer);
                out[0] = packC(overlapMix(reC(x[0]), C.k[DCS_K94_OVLA] & 0xFFFFu, reC(theirTail), C.k[DCS_K94_OVLB] & 0xFFFFu),
                               overlapMix(imC(x[0]), C.k[DCS_K94_OVLA] >> 16, imC(theirTail), C.k[DCS_K94_OVLB] >> 16));
            }
            if (exporter && handoffMeets(metAsProducer, a.epoch, 1u))
            {
                const uint32_t theirs = static_cast<uint32_t>(metAsProducer);
                reinterpret_cast<uint32_t *>(a.pcm)[static_cast<size_t>(exportNext) * (DCS_FRAME_SAMPLES / 2) + lrA] =
                    packC(overlapMix(reC(theirs), C.k[DCS_K94_OVLA] & 0xFFFFu, reC(x[15]), C.k[DCS_K94_OVLB] & 0xFFFFu),
                          overlapMix(imC(theirs), C.k[DCS_K94_OVLA] >> 16, imC(x[15]), C.k[DCS_K94_OVLB] >> 16));
            }
        }
        else if constexpr (!kOnePass)
        {
            // overlap-add on sample i = bitrev4(l) (register 0) (:789-802)
            int tailSample = static_cast<int16_t>(reinterpret_cast<const uint16_t *>(tails)[(hasPrev ? myPrevSlot : mySlot) * 16 + lr]);
            tailSample = hasPrev ? tailSample : sx16(extTail);
            const uint32_t mixed = static_cast<uint32_t>(overlapMix(reC(x[0]), C.k[DCS_K93_OVL] & 0xFFFFu, tailSample, C.k[DCS_K93_OVL] >> 16)) & 0xFFFFu;
            x[0] = deferred ? (x[0] & 0xFFFFu) : mixed;
            int16_t *out = a.pcm + static_cast<size_t>(myJob) * DCS_FRAME_SAMPLES + lrA;
            if (emit)
            {
                if (!deferred)
                    out[0] = static_cast<int16_t>(x[0]);
#pragma unroll
                for (int r = 1 ; r < kSplit ; ++r)
                    out[16 * bitrevN(r, 4)] = static_cast<int16_t>(x[r]);          // sample 16*bitrev4(r) + bitrev4(l)
            }
            rendezvous(x[0], x[15] & 0xFFFFu);
            if (emit)
            {
#pragma unroll
                for (int r = kSplit ; r < 15 ; ++r)
                    out[16 * bitrevN(r, 4)] = static_cast<int16_t>(x[r]);
                if (a.tailsOut != nullptr && (myFlags & DCS_SLOT_KEEP_TAIL))
                    a.tailsOut[static_cast<size_t>(myJob) * 16 + lrA] = static_cast<int16_t>(x[15]);
            }
            if (deferred && handoffMeets(metAsConsumer, a.epoch, 0u))
                out[0] = static_cast<int16_t>(overlapMix(reC(x[0]), C.k[DCS_K93_OVL] & 0xFFFFu, sx16(static_cast<uint32_t>(metAsConsumer)), C.k[DCS_K93_OVL] >> 16));
            if (exporter && handoffMeets(metAsProducer, a.epoch, 1u))
                a.pcm[static_cast<size_t>(exportNext) * DCS_FRAME_SAMPLES + lrA] =
                    static_cast<int16_t>(overlapMix(reC(static_cast<uint32_t>(metAsProducer)), C.k[DCS_K93_OVL] & 0xFFFFu, sx16(x[15]), C.k[DCS_K93_OVL] >> 16));
        }
        waveSync();
        s0 += n;
        if constexpr (kOnePass)
            break;
    }

    DCS_STAMP(6);
