// dcs_encode_files.hip.h -- the reference's EncodeFile on files held in memory (DCSEncodeFile.cpp:29-105): a "DCSa"
// container goes through transcoding (EncodeDCSFile), a RIFF/WAVE file (dcs_wav.hip.h) or a native FLAC file
// (dcs_flac.hip.h) is read as libnyquist reads it, downmixed, resampled and encoded.  Included last in dcs_encode.hip: it
// drives both readers (wavStageOnDevice launches W0 / W1 and calls flacStage), plans the files of a call on the host
// (planFiles), routes the walk by size (rsHostRoute) and hands the converted signal to the chain the streams use
// (rsEncodeConverted, dcs_resample.hip.h).  dcs_wav_decode and dcs_flac_decode stop after the readers.
#pragma once

namespace {

// The parsed WAV and FLAC files of one call on the device: payloads up, W0, W1; frames up, F1, F2, F3 (flac null: no FLAC
// file).  On DCS_OK *dMono holds file k's mono samples from files[k].monoOff; bad[k] is set where a value or a pair's mean is
// not finite, or (top bit) where a FLAC frame is refused on the device: stageWhy says which.  Buffers belong to `held`.
DcsStatus wavStageOnDevice(DcsCtx *ctx, const uint8_t *const *bytes, const DcsWavInfo *infos, const FlacSource *flac, uint32_t n,
                           std::vector<WavFile> &wf, CacheArena &held, float **dMonoOut, std::vector<uint32_t> &bad)
{
    const auto isFlac = [&](uint32_t k) { return flac != nullptr && flac[k].info != nullptr; };
    bool anyFlac = false;
    wf.assign(n, WavFile{});
    uint64_t blobBytes = 0, nStaged = 0, nMono = 0, maxMono = 0, maxLanes = 0;
    std::vector<uint32_t> byFormat[DCS_WAV_IMA + 1];
    for (uint32_t k = 0 ; k < n ; ++k)
    {
        const DcsWavInfo &w = infos[k];
        WavFile &f = wf[k];
        const bool ima = w.sampleFormat == DCS_WAV_IMA;
        const uint64_t payload = isFlac(k) ? 0 : ima ? w.nBlocks * static_cast<uint64_t>(w.blockAlign) : w.nValues * wavWidth(w.sampleFormat);
        f.blobOff = blobBytes;
        f.payOff = ima ? nStaged : blobBytes;
        blobBytes += (payload + 255) & ~uint64_t(255);
        nStaged += ima ? w.nValues : 0;
        f.nValues = w.nValues;
        f.nMono = rsMonoLength(w.nValues, w.channels);
        f.monoOff = nMono;
        f.nBlocks = static_cast<uint32_t>(w.nBlocks);
        f.blockAlign = w.blockAlign;
        f.channels = w.channels;
        f.sampleFormat = w.sampleFormat;
        nMono += f.nMono;
        maxMono = f.nMono > maxMono ? f.nMono : maxMono;
        if (ima)
            maxLanes = w.nBlocks * w.channels > maxLanes ? w.nBlocks * w.channels : maxLanes;
        if (isFlac(k))
            anyFlac = true;
        else
            byFormat[w.sampleFormat].push_back(k);
    }
    const hipStream_t st = dcsCtxStream(ctx);
    uint8_t *dBlob;
    int16_t *dStaged;
    float *dMono;
    WavFile *dFiles;
    uint32_t *dWhich, *dBad;
    ENCCHK(hipSetDevice(dcsCtxDevice(ctx)));
    ENCCHK(held.alloc(&dBlob, blobBytes ? blobBytes : 1));
    ENCCHK(held.alloc(&dStaged, nStaged ? nStaged : 1));
    ENCCHK(held.alloc(&dMono, nMono ? nMono : 1));
    ENCCHK(held.alloc(&dFiles, n));
    ENCCHK(held.alloc(&dWhich, n));
    ENCCHK(held.alloc(&dBad, n));
    for (uint32_t k = 0 ; k < n ; ++k)
    {
        const DcsWavInfo &w = infos[k];
        const uint64_t payload = w.sampleFormat == DCS_WAV_IMA ? w.nBlocks * static_cast<uint64_t>(w.blockAlign)
                                                               : w.nValues * wavWidth(w.sampleFormat);
        if (payload != 0 && !isFlac(k))
            ENCCHK(hipMemcpyAsync(dBlob + wf[k].blobOff, bytes[k] + w.dataOffset, payload, hipMemcpyHostToDevice, st));
    }
    std::vector<uint32_t> which;
    std::vector<size_t> whichOff(DCS_WAV_IMA + 2, 0);
    for (int fmt = 0 ; fmt <= DCS_WAV_IMA ; ++fmt)
    {
        whichOff[fmt] = which.size();
        which.insert(which.end(), byFormat[fmt].begin(), byFormat[fmt].end());
    }
    whichOff[DCS_WAV_IMA + 1] = which.size();
    ENCCHK(hipMemcpyAsync(dFiles, wf.data(), sizeof(WavFile) * n, hipMemcpyHostToDevice, st));
    if (!which.empty())
        ENCCHK(hipMemcpyAsync(dWhich, which.data(), sizeof(uint32_t) * which.size(), hipMemcpyHostToDevice, st));
    ENCCHK(hipMemsetAsync(dBad, 0, sizeof(uint32_t) * n, st));
    const uint32_t nIma = static_cast<uint32_t>(byFormat[DCS_WAV_IMA].size());
    if (nIma != 0)
    {
        // the values no block writes stay zero, as in the reference's zero-filled vector
        ENCCHK(hipMemsetAsync(dStaged, 0, sizeof(int16_t) * nStaged, st));
        if (maxLanes != 0)
        {
            const uint64_t lb = (maxLanes + 63) / 64;
            hipLaunchKernelGGL(wavImaKernel, dim3(static_cast<unsigned>(lb < 65535 ? lb : 65535), nIma < 65535 ? nIma : 65535), dim3(64),
                               0, st, dBlob, dFiles, dWhich + whichOff[DCS_WAV_IMA], nIma, dStaged);
        }
    }
    for (int fmt = 0 ; fmt <= DCS_WAV_IMA ; ++fmt)
    {
        const uint32_t m = static_cast<uint32_t>(byFormat[fmt].size());
        if (m == 0)
            continue;
        const dim3 grid = streamGrid(m, maxMono, 0, 1024);
        const uint32_t *w = dWhich + whichOff[fmt];
        switch (fmt)
        {
            case DCS_WAV_U8: hipLaunchKernelGGL(wavUnpackKernel<DCS_WAV_U8>, grid, dim3(256), 0, st, dBlob, dStaged, dFiles, w, m, dMono, dBad); break;
            case DCS_WAV_S16: hipLaunchKernelGGL(wavUnpackKernel<DCS_WAV_S16>, grid, dim3(256), 0, st, dBlob, dStaged, dFiles, w, m, dMono, dBad); break;
            case DCS_WAV_S24: hipLaunchKernelGGL(wavUnpackKernel<DCS_WAV_S24>, grid, dim3(256), 0, st, dBlob, dStaged, dFiles, w, m, dMono, dBad); break;
            case DCS_WAV_S32: hipLaunchKernelGGL(wavUnpackKernel<DCS_WAV_S32>, grid, dim3(256), 0, st, dBlob, dStaged, dFiles, w, m, dMono, dBad); break;
            case DCS_WAV_F32: hipLaunchKernelGGL(wavUnpackKernel<DCS_WAV_F32>, grid, dim3(256), 0, st, dBlob, dStaged, dFiles, w, m, dMono, dBad); break;
            case DCS_WAV_F64: hipLaunchKernelGGL(wavUnpackKernel<DCS_WAV_F64>, grid, dim3(256), 0, st, dBlob, dStaged, dFiles, w, m, dMono, dBad); break;
            default: hipLaunchKernelGGL(wavUnpackKernel<DCS_WAV_IMA>, grid, dim3(256), 0, st, dBlob, dStaged, dFiles, w, m, dMono, dBad); break;
        }
    }
    ENCCHK(hipGetLastError());
    std::vector<uint32_t> flacErr;
    if (anyFlac)
        ENCTRY(flacStage(ctx, held, st, bytes, flac, n, wf, dMono, flacErr));
    bad.assign(n, 0);
    ENCCHK(hipMemcpyAsync(bad.data(), dBad, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, st));
    ENCCHK(hipStreamSynchronize(st));
    for (uint32_t k = 0 ; anyFlac && k < n ; ++k)
        if (flacErr[k] != 0xFFFFFFFFu)
            bad[k] = 0x80000000u | flacErr[k];
    *dMonoOut = dMono;
    return DCS_OK;
}

bool isDcsaFile(const uint8_t *f, uint64_t len)          // DCSEncoder::IsDCSFile (DCSEncoder.cpp:381-386)
{
    return len >= 36 && memcmp(f, "DCSa", 4) == 0 && (f[4] == 0x93 || f[4] == 0x94) && f[6] == 0 && f[7] == 1 && f[8] == 0x7A
           && f[9] == 0x12;
}

bool isRiffFile(const uint8_t *f, uint64_t len)
{
    return len >= 4 && (memcmp(f, "RIFF", 4) == 0 || memcmp(f, "RIFX", 4) == 0 || memcmp(f, "FFIR", 4) == 0);
}

// "stream <k>" at the start of a message from a sub-call -> "file <map[k]>" (map null: "file <k>")
void renameError(DcsCtx *ctx, const std::vector<uint32_t> *map)
{
    const std::string msg = dcs_last_error(ctx);
    if (msg.compare(0, 7, "stream ") != 0)
        return;
    size_t end = 7;
    uint64_t k = 0;
    while (end < msg.size() && msg[end] >= '0' && msg[end] <= '9')
        k = k * 10 + static_cast<uint64_t>(msg[end++] - '0');
    if (end == 7 || (map != nullptr && k >= map->size()))
        return;
    dcsCtxSetError(ctx, ("file " + std::to_string(map != nullptr ? (*map)[k] : k) + msg.substr(end)).c_str());
}

// INTEGRATION rule 12: the largest |x| the encoder accepts from a file, the most negative value of its source format as
// libnyquist converts it: -32768 / 32767 for 16-bit PCM, ADPCM and FLAC, (0 - 128) / 127 for u8 and -128 / 127 for FLAC's
// signed 8 bits (rule 25); 1 for the others
float wavBound(int32_t fmt)
{
    if (fmt == DCS_WAV_S16 || fmt == DCS_WAV_IMA)
        return 32768.0f / 32767.0f;
    if (fmt == DCS_WAV_U8 || fmt == DCS_WAV_S8)
        return 128.0f / 127.0f;
    return 1.0f;
}

// What the plan knows of one file without a GPU
struct FilePlan
{
    int32_t kind = -1;
    DcsStatus status = DCS_OK;
    std::string why;
    DcsWavInfo wav{};               // (a FLAC file's is flacAsWav's)
    DcsFlacInfo flac{};
    std::vector<DcsFlacFrame> flacFrames;
    DcsStreamRef ref{};
    uint64_t bound = 0;
};

// the index of every FLAC file of a list, on the host pool (files are independent)
void flacParseMany(const uint8_t *files, const uint64_t *fileOffsets, const std::vector<uint32_t> &which, std::vector<FilePlan> &plan)
{
    std::atomic<size_t> next{ 0 };
    const auto worker = [&] {
        for (size_t j ; (j = next.fetch_add(1)) < which.size() ; )
        {
            FilePlan &p = plan[which[j]];
            p.status = flacParse(files + fileOffsets[which[j]], fileOffsets[which[j] + 1] - fileOffsets[which[j]], &p.flac, &p.flacFrames);
        }
    };
    int nThreads = dcs_host_threads();
    nThreads = nThreads < 1 ? 1 : nThreads > static_cast<int>(which.size()) ? static_cast<int>(which.size()) : nThreads;
    std::vector<std::thread> pool;
    for (int t = 1 ; t < nThreads ; ++t)
        pool.emplace_back(worker);
    worker();
    for (std::thread &t : pool)
        t.join();
}

// The length limit, checked before anything is allocated: fewer than 2^31 mono samples (what the resampler's walk indexes,
// as rsCheck requires of the other entry points) and, for encoding (s given), a 31 250 Hz length the encoder's 65 535 frames
// can take.  The walk's exact count is known only after it runs, so a file is refused here when even its room less twice the
// filter's reach and the end-of-input flush exceeds 65 535 frames; nearer the limit the exact count decides after the walk.
bool wavLengthOk(const DcsWavInfo &w, const RsStream *s, std::string &why)
{
    const uint64_t m = rsMonoLength(w.nValues, w.channels), cap = uint64_t(65535) * 240;
    if (m >= (uint64_t(1) << 31))
    {
        why = "2^31 mono samples or more";
        return false;
    }
    if (s == nullptr)
        return true;
    const uint64_t reach = static_cast<uint64_t>(2.0 * static_cast<double>(s->half) / s->step) + kRsFlushCap + 8;
    const uint64_t room = s->passThrough ? m : rsSlots(*s);
    if (room > cap + reach)
    {
        why = "resamples to more than 65 535 frames";
        return false;
    }
    return true;
}

DcsStatus planFiles(const uint8_t *files, const uint64_t *fileOffsets, uint32_t nFiles, const DcsEncodeParams *params,
                    const DcsResampleFilter &f, uint32_t flags, std::vector<FilePlan> &plan)
{
    plan.assign(nFiles, FilePlan{});
    const bool os93 = params->formatVersion != 0x9400;
    std::vector<uint32_t> flacIdx;
    for (uint32_t i = 0 ; i < nFiles ; ++i)
        if (!isDcsaFile(files + fileOffsets[i], fileOffsets[i + 1] - fileOffsets[i]) && !isRiffFile(files + fileOffsets[i], fileOffsets[i + 1] - fileOffsets[i])
            && isFlacFile(files + fileOffsets[i], fileOffsets[i + 1] - fileOffsets[i]))
            flacIdx.push_back(i);
    if (!flacIdx.empty())
        flacParseMany(files, fileOffsets, flacIdx, plan);
    for (uint32_t i = 0 ; i < nFiles ; ++i)
    {
        FilePlan &p = plan[i];
        const std::string name = "file " + std::to_string(i);
        const uint8_t *b = files + fileOffsets[i];
        const uint64_t len = fileOffsets[i + 1] - fileOffsets[i];
        if (isDcsaFile(b, len))
        {
            DcsOsVersion os;
            const uint8_t *s;
            uint32_t nBytes;
            if (dcs_dcsa_parse(b, len, &os, &s, &nBytes) != DCS_OK)
            {
                p.status = DCS_ERR_BAD_STREAM;
                p.why = name + ": a DCSa container whose data size runs past the end of the file";
                continue;
            }
            p.ref = DcsStreamRef{ s, nBytes, os, 0x67, 0xFF, 0xFF };        // EncodeDCSFile's decode settings
            int32_t action;
            std::string why;
            p.status = dcsTranscodePlan(&p.ref, 1, params, 0, &action, &p.bound, why);
            if (p.status != DCS_OK)
            {
                p.why = why.compare(0, 9, "stream 0:") == 0 ? name + why.substr(8) : name + ": " + why;
                continue;
            }
            p.kind = action == DCS_TRANSCODE_COPIED ? DCS_FILE_DCSA_COPY : DCS_FILE_DCSA_REENCODE;
            continue;
        }
        const bool flac = !isRiffFile(b, len) && isFlacFile(b, len);
        if (flac)
        {
            if (p.status != DCS_OK)                         // (flacParseMany's)
            {
                p.why = name + ": " + p.flac.reason;
                continue;
            }
            p.wav = flacAsWav(p.flac);
        }
        else if (!isRiffFile(b, len))
        {
            p.status = DCS_ERR_INVALID_ARG;
            p.why = name + ": not a DCSa container, a RIFF/WAVE file or a FLAC file";
            continue;
        }
        else
        {
            p.status = wavParse(b, len, &p.wav);
            if (p.status != DCS_OK)
            {
                p.why = name + ": " + p.wav.reason;
                continue;
            }
        }
        const DcsWavInfo &w = p.wav;
        if (w.rate < kRsMinRate || w.rate > kRsMaxRate)
        {
            p.status = DCS_ERR_INVALID_ARG;
            p.why = name + ": rate " + std::to_string(w.rate) + " Hz is outside 4 000 .. 384 000";
            continue;
        }
        const uint64_t m = rsMonoLength(w.nValues, w.channels);
        if (m == 0)
        {
            p.status = DCS_ERR_INVALID_ARG;
            p.why = name + ": no samples";
            continue;
        }
        const RsStream s = rsStreamOf(m, w.rate, f, flags);
        if (!wavLengthOk(w, &s, p.why))
        {
            p.status = DCS_ERR_INVALID_ARG;
            p.why = name + ": " + p.why;
            continue;
        }
        p.kind = flac ? DCS_FILE_FLAC : DCS_FILE_WAV;
        const uint64_t count = s.passThrough ? m : rsSlots(s);
        const uint64_t cap = uint64_t(65535) * 240;
        p.bound = (os93 ? dcs_encode93_bound : dcs_encode_bound)(count < cap ? count : cap);
    }
    for (uint32_t i = 0 ; i < nFiles ; ++i)
        if (plan[i].status != DCS_OK)
            return plan[i].status;
    return DCS_OK;
}

DcsStatus filesArgs(const uint8_t *files, const uint64_t *fileOffsets, uint32_t nFiles, const DcsEncodeParams *params,
                    const DcsResampleFilter *filter, uint32_t flags, DcsResampleFilter &f, std::string &why)
{
    if (fileOffsets == nullptr || (nFiles != 0 && files == nullptr))
        return DCS_ERR_INVALID_ARG;
    for (uint32_t i = 0 ; i < nFiles ; ++i)
        if (fileOffsets[i + 1] < fileOffsets[i])
            return DCS_ERR_INVALID_ARG;
    const bool os93 = params != nullptr && params->formatVersion != 0x9400;
    if (!paramsValid(params, os93))
    {
        if (const char *type1 = whyOs93aType1(params, os93))
            why = type1;
        return DCS_ERR_INVALID_ARG;
    }
    const uint64_t none[1] = { 0 };
    return rsCheck(0, none, nullptr, nullptr, filter, flags, f, why);
}

}  // namespace

extern "C" DcsStatus dcs_encode_files_plan(const uint8_t *files, const uint64_t *fileOffsets, uint32_t nFiles,
                                           const DcsEncodeParams *params, const DcsResampleFilter *filter, uint32_t flags,
                                           int32_t *kindOut, uint64_t *boundOut, int32_t *statusOut)
{
    return encGuard([&] {
        DcsResampleFilter f;
        std::string why;
        DcsStatus st = filesArgs(files, fileOffsets, nFiles, params, filter, flags, f, why);
        if (st != DCS_OK)
            return st;
        std::vector<FilePlan> plan;
        st = planFiles(files, fileOffsets, nFiles, params, f, flags, plan);
        for (uint32_t i = 0 ; i < nFiles ; ++i)
        {
            if (kindOut != nullptr) kindOut[i] = plan[i].kind;
            if (boundOut != nullptr) boundOut[i] = plan[i].bound;
            if (statusOut != nullptr) statusOut[i] = plan[i].status;
        }
        return st;
    });
}

namespace {
// dcs_wav_decode (flac false) and dcs_flac_decode (true): each takes its own kind of file only
DcsStatus wavDecode(DcsCtx *ctx, const uint8_t *files, const uint64_t *fileOffsets, uint32_t nFiles, float *out,
                                    size_t outCap, uint64_t *outOffsets, bool flac)
{
    if (ctx == nullptr || fileOffsets == nullptr || outOffsets == nullptr || (nFiles != 0 && files == nullptr))
        return DCS_ERR_INVALID_ARG;
    std::vector<DcsWavInfo> infos(nFiles);
    std::vector<const uint8_t *> bytes(nFiles);
    std::vector<DcsFlacInfo> flacInfos(flac ? nFiles : 0);
    std::vector<std::vector<DcsFlacFrame>> flacFrames(flac ? nFiles : 0);
    std::vector<FlacSource> sources(flac ? nFiles : 0);
    outOffsets[0] = 0;
    for (uint32_t i = 0 ; i < nFiles ; ++i)
    {
        if (fileOffsets[i + 1] < fileOffsets[i])
            return DCS_ERR_INVALID_ARG;
        bytes[i] = files + fileOffsets[i];
        DcsStatus st;
        std::string why;
        if (flac)
        {
            st = flacParse(bytes[i], fileOffsets[i + 1] - fileOffsets[i], &flacInfos[i], &flacFrames[i]);
            why = flacInfos[i].reason;
            infos[i] = flacAsWav(flacInfos[i]);
            sources[i] = FlacSource{ &flacInfos[i], &flacFrames[i] };
        }
        else
        {
            st = wavParse(bytes[i], fileOffsets[i + 1] - fileOffsets[i], &infos[i]);
            why = infos[i].reason;
        }
        if (st == DCS_OK && !wavLengthOk(infos[i], nullptr, why))
            st = DCS_ERR_INVALID_ARG;
        if (st != DCS_OK)
        {
            dcsCtxSetError(ctx, ("file " + std::to_string(i) + ": " + why).c_str());
            return st;
        }
    }
    for (uint32_t i = 0 ; i < nFiles ; ++i)
        outOffsets[i + 1] = outOffsets[i] + rsMonoLength(infos[i].nValues, infos[i].channels);
    if (nFiles == 0)
        return DCS_OK;
    CacheArena held(ctx);
    std::vector<WavFile> wf;
    std::vector<uint32_t> bad;
    float *dMono = nullptr;
    ENCTRY(wavStageOnDevice(ctx, bytes.data(), infos.data(), flac ? sources.data() : nullptr, nFiles, wf, held, &dMono, bad));
    for (uint32_t i = 0 ; flac && i < nFiles ; ++i)
        if (bad[i])
        {
            dcsCtxSetError(ctx, ("file " + std::to_string(i) + ": " + stageWhy(bad[i])).c_str());
            return DCS_ERR_BAD_STREAM;
        }
    if (out == nullptr || outCap < outOffsets[nFiles])
        return DCS_ERR_CAPACITY;
    if (outOffsets[nFiles] != 0)
        ENCCHK(hipMemcpyAsync(out, dMono, sizeof(float) * outOffsets[nFiles], hipMemcpyDeviceToHost, held.stream()));
    ENCCHK(hipStreamSynchronize(held.stream()));
    return DCS_OK;
}

DcsStatus encodeFiles(DcsCtx *ctx, const uint8_t *files, const uint64_t *fileOffsets, uint32_t nFiles,
                                      const DcsEncodeParams *params, const DcsResampleFilter *filter, uint32_t flags, uint8_t *out,
                                      size_t outCap, uint64_t *outOffsets, DcsEncodeFileInfo *info,
                                      const DcsLevel *levels, uint32_t nLevels, DcsLevelInfo *levelInfo)
{
    if (ctx == nullptr || outOffsets == nullptr)
        return DCS_ERR_INVALID_ARG;
    DcsResampleFilter f;
    std::string why;
    DcsStatus status = filesArgs(files, fileOffsets, nFiles, params, filter, flags, f, why);
    if (status != DCS_OK)
    {
        if (!why.empty())
            dcsCtxSetError(ctx, why.c_str());
        return status;
    }
    LevelStage lv{ ctx, levels, nLevels };
    ENCTRY(lv.check(nFiles, "file"));
    std::vector<FilePlan> plan;
    status = planFiles(files, fileOffsets, nFiles, params, f, flags, plan);
    if (status != DCS_OK)
    {
        for (const FilePlan &p : plan)
            if (p.status != DCS_OK)
            {
                dcsCtxSetError(ctx, p.why.c_str());
                break;
            }
        return status;
    }
    outOffsets[0] = 0;
    if (nFiles == 0)
        return DCS_OK;
    // (a DCSa container keeps this record: the stage is for the signal the converter hands the encoder)
    std::vector<DcsLevelInfo> fileLevel(lv.on() ? nFiles : 0, DcsLevelInfo{ 0.0f, 1.0f, 0.0f, 0, 0 });
    std::vector<uint32_t> wavIdx, dcsaIdx;
    for (uint32_t i = 0 ; i < nFiles ; ++i)
        (plan[i].kind == DCS_FILE_WAV || plan[i].kind == DCS_FILE_FLAC ? wavIdx : dcsaIdx).push_back(i);
    const bool os93 = params->formatVersion != 0x9400;
    std::vector<uint64_t> size(nFiles, 0);
    std::vector<DcsEncodeFileInfo> fi(nFiles);
    // the WAV and FLAC group: upload, W0 / W1 and F1 / F2 / F3, walk, convolve, encode where it lies; the stream bytes come down into wavOut
    const uint32_t nW = static_cast<uint32_t>(wavIdx.size());
    std::vector<uint8_t> wavOut;
    std::vector<uint64_t> wavOffsets(static_cast<size_t>(nW) + 1, 0);
    if (nW != 0)
    {
        CacheArena held(ctx);               // (given back at the end of this block, before the DCSa group borrows its own)
        std::vector<DcsWavInfo> infos(nW);
        std::vector<const uint8_t *> bytes(nW);
        std::vector<FlacSource> sources(nW, FlacSource{ nullptr, nullptr });
        for (uint32_t k = 0 ; k < nW ; ++k)
        {
            const FilePlan &p = plan[wavIdx[k]];
            infos[k] = p.wav;
            bytes[k] = files + fileOffsets[wavIdx[k]];
            if (p.kind == DCS_FILE_FLAC)
                sources[k] = FlacSource{ &p.flac, &p.flacFrames };
        }
        std::vector<WavFile> wf;
        std::vector<uint32_t> bad;
        float *dMono = nullptr;
        ENCTRY(wavStageOnDevice(ctx, bytes.data(), infos.data(), sources.data(), nW, wf, held, &dMono, bad));
        for (uint32_t k = 0 ; k < nW ; ++k)
            if (bad[k])
            {
                dcsCtxSetError(ctx, ("file " + std::to_string(wavIdx[k]) + ": " + stageWhy(bad[k])).c_str());
                return DCS_ERR_BAD_STREAM;
            }
        std::vector<RsStream> hs(nW);
        for (uint32_t k = 0 ; k < nW ; ++k)
        {
            hs[k] = rsStreamOf(wf[k].nMono, infos[k].rate, f, flags);
            hs[k].inOff = wf[k].monoOff;
        }
        rsHostRoute(hs);
        RsConverted c;
        ENCTRY(rsWalkConvolve(ctx, hs, dMono, nullptr, f, wavIdx.data(), "file", held, c));
        const std::vector<uint64_t> &resOffsets = c.offsets;
        uint64_t cap = 0;
        std::vector<float> bound(nW);
        for (uint32_t k = 0 ; k < nW ; ++k)
        {
            bound[k] = wavBound(infos[k].sampleFormat);
            cap += (os93 ? dcs_encode93_bound : dcs_encode_bound)(resOffsets[k + 1] - resOffsets[k]);
        }
        wavOut.resize(cap ? cap : 1);
        std::vector<DcsEncodeInfo> enc(nW);
        // (the records reach fileLevel, and from there the caller, only once the group is encoded)
        lv.which = wavIdx.data();
        status = rsEncodeConverted(ctx, held, c, lv, wavIdx.data(), "file", bound.data(),
                                   "%s: the signal the encoder reads peaks at |x| = %.9g, beyond %.9g (attenuate the input)", false,
                                   fileLevel.data(), params, os93, EncOutput{ wavOut.data(), cap, wavOffsets.data(), enc.data(), nullptr });
        if (status != DCS_OK)
        {
            renameError(ctx, nullptr);           // (the encoder's messages give the file's own index: in.label)
            return status;
        }
        for (uint32_t k = 0 ; k < nW ; ++k)
        {
            DcsEncodeFileInfo &t = fi[wavIdx[k]];
            t.kind = plan[wavIdx[k]].kind;
            t.sourceFormat = infos[k].formatCode;
            t.rate = infos[k].rate;
            t.channels = infos[k].channels;
            t.nValues = infos[k].nValues;
            t.nSamples = resOffsets[k + 1] - resOffsets[k];
            t.walk = hs[k].passThrough ? DCS_FILE_WALK_NONE : hs[k].hostWalk ? DCS_FILE_WALK_HOST : DCS_FILE_WALK_DEVICE;
            t.enc = enc[k];
            size[wavIdx[k]] = wavOffsets[k + 1] - wavOffsets[k];
        }
    }
    // the DCSa group: EncodeDCSFile's copy or re-encode (dcs_transcode_streams)
    const uint32_t nD = static_cast<uint32_t>(dcsaIdx.size());
    std::vector<uint8_t> dOut;
    std::vector<uint64_t> dOffsets(static_cast<size_t>(nD) + 1, 0);
    if (nD != 0)
    {
        std::vector<DcsStreamRef> refs(nD);
        uint64_t cap = 0;
        for (uint32_t k = 0 ; k < nD ; ++k)
        {
            refs[k] = plan[dcsaIdx[k]].ref;
            cap += plan[dcsaIdx[k]].bound;
        }
        dOut.resize(cap ? cap : 1);
        std::vector<DcsTranscodeInfo> ti(nD);
        status = dcs_transcode_streams(ctx, refs.data(), nD, params, 0, dOut.data(), cap, dOffsets.data(), ti.data());
        if (status != DCS_OK)
        {
            renameError(ctx, &dcsaIdx);
            return status;
        }
        for (uint32_t k = 0 ; k < nD ; ++k)
        {
            DcsEncodeFileInfo &t = fi[dcsaIdx[k]];
            t.kind = ti[k].action == DCS_TRANSCODE_COPIED ? DCS_FILE_DCSA_COPY : DCS_FILE_DCSA_REENCODE;
            t.sourceFormat = refs[k].os;
            t.rate = 31250;
            t.channels = 1;
            t.nValues = refs[k].len;
            t.nSamples = static_cast<uint64_t>(ti[k].srcFrames) * DCS_FRAME_SAMPLES;
            t.walk = DCS_FILE_WALK_NONE;
            t.srcFrames = ti[k].srcFrames;
            t.enc = ti[k].enc;
            size[dcsaIdx[k]] = dOffsets[k + 1] - dOffsets[k];
        }
    }
    for (uint32_t i = 0 ; i < nFiles ; ++i)
        outOffsets[i + 1] = outOffsets[i] + size[i];
    if (info != nullptr)
        memcpy(info, fi.data(), sizeof(DcsEncodeFileInfo) * nFiles);
    if (lv.on() && levelInfo != nullptr)
        memcpy(levelInfo, fileLevel.data(), sizeof(DcsLevelInfo) * nFiles);
    if (out == nullptr || outCap < outOffsets[nFiles])
        return DCS_ERR_CAPACITY;
    for (uint32_t k = 0 ; k < nW ; ++k)
        memcpy(out + outOffsets[wavIdx[k]], wavOut.data() + wavOffsets[k], wavOffsets[k + 1] - wavOffsets[k]);
    for (uint32_t k = 0 ; k < nD ; ++k)
        memcpy(out + outOffsets[dcsaIdx[k]], dOut.data() + dOffsets[k], dOffsets[k + 1] - dOffsets[k]);
    return DCS_OK;
}

}  // namespace

extern "C" DcsStatus dcs_wav_decode(DcsCtx *ctx, const uint8_t *files, const uint64_t *fileOffsets, uint32_t nFiles, float *out,
                                    size_t outCap, uint64_t *outOffsets)
{
    return encGuard([&] { return wavDecode(ctx, files, fileOffsets, nFiles, out, outCap, outOffsets, false); });
}

extern "C" DcsStatus dcs_flac_decode(DcsCtx *ctx, const uint8_t *files, const uint64_t *fileOffsets, uint32_t nFiles, float *out,
                                     size_t outCap, uint64_t *outOffsets)
{
    return encGuard([&] { return wavDecode(ctx, files, fileOffsets, nFiles, out, outCap, outOffsets, true); });
}

extern "C" DcsStatus dcs_encode_files(DcsCtx *ctx, const uint8_t *files, const uint64_t *fileOffsets, uint32_t nFiles,
                                      const DcsEncodeParams *params, const DcsResampleFilter *filter, uint32_t flags, uint8_t *out,
                                      size_t outCap, uint64_t *outOffsets, DcsEncodeFileInfo *info)
{
    return dcs_encode_files_level(ctx, files, fileOffsets, nFiles, params, filter, flags, out, outCap, outOffsets, info, nullptr, 0, nullptr);
}

extern "C" DcsStatus dcs_encode_files_level(DcsCtx *ctx, const uint8_t *files, const uint64_t *fileOffsets, uint32_t nFiles,
                                            const DcsEncodeParams *params, const DcsResampleFilter *filter, uint32_t flags, uint8_t *out,
                                            size_t outCap, uint64_t *outOffsets, DcsEncodeFileInfo *info,
                                            const DcsLevel *levels, uint32_t nLevels, DcsLevelInfo *levelInfo)
{
    return encGuard([&] {
        return encodeFiles(ctx, files, fileOffsets, nFiles, params, filter, flags, out, outCap, outOffsets, info, levels, nLevels, levelInfo);
    });
}
