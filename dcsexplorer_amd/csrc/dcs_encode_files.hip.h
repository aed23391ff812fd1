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
    uint64_t maxSamples = 0;        // a WAV or FLAC file: the most samples it can convert to (what `bound` was taken of)
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
        p.maxSamples = count < cap ? count : cap;
        p.bound = (os93 ? dcs_encode93_bound : dcs_encode_bound)(p.maxSamples);
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

// The WAV and FLAC files of a list (wavIdx, in input order) up to the converter's output, for encodeFiles and
// encodeFilesBudget: upload, W0 / W1 and F1 / F2 / F3, walk, convolve; the floats lie in `held`, c.room more behind them.
struct FilesConverted
{
    std::vector<DcsWavInfo> infos;
    std::vector<RsStream> hs;
    RsConverted c;
    std::vector<float> bound;               // the source format's full scale per file (INTEGRATION rule 12)
};
DcsStatus filesConvert(DcsCtx *ctx, const uint8_t *files, const uint64_t *fileOffsets, const std::vector<FilePlan> &plan,
                       const std::vector<uint32_t> &wavIdx, const DcsResampleFilter &f, uint32_t flags, CacheArena &held, FilesConverted &w)
{
    const uint32_t nW = static_cast<uint32_t>(wavIdx.size());
    w.infos.resize(nW);
    std::vector<const uint8_t *> bytes(nW);
    std::vector<FlacSource> sources(nW, FlacSource{ nullptr, nullptr });
    for (uint32_t k = 0 ; k < nW ; ++k)
    {
        const FilePlan &p = plan[wavIdx[k]];
        w.infos[k] = p.wav;
        bytes[k] = files + fileOffsets[wavIdx[k]];
        if (p.kind == DCS_FILE_FLAC)
            sources[k] = FlacSource{ &p.flac, &p.flacFrames };
    }
    std::vector<WavFile> wf;
    std::vector<uint32_t> bad;
    float *dMono = nullptr;
    ENCTRY(wavStageOnDevice(ctx, bytes.data(), w.infos.data(), sources.data(), nW, wf, held, &dMono, bad));
    for (uint32_t k = 0 ; k < nW ; ++k)
        if (bad[k])
        {
            dcsCtxSetError(ctx, ("file " + std::to_string(wavIdx[k]) + ": " + stageWhy(bad[k])).c_str());
            return DCS_ERR_BAD_STREAM;
        }
    w.hs.resize(nW);
    for (uint32_t k = 0 ; k < nW ; ++k)
    {
        w.hs[k] = rsStreamOf(wf[k].nMono, w.infos[k].rate, f, flags);
        w.hs[k].inOff = wf[k].monoOff;
    }
    rsHostRoute(w.hs);
    ENCTRY(rsWalkConvolve(ctx, w.hs, dMono, nullptr, f, wavIdx.data(), "file", held, w.c));
    w.bound.resize(nW);
    for (uint32_t k = 0 ; k < nW ; ++k)
        w.bound[k] = wavBound(w.infos[k].sampleFormat);
    return DCS_OK;
}

// file k of the converted group in the caller's record (enc: the encoder's own)
void filesWavInfo(const FilePlan &p, const FilesConverted &w, uint32_t k, const DcsEncodeInfo &enc, DcsEncodeFileInfo &t)
{
    t.kind = p.kind;
    t.sourceFormat = w.infos[k].formatCode;
    t.rate = w.infos[k].rate;
    t.channels = w.infos[k].channels;
    t.nValues = w.infos[k].nValues;
    t.nSamples = w.c.offsets[k + 1] - w.c.offsets[k];
    t.walk = w.hs[k].passThrough ? DCS_FILE_WALK_NONE : w.hs[k].hostWalk ? DCS_FILE_WALK_HOST : DCS_FILE_WALK_DEVICE;
    t.enc = enc;
}

// a DCSa container in the caller's record (ti: what transcoding says of its stream)
void filesDcsaInfo(const DcsStreamRef &ref, const DcsTranscodeInfo &ti, DcsEncodeFileInfo &t)
{
    t.kind = ti.action == DCS_TRANSCODE_COPIED ? DCS_FILE_DCSA_COPY : DCS_FILE_DCSA_REENCODE;
    t.sourceFormat = ref.os;
    t.rate = 31250;
    t.channels = 1;
    t.nValues = ref.len;
    t.nSamples = static_cast<uint64_t>(ti.srcFrames) * DCS_FRAME_SAMPLES;
    t.walk = DCS_FILE_WALK_NONE;
    t.srcFrames = ti.srcFrames;
    t.enc = ti.enc;
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
        FilesConverted w;
        ENCTRY(filesConvert(ctx, files, fileOffsets, plan, wavIdx, f, flags, held, w));
        const std::vector<uint64_t> &resOffsets = w.c.offsets;
        uint64_t cap = 0;
        for (uint32_t k = 0 ; k < nW ; ++k)
            cap += (os93 ? dcs_encode93_bound : dcs_encode_bound)(resOffsets[k + 1] - resOffsets[k]);
        wavOut.resize(cap ? cap : 1);
        std::vector<DcsEncodeInfo> enc(nW);
        // (the records reach fileLevel, and from there the caller, only once the group is encoded)
        lv.which = wavIdx.data();
        status = rsEncodeConverted(ctx, held, w.c, lv, wavIdx.data(), "file", w.bound.data(),
                                   "%s: the signal the encoder reads peaks at |x| = %.9g, beyond %.9g (attenuate the input)", false,
                                   fileLevel.data(), params, os93, EncOutput{ wavOut.data(), cap, wavOffsets.data(), enc.data(), nullptr });
        if (status != DCS_OK)
        {
            renameError(ctx, nullptr);           // (the encoder's messages give the file's own index: in.label)
            return status;
        }
        for (uint32_t k = 0 ; k < nW ; ++k)
        {
            filesWavInfo(plan[wavIdx[k]], w, k, enc[k], fi[wavIdx[k]]);
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
            filesDcsaInfo(refs[k], ti[k], fi[dcsaIdx[k]]);
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

// J1 (dcs_encode_join.hip.h, behind every other kernel of the unit): n decoded streams' int16 PCM, stream k from sample
// srcOffsets[k] of dPcm, as floats into `arena` from float dstOffsets[k]; their frames' error words ORed into dStreamErr[k]
DcsStatus encJoinPcm(DcsCtx *ctx, CacheArena &held, const int16_t *dPcm, const uint32_t *dErr, const uint64_t *srcOffsets, uint32_t n,
                     float *arena, const uint64_t *dstOffsets, uint32_t *dStreamErr);

// What dcs_encode_files_budget knows of its list before any device work, and dcs_encode_files_plan_budget's whole answer:
// the arguments checked, the files planned as encodeFiles plans them, and the units in file order: a WAV or FLAC file is
// searched (stream w of the converter's, in wavIdx), a container copied or searched by the budget's rule (searched: stream
// nW + its place in refs / conIdx).  A refusal's message is in `why`.
struct FilesBudgetPlan
{
    DcsResampleFilter f;
    uint32_t rsFlags = 0;
    std::vector<FilePlan> plan;
    std::vector<int32_t> action;            // a container's DCS_TRANSCODE_COPIED / _REENCODED
    std::vector<uint64_t> bound;            // per file: a copy's length, the searched encoder's bound of any other
    std::vector<uint32_t> wavIdx, conIdx;
    std::vector<DcsStreamRef> refs;
    BudgetUnits u;
};
DcsStatus planFilesBudget(const uint8_t *files, const uint64_t *fileOffsets, uint32_t nFiles, const DcsEncodeParams *params,
                          const DcsResampleFilter *filter, uint32_t flags, const DcsBudget *budget, FilesBudgetPlan &b, std::string &why)
{
    const bool os93 = budgetOs93(params);
    const auto say = [&](const char *text) { why = text; };
    if (!searchedParams("dcs_encode_files_budget", params, os93, say) || !budgetValid("dcs_encode_files_budget", budget, say))
        return DCS_ERR_INVALID_ARG;
    // (the plan reads the set as the reference-equal encoders do, which know no OS93 sub-type but 0 .. 3; the search reads none)
    DcsEncodeParams planned = *params;
    if (os93)
        planned.streamFormatSubType = 0;
    b.rsFlags = flags & ~DCS_FILES_REENCODE_ALL;
    ENCTRY(filesArgs(files, fileOffsets, nFiles, &planned, filter, b.rsFlags, b.f, why));
    const DcsStatus status = planFiles(files, fileOffsets, nFiles, &planned, b.f, b.rsFlags, b.plan);
    if (status != DCS_OK)
    {
        for (const FilePlan &p : b.plan)
            if (p.status != DCS_OK)
            {
                why = p.why;
                break;
            }
        return status;
    }
    const std::vector<FilePlan> &plan = b.plan;
    b.action.assign(nFiles, DCS_TRANSCODE_REENCODED);
    b.bound.assign(nFiles, 0);
    for (uint32_t i = 0 ; i < nFiles ; ++i)
        if (plan[i].kind == DCS_FILE_WAV || plan[i].kind == DCS_FILE_FLAC)
            b.wavIdx.push_back(i);
    const uint32_t nW = static_cast<uint32_t>(b.wavIdx.size());
    for (uint32_t i = 0, w = 0 ; i < nFiles ; ++i)
    {
        if (plan[i].kind == DCS_FILE_WAV || plan[i].kind == DCS_FILE_FLAC)
        {
            b.u.search(w++);
            b.bound[i] = (os93 ? dcs_encode93_rd_bound : dcs_encode_rd_bound)(plan[i].maxSamples);
            continue;
        }
        DcsBudget own = *budget;                // (the file's own bound, where the call has bounds)
        own.budgetBytes = budget->budgetBytes != nullptr ? budget->budgetBytes + i : nullptr;
        own.capBytes = budget->capBytes != nullptr ? budget->capBytes + i : nullptr;
        std::string text;
        const DcsStatus st = dcsTranscodePlanBudget(&plan[i].ref, 1, params, (flags & DCS_FILES_REENCODE_ALL) != 0 ? DCS_TRANSCODE_REENCODE_ALL : 0,
                                                    &own, &b.action[i], &b.bound[i], text);
        if (st != DCS_OK)
        {
            why = text.compare(0, 9, "stream 0:") == 0 ? "file " + std::to_string(i) + text.substr(8) : "file " + std::to_string(i) + ": " + text;
            return st;
        }
        if (b.action[i] == DCS_TRANSCODE_COPIED)
            b.u.keep(plan[i].ref.data, plan[i].ref.len);
        else
        {
            b.u.search(nW + static_cast<uint32_t>(b.refs.size()));
            b.refs.push_back(plan[i].ref);
            b.conIdx.push_back(i);
        }
    }
    return DCS_OK;
}

// dcs_encode_files_budget: encodeFiles' front half, then ONE searched EncRun over every file that is not
// a copy.  Its input is one float arena of the call's lifetime: the converter's output for the WAV and FLAC files (streams
// 0 .. nW - 1, as the converter lays them), and behind it the searched containers' decoded PCM (streams nW .., J1); the
// jobs name those streams in file order.  A list without searched containers launches no join; a list of searched
// containers only has an arena of their samples alone.
DcsStatus encodeFilesBudget(DcsCtx *ctx, const uint8_t *files, const uint64_t *fileOffsets, uint32_t nFiles,
                            const DcsEncodeParams *params, const DcsResampleFilter *filter, uint32_t flags, const DcsBudget *budget,
                            uint8_t *out, size_t outCap, uint64_t *outOffsets, DcsEncodeFileInfo *info, DcsEncodeRdInfo *infoRd,
                            const DcsLevel *levels, uint32_t nLevels, DcsLevelInfo *levelInfo)
{
    if (ctx == nullptr || outOffsets == nullptr || budget == nullptr)
        return DCS_ERR_INVALID_ARG;
    FilesBudgetPlan fb;
    std::string why;
    DcsStatus status = planFilesBudget(files, fileOffsets, nFiles, params, filter, flags, budget, fb, why);
    if (status != DCS_OK)
    {
        if (!why.empty())
            dcsCtxSetError(ctx, why.c_str());
        return status;
    }
    LevelStage lv{ ctx, levels, nLevels };
    ENCTRY(lv.check(nFiles, "file"));
    outOffsets[0] = 0;
    if (nFiles == 0)
        return DCS_OK;
    const bool os93 = budgetOs93(params);
    const DcsResampleFilter &f = fb.f;
    const uint32_t rsFlags = fb.rsFlags;
    const std::vector<FilePlan> &plan = fb.plan;
    const std::vector<uint32_t> &wavIdx = fb.wavIdx, &conIdx = fb.conIdx;
    const std::vector<DcsStreamRef> &refs = fb.refs;
    const std::vector<int32_t> &action = fb.action;
    const BudgetUnits &u = fb.u;
    const uint32_t nW = static_cast<uint32_t>(wavIdx.size());
    const uint32_t nC = static_cast<uint32_t>(refs.size());
    uint64_t conSamples = 0;
    for (const DcsStreamRef &r : refs)
        conSamples += (((static_cast<uint64_t>(r.data[0]) << 8) | r.data[1]) + 1) * DCS_FRAME_SAMPLES;
    // (a DCSa container keeps this record: the stage is for the signal the converter hands the encoder)
    std::vector<DcsLevelInfo> fileLevel(lv.on() ? nFiles : 0, DcsLevelInfo{ 0.0f, 1.0f, 0.0f, 0, 0 });
    CacheArena held(ctx);                   // the input arena: of the call, so that it outlives every group of the search
    FilesConverted w;
    w.c.room = conSamples;
    if (nW != 0)
        ENCTRY(filesConvert(ctx, files, fileOffsets, plan, wavIdx, f, rsFlags, held, w));
    else
    {
        w.c.offsets.assign(1, 0);
        if (conSamples != 0)
        {
            ENCCHK(hipSetDevice(dcsCtxDevice(ctx)));
            ENCCHK(held.alloc(&w.c.d, conSamples));
        }
    }
    // the streams of the one input: the converter's, then the containers'
    std::vector<uint32_t> label(wavIdx);
    label.insert(label.end(), conIdx.begin(), conIdx.end());
    std::vector<float> bound(w.bound);
    bound.resize(nW + nC, 1.0f);
    std::vector<DcsEncodeInfo> enc;
    const auto search = [&](EncInput &in) { return encodeBudgeted(ctx, in, u, params, os93, *budget, out, outCap, outOffsets, enc, infoRd); };
    const RsEncode joined = [&](EncInput &in) -> DcsStatus {
        in.label = label.data();
        in.bound = bound.data();
        if (nC == 0)
            return search(in);
        // (a message of the decode itself counts the searched containers; the encoder's gives the file's own index, in.label)
        bool encoding = false;
        const DcsStatus joinedStatus = dcsTranscodeDecoded(ctx, refs.data(), nC, [&](const int16_t *dPcm, const uint32_t *dErr, const volatile uint32_t *planFlag,
                                                             const uint64_t *srcOffsets, bool *unusable) -> DcsStatus {
            std::vector<uint64_t> offsets(w.c.offsets);
            for (uint32_t k = 0 ; k < nC ; ++k)
                offsets.push_back(offsets.back() + (srcOffsets[k + 1] - srcOffsets[k]));
            if (offsets.back() - w.c.offsets.back() != conSamples)
            {
                dcsCtxSetError(ctx, "internal error: the decode of the containers is not as long as their frame counts say");
                return DCS_ERR_HIP;
            }
            uint32_t *dStreamErr;
            ENCCHK(held.alloc(&dStreamErr, size_t(nW) + nC));
            ENCCHK(hipMemsetAsync(dStreamErr, 0, sizeof(uint32_t) * (size_t(nW) + nC), held.stream()));
            ENCTRY(encJoinPcm(ctx, held, dPcm, dErr, srcOffsets, nC, w.c.d, offsets.data() + nW, dStreamErr + nW));
            EncInput all = in;
            all.sampleOffsets = offsets.data();
            all.nStreams = nW + nC;
            all.devFloat = w.c.d;
            all.devStreamErr = dStreamErr;
            all.planFlag = planFlag;
            encoding = true;
            const DcsStatus st = search(all);
            *unusable = all.unusable;
            encoding = !all.unusable;
            return st;
        });
        if (joinedStatus != DCS_OK && joinedStatus != DCS_ERR_CAPACITY && !encoding)
            renameError(ctx, &conIdx);
        return joinedStatus;
    };
    lv.which = wavIdx.data();
    status = rsEncodeConverted(ctx, held, w.c, lv, wavIdx.data(), "file", w.bound.data(),
                               "%s: the signal the encoder reads peaks at |x| = %.9g, beyond %.9g (attenuate the input)", true,
                               fileLevel.data(), params, os93, EncOutput{}, &joined);    // (early into fileLevel, which is the call's own)
    if (status != DCS_OK && status != DCS_ERR_CAPACITY)
    {
        renameError(ctx, nullptr);           // (the encoder's messages give the file's own index: in.label)
        return status;
    }
    if (info != nullptr)
        for (uint32_t i = 0, k = 0 ; i < nFiles ; ++i)
        {
            DcsEncodeFileInfo t{};
            if (plan[i].kind == DCS_FILE_WAV || plan[i].kind == DCS_FILE_FLAC)
                filesWavInfo(plan[i], w, k++, enc[i], t);
            else
            {
                const DcsStreamRef &r = plan[i].ref;
                const int32_t srcFrames = static_cast<int32_t>((static_cast<uint32_t>(r.data[0]) << 8) | r.data[1]);
                filesDcsaInfo(r, DcsTranscodeInfo{ action[i], srcFrames, action[i] == DCS_TRANSCODE_COPIED ? dcsTranscodeCopyInfo(r) : enc[i] }, t);
            }
            info[i] = t;
        }
    if (lv.on() && levelInfo != nullptr)
        memcpy(levelInfo, fileLevel.data(), sizeof(DcsLevelInfo) * nFiles);
    return status;
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

extern "C" DcsStatus dcs_encode_files_budget(DcsCtx *ctx, const uint8_t *files, const uint64_t *fileOffsets, uint32_t nFiles,
                                             const DcsEncodeParams *params, const DcsResampleFilter *filter, uint32_t flags,
                                             const DcsBudget *budget, uint8_t *out, size_t outCap, uint64_t *outOffsets,
                                             DcsEncodeFileInfo *info, DcsEncodeRdInfo *infoRd,
                                             const DcsLevel *levels, uint32_t nLevels, DcsLevelInfo *levelInfo)
{
    return encGuard([&] {
        return encodeFilesBudget(ctx, files, fileOffsets, nFiles, params, filter, flags, budget, out, outCap, outOffsets, info, infoRd,
                                 levels, nLevels, levelInfo);
    });
}

extern "C" DcsStatus dcs_encode_files_plan_budget(const uint8_t *files, const uint64_t *fileOffsets, uint32_t nFiles,
                                                  const DcsEncodeParams *params, const DcsResampleFilter *filter, uint32_t flags,
                                                  const DcsBudget *budget, int32_t *kindOut, uint64_t *boundOut)
{
    return encGuard([&]() -> DcsStatus {
        if (budget == nullptr)
            return DCS_ERR_INVALID_ARG;
        FilesBudgetPlan fb;
        std::string why;
        ENCTRY(planFilesBudget(files, fileOffsets, nFiles, params, filter, flags, budget, fb, why));
        for (uint32_t i = 0 ; i < nFiles ; ++i)
        {
            const int32_t kind = fb.plan[i].kind;
            if (kindOut != nullptr)
                kindOut[i] = kind == DCS_FILE_WAV || kind == DCS_FILE_FLAC ? kind
                             : fb.action[i] == DCS_TRANSCODE_COPIED ? DCS_FILE_DCSA_COPY : DCS_FILE_DCSA_REENCODE;
            if (boundOut != nullptr)
                boundOut[i] = fb.bound[i];
        }
        return DCS_OK;
    });
}
