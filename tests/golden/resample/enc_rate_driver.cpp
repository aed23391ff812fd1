// Fixture generator (build container only): the reference's EncodeFile for float input at any rate (DCSEncodeFile.cpp:
// 75-105, restated here because EncodeFile reads its input through libnyquist): EncodeFile's loop of up to 256 mono samples
// (a stereo pair averaged, a final unpaired value alone) into DCSEncoder::WriteStream(const float *, n), after
// OpenStream(rate), then CloseStream.  Linked with the vendored libsamplerate.
//   enc_rate_driver <in.f32> <out.bin> <rate> <channels> <formatVersion hex> <type> <subtype>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "DCSEncoder.h"

int main(int argc, char **argv)
{
    if (argc != 8) { fprintf(stderr, "usage: enc_rate_driver <in.f32> <out.bin> <rate> <channels> <fv> <type> <sub>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (f == nullptr) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<float> pcm;
    float buf[4096];
    size_t got;
    while ((got = fread(buf, sizeof(float), 4096, f)) != 0)
        pcm.insert(pcm.end(), buf, buf + got);
    fclose(f);
    const int rate = atoi(argv[3]), channels = atoi(argv[4]);
    DCSEncoder enc;
    enc.compressionParams.formatVersion = static_cast<uint16_t>(strtoul(argv[5], nullptr, 16));
    enc.compressionParams.streamFormatType = atoi(argv[6]);
    enc.compressionParams.streamFormatSubType = atoi(argv[7]);
    std::string err;
    DCSEncoder::Stream *s = enc.OpenStream(rate, err);
    if (s == nullptr) { fprintf(stderr, "OpenStream: %s\n", err.c_str()); return 3; }
    const float *p = pcm.data(), *endp = p + pcm.size();
    while (p < endp)
    {
        float samples[256];
        int nSamples;
        for (nSamples = 0 ; nSamples < 256 && p < endp ; )
        {
            float sample = *p++;
            if (channels == 2 && p < endp)
                sample = (sample + *p++) / 2.0f;
            samples[nSamples++] = sample;
        }
        enc.WriteStream(s, samples, nSamples);
    }
    DCSEncoder::DCSAudio obj;
    if (!enc.CloseStream(s, obj, err)) { fprintf(stderr, "CloseStream: %s\n", err.c_str()); return 4; }
    FILE *o = fopen(argv[2], "wb");
    fwrite(obj.data.get(), 1, obj.nBytes, o);
    fclose(o);
    return 0;
}
