// Fixture generator (build container only): encodes caller-given PCM with the reference's own encoder
// (DCSEncoder::OpenStream(31250) / WriteStream(const float *, n) / CloseStream, DCSEncoder.h:238-249).
//   enc_pcm_driver <in.f32> <out.bin> <formatVersion hex> <type -1|0|1> <subtype -1|0|3>
//                  <powerBandCutoff> <targetBitRate> <minimumDynamicRange> <maximumQuantizationError>
// in.f32 is raw little-endian float32 samples at 31 250 Hz; the float parameters are C99 hex floats ("%a"), so the
// value the encoder sees is exactly the binary32 the test records.
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "DCSEncoder.h"

int main(int argc, char **argv)
{
    if (argc != 10) { fprintf(stderr, "usage: enc_pcm_driver <in.f32> <out.bin> <fv> <type> <sub> <cutoff> <rate> <minDR> <maxQE>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (f == nullptr) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<float> pcm;
    float buf[4096];
    size_t got;
    while ((got = fread(buf, sizeof(float), 4096, f)) != 0)
        pcm.insert(pcm.end(), buf, buf + got);
    fclose(f);

    DCSEncoder enc;
    enc.compressionParams.formatVersion = static_cast<uint16_t>(strtoul(argv[3], nullptr, 16));
    enc.compressionParams.streamFormatType = atoi(argv[4]);
    enc.compressionParams.streamFormatSubType = atoi(argv[5]);
    enc.compressionParams.powerBandCutoff = strtof(argv[6], nullptr);
    enc.compressionParams.targetBitRate = atoi(argv[7]);
    enc.compressionParams.minimumDynamicRange = strtof(argv[8], nullptr);
    enc.compressionParams.maximumQuantizationError = strtof(argv[9], nullptr);
    std::string err;
    DCSEncoder::Stream *s = enc.OpenStream(31250, err);
    if (s == nullptr) { fprintf(stderr, "OpenStream: %s\n", err.c_str()); return 3; }
    enc.WriteStream(s, pcm.data(), pcm.size());
    DCSEncoder::DCSAudio obj;
    if (!enc.CloseStream(s, obj, err)) { fprintf(stderr, "CloseStream: %s\n", err.c_str()); return 4; }
    FILE *o = fopen(argv[2], "wb");
    fwrite(obj.data.get(), 1, obj.nBytes, o);
    fclose(o);
    return 0;
}
