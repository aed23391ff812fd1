/* Fixture generator (build container only): runs libsamplerate's sinc converter the way the reference encoder does
 * (DCSEncoder::OpenStream / WriteStream / CloseStream, DCSEncoder.cpp:165-185, :650-721), after EncodeFile's stereo
 * downmix (DCSEncodeFile.cpp:81-102), and writes what the encoder would receive.
 *   rs_driver <in.f32> <out.f32> <converter 0 best | 1 medium | 2 fastest> <rate> <channels 1|2>
 * in.f32 holds raw little-endian float32 values (interleaved when channels == 2); out.f32 the 31 250 Hz samples.  The
 * ratio is 31250.0 / rate at every rate, 31 250 included: the pass-through is the library's, not libsamplerate's. */
#include <stdio.h>
#include <stdlib.h>
#include "samplerate.h"

static float *out;
static long nOut, capOut;

static void put(const float *p, long n)
{
    if (nOut + n > capOut)
    {
        capOut = 2 * (nOut + n) + 1024;
        out = (float *)realloc(out, (size_t)capOut * sizeof(float));
    }
    for (long i = 0 ; i < n ; ++i)
        out[nOut++] = p[i];
}

/* WriteStream(const float *, n, eof): 16 input samples per src_process call, a 512-float output buffer */
static int write_stream(SRC_STATE *s, double ratio, const float *pcm, long numSamples, int eof)
{
    while (numSamples != 0 || eof)
    {
        float inbuf[16], outbuf[512];
        SRC_DATA d;
        long cur = numSamples < 16 ? numSamples : 16;
        for (long i = 0 ; i < cur ; ++i)
            inbuf[i] = *pcm++;
        numSamples -= cur;
        d.data_in = inbuf;
        d.input_frames = cur;
        d.src_ratio = ratio;
        d.end_of_input = (numSamples == 0 && eof);
        if (numSamples == 0)
            eof = 0;
        d.data_out = outbuf;
        d.output_frames = 512;
        d.output_frames_gen = 0;
        d.input_frames_used = 0;
        if (src_process(s, &d) != 0)
            return 1;
        put(outbuf, d.output_frames_gen);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 6) { fprintf(stderr, "usage: rs_driver <in.f32> <out.f32> <converter> <rate> <channels>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (f == NULL) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    long n = 0, cap = 4096;
    float *in = (float *)malloc((size_t)cap * sizeof(float));
    size_t got;
    while ((got = fread(in + n, sizeof(float), (size_t)(cap - n), f)) != 0)
    {
        n += (long)got;
        if (n == cap) { cap *= 2; in = (float *)realloc(in, (size_t)cap * sizeof(float)); }
    }
    fclose(f);
    const int conv = atoi(argv[3]), rate = atoi(argv[4]), channels = atoi(argv[5]);
    const double ratio = 31250.0 / rate;
    int err = 0;
    SRC_STATE *s = src_new(conv, 1, &err);
    if (s == NULL) { fprintf(stderr, "src_new: %d\n", err); return 3; }
    src_set_ratio(s, ratio);
    /* EncodeFile's loop: blocks of up to 256 mono samples, a stereo pair averaged, a final unpaired value alone */
    const float *p = in, *endp = in + n;
    while (p < endp)
    {
        float samples[256];
        int ns;
        for (ns = 0 ; ns < 256 && p < endp ; )
        {
            float sample = *p++;
            if (channels == 2 && p < endp)
                sample = (sample + *p++) / 2.0f;
            samples[ns++] = sample;
        }
        if (write_stream(s, ratio, samples, ns, 0)) return 4;
    }
    if (write_stream(s, ratio, NULL, 0, 1)) return 4;      /* CloseStream's end-of-input call */
    src_delete(s);
    FILE *o = fopen(argv[2], "wb");
    fwrite(out, sizeof(float), (size_t)nOut, o);
    fclose(o);
    return 0;
}
