/* fw_driver.c -- runs libFLAC's stream decoder, MD5 checking on, over the FLAC streams of a pack file and compares what it
 * decodes with the source samples (tests/golden/make_flac_write_golden.py builds and runs it; build container only).
 * Pack file: u32 count, then per stream u64 flacBytes, u64 nSamples, the FLAC stream, the samples as little-endian int16.
 * Output: one line per stream, "<index> ok" or "<index> <what failed>"; exit status 1 if any stream failed. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "FLAC/stream_decoder.h"

typedef struct
{
    const uint8_t *flac;
    uint64_t len, pos;
    const int16_t *pcm;
    uint64_t nSamples, got;
    int mismatch, errors, shape;
} Client;

static FLAC__StreamDecoderReadStatus readCb(const FLAC__StreamDecoder *d, FLAC__byte buffer[], size_t *bytes, void *p)
{
    Client *c = (Client *)p;
    size_t n = *bytes;
    if (c->pos >= c->len) { *bytes = 0; return FLAC__STREAM_DECODER_READ_STATUS_END_OF_STREAM; }
    if (n > c->len - c->pos) n = (size_t)(c->len - c->pos);
    memcpy(buffer, c->flac + c->pos, n);
    c->pos += n;
    *bytes = n;
    return FLAC__STREAM_DECODER_READ_STATUS_CONTINUE;
}

static FLAC__StreamDecoderWriteStatus writeCb(const FLAC__StreamDecoder *d, const FLAC__Frame *f, const FLAC__int32 *const buffer[], void *p)
{
    Client *c = (Client *)p;
    unsigned i;
    if (f->header.channels != 1 || f->header.bits_per_sample != 16) c->shape = 1;
    for (i = 0 ; i < f->header.blocksize ; ++i, ++c->got)
        if (c->got >= c->nSamples || buffer[0][i] != c->pcm[c->got]) c->mismatch = 1;
    return FLAC__STREAM_DECODER_WRITE_STATUS_CONTINUE;
}

static void metaCb(const FLAC__StreamDecoder *d, const FLAC__StreamMetadata *m, void *p)
{
    Client *c = (Client *)p;
    if (m->type == FLAC__METADATA_TYPE_STREAMINFO
        && (m->data.stream_info.total_samples != c->nSamples || m->data.stream_info.channels != 1 || m->data.stream_info.bits_per_sample != 16))
        c->shape = 1;
}

static void errorCb(const FLAC__StreamDecoder *d, FLAC__StreamDecoderErrorStatus s, void *p) { ((Client *)p)->errors++; }

int main(int argc, char **argv)
{
    FILE *f = argc > 1 ? fopen(argv[1], "rb") : NULL;
    uint32_t count = 0, i;
    int failed = 0;
    if (f == NULL || fread(&count, 4, 1, f) != 1) return 2;
    for (i = 0 ; i < count ; ++i)
    {
        uint64_t head[2];
        Client c;
        uint8_t *flac;
        int16_t *pcm;
        FLAC__StreamDecoder *d;
        const char *why = NULL;
        if (fread(head, 8, 2, f) != 2) return 2;
        flac = (uint8_t *)malloc(head[0] + 1);
        pcm = (int16_t *)malloc(2 * head[1] + 2);
        if (fread(flac, 1, head[0], f) != head[0] || fread(pcm, 2, head[1], f) != head[1]) return 2;
        memset(&c, 0, sizeof(c));
        c.flac = flac; c.len = head[0]; c.pcm = pcm; c.nSamples = head[1];
        d = FLAC__stream_decoder_new();
        FLAC__stream_decoder_set_md5_checking(d, 1);
        if (FLAC__stream_decoder_init_stream(d, readCb, NULL, NULL, NULL, NULL, writeCb, metaCb, errorCb, &c) != FLAC__STREAM_DECODER_INIT_STATUS_OK)
            why = "init";
        else if (!FLAC__stream_decoder_process_until_end_of_stream(d))
            why = "process";
        else if (FLAC__stream_decoder_get_state(d) != FLAC__STREAM_DECODER_END_OF_STREAM)
            why = "state";
        if (!FLAC__stream_decoder_finish(d) && why == NULL)
            why = "md5";
        if (why == NULL && c.errors) why = "decoder error";
        if (why == NULL && c.shape) why = "shape";
        if (why == NULL && (c.mismatch || c.got != c.nSamples)) why = "samples";
        if (why == NULL && c.pos != c.len) why = "bytes left over";
        printf("%u %s\n", i, why ? why : "ok");
        failed |= why != NULL;
        FLAC__stream_decoder_delete(d);
        free(flac);
        free(pcm);
    }
    fclose(f);
    return failed;
}
