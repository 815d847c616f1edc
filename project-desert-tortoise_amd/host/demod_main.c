/*
 * demod_main.c -- demodPOES / demodARGOS (build with -DPDT_ARGOS) on an MI355X.
 *
 * Host side of the drop-in: plain C, same command line, console messages and output-file
 * surface as the reference programs, with the DSP chain executed by libpdt.so (HIP kernels)
 * through the C ABI of include/pdt.h.  There is no CPU DSP path in this program: without a
 * GPU, pdt_open fails and the program exits with an error.
 *
 * Behaviour mirrored from the reference (file:line):
 *   options -s <kHz> -r -n <gain> -c <chunk>           POESTIPdemod/main.c:185-234
 *           -r -n -c                                   ARGOSdemod/main.c:121-164
 *   -s with a WAV overrides the rate with the kHz number taken as Hz (Q6)   main.c:343-344
 *   -r POES: opens/creates an empty output.raw (all writes are commented out)   main.c:299-307
 *      ARGOS: output.raw receives the AGC output before Squelch (doubles)      ARGOSdemod/main.c:171-180,273-274
 *   44-byte canonical header, no chunk walk            common/wave.c:303-378
 *   every byte after the header is sample data (while(!feof))               main.c:373
 *   output name minorFrames_YYYYMMDD_HHMMSS.txt / packets_YYYYMMDD_HHMMSS.txt   main.c:289 / ARGOS main.c:213
 *   "Normalization Factor: %f", " : PLL locked at %0.2fHz"                  main.c:388, CarrierTrackingPLL.c:269
 *   output removed when no frame was found             main.c:508-512
 * A capture of any length is taken (main.c:373 reads until end of file): one that does not fit the GPU's free memory goes through
 * the library's bounded window (pdt.h, ABI 4).
 * Additions: -o <file> chooses the output name (tests), -d <n> picks the GPU, -D NAME=VALUE sets a developer switch of the library, -P drops the progress lines, -q (POES) prints the frame
 * validation the reference keeps in MATLAB (checkParity.m:91-92, daytimeDecode.m:36,82-95) after decoding,
 * -m selects MMClockRecovery (the sampler the reference keeps commented out at ARGOSdemod/main.c:277),
 * -l (POES) runs the sound-card twin's chain (POESTIPdemodPortAudio/main.c:41-65,324-393: its PLL constants,
 * Squelch between PLL and FIR, Manchester threshold 0.75, blocks of 2400); with the file name "-" it is the twin's
 * loop itself, reading float32 I,Q blocks from standard input (e.g. a sound-card recorder's pipe, -s 48) until
 * end of file and appending every minor frame to the output as soon as it is final.
 * The per-chunk "\r" progress line (main.c:461-481 with its quality figure, ARGOSdemod/main.c:290-296) is printed after the
 * run, chunk by chunk from the library's per-chunk reports (pdt_keep_quality), with the reference's arithmetic and under the
 * reference's condition (progress of more than 0.15 %, or end of file); one summary line follows.  RAW float32 input (".raw", -s mandatory) is supported for POES
 * exactly as in POESTIPdemod/main.c:313-339.
 * -f <kHz> (an addition): the input is a single-channel recording (SatNOGS audio, an SDR in USB mode, a one-input sound card)
 * whose signal sits around that audio frequency; the library turns it into I,Q through its Hilbert front end
 * (pdt_set_real_input / pdt_demod_file with PDT_FMT_REAL_*): a mono 16-bit WAV, for POES also a mono float32 .raw
 * (-s), and with -l and the file name "-" mono float32 blocks from standard input.  A 2-channel file is refused under -f;
 * without -f a mono file is refused as before.
 * -x <decim> with one or more -t <kHz> (an addition): the input is a wideband I,Q capture (RTL-SDR, HackRF, ...) at decim times the
 * channel rate, the beacon -t kHz (signed) off its centre; the library tunes, filters and decimates on the GPU
 * (pdt_set_channel / PDT_FMT_WB_*).  The WAV header's rate, or -s in kHz, is the WIDEBAND rate and must be divisible by
 * decim; files named .cu8 / .cs8 are headerless unsigned / signed 8-bit pairs (-s required).  With several -t the capture is
 * ingested once for all channels (pdt_demod_channels: one conversion launch per channel) and each writes its own file, the channel's index appended to the usual name
 * (".0", ".1", ...).  -l -x .. -t .. - reads blocks from standard input through pdt_stream_push_channel, in the format -F names
 * (cu8, the default, cs8, s16 or f32).  Without -x nothing changes, the refusal of rates above 300 kHz included.
 * -t auto or -t auto:N (an addition, with -x, not beside numeric -t): the carriers are looked for instead of given -- the capture's
 * averaged spectrum is surveyed on the GPU (pdt_survey), the (N) strongest carriers found are printed like the -t lines
 * and the run goes on as if their offsets had been given.  No carrier: one line, no output file, exit status 1.  Not from a pipe.
 * -t bursts or -t bursts:N (an addition, under -t auto's rules): the platforms are looked for in the spectrum over time -- the
 * capture's short transmissions are searched for on the GPU (pdt_bursts), one line is printed per burst, the (N)
 * strongest platforms among them are printed like the -t lines and the run goes on as if their offsets had been given.  No burst:
 * one line, no output file, exit status 1.  -B <seconds> is the longest transmission that counts as a burst (pdt_bursts_cfg.max_s),
 * 5 by default: what lasts longer -- a receiver's DC spike, a birdie, a continuous beacon -- is no platform; -B 0 sets no limit.
 * -t each (an addition, under -t bursts' rules, -B included): the same burst search and the same line per burst, but then every burst is
 * demodulated in a window of its own at its own offset (pdt_burst_windows at its defaults, pdt_demod_windows_held in rounds through a
 * pool of at most 64 contexts) -- what a platform whose Doppler moves over the pass, and a recording that opens with
 * noise, need.  ONE output file under the usual name: every window's records in window order, each time increased by the window's
 * start in the capture; one line per burst with its lock and its packets, then one summary line.  Bursts found but no packet in
 * any of them: the lines are printed, the file is removed as after any run without packets, exit status 0.  -t each:N (1 .. 64)
 * makes the pool N contexts: more rounds, less memory, the same file.
 * -M <file> (an addition, with -x and a capture file): the carrier as a measurement (pdt_tones), written to <file>.  With
 * -t each one line per window after each round, "%d %.5f %.2f %.1f %.1f": the window's index, the capture's seconds at the middle of
 * the window's first segment, the carrier's frequency from the capture's centre in Hz, its C/N0 in dB-Hz and its power in dB; only the
 * first segment of a window is measured, the 128 ms of unmodulated carrier a burst opens with.  With -t <kHz>, -t auto or -t bursts one
 * line per segment at stride N along the channel, without the index: the Doppler curve (several channels: a file each, the index
 * appended as to the output's name).  Not from a pipe, not with -l, and not for a capture that left no channel stream in one piece: a
 * message, exit status 1.  Without -M nothing changes.
 * -A <file> (an addition, demodARGOS): who sent what -- the ARGOS messages in the bits of whatever was demodulated (pdt_argos_messages,
 * either polarity, 1 .. 8 blocks, the platform ID), one line per complete message, "%.5f" of its time, "i" when its bits
 * arrived complemented, " %d %05X" of its blocks and ID, " %02X" per data byte.  One-shot runs, -x with -t <kHz>, -t auto and -t bursts
 * (several channels: a file each, the index appended); -t each: every window's messages through one pdt_argos_messages_batch per round,
 * beside the -M pass, their times counted from the capture's start as the packets' are.  The packets file is what it was.  Not for
 * demodPOES, not from a pipe (-l -), and not for a capture that left no bit stream in one piece (one taken through the bounded
 * window): a message, exit status 1.  Without -A nothing changes.
 * -R first|best (an addition, demodARGOS, with -A): the rule that picks the messages' heads.  first, or no -R: PDT_ARGOS_RULE_FIRST, what
 * -A did before there was a choice.  best: PDT_ARGOS_RULE_BEST -- one stray bit between run and sync is tolerated and, of heads whose
 * spans overlap, the one with the longest run wins; on every route -A has.
 * -b (an addition, demodARGOS, with -A): the messages are read out of feed-forward bits instead of the loop's.  With -t each
 * every window's carrier is measured, its bit timing searched and its messages decoded by one pdt_ff_messages_batch per round, times from
 * the capture's start as -A has them.  With a plain I,Q file -- one recording of one burst, no -x, no -f, no -l -- the first two seconds
 * of the file go through pdt_stage_ff_bits and the message kernels; a message's time is its sample index / Fs.  The packets file is what
 * it was: the chain runs as always.  On any other route and without -A: a message, exit status 1.
 * -b -W <file> (demodPOES): -W's file holds the flywheel's frames out of feed-forward POES bits instead of the loop's: with -x
 * and one -t the channel stream goes through pdt_ffp_frames, a plain 16-bit I,Q file's samples / 32768 through pdt_stage_ffp_frames; a
 * frame's time is its sample index / Fs.  -w and -q work as before; the minorFrames file is what it was.  -b without -W, with -l, -f, a
 * pipe or several -t: a message, exit status 1.
 * -b -W <file> -Q <report> (demodPOES): the -W frames' failed parity groups are repaired from the feed-forward bits' soft values before they
 * are written (pdt_tip_repair); <report> gets one line per record that had a failing group -- its time, then group, frame bit,
 * least and next for each failing group --, and a summary line precedes the -W count.  After the repair every group
 * passes by construction: -q's flywheel line on these frames says nothing, the report is the parity record to keep.  -Q without -b (the
 * loop's bits carry no soft values) or for demodARGOS: a message, exit status 1.
 * -C <file> (an addition, demodPOES): the DCS-2 platform messages the run's minor frames relay (pdt_tip_dcs), one line per
 * packet -- "%.5f %u %u %07u %08X %s " of its time, channel, blocks, time code, ID and Doppler ("%.5f" of the word / 32, behind a '*' when
 * the word's parity is odd, "-" for a packet that is cut off), "%02X " per byte --, then a blank line and the table the reference ends
 * with (POES.m:1291-1307): "%08X %u" per platform ID, most frequent first, ties by ascending ID.  With -W the packets are those of -W's
 * records (after -Q's repair when that is given), otherwise those of the minorFrames file's frames; a run without frames writes an empty
 * file.  One console line reports packets, complete packets, Doppler parity failures and segments.  One channel of a capture taken in one
 * piece, as -W: demodARGOS, a pipe, -l and several -t refuse it.
 * -E <file>, -H <file> (additions, demodPOES): the subcommutated bytes of the run's minor frames (pdt_tip_subcom) -- -E the 60
 * SEM-2 channels of bytes 20 and 21, -H the five analogue housekeeping points of bytes 11 and 14 --, one line per sample, channel by
 * channel: "%.5f %s %u %u %s" of the frame byte's time, the channel's name, the minor-frame counter, the value and the flags (a subset of
 * the letters b i u s: the byte's parity group fails, the counter's group fails, the byte lies in no group, a spike; or "-").  The frames
 * are those -C takes: -W's records (after -Q's repair) where -W is given, otherwise the minorFrames file's; a run without frames writes an
 * empty file.  One console line each reports samples, channels, parity flags and spikes.  The same runs as -C refuse them.
 * -W <file> (an addition, demodPOES): the minor frames a flywheel synchroniser finds in the bits of the capture (pdt_tip_sync, DESIGN
 * 4.18), in the minor-frame text format, beside the unchanged minorFrames file.  -w E,W,G sets its three constants (max_errors, window,
 * fly; default 2,2,3); with -q a second validation line, for these frames, follows the reference's.  One channel of a capture taken
 * in one piece: demodARGOS, a pipe and several -t refuse both switches, and a file demodulated in pieces ends with a message that says so.
 */
#include <ctype.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <time.h>
#include <unistd.h>

#include "pdt.h"
#include "pdt_dev.h"                   /* -D NAME=VALUE: the library's developer switches (tests; the library never reads the environment) */

#ifdef PDT_ARGOS
#define MODE PDT_MODE_ARGOS
#define DEFAULT_CHUNKSIZE 2400
#define OPTS "s:rn:c:o:d:mlPTD:f:x:t:F:B:M:A:R:bW:w:Q:C:E:H:" /* -l (round 4): the sound-card twin's chain, -s its rate in kHz when the samples come from a pipe */
#define BANNER "Project Desert Tortoise: Wave file ARGOS Demodulator (MI355X build)\n"
#define PREFIX "packets"
#define UNIT "Packets"
#else
#define MODE PDT_MODE_POES
#define DEFAULT_CHUNKSIZE 10000
#define OPTS "s:rn:c:o:d:qmlPTD:f:x:t:F:B:M:A:bW:w:Q:C:E:H:"
#define BANNER "Project Desert Tortoise: Wave file NOAA TIP Demodulator (MI355X build)\n"
#define PREFIX "minorFrames"
#define UNIT "Frames"
#endif

/* The reference's progress line, chunk by chunk (POESTIPdemod/main.c:457-481, ARGOSdemod/main.c:286-296).  The loop runs once
 * more with zero samples when the data end exactly at a chunk boundary (fread does not set the end-of-file flag before it
 * comes up short, wave.c:125; main.c:372): that pass prints the line again, feof() being true at last.                      */
#define ANSI_COLOR_RED "\x1b[31m"
#define ANSI_COLOR_GREEN "\x1b[32m"
#define ANSI_COLOR_YELLOW "\x1b[33m"
#define ANSI_COLOR_RESET "\x1b[0m"
/* The lines are printed from the library's progress function (pdt_set_progress): a large capture is demodulated in segments
 * while it is still being read, and every finished segment's chunks are reported while the next one runs.                      */
typedef struct progress_state {
    long num_samples;
    unsigned long chunkSize;
    uint64_t total_chunks;                 /* of the capture */
    int extra;                             /* the zero-sample pass at the end of the file */
    int norm_wanted, norm_printed, lock_printed, any;
    unsigned long i, totalSymbols, totalBits, totalSamples;
    int totalFrames;
#ifdef PDT_ARGOS
    double percentComplete;
#else
    float percentComplete;
#endif
} progress_state;

static void print_norm_and_lock(progress_state *P, const pdt_stats *st)
{
    if (P->norm_wanted && !P->norm_printed) {
        printf("Normalization Factor: %f\n", st->norm_factor);                  /* main.c:420 */
        P->norm_printed = 1;
    }
    if (!P->lock_printed && st->lock_sample >= 0) {
        printf(" : PLL locked at %0.2fHz\n", st->lock_freq_hz);                 /* CarrierTrackingPLL.c:269 */
        P->lock_printed = 1;
    }
}

static void progress_line(progress_state *P, const pdt_chunk_report *q, int last)
{
#ifdef PDT_ARGOS
    if ((((double)(P->i) / P->num_samples) * 100.0 - P->percentComplete > 0.15) || last) {
        P->percentComplete = ((double)(P->i) / P->num_samples) * 100.0;
        printf("\r");
        printf("%0.1f%% %0.3f Ks : %0.1f Sec: %ld Sym : %ld Bits : %d Packets", ((double)(P->i) / P->num_samples) * 100.0,
               (P->totalSamples) / 1000.0, q->time0, P->totalSymbols, P->totalBits, P->totalFrames);
    }
#else
    float averagePhase;
    char qualityString[20];
    if ((((float)(P->i) / P->num_samples) * 100.0 - P->percentComplete > 0.15) || last) {
        P->percentComplete = ((float)(P->i) / P->num_samples) * 100.0;
        averagePhase = (float)q->avg_phase;
        printf("\r");
        printf("%f\t", fabs(M_PI / 2.0 - averagePhase));
        averagePhase = 10.0 * log10f(powf(fabs(M_PI / 2.0 - averagePhase), 2));
        if (averagePhase > -4.3)
            snprintf(qualityString, 20, "%s%02.1fQ%s", ANSI_COLOR_GREEN, averagePhase, ANSI_COLOR_RESET);
        else if (averagePhase > -5)
            snprintf(qualityString, 20, "%s%02.1fQ%s", ANSI_COLOR_YELLOW, averagePhase, ANSI_COLOR_RESET);
        else if (averagePhase > -6)
            snprintf(qualityString, 20, "%s%02.1fQ%s", ANSI_COLOR_YELLOW, averagePhase, ANSI_COLOR_RESET);
        else
            snprintf(qualityString, 20, "%s%02.1fQ%s", ANSI_COLOR_RED, averagePhase, ANSI_COLOR_RESET);
        printf("%0.1f%% %0.3f Ks : %0.1f Sec: %ld Sym : %ld Bits : %d Frames : %s   ", ((float)(P->i) / P->num_samples) * 100.0,
               (P->totalSamples) / 1000.0, (float)q->time0, P->totalSymbols, P->totalBits, P->totalFrames, qualityString);
    }
#endif
}

static void on_progress(void *user, uint64_t first_chunk, const pdt_chunk_report *r, uint64_t n, const pdt_stats *so_far)
{
    progress_state *P = (progress_state *)user;
    print_norm_and_lock(P, so_far);
    for (uint64_t k = 0; k < n; k++) {
        const pdt_chunk_report *q = &r[k];
        const int final_chunk = first_chunk + k + 1 == P->total_chunks;
        P->i += q->samples;
        P->totalBits += q->bits;
        P->totalFrames += (int)q->frames;
        P->totalSymbols += q->symbols;
        P->totalSamples += q->samples;
        progress_line(P, q, final_chunk && !P->extra);                 /* last: feof(inFilePtr) */
        if (final_chunk && P->extra) progress_line(P, q, 1);
        if (final_chunk) printf("\n");
    }
    P->any = 1;
    fflush(stdout);
}

static const char *get_filename_ext(const char *filename)
{
    const char *dot = strrchr(filename, '.');
    if (!dot || dot == filename) return "";
    return dot + 1;
}

static void put_frames(FILE *out, const pdt_frame *f, uint64_t n)
{
    for (uint64_t k = 0; k < n; k++) {                                /* POESTIPdemod/ByteSync.c:62-69,96-101 */
        fprintf(out, f[k].inverted ? "%.5fi " : "%.5f ", f[k].time);
        for (unsigned b = 0; b < f[k].nbytes; b++) fprintf(out, "%.2X ", f[k].bytes[b]);
        if (f[k].complete) fprintf(out, "\n");
    }
    fflush(out);
}

/* The twin's loop (POESTIPdemodPortAudio/main.c:324-393, ARGOSdemodPortAudio/main.c:266-329) with standard input as the sound card: blocks of `chunk`
 * float32 I,Q frames until end of file (there: until a key is hit); frames are appended as they become final. */
static int live_loop(FILE *in, FILE *out, const char *outFileName, double sampleRate, unsigned long chunk, double normFactor,
                     int device, int sampler, int real, double realCenterHz, int decim, double offsetHz, int wbFormat)
{
    if (sampleRate < 1) sampleRate = 48.0;                            /* twin: SAMPLE_RATE 48000 (main.c:27) */
    if (decim) sampleRate /= decim;                                   /* -x: -s is the wideband rate, the context runs at the channel's */
    pdt_config cfg;
    memset(&cfg, 0, sizeof cfg);
#ifdef PDT_ARGOS
    cfg.mode = PDT_MODE_ARGOS;                                        /* + PDT_CHAIN_LIVE: the float build of the ARGOS chain */
#else
    cfg.mode = PDT_MODE_POES;
#endif
    cfg.sample_rate = (uint32_t)(sampleRate * 1000.0);
    cfg.chunk = chunk;
    cfg.norm_override = normFactor;
    cfg.device = device;
    cfg.sampler = sampler;
    cfg.chain = PDT_CHAIN_LIVE;
    pdt_ctx *ctx = NULL;
    int rc = pdt_open(&cfg, &ctx);
    if (rc != PDT_OK) {
        printf("GPU demodulator unavailable: %s\n", pdt_strerror(rc));
        fclose(out);
        remove(outFileName);
        return 1;
    }
    if (real && pdt_set_real_input(ctx, realCenterHz) != PDT_OK) {
        printf("Centre frequency %0.3f kHz must lie between 0 and half the sample rate\n", realCenterHz / 1000.0);
        return 1;
    }
    if (decim && pdt_set_channel(ctx, decim, offsetHz) != PDT_OK) {
        printf("Decimation must be 2 .. 64 and the offset %0.3f kHz below half the wideband rate\n", offsetHz / 1000.0);
        return 1;
    }
    const size_t wbBytes = wbFormat == PDT_FMT_WB_PCM16 ? 4 : wbFormat == PDT_FMT_WB_F32 ? 8 : 2;
    const size_t inFrame = decim ? wbBytes : (real ? 1 : 2) * sizeof(float);        /* -f: mono float32 samples */
    if (decim) chunk *= (unsigned long)decim;                         /* (blocks of one chunk of the channel) */
    float *block = (float *)malloc(sizeof(float) * 2 * chunk);
    pdt_frame *fr = NULL;
    uint64_t cap = 0, total = 0, samples = 0, fresh = 0;
    if (!block || pdt_stream_begin(ctx) != PDT_OK) {
        printf("Error in malloc\n");
        return 1;
    }
    for (;;) {
        const size_t got = fread(block, inFrame, chunk, in);
        if (got) {
            rc = decim ? pdt_stream_push_channel(ctx, block, got, wbFormat, &fresh) : real ? pdt_stream_push_real(ctx, block, got, PDT_FMT_REAL_F32, &fresh) : pdt_stream_push_f32(ctx, block, got, &fresh);
        } else {
            rc = pdt_stream_end(ctx, &fresh);
        }
        if (rc != PDT_OK) {
            printf("Demodulation failed: %s\n", pdt_strerror(rc));
            return 1;
        }
        if (fresh > cap) {
            cap = fresh + 64;
            fr = (pdt_frame *)realloc(fr, cap * sizeof *fr);
            if (!fr) return 1;
        }
        if (fresh) put_frames(out, fr, pdt_stream_frames(ctx, fr, fresh));
        total += fresh;
        samples += got;
        if (!got) break;
        printf("\r%0.1fKsps :%0.3f Sec: %llu Frames", sampleRate, (double)samples / (sampleRate * 1000.0), (unsigned long long)total);
        fflush(stdout);
    }
    pdt_stats st;
    pdt_get_stats(ctx, &st);
    if (st.lock_sample >= 0) printf("\n : PLL locked at %0.2fHz", st.lock_freq_hz);
    printf("\nNormalization Factor: %f\n%llu samples, %llu " UNIT "\n", st.norm_factor, (unsigned long long)samples,
           (unsigned long long)total);
    fclose(out);
    if (total == 0) remove(outFileName);
    free(block);
    free(fr);
    pdt_close(ctx);
    return 0;
}

/* -M: the carrier of ctx's channel stream, every segment at stride N, one line each (pdt_tones at its defaults).
 * Returns 0 when the file is written. */
static int write_tones(pdt_ctx *ctx, const char *name)
{
    const int cap = (int)(pdt_stage_len(ctx, PDT_ST_CHANNEL) / 1024 + 1);
    pdt_tone *tones = (pdt_tone *)malloc((size_t)cap * sizeof *tones);
    int n = 0;
    const int rc = tones ? pdt_tones(ctx, NULL, tones, cap, &n) : PDT_ERR_NOMEM;
    if (rc == PDT_ERR_STATE) printf("-M needs a wideband capture taken in one piece: this one left no channel stream\n");
    else if (rc != PDT_OK) printf("Carrier measurement failed: %s\n", pdt_strerror(rc));
    FILE *m = rc == PDT_OK ? fopen(name, "w") : NULL;
    if (rc == PDT_OK && !m) printf("Error opening %s\n", name);
    if (!m) {
        free(tones);
        return 1;
    }
    for (int i = 0; i < n; i++) fprintf(m, "%.5f %.2f %.1f %.1f\n", tones[i].time_s, tones[i].freq_hz, tones[i].cn0_dbhz, 10.0 * log10(tones[i].power));
    fclose(m);
    free(tones);
    printf("Carrier: %d segments -> %s\n", n, name);
    return 0;
}

/* -R: the rule -A decodes by; NULL = the library's defaults */
static pdt_argos_cfg messageCfgBest;
static const pdt_argos_cfg *messageCfg = NULL;

/* -b: -A's messages come from feed-forward bits (pdt_ff_messages_batch, pdt_stage_ff_bits) */
static int feedForward = 0;

/* -A -b on a plain I,Q file: the file's first two seconds, as float32 (a 16-bit sample / 32768), through the feed-forward kernels and the
 * message kernels; a message's time is the sample index of its bit / Fs.  Returns 0 when the file is written. */
static int write_messages_ff(pdt_ctx *ctx, const int16_t *iq16, uint64_t n, uint32_t rate, const char *name)
{
    float *iq = (float *)malloc((size_t)(n ? n : 1) * 2 * sizeof *iq);
    pdt_ff_sync sync;
    uint64_t nbits = 0;
    int rc = iq ? PDT_OK : PDT_ERR_NOMEM;
    for (uint64_t i = 0; rc == PDT_OK && i < 2 * n; i++) iq[i] = (float)iq16[i] / 32768.0f;
    if (rc == PDT_OK) rc = pdt_stage_ff_bits(ctx, rate, iq, n, NULL, &sync);
    free(iq);
    if (rc == PDT_OK) rc = pdt_ff_read(ctx, NULL, NULL, NULL, NULL, 0, &nbits);
    uint8_t *bits = (uint8_t *)malloc((size_t)nbits + 1);
    int64_t *index = (int64_t *)malloc(((size_t)nbits + 1) * sizeof *index);
    const int cap = (int)(nbits / 65 + 1);
    pdt_argos_msg *msgs = (pdt_argos_msg *)malloc((size_t)cap * sizeof *msgs);
    int found = 0;
    if (rc == PDT_OK && (!bits || !index || !msgs)) rc = PDT_ERR_NOMEM;
    if (rc == PDT_OK) rc = pdt_ff_read(ctx, NULL, bits, NULL, index, nbits, &nbits);
    if (rc == PDT_OK) rc = pdt_stage_argos_messages(ctx, bits, nbits, messageCfg, msgs, cap, &found);
    if (rc == PDT_ERR_ARG) printf("-b needs a sample rate that 800 divides, from 3.2 to 102.4 kHz\n");
    else if (rc != PDT_OK) printf("Message decoding failed: %s\n", pdt_strerror(rc));
    FILE *m = rc == PDT_OK ? fopen(name, "w") : NULL;
    if (rc == PDT_OK && !m) printf("Error opening %s\n", name);
    int bad = !m;
    if (m) {
        if (found > cap) found = cap;
        for (int i = 0; i < found; i++) {
            msgs[i].time_src = index[msgs[i].bit_index];
            msgs[i].time = (double)msgs[i].time_src / (double)rate;
        }
        printf("Feed-forward bits: %llu, carrier %.2f Hz, offset %d, rate step %d\n", (unsigned long long)nbits, sync.residual_hz, (int)sync.tau,
               (int)sync.rate);
        fflush(m);
        bad = pdt_write_argos_messages(msgs, (uint64_t)found, fileno(m), NULL) != PDT_OK;
        fclose(m);
        if (bad) printf("Error writing %s\n", name);
        else printf("Messages: %d -> %s\n", found, name);
    }
    free(bits);
    free(index);
    free(msgs);
    return bad;
}

/* -W: the minor frames the flywheel synchroniser finds in the bits of ctx's last capture, in the minor-frame text format (pdt_tip_sync at
 * its defaults or with -w's constants).  Returns 0 when the file is written; the records stay in *frames for -q. */
static int write_flywheel(pdt_ctx *ctx, const pdt_tip_sync_cfg *cfg, const char *name, pdt_frame **frames, int *count)
{
    const int cap = (int)(pdt_stage_len(ctx, PDT_ST_BITS) / 829 + 1);     /* (emitted frames lie at least 829 bits apart) */
    pdt_frame *fr = (pdt_frame *)malloc((size_t)cap * sizeof *fr);
    int n = 0;
    const int rc = fr ? pdt_tip_sync(ctx, cfg, fr, NULL, cap, &n) : PDT_ERR_NOMEM;
    if (rc == PDT_ERR_STATE) printf("-W needs a capture taken in one piece: this one was demodulated in pieces and left no whole bit stream\n");
    else if (rc == PDT_ERR_ARG) printf("-w E,W,G: E from 0 to 3, W from 1 to 8, G from 2 to 2 W\n");
    else if (rc != PDT_OK) printf("Flywheel synchroniser failed: %s\n", pdt_strerror(rc));
    FILE *m = rc == PDT_OK ? fopen(name, "w") : NULL;
    if (rc == PDT_OK && !m) printf("Error opening %s\n", name);
    if (!m) {
        free(fr);
        return 1;
    }
    if (n > cap) n = cap;
    fflush(m);
    const int wrc = pdt_write_records(fr, (uint64_t)n, fileno(m), NULL);
    fclose(m);
    if (wrc != PDT_OK) {
        printf("Error writing %s\n", name);
        free(fr);
        return 1;
    }
    printf("Flywheel frames: %d -> %s\n", n, name);
    *frames = fr;
    *count = n;
    return 0;
}

/* -C: the DCS packets of -W's records, or (fr == NULL) of the frames of ctx's last capture, which are still on the device, one line each;
 * a blank line; the per-ID table, built here from the packets.  Returns 0 when the file is written. */
typedef struct { uint32_t id, count; } dcs_id_count;
static int dcs_id_order(const void *a, const void *b)
{
    const dcs_id_count *x = (const dcs_id_count *)a, *y = (const dcs_id_count *)b;
    if (x->count != y->count) return x->count > y->count ? -1 : 1;
    return x->id < y->id ? -1 : x->id > y->id;
}
static int dcs_id_value(const void *a, const void *b)
{
    const uint32_t x = ((const dcs_id_count *)a)->id, y = ((const dcs_id_count *)b)->id;
    return x < y ? -1 : x > y;
}

static int write_dcs(pdt_ctx *ctx, const pdt_frame *fr, int nfr, const char *name)
{
    pdt_dcs_summary sum;
    int found = 0;
    memset(&sum, 0, sizeof sum);
    int rc = fr ? pdt_tip_dcs_records(ctx, fr, (uint64_t)nfr, NULL, NULL, 0, &found, &sum) : pdt_tip_dcs(ctx, NULL, NULL, 0, &found, &sum);
    if (!fr && rc == PDT_ERR_STATE) {
        if (pdt_num_frames(ctx)) {
            printf("-C needs a capture taken in one piece: this one was demodulated in pieces and left its frames in no one place\n");
            return 1;
        }
        rc = PDT_OK;                                                   /* (a run without frames: an empty file) */
        found = 0;
    }
    pdt_dcs_packet *pk = (pdt_dcs_packet *)malloc((size_t)(found ? found : 1) * sizeof *pk);
    dcs_id_count *ids = (dcs_id_count *)malloc((size_t)(found ? found : 1) * sizeof *ids);
    if (rc == PDT_OK && (!pk || !ids)) rc = PDT_ERR_NOMEM;
    if (rc == PDT_OK && found) {
        const int cap = found;
        rc = fr ? pdt_tip_dcs_records(ctx, fr, (uint64_t)nfr, NULL, pk, cap, &found, &sum) : pdt_tip_dcs(ctx, NULL, pk, cap, &found, &sum);
        if (found > cap) found = cap;
    }
    if (rc != PDT_OK) printf("DCS decommutation failed: %s\n", pdt_strerror(rc));
    FILE *m = rc == PDT_OK ? fopen(name, "w") : NULL;
    if (rc == PDT_OK && !m) printf("Error opening %s\n", name);
    if (!m) {
        free(pk);
        free(ids);
        return 1;
    }
    int bad = 0;
    if (found) {
        fflush(m);
        bad = pdt_write_dcs_packets(pk, (uint64_t)found, fileno(m), NULL) != PDT_OK;
        fseek(m, 0, SEEK_END);
        for (int k = 0; k < found; k++) ids[k].id = pk[k].id, ids[k].count = 1;
        qsort(ids, (size_t)found, sizeof *ids, dcs_id_value);
        int nid = 0;
        for (int k = 0; k < found; k++) {
            if (nid && ids[nid - 1].id == ids[k].id) ids[nid - 1].count++;
            else ids[nid++] = ids[k];
        }
        qsort(ids, (size_t)nid, sizeof *ids, dcs_id_order);
        fprintf(m, "\n");
        for (int k = 0; k < nid; k++) fprintf(m, "%08X %u\n", (unsigned)ids[k].id, (unsigned)ids[k].count);
    }
    bad |= fclose(m) != 0;
    free(pk);
    free(ids);
    if (bad) {
        printf("Error writing %s\n", name);
        return 1;
    }
    printf("DCS packets: %llu, %llu complete, %llu Doppler parity failures, %llu segments -> %s\n", (unsigned long long)sum.packets,
           (unsigned long long)sum.complete, (unsigned long long)sum.doppler_bad, (unsigned long long)sum.segments, name);
    return 0;
}

/* -E, -H: the samples of built-in table `which` in -W's records, or (fr == NULL) in the frames of ctx's last capture, which are still on
 * the device, one line each.  Returns 0 when the file is written. */
static int write_subcom(pdt_ctx *ctx, const pdt_frame *fr, int nfr, int which, const char *what, const char *name)
{
    pdt_subcom_entry table[256];
    pdt_subcom_summary sum;
    int found = 0;
    const int ne = pdt_subcom_table(which, table, 256);
    memset(&sum, 0, sizeof sum);
    int rc = fr ? pdt_tip_subcom_records(ctx, fr, (uint64_t)nfr, table, (uint64_t)ne, NULL, NULL, 0, &found, NULL, &sum)
                : pdt_tip_subcom(ctx, table, (uint64_t)ne, NULL, NULL, 0, &found, NULL, &sum);
    if (!fr && rc == PDT_ERR_STATE) {
        if (pdt_num_frames(ctx)) {
            printf("%s needs a capture taken in one piece: this one was demodulated in pieces and left its frames in no one place\n", what);
            return 1;
        }
        rc = PDT_OK;                                                   /* (a run without frames: an empty file) */
        found = 0;
    }
    pdt_subcom_sample *sm = (pdt_subcom_sample *)malloc((size_t)(found ? found : 1) * sizeof *sm);
    if (rc == PDT_OK && !sm) rc = PDT_ERR_NOMEM;
    if (rc == PDT_OK && found) {
        const int cap = found;
        rc = fr ? pdt_tip_subcom_records(ctx, fr, (uint64_t)nfr, table, (uint64_t)ne, NULL, sm, cap, &found, NULL, &sum)
                : pdt_tip_subcom(ctx, table, (uint64_t)ne, NULL, sm, cap, &found, NULL, &sum);
        if (found > cap) found = cap;
    }
    if (rc != PDT_OK) printf("Decommutation (%s) failed: %s\n", what, pdt_strerror(rc));
    FILE *m = rc == PDT_OK ? fopen(name, "w") : NULL;
    if (rc == PDT_OK && !m) printf("Error opening %s\n", name);
    if (!m) {
        free(sm);
        return 1;
    }
    int bad = 0;
    if (found) {
        fflush(m);
        bad = pdt_write_subcom(sm, (uint64_t)found, which, fileno(m), NULL) != PDT_OK;
    }
    bad |= fclose(m) != 0;
    free(sm);
    if (bad) {
        printf("Error writing %s\n", name);
        return 1;
    }
    printf("%s samples: %llu in %llu channels, %llu byte parity, %llu counter parity, %llu spikes -> %s\n", which == PDT_SUBCOM_SEM ? "SEM" : "Housekeeping",
           (unsigned long long)sum.samples, (unsigned long long)sum.channels_hit, (unsigned long long)sum.byte_parity, (unsigned long long)sum.id_parity,
           (unsigned long long)sum.spikes, name);
    return 0;
}

/* -b -W (demodPOES): the flywheel's frames out of feed-forward bits (pdt_ffp_frames on the channel stream of a -x capture,
 * pdt_stage_ffp_frames on a plain I,Q file's samples); a frame's time is the sample index of its bit / Fs, seconds of the
 * stream.  Returns 0 when the file is written; the records stay in *frames for -q. */
static int write_repair_report(pdt_ctx *ctx, pdt_frame *fr, int found, const char *name);

static int write_flywheel_ffp(pdt_ctx *ctx, const pdt_tip_sync_cfg *cfg, const char *name, const float *iq, uint64_t n, uint32_t rate, int channel,
                              const char *repairName, pdt_frame **frames, int *count)
{
    const uint64_t ns = channel ? pdt_stage_len(ctx, PDT_ST_CHANNEL) : n;
    const int cap = (int)(ns / (829 * 6) + 2);                            /* (a bit lasts at least 6 samples, frames lie 829 bits apart) */
    pdt_frame *fr = (pdt_frame *)malloc((size_t)cap * sizeof *fr);
    pdt_ffp_sync sync;
    int found = 0;
    memset(&sync, 0, sizeof sync);
    const int rc = !fr ? PDT_ERR_NOMEM : channel ? pdt_ffp_frames(ctx, NULL, cfg, &sync, fr, NULL, cap, &found)
                                                 : pdt_stage_ffp_frames(ctx, rate, iq, n, NULL, cfg, &sync, fr, NULL, cap, &found);
    if (rc == PDT_ERR_STATE) printf("-b -W needs a capture taken in one piece: this one left no whole channel stream\n");
    else if (rc == PDT_ERR_ARG) printf("-b needs a sample rate from 49.92 to 1064.96 kHz; -w E,W,G: E from 0 to 3, W from 1 to 8, G from 2 to 2 W\n");
    else if (rc != PDT_OK) printf("Feed-forward bits failed: %s\n", pdt_strerror(rc));
    FILE *m = rc == PDT_OK ? fopen(name, "w") : NULL;
    if (rc == PDT_OK && !m) printf("Error opening %s\n", name);
    if (!m) {
        free(fr);
        return 1;
    }
    if (found > cap) found = cap;
    printf("Feed-forward bits: %llu in %llu blocks, carrier %.2f Hz, %llu of %llu tone segments valid\n", (unsigned long long)sync.nbits,
           (unsigned long long)sync.nblocks, sync.residual_hz, (unsigned long long)sync.segs_valid, (unsigned long long)sync.segs);
    if (repairName && write_repair_report(ctx, fr, found, repairName)) {
        fclose(m);
        remove(name);
        free(fr);
        return 1;
    }
    fflush(m);
    const int wrc = pdt_write_records(fr, (uint64_t)found, fileno(m), NULL);
    fclose(m);
    if (wrc != PDT_OK) {
        printf("Error writing %s\n", name);
        free(fr);
        return 1;
    }
    printf("Flywheel frames: %d -> %s\n", found, name);
    *frames = fr;
    *count = found;
    return 0;
}

/* -Q: the failed parity groups of the -b -W frames repaired in place from the soft values the feed-forward call left on the device
 * (pdt_tip_repair), and the report: one line per record that had a failing group -- "%.5f" of its time, then " g bit least
 * next" ("%d %d %.9g %.9g") for each failing group in ascending g.  Returns 0 when the report is written. */
static int write_repair_report(pdt_ctx *ctx, pdt_frame *fr, int found, const char *name)
{
    pdt_tip_repair_info *info = (pdt_tip_repair_info *)malloc((size_t)(found ? found : 1) * sizeof *info);
    pdt_tip_repair_summary sum;
    const int rc = !info ? PDT_ERR_NOMEM : pdt_tip_repair(ctx, fr, (uint64_t)found, info, &sum);
    if (rc != PDT_OK) printf("Parity repair failed: %s\n", pdt_strerror(rc));
    FILE *q = rc == PDT_OK ? fopen(name, "w") : NULL;
    if (rc == PDT_OK && !q) printf("Error opening %s\n", name);
    if (!q) {
        free(info);
        return 1;
    }
    for (int f = 0; f < found; f++) {
        if (!info[f].failed) continue;
        fprintf(q, "%.5f", fr[f].time);
        for (int g = 0; g < 5; g++)
            if (info[f].failed >> g & 1) fprintf(q, " %d %d %.9g %.9g", g, (int)info[f].pos[g], (double)info[f].least[g], (double)info[f].next[g]);
        fprintf(q, "\n");
    }
    free(info);
    if (fclose(q)) {
        printf("Error writing %s\n", name);
        return 1;
    }
    printf("Parity repair: %llu records checked, %llu skipped, %llu with a failing group, %llu groups repaired -> %s\n",
           (unsigned long long)sum.checked, (unsigned long long)sum.skipped, (unsigned long long)sum.failing, (unsigned long long)sum.repaired, name);
    return 0;
}

/* -A: the messages in the bits of ctx's last capture, one line each (pdt_argos_messages at its defaults or by -R's rule).
 * Returns 0 when the file is written. */
static int write_messages(pdt_ctx *ctx, const char *name)
{
    const int cap = (int)(pdt_stage_len(ctx, PDT_ST_BITS) / 65 + 1);      /* (messages lie at least 65 bits apart) */
    pdt_argos_msg *msgs = (pdt_argos_msg *)malloc((size_t)cap * sizeof *msgs);
    int n = 0;
    const int rc = msgs ? pdt_argos_messages(ctx, messageCfg, msgs, cap, &n) : PDT_ERR_NOMEM;
    if (rc == PDT_ERR_STATE) printf("-A needs a capture taken in one piece: this one left no bit stream\n");
    else if (rc != PDT_OK) printf("Message decoding failed: %s\n", pdt_strerror(rc));
    FILE *m = rc == PDT_OK ? fopen(name, "w") : NULL;
    if (rc == PDT_OK && !m) printf("Error opening %s\n", name);
    if (!m) {
        free(msgs);
        return 1;
    }
    if (n > cap) n = cap;
    fflush(m);
    const int wrc = pdt_write_argos_messages(msgs, (uint64_t)n, fileno(m), NULL);
    fclose(m);
    free(msgs);
    if (wrc != PDT_OK) {
        printf("Error writing %s\n", name);
        return 1;
    }
    printf("Messages: %d -> %s\n", n, name);
    return 0;
}

/* -x with several -t: one wideband capture, one context per channel, the capture ingested once (pdt_demod_channels); every
 * channel's frames go to a file of its own, outFileName with ".<index>" appended */
static int multi_channel(FILE *in, long data_offset, uint64_t nframes, size_t frame_bytes, int fmt, const pdt_config *cfg, int decim,
                         const double *offsetsHz, int nch, const char *outFileName, const char *measureName, const char *messageName)
{
    pdt_ctx *ctxs[16];
    int rc = PDT_OK;
    for (int i = 0; i < nch && rc == PDT_OK; i++) {
        ctxs[i] = NULL;
        rc = pdt_open(cfg, &ctxs[i]);
        if (rc != PDT_OK) {
            printf("GPU demodulator unavailable: %s\n", pdt_strerror(rc));
            return 1;
        }
        if (pdt_set_channel(ctxs[i], decim, offsetsHz[i]) != PDT_OK) {
            printf("Decimation must be 2 .. 64 and the offset %0.3f kHz below half the wideband rate\n", offsetsHz[i] / 1000.0);
            return 1;
        }
        pdt_keep_pll(ctxs[i], 0);
    }
    unsigned char *buf = (unsigned char *)malloc((size_t)nframes * frame_bytes + 16);
    if (!buf || fseek(in, data_offset, SEEK_SET) != 0 || fread(buf, frame_bytes, (size_t)nframes, in) != (size_t)nframes) {
        printf("Error reading the capture\n");
        return 1;
    }
    rc = pdt_demod_channels(ctxs, nch, buf, nframes, fmt);
    free(buf);
    if (rc != PDT_OK) {
        printf("Demodulation failed: %s\n", pdt_strerror(rc));
        return 1;
    }
    for (int i = 0; i < nch; i++) {
        char name[1200];
        snprintf(name, sizeof name, "%s.%d", outFileName, i);
        FILE *o = fopen(name, "w+");
        if (!o || pdt_write_frames(ctxs[i], fileno(o), NULL) != PDT_OK) {
            printf("Error writing output file\n");
            return 1;
        }
        fclose(o);
        pdt_stats st;
        pdt_get_stats(ctxs[i], &st);
        printf("Channel %d (%+0.3f kHz): ", i, offsetsHz[i] / 1000.0);
        if (st.lock_sample >= 0) printf("PLL locked at %0.2fHz : ", st.lock_freq_hz);
        printf("%0.3f Ks : %llu Sym : %llu Bits : %llu " UNIT " -> %s\n", st.samples / 1000.0, (unsigned long long)st.symbols,
               (unsigned long long)st.bits, (unsigned long long)st.frames, name);
        if (st.frames == 0) remove(name);
        if (measureName) {
            snprintf(name, sizeof name, "%s.%d", measureName, i);
            if (write_tones(ctxs[i], name)) return 1;
        }
        if (messageName) {
            snprintf(name, sizeof name, "%s.%d", messageName, i);
            if (write_messages(ctxs[i], name)) return 1;
        }
        pdt_close(ctxs[i]);
    }
    return 0;
}

static int cmp_float(const void *a, const void *b)
{
    const float x = *(const float *)a, y = *(const float *)b;
    return (x > y) - (x < y);
}

/* -t auto: survey the capture for its carriers (pdt_survey), at most `want` of them, strongest first.  The offsets come back as the
 * printed lines show them, so that a run given those numbers with -t is this run.  Returns 0 when there is at least one. */
static int auto_channels(FILE *in, long data_offset, uint64_t nframes, size_t frame_bytes, int fmt, const pdt_config *cfg, int decim, int want,
                         double *offsetsHz, int *nch)
{
    pdt_ctx *ctx = NULL;
    int rc = pdt_open(cfg, &ctx);
    if (rc != PDT_OK) {
        printf("GPU demodulator unavailable: %s\n", pdt_strerror(rc));
        return 1;
    }
    unsigned char *buf = (unsigned char *)malloc((size_t)nframes * frame_bytes + 16);
    if (!buf || fseek(in, data_offset, SEEK_SET) != 0 || fread(buf, frame_bytes, (size_t)nframes, in) != (size_t)nframes) {
        printf("Error reading the capture\n");
        return 1;
    }
    pdt_survey_cfg sc;
    memset(&sc, 0, sizeof sc);
    sc.max_carriers = want;
    pdt_carrier found[16];
    int count = 0;
    rc = pdt_set_channel(ctx, decim, 0.0);
    if (rc == PDT_OK) rc = pdt_survey(ctx, buf, nframes, fmt, &sc, found, 16, &count);
    free(buf);
    if (rc != PDT_OK) {
        printf("Survey failed: %s\n", pdt_strerror(rc));
        pdt_close(ctx);
        return 1;
    }
    if (count == 0) {
        static float spec[16384];
        double over = 0.0;
        if (pdt_survey_spectrum(ctx, spec, 16384) == PDT_OK) {
            float top = spec[0];
            for (int i = 1; i < 16384; i++)
                if (spec[i] > top) top = spec[i];
            qsort(spec, 16384, sizeof spec[0], cmp_float);
            const double floor = 0.5 * ((double)spec[8191] + (double)spec[8192]);
            over = floor > 0 && top > 0 ? 10.0 * log10((double)top / floor) : 0.0;
        }
        printf("No carrier found (strongest bin %.1f dB over the floor)\n", over);
        pdt_close(ctx);
        return 1;
    }
    for (int i = 0; i < count; i++) {
        char khz[64];
        snprintf(khz, sizeof khz, "%+f", found[i].offset_hz / 1000.0);
        offsetsHz[i] = atof(khz) * 1000.0;
        printf("Channel %d at %s Khz (found, %.1f dB over the floor)\n", i, khz, found[i].peak_db);
    }
    *nch = count;
    pdt_close(ctx);
    return 0;
}

/* The burst search of -t bursts and -t each: one context, the capture read from the file, pdt_bursts (a second call when there are
 * more bursts than the first had room for: all of them count), one line per burst.  Returns 0 when there is at least one burst, in
 * *found_out (the caller's to free), *count_out of them; otherwise the message has been printed.  `keep` not NULL: the context is
 * left open in *keep -- the search left the capture in its input buffer (pdt_demod_windows_held); otherwise it is closed. */
static int burst_search(FILE *in, long data_offset, uint64_t nframes, size_t frame_bytes, int fmt, const pdt_config *cfg, int decim, double max_s,
                        pdt_burst **found_out, int *count_out, pdt_ctx **keep)
{
    enum { ROOM = 4096 };                                /* bursts asked for at first; when there are more, all of them in a second call */
    pdt_ctx *ctx = NULL;
    int rc = pdt_open(cfg, &ctx);
    if (rc != PDT_OK) {
        printf("GPU demodulator unavailable: %s\n", pdt_strerror(rc));
        return 1;
    }
    unsigned char *buf = (unsigned char *)malloc((size_t)nframes * frame_bytes + 16);
    pdt_burst *found = (pdt_burst *)malloc(ROOM * sizeof *found);
    if (!buf || !found || fseek(in, data_offset, SEEK_SET) != 0 || fread(buf, frame_bytes, (size_t)nframes, in) != (size_t)nframes) {
        printf("Error reading the capture\n");
        return 1;
    }
    pdt_bursts_cfg bc;
    memset(&bc, 0, sizeof bc);
    bc.max_s = max_s;
    int count = 0;
    rc = pdt_set_channel(ctx, decim, 0.0);
    if (rc == PDT_OK) rc = pdt_bursts(ctx, buf, nframes, fmt, &bc, found, ROOM, &count);
    if (rc == PDT_OK && count > ROOM) {                  /* platforms are taken from the whole recording, not from its beginning */
        const int room = count;
        free(found);
        found = (pdt_burst *)malloc((size_t)room * sizeof *found);
        rc = found ? pdt_bursts(ctx, buf, nframes, fmt, &bc, found, room, &count) : PDT_ERR_NOMEM;
        if (count > room) count = room;
    }
    free(buf);
    if (rc != PDT_OK || count == 0 || !keep) {
        pdt_close(ctx);
        ctx = NULL;
    }
    if (rc != PDT_OK) {
        printf("Burst search failed: %s\n", pdt_strerror(rc));
        free(found);
        return 1;
    }
    if (count == 0) {
        printf("No burst found\n");
        free(found);
        return 1;
    }
    for (int i = 0; i < count; i++)
        printf("Burst at %.3f s, %.3f s long, %+f Khz, %.1f dB over the floor\n", found[i].start_s, found[i].duration_s, found[i].offset_hz / 1000.0,
               found[i].peak_db);
    if (keep) *keep = ctx;
    *found_out = found;
    *count_out = count;
    return 0;
}

/* -t bursts: search the capture for short transmissions (burst_search) and take the platforms among them (pdt_burst_carriers), at
 * most `want`, strongest first.  Offsets come back as printed, like auto_channels'.  Returns 0 when there is at least one. */
static int burst_channels(FILE *in, long data_offset, uint64_t nframes, size_t frame_bytes, int fmt, const pdt_config *cfg, int decim, int want,
                          double max_s, double *offsetsHz, int *nch)
{
    pdt_burst *found = NULL;
    int count = 0, nplat = 0, rc;
    pdt_carrier plat[16];
    if (burst_search(in, data_offset, nframes, frame_bytes, fmt, cfg, decim, max_s, &found, &count, NULL)) return 1;
    rc = pdt_burst_carriers(found, count, MODE == PDT_MODE_ARGOS ? 550.0 : 4500.0, plat, 16, &nplat);
    free(found);
    if (rc != PDT_OK) {
        printf("Burst search failed: %s\n", pdt_strerror(rc));
        return 1;
    }
    if (nplat > want) nplat = want;
    for (int i = 0; i < nplat; i++) {
        char khz[64];
        snprintf(khz, sizeof khz, "%+f", plat[i].offset_hz / 1000.0);
        offsetsHz[i] = atof(khz) * 1000.0;
        printf("Channel %d at %s Khz (found, %.1f dB over the floor)\n", i, khz, plat[i].peak_db);
    }
    *nch = nplat;
    return 0;
}

/* -t each: search the capture for short transmissions (burst_search), cut a window per burst (pdt_burst_windows) and demodulate the
 * windows in rounds on a pool of contexts, from the copy of the capture the search left on the device (pdt_demod_windows_held).
 * Every window's records, their times counted from the capture's start, go to one file. */
static int each_burst(FILE *in, long data_offset, uint64_t nframes, size_t frame_bytes, int fmt, const pdt_config *cfg, int decim, double max_s,
                      int poolSize, const char *outFileName, const char *measureName, const char *messageName)
{
    enum { POOL = 64 };
    pdt_ctx *holder = NULL, *pool[POOL];
    memset(pool, 0, sizeof pool);
    pdt_burst *found = NULL;
    int count = 0, rc;
    if (burst_search(in, data_offset, nframes, frame_bytes, fmt, cfg, decim, max_s, &found, &count, &holder)) return 1;
    const uint32_t in_rate = cfg->sample_rate * (uint32_t)decim;
    pdt_window *win = (pdt_window *)malloc((size_t)count * sizeof *win);
    rc = win ? pdt_burst_windows(found, count, in_rate, nframes, -1.0, -1.0, win) : PDT_ERR_NOMEM;
    free(found);
    const int npool = count < poolSize ? count : poolSize;
    for (int i = 0; i < npool && rc == PDT_OK; i++) {
        rc = pdt_open(cfg, &pool[i]);
        if (rc == PDT_OK) rc = pdt_set_channel(pool[i], decim, 0.0);
        if (rc == PDT_OK) pdt_keep_pll(pool[i], 0);
    }
    pdt_frame *all = NULL;
    uint64_t total = 0, room = 0;
    pdt_argos_msg *msgs = NULL;                          /* -A: every window's messages, in window order */
    uint64_t nmsgs = 0, msgRoom = 0;
    int locked = 0;
    FILE *measure = measureName && rc == PDT_OK ? fopen(measureName, "w") : NULL;
    if (measureName && rc == PDT_OK && !measure) {
        printf("Error opening %s\n", measureName);
        return 1;
    }
    for (int r0 = 0; r0 < count && rc == PDT_OK; r0 += npool) {
        const int k = count - r0 < npool ? count - r0 : npool;
        rc = pdt_demod_windows_held(holder, pool, k, win + r0);
        if (measure && rc == PDT_OK) {
            /* -M: the first segment of every window of the round that holds one, all in one launch (pdt_tones_batch) */
            pdt_ctx *with[POOL];
            int index[POOL], counts[POOL], m = 0;
            pdt_tone tones[POOL];
            pdt_tone_cfg tc;
            memset(&tc, 0, sizeof tc);
            tc.count = 1;
            for (int i = 0; i < k; i++)
                if (pdt_stage_len(pool[i], PDT_ST_CHANNEL)) {
                    with[m] = pool[i];
                    index[m++] = r0 + i;
                }
            rc = pdt_tones_batch(with, m, &tc, tones, 1, counts);
            for (int i = 0; i < m && rc == PDT_OK; i++)
                if (counts[i])
                    fprintf(measure, "%d %.5f %.2f %.1f %.1f\n", index[i], (double)win[index[i]].first_frame / (double)in_rate + tones[i].time_s,
                            tones[i].freq_hz, tones[i].cn0_dbhz, 10.0 * log10(tones[i].power));
        }
        if (messageName && rc == PDT_OK) {
            /* -A: the messages of every window of the round, all in one launch (pdt_argos_messages_batch); a window of a burst holds
             * a handful at most */
            enum { EACH = 16 };
            static pdt_argos_msg got[POOL * EACH];
            int counts[POOL];
            if (feedForward) {
                /* -b: feed-forward bits of every window that left a channel stream, then the same message kernels, one launch each */
                pdt_ctx *with[POOL];
                static pdt_argos_msg some[POOL * EACH];
                int index[POOL], part[POOL], m = 0;
                for (int i = 0; i < k; i++) {
                    counts[i] = 0;
                    if (pdt_stage_len(pool[i], PDT_ST_CHANNEL)) {
                        with[m] = pool[i];
                        index[m++] = i;
                    }
                }
                rc = pdt_ff_messages_batch(with, m, NULL, messageCfg, NULL, some, EACH, part);
                for (int i = 0; i < m && rc == PDT_OK; i++) {
                    counts[index[i]] = part[i];
                    memcpy(got + index[i] * EACH, some + i * EACH, EACH * sizeof *got);
                }
            } else
                rc = pdt_argos_messages_batch(pool, k, messageCfg, got, EACH, counts);
            for (int i = 0; i < k && rc == PDT_OK; i++) {
                const int n = counts[i] < EACH ? counts[i] : EACH;
                if (nmsgs + (uint64_t)n > msgRoom) {
                    msgRoom = 2 * (nmsgs + (uint64_t)n) + 64;
                    pdt_argos_msg *grown = (pdt_argos_msg *)realloc(msgs, (size_t)msgRoom * sizeof *msgs);
                    if (!grown) {
                        rc = PDT_ERR_NOMEM;
                        break;
                    }
                    msgs = grown;
                }
                const double shift = (double)win[r0 + i].first_frame / (double)in_rate;
                for (int f = 0; f < n; f++) {
                    msgs[nmsgs] = got[i * EACH + f];
                    msgs[nmsgs++].time += shift;
                }
            }
        }
        for (int i = 0; i < k && rc == PDT_OK; i++) {
            const uint64_t n = pdt_num_frames(pool[i]);
            if (total + n > room) {
                room = 2 * (total + n) + 64;
                pdt_frame *grown = (pdt_frame *)realloc(all, (size_t)room * sizeof *all);
                if (!grown) {
                    rc = PDT_ERR_NOMEM;
                    break;
                }
                all = grown;
            }
            pdt_frames(pool[i], all + total, n);
            const double shift = (double)win[r0 + i].first_frame / (double)in_rate;
            for (uint64_t f = 0; f < n; f++) all[total + f].time += shift;
            total += n;
            pdt_stats st;
            pdt_get_stats(pool[i], &st);
            char lock[64] = "none";
            if (st.lock_sample >= 0) {
                snprintf(lock, sizeof lock, "%+.2f Hz", st.lock_freq_hz);
                locked++;
            }
            printf("Burst %d: lock %s, %d packets\n", r0 + i, lock, (int)n);
        }
    }
    for (int i = 0; i < npool; i++)
        if (pool[i]) pdt_close(pool[i]);
    pdt_close(holder);
    free(win);
    if (measure) fclose(measure);
    if (rc != PDT_OK) {
        printf("Demodulation failed: %s\n", pdt_strerror(rc));
        free(all);
        return 1;
    }
    printf("Bursts: %d, locked: %d, packets: %d\n", count, locked, (int)total);
    if (messageName) {
        FILE *m = fopen(messageName, "w");
        if (!m || pdt_write_argos_messages(msgs, nmsgs, fileno(m), NULL) != PDT_OK) {
            printf("Error writing %s\n", messageName);
            return 1;
        }
        fclose(m);
        printf("Messages: %d -> %s\n", (int)nmsgs, messageName);
    }
    free(msgs);
    FILE *o = fopen(outFileName, "w+");
    if (!o || pdt_write_records(all, total, fileno(o), NULL) != PDT_OK) {
        printf("Error writing output file\n");
        return 1;
    }
    fclose(o);
    free(all);
    if (total == 0) remove(outFileName);                 /* as everywhere: no packet, no file (main.c:508-512) */
    return 0;
}

static double now_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return 1e3 * (double)ts.tv_sec + 1e-6 * (double)ts.tv_nsec;
}

int main(int argc, char **argv)
{
    const double t_main = now_ms();                      /* -T: where the run's time goes, one JSON line on stderr at the end */
    int timing = 0;
    unsigned long chunkSize = DEFAULT_CHUNKSIZE;
    double normFactor = 0, sampleRate = 0;
    int outputRawFiles = 0, device = 0, quality = 0, sampler = 0, live = 0, chunkGiven = 0, noProgress = 0, real = 0, c;
    double realCenterHz = 0;
    int decim = 0, nOffsets = 0, wbFormat = PDT_FMT_WB_CU8, autoCarriers = 0;      /* -t auto[:N]: look for up to N carriers */
    double burstMaxS = 5.0;                                                         /* -B: pdt_bursts_cfg.max_s of -t bursts */
    int autoBursts = 0;                                                             /* -t bursts[:N]: autoCarriers platforms, from the burst search */
    int eachBurst = 0;                                                              /* -t each[:N]: every burst in a window of its own, N contexts */
    double offsetsHz[16];
    const char *outOverride = NULL, *measureName = NULL;                            /* -M: the carrier measurement's file */
    const char *messageName = NULL;                                                 /* -A: the ARGOS messages' file */
    const char *flywheelName = NULL;                                                /* -W: the flywheel synchroniser's frames' file */
    const char *repairName = NULL;                                                  /* -Q: the parity repair's report */
    const char *dcsName = NULL;                                                     /* -C: the DCS packets' file */
    const char *semName = NULL, *hkName = NULL;                                     /* -E, -H: the SEM and the housekeeping samples' files */
    pdt_tip_sync_cfg flywheelCfg;                                                   /* -w E,W,G: its constants */
    int flywheelCfgGiven = 0;
    char outFileName[1100];

    printf(BANNER);
    while ((c = getopt(argc, argv, OPTS)) != -1) {
        switch (c) {
        case 's':
            sampleRate = atof(optarg);
            printf("Sample Rate Set To %f Khz\n", sampleRate);
            break;
        case 'r':
            outputRawFiles = 1;
            printf("Outputting Debugging Raw Files\n");
            break;
        case 'n':
            normFactor = atof(optarg);
            printf("Static Gain Override %f\n", normFactor);
            break;
        case 'c':
            chunkSize = (unsigned long)atoi(optarg);
            chunkGiven = 1;
            if (chunkSize != DEFAULT_CHUNKSIZE) printf("Override: Using %ld chunkSize\n", chunkSize);
            break;
        case 'o':
            outOverride = optarg;
            break;
        case 'd':
            device = atoi(optarg);
            break;
        case 'q':
            quality = 1;
            break;
        case 'T':
            timing = 1;
            break;
        case 'D': {                                     /* developer switch, e.g. -D PDT_HBM_LIMIT_MB=2048 (before the context opens) */
            char name[64];
            const char *eq = strchr(optarg, '=');
            const size_t len = eq ? (size_t)(eq - optarg) : strlen(optarg);
            if (len == 0 || len >= sizeof name) return 1;
            memcpy(name, optarg, len);
            name[len] = 0;
            pdt_dev_set(name, eq ? eq + 1 : "1");
            break;
        }
        case 'P':                                       /* no progress lines (and no averagePhase pass on the GPU) */
            noProgress = 1;
            break;
        case 'l':                                       /* the sound-card twin's chain */
            live = 1;
            printf("Using the live (sound card) chain\n");
            break;
        case 'f':                                       /* single-channel input centred at this audio frequency */
            real = 1;
            realCenterHz = atof(optarg) * 1000.0;
            printf("Single-channel input centred at %f Khz\n", atof(optarg));
            break;
        case 'x':                                       /* wideband input at this many times the channel rate */
            decim = atoi(optarg);
            printf("Wideband input, decimation %d\n", decim);
            break;
        case 't':                                       /* a channel's offset from the capture's centre, signed; or auto[:N] */
            if (strncmp(optarg, "auto", 4) == 0) {
                autoCarriers = optarg[4] == ':' ? atoi(optarg + 5) : optarg[4] == 0 ? 16 : 0;
                if (autoCarriers < 1 || autoCarriers > 16) {
                    printf("-t auto or -t auto:N with N from 1 to 16\n");
                    return 1;
                }
                printf("Channels: the %d strongest carriers found\n", autoCarriers);
                break;
            }
            if (strncmp(optarg, "bursts", 6) == 0) {
                autoCarriers = optarg[6] == ':' ? atoi(optarg + 7) : optarg[6] == 0 ? 16 : 0;
                if (autoCarriers < 1 || autoCarriers > 16) {
                    printf("-t bursts or -t bursts:N with N from 1 to 16\n");
                    return 1;
                }
                autoBursts = 1;
                printf("Channels: the %d strongest platforms found by their bursts\n", autoCarriers);
                break;
            }
            if (strncmp(optarg, "each", 4) == 0) {
                eachBurst = optarg[4] == ':' ? atoi(optarg + 5) : optarg[4] == 0 ? 64 : 0;
                if (eachBurst < 1 || eachBurst > 64) {
                    printf("-t each or -t each:N with N from 1 to 64\n");
                    return 1;
                }
                autoCarriers = 16;
                autoBursts = 1;
                printf("Channels: every burst found, in a window of its own\n");
                break;
            }
            if (nOffsets >= 16) {
                printf("At most 16 channels\n");
                return 1;
            }
            offsetsHz[nOffsets++] = atof(optarg) * 1000.0;
            printf("Channel %d at %+f Khz\n", nOffsets - 1, atof(optarg));
            break;
        case 'M':                                       /* the carrier of every burst, or of the channel at a stride, to this file */
            measureName = optarg;
            break;
        case 'A':                                       /* the ARGOS messages in the bits, to this file */
            messageName = optarg;
            break;
#ifdef PDT_ARGOS
        case 'R':                                       /* the rule that picks the messages' heads */
            if (strcmp(optarg, "best") == 0) {
                memset(&messageCfgBest, 0, sizeof messageCfgBest);
                messageCfgBest.rule = PDT_ARGOS_RULE_BEST;
                messageCfg = &messageCfgBest;
            } else if (strcmp(optarg, "first") == 0) messageCfg = NULL;
            else {
                printf("-R first or -R best\n");
                return 1;
            }
            break;
#endif
        case 'W':                                       /* the flywheel synchroniser's minor frames, to this file */
            flywheelName = optarg;
            break;
        case 'Q':                                       /* -b -W: repair the frames' failed parity groups, the report to this file */
            repairName = optarg;
            break;
        case 'C':                                       /* the DCS packets the minor frames relay, to this file */
            dcsName = optarg;
            break;
        case 'E':                                       /* the SEM-2 samples the minor frames carry, to this file */
            semName = optarg;
            break;
        case 'H':                                       /* the analogue housekeeping samples, to this file */
            hkName = optarg;
            break;
        case 'w': {                                     /* max_errors, window, fly of the flywheel's rule */
            int e = 0, w = 0, g = 0;
            char tail = 0;
            if (sscanf(optarg, "%d,%d,%d%c", &e, &w, &g, &tail) != 3 || e < 0 || w < 1 || g < 2) {
                printf("-w E,W,G: E from 0 to 3, W from 1 to 8, G from 2 to 2 W\n");
                return 1;
            }
            memset(&flywheelCfg, 0, sizeof flywheelCfg);
            flywheelCfg.max_errors = e;
            flywheelCfg.window = w;
            flywheelCfg.fly = g;
            flywheelCfg.zero_mask = e == 0 ? PDT_TIP_SYNC_ZERO_MAX_ERRORS : 0;
            flywheelCfgGiven = 1;
            break;
        }
        case 'b':                                       /* -A's messages out of feed-forward bits */
            feedForward = 1;
            break;
        case 'B':                                       /* -t bursts: the longest transmission that is a burst, seconds (0: no limit) */
            burstMaxS = atof(optarg);
            if (!(burstMaxS >= 0)) {
                printf("-B <seconds> must not be negative\n");
                return 1;
            }
            break;
        case 'F':                                       /* the format of the wideband blocks read from a pipe */
            if (strcasecmp(optarg, "cu8") == 0) wbFormat = PDT_FMT_WB_CU8;
            else if (strcasecmp(optarg, "cs8") == 0) wbFormat = PDT_FMT_WB_CS8;
            else if (strcasecmp(optarg, "s16") == 0) wbFormat = PDT_FMT_WB_PCM16;
            else if (strcasecmp(optarg, "f32") == 0) wbFormat = PDT_FMT_WB_F32;
            else {
                printf("Unknown wideband format %s (cu8, cs8, s16, f32)\n", optarg);
                return 1;
            }
            break;
        case 'm':                                       /* MMClockRecovery instead of Gardner (ARGOSdemod/main.c:277) */
            sampler = PDT_SAMPLER_MM;
            printf("Using M&M clock recovery\n");
            break;
        case '?':
            if (optopt == 's' || optopt == 'c' || optopt == 'n')
                fprintf(stderr, "Option -%c requires an argument.\n", optopt);
            else if (isprint(optopt))
                fprintf(stderr, "Unknown option `-%c'.\n", optopt);
            else
                fprintf(stderr, "Unknown option character `\\x%x'.\n", optopt);
            return 1;
        default:
            abort();
        }
    }
    if (autoCarriers && nOffsets) {
        printf("-t %s cannot be combined with -t <kHz>\n", eachBurst ? "each" : autoBursts ? "bursts" : "auto");
        return 1;
    }
    if ((nOffsets || autoCarriers) && !decim) {
        printf("-t requires -x <decimation>\n");
        return 1;
    }
    if (decim && (decim < 2 || decim > 64 || real)) {
        printf("Decimation (-x) must be 2 .. 64, and cannot be combined with -f\n");
        return 1;
    }
    if (decim && !nOffsets && !autoCarriers) offsetsHz[nOffsets++] = 0.0;
    if (live && !chunkGiven) chunkSize = 2400;          /* POESTIPdemodPortAudio/main.c:34 */
    if (chunkSize == (live ? 2400 : DEFAULT_CHUNKSIZE)) printf("Using default %ld chunkSize\n", chunkSize);
    if (optind >= argc) {
        printf("No wave file specified\n");
        return 1;
    }
    const char *inFileName = argv[optind];
    printf("%s\n", inFileName);
    printf("Opening IO files..\n");
    const int from_stdin = live && strcmp(inFileName, "-") == 0;
    if (from_stdin && autoCarriers) {
        printf("-t %s needs a capture file: the spectrum of a stream is not known in advance\n", eachBurst ? "each" : autoBursts ? "bursts" : "auto");
        return 1;
    }
    if (measureName && (from_stdin || live || !decim)) {
        printf("-M needs a wideband capture file (-x) taken in one piece: not a pipe, not -l\n");
        return 1;
    }
    if (feedForward && MODE == PDT_MODE_POES && (!flywheelName || messageName || from_stdin || live || real || nOffsets > 1 || autoCarriers)) {
        printf("-b needs demodARGOS with -A, or demodPOES with -W <file> and a plain I,Q file or one -x channel: not -l, -f, a pipe or several -t\n");
        return 1;
    }
    if (feedForward && MODE == PDT_MODE_ARGOS && (!messageName || from_stdin || live || real || (decim && !eachBurst))) {
        printf("-b needs demodARGOS with -A, and -t each or a plain I,Q file: not -l, -f or another -t\n");
        return 1;
    }
    if (messageName && (MODE != PDT_MODE_ARGOS || from_stdin)) {
        printf("-A needs demodARGOS and a capture taken in one piece: not a pipe\n");
        return 1;
    }
    if ((flywheelName || flywheelCfgGiven) && (MODE != PDT_MODE_POES || from_stdin || nOffsets > 1 || autoCarriers)) {
        printf("-W and -w need demodPOES, one channel and a capture taken in one piece: not a pipe, not several -t\n");
        return 1;
    }
    if (repairName && (MODE != PDT_MODE_POES || !feedForward || !flywheelName)) {
        printf("-Q needs demodPOES with -b -W <file>: the loop's bits carry no soft values\n");
        return 1;
    }
    if (flywheelCfgGiven && !flywheelName) {
        printf("-w sets the constants of -W <file>\n");
        return 1;
    }
    if (dcsName && (MODE != PDT_MODE_POES || from_stdin || live || nOffsets > 1 || autoCarriers)) {
        printf("-C needs demodPOES, one channel and a capture taken in one piece: not a pipe, not -l, not several -t\n");
        return 1;
    }
    if ((semName || hkName) && (MODE != PDT_MODE_POES || from_stdin || live || nOffsets > 1 || autoCarriers)) {
        printf("%s needs demodPOES, one channel and a capture taken in one piece: not a pipe, not -l, not several -t\n", semName ? "-E" : "-H");
        return 1;
    }
    FILE *in = from_stdin ? stdin : fopen(inFileName, "rb");

    time_t t = time(NULL);
    struct tm tm = *localtime(&t);
    if (outOverride)
        snprintf(outFileName, sizeof outFileName, "%s", outOverride);
    else
        snprintf(outFileName, sizeof outFileName, PREFIX "_%4d%02d%02d_%02d%02d%02d.txt", tm.tm_year + 1900, tm.tm_mon + 1,
                 tm.tm_mday, tm.tm_hour, tm.tm_min, tm.tm_sec);
    /* (several channels: a file each, multi_channel; -t auto: the file is opened once the carriers are known) */
    FILE *out = autoCarriers ? NULL : nOffsets > 1 ? stdout : fopen(outFileName, "w+");
    if (!in || (!out && !autoCarriers)) {
        printf("Error opening output files\n");
        exit(1);
    }
    if (outputRawFiles) {
        FILE *raw = fopen("output.raw", "wb");
        if (!raw) {
            printf("Error opening output file\n");
            exit(1);
        }
        fclose(raw);
    }

    if (from_stdin && nOffsets > 1) {
        printf("One channel only from a pipe\n");
        return 1;
    }
    if (from_stdin) return live_loop(in, out, outFileName, sampleRate, chunkSize, normFactor, device, sampler, real, realCenterHz, decim, offsetsHz[0], wbFormat);
    int is_raw = 0, is_8bit = 0;
    if (decim && (strcasecmp(get_filename_ext(inFileName), "cu8") == 0 || strcasecmp(get_filename_ext(inFileName), "cs8") == 0)) {
        if (sampleRate < 1) {
            printf("Sample Rate (in Khz) must be specified when using 8-bit files\n");
            exit(1);
        }
        is_8bit = strcasecmp(get_filename_ext(inFileName), "cu8") == 0 ? PDT_FMT_WB_CU8 : PDT_FMT_WB_CS8;
        printf("Assuming headerless %s 8-bit I,Q input\n", is_8bit == PDT_FMT_WB_CU8 ? "unsigned" : "signed");
    } else if (strcasecmp(get_filename_ext(inFileName), "wav") != 0) {
#ifdef PDT_ARGOS
        printf("RAW files not yet supported :(\n");
        exit(1);
#else
        if (strcasecmp(get_filename_ext(inFileName), "raw") == 0) {
            if (sampleRate < 1) {                                     /* main.c:317-321 */
                printf("Sample Rate (in Khz) must be specified when using RAW files\n");
                exit(1);
            }
            printf(real ? "Assuming single-channel 32-bit IEEE Floating Point RAW input\n" : "Assuming 32-bit IEEE Floating Point RAW input\n");
            is_raw = 1;
        } else {
            printf("Unrecognized file format %s\n", get_filename_ext(inFileName));
            exit(1);
        }
#endif
    }

    uint32_t rate = 0, channels = 2, bits = 32, format = 1, data_bytes = 0;
    long data_offset = 0;
    long num_samples = 44515000;                                     /* RAW: main.c:337 (progress bar only) */
    if (!is_raw && !is_8bit) {
        uint8_t hdr[44];
        if (fread(hdr, 1, 44, in) != 44) {
            printf("Error reading WAV header\n");
            exit(1);
        }
        pdt_wav_parse_header(hdr, &rate, &channels, &bits, &format, &data_bytes);
        data_offset = 44;
        if (real && channels != 1) {
            printf("Single-channel input (-f) requires a mono file, this one has %u channels\n", channels);
            exit(1);
        }
        if (!real && channels != 2) {
            printf("Complex read requires 2 channels (I and Q)\n");
            exit(1);
        }
        if (format != 1) {
            printf("Only PCM is currently supported :(\n");
            exit(1);
        }
        if (bits != 16) {
            printf("Only 16-bit PCM is supported by the MI355X build (the reference truncates other widths, Q5)\n");
            exit(1);
        }
#ifndef PDT_ARGOS
        if (sampleRate > 1 && !decim) rate = (uint32_t)sampleRate;   /* main.c:343-344 (Q6) */
#endif
        if (sampleRate >= 1 && decim) rate = (uint32_t)(sampleRate * 1000.0);          /* -x: -s is the wideband rate in kHz */
#ifdef PDT_ARGOS
        num_samples = (long)((uint32_t)(8u * data_bytes) / (channels * bits));   /* ARGOSdemod/main.c:244, unsigned int arithmetic */
#else
        num_samples = (long)(unsigned long)((8.0 * data_bytes) / (channels * bits));   /* main.c:349 */
#endif
        printf("Sample Rate %.2fKHz and %d bits per sample. Total samples %ld\n", (float)rate / 1000.0, bits, num_samples);
    } else {
        rate = (uint32_t)(sampleRate * 1000.0);                      /* main.c:329: entered in kHz */
    }

    /* the reference reads until EOF, not header.data_size; the library reads the file itself (threaded reads into pinned
     * memory overlapped with the copy to the GPU: pdt_demod_fd) */
    fseek(in, 0, SEEK_END);
    long fsz = ftell(in);
    const size_t frame_bytes = is_8bit ? 2 : (is_raw ? 8 : 4) / (real ? 2 : 1);
    const int sample_format = decim ? (is_8bit ? is_8bit : is_raw ? PDT_FMT_WB_F32 : PDT_FMT_WB_PCM16)
                                    : real ? (is_raw ? PDT_FMT_REAL_F32 : PDT_FMT_REAL_PCM16) : (is_raw ? PDT_FMT_F32 : PDT_FMT_PCM16);
    uint64_t nframes = fsz > data_offset ? (uint64_t)(fsz - data_offset) / frame_bytes : 0;
    const uint64_t in_frames = nframes;
    if (decim) {
        if (rate % (uint32_t)decim) {
            printf("The wideband rate %u Hz is not divisible by the decimation %d\n", rate, decim);
            if (out && out != stdout) {
                fclose(out);
                remove(outFileName);
            }
            exit(1);
        }
        rate /= (uint32_t)decim;
        num_samples = (long)((nframes + (uint64_t)decim - 1) / (uint64_t)decim);      /* (progress runs over the channel's samples) */
        printf("Channel rate %.2fKHz\n", (float)rate / 1000.0);
    }

    pdt_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.mode = MODE;
    cfg.sample_rate = rate;
    cfg.chunk = chunkSize;
    cfg.norm_override = normFactor;
    cfg.device = device;
    cfg.sampler = sampler;
    cfg.chain = live ? PDT_CHAIN_LIVE : PDT_CHAIN_FILE;
    if (eachBurst) return each_burst(in, data_offset, nframes, frame_bytes, sample_format, &cfg, decim, burstMaxS, eachBurst, outFileName, measureName, messageName);
    if (autoCarriers) {
        if (autoBursts ? burst_channels(in, data_offset, nframes, frame_bytes, sample_format, &cfg, decim, autoCarriers, burstMaxS, offsetsHz, &nOffsets)
                       : auto_channels(in, data_offset, nframes, frame_bytes, sample_format, &cfg, decim, autoCarriers, offsetsHz, &nOffsets))
            return 1;
        out = nOffsets > 1 ? stdout : fopen(outFileName, "w+");
        if (!out) {
            printf("Error opening output files\n");
            exit(1);
        }
    }
    if (nOffsets > 1) return multi_channel(in, data_offset, nframes, frame_bytes, sample_format, &cfg, decim, offsetsHz, nOffsets, outFileName, measureName, messageName);
    pdt_ctx *ctx = NULL;
    const double t_open0 = now_ms();
    int rc = pdt_open(&cfg, &ctx);
    const double t_open1 = now_ms();
    if (rc != PDT_OK) {
        printf("GPU demodulator unavailable: %s\n", pdt_strerror(rc));
        fclose(out);
        remove(outFileName);
        exit(1);
    }
#ifdef PDT_ARGOS
    if (outputRawFiles) pdt_keep_presquelch(ctx, 1);                 /* -r: the AGC output before Squelch, ARGOSdemod/main.c:273-274 */
#endif
    if (real && pdt_set_real_input(ctx, realCenterHz) != PDT_OK) {
        printf("Centre frequency %0.3f kHz must lie between 0 and half the sample rate\n", realCenterHz / 1000.0);
        fclose(out);
        remove(outFileName);
        exit(1);
    }
    if (decim && pdt_set_channel(ctx, decim, offsetsHz[0]) != PDT_OK) {
        printf("The offset %0.3f kHz must lie below half the wideband rate\n", offsetsHz[0] / 1000.0);
        fclose(out);
        remove(outFileName);
        exit(1);
    }
    pdt_keep_pll(ctx, 0);                                            /* nothing here reads the PLL output stream */
    if (decim) nframes = (nframes + (uint64_t)decim - 1) / (uint64_t)decim;           /* (the progress lines count channel samples) */
    progress_state prog;
    memset(&prog, 0, sizeof prog);
    prog.num_samples = num_samples;
    prog.chunkSize = (unsigned long)chunkSize;
    prog.total_chunks = (nframes + (uint64_t)chunkSize - 1) / (uint64_t)chunkSize;
    prog.extra = nframes % (uint64_t)chunkSize == 0;
    prog.norm_wanted = normFactor == 0;
    if (!noProgress && num_samples > 0) {                            /* the chunk loop's progress / quality line */
        pdt_keep_quality(ctx, 1);
        pdt_set_progress(ctx, on_progress, &prog);
    }
    /* POES: the one-call form -- a large file is demodulated in segments while it is still being read; a finished segment's
     * text goes to the file (as the reference's fprintf calls do, ByteSync.c:62-101) and its progress lines to the console
     * while the next one runs */
    int text_written = 0;
    fflush(out);
#ifndef PDT_ARGOS
    rc = pdt_demod_file(ctx, fileno(in), (uint64_t)data_offset, in_frames, sample_format, fileno(out), NULL);
    text_written = 1;
#else
    rc = pdt_demod_fd(ctx, fileno(in), (uint64_t)data_offset, in_frames, sample_format);
#endif
    const double t_demod1 = now_ms();
    int16_t *ffIq = NULL;                                            /* -b: the recording's first two seconds (demodPOES: all of it) */
    uint64_t ffFrames = 0;
    if (feedForward && rc == PDT_OK && MODE == PDT_MODE_POES && !decim && sample_format != PDT_FMT_PCM16) {
        printf("-b -W on a plain file needs 16-bit I,Q samples\n");
        rc = PDT_ERR_FORMAT;
    }
    if (feedForward && rc == PDT_OK && !(MODE == PDT_MODE_POES && decim)) {
        ffFrames = in_frames < 2ull * rate || MODE == PDT_MODE_POES ? in_frames : 2ull * rate;
        ffIq = (int16_t *)malloc((size_t)(ffFrames ? ffFrames : 1) * 4);
        if (!ffIq || fseek(in, data_offset, SEEK_SET) || fread(ffIq, 4, (size_t)ffFrames, in) != (size_t)ffFrames) {
            printf("Error reading %s\n", inFileName);
            rc = PDT_ERR_IO;
        }
    }
    fclose(in);
    if (rc != PDT_OK) {
        printf("Demodulation failed: %s\n", pdt_strerror(rc));
        fclose(out);
        remove(outFileName);
        exit(1);
    }
#ifdef PDT_ARGOS
    if (rc == PDT_OK && outputRawFiles) {
        /* ARGOSdemod -r: every chunk's post-AGC, pre-Squelch doubles, appended to output.raw (main.c:171-180,273-274) */
        FILE *raw = fopen("output.raw", "wb");
        /* (the sound-card twin, -l, is the float build: its DECIMAL_TYPE -- and this context's stage elements -- are floats) */
        const size_t es = live ? sizeof(float) : sizeof(double);
        const uint64_t total = pdt_stage_len(ctx, PDT_ST_AGC_RAW), piece = 1u << 20;
        void *tmp = malloc((size_t)piece * sizeof(double));
        if (!raw || !tmp) {
            printf("Error opening output file\n");
            exit(1);
        }
        for (uint64_t at = 0; at < total; at += piece) {
            const int64_t got = pdt_read_stage(ctx, PDT_ST_AGC_RAW, at, piece, tmp);
            if (got <= 0) break;
            fwrite(tmp, es, (size_t)got, raw);
        }
        fclose(raw);
        free(tmp);
    }
#endif
    if (measureName && write_tones(ctx, measureName)) {
        fclose(out);
        remove(outFileName);
        exit(1);
    }
    if (messageName && (feedForward ? write_messages_ff(ctx, ffIq, ffFrames, rate, messageName) : write_messages(ctx, messageName))) {
        fclose(out);
        remove(outFileName);
        exit(1);
    }
    pdt_frame *flyFrames = NULL;
    int flyCount = 0;
    float *ffpIq = NULL;                                             /* -b -W on a plain file: its samples / 32768 */
    if (flywheelName && feedForward && !decim) {
        ffpIq = (float *)malloc((size_t)(ffFrames ? ffFrames : 1) * 2 * sizeof *ffpIq);
        if (!ffpIq) {
            printf("Out of memory\n");
            exit(1);
        }
        for (uint64_t i = 0; i < 2 * ffFrames; i++) ffpIq[i] = (float)ffIq[i] / 32768.0f;
        free(ffIq);
        ffIq = NULL;
    }
    const int flyBad = !flywheelName ? 0
                       : feedForward ? write_flywheel_ffp(ctx, flywheelCfgGiven ? &flywheelCfg : NULL, flywheelName, ffpIq, ffFrames, rate, decim != 0, repairName, &flyFrames, &flyCount)
                                     : write_flywheel(ctx, flywheelCfgGiven ? &flywheelCfg : NULL, flywheelName, &flyFrames, &flyCount);
    free(ffpIq);
    free(ffIq);
    if (flyBad) {
        fclose(out);
        remove(outFileName);
        exit(1);
    }
    if (dcsName && write_dcs(ctx, flywheelName ? flyFrames : NULL, flyCount, dcsName)) {
        fclose(out);
        remove(outFileName);
        exit(1);
    }
    if ((semName && write_subcom(ctx, flywheelName ? flyFrames : NULL, flyCount, PDT_SUBCOM_SEM, "-E", semName)) ||
        (hkName && write_subcom(ctx, flywheelName ? flyFrames : NULL, flyCount, PDT_SUBCOM_HK, "-H", hkName))) {
        fclose(out);
        remove(outFileName);
        exit(1);
    }
    pdt_stats st;
    pdt_get_stats(ctx, &st);
    print_norm_and_lock(&prog, &st);                                 /* (what the progress function has not printed) */

    char *text = NULL;
    fflush(out);
    const double t_text0 = now_ms();
    if (!text_written && pdt_write_frames(ctx, fileno(out), NULL) != PDT_OK) {        /* the minor frames / packets, all at once */
        printf("Error writing output file\n");
        exit(1);
    }
    const double t_text1 = now_ms();
#ifdef PDT_ARGOS
    {
        uint64_t need = pdt_format_frames(ctx, NULL, 0);
        text = (char *)malloc(need + 1);
        pdt_format_frames(ctx, text, need);
        fwrite(text, 1, need, stdout);                               /* ARGOSdemod/ByteSync.c mirrors to stdout */
    }
#endif
    printf("100.0%% %0.3f Ks : %llu Sym : %llu Bits : %llu " UNIT "   (GPU %.3f ms)\n", st.samples / 1000.0,
           (unsigned long long)st.symbols, (unsigned long long)st.bits, (unsigned long long)st.frames, st.gpu_ms);

#ifndef PDT_ARGOS
    if (quality) {
        pdt_tip_summary q;
        if (pdt_tip_check(ctx, &q) == PDT_OK) {
            const char *name = q.spacecraft == 8 ? "NOAA-15" : q.spacecraft == 13 ? "NOAA-18" : q.spacecraft == 15 ? "NOAA-19" : "A UFO!";
            printf("\n%llu out of %llu Error Free Frames\n\n", (unsigned long long)q.good_frames, (unsigned long long)q.frames_checked);
            printf("%llu Good Chunks and %llu Bad Chunks\n\n", (unsigned long long)q.good_chunks, (unsigned long long)q.bad_chunks);
            if (q.t0_ms >= 0) {
                const double h = (double)q.t0_ms / 3600000.0;
                const int hh = (int)h, mm = (int)((h - hh) * 60.0);
                printf("T0 Best Guess: %lld which is %d:%d:%g\n", (long long)q.t0_ms, hh, mm, ((h - hh) * 60.0 - mm) * 60.0);
            }
            printf("Spacecraft: %d=>%s\n", q.spacecraft, name);
            if (q.day >= 0) printf("Julean Day: %d \n", q.day);
        }
        if (flywheelName && pdt_tip_check_records(ctx, flyFrames, (uint64_t)flyCount, &q, NULL) == PDT_OK)
            printf("\nFlywheel: %llu out of %llu Error Free Frames, %llu Good Chunks and %llu Bad Chunks%s\n", (unsigned long long)q.good_frames,
                   (unsigned long long)q.frames_checked, (unsigned long long)q.good_chunks, (unsigned long long)q.bad_chunks,
                   repairName ? " (after -Q's repair every group passes by construction: its report is the parity record)" : "");
    }
#else
    (void)quality;
#endif
    free(flyFrames);
    time_t t2 = time(NULL);
    struct tm tm2 = *localtime(&t2);
    printf("\nThat took %d seconds!\n", (tm2.tm_min * 60 + tm2.tm_sec) - (tm.tm_min * 60 + tm.tm_sec));
    if (fclose(out)) {
        printf("error closing file.");
        exit(-1);
    }
    if (st.frames == 0) {
        printf("\n\nNone bits found :(\nRemoving output file and exiting.\nMAY YOU HAVE MORE BETTER BITS ANOTHER DAY\n");
        remove(outFileName);
    } else {
        printf("\nAll done! Closing files and exiting.\nENJOY YOUR BITS AND HAVE A NICE DAY\n");
    }
    free(text);
    const double t_close0 = now_ms();
    pdt_get_stats(ctx, &st);
    /* (leaving the ~25 GB of buffers to the driver -- no pdt_close, _exit -- was measured: this process ends 30 ms sooner and the
     * NEXT one waits 0.8 s in its runtime start-up while the driver reclaims them) */
    pdt_close(ctx);
    if (timing)          /* (process start -> main and the dynamic loader's share are the caller's wall time minus `total`) */
        fprintf(stderr, "{\"timing_ms\": {\"main_to_open\": %.2f, \"open_hip_ready\": %.2f, \"demod_call\": %.2f, \"of_it_alloc\": %.2f, "
                        "\"of_it_ingest\": %.2f, \"of_it_gpu_last_run\": %.2f, \"progress_and_stats\": %.2f, \"text_write\": %.2f, \"report_and_close_file\": %.2f, "
                        "\"context_close\": %.2f, \"total\": %.2f}}\n",
                t_open0 - t_main, t_open1 - t_open0, t_demod1 - t_open1, st.alloc_ms, st.ingest_ms, st.gpu_ms, t_text0 - t_demod1, t_text1 - t_text0,
                t_close0 - t_text1, now_ms() - t_close0, now_ms() - t_main);
    return 0;
}
