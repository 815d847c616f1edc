/*
 * include/pdt.h -- C ABI of libpdt.so, the MI355X (gfx950) implementation of the
 * POES-TIP / ARGOS IQ demodulation chain of nebarnix/Project-Desert-Tortoise.
 *
 * The reference has no FFI layer: its boundary is (i) the demodPOES/demodARGOS
 * command lines with their minorFrames_*.txt / packets_*.txt files and (ii) the
 * C functions of common/ that POESTIPdemod/main.c and ARGOSdemod/main.c call
 * once per 10 000-sample chunk.  A GPU cannot usefully be entered once per
 * chunk per stage, so this ABI sits one level up: a re-entrant context receives
 * a whole capture (or a large span of it), emulates the reference's chunked
 * semantics internally (chunk size is observable in the output)
 * and hands back decoded frame records; the host program formats the text
 * exactly like POESTIPdemod/ByteSync.c:62-69,96-101 / ARGOSdemod/ByteSync.c:62-70,99-103.
 * Per-stage read-back (pdt_read_stage) exposes every intermediate stream that
 * the reference passes between its stage functions so each stage can be
 * compared with the reference's own output.
 *
 * Plain C types only; caller-owned memory; integer error codes; no globals:
 * one context per capture, contexts are independent (one per GPU / stream).
 *
 * Reference interface replaced by each entry point:
 *   pdt_open            the lazy first-call initialisation of every stage
 *                       (CarrierTrackingPLL.c:88-100, LowPassFilter.c:30-40, AGC.c:92-96,
 *                       GardenerClockRecovery.c:17-21, ByteSync.c:28-39) plus the
 *                       constants at the call sites POESTIPdemod/main.c:346-369,413-454,
 *                       ARGOSdemod/main.c:248-284
 *   pdt_demod_pcm16     the while(!feof) chunk loop POESTIPdemod/main.c:373-492 /
 *                       ARGOSdemod/main.c:250-306 over GetComplexWaveChunk (wave.c:59-175),
 *                       StaticGain (AGC.c:48-75), CarrierTrackPLL (CarrierTrackingPLL.c:54-278),
 *                       LowPassFilterInterp / LowPassFilter (LowPassFilter.c:13-71,76-125),
 *                       NormalizingAGC (AGC.c:78-132), Squelch (AGC.c:24-46),
 *                       GardenerClockRecovery (GardenerClockRecovery.c:5-114) or, on request,
 *                       MMClockRecovery (MMClockRecovery.c:5-83),
 *                       ManchesterDecode (ManchesterDecode.c:10-100),
 *                       ByteSyncOnSyncword (POESTIPdemod/ByteSync.c:16-150) /
 *                       FindSyncWords (ARGOSdemod/ByteSync.c:17-150)
 *   pdt_demod_fd        same, reading the capture file itself: the fread loops of GetComplexWaveChunk / GetComplexRawChunk
 *                       (wave.c:126-172, 483-537) become a threaded read into pinned memory overlapped with the copy to HBM
 *   pdt_demod_device    same, input already resident in HBM (bench / multi-capture)
 *   pdt_demod_f32       the same loop over GetComplexRawChunk (wave.c:413-540): RAW float32 captures
 *   pdt_stream_*        the same loop fed block by block, as POESTIPdemodPortAudio/main.c:324-393 is by
 *                       Pa_ReadStream (the sound-card side itself is out of scope); the function-local statics that carry
 *                       each stage from chunk to chunk there (CarrierTrackingPLL.c:60-75, LowPassFilter.c:21-27, AGC.c:83-84,
 *                       GardenerClockRecovery.c:11-15, ManchesterDecode.c:16-21, ByteSync.c:18-22) are the carried state here
 *   pdt_frames          the fprintf stream of ByteSync.c, as records
 *   pdt_format_frames   the text ByteSync.c writes to the output file
 *   pdt_tip_check       the downstream frame validation the reference keeps in MATLAB:
 *                       standalone_matlab/Functionized/checkParity.m:1-92 (five even-parity checks per TIP
 *                       minor frame) and daytimeDecode.m:1-40 (minor-frame counter, spacecraft id, day,
 *                       millisecond of day, T0) -- SURVEY 8f #2
 *   pdt_make_lpf        MakeLPFIR (LowPassFilter.c:127-175)
 *   pdt_wav_parse_header ReadWavHeader (wave.c:303-378)
 */
#ifndef PDT_H
#define PDT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4, additions without a bump (round 28): the subcommutated bytes of TIP minor frames by table, SEM-2 and the analogue housekeeping points
 * built in -- pdt_subcom_entry, pdt_subcom_cfg, pdt_subcom_sample, pdt_subcom_summary, pdt_tip_subcom, pdt_tip_subcom_records,
 * pdt_host_tip_subcom, pdt_subcom_table, pdt_subcom_name, pdt_tip_subcom_tile, pdt_format_subcom, pdt_write_subcom: a result beside the
 * frames, which stay as they are.
 * 4, additions without a bump (round 27): the DCS-2 platform messages that TIP minor frames relay -- pdt_dcs_cfg, pdt_dcs_packet,
 * pdt_dcs_summary, pdt_tip_dcs, pdt_tip_dcs_records, pdt_host_tip_dcs, pdt_format_dcs_packets, pdt_write_dcs_packets, pdt_tip_dcs_tile: a
 * result beside the frames, which stay as they are.
 * 4, additions without a bump (round 23): POES frames' failed parity groups repaired from the soft bit values -- pdt_tip_repair_info,
 * pdt_tip_repair_summary, pdt_tip_repair, pdt_stage_tip_repair, pdt_host_tip_repair: opt-in, beside everything else.
 * 4, additions without a bump (round 22): POES bits without a loop -- pdt_ffp_cfg, pdt_ffp_sync, pdt_ffp_block, pdt_ffp_bits, pdt_ffp_read,
 * pdt_ffp_blocks, pdt_ffp_frames, pdt_stage_ffp_bits, pdt_stage_ffp_frames, pdt_host_ffp_bits, pdt_host_ffp_mix: a second, opt-in source
 * of POES bits and, through the flywheel, of minor frames, beside everything else.
 * 4, additions without a bump (round 18): a second, opt-in rule for the ARGOS messages' heads -- pdt_argos_cfg.rule (the first of the two
 * reserved words: a zeroed cfg is the rule there was), PDT_ARGOS_RULE_FIRST, PDT_ARGOS_RULE_BEST, PDT_ARGOS_MSG_RUN_LEN,
 * PDT_ARGOS_MSG_SLIP; no new symbol.
 * 4, additions without a bump (round 17): the ARGOS messages in the bits, either polarity, 1 .. 8 blocks, with the platform ID --
 * pdt_argos_cfg, pdt_argos_msg, pdt_argos_messages, pdt_argos_messages_batch, pdt_stage_argos_messages, pdt_host_argos_messages,
 * pdt_argos_msg_tile, pdt_format_argos_messages, pdt_write_argos_messages: a result beside the frames, which stay the reference's.
 * 4, additions without a bump (round 13): the carrier of a channel stream as a measurement -- pdt_tone_cfg, pdt_tone, pdt_tones,
 * pdt_tones_batch, pdt_host_tones: frequency, level and C/N0 of every burst's carrier, or of a channel's carrier at a stride (the
 * Doppler curve).
 * 4, additions without a bump (round 12): every burst of a wideband capture in a window of its own -- pdt_window, pdt_burst_windows,
 * pdt_demod_windows_device, pdt_demod_windows, pdt_demod_windows_held: the bursts of pdt_bursts, each cut out of the capture at its own
 * offset, all windows in one conversion launch.
 * 4, additions without a bump (round 11, test hooks only): pdt_device_math and pdt_device_math_layout -- the kernels' scalar
 * primitives evaluated on the device one record per lane; pdt_host_math codes 9 - 13.
 * 4, additions without a bump (round 10): short transmissions in a wideband capture -- pdt_bursts_cfg, pdt_burst, pdt_row_peak,
 * pdt_bursts, pdt_bursts_device, pdt_burst_carriers, pdt_waterfall_rows, pdt_bursts_shape, pdt_burst_peaks, pdt_host_bursts: when and where the
 * platforms of a capture send, for pdt_set_channel.
 * 4, additions without a bump (round 9): the carrier survey of wideband captures -- pdt_survey_cfg, pdt_carrier, pdt_survey,
 * pdt_survey_device, pdt_survey_spectrum, pdt_host_survey: where the carriers of a capture are, for pdt_set_channel.
 * 4, additions without a bump (round 8): wideband SDR captures through a digital down-converter -- the sample formats
 * PDT_FMT_WB_PCM16 / _F32 / _CU8 / _CS8, the stage PDT_ST_CHANNEL, pdt_set_channel, pdt_demod_channel, pdt_demod_device_channel,
 * pdt_demod_channels_device, pdt_demod_channels, pdt_stream_push_channel, pdt_host_ddc; pdt_demod_fd / pdt_demod_file accept the wideband formats.
 * 4, additions without a bump (round 7): single-channel (real) captures through a Hilbert front end -- the sample formats
 * PDT_FMT_REAL_PCM16 / PDT_FMT_REAL_F32, the stage PDT_ST_ANALYTIC, pdt_set_real_input, pdt_demod_real, pdt_demod_device_real,
 * pdt_stream_push_real, pdt_host_analytic; pdt_demod_fd / pdt_demod_file accept the two real formats.
 * 4 (round 6): a capture that does not fit the device's free memory is demodulated through a bounded window (the streaming
 * path, fed from the file or the caller's memory piece by piece) instead of failing with PDT_ERR_NOMEM -- the reference's chunk
 * loop needs O(chunk) memory whatever the file's length (POESTIPdemod/main.c:373); pdt_stats.segments / .windowed say how a
 * capture was taken; pdt_loop_params.zero_mask; a context whose caller asked for the PLL stream (pdt_keep_pll(ctx, 1)) is
 * never demodulated in overlapped segments.
 * 3 (round 5): + pdt_demod_file (capture file in, frame text out, in one call); pdt_demod_fd / pdt_demod_file demodulate a
 * large POES file in segments while it is still being read BY DEFAULT again (round 4: only on request), after which
 * pdt_read_stage / pdt_stage_len describe the last segment only.
 * 2 (round 4): + pdt_write_frames / pdt_write_records.  Behaviour a client of version 1 should know about, all of it
 * introduced under version 1 in round 3 without a bump: pdt_build_tag, pdt_keep_pll, pdt_stage_bytesync_from and the error
 * code PDT_ERR_IO exist; every pdt_demod_* and pdt_stage_* entry returns PDT_ERR_STATE while a stream is open, and the first
 * pdt_stream_push_* opens one by itself (resetting frames and statistics).                                              */
#define PDT_ABI_VERSION 4

enum { PDT_MODE_POES = 0, PDT_MODE_ARGOS = 1 };
enum { PDT_SAMPLER_GARDNER = 0, PDT_SAMPLER_MM = 1 };

enum {
    PDT_OK = 0,
    PDT_ERR_ARG = -1,       /* bad argument                                  */
    PDT_ERR_NOGPU = -2,     /* no HIP device / HIP runtime failure           */
    PDT_ERR_NOMEM = -3,
    PDT_ERR_FORMAT = -4,    /* unsupported WAV format                        */
    PDT_ERR_RATE = -5,      /* sample rate gives interpolation factor 0 (Fs > 300 kHz, POESTIPdemod/main.c:347) */
    PDT_ERR_STATE = -6,     /* call sequence error                           */
    PDT_ERR_IO = -7         /* read error on the capture file (pdt_demod_fd) */
};

/* intermediate streams, in the order the reference produces them */
enum {
    PDT_ST_PLL = 0,     /* realDataOut of CarrierTrackPLL            DT per input sample        */
    PDT_ST_LOCK,        /* lockSignalStreamOut (ARGOS only)          DT per input sample        */
    PDT_ST_FIR,         /* low-pass output                           DT per interpolated sample */
    PDT_ST_AGC,         /* NormalizingAGC (+Squelch, ARGOS) output   DT per interpolated sample */
    PDT_ST_SYM,         /* Gardner symbols                           DT per symbol              */
    PDT_ST_SYMIDX,      /* global interpolated-sample index each symbol was taken at, int64    */
    PDT_ST_BITS,        /* Manchester bits, '0'/'1'                  uint8 per bit              */
    PDT_ST_BITSYM,      /* global symbol index each bit's time stamp comes from, uint32         */
    PDT_ST_AGC_RAW,     /* NormalizingAGC output BEFORE Squelch (only after pdt_keep_presquelch): what ARGOSdemod -r
                           writes to output.raw (ARGOSdemod/main.c:273-274); equal to PDT_ST_AGC for POES     */
    PDT_ST_ANALYTIC,    /* real captures only: the analytic stream the chain demodulated, float32 I,Q per input sample
                           (pdt_demod_real / pdt_demod_device_real / pdt_demod_fd of a real format in one piece); 0 otherwise */
    PDT_ST_CHANNEL,     /* wideband captures only: the channel stream the chain demodulated, float32 I,Q per channel sample,
                           ceil(N / decim) of them (pdt_demod_channel and its kin); 0 otherwise */
    PDT_ST_COUNT
};

enum { PDT_CHAIN_FILE = 0, PDT_CHAIN_LIVE = 1 };
enum { PDT_FMT_PCM16 = 0, PDT_FMT_F32 = 1 };   /* interleaved little-endian int16 I,Q pairs / IEEE float32 I,Q pairs */
enum { PDT_FMT_REAL_PCM16 = 2, PDT_FMT_REAL_F32 = 3 };   /* single channel: one little-endian int16 / float32 sample per frame */
/* wideband I,Q captures (pdt_set_channel): int16 pairs, float32 pairs, unsigned 8-bit pairs (RTL-SDR), signed 8-bit pairs (HackRF);
 * the 8-bit formats exist only as wideband formats */
enum { PDT_FMT_WB_PCM16 = 16, PDT_FMT_WB_F32 = 17, PDT_FMT_WB_CU8 = 18, PDT_FMT_WB_CS8 = 19 };

typedef struct pdt_config {
    int32_t  mode;            /* PDT_MODE_POES / PDT_MODE_ARGOS                                   */
    uint32_t sample_rate;     /* Hz, the WAV header value (after the -s override, Q6)             */
    uint64_t chunk;           /* reference chunk size in input samples; 0 = 10000 / 2400          */
    double   norm_override;   /* -n option; 0 = StaticGain of the first chunk                     */
    int32_t  device;          /* HIP device ordinal                                               */
    int32_t  profile;         /* 1 = bracket every kernel with HIP events (pdt_kernel_times)      */
    /* Block-parallel evaluation of the PLL / AGC recurrences: each block replays
     * `warm` samples before its own `block` samples; seams are validated bitwise
     * and re-run sequentially on mismatch, so results never depend on these.
     * 0 = defaults derived from the sample rate.                                                  */
    uint32_t pll_block, pll_warm, agc_block, agc_warm;
    /* Gardner boundary-state tables: candidate entry states are tabulated within this many samples of
     * the end point of each of 64 scout trajectories (0 = default 1/8; the true state was further
     * from every scout in ~1 chunk per 9000 of the test captures; candidates merge within a few hundred
     * symbols, so a wider pad costs little).  Smaller = less work, more chunks
     * walked serially; the result never depends on it.                                            */
    double   gardner_band_pad;
    /* Symbol sampler: 0 = GardenerClockRecovery (what the reference runs); 1 = MMClockRecovery
     * (common/MMClockRecovery.c:5-83) at the same call site -- the switch the reference keeps commented out
     * (ARGOSdemod/main.c:277) -- with stepRange / kp below (0 = that call's values, 3 and 0.15).          */
    int32_t  sampler;
    /* Chain variant: 0 = the file programs (POESTIPdemod / ARGOSdemod, what BASELINE measures); 1 = the sound-card
     * twin POESTIPdemodPortAudio (main.c:41-65,324-393): same stage functions, acquisition gain 198.9437, lock threshold
     * 0.10, the lock signal kept and Squelch(0.05) applied between PLL and FIR, Manchester threshold 0.75; default
     * chunk 2400 (its block size).  Feed it float32 frames at 48 kHz to be the twin.  POES only (the ARGOS twin is
     * the float build of the ARGOS chain): PDT_ERR_ARG otherwise.                                                     */
    int32_t  chain;
    double   mm_step_range, mm_kp;
} pdt_config;

typedef struct pdt_frame {
    double   time;        /* time stamp the reference prints with "%.5f"                          */
    int64_t  bit_index;   /* global index of the bit that completed the sync word                 */
    int64_t  time_src;    /* global interpolated-sample index the time stamp derives from         */
    uint8_t  inverted;    /* found through the inverse sync word ("i" suffix, POES only)          */
    uint8_t  nbytes;      /* bytes present: 104 (POES) / 7 (ARGOS) when complete                  */
    uint8_t  complete;    /* all bytes seen (newline emitted)                                     */
    uint8_t  pad;
    uint8_t  bytes[104];
} pdt_frame;

typedef struct pdt_stats {
    uint64_t samples, out_samples, symbols, bits, frames;
    int64_t  lock_sample;         /* global sample index of the one-time PLL lock, -1 = never     */
    double   lock_freq_hz;        /* " : PLL locked at %0.2fHz"                                   */
    double   norm_factor;         /* "Normalization Factor: %f"                                   */
    double   avg_phase;           /* CarrierTrackPLL return value at the lock sample (quality)    */
    uint32_t interp, ntaps;
    uint32_t pll_blocks, pll_seam_fixes, agc_blocks, agc_seam_fixes;
    double   gpu_ms;              /* device time of the last pdt_demod_* call (HIP events)        */
    uint32_t gardner_parallel;    /* 1 = symbol sampler ran through the parallel boundary-state tables,
                                     0 = single-wavefront sequential chain                         */
    uint32_t gardner_walked;      /* chunks whose entry state was outside the tabulated band (walked by the chain) */
    uint32_t gardner_full_domain; /* chunks tabulated over the full boundary-state domain (scouts not locked)       */
    uint32_t sync_overflow;       /* 4096-bit tiles with more than 31 sync hits (generic path used)                */
    uint64_t gardner_candidates;  /* boundary states evaluated by the table kernel                                  */
    double   ingest_ms;           /* (ABI 3) host wall time from the call's start until the capture's last byte had been queued
                                     for the copy to HBM (pdt_demod_fd / _file / _pcm16 / _f32; 0: input was resident)     */
    double   alloc_ms;            /* (ABI 3) host time this PROCESS has spent in device / pinned allocations so far (the cold
                                     path's breakdown: a context's first capture of a size pays for its buffers)          */
    uint32_t segments;            /* (ABI 4) pieces the last capture was demodulated in: 1 = one piece; more (the overlapped
                                     ingest of a large file, the bounded window): pdt_read_stage / pdt_stage_len, the seam
                                     counters and pdt_kernel_times describe the LAST piece only                            */
    uint32_t windowed;            /* (ABI 4) 1 = the capture did not fit the device's free memory and went through the
                                     bounded window (same frames, text, counts and per-chunk reports)                      */
    uint32_t ingest_direct;       /* (ABI 4) 1 = the capture file was read with O_DIRECT straight into the pinned staging (its
                                     pages were not in the page cache, the file system offers it): two passes over host memory
                                     per byte instead of three                                                              */
    int32_t  ingest_numa_node;    /* (ABI 4) NUMA node the reader threads and the staging memory were bound to (the GPU's, when
                                     the file's cached pages lie there or it was read directly); -1 = not bound             */
} pdt_stats;

typedef struct pdt_kernel_time {
    char     name[32];
    uint32_t launches;
    double   total_ms;
} pdt_kernel_time;

typedef struct pdt_ctx pdt_ctx;

int  pdt_abi_version(void);
/* Identifies the build: the first 12 hex digits of the SHA-1 over the library's sources (csrc/, include/pdt.h), set by the
 * Makefile.  Profiles committed under profiles/ record it, so that a figure measured with another build is never quoted. */
const char *pdt_build_tag(void);
const char *pdt_strerror(int code);
int  pdt_device_count(void);

int  pdt_open(const pdt_config *cfg, pdt_ctx **out);

/* The loop constants of the chain (ABI 3).  The reference's stage functions take them as arguments -- CarrierTrackPLL(...,
 * Fs, freqRange, d_lock_threshold, lockSigAlpha, loopbw_acq, loopbw_track) (CarrierTrackPLL.h:11), NormalizingAGC(..., attack_rate,
 * decay_rate) (AGC.h:7), GardenerClockRecovery(..., baud, stepRange, kp) (GardenerClockRecovery.h:3), ManchesterDecode(...,
 * resyncThreshold) (ManchesterDecode.h:3) -- and its mains pass the values a context uses by default (POESTIPdemod/main.c:413,429,
 * 438,445; ARGOSdemod/main.c:265,276-282).  A field left 0 keeps that default; the others replace it in every later
 * pdt_demod_* / pdt_stream_* / pdt_stage_* call of the context, as the value of the context's DECIMAL_TYPE the reference's
 * function would have received.  Nothing else changes: the block-parallel evaluation derives its warm-up lengths from the loop
 * gains it is given and validates every seam bitwise, so the result is the sequential loop's for any constants (only the time
 * moves: loops that contract slowly mean longer warm-ups and more repairs).  pdt_stage_agc's own rate arguments still win
 * over agc_attack / agc_decay.  PDT_ERR_ARG: a negative or non-finite value, a baud rate that leaves fewer than two samples per
 * symbol, a frequency range of half the sample rate or more, a step range above the mains' 0.1 (the samplers' windows and symbol
 * capacities are sized for it).  PDT_ERR_STATE while a stream is open.                                                                          */
typedef struct pdt_loop_params {
    double pll_freq_range_hz;      /* frequency limit of the loop, Hz                                  4500 / 550        */
    double pll_lock_threshold;     /* lock detector threshold                                         0.08 (twin 0.10) / 0.1 */
    double pll_lock_alpha;         /* lockSigAlpha, per sample                                        0.3979 w / 3.1831 w, w = 2 pi / Fs */
    double pll_loopbw_acq;         /* loop bandwidth before the lock, radians per sample              127.3240 w (twin 198.9437 w) / 16 w */
    double pll_loopbw_track;       /* ... after it                                                    10.3451 w / 16 w  */
    double agc_attack, agc_decay;  /* NormalizingAGC rates, per output sample                         79.5775 w', 159.1549 w', w' = 2 pi / (Fs interp) */
    double gardner_baud;           /* symbols per second (Manchester half bits)                       16640.3 / 800     */
    double gardner_step_range;     /* clip of the timing error, at most 0.1                           0.1               */
    double gardner_kp;             /* timing loop gain                                                3.0               */
    double manchester_threshold;   /* resyncThreshold                                                 1.0 (twin 0.75) / 0.5 */
    uint32_t zero_mask;            /* (ABI 4) PDT_LP_ZERO_* bits: the field IS zero (not "keep the default") -- a lock threshold of 0
                                      (lock on the first positive detector value), a timing gain or clip of 0 (open-loop
                                      sampler), a resync threshold of 0.  The other constants must be positive to mean anything */
    uint32_t reserved_;
} pdt_loop_params;
enum { PDT_LP_ZERO_LOCK_THRESHOLD = 1, PDT_LP_ZERO_GARDNER_KP = 2, PDT_LP_ZERO_GARDNER_STEP_RANGE = 4, PDT_LP_ZERO_MANCHESTER_THRESHOLD = 8 };
int  pdt_set_loop_params(pdt_ctx *ctx, const pdt_loop_params *params);
int  pdt_get_device(const pdt_ctx *ctx);          /* the HIP device ordinal the context lives on */
void pdt_close(pdt_ctx *ctx);

/* Use an existing HIP stream (hipStream_t passed as void*) for all work; NULL = own stream. */
int  pdt_set_stream(pdt_ctx *ctx, void *hip_stream);
/* Also keep the AGC output before Squelch (stage PDT_ST_AGC_RAW) in the following pdt_demod_* calls: the stream the
 * reference's `-r` option dumps (ARGOSdemod/main.c:171-180,273-274).  Costs one more stream-sized buffer.            */
int  pdt_keep_presquelch(pdt_ctx *ctx, int enable);

/* Whether the PLL output stream (stage PDT_ST_PLL = CarrierTrackPLL's realDataOut, CarrierTrackingPLL.c:113) is written out in
 * the following pdt_demod_* calls.  At INTERP 1 (sample rates from 150 ksps up) the float chain mixes and filters in one kernel
 * (k_mix_fir): nothing but the filter reads that stream, and with enable = 0 it never goes through HBM -- pdt_stage_len /
 * pdt_read_stage of PDT_ST_PLL then report 0 samples / PDT_ERR_ARG.  On by default (every stage readable after a call); the
 * host programs and the benchmark switch it off.  No effect on the other chains, which always keep the stream.           */
int  pdt_keep_pll(pdt_ctx *ctx, int enable);

/* Also keep what the reference's chunk loop knows after every chunk, in the following pdt_demod_* calls (whole captures; not
 * the streaming entry points): the value CarrierTrackPLL returns for the chunk -- averagePhase, the running mean of
 * |arg(PLL output)| with alpha 0.00005, after the chunk's last sample (CarrierTrackingPLL.c:80,124,152,277), from which
 * POESTIPdemod/main.c:461-481 prints its quality figure 10 log10((pi/2 - averagePhase)^2) -- and the return values of the
 * sampler, the Manchester decoder and the byte synchroniser for that chunk (main.c:438,445,454-460), i.e. everything the
 * "\r" progress line shows.  Before the lock the acquisition kernel delivers averagePhase as it goes; after it, one more
 * block-parallel EMA over the whole capture (same scheme and the same bit-for-bit guarantee as the lock detector's stream).
 * Costs two stream-sized buffers and the EMA walkers' time (16 time constants of 20 000 samples per block: ~6 ms whatever the
 * capture's length).  The overlapped ingest of large captures (pdt_demod_fd / pdt_demod_file) keeps the reports too: its
 * segments end on chunk boundaries, averagePhase and the counts are carried from one to the next.  Off by default.        */
int  pdt_keep_quality(pdt_ctx *ctx, int enable);
typedef struct pdt_chunk_report {
    uint64_t samples;     /* nSamples of the chunk (the last one may be short)                                          */
    double   avg_phase;   /* CarrierTrackPLL's return value for this chunk, exactly (float widened for POES)            */
    uint64_t symbols;     /* GardenerClockRecovery / MMClockRecovery return value                                       */
    uint64_t bits;        /* ManchesterDecode return value                                                              */
    uint64_t frames;      /* ByteSyncOnSyncword / FindSyncWords return value (sync words found in this chunk's bits)    */
    double   time0;       /* waveDataTime[0] when the progress line is printed (ARGOS: after the in-place compactions)  */
} pdt_chunk_report;
/* Per-chunk reports of the last pdt_demod_* call, in chunk order; returns the number copied (out == NULL: the number
 * available; 0 unless pdt_keep_quality was on).                                                                          */
uint64_t pdt_chunk_reports(const pdt_ctx *ctx, pdt_chunk_report *out, uint64_t max_chunks);
/* The same reports WHILE a call runs -- the reference prints its progress line after every chunk (POESTIPdemod/main.c:457-481).
 * With pdt_keep_quality on, `fn` is handed the reports of chunks [first_chunk, first_chunk + n) as soon as they are final:
 * once per completed segment of an overlapped pdt_demod_fd / pdt_demod_file (from a thread of the library, in chunk order,
 * never two calls at a time, the last one before the demod call returns), once at the end of any other whole-capture call
 * (from the caller's thread).  `so_far`: pdt_get_stats as of the last of these chunks (norm_factor from the first chunk on,
 * lock_sample / lock_freq_hz once the PLL has locked: what the reference prints between its progress lines, main.c:420,
 * CarrierTrackingPLL.c:269).  Both pointers are only valid during the call; the callback must not call into the context.
 * fn == NULL switches it off.                                                                                            */
typedef void (*pdt_progress_fn)(void *user, uint64_t first_chunk, const pdt_chunk_report *reports, uint64_t n, const pdt_stats *so_far);
int  pdt_set_progress(pdt_ctx *ctx, pdt_progress_fn fn, void *user);

/* Demodulate one whole capture: nframes interleaved little-endian int16 I,Q pairs
 * in host memory (copied to the GPU) ...                                                        */
int  pdt_demod_pcm16(pdt_ctx *ctx, const int16_t *iq_host, uint64_t nframes);
/* ... or straight from the file the caller opened (what GetComplexWaveChunk / GetComplexRawChunk do with their FILE*,
 * wave.c:59-175,413-540, once per chunk): nframes I,Q pairs of `sample_format` starting at byte_offset (44 for the
 * canonical WAV header ReadWavHeader accepts, 0 for RAW).  The library reads the file in 2 MiB spans with a few host
 * threads into pinned memory and copies them to the GPU while the next spans are being read, so a capture is in HBM about
 * as soon as the page cache and the PCIe link allow.  PDT_ERR_FORMAT when the file ends early, PDT_ERR_IO on a read error
 * (EINTR is retried).
 * Large POES captures (2.5 GiB and more -- below that the segments' latency floors cost more than the overlap hides --, Gardner sampler): the chain starts before the last span has
 * arrived and runs in three unequal segments with carried state (the streaming path over the resident capture; 55 / 28 /
 * 17 % of the capture, cut where a segment can use the whole-capture kernels, so that only the last, small one is left to run
 * when the last byte has arrived).  Frames, text and pdt_get_stats' counts then describe the whole capture as ever; but
 * pdt_read_stage / pdt_stage_len describe the LAST SEGMENT only (window-local indices), the pll / agc seam counters and
 * gpu_ms are the last segment's, and no stream is left open behind the call (pdt_stats.segments says so; a context
 * whose caller switched the PLL stream on, pdt_keep_pll(ctx, 1), is demodulated in one piece).
 * A capture that does not fit (ABI 4): when the buffers of a whole capture -- about 8 x the file for POES at 250 ksps --
 * exceed the device's free memory, the capture goes through a bounded window instead (pieces of the file pushed through the
 * streaming path with carried state: same frames, text, counts and reports; pdt_stats.windowed = 1).  The reference's loop
 * takes a file of any length (POESTIPdemod/main.c:373, while(!feof)); so do pdt_demod_fd / _file / _pcm16 / _f32.            */
/* sample_format PDT_FMT_REAL_PCM16 / _F32 (2 / 4 bytes per frame): a single-channel capture (pdt_demod_real below).         */
/* sample_format PDT_FMT_WB_* (4 / 8 / 2 / 2 bytes per frame), once pdt_set_channel has been called: a wideband capture of
 * nframes input frames (pdt_demod_channel below); it is ingested whole, then converted -- never in overlapped segments, and one
 * that does not fit the device's memory returns PDT_ERR_NOMEM (the bounded window for wideband input does not exist yet).    */
int  pdt_demod_fd(pdt_ctx *ctx, int fd, uint64_t byte_offset, uint64_t nframes, int sample_format);
/* The whole job of POESTIPdemod/main.c:373-492 / ARGOSdemod/main.c:250-306 in one call: capture file in (as pdt_demod_fd), the
 * minor-frame / packet text out to the descriptor text_fd, from its position on -- the reference's ByteSync.c:62-101 writes
 * that text with fprintf WHILE it demodulates, and so does this: where the capture is demodulated in segments (above) the
 * text of a finished segment is formatted and written while the next segment runs, so that what is left behind the last
 * kernel is the last segment's text alone.  Otherwise it is pdt_demod_fd followed by pdt_write_frames.  *text_bytes (may be
 * NULL) = bytes written.  pdt_frames / pdt_get_stats / pdt_format_frames afterwards as after pdt_demod_fd.  (ABI 3)     */
int  pdt_demod_file(pdt_ctx *ctx, int fd, uint64_t byte_offset, uint64_t nframes, int sample_format, int text_fd,
                    uint64_t *text_bytes);
/* ... or already resident in device memory (no copy; buffer is only read).                      */
int  pdt_demod_device(pdt_ctx *ctx, const void *iq_device, uint64_t nframes);

/* Batched many-capture mode: `count` independent captures, one context each, inputs resident in
 * device memory.  The kernels of all captures are enqueued back to back on the contexts' own streams -- they
 * overlap on the GPU, whose serial recurrences leave most of it idle for a single capture -- and the results are
 * collected afterwards; each context then holds exactly what pdt_demod_device would have produced.
 * (Measured: 1.5x the single-capture throughput at 8 captures of 30 M samples.)                             */
int  pdt_demod_batch_device(pdt_ctx *const *ctxs, const void *const *iq_device, const uint64_t *nframes, int count);

/* RAW input of demodPOES (".raw": interleaved IEEE float32 I,Q used as they are, no normalisation;
 * GetComplexRawChunk, wave.c:413-540, POESTIPdemod/main.c:313-339; the sample rate comes from -s).
 * POES only -- ARGOSdemod/main.c:238-241 refuses RAW files.  Non-finite samples (NaN, +-infinity) are
 * taken as the reference takes them: every stream, the norm factor and the frames are the reference's.  */
int  pdt_demod_f32(pdt_ctx *ctx, const float *iq_host, uint64_t nframes);
int  pdt_demod_device_f32(pdt_ctx *ctx, const void *iq_device, uint64_t nframes);

/* Streaming front end: feed a capture piece by piece, as the reference's real-time twin does with
 * 2 400-frame sound-card blocks (POESTIPdemodPortAudio/main.c:324-393), and collect minor frames as they become final.
 * Like the reference's chunk loop, every stage carries its state from one piece of work to the next: whenever a push
 * completes one or more reference chunks, exactly those new chunks are demodulated -- PLL phase / frequency / lock state,
 * the FIR's last inputs, AGC gain, sampler state (nextSample, halfSample, prev), Manchester history and clock phase, the
 * byte synchroniser's last bits and open frame all continue from where the previous segment ended -- and the frames
 * completed by these chunks are reported.  Cost per push depends on the push, not on the length of the stream; the device
 * keeps a bounded window of the input (the PLL's warm-up history, see pdt_stream_retained) and nothing else of the past.
 * Guarantee: the frames reported by the pushes followed by those of pdt_stream_end are exactly the frames of one
 * pdt_demod_* call on the whole capture.
 *   pdt_stream_begin      forget any stream in progress (the sample format is fixed by the first push); optional: the first
 *                         push after pdt_open / pdt_stream_end opens a new stream by itself.  While a stream is open (first
 *                         push .. pdt_stream_end / pdt_stream_begin) the stage buffers hold the tails the next push continues
 *                         from: every pdt_demod_* and pdt_stage_* entry returns PDT_ERR_STATE
 *   pdt_stream_push_*     append nframes I,Q pairs; *new_frames = frames that became final with this push
 *   pdt_stream_end        the capture is over: demodulate the short last chunk, report the remaining frames (a frame cut
 *                         by the end stays partial, Q11); afterwards pdt_frames / pdt_get_stats / pdt_format_frames
 *                         describe the whole stream
 *   pdt_stream_frames     the frames reported by the last push / end, in order
 *   pdt_stream_retained   input samples the device currently holds (history + not yet demodulated)                  */
int      pdt_stream_begin(pdt_ctx *ctx);
int      pdt_stream_push_pcm16(pdt_ctx *ctx, const int16_t *iq_host, uint64_t nframes, uint64_t *new_frames);
int      pdt_stream_push_f32(pdt_ctx *ctx, const float *iq_host, uint64_t nframes, uint64_t *new_frames);
int      pdt_stream_end(pdt_ctx *ctx, uint64_t *new_frames);
uint64_t pdt_stream_frames(const pdt_ctx *ctx, pdt_frame *out, uint64_t max_frames);
uint64_t pdt_stream_retained(const pdt_ctx *ctx);

/* Single-channel (real) captures: SatNOGS audio, an SDR in USB mode, a sound card with one input.  A real capture x[n] at
 * the context's sample rate becomes one float32 I,Q pair per sample on the GPU -- z[n] = (x[n] + j H{x}[n]) e^{-j 2 pi p[n] / 2^32},
 * H a 63-tap Blackman-windowed Hilbert transformer (centred, no delay; x = 0 outside the capture), p[n] = step n mod 2^32 on the
 * global sample index, step = round(centre 2^32 / Fs) -- and the chain demodulates that stream exactly as it would a RAW float
 * capture of the same length (POES: pdt_demod_f32, StaticGain of the first chunk included; ARGOS: the double chain reading the
 * float pairs).  Int16 samples are s / 32768, float32 samples are used as they are.  The arithmetic is fixed:
 * pdt_host_analytic restates it bit for bit on the host.
 *   pdt_set_real_input     the centre frequency the real captures of this context are mixed down from: 0 < centre_hz < Fs / 2,
 *                          0 = Fs / 4 (also the default); PDT_ERR_ARG otherwise, PDT_ERR_STATE while a stream is open
 *   pdt_demod_real         a whole real capture in host memory, n samples of sample_format (PDT_FMT_REAL_PCM16 / _F32, else
 *                          PDT_ERR_ARG); results through pdt_frames / pdt_get_stats / pdt_format_frames / pdt_read_stage
 *                          (PDT_ST_ANALYTIC = the converted stream), reports and progress as for I,Q captures.  One that does not
 *                          fit the device goes through the bounded window (pdt_stats.windowed); never in overlapped segments
 *   pdt_demod_device_real  the same with the samples resident in device memory (only read)
 *   pdt_stream_push_real   append n real samples to the open stream: the last 31 samples are held back until their right-hand
 *                          neighbours arrive (pdt_stream_end closes them with zeros; pdt_stream_retained counts them); the frames
 *                          of the pushes and of the end are those of one pdt_demod_real call.  A stream takes real pushes of one
 *                          format or I,Q pushes: mixing them returns PDT_ERR_ARG
 *   pdt_host_analytic      test hook, host only: out[2 n], out[2 n + 1] = the I,Q pair of sample n, as the kernel computes it   */
int  pdt_set_real_input(pdt_ctx *ctx, double center_hz);
int  pdt_demod_real(pdt_ctx *ctx, const void *x_host, uint64_t n, int sample_format);
int  pdt_demod_device_real(pdt_ctx *ctx, const void *x_device, uint64_t n, int sample_format);
int  pdt_stream_push_real(pdt_ctx *ctx, const void *x_host, uint64_t n, int sample_format, uint64_t *new_frames);
int  pdt_host_analytic(uint32_t sample_rate, double center_hz, const void *x, uint64_t n, int sample_format, float *out);

/* Wideband SDR captures: an RTL-SDR, a HackRF or any receiver that records complex samples at Fs_in with the beacon some
 * hundreds of kHz off centre, perhaps several carriers at once.  The context is opened at the CHANNEL rate; the wideband input is
 * at Fs_in = decim x sample_rate.  On the GPU the capture x[n] becomes the channel stream
 *   y[m] = sum_{k = -8 decim .. 8 decim} h[k] x[m decim + k] e^{-j 2 pi p[m decim + k] / 2^32},   0 <= m < ceil(N / decim),
 * p[n] = step n mod 2^32 on the global sample index, step = round(offset_hz 2^32 / Fs_in), h the Blackman-windowed sinc of
 * 16 decim + 1 taps with its cut-off at 0.4 of the channel rate (x = 0 outside the capture), and the chain demodulates that stream
 * exactly as it would a RAW float capture of the same length (POES: pdt_demod_f32; ARGOS: the double chain reading the float
 * pairs).  Samples are scaled by format: int16 s / 32768, float32 as they are, unsigned 8-bit (u - 127.5) / 128, signed 8-bit
 * s / 128.  Time stamps are seconds of the channel stream.  The arithmetic is fixed: pdt_host_ddc restates it bit
 * for bit on the host.
 *   pdt_set_channel            the channel of this context's wideband captures: PDT_ERR_ARG unless 2 <= decim <= 64 and
 *                              |offset_hz| < Fs_in / 2; PDT_ERR_STATE while a stream is open
 *   pdt_demod_channel          a whole wideband capture in host memory, nframes input frames of sample_format (PDT_FMT_WB_*, else
 *                              PDT_ERR_ARG; PDT_ERR_STATE before pdt_set_channel); results, reports, progress and statistics as for
 *                              any capture; PDT_ST_CHANNEL = the converted stream.  One that does not fit the device's memory
 *                              returns PDT_ERR_NOMEM: the bounded window for wideband input does not exist yet
 *   pdt_demod_device_channel   the same with the samples resident in device memory (only read).  The address must be aligned
 *                              to the format's element (2 bytes for int16, 4 for float32, 1 for the 8-bit formats), not to
 *                              the I,Q pair or to 16 bytes: any such address is served, the aligned ones with wider loads;
 *                              so too for pdt_demod_channels_device and pdt_survey_device
 *   pdt_demod_channels_device  ONE wideband capture in device memory, `count` contexts with a channel each: one conversion
 *                              launch per context fills that context's channel stream, then the contexts go
 *                              through the batched chain (pdt_demod_batch_device's, on float input).  All contexts must have the
 *                              same decim and live on the same device (else PDT_ERR_ARG); their modes may differ.  Each context
 *                              ends up holding exactly what pdt_demod_device_channel alone would have produced
 *   pdt_demod_channels         pdt_demod_channels_device for a capture in host memory: it is copied to the device once, into
 *                              the first context's input buffer (PDT_ERR_NOMEM when it does not fit)
 *   pdt_stream_push_channel    append nframes wideband frames to the open stream: the last 8 decim + (pushed mod decim) input
 *                              samples are held back until their neighbours arrive (pdt_stream_end closes them with zeros;
 *                              pdt_stream_retained counts them); the frames of the pushes and of the end are those of one
 *                              pdt_demod_channel call.  A stream takes pushes of one kind and format: mixing them returns
 *                              PDT_ERR_ARG
 *   pdt_host_ddc               test hook, host only: out[2 m], out[2 m + 1] = the I,Q pair of channel sample m, as the kernel
 *                              computes it; in_rate is Fs_in                                                                   */
int  pdt_set_channel(pdt_ctx *ctx, int decim, double offset_hz);
int  pdt_demod_channel(pdt_ctx *ctx, const void *iq_host, uint64_t nframes, int sample_format);
int  pdt_demod_device_channel(pdt_ctx *ctx, const void *iq_device, uint64_t nframes, int sample_format);
int  pdt_demod_channels_device(pdt_ctx *const *ctxs, int count, const void *iq_device, uint64_t nframes, int sample_format);
int  pdt_demod_channels(pdt_ctx *const *ctxs, int count, const void *iq_host, uint64_t nframes, int sample_format);
int  pdt_stream_push_channel(pdt_ctx *ctx, const void *iq_host, uint64_t nframes, int sample_format, uint64_t *new_frames);
int  pdt_host_ddc(uint32_t in_rate, int decim, double offset_hz, const void *x, uint64_t n, int sample_format, float *out);

/* The carrier survey of a wideband capture: which offsets to give pdt_set_channel.  The chain's PLL sweeps a few kHz at most (4500 Hz
 * POES, 550 Hz ARGOS), a cheap receiver's crystal alone is off by more.  The stretch [first_frame, first_frame + nframes) of the
 * capture is cut into consecutive segments of nfft samples (a last incomplete one is dropped), each is Blackman-windowed and
 * transformed in float32 on the GPU, the segments' power spectra are averaged in a fixed order, and the host looks for carriers in
 * the average: noise floor = its median; repeatedly the strongest bin left, as long as it stands threshold_db over the floor, its
 * frequency the centroid of the power above the floor within merge_hz of it, then the bins within guard_hz of it are blanked.
 * The arithmetic is fixed: pdt_host_survey restates it bit for bit on the host.
 * pdt_survey_cfg: a zero in a field means its default -- nfft 16384 (1024, 4096 and 16384 are allowed), max_carriers 16,
 * threshold_db 15, guard_hz half the channel rate, merge_hz the mode's PLL frequency range (pdt_loop_params.pll_freq_range_hz when
 * set), first_frame 0, nframes to the end of the capture.
 *   pdt_survey_device    the capture resident in device memory (only read), nframes frames of sample_format (PDT_FMT_WB_*); the
 *                        context supplies device, stream, mode and the wideband rate decim x sample_rate (PDT_ERR_STATE before
 *                        pdt_set_channel, whose offset plays no part).  Up to min(cap, max_carriers) carriers, strongest first, in
 *                        found[], their number in *count.  PDT_ERR_ARG: another format, an nfft that is not allowed, a stretch
 *                        outside the capture or shorter than one segment, cap < 1.  The context's demodulation results, stages
 *                        and statistics are left alone, and a later demodulation is what it would have been without the survey
 *   pdt_survey           the same for a capture in host memory: copied to the device once, into the context's input buffer
 *   pdt_survey_spectrum  the averaged spectrum of the context's last survey, n = its nfft floats (else PDT_ERR_ARG; PDT_ERR_STATE
 *                        before a survey): bin b at b Fs_in / nfft, the upper half the negative frequencies
 *   pdt_host_survey      test hook, host only: the same spectrum (spectrum_out, nfft floats, may be NULL) and carriers as the
 *                        kernels and the host search produce; in_rate is Fs_in, mode_range_hz and channel_rate stand for what the
 *                        context supplies to the defaults of merge_hz and guard_hz                                              */
typedef struct pdt_survey_cfg {
    int nfft;
    int max_carriers;
    double threshold_db, guard_hz, merge_hz;
    uint64_t first_frame, nframes;
} pdt_survey_cfg;
typedef struct pdt_carrier {
    double offset_hz;       /* from the capture's centre, [-Fs_in / 2, Fs_in / 2) */
    float peak_db;          /* the strongest bin over the floor */
    float floor_power;      /* the median of the averaged spectrum */
} pdt_carrier;
int  pdt_survey_device(pdt_ctx *ctx, const void *iq_device, uint64_t nframes, int sample_format, const pdt_survey_cfg *cfg,
                       pdt_carrier *found, int cap, int *count);
int  pdt_survey(pdt_ctx *ctx, const void *iq_host, uint64_t nframes, int sample_format, const pdt_survey_cfg *cfg,
                pdt_carrier *found, int cap, int *count);
int  pdt_survey_spectrum(const pdt_ctx *ctx, float *out, int n);
int  pdt_host_survey(uint32_t in_rate, double mode_range_hz, uint32_t channel_rate, int sample_format, const void *x, uint64_t nframes,
                     const pdt_survey_cfg *cfg, float *spectrum_out, pdt_carrier *found, int cap, int *count);

/* Short transmissions in a wideband capture: the spectrum over time and the bursts in it.  The survey above looks at ONE spectrum
 * averaged over the stretch: a platform that sends for half a second every two minutes (ARGOS) stands 23 dB lower in it than while
 * it is on, and a line that is always there (the DC spike of a cheap receiver, a birdie) looks like a carrier.  Here the stretch's
 * segments -- the survey's, transformed in the same way -- are added in rows of rows_per consecutive ones (a last incomplete row
 * is dropped), every row is searched for up to 8 bins that stand threshold_db over the survey's floor (the median of the survey's
 * averaged spectrum of the same stretch at the same nfft; the bins within guard_hz of a peak are blanked for the next), and the host
 * links the rows' peaks into bursts: a peak continues the open track whose last bin is nearest within merge_hz, a track not
 * continued for more than gap_rows rows closes, and a closed track whose length lies in [min_s, max_s] is a burst -- max_s is what
 * drops the lines that are always there.  A strong transmitter's modulation sidebands reach beyond guard_hz: a peak is not linked when
 * its own row holds a peak at least 25 dB stronger within 4 guard_hz of it (the rows' peak records keep it).  The arithmetic is fixed: pdt_host_bursts restates it bit for bit.
 * pdt_bursts_cfg: a zero in a field means its default -- nfft 4096 (1024, 4096, 16384), rows_per 8 (1 .. 64), threshold_db 15,
 * guard_hz half the channel rate, merge_hz the mode's PLL frequency range, gap_rows 1, min_s two rows, max_s no upper limit,
 * first_frame 0, nframes to the end of the capture.
 *   pdt_bursts_device    the capture resident in device memory (only read); context, preconditions and error codes as for
 *                        pdt_survey_device (PDT_ERR_ARG also for rows_per outside 1 .. 64 and a stretch shorter than one row).
 *                        *count = the number of bursts found, found[] = the first min(cap, *count), ordered by start, then
 *                        offset.  The rows live on the device a slab at a time, whatever the capture's length.  Like a survey it
 *                        leaves the context's results, stages, statistics and pdt_survey_spectrum alone
 *   pdt_bursts           the same for a capture in host memory: copied to the device once, into the context's input buffer
 *   pdt_burst_carriers   host only: bursts whose offsets lie within merge_hz of each other are one platform, its offset the mean
 *                        of theirs weighted by their peak power; the platforms strongest first, for pdt_set_channel; *n = their
 *                        number, carriers[] = the first min(cap, *n)
 *   pdt_waterfall_rows   rows first_row .. first_row + nrows - 1 of the context's last burst search (for plots and tests), nrows x
 *                        nfft floats, bin b of a row at b Fs_in / nfft: they are computed again from the capture, which must still
 *                        be where it was.  PDT_ERR_STATE before a burst search, and after pdt_bursts once the context's input
 *                        buffer has taken another capture; PDT_ERR_ARG for rows outside the search
 *   pdt_bursts_shape     nfft, rows_per and the number of rows of the context's last burst search (each pointer may be NULL;
 *                        PDT_ERR_STATE as for pdt_waterfall_rows): how large the buffers of the two calls around it must be
 *   pdt_burst_peaks      the peaks of those rows as the search found them: out[8 r + k], k < counts[r] (the rest zero), strongest
 *                        first; kept on the host, the capture is not needed
 *   pdt_host_bursts      test hook, host only: rows (rows_out), peaks (peaks_out, 8 a row, and peak_counts_out) and bursts as the
 *                        kernels and the host linking produce them; each of the three outputs may be NULL                        */
typedef struct pdt_bursts_cfg {
    int nfft;
    int rows_per;
    int gap_rows;
    double threshold_db, guard_hz, merge_hz;
    double min_s, max_s;
    uint64_t first_frame, nframes;
} pdt_bursts_cfg;
typedef struct pdt_burst {
    uint64_t first_row, rows;       /* rows of the search: rows_per nfft input frames each */
    double start_s;                 /* (first_frame + first_row rows_per nfft) / Fs_in */
    double duration_s;              /* rows rows_per nfft / Fs_in */
    double offset_hz;               /* from the capture's centre, [-Fs_in / 2, Fs_in / 2) */
    float peak_db;                  /* its strongest row bin over floor x rows_per */
    float floor_power;              /* the median of the survey's averaged spectrum */
} pdt_burst;
typedef struct pdt_row_peak {
    int32_t bin;
    float below, power, above;      /* the row at bin - 1, bin, bin + 1 (wrapping at the band's edge) */
} pdt_row_peak;
int  pdt_bursts_device(pdt_ctx *ctx, const void *iq_device, uint64_t nframes, int sample_format, const pdt_bursts_cfg *cfg,
                       pdt_burst *found, int cap, int *count);
int  pdt_bursts(pdt_ctx *ctx, const void *iq_host, uint64_t nframes, int sample_format, const pdt_bursts_cfg *cfg,
                pdt_burst *found, int cap, int *count);
int  pdt_burst_carriers(const pdt_burst *bursts, int count, double merge_hz, pdt_carrier *carriers, int cap, int *n);
int  pdt_waterfall_rows(pdt_ctx *ctx, uint64_t first_row, uint64_t nrows, float *out);
int  pdt_bursts_shape(const pdt_ctx *ctx, int *nfft, int *rows_per, uint64_t *nrows);
int  pdt_burst_peaks(const pdt_ctx *ctx, uint64_t first_row, uint64_t nrows, pdt_row_peak *out, int *counts);
int  pdt_host_bursts(uint32_t in_rate, double mode_range_hz, uint32_t channel_rate, int sample_format, const void *x, uint64_t nframes,
                     const pdt_bursts_cfg *cfg, float *rows_out, pdt_row_peak *peaks_out, int *peak_counts_out, pdt_burst *found,
                     int cap, int *count);

/* Every burst in a window of its own.  pdt_burst_carriers merges the bursts of a capture into platforms and the whole capture is then
 * demodulated once per platform at one offset.  That fails where it matters: a platform's Doppler moves by kilohertz over a pass while
 * the ARGOS loop sweeps 550 Hz, and a capture that opens with noise takes its normalisation from noise and winds the acquisition loop
 * up on it.  Here each burst is cut out of the capture at its own measured offset: a window [first_frame, first_frame +
 * nframes) of the capture is a capture of its own -- samples outside it count as zero although the capture has neighbours, the
 * mixer's phase is counted from the window's first sample, time stamps are seconds of the window's channel stream -- and all windows
 * of a call are converted by ONE launch (k_ddc over a table of their tiles), then the contexts go through the batched chain.
 *   pdt_burst_windows          host only: window i from burst i.  first_frame = llround((start_s + skip) Fs_in), the end is
 *                              min(capture_frames, llround((start_s + duration_s + tail) Fs_in)), offset_hz the burst's; a window whose
 *                              start reaches its end has nframes 0.  skip_s < 0: the default, one row of that burst (duration_s /
 *                              rows) -- start_s lies up to a row BEFORE the transmission, and a window must begin inside the carrier,
 *                              not in the noise in front of it; tail_s < 0: 0.1 s.  PDT_ERR_ARG: a null pointer with count > 0,
 *                              in_rate 0, a non-finite argument or burst
 *   pdt_demod_windows_device   ONE wideband capture in device memory (only read), `count` contexts with a window each.  Context i ends
 *                              up holding byte for byte what
 *                                  pdt_set_channel(ctxs[i], decim, win[i].offset_hz);
 *                                  pdt_demod_device_channel(ctxs[i], (const char *)iq_device + win[i].first_frame * frame_bytes,
 *                                                           win[i].nframes, sample_format);
 *                              alone would have produced -- frames, text, statistics, PDT_ST_CHANNEL, reports and progress -- and its
 *                              channel offset is left at its window's.  Preconditions and errors as for pdt_demod_channels_device
 *                              (every context after pdt_set_channel, same decim and device, all distinct, no open stream; modes may
 *                              differ); PDT_ERR_ARG also for a window that reaches beyond nframes or whose |offset_hz| >= Fs_in / 2.
 *                              Windows may overlap, repeat and be empty
 *   pdt_demod_windows          the same for a capture in host memory: copied to the device once, into the first context's input buffer
 *                              (PDT_ERR_NOMEM when it does not fit)
 *   pdt_demod_windows_held     the same for the capture that `holder`'s last pdt_bursts or pdt_survey call (or their _device forms)
 *                              read, which must still be where it was: search, then demodulate in rounds, with one copy of the
 *                              capture.  PDT_ERR_STATE before such a call and once the holder's input buffer has taken another
 *                              capture (pdt_waterfall_rows' rule); PDT_ERR_ARG when holder is among ctxs.  The holder's results,
 *                              spectrum, burst list and pdt_waterfall_rows are left alone                                          */
typedef struct pdt_window {
    uint64_t first_frame, nframes;  /* of the capture */
    double offset_hz;               /* from the capture's centre */
} pdt_window;
int  pdt_burst_windows(const pdt_burst *bursts, int count, uint32_t in_rate, uint64_t capture_frames, double skip_s, double tail_s,
                       pdt_window *out);
int  pdt_demod_windows_device(pdt_ctx *const *ctxs, int count, const pdt_window *win, const void *iq_device, uint64_t nframes,
                              int sample_format);
int  pdt_demod_windows(pdt_ctx *const *ctxs, int count, const pdt_window *win, const void *iq_host, uint64_t nframes, int sample_format);
int  pdt_demod_windows_held(pdt_ctx *holder, pdt_ctx *const *ctxs, int count, const pdt_window *win);

/* The carrier as a measurement: its frequency, its level and its C/N0.  ARGOS locates platforms from the Doppler shift of their carrier;
 * pdt_burst.offset_hz is a centroid of 250 Hz bins and pdt_stats.lock_freq_hz the loop's integrator at one instant -- neither is a
 * measurement.  Every ARGOS burst opens with 160 ms of unmodulated carrier and a window of pdt_burst_windows begins inside it; a POES
 * channel carries a residual carrier all the time.  The channel stream of the context's last whole-capture call (PDT_ST_CHANNEL, in
 * device memory) is cut into segments of nfft samples, segment i from first + i stride on; only segments wholly inside the stream are
 * measured.  Each is Blackman-windowed and transformed as a segment of the survey is; the strongest bin with |f_b| <= search_hz is the
 * peak (of equal ones the lowest bin), a log-parabola through it and its two neighbours gives frequency and level, and the float sum
 * of the bins at circular distance noise_lo .. noise_hi from the peak gives the noise density.  The arithmetic is fixed (DESIGN 4.15,
 * csrc/pdt_tone.h): pdt_host_tones restates it bit for bit on the host.
 * pdt_tone_cfg: a zero in a field means its default -- nfft the largest of 1024, 4096, 16384 with nfft / Fs <= 0.128 s (PDT_ERR_ARG
 * when there is none), search_hz the mode's PLL frequency range (pdt_loop_params.pll_freq_range_hz when set; pdt_host_tones, which has
 * no mode: every bin but the band's edge), noise_lo 8 and noise_hi 71 (128 bins), first 0, stride nfft, count to the end of the stream.
 *   pdt_tones        the context's channel stream: out[i] = segment i, *count = the number measured = min(cap, segments asked for and
 *                    present) -- 0 for a stream shorter than first + nfft.  PDT_ERR_STATE when the last call left no PDT_ST_CHANNEL
 *                    (no wideband capture yet, another kind of capture, a stream open or ended, a capture taken in pieces);
 *                    PDT_ERR_ARG for an nfft that is not allowed, a negative or non-finite search_hz or one >= Fs / 2, noise_lo < 1,
 *                    noise_lo > noise_hi, noise_hi >= nfft / 2, cap < 1.  Like a survey it leaves the context's results, stages,
 *                    statistics, pdt_survey_spectrum and burst list exactly as they were (a profiled context's pdt_kernel_times
 *                    gain the entry k_tones)
 *   pdt_tones_batch  the same for `count` contexts in ONE launch (the windows of a round of pdt_demod_windows_*): context i's
 *                    records at out + i cap_each, their number in counts[i].  The contexts must be distinct, live on one device and
 *                    have one sample rate (else PDT_ERR_ARG); every one is checked as pdt_tones checks its own before anything runs
 *   pdt_host_tones   test hook, host only: the same records for any float32 I,Q stream of n samples at `rate`; offset_hz stands for
 *                    the context's channel offset
 * pdt_tone: time_s = the segment's middle, (first + i stride + (nfft - 1) / 2) / Fs, in seconds of the channel stream; residual_hz
 * = the carrier's frequency in the channel stream, freq_hz = the channel's offset + residual_hz, from the capture's centre; power = the
 * carrier's power, |amplitude|^2 of the stream's samples; cn0_dbhz = 10 log10(power / noise density); then the raw record as the
 * kernel leaves it: the peak's bin, the segment's power spectrum at bin - 1, bin, bin + 1 (wrapping at nfft), the noise bins' sum and
 * their number.  valid = 0 -- a neighbour that is not > 0, no maximum in the log-parabola, an all-zero search set --: the frequencies
 * are the bin's centre, power the bin's own, cn0_dbhz NaN.                                                                          */
typedef struct pdt_tone_cfg {
    int32_t nfft;
    int32_t noise_lo, noise_hi;
    int32_t reserved_;
    double search_hz;
    uint64_t first, stride, count;
} pdt_tone_cfg;
typedef struct pdt_tone {
    double time_s, freq_hz, residual_hz, power, cn0_dbhz;
    int32_t valid;
    int32_t bin;
    float below, peak, above, noise_sum;
    int32_t noise_bins;
    int32_t reserved_;
} pdt_tone;
int  pdt_tones(pdt_ctx *ctx, const pdt_tone_cfg *cfg, pdt_tone *out, int cap, int *count);
int  pdt_tones_batch(pdt_ctx *const *ctxs, int count, const pdt_tone_cfg *cfg, pdt_tone *out, int cap_each, int *counts);
int  pdt_host_tones(uint32_t rate, double offset_hz, const float *iq, uint64_t n, const pdt_tone_cfg *cfg, pdt_tone *out, int cap, int *count);

/* Who sent what: the ARGOS messages in the Manchester bits (ARGOS contexts).  The frames above are the reference's, byte for byte: one
 * 13-bit word, upright only, so one-block messages of one polarity and 56 bits printed of the 52.  A platform sends 1 .. 8 blocks of 32
 * bits behind a 20-bit ID, and a mirrored spectrum (I and Q swapped, a conjugated capture) complements every bit.  The messages are a
 * result BESIDE the frames; the rule is fixed in csrc/pdt_argos_msg.h and pdt_host_argos_messages restates it on the host:
 * with c[i] = bit i XOR the polarity, a head ends at bit e when c[e-12 .. e-4] = 000101111 (frame sync and initialisation bit), c[e-3 .. e]
 * is a length code (N - 1 in three bits and an even-parity bit, N = 1 .. 8), the min_run raw bits in front of the sync are all equal --
 * EITHER value: they are the bit-sync ones, whose Manchester pairing is arbitrary until the first data transition -- and e >= 12 + min_run;
 * the body is the 20 + 32 N bits behind e.  Heads are taken in ascending e; one that begins inside the body of the message accepted
 * before it is dropped.  28-bit IDs cannot be told from 20-bit ones without the platform registry: such a platform's first data byte is
 * the rest of its ID.
 * pdt_argos_cfg: NULL or a zero field = the default, min_run 6 (allowed 0 .. 15); min_run 0 with PDT_ARGOS_ZERO_MIN_RUN in zero_mask
 * asks for no run at all (as pdt_loop_params.zero_mask does for a loop constant).
 * pdt_argos_cfg.rule: PDT_ARGOS_RULE_FIRST (0, the default) is the rule above.  PDT_ARGOS_RULE_BEST (1) tolerates one stray bit and picks
 * among overlapping heads by the length of their run: with run_len(s), s in {0, 1}, = the number of equal raw bits that end at bit
 * e-13-s (counted backwards to at most 15, not past bit 0; 0 when that bit does not exist), a head at e -- sync and length code as
 * above -- takes s = 0 if run_len(0) >= min_run, otherwise s = 1 if run_len(1) >= min_run, otherwise it is none (min_run 0: s = 0); the
 * bit e-13 of an s = 1 head is a stray bit of either value.  Its score is 2 run_len(s) + (1 - s), its span [e-12, e+20+32 N].  A head
 * is accepted if and only if no accepted head of higher priority -- the higher score, at equal score the smaller e -- has a span that
 * overlaps its own; rejected heads leave no trace and the records come in ascending e.  Selection runs per cluster: in ascending e a
 * head joins the current cluster if its span begins at or before the largest span end seen in it and the cluster holds fewer than 256
 * heads, else it opens a new one; the heads accepted in the preceding cluster count as accepted (this matters only where the cap of 256
 * closed it).  Under rule 1 run_value = the bit e-13-s as the polarity reads it (0 when run_len is 0) and reserved_ carries run_len and
 * s (PDT_ARGOS_MSG_RUN_LEN, PDT_ARGOS_MSG_SLIP); under rule 0 reserved_ is 0.  Any other rule is PDT_ERR_ARG at every entry.  A profiled
 * context's kernel times name rule 1's kernels k_argos_heads and k_argos_pick.
 * pdt_argos_msg: bit_index = e; time_src and time = those of a pdt_frame whose sync word completes at bit e (an upright one-block
 * message carries exactly its frame's); id, blocks = N, inverted = the polarity, run_value = the run's bits as that polarity reads them
 * (1: the bit-sync ones came out as ones; 0 when min_run is 0); data = the 32 N data bits, MSB first, in 4 N bytes, the rest 0; complete = 1 when the stream holds the whole body, else
 * data_bits (otherwise 32 N) says how many data bits are present, and the missing bits are 0.
 *   pdt_argos_messages        the bits of the context's last whole-capture call (PDT_ST_BITS, in device memory; their count is read
 *                             there): *count = the messages found, the first min(cap, *count) of them in out, in ascending bit_index.
 *                             PDT_ERR_STATE when the last call left no resident bit stream (none yet, a stream open or ended, a capture
 *                             taken in pieces, a stage-level call); PDT_ERR_ARG for a POES context, min_run outside 0 .. 15, cap < 0.
 *                             Like pdt_tones it leaves frames, text, stages, statistics, survey and burst results exactly as they were
 *                             (a profiled context's pdt_kernel_times gain the entries k_argos_msgs and k_argos_finish)
 *   pdt_argos_messages_batch  the same for `count` contexts with ONE launch of each kernel (the windows of a round of
 *                             pdt_demod_windows_*): context i's records at out + i cap_each, their number in counts[i].  The contexts
 *                             must be distinct and live on one device (else PDT_ERR_ARG); every one is checked before anything runs
 *   pdt_stage_argos_messages  stage-level entry: the kernels on a caller's string of '0'/'1' characters (any byte other than '0' is a
 *                             one); the time stamp of bit k is k, as in pdt_stage_bytesync.  Nothing of the context's results changes
 *   pdt_host_argos_messages   host only, no GPU: the same records for the same string
 *   pdt_argos_msg_tile        the bits one workgroup tests (tests place heads at its seams)
 * Text, host only: one line per COMPLETE message -- "%.5f" of time, "i" when inverted, " %d %05X" of blocks and id, " %02X" per data
 * byte, "\n" -- through pdt_format_argos_messages (returns the bytes needed, writes at most cap) or pdt_write_argos_messages (to an
 * open descriptor; PDT_ERR_IO when a write fails; *bytes_written may be NULL).                                                        */
#define PDT_ARGOS_ZERO_MIN_RUN 1u
#define PDT_ARGOS_RULE_FIRST 0
#define PDT_ARGOS_RULE_BEST  1
#define PDT_ARGOS_MSG_RUN_LEN(m) ((int)((m)->reserved_ & 0xffu))        /* rule 1: run_len(s) of the record *m */
#define PDT_ARGOS_MSG_SLIP(m)    ((int)(((m)->reserved_ >> 8) & 1u))    /* rule 1: s, 1 = a stray bit between run and sync */
typedef struct pdt_argos_cfg {
    int32_t  min_run;
    uint32_t zero_mask;
    int32_t  rule;
    int32_t  reserved_;
} pdt_argos_cfg;
typedef struct pdt_argos_msg {
    double   time;
    int64_t  bit_index;
    int64_t  time_src;
    uint32_t id;
    uint8_t  blocks, inverted, complete, run_value;
    uint32_t data_bits;
    uint32_t reserved_;
    uint8_t  data[32];
} pdt_argos_msg;
int  pdt_argos_messages(pdt_ctx *ctx, const pdt_argos_cfg *cfg, pdt_argos_msg *out, int cap, int *count);
int  pdt_argos_messages_batch(pdt_ctx *const *ctxs, int count, const pdt_argos_cfg *cfg, pdt_argos_msg *out, int cap_each, int *counts);
int  pdt_stage_argos_messages(pdt_ctx *ctx, const uint8_t *bits_host, uint64_t nbits, const pdt_argos_cfg *cfg, pdt_argos_msg *out, int cap,
                              int *count);
int  pdt_host_argos_messages(const uint8_t *bits, uint64_t nbits, const pdt_argos_cfg *cfg, pdt_argos_msg *out, int cap, int *count);
int  pdt_argos_msg_tile(void);
uint64_t pdt_format_argos_messages(const pdt_argos_msg *msgs, uint64_t n, char *buf, uint64_t cap);
int  pdt_write_argos_messages(const pdt_argos_msg *msgs, uint64_t n, int fd, uint64_t *bytes_written);

/* POES frames from a flywheel synchroniser (POES contexts).  The frames above are the reference's: a minor frame is taken
 * only if all 19 bits of its sync word (or of the complement) are right, sync words are ignored while a frame is open, and the first
 * match wins.  One wrong bit among the 19 loses 832 good ones, and one false match swallows the true sync word behind it.  Minor frames
 * come every F = 832 bits, so these entries believe a sync word because its neighbours are where they should be: a second, opt-in
 * source of pdt_frame records BESIDE the frames; the rule is fixed in csrc/pdt_tip_sync.h and pdt_host_tip_sync restates it on the host.
 * With S = 1110110111100010000 and a position p = the index of the bit that would complete a sync word (pdt_frame.bit_index),
 * 18 <= p < n: dist+(p) = the Hamming distance of bits p-18 .. p to S and dist-(p) = 19 - dist+(p); p is a CANDIDATE of polarity s when
 * dist_s(p) <= max_errors; its SUPPORT u_s(p) is the number of k in {-window .. -1, 1 .. window} for which p + k F is a candidate of s
 * (exact multiples of F only; a position outside [18, n) is none).  p is a HEAD of s when p + 813 < n -- the whole frame is present,
 * incomplete frames are not emitted -- and either it is a candidate with u_s >= 1, or u_s >= fly: the flywheel, whose own sync word
 * may be arbitrarily damaged.  A head's key is (u_s, candidate, -dist_s), compared lexicographically; where both polarities are heads
 * at one p the larger key stands, the upright one at equal keys.  A head h is emitted if and only if no other head g with
 * |g - h| <= F - 4 has a larger key, or an equal one and g < h -- judged against all heads, emitted or not, so the result depends on no
 * order, and frames that overlap by up to three bits (a slipped bit) are both emitted.  A record is filled as the reference prints a
 * frame: bytes 0xED 0xE2, the five bits behind p under three zero bits, then 101 bytes MSB first, every data bit complemented for an
 * inverted head; nbytes 104, complete 1; time and time_src those of a pdt_frame whose sync word completes at bit p.  Records come in
 * ascending bit_index; pdt_write_records / pdt_format_records print them, pdt_tip_check_records validates them.
 * pdt_tip_sync_cfg: NULL or a zero field = the default -- max_errors 2 (allowed 0 .. 3; a real 0 with PDT_TIP_SYNC_ZERO_MAX_ERRORS in
 * zero_mask), window 2 (1 .. 8), fly 3 (2 .. 2 window).  pdt_tip_sync_info (optional, parallel to the records): the distance, support
 * and candidate bit of the polarity that stands.
 *   pdt_tip_sync         the bits of the context's last whole-capture call (PDT_ST_BITS, in device memory; their count is read there):
 *                        *count = the frames found, the first min(cap, *count) of them in out (and info, when not NULL).
 *                        PDT_ERR_STATE when the last call left no resident bit stream (none yet, a stream open or ended, a capture
 *                        taken in pieces, a stage-level call); PDT_ERR_ARG for an ARGOS context, a cfg out of range, cap < 0.  It leaves
 *                        frames, text, stages, statistics and every other result exactly as they were (a profiled context's
 *                        pdt_kernel_times gain the entries k_tip_cand, k_tip_heads, k_tip_pick, k_tip_scan and k_tip_pack)
 *   pdt_tip_sync_batch   the same for `count` contexts with ONE launch of each kernel (the slots of pdt_demod_batch_device): context
 *                        i's records at out + i cap_each (info + i cap_each), their number in counts[i].  The contexts must be
 *                        distinct and live on one device (else PDT_ERR_ARG); every one is checked before anything runs
 *   pdt_stage_tip_sync   stage-level entry: the kernels on a caller's string of '0'/'1' characters (any byte other than '0' is a one);
 *                        the time stamp of bit k is k.  Nothing of the context's results changes
 *   pdt_host_tip_sync    host only, no GPU: the same records for the same string
 *   pdt_tip_sync_tile    the bits one workgroup tests (tests place sync words at its seams)                                          */
#define PDT_TIP_SYNC_ZERO_MAX_ERRORS 1u
typedef struct pdt_tip_sync_cfg {
    int32_t  max_errors;
    int32_t  window;
    int32_t  fly;
    uint32_t zero_mask;
} pdt_tip_sync_cfg;
typedef struct pdt_tip_sync_info {
    uint8_t  sync_errors;  /* dist_s(p) of the polarity that stands: wrong bits among the 19                                 */
    uint8_t  support;      /* u_s(p): neighbouring slots with a candidate                                                    */
    uint8_t  candidate;    /* 1 = the head's own sync word is within max_errors; 0 = a flywheel head                          */
    uint8_t  reserved;
} pdt_tip_sync_info;
int  pdt_tip_sync(pdt_ctx *ctx, const pdt_tip_sync_cfg *cfg, pdt_frame *out, pdt_tip_sync_info *info, int cap, int *count);
int  pdt_tip_sync_batch(pdt_ctx *const *ctxs, int count, const pdt_tip_sync_cfg *cfg, pdt_frame *out, pdt_tip_sync_info *info, int cap_each,
                        int *counts);
int  pdt_stage_tip_sync(pdt_ctx *ctx, const uint8_t *bits_host, uint64_t nbits, const pdt_tip_sync_cfg *cfg, pdt_frame *out,
                        pdt_tip_sync_info *info, int cap, int *count);
int  pdt_host_tip_sync(const uint8_t *bits, uint64_t nbits, const pdt_tip_sync_cfg *cfg, pdt_frame *out, pdt_tip_sync_info *info, int cap,
                       int *count);
int  pdt_tip_sync_tile(void);

/* ARGOS bits without a loop: feed-forward bit decisions per burst window (ARGOS contexts).  The bits above come out of the reference's
 * chain -- a PLL that must pull in, a squelch, a Gardner loop, a Manchester decoder that guesses the symbol pairing -- and a window whose
 * carrier lies at the edge of the loop's range, or whose pairing is never found, holds no message under either rule.  A burst needs no
 * loop: pdt_tones measures its carrier in the 160 ms it opens with, and the modulation is +-1.1 rad Manchester at 400 bit/s, so with
 * half-bit sums h0, h1 the sign of Im(h0 conj h1) is the bit, whatever the residual carrier.  These entries are a second, opt-in source
 * of bits BESIDE everything else; the rule is fixed in csrc/pdt_ff.h and pdt_host_ff_bits restates it on the host.  Of a
 * float32 I,Q stream at Fs -- 800 must divide Fs, H = Fs / 800 in 4 .. 128 -- the first L = min(n, 2 Fs) samples are used.  The carrier is
 * taken out with the down-converter's mixer at step = round(residual_hz 2^32 / Fs).  Hypothesis (r, tau), r = -R .. R, tau = 0 .. 2 H - 1:
 * half-bit k covers the samples [tau + b_k, tau + b_{k+1}), b_k = (k P_r + 32768) >> 16, P_r = llrint(H 65536 (1 + r ppm 1e-6)); it holds
 * K / 2 bits, K the largest even number with tau + b_K <= L.  s_k = the float sum over half-bit k (I and Q each, in ascending index),
 * d_m = Im(s_2m conj s_2m+1), the metric M(r, tau) = the uint64 sum of |d_m| 2^32 truncated (0 for a d_m that is not finite, 2^52 from
 * |d_m| = 2^20 on).  The winner is the largest M -- ties: the smaller |r|, then the smaller r, then the smaller tau -- and bit m is '1'
 * when d_m > 0, its soft value d_m, its sample index tau + b_{2m+2}.  tau spans both pairings and the message rule reads either polarity.
 * pdt_ff_cfg: NULL or a zero field = the default -- rate_steps R = 20 (allowed 0 .. 32; 0 with PDT_FF_ZERO_RATE_STEPS in zero_mask asks for
 * the nominal rate alone), rate_step_ppm 625 (R ppm 1e-6 may not exceed 0.1), and the residual MEASURED: the residual_hz of the first
 * segment of pdt_tones at that call's defaults (a context: its mode's search range; pdt_stage_ff_bits and pdt_host_ff_bits: pdt_host_tones'
 * defaults); a stream shorter than the segment, a rate without an allowed segment length or a record with valid = 0 gives residual 0 and
 * tone_valid 0.  PDT_FF_RESIDUAL_GIVEN in flags: residual_hz is the caller's (finite, |residual_hz| < Fs / 2) and tone_valid is 1.
 * pdt_ff_sync: residual_hz, tone_valid and step as used, the winner's tau, rate = r, period = P_r and metric = M, nbits = K / 2.
 *   pdt_ff_bits          the context's channel stream (PDT_ST_CHANNEL of its last whole-capture call): *sync = the record; the bits stay
 *                        on the device, in buffers of the context's own (not PDT_ST_BITS), for pdt_ff_read.  PDT_ERR_STATE as for
 *                        pdt_tones; PDT_ERR_ARG for a POES context, a sample rate or a cfg that is not allowed.  Like pdt_tones it leaves
 *                        frames, text, stages, statistics, survey, burst, tone and message results exactly as they were (a profiled
 *                        context's pdt_kernel_times gain the entries k_ff_mix, k_ff_search and k_ff_pick).  The tone record is the
 *                        call's one round trip to the host: its frequency is derived there, in double
 *   pdt_ff_bits_batch    the same for `count` contexts with ONE launch of each kernel (the windows of a round of pdt_demod_windows_*):
 *                        context i's record in syncs[i].  The contexts must be distinct, live on one device and have one sample rate
 *                        (else PDT_ERR_ARG); every one is checked before anything runs
 *   pdt_ff_read          the bits of the context's last pdt_ff_* or pdt_stage_ff_bits call: *count = their number, the first
 *                        min(cap, *count) characters, soft values and sample indices in bits, soft and index (each may be NULL), the
 *                        record in *sync (may be NULL).  PDT_ERR_STATE before such a call
 *   pdt_ff_messages      pdt_ff_bits, then the messages of pdt_argos_cfg's rule in those bits (pdt_argos_messages' kernels, unchanged, on
 *                        the device's own bit count): records as pdt_argos_messages gives them with time_src = the sample index of bit
 *                        bit_index and time = time_src / Fs, seconds of the channel stream.  sync may be NULL
 *   pdt_ff_messages_batch  the same for `count` contexts, ONE launch of each kernel: context i's records at out + i cap_each, their
 *                        number in counts[i], its record in syncs[i] (syncs may be NULL)
 *   pdt_stage_ff_bits    stage-level entry: the kernels on a caller's float32 I,Q stream of n samples at `rate` (the way in for a plain
 *                        recording of one burst); results through *sync and pdt_ff_read.  Nothing of the context's results changes
 *   pdt_host_ff_bits     host only, no GPU: the same record, bits, soft values and sample indices for the same stream
 *   pdt_host_ff_mix      host only: the stream v the rule sums, out = n pairs (every sample, not only the first L)                    */
#define PDT_FF_ZERO_RATE_STEPS 1u
#define PDT_FF_RESIDUAL_GIVEN  1u
typedef struct pdt_ff_cfg {
    int32_t  rate_steps;
    uint32_t zero_mask;
    double   rate_step_ppm;
    double   residual_hz;
    uint32_t flags;
    uint32_t reserved_;
} pdt_ff_cfg;
typedef struct pdt_ff_sync {
    double   residual_hz;
    int32_t  tone_valid;
    uint32_t step;
    int32_t  tau, rate;
    int64_t  period;
    uint64_t metric;
    uint64_t nbits;
} pdt_ff_sync;
int  pdt_ff_bits(pdt_ctx *ctx, const pdt_ff_cfg *cfg, pdt_ff_sync *sync);
int  pdt_ff_bits_batch(pdt_ctx *const *ctxs, int count, const pdt_ff_cfg *cfg, pdt_ff_sync *syncs);
int  pdt_ff_read(pdt_ctx *ctx, pdt_ff_sync *sync, uint8_t *bits, float *soft, int64_t *index, uint64_t cap, uint64_t *count);
int  pdt_ff_messages(pdt_ctx *ctx, const pdt_ff_cfg *cfg, const pdt_argos_cfg *rule, pdt_ff_sync *sync, pdt_argos_msg *out, int cap, int *count);
int  pdt_ff_messages_batch(pdt_ctx *const *ctxs, int count, const pdt_ff_cfg *cfg, const pdt_argos_cfg *rule, pdt_ff_sync *syncs,
                           pdt_argos_msg *out, int cap_each, int *counts);
int  pdt_stage_ff_bits(pdt_ctx *ctx, uint32_t rate, const float *iq_host, uint64_t n, const pdt_ff_cfg *cfg, pdt_ff_sync *sync);
int  pdt_host_ff_bits(uint32_t rate, const float *iq, uint64_t n, const pdt_ff_cfg *cfg, pdt_ff_sync *sync, uint8_t *bits, float *soft,
                      int64_t *index, uint64_t cap, uint64_t *count);
int  pdt_host_ff_mix(uint32_t rate, double residual_hz, const float *iq, uint64_t n, float *out);

/* POES bits without a loop: feed-forward carrier, clock and bit decisions on a whole stream (POES contexts).  The bits above
 * come out of the reference's chain -- a PLL that must pull in, an AGC, a Gardner loop, a Manchester decoder -- whose acquisition is a
 * serial walk, and weak passes lose frames before the flywheel (pdt_tip_sync) ever sees their bits.  A TIP signal needs no loop: it
 * carries a residual carrier all the time, the modulation is +-1.06 rad Manchester at 8320 bit/s, so the full-bit sum h0 + h1 of any
 * bit is a piece of bare carrier, the sum of these pieces over neighbouring bits is a phase reference, Im((h0 - h1) conj ref) is the
 * bit's soft value, and the bit clock is found block by block by exhaustive search.  These entries are a second, opt-in source of bits --
 * and, through the flywheel's unchanged kernels, of minor frames -- BESIDE everything else; the rule is fixed in csrc/pdt_ffp.h and
 * pdt_host_ffp_bits restates it on the host:
 *   input     a float32 I,Q stream y of n samples at Fs, n < 2^36; the half-bit lasts P = Fs / 16640 samples, 3 <= P <= 64: 49920 <= Fs <=
 *             1064960.  cfg: B bits per block (208; 64 .. 832), T clock hypotheses (32; 8 .. 64), W bits of reference either side (16;
 *             0 .. 64), J blocks of smoothing either side (4; 0 .. 16)
 *   time grid every point of the time axis is an integer in Q16, 1 / 65536 sample, int64.  The nominal start of half-bit k is
 *             t_k = (k Fs 65536) / 16640, rounded down (= (k Fs 256) / 65); the offset of clock phase f (any integer, in steps of 1 / T bit)
 *             is o(f) = (f 2 Fs 65536) / (16640 T), rounded down (towards minus infinity for a negative f).  Under f, bit m >= 0 covers
 *             [t_2m + o, t_2m+2 + o), its half-bits meet at t_2m+1 + o.  A bit EXISTS under f when t_2m + o >= 0 and t_2m+2 + o <= n 65536
 *   carrier   measured (the default): pdt_tones' arithmetic (k_tones, tone_derive, unchanged) over the segments of nfft samples at stride
 *             nfft from sample 0, nfft and the search set that call's defaults; residual_j = the record's residual_hz, derived on the
 *             host in double (the call's one round trip).  step_j = ddc_step(Fs, residual_j); a segment with valid = 0 takes the step of
 *             the nearest earlier valid one, or 0 when there is none; the tail behind the last whole segment takes the last segment's
 *             step; a stream without a whole segment, or a rate without an allowed nfft, has step 0 throughout.  Given
 *             (PDT_FFP_RESIDUAL_GIVEN): one step = ddc_step(Fs, residual_hz) for the whole stream.  The mixer's phase is continuous:
 *             the start phase of segment j is the uint32 wrap-around sum of step_i nfft over the earlier segments, sample i of segment
 *             j (the tail counts to the last segment) has phase(i) = start_j + (i - j nfft) step_j mod 2^32
 *   v[i]      = ddc_mix(y[i], phase(i)) with the down-converter's table; v = 0 outside [0, n)
 *   sums      the sum over a Q16 interval [a, b), a < b, is the fma chain s = fmaf(v[i], w_i, s) from +0 in ascending i, I and Q each,
 *             over the samples i = a >> 16 .. (b - 1) >> 16, w_i = the part of [i, i + 1) inside [a, b) as a float, frac / 65536
 *             (exact; a sample wholly inside has w = 1)
 *   bit       h0, h1 = the sums of its two half-bits; c = h0 + h1 and e = h0 - h1, component by component
 *   ref_m     under f: the float addition chain from +0 of c over the bits m - W .. m + W that exist under f, in ascending order
 *   d_m       = fmaf(e.im, ref.re, -(e.re ref.im)), the product rounded first: Im(e conj ref)
 *   q(d)      pdt_ff_bits': 0 when d is not finite, 2^52 when |d| >= 2^20, else (uint64)(|d| 2^32), truncated
 *   blocks    L = (2 B Fs + 8320) / 16640 samples, B nominal bits rounded to the nearest sample; block b covers the samples [b L, (b + 1) L),
 *             nb = ceil(n / L) of them.  M(b, tau), tau = 0 .. T - 1: the uint64 sum of q(d_m) over the bits that exist under tau and
 *             start inside block b
 *   smoothing Ms(b, tau) = the sum of M(b + j, tau) over |j| <= J, blocks outside the stream left out; tau_b = the arg-max of Ms(b, .),
 *             ties to the smaller tau
 *   unwrap    phi_0 = tau_0; phi_b = phi_{b-1} + delta_b, delta_b = (tau_b - tau_{b-1}) mod T folded into (-T / 2, T / 2] (2 delta > T:
 *             delta - T).  A drifting recorder clock lets phi run on; the bit index m stays the index of one physical bit
 *   ownership m_lo(b) = the smallest m >= 0 whose start under phi_b is >= b L 65536; m_end(b) = the largest m that exists under phi_b (-1
 *             when none).  Block b decides the bits m_lo(b) <= m < m_hi(b), all of them under phi_b: m_hi(b) = min(m_lo(b + 1), m_end(b)
 *             + 1) (the last block: m_end(b) + 1); its count is max(0, m_hi - m_lo).  Output positions are the exclusive scan of the counts
 *   decision  bit '1' when d_m > 0, else '0'; the soft value is d_m (every NaN as the quiet NaN 0x7fc00000); the time source is the
 *             sample index at which the bit ends, (t_2m+2 + o + 65535) >> 16
 * The carrier reference is absolute, so there is no pairing or polarity guess; a mirrored spectrum complements the bits and the
 * flywheel reads either polarity.  A jump of phi in a stretch of noise costs a bit slip there; slips are the flywheel's business.
 * pdt_ffp_cfg: NULL or a zero field = the default; ref_bits 0 with PDT_FFP_ZERO_REF_BITS and smooth_blocks 0 with PDT_FFP_ZERO_SMOOTH in
 * zero_mask are real zeros.  PDT_FFP_RESIDUAL_GIVEN in flags: residual_hz is the caller's (finite, |residual_hz| < Fs / 2).
 * pdt_ffp_sync: residual_hz and step = the caller's, or those of the first valid segment (0 when there is none); nfft = the segments' length
 * (0 when the residual was given), segs and segs_valid = the tone segments measured and how many were valid; nblocks, nbits, block_len = L,
 * and B, T, W, J as used.  pdt_ffp_block: block b's tau_b, phi_b, first_bit = m_lo(b), count and metric = Ms(b, tau_b).
 *   pdt_ffp_bits         the context's channel stream (PDT_ST_CHANNEL of its last whole-capture call): *sync = the record; the bits stay
 *                        on the device, in buffers of the context's own (not PDT_ST_BITS), for pdt_ffp_read.  PDT_ERR_STATE as for
 *                        pdt_tones; PDT_ERR_ARG for an ARGOS context, a sample rate or a cfg that is not allowed.  Like pdt_tones it leaves
 *                        frames, text, stages, statistics, survey, burst, tone and flywheel results exactly as they were (a profiled
 *                        context's pdt_kernel_times gain the entries k_ffp_mix, k_ffp_search, k_ffp_track and k_ffp_bits).  The tone
 *                        records are the call's one round trip to the host: the frequencies are derived there, in double
 *   pdt_ffp_read         the bits of the context's last pdt_ffp_* or pdt_stage_ffp_* call: *count = their number, the first
 *                        min(cap, *count) characters, soft values and sample indices in bits, soft and index (each may be NULL), the
 *                        record in *sync (may be NULL).  PDT_ERR_STATE before such a call
 *   pdt_ffp_blocks       the per-block table of that call: *count = the number of blocks, the first min(cap, *count) records in out
 *   pdt_ffp_frames       pdt_ffp_bits, then the minor frames of pdt_tip_sync_cfg's rule in those bits (pdt_tip_sync's kernels, unchanged,
 *                        on the device's own bit count): records as pdt_tip_sync gives them with time_src = the sample index at which
 *                        bit bit_index ends and time = time_src / Fs -- seconds of the stream, NOT the reference's running sum of
 *                        symbol periods.  sync and info may be NULL.  max_errors 0, window 1 and fly 2 is as strict as the rule gets
 *   pdt_stage_ffp_bits   stage-level entry: the kernels on a caller's float32 I,Q stream of n samples at `rate` (the way in for a plain
 *                        recording); results through *sync, pdt_ffp_read and pdt_ffp_blocks.  The whole stream is resident on the
 *                        device (PDT_ERR_NOMEM otherwise).  Nothing of the context's results changes
 *   pdt_stage_ffp_frames the same, then the frames as pdt_ffp_frames gives them
 *   pdt_host_ffp_bits    host only, no GPU: the same record, bits, soft values, sample indices and per-block table for the same stream,
 *                        written from the rule's text (blocks may be NULL)
 *   pdt_host_ffp_mix     host only: the stream v the rule sums, out = n pairs                                                          */
#define PDT_FFP_ZERO_REF_BITS  1u
#define PDT_FFP_ZERO_SMOOTH    2u
#define PDT_FFP_RESIDUAL_GIVEN 1u
typedef struct pdt_ffp_cfg {
    int32_t  block_bits;      /* B */
    int32_t  clock_steps;     /* T */
    int32_t  ref_bits;        /* W */
    int32_t  smooth_blocks;   /* J */
    uint32_t zero_mask;
    uint32_t flags;
    double   residual_hz;
} pdt_ffp_cfg;
typedef struct pdt_ffp_sync {
    double   residual_hz;
    uint32_t step;
    int32_t  nfft;
    uint64_t segs, segs_valid;
    uint64_t nblocks, nbits;
    int64_t  block_len;
    int32_t  block_bits, clock_steps, ref_bits, smooth_blocks;
} pdt_ffp_sync;
typedef struct pdt_ffp_block {
    int64_t  phi;
    int64_t  first_bit;
    uint64_t count;
    uint64_t metric;
    int32_t  tau;
    int32_t  reserved_;
} pdt_ffp_block;
int  pdt_ffp_bits(pdt_ctx *ctx, const pdt_ffp_cfg *cfg, pdt_ffp_sync *sync);
int  pdt_ffp_read(pdt_ctx *ctx, pdt_ffp_sync *sync, uint8_t *bits, float *soft, int64_t *index, uint64_t cap, uint64_t *count);
int  pdt_ffp_blocks(pdt_ctx *ctx, pdt_ffp_block *out, uint64_t cap, uint64_t *count);
int  pdt_ffp_frames(pdt_ctx *ctx, const pdt_ffp_cfg *cfg, const pdt_tip_sync_cfg *tip_cfg, pdt_ffp_sync *sync, pdt_frame *out,
                    pdt_tip_sync_info *info, int cap, int *count);
int  pdt_stage_ffp_bits(pdt_ctx *ctx, uint32_t rate, const float *iq_host, uint64_t n, const pdt_ffp_cfg *cfg, pdt_ffp_sync *sync);
int  pdt_stage_ffp_frames(pdt_ctx *ctx, uint32_t rate, const float *iq_host, uint64_t n, const pdt_ffp_cfg *cfg, const pdt_tip_sync_cfg *tip_cfg,
                          pdt_ffp_sync *sync, pdt_frame *out, pdt_tip_sync_info *info, int cap, int *count);
int  pdt_host_ffp_bits(uint32_t rate, const float *iq, uint64_t n, const pdt_ffp_cfg *cfg, pdt_ffp_sync *sync, uint8_t *bits, float *soft,
                       int64_t *index, uint64_t cap, uint64_t *count, pdt_ffp_block *blocks, uint64_t block_cap);
int  pdt_host_ffp_mix(uint32_t rate, const float *iq, uint64_t n, const pdt_ffp_cfg *cfg, float *out);

/* POES frames: repair of failed parity groups from the soft bit values (POES contexts).  The flywheel places the minor frames
 * of a weak pass; what it hands out are hard decisions, and pdt_tip_check only REPORTS the five even-parity groups of a frame.  Where a
 * group's parity is odd, complementing its least reliable bit (Wagner's rule for a single-parity code) is the most likely correction.
 * These entries are opt-in and stand BESIDE everything else; the rule is fixed in csrc/pdt_tip_repair.h and pdt_host_tip_repair restates
 * it on the host:
 *   input     pdt_frame records as pdt_tip_sync / pdt_ffp_frames give them, and a stream of n float32 soft values: value k belongs to
 *             bit k of the stream the records were found in (pdt_ffp_read's soft)
 *   CHECKED   a record is checked <=> complete == 1 and nbytes == 104 and 18 <= bit_index and bit_index + 813 < n.  Any other record is
 *             left as it is and marked skipped
 *   BITS      frame bit j, 0 <= j < 832, is bit 7 - (j & 7) of bytes[j >> 3]; its soft value is soft[bit_index - 18 + j]
 *   GROUPS    pdt_tip_check's, unchanged: group g = 0 .. 4 covers frame bits 16 + 136 g .. 151 + 136 g (bytes 2 + 17 g .. 18 + 17 g) and
 *             its parity bit, frame bit 826 + g (bit 5 - g of bytes[103]).  The group FAILS when the number of ones among these 137 bits
 *             OF THE RECORD is odd; the record of an inverted head is already complemented back, so polarity plays no part
 *   CANDIDATE the group's bits that came from the stream.  In group 0 frame bits 16, 17 and 18 are the sync word's last three bits, which
 *             the flywheel writes as zeros: they count toward the parity but are never candidates -- 134 candidates in group 0, 137 in
 *             the others
 *   r(k)      the uint32 bit pattern of |soft[k]|: a NaN counts as 0, -0 as 0, Inf sorts above every finite value
 *   KEY       of the candidate at frame bit j: (uint64) r << 16 | j
 *   REPAIR    in a failing group the candidate with the smallest key is complemented in the record: ties go to the earlier bit, a data
 *             bit goes before the parity bit.  Nothing else changes -- not time, bit_index, time_src, inverted or bytes 0 - 1
 *   INFO      per record: status (1 checked, 0 skipped); failed, bit g set where group g failed BEFORE the repair; pos[g] = the frame bit
 *             complemented in group g, or 0xFFFF; least[g] and next[g] = the floats whose bit patterns are the r of the smallest and the
 *             second smallest key of group g, filled whether or not the group failed (a repair is judged by its margin).  A skipped
 *             record: failed 0, pos 0xFFFF, least and next 0
 *   SUMMARY   records checked, records skipped, records with a failing group, groups repaired
 * After the repair every group of a checked record passes BY CONSTRUCTION: -q and pdt_tip_check_records on repaired records say nothing,
 * and `failed` is the parity record to keep.  A group with two wrong bits passes as it is, one with three is made worse: the rule helps
 * while single errors dominate -- at 9 x the noise of the weak capture it turns most damaged frames right, at 12 x it does not help
 * (DESIGN 4.20's table).  The 131 bits of bytes 87 - 103 that no group covers are never touched.
 *   pdt_tip_repair        the caller's records (uploaded to a buffer of their own, as pdt_tip_check_records uploads its) against the soft
 *                         values of the context's last pdt_ffp_* / pdt_stage_ffp_* call, which are still in device memory, on the
 *                         device's own bit count: frames[0 .. n) repaired in place, info[0 .. n) (may be NULL) and *summary filled.
 *                         PDT_ERR_STATE when no such call left bits, or a stream is open; PDT_ERR_ARG for an ARGOS context, a null
 *                         pointer with n > 0, a null summary, or n >= 2^31.  No other result of the context changes (a profiled context's
 *                         pdt_kernel_times gain the entry k_tip_repair)
 *   pdt_stage_tip_repair  stage-level entry: the kernel on a caller's nbits soft values from any source (nbits < 2^31, else PDT_ERR_ARG).
 *                         Nothing of the context's results changes, the feed-forward bits included
 *   pdt_host_tip_repair   host only, no GPU: the same bytes in frames, info and summary                                                */
#define PDT_TIP_REPAIR_NONE 0xFFFFu
typedef struct pdt_tip_repair_info {
    uint8_t  status;       /* 1 = checked, 0 = skipped                                                                       */
    uint8_t  failed;       /* bit g set = group g failed before the repair: the parity record to keep                        */
    uint16_t pos[5];       /* the frame bit complemented in group g, PDT_TIP_REPAIR_NONE when the group passed                */
    float    least[5];     /* the smallest |soft| among group g's candidates ...                                             */
    float    next[5];      /* ... and the second smallest: the margin of a repair                                            */
} pdt_tip_repair_info;
typedef struct pdt_tip_repair_summary {
    uint64_t checked;      /* records checked                                                                                */
    uint64_t skipped;      /* records left as they were                                                                      */
    uint64_t failing;      /* checked records with at least one failing group                                                */
    uint64_t repaired;     /* groups repaired = bits complemented                                                            */
} pdt_tip_repair_summary;
int  pdt_tip_repair(pdt_ctx *ctx, pdt_frame *frames, uint64_t n, pdt_tip_repair_info *info, pdt_tip_repair_summary *summary);
int  pdt_stage_tip_repair(pdt_ctx *ctx, const float *soft_host, uint64_t nbits, pdt_frame *frames, uint64_t n, pdt_tip_repair_info *info,
                          pdt_tip_repair_summary *summary);
int  pdt_host_tip_repair(const float *soft, uint64_t nbits, pdt_frame *frames, uint64_t n, pdt_tip_repair_info *info,
                         pdt_tip_repair_summary *summary);

/* POES frames: the DCS-2 platform messages they relay (POES contexts).  The satellite receives the ARGOS platforms on
 * 401.65 MHz and relays each message -- platform ID, sensor data, its own time code, the measured Doppler word -- in 32 bytes of every TIP
 * minor frame (standalone_matlab/Functionized/POES.m:868-1311).  These entries are opt-in and stand BESIDE everything else; the rule is
 * fixed in csrc/pdt_tip_dcs.h and pdt_host_tip_dcs restates it on the host:
 *   input     pdt_frame records from any source, repaired or not.  A record is ELIGIBLE <=> complete == 1 and nbytes == 104; `inverted`
 *             plays no part
 *   SLOTS     the DCS bytes of a frame are bytes[b] for b = 18 19 24 25 28 29 32 33 40 41 44 45 52 53 56 57 60 61 64 65 68 69 72 73 76 77
 *             86 87 90 91 94 95 (POES.m:869-932, 0-based here): 32 slots; the time of slot byte b is time + b * (0.1 / 104) (POES.m:257)
 *   SEGMENTS  record i+1 continues record i <=> both are eligible and bit_index[i+1] - bit_index[i] == 832.  A segment is a maximal run of
 *             such records, its stream S the concatenation of their slots.  An ineligible record belongs to no segment and is counted as
 *             skipped.  Nothing is joined across a gap (the reference concatenates whatever frames it has)
 *   HEAD      position k of a segment is a head <=> k + 2 lies inside the segment, S[k] == 0xD6, S[k+1] < channel_max (0 means 8; the
 *             reference uses 9 for NOAA-19, POES.m:942-946; 1 .. 16) and the high nibble c of S[k+2] is a valid length code: with
 *             n1 = c >> 1, (c & 1) == ((n1 >> 2) ^ (n1 >> 1) ^ n1) & 1 -- the codes 0 3 5 6 9 A C F of POES.m:1195-1214.  Then
 *             blocks = n1 + 1 and L = 12 + 4 blocks.  A D6 with a good channel byte and an invalid code is counted (bad_code) and is no
 *             head (the reference takes 44 bytes).  A D6 that is a segment's first byte is a head like any other (the reference never sees
 *             the stream's first byte)
 *   ACCEPTED  within a segment, in ascending order, a head is accepted <=> k >= the end k' + L' of the previously accepted one; any other
 *             head is SHADOWED and counted (the reference cuts a packet wherever a data byte pair looks like a head)
 *   PACKET    of an accepted head: nbytes = min(L, segment_len - k), complete = (nbytes == L), bytes[0 .. nbytes) from the stream, the rest
 *             zero; channel = S[k+1]; time_code = (S[k+3] & 31) << 16 | S[k+4] << 8 | S[k+5] (nbytes >= 6, else 0); id = big-endian
 *             S[k+6 .. k+9] (nbytes >= 10, else 0; the reference's TXID, POES.m:1184); when complete, w = the last three bytes, big-endian,
 *             doppler_ok = 1 when w has an even number of ones, doppler_raw = (int32)(w >> 1) - (1 << 22) (the reference prints
 *             doppler_raw / 32.0, POES.m:1261-1271), both 0 otherwise; frame and slot = the record and the slot 0 .. 31 that hold the D6;
 *             stream_index = that byte's position when every eligible record's slots are counted in record order; time = the time of the
 *             D6 byte ITSELF (the reference stamps a packet with the time of the byte in front of its D6)
 *   SUMMARY   totals over the call: records used, records skipped, segments, stream bytes, heads, shadowed, bad_code, packets, complete,
 *             doppler_bad (complete packets whose Doppler word has odd parity)
 * Packets come out in ascending record order.  *count = the packets found; at most cap are written (cap = 0 with out = NULL only counts);
 * the summary is always complete.
 *   pdt_tip_dcs             the frames of the context's last pdt_demod_* call, which are still in device memory (as pdt_tip_check).
 *                           PDT_ERR_STATE when nothing has been demodulated or a stream is open; PDT_ERR_ARG for an ARGOS context, a null
 *                           count or summary, cap < 0, a null out with cap > 0, channel_max > 16.  No other result of the context changes (a
 *                           profiled context's pdt_kernel_times gain the entries k_dcs_gather, k_dcs_maps, k_dcs_scan and k_dcs_pack)
 *   pdt_tip_dcs_records     a caller's records (uploaded to a buffer of their own, as pdt_tip_check_records uploads its); n >= 2^31 or a
 *                           null pointer with n > 0: PDT_ERR_ARG
 *   pdt_host_tip_dcs        host only, no GPU: the same packets and summary, `time` included, bit for bit
 *   pdt_tip_dcs_tile        the stream bytes one tile covers (tests place packets at its seams)
 *   pdt_format_dcs_packets  the packets' text; returns the bytes needed, writes at most cap.  One line per packet:
 *                             "%.5f %u %u %07u %08X %s " (time, channel, blocks, time_code, id, Doppler), "%02X " per byte, "\n"
 *                           where the Doppler is "%.5f" of doppler_raw / 32.0 for a complete packet with even parity, the same behind a '*'
 *                           when the parity is odd, and "-" for a packet that is cut off
 *   pdt_write_dcs_packets   the same text to a file descriptor; PDT_ERR_IO when a write fails                                            */
typedef struct pdt_dcs_cfg {
    uint32_t channel_max;  /* the channel byte's bound, 1 .. 16; 0 = 8                                                       */
    uint32_t reserved;
} pdt_dcs_cfg;             /* NULL or zeroed = default                                                                       */
typedef struct pdt_dcs_packet {
    double   time;         /* of the D6 byte                                                                                 */
    int64_t  stream_index; /* of the D6 byte, over the slots of every eligible record                                        */
    uint32_t frame;        /* the record that holds the D6                                                                   */
    uint32_t time_code, id;
    int32_t  doppler_raw;
    uint8_t  slot, channel, blocks, nbytes, complete, doppler_ok, pad[2];
    uint8_t  bytes[44];
} pdt_dcs_packet;
typedef struct pdt_dcs_summary {
    uint64_t used, skipped, segments, stream_bytes, heads, shadowed, bad_code, packets, complete, doppler_bad;
} pdt_dcs_summary;
int      pdt_tip_dcs(pdt_ctx *ctx, const pdt_dcs_cfg *cfg, pdt_dcs_packet *out, int cap, int *count, pdt_dcs_summary *summary);
int      pdt_tip_dcs_records(pdt_ctx *ctx, const pdt_frame *frames, uint64_t n, const pdt_dcs_cfg *cfg, pdt_dcs_packet *out, int cap, int *count,
                             pdt_dcs_summary *summary);
int      pdt_host_tip_dcs(const pdt_frame *frames, uint64_t n, const pdt_dcs_cfg *cfg, pdt_dcs_packet *out, int cap, int *count,
                          pdt_dcs_summary *summary);
uint64_t pdt_format_dcs_packets(const pdt_dcs_packet *packets, uint64_t n, char *buf, uint64_t cap);
int      pdt_write_dcs_packets(const pdt_dcs_packet *packets, uint64_t n, int fd, uint64_t *bytes_written);
int      pdt_tip_dcs_tile(void);

/* POES frames: the subcommutated bytes (POES contexts).  A fixed byte of the minor frame belongs to a different measurement
 * depending on the frame's 9-bit minor-frame counter: SEM-2, the space environment monitor, reads out 22 MEPED and 38 TED channels through
 * bytes 20 and 21 (standalone_matlab/Functionized/POES.m:1314-1700), the 16-second analogue housekeeping points use bytes 11 and 14
 * (POES.m:462-513).  One table-driven rule covers them; both tables are built in and any other is the caller's.  These entries are opt-in
 * and stand BESIDE everything else; the rule is fixed in csrc/pdt_tip_subcom.h and pdt_host_tip_subcom restates it on the host:
 *   input     pdt_frame records from any source, repaired or not.  A record is ELIGIBLE <=> complete == 1 and nbytes == 104.  Its
 *             counter is id = (bytes[4] & 1) << 8 | bytes[5].  An eligible record with id >= 320 is counted bad_id and yields nothing; an
 *             ineligible record is counted skipped; every other record is used
 *   TABLE     1 .. 256 entries {channel, byte, period, phase, mask, shift, invert}: channel < 128, byte 0 .. 103, period divides 320,
 *             phase < period, mask != 0, shift 0 .. 7, invert 0 or 1; any other table: PDT_ERR_ARG.  Entries need not be sorted; nchan =
 *             the largest channel + 1, empty channels are allowed
 *   FIRES     an entry fires in a used record <=> id % period == phase.  raw = bytes[byte], value = ((invert ? 255 - raw : raw) & mask) >> shift
 *   SAMPLE    every firing is a sample: time = the frame byte's own, record's time + byte * (0.1 / 104); frame = the record's index;
 *             minor_id = id; channel; entry = the entry's index; value; raw; flags:
 *               PDT_SUBCOM_BYTE_PARITY (1)  the even-parity group that covers `byte` fails (pdt_tip_check's groups: group g = 0 .. 4 covers
 *                                           bytes 2 + 17 g .. 18 + 17 g against bit 5 - g of byte 103)
 *               PDT_SUBCOM_ID_PARITY   (2)  group 0 fails: it covers bytes 4 and 5, so the counter that chose the channel is in doubt
 *               PDT_SUBCOM_UNCOVERED   (4)  `byte` lies in no group (0, 1, 87 .. 103)
 *               PDT_SUBCOM_SPIKE       (8)  see below
 *             With cfg.trusted_only a sample with bit 1 or bit 2 set is counted `dropped` and does not exist for anything that follows:
 *             not for the order, the spike test or the counts samples, byte_parity, id_parity (both 0 then) and channels_hit
 *   ORDER     channel-major: channel 0's samples, then channel 1's ...; within a channel ascending by (record, entry index).
 *             offsets[0 .. nchan] (nchan + 1 values; NULL: not wanted) gives each channel's place and is always complete, whatever cap is
 *   SPIKE     sample j of a channel is a spike <=> both neighbours j - 1 and j + 1 lie in the same channel and |v[j-1] - v[j]| > thr and
 *             |v[j+1] - v[j]| > thr, on the values as decoded; thr = cfg.spike_threshold, 0 means 20 (the reference's FilterThreshold),
 *             above 255: PDT_ERR_ARG
 *   SUMMARY   used, skipped, bad_id, samples, dropped, byte_parity, id_parity, spikes, channels_hit (channels with a sample)
 * Three departures from POES.m:1379-1490: the reference zeroes a spike in place, so its test of the next sample sees the zero -- a
 * sequential dependence, and a lost value --, here a spike is flagged and keeps its value; the reference's series start with a dummy 0
 * (X(1) = 0), here a channel's first and last sample never spike; neighbours are neighbours in the series whatever gap lies between them,
 * as in the reference.
 * *count = the samples found; at most cap are written, the first cap of the order above (cap = 0 with out = NULL only counts); the summary
 * and offsets are always complete.  A call whose records could give 2^31 samples or more (n times the most entries that fire in one
 * record): PDT_ERR_ARG.
 *   pdt_tip_subcom          the frames of the context's last pdt_demod_* call, which are still in device memory (as pdt_tip_dcs).
 *                           PDT_ERR_STATE when nothing has been demodulated or a stream is open; PDT_ERR_ARG for an ARGOS context, a table
 *                           or cfg that is not allowed, a null count or summary, cap < 0, a null out with cap > 0.  No other result of the
 *                           context changes (a profiled context's pdt_kernel_times gain the entries k_subcom_mark, k_subcom_count,
 *                           k_subcom_scan, k_subcom_place and k_subcom_spikes)
 *   pdt_tip_subcom_records  a caller's records (uploaded to a buffer of their own); n >= 2^31 or a null pointer with n > 0: PDT_ERR_ARG
 *   pdt_host_tip_subcom     host only, no GPU: the same samples, offsets and summary, `time` included, bit for bit
 *   pdt_subcom_table        a built-in table: returns its number of entries (0: there is no such table), writes at most cap.
 *                           PDT_SUBCOM_SEM: 76 entries, 60 channels, bytes 20 and 21, every entry inverted (the data is sent complemented,
 *                           POES.m:1317-1318) -- MEPED 0P1 .. 0P6 0E1 .. 0E3 9P1 .. 9P6 9E1 .. 9E3 P6 .. P9 (POES.m:1340-1377), TED 0EFL 3EFL
 *                           0PFL 3PFL 0EFH 3EFH 0PFH 3PFH 0EM 0PM 0DEM 0DPM 3EM 3PM 3DEM 3DPM 0DE1 0DE2 3DE1 3DE2 0DP1 0DP2 3DP1 3DP2 0EBKL
 *                           0EBKH 3PBKL 0DE3 0DE4 3DE3 3DE4 0DP3 0DP4 3DP3 3DP4 0PBKL 0PBKH 3PBKH (POES.m:1561-1621), channels numbered in
 *                           this order.  PDT_SUBCOM_HK: 5 entries, not inverted -- byte 11 every 80 frames: STX1 at 48, STX2 at 50, STX3 at
 *                           40; byte 14 every 160: SARR-A at 114, SARR-B at 2 (POES.m:492-508; line 506 names the wrong array, the counter
 *                           is the same)
 *   pdt_subcom_name         a built-in table's name of a channel, or NULL
 *   pdt_tip_subcom_tile     the records one tile of the kernels covers (tests place samples at its seams)
 *   pdt_format_subcom       the samples' text; returns the bytes needed, writes at most cap.  One line per sample, "%.5f %s %u %u %s\n":
 *                           the time, the channel's name in table `which` (c<channel> where that has none: PDT_SUBCOM_CUSTOM), the
 *                           counter, the value and the flags as a subset of the letters b i u s in that order, or "-"
 *   pdt_write_subcom        the same text to a file descriptor; PDT_ERR_IO when a write fails                                           */
#define PDT_SUBCOM_BYTE_PARITY 1
#define PDT_SUBCOM_ID_PARITY 2
#define PDT_SUBCOM_UNCOVERED 4
#define PDT_SUBCOM_SPIKE 8
#define PDT_SUBCOM_SEM 0
#define PDT_SUBCOM_HK 1
#define PDT_SUBCOM_CUSTOM (-1)
typedef struct pdt_subcom_entry {
    uint8_t  channel;      /* < 128                                                                                          */
    uint8_t  byte;         /* of the frame, 0 .. 103                                                                         */
    uint16_t period;       /* divides 320                                                                                    */
    uint16_t phase;        /* < period: the entry fires when id % period == phase                                            */
    uint8_t  mask, shift;  /* value = ((invert ? 255 - raw : raw) & mask) >> shift                                           */
    uint8_t  invert, pad;
} pdt_subcom_entry;
typedef struct pdt_subcom_cfg {
    uint32_t trusted_only;    /* nonzero: samples whose byte's or whose counter's parity group fails are dropped             */
    uint32_t spike_threshold; /* 1 .. 255; 0 = 20                                                                            */
} pdt_subcom_cfg;             /* NULL or zeroed = default                                                                    */
typedef struct pdt_subcom_sample {
    double   time;         /* of the frame byte                                                                              */
    uint32_t frame;        /* the record                                                                                     */
    uint16_t minor_id;
    uint8_t  channel, entry, value, raw, flags, pad[5];
} pdt_subcom_sample;
typedef struct pdt_subcom_summary {
    uint64_t used, skipped, bad_id, samples, dropped, byte_parity, id_parity, spikes, channels_hit;
} pdt_subcom_summary;
int      pdt_tip_subcom(pdt_ctx *ctx, const pdt_subcom_entry *entries, uint64_t nentries, const pdt_subcom_cfg *cfg, pdt_subcom_sample *out, int cap,
                        int *count, uint64_t *offsets, pdt_subcom_summary *summary);
int      pdt_tip_subcom_records(pdt_ctx *ctx, const pdt_frame *frames, uint64_t n, const pdt_subcom_entry *entries, uint64_t nentries,
                                const pdt_subcom_cfg *cfg, pdt_subcom_sample *out, int cap, int *count, uint64_t *offsets, pdt_subcom_summary *summary);
int      pdt_host_tip_subcom(const pdt_frame *frames, uint64_t n, const pdt_subcom_entry *entries, uint64_t nentries, const pdt_subcom_cfg *cfg,
                             pdt_subcom_sample *out, int cap, int *count, uint64_t *offsets, pdt_subcom_summary *summary);
int      pdt_subcom_table(int which, pdt_subcom_entry *entries, int cap);
const char *pdt_subcom_name(int which, int channel);
int      pdt_tip_subcom_tile(void);
uint64_t pdt_format_subcom(const pdt_subcom_sample *samples, uint64_t n, int which, char *buf, uint64_t cap);
int      pdt_write_subcom(const pdt_subcom_sample *samples, uint64_t n, int which, int fd, uint64_t *bytes_written);

/* Results of the last pdt_demod_* call. */
uint64_t pdt_num_frames(const pdt_ctx *ctx);
uint64_t pdt_frames(const pdt_ctx *ctx, pdt_frame *out, uint64_t max_frames);
int      pdt_get_stats(const pdt_ctx *ctx, pdt_stats *out);
/* Text exactly as the reference writes it to minorFrames_*.txt / packets_*.txt.
 * Returns the number of bytes needed; writes at most `cap` bytes.                               */
uint64_t pdt_format_frames(const pdt_ctx *ctx, char *buf, uint64_t cap);
/* The same text for any array of frame records (e.g. the records of several captures gathered on one rank); host only, no
 * context and no GPU needed.  POESTIPdemod/ByteSync.c:62-69,96-101, ARGOSdemod/ByteSync.c:62-70,99-103.                 */
uint64_t pdt_format_records(const pdt_frame *frames, uint64_t nframes, char *buf, uint64_t cap);
/* The same text written to an open file descriptor, from the descriptor's position on (the reference's fprintf calls,
 * ByteSync.c:62-101, all at once): slices of the frames are formatted and written side by side (pwrite) when the
 * descriptor can seek, in order otherwise; the position ends behind the text.  *bytes_written may be NULL.
 * PDT_ERR_IO when a write fails.  (ABI 2)                                                                         */
int      pdt_write_frames(const pdt_ctx *ctx, int fd, uint64_t *bytes_written);
int      pdt_write_records(const pdt_frame *frames, uint64_t nframes, int fd, uint64_t *bytes_written);

/* Copy an intermediate stream back to the host (elements [first, first+count)); returns the
 * number of elements copied, or a negative error.  Element type per the PDT_ST_* table;
 * DT = float (POES) / double (ARGOS).                                                           */
int64_t  pdt_read_stage(const pdt_ctx *ctx, int stage, uint64_t first, uint64_t count, void *out);
uint64_t pdt_stage_len(const pdt_ctx *ctx, int stage);

/* Stage-level entry: run only the sync-word search + frame extraction kernels
 * (ByteSyncOnSyncword, POESTIPdemod/ByteSync.c:16-150 / FindSyncWords, ARGOSdemod/ByteSync.c:17-150)
 * on a string of '0'/'1' characters; the time stamp of bit k is k.  Results through pdt_frames /
 * pdt_format_frames.  (The reference ships exactly such a bit-string harness, commented out, at
 * POESTIPdemod/ByteSync.c:6-14.)                                                                  */
int      pdt_stage_bytesync(pdt_ctx *ctx, const uint8_t *bits_host, uint64_t nbits);
/* The same when the string continues an earlier one (the synchronisers keep their last bits and an open frame in statics
 * between calls, ByteSync.c:18-22): no sync word may COMPLETE before bit first_sync_end -- one that ends inside the bits the
 * caller kept from the previous call was seen there, with the real bits in front of it instead of the zeros the ring starts
 * with.  pdt_compat.c continues the reference's call-by-call state with this.                                            */
int      pdt_stage_bytesync_from(pdt_ctx *ctx, const uint8_t *bits_host, uint64_t nbits, uint64_t first_sync_end);

/* More stage-level entries: one stage of the chain on caller data in host memory (DT = float for POES
 * contexts, double for ARGOS), through the kernels the whole-capture path uses, with the reference function's hidden
 * `static` variables as an explicit state record the caller keeps -- so that per-chunk dumps of the reference can be
 * replayed stage by stage, chunk after chunk.  state == NULL: a fresh stage, nothing carried out.  A zeroed record is the
 * reference's state before its first call.                                                                           */
typedef struct pdt_manchester_state {   /* ManchesterDecode.c:16-20 */
    double   current, previous;         /* currentSample, prevSample after the last call (exact for float and double)  */
    uint32_t clockmod;                  /* which symbol parity ends a bit                                              */
    uint32_t even_odd;                  /* evenOddCounter (an unsigned char there: counted modulo 256)                 */
} pdt_manchester_state;
/* unsigned long ManchesterDecode(DT *dataStreamIn, DT *dataStreamTime, unsigned long nSymbols, unsigned char *bitStream,
 * DT resyncThreshold) (ManchesterDecode.h:3): bits_out receives the '0'/'1' characters (room for nsymbols: after a
 * resynchronisation consecutive symbols can both end a bit),
 * *nbits_out their number (the return value); bit_symbol_out[j] (optional) = index idxi of the symbol whose time stamp the
 * reference's in-place compaction gives bit j (:86).                                                                   */
int      pdt_stage_manchester(pdt_ctx *ctx, const void *symbols_host, uint64_t nsymbols, double resync_threshold,
                              pdt_manchester_state *state, uint8_t *bits_out, uint32_t *bit_symbol_out, uint64_t *nbits_out);
typedef struct pdt_fir_state {          /* LowPassFilter.c:13-41 (interpolating form) / :76-100 (in place)               */
    uint64_t count;                     /* inputs filtered so far: the interpolating form's ring position is count mod K */
    double   history[64];               /* the last K inputs, oldest first; K = ntaps / interp (POES, 26) or ntaps (ARGOS, 50) */
} pdt_fir_state;
/* void LowPassFilterInterp(DT *inTime, DT *in, DT *out, DT *outTime, unsigned long n, DT *h, int N, int interp) with the
 * context's taps and interpolation factor (LowPassFilter.h:4; POES), void LowPassFilter(DT *data, unsigned long n, DT *h,
 * int N) (:6; ARGOS): n inputs -> n * interp outputs in out_host.  The time streams are closed-form here
 * (pdt_time_axis).                                                                                                    */
int      pdt_stage_fir(pdt_ctx *ctx, const void *in_host, uint64_t n, pdt_fir_state *state, void *out_host);

typedef struct pdt_pll_state {          /* CarrierTrackingPLL.c:60-75 */
    int32_t  started;                   /* 0 = the next call is the first one (firstLock == -2: the statics get their start values) */
    int32_t  locked;                    /* firstLock >= 0: the one-time lock has happened, the tracking gains are in force   */
    int64_t  lock_index;                /* firstLock: index, within the call that saw it, of the sample that declared the lock */
    double   lock_freq_hz;              /* " : PLL locked at %0.2fHz" (:269)                                                  */
    double   phase, freq;               /* d_phase, d_freq after the last sample                                              */
    double   avg_phase;                 /* averagePhase (the return value)                                                    */
    double   locksig;                   /* d_locksig                                                                          */
    double   sweep;                     /* sweep (signed, :232-246); frozen at the lock                                       */
} pdt_pll_state;
/* DT CarrierTrackPLL(DT complex *complexDataIn, DT *realDataOut, DT *lockSignalStreamOut, unsigned int nSamples, DT Fs, ...)
 * (CarrierTrackPLL.h:11) with the constants the context's main passes (POESTIPdemod/main.c:413-420, ARGOSdemod/main.c:265; the
 * twin's with PDT_CHAIN_LIVE).  iq_host = n samples as the capture file holds them: PDT_FMT_PCM16 (int16 pairs, converted to
 * `DT complex` as wave.c:127-172 does) or PDT_FMT_F32 (pairs of float = `float complex` as they are; float contexts only,
 * PDT_ERR_FORMAT otherwise); out_host = realDataOut, lock_out_host (optional) = lockSignalStreamOut, *avg_phase_ret (optional)
 * = the return value.  Runs the whole-capture path's PLL kernels (sequential acquisition, block-parallel tracking with
 * validated seams, lock-detector and averagePhase EMAs) from the record's state and stops behind the PLL.  Not with
 * cfg.profile (PDT_ERR_STATE; like every stage entry, not while a stream is open).                                                                          */
int      pdt_stage_pll(pdt_ctx *ctx, const void *iq_host, uint64_t n, int sample_format, pdt_pll_state *state, void *out_host,
                       void *lock_out_host, double *avg_phase_ret);
/* DT StaticGain(DT complex *complexData, unsigned int nSamples, DT desiredLevel) (AGC.h:4, AGC.c:48-74): the gain the mains
 * take from their first chunk (main.c:384-389, level 1.0).  The samples as the capture file holds them (PDT_FMT_PCM16: int16
 * pairs, converted as wave.c:127-172 does; PDT_FMT_F32: float pairs as they are); stateless.                              */
int      pdt_stage_static_gain(pdt_ctx *ctx, const void *iq_host, uint64_t n, int sample_format, double level, double *gain_out);
typedef struct pdt_gardner_state {      /* GardenerClockRecovery.c:12-15 */
    double   next_sample;               /* nextSample, rolled over by the chunk length at the end of the call (:113)          */
    double   prev_bit;                  /* prevBit                                                                            */
    double   half_sample;               /* halfSample: the mid-point INDEX of the next symbol, not rolled over (Q3)           */
} pdt_gardner_state;
/* unsigned long GardenerClockRecovery(DT *dataStreamIn, DT *dataStreamInTime, unsigned long numSamples, DT *dataStreamOut,
 * int Fs, DT baud, DT stepRange, DT kp) (GardenerClockRecovery.h:3) with the context's rate / baud / limits (main.c:438,
 * ARGOSdemod/main.c:278).  in_host is the caller's BUFFER: `capacity` elements of which the first n are this call's samples --
 * the function reads a few elements past n (the stale mid-point index of the first symbol, the look-ahead of the last), i.e.
 * whatever the buffer still holds there from earlier calls, zeros behind `capacity` (the mains over-allocate; fresh pages).
 * ARGOS: neighbour_host (optional) = the `capacity` elements of the array the main allocated right behind the buffer
 * (lockSignalStream, ARGOSdemod/main.c:169-176) -- with glibc's heap layout the reads past the buffer land there (Q16).
 * out_host: the symbols (room for n / (step - 0.25) + 2), pick_out[k] (optional) = index of the sample symbol k was taken
 * at (dataStreamInTime[k] = dataStreamInTime[pick_out[k]] is the in-place compaction), *nsym_out = the return value.
 * Runs the sequential sampler kernel of the streaming path (one wavefront).                                              */
int      pdt_stage_gardner(pdt_ctx *ctx, const void *in_host, uint64_t n, uint64_t capacity, const void *neighbour_host,
                           pdt_gardner_state *state, void *out_host, uint64_t *pick_out, uint64_t *nsym_out);
typedef struct pdt_mm_state {           /* MMClockRecovery.c:12-22 */
    int32_t  started;                   /* 0 = the next call is the first one (stepSize = Fs / baud, :20)                     */
    int32_t  pad;
    double   next_sample, step_size, sample_last;   /* nextSample (rolled over, :80), stepSize, sampleLast                    */
} pdt_mm_state;
/* unsigned long MMClockRecovery(DT *dataStreamIn, DT *dataStreamInTime, unsigned long numSamples, DT *dataStreamOut, int Fs,
 * DT baud, DT stepRange, DT kp) (MMClockRecovery.h:3) with the context's rate / baud and cfg.mm_step_range / mm_kp (0 = 3 and
 * 0.15, the commented-out call of ARGOSdemod/main.c:277).  Outputs as pdt_stage_gardner's; this sampler never reads past n.  */
int      pdt_stage_mm(pdt_ctx *ctx, const void *in_host, uint64_t n, pdt_mm_state *state, void *out_host, uint64_t *pick_out,
                      uint64_t *nsym_out);
typedef struct pdt_agc_state {          /* AGC.c:84-95 */
    int32_t  started;                   /* 0 = the next call is the first one: its `initial` becomes the gain           */
    int32_t  pad;
    double   gain;                      /* the static gain after the last call                                          */
} pdt_agc_state;
/* void NormalizingAGC(DT *dataStreamIn, unsigned long nSamples, DT initial, DT attack_rate, DT decay_rate) (AGC.h:6): in place
 * on data_host.  attack / decay 0 = the values the mains pass for this context's rate (POESTIPdemod/main.c:429-430,
 * ARGOSdemod/main.c:270).  Evaluated block-parallel with validated seams like the whole-capture path (k_agc_affine / _guess /
 * _block / _scan / _fix).                                                                                               */
int      pdt_stage_agc(pdt_ctx *ctx, void *data_host, uint64_t n, double initial, double attack, double decay,
                       pdt_agc_state *state);
/* void Squelch(DT *dataStream, DT *squelchStreamIn, unsigned long nSamples, DT squelchThreshold) (AGC.h:8): in place; its only
 * static (lastSquelch) feeds commented-out console output.                                                               */
int      pdt_stage_squelch(pdt_ctx *ctx, void *data_host, const void *lock_host, uint64_t n, double threshold);

/* Frame validation of the POES minor frames of the last pdt_demod_* call (a per-frame kernel and a
 * reduction on the GPU; the reference does this offline in MATLAB from the text file).  MATLAB is
 * 1-indexed: its minorFrames(frame, w) is bytes[w-1] here.                                          */
typedef struct pdt_tip_frame {
    uint16_t minor_id;     /* 9-bit minor-frame counter ((bytes[4] & 1) << 8) | bytes[5]   (daytimeDecode.m:4)      */
    uint8_t  spacecraft;   /* bytes[2]: 8 = NOAA-15, 13 = NOAA-18, 15 = NOAA-19            (daytimeDecode.m:16,82-93) */
    uint8_t  parity;       /* bit g set = even-parity check g failed; g = 0..4 covers bytes 2-18, 19-35, 36-52,
                              53-69, 70-86 against bits 5,4,3,2,1 of bytes[103]             (checkParity.m:20-86)  */
    uint8_t  checked;      /* 1 = complete frame (only whole frames are rows of the reference's matrix)            */
    uint8_t  has_time;     /* 1 = minor_id == 0: day / day_ms are valid                     (daytimeDecode.m:18)    */
    uint16_t day;          /* (bytes[8] << 1) + ((bytes[9] | 128) >> 7), as the reference computes it (:19)         */
    int32_t  day_ms;       /* ((bytes[9] & 7) << 24) + (bytes[10] << 16) + (bytes[11] << 8) + bytes[12];
                              -1 when not below 86 400 000                                  (:22-29)               */
} pdt_tip_frame;

typedef struct pdt_tip_summary {
    uint64_t frames_checked, good_frames;   /* "<good> out of <checked> Error Free Frames"  (checkParity.m:91)      */
    uint64_t good_chunks, bad_chunks;       /* zeros / ones of the parity matrix            (checkParity.m:92)      */
    int32_t  spacecraft;                    /* mode of the spacecraft ids, -1 = no frame    (daytimeDecode.m:82)    */
    int32_t  day;                           /* mode of the day numbers of the major-frame starts, -1 = none (:95)   */
    int64_t  t0_ms;                         /* mode(round(day_ms - 1000 * frame time)) over the positive ones,
                                               -1 = none (capture start in spacecraft ms of day, :34-36)            */
    uint64_t time_frames;                   /* frames with minor_id == 0                                             */
} pdt_tip_summary;

/* Runs the validation kernels on the frames of the last pdt_demod_* call (POES contexts only). */
int      pdt_tip_check(pdt_ctx *ctx, pdt_tip_summary *out);
/* Per-frame records of the last pdt_tip_check, in frame order; returns the number copied. */
uint64_t pdt_tip_frames(const pdt_ctx *ctx, pdt_tip_frame *out, uint64_t max_frames);
/* The same validation kernel on a caller's array of frame records (those of pdt_tip_sync, say): the summary in *out, the per-frame
 * records in per_frame[0 .. n) when not NULL.  POES contexts only; the context supplies device and stream, and nothing of its results
 * -- pdt_tip_frames included -- changes.  PDT_ERR_ARG for a null pointer with n > 0 or n >= 2^31; PDT_ERR_STATE while a stream is open. */
int      pdt_tip_check_records(pdt_ctx *ctx, const pdt_frame *frames, uint64_t n, pdt_tip_summary *out, pdt_tip_frame *per_frame);

/* Per-kernel device times of the last call (cfg.profile = 1). Returns the entry count. */
int      pdt_kernel_times(const pdt_ctx *ctx, pdt_kernel_time *out, int max_entries);

/* Host-side helpers */
int  pdt_make_lpf(int mode, uint32_t sample_rate, void *taps_out, int *ntaps, int *interp);
int  pdt_wav_parse_header(const uint8_t hdr[44], uint32_t *sample_rate, uint32_t *channels,
                          uint32_t *bits_per_sample, uint32_t *format, uint32_t *data_bytes);
/* Test hook, host only: the library's own restatements of the C-library functions the reference calls (sincos / sin / cos /
 * sincosf / hypot / hypotf; CarrierTrackingPLL.c:106-107,134-135, LowPassFilter.c:148,163, AGC.c:57-67) evaluated on the host
 * over an array.  fn: 0 sincos -> out0 = sin, out1 = cos; 1 sin; 2 cos; 3 sincosf of (float)x, widened; 4 hypot of the pairs
 * (x[2i], x[2i+1]) -> out0[i]; 5 hypotf of the pairs; 6 the branch-free sincosf of the fused mix + FIR kernel; 7 / 8 the error
 * and phase wraps of one float PLL step (CarrierTrackingPLL.c:168-188) in their fused form; 9 / 10 the error wrap as the plain
 * expression (compare with M_PI, correct by -+2 M_PI in double, narrow) in float (widened) / double; 11 / 12 arctan2_ref of the
 * pairs (y, x) = (x[2i], x[2i+1]) in float (widened) / double (CarrierTrackingPLL.c:15-40); 13 q_rsqrt of (float)x (:43-52).
 * The kernels run the same code (9 / 10: the same expression in another form); pdt_device_math evaluates it on the device.   */
int  pdt_host_math(int fn, const double *x, uint64_t n, double *out0, double *out1);

/* Test hook, device: the scalar primitives the kernels are made of (csrc/pdt_device_math.h, csrc/pdt_kernels_front.h,
 * csrc/pdt_kernels_back.h), each evaluated by itself on the GPU -- one record per lane, the very functions (and the very
 * machine-code blocks) the kernels call.  `n` records of `nin` elements go in, `n` records of `nout` elements come out, record
 * after record; an element is a float (4 bytes) or a double (8) as the table says, never widened.  Codes 0 - 8 mean what they
 * mean in pdt_host_math.
 *
 *   fn  elem  nin  nout  function                                   record in -> out
 *    0   f64    1    2   sincos_glibc                               x -> sin, cos
 *    1   f64    1    1   sin_glibc                                  x -> sin
 *    2   f64    1    1   cos_glibc                                  x -> cos
 *    3   f32    1    2   sincosf_glibc                              x -> sin, cos
 *    4   f64    2    1   hypot_glibc                                x, y -> h
 *    5   f32    2    1   hypotf_glibc                               x, y -> h
 *    6   f32    1    2   sincosf_flat                               x -> sin, cos
 *    7   f32    1    1   pll_wrap_error_f32 (its machine-code form) x -> r
 *    8   f32    1    1   pll_wrap_phase_f32                         x -> r
 *    9   f32    1    1   PiAbs::ge_pi(x) ? unwrap_2pi(x) : x        x -> r      (the error wrap of the generic loop-filter step)
 *   10   f64    1    1   the same in double                         x -> r
 *   11   f32    2    1   arctan2_ref                                y, x -> angle
 *   12   f64    2    1   arctan2_ref                                y, x -> angle
 *   13   f32    1    1   q_rsqrt                                    x -> r
 *   14   f32    6    2   pll_phase_step<float, false>               th, phase, freq, alpha, beta, maxf -> phase', freq'   (minf = -maxf)
 *   15   f32    6    2   pll_phase_step<float, true>                 "
 *   16   f64    6    2   pll_phase_step<double, false>               "
 *   17   f64    6    2   pll_phase_step<double, true>                "
 *   18   f32   10    7   acq_vec4_asm<false>                        th0..th3, phase, freq, sweep, alpha, beta, maxf -> pb[0..3], phase', freq', sweep'
 *   19   f32   10    7   acq_vec4_asm<true>                          "
 *   20   f32   10    7   pll_vec4_asm                               the same record -> p[0..3], phase' (= p[3]), freq', sweep (as given)
 *   21   f32    4    2   pll_sweep_sel<float>                       fr, sw, maxf, on (0 = off) -> fr', sw'                (minf = -maxf)
 *   22   f64    4    2   pll_sweep_sel<double>                       "
 *   23   f32    1    2   rint_index, Real<float>::rint              x -> the index (an int32 in the element's bytes), rint(x)
 *   24   f64    1    2   rint_index, Real<double>::rint             x -> the index (an int64 in the element's bytes), rint(x)
 *   25   f32    2    1   clip_finite                                e, lim -> clipped
 *   26   f64    2    1   clip_finite                                e, lim -> clipped
 *   27   f32   19   35   agc_calm<float, 4>, agc_step, agc_step_calm  x[16], gain, attack, decay -> calm (0 / 1), y[16] and the gain
 *                                                                   after the batch through agc_step, the same through agc_step_calm
 *
 * 18 - 20: alpha, beta and maxf are scalar-register operands of the blocks, as in the kernels (launch constants there): they
 * must be the same in every record of a call (PDT_ERR_ARG otherwise).  20 ends in an LDS-direct load, the refill of a walker's
 * look-ahead ring: the probe gives every lane 16 bytes of a buffer of its own to fetch and a slot of its own workgroup's LDS.
 * One ordinary launch per call on the context's stream; returns when the results are in `out`.                              */
#define PDT_DEVICE_MATH_FNS 28
int  pdt_device_math(pdt_ctx *ctx, int fn, const void *in, uint64_t n, void *out);
/* The table above: bytes per element, elements per record in and out (NULL = not wanted); PDT_ERR_ARG for an unknown fn. */
int  pdt_device_math_layout(int fn, int *elem_bytes, int *nin, int *nout);
/* The reference's running-sum time axis (wave.c:91,96-97,167-168): value after m additions of Ts. */
double pdt_time_axis(int mode, uint32_t sample_rate, uint64_t m);

#ifdef __cplusplus
}
#endif
#endif
