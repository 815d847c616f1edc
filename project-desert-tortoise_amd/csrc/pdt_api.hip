// pdt_api.hip -- libpdt.so: context management, kernel orchestration and the C ABI of
// include/pdt.h (the host -> HBM ingest the entries go through: pdt_ingest.hip).  Compiled for gfx950 only, with
// -ffp-contract=off (see pdt_device_math.h).
#include "pdt_rt.h"
#include "pdt_analytic.h"
#include "pdt_ddc.h"
#include "pdt_survey.h"
#include "pdt_bursts.h"
#include "pdt_tone.h"
#include "pdt_argos_msg.h"
#include "pdt_tip_sync.h"
#include "pdt_ff.h"
#include "pdt_ffp.h"
#include "pdt_tip_dcs.h"
#include "pdt_tip_subcom.h"

#include <sys/stat.h>

namespace pdtrt {
PDT_CHAIN_INSTANCES(extern, float)
PDT_CHAIN_INSTANCES(extern, double)
std::atomic<long long> g_alloc_ns{0};
// pdt_analytic.hip
hipError_t analytic_launch(hipStream_t st, int fmt, const void *x, long long lo, long long hi, unsigned long long n_out, unsigned long long g0,
                           uint32_t step, const float *tab_dev, void *out);
// pdt_survey.hip
size_t survey_part_floats(uint64_t nseg, int nfft);
hipError_t survey_launch(hipStream_t st, int fmt, const void *x, uint64_t nseg, int nfft, const float *win, const float *tw, float *part, float *out);
int survey_plan(const pdt_survey_cfg *cfg, double mode_range_hz, double channel_rate, uint64_t nframes, int cap, pdt::SurveyPlan *p);
int survey_carriers(const float *P, const pdt::SurveyPlan &p, double in_rate, pdt_carrier *found);
// pdt_bursts.hip
hipError_t waterfall_launch(hipStream_t st, int fmt, const void *x, uint64_t nrows, int rows_per, int nfft, const float *win, const float *tw, float *rows);
hipError_t row_peaks_launch(hipStream_t st, const float *rows, uint64_t nrows, int nfft, float level, int gb, void *peaks, int *counts);
int bursts_plan(const pdt_bursts_cfg *cfg, double mode_range_hz, double channel_rate, double in_rate, uint64_t nframes, int cap, pdt::BurstPlan *p);
pdt::SurveyPlan bursts_survey_plan(const pdt::BurstPlan &p, const pdt_bursts_cfg *cfg, uint64_t nframes);
int bursts_link(const void *peaks, const int *counts, bool compact, const pdt::BurstPlan &p, double floor, double in_rate, pdt_burst *found, int cap);
// pdt_tone.hip
hipError_t tones_launch(hipStream_t st, int nfft, const void *segs_dev, uint64_t nsegs, int lo, int hi, const float *win, const float *tw, void *out);
int tone_plan(const pdt_tone_cfg *cfg, double fs, double range_hz, uint64_t len, int cap, pdt::TonePlan *p);
void tone_sums(int nfft, double *sw, double *sw2);
void tones_derive(const void *raw, const pdt::TonePlan &p, double fs, double offset_hz, double sw, double sw2, pdt_tone *out);
// pdt_argos_msg.hip
// (every *_launch below: `inner` is NULL, or the events recorded between its kernels -- CallTimer::inner)
hipError_t argos_msgs_launch(hipStream_t st, const void *table_dev, int nctx, long long tiles, int K, int rule, hipEvent_t *inner);
int argos_min_run(const pdt_argos_cfg *cfg, int *K, int *rule);
// pdt_tip_sync.hip
extern const char *const tip_sync_kernel_names[5];
hipError_t tip_sync_launch(hipStream_t st, const void *table_dev, int nctx, long long tiles, pdt::TipSyncRule R, hipEvent_t *inner);
int tip_sync_rule(const pdt_tip_sync_cfg *cfg, pdt::TipSyncRule *R);
// pdt_ff.hip
hipError_t ff_launch(hipStream_t st, const void *table_dev, int nwin, long long mix_tiles, long long groups, const long long *periods_dev, int R,
                     int H, long long pmax, const float *tab_dev, void *metric_dev, size_t metric_bytes, void *syncs_dev, hipEvent_t *inner);
int ff_plan(const pdt_ff_cfg *cfg, uint32_t rate, int *H, int *R, double *ppm, int *given, double *residual);
// pdt_ffp.hip
int ffp_plan(const pdt_ffp_cfg *cfg, uint32_t rate, uint64_t n, pdt::FfpRule *r, int *given, double *residual);
int ffp_run_device(hipStream_t st, const float *y, const pdt::FfpRule &r, const pdt::FfpSync &head, const std::vector<uint32_t> &steps,
                   const std::vector<uint32_t> &starts, const float *tab_dev, void *work, const pdt::FfpOutPtrs &out, uint64_t bit_cap, hipEvent_t *inner);
uint64_t ffp_bit_cap(const pdt::FfpRule &r);
size_t ffp_work_bytes(const pdt::FfpRule &r, size_t nent);
void ffp_steps(const pdt_tone *tones, uint64_t nseg, int nfft, const pdt::FfpRule &r, int given, double residual, std::vector<uint32_t> &steps,
               std::vector<uint32_t> &starts, pdt::FfpSync *head);
// pdt_tip_repair.hip
hipError_t tip_repair_launch(hipStream_t st, void *recs_dev, unsigned nrec, const float *soft_dev, const unsigned long long *nbits_dev, long long bit_cap,
                             void *info_dev, void *sum_dev);
// pdt_tip_dcs.hip
extern const char *const tip_dcs_kernel_names[4];
size_t tip_dcs_map_bytes();
size_t tip_dcs_entry_bytes();
hipError_t tip_dcs_launch(hipStream_t st, const void *recs_dev, bool chain_layout, const void *times_dev, unsigned long long n, unsigned channel_max,
                          void *sum_dev, void *flags_dev, void *stream_dev, void *head_dev, void *bad_dev, void *maps_dev, void *entry_dev, void *out_dev,
                          unsigned long long cap, hipEvent_t *inner);
void tip_dcs_summary(const unsigned long long *c, unsigned long long n, pdt_dcs_summary *s);
int tip_dcs_rule(const pdt_dcs_cfg *cfg, unsigned *channel_max);
// pdt_tip_subcom.hip
extern const char *const tip_subcom_kernel_names[5];
hipError_t tip_subcom_launch(hipStream_t st, const void *recs_dev, bool chain_layout, const void *times_dev, unsigned long long n, const void *table_dev, int ne,
                             int nchan, int trusted_only, int thr, void *sum_dev, void *marks_dev, void *cnt_dev, void *offsets_dev, void *vals_dev,
                             unsigned long long limit, void *out_dev, unsigned long long cap, hipEvent_t *inner);
void tip_subcom_summary(const unsigned long long *c, pdt_subcom_summary *s);
int tip_subcom_rule(const pdt_subcom_entry *entries, uint64_t nentries, const pdt_subcom_cfg *cfg, uint64_t n, int *nchan, int *max_fire, int *trusted_only, int *thr);
// pdt_ddc.hip
long long ddc_windows_table(int decim, pdt::DdcWindow *win, int count, std::vector<unsigned char> &table);
hipError_t ddc_windows_launch(hipStream_t st, int fmt, int decim, const float *taps_dev, const float *tab_dev, const void *table_dev, int count,
                              long long tiles);
hipError_t ddc_launch(hipStream_t st, int fmt, int decim, const float *taps_dev, const float *tab_dev, pdt::DdcWindow w);
}  // namespace pdtrt

static std::mutex g_dev_mu;
static std::map<std::string, std::string> g_dev;
void Tuning::load()
{
    std::lock_guard<std::mutex> lock(g_dev_mu);
    if (g_dev.empty()) return;
    auto get = [&](const char *n) -> const char * { auto it = g_dev.find(n); return it == g_dev.end() ? nullptr : it->second.c_str(); };
    if (const char *e = get("PDT_PLL_WARM_SCALE")) pll_warm_scale = atof(e);
    if (const char *e = get("PDT_HEAD_TAUS")) head_taus = atof(e);
    if (const char *e = get("PDT_BAND_PAD")) band_pad = atof(e);
    if (const char *e = get("PDT_PLL_WARM_S")) pll_warm_s = atof(e);
    if (const char *e = get("PDT_AGC_WARM_S")) agc_warm_s = atof(e);
    if (const char *e = get("PDT_AGC_K")) agc_k = atof(e);
    if (const char *e = get("PDT_AGC_TPB")) agc_tpb = std::max(1, atoi(e));
    if (const char *e = get("PDT_PLL_BLOCK")) pll_block = atoi(e);
    if (const char *e = get("PDT_HBM_LIMIT_MB")) hbm_limit_mb = std::max(1ll, atoll(e));        // (tests: pretend the device has this much free memory)
    if (const char *e = get("PDT_BURST_SLAB_ROWS")) burst_slab_rows = std::max(1ll, atoll(e));    // (tests: rows per slab of a burst search, to cross a seam)
    if (const char *e = get("PDT_WINDOW_PIECE")) window_piece = std::max(1ll, atoll(e));          // (tests: samples per piece of the bounded window)
    if (const char *e = get("PDT_SCOUT_SYMS")) scout_syms = std::max(16, atoi(e));
    if (const char *e = get("PDT_FIR_WG_PER_CU")) fir_wg_per_cu = std::min(4096, std::max(1, atoi(e)));
    if (const char *e = get("PDT_INGEST_THREADS")) ingest_threads = std::min(128, std::max(1, atoi(e)));
    if (const char *e = get("PDT_INGEST_SPAN_MB")) ingest_span_mb = std::min(256, std::max(1, atoi(e)));
    if (const char *e = get("PDT_INGEST_STREAMS")) ingest_streams = std::min(4, std::max(1, atoi(e)));
    if (const char *e = get("PDT_INGEST_DIRECT")) ingest_direct = atoi(e) ? 1 : 0;
    if (const char *e = get("PDT_INGEST_NUMA")) ingest_numa = atoi(e) ? 1 : 0;
    if (const char *e = get("PDT_FIX_PASSES")) fix_passes = atoi(e);
    if (const char *e = get("PDT_GSEG")) gseg = std::min(64, std::max(2, atoi(e)));
    if (const char *e = get("PDT_GSPAN")) gspan = std::min(256, std::max(1, atoi(e)));
    if (const char *e = get("PDT_GSPAN_REKEY")) gspan_rekey = std::min(255, std::max(0, atoi(e)));      // chunks walked before the re-key; 0: single stage
    if (const char *e = get("PDT_GSPAN_SUB")) gspan_sub = atoi(e);                                     // lanes per row in stage 2: 8, 16 or 32
    if (const char *e = get("PDT_GSPAN_WIN2")) gspan_win2 = atoi(e);                                   // stage 2's LDS window per row: 512, 1024 or 2048 floats
    if (const char *e = get("PDT_GSPAN_FIT")) gspan_fit = std::min(64, std::max(2, atoi(e)));            // the span the rule would want (the search for a short last group still runs)
    if (const char *e = get("PDT_GSPAN_CAP")) gspan_cap = std::max(64, atoi(e));          // (tests: rows that do not fit the key list)
    fir_generic = get("PDT_FIR_GENERIC") != nullptr;
    mix_unfused = get("PDT_MIX_UNFUSED") != nullptr;
    quality_inline = get("PDT_QUALITY_INLINE") != nullptr;
    gardner_nostride = get("PDT_GARDNER_NOSTRIDE") != nullptr;
    gemit_groups = get("PDT_GEMIT_GROUPS") != nullptr;
    agc_unfused = get("PDT_AGC_UNFUSED") != nullptr;
    manch_3pass = get("PDT_MANCH_3PASS") != nullptr;        // Manchester as tile summaries, one-workgroup scan, emission
    sync_serial = get("PDT_SYNC_SERIAL") != nullptr;        // frame filter in one workgroup (k_sync_frames_tiles)
    agc_lanes = get("PDT_AGC_LANES") != nullptr;           // the per-lane walkers of rounds 1 - 3 (k_agc_block)
    no_excl = get("PDT_NO_EXCL") != nullptr;
    gardner_onebuf = get("PDT_GARDNER_ONEBUF") != nullptr;
    gardner_noring = get("PDT_GARDNER_NORING") != nullptr;
    ema_noguess = get("PDT_EMA_NOGUESS") != nullptr;
    gardner_sequential = get("PDT_GARDNER_SEQUENTIAL") != nullptr;
    seg_sequential = get("PDT_SEG_SEQUENTIAL") != nullptr;
    overlap = get("PDT_NO_OVERLAP") == nullptr;            // (round 4: off unless PDT_OVERLAP; round 5: on)
    if (const char *e = get("PDT_OVERLAP_SPLIT")) {          // "0.55,0.28,0.17": the segments' fractions of the capture
        int k = 0;
        for (const char *q = e; *q && k < 8; k++) {
            char *end = nullptr;
            overlap_split[k] = strtod(q, &end);
            if (end == q) break;
            q = (*end == ',') ? end + 1 : end;
        }
    }
    chain_one_range = get("PDT_CHAIN_ONE_RANGE") != nullptr;
    debug_overlap = get("PDT_DEBUG_OVERLAP") != nullptr;
    if (const char *e = get("PDT_OVERLAP_SEGMENTS")) overlap_segments = std::min(64, std::max(1, atoi(e)));
    if (const char *e = get("PDT_OVERLAP_MIN_MB")) overlap_min_mb = std::min(1 << 20, std::max(1, atoi(e)));
    debug_sync = get("PDT_DEBUG_SYNC") != nullptr;
    pll_noshort = get("PDT_PLL_NOSHORT") != nullptr;
    pll_nockpt = get("PDT_PLL_NOCKPT") != nullptr;
    pll_noconsensus = get("PDT_PLL_NOCONSENSUS") != nullptr;
    pll_notail = get("PDT_PLL_NOTAIL") != nullptr;
    seg_plain = get("PDT_SEG_PLAIN") != nullptr;
    sync_block = get("PDT_SYNC_BLOCK") != nullptr;
}

namespace pdtrt {

// Run the plans of M contexts (all of one shape, see Plan::same_shape) as one sequence of operations on the streams of
// ctxs[0]: each launch covers the M captures through grid.z, memsets and copies are issued per capture.  No host wait.
int execute_plans(pdt_ctx *const *ctxs, int M)
{
    pdt_ctx *L0 = ctxs[0];
    HIP_TRY(hipSetDevice(L0->cfg.device));
    const Plan &P0 = L0->plan;
    for (int m = 1; m < M; m++)
        if (!P0.same_shape(ctxs[m]->plan)) return PDT_ERR_STATE;
    const size_t per = P0.packs.size();
    const size_t total = per * (size_t)M;
    int rc;
    if ((rc = L0->packs_dev.ensure(total + 64))) return rc;
    if (total + 64 > L0->packs_pin_cap) {
        if (L0->packs_pin) (void)hipHostFree(L0->packs_pin);
        L0->packs_pin = nullptr;
        L0->packs_pin_cap = 0;
        const size_t want = 2 * total + 4096;
        if (timed_host_malloc((void **)&L0->packs_pin, want) != hipSuccess) { (void)hipGetLastError(); return PDT_ERR_NOMEM; }
        L0->packs_pin_cap = want;
    }
    // pack of capture m for the launch at offset `off`: M * off + m * size
    unsigned char *pin = (unsigned char *)L0->packs_pin;
    for (const PlanOp &o : P0.ops) {
        if (o.op != OP_LAUNCH) continue;
        for (int m = 0; m < M; m++)
            memcpy(pin + (size_t)M * o.pack_off + (size_t)m * o.pack_size, ctxs[m]->plan.packs.data() + o.pack_off, o.pack_size);
    }
    hipStream_t st[2] = { L0->stream, L0->stream2 };
    if (total) HIP_TRY(hipMemcpyAsync(L0->packs_dev.p, pin, total, hipMemcpyHostToDevice, st[0]));
    Launcher T(L0);
    const unsigned char *dev = (const unsigned char *)L0->packs_dev.p;
    for (size_t i = 0; i < P0.ops.size(); i++) {
        const PlanOp &o = P0.ops[i];
        switch (o.op) {
        case OP_LAUNCH: {
            dim3 g = o.grid;
            for (int m = 1; m < M; m++) {
                const dim3 gm = ctxs[m]->plan.ops[i].grid;
                g.x = std::max(g.x, gm.x);
                g.y = std::max(g.y, gm.y);
            }
            g.z = (unsigned)M;
            o.go(g, o.block, o.shmem, st[o.side], dev + (size_t)M * o.pack_off);
            if (L0->tune.debug_sync) {                                  // developer switch: find the launch that faults
                const hipError_t e = hipStreamSynchronize(st[o.side]);
                fprintf(stderr, "libpdt: [%zu] %s grid (%u,%u,%u) block %u lds %zu: %s\n", i, o.name, g.x, g.y, g.z, o.block.x, o.shmem,
                        hipGetErrorString(e));
            }
            break;
        }
        case OP_MEMSET:
            for (int m = 0; m < M; m++) {
                const PlanOp &om = ctxs[m]->plan.ops[i];
                if (om.bytes) HIP_TRY(hipMemsetAsync(om.dst, om.value, om.bytes, st[om.side]));
            }
            T.gap();
            break;
        case OP_D2H:
        case OP_H2D:
            for (int m = 0; m < M; m++) {
                const PlanOp &om = ctxs[m]->plan.ops[i];
                if (om.bytes)
                    HIP_TRY(hipMemcpyAsync(om.dst, om.src, om.bytes, o.op == OP_D2H ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice, st[0]));
            }
            T.gap();
            break;
        case OP_FORK:
            HIP_TRY(hipEventRecord(L0->ev_fork, st[0]));
            HIP_TRY(hipStreamWaitEvent(st[1], L0->ev_fork, 0));
            break;
        case OP_JOIN_RECORD: HIP_TRY(hipEventRecord(L0->ev_join, st[1])); break;
        case OP_JOIN_WAIT: HIP_TRY(hipStreamWaitEvent(st[0], L0->ev_join, 0)); break;
        case OP_TBEGIN: T.begin(o.name, st[o.side]); break;
        case OP_TEND: T.end(); break;
        case OP_TGAP: T.gap(); break;
        case OP_EV0: HIP_TRY(hipEventRecord(L0->ev0, st[0])); break;
        case OP_EV1: HIP_TRY(hipEventRecord(L0->ev1, st[0])); break;
        }
    }
    HIP_TRY(hipGetLastError());
    for (int m = 0; m < M; m++) ctxs[m]->leader = L0;
    return PDT_OK;
}

void launch_bytesync(pdt_ctx *ctx, Plan &PL, hipStream_t st, const SyncParams &SP, DevScalars *d_sc, long long bit_cap, uint32_t hit_cap,
                     uint32_t frame_cap, long long min_pos)
{
    unsigned char *d_bits = (unsigned char *)ctx->bits.p;
    unsigned *d_bitsym = (unsigned *)ctx->bitsym.p;
    long long *d_symidx = (long long *)ctx->symidx.p;
    unsigned *d_hits = (unsigned *)ctx->hits.p;
    FrameRec *d_frames = (FrameRec *)ctx->frames.p;
    const long long n_stiles = (bit_cap + 4095) / 4096;
    SyncTile *d_stiles = (SyncTile *)ctx->stiles.p;
    PDT_LAUNCH(256, k_sync_hits_tile, dim3((unsigned)n_stiles), dim3(256), 0, st, d_bits, &d_sc->nbits, SP, d_stiles,
                       &d_sc->sync_overflow, min_pos);
    unsigned *d_scr = (unsigned *)ctx->sync_scr.p;
    if (ctx->tune.sync_serial) {
        PDT_LAUNCH(PDT_SYNC_THREADS, k_sync_frames_tiles, dim3(1), dim3(PDT_SYNC_THREADS), 0, st, (const SyncTile *)d_stiles, &d_sc->nbits, SP, d_hits,
                           hit_cap, d_frames, &d_sc->nframes, frame_cap, &d_sc->sync_overflow, d_scr);
    } else {
        // the batches are counted on the device: a grid of fixed size walks them (at most the capacity's)
        const unsigned n_batch = (unsigned)std::min<long long>(256, ((long long)hit_cap + PDT_SYNC_PB - 1) / PDT_SYNC_PB);
        PDT_LAUNCH(PDT_SYNC_THREADS, k_sync_dense, dim3(1), dim3(PDT_SYNC_THREADS), 0, st, (const SyncTile *)d_stiles, &d_sc->nbits, n_stiles,
                           hit_cap, &d_sc->sync_overflow, d_scr);
        PDT_LAUNCH(256, k_sync_gather, dim3((unsigned)std::min<long long>(1024, (n_stiles + 255) / 256)), dim3(256), 0, st,
                           (const SyncTile *)d_stiles, &d_sc->nbits, n_stiles, d_hits, hit_cap, &d_sc->sync_overflow, (const unsigned *)d_scr);
        PDT_LAUNCH(PDT_SYNC_PT, k_sync_links, dim3(n_batch), dim3(PDT_SYNC_PT), 0, st, SP, (const unsigned *)d_hits, &d_sc->sync_overflow, d_scr,
                           hit_cap);
        PDT_LAUNCH(PDT_SYNC_PT, k_sync_mark, dim3(n_batch), dim3(PDT_SYNC_PT), 0, st, SP, (const unsigned *)d_hits, d_frames, &d_sc->nframes,
                           frame_cap, &d_sc->sync_overflow, (const unsigned *)d_scr, hit_cap);
    }
    // generic path (atomic append + sort), only when a tile overflowed; the fixed grids below walk what the device counted
    const long long grid = std::min<long long>(2048, (bit_cap + 255) / 256);
    PDT_LAUNCH(256, k_sync_hits, dim3((unsigned)grid), dim3(256), 0, st, d_bits, &d_sc->nbits, SP, d_hits, &d_sc->nhits, hit_cap,
                       &d_sc->sync_overflow, min_pos);
    PDT_LAUNCH(256, k_sync_frames, dim3(1), dim3(256), 0, st, d_hits, &d_sc->nhits, hit_cap, SP, d_frames, &d_sc->nframes,
                       frame_cap, &d_sc->sync_overflow);
    PDT_LAUNCH(128, k_frame_pack, dim3(std::min<uint32_t>(frame_cap, 16384)), dim3(128), 0, st, d_bits, &d_sc->nbits, d_bitsym, d_symidx, SP,
                       d_frames, &d_sc->nframes, frame_cap);
}

// reports of chunks [c0, c1) of the capture (c1 <= chunk_host.size()); `total`: the capture's length as far as it is known
// `open_frame`: a frame whose sync word has been seen and whose last byte has not (a segment's end) -- counted where ByteSync
// counts it, at the sync word
void chunk_reports_range(const pdt_ctx *ctx, uint64_t c0, uint64_t c1, uint64_t total, pdt_chunk_report *out, const pdt_frame *open_frame)
{
    const bool argos = ctx->cfg.mode == PDT_MODE_ARGOS;
    const uint64_t chunk = ctx->cfg.chunk;
    uint64_t sym_prev = c0 ? ctx->chunk_host[(size_t)c0 - 1].sym_upto : 0, bits_prev = c0 ? ctx->chunk_host[(size_t)c0 - 1].bits_upto : 0;
    size_t f = 0;
    if (c0) {                                            // first frame whose sync word was completed behind chunk c0 - 1
        size_t lo = 0, hi = ctx->frames_host.size();
        while (lo < hi) {
            const size_t mid = (lo + hi) / 2;
            if ((uint64_t)ctx->frames_host[mid].bit_index < bits_prev) lo = mid + 1; else hi = mid;
        }
        f = lo;
    }
    for (uint64_t c = c0; c < c1; c++) {
        const pdt::ChunkInfo &ci = ctx->chunk_host[(size_t)c];
        pdt_chunk_report &o = out[c - c0];
        memset(&o, 0, sizeof o);
        o.samples = std::min<uint64_t>(chunk, total - c * chunk);
        o.avg_phase = ci.avg_phase;
        o.symbols = ci.sym_upto - sym_prev;
        o.bits = ci.bits_upto - bits_prev;
        // ByteSyncOnSyncword / FindSyncWords count a frame at the bit that completes its sync word (ByteSync.c:105,139)
        while (f < ctx->frames_host.size() && (uint64_t)ctx->frames_host[f].bit_index < ci.bits_upto) { o.frames++; f++; }
        if (open_frame && (uint64_t)open_frame->bit_index >= bits_prev && (uint64_t)open_frame->bit_index < ci.bits_upto) o.frames++;
        // waveDataTime[0] as the progress line prints it: POES keeps the input time axis apart (main.c:424,438,445), ARGOS
        // compacts the symbol and bit times into it (ARGOSdemod/main.c:278,282)
        o.time0 = (argos && ctx->elem == 8) ? const_cast<pdt_ctx *>(ctx)->axis_d.at((uint64_t)ci.t0_src + 1)
                  : argos ? (double)const_cast<pdt_ctx *>(ctx)->axis_f.at((uint64_t)ci.t0_src + 1)
                          : (double)const_cast<pdt_ctx *>(ctx)->axis_f.at(c * chunk + 1);
        sym_prev = ci.sym_upto;
        bits_prev = ci.bits_upto;
    }
}


}  // namespace pdtrt

// ================================================================================= C ABI
extern "C" {

int pdt_abi_version(void) { return PDT_ABI_VERSION; }
#ifndef PDT_BUILD_TAG
#define PDT_BUILD_TAG "untagged"
#endif
const char *pdt_build_tag(void) { return PDT_BUILD_TAG; }

// test-only (include/pdt_dev.h): set (value != NULL), remove (value == NULL) or clear (name == NULL) developer switches
int pdt_dev_set(const char *name, const char *value)
{
    try {
        std::lock_guard<std::mutex> lock(g_dev_mu);
        if (!name) g_dev.clear();
        else if (!value) g_dev.erase(name);
        else g_dev[name] = value;
    } catch (const std::exception &) { return PDT_ERR_NOMEM; }
    return PDT_OK;
}

unsigned long long pdt_dev_span_rows(const pdt_ctx *ctx, unsigned *n_exits_out, unsigned long long max)
{
    if (!ctx || ctx->gspan_nrows <= 0 || !ctx->gspan_rows.p) return 0;
    const unsigned long long n = (unsigned long long)ctx->gspan_nrows, m = std::min(n, max);
    if (n_exits_out && m) {
        std::vector<GardnerSpanRow> rows((size_t)m);
        if (hipSetDevice(ctx->cfg.device) != hipSuccess ||
            hipMemcpy(rows.data(), ctx->gspan_rows.p, (size_t)m * sizeof(GardnerSpanRow), hipMemcpyDeviceToHost) != hipSuccess) {
            (void)hipGetLastError();
            return 0;
        }
        for (size_t k = 0; k < (size_t)m; k++) n_exits_out[k] = rows[k].n;
    }
    return n;
}

unsigned long long pdt_dev_span_rekey(const pdt_ctx *ctx, unsigned *out, unsigned long long max)
{
    if (!ctx || ctx->gspan_nrows <= 0 || !ctx->gspan_rows.p) return 0;
    const unsigned long long n = (unsigned long long)ctx->gspan_nrows, m = std::min(n, max);
    if (out && m) {
        const bool staged = ctx->gspan_rekey > 0 && ctx->gspan_info.p;
        std::vector<GardnerSpanRow> rows((size_t)m);
        std::vector<GardnerSpanRowInfo> info((size_t)m);
        if (hipSetDevice(ctx->cfg.device) != hipSuccess ||
            hipMemcpy(rows.data(), ctx->gspan_rows.p, (size_t)m * sizeof(GardnerSpanRow), hipMemcpyDeviceToHost) != hipSuccess ||
            (staged && hipMemcpy(info.data(), ctx->gspan_info.p, (size_t)m * sizeof(GardnerSpanRowInfo), hipMemcpyDeviceToHost) != hipSuccess)) {
            (void)hipGetLastError();
            return 0;
        }
        for (size_t k = 0; k < (size_t)m; k++) {
            out[3 * k] = rows[k].n;
            out[3 * k + 1] = staged ? info[k].states : 0u;
            out[3 * k + 2] = staged ? info[k].items : 0u;
        }
    }
    return n;
}

// test-only (include/pdt_dev.h): which filter kernel the last run took, and how many AGC maps it wrote
unsigned pdt_dev_fir_form(const pdt_ctx *ctx, unsigned long long *fused_tiles_out)
{
    if (fused_tiles_out) *fused_tiles_out = ctx ? (unsigned long long)ctx->fir_fused_tiles : 0ull;
    return ctx ? (unsigned)ctx->fir_form : 0u;
}

// test-only (include/pdt_dev.h): the down-converter on exactly this record, one launch by value; no context
int pdt_dev_ddc(int device, uint32_t in_rate, int decim, double offset_hz, int sample_format, const void *x_dev, long long lo, long long hi,
                uint64_t n_out, uint64_t g0, void *out_dev)
{
    if (in_rate == 0 || decim < DDC_MIN_DECIM || decim > DDC_MAX_DECIM || !ddc_fmt(sample_format) || !x_dev || !out_dev) return PDT_ERR_ARG;
    if (!(std::isfinite(offset_hz) && std::fabs(offset_hz) < 0.5 * (double)in_rate)) return PDT_ERR_ARG;
    HIP_TRY(hipSetDevice(device));
    const std::vector<float> taps = ddc_taps(decim);
    std::vector<float> tab(2 * AN_TAB);
    analytic_table(tab.data());
    DevBuf dtaps, dtab;
    auto run = [&]() -> int {
        int rc;
        if ((rc = dtaps.ensure(taps.size() * sizeof(float) + 16)) || (rc = dtab.ensure(tab.size() * sizeof(float) + 16))) return rc;
        HIP_TRY(hipMemcpy(dtaps.p, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dtab.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
        const DdcWindow r = { x_dev, out_dev, lo, hi, (long long)n_out, ddc_step((double)in_rate, offset_hz), (uint32_t)g0, 0 };
        HIP_TRY(ddc_launch(nullptr, sample_format, decim, (const float *)dtaps.p, (const float *)dtab.p, r));
        HIP_TRY(hipStreamSynchronize(nullptr));
        return PDT_OK;
    };
    const int rc = run();
    dtaps.release();
    dtab.release();
    return rc;
}

const char *pdt_strerror(int code)
{
    switch (code) {
    case PDT_OK: return "ok";
    case PDT_ERR_ARG: return "bad argument";
    case PDT_ERR_NOGPU: return "no usable HIP device / HIP runtime error";
    case PDT_ERR_NOMEM: return "out of device memory";
    case PDT_ERR_FORMAT: return "unsupported WAV format (need 16-bit PCM, 2 channels)";
    case PDT_ERR_RATE: return "sample rate too high: interpolation factor would be 0";
    case PDT_ERR_STATE: return "call sequence / internal capacity error";
    case PDT_ERR_IO: return "read error on the capture file";
    default: return "unknown error";
    }
}

int pdt_get_device(const pdt_ctx *ctx) { return ctx ? ctx->cfg.device : -1; }

int pdt_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

// Host evaluation of the library's own restatements of the C-library functions the reference calls (test hook: the CPU
// tests compare them with the C library of the machine, bit for bit).  fn: 0 sincos(x) -> out0 sin, out1 cos; 1 sin; 2 cos;
// 3 sincosf((float)x) widened; 4 hypot(x[2i], x[2i+1]) -> out0[i]; 5 hypotf of the pair, widened; 6 the branch-free form
// of 3 (sincosf_flat: what the fused mix + FIR kernel evaluates); 7 / 8 the error and phase wraps of one float PLL step
// (pll_wrap_error_f32 / pll_wrap_phase_f32), widened; 9 / 10 the error wrap as the reference writes it (CarrierTrackingPLL.c:168-173: the
// difference compared with M_PI as a double, corrected by -+2 M_PI in double, narrowed) for (float)x / x; 11 / 12 arctan2_ref of the
// pairs (y, x) in float / double; 13 q_rsqrt of (float)x.
int pdt_host_math(int fn, const double *x, uint64_t n, double *out0, double *out1)
{
    if (!x || !out0) return PDT_ERR_ARG;
    for (uint64_t i = 0; i < n; i++) {
        switch (fn) {
        case 0: { double sv, cv; sincos_glibc(x[i], sv, cv); out0[i] = sv; if (out1) out1[i] = cv; break; }
        case 1: out0[i] = sin_glibc(x[i]); break;
        case 2: out0[i] = cos_glibc(x[i]); break;
        case 3: { float sf, cf; sincosf_glibc((float)x[i], sf, cf); out0[i] = sf; if (out1) out1[i] = cf; break; }
        case 4: out0[i] = hypot_glibc(x[2 * i], x[2 * i + 1]); break;
        case 5: out0[i] = hypotf_glibc((float)x[2 * i], (float)x[2 * i + 1]); break;
        case 6: { float sf, cf; sincosf_flat((float)x[i], sf, cf); out0[i] = sf; if (out1) out1[i] = cf; break; }
        case 7: out0[i] = pll_wrap_error_f32((float)x[i]); break;
        case 8: out0[i] = pll_wrap_phase_f32((float)x[i]); break;
        case 9: { const float v = (float)x[i]; out0[i] = ((double)v > M_PI) ? (float)((double)v - 2 * M_PI) : ((double)v < -M_PI) ? (float)((double)v + 2 * M_PI) : v; break; }
        case 10: out0[i] = (x[i] > M_PI) ? x[i] - 2 * M_PI : (x[i] < -M_PI) ? x[i] + 2 * M_PI : x[i]; break;
        case 11: out0[i] = arctan2_ref((float)x[2 * i], (float)x[2 * i + 1]); break;
        case 12: out0[i] = arctan2_ref(x[2 * i], x[2 * i + 1]); break;
        case 13: out0[i] = q_rsqrt((float)x[i]); break;
        default: return PDT_ERR_ARG;
        }
    }
    return PDT_OK;
}

int pdt_make_lpf(int mode, uint32_t sample_rate, void *taps_out, int *ntaps, int *interp)
{
    if (!sample_rate) return PDT_ERR_ARG;
    if (mode == PDT_MODE_ARGOS) {
        if (ntaps) *ntaps = 50;
        if (interp) *interp = 1;
        if (taps_out) make_lpf<double>((double *)taps_out, 50, 700.0, (double)sample_rate, 1);   // ARGOSdemod/main.c:248
        return PDT_OK;
    }
    const int ip = poes_interp(sample_rate);
    if (ip < 1) return PDT_ERR_RATE;
    const int N = 26 * ip;
    if (ntaps) *ntaps = N;
    if (interp) *interp = ip;
    if (taps_out) {
        const float Fs = (float)sample_rate;
        make_lpf<float>((float *)taps_out, N, (float)11000.0, Fs * (float)ip, ip);              // POESTIPdemod/main.c:369
    }
    return PDT_OK;
}

int pdt_wav_parse_header(const uint8_t h[44], uint32_t *sample_rate, uint32_t *channels, uint32_t *bits_per_sample,
                         uint32_t *format, uint32_t *data_bytes)
{
    if (!h) return PDT_ERR_ARG;
    auto r32 = [&](int o) { return (uint32_t)h[o] | ((uint32_t)h[o + 1] << 8) | ((uint32_t)h[o + 2] << 16) | ((uint32_t)h[o + 3] << 24); };
    auto r16 = [&](int o) { return (uint32_t)h[o] | ((uint32_t)h[o + 1] << 8); };
    if (format) *format = r16(20);
    if (channels) *channels = r16(22);
    if (sample_rate) *sample_rate = r32(24);
    if (bits_per_sample) *bits_per_sample = r16(34);
    if (data_bytes) *data_bytes = r32(40);
    return PDT_OK;
}

double pdt_time_axis(int mode, uint32_t sample_rate, uint64_t m)
{
    if (mode == PDT_MODE_ARGOS) {
        TimeAxis<double> ax;
        ax.init(1.0 / (double)sample_rate);
        return ax.at(m);
    }
    TimeAxis<float> ax;
    ax.init((float)(1.0 / (double)(float)sample_rate));
    return (double)ax.at(m);
}

int pdt_open(const pdt_config *cfg, pdt_ctx **out)
{
    if (!cfg || !out) return PDT_ERR_ARG;
    if (cfg->mode != PDT_MODE_POES && cfg->mode != PDT_MODE_ARGOS) return PDT_ERR_ARG;
    if (!cfg->sample_rate) return PDT_ERR_ARG;
    if (cfg->chain != PDT_CHAIN_FILE && cfg->chain != PDT_CHAIN_LIVE) return PDT_ERR_ARG;
    // (ARGOS + PDT_CHAIN_LIVE = the ARGOS sound-card twin: the FLOAT build of the ARGOS chain, ARGOSdemodPortAudio/config.h;
    // round 4)
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        fprintf(stderr, "libpdt: no HIP device available -- this library has no CPU path\n");
        return PDT_ERR_NOGPU;
    }
    if (cfg->device < 0 || cfg->device >= ndev) return PDT_ERR_ARG;
    HIP_TRY(hipSetDevice(cfg->device));
    pdt_ctx *ctx = new pdt_ctx();
    ctx->cfg = *cfg;
    ctx->tune.load();
    if (ctx->tune.pll_block && !ctx->cfg.pll_block) ctx->cfg.pll_block = (uint32_t)ctx->tune.pll_block;
    if (ctx->tune.pll_warm_s > 0 && !ctx->cfg.pll_warm) ctx->cfg.pll_warm = (uint32_t)(ctx->tune.pll_warm_s * cfg->sample_rate);
    if (ctx->tune.agc_warm_s > 0 && !ctx->cfg.agc_warm) ctx->cfg.agc_warm = (uint32_t)(ctx->tune.agc_warm_s * cfg->sample_rate);
    if (!ctx->cfg.chunk) ctx->cfg.chunk = (cfg->mode == PDT_MODE_ARGOS || cfg->chain == PDT_CHAIN_LIVE) ? 2400 : 10000;
    const bool argos_twin = cfg->mode == PDT_MODE_ARGOS && cfg->chain == PDT_CHAIN_LIVE;
    ctx->elem = (int)((cfg->mode == PDT_MODE_ARGOS && !argos_twin) ? sizeof(double) : sizeof(float));
    int nt = 0, ip = 0;
    int rc = pdt_make_lpf(cfg->mode, cfg->sample_rate, nullptr, &nt, &ip);
    if (rc) { pdt_close(ctx); return rc; }
    ctx->interp = (uint32_t)ip;
    ctx->ntaps = (uint32_t)nt;
    ctx->taps_host.resize((size_t)nt * ctx->elem);
    if (argos_twin)           // MakeLPFIR(filterCoeffs, 50, 700, Fs, 1) in float (ARGOSdemodPortAudio/main.c:264)
        make_lpf<float>((float *)ctx->taps_host.data(), 50, (float)700, (float)cfg->sample_rate, 1);
    else
    pdt_make_lpf(cfg->mode, cfg->sample_rate, ctx->taps_host.data(), nullptr, nullptr);
    if ((rc = ctx->taps.ensure(ctx->taps_host.size()))) { pdt_close(ctx); return rc; }
    if (hipMemcpy(ctx->taps.p, ctx->taps_host.data(), ctx->taps_host.size(), hipMemcpyHostToDevice) != hipSuccess) {
        pdt_close(ctx);
        return PDT_ERR_NOGPU;
    }
    if (cfg->mode == PDT_MODE_POES && nt == 26 * ip) {
        // tap table of the register-tiled FIR, rotated per ring residue: rot[c][t][r] = h[N-1-r-((c-t) mod K)*interp]
        const int K = 26, rs = ip;                  // rows of `interp` taps, one residue = K * interp consecutive floats
        const int cs = (K * rs + 15) & ~15;         // residue stride: every residue's block starts on a 64-byte boundary
        std::vector<float> rot((size_t)K * cs, 0.0f);
        const float *h = (const float *)ctx->taps_host.data();
        for (int c = 0; c < K; c++)
            for (int t = 0; t < K; t++)
                for (int r = 0; r < ip; r++) rot[(size_t)c * cs + (size_t)t * rs + r] = h[nt - 1 - r - ((c - t + K) % K) * ip];
        if ((rc = ctx->taps_rot.ensure(rot.size() * sizeof(float)))) { pdt_close(ctx); return rc; }
        if (hipMemcpy(ctx->taps_rot.p, rot.data(), rot.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
            pdt_close(ctx);
            return PDT_ERR_NOGPU;
        }
    }
    // (the two streams side by side: ~10 ms each, 20 for a process's first -- tools/probes/cold_path_probe.hip)
    std::thread side_stream_task;
    auto make_side_stream = [ctx]() {
        // the side stream at another priority than the main one: streams of one priority share a few hardware queues round
        // robin, and two streams that land on the same queue run one after the other (seen in a batch trace: the block-parallel
        // PLL kernel and the acquisition it should run beside, serialised); another priority is another set of queues
        if (hipSetDevice(ctx->cfg.device) != hipSuccess) { (void)hipGetLastError(); return; }
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (hipStreamCreateWithPriority(&ctx->stream2, hipStreamNonBlocking, greatest) != hipSuccess) {
            (void)hipGetLastError();
            if (hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); ctx->stream2 = nullptr; }
        }
    };
    try { side_stream_task = std::thread(make_side_stream); } catch (const std::exception &) { make_side_stream(); }
    auto join_side = [&]() { if (side_stream_task.joinable()) side_stream_task.join(); };     // (before the context goes away)
    if (hipStreamCreate(&ctx->stream) != hipSuccess) { ctx->stream = nullptr; join_side(); pdt_close(ctx); return PDT_ERR_NOGPU; }
    ctx->own_stream = true;
    {
        void *small = nullptr;
        if (timed_host_malloc((void **)&small, sizeof(DevScalars) + 128 + 32768) != hipSuccess) { join_side(); pdt_close(ctx); return PDT_ERR_NOMEM; }
        ctx->pend_sc = (DevScalars *)small;
        ctx->pend_info = (unsigned char *)small + ((sizeof(DevScalars) + 15) & ~(size_t)15);
        ctx->seg_pin = ctx->pend_info + 128;          // 4 KiB up (kept bits, history symbols, lock record, gain), the rest down (SegTail)
    }
    (void)hipEventCreate(&ctx->ev0);
    (void)hipEventCreate(&ctx->ev1);
    (void)hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming);
    (void)hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming);
    join_side();
    if (!ctx->stream2) { pdt_close(ctx); return PDT_ERR_NOGPU; }
    memset(&ctx->stats, 0, sizeof ctx->stats);
    memset(ctx->stage_len, 0, sizeof ctx->stage_len);
    ctx->axis_f.init((float)(1.0 / (double)(float)cfg->sample_rate));        // wave.c:96-97
    if (argos_twin) ctx->axis_f.init(1 / (float)cfg->sample_rate);           // "Time += (1/Fs)", all float (ARGOSdemodPortAudio/main.c:285)
    ctx->axis_d.init(1.0 / (double)cfg->sample_rate);
    ctx->counted = true;
    ingest_open_contexts().fetch_add(1);
    *out = ctx;
    return PDT_OK;
}

void pdt_close(pdt_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->cfg.device);
    DevBuf *bufs[] = { &ctx->pcm, &ctx->pll, &ctx->lock, &ctx->fir, &ctx->agc, &ctx->sym, &ctx->symidx, &ctx->bits, &ctx->bitsym,
                       &ctx->hits, &ctx->frames, &ctx->taps, &ctx->mag, &ctx->seams_pll, &ctx->seams_agc, &ctx->scal, &ctx->lockinfo,
                       &ctx->term, &ctx->seams_ema, &ctx->gtable, &ctx->gentries, &ctx->gcand,
                       &ctx->gmfirst, &ctx->stiles, &ctx->gsegmap, &ctx->gsegstart, &ctx->gbands, &ctx->gclist, &ctx->gspan_keys, &ctx->gspan_tails, &ctx->gspan_rows, &ctx->gspan_items, &ctx->gspan_ctl, &ctx->gspan_recs, &ctx->gspan_rep, &ctx->gspan_list2, &ctx->gspan_items2, &ctx->gspan_info, &ctx->gcentries, &ctx->gflags, &ctx->agc_maps, &ctx->pll_head, &ctx->taps_rot, &ctx->pll_scratch, &ctx->tip, &ctx->stream_in, &ctx->sync_scr, &ctx->agc_raw, &ctx->agc_ckpt, &ctx->pll_ckpt, &ctx->packs_dev, &ctx->seg_dev, &ctx->lt_theta, &ctx->lt_phi,
                       &ctx->avgph, &ctx->term_ap, &ctx->seams_q, &ctx->chunkinfo, &ctx->an_tab, &ctx->analytic, &ctx->halo.buf[0], &ctx->halo.buf[1],
                       &ctx->ddc_taps, &ctx->channel, &ctx->survey_win, &ctx->survey_tw, &ctx->survey_part, &ctx->survey_out,
                       &ctx->bursts_rows, &ctx->bursts_peaks, &ctx->bursts_counts, &ctx->win_table, &ctx->tone_table, &ctx->tone_out,
                       &ctx->staged_bits, &ctx->staged_iq, &ctx->argos_work, &ctx->ff_work, &ctx->ff_out, &ctx->ffp_work, &ctx->ffp_out,
                       &ctx->tip_sync_work, &ctx->tip_recs, &ctx->tip_repair_work, &ctx->tip_repair_soft, &ctx->tip_dcs_work, &ctx->tip_subcom_work };
    for (DevBuf *b : bufs) b->release();
    for (hipEvent_t e : ctx->event_pool) (void)hipEventDestroy(e);
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    if (ctx->qual_pin) (void)hipHostFree(ctx->qual_pin);
    if (ctx->packs_pin) (void)hipHostFree(ctx->packs_pin);
    ctx->ingest.release();
    if (ctx->pend_sc) (void)hipHostFree(ctx->pend_sc);
    for (auto &t : ctx->timers) { if (!t.shared_a) (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->counted) ingest_open_contexts().fetch_sub(1);
    delete ctx;
}

int pdt_set_stream(pdt_ctx *ctx, void *hip_stream)
{
    if (!ctx) return PDT_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->cfg.device));
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    ctx->own_stream = false;
    ctx->stream = (hipStream_t)hip_stream;
    if (!hip_stream) {
        if (hipStreamCreate(&ctx->stream) != hipSuccess) return PDT_ERR_NOGPU;
        ctx->own_stream = true;
    }
    return PDT_OK;
}

int pdt_set_loop_params(pdt_ctx *ctx, const pdt_loop_params *p)
{
    if (!ctx || !p) return PDT_ERR_ARG;
    if (ctx->stream_open) return PDT_ERR_STATE;
    const double v[] = { p->pll_freq_range_hz, p->pll_lock_threshold, p->pll_lock_alpha, p->pll_loopbw_acq, p->pll_loopbw_track, p->agc_attack,
                         p->agc_decay, p->gardner_baud, p->gardner_step_range, p->gardner_kp, p->manchester_threshold };
    for (double x : v)
        if (!(x >= 0.0) || !std::isfinite(x)) return PDT_ERR_ARG;
    if (p->gardner_baud != 0 && (double)ctx->cfg.sample_rate * (double)ctx->interp / p->gardner_baud < 2.0) return PDT_ERR_ARG;
    if (p->pll_freq_range_hz != 0 && p->pll_freq_range_hz >= 0.5 * (double)ctx->cfg.sample_rate) return PDT_ERR_ARG;
    if ((float)p->gardner_step_range > 0.1f) return PDT_ERR_ARG;      // (the samplers' window margins and symbol capacities are sized for the mains' 0.1)
    if (p->zero_mask & ~(uint32_t)(PDT_LP_ZERO_LOCK_THRESHOLD | PDT_LP_ZERO_GARDNER_KP | PDT_LP_ZERO_GARDNER_STEP_RANGE | PDT_LP_ZERO_MANCHESTER_THRESHOLD))
        return PDT_ERR_ARG;
    // a baud rate whose step would not fit the sequential samplers' LDS windows (a symbol and its mid-point must lie inside
    // one; the casts of the step to integers further down stay in range with it): at most 4 096 samples per symbol
    if (p->gardner_baud != 0 && !((double)ctx->cfg.sample_rate * (double)ctx->interp / p->gardner_baud <= 4096.0)) return PDT_ERR_ARG;
    ctx->lp = *p;
    ctx->gcand_key = -1;                    // (the sampler's candidate list depends on the step)
    return PDT_OK;
}

int pdt_keep_quality(pdt_ctx *ctx, int enable)
{
    if (!ctx) return PDT_ERR_ARG;
    ctx->keep_quality = enable != 0;
    if (!enable) ctx->chunk_host.clear();
    return PDT_OK;
}

uint64_t pdt_chunk_reports(const pdt_ctx *ctx, pdt_chunk_report *out, uint64_t max_chunks)
{
    if (!ctx) return 0;
    const uint64_t nc = ctx->chunk_host.size();
    if (!out) return nc;
    const uint64_t m = std::min<uint64_t>(nc, max_chunks);
    chunk_reports_range(ctx, 0, m, ctx->report_samples, out, nullptr);
    return m;
}

int pdt_set_progress(pdt_ctx *ctx, pdt_progress_fn fn, void *user)
{
    if (!ctx) return PDT_ERR_ARG;
    ctx->progress_fn = fn;
    ctx->progress_user = user;
    return PDT_OK;
}

int pdt_keep_pll(pdt_ctx *ctx, int enable)
{
    if (!ctx) return PDT_ERR_ARG;
    ctx->keep_pll = enable != 0;
    ctx->keep_pll_asked = enable != 0;
    return PDT_OK;
}

int pdt_keep_presquelch(pdt_ctx *ctx, int enable)
{
    if (!ctx) return PDT_ERR_ARG;
    ctx->keep_agc_raw = enable != 0;
    if (!enable) ctx->stage_len[PDT_ST_AGC_RAW] = 0;
    return PDT_OK;
}

static int demod_common(pdt_ctx *ctx, uint64_t nframes, int phase = RUN_ALL)
{
    if (phase == RUN_ALL) ctx->batch_hint = 1;
    HIP_TRY(hipSetDevice(ctx->cfg.device));
    ctx->n_samples = nframes;
    ctx->n_out = nframes * ctx->interp;
    ctx->stage_len[PDT_ST_ANALYTIC] = ctx->analytic_len;             // (a real capture's entry sets it just before; 0 otherwise)
    ctx->analytic_len = 0;
    if (phase != RUN_FINISH) {                                       // (a wideband capture's entry sets it just before; 0 otherwise)
        ctx->stage_len[PDT_ST_CHANNEL] = ctx->channel_len;
        ctx->channel_len = 0;
    }
    if (ctx->elem == 8) return run_capture<double>(ctx, nframes, phase);
    return run_capture<float>(ctx, nframes, phase);                 // POES, both twins
}

static int demod_overlapped(pdt_ctx *ctx, const IngestSrc &src, uint64_t nframes, const InFmt &f, int text_fd, uint64_t *text_bytes);
static int demod_windowed(pdt_ctx *ctx, const IngestSrc &src, uint64_t nframes, const InFmt &f, int text_fd, uint64_t *text_bytes, uint64_t piece);
static int demod_batch(pdt_ctx *const *ctxs, const void *const *iq_device, const uint64_t *nframes, int count, int fmt);
static uint64_t stream_history(const pdt_ctx *ctx);

// ---------------------------------------------------------------- the input front end: I,Q, real and wideband captures
// A host table on the device, once per key (*slot = the key of what the device holds, 0 = nothing).  A launch that reads the
// previous table may be in flight: synchronize before overwriting.
static int table_upload(pdt_ctx *ctx, const std::vector<float> &host, DevBuf &buf, int key, int *slot)
{
    *slot = 0;
    const int rc = buf.ensure(host.size() * sizeof(float) + 16);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(buf.p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    *slot = key;
    return PDT_OK;
}

// the rotation table (once per context), and with it the channel filter's taps (once per decimation)
static int real_table(pdt_ctx *ctx)
{
    if (ctx->an_tab_ready) return PDT_OK;
    std::vector<float> tab(2 * AN_TAB);
    analytic_table(tab.data());
    return table_upload(ctx, tab, ctx->an_tab, 1, &ctx->an_tab_ready);
}

static int channel_tables(pdt_ctx *ctx)
{
    const int rc = real_table(ctx);
    if (rc || ctx->ddc_taps_decim == ctx->ch_decim) return rc;
    return table_upload(ctx, ddc_taps(ctx->ch_decim), ctx->ddc_taps, ctx->ch_decim, &ctx->ddc_taps_decim);
}

static uint64_t channel_count(const pdt_ctx *ctx, uint64_t n) { return (n + (uint64_t)ctx->ch_decim - 1) / (uint64_t)ctx->ch_decim; }

// room for the channel stream of a whole wideband capture of n frames, and the tables
static int channel_prepare(pdt_ctx *ctx, uint64_t n)
{
    const int rc = ctx->channel.ensure((size_t)channel_count(ctx, n) * 8 + 16);
    return rc ? rc : channel_tables(ctx);
}

// the down-converter's record (pdt_ddc.h) of a conversion at ctx's offset: input 0 at x, [lo, hi) present, n_out pairs to out
static DdcWindow channel_record(const pdt_ctx *ctx, const void *x, long long lo, long long hi, uint64_t n_out, uint64_t g0, void *out)
{
    return DdcWindow{ x, out, lo, hi, (long long)n_out, ctx->ch_step, (uint32_t)g0, 0 };
}

// A whole capture resident at x, n frames of f: convert it if its kind has a converter, then the chain (real and wideband
// input: the RAW float path on the converter's pairs).
static int demod_resident(pdt_ctx *ctx, const void *x, uint64_t n, const InFmt &f)
{
    int rc;
    ctx->pcm_fmt = f.pcm_fmt;
    switch (f.kind) {
    case IN_IQ:
        ctx->pcm_dev = x;
        return demod_common(ctx, n);
    case IN_REAL:
        if ((rc = ctx->analytic.ensure((size_t)n * 8 + 16)) || (rc = real_table(ctx))) return rc;
        HIP_TRY(analytic_launch(ctx->stream, f.code, x, 0, (long long)n, n, 0, ctx->real_step, (const float *)ctx->an_tab.p, ctx->analytic.p));
        ctx->pcm_dev = ctx->analytic.p;
        ctx->analytic_len = n;
        return demod_common(ctx, n);
    case IN_WB: {
        if ((rc = channel_prepare(ctx, n))) return rc;
        const uint64_t m = channel_count(ctx, n);
        HIP_TRY(ddc_launch(ctx->stream, f.code, ctx->ch_decim, (const float *)ctx->ddc_taps.p, (const float *)ctx->an_tab.p,
                           channel_record(ctx, x, 0, (long long)n, m, 0, ctx->channel.p)));
        ctx->pcm_dev = ctx->channel.p;
        ctx->channel_len = m;
        return demod_common(ctx, m);
    }
    }
    return PDT_ERR_ARG;
}

// Does a capture of nframes fit the device in one piece?  The reference's chunk loop takes a file of any length in O(chunk)
// memory (POESTIPdemod/main.c:373, while(!feof)); the one-piece path here keeps every stage's stream of the whole capture
// resident -- about 8 x the file for POES at 250 ksps.  Returns 0 when that fits what the device has free (plus
// what this context already holds), otherwise the number of samples per piece of the bounded window (demod_windowed), or a
// negative error code when not even a window of a few chunks fits.
static long long window_piece_for(pdt_ctx *ctx, uint64_t nframes, size_t fb)
{
    const bool need_lock = ctx->cfg.mode == PDT_MODE_ARGOS || ctx->cfg.chain == PDT_CHAIN_LIVE;
    const double es = (double)ctx->elem, ip = (double)ctx->interp;
    // bytes per input sample: input, PLL output, theta / phases (their own buffers when the capture is taken in segments), filter
    // and AGC output, lock signal + its input term, the quality EMA's two streams, symbols / bits / tables (a few per cent)
    const double per = (double)fb + es * (3.0 + 2.5 * ip) + 8.0 + (need_lock ? 2.0 * es : 0.0) + (ctx->keep_quality ? 2.0 * es : 0.0) +
                       (ctx->keep_agc_raw ? es * ip : 0.0);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return 0; }
    // what the context already holds is its to re-use
    const DevBuf *held[] = { &ctx->pcm, &ctx->pll, &ctx->lock, &ctx->fir, &ctx->agc, &ctx->term, &ctx->stream_in, &ctx->lt_theta, &ctx->lt_phi,
                             &ctx->avgph, &ctx->term_ap, &ctx->agc_raw, &ctx->gtable, &ctx->sym, &ctx->symidx, &ctx->analytic };
    double avail = (double)free_b;
    for (const DevBuf *b : held) avail += (double)b->cap;
    if (ctx->tune.hbm_limit_mb > 0) avail = (double)ctx->tune.hbm_limit_mb * 1048576.0;
    const double need = per * (double)nframes + 256.0 * 1048576.0;
    if (need <= 0.92 * avail && !ctx->tune.window_piece) return 0;
    // the window: its history (PLL warm-ups) + one piece, with the growth margins of the stream's buffers
    const double per_win = 1.3 * per + 2.0 * es;
    const uint64_t chunk = ctx->cfg.chunk, hist = stream_history(ctx) + 2 * chunk;
    double piece = 0.5 * avail / per_win - (double)hist;
    piece = std::min(piece, 64.0 * 1048576.0);                        // (a piece is a few ms of GPU time: no need for more)
    if (ctx->tune.window_piece) piece = (double)ctx->tune.window_piece;
    if (!(piece >= 16.0 * (double)chunk)) return PDT_ERR_NOMEM;
    return (long long)((uint64_t)piece / chunk * chunk);
}

// a whole wideband capture of n frames beside what the chain keeps -- per channel sample: D input frames and the float pair
static bool channel_fits(pdt_ctx *ctx, uint64_t n, const InFmt &f)
{
    return window_piece_for(ctx, channel_count(ctx, n), (size_t)f.bytes * (size_t)ctx->ch_decim + 8) == 0;
}

// hour-long POES captures: the chain starts on the part of the capture that has arrived (demod_overlapped)
static bool overlap_ingest(const pdt_ctx *ctx, uint64_t nframes, size_t fb)
{
    // Round 5: on by default (PDT_NO_OVERLAP switches it off) -- the segments are cut where they can take the whole-capture
    // kernels and keep the per-chunk reports (demod_overlapped); 3.6 GB file to frame file 82-91 ms against 89-94 ms with the
    // capture ingested first (profiles/r5).  From 2.5 GiB on: every segment pays the block-parallel stages' latency floors again
    // (~7 ms), hidden only while the next segment's samples take longer than that to arrive -- 0.6 GB: 30.8 ms overlapped
    // against 21.3 ms, 1.2 GB: 40.7 / 37.3, 2.4 GB: 63.5 / 63.5, 3.0 GB: 75.2 / 76.5 (profiles/r5/e2e_ab_overlap_by_size.txt).
    if (ctx->keep_pll_asked) return false;           // the caller asked for the stage arrays of the whole capture
    return ctx->tune.overlap && ctx->cfg.mode == PDT_MODE_POES && ctx->cfg.sampler != PDT_SAMPLER_MM && ctx->cfg.chain != PDT_CHAIN_LIVE &&
           (size_t)nframes * fb >= ((size_t)(ctx->tune.overlap_min_mb > 0 ? ctx->tune.overlap_min_mb : 2560) << 20) && ctx->cfg.chunk > 0 &&
           nframes / ctx->cfg.chunk >= 64;
}

// A whole capture into ctx->pcm: room for it, the ingest, its host time in ctx->ingest_ms.  What the statistics say about it
// is the caller's decision (ingest_publish): a survey leaves the context's results as they are.
static int ingest_whole(pdt_ctx *ctx, const IngestSrc &src, size_t bytes)
{
    ctx->pcm_retaken();                                                       // (a search of host memory read this buffer)
    int rc = ctx->pcm.ensure(bytes + 16);
    if (rc) return rc;
    const auto t_in = std::chrono::steady_clock::now();
    if ((rc = ingest_capture(ctx, src, bytes, ctx->pcm.p))) return rc;
    ctx->ingest_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_in).count();
    return PDT_OK;
}

static void ingest_publish(pdt_ctx *ctx)
{
    ctx->stats.ingest_ms = ctx->ingest_ms;
    ctx->stats.ingest_direct = (uint32_t)ctx->ingest.was_direct;
    ctx->stats.ingest_numa_node = ctx->ingest.numa_node;
}

// One capture from host memory or a file, of any format the entry has let through: the bounded window when it does not fit
// (wideband input has none yet: PDT_ERR_NOMEM), overlapped segments for a large I,Q file, else ingest + convert + chain; the
// frame text when a text_fd was given.  PDT_ERR_FORMAT comes before PDT_ERR_STATE here, the order of pdt_demod_fd and
// pdt_demod_file; the entries from host memory answer an open stream before they come here (demod_host).
static int demod_src(pdt_ctx *ctx, const IngestSrc &src, uint64_t n, int format, int text_fd, uint64_t *text_bytes)
{
    const InFmt f = in_fmt(format);
    if (f.kind == IN_IQ && f.pcm_fmt && ctx->elem != 4) return PDT_ERR_FORMAT;       // ARGOSdemod/main.c:238-241: "RAW files not yet supported"
    if (ctx->stream_open || (f.kind == IN_WB && !ctx->ch_decim)) return PDT_ERR_STATE;   // pdt_stream_end / _begin resp. pdt_set_channel first
    HIP_TRY(hipSetDevice(ctx->cfg.device));
    if (f.kind == IN_WB) {
        if (!channel_fits(ctx, n, f)) return PDT_ERR_NOMEM;
    } else {
        // (a real capture's analytic stream is one more buffer of the capture's length; it is never taken in overlapped segments)
        const long long piece = window_piece_for(ctx, n, (size_t)f.bytes + (f.kind == IN_REAL ? 8 : 0));
        if (piece) return piece < 0 ? (int)piece : demod_windowed(ctx, src, n, f, text_fd, text_bytes, (uint64_t)piece);
        if (f.kind == IN_IQ && src.fd >= 0 && overlap_ingest(ctx, n, (size_t)f.bytes)) return demod_overlapped(ctx, src, n, f, text_fd, text_bytes);
    }
    int rc = ingest_whole(ctx, src, (size_t)n * (size_t)f.bytes);
    if (rc) return rc;
    rc = demod_resident(ctx, ctx->pcm.p, n, f);
    ingest_publish(ctx);
    if (rc || text_fd < 0) return rc;
    return pdt_write_frames(ctx, text_fd, text_bytes);
}

// the whole-capture entries from host memory and from device memory: each takes the formats of its kind only
static int demod_host(pdt_ctx *ctx, const void *host, uint64_t n, int format, int kind)
{
    if (!ctx || (!host && n) || in_fmt(format).kind != kind) return PDT_ERR_ARG;
    if (ctx->stream_open) return PDT_ERR_STATE;                      // (before PDT_ERR_FORMAT: pdt_demod_f32's order)
    IngestSrc src;
    src.mem = (const unsigned char *)host;
    return demod_src(ctx, src, n, format, -1, nullptr);
}

static int demod_device(pdt_ctx *ctx, const void *dev, uint64_t n, int format, int kind)
{
    const InFmt f = in_fmt(format);
    if (!ctx || (!dev && n) || f.kind != kind) return PDT_ERR_ARG;
    if (ctx->stream_open || (kind == IN_WB && !ctx->ch_decim)) return PDT_ERR_STATE;     // pdt_stream_end / _begin resp. pdt_set_channel first
    if (kind == IN_IQ && f.pcm_fmt && ctx->elem != 4) return PDT_ERR_FORMAT;
    HIP_TRY(hipSetDevice(ctx->cfg.device));
    return demod_resident(ctx, dev, n, f);
}

int pdt_demod_pcm16(pdt_ctx *ctx, const int16_t *iq_host, uint64_t nframes) { return demod_host(ctx, iq_host, nframes, PDT_FMT_PCM16, IN_IQ); }
int pdt_demod_f32(pdt_ctx *ctx, const float *iq_host, uint64_t nframes) { return demod_host(ctx, iq_host, nframes, PDT_FMT_F32, IN_IQ); }
int pdt_demod_real(pdt_ctx *ctx, const void *x_host, uint64_t n, int sample_format) { return demod_host(ctx, x_host, n, sample_format, IN_REAL); }
int pdt_demod_channel(pdt_ctx *ctx, const void *iq_host, uint64_t nframes, int sample_format) { return demod_host(ctx, iq_host, nframes, sample_format, IN_WB); }

int pdt_demod_device(pdt_ctx *ctx, const void *iq_device, uint64_t nframes) { return demod_device(ctx, iq_device, nframes, PDT_FMT_PCM16, IN_IQ); }
int pdt_demod_device_f32(pdt_ctx *ctx, const void *iq_device, uint64_t nframes) { return demod_device(ctx, iq_device, nframes, PDT_FMT_F32, IN_IQ); }
int pdt_demod_device_real(pdt_ctx *ctx, const void *x_device, uint64_t n, int sample_format) { return demod_device(ctx, x_device, n, sample_format, IN_REAL); }
int pdt_demod_device_channel(pdt_ctx *ctx, const void *iq_device, uint64_t nframes, int sample_format)
{
    return demod_device(ctx, iq_device, nframes, sample_format, IN_WB);
}

int pdt_demod_fd(pdt_ctx *ctx, int fd, uint64_t byte_offset, uint64_t nframes, int sample_format)
{
    if (!ctx || fd < 0 || in_fmt(sample_format).kind == IN_NONE) return PDT_ERR_ARG;
    IngestSrc src;
    src.fd = fd;
    src.off = byte_offset;
    return demod_src(ctx, src, nframes, sample_format, -1, nullptr);
}

int pdt_demod_file(pdt_ctx *ctx, int fd, uint64_t byte_offset, uint64_t nframes, int sample_format, int text_fd, uint64_t *text_bytes)
{
    if (text_bytes) *text_bytes = 0;
    if (!ctx || fd < 0 || text_fd < 0 || in_fmt(sample_format).kind == IN_NONE) return PDT_ERR_ARG;
    IngestSrc src;
    src.fd = fd;
    src.off = byte_offset;
    return demod_src(ctx, src, nframes, sample_format, text_fd, text_bytes);
}

int pdt_set_real_input(pdt_ctx *ctx, double center_hz)
{
    if (!ctx) return PDT_ERR_ARG;
    if (!(std::isfinite(center_hz) && center_hz >= 0.0 && center_hz < 0.5 * (double)ctx->cfg.sample_rate)) return PDT_ERR_ARG;
    if (ctx->stream_open) return PDT_ERR_STATE;
    ctx->real_center = center_hz;
    ctx->real_step = analytic_step(ctx->cfg.sample_rate, center_hz);
    return PDT_OK;
}

int pdt_set_channel(pdt_ctx *ctx, int decim, double offset_hz)
{
    if (!ctx || decim < DDC_MIN_DECIM || decim > DDC_MAX_DECIM) return PDT_ERR_ARG;
    const double in_rate = (double)decim * (double)ctx->cfg.sample_rate;
    if (!(std::isfinite(offset_hz) && std::fabs(offset_hz) < 0.5 * in_rate)) return PDT_ERR_ARG;
    if (ctx->stream_open) return PDT_ERR_STATE;
    ctx->ch_decim = decim;
    ctx->ch_offset = offset_hz;
    ctx->ch_step = ddc_step(in_rate, offset_hz);
    return PDT_OK;
}

// ---------------------------------------------------------------- several contexts on one capture: channels and windows
// Every context converts a window of the resident capture at an offset of its own, then the batched chain runs on the channel streams
// (the groups of the batch run on their leaders' streams: they start when the conversion is over).  windows: win[i] is context
// i's, which is tuned to its offset; otherwise (the channels entries) every context takes the whole capture at the offset it has.
// The windows of a call, many and short, are converted by one launch over a table of their tiles; whole captures by a launch
// each, record by value, on the first context's stream -- a capture has tiles enough to fill the device, and the table's 4 bytes
// a tile would be built and copied per call.  `forbid`: a context that may not be among ctxs (the holder of the capture).
static int demod_each(pdt_ctx *const *ctxs, int count, const pdt_window *win, bool windows, const void *iq_device, uint64_t nframes,
                      int sample_format, const pdt_ctx *forbid)
{
    const InFmt f = in_fmt(sample_format);
    if (count < 0 || (count && (!ctxs || (windows && !win))) || (!iq_device && nframes) || f.kind != IN_WB) return PDT_ERR_ARG;
    auto window_of = [&](int i) { return windows ? win[i] : pdt_window{ 0, nframes, ctxs[i]->ch_offset }; };
    for (int i = 0; i < count; i++) {
        if (!ctxs[i] || ctxs[i] == forbid) return PDT_ERR_ARG;
        if (ctxs[i]->stream_open || !ctxs[i]->ch_decim) return PDT_ERR_STATE;
        if (ctxs[i]->ch_decim != ctxs[0]->ch_decim || ctxs[i]->cfg.device != ctxs[0]->cfg.device) return PDT_ERR_ARG;
        for (int j = 0; j < i; j++)
            if (ctxs[j] == ctxs[i]) return PDT_ERR_ARG;               // one context per channel, per window
        // (channels: deliberately redundant -- a context's own offset has passed pdt_set_channel's test, the same one, the whole
        // capture is in range, and pdt_set_channel below sets what is set already: one loop for both entries)
        const pdt_window w = window_of(i);
        const double in_rate = (double)ctxs[i]->ch_decim * (double)ctxs[i]->cfg.sample_rate;
        if (!(std::isfinite(w.offset_hz) && std::fabs(w.offset_hz) < 0.5 * in_rate)) return PDT_ERR_ARG;
        if (w.nframes && (w.first_frame > nframes || w.nframes > nframes - w.first_frame)) return PDT_ERR_ARG;
    }
    if (!count) return PDT_OK;
    pdt_ctx *c0 = ctxs[0];
    HIP_TRY(hipSetDevice(c0->cfg.device));
    std::vector<DdcWindow> recs((size_t)count);
    std::vector<void *> outs((size_t)count);
    std::vector<uint64_t> lens((size_t)count);
    for (int i = 0; i < count; i++) {
        pdt_ctx *c = ctxs[i];
        const pdt_window w = window_of(i);
        int rc = pdt_set_channel(c, c->ch_decim, w.offset_hz);
        if (!rc) rc = i ? c->channel.ensure((size_t)channel_count(c, w.nframes) * 8 + 16) : channel_prepare(c0, w.nframes);
        if (rc) return rc;
        lens[(size_t)i] = channel_count(c, w.nframes);
        const void *x = w.nframes ? (const unsigned char *)iq_device + (size_t)w.first_frame * (size_t)f.bytes : (const unsigned char *)iq_device;
        recs[(size_t)i] = channel_record(c, x, 0, (long long)w.nframes, lens[(size_t)i], 0, outs[(size_t)i] = c->channel.p);
    }
    const float *taps = (const float *)c0->ddc_taps.p, *tab = (const float *)c0->an_tab.p;
    if (windows) {
        std::vector<unsigned char> table;
        const long long tiles = ddc_windows_table(c0->ch_decim, recs.data(), count, table);
        if (tiles < 0) return PDT_ERR_ARG;
        if (tiles) {
            // (the table of the previous call is no longer read: every call ends its conversion with a synchronize)
            const int rc = c0->win_table.ensure(table.size() + 16);
            if (rc) return rc;
            HIP_TRY(hipMemcpy(c0->win_table.p, table.data(), table.size(), hipMemcpyHostToDevice));
            HIP_TRY(ddc_windows_launch(c0->stream, sample_format, c0->ch_decim, taps, tab, c0->win_table.p, count, tiles));
        }
    } else {
        for (int i = 0; i < count; i++) HIP_TRY(ddc_launch(c0->stream, sample_format, c0->ch_decim, taps, tab, recs[(size_t)i]));
    }
    HIP_TRY(hipStreamSynchronize(c0->stream));
    for (int i = 0; i < count; i++) ctxs[i]->channel_len = lens[(size_t)i];
    return demod_batch(ctxs, (const void *const *)outs.data(), lens.data(), count, PDT_FMT_F32);
}

// the same for a capture in host memory: check, fit, ingest into the first context's input buffer -- timed but not published: the
// contexts of a batch report no ingest, as they never have
static int demod_each_host(pdt_ctx *const *ctxs, int count, const pdt_window *win, bool windows, const void *iq_host, uint64_t nframes,
                           int sample_format)
{
    const InFmt f = in_fmt(sample_format);
    if (count < 0 || (count && (!ctxs || (windows && !win))) || (!iq_host && nframes) || f.kind != IN_WB) return PDT_ERR_ARG;
    if (!count) return PDT_OK;
    pdt_ctx *c0 = ctxs[0];
    if (!c0) return PDT_ERR_ARG;
    if (c0->stream_open || !c0->ch_decim) return PDT_ERR_STATE;
    HIP_TRY(hipSetDevice(c0->cfg.device));
    if (!channel_fits(c0, nframes, f)) return PDT_ERR_NOMEM;
    IngestSrc src;
    src.mem = (const unsigned char *)iq_host;
    const int rc = ingest_whole(c0, src, (size_t)nframes * (size_t)f.bytes);
    return rc ? rc : demod_each(ctxs, count, win, windows, c0->pcm.p, nframes, sample_format, nullptr);
}

int pdt_demod_channels_device(pdt_ctx *const *ctxs, int count, const void *iq_device, uint64_t nframes, int sample_format)
{
    return demod_each(ctxs, count, nullptr, false, iq_device, nframes, sample_format, nullptr);
}

int pdt_demod_channels(pdt_ctx *const *ctxs, int count, const void *iq_host, uint64_t nframes, int sample_format)
{
    return demod_each_host(ctxs, count, nullptr, false, iq_host, nframes, sample_format);
}

int pdt_demod_windows_device(pdt_ctx *const *ctxs, int count, const pdt_window *win, const void *iq_device, uint64_t nframes, int sample_format)
{
    return demod_each(ctxs, count, win, true, iq_device, nframes, sample_format, nullptr);
}

int pdt_demod_windows(pdt_ctx *const *ctxs, int count, const pdt_window *win, const void *iq_host, uint64_t nframes, int sample_format)
{
    return demod_each_host(ctxs, count, win, true, iq_host, nframes, sample_format);
}

int pdt_demod_windows_held(pdt_ctx *holder, pdt_ctx *const *ctxs, int count, const pdt_window *win)
{
    if (!holder) return PDT_ERR_ARG;
    if (!holder->held_src) return PDT_ERR_STATE;
    for (int i = 0; i < count && ctxs; i++)
        if (ctxs[i] && ctxs[i]->cfg.device != holder->cfg.device) return PDT_ERR_ARG;    // (the capture lies in the holder's device's memory)
    return demod_each(ctxs, count, win, true, holder->held_src, holder->held_frames, holder->held_fmt, holder);
}

// ---------------------------------------------------------------- carrier survey (pdt_survey.h)
// window and twiddles under one key: it is set when both are on the device
static int survey_tables(pdt_ctx *ctx, int nfft)
{
    if (ctx->survey_tab_nfft == nfft) return PDT_OK;
    ctx->survey_tab_nfft = 0;
    int rc = ctx->survey_out.ensure((size_t)nfft * sizeof(float)), win_key = 0;
    if (!rc) rc = table_upload(ctx, survey_window(nfft), ctx->survey_win, nfft, &win_key);
    return rc ? rc : table_upload(ctx, survey_twiddles(nfft), ctx->survey_tw, nfft, &ctx->survey_tab_nfft);
}

// the mode's PLL frequency range: the default of a search's merge_hz (that of guard_hz is half the channel rate)
static double search_range_hz(const pdt_ctx *ctx)
{
    return ctx->lp.pll_freq_range_hz != 0 ? ctx->lp.pll_freq_range_hz : ctx->cfg.mode == PDT_MODE_ARGOS ? 550.0 : 4500.0;
}

// P = the averaged spectrum of the nseg whole segments from `first` on, a resident stretch: the survey's kernels into the survey's
// device buffers, read back.  Nothing of the context's demodulation state is touched.
static int search_spectrum(pdt_ctx *ctx, const unsigned char *first, const InFmt &f, uint64_t nseg, int nfft, std::vector<float> &P)
{
    int rc = survey_tables(ctx, nfft);
    if (!rc) rc = ctx->survey_part.ensure(survey_part_floats(nseg, nfft) * sizeof(float));
    if (rc) return rc;
    HIP_TRY(survey_launch(ctx->stream, f.code, first, nseg, nfft, (const float *)ctx->survey_win.p, (const float *)ctx->survey_tw.p,
                          (float *)ctx->survey_part.p, (float *)ctx->survey_out.p));
    P.resize((size_t)nfft);
    HIP_TRY(hipMemcpyAsync(P.data(), ctx->survey_out.p, P.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PDT_OK;
}

// x: the capture, resident
static int survey_resident(pdt_ctx *ctx, const void *x, const InFmt &f, const SurveyPlan &p, pdt_carrier *found, int *count)
{
    std::vector<float> P;
    const int rc = search_spectrum(ctx, (const unsigned char *)x + (size_t)p.first * (size_t)f.bytes, f, p.nseg, p.nfft, P);
    if (rc) return rc;
    ctx->survey_spec.swap(P);
    *count = survey_carriers(ctx->survey_spec.data(), p, (double)ctx->ch_decim * (double)ctx->cfg.sample_rate, found);
    return PDT_OK;
}

// All four entries of the survey and of the burst search.  plan(range): the search's plan from its cfg, the mode's range for the
// default of merge_hz; search(x, f): the search itself over the resident capture.  A capture in host memory goes where
// pdt_demod_channel would put it, whole -- the same condition on the device's memory -- and its ingest is not published: a search
// leaves the context's results and statistics unchanged.  The capture searched is the one pdt_demod_windows_held reads, once
// the search has succeeded.
static int search_any(pdt_ctx *ctx, const void *iq, bool resident, uint64_t nframes, int sample_format, bool results, bool bursts,
                      const std::function<int(double)> &plan, const std::function<int(const void *, const InFmt &)> &search)
{
    const InFmt f = in_fmt(sample_format);
    if (!ctx || !iq || f.kind != IN_WB || !results) return PDT_ERR_ARG;
    if (ctx->stream_open || !ctx->ch_decim) return PDT_ERR_STATE;
    int rc = plan(search_range_hz(ctx));
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->cfg.device));
    if (!resident) {
        if (!channel_fits(ctx, nframes, f)) return PDT_ERR_NOMEM;
        if (bursts) ctx->bursts_done = false;                               // (the rows of the last search: their capture may lie elsewhere)
        IngestSrc src;
        src.mem = (const unsigned char *)iq;
        if ((rc = ingest_whole(ctx, src, (size_t)nframes * (size_t)f.bytes))) return rc;
        iq = ctx->pcm.p;
    }
    ctx->held_src = nullptr;
    if ((rc = search(iq, f))) return rc;
    ctx->held_src = iq;
    ctx->held_frames = nframes;
    ctx->held_fmt = f.code;
    return PDT_OK;
}

static int survey_any(pdt_ctx *ctx, const void *iq, bool resident, uint64_t nframes, int sample_format, const pdt_survey_cfg *cfg, pdt_carrier *found,
                      int cap, int *count)
{
    SurveyPlan p;
    return search_any(ctx, iq, resident, nframes, sample_format, found && count, false,
                      [&](double range) { return survey_plan(cfg, range, (double)ctx->cfg.sample_rate, nframes, cap, &p); },
                      [&](const void *x, const InFmt &f) { return survey_resident(ctx, x, f, p, found, count); });
}

int pdt_survey_device(pdt_ctx *ctx, const void *iq_device, uint64_t nframes, int sample_format, const pdt_survey_cfg *cfg, pdt_carrier *found,
                      int cap, int *count)
{
    return survey_any(ctx, iq_device, true, nframes, sample_format, cfg, found, cap, count);
}

int pdt_survey(pdt_ctx *ctx, const void *iq_host, uint64_t nframes, int sample_format, const pdt_survey_cfg *cfg, pdt_carrier *found, int cap,
               int *count)
{
    return survey_any(ctx, iq_host, false, nframes, sample_format, cfg, found, cap, count);
}

int pdt_survey_spectrum(const pdt_ctx *ctx, float *out, int n)
{
    if (!ctx || !out) return PDT_ERR_ARG;
    if (ctx->survey_spec.empty()) return PDT_ERR_STATE;
    if (n < 0 || (size_t)n != ctx->survey_spec.size()) return PDT_ERR_ARG;
    memcpy(out, ctx->survey_spec.data(), ctx->survey_spec.size() * sizeof(float));
    return PDT_OK;
}

// ---------------------------------------------------------------- burst search (pdt_bursts.h)
// rows of a slab: what fits BURST_SLAB_BYTES (the developer switch PDT_BURST_SLAB_ROWS: that many)
static uint64_t bursts_slab_rows(const pdt_ctx *ctx, int nfft)
{
    if (ctx->tune.burst_slab_rows > 0) return (uint64_t)ctx->tune.burst_slab_rows;
    return std::max<uint64_t>(1, BURST_SLAB_BYTES / ((size_t)nfft * sizeof(float)));
}

// The waterfall of nrows rows from `first` on, at most `slab` rows at a time in bursts_rows (ensured here): after the launch of rows
// t0 .. t0 + nt - 1, each(t0, nt) does with them what the caller wants, the wait for the stream included.
static int waterfall_slabs(pdt_ctx *ctx, const unsigned char *first, const InFmt &f, int nfft, int rows_per, uint64_t nrows, uint64_t slab,
                           const std::function<int(uint64_t, uint64_t)> &each)
{
    int rc = ctx->bursts_rows.ensure((size_t)slab * (size_t)nfft * sizeof(float));
    if (rc) return rc;
    const size_t row_bytes = (size_t)rows_per * (size_t)nfft * (size_t)f.bytes;
    for (uint64_t t0 = 0; t0 < nrows; t0 += slab) {
        const uint64_t nt = std::min(slab, nrows - t0);
        HIP_TRY(waterfall_launch(ctx->stream, f.code, first + (size_t)t0 * row_bytes, nt, rows_per, nfft, (const float *)ctx->survey_win.p,
                                 (const float *)ctx->survey_tw.p, (float *)ctx->bursts_rows.p));
        if ((rc = each(t0, nt))) return rc;
    }
    return PDT_OK;
}

// x: the capture, resident.  The survey's kernels first, as they are, for the floor (into the survey's device buffers: the context's
// last survey spectrum lives on the host and stays); then slab by slab the rows and their peaks.  Nothing of the context's
// demodulation state is touched.
static int bursts_resident(pdt_ctx *ctx, const void *x, const InFmt &f, const BurstPlan &p, const SurveyPlan &sp, pdt_burst *found, int cap, int *count)
{
    ctx->bursts_done = false;
    const unsigned char *first = (const unsigned char *)x + (size_t)p.first * (size_t)f.bytes;
    std::vector<float> P;
    int rc = search_spectrum(ctx, first, f, sp.nseg, p.nfft, P);
    const uint64_t slab = std::min(bursts_slab_rows(ctx, p.nfft), p.nrows);
    if (!rc) rc = ctx->bursts_peaks.ensure((size_t)slab * BURST_ROW_PEAKS * sizeof(BurstPeak));
    if (!rc) rc = ctx->bursts_counts.ensure((size_t)slab * sizeof(int));
    if (rc) return rc;
    const double in_rate = (double)ctx->ch_decim * (double)ctx->cfg.sample_rate, floor = survey_floor(P.data(), p.nfft);
    const float level = burst_level(floor, p.threshold_db, p.rows_per);
    const int gb = burst_guard_bins(p.guard_hz, in_rate, p.nfft);
    // the rows' peaks come back a slab at a time and are kept compact on the host: a row's count and its found records only
    ctx->bursts_pk.clear();
    ctx->bursts_cnt.assign((size_t)p.nrows, 0);
    std::vector<pdt_row_peak> back((size_t)slab * BURST_ROW_PEAKS);
    rc = waterfall_slabs(ctx, first, f, p.nfft, p.rows_per, p.nrows, slab, [&](uint64_t t0, uint64_t nt) -> int {
        HIP_TRY(row_peaks_launch(ctx->stream, (const float *)ctx->bursts_rows.p, nt, p.nfft, level, gb, ctx->bursts_peaks.p, (int *)ctx->bursts_counts.p));
        HIP_TRY(hipMemcpyAsync(back.data(), ctx->bursts_peaks.p, (size_t)nt * BURST_ROW_PEAKS * sizeof(BurstPeak), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(&ctx->bursts_cnt[(size_t)t0], ctx->bursts_counts.p, (size_t)nt * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (uint64_t t = 0; t < nt; t++) {
            const int c = ctx->bursts_cnt[(size_t)(t0 + t)];
            if (c < 0 || c > BURST_ROW_PEAKS) return PDT_ERR_STATE;
            ctx->bursts_pk.insert(ctx->bursts_pk.end(), back.begin() + (size_t)t * BURST_ROW_PEAKS, back.begin() + (size_t)t * BURST_ROW_PEAKS + c);
        }
        return PDT_OK;
    });
    if (rc) return rc;
    *count = bursts_link(ctx->bursts_pk.data(), ctx->bursts_cnt.data(), true, p, floor, in_rate, found, cap);
    ctx->bursts_nfft = p.nfft;
    ctx->bursts_rows_per = p.rows_per;
    ctx->bursts_first = p.first;
    ctx->bursts_nrows = p.nrows;
    ctx->bursts_src = x;
    ctx->bursts_fmt = f.code;
    ctx->bursts_done = true;
    return PDT_OK;
}

static int bursts_any(pdt_ctx *ctx, const void *iq, bool resident, uint64_t nframes, int sample_format, const pdt_bursts_cfg *cfg, pdt_burst *found,
                      int cap, int *count)
{
    BurstPlan p;
    return search_any(ctx, iq, resident, nframes, sample_format, found && count, true,
                      [&](double range) -> int {
                          return bursts_plan(cfg, range, (double)ctx->cfg.sample_rate, (double)ctx->ch_decim * (double)ctx->cfg.sample_rate, nframes, cap, &p);
                      },
                      [&](const void *x, const InFmt &f) { return bursts_resident(ctx, x, f, p, bursts_survey_plan(p, cfg, nframes), found, cap, count); });
}

int pdt_bursts_device(pdt_ctx *ctx, const void *iq_device, uint64_t nframes, int sample_format, const pdt_bursts_cfg *cfg, pdt_burst *found,
                      int cap, int *count)
{
    return bursts_any(ctx, iq_device, true, nframes, sample_format, cfg, found, cap, count);
}

int pdt_bursts(pdt_ctx *ctx, const void *iq_host, uint64_t nframes, int sample_format, const pdt_bursts_cfg *cfg, pdt_burst *found, int cap,
               int *count)
{
    return bursts_any(ctx, iq_host, false, nframes, sample_format, cfg, found, cap, count);
}

int pdt_waterfall_rows(pdt_ctx *ctx, uint64_t first_row, uint64_t nrows, float *out)
{
    if (!ctx || !out) return PDT_ERR_ARG;
    if (!ctx->bursts_done) return PDT_ERR_STATE;
    struct { int nfft, rows_per; uint64_t first; } p = { ctx->bursts_nfft, ctx->bursts_rows_per, ctx->bursts_first };
    if (!nrows || first_row >= ctx->bursts_nrows || nrows > ctx->bursts_nrows - first_row) return PDT_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->cfg.device));
    const int rc = survey_tables(ctx, p.nfft);
    if (rc) return rc;
    const InFmt f = in_fmt(ctx->bursts_fmt);
    const size_t row_bytes = (size_t)p.rows_per * (size_t)p.nfft * (size_t)f.bytes;
    const unsigned char *first = (const unsigned char *)ctx->bursts_src + (size_t)p.first * (size_t)f.bytes + (size_t)first_row * row_bytes;
    const int log4 = survey_log4(p.nfft);
    const uint64_t slab = std::min(bursts_slab_rows(ctx, p.nfft), nrows);
    std::vector<float> place((size_t)slab * (size_t)p.nfft);
    return waterfall_slabs(ctx, first, f, p.nfft, p.rows_per, nrows, slab, [&](uint64_t t0, uint64_t nt) -> int {
        HIP_TRY(hipMemcpyAsync(place.data(), ctx->bursts_rows.p, (size_t)nt * (size_t)p.nfft * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (uint64_t t = 0; t < nt; t++)                                   // place i of a row holds bin survey_rev(i)
            for (int i = 0; i < p.nfft; i++)
                out[(size_t)(t0 + t) * (size_t)p.nfft + survey_rev((uint32_t)i, log4)] = place[(size_t)t * (size_t)p.nfft + (size_t)i];
        return PDT_OK;
    });
}

int pdt_burst_peaks(const pdt_ctx *ctx, uint64_t first_row, uint64_t nrows, pdt_row_peak *out, int *counts)
{
    if (!ctx || !out || !counts) return PDT_ERR_ARG;
    if (!ctx->bursts_done) return PDT_ERR_STATE;
    if (!nrows || first_row >= ctx->bursts_nrows || nrows > ctx->bursts_nrows - first_row) return PDT_ERR_ARG;
    size_t at = 0;
    for (uint64_t t = 0; t < first_row; t++) at += (size_t)ctx->bursts_cnt[(size_t)t];
    memset(out, 0, (size_t)nrows * BURST_ROW_PEAKS * sizeof(pdt_row_peak));
    for (uint64_t t = 0; t < nrows; t++) {
        const int c = counts[t] = ctx->bursts_cnt[(size_t)(first_row + t)];
        if (c) memcpy(out + (size_t)t * BURST_ROW_PEAKS, &ctx->bursts_pk[at], (size_t)c * sizeof(pdt_row_peak));
        at += (size_t)c;
    }
    return PDT_OK;
}

int pdt_bursts_shape(const pdt_ctx *ctx, int *nfft, int *rows_per, uint64_t *nrows)
{
    if (!ctx) return PDT_ERR_ARG;
    if (!ctx->bursts_done) return PDT_ERR_STATE;
    if (nfft) *nfft = ctx->bursts_nfft;
    if (rows_per) *rows_per = ctx->bursts_rows_per;
    if (nrows) *nrows = ctx->bursts_nrows;
    return PDT_OK;
}

// ---------------------------------------------------------------- second-pass entries: what they share
// Calls that read what a demodulation left on the device and run a few kernels of their own.  Their kernel times: CallTimer (pdt_rt.h);
// where their buffers' regions lie: pdt_work_layout.h; the rest is here.
enum { MODE_ANY = -1 };

// Context i of a call's list against those in front of it: there, of the mode asked for, on the first one's device (same_rate: and at
// its sample rate), and not in the list twice.  What fails here is PDT_ERR_ARG.
static bool list_arg_ok(pdt_ctx *const *ctxs, int i, int mode, bool same_rate)
{
    const pdt_ctx *c = ctxs[i];
    if (!c || (mode != MODE_ANY && c->cfg.mode != mode)) return false;
    if (c->cfg.device != ctxs[0]->cfg.device || (same_rate && c->cfg.sample_rate != ctxs[0]->cfg.sample_rate)) return false;
    for (int j = 0; j < i; j++)
        if (ctxs[j] == c) return false;
    return true;
}

// a whole-capture call has left a channel stream on the device
static bool channel_resident(const pdt_ctx *c) { return !c->stream_open && c->stage_len[PDT_ST_CHANNEL] && c->channel.p; }

// the whole capture's bits are on the device: a whole-capture call in one piece was the last to write them (stage-level calls and
// pdt_stream_begin zero every stage length; a piece of a capture or of a stream clears bits_whole)
static bool bits_resident(const pdt_ctx *c) { return c->bits_whole && !c->stream_open && c->stage_len[PDT_ST_FIR] != 0 && c->bit_time; }

// `count` elements of the host's in a buffer of the context's own, their count in front of them and the data 16 bytes in: nothing the
// context's results live in is touched.  Both copies are synchronous (the count is a local).
static int stage_counted(pdt_ctx *ctx, DevBuf &b, const void *host, uint64_t count, size_t elem_bytes)
{
    HIP_TRY(hipSetDevice(ctx->cfg.device));
    const int rc = b.ensure(16 + (size_t)count * elem_bytes);
    if (rc) return rc;
    const unsigned long long n = count;
    HIP_TRY(hipMemcpy(b.p, &n, sizeof n, hipMemcpyHostToDevice));
    if (count) HIP_TRY(hipMemcpy((unsigned char *)b.p + 16, host, (size_t)count * elem_bytes, hipMemcpyHostToDevice));
    return PDT_OK;
}

// ... and n I,Q pairs of the host's, likewise
static int stage_iq(pdt_ctx *ctx, DevBuf &b, const float *iq_host, uint64_t n)
{
    HIP_TRY(hipSetDevice(ctx->cfg.device));
    const int rc = b.ensure((size_t)n * 8 + 16);
    if (rc) return rc;
    if (n) HIP_TRY(hipMemcpy(b.p, iq_host, (size_t)n * 8, hipMemcpyHostToDevice));
    return PDT_OK;
}

// One bit stream of a call: where it is, where its count is (both on the device), what its buffers hold, how many records are wanted
struct BitJob {
    const unsigned char *bits;
    const unsigned long long *nbits_dev;
    const unsigned *bitsym;
    const long long *symidx;
    long long bit_cap;
    int cap;
};

// ... the bits a context's demodulation left (bits_resident)
static BitJob job_resident(const pdt_ctx *c, int cap)
{
    const uint64_t nb = c->stage_len[PDT_ST_BITS];              // (what the host read back; the kernels read the device's own count)
    return BitJob{ (const unsigned char *)c->bits.p, &((const DevScalars *)c->scal.p)->nbits, (const unsigned *)c->bitsym.p, (const long long *)c->symidx.p,
                   nb && c->bits.p && c->scal.p ? (long long)nb : 0, cap };
}

// ... the bits of a feed-forward result buffer (FfOut, FfpOut: the count in front, the tail t), on the device's own count
static BitJob job_result(const void *buf, const BitsTail &t, uint64_t bit_cap, int cap)
{
    const unsigned char *p = (const unsigned char *)buf;
    return BitJob{ p + t.o_bits, (const unsigned long long *)p, (const unsigned *)(p + t.o_sym), (const long long *)(p + t.o_idx), (long long)bit_cap, cap };
}

// ... a string that stage_counted has brought up
static BitJob job_staged(const DevBuf &b, uint64_t nbits, int cap)
{
    return BitJob{ (const unsigned char *)b.p + 16, (const unsigned long long *)b.p, nullptr, nullptr, (long long)nbits, cap };
}

// The room every stream's records take -- at most one per min_gap bits, at most the cap: stream i's from at[i] on -- and its tiles;
// the sum of the tiles
static long long job_rooms(const std::vector<BitJob> &jobs, long long min_gap, long long tile, std::vector<size_t> &at, std::vector<long long> &tiles)
{
    at.assign(jobs.size() + 1, 0);
    tiles.resize(jobs.size());
    long long ntiles = 0;
    for (size_t i = 0; i < jobs.size(); i++) {
        at[i + 1] = at[i] + (size_t)std::min<long long>(jobs[i].cap, jobs[i].bit_cap / min_gap + 1);
        ntiles += tiles[i] = (jobs[i].bit_cap + tile - 1) / tile;
    }
    return ntiles;
}

extern "C++" {      // (templates: this part of the file lies inside extern "C")
// What a run read back in one copy (`back`: the records of all streams side by side at o_rec, their counts at o_cnt) into the
// run's results: recs holds stream i's records from at[i] on, found[i] of them counted, min(found[i], room) present
template <typename Rec> static void unpack_back(const unsigned char *back, size_t o_rec, size_t o_cnt, size_t nrec, size_t n, std::vector<Rec> &recs,
                                                std::vector<unsigned> &found)
{
    recs.resize(nrec);
    if (nrec) memcpy(recs.data(), back + o_rec, nrec * sizeof(Rec));
    found.resize(n);
    if (n) memcpy(found.data(), back + o_cnt, n * sizeof(unsigned));
}

// the time stamp of stream i's source index; an empty one leaves the records' time as the kernels wrote it (the stage entries)
typedef std::function<double(size_t, long long)> TimeOf;

// Stream i's records of a run to the caller (out, and info_out where both it and infos are there: room for the stream's cap), stamped;
// returns the number found, which may exceed the number present
template <typename Rec, typename Info = char>
static int deliver(const std::vector<Rec> &recs, const std::vector<size_t> &at, const std::vector<unsigned> &found, size_t i, const TimeOf &time_of, void *out,
                   const std::vector<Info> *infos = nullptr, void *info_out = nullptr)
{
    const size_t have = std::min<size_t>(found[i], at[i + 1] - at[i]);
    for (size_t k = 0; k < have; k++) {
        Rec m = recs[at[i] + k];
        if (time_of) m.time = time_of(i, m.time_src);
        memcpy((unsigned char *)out + k * sizeof m, &m, sizeof m);
        if (infos && info_out) memcpy((unsigned char *)info_out + k * sizeof(Info), &(*infos)[at[i] + k], sizeof(Info));
    }
    return (int)found[i];
}
}  // extern "C++"

// ---------------------------------------------------------------- carrier measurement (pdt_tone.h)
// k_tones over a table of segments that share p's geometry (nfft, the noise bins), through c0's tables, buffers and stream: the table
// up, one launch, the raw records back, one synchronize (the table of the previous call is no longer read: every call ends with one);
// then the window's sums, once per context and NFFT.  timer (may be NULL): a profiled c0's kernel times gain k_tones.
static int tones_measure(pdt_ctx *c0, const TonePlan &p, const std::vector<ToneSeg> &table, std::vector<ToneRaw> &raw, CallTimer *timer)
{
    raw.resize(table.size());
    if (!table.empty()) {
        int rc = survey_tables(c0, p.nfft);
        if (!rc) rc = c0->tone_table.ensure(table.size() * sizeof(ToneSeg));
        if (!rc) rc = c0->tone_out.ensure(table.size() * sizeof(ToneRaw));
        if (rc) return rc;
        HIP_TRY(hipMemcpy(c0->tone_table.p, table.data(), table.size() * sizeof(ToneSeg), hipMemcpyHostToDevice));
        if (timer) HIP_TRY(timer->begin());
        HIP_TRY(tones_launch(c0->stream, p.nfft, c0->tone_table.p, table.size(), p.noise_lo, p.noise_hi, (const float *)c0->survey_win.p,
                             (const float *)c0->survey_tw.p, c0->tone_out.p));
        if (timer) HIP_TRY(timer->end());
        HIP_TRY(hipMemcpyAsync(raw.data(), c0->tone_out.p, raw.size() * sizeof(ToneRaw), hipMemcpyDeviceToHost, c0->stream));
        HIP_TRY(hipStreamSynchronize(c0->stream));
        if (timer) timer->commit();
    }
    if (c0->tone_sum_nfft != p.nfft) {
        tone_sums(p.nfft, &c0->tone_sw, &c0->tone_sw2);
        c0->tone_sum_nfft = p.nfft;
    }
    return PDT_OK;
}

// The segments of all contexts of a call in one launch over a table on the device, as the windows of a call are converted
// (ddc_windows_launch): the first context supplies stream, tables and the two device buffers.  Every context is checked before
// anything runs.  Nothing of any context's demodulation state is touched; a profiled first context's kernel times gain k_tones.
int pdt_tones_batch(pdt_ctx *const *ctxs, int count, const pdt_tone_cfg *cfg, pdt_tone *out, int cap_each, int *counts)
{
    if (count < 0 || (count && (!ctxs || !out || !counts))) return PDT_ERR_ARG;
    std::vector<TonePlan> plans((size_t)count);
    for (int i = 0; i < count; i++) {
        if (!list_arg_ok(ctxs, i, MODE_ANY, true)) return PDT_ERR_ARG;
        const pdt_ctx *c = ctxs[i];
        if (!channel_resident(c)) return PDT_ERR_STATE;
        const int rc = tone_plan(cfg, (double)c->cfg.sample_rate, search_range_hz(c), c->stage_len[PDT_ST_CHANNEL], cap_each, &plans[(size_t)i]);
        if (rc) return rc;
    }
    if (!count) return PDT_OK;
    pdt_ctx *c0 = ctxs[0];
    std::vector<ToneSeg> table;
    for (int i = 0; i < count; i++) {
        const TonePlan &p = plans[(size_t)i];
        for (uint64_t k = 0; k < p.nseg; k++)
            table.push_back(ToneSeg{ ctxs[i]->channel.p, (long long)(p.first + k * p.stride), (int32_t)table.size(), p.kmax });
    }
    if (table.size() > 0x7fffffffu) return PDT_ERR_ARG;
    if (!table.empty()) HIP_TRY(hipSetDevice(c0->cfg.device));
    static const char *const names[1] = { "k_tones" };
    CallTimer timer(c0, c0->stream, names, nullptr, 1);
    std::vector<ToneRaw> raw;
    const int rc = tones_measure(c0, plans[0], table, raw, &timer);
    if (rc) return rc;
    size_t at = 0;
    for (int i = 0; i < count; i++) {
        const TonePlan &p = plans[(size_t)i];
        tones_derive(raw.data() + at, p, (double)ctxs[i]->cfg.sample_rate, ctxs[i]->ch_offset, c0->tone_sw, c0->tone_sw2, out + (size_t)i * (size_t)cap_each);
        counts[i] = (int)p.nseg;
        at += (size_t)p.nseg;
    }
    return PDT_OK;
}

int pdt_tones(pdt_ctx *ctx, const pdt_tone_cfg *cfg, pdt_tone *out, int cap, int *count)
{
    if (!ctx || !out || !count) return PDT_ERR_ARG;
    return pdt_tones_batch(&ctx, 1, cfg, out, cap, count);
}

// ---------------------------------------------------------------- ARGOS messages (pdt_argos_msg.h)
// The streams of a call through one launch of each kernel over a table on the device, as the segments of pdt_tones are measured: the first
// context supplies stream and work buffer (ArgosWork).  recs: stream i's records from at[i] on, found[i] of them counted, min(found[i],
// room) present.
static int argos_run(pdt_ctx *c0, const std::vector<BitJob> &jobs, int K, int rule, std::vector<ArgosMsg> &recs, std::vector<size_t> &at,
                     std::vector<unsigned> &found)
{
    const size_t n = jobs.size();
    std::vector<ArgosCtx> table(n);
    std::vector<long long> tiles;
    // accepted messages lie at least 65 bits apart (a head's first bit behind a body of 52 bits or more; rule 1: spans do not overlap)
    const long long ntiles = job_rooms(jobs, 65, ARGOS_MSG_TILE, at, tiles);
    if (ntiles > 0x7fffffffll) return PDT_ERR_ARG;
    const ArgosWork L = argos_work_layout(n, at[n], (size_t)ntiles, sizeof(ArgosMsg), sizeof(ArgosCtx), ARGOS_MSG_WORDS * 8);
    HIP_TRY(hipSetDevice(c0->cfg.device));
    int rc;
    if ((rc = c0->argos_work.ensure(L.total))) return rc;
    unsigned char *w = (unsigned char *)c0->argos_work.p;
    long long t0 = 0;
    for (size_t i = 0; i < n; i++) {
        ArgosCtx &r = table[i];
        r.bits = jobs[i].bits;
        r.nbits = jobs[i].nbits_dev;
        r.bitsym = jobs[i].bitsym;
        r.symidx = jobs[i].symidx;
        r.cand = (unsigned long long *)(w + L.o_cand) + (size_t)t0 * ARGOS_MSG_WORDS;
        r.tile_any = (unsigned *)(w + L.o_any) + t0;
        r.out = (ArgosMsg *)(w + L.o_rec) + at[i];
        r.count = (unsigned *)(w + L.o_cnt) + i;
        r.bit_cap = jobs[i].bit_cap;
        r.cap = (int)(at[i + 1] - at[i]);
        r.first_tile = (int)t0;
        t0 += tiles[i];
    }
    // (the table of the previous call is no longer read: every call ends with a synchronize)
    HIP_TRY(hipMemcpy(w + L.o_tab, table.data(), n * sizeof(ArgosCtx), hipMemcpyHostToDevice));
    static const char *const names[2][2] = { { "k_argos_msgs", "k_argos_finish" }, { "k_argos_heads", "k_argos_pick" } };
    CallTimer timer(c0, c0->stream, names[rule == ARGOS_RULE_BEST], nullptr, 2);
    HIP_TRY(timer.begin());
    HIP_TRY(argos_msgs_launch(c0->stream, w + L.o_tab, (int)n, ntiles, K, rule, timer.inner()));
    HIP_TRY(timer.end());
    std::vector<unsigned char> back(L.o_tab);
    HIP_TRY(hipMemcpyAsync(back.data(), w, L.o_tab, hipMemcpyDeviceToHost, c0->stream));
    HIP_TRY(hipStreamSynchronize(c0->stream));
    timer.commit();
    unpack_back(back.data(), L.o_rec, L.o_cnt, at[n], n, recs, found);
    return PDT_OK;
}

// the jobs through argos_run; stream i's records to out + i * cap_each, its count to counts[i]
static int argos_deliver(pdt_ctx *c0, const std::vector<BitJob> &jobs, int K, int rule, const TimeOf &time_of, pdt_argos_msg *out, int cap_each, int *counts)
{
    std::vector<ArgosMsg> recs;
    std::vector<size_t> at;
    std::vector<unsigned> found;
    const int rc = argos_run(c0, jobs, K, rule, recs, at, found);
    if (rc) return rc;
    for (size_t i = 0; i < jobs.size(); i++) counts[i] = deliver(recs, at, found, i, time_of, out + i * (size_t)cap_each);
    return PDT_OK;
}

int pdt_argos_messages_batch(pdt_ctx *const *ctxs, int count, const pdt_argos_cfg *cfg, pdt_argos_msg *out, int cap_each, int *counts)
{
    int K, rule;
    if (count < 0 || cap_each < 0 || (count && (!ctxs || !counts || (!out && cap_each))) || argos_min_run(cfg, &K, &rule)) return PDT_ERR_ARG;
    for (int i = 0; i < count; i++)
        if (!list_arg_ok(ctxs, i, PDT_MODE_ARGOS, false)) return PDT_ERR_ARG;
    for (int i = 0; i < count; i++)
        if (!bits_resident(ctxs[i])) return PDT_ERR_STATE;
    if (!count) return PDT_OK;
    try {
        std::vector<BitJob> jobs;
        for (int i = 0; i < count; i++) jobs.push_back(job_resident(ctxs[i], cap_each));
        return argos_deliver(ctxs[0], jobs, K, rule, [&](size_t i, long long src) { return ctxs[i]->bit_time(src); }, out, cap_each, counts);
    } catch (const std::exception &) { return PDT_ERR_NOMEM; }
}

int pdt_argos_messages(pdt_ctx *ctx, const pdt_argos_cfg *cfg, pdt_argos_msg *out, int cap, int *count)
{
    if (!ctx || !count) return PDT_ERR_ARG;
    return pdt_argos_messages_batch(&ctx, 1, cfg, out, cap, count);
}

int pdt_stage_argos_messages(pdt_ctx *ctx, const uint8_t *bits_host, uint64_t nbits, const pdt_argos_cfg *cfg, pdt_argos_msg *out, int cap, int *count)
{
    int K, rule;
    if (!ctx || (!bits_host && nbits) || nbits >= (1ull << 31) || cap < 0 || (!out && cap) || !count || argos_min_run(cfg, &K, &rule)) return PDT_ERR_ARG;
    if (ctx->cfg.mode != PDT_MODE_ARGOS) return PDT_ERR_ARG;
    if (ctx->stream_open) return PDT_ERR_STATE;
    const int rc = stage_counted(ctx, ctx->staged_bits, bits_host, nbits, 1);
    if (rc) return rc;
    try {
        return argos_deliver(ctx, std::vector<BitJob>(1, job_staged(ctx->staged_bits, nbits, cap)), K, rule, TimeOf(), out, cap, count);
    } catch (const std::exception &) { return PDT_ERR_NOMEM; }
}

// ---------------------------------------------------------------- flywheel frame synchroniser (pdt_tip_sync.h)
// The streams of a call through one launch of each kernel over a table on the device, as argos_run does it: the first context supplies
// stream and work buffer (TipSyncWork).  recs / infos: stream i's records from at[i] on, found[i] of them counted, min(found[i], room)
// present.
static int tip_sync_run(pdt_ctx *c0, const std::vector<BitJob> &jobs, TipSyncRule R, std::vector<TipSyncRec> &recs, std::vector<TipSyncInfo> &infos,
                        std::vector<size_t> &at, std::vector<unsigned> &found)
{
    const size_t n = jobs.size();
    std::vector<TipSyncCtx> table(n);
    std::vector<long long> tiles;
    const long long ntiles = job_rooms(jobs, TIP_SYNC_MIN_GAP, TIP_SYNC_TILE, at, tiles);        // (emitted heads lie at least 829 bits apart)
    if (ntiles > 0x7fffffffll) return PDT_ERR_ARG;
    const TipSyncWork L = tip_sync_work_layout(n, at[n], (size_t)ntiles, sizeof(TipSyncRec), sizeof(TipSyncInfo), sizeof(TipSyncCtx), TIP_SYNC_WORDS * 8);
    HIP_TRY(hipSetDevice(c0->cfg.device));
    int rc;
    if ((rc = c0->tip_sync_work.ensure(L.total))) return rc;
    unsigned char *w = (unsigned char *)c0->tip_sync_work.p;
    long long t0 = 0;
    for (size_t i = 0; i < n; i++) {
        TipSyncCtx &r = table[i];
        auto map = [&](int k) { return (unsigned long long *)(w + L.o_maps + (size_t)k * L.map_bytes) + (size_t)t0 * TIP_SYNC_WORDS; };
        r.bits = jobs[i].bits;
        r.nbits = jobs[i].nbits_dev;
        r.bitsym = jobs[i].bitsym;
        r.symidx = jobs[i].symidx;
        r.packed = map(0);
        r.cand[0] = map(1);
        r.cand[1] = map(2);
        r.head[0] = map(3);
        r.head[1] = map(4);
        r.emit = map(5);
        r.tile_cnt = (unsigned *)(w + L.o_tcnt) + t0;
        r.tile_off = (unsigned *)(w + L.o_toff) + t0;
        r.out = (TipSyncRec *)(w + L.o_rec) + at[i];
        r.info = (TipSyncInfo *)(w + L.o_info) + at[i];
        r.count = (unsigned *)(w + L.o_cnt) + i;
        r.bit_cap = jobs[i].bit_cap;
        r.cap = (int)(at[i + 1] - at[i]);
        r.first_tile = (int)t0;
        t0 += tiles[i];
    }
    // (the table of the previous call is no longer read: every call ends with a synchronize)
    HIP_TRY(hipMemcpy(w + L.o_tab, table.data(), n * sizeof(TipSyncCtx), hipMemcpyHostToDevice));
    CallTimer timer(c0, c0->stream, tip_sync_kernel_names, nullptr, 5);
    HIP_TRY(timer.begin());
    HIP_TRY(tip_sync_launch(c0->stream, w + L.o_tab, (int)n, ntiles, R, timer.inner()));
    HIP_TRY(timer.end());
    std::vector<unsigned char> back(L.o_tab);
    HIP_TRY(hipMemcpyAsync(back.data(), w, L.o_tab, hipMemcpyDeviceToHost, c0->stream));
    HIP_TRY(hipStreamSynchronize(c0->stream));
    timer.commit();
    unpack_back(back.data(), L.o_rec, L.o_cnt, at[n], n, recs, found);
    infos.resize(at[n]);
    if (at[n]) memcpy(infos.data(), back.data() + L.o_info, at[n] * sizeof(TipSyncInfo));
    return PDT_OK;
}

// the jobs through tip_sync_run; stream i's records to out + i * cap_each (its info records to info + i * cap_each where info is
// there), its count to counts[i]
static int tip_sync_deliver(pdt_ctx *c0, const std::vector<BitJob> &jobs, TipSyncRule R, const TimeOf &time_of, pdt_frame *out, pdt_tip_sync_info *info,
                            int cap_each, int *counts)
{
    std::vector<TipSyncRec> recs;
    std::vector<TipSyncInfo> infos;
    std::vector<size_t> at;
    std::vector<unsigned> found;
    const int rc = tip_sync_run(c0, jobs, R, recs, infos, at, found);
    if (rc) return rc;
    for (size_t i = 0; i < jobs.size(); i++)
        counts[i] = deliver(recs, at, found, i, time_of, out + i * (size_t)cap_each, &infos, info ? info + i * (size_t)cap_each : nullptr);
    return PDT_OK;
}

int pdt_tip_sync_batch(pdt_ctx *const *ctxs, int count, const pdt_tip_sync_cfg *cfg, pdt_frame *out, pdt_tip_sync_info *info, int cap_each, int *counts)
{
    TipSyncRule R;
    if (count < 0 || cap_each < 0 || (count && (!ctxs || !counts || (!out && cap_each))) || tip_sync_rule(cfg, &R)) return PDT_ERR_ARG;
    for (int i = 0; i < count; i++)
        if (!list_arg_ok(ctxs, i, PDT_MODE_POES, false)) return PDT_ERR_ARG;
    for (int i = 0; i < count; i++)
        if (!bits_resident(ctxs[i])) return PDT_ERR_STATE;
    if (!count) return PDT_OK;
    try {
        std::vector<BitJob> jobs;
        for (int i = 0; i < count; i++) jobs.push_back(job_resident(ctxs[i], cap_each));
        return tip_sync_deliver(ctxs[0], jobs, R, [&](size_t i, long long src) { return ctxs[i]->bit_time(src); }, out, info, cap_each, counts);
    } catch (const std::exception &) { return PDT_ERR_NOMEM; }
}

int pdt_tip_sync(pdt_ctx *ctx, const pdt_tip_sync_cfg *cfg, pdt_frame *out, pdt_tip_sync_info *info, int cap, int *count)
{
    if (!ctx || !count) return PDT_ERR_ARG;
    return pdt_tip_sync_batch(&ctx, 1, cfg, out, info, cap, count);
}

int pdt_stage_tip_sync(pdt_ctx *ctx, const uint8_t *bits_host, uint64_t nbits, const pdt_tip_sync_cfg *cfg, pdt_frame *out, pdt_tip_sync_info *info,
                       int cap, int *count)
{
    TipSyncRule R;
    if (!ctx || (!bits_host && nbits) || nbits >= (1ull << 31) || cap < 0 || (!out && cap) || !count || tip_sync_rule(cfg, &R)) return PDT_ERR_ARG;
    if (ctx->cfg.mode != PDT_MODE_POES) return PDT_ERR_ARG;
    if (ctx->stream_open) return PDT_ERR_STATE;
    const int rc = stage_counted(ctx, ctx->staged_bits, bits_host, nbits, 1);
    if (rc) return rc;
    try {
        return tip_sync_deliver(ctx, std::vector<BitJob>(1, job_staged(ctx->staged_bits, nbits, cap)), R, TimeOf(), out, info, cap, count);
    } catch (const std::exception &) { return PDT_ERR_NOMEM; }
}

// ---------------------------------------------------------------- feed-forward bits (pdt_ff.h)
// One stream of a call: the context whose result buffers take its bits, where it is (device), its samples, the search range of its tone
struct FfJob {
    pdt_ctx *owner;
    const float *y;
    uint64_t n;
    double range_hz;
};

// The carrier of every stream: the first segment of pdt_tones at its defaults, all streams in one launch of k_tones through the first
// context's tables and buffers (tones_measure); the frequency is derived here, on the host, in double.  A stream without a whole
// segment, a rate without an allowed segment length and a record that is not valid leave residual 0 and valid 0.
static int ff_tones(pdt_ctx *c0, const std::vector<FfJob> &jobs, uint32_t rate, std::vector<double> &residual, std::vector<int> &valid)
{
    const size_t n = jobs.size();
    std::vector<ToneSeg> table;
    std::vector<int> rec(n, -1);
    TonePlan plan;
    memset(&plan, 0, sizeof plan);
    for (size_t i = 0; i < n; i++) {
        TonePlan p;
        if (tone_plan(nullptr, (double)rate, jobs[i].range_hz, jobs[i].n, 1, &p) != PDT_OK || !p.nseg) continue;
        rec[i] = (int)table.size();
        table.push_back(ToneSeg{ jobs[i].y, (long long)p.first, rec[i], p.kmax });
        plan = p;
    }
    if (table.empty()) return PDT_OK;
    std::vector<ToneRaw> raw;
    const int rc = tones_measure(c0, plan, table, raw, nullptr);
    if (rc) return rc;
    plan.nseg = 1;
    for (size_t i = 0; i < n; i++) {
        if (rec[i] < 0) continue;
        pdt_tone t;
        tones_derive(&raw[(size_t)rec[i]], plan, (double)rate, 0.0, c0->tone_sw, c0->tone_sw2, &t);
        if (t.valid) {
            residual[i] = t.residual_hz;
            valid[i] = 1;
        }
    }
    return PDT_OK;
}

// The streams of a call through one launch of each kernel over a table on the device: the first context supplies stream, rotation table
// and the work buffer (FfWork); every stream's bits, count and record go to its owner's buffer (FfOut) and stay there.  syncs (may be
// NULL): the records, which k_ff_pick also leaves side by side in the work buffer, read back in one copy before the one synchronize
// that ends the call.
static int ff_run(pdt_ctx *c0, const std::vector<FfJob> &jobs, uint32_t rate, const pdt_ff_cfg *cfg, pdt_ff_sync *syncs)
{
    int H, R, given;
    double ppm, res0;
    int rc = ff_plan(cfg, rate, &H, &R, &ppm, &given, &res0);
    if (rc) return rc;
    const size_t n = jobs.size();
    if (!n) return PDT_OK;
    HIP_TRY(hipSetDevice(c0->cfg.device));
    if ((rc = real_table(c0))) return rc;
    std::vector<double> residual(n, res0);
    std::vector<int> valid(n, given);
    if (!given && (rc = ff_tones(c0, jobs, rate, residual, valid))) return rc;
    const int nr = 2 * R + 1;
    std::vector<long long> periods((size_t)nr);
    for (int r = -R; r <= R; r++) periods[(size_t)(r + R)] = ff_period(H, r, ppm);
    const long long pmin = periods.front(), pmax = periods.back();
    std::vector<long long> len(n);
    for (size_t i = 0; i < n; i++) len[i] = (long long)std::min<uint64_t>(jobs[i].n, 2ull * rate);
    const FfWork W(len, (size_t)nr, (size_t)H, sizeof(FfWin), sizeof(FfSync));
    std::vector<unsigned char> head(W.o_v);
    FfWin *table = (FfWin *)(head.data() + W.o_tab);
    memcpy(head.data() + W.o_per, periods.data(), (size_t)nr * 8);
    long long tiles = 0, groups = 0;
    for (size_t i = 0; i < n; i++) {
        const uint64_t cap = (uint64_t)(ff_halves(len[i], 0, pmin) >> 1);
        const FfOut o = ff_out_layout(cap);
        pdt_ctx *own = jobs[i].owner;
        own->ff_rate = 0;
        if ((rc = own->ff_out.ensure(o.total))) return rc;
        own->ff_cap = cap;
        FfWin &w = table[i];
        unsigned char *p = (unsigned char *)own->ff_out.p;
        w.y = jobs[i].y;
        w.bits = p + o.t.o_bits;
        w.soft = (float *)(p + o.t.o_soft);
        w.symidx = (long long *)(p + o.t.o_idx);
        w.bitsym = (unsigned *)(p + o.t.o_sym);
        w.nbits = (unsigned long long *)p;
        w.sync = (FfSync *)(p + 16);
        w.L = len[i];
        w.residual_hz = residual[i];
        w.step = ddc_step((double)rate, residual[i]);
        w.tone_valid = valid[i];
        w.tile0 = (int32_t)tiles;
        w.group0 = (int32_t)groups;
        w.segs = (int32_t)((cap + FF_SEARCH_BITS - 1) / FF_SEARCH_BITS);
        w.reserved_ = 0;
        tiles += (len[i] + FF_MIX_TILE - 1) / FF_MIX_TILE;
        groups += (long long)nr * w.segs;
        if (tiles > 0x7fffffffll || groups > 0x7fffffffll) return PDT_ERR_ARG;
    }
    if ((rc = c0->ff_work.ensure(W.total))) return rc;
    unsigned char *wk = (unsigned char *)c0->ff_work.p;
    for (size_t i = 0; i < n; i++) {
        table[i].v = (float *)(wk + W.v[i]);
        table[i].metric = (unsigned long long *)(wk + W.o_metric + i * W.metric_each);
    }
    // (the table of the previous call is no longer read: every call ends with a synchronize)
    HIP_TRY(hipMemcpy(wk, head.data(), W.o_v, hipMemcpyHostToDevice));
    static const char *const names[3] = { "k_ff_mix", "k_ff_search", "k_ff_pick" };
    CallTimer timer(c0, c0->stream, names, nullptr, 3);
    HIP_TRY(timer.begin());
    HIP_TRY(ff_launch(c0->stream, wk + W.o_tab, (int)n, tiles, groups, (const long long *)(wk + W.o_per), R, H, pmax, (const float *)c0->an_tab.p,
                      wk + W.o_metric, n * W.metric_each, wk + W.o_syncs, timer.inner()));
    HIP_TRY(timer.end());
    std::vector<FfSync> back(n);
    HIP_TRY(hipMemcpyAsync(back.data(), wk + W.o_syncs, n * sizeof(FfSync), hipMemcpyDeviceToHost, c0->stream));
    HIP_TRY(hipStreamSynchronize(c0->stream));
    timer.commit();
    for (size_t i = 0; i < n; i++) {
        jobs[i].owner->ff_rate = rate;
        if (syncs) memcpy(&syncs[i], &back[i], sizeof(pdt_ff_sync));
    }
    return PDT_OK;
}

// the contexts of a call, checked as pdt_tones checks its own, and ARGOS ones
static int ff_check(pdt_ctx *const *ctxs, int count)
{
    if (count < 0 || (count && !ctxs)) return PDT_ERR_ARG;
    for (int i = 0; i < count; i++)
        if (!list_arg_ok(ctxs, i, PDT_MODE_ARGOS, true)) return PDT_ERR_ARG;
    int H, R, given;
    double ppm, res;
    if (count && ff_plan(nullptr, ctxs[0]->cfg.sample_rate, &H, &R, &ppm, &given, &res)) return PDT_ERR_ARG;
    for (int i = 0; i < count; i++)
        if (!channel_resident(ctxs[i])) return PDT_ERR_STATE;
    return PDT_OK;
}

static int ff_each(pdt_ctx *const *ctxs, int count, const pdt_ff_cfg *cfg, pdt_ff_sync *syncs)
{
    const int rc = ff_check(ctxs, count);
    if (rc || !count) return rc;
    try {
        std::vector<FfJob> jobs((size_t)count);
        for (int i = 0; i < count; i++)
            jobs[(size_t)i] = FfJob{ ctxs[i], (const float *)ctxs[i]->channel.p, ctxs[i]->stage_len[PDT_ST_CHANNEL], search_range_hz(ctxs[i]) };
        return ff_run(ctxs[0], jobs, ctxs[0]->cfg.sample_rate, cfg, syncs);
    } catch (const std::exception &) { return PDT_ERR_NOMEM; }
}

int pdt_ff_bits_batch(pdt_ctx *const *ctxs, int count, const pdt_ff_cfg *cfg, pdt_ff_sync *syncs)
{
    if (count > 0 && !syncs) return PDT_ERR_ARG;
    return ff_each(ctxs, count, cfg, syncs);
}

int pdt_ff_bits(pdt_ctx *ctx, const pdt_ff_cfg *cfg, pdt_ff_sync *sync)
{
    if (!ctx || !sync) return PDT_ERR_ARG;
    return ff_each(&ctx, 1, cfg, sync);
}

int pdt_stage_ff_bits(pdt_ctx *ctx, uint32_t rate, const float *iq_host, uint64_t n, const pdt_ff_cfg *cfg, pdt_ff_sync *sync)
{
    int H, R, given;
    double ppm, res;
    if (!ctx || !sync || (!iq_host && n) || ctx->cfg.mode != PDT_MODE_ARGOS || ff_plan(cfg, rate, &H, &R, &ppm, &given, &res)) return PDT_ERR_ARG;
    if (ctx->stream_open) return PDT_ERR_STATE;
    // (the first 2 Fs samples are all that is read, the tone's segment lies inside them)
    const uint64_t keep = std::min<uint64_t>(n, 2ull * rate);
    const int rc = stage_iq(ctx, ctx->staged_iq, iq_host, keep);
    if (rc) return rc;
    try {
        const std::vector<FfJob> jobs(1, FfJob{ ctx, (const float *)ctx->staged_iq.p, keep, -1.0 });
        return ff_run(ctx, jobs, rate, cfg, sync);
    } catch (const std::exception &) { return PDT_ERR_NOMEM; }
}

// What pdt_ff_read and pdt_ffp_read answer from a result buffer (FfOut, FfpOut: `head` bytes with the count and, at 16, the record;
// the tail t of bit_cap bits): the record, the count, and the first min(cap, count) bits, soft values and time sources
static int read_bits_result(pdt_ctx *ctx, const DevBuf &buf, size_t head_bytes, const BitsTail &t, uint64_t bit_cap, void *sync, size_t sync_bytes,
                            uint8_t *bits, float *soft, int64_t *index, uint64_t cap, uint64_t *count)
{
    HIP_TRY(hipSetDevice(ctx->cfg.device));
    unsigned char head[128];
    if (head_bytes > sizeof head) return PDT_ERR_ARG;
    HIP_TRY(hipMemcpy(head, buf.p, head_bytes, hipMemcpyDeviceToHost));
    unsigned long long nb;
    memcpy(&nb, head, sizeof nb);
    nb = std::min<unsigned long long>(nb, bit_cap);
    if (sync) memcpy(sync, head + 16, sync_bytes);
    const unsigned char *p = (const unsigned char *)buf.p;
    const size_t k = (size_t)std::min<uint64_t>(cap, nb);
    if (bits && k) HIP_TRY(hipMemcpy(bits, p + t.o_bits, k, hipMemcpyDeviceToHost));
    if (soft && k) HIP_TRY(hipMemcpy(soft, p + t.o_soft, k * 4, hipMemcpyDeviceToHost));
    if (index && k) HIP_TRY(hipMemcpy(index, p + t.o_idx, k * 8, hipMemcpyDeviceToHost));
    *count = nb;
    return PDT_OK;
}

int pdt_ff_read(pdt_ctx *ctx, pdt_ff_sync *sync, uint8_t *bits, float *soft, int64_t *index, uint64_t cap, uint64_t *count)
{
    if (!ctx || !count) return PDT_ERR_ARG;
    if (!ctx->ff_rate || !ctx->ff_out.p) return PDT_ERR_STATE;
    const FfOut o = ff_out_layout(ctx->ff_cap);
    return read_bits_result(ctx, ctx->ff_out, o.head, o.t, ctx->ff_cap, sync, sizeof *sync, bits, soft, index, cap, count);
}

int pdt_ff_messages_batch(pdt_ctx *const *ctxs, int count, const pdt_ff_cfg *cfg, const pdt_argos_cfg *rule_cfg, pdt_ff_sync *syncs, pdt_argos_msg *out,
                          int cap_each, int *counts)
{
    int K, rule;
    if (count < 0 || cap_each < 0 || (count && (!ctxs || !counts || (!out && cap_each))) || argos_min_run(rule_cfg, &K, &rule)) return PDT_ERR_ARG;
    const int rc = ff_each(ctxs, count, cfg, syncs);
    if (rc || !count) return rc;
    try {
        std::vector<BitJob> jobs;
        for (int i = 0; i < count; i++) jobs.push_back(job_result(ctxs[i]->ff_out.p, ff_out_layout(ctxs[i]->ff_cap).t, ctxs[i]->ff_cap, cap_each));
        const double fs = (double)ctxs[0]->cfg.sample_rate;
        return argos_deliver(ctxs[0], jobs, K, rule, [fs](size_t, long long src) { return (double)src / fs; }, out, cap_each, counts);
    } catch (const std::exception &) { return PDT_ERR_NOMEM; }
}

int pdt_ff_messages(pdt_ctx *ctx, const pdt_ff_cfg *cfg, const pdt_argos_cfg *rule, pdt_ff_sync *sync, pdt_argos_msg *out, int cap, int *count)
{
    if (!ctx || !count) return PDT_ERR_ARG;
    return pdt_ff_messages_batch(&ctx, 1, cfg, rule, sync, out, cap, count);
}

// ---------------------------------------------------------------- feed-forward POES bits (pdt_ffp.h)
// where the regions of a context's result buffer lie
static FfpOut ffp_out_of(const pdt_ctx *c) { return ffp_out_layout((size_t)c->ffp_blocks, (size_t)c->ffp_cap, sizeof(FfpBlock)); }

// The carrier of the stream y (device, n samples): every segment of pdt_tones at its defaults and stride nfft, in one launch of k_tones
// through the context's tables and buffers (tones_measure); the frequencies are derived here, on the host, in double.  tones: one record
// per segment.
static int ffp_tones(pdt_ctx *c, const float *y, uint64_t n, uint32_t rate, double range_hz, std::vector<pdt_tone> &tones, int *nfft)
{
    tones.clear();
    *nfft = tone_default_nfft((double)rate);
    TonePlan plan;
    if (!*nfft || n < (uint64_t)*nfft) return PDT_OK;
    const uint64_t want = n / (uint64_t)*nfft;
    if (want > 0x7fffffffull) return PDT_ERR_ARG;
    if (tone_plan(nullptr, (double)rate, range_hz, n, (int)want, &plan) != PDT_OK || !plan.nseg) return PDT_OK;
    std::vector<ToneSeg> table((size_t)plan.nseg);
    for (uint64_t j = 0; j < plan.nseg; j++) table[(size_t)j] = ToneSeg{ y, (long long)(plan.first + j * plan.stride), (int32_t)j, plan.kmax };
    std::vector<ToneRaw> raw;
    const int rc = tones_measure(c, plan, table, raw, nullptr);
    if (rc) return rc;
    tones.resize(table.size());
    tones_derive(raw.data(), plan, (double)rate, 0.0, c->tone_sw, c->tone_sw2, tones.data());
    return PDT_OK;
}

// The stream y (device, n samples at `rate`) through the four kernels: the context supplies stream, rotation table, work buffer and the
// result buffer the bits stay in.  One synchronize ends the call; the record comes back with it.
static int ffp_run(pdt_ctx *c, const float *y, uint64_t n, uint32_t rate, double range_hz, const pdt_ffp_cfg *cfg, pdt_ffp_sync *sync)
{
    FfpRule r;
    int given;
    double residual;
    int rc = ffp_plan(cfg, rate, n, &r, &given, &residual);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->cfg.device));
    if ((rc = real_table(c))) return rc;
    std::vector<pdt_tone> tones;
    int nfft = 0;
    if (!given && (rc = ffp_tones(c, y, n, rate, range_hz, tones, &nfft))) return rc;
    std::vector<uint32_t> steps, starts;
    FfpSync head;
    ffp_steps(tones.data(), tones.size(), nfft, r, given, residual, steps, starts, &head);
    const uint64_t cap = ffp_bit_cap(r);
    if (cap >= (1ull << 31)) return PDT_ERR_ARG;
    const FfpOut o = ffp_out_layout((size_t)r.nb, (size_t)cap, sizeof(FfpBlock));
    c->ffp_rate = 0;
    if ((rc = c->ffp_out.ensure(o.total))) return rc;
    if ((rc = c->ffp_work.ensure(ffp_work_bytes(r, steps.size())))) return rc;
    c->ffp_cap = cap;
    c->ffp_blocks = (uint64_t)r.nb;
    static const char *const names[4] = { "k_ffp_mix", "k_ffp_search", "k_ffp_track", "k_ffp_bits" };
    static const int launches[4] = { 1, 1, 2, 1 };
    CallTimer timer(c, c->stream, names, launches, 4);
    HIP_TRY(timer.begin());                                                // (in front of ffp_run_device's uploads)
    unsigned char *p = (unsigned char *)c->ffp_out.p;
    const FfpOutPtrs ptrs{ (unsigned long long *)p, (FfpSync *)(p + 16), (FfpBlock *)(p + o.o_blocks), (unsigned long long *)(p + o.o_pos),
                           (long long *)(p + o.t.o_idx), (float *)(p + o.t.o_soft), (unsigned *)(p + o.t.o_sym), p + o.t.o_bits };
    if ((rc = ffp_run_device(c->stream, y, r, head, steps, starts, (const float *)c->an_tab.p, c->ffp_work.p, ptrs, cap, timer.inner()))) return rc;
    HIP_TRY(timer.end());
    FfpSync back;
    HIP_TRY(hipMemcpyAsync(&back, p + 16, sizeof back, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    timer.commit();
    c->ffp_rate = rate;
    if (sync) memcpy(sync, &back, sizeof back);
    return PDT_OK;
}

// the context of a call, checked as pdt_tones checks its own, and a POES one
static int ffp_check(const pdt_ctx *c, const pdt_ffp_cfg *cfg)
{
    if (!c || c->cfg.mode != PDT_MODE_POES) return PDT_ERR_ARG;
    FfpRule r;
    int given;
    double res;
    if (ffp_plan(cfg, c->cfg.sample_rate, 0, &r, &given, &res)) return PDT_ERR_ARG;
    if (!channel_resident(c)) return PDT_ERR_STATE;
    return PDT_OK;
}

int pdt_ffp_bits(pdt_ctx *ctx, const pdt_ffp_cfg *cfg, pdt_ffp_sync *sync)
{
    if (!ctx || !sync) return PDT_ERR_ARG;
    const int rc = ffp_check(ctx, cfg);
    if (rc) return rc;
    try {
        return ffp_run(ctx, (const float *)ctx->channel.p, ctx->stage_len[PDT_ST_CHANNEL], ctx->cfg.sample_rate, search_range_hz(ctx), cfg, sync);
    } catch (const std::exception &) { return PDT_ERR_NOMEM; }
}

// the caller's stream in a buffer of the context's own: nothing its results live in is touched
static int ffp_stage_in(pdt_ctx *ctx, uint32_t rate, const float *iq_host, uint64_t n, const pdt_ffp_cfg *cfg)
{
    FfpRule r;
    int given;
    double res;
    if (!ctx || (!iq_host && n) || ctx->cfg.mode != PDT_MODE_POES || ffp_plan(cfg, rate, n, &r, &given, &res)) return PDT_ERR_ARG;
    if (ctx->stream_open) return PDT_ERR_STATE;
    return stage_iq(ctx, ctx->staged_iq, iq_host, n);
}

int pdt_stage_ffp_bits(pdt_ctx *ctx, uint32_t rate, const float *iq_host, uint64_t n, const pdt_ffp_cfg *cfg, pdt_ffp_sync *sync)
{
    if (!sync) return PDT_ERR_ARG;
    const int rc = ffp_stage_in(ctx, rate, iq_host, n, cfg);
    if (rc) return rc;
    try {
        return ffp_run(ctx, (const float *)ctx->staged_iq.p, n, rate, -1.0, cfg, sync);
    } catch (const std::exception &) { return PDT_ERR_NOMEM; }
}

int pdt_ffp_read(pdt_ctx *ctx, pdt_ffp_sync *sync, uint8_t *bits, float *soft, int64_t *index, uint64_t cap, uint64_t *count)
{
    if (!ctx || !count) return PDT_ERR_ARG;
    if (!ctx->ffp_rate || !ctx->ffp_out.p) return PDT_ERR_STATE;
    const FfpOut o = ffp_out_of(ctx);
    return read_bits_result(ctx, ctx->ffp_out, o.head, o.t, ctx->ffp_cap, sync, sizeof *sync, bits, soft, index, cap, count);
}

int pdt_ffp_blocks(pdt_ctx *ctx, pdt_ffp_block *out, uint64_t cap, uint64_t *count)
{
    if (!ctx || !count || (!out && cap)) return PDT_ERR_ARG;
    if (!ctx->ffp_rate || !ctx->ffp_out.p) return PDT_ERR_STATE;
    HIP_TRY(hipSetDevice(ctx->cfg.device));
    const size_t k = (size_t)std::min<uint64_t>(cap, ctx->ffp_blocks);
    if (k) HIP_TRY(hipMemcpy(out, (const unsigned char *)ctx->ffp_out.p + ffp_out_of(ctx).o_blocks, k * sizeof(pdt_ffp_block), hipMemcpyDeviceToHost));
    *count = ctx->ffp_blocks;
    return PDT_OK;
}

// The feed-forward bits by bits_call, then the flywheel's kernels on the bits it left in the context's buffer, on the device's own count
extern "C++" template <typename Bits>
int ffp_frames_after(pdt_ctx *ctx, Bits bits_call, const pdt_tip_sync_cfg *tip_cfg, pdt_ffp_sync *sync, pdt_frame *out, pdt_tip_sync_info *info, int cap,
                     int *count)
{
    TipSyncRule R;
    if (!ctx || !count || cap < 0 || (!out && cap) || tip_sync_rule(tip_cfg, &R)) return PDT_ERR_ARG;
    pdt_ffp_sync s;
    const int rc = bits_call(&s);
    if (rc) return rc;
    if (sync) *sync = s;
    try {
        const double fs = (double)ctx->ffp_rate;
        return tip_sync_deliver(ctx, std::vector<BitJob>(1, job_result(ctx->ffp_out.p, ffp_out_of(ctx).t, ctx->ffp_cap, cap)), R,
                                [fs](size_t, long long src) { return (double)src / fs; }, out, info, cap, count);
    } catch (const std::exception &) { return PDT_ERR_NOMEM; }
}

int pdt_ffp_frames(pdt_ctx *ctx, const pdt_ffp_cfg *cfg, const pdt_tip_sync_cfg *tip_cfg, pdt_ffp_sync *sync, pdt_frame *out, pdt_tip_sync_info *info,
                   int cap, int *count)
{
    return ffp_frames_after(ctx, [&](pdt_ffp_sync *s) { return pdt_ffp_bits(ctx, cfg, s); }, tip_cfg, sync, out, info, cap, count);
}

int pdt_stage_ffp_frames(pdt_ctx *ctx, uint32_t rate, const float *iq_host, uint64_t n, const pdt_ffp_cfg *cfg, const pdt_tip_sync_cfg *tip_cfg,
                         pdt_ffp_sync *sync, pdt_frame *out, pdt_tip_sync_info *info, int cap, int *count)
{
    return ffp_frames_after(ctx, [&](pdt_ffp_sync *s) { return pdt_stage_ffp_bits(ctx, rate, iq_host, n, cfg, s); }, tip_cfg, sync, out, info, cap, count);
}

// ---------------------------------------------------------------- parity repair from the soft values (pdt_tip_repair.h)
// k_tip_repair on the caller's records against soft values that are on the device (their count too: read as min(*nbits_dev, bit_cap)).
// The records go up as they are, into a buffer of their own beside their info records and the counters (RepairWork); one synchronize
// ends the call.
static int tip_repair_run(pdt_ctx *c, const float *soft_dev, const unsigned long long *nbits_dev, long long bit_cap, pdt_frame *frames, uint64_t n,
                          pdt_tip_repair_info *info, pdt_tip_repair_summary *summary)
{
    memset(summary, 0, sizeof *summary);
    if (n == 0) return PDT_OK;
    const RepairWork L = repair_work_layout((size_t)n, sizeof(pdt_frame), sizeof(pdt_tip_repair_info));
    int rc;
    if ((rc = c->tip_repair_work.ensure(L.total))) return rc;
    unsigned char *w = (unsigned char *)c->tip_repair_work.p;
    hipStream_t st = c->stream;
    HIP_TRY(hipMemsetAsync(w + L.o_sum, 0, 64, st));
    HIP_TRY(hipMemcpyAsync(w + L.o_rec, frames, (size_t)n * sizeof(pdt_frame), hipMemcpyHostToDevice, st));
    static const char *const names[1] = { "k_tip_repair" };
    CallTimer timer(c, st, names, nullptr, 1);
    HIP_TRY(timer.begin());
    HIP_TRY(tip_repair_launch(st, w + L.o_rec, (unsigned)n, soft_dev, nbits_dev, bit_cap, w + L.o_info, w + L.o_sum));
    HIP_TRY(timer.end());
    HIP_TRY(hipMemcpyAsync(frames, w + L.o_rec, (size_t)n * sizeof(pdt_frame), hipMemcpyDeviceToHost, st));
    if (info) HIP_TRY(hipMemcpyAsync(info, w + L.o_info, (size_t)n * sizeof(pdt_tip_repair_info), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(summary, w + L.o_sum, sizeof *summary, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    timer.commit();
    return PDT_OK;
}

int pdt_tip_repair(pdt_ctx *ctx, pdt_frame *frames, uint64_t n, pdt_tip_repair_info *info, pdt_tip_repair_summary *summary)
{
    if (!ctx || !summary || (!frames && n) || n >= (1ull << 31)) return PDT_ERR_ARG;
    if (ctx->cfg.mode != PDT_MODE_POES) return PDT_ERR_ARG;             // TIP minor frames only
    if (ctx->stream_open || !ctx->ffp_rate || !ctx->ffp_out.p) return PDT_ERR_STATE;
    HIP_TRY(hipSetDevice(ctx->cfg.device));
    const unsigned char *p = (const unsigned char *)ctx->ffp_out.p;
    return tip_repair_run(ctx, (const float *)(p + ffp_out_of(ctx).t.o_soft), (const unsigned long long *)p, (long long)ctx->ffp_cap, frames, n, info, summary);
}

int pdt_stage_tip_repair(pdt_ctx *ctx, const float *soft_host, uint64_t nbits, pdt_frame *frames, uint64_t n, pdt_tip_repair_info *info,
                         pdt_tip_repair_summary *summary)
{
    if (!ctx || !summary || (!frames && n) || n >= (1ull << 31) || (!soft_host && nbits) || nbits >= (1ull << 31)) return PDT_ERR_ARG;
    if (ctx->cfg.mode != PDT_MODE_POES) return PDT_ERR_ARG;
    if (ctx->stream_open) return PDT_ERR_STATE;
    const int rc = stage_counted(ctx, ctx->tip_repair_soft, soft_host, nbits, sizeof(float));
    if (rc) return rc;
    const unsigned char *p = (const unsigned char *)ctx->tip_repair_soft.p;
    return tip_repair_run(ctx, (const float *)(p + 16), (const unsigned long long *)p, (long long)nbits, frames, n, info, summary);
}

// ---------------------------------------------------------------- DCS packets of TIP minor frames (pdt_tip_dcs.h)
// The four kernels on n records: the caller's (uploaded into the work buffer as they are) or, with frames == NULL, the chain's own in
// ctx->frames, whose time stamps go up from frames_host beside them.  The counters come back first -- the packet count has stayed on the
// device until then --, then as many packets as were found and fit.
static_assert(sizeof(FrameRec) == sizeof(pdt::TipDcsChainRec) && offsetof(FrameRec, nbytes) == offsetof(pdt::TipDcsChainRec, nbytes) &&
              offsetof(FrameRec, complete) == offsetof(pdt::TipDcsChainRec, complete) && offsetof(FrameRec, bytes) == offsetof(pdt::TipDcsChainRec, bytes), "FrameRec");
static int tip_dcs_run(pdt_ctx *c, const pdt_frame *frames, uint64_t n, unsigned channel_max, pdt_dcs_packet *out, int cap, int *count, pdt_dcs_summary *summary)
{
    memset(summary, 0, sizeof *summary);
    *count = 0;
    if (n == 0) return PDT_OK;
    const size_t tiles = ((size_t)n + pdt::TIP_DCS_TILE_RECS - 1) / pdt::TIP_DCS_TILE_RECS;
    const size_t room = (size_t)std::min<uint64_t>((uint64_t)cap, 3 * n);                       // (a record holds at most three heads' packets)
    const DcsWork L = dcs_work_layout((size_t)n, tiles, pdt::TIP_DCS_TILE, tip_dcs_map_bytes(), tip_dcs_entry_bytes(),
                                      (size_t)n * (frames ? sizeof(pdt_frame) : sizeof(double)), room * sizeof(pdt_dcs_packet));
    int rc;
    if ((rc = c->tip_dcs_work.ensure(L.total))) return rc;
    unsigned char *w = (unsigned char *)c->tip_dcs_work.p;
    hipStream_t st = c->stream;
    std::vector<double> times;
    HIP_TRY(hipMemsetAsync(w + L.o_sum, 0, L.o_stream - L.o_sum, st));                               // the counters and the flags
    if (frames) HIP_TRY(hipMemcpyAsync(w + L.o_src, frames, (size_t)n * sizeof(pdt_frame), hipMemcpyHostToDevice, st));
    else {
        times.resize((size_t)n);
        for (size_t f = 0; f < (size_t)n; f++) times[f] = c->frames_host[f].time;
        HIP_TRY(hipMemcpyAsync(w + L.o_src, times.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
    }
    CallTimer timer(c, st, tip_dcs_kernel_names, nullptr, 4);
    HIP_TRY(timer.begin());
    HIP_TRY(tip_dcs_launch(st, frames ? (const void *)(w + L.o_src) : c->frames.p, !frames, w + L.o_src, n, channel_max, w + L.o_sum, w + L.o_flags, w + L.o_stream,
                           w + L.o_head, w + L.o_bad, w + L.o_maps, w + L.o_entry, w + L.o_out, room, timer.inner()));
    HIP_TRY(timer.end());
    unsigned long long counters[16];
    HIP_TRY(hipMemcpyAsync(counters, w + L.o_sum, sizeof counters, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    timer.commit();
    tip_dcs_summary(counters, n, summary);
    const size_t give = (size_t)std::min<uint64_t>(summary->packets, room);
    if (give) HIP_TRY(hipMemcpy(out, w + L.o_out, give * sizeof(pdt_dcs_packet), hipMemcpyDeviceToHost));
    *count = (int)std::min<uint64_t>(summary->packets, 0x7fffffffull);
    return PDT_OK;
}

int pdt_tip_dcs(pdt_ctx *ctx, const pdt_dcs_cfg *cfg, pdt_dcs_packet *out, int cap, int *count, pdt_dcs_summary *summary)
{
    unsigned channel_max;
    if (!ctx || !count || !summary || cap < 0 || (!out && cap) || tip_dcs_rule(cfg, &channel_max)) return PDT_ERR_ARG;
    if (ctx->cfg.mode != PDT_MODE_POES) return PDT_ERR_ARG;             // TIP minor frames only
    const unsigned nf = ctx->frames_on_device;
    if (ctx->stream_open || !ctx->have_frames || nf != ctx->frames_host.size()) return PDT_ERR_STATE;
    if (hipSetDevice(ctx->cfg.device) != hipSuccess) return PDT_ERR_NOGPU;
    try {
        return tip_dcs_run(ctx, nullptr, nf, channel_max, out, cap, count, summary);
    } catch (const std::exception &) { return PDT_ERR_NOMEM; }
}

int pdt_tip_dcs_records(pdt_ctx *ctx, const pdt_frame *frames, uint64_t n, const pdt_dcs_cfg *cfg, pdt_dcs_packet *out, int cap, int *count,
                        pdt_dcs_summary *summary)
{
    unsigned channel_max;
    if (!ctx || !count || !summary || (!frames && n) || n >= (1ull << 31) || cap < 0 || (!out && cap) || tip_dcs_rule(cfg, &channel_max)) return PDT_ERR_ARG;
    if (ctx->cfg.mode != PDT_MODE_POES) return PDT_ERR_ARG;
    if (ctx->stream_open) return PDT_ERR_STATE;
    if (hipSetDevice(ctx->cfg.device) != hipSuccess) return PDT_ERR_NOGPU;
    try {
        return tip_dcs_run(ctx, frames, n, channel_max, out, cap, count, summary);
    } catch (const std::exception &) { return PDT_ERR_NOMEM; }
}

// ---------------------------------------------------------------- subcommutated bytes of TIP minor frames (pdt_tip_subcom.h)
// The five kernels on n records: the caller's (uploaded into the work buffer as they are) or, with frames == NULL, the chain's own in
// ctx->frames, whose time stamps go up from frames_host beside them.  The counters and offsets come back first -- the sample count has
// stayed on the device until then --, then as many samples as were found and fit.
struct SubcomRuleHost { int nchan, max_fire, trusted_only, thr; };
static int tip_subcom_run(pdt_ctx *c, const pdt_frame *frames, uint64_t n, const pdt_subcom_entry *entries, int ne, const SubcomRuleHost &R, pdt_subcom_sample *out,
                          int cap, int *count, uint64_t *offsets, pdt_subcom_summary *summary)
{
    memset(summary, 0, sizeof *summary);
    *count = 0;
    if (offsets) memset(offsets, 0, ((size_t)R.nchan + 1) * sizeof *offsets);
    if (n == 0) return PDT_OK;
    const size_t tiles = ((size_t)n + pdt::TIP_SUBCOM_TILE - 1) / pdt::TIP_SUBCOM_TILE;
    const size_t limit = (size_t)n * (size_t)R.max_fire, room = std::min((size_t)cap, limit);
    const SubcomWork L = subcom_work_layout((size_t)n, tiles, (size_t)R.nchan, (size_t)ne * sizeof(pdt_subcom_entry),
                                            (size_t)n * (frames ? sizeof(pdt_frame) : sizeof(double)), limit, room * sizeof(pdt_subcom_sample));
    int rc;
    if ((rc = c->tip_subcom_work.ensure(L.total))) return rc;
    unsigned char *w = (unsigned char *)c->tip_subcom_work.p;
    hipStream_t st = c->stream;
    std::vector<double> times;
    HIP_TRY(hipMemsetAsync(w + L.o_sum, 0, L.o_table - L.o_sum, st));                                // the counters and the offsets
    HIP_TRY(hipMemcpyAsync(w + L.o_table, entries, (size_t)ne * sizeof(pdt_subcom_entry), hipMemcpyHostToDevice, st));
    if (frames) HIP_TRY(hipMemcpyAsync(w + L.o_src, frames, (size_t)n * sizeof(pdt_frame), hipMemcpyHostToDevice, st));
    else {
        times.resize((size_t)n);
        for (size_t f = 0; f < (size_t)n; f++) times[f] = c->frames_host[f].time;
        HIP_TRY(hipMemcpyAsync(w + L.o_src, times.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
    }
    CallTimer timer(c, st, tip_subcom_kernel_names, nullptr, 5);
    HIP_TRY(timer.begin());
    HIP_TRY(tip_subcom_launch(st, frames ? (const void *)(w + L.o_src) : c->frames.p, !frames, w + L.o_src, n, w + L.o_table, ne, R.nchan, R.trusted_only, R.thr,
                              w + L.o_sum, w + L.o_marks, w + L.o_cnt, w + L.o_offsets, w + L.o_vals, limit, w + L.o_out, room, timer.inner()));
    HIP_TRY(timer.end());
    unsigned long long head[16 + 129];
    HIP_TRY(hipMemcpyAsync(head, w + L.o_sum, sizeof head, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    timer.commit();
    tip_subcom_summary(head, summary);
    if (offsets)
        for (int k = 0; k <= R.nchan; k++) offsets[k] = head[16 + k];
    const size_t give = (size_t)std::min<uint64_t>(summary->samples, room);
    if (give) HIP_TRY(hipMemcpy(out, w + L.o_out, give * sizeof(pdt_subcom_sample), hipMemcpyDeviceToHost));
    *count = (int)std::min<uint64_t>(summary->samples, 0x7fffffffull);
    return PDT_OK;
}

int pdt_tip_subcom(pdt_ctx *ctx, const pdt_subcom_entry *entries, uint64_t nentries, const pdt_subcom_cfg *cfg, pdt_subcom_sample *out, int cap, int *count,
                   uint64_t *offsets, pdt_subcom_summary *summary)
{
    SubcomRuleHost R;
    if (!ctx || !count || !summary || cap < 0 || (!out && cap)) return PDT_ERR_ARG;
    if (tip_subcom_rule(entries, nentries, cfg, ctx->frames_on_device, &R.nchan, &R.max_fire, &R.trusted_only, &R.thr)) return PDT_ERR_ARG;
    if (ctx->cfg.mode != PDT_MODE_POES) return PDT_ERR_ARG;             // TIP minor frames only
    const unsigned nf = ctx->frames_on_device;
    if (ctx->stream_open || !ctx->have_frames || nf != ctx->frames_host.size()) return PDT_ERR_STATE;
    if (hipSetDevice(ctx->cfg.device) != hipSuccess) return PDT_ERR_NOGPU;
    try {
        return tip_subcom_run(ctx, nullptr, nf, entries, (int)nentries, R, out, cap, count, offsets, summary);
    } catch (const std::exception &) { return PDT_ERR_NOMEM; }
}

int pdt_tip_subcom_records(pdt_ctx *ctx, const pdt_frame *frames, uint64_t n, const pdt_subcom_entry *entries, uint64_t nentries, const pdt_subcom_cfg *cfg,
                           pdt_subcom_sample *out, int cap, int *count, uint64_t *offsets, pdt_subcom_summary *summary)
{
    SubcomRuleHost R;
    if (!ctx || !count || !summary || (!frames && n) || n >= (1ull << 31) || cap < 0 || (!out && cap)) return PDT_ERR_ARG;
    if (tip_subcom_rule(entries, nentries, cfg, n, &R.nchan, &R.max_fire, &R.trusted_only, &R.thr)) return PDT_ERR_ARG;
    if (ctx->cfg.mode != PDT_MODE_POES) return PDT_ERR_ARG;
    if (ctx->stream_open) return PDT_ERR_STATE;
    if (hipSetDevice(ctx->cfg.device) != hipSuccess) return PDT_ERR_NOGPU;
    try {
        return tip_subcom_run(ctx, frames, n, entries, (int)nentries, R, out, cap, count, offsets, summary);
    } catch (const std::exception &) { return PDT_ERR_NOMEM; }
}

int pdt_stage_bytesync(pdt_ctx *ctx, const uint8_t *bits_host, uint64_t nbits)
{
    return pdt_stage_bytesync_from(ctx, bits_host, nbits, 0);
}

int pdt_stage_bytesync_from(pdt_ctx *ctx, const uint8_t *bits_host, uint64_t nbits, uint64_t first_sync_end)
{
    if (!ctx || (!bits_host && nbits)) return PDT_ERR_ARG;
    if (nbits >= (1ull << 31)) return PDT_ERR_ARG;
    if (ctx->stream_open) return PDT_ERR_STATE;              // (the stage buffers carry an open stream's tails)
    HIP_TRY(hipSetDevice(ctx->cfg.device));
    const bool argos = ctx->cfg.mode == PDT_MODE_ARGOS;
    const SyncParams SP = make_sync_params(argos);
    const long long bit_cap = (long long)nbits + 64;
    const uint32_t hit_cap = next_pow2((uint32_t)(bit_cap / 4 + 4096));
    const uint32_t frame_cap = (uint32_t)(bit_cap / SP.span + 16);
    int rc;
    if ((rc = ctx->bits.ensure((size_t)bit_cap))) return rc;
    if ((rc = ctx->bitsym.ensure((size_t)bit_cap * sizeof(unsigned)))) return rc;
    if ((rc = ctx->symidx.ensure((size_t)bit_cap * sizeof(long long)))) return rc;
    if ((rc = ctx->hits.ensure((size_t)hit_cap * sizeof(unsigned)))) return rc;
    if ((rc = ctx->sync_scr.ensure((2 * ((size_t)hit_cap + 1) + hit_cap / 32 + 2) * sizeof(unsigned)))) return rc;
    if ((rc = ctx->frames.ensure((size_t)frame_cap * sizeof(FrameRec)))) return rc;
    if ((rc = ctx->stiles.ensure((size_t)((bit_cap + 4095) / 4096 + 1) * sizeof(SyncTile)))) return rc;
    if ((rc = ctx->scal.ensure(sizeof(DevScalars)))) return rc;
    hipStream_t st = ctx->stream;
    DevScalars *d_sc = (DevScalars *)ctx->scal.p;
    DevScalars sc;
    memset(&sc, 0, sizeof sc);
    sc.nbits = nbits;
    Plan &PL = oneshot_begin(ctx);
    PL.copy(OP_H2D, d_sc, &sc, sizeof sc);
    if (nbits) PL.copy(OP_H2D, ctx->bits.p, bits_host, (size_t)nbits);
    PL.memset_async(ctx->frames.p, 0, (size_t)frame_cap * sizeof(FrameRec));
    PDT_LAUNCH(256, k_iota, dim3((unsigned)((bit_cap + 255) / 256)), dim3(256), 0, st, (unsigned *)ctx->bitsym.p,
               (long long *)ctx->symidx.p, bit_cap);
    launch_bytesync(ctx, PL, st, SP, d_sc, bit_cap, hit_cap, frame_cap, (long long)first_sync_end);
    if ((rc = oneshot_run(ctx, d_sc, &sc))) return rc;
    if (sc.nframes > frame_cap || (sc.sync_overflow && sc.nhits > hit_cap)) return PDT_ERR_STATE;
    std::vector<FrameRec> recs(sc.nframes);
    if (sc.nframes) HIP_TRY(hipMemcpy(recs.data(), ctx->frames.p, (size_t)sc.nframes * sizeof(FrameRec), hipMemcpyDeviceToHost));
    ctx->frames_host.resize(sc.nframes);
    ctx->frames_on_device = sc.nframes;
    ctx->have_frames = true;
    ctx->tip_host.clear();
    for (unsigned f = 0; f < sc.nframes; f++) {
        pdt_frame &o = ctx->frames_host[f];
        memset(&o, 0, sizeof o);
        o.bit_index = recs[f].bit_index;
        o.time_src = recs[f].time_src;
        o.time = (double)recs[f].time_src;
        o.inverted = recs[f].inverted;
        o.nbytes = recs[f].nbytes;
        o.complete = recs[f].complete;
        memcpy(o.bytes, recs[f].bytes, 104);
    }
    memset(&ctx->stats, 0, sizeof ctx->stats);
    ctx->stats.bits = nbits;
    ctx->stats.frames = sc.nframes;
    ctx->stats.sync_overflow = sc.sync_overflow;
    memset(ctx->stage_len, 0, sizeof ctx->stage_len);
    return PDT_OK;
}


int pdt_stage_pll(pdt_ctx *ctx, const void *iq_host, uint64_t n, int sample_format, pdt_pll_state *state, void *out_host,
                  void *lock_out_host, double *avg_phase_ret)
{
    if (!ctx || (!iq_host && n) || n >= (1ull << 31) || (sample_format != PDT_FMT_PCM16 && sample_format != PDT_FMT_F32)) return PDT_ERR_ARG;
    if (ctx->elem != 4 && sample_format == PDT_FMT_F32) return PDT_ERR_FORMAT;   // (double contexts: no `double complex` sample source)
    if (ctx->cfg.profile || ctx->stream_open) return PDT_ERR_STATE;
    HIP_TRY(hipSetDevice(ctx->cfg.device));
    if (ctx->elem == 8) return stage_pll<double>(ctx, iq_host, n, sample_format, state, out_host, lock_out_host, avg_phase_ret);
    return stage_pll<float>(ctx, iq_host, n, sample_format, state, out_host, lock_out_host, avg_phase_ret);
}

int pdt_stage_gardner(pdt_ctx *ctx, const void *in_host, uint64_t n, uint64_t capacity, const void *neighbour_host,
                      pdt_gardner_state *state, void *out_host, uint64_t *pick_out, uint64_t *nsym_out)
{
    if (!ctx || !in_host || capacity == 0 || n > capacity || capacity >= (1ull << 30)) return PDT_ERR_ARG;
    if (ctx->cfg.sampler != PDT_SAMPLER_GARDNER) return PDT_ERR_ARG;
    if (ctx->stream_open) return PDT_ERR_STATE;              // (the stage buffers carry an open stream's tails)
    HIP_TRY(hipSetDevice(ctx->cfg.device));
    if (ctx->elem == 8) return stage_gardner<double>(ctx, in_host, n, capacity, neighbour_host, state, out_host, pick_out, nsym_out);
    return stage_gardner<float>(ctx, in_host, n, capacity, neighbour_host, state, out_host, pick_out, nsym_out);
}

int pdt_stage_static_gain(pdt_ctx *ctx, const void *iq_host, uint64_t n, int sample_format, double level, double *gain_out)
{
    if (!ctx || !iq_host || n == 0 || n >= (1ull << 31) || (sample_format != PDT_FMT_PCM16 && sample_format != PDT_FMT_F32)) return PDT_ERR_ARG;
    if (ctx->stream_open) return PDT_ERR_STATE;              // (the stage buffers carry an open stream's tails)
    HIP_TRY(hipSetDevice(ctx->cfg.device));
    if (ctx->elem == 8) return stage_static_gain<double>(ctx, iq_host, n, sample_format, level, gain_out);
    return stage_static_gain<float>(ctx, iq_host, n, sample_format, level, gain_out);
}

int pdt_stage_mm(pdt_ctx *ctx, const void *in_host, uint64_t n, pdt_mm_state *state, void *out_host, uint64_t *pick_out,
                 uint64_t *nsym_out)
{
    if (!ctx || (!in_host && n) || n >= (1ull << 30)) return PDT_ERR_ARG;
    // (the range the whole-capture entries refuse, against the context's own baud rate)
    if (ctx->elem == 8 ? make_mm_params<double>(ctx, 0, 0, nullptr) : make_mm_params<float>(ctx, 0, 0, nullptr)) return PDT_ERR_ARG;
    if (ctx->stream_open) return PDT_ERR_STATE;              // (the stage buffers carry an open stream's tails)
    HIP_TRY(hipSetDevice(ctx->cfg.device));
    if (ctx->elem == 8) return stage_mm<double>(ctx, in_host, n, state, out_host, pick_out, nsym_out);
    return stage_mm<float>(ctx, in_host, n, state, out_host, pick_out, nsym_out);
}

int pdt_stage_agc(pdt_ctx *ctx, void *data_host, uint64_t n, double initial, double attack, double decay, pdt_agc_state *state)
{
    if (!ctx || (!data_host && n) || n >= (1ull << 31)) return PDT_ERR_ARG;
    if (ctx->stream_open) return PDT_ERR_STATE;              // (the stage buffers carry an open stream's tails)
    HIP_TRY(hipSetDevice(ctx->cfg.device));
    if (ctx->elem == 8) return stage_agc<double>(ctx, data_host, n, initial, attack, decay, state);
    return stage_agc<float>(ctx, data_host, n, initial, attack, decay, state);
}

int pdt_stage_squelch(pdt_ctx *ctx, void *data_host, const void *lock_host, uint64_t n, double threshold)
{
    if (!ctx || ((!data_host || !lock_host) && n) || n >= (1ull << 31)) return PDT_ERR_ARG;
    if (ctx->stream_open) return PDT_ERR_STATE;              // (the stage buffers carry an open stream's tails)
    HIP_TRY(hipSetDevice(ctx->cfg.device));
    if (ctx->elem == 8) return stage_squelch<double>(ctx, data_host, lock_host, n, threshold);
    return stage_squelch<float>(ctx, data_host, lock_host, n, threshold);
}

int pdt_stage_manchester(pdt_ctx *ctx, const void *symbols_host, uint64_t nsymbols, double resync_threshold,
                         pdt_manchester_state *state, uint8_t *bits_out, uint32_t *bit_symbol_out, uint64_t *nbits_out)
{
    if (!ctx || (!symbols_host && nsymbols) || nsymbols >= (1ull << 31)) return PDT_ERR_ARG;
    if (nbits_out) *nbits_out = 0;
    if (nsymbols == 0) return PDT_OK;                                 // the loop body never runs: nothing changes
    if (ctx->stream_open) return PDT_ERR_STATE;              // (the stage buffers carry an open stream's tails)
    HIP_TRY(hipSetDevice(ctx->cfg.device));
    if (ctx->elem == 8)
        return stage_manchester<double>(ctx, symbols_host, nsymbols, resync_threshold, state, bits_out, bit_symbol_out, nbits_out);
    return stage_manchester<float>(ctx, symbols_host, nsymbols, resync_threshold, state, bits_out, bit_symbol_out, nbits_out);
}

int pdt_stage_fir(pdt_ctx *ctx, const void *in_host, uint64_t n, pdt_fir_state *state, void *out_host)
{
    if (!ctx || (!in_host && n) || n >= (1ull << 31)) return PDT_ERR_ARG;
    if (ctx->stream_open) return PDT_ERR_STATE;              // (the stage buffers carry an open stream's tails)
    HIP_TRY(hipSetDevice(ctx->cfg.device));
    if (ctx->elem == 8) return stage_fir<double>(ctx, in_host, n, state, out_host);
    return stage_fir<float>(ctx, in_host, n, state, out_host);
}

// ---------------------------------------------------------------- batched many-capture mode
int pdt_demod_batch_device(pdt_ctx *const *ctxs, const void *const *iq_device, const uint64_t *nframes, int count)
{
    return demod_batch(ctxs, iq_device, nframes, count, PDT_FMT_PCM16);
}

// fmt: PDT_FMT_PCM16, or PDT_FMT_F32 for the channel streams of pdt_demod_channels_device
static int demod_batch(pdt_ctx *const *ctxs, const void *const *iq_device, const uint64_t *nframes, int count, int fmt)
{
    if (count < 0 || (count && (!ctxs || !iq_device || !nframes))) return PDT_ERR_ARG;
    for (int i = 0; i < count; i++) {
        if (!ctxs[i] || (!iq_device[i] && nframes[i])) return PDT_ERR_ARG;
        if (ctxs[i]->stream_open) return PDT_ERR_STATE;
        for (int j = 0; j < i; j++)
            if (ctxs[j] == ctxs[i]) return PDT_ERR_ARG;               // one context per capture
    }
    int first_err = PDT_OK, enq = 0;
    for (; enq < count; enq++) {                                        // the plan of every capture (host only)
        pdt_ctx *c = ctxs[enq];
        c->batch_hint = 0;
        for (int k = 0; k < count; k++) c->batch_hint += (ctxs[k]->cfg.device == c->cfg.device) ? 1 : 0;
        c->pcm_dev = iq_device[enq];
        c->pcm_fmt = in_fmt(fmt).pcm_fmt;
        const int rc = demod_common(c, nframes[enq], RUN_ENQUEUE);
        if (rc) { first_err = rc; break; }
    }
    // captures whose plans have the same shape (same mode, rate, chunk geometry, code path) and live on the same GPU
    // share their launches: one launch per stage for the whole group, the capture index in blockIdx.z
    std::vector<char> done((size_t)enq, 0);
    for (int i = 0; i < enq; i++) {
        if (done[(size_t)i]) continue;
        std::vector<pdt_ctx *> group{ctxs[i]};
        done[(size_t)i] = 1;
        for (int j = i + 1; j < enq && (int)group.size() < 65535; j++)
            if (!done[(size_t)j] && ctxs[j]->cfg.device == ctxs[i]->cfg.device && ctxs[i]->plan.same_shape(ctxs[j]->plan)) {
                group.push_back(ctxs[j]);
                done[(size_t)j] = 1;
            }
        const int rc = execute_plans(group.data(), (int)group.size());
        if (rc) {
            if (!first_err) first_err = rc;
            for (pdt_ctx *c : group) c->pending = false;
        }
    }
    for (int i = 0; i < enq; i++) {                                     // then collect them in order
        if (!ctxs[i]->pending) continue;
        const int rc = demod_common(ctxs[i], nframes[i], RUN_FINISH);
        if (rc && !first_err) first_err = rc;
    }
    return first_err;
}

// ---------------------------------------------------------------- streaming front end
// No stream: what pdt_stream_begin starts from, and what the whole-capture paths that borrow the stream machinery leave behind
// (demod_overlapped, demod_windowed: a later push starts a new stream).  Results and statistics are not touched.
static void stream_reset(pdt_ctx *ctx)
{
    ctx->sc = StreamCarry();
    ctx->stream_have = ctx->stream_done = ctx->stream_total = 0;
    ctx->stream_fmt = -1;
    ctx->halo.left = ctx->halo.pending = ctx->halo.in = ctx->halo.out = 0;
    ctx->stream_open = false;
}

int pdt_stream_begin(pdt_ctx *ctx)
{
    if (!ctx) return PDT_ERR_ARG;
    stream_reset(ctx);
    ctx->stream_new.clear();
    ctx->frames_host.clear();
    ctx->chunk_host.clear();
    ctx->report_samples = 0;
    ctx->tip_host.clear();
    ctx->frames_on_device = 0;
    memset(&ctx->stats, 0, sizeof ctx->stats);
    memset(ctx->stage_len, 0, sizeof ctx->stage_len);
    ctx->stats.lock_sample = -1;
    ctx->stream_gpu_ms = 0;
    return PDT_OK;
}

// history a segment keeps in front of its new samples: the longest PLL warm-up (0.6 s of signal at most; the ARGOS build
// warms up for 8 s), the starting guess, and slack for the look-ahead of the block walkers
static uint64_t stream_history(const pdt_ctx *ctx)
{
    const double fs = (double)ctx->cfg.sample_rate;
    const double w = ctx->cfg.pll_warm ? (double)ctx->cfg.pll_warm : (ctx->cfg.mode == PDT_MODE_ARGOS ? 2.0 : 0.6) * fs;
    return (uint64_t)(w + 0.03 * fs) + 8192;
}

// local origin alignment: reference chunks (sampler seams), and for the interpolating FIR its ring of 26 inputs, whose
// phase decides the order of every output's accumulation
static uint64_t stream_align(const pdt_ctx *ctx)
{
    const uint64_t chunk = ctx->cfg.chunk;
    if (ctx->cfg.mode == PDT_MODE_ARGOS) return chunk;
    uint64_t a = chunk, b = 26;
    while (b) { const uint64_t t = a % b; a = b; b = t; }
    return chunk / a * 26;
}

// Demodulate the samples [stream_done, upto) of the window (whole chunks, or everything at the end of the stream) from the
// carried state, append the frames that became final to frames_host / stream_new, then let the window slide.
// segment_begin / segment_end bracket the run (demod_common in one piece, or its enqueue and finish phases with the wait for
// the segment's last bytes in between: demod_overlapped).
static void segment_begin(pdt_ctx *ctx, bool final_seg)
{
    StreamCarry &C = ctx->sc;
    const InFmt f = in_fmt(ctx->stream_fmt);
    C.active = true;
    C.final_seg = final_seg;
    C.first = (long long)ctx->stream_done;
    // (in place: the window is a view into the resident capture -- it "slides" by moving its base, not its samples)
    ctx->pcm_dev = (const unsigned char *)ctx->stream_in.p + (C.in_place ? (size_t)C.origin * (size_t)f.pcm_bytes : 0);
    ctx->pcm_fmt = f.pcm_fmt;
}

static int segment_end(pdt_ctx *ctx, uint64_t upto, bool final_seg);

static int stream_segment(pdt_ctx *ctx, uint64_t upto, bool final_seg)
{
    segment_begin(ctx, final_seg);
    const int rc = demod_common(ctx, upto);
    ctx->sc.active = false;
    if (rc) return rc;
    return segment_end(ctx, upto, final_seg);
}

static int segment_end(pdt_ctx *ctx, uint64_t upto, bool final_seg)
{
    StreamCarry &C = ctx->sc;
    for (const pdt_frame &f : C.seg_frames) {
        ctx->frames_host.push_back(f);
        ctx->stream_new.push_back(f);
    }
    ctx->stream_done = upto;
    ctx->have_frames = true;
    ctx->frames_on_device = 0;                      // (the device holds the last segment's records only)
    pdt_stats &S = ctx->stats;
    S.samples = C.origin + upto;
    S.out_samples = S.samples * ctx->interp;
    S.symbols = C.nsym_total;
    S.bits = C.nbits_total;
    S.frames = ctx->frames_host.size();
    S.lock_sample = C.lock_sample;
    S.lock_freq_hz = C.lock_freq_hz;
    S.avg_phase = C.avg_at_lock;
    S.norm_factor = C.norm_factor;
    S.interp = ctx->interp;
    S.ntaps = ctx->ntaps;
    ctx->stream_gpu_ms += S.gpu_ms;
    S.gpu_ms = ctx->stream_gpu_ms;
    S.segments += 1;
    if (final_seg) return PDT_OK;
    // ---- slide the window: the new origin is the largest aligned position that leaves the history in front of the next
    // new sample; the input window and the tails later segments look back on move with it
    uint64_t align = stream_align(ctx);
    if (C.in_place && (align & 3)) align *= (align & 1) ? 4 : 2;     // the view's base stays 16-byte aligned
    // (the overlapped ingest cuts its segments where the whole-capture kernels' units begin, and keeps the window's origin --
    // and with it every segment's first new sample -- on the same grid: demod_overlapped, run_capture's seg_fast)
    if (C.place_align) align = C.place_align;
    const uint64_t hist = stream_history(ctx);
    const uint64_t done_g = C.origin + ctx->stream_done;
    const uint64_t new_origin = done_g > hist ? (done_g - hist) / align * align : 0;
    if (new_origin > C.origin) {
        const uint64_t d = new_origin - C.origin;
        const size_t fb = (size_t)in_fmt(ctx->stream_fmt).pcm_bytes, es = (size_t)ctx->elem;
        const uint32_t ip = ctx->interp;
        const bool need_lock = ctx->cfg.mode == PDT_MODE_ARGOS || ctx->cfg.chain == PDT_CHAIN_LIVE;
        const uint64_t chunk = ctx->cfg.chunk;
        // (source and destination overlap: through a scratch buffer)
        auto slide = [&](DevBuf &buf, size_t elem, uint64_t src_first, uint64_t count) -> int {
            if (!count || !buf.p) return PDT_OK;
            int r = ctx->mag.ensure((size_t)count * elem + 64);
            if (r) return r;
            HIP_TRY(hipMemcpyAsync(ctx->mag.p, (unsigned char *)buf.p + (size_t)src_first * elem, (size_t)count * elem, hipMemcpyDeviceToDevice, ctx->stream));
            HIP_TRY(hipMemcpyAsync((unsigned char *)buf.p + (size_t)(src_first - d) * elem, ctx->mag.p, (size_t)count * elem, hipMemcpyDeviceToDevice, ctx->stream));
            return PDT_OK;
        };
        int r;
        // input: everything from the new origin on
        if (!C.in_place && (r = slide(ctx->stream_in, fb, d, ctx->stream_have - d))) return r;
        // PLL output: the FIR looks 25 inputs back; lock signal / AGC output: the sampler's stale reads reach one chunk back
        const uint64_t keep_pll = std::min<uint64_t>(ctx->stream_done - d, 256);
        {
            // these windows are indexed like the input (x interp for the AGC output): move [done - keep, done) down by d
            auto slide_tail = [&](DevBuf &buf, uint64_t scale, uint64_t keep) -> int {
                if (!buf.p) return PDT_OK;
                const uint64_t end = ctx->stream_done * scale, dd = d * scale;
                const uint64_t k = std::min<uint64_t>(keep, end - dd);
                int r2 = ctx->mag.ensure((size_t)k * es + 64);
                if (r2) return r2;
                HIP_TRY(hipMemcpyAsync(ctx->mag.p, (unsigned char *)buf.p + (size_t)(end - k) * es, (size_t)k * es, hipMemcpyDeviceToDevice, ctx->stream));
                HIP_TRY(hipMemcpyAsync((unsigned char *)buf.p + (size_t)(end - k - dd) * es, ctx->mag.p, (size_t)k * es, hipMemcpyDeviceToDevice, ctx->stream));
                return PDT_OK;
            };
            if ((r = slide_tail(ctx->pll, 1, keep_pll))) return r;
            if (need_lock && (r = slide_tail(ctx->lock, 1, chunk + 256))) return r;
            if ((r = slide_tail(ctx->agc, ip, (chunk + 256) * ip))) return r;
        }
        C.origin = new_origin;
        ctx->stream_have -= d;
        ctx->stream_done -= d;
    }
    return PDT_OK;
}

// n_new input samples have landed behind the kept ones of a real or wideband stream (HaloCarry): produce every output whose
// right halo is there (all of them when the stream ends: zeros beyond), append them to the stream's window, keep the next
// output's left halo and everything from the sample it is centred on.  A converter makes one output per D inputs and reads
// `span` inputs on either side of an output's centre: the Hilbert front end is D = 1, span = AN_HALF (31 samples held back),
// the down-converter D = ch_decim, span = DDC_SPAN D (floor(in / D) - 8 outputs so far).  base = out D is the input the next
// output is centred on, and buf[cur] begins at input base - left.  That D = 1 is the real front end as it used to be written:
//   m          = floor(in / D) - span / D - out; with D = 1, pending = in - out before the push, so m = pending + n_new - AN_HALF;
//   keep_left  = min(span, nbase), nbase = (out + m) D; with D = 1, left = min(AN_HALF, out) by induction, so it is min(AN_HALF, left + m);
//   kept tail  : from buffer offset nbase - keep_left - (base - left) = left + m - keep_left, of in - (nbase - keep_left) =
//                keep_left + pending + n_new - m samples; g0, the index of the first output, is base / D = out.
// After the final piece nothing is kept (no copy): the counters stay until pdt_stream_begin, nothing reads them.
static int front_convert(pdt_ctx *ctx, uint64_t n_new, bool final_piece)
{
    const InFmt f = in_fmt(ctx->stream_fmt);
    const bool wb = f.kind == IN_WB;
    int rc = wb ? channel_tables(ctx) : real_table(ctx);
    if (rc) return rc;
    HaloCarry &h = ctx->halo;
    const uint64_t D = wb ? (uint64_t)ctx->ch_decim : 1, span = wb ? (uint64_t)DDC_SPAN * D : (uint64_t)AN_HALF;
    const size_t fb = (size_t)f.bytes;
    const uint64_t base = h.out * D, total_in = h.in + n_new;
    const uint64_t outs = final_piece ? (total_in + D - 1) / D : (total_in / D > span / D ? total_in / D - span / D : 0);
    const uint64_t m = outs > h.out ? outs - h.out : 0;
    if ((rc = ctx->stream_in.ensure_keep(((size_t)(ctx->stream_have + m) + 64) * 8, (size_t)ctx->stream_have * 8))) return rc;
    const unsigned char *x = (const unsigned char *)h.buf[h.cur].p + (size_t)h.left * fb;
    void *out = (unsigned char *)ctx->stream_in.p + (size_t)ctx->stream_have * 8;
    const long long lo = -(long long)h.left, hi = (long long)(h.pending + n_new);
    if (wb)
        HIP_TRY(ddc_launch(ctx->stream, f.code, ctx->ch_decim, (const float *)ctx->ddc_taps.p, (const float *)ctx->an_tab.p,
                           channel_record(ctx, x, lo, hi, m, base, out)));
    else
        HIP_TRY(analytic_launch(ctx->stream, f.code, x, lo, hi, m, base, ctx->real_step, (const float *)ctx->an_tab.p, out));
    const uint64_t nbase = (h.out + m) * D;
    if (!final_piece) {
        const uint64_t keep_left = std::min<uint64_t>(span, nbase), start = nbase - keep_left - (base - h.left), keep = total_in - (nbase - keep_left);
        if (start) {
            DevBuf &dst = h.buf[h.cur ^ 1];
            if ((rc = dst.ensure((size_t)(keep + 64) * fb))) return rc;
            if (keep)
                HIP_TRY(hipMemcpyAsync(dst.p, (const unsigned char *)h.buf[h.cur].p + (size_t)start * fb, (size_t)keep * fb, hipMemcpyDeviceToDevice,
                                       ctx->stream));
            h.cur ^= 1;
        }
        h.left = keep_left;
        h.pending = total_in - nbase;
    } else {
        h.left = h.pending = 0;
    }
    h.in = total_in;
    h.out += m;
    ctx->stream_have += m;
    ctx->stream_total += m;
    return PDT_OK;
}

// Where the next n frames of the stream's input land: behind the window's samples (I,Q: the window grows only with the size
// of the pushes, not with the length of the stream), resp. behind the samples the converter keeps ...
static int stream_room(pdt_ctx *ctx, const InFmt &f, uint64_t n, unsigned char **at)
{
    const bool iq = f.kind == IN_IQ;
    DevBuf &buf = iq ? ctx->stream_in : ctx->halo.buf[ctx->halo.cur];
    const size_t held = (size_t)(iq ? ctx->stream_have : ctx->halo.left + ctx->halo.pending) * (size_t)f.bytes;
    const int rc = buf.ensure_keep(held + ((size_t)n + 64) * (size_t)f.bytes, held);
    *at = (unsigned char *)buf.p + held;
    return rc;
}

// ... and they are there: part of the window, resp. converted into it
static int stream_landed(pdt_ctx *ctx, const InFmt &f, uint64_t n, bool final_piece)
{
    if (f.kind != IN_IQ) return front_convert(ctx, n, final_piece);
    ctx->stream_have += n;
    ctx->stream_total += n;
    return PDT_OK;
}
// A large capture from a file: the spans arrive in the background (ingest_capture with a job) straight into the stream window,
// which holds the whole capture (its origin moves, its samples never do); the chain runs over it in a few segments with carried
// state -- the streaming path -- each as soon as its samples are there.  What the call leaves behind is what pdt_stream_end
// leaves: frames and statistics; the stage arrays are those of the last segment.
//
// Round 5.  (i) The segments are cut on the grid where a segment may use the whole-capture kernels (run_capture's seg_fast:
// k_mix_fir, k_agc_block_tr, table rows of several chunks): a multiple of the reference chunk, of the AGC maps' runs, of a
// 128-byte line and of 16 x 13 chunks (so that the table rows of either span begin at the first new chunk); the window's origin
// stays on that grid too.  (ii) They are UNEQUAL.  A segment of the fraction x of an hour at 250 ksps costs about 7 + 11.5 x ms
// of GPU time (the 7: one PLL warm-up of ~100 000 steps and the other stages' latency floors, whatever the length), the
// segments run one after the other, and the ingest takes ~67 ms: segment j + 1's samples must take at least as long to arrive
// as segment j takes to run -- x_{j+1} >= 0.104 + 0.172 x_j -- and what is exposed behind the last byte is the last segment
// alone.  By that model three segments of 64 / 22 / 14 % leave 8.6 ms there (two: 76 / 24 %, 9.7 ms; four equal ones, round 3:
// 12 ms of floor each, 49 ms in all); measured round robin on one box, 55 / 28 / 17 % did best (beside the running ingest a
// segment costs 5 + 25 x ms) and is the default below.  (iii) A segment's launch plan is recorded BEFORE the host waits for its last span, and the text
// of a finished segment is formatted and written (text_fd) while the next one runs.
// ... and so are its per-chunk reports handed to the caller's progress function (pdt_set_progress)
struct TextSink {
    int fd = -1;
    uint64_t bytes = 0;
    int rc = PDT_OK;
    pdt_progress_fn fn = nullptr;
    void *user = nullptr;
    std::thread th;
    std::vector<pdt_frame> batch;
    std::vector<pdt_chunk_report> reports;
    uint64_t rep_first = 0;
    pdt_stats so_far;
    void wait() { if (th.joinable()) th.join(); }
    void work()
    {
        if (fd >= 0 && !batch.empty()) {
            uint64_t w = 0;
            const int r = pdt_write_records(batch.data(), batch.size(), fd, &w);
            bytes += w;
            if (r) rc = r;
        }
        if (fn && !reports.empty()) fn(user, rep_first, reports.data(), reports.size(), &so_far);
    }
    // (the previous batch is on the file and reported before the next one starts)
    void push(const std::vector<pdt_frame> &frames, std::vector<pdt_chunk_report> &&rep, uint64_t first_chunk, const pdt_stats &st, bool in_background)
    {
        if ((fd < 0 || frames.empty()) && (!fn || rep.empty())) return;
        wait();
        if (rc) return;
        reports = std::move(rep);
        rep_first = first_chunk;
        so_far = st;
        try {
            if (fd >= 0) batch = frames; else batch.clear();
            if (in_background) {
                th = std::thread([this] { work(); });
                return;
            }
        } catch (const std::bad_alloc &) {
            rc = PDT_ERR_NOMEM;
            return;
        } catch (const std::exception &) {
        }
        work();
    }
};

static uint64_t lcm_u64(uint64_t a, uint64_t b)
{
    uint64_t x = a, y = b;
    while (y) { const uint64_t t = x % y; x = y; y = t; }
    return a / x * b;
}

static int demod_overlapped(pdt_ctx *ctx, const IngestSrc &src, uint64_t nframes, const InFmt &f, int text_fd, uint64_t *text_bytes)
{
    const size_t fb = (size_t)f.bytes;
    const auto t_call = std::chrono::steady_clock::now();
    int rc = pdt_stream_begin(ctx);
    if (rc) return rc;
    ctx->stream_fmt = f.code;
    if ((rc = ctx->stream_in.ensure(((size_t)nframes + 64) * fb))) return rc;
    IngestJob job;
    ctx->sc.in_place = true;
    ctx->sc.quality = ctx->keep_quality;          // (every cut below is a chunk boundary)
    ctx->report_samples = nframes;
    const uint64_t chunk = ctx->cfg.chunk;
    // the grid of the segment boundaries and of the window's origin (see above)
    const uint64_t grid = lcm_u64(lcm_u64(chunk * 208, 64 * 26 * (uint64_t)ctx->interp), 416);
    std::vector<double> cut;                                  // cumulative fractions of the capture at the segments' ends
    if (ctx->tune.overlap_segments > 0) {
        for (int k = 1; k < ctx->tune.overlap_segments; k++) cut.push_back((double)k / ctx->tune.overlap_segments);
    } else if (ctx->tune.overlap_split[0] > 0) {
        double acc = 0;
        for (int k = 0; k < 8 && ctx->tune.overlap_split[k] > 0; k++) { acc += ctx->tune.overlap_split[k]; if (acc < 1.0) cut.push_back(acc); }
    } else {
        cut = { 0.55, 0.83 };
    }
    std::vector<uint64_t> ends;
    if (grid * 8 <= nframes) {
        ctx->sc.place_align = grid;
        for (double c : cut) {
            const uint64_t e = (uint64_t)llround(c * (double)nframes / (double)grid) * grid;
            if (e > (ends.empty() ? 0 : ends.back()) && e + grid <= nframes) ends.push_back(e);
        }
    } else {
        // (an unusual chunk size: no such grid inside the capture -- the round-3 form: equal segments on chunk boundaries, the
        // stream path's kernels)
        for (double c : cut) {
            const uint64_t e = (uint64_t)(c * (double)nframes) / chunk * chunk;
            if (e > (ends.empty() ? 0 : ends.back()) && e < nframes) ends.push_back(e);
        }
    }
    ends.push_back(nframes);
    for (uint64_t e : ends) job.mark_bytes.push_back((size_t)e * fb);
    if ((rc = ingest_capture(ctx, src, (size_t)nframes * fb, ctx->stream_in.p, &job))) {
        (void)ingest_join(job);
        ctx->sc = StreamCarry();
        return rc;
    }
    TextSink sink;
    sink.fd = text_fd;
    sink.fn = ctx->progress_fn;
    sink.user = ctx->progress_user;
    uint64_t reported = 0;                        // chunks whose reports have been handed on
    auto segment_reports = [&]() {                // those of the segment that has just ended
        std::vector<pdt_chunk_report> r;
        const uint64_t have = ctx->chunk_host.size();
        if (sink.fn && have > reported) {
            r.resize((size_t)(have - reported));
            chunk_reports_range(ctx, reported, have, nframes, r.data(), ctx->sc.have_pending ? &ctx->sc.pending : nullptr);
        }
        return r;
    };
    ctx->batch_hint = 1;
    for (size_t k = 0; k < ends.size() && !rc; k++) {
        const bool last = k + 1 == ends.size();
        const uint64_t upto = ends[k];
        const auto t0 = std::chrono::steady_clock::now();
        ctx->stream_have = upto - ctx->sc.origin;                   // (window-local, as the pushes keep it)
        ctx->stream_total = upto;
        const uint64_t win = upto - ctx->sc.origin;
        segment_begin(ctx, last);
        rc = demod_common(ctx, win, RUN_ENQUEUE);                   // the segment's launch plan (host only) ...
        const auto t1 = std::chrono::steady_clock::now();
        if (!rc) rc = ingest_wait_mark(ctx, job, k, ctx->stream);      // ... then its last bytes ...
        const auto t2 = std::chrono::steady_clock::now();
        if (last) ctx->ingest_ms = std::chrono::duration<double, std::milli>(t2 - t_call).count();
        if (!rc) {
            pdt_ctx *self = ctx;
            rc = execute_plans(&self, 1);                           // ... then the launches
        }
        const auto t2a = std::chrono::steady_clock::now();
        if (!rc) rc = demod_common(ctx, win, RUN_FINISH);
        const auto t2b = std::chrono::steady_clock::now();
        ctx->sc.active = false;
        ctx->pending = false;
        if (!rc) rc = segment_end(ctx, win, last);
        const auto t2c = std::chrono::steady_clock::now();
        if (!rc && !last) {
            try {
                const uint64_t first_chunk = reported;
                std::vector<pdt_chunk_report> r = segment_reports();
                reported += r.size();
                sink.push(ctx->sc.seg_frames, std::move(r), first_chunk, ctx->stats, true);
            } catch (const std::bad_alloc &) {
                rc = PDT_ERR_NOMEM;
            }
        }
        if (ctx->tune.debug_overlap) {
            const auto t3 = std::chrono::steady_clock::now();
            auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
            fprintf(stderr, "segment %zu: upto %llu window %llu: plan %.2f ms, waited %.2f ms for the spans, run %.2f ms = launch %.2f + finish %.2f + end %.2f + sink %.2f (gpu %.2f so far)\n", k,
                    (unsigned long long)upto, (unsigned long long)win, ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t2, t2a), ms(t2a, t2b), ms(t2b, t2c), ms(t2c, t3), ctx->stats.gpu_ms);
            for (const pdt_kernel_time &kt : ctx->ktimes) fprintf(stderr, "    %-16s %8.3f ms\n", kt.name, kt.total_ms);
        }
    }
    ctx->sc.in_place = false;
    const int rj = ingest_join(job);
    sink.wait();
    if (!rc && !rj) {
        if (sink.rc) rc = sink.rc;
        else {
            try {
                const uint64_t first_chunk = reported;
                std::vector<pdt_chunk_report> r = segment_reports();
                sink.push(ctx->sc.seg_frames, std::move(r), first_chunk, ctx->stats, false);
                rc = sink.rc;
            } catch (const std::bad_alloc &) {
                rc = PDT_ERR_NOMEM;
            }
        }
    }
    if (text_bytes) *text_bytes = sink.bytes;
    ingest_publish(ctx);
    stream_reset(ctx);          // the stream machinery was borrowed: leave no stream behind, keep frames and statistics
    return rc ? rc : rj;
}

// A capture that does not fit the device in one piece (window_piece_for): the streaming path with a bounded window, fed from
// the file (or the caller's memory) `piece` samples at a time -- what a caller of pdt_stream_push_* would do by hand, with the
// threaded ingest in place of one pageable copy per push, the text of a finished piece written and its per-chunk reports
// handed on while the next piece is read (as demod_overlapped does).  Every cut is a chunk boundary; the window's origin
// stays on the grid where a segment may take the whole-capture kernels (run_capture: seg_fast) when the pieces are large
// enough for that to matter.  The state it leaves is demod_overlapped's: frames, text, statistics and reports of the whole
// capture, stage arrays of the last piece.
static int demod_windowed(pdt_ctx *ctx, const IngestSrc &src, uint64_t nframes, const InFmt &f, int text_fd, uint64_t *text_bytes, uint64_t piece)
{
    if (ctx->keep_agc_raw) return PDT_ERR_NOMEM;      // (the pre-Squelch stream of the WHOLE capture was asked for: that does not fit)
    const size_t fb = (size_t)f.bytes;                // per frame of the source
    int rc = pdt_stream_begin(ctx);
    if (rc) return rc;
    ctx->stream_fmt = f.code;
    ctx->sc.quality = ctx->keep_quality;              // (every cut below is a chunk boundary)
    ctx->report_samples = nframes;
    const uint64_t chunk = ctx->cfg.chunk;
    const uint64_t grid = lcm_u64(lcm_u64(chunk * 208, 64 * 26 * (uint64_t)ctx->interp), 416);
    if (piece >= 4 * grid) {
        piece = piece / grid * grid;
        ctx->sc.place_align = grid;
    }
    TextSink sink;
    sink.fd = text_fd;
    sink.fn = ctx->progress_fn;
    sink.user = ctx->progress_user;
    uint64_t reported = 0, pushed = 0;
    double ingest_ms = 0;
    auto segment_reports = [&]() {
        std::vector<pdt_chunk_report> r;
        const uint64_t have = ctx->chunk_host.size();
        if (sink.fn && have > reported) {
            r.resize((size_t)(have - reported));
            chunk_reports_range(ctx, reported, have, nframes, r.data(), ctx->sc.have_pending ? &ctx->sc.pending : nullptr);
        }
        return r;
    };
    for (bool last = false; !last && !rc;) {
        const uint64_t cnt = std::min<uint64_t>(piece, nframes - pushed);
        last = pushed + cnt == nframes;
        IngestSrc s = src;
        if (s.mem) s.mem += (size_t)pushed * fb; else s.off += pushed * fb;
        // the piece lands behind the window's samples, or behind the ones a real stream keeps and is converted into the window
        unsigned char *at = nullptr;
        if ((rc = stream_room(ctx, f, cnt, &at))) break;
        const auto t0 = std::chrono::steady_clock::now();
        if ((rc = ingest_capture(ctx, s, (size_t)cnt * fb, at))) break;
        ingest_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if ((rc = stream_landed(ctx, f, cnt, last))) break;
        pushed += cnt;
        const uint64_t upto = last ? ctx->stream_have : (ctx->sc.origin + ctx->stream_have) / chunk * chunk - ctx->sc.origin;
        if (upto <= ctx->stream_done && !last) continue;
        if ((rc = stream_segment(ctx, upto, last))) break;
        try {
            const uint64_t first_chunk = reported;
            std::vector<pdt_chunk_report> r = segment_reports();
            reported += r.size();
            sink.push(ctx->sc.seg_frames, std::move(r), first_chunk, ctx->stats, !last);
        } catch (const std::bad_alloc &) {
            rc = PDT_ERR_NOMEM;
        }
    }
    sink.wait();
    if (!rc && sink.rc) rc = sink.rc;
    if (text_bytes) *text_bytes = sink.bytes;
    ctx->ingest_ms = ingest_ms;
    ingest_publish(ctx);
    ctx->stats.windowed = 1;
    stream_reset(ctx);
    return rc;
}

static int stream_advance(pdt_ctx *ctx, uint64_t pushed, uint64_t *new_frames);

// All four push entries.  The first push opens a stream (as if pdt_stream_begin had been called), and the stream has the kind
// and format of its first push: a push of another one is refused -- PDT_ERR_STATE between the two I,Q formats, PDT_ERR_ARG
// wherever real or wideband input is involved (the codes the three front ends have always given).
static int stream_push(pdt_ctx *ctx, const void *host, uint64_t n, int format, uint64_t *new_frames)
{
    const InFmt f = in_fmt(format);
    if (!ctx || (!host && n) || f.kind == IN_NONE) return PDT_ERR_ARG;
    if (f.kind == IN_IQ && f.pcm_fmt && ctx->elem != 4) return PDT_ERR_FORMAT;
    if (f.kind == IN_WB && !ctx->ch_decim) return PDT_ERR_STATE;
    if (!ctx->stream_open) {
        int rb = pdt_stream_begin(ctx);
        if (rb) return rb;
        ctx->stream_open = true;
    }
    if (ctx->stream_fmt >= 0 && ctx->stream_fmt != format) return f.kind == IN_IQ && in_fmt(ctx->stream_fmt).kind == IN_IQ ? PDT_ERR_STATE : PDT_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->cfg.device));
    ctx->stream_fmt = format;
    ctx->stream_new.clear();
    if (new_frames) *new_frames = 0;
    unsigned char *at = nullptr;
    int rc = stream_room(ctx, f, n, &at);
    if (rc) return rc;
    if (n) HIP_TRY(hipMemcpyAsync(at, host, (size_t)n * (size_t)f.bytes, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = stream_landed(ctx, f, n, false))) return rc;
    return stream_advance(ctx, n, new_frames);
}

// demodulate the complete chunks the window holds now
static int stream_advance(pdt_ctx *ctx, uint64_t pushed, uint64_t *new_frames)
{
    const uint64_t chunk = ctx->cfg.chunk;
    const uint64_t whole = (ctx->sc.origin + ctx->stream_have) / chunk * chunk - ctx->sc.origin;   // local end of the complete chunks
    if (whole > ctx->stream_done) {
        const int rc = stream_segment(ctx, whole, false);
        if (rc) return rc;
    } else if (pushed) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));      // the caller's buffer is free to be reused when this returns
    }
    if (new_frames) *new_frames = ctx->stream_new.size();
    return PDT_OK;
}

int pdt_stream_push_pcm16(pdt_ctx *ctx, const int16_t *iq_host, uint64_t nframes, uint64_t *new_frames)
{
    return stream_push(ctx, iq_host, nframes, PDT_FMT_PCM16, new_frames);
}

int pdt_stream_push_f32(pdt_ctx *ctx, const float *iq_host, uint64_t nframes, uint64_t *new_frames)
{
    return stream_push(ctx, iq_host, nframes, PDT_FMT_F32, new_frames);
}

// (the real and the wideband entry report no new frames when they refuse a push; the I,Q entries leave *new_frames alone then)
int pdt_stream_push_real(pdt_ctx *ctx, const void *x_host, uint64_t n, int sample_format, uint64_t *new_frames)
{
    if (new_frames) *new_frames = 0;
    return in_fmt(sample_format).kind == IN_REAL ? stream_push(ctx, x_host, n, sample_format, new_frames) : PDT_ERR_ARG;
}

int pdt_stream_push_channel(pdt_ctx *ctx, const void *iq_host, uint64_t nframes, int sample_format, uint64_t *new_frames)
{
    if (new_frames) *new_frames = 0;
    return in_fmt(sample_format).kind == IN_WB ? stream_push(ctx, iq_host, nframes, sample_format, new_frames) : PDT_ERR_ARG;
}

int pdt_stream_end(pdt_ctx *ctx, uint64_t *new_frames)
{
    if (!ctx) return PDT_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->cfg.device));
    ctx->stream_open = false;                        // (whatever happens below, the stream is over)
    if (ctx->stream_fmt >= 0 && in_fmt(ctx->stream_fmt).kind != IN_IQ) {      // the held-back samples, closed with zeros
        const int rr = front_convert(ctx, 0, true);
        if (rr) return rr;
    }
    if (ctx->stream_fmt < 0) {                       // nothing was pushed: an empty capture
        ctx->stream_fmt = PDT_FMT_PCM16;
        int rc = ctx->stream_in.ensure(64);
        if (rc) return rc;
    }
    ctx->stream_new.clear();
    int rc = PDT_OK;
    if (ctx->stream_have > ctx->stream_done || ctx->stream_total == 0) {
        rc = stream_segment(ctx, ctx->stream_have, true);            // the short last chunk
    } else if (ctx->sc.have_pending) {
        // the stream ended on a chunk boundary inside a frame: the reference leaves that frame partial (Q11)
        ctx->frames_host.push_back(ctx->sc.pending);
        ctx->stream_new.push_back(ctx->sc.pending);
        ctx->sc.have_pending = false;
        ctx->stats.frames = ctx->frames_host.size();
    }
    if (new_frames) *new_frames = ctx->stream_new.size();
    return rc;
}

uint64_t pdt_stream_retained(const pdt_ctx *ctx) { return ctx ? ctx->stream_have + ctx->halo.pending : 0; }

uint64_t pdt_stream_frames(const pdt_ctx *ctx, pdt_frame *out, uint64_t max_frames)
{
    if (!ctx) return 0;
    const uint64_t n = std::min<uint64_t>(max_frames, ctx->stream_new.size());
    if (out && n) memcpy(out, ctx->stream_new.data(), (size_t)n * sizeof(pdt_frame));
    return n;
}

// ---------------------------------------------------------------- frame validation
static_assert(sizeof(pdt_tip_frame) == sizeof(pdt::TipFrame) && sizeof(pdt_tip_frame) == 12, "pdt_tip_frame layout");

// the summary of a validation run: the kernel's counters, and the modes MATLAB forms over the per-frame records
static void tip_reduce(const TipCounters &cnt, const pdt_tip_frame *recs, const pdt_frame *frames, unsigned nf, pdt_tip_summary *out)
{
    out->frames_checked = cnt.frames_checked;
    out->good_frames = cnt.good_frames;
    out->bad_chunks = cnt.bad_chunks;
    out->good_chunks = 5 * cnt.frames_checked - cnt.bad_chunks;
    out->time_frames = cnt.time_frames;
    // MATLAB mode(): most frequent value, the smallest one on ties
    unsigned best = 0;
    for (int v = 0; v < 256; v++) if (cnt.hist_sc[v] > best) { best = cnt.hist_sc[v]; out->spacecraft = v; }
    best = 0;
    for (int v = 0; v < 512; v++) if (cnt.hist_day[v] > best) { best = cnt.hist_day[v]; out->day = v; }
    // T0 = spacecraft ms of day minus the local frame time (daytimeDecode.m:26,34); frameTime is what the text
    // file holds ("%.5f"); the time stamps live on the host (pdt_timeaxis.h), so this small reduction does too
    std::vector<double> t0;
    for (unsigned f = 0; f < nf; f++) {
        const pdt_tip_frame &r = recs[f];
        if (r.has_time && r.day_ms >= 0) {
            const double t = round(frames[f].time * 1e5) / 1e5;
            const double v = (double)r.day_ms - t * 1000.0;
            if (v > 0) t0.push_back(round(v));
        }
    }
    std::sort(t0.begin(), t0.end());
    size_t best_n = 0;
    for (size_t i = 0; i < t0.size();) {
        size_t j = i;
        while (j < t0.size() && t0[j] == t0[i]) j++;
        if (j - i > best_n) { best_n = j - i; out->t0_ms = (int64_t)t0[i]; }
        i = j;
    }
}

int pdt_tip_check(pdt_ctx *ctx, pdt_tip_summary *out)
{
    if (!ctx || !out) return PDT_ERR_ARG;
    if (ctx->cfg.mode != PDT_MODE_POES) return PDT_ERR_ARG;             // TIP minor frames only
    if (hipSetDevice(ctx->cfg.device) != hipSuccess) return PDT_ERR_NOGPU;
    const unsigned nf = ctx->frames_on_device;
    if (!ctx->have_frames || nf != ctx->frames_host.size()) return PDT_ERR_STATE;   // nothing demodulated yet
    memset(out, 0, sizeof *out);
    out->spacecraft = -1;
    out->day = -1;
    out->t0_ms = -1;
    ctx->tip_host.assign(nf, pdt_tip_frame{});
    if (nf == 0) return PDT_OK;
    int rc;
    if ((rc = ctx->tip.ensure(sizeof(TipCounters) + (size_t)nf * sizeof(TipFrame)))) return rc;
    TipCounters *d_cnt = (TipCounters *)ctx->tip.p;
    TipFrame *d_rec = (TipFrame *)(d_cnt + 1);
    hipStream_t st = ctx->stream;
    Plan &PL = oneshot_begin(ctx);
    PL.memset_async(d_cnt, 0, sizeof(TipCounters));
    PDT_LAUNCH(256, k_tip_check, dim3((nf + 255) / 256), dim3(256), 0, st, (const FrameRec *)ctx->frames.p, nf, d_rec, d_cnt);
    TipCounters cnt;
    PL.copy(OP_D2H, &cnt, d_cnt, sizeof cnt);
    PL.copy(OP_D2H, ctx->tip_host.data(), d_rec, (size_t)nf * sizeof(TipFrame));
    if ((rc = oneshot_run(ctx))) return rc;
    tip_reduce(cnt, ctx->tip_host.data(), ctx->frames_host.data(), nf, out);
    return PDT_OK;
}

uint64_t pdt_tip_frames(const pdt_ctx *ctx, pdt_tip_frame *out, uint64_t max_frames)
{
    if (!ctx) return 0;
    const uint64_t n = std::min<uint64_t>(max_frames, ctx->tip_host.size());
    if (out && n) memcpy(out, ctx->tip_host.data(), (size_t)n * sizeof(pdt_tip_frame));
    return n;
}

// k_tip_check on a caller's records: they go to the device as the FrameRec the kernel reads, in a buffer of their own -- ctx->tip and
// tip_host (pdt_tip_frames) keep what the last pdt_tip_check left
int pdt_tip_check_records(pdt_ctx *ctx, const pdt_frame *frames, uint64_t n, pdt_tip_summary *out, pdt_tip_frame *per_frame)
{
    if (!ctx || !out || (!frames && n) || n >= (1ull << 31)) return PDT_ERR_ARG;
    if (ctx->cfg.mode != PDT_MODE_POES) return PDT_ERR_ARG;             // TIP minor frames only
    if (ctx->stream_open) return PDT_ERR_STATE;
    if (hipSetDevice(ctx->cfg.device) != hipSuccess) return PDT_ERR_NOGPU;
    memset(out, 0, sizeof *out);
    out->spacecraft = -1;
    out->day = -1;
    out->t0_ms = -1;
    if (n == 0) return PDT_OK;
    const unsigned nf = (unsigned)n;
    try {
        std::vector<FrameRec> in(nf);
        for (unsigned f = 0; f < nf; f++) {
            FrameRec &r = in[f];
            memset(&r, 0, sizeof r);
            r.bit_index = frames[f].bit_index;
            r.time_src = frames[f].time_src;
            r.inverted = frames[f].inverted;
            r.nbytes = frames[f].nbytes;
            r.complete = frames[f].complete;
            memcpy(r.bytes, frames[f].bytes, sizeof r.bytes);
        }
        std::vector<pdt_tip_frame> recs(nf);
        const size_t o_rec = (sizeof(TipCounters) + 15) & ~(size_t)15, o_in = (o_rec + (size_t)nf * sizeof(TipFrame) + 15) & ~(size_t)15;
        int rc;
        if ((rc = ctx->tip_recs.ensure(o_in + (size_t)nf * sizeof(FrameRec)))) return rc;
        unsigned char *w = (unsigned char *)ctx->tip_recs.p;
        TipCounters *d_cnt = (TipCounters *)w;
        TipFrame *d_rec = (TipFrame *)(w + o_rec);
        FrameRec *d_in = (FrameRec *)(w + o_in);
        hipStream_t st = ctx->stream;
        Plan &PL = oneshot_begin(ctx);
        PL.memset_async(d_cnt, 0, sizeof(TipCounters));
        PL.copy(OP_H2D, d_in, in.data(), (size_t)nf * sizeof(FrameRec));
        PDT_LAUNCH(256, k_tip_check, dim3((nf + 255) / 256), dim3(256), 0, st, (const FrameRec *)d_in, nf, d_rec, d_cnt);
        TipCounters cnt;
        PL.copy(OP_D2H, &cnt, d_cnt, sizeof cnt);
        PL.copy(OP_D2H, recs.data(), d_rec, (size_t)nf * sizeof(TipFrame));
        if ((rc = oneshot_run(ctx))) return rc;
        tip_reduce(cnt, recs.data(), frames, nf, out);
        if (per_frame) memcpy(per_frame, recs.data(), (size_t)nf * sizeof(pdt_tip_frame));
    } catch (const std::exception &) { return PDT_ERR_NOMEM; }
    return PDT_OK;
}

uint64_t pdt_num_frames(const pdt_ctx *ctx) { return ctx ? ctx->frames_host.size() : 0; }

uint64_t pdt_frames(const pdt_ctx *ctx, pdt_frame *out, uint64_t max_frames)
{
    if (!ctx) return 0;
    const uint64_t n = std::min<uint64_t>(max_frames, ctx->frames_host.size());
    if (out && n) memcpy(out, ctx->frames_host.data(), (size_t)n * sizeof(pdt_frame));
    return n;
}

int pdt_get_stats(const pdt_ctx *ctx, pdt_stats *out)
{
    if (!ctx || !out) return PDT_ERR_ARG;
    *out = ctx->stats;
    out->alloc_ms = (double)g_alloc_ns.load() * 1e-6;
    return PDT_OK;
}

// "%.5f" of a non-negative double without printf: value * 10^5 rounded to nearest, ties to even, on the EXACT binary value
// -- what glibc prints.  x = m * 2^e with a 53-bit m; m * 100000 fits 70 bits.  Returns the number of characters.
enum { PDT_TIME5_MAX = 336 };
static int format_time5(double x, char *out)
{
    if (!(x >= 0.0) || x >= 1e15) return snprintf(out, PDT_TIME5_MAX, "%.5f", x);   // (never the reference's range; DBL_MAX prints 315 characters)
    uint64_t bits;
    memcpy(&bits, &x, sizeof bits);
    const int be = (int)((bits >> 52) & 0x7ff);
    uint64_t m = bits & ((1ull << 52) - 1);
    int e;
    if (be == 0) e = -1074; else { m |= 1ull << 52; e = be - 1075; }
    unsigned __int128 N = (unsigned __int128)m * 100000u;
    unsigned __int128 q;
    if (e >= 0) {
        q = N << e;                                   // x < 1e15: no overflow
    } else {
        const int sh = -e;
        if (sh >= 120) q = 0;                         // x * 1e5 < 2^-49: rounds to zero
        else {
            q = N >> sh;
            const unsigned __int128 rem = N & (((unsigned __int128)1 << sh) - 1), half = (unsigned __int128)1 << (sh - 1);
            if (rem > half || (rem == half && (q & 1))) q++;
        }
    }
    const uint64_t ip = (uint64_t)(q / 100000u);
    unsigned fp = (unsigned)(q % 100000u);
    char tmp[24];
    int n = 0;
    uint64_t v = ip;
    do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    int w = 0;
    while (n) out[w++] = tmp[--n];
    out[w++] = '.';
    for (int d = 4; d >= 0; d--) { out[w + d] = (char)('0' + fp % 10); fp /= 10; }
    return w + 5;
}

uint64_t pdt_format_records(const pdt_frame *frames, uint64_t nframes, char *buf, uint64_t cap)
{
    // ByteSync.c:96-99,126-129 ("%.5f " / "%.5fi "), :62,100-101 ("%.2X "), :66-70 (newline after the last byte)
    static const char hex[] = "0123456789ABCDEF";
    uint64_t need = 0;
    char line[PDT_TIME5_MAX + 4 + 3 * 104 + 2];
    for (uint64_t k = 0; k < nframes; k++) {
        const pdt_frame &f = frames[k];
        int w = format_time5(f.time, line);
        if (f.inverted) line[w++] = 'i';
        line[w++] = ' ';
        const unsigned nb = f.nbytes > 104 ? 104u : f.nbytes;
        for (unsigned b = 0; b < nb; b++) {
            line[w++] = hex[f.bytes[b] >> 4];
            line[w++] = hex[f.bytes[b] & 15];
            line[w++] = ' ';
        }
        if (f.complete) line[w++] = '\n';
        if (buf && need < cap) memcpy(buf + need, line, (size_t)std::min<uint64_t>((uint64_t)w, cap - need));
        need += (uint64_t)w;
    }
    return need;
}

uint64_t pdt_format_frames(const pdt_ctx *ctx, char *buf, uint64_t cap)
{
    if (!ctx) return 0;
    return pdt_format_records(ctx->frames_host.data(), ctx->frames_host.size(), buf, cap);
}

// The reference writes its output file byte by byte while it demodulates (fprintf, ByteSync.c:62-101).  Here the text exists
// only after the run: an hour of POES is 36 000 lines, 12 MB.  A few threads take a slice of the frames each: format it into a
// buffer of their own and pwrite it at its place as soon as the sizes of the slices in front are known (the writes queue on
// the inode, but behind the formatting of the other slices instead of after it).  Measured on the GPU box's tmpfs: formatting
// 2.5 ms on one thread, the write 2.3 ms; a shared mapping of the file filled in place by all threads was slower (4.3 ms: the
// page faults of a fresh tmpfs mapping cost more than the copy they save).  A descriptor that cannot seek takes the text in order.
int pdt_write_records(const pdt_frame *frames, uint64_t nframes, int fd, uint64_t *bytes_written)
{
    if (bytes_written) *bytes_written = 0;
    if (fd < 0 || (!frames && nframes)) return PDT_ERR_ARG;
    if (!nframes) return PDT_OK;
    off_t at0 = lseek(fd, 0, SEEK_CUR);
    {
        // pwrite on an O_APPEND descriptor ignores its offset and appends (Linux): the slices would land in completion order
        const int fl = fcntl(fd, F_GETFL);
        if (fl >= 0 && (fl & O_APPEND)) at0 = -1;            // ... so such a descriptor takes the text in order, like a pipe
    }
    const int T = at0 < 0 ? 1 : (int)std::max<uint64_t>(1, std::min<uint64_t>(6, nframes / 2048));
    std::vector<uint64_t> first;
    std::unique_ptr<std::atomic<long long>[]> size;
    try {                                                     // (no exception crosses the C boundary, in this thread or a worker)
        first.resize((size_t)T + 1);
        size.reset(new std::atomic<long long>[(size_t)T]);
    } catch (const std::bad_alloc &) { return PDT_ERR_NOMEM; }
    for (int t = 0; t <= T; t++) first[(size_t)t] = nframes * (uint64_t)t / (uint64_t)T;
    for (int t = 0; t < T; t++) size[(size_t)t].store(-1);
    std::atomic<int> bad{0};                                  // 1: write error, 2: out of memory
    auto work = [&](int t) {
        const uint64_t a = first[(size_t)t], b = first[(size_t)t + 1];
        std::unique_ptr<char[]> buf(new (std::nothrow) char[(size_t)(b - a) * (PDT_TIME5_MAX + 4 + 3 * 104 + 2)]);     // (not touched beyond the text)
        if (!buf) {
            bad = 2;
            size[(size_t)t].store(0, std::memory_order_release);         // (the slices behind this one must not wait for ever)
            return;
        }
        const uint64_t sz = pdt_format_records(frames + a, b - a, buf.get(), ~0ull);
        size[(size_t)t].store((long long)sz, std::memory_order_release);
        uint64_t off = 0;
        for (int u = 0; u < t; u++) {
            long long v;
            while ((v = size[(size_t)u].load(std::memory_order_acquire)) < 0) std::this_thread::yield();
            off += (uint64_t)v;
        }
        size_t done = 0;
        while (done < sz && !bad) {
            const ssize_t r = at0 >= 0 ? pwrite(fd, buf.get() + done, sz - done, at0 + (off_t)off + (off_t)done)
                                       : write(fd, buf.get() + done, sz - done);
            if (r < 0 && errno == EINTR) continue;
            if (r <= 0) { bad = 1; return; }
            done += (size_t)r;
        }
    };
    std::vector<std::thread> pool;
    int started = 1;
    try {
        for (int t = 1; t < T; t++, started++) pool.emplace_back(work, t);
    } catch (const std::exception &) {                        // std::system_error (no thread), std::bad_alloc
    }
    work(0);
    for (int t = started; t < T; t++) work(t);                // slices that got no thread: here, in order
    for (auto &th : pool) th.join();
    if (bad == 2) return PDT_ERR_NOMEM;
    if (bad) return PDT_ERR_IO;
    uint64_t total = 0;
    for (int t = 0; t < T; t++) total += (uint64_t)size[(size_t)t].load();
    if (at0 >= 0) (void)lseek(fd, at0 + (off_t)total, SEEK_SET);
    if (bytes_written) *bytes_written = total;
    return PDT_OK;
}

int pdt_write_frames(const pdt_ctx *ctx, int fd, uint64_t *bytes_written)
{
    if (!ctx) return PDT_ERR_ARG;
    return pdt_write_records(ctx->frames_host.data(), ctx->frames_host.size(), fd, bytes_written);
}

uint64_t pdt_stage_len(const pdt_ctx *ctx, int stage)
{
    if (!ctx || stage < 0 || stage >= PDT_ST_COUNT) return 0;
    return ctx->stage_len[stage];
}

int64_t pdt_read_stage(const pdt_ctx *ctx, int stage, uint64_t first, uint64_t count, void *out)
{
    if (!ctx || !out || stage < 0 || stage >= PDT_ST_COUNT) return PDT_ERR_ARG;
    const uint64_t len = ctx->stage_len[stage];
    if (first >= len) return 0;
    count = std::min<uint64_t>(count, len - first);
    const void *src = nullptr;
    size_t es = ctx->elem;
    switch (stage) {
    case PDT_ST_PLL: src = ctx->pll.p; break;
    case PDT_ST_LOCK: src = ctx->lock.p; break;
    case PDT_ST_FIR: src = ctx->fir.p; break;
    case PDT_ST_AGC: src = ctx->agc.p; break;
    case PDT_ST_AGC_RAW: src = ctx->agc_raw.p; break;
    case PDT_ST_SYM: src = ctx->sym.p; break;
    case PDT_ST_SYMIDX: src = ctx->symidx.p; es = 8; break;
    case PDT_ST_BITS: src = ctx->bits.p; es = 1; break;
    case PDT_ST_BITSYM: src = ctx->bitsym.p; es = 4; break;
    case PDT_ST_ANALYTIC: src = ctx->analytic.p; es = 8; break;
    case PDT_ST_CHANNEL: src = ctx->channel.p; es = 8; break;
    }
    if (!src) return PDT_ERR_STATE;
    if (hipSetDevice(ctx->cfg.device) != hipSuccess) return PDT_ERR_NOGPU;
    if (hipMemcpy(out, (const unsigned char *)src + first * es, (size_t)count * es, hipMemcpyDeviceToHost) != hipSuccess)
        return PDT_ERR_NOGPU;
    return (int64_t)count;
}

int pdt_kernel_times(const pdt_ctx *ctx, pdt_kernel_time *out, int max_entries)
{
    if (!ctx) return 0;
    const int n = std::min<int>(max_entries, (int)ctx->ktimes.size());
    if (out)
        for (int i = 0; i < n; i++) out[i] = ctx->ktimes[i];
    return (int)ctx->ktimes.size();
}

}  // extern "C"

