// pdt_chain.inc -- the chain's launch recording, templated on the build's DECIMAL_TYPE: run_capture (every stage of
// POESTIPdemod/main.c:373-492 resp. ARGOSdemod/main.c:250-306 recorded as a launch plan), finish_capture (read-back, time stamps,
// the state a stream segment hands on) and the stage-level entries.  Included by pdt_chain_f32.hip and pdt_chain_f64.hip, each
// of which instantiates it for one type -- and with it every kernel that type's chain launches.
#include "pdt_rt.h"

namespace pdtrt {
PDT_WIDE_INSTANCES(extern, float)
PDT_WIDE_INSTANCES(extern, double)

// The finish phase of a demodulation call (RUN_ALL / RUN_FINISH): wait for the launches, read the scalars, the lock record and
// the frame records back, put the host-side time stamps on the frames (SURVEY Appendix B Q1/Q2/Q4), fill the statistics; for
// a stream segment, carry every stage's state to the next one.  (Round 5: split off run_capture.)
template <typename T> int finish_capture(pdt_ctx *ctx, uint64_t n, const FinishArgs &FA)
{
    const bool argos = FA.argos, need_lock = FA.need_lock, fuse_mix = FA.fuse_mix;
    const long long N = FA.N, n_out = FA.n_out, chunk = FA.chunk, chunk_out = FA.chunk_out, first = FA.first, first_out = FA.first_out,
                    sym_cap = FA.sym_cap;
    const int interp = FA.interp, ntaps = FA.ntaps;
    const uint32_t hit_cap = FA.hit_cap, frame_cap = FA.frame_cap;
    const SyncParams &SP = FA.SP;
    const T Fs = (T)ctx->cfg.sample_rate;
    StreamCarry *seg = ctx->sc.active ? &ctx->sc : nullptr;
    FrameRec *d_frames = (FrameRec *)ctx->frames.p;
    (void)first_out;
    if (!ctx->pending || ctx->pend_n != n) return PDT_ERR_STATE;
    ctx->pending = false;
    pdt_ctx *lead = ctx->leader ? ctx->leader : ctx;
    if (seg && seg->in_place && !ctx->tune.sync_block) {
        // the overlapped ingest: wait for the segment WITHOUT sitting inside the runtime -- the ingest's submitter thread is
        // queueing copies all the while (a blocking hipStreamSynchronize here held it up: the copies stopped for as long as a
        // segment's kernels ran, tools/jobs/r5_e2e_ab.sh)
        for (;;) {
            const hipError_t e = hipEventQuery(lead->ev1);
            if (e == hipSuccess) break;
            if (e != hipErrorNotReady) { HIP_TRY(e); }
            (void)hipGetLastError();
            std::this_thread::sleep_for(std::chrono::microseconds(40));
        }
    }
    HIP_TRY(hipStreamSynchronize(lead->stream));
    const DevScalars &sc = *ctx->pend_sc;
    PllLockInfo<T> info;
    memcpy(&info, ctx->pend_info, sizeof info);
    const uint32_t got_frames = ctx->pend_got_frames;
    if (sc.nframes > frame_cap || sc.nhits > hit_cap || (long long)sc.nsym > sym_cap) {
        fprintf(stderr, "libpdt: internal capacity exceeded (frames %u/%u hits %u/%u symbols %llu/%lld)\n", sc.nframes,
                frame_cap, sc.nhits, hit_cap, sc.nsym, sym_cap);
        return PDT_ERR_STATE;
    }
    std::vector<FrameRec> recs(sc.nframes);
    if (sc.nframes) {
        const uint32_t have = std::min<uint32_t>(sc.nframes, got_frames);
        if (have) memcpy(recs.data(), ctx->pinned, (size_t)have * sizeof(FrameRec));
        if (sc.nframes > have)
            HIP_TRY(hipMemcpy(recs.data() + have, d_frames + have, (size_t)(sc.nframes - have) * sizeof(FrameRec), hipMemcpyDeviceToHost));
    }
    ctx->last_nframes = sc.nframes;
    const uint64_t got_chunks = ctx->pend_chunks;     // (a segment: those of its new chunks, window-local counts -- see below)
    if (!seg) {
        ctx->chunk_host.clear();
        ctx->report_samples = n;
        if (got_chunks) {
            ctx->chunk_host.resize((size_t)got_chunks);
            memcpy(ctx->chunk_host.data(), ctx->qual_pin, (size_t)got_chunks * sizeof(ChunkInfo));
        }
    }
    ctx->pend_chunks = 0;

    float ms = 0;
    (void)hipEventElapsedTime(&ms, lead->ev0, lead->ev1);

    // time stamp of the bit whose symbol was taken at global interpolated-sample index g, in a capture of n_all samples
    // (SURVEY Appendix B Q1/Q2/Q4)
    // (captured by value: pdt_argos_messages stamps bits with it after this call has returned)
    auto frame_time = [ctx, argos, chunk, chunk_out, interp](long long g, long long n_all) -> double {
        if (argos && sizeof(T) == 4) return (double)ctx->axis_f.at((uint64_t)g + 1);     // the twin: float stamps (pdt_open)
        if (argos) return ctx->axis_d.at((uint64_t)g + 1);                   // waveDataTime[i] = (i+1)-th partial sum
        const long long c = g / chunk_out, rr = g % chunk_out;
        const long long j = rr / interp + 1;                                  // Q2: time of the *next* input sample
        const long long ns_c = std::min<long long>(chunk, n_all - c * chunk);
        if (j < ns_c) return (double)ctx->axis_f.at((uint64_t)(c * chunk + j + 1));
        if (ns_c == chunk || c == 0) return 0.0;                              // one past the array: never-written zero
        return (double)ctx->axis_f.at((uint64_t)((c - 1) * chunk + j + 1));   // stale value of the previous chunk
    };

    // ---- per-kernel timings (profile mode)
    auto collect_timers = [&]() {
    ctx->ktimes.clear();
    for (auto &t : ctx->timers) {
        float tms = 0;
        (void)hipEventElapsedTime(&tms, t.a, t.b);
        bool found = false;
        for (auto &k : ctx->ktimes)
            if (t.name == k.name) {
                k.launches++;
                k.total_ms += tms;
                found = true;
            }
        if (!found) {
            pdt_kernel_time k;
            memset(&k, 0, sizeof k);
            snprintf(k.name, sizeof k.name, "%s", t.name.c_str());
            k.launches = 1;
            k.total_ms = tms;
            ctx->ktimes.push_back(k);
        }
        if (!t.shared_a) ctx->event_pool.push_back(t.a);
        ctx->event_pool.push_back(t.b);
    }
    ctx->timers.clear();
    };

    ctx->bits_whole = !seg;                   // (pdt_argos_messages: a piece's bits are not the capture's)
    if (seg) {
        // ---- stream segment: hand the new frames to the stream code, carry every stage's state to the next segment
        SegTail<T> tail;
        memcpy(&tail, ctx->seg_pin + 4096, sizeof tail);
        const long long org_out = (long long)seg->origin * interp;
        const long long n_all = (long long)seg->origin + N;                   // samples of the stream so far
        const long long kept = (long long)seg->kept_bits.size();
        const long long sym_pad = 2 + (long long)(seg->nsym_total & 1u);
        const long long nbits_loc = (long long)sc.nbits;
        if ((long long)sc.nsym < sym_pad || nbits_loc < kept) return PDT_ERR_STATE;
        const uint64_t new_syms = sc.nsym - (uint64_t)sym_pad, new_bits = (uint64_t)(nbits_loc - kept);
        // PLL
        if (!seg->locked && info.lock_sample >= 0) {
            seg->locked = true;
            seg->lock_sample = info.lock_sample + (long long)seg->origin;
            seg->lock_freq_hz = (double)(info.freq_at_lock * Fs) / (2.0 * M_PI);
            seg->avg_at_lock = (double)info.avg_at_lock;
        }
        if (N > first || first == 0) {
            if (seg->locked && N > 0) {
                seg->phase = (double)tail.pll_phase;
                seg->freq = (double)tail.pll_freq;
                if (info.lock_sample == N - 1) {                              // locked on the very last sample: nothing walked after it
                    seg->phase = (double)info.st.phase;
                    seg->freq = (double)info.st.freq;
                }
                seg->locksig = need_lock ? (double)tail.locksig : (double)info.st.locksig;
                seg->avg = (double)info.st.avg_phase;
                seg->sweep = (double)info.st.sweep;
            } else if (N > 0) {
                seg->phase = (double)info.st.phase; seg->freq = (double)info.st.freq; seg->avg = (double)info.st.avg_phase;
                seg->locksig = (double)info.st.locksig; seg->sweep = (double)info.st.sweep;
            }
        }
        // StaticGain / AGC
        if (!seg->have_norm && N > 0) {
            T nv;
            memcpy(&nv, &sc.norm, sizeof(T));
            seg->norm_factor = (double)nv;
            seg->gain = (double)nv;
            seg->have_norm = true;
        }
        if (n_out - first_out > 0) seg->gain = (double)tail.agc_gain;
        // sampler, Manchester
        seg->sa = (double)tail.sampler.a; seg->sb = (double)tail.sampler.b; seg->sc = (double)tail.sampler.c;
        seg->have_sampler = true;
        if (sc.nsym >= 1) { seg->sym_m2 = (double)tail.sym_m2; seg->sym_m1 = (double)tail.sym_m1; }
        seg->clockmod = tail.clock;
        if (got_chunks) {
            // the reports of this segment's chunks: the window's counts include the history symbols and the kept bits (all in
            // front of the first new chunk), the capture's counts those of the earlier segments
            const ChunkInfo *ci = (const ChunkInfo *)ctx->qual_pin;
            for (uint64_t c = 0; c < got_chunks; c++) {
                ChunkInfo o = ci[c];
                if ((long long)o.sym_upto < sym_pad || (long long)o.bits_upto < kept) return PDT_ERR_STATE;
                o.sym_upto = o.sym_upto - (uint64_t)sym_pad + seg->nsym_total;
                o.bits_upto = o.bits_upto - (uint64_t)kept + seg->nbits_total;
                o.t0_src += org_out;
                ctx->chunk_host.push_back(o);
            }
            // averagePhase goes on behind the lock (the lock record holds its value AT the lock): the next segment's walkers
            // start from the value behind this segment's last sample = its last chunk's
            if (seg->locked && N > first) seg->avg = ci[got_chunks - 1].avg_phase;
        }
        seg->nsym_total += new_syms;
        seg->nbits_total += new_bits;
        seg->seg_new_symbols = new_syms;
        seg->seg_new_bits = new_bits;
        // bits the device kept: local indices [b0, nbits_loc)
        const long long b0 = nbits_loc - (long long)tail.nkeep;
        auto src_of = [&](long long pos) -> long long {                      // global interpolated-sample index behind local bit pos
            if (pos < kept) return seg->kept_src[(size_t)pos];
            return tail.src[pos - b0] + org_out;
        };
        // frames
        seg->seg_frames.clear();
        long long open_pos = -1;
        bool pend = false;
        for (unsigned f = 0; f < sc.nframes; f++) {
            const FrameRec &r = recs[f];
            if (!r.complete && !seg->final_seg) { open_pos = r.bit_index; }
            pdt_frame o;
            memset(&o, 0, sizeof o);
            o.bit_index = r.bit_index + (long long)seg->bit_base;
            o.inverted = argos ? 0 : r.inverted;      // (the ARGOS twin re-inverts such a packet's bits but stamps it like any other)
            o.nbytes = r.nbytes;
            o.complete = r.complete;
            memcpy(o.bytes, r.bytes, 104);
            const long long g = (r.bit_index < kept) ? seg->kept_src[(size_t)r.bit_index] : r.time_src + org_out;
            o.time_src = g;
            o.time = frame_time(g, n_all);
            if (!r.complete && !seg->final_seg) {
                seg->pending = o;                                             // reported when it completes (or at the stream's end)
                pend = true;
                break;
            }
            seg->seg_frames.push_back(o);
            seg->next_free = std::max<long long>(seg->next_free, o.bit_index + (long long)SP.span);
        }
        seg->have_pending = pend;
        // what the next segment sees of these bits: from the sync word of the open frame, else the last len - 1
        long long keep_from = std::max<long long>(0, nbits_loc - (long long)(SP.len - 1));
        if (open_pos >= 0) keep_from = std::max<long long>(0, open_pos - (long long)(SP.len - 1));
        if (keep_from < b0) return PDT_ERR_STATE;                             // (an open frame is shorter than the kept tail)
        std::vector<unsigned char> nb((size_t)(nbits_loc - keep_from));
        std::vector<long long> ns((size_t)(nbits_loc - keep_from));
        for (long long q = keep_from; q < nbits_loc; q++) {
            nb[(size_t)(q - keep_from)] = tail.bits[q - b0];
            ns[(size_t)(q - keep_from)] = src_of(q);
        }
        seg->kept_bits.swap(nb);
        seg->kept_src.swap(ns);
        seg->bit_base += (uint64_t)keep_from;
        ctx->stats.gpu_ms = ms;
        // pdt_read_stage after a push: the segment's own arrays, window-local (PLL / FIR / AGC from the window's origin; symbols
        // behind the two or three history symbols; bits behind the kept ones) -- a debugging aid, see tools/probes/stream_debug.py
        ctx->stage_len[PDT_ST_PLL] = (uint64_t)N;
        ctx->stage_len[PDT_ST_LOCK] = need_lock ? (uint64_t)N : 0;
        ctx->stage_len[PDT_ST_FIR] = ctx->stage_len[PDT_ST_AGC] = (uint64_t)n_out;
        ctx->stage_len[PDT_ST_AGC_RAW] = 0;
        ctx->stage_len[PDT_ST_SYM] = ctx->stage_len[PDT_ST_SYMIDX] = sc.nsym;
        ctx->stage_len[PDT_ST_BITS] = ctx->stage_len[PDT_ST_BITSYM] = sc.nbits;
        collect_timers();                     // (profile mode: the kernel groups of the LAST segment)
        return PDT_OK;
    }

    T norm_val;
    memcpy(&norm_val, &sc.norm, sizeof(T));
    pdt_stats &S = ctx->stats;
    memset(&S, 0, sizeof S);
    S.samples = n;
    S.out_samples = (uint64_t)n_out;
    S.symbols = sc.nsym;
    S.bits = sc.nbits;
    S.frames = sc.nframes;
    S.lock_sample = info.lock_sample;
    S.lock_freq_hz = (double)(info.freq_at_lock * Fs) / (2.0 * M_PI);         // CarrierTrackingPLL.c:269
    S.avg_phase = (double)info.avg_at_lock;
    S.norm_factor = (double)norm_val;
    S.interp = (uint32_t)interp;
    S.ntaps = (uint32_t)ntaps;
    S.pll_blocks = sc.counters[0];
    S.pll_seam_fixes = sc.counters[1];
    S.agc_blocks = sc.counters[2];
    S.agc_seam_fixes = sc.counters[3];
    S.gpu_ms = ms;
    S.gardner_parallel = (uint32_t)ctx->gardner_mode;
    const bool tabled = ctx->gardner_mode != 0;
    S.gardner_walked = tabled ? sc.gstats[2] : 0u;
    S.gardner_full_domain = tabled ? sc.gstats[1] : 0u;
    S.gardner_candidates = tabled ? sc.gstats[3] : 0u;
    S.sync_overflow = sc.sync_overflow;
    S.segments = 1;

    ctx->stage_len[PDT_ST_PLL] = (fuse_mix && !ctx->keep_pll) ? 0 : n;       // (k_mix_fir: the stream exists on request only)
    ctx->stage_len[PDT_ST_LOCK] = need_lock ? n : 0;
    ctx->stage_len[PDT_ST_FIR] = (uint64_t)n_out;
    ctx->stage_len[PDT_ST_AGC] = (uint64_t)n_out;
    ctx->stage_len[PDT_ST_AGC_RAW] = ctx->keep_agc_raw ? (uint64_t)n_out : 0;
    ctx->stage_len[PDT_ST_SYM] = sc.nsym;
    ctx->stage_len[PDT_ST_SYMIDX] = sc.nsym;
    ctx->stage_len[PDT_ST_BITS] = sc.nbits;
    ctx->stage_len[PDT_ST_BITSYM] = sc.nbits;

    // ---- time stamps (host): SURVEY Appendix B Q1/Q2/Q4
    ctx->frames_host.resize(sc.nframes);
    ctx->frames_on_device = sc.nframes;
    ctx->have_frames = true;
    ctx->tip_host.clear();
    for (unsigned f = 0; f < sc.nframes; f++) {
        pdt_frame &o = ctx->frames_host[f];
        const FrameRec &r = recs[f];
        memset(&o, 0, sizeof o);
        o.bit_index = r.bit_index;
        o.time_src = r.time_src;
        o.inverted = argos ? 0 : r.inverted;          // ARGOSdemodPortAudio/ByteSync.c:128: "%.5f " for the inverse word as well
        o.nbytes = r.nbytes;
        o.complete = r.complete;
        memcpy(o.bytes, r.bytes, 104);
        o.time = frame_time(r.time_src, N);
    }
    // the same stamp for any bit of this capture, for as long as its bits stay resident (pdt_argos_messages)
    ctx->bit_time = [frame_time, N](long long g) -> double { return frame_time(g, N); };

    collect_timers();
    if (ctx->progress_fn && !ctx->chunk_host.empty()) {          // pdt_set_progress: a whole capture reports once, at its end
        try {
            std::vector<pdt_chunk_report> rep(ctx->chunk_host.size());
            chunk_reports_range(ctx, 0, rep.size(), ctx->report_samples, rep.data(), nullptr);
            ctx->progress_fn(ctx->progress_user, 0, rep.data(), rep.size(), &ctx->stats);
        } catch (const std::bad_alloc &) {
            return PDT_ERR_NOMEM;
        }
    }
    return PDT_OK;
}

// ---------------------------------------------------------------- launch recipes
// One stage's launches on explicit pointers, lengths and parameters, recorded into PL.  The chain's rec_* methods call them where a
// capture takes that path, the stage entries (stage_*, below) call them on caller data: one copy of every grid and LDS rule.

// The AGC walkers' block and the cap of a block's warm-up, the caller's (pdt_config) or the defaults, in whole groups of four
// samples (any values give the same output; they only move time around).
// (the cap of a block's warm-up, which is 11 gain time constants = 11 gain / decay samples: weak input -- the noise in front
// of a pass -- means a high gain and a long memory; capped at one second, every seam of a minute of noise failed its check
// and was repaired in order, 219 ms; eight seconds cover gains up to ~700)
inline void agc_block_warm(const pdt_ctx *ctx, long long *Ba, long long *Wa)
{
    const bool argos = ctx->cfg.mode == PDT_MODE_ARGOS;
    const double fs_d = (double)ctx->cfg.sample_rate;
    const int interp = (int)ctx->interp;
    auto round4 = [](long long v) { return (v + 3) / 4 * 4; };
    *Ba = std::max<long long>(64, round4(ctx->cfg.agc_block ? ctx->cfg.agc_block : (long long)((argos ? 0.125 : 0.0625) * fs_d * interp)));
    *Wa = round4(ctx->cfg.agc_warm ? ctx->cfg.agc_warm : (long long)((argos ? 2.0 : 8.0) * fs_d * interp));
}

// StaticGain (main.c:384-389)
template <typename T> void rec_static_gain(Plan &PL, hipStream_t st, IqSrc src, long long n, T *mag, T level, double norm_override, T *d_norm)
{
    PDT_LAUNCH(256, k_static_gain<T>, dim3(1), dim3(256), 0, st, src, n, mag, level, norm_override, d_norm);
}

// Squelch (twin main.c:370)
template <typename T> void rec_squelch(Plan &PL, hipStream_t st, T *data, const T *lock, long long n, T thr)
{
    PDT_LAUNCH(256, k_squelch<T>, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, st, data, lock, n, thr);
}

// the low-pass filter on its own (LowPassFilter.c:13-125): k_fir_plain (ARGOS), the register-tiled interpolating form -- which
// also writes the AGC's affine tile maps when it is given a place for them -- or the generic one.  True: the register-tiled form.
template <typename T> bool rec_fir_unfused(pdt_ctx *ctx, Plan &PL, hipStream_t st, const T *d_in, long long N, T *d_out, AgcMap *tile_maps, T agc_decay)
{
    const bool argos = ctx->cfg.mode == PDT_MODE_ARGOS;
    const int interp = (int)ctx->interp, ntaps = (int)ctx->ntaps;
    const T *d_taps = (const T *)ctx->taps.p;
    const int opt = 8;
    const long long tile = (long long)PDT_FIR_THREADS * opt;
    const long long grid = (N * interp + tile - 1) / tile;
    if (argos) {
        const size_t sh = (size_t)(ntaps + tile + ntaps + 8) * sizeof(T);
        PDT_LAUNCH(PDT_FIR_THREADS, k_fir_plain<T>, dim3((unsigned)grid), dim3(PDT_FIR_THREADS), sh, st, d_in, N, ntaps, d_taps, d_out, opt);
        return false;
    }
    const int K = ntaps / interp;
    if constexpr (std::is_same<T, float>::value) {                     // (the float chain: POES is never built in double)
        const size_t sh_rt = (size_t)(65 * (K + 1) + 3 + 64 * K * interp) * sizeof(T);
        const long long tiles_rt = (N + 64ll * K - 1) / (64ll * K);
        // workgroups take tiles round robin; 32 per CU measured best (c3: 3.9 / 3.7 / 3.2 / 3.1 / 3.1 ms at 4 / 8 / 16 / 32 / 64):
        // the taps come by scalar loads per residue, nothing is kept across tiles, and a finer grain balances the tail
        const long long fir_tpb = ctx->tune.fir_wg_per_cu > 0 ? ctx->tune.fir_wg_per_cu : 32;
        const unsigned grid_rt = (unsigned)std::min<long long>(tiles_rt, 256ll * fir_tpb);
        if (K == 26 && sh_rt <= 64000 && ctx->taps_rot.p && !ctx->tune.fir_generic) {
            switch (interp) {
#define PDT_FIR_CASE(I)                                                                                                       \
    case I:                                                                                                                   \
        PDT_LAUNCH(PDT_FIR_THREADS, (k_fir_interp_rt<T, I, 26>), dim3(grid_rt), dim3(PDT_FIR_THREADS), sh_rt, st, d_in, N, (const T *)ctx->taps_rot.p, d_out, \
                           tile_maps, agc_decay);                                                                             \
        return true;
                PDT_FIR_CASE(1) PDT_FIR_CASE(2) PDT_FIR_CASE(3) PDT_FIR_CASE(4) PDT_FIR_CASE(5) PDT_FIR_CASE(6) PDT_FIR_CASE(7) PDT_FIR_CASE(8)
#undef PDT_FIR_CASE
            }
        }
    }
    const size_t sh = (size_t)(ntaps + tile / interp + K + 8) * sizeof(T);   // any other interpolation factor: generic form
    PDT_LAUNCH(PDT_FIR_THREADS, k_fir_interp<T>, dim3((unsigned)grid), dim3(PDT_FIR_THREADS), sh, st, d_in, N, interp, K, d_taps, d_out, opt);
    return false;
}

// NormalizingAGC through the per-lane block walkers (AGC.c:24-46,78-132): the affine block maps and the gain guesses from them
// (own_maps; else the caller has written d_guess), then the walkers.  *ckpt: the gain checkpoints they left for rec_agc_fix, or none.
template <typename T> int rec_agc_lanes(pdt_ctx *ctx, Plan &PL, hipStream_t st, const T *a_in, long long na, const AgcParams<T> &AP, T *d_norm,
                                        long long Ba, long long Wa, bool own_maps, AgcMap *d_maps, double *d_guess, const T *a_lock, T *a_out, T **ckpt)
{
    const long long nb = (na + Ba - 1) / Ba;
    if (own_maps) {
        PDT_LAUNCH(256, k_agc_affine<T>, dim3((unsigned)nb), dim3(256), 0, st, a_in, na, AP.decay, Ba, d_maps);
        PDT_LAUNCH(1024, k_agc_guess<T>, dim3(1), dim3(1024), 0, st, (const AgcMap *)d_maps, nb, (const T *)d_norm, d_guess, 1, nb);
    }
    // warm-up length in gain time constants: the affine guess is off by the accumulated float rounding of
    // the true recurrence only, so a few time constants make the trajectories agree to the last bit
    const double agc_K = ctx->tune.agc_k > 0 ? ctx->tune.agc_k : (sizeof(T) == 4) ? 11.0 : 34.0;
    // the walkers of the double-precision build leave checkpoints (blocks of at least two of them)
    *ckpt = nullptr;
    if (sizeof(T) == 8 && Ba >= 2 * PDT_AGC_CKPT) {
        const int rc = ctx->agc_ckpt.ensure((size_t)(nb + 64) * (size_t)(Ba / PDT_AGC_CKPT) * sizeof(T));
        if (rc) return rc;
        *ckpt = (T *)ctx->agc_ckpt.p;
    }
    PDT_LAUNCH(64, k_agc_block<T>, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, st, a_in, na, AP, d_norm, Ba, Wa, (const double *)d_guess, a_lock,
               a_out, (AgcSeam<T> *)ctx->seams_agc.p, agc_K, *ckpt);
    return PDT_OK;
}

// ... and the repair of the seams that did not close, in order from the first one
template <typename T> void rec_agc_fix(pdt_ctx *ctx, Plan &PL, hipStream_t st, const T *a_in, long long na, const AgcParams<T> &AP, long long Ba,
                                       const T *a_lock, T *a_out, DevScalars *d_sc, T *ckpt)
{
    PDT_LAUNCH(1024, k_agc_scan<T>, dim3(1), dim3(1024), 0, st, na, Ba, (const AgcSeam<T> *)ctx->seams_agc.p, &d_sc->agc_first_bad);
    PDT_LAUNCH(64, k_agc_fix<T>, dim3(1), dim3(64), 0, st, a_in, na, AP, Ba, a_lock, a_out, (AgcSeam<T> *)ctx->seams_agc.p, d_sc->counters,
               (const long long *)&d_sc->agc_first_bad, ckpt);
}

// MMClockRecovery: sequential, one wavefront
template <typename T> void rec_mm(Plan &PL, hipStream_t st, const T *in, const MmParams<T> &MP, T *d_sym, long long *d_symidx, DevScalars *d_sc,
                                  long long sym_cap, const SamplerCarry<T> &carry_in, int have_carry, SamplerCarry<T> *carry_out)
{
    PDT_LAUNCH(PDT_GARDNER_THREADS, (k_mm<T, 8192, 1024>), dim3(1), dim3(PDT_GARDNER_THREADS), 0, st, in, MP, d_sym, d_symidx, &d_sc->nsym, sym_cap,
               carry_in, have_carry, carry_out);
}

// GardenerClockRecovery by the sequential walker: one workgroup, chunk after chunk from the carried state
template <typename T> void rec_gardner_walk(Plan &PL, hipStream_t st, const T *in, const T *lock, const GardnerParams<T> &GP, T *d_sym, long long *d_symidx,
                                            DevScalars *d_sc, long long sym_cap, const SamplerCarry<T> &carry_in, SamplerCarry<T> *carry_out)
{
    PDT_LAUNCH(256, (k_gardner<T, GardnerLds<T>::LEN, GardnerLds<T>::OUT>), dim3(1), dim3(256), 0, st, in, lock, GP, d_sym, d_symidx, &d_sc->nsym,
               sym_cap, (const GardnerEntry<T> *)nullptr, carry_in, carry_out, 0ll, 1, (const unsigned char *)nullptr);
}

// ManchesterDecode in three passes: tile summaries, their scan, emission.  pad: the history symbols in front of the first one to
// decide; clock0 / bit0: the clock and the bits a stream has so far; clock_out: where the clock after the last symbol goes, or null.
template <typename T> void rec_manch_3pass(Plan &PL, hipStream_t st, const T *d_sym, DevScalars *d_sc, T thr, ManchTile *d_tiles, long long n_tiles,
                                           long long pad, unsigned clock0, unsigned long long bit0, unsigned *clock_out, unsigned char *d_bits,
                                           unsigned *d_bitsym, long long bit_cap)
{
    const unsigned long long *d_nsym = &d_sc->nsym;
    PDT_LAUNCH(PDT_TILE_THREADS, k_manch_tile<T>, dim3((unsigned)n_tiles), dim3(PDT_TILE_THREADS), 0, st, d_sym, d_nsym, thr, d_tiles, pad);
    PDT_LAUNCH(1024, k_manch_scan, dim3(1), dim3(1024), 0, st, d_tiles, d_nsym, &d_sc->nbits, pad, clock0, bit0, clock_out);
    PDT_LAUNCH(PDT_TILE_THREADS, k_manch_emit<T>, dim3((unsigned)n_tiles), dim3(PDT_TILE_THREADS), 0, st, d_sym, d_nsym, thr, d_tiles, d_bits, d_bitsym,
               bit_cap, pad);
}

// The chain's launch recording for one capture (or one segment of a stream): every stage of POESTIPdemod/main.c:373-492 resp.
// ARGOSdemod/main.c:250-306 recorded into the context's launch plan.  Round 6: one object per call, a method per stage (run_capture
// was one function of 1 080 lines); what the stages share -- constants, geometry, capacities, device pointers -- are its members,
// set by params() / geometry() / allocate() in that order.
template <typename T> struct Chain {
    pdt_ctx *ctx;
    uint64_t n;
    int phase;
    Plan &PL;
    PlanGroups L;
    Chain(pdt_ctx *c, uint64_t n_, int ph) : ctx(c), n(n_), phase(ph), PL(c->plan), L{c->plan, c->cfg.profile != 0} {}
    static long long round4(long long v) { return (v + 3) / 4 * 4; }

    bool argos = false;
    bool live = false;
    bool inject = false;
    bool need_lock = false;
    long long N = 0;
    int interp = 0;
    int ntaps = 0;
    long long n_out = 0;
    long long chunk = 0;
    long long chunk_out = 0;
    hipStream_t st = nullptr;
    StreamCarry *seg = nullptr;
    long long first = 0;
    long long first_out = 0;
    T Fs = 0;
    PllParams<T> PP{};
    AgcParams<T> AP{};
    T fsi = 0;
    GardnerParams<T> GP{};
    T baud = 0;
    bool argos_twin = false;
    T manch_thr = 0;
    SyncParams SP{};
    double fs_d = 0;
    long long Bp = 0;
    long long Wp = 0;
    long long Wacq = 0;
    long long Ba = 0;
    long long Wa = 0;
    bool seg_fast = false;
    bool fuse_mix = false;
    long long agc_tiles_per_block = 0;
    long long fused_tiles = 0;
    long long agc_maps_per_block = 0;
    double sym_rate = 0;
    double f_lim = 0;
    int lag = 0;
    long long nb_pll = 0;
    long long nb_agc = 0;
    double min_step = 0;
    long long n_chunks = 0;
    long long sym_cap = 0;
    long long bit_cap = 0;
    uint32_t hit_cap = 0;
    uint32_t frame_cap = 0;
    long long n_tiles = 0;
    long long n0 = 0;
    long long lt_tiles = 0;
    long long lt_elems = 0;
    bool quality = false;
    T avg_alpha = 0;
    long long tau_q = 0;
    long long Bq = 0;
    long long Wq = 0;
    long long nb_q = 0;
    double *d_q_zresp = nullptr;
    double *d_q_guess = nullptr;
    T *d_avgph = nullptr;
    bool ema_guess = false;
    long long We = 0;
    long long Be = 0;
    long long nb_ema = 0;
    double *d_ema_zresp = nullptr;
    double *d_ema_guess = nullptr;
    IqSrc d_pcm{};
    T *d_pll = nullptr;
    T *d_lock = nullptr;
    T *d_fir = nullptr;
    T *d_agc = nullptr;
    T *d_sym = nullptr;
    long long *d_symidx = nullptr;
    unsigned char *d_bits = nullptr;
    unsigned *d_bitsym = nullptr;
    ManchTile *d_tiles = nullptr;
    FrameRec *d_frames = nullptr;
    DevScalars *d_sc = nullptr;
    PllLockInfo<T> *d_info = nullptr;
    T *d_norm = nullptr;
    T *d_taps = nullptr;
    unsigned char *spin = nullptr;
    T *d_theta = nullptr;
    T *d_phi = nullptr;
    long long lt_groups = 0;
    long long grid_pll = 0;
    bool short_pays = false;
    int short_group = 0;
    T pll_consensus = 0;
    long long phase_groups = 0;
    double worst = 0;
    bool slow_wrap = false;
    T *d_ckpt = nullptr;
    PllPhaseHint *d_hint = nullptr;
    bool serial_excl = false;
    long long fix_regions = 0;
    long long fix_region_blocks = 0;
    bool quality_side = false;
    bool quality_term_fused = false;
    bool quality_after_fir = false;
    size_t ops_after_pll = 0;
    long long agc_last_block = 0;
    bool use_mm = false;
    bool use_table = false;
    GardnerDomain GD{};
    int span_rekey = 0, span_sub = 16, span_win2 = 1024;     // the staged span walk: chunks before the re-key (0: one stage), stage 2's lanes and window per row
    SamplerCarry<T> carry_in{};
    SegTail<T> *d_tail = nullptr;
    SamplerCarry<T> *d_carry_out = nullptr;
    long long sym_pad = 0;
    unsigned clock0 = 0;
    unsigned long long bit0 = 0;
    long long sync_min_pos = 0;

    // the loop constants of the chain: the mains' call-site constants (POESTIPdemod/main.c:32-46,413,429,438,445; ARGOSdemod/main.c:33-64,265-282)
    // or the caller's (pdt_set_loop_params); a stream segment's carried acquisition state
    int params()
    {
        int rc = PDT_OK;
        (void)rc;
        argos = ctx->cfg.mode == PDT_MODE_ARGOS;
        // the sound-card twin's chain (POESTIPdemodPortAudio/main.c:324-393): the twin's constants, the lock signal kept and
        // Squelch between PLL and FIR
        live = !argos && ctx->cfg.chain == PDT_CHAIN_LIVE;
        inject = ctx->inj.active && !ctx->sc.active;          // pdt_stage_pll
        need_lock = argos || live || inject;
        N = (long long)n;
        interp = (int)ctx->interp;
        ntaps = (int)ctx->ntaps;
        n_out = N * interp;
        chunk = (long long)ctx->cfg.chunk;
        chunk_out = chunk * interp;
        st = ctx->stream;
        // stream segment: the window [0, n) holds history before `first`; every stage starts at `first` from the carried state
        seg = ctx->sc.active ? &ctx->sc : nullptr;
        first = seg ? seg->first : 0;
        first_out = first * interp;

        // ---- parameters
        Fs = (T)ctx->cfg.sample_rate;
        PP = make_pll_params<T>(ctx);
        if (inject) {
            PP.want_lock = 1;
            if (ctx->inj.started && !ctx->inj.locked) {  // the acquisition goes on from the caller's state record
                PP.phase0 = (T)ctx->inj.phase; PP.freq0 = (T)ctx->inj.freq; PP.avg0 = (T)ctx->inj.avg; PP.locksig0 = (T)ctx->inj.locksig;
                PP.sweep0 = (T)ctx->inj.sweep; PP.i0 = 0;
            }
        }
        if (seg && first > 0 && !seg->locked) {          // the acquisition goes on where the last segment left it
            PP.phase0 = (T)seg->phase; PP.freq0 = (T)seg->freq; PP.avg0 = (T)seg->avg; PP.locksig0 = (T)seg->locksig;
            PP.sweep0 = (T)seg->sweep; PP.i0 = first;
        }
        fsi = output_rate<T>(ctx);
        AP = make_agc_params<T>(ctx);
        AP.squelch = argos ? 1 : 0;
        AP.squelch_thr = (T)0.15;                                                  // ARGOSdemod/main.c:46,276
        baud = sampler_baud<T>(ctx);
        GP = make_gardner_params<T>(ctx, n_out, chunk_out);
        if (argos && (size_t)chunk * sizeof(T) < 128 * 1024) {                    // Q16, below M_MMAP_THRESHOLD
            // (sizeof(T) = 4: the ARGOS sound-card twin, whose buffers are `chunk` floats, ARGOSdemodPortAudio/main.c:61-63)
            const unsigned long long req = (unsigned long long)sizeof(T) * (unsigned long long)chunk;
            const unsigned long long csz = (req + 8 + 15) & ~15ull;
            GP.argos_heap = 1;
            GP.argos_field_bits = csz | 1ull;
            GP.argos_even = (int)((csz - 8 - req) / sizeof(T));
        }
        argos_twin = argos && ctx->cfg.chain == PDT_CHAIN_LIVE;
        manch_thr = manchester_threshold<T>(ctx, argos, live);
        SP = make_sync_params(argos, argos_twin);

        return PDT_OK;
    }

    // block-parallel geometry: block and warm-up lengths of the PLL / AGC walkers, which kernels a segment may take (any values give the
    // same output; they only move time around)
    int geometry()
    {
        int rc = PDT_OK;
        (void)rc;
        // ---- block-parallel geometry (any values give the same output; they only move time around)
        fs_d = (double)ctx->cfg.sample_rate;
        Bp = ctx->cfg.pll_block ? ctx->cfg.pll_block : (long long)((argos ? 0.5 : 0.05) * fs_d);
        // (ARGOS: the loops only contract while a burst is on the air -- between bursts the detector sees noise and two close
        // trajectories are kicked apart as fast as they are pulled together -- so a warm-up must contain one whole burst: 2 s cover
        // a 1.5 s repetition period + one 0.36 s burst; measured on the 5-minute capture: 8 / 4 / 2 / 1 s -> 0 / 0 / 0 / 192 repaired
        // seams.  Sparser transmissions fall back on the seam repairs, as ever.)
        Wp = ctx->cfg.pll_warm ? ctx->cfg.pll_warm : (long long)((argos ? 2.0 : 0.3) * fs_d);
        if (!ctx->cfg.pll_warm && !argos) {
            // Measured (tools/pll_geom.py, 50 ksps): the probability that a block has not merged bit for bit after a
            // warm-up of W samples falls like 200 exp(-W / 2.82 tau), tau = 2 / alpha_trk the tracking loop's time
            // constant.  Aim at ~0.1 unhealthy seam per capture (a repair costs a sequential block walk, ~0.2 ms, against ~0.08 ms
            // for the extra 1.6 tau of warm-up): short captures get away with less than 0.3 s, hour-long ones need a little more.
            const double tau = 2.0 / (double)PP.alpha_trk;
            const double nb = std::max(1.0, (double)N / (double)std::max<long long>(1, Bp));
            // 200 nb exp(-w / 2.82 tau) = 0.1 expected unhealthy seams per capture.  (Round 3, an hour of 250 ksps, 61 000 blocks:
            // warm-up x1 / 0.85 / 0.7 / 0.55 -> 1 / 1 / 52 / 837 repairs, phase kernel 7.6 / 6.7 / 6.0 / 5.2 ms, repairs 1.4 / 1.2 / 2.0 /
            // 10.0 ms -- but the law with 50 in place of 2000 (x0.8) turned the same capture at six times the noise from 26 repairs in
            // 3 ms into 315 in 202 ms: where the loop barely contracts every open seam starts a cascade.  The long warm-up stays.)
            double w = 2.82 * tau * log(2000.0 * nb);
            w *= ctx->tune.pll_warm_scale;
            Wp = (long long)std::min(std::max(w, 0.15 * fs_d), 0.6 * fs_d);
        }
        Wacq = (long long)(0.02 * fs_d);             // acquisition-gain stage of the warm-up
        agc_block_warm(ctx, &Ba, &Wa);
        // (Round 6, ARGOS captures demodulated many at a time -- pdt_demod_batch_device: between bursts the AGC's gain is high and its
        // memory, gain / decay samples, long: most walkers replay the whole two-second cap of their warm-up for a block of an eighth
        // of a second, every sample is read 17 times -- 64 captures: 83 GB, 28 ms of the batch's 81.  A single capture needs the many
        // short blocks for their lanes, a batch has lanes to spare: blocks of one second, every sample read three times.)
        // (two-second blocks were measured too, for 32 and 64 captures: 17.8 / 19.7 ms against 11.8 / 15.0 -- too few lanes then)
        if (argos && !ctx->cfg.agc_block && ctx->batch_hint >= 8) Ba = (long long)(1.0 * fs_d * interp);
        if (!ctx->cfg.pll_block) {
            // One walker wavefront saturates the vector ALU of its SIMD (a wave64 instruction occupies the 16 lanes for 4 clocks), so
            // a second one on the same SIMD doubles the time of both: keep the walkers of everything that runs together -- this
            // capture, or the whole batch -- under ~one per SIMD (240 groups of four; the rest is left to the serial kernels).
            // (A capture on its own, round 3: 180 -- an hour at 250 ksps, where the warm-ups' re-reads press on HBM: blocks of 15 / 20 /
            // 25 / 30 / 40 thousand samples -> phase kernel 7.6 / 6.9 / 6.8 / 7.7 / 8.3 ms.)
            // (Round 4, with wavefront 0 out of the way -- it had been walking 7 B steps and favoured short blocks: the kernel sits under
            // the issue roof, (W + B) steps, and the HBM roof of its re-reads, W / B + 2 passes over the capture, at once; blocks of
            // 20 / 22.5 / 24 / 25 / 28 thousand samples -> 5.55 / 5.45 / 5.27 / 5.25 / 5.29 ms: 150 groups.)
            const long long groups_max = ctx->batch_hint > 1 ? 240 : 150;
            const long long share = std::max<long long>(1, groups_max / std::max(1, ctx->batch_hint));
            const long long b_min = (N + share * 256 - 1) / (share * 256);
            Bp = std::max(Bp, b_min);
        }
        Bp = std::min<long long>(Bp, std::max<long long>(N, 1));   // (one block at most: the LT layout keeps 64 blocks per tile)
        Bp = std::max<long long>(64, (Bp + 63) / 64 * 64);         // whole transposition groups of the LT layout (pdt_kernels_front.h)
        // mix and filter in one kernel (k_mix_fir: the PLL output never goes through HBM): the float chain at INTERP 1 with the
        // register-tiled taps; its runs and ring phases need blocks of a multiple of lcm(64, 208) = 832 samples
        // A stream segment may take the whole-capture kernels (k_mix_fir, the FIR kernel's AGC maps, k_agc_block_tr, table rows of
        // several chunks) when its first new sample sits where those kernels' units begin: a multiple of the mix + FIR kernel's run
        // (208 outputs: the AGC maps) and of a 128-byte line of the output streams (32 floats).  Round 5: the overlapped ingest of
        // an hour-long file cuts its segments there (demod_overlapped); a pushed stream gets there when its pushes happen to.
        seg_fast = seg && first_out % PDT_MF_RUN == 0 && first_out % 32 == 0 && !ctx->tune.seg_plain;
        fuse_mix = false;
        if constexpr (std::is_same<T, float>::value) {
            fuse_mix = !argos && !live && !inject && (!seg || seg_fast) && interp == 1 && ntaps == 26 && ctx->taps_rot.p && !ctx->tune.fir_generic &&
                       !ctx->tune.mix_unfused && N >= 832;
            if (fuse_mix && !ctx->cfg.pll_block) Bp = (Bp + 831) / 832 * 832;
            if (fuse_mix && Bp % 832 != 0) fuse_mix = false;
        }
        Ba = std::max<long long>(64, round4(Ba));
        // POES with the register-tiled FIR: AGC blocks made of whole FIR tiles (64 * 26 inputs), so that the FIR kernel can
        // deliver the AGC's affine tile maps itself (0 = not fused: explicit block size, ARGOS, generic FIR)
        agc_tiles_per_block = 0;
        fused_tiles = 0;
        agc_maps_per_block = 0;
        if (!argos && !ctx->cfg.agc_block && ntaps == 26 * interp && ctx->taps_rot.p && !ctx->tune.fir_generic &&
            !ctx->tune.agc_unfused && (!seg || (seg_fast && first_out % (64ll * 26 * interp) == 0) || (seg_fast && fuse_mix))) {
            const long long tile_out = 64ll * 26 * interp;
            agc_tiles_per_block = std::max<long long>(1, (Ba + tile_out / 2) / tile_out);
            // a walker's look-ahead ring takes 64 KiB of LDS: two wavefronts per CU, 512 on the chip.  An hour at 250 ksps has more
            // blocks than that (940 wavefronts = two rounds, the second one of a few stragglers): longer blocks, one round
            // (4.2 -> 3.5 ms; tools/jobs/agc_tpb.sh).  (A batch shares the chip: no gain measured there.)
            {
                const long long tiles = (n_out - first_out + tile_out - 1) / tile_out;
                const long long one_round = (tiles + 500ll * 64 - 1) / (500ll * 64);
                if (ctx->batch_hint <= 1 && tiles / agc_tiles_per_block > 512ll * 64 && one_round <= 4 * agc_tiles_per_block)
                    agc_tiles_per_block = one_round;
            }
            if (ctx->tune.agc_tpb) agc_tiles_per_block = ctx->tune.agc_tpb;
            Ba = agc_tiles_per_block * tile_out;
        }
        Wp = round4(Wp);
        Wa = round4(Wa);
        Wacq = round4(Wacq);
        // lag of the autocorrelation frequency guess: at least one Manchester symbol (so that the
        // modulation of the two samples is independent and the carrier term dominates the mean), while
        // pi/lag stays above the PLL's frequency limit
        sym_rate = (double)baud;
        f_lim = (double)PP.max_freq * fs_d / (2.0 * M_PI);
        lag = (int)ceil(fs_d / sym_rate);
        lag = std::max(1, std::min(lag, (int)(fs_d / (2.2 * f_lim))));
        lag = std::min(lag, 64);
        nb_pll = N / Bp + 2;
        nb_agc = (n_out - first_out + Ba - 1) / Ba + 1;

        return PDT_OK;
    }

    // capacities and buffers (a context keeps its buffers from capture to capture: DevBuf::ensure), the device pointers of this run
    int allocate()
    {
        int rc = PDT_OK;
        (void)rc;
        // ---- capacities
        min_step = (double)GP.step - 0.25;
        if (ctx->cfg.sampler == PDT_SAMPLER_MM) {
            if ((rc = make_mm_params<T>(ctx, n_out, chunk_out, nullptr))) return rc;     // stepMax must stay positive and finite
            min_step = (double)(int)fsi / ((double)baud + mm_step_range(ctx)) * 0.999;
        }
        n_chunks = chunk_out > 0 ? (n_out + chunk_out - 1) / chunk_out : 0;
        sym_cap = (long long)((double)n_out / min_step) + n_chunks + 64 + (seg ? 2 * PDT_SEG_KEEP : 0);
        bit_cap = sym_cap;
        // worst legal hit density: the ARGOS word overlaps itself by 3 bits (one hit per 10 bits), the POES word followed by
        // its inverse by 3 (one per 16) -- e.g. a repeated sync-word test pattern; the reference decodes such streams
        hit_cap = next_pow2((uint32_t)(bit_cap / 10 + 4096));
        frame_cap = (uint32_t)(bit_cap / SP.span + 16);
        n_tiles = (sym_cap + PDT_TILE - 1) / PDT_TILE;
        n0 = std::min<long long>(chunk, N);

        if (seg) {
            // the windows of a stream keep what earlier segments wrote (FIR history, stale reads of the sampler's chunk seams)
            if ((rc = ctx->pll.ensure_keep((size_t)(N + 1) * sizeof(T), (size_t)first * sizeof(T)))) return rc;
            if (need_lock && (rc = ctx->lock.ensure_keep((size_t)(N + 1) * sizeof(T), (size_t)first * sizeof(T)))) return rc;
        }
        if ((rc = ctx->pll.ensure((size_t)(N + 1) * sizeof(T)))) return rc;
        if (need_lock && (rc = ctx->lock.ensure((size_t)(N + 1) * sizeof(T)))) return rc;
        // theta and the phases live in the FIR / AGC buffers before those are written, in the lane-tiled layout: whole tiles of
        // 64 blocks, plus the rows the walkers' look-ahead loads may touch past a tile
        lt_tiles = (N / Bp + 1 + 63) / 64;
        lt_elems = lt_tiles * 64 * Bp + 48 * 64 * (16 / (long long)sizeof(T)) + 64;
        if (seg) {
            // ... so theta and the phases get buffers of their own there (the AGC window must survive the PLL)
            if ((rc = ctx->agc.ensure_keep((size_t)(n_out + 1) * sizeof(T), (size_t)first_out * sizeof(T)))) return rc;
            if ((rc = ctx->lt_theta.ensure((size_t)(lt_elems + 1) * sizeof(T)))) return rc;
            if ((rc = ctx->lt_phi.ensure((size_t)(lt_elems + 1) * sizeof(T)))) return rc;
            if ((rc = ctx->seg_dev.ensure(sizeof(SegTail<T>) + 256))) return rc;
        }
        // (+ Ba + 1024: the full-line AGC walkers read whole super-batches of a last, partial block and a few beyond it)
        if ((rc = ctx->fir.ensure((size_t)((seg ? n_out : std::max(n_out, lt_elems)) + 1 + Ba + 1024) * sizeof(T)))) return rc;
        if ((rc = ctx->agc.ensure((size_t)((seg ? n_out : std::max(n_out, lt_elems)) + 1 + Ba + 1024) * sizeof(T)))) return rc;
        if (ctx->keep_agc_raw && (rc = ctx->agc_raw.ensure((size_t)(n_out + 1) * sizeof(T)))) return rc;
        if (ctx->keep_agc_raw) AP.raw_out = (T *)ctx->agc_raw.p;
        // quality figure (pdt_keep_quality; whole captures only): averagePhase is one more EMA of the lock detector's kind
        // (CarrierTrackingPLL.c:80,124,152), alpha 0.00005 -> blocks of one time constant, 16 of warm-up behind the affine guess
        // (in the segments of the overlapped ingest too: they begin and end on chunk boundaries, StreamCarry::quality)
        quality = (ctx->keep_quality || inject) && (!seg || (seg->quality && first % chunk == 0)) && N > 0;
        avg_alpha = (T)0.00005;
        // Blocks of one time constant for captures up to ~8 000 of them; longer captures get longer blocks (up to eight time
        // constants), the warm-up stays 16 time constants: with one-time-constant blocks an hour at 250 ksps re-read its input 17
        // times (61 GB, 18.7 ms -- and 59 ms beside the chain's kernels on the side stream); 45 000 blocks -> 8 192: 14 GB.
        tau_q = std::max<long long>(64, round4((long long)(1.0 / (double)avg_alpha)));
        Bq = std::max(tau_q, std::min(8 * tau_q, round4(N / 8192)));
        Wq = 16 * tau_q;
        nb_q = N / Bq + 2;
        d_q_zresp = nullptr;
        d_q_guess = nullptr;
        if (quality) {
            if ((rc = ctx->avgph.ensure((size_t)(N + 1) * sizeof(T)))) return rc;
            if ((rc = ctx->term_ap.ensure((size_t)(N + 1) * sizeof(T)))) return rc;
            if ((rc = ctx->seams_q.ensure((size_t)nb_q * (sizeof(EmaSeam<T>) + 2 * sizeof(double))))) return rc;
            if ((rc = ctx->chunkinfo.ensure((size_t)(n_chunks + 1) * sizeof(ChunkInfo)))) return rc;
            d_q_zresp = (double *)((EmaSeam<T> *)ctx->seams_q.p + nb_q);
            d_q_guess = d_q_zresp + nb_q;
            const size_t want = (size_t)(n_chunks + 1) * sizeof(ChunkInfo);
            if (want > ctx->qual_pin_cap) {
                if (ctx->qual_pin) (void)hipHostFree(ctx->qual_pin);
                ctx->qual_pin = nullptr;
                ctx->qual_pin_cap = 0;
                if (timed_host_malloc((void **)&ctx->qual_pin, want + want / 4) != hipSuccess) {
                    (void)hipGetLastError();
                    return PDT_ERR_NOMEM;
                }
                ctx->qual_pin_cap = want + want / 4;
            }
        }
        d_avgph = quality ? (T *)ctx->avgph.p : nullptr;
        if ((rc = ctx->sym.ensure((size_t)sym_cap * sizeof(T)))) return rc;
        if ((rc = ctx->symidx.ensure((size_t)sym_cap * sizeof(long long)))) return rc;
        if ((rc = ctx->bits.ensure((size_t)bit_cap))) return rc;
        if ((rc = ctx->bitsym.ensure((size_t)bit_cap * sizeof(unsigned)))) return rc;
        if ((rc = ctx->hits.ensure((size_t)hit_cap * sizeof(unsigned) + (size_t)n_tiles * sizeof(ManchTile)))) return rc;
        if ((rc = ctx->sync_scr.ensure((2 * ((size_t)hit_cap + 1) + hit_cap / 32 + 2) * sizeof(unsigned)))) return rc;
        if ((rc = ctx->frames.ensure((size_t)frame_cap * sizeof(FrameRec)))) return rc;
        if ((rc = ctx->stiles.ensure((size_t)((bit_cap + 4095) / 4096 + 1) * sizeof(SyncTile)))) return rc;
        if ((rc = ctx->mag.ensure((size_t)(n0 + 1) * sizeof(T)))) return rc;
        if ((rc = ctx->seams_pll.ensure((size_t)nb_pll * sizeof(PllSeam<T>)))) return rc;
        if ((rc = ctx->seams_agc.ensure((size_t)nb_agc * sizeof(AgcSeam<T>)))) return rc;
        if (need_lock && (rc = ctx->term.ensure((size_t)(N + 1) * sizeof(T)))) return rc;
        // lock-detector EMA (ARGOS): a pure contraction with factor 1 - lockSigAlpha per sample, so its own, much
        // shorter geometry: 45 time constants of warm-up agree in 53 bits (20 in 24), blocks a quarter of that
        // With the affine guess of the state at every block boundary (k_lock_ema_zero / _guess) 16 time constants do.
        ema_guess = !ctx->tune.ema_noguess;
        We = round4((long long)((sizeof(T) == 8 ? 45.0 : 20.0) / (double)PP.lock_alpha) + 64);
        Be = std::max<long long>(64, round4(We / 4));
        if (ema_guess) {
            Be = std::max<long long>(64, round4((long long)(1.0 / (double)PP.lock_alpha)));
            We = 16 * Be;                  // a difference of D ulps survives n steps with probability ~ D (1 - alpha)^n; D is a few tens
            if (argos && ctx->batch_hint >= 8) Be = We / 2;         // (a batch: longer blocks, every term read three times instead of 17)
        }
        nb_ema = N / Be + 2;
        if (need_lock && (rc = ctx->seams_ema.ensure((size_t)nb_ema * (sizeof(EmaSeam<T>) + 2 * sizeof(double))))) return rc;
        d_ema_zresp = need_lock ? (double *)((EmaSeam<T> *)ctx->seams_ema.p + nb_ema) : nullptr;
        d_ema_guess = need_lock ? d_ema_zresp + nb_ema : nullptr;
        if ((rc = ctx->scal.ensure(sizeof(DevScalars)))) return rc;
        if ((rc = ctx->lockinfo.ensure(sizeof(PllLockInfo<T>)))) return rc;

        d_pcm.p = ctx->pcm_dev;
        d_pcm.fmt = ctx->pcm_fmt;
        d_pll = (T *)ctx->pll.p;
        d_lock = need_lock ? (T *)ctx->lock.p : nullptr;
        d_fir = (T *)ctx->fir.p;
        d_agc = (T *)ctx->agc.p;
        d_sym = (T *)ctx->sym.p;
        d_symidx = (long long *)ctx->symidx.p;
        d_bits = (unsigned char *)ctx->bits.p;
        d_bitsym = (unsigned *)ctx->bitsym.p;
        d_tiles = (ManchTile *)((unsigned char *)ctx->hits.p + (size_t)hit_cap * sizeof(unsigned));
        d_frames = (FrameRec *)ctx->frames.p;
        d_sc = (DevScalars *)ctx->scal.p;
        d_info = (PllLockInfo<T> *)ctx->lockinfo.p;
        d_norm = (T *)&d_sc->norm;
        d_taps = (T *)ctx->taps.p;

        return PDT_OK;
    }

    // the plan begins: scalars and frame records cleared, StaticGain over the first chunk (main.c:384-389) or the carried gain
    int rec_begin()
    {
        int rc = PDT_OK;
        (void)rc;
        PL.clear();
        PL.side_stream = ctx->stream2;
        PL.simple(OP_EV0);
        PL.memset_async(d_sc, 0, sizeof(DevScalars));
        PL.memset_async(d_frames, 0, (size_t)frame_cap * sizeof(FrameRec));

        // ---- StaticGain over the first chunk (main.c:384-389)
        // per-segment staging in pinned memory (lives until the plan has run): [0] AGC gain, [64] lock record, [256] two
        // history symbols, [512] kept bits
        spin = ctx->seg_pin;
        if (seg && seg->have_norm) {
            const T g = (T)seg->gain;                    // the AGC goes on from its gain at the end of the last segment
            memcpy(spin, &g, sizeof g);
            PL.copy(OP_H2D, d_norm, spin, sizeof(T));
        } else {
            L.begin("static_gain");
            rec_static_gain<T>(PL, st, d_pcm, n0, (T *)ctx->mag.p, (T)1.0, ctx->cfg.norm_override, d_norm);
            L.end();
        }

        return PDT_OK;
    }

    // PLL, the block-parallel part on the side stream: theta, the (phase, freq) walkers, the tail pass
    int rec_pll_walkers()
    {
        int rc = PDT_OK;
        (void)rc;
        // ---- PLL: sequential acquisition, then theta / block-parallel phase recurrence / seam repair / mix.
        // theta and phase live in the (not yet used) FIR and AGC buffers.
        d_theta = seg ? (T *)ctx->lt_theta.p : d_fir;
        d_phi = seg ? (T *)ctx->lt_phi.p : d_agc;
        lt_groups = lt_tiles * (Bp / (16 * (16 / (long long)sizeof(T))));      // workgroups of the transposing kernels
        if (N > 0) {
            L.begin("pll_theta");
            PDT_LAUNCH(256, k_pll_theta<T>, dim3((unsigned)lt_groups), dim3(256), 0, st, d_pcm, N, Bp, d_theta);
            L.end();
        }
        // fork: the block-parallel phase recurrence (side stream) runs beside the sequential acquisition
        // workgroups of four wavefronts: the dispatcher spreads a workgroup's wavefronts over the four SIMDs of a CU, so the
        // walkers are balanced over the SIMDs by construction (single-wavefront groups piled up on some SIMDs once there were
        // more than ~1000 of them: 250 ksps hour-long captures, batches)
        grid_pll = (nb_pll + 255) / 256;
        // one more workgroup for the walkers whose warm-up begins at sample 0 (k_pll_phase), when they fit into a wavefront
        // ... and when it pays: in place, wavefront 0 runs every segment of the tracking stage for the longer of its two kinds of lane --
        // the early walkers' first segment is B - (wide + acquisition stage), everybody else's W mod B (a wavefront with few lanes
        // is not faster, rather the opposite: ARGOS, W = 4 B, +0.3 ms with the extra workgroup)
        short_pays = false;
        {
            const long long w0 = ((Wacq / 4 + 3) & ~3ll) + Wacq;
            const long long a = (Wp % Bp) ? Wp % Bp : Bp, s_first = Bp - w0 % Bp;
            short_pays = (s_first - a) * 50 > w0 + Wp + Bp;
        }
        short_group = (short_pays && (((Wacq / 4 + 3) & ~3ll) + Wacq + Wp + Bp - 1) / Bp <= 64 && nb_pll > 64 && !ctx->tune.pll_noshort) ? (int)grid_pll : -1;
        // outliers behind the wide-band stage take their wavefront's median frequency (k_pll_phase): POES only -- an ARGOS capture holds
        // many transmitters, each at its own offset
        pll_consensus = (!argos && !ctx->tune.pll_noconsensus) ? (T)(2.0 * M_PI * 800.0 / fs_d) : (T)0;
        phase_groups = grid_pll + (short_group >= 0 ? 1 : 0);
        // a single +-2pi correction per step is exact as long as one step cannot move the phase by 2pi
        worst = (double)PP.max_freq + M_PI * std::max({(double)PP.alpha_acq + (double)PP.beta_acq,
                                                                    (double)PP.alpha_trk + (double)PP.beta_trk,
                                                                    (double)PP.alpha_wide + (double)PP.beta_wide});
        slow_wrap = worst >= 2.0 * M_PI - 0.05;
        // the walkers' frequency checkpoints (pll_phase_range): with them a seam repair stops where it has merged with the stored
        // trajectory.  All ones = a NaN no loop state equals: a checkpoint nobody wrote never matches.
        d_ckpt = nullptr;
        if (N > 0 && !ctx->tune.pll_nockpt) {
            const size_t ck_bytes = (size_t)((nb_pll + 63) / 64 + 1) * (size_t)pll_ckpt_count(Bp) * 64 * sizeof(T);
            if ((rc = ctx->pll_ckpt.ensure(ck_bytes))) return rc;
            d_ckpt = (T *)ctx->pll_ckpt.p;
            PL.memset_async(d_ckpt, 0xff, ck_bytes);
        }
        d_hint = &d_sc->phase_hint;
        if (N > 0) {
            PL.simple(OP_FORK);
            L.begin("pll_phase", ctx->stream2);
            if (slow_wrap)
                PDT_LAUNCH(256, (k_pll_phase<T, true>), dim3((unsigned)phase_groups), dim3(256), 0, ctx->stream2, d_pcm, d_theta, N, PP, Bp,
                                   Wacq, Wp, lag, d_phi, (PllSeam<T> *)ctx->seams_pll.p, d_hint, short_group, d_ckpt, pll_consensus);
            else
                PDT_LAUNCH(256, (k_pll_phase<T, false>), dim3((unsigned)phase_groups), dim3(256), 0, ctx->stream2, d_pcm, d_theta, N, PP, Bp,
                                   Wacq, Wp, lag, d_phi, (PllSeam<T> *)ctx->seams_pll.p, d_hint, short_group, d_ckpt, pll_consensus);
            L.end();
            // the tail pass (k_pll_tail): the stretches of noise behind a signal -- the end of the capture after the satellite has set,
            // fades inside the pass -- are walked from the last block that merged in front of each, on this stream, beside the
            // acquisition, instead of by k_pll_fix behind it (POES: an ARGOS capture is bursts between which every seam is open by
            // design, its warm-ups span them).  Two launches: the list of stretches, then a workgroup per stretch.
            if (!argos && !inject && !ctx->tune.pll_notail && nb_pll > 64) {
                PllTailList *d_tails = &d_sc->tail_list;
                L.begin("pll_tail", ctx->stream2);
                PDT_LAUNCH(1024, k_pll_tail_scan<T>, dim3(1), dim3(1024), 0, ctx->stream2, N, Bp, (const PllSeam<T> *)ctx->seams_pll.p, d_tails, 8);
                if (slow_wrap)
                    PDT_LAUNCH(64, (k_pll_tail<T, true>), dim3(PDT_TAIL_MAX), dim3(64), 0, ctx->stream2, (const T *)d_theta, N, PP, Bp, d_phi,
                               (PllSeam<T> *)ctx->seams_pll.p, d_sc->counters, d_ckpt, (const PllTailList *)d_tails, 8);
                else
                    PDT_LAUNCH(64, (k_pll_tail<T, false>), dim3(PDT_TAIL_MAX), dim3(64), 0, ctx->stream2, (const T *)d_theta, N, PP, Bp, d_phi,
                               (PllSeam<T> *)ctx->seams_pll.p, d_sc->counters, d_ckpt, (const PllTailList *)d_tails, 8);
                L.end();
            }
            PL.simple(OP_JOIN_RECORD);
        }
        return PDT_OK;
    }

    // PLL, the serial part beside it and everything behind the join: acquisition (or the carried lock), head, seam repairs, mix,
    // lock-detector EMA, the averagePhase walkers, the twin's Squelch
    int rec_pll_serial()
    {
        int rc = PDT_OK;
        (void)rc;
        // the serial kernels (acquisition, head) ask for SIMDs of their own while the block-parallel kernel beside them
        // leaves some free (1 024 SIMDs; it runs one wavefront per 64 blocks)
        serial_excl = 4 * grid_pll <= 960 && !ctx->tune.no_excl;
        fix_regions = 1;
        fix_region_blocks = 0;
        quality_side = false;            // the averagePhase EMA of pdt_keep_quality runs on the side stream
        quality_term_fused = false;                  // ... its input term written by k_mix_fir, its walkers launched behind that kernel
        quality_after_fir = false;
        L.begin("pll_acquire");
        if (inject && ctx->inj.locked) {
            // pdt_stage_pll after the lock: sample 0 is a dummy the caller put in front, "locked at sample 0" with the state record
            // = the state after it; the kernels that start behind the lock do the rest
            PllLockInfo<T> li;
            memset(&li, 0, sizeof li);
            li.lock_sample = 0;
            li.st.phase = (T)ctx->inj.phase; li.st.freq = (T)ctx->inj.freq; li.st.avg_phase = (T)ctx->inj.avg;
            li.st.locksig = (T)ctx->inj.locksig; li.st.sweep = (T)ctx->inj.sweep;
            memcpy(spin + 64, &li, sizeof li);
            PL.copy(OP_H2D, d_info, spin + 64, sizeof li);
            PL.memset_async(d_pll, 0, sizeof(T));
            PL.memset_async(d_lock, 0, sizeof(T));
            PL.memset_async(d_avgph, 0, sizeof(T));
        } else if (seg && seg->locked) {
            // the lock happened in an earlier segment: the kernels that start "after the lock" start at `first` with the carried
            // true state (the head walks the first samples, the block-parallel results are validated against it as ever)
            PllLockInfo<T> li;
            memset(&li, 0, sizeof li);
            li.lock_sample = first - 1;
            li.st.phase = (T)seg->phase; li.st.freq = (T)seg->freq; li.st.avg_phase = (T)seg->avg;
            li.st.locksig = (T)seg->locksig; li.st.sweep = (T)seg->sweep;
            li.freq_at_lock = 0; li.avg_at_lock = (T)seg->avg_at_lock;
            memcpy(spin + 64, &li, sizeof li);
            PL.copy(OP_H2D, d_info, spin + 64, sizeof li);
        } else if (slow_wrap)
            PDT_LAUNCH(128, (k_pll_acquire_pipe<T, true>), dim3(1), dim3(128), 0, st, d_pcm, N, PP, d_pll, d_lock,
                               d_info, d_avgph);
        else if (serial_excl)
            PDT_LAUNCH(128, (k_pll_acquire_pipe<T, false, true>), dim3(1), dim3(128), 0, st, d_pcm, N, PP, d_pll, d_lock,
                               d_info, d_avgph);
        else
            PDT_LAUNCH(128, (k_pll_acquire_pipe<T, false>), dim3(1), dim3(128), 0, st, d_pcm, N, PP, d_pll, d_lock,
                               d_info, d_avgph);
        L.end();
        if (N > 0) {
            const long long grid = grid_pll;
            // the sequential head (true state from the lock onwards, ~W samples) also runs beside k_pll_phase
            // its length: until the true state has (nearly) forgotten the acquisition -- time constant of the critically
            // damped tracking loop = 2 / alpha samples; 30 of them for 24 bits (measured: 28 suffice on every test
            // capture, 40 never needed), 90 for 53 bits; a block that still disagrees afterwards is simply re-run
            const double tau_trk = 2.0 / (double)PP.alpha_trk;
            double head_taus = (sizeof(T) == 4) ? 30.0 : 90.0;
            if (ctx->tune.head_taus > 0) head_taus = ctx->tune.head_taus;
            long long Hd = std::min<long long>(Wp, (long long)(head_taus * tau_trk));
            // A stream segment that continues a lock taken long ago starts from a state that remembers the acquisition no more than
            // any other sample of the capture does: the head then only has to reach the next block boundary -- the warm-ups of the
            // blocks behind it merge with the truth as anywhere else, and the seams are validated as ever (round 5: the mandatory
            // 30 time constants kept a SIMD busy for 2.5 ms of every segment of the overlapped ingest).  What is left of the 30 since
            // the lock stays.
            if (seg && seg->locked && first > 0 && seg->in_place && !ctx->tune.head_taus) {
                const long long since = (long long)seg->origin + first - 1 - (long long)seg->lock_sample;
                Hd = std::max<long long>(0, std::min<long long>(Hd, Hd - since));
            }
            // ... and further -- up to half as long again -- for as long as the block-parallel kernel beside it is still running: those
            // blocks cost nothing, and the first block behind a 30-tau head fails its seam now and then (an hour at 250 ksps: one
            // repair of two block walks, 1.6 ms; the head stopped 0.9 ms before the kernel beside it)
            // Only where the kernel beside it is bound by HBM (its warm-ups re-read more than ~12 GB: hour-long captures) -- there it
            // runs ~25 % longer than acquisition + head; elsewhere the two finish together and an extra block is a block too many
            // (10 min at 50 ksps: +0.1 ms; 10 min at 250 ksps: +0.45 ms).
            const bool head_slack = (double)nb_pll * (double)(Wp + Bp) * sizeof(T) >= 12e9 && !ctx->tune.head_taus;
            const long long Hd_max = head_slack ? std::min<long long>(Wp, Hd + Hd / 2) : Hd;
            const long long head_blocks = Hd_max / Bp + 3;
            if ((rc = ctx->pll_head.ensure((size_t)(head_blocks * Bp + 64) * sizeof(T) + (size_t)head_blocks * sizeof(PllSeam<T>) +
                                           sizeof(PllHeadInfo<T>) + 64)))
                return rc;
            PllHeadInfo<T> *d_hinfo = (PllHeadInfo<T> *)ctx->pll_head.p;
            PllSeam<T> *d_hseams = (PllSeam<T> *)((unsigned char *)ctx->pll_head.p + 64);
            T *d_hphi = (T *)((unsigned char *)d_hseams + (((size_t)head_blocks * sizeof(PllSeam<T>) + 63) & ~(size_t)63));
            // seam repairs: regions of the capture are validated and repaired side by side before the final in-order pass
            // (k_pll_fix); every region workgroup has scratch for its 16 concurrent block re-runs
            const long long nb_fix = (N + Bp - 1) / Bp;
            fix_regions = (nb_fix >= 128) ? std::min<long long>(64, nb_fix / 16) : 1;
            fix_region_blocks = (nb_fix + fix_regions - 1) / fix_regions;
            if ((rc = ctx->pll_scratch.ensure((size_t)(fix_regions + 2) * (size_t)(PDT_FIX_THREADS / 64) *
                                              (size_t)(((Bp + 63) & ~63ll) + ((pll_ckpt_count(Bp) + 63) & ~63ll) + 64) * sizeof(T)))) return rc;
            L.begin("pll_head");
            if (slow_wrap)
                PDT_LAUNCH(64, (k_pll_head<T, true>), dim3(1), dim3(64), 0, st, d_theta, N, PP, d_info, Bp, Hd, d_hphi, d_hseams,
                                   d_hinfo, head_blocks, Hd_max, (const PllPhaseHint *)d_hint, (unsigned)phase_groups,
                                   ((Wacq / 4 + 3) & ~3ll) + Wacq + Wp + Bp);
            else if (serial_excl)
                PDT_LAUNCH(64, (k_pll_head<T, false, true>), dim3(1), dim3(64), 0, st, d_theta, N, PP, d_info, Bp, Hd, d_hphi, d_hseams,
                                   d_hinfo, head_blocks, Hd_max, (const PllPhaseHint *)d_hint, (unsigned)phase_groups,
                                   ((Wacq / 4 + 3) & ~3ll) + Wacq + Wp + Bp);
            else
                PDT_LAUNCH(64, (k_pll_head<T, false>), dim3(1), dim3(64), 0, st, d_theta, N, PP, d_info, Bp, Hd, d_hphi, d_hseams,
                                   d_hinfo, head_blocks, Hd_max, (const PllPhaseHint *)d_hint, (unsigned)phase_groups,
                                   ((Wacq / 4 + 3) & ~3ll) + Wacq + Wp + Bp);
            L.end();
            PL.simple(OP_JOIN_WAIT);                                           // join
            L.gap();                                                           // (the wait is not part of pll_fix)
            L.begin("pll_fix");
            {
                // graft the head, two optimistic region passes (region boundaries half a region apart), the final pass
                auto fix = [&](int mode, unsigned grid, long long rb, long long ro) {
                    if (slow_wrap)
                        PDT_LAUNCH(PDT_FIX_THREADS, (k_pll_fix<T, true>), dim3(grid), dim3(PDT_FIX_THREADS), 0, st, d_theta, N, PP, d_info, Bp, d_phi,
                                   (PllSeam<T> *)ctx->seams_pll.p, (const T *)d_hphi, (const PllSeam<T> *)d_hseams,
                                   (const PllHeadInfo<T> *)d_hinfo, (T *)ctx->pll_scratch.p, d_sc->counters, mode, rb, ro, d_ckpt);
                    else
                        PDT_LAUNCH(PDT_FIX_THREADS, (k_pll_fix<T, false>), dim3(grid), dim3(PDT_FIX_THREADS), 0, st, d_theta, N, PP, d_info, Bp, d_phi,
                                   (PllSeam<T> *)ctx->seams_pll.p, (const T *)d_hphi, (const PllSeam<T> *)d_hseams,
                                   (const PllHeadInfo<T> *)d_hinfo, (T *)ctx->pll_scratch.p, d_sc->counters, mode, rb, ro, d_ckpt);
                };
                fix(0, 32, 0, 0);
                if (fix_regions > 1) {
                    for (int pass = 0; pass < ctx->tune.fix_passes; pass++) {
                        if (pass & 1) fix(1, (unsigned)fix_regions + 1, fix_region_blocks, fix_region_blocks / 2);
                        else fix(1, (unsigned)fix_regions, fix_region_blocks, 0);
                    }
                }
                fix(2, 1, 0, 0);
            }
            L.end();
            (void)grid;
            if (!fuse_mix) {
            L.begin("pll_mix");
            if (need_lock)
                PDT_LAUNCH(256, (k_pll_mix<T, true>), dim3((unsigned)lt_groups), dim3(256), 0, st, d_pcm, d_phi, N, Bp, PP,
                                   d_info, d_pll, (T *)ctx->term.p);
            else
                PDT_LAUNCH(256, (k_pll_mix<T, false>), dim3((unsigned)lt_groups), dim3(256), 0, st, d_pcm, d_phi, N, Bp, PP,
                                   d_info, d_pll, (T *)nullptr);
            L.end();
            }
            if (need_lock) {
                L.begin("lock_ema");
                if (ema_guess) {
                    PDT_LAUNCH(64, k_lock_ema_zero<T>, dim3((unsigned)((nb_ema + 63) / 64)), dim3(64), 0, st, (const T *)ctx->term.p, N,
                                       PP.lock_alpha, d_info, Be, d_ema_zresp);
                    PDT_LAUNCH(1024, k_lock_ema_guess<T>, dim3(1), dim3(1024), 0, st, (const double *)d_ema_zresp, N, PP.lock_alpha, d_info, Be,
                                       pow(1.0 - (double)PP.lock_alpha, (double)Be), d_ema_guess);
                }
                PDT_LAUNCH(64, k_lock_ema<T>, dim3((unsigned)((nb_ema + 63) / 64)), dim3(64), 0, st, (const T *)ctx->term.p, N, PP.lock_alpha,
                                   d_info, Be, We, d_lock, (EmaSeam<T> *)ctx->seams_ema.p, (const double *)(ema_guess ? d_ema_guess : nullptr), 0ll);
                PDT_LAUNCH(64, k_lock_ema_fix<T>, dim3(1), dim3(64), 0, st, (const T *)ctx->term.p, N, PP.lock_alpha, d_info,
                                   Be, d_lock, (EmaSeam<T> *)ctx->seams_ema.p, &d_sc->counters[1]);
                L.end();
            }
            if (quality) {
                // averagePhase after the lock: its input term from the phases (still in place), then the EMA like the lock detector's.
                // Nothing later in the chain needs it (only k_chunk_info, at the very end): whole captures run it on the side stream,
                // beside the filter, the AGC and the sampler; the chain only waits for the kernel that reads the phases (the AGC
                // output will take their place).
                quality_side = !inject && !ctx->tune.quality_inline;
                // Round 4: where mix and filter are one kernel (k_mix_fir, eight wavefronts) that kernel writes the EMA's input term
                // on its way; the walkers below are then launched behind it (quality_walkers, further down)
                quality_term_fused = quality_side && fuse_mix && std::is_same<T, float>::value;
                }
            if (quality && !quality_term_fused) rec_quality_walkers(true);
            quality_after_fir = quality && quality_term_fused;
            if (live) {                                            // twin main.c:370, DSP_SQLCH_THRESH 0.05 (:55)
                L.begin("squelch");
                rec_squelch<T>(PL, st, d_pll, d_lock, N, (T)0.05);
                L.end();
            }
        }

        return PDT_OK;
    }

    // the averagePhase walkers (pdt_keep_quality): after the lock the EMA of CarrierTrackingPLL.c:80,124,152 is one more contraction of the
    // lock detector's kind -- its input term from the phases (term_here) or already written by k_mix_fir, then zero responses, affine
    // guess, block walkers, seam repair; on the side stream where nothing in the chain waits for it
    void rec_quality_walkers(bool term_here)
    {
        hipStream_t sq = quality_side ? ctx->stream2 : st;
        if (quality_side) PL.simple(OP_FORK);
        L.begin("quality", sq);
        T *d_tap = (T *)ctx->term_ap.p;
        if (term_here)
        PDT_LAUNCH(256, (k_pll_mix<T, false, true>), dim3((unsigned)lt_groups), dim3(256), 0, sq, d_pcm, d_phi, N, Bp, PP,
                           d_info, (T *)nullptr, d_tap);
        if (quality_side && term_here) PL.simple(OP_JOIN_RECORD);
        PDT_LAUNCH(64, k_lock_ema_zero_wave<T>, dim3((unsigned)nb_q), dim3(64), 0, sq, (const T *)d_tap, N,
                           avg_alpha, d_info, Bq, d_q_zresp);
        PDT_LAUNCH(1024, (k_lock_ema_guess<T, true>), dim3(1), dim3(1024), 0, sq, (const double *)d_q_zresp, N, avg_alpha, d_info, Bq,
                           pow(1.0 - (double)avg_alpha, (double)Bq), d_q_guess);
        PDT_LAUNCH(64, (k_lock_ema<T, true>), dim3((unsigned)((nb_q + 63) / 64)), dim3(64), 0, sq, (const T *)d_tap, N, avg_alpha,
                           d_info, Bq, Wq, d_avgph, (EmaSeam<T> *)ctx->seams_q.p, (const double *)d_q_guess, (long long)chunk);
        PDT_LAUNCH(64, k_lock_ema_fix<T>, dim3(1), dim3(64), 0, sq, (const T *)d_tap, N, avg_alpha, d_info,
                           Bq, d_avgph, (EmaSeam<T> *)ctx->seams_q.p, &d_sc->pad0_);
        L.end();
    }

    // the low-pass filter: k_fir_plain (ARGOS), k_mix_fir (mix and filter in one kernel at INTERP 1), the register-tiled or the generic
    // interpolating form (LowPassFilter.c:13-125)
    int rec_fir()
    {
        int rc = PDT_OK;
        (void)rc;
        // ---- FIR
        ctx->fir_form = 0;                                     // (what pdt_dev_fir_form reports: set below, where a kernel is taken)
        if (n_out > 0) {
            L.begin(fuse_mix ? "mix_fir" : "fir");
            bool done = false;                                 // the kernel that writes the AGC's tile maps was taken
            AgcMap *fir_tile_maps = nullptr;
            if (!argos && agc_tiles_per_block > 0) {
                // the AGC's affine tile maps are folded into the filter when the AGC blocks are whole FIR tiles
                const int K = ntaps / interp;
                const long long tiles_rt = (N + 64ll * K - 1) / (64ll * K);
                if ((rc = ctx->agc_maps.ensure((size_t)(tiles_rt + 1) * sizeof(AgcMap) + (size_t)(nb_agc + 2) * (sizeof(double) + sizeof(AgcMap))))) return rc;
                fir_tile_maps = (AgcMap *)ctx->agc_maps.p;
                fused_tiles = tiles_rt;
            }
            if constexpr (std::is_same<T, float>::value) if (fuse_mix) {
                // one map per run of 208 outputs instead of one per FIR tile of 1 664 (AGC blocks are whole tiles = 8 runs each)
                const long long runs_nat = (N + PDT_MF_RUN - 1) / PDT_MF_RUN;
                AgcMap *run_maps = nullptr;
                if (agc_tiles_per_block > 0) {
                    if ((rc = ctx->agc_maps.ensure((size_t)(runs_nat + 1) * sizeof(AgcMap) + (size_t)(nb_agc + 2) * (sizeof(double) + sizeof(AgcMap))))) return rc;
                    run_maps = (AgcMap *)ctx->agc_maps.p;
                    fused_tiles = runs_nat;
                    agc_maps_per_block = agc_tiles_per_block * (64 * 26 / PDT_MF_RUN);
                }
                // eight wavefronts per workgroup (two workgroups per CU = four wavefronts per SIMD)
                const unsigned mf_grid = (unsigned)(lt_tiles * (Bp / PDT_MF_RUN));
                // (a stream segment keeps the PLL output's tail: the next segment's filter starts from its last 25 samples)
                float *mf_pll = (ctx->keep_pll || seg) ? (float *)d_pll : (float *)nullptr;
                const long long mf_pll_from = (seg && !ctx->keep_pll) ? std::max<long long>(0, N - 256) : 0ll;
#define PDT_MF_ARGS d_pcm, (const float *)d_phi, (const float *)d_pll, N, Bp, (const PllLockInfo<float> *)d_info, (const float *)ctx->taps_rot.p, (float *)d_fir, mf_pll, run_maps, (float)AP.decay
                if (quality_after_fir) {
                    float *d_tap = (float *)ctx->term_ap.p;
                    if (d_pcm.fmt == 0) PDT_LAUNCH(512, (k_mix_fir<26, 0, 8, true>), dim3(mf_grid), dim3(512), 0, st, PDT_MF_ARGS, d_tap, mf_pll_from);
                    else PDT_LAUNCH(512, (k_mix_fir<26, 1, 8, true>), dim3(mf_grid), dim3(512), 0, st, PDT_MF_ARGS, d_tap, mf_pll_from);
                } else {
                    if (d_pcm.fmt == 0) PDT_LAUNCH(512, (k_mix_fir<26, 0, 8>), dim3(mf_grid), dim3(512), 0, st, PDT_MF_ARGS, (float *)nullptr, mf_pll_from);
                    else PDT_LAUNCH(512, (k_mix_fir<26, 1, 8>), dim3(mf_grid), dim3(512), 0, st, PDT_MF_ARGS, (float *)nullptr, mf_pll_from);
                }
#undef PDT_MF_ARGS
                done = true;
            }
            if (!done) done = rec_fir_unfused<T>(ctx, PL, st, (const T *)d_pll, N, d_fir, fir_tile_maps, AP.decay);
            if (!done) fused_tiles = 0;
            ctx->fir_form = fuse_mix ? 2 : done ? 3 : argos ? 1 : 4;
            L.end();
        }
        ctx->fir_fused_tiles = fused_tiles;

        return PDT_OK;
    }

    // NormalizingAGC (+ Squelch): affine block maps -> gain guesses -> block walkers -> seam repair (AGC.c:24-46,78-132)
    int rec_agc()
    {
        int rc = PDT_OK;
        (void)rc;
        // ---- AGC (+Squelch); in a stream segment over the new outputs only, from the carried gain (*d_norm)
        agc_last_block = -1;
        if (n_out - first_out > 0) {
            const long long na = n_out - first_out;
            const T *a_in = d_fir + first_out;
            T *a_out = d_agc + first_out;
            const T *a_lock = d_lock ? d_lock + first_out : nullptr;       // (indexed like the outputs: interp is 1 where it is read)
            AgcParams<T> APs = AP;
            if (APs.raw_out) APs.raw_out += first_out;
            const long long nb = (na + Ba - 1) / Ba;
            agc_last_block = nb - 1;
            const bool fused = fused_tiles > 0;                    // tile maps already written by the FIR kernel
            if (!fused && (rc = ctx->agc_maps.ensure((size_t)(nb + 1) * (sizeof(AgcMap) + sizeof(double))))) return rc;
            AgcMap *d_maps = (AgcMap *)ctx->agc_maps.p;
            double *d_guess = (double *)(d_maps + (fused ? fused_tiles : nb) + 1);
            // (a stream segment: the FIR kernel's maps are indexed from the window's first output, the AGC's blocks from the first
            // NEW one -- a whole number of maps further on, seg_fast)
            const long long map_len_fused = fuse_mix ? (long long)PDT_MF_RUN : 64ll * 26 * interp;
            const long long map_first = fused ? first_out / map_len_fused : 0;
            const AgcMap *d_maps_in = d_maps + map_first;
            const long long n_maps_in = fused ? fused_tiles - map_first : nb;
            if (quality_side && !quality_term_fused) PL.simple(OP_JOIN_WAIT);          // the phases (in the AGC output's buffer) have been read
            L.begin("agc_block");
            if (agc_maps_per_block == 0) agc_maps_per_block = agc_tiles_per_block;        // (the FIR kernel's maps: one per tile)
            // the gain guesses from the FIR kernel's maps (not fused: rec_agc_lanes makes its own maps and guesses)
            if (fused && agc_maps_per_block > 1) {
                AgcMap *d_bmaps = (AgcMap *)(d_guess + nb + 1);
                PDT_LAUNCH(256, k_agc_blockmaps, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, d_maps_in, nb,
                                   (int)agc_maps_per_block, n_maps_in, d_bmaps);
                PDT_LAUNCH(1024, k_agc_guess<T>, dim3(1), dim3(1024), 0, st, (const AgcMap *)d_bmaps, nb, (const T *)d_norm, d_guess, 1, nb);
            } else if (fused)
                PDT_LAUNCH(1024, k_agc_guess<T>, dim3(1), dim3(1024), 0, st, d_maps_in, nb, (const T *)d_norm, d_guess, (int)agc_maps_per_block, n_maps_in);
            // (Round 3: walkers that store only the gain in front of every 16-sample batch + a streaming kernel that applies them were
            // slower, 4.2 against 3.3 ms at an hour of 250 ksps: the walkers are not held up by their output stores.)
            // Round 4: the walkers move whole lines (k_agc_block_tr) wherever the FIR kernel delivered its tile maps -- float chain,
            // no Squelch, no raw copy; the double build, stream segments and explicit block sizes keep the per-lane form.
            bool agc_tr = false;
            float *agc_ckpt = nullptr;
            if constexpr (std::is_same<T, float>::value) {
                agc_tr = fused && !ctx->tune.agc_lanes && !APs.squelch && !APs.raw_out && first_out % 32 == 0 && Ba % 32 == 0 &&
                         agc_maps_per_block > 0 && Ba % agc_maps_per_block == 0;
                if (agc_tr) {
                    const long long tile_len = 64ll * 26 * interp;                         // a FIR tile (= 8 runs of k_mix_fir)
                    const long long map_len = Ba / agc_maps_per_block;                     // samples per map
                    agc_tr = tile_len % 32 == 0 && tile_len % map_len == 0 && Ba % tile_len == 0;
                    if (agc_tr) {
                        // (no slack of a whole block behind the time constants any more.  An hour at 250 ksps: K = 10 / 11 / 12 / 13 / 14 / 16
                        // -> 4 / 3 / 0 / 0 / 0 / 0 open seams, walkers 1.76 / 1.80 / 1.84 / 1.86 / 1.91 / 2.06 ms; a minute of noise in front:
                        // 3 / 1 / 2 / 1 / 1 / 0 and 12.1 ... 19.1 ms.  A seam that stays open is cheap since the repairs stop at the first
                        // checkpoint they reproduce.)
                        const double agc_K = ctx->tune.agc_k > 0 ? ctx->tune.agc_k : 12.0;
                        const size_t ck_bytes = (size_t)(nb + 64) * (size_t)(Ba / PDT_AGC_CKPT + 1) * sizeof(float);
                        if ((rc = ctx->agc_ckpt.ensure(ck_bytes))) return rc;
                        agc_ckpt = (float *)ctx->agc_ckpt.p;
                        PDT_LAUNCH(64, (k_agc_block_tr<PDT_AGC_TR_R>), dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, st, (const float *)a_in, na, APs,
                                   (const float *)d_norm, Ba, Wa, (const double *)d_guess, d_maps_in, (int)agc_maps_per_block,
                                   (int)(tile_len / map_len), n_maps_in, tile_len, (float *)a_out, (AgcSeam<float> *)ctx->seams_agc.p, agc_K, agc_ckpt);
                    }
                }
            }
            T *agc_ckpt_any = (T *)agc_ckpt;
            if (!agc_tr && (rc = rec_agc_lanes<T>(ctx, PL, st, a_in, na, APs, d_norm, Ba, Wa, !fused, d_maps, d_guess, a_lock, a_out, &agc_ckpt_any))) return rc;
            L.end();
            L.begin("agc_fix");
            rec_agc_fix<T>(ctx, PL, st, a_in, na, APs, Ba, a_lock, a_out, d_sc, agc_ckpt_any);
            L.end();
        }

        return PDT_OK;
    }

    // which sampler: the boundary-state tables when the chunk geometry allows them (float build, boundary states in one binade) --
    // their key domain and the chunks per table row -- else M&M or the sequential Gardner walker
    int sampler_domain()
    {
        int rc = PDT_OK;
        (void)rc;
        // ---- Gardner: exact parallel evaluation through boundary-state tables when the chunk geometry
        // allows it (float build, chunk fits the LDS window, boundary states in one binade), otherwise the
        // single-wavefront sequential chain.
        use_mm = ctx->cfg.sampler == PDT_SAMPLER_MM;
        use_table = false;
        GD.q_min = 0; GD.u = 0; GD.n_q = 0; GD.n_cand = 0; GD.pad_q = 0; GD.idx_bits = 20; GD.span = 1;
        span_rekey = 0;
        if constexpr (std::is_same<T, float>::value) {
            const int table_len = 1 << 22;     // the table kernel walks the chunk in LDS windows: no size limit of its own
            const float nT = (float)chunk_out, stepf = (float)GP.step;
            const long long seg_c_first = (seg && chunk > 0) ? first / chunk : 0;
            if (!argos && !use_mm && !ctx->tune.gardner_sequential && n_chunks - seg_c_first >= 4 && chunk_out >= 256 &&
                !(seg && ctx->tune.seg_sequential) &&
                chunk_out + 2 * (long long)stepf + 24 <= table_len && 8 * (long long)stepf + 256 < PDT_GTAB_WIN && chunk_out < (1 << 22)) {
                int e;
                (void)frexpf(nT - stepf - 1.0f, &e);                              // value in [2^(e-1), 2^e)
                const float u = ldexpf(1.0f, e - 24);
                const float q_min = u * floorf((nT - stepf - 1.0f) / u);
                const int n_q = (int)ceilf((stepf + 1.8f) / u);
                const float q_max = q_min + (float)n_q * u;
                const double max_count = (double)chunk_out / ((double)stepf - 0.11) + 2.0;
                int idx_bits = 1;
                while ((1ll << idx_bits) < 2 * (long long)n_q) idx_bits++;
                if (q_min >= ldexpf(1.0f, e - 1) && q_max < ldexpf(1.0f, e) && idx_bits <= 20 &&
                    max_count < (double)((1u << (32 - idx_bits)) - 2u) && max_count < 65000.0) {
                    use_table = true;
                    GD.q_min = q_min;
                    GD.u = u;
                    GD.n_q = n_q;
                    GD.idx_bits = idx_bits;
                    const double pad = ctx->cfg.gardner_band_pad > 0 ? ctx->cfg.gardner_band_pad : (ctx->tune.band_pad > 0 ? ctx->tune.band_pad : 1.0 / 8.0);
                    GD.pad_q = std::max(2, (int)(pad / (double)u));
                    // Chunks per table row.  Many short chunks (an hour at 250 ksps: 90 000 of 666 symbols): the candidates of a chunk
                    // merge onto a handful of trajectories within it, so boundary states are tabulated in front of every span-th chunk
                    // only and the few distinct exits of a row's first chunk are walked on through the others (k_gardner_span):
                    // scouts, candidate walks and chain hops per span chunks instead of per chunk.  A row's symbol count must fit
                    // the table cell.  Stream segments keep one chunk per row (they are short, and enter with a carried state).
                    // (Round 5: a stream segment too, when its first new chunk is where a row begins -- the rows are counted from the
                    // window's chunk 0, the few in front of the first new chunk are history nobody asks for.)
                    // (Round 6: how many.  The candidate walks in front of a row's first chunk are chip-wide work, ~0.13 ns per symbol of
                    // the capture / span; the walk of a row's exits through its other chunks is ONE lane's latency, ~58 ns x (span - 1) x
                    // the symbols of a chunk: 16 chunks suit an hour at 250 ksps (666 symbols a chunk) and cost an hour at 18.75 ksps
                    // (8 876 a chunk: 7.7 of its 16 ms) or at 50 ksps (3 328: 3.4 of 13 ms) most of their sampler's time.  The minimum
                    // of the sum: span = sqrt(138 000 / symbols per chunk) -- 14, 6 and 4.)
                    // (Round 20: chunks of few symbols -- 666 at an hour of 250 ksps -- take the staged walk, whose stage 2 carries four
                    // rows per wavefront, so rows are walked in one round of wavefronts however many there are; measured there with the
                    // wanted span at 14, 18, 22 / 26 and 32 -- rows of 13, 17, 23 and 31 chunks after the search below -- tables + chain
                    // + emission 4.05, 3.69, 3.57 and 3.86 ms: sqrt(322 000 / symbols per chunk), at most 24.  Chunks of more symbols
                    // keep the rule above and its single stage.)
                    const double chunk_syms = (double)chunk_out / (double)stepf;
                    const int rekey_rule = (int)std::min(3.0, std::round(1332.0 / chunk_syms));       // chunks in front of the re-key point
                    const int rekey_want = ctx->tune.gspan_rekey >= 0 ? ctx->tune.gspan_rekey : rekey_rule;
                    int span_fit = rekey_want > 0 ? (int)std::min(24.0, std::max(2.0, std::round(std::sqrt(322000.0 / chunk_syms))))
                                                  : (int)std::min(16.0, std::max(2.0, std::round(std::sqrt(138000.0 / chunk_syms))));
                    if (ctx->tune.gspan_fit > 0) span_fit = ctx->tune.gspan_fit;
                    int span = ctx->tune.gspan > 0 ? ctx->tune.gspan : ((n_chunks - seg_c_first >= 4096 && (!seg || seg_fast)) ? span_fit : 1);
                    if (2 * n_q > 32 * PDT_GSPAN_BITMAP_WORDS || 8 * (long long)stepf + 256 >= PDT_GSUB_WIN) span = 1;
                    while (span > 1 && ((double)span * max_count >= (double)((1u << (32 - idx_bits)) - 2u) || (n_chunks - 1) / span - seg_c_first / span < 4))
                        span /= 2;
                    auto row_aligned = [&](int sp) { return !seg || seg_c_first % sp == 0; };
                    if (span >= 3 && !ctx->tune.gspan) {
                        // the group behind the last row is walked by one wavefront, chunk after chunk (0.8 ms for 16 chunks): take the span
                        // near the wanted one that leaves the fewest chunks there
                        int best = span;
                        long long best_left = row_aligned(span) ? n_chunks - ((n_chunks - 1) / span) * span : (1ll << 62);
                        for (int sp = span - std::max(1, span / 4); sp <= span + std::max(1, span / 4); sp++) {
                            const long long left = n_chunks - ((n_chunks - 1) / sp) * sp;
                            if (left < best_left && row_aligned(sp) && (double)sp * max_count < (double)((1u << (32 - idx_bits)) - 2u)) { best = sp; best_left = left; }
                        }
                        span = best;
                    }
                    if (!row_aligned(span)) span = 1;
                    GD.span = span;
                    // The staged span walk (k_gardner_span_rekey).  The exits of a row's first chunk go on merging behind it, by symbols
                    // walked: 28 -> 17 -> 12 states after 666 and 1 332 more symbols, ~8 after 3 300 (DESIGN 4.7).  The re-key point lies
                    // where about 1 300 symbols are through -- two chunks at an hour of 250 ksps; with chunks of 3 328 or 8 876 symbols a
                    // row starts with ~7 keys and is short: one stage, as before.  Behind the re-key point a row takes 16 lanes (a second
                    // item where it has more states) and 1 024 floats of LDS (measured: 8 lanes and 512 floats, 16 and 512 or 2 048,
                    // 32 and 2 048 all lose 0.1 - 0.3 ms to it; 8 lanes and 1 024 floats are 32 KiB and 256 registers a wavefront).
                    span_rekey = 0;
                    span_sub = (ctx->tune.gspan_sub == 8 || ctx->tune.gspan_sub == 32) ? ctx->tune.gspan_sub : 16;
                    span_win2 = (ctx->tune.gspan_win2 == 512 || ctx->tune.gspan_win2 == 1024 || ctx->tune.gspan_win2 == 2048)
                                    ? ctx->tune.gspan_win2 : 1024;
                    if (span_sub == 32) span_win2 = 2048;                  // (two rows: the window stage 1 has)
                    if (span_sub == 8 && span_win2 > 1024) span_win2 = 1024;      // (eight rows: 32 KiB)
                    if (span >= 3) {
                        int a = rekey_want;
                        if (ctx->tune.gspan_rekey < 0 && span - 1 - a < 4) a = 0;      // too little left behind it for three more launches
                        if (a >= span - 1) a = 0;                          // (nothing left for stage 2: stage 1 walks the rows through)
                        if (8 * (long long)stepf + 256 >= span_win2) a = 0;
                        span_rekey = a;
                    }
                }
            }
        }
        return PDT_OK;
    }

    // a stream segment: where the sequential samplers go on, the history symbols and kept bits in front of the new ones
    int sampler_carry()
    {
        int rc = PDT_OK;
        (void)rc;
        ctx->gardner_mode = use_table ? 1 : 0;
        ctx->gspan_rekey = (use_table && GD.span > 1) ? span_rekey : 0;
        ctx->gspan_nrows = (use_table && GD.span > 1 && chunk_out > 0) ? (n_out + chunk_out - 1) / chunk_out > 0 ? ((n_out + chunk_out - 1) / chunk_out - 1) / GD.span : 0 : 0;
        // stream segment: the sequential samplers go on from the carried state at chunk first / chunk; the symbol buffer starts
        // with the two symbols the Manchester stage looks back on, placed so that local and global symbol parities agree
        carry_in.a = 0; carry_in.b = 0; carry_in.c = 0; carry_in.c_first = 0; carry_in.count0 = 0;
        d_tail = seg ? (SegTail<T> *)ctx->seg_dev.p : nullptr;
        d_carry_out = seg ? &d_tail->sampler : nullptr;
        sym_pad = 0;
        clock0 = 0;
        bit0 = 0;
        sync_min_pos = 0;
        if (seg) {
            sym_pad = 2 + (long long)(seg->nsym_total & 1u);
            carry_in.c_first = chunk > 0 ? first / chunk : 0;
            carry_in.count0 = sym_pad;
            if (seg->have_sampler) { carry_in.a = (T)seg->sa; carry_in.b = (T)seg->sb; carry_in.c = (T)seg->sc; }
            T hist[4] = { 0, 0, 0, 0 };
            hist[sym_pad - 2] = (T)seg->sym_m2;
            hist[sym_pad - 1] = (T)seg->sym_m1;
            memcpy(spin + 256, hist, sizeof hist);
            PL.copy(OP_H2D, d_sym, spin + 256, (size_t)sym_pad * sizeof(T));
            if (quality) PL.memset_async(d_symidx, 0, (size_t)sym_pad * sizeof(long long));   // (k_chunk_info searches the picks' indices)
            clock0 = seg->clockmod;
            bit0 = seg->kept_bits.size();
            if (bit0) {
                memcpy(spin + 512, seg->kept_bits.data(), (size_t)bit0);
                PL.copy(OP_H2D, d_bits, spin + 512, (size_t)bit0);
                PL.memset_async(d_bitsym, 0, (size_t)bit0 * sizeof(unsigned));
            }
            sync_min_pos = std::max<long long>(0, seg->next_free - (long long)seg->bit_base);
            // The search treats the bits in front of local bit 0 as the zeros the reference's ring starts with -- true at the start
            // of the stream only.  Later the kept bits are the last len - 1 (or more) of the previous segment: a sync word that ends
            // inside them was looked at there with its real bits, and one that ends further on lies entirely inside this segment.
            if (seg->bit_base > 0) sync_min_pos = std::max<long long>(sync_min_pos, (long long)SP.len - 1);
        }
        return PDT_OK;
    }

    // GardenerClockRecovery through the boundary-state tables (DESIGN 4.1, 4.7): scouts, candidate walks, rows of several chunks,
    // the chain, entry states and emission
    int rec_sampler_table()
    {
        int rc = PDT_OK;
        (void)rc;
        if constexpr (std::is_same<T, float>::value) {
            // consistent (q, last pick) combinations: the last pick is rint(q + err), |err| <= 0.1
            std::vector<unsigned> cand;
            std::vector<int> mfirst((size_t)GD.n_q + 1);
            cand.reserve((size_t)GD.n_q * 2);
            for (int m = 0; m < GD.n_q; m++) {
                mfirst[(size_t)m] = (int)cand.size();
                const float q = GD.q_min + (float)m * GD.u;
                const float fr = q - floorf(q);
                if (fr <= 0.61f) cand.push_back((unsigned)(2 * m));
                if (fr >= 0.39f) cand.push_back((unsigned)(2 * m + 1));
            }
            mfirst[(size_t)GD.n_q] = (int)cand.size();
            GD.n_cand = (int)cand.size();
            const long long key = chunk_out * 1000003ll + (long long)llround((double)GP.step * 4096.0);
            if ((rc = ctx->gcand.ensure(cand.size() * sizeof(unsigned)))) return rc;
            if ((rc = ctx->gmfirst.ensure(mfirst.size() * sizeof(int)))) return rc;
            if (ctx->gcand_key != key) {
                HIP_TRY(hipMemcpyAsync(ctx->gcand.p, cand.data(), cand.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(ctx->gmfirst.p, mfirst.data(), mfirst.size() * sizeof(int), hipMemcpyHostToDevice, st));
                HIP_TRY(hipStreamSynchronize(st));              // the host vectors die at the end of this scope
                ctx->gcand_key = key;
            }
            const long long n_tab = (n_chunks - 1) / GD.span;        // table rows: groups of span full chunks that have a successor
            const long long n_groups = n_tab + 1;                    // ... and the group behind the last row (<= span chunks, the last may be short)
            SamplerCarry<float> tab_carry;                   // where the chain starts: chunk, state, symbols already in the buffer
            tab_carry.a = (float)carry_in.a; tab_carry.b = (float)carry_in.b; tab_carry.c = (float)carry_in.c;
            tab_carry.c_first = carry_in.c_first; tab_carry.count0 = carry_in.count0;
            SamplerCarry<float> chain_carry = tab_carry;     // the chain counts in table rows (groups of GD.span chunks)
            chain_carry.c_first = tab_carry.c_first / GD.span;
            const long long g_first = chain_carry.c_first;
            if ((rc = ctx->gtable.ensure((size_t)n_tab * (size_t)(2 * GD.n_q) * sizeof(unsigned)))) return rc;
            if ((rc = ctx->gentries.ensure((size_t)n_chunks * sizeof(GardnerEntry<float>)))) return rc;
            if ((rc = ctx->gbands.ensure((size_t)n_tab * sizeof(GardnerBand)))) return rc;
            L.begin("gardner_table");
            if ((rc = ctx->gclist.ensure((size_t)n_tab * PDT_GTAB_LIST * sizeof(unsigned)))) return rc;
            // (the table is never initialised as a whole -- 12 GB for an hour at 250 ksps: every look-up checks the chunk's band)
            // the scouts need symbols, not samples, to settle on the chunk's timing: the same number of them at every rate
            const int scout_syms = ctx->tune.scout_syms > 0 ? ctx->tune.scout_syms : 455;
            const int scout_tail = (int)std::min<long long>(PDT_GTAB_TAIL, std::max<long long>(256, (long long)((double)scout_syms * (double)GP.step) + 16));
            PDT_LAUNCH(64, k_gardner_scout, dim3((unsigned)n_tab), dim3(64), 0, st, (const float *)d_agc, GP, GD, n_tab,
                               (const int *)ctx->gmfirst.p, (const unsigned *)ctx->gcand.p, (unsigned *)ctx->gtable.p,
                               (GardnerBand *)ctx->gbands.p, (unsigned *)ctx->gclist.p, d_sc->gstats, scout_tail);
            {
                // locked chunks carry 100-300 candidates that merge quickly: see k_gardner_table_merge
                {
                    const unsigned parts = (unsigned)((GD.n_cand + PDT_GTM_SLOTS - 1) / PDT_GTM_SLOTS);
                    PDT_LAUNCH(PDT_GTM_THREADS, (k_gardner_table_merge<PDT_GTAB_WIN>), dim3((unsigned)n_tab, parts), dim3(PDT_GTM_THREADS), 0, st,
                                       (const float *)d_agc, GP, GD, n_tab, (const unsigned *)ctx->gcand.p,
                                       (const GardnerBand *)ctx->gbands.p, (const unsigned *)ctx->gclist.p,
                                       (unsigned *)ctx->gtable.p, d_sc->gstats);
                }
                if (GD.span > 1) {
                    // the distinct exits of every row's first chunk, walked on through the row's other chunks (see k_gardner_span_keys)
                    const unsigned cap_keys = ctx->tune.gspan_cap ? (unsigned)ctx->tune.gspan_cap
                                                                  : (unsigned)std::min<long long>(std::max<long long>(n_tab * 128, 1ll << 20), 1ll << 28);
                    const size_t cap_items = (size_t)cap_keys / PDT_GSUB_KEYS + (size_t)n_tab + 1;
                    if ((rc = ctx->gspan_keys.ensure((size_t)cap_keys * sizeof(unsigned)))) return rc;
                    if ((rc = ctx->gspan_tails.ensure((size_t)cap_keys * sizeof(unsigned)))) return rc;
                    if ((rc = ctx->gspan_recs.ensure((size_t)cap_keys * (size_t)(GD.span - 1) * sizeof(GardnerSpanRec)))) return rc;
                    if ((rc = ctx->gspan_rows.ensure((size_t)n_tab * sizeof(GardnerSpanRow)))) return rc;
                    if ((rc = ctx->gspan_items.ensure(cap_items * sizeof(GardnerSpanItem)))) return rc;
                    if ((rc = ctx->gspan_ctl.ensure(sizeof(GardnerSpanCtl)))) return rc;
                    PL.memset_async(ctx->gspan_ctl.p, 0, sizeof(GardnerSpanCtl));
                    PDT_LAUNCH(256, k_gardner_span_keys, dim3((unsigned)n_tab), dim3(256), 0, st, GD, n_tab, (const unsigned *)ctx->gcand.p,
                                       (GardnerBand *)ctx->gbands.p, (const unsigned *)ctx->gclist.p, (const unsigned *)ctx->gtable.p,
                                       (unsigned *)ctx->gspan_keys.p, cap_keys, (GardnerSpanRow *)ctx->gspan_rows.p,
                                       (GardnerSpanItem *)ctx->gspan_items.p, (GardnerSpanCtl *)ctx->gspan_ctl.p);
                    if (span_rekey > 0) {
                        // stage 2's lists: a representative per distinct state (at most the keys), their items, a note per row
                        if ((rc = ctx->gspan_rep.ensure((size_t)cap_keys * sizeof(unsigned)))) return rc;
                        if ((rc = ctx->gspan_list2.ensure((size_t)cap_keys * sizeof(unsigned)))) return rc;
                        if ((rc = ctx->gspan_items2.ensure(((size_t)cap_keys / (size_t)span_sub + (size_t)n_tab + 1) * sizeof(GardnerSpanItem)))) return rc;
                        if ((rc = ctx->gspan_info.ensure((size_t)n_tab * sizeof(GardnerSpanRowInfo)))) return rc;
                    }
                    const unsigned walkers = (unsigned)std::min<long long>(n_tab / PDT_GSUB + 64, 256ll * 16);     // persistent wavefronts (8 KiB of LDS each)
                    PDT_LAUNCH(64, (k_gardner_span_walk<PDT_GSUB_WIN, PDT_GSUB, false>), dim3(walkers), dim3(64), 0, st, (const float *)d_agc, GP, GD,
                                       (const unsigned *)ctx->gspan_keys.p, (const GardnerSpanItem *)ctx->gspan_items.p,
                                       (GardnerSpanCtl *)ctx->gspan_ctl.p, (unsigned *)ctx->gspan_tails.p, (GardnerSpanRec *)ctx->gspan_recs.p,
                                       (const GardnerSpanRow *)ctx->gspan_rows.p, (const unsigned *)nullptr, span_rekey);
                    if (span_rekey > 0) {
                        PDT_LAUNCH(64 * PDT_GSPAN_REKEY_ROWS, k_gardner_span_rekey, dim3((unsigned)((n_tab + PDT_GSPAN_REKEY_ROWS - 1) / PDT_GSPAN_REKEY_ROWS)), dim3(64 * PDT_GSPAN_REKEY_ROWS), 0, st, GD, n_tab, (const GardnerSpanRow *)ctx->gspan_rows.p,
                                           (const GardnerSpanRec *)ctx->gspan_recs.p, span_rekey, (unsigned)span_sub, (unsigned *)ctx->gspan_rep.p,
                                           (unsigned *)ctx->gspan_list2.p, (GardnerSpanItem *)ctx->gspan_items2.p, (GardnerSpanCtl *)ctx->gspan_ctl.p,
                                           (GardnerSpanRowInfo *)ctx->gspan_info.p);
                        // persistent wavefronts again: as many as two items a row would fill, within what the LDS lets be resident
                        const int nsub = 64 / span_sub;
                        const long long resident = 256ll * std::max(1, (140 * 1024) / (nsub * span_win2 * 4));
                        const unsigned walkers2 = (unsigned)std::min<long long>(2 * n_tab / nsub + 64, resident);
#define PDT_SPAN_STAGE2(NSUB, WIN2)                                                                                                          \
    PDT_LAUNCH(64, (k_gardner_span_walk<WIN2, NSUB, true>), dim3(walkers2), dim3(64), 0, st, (const float *)d_agc, GP, GD,                   \
               (const unsigned *)ctx->gspan_keys.p, (const GardnerSpanItem *)ctx->gspan_items2.p, (GardnerSpanCtl *)ctx->gspan_ctl.p,        \
               (unsigned *)ctx->gspan_tails.p, (GardnerSpanRec *)ctx->gspan_recs.p, (const GardnerSpanRow *)ctx->gspan_rows.p,               \
               (const unsigned *)ctx->gspan_list2.p, span_rekey)
                        if (span_sub == 8 && span_win2 == 512) PDT_SPAN_STAGE2(8, 512);
                        else if (span_sub == 8) PDT_SPAN_STAGE2(8, 1024);
                        else if (span_sub == 16 && span_win2 == 512) PDT_SPAN_STAGE2(4, 512);
                        else if (span_sub == 16 && span_win2 == 1024) PDT_SPAN_STAGE2(4, 1024);
                        else if (span_sub == 16) PDT_SPAN_STAGE2(4, 2048);
                        else PDT_SPAN_STAGE2(2, 2048);
#undef PDT_SPAN_STAGE2
                        PDT_LAUNCH(64, k_gardner_span_spread, dim3((unsigned)n_tab), dim3(64), 0, st, GD, n_tab, (const GardnerSpanRow *)ctx->gspan_rows.p,
                                           (const GardnerSpanRowInfo *)ctx->gspan_info.p, (const unsigned *)ctx->gspan_rep.p, span_rekey,
                                           (unsigned *)ctx->gspan_tails.p, (GardnerSpanRec *)ctx->gspan_recs.p);
                    }
                    PDT_LAUNCH(128, k_gardner_span_join, dim3((unsigned)n_tab), dim3(128), 0, st, GD, n_tab, (const unsigned *)ctx->gcand.p,
                                       (const GardnerBand *)ctx->gbands.p, (const unsigned *)ctx->gclist.p, (unsigned *)ctx->gtable.p,
                                       (const unsigned *)ctx->gspan_keys.p, (const unsigned *)ctx->gspan_tails.p,
                                       (const GardnerSpanRow *)ctx->gspan_rows.p, d_sc->gstats);
                }
            }
            L.end();
            // chunks per chain segment: the chain hops one segment per ~1 us of dependent L2 look-ups, the composite maps and
            // the re-trace of a segment take G such look-ups each but run in parallel over the segments
            // (at most 64: k_gardner_segfill re-traces a segment with one lane per chunk)
            int G = (n_groups < 8000) ? 32 : 64;
            if (ctx->tune.gseg) G = ctx->tune.gseg;
            const long long n_seg = (n_groups + G - 1) / G;
            if ((rc = ctx->gsegmap.ensure((size_t)n_seg * (size_t)(2 * GD.n_q) * sizeof(GardnerSegCell)))) return rc;
            if ((rc = ctx->gsegstart.ensure((size_t)n_seg * sizeof(GardnerSegStart)))) return rc;
            L.begin("gardner_chain");
            PL.memset_async(ctx->gsegstart.p, 0, (size_t)n_seg * sizeof(GardnerSegStart));
            PDT_LAUNCH(1024, k_gardner_segmap, dim3((unsigned)n_seg), dim3(1024), 0, st, (const unsigned *)ctx->gtable.p, GD, n_groups,
                               G, (GardnerSegCell *)ctx->gsegmap.p, (const GardnerBand *)ctx->gbands.p);
            // Long captures: the chain runs range by range; as soon as a range is through, its entry states and symbols are produced
            // on the side stream (segfill, emission -- chip-wide kernels) while the single workgroup of the chain hops on
            // (an hour at 250 ksps: chain 1.6 ms + emission 1.8 ms one after the other -> the emission behind the chain).
            const int n_ranges = (!seg && n_groups >= 8192 && GD.span == 1 && !ctx->tune.chain_one_range) ? 4 : 1;
            if ((rc = ctx->gchain.ensure(sizeof(GardnerChainState)))) return rc;
            const bool side = n_ranges > 1;
            hipStream_t st_emit = side ? ctx->stream2 : st;
            L.end();
            long long c_lo = 0;
            for (int r = 0; r < n_ranges; r++) {
                const long long c_hi = (r == n_ranges - 1) ? n_groups : (n_groups * (r + 1) / n_ranges) / G * G;      // (groups)
                L.begin("gardner_chain");
                PDT_LAUNCH(256, k_gardner_chain, dim3(1), dim3(256), 0, st,      // 4 wavefronts: a walked chunk is staged 4x faster
                                   (const float *)d_agc, GP, GD, n_groups,
                                   (const unsigned *)ctx->gtable.p, (const GardnerSegCell *)ctx->gsegmap.p, G,
                                   (GardnerSegStart *)ctx->gsegstart.p, (GardnerEntry<float> *)ctx->gentries.p, d_sc->gstats,
                                   (const GardnerBand *)ctx->gbands.p, n_tab, chain_carry, (seg && seg->have_sampler) ? 1 : 0, c_hi,
                                   (GardnerChainState *)ctx->gchain.p, r == 0 ? 1 : 0,
                                   (const unsigned *)(GD.span > 1 ? ctx->gspan_keys.p : nullptr), (const unsigned *)(GD.span > 1 ? ctx->gspan_tails.p : nullptr),
                                   (const GardnerSpanRow *)(GD.span > 1 ? ctx->gspan_rows.p : nullptr));
                L.end();
                if (side) PL.simple(OP_FORK);
                const long long s_lo = c_lo / G, s_hi = (c_hi + G - 1) / G;
                L.begin("gardner", st_emit);
                if (s_hi > s_lo)
                    PDT_LAUNCH(64, k_gardner_segfill, dim3((unsigned)(s_hi - s_lo)), dim3(64), 0, st_emit, (const float *)d_agc, GP, GD, n_groups,
                                       (const unsigned *)ctx->gtable.p, G, (const GardnerSegStart *)ctx->gsegstart.p,
                                       (GardnerEntry<float> *)ctx->gentries.p, s_lo);
                // per-chunk emission: small LDS windows so that every chunk of a 10-minute capture is resident at once
                const unsigned char *d_flags = nullptr;
                if (GD.span > 1 && 8 * (long long)GP.step + 256 < PDT_GEMIT_SUB_WIN && !ctx->tune.gemit_groups &&
                    (double)PDT_GEMIT_SUB_WIN / ((double)GP.step - 0.2) + 2.0 < (double)PDT_GSUB_OUT) {
                    // rows of several chunks: four CHUNKS per wavefront (k_gardner_emit_first / _rest); the groups these cannot resolve,
                    // and the one behind the last row, go through the wavefront-per-group kernel below
                    if ((rc = ctx->gcentries.ensure((size_t)n_chunks * sizeof(GardnerEntry<float>)))) return rc;
                    if ((rc = ctx->gflags.ensure((size_t)n_groups + 64))) return rc;
                    PL.memset_async(ctx->gflags.p, 1, (size_t)n_groups, PL.side_of(st_emit));
                    PDT_LAUNCH(64, (k_gardner_emit_first<PDT_GEMIT_SUB_WIN>), dim3((unsigned)((n_tab - g_first + 3) / 4)), dim3(64), 0, st_emit, (const float *)d_agc, GP, GD,
                                       n_tab, (const GardnerEntry<float> *)ctx->gentries.p, (const unsigned *)ctx->gspan_keys.p,
                                       (const GardnerSpanRow *)ctx->gspan_rows.p, (const GardnerSpanRec *)ctx->gspan_recs.p,
                                       (GardnerEntry<float> *)ctx->gcentries.p, (unsigned char *)ctx->gflags.p, (float *)d_sym, d_symidx, sym_cap, g_first,
                                       (const unsigned *)ctx->gspan_tails.p);
                    PDT_LAUNCH(64, (k_gardner_emit_rest<PDT_GEMIT_SUB_WIN>), dim3((unsigned)(((n_tab - g_first) * (GD.span - 1) + 3) / 4)), dim3(64), 0, st_emit,
                                       (const float *)d_agc, GP, GD, n_tab, (const GardnerEntry<float> *)ctx->gcentries.p,
                                       (const unsigned char *)ctx->gflags.p, (float *)d_sym, d_symidx, sym_cap, g_first);
                    d_flags = (const unsigned char *)ctx->gflags.p;
                }
                if (c_hi > c_lo)
                    PDT_LAUNCH(256, (k_gardner<float, PDT_GEMIT_LEN, PDT_GEMIT_OUT>), dim3((unsigned)(c_hi - c_lo)), dim3(PDT_GARDNER_THREADS), 0, st_emit,
                                       (const float *)d_agc, (const float *)d_lock, GP, (float *)d_sym, d_symidx, &d_sc->nsym, sym_cap,
                                       (const GardnerEntry<float> *)ctx->gentries.p, tab_carry, (SamplerCarry<float> *)d_carry_out, c_lo, GD.span, d_flags);
                L.end();
                c_lo = c_hi;
            }
            if (side) {
                PL.simple(OP_JOIN_RECORD);
                PL.simple(OP_JOIN_WAIT);
            }
        }
        return PDT_OK;
    }

    // the symbol sampler: tables, MMClockRecovery (one wavefront), or the sequential Gardner kernels (ring / small / generic)
    int rec_sampler()
    {
        int rc = PDT_OK;
        (void)rc;
        if (use_table) {
            if ((rc = rec_sampler_table())) return rc;
        } else if (use_mm) {
            // MMClockRecovery at the sampler's call site (SURVEY 8 row a13): sequential, one wavefront
            MmParams<T> MP;
            if ((rc = make_mm_params<T>(ctx, n_out, chunk_out, &MP))) return rc;
            L.begin("gardner");
            if (seg && !seg->have_sampler) carry_in.b = MP.step0;                 // (the M&M state starts at stepSize = Fs / baud, MMClockRecovery.c:20)
            rec_mm<T>(PL, st, d_agc, MP, d_sym, d_symidx, d_sc, sym_cap, carry_in, seg ? 1 : 0, d_carry_out);
            L.end();
        } else {
            L.begin("gardner");
            constexpr int SMALL_LEN = 32768 / (int)sizeof(T), SMALL_OUT = 1024;    // two 32 KiB windows
            const long long small_need = chunk_out + 2 * (long long)GP.step + 24;
            const double small_syms = (double)chunk_out / ((double)GP.step - 0.25) + 4.0;
            constexpr int RING_LEN = 20480 / (int)sizeof(T), RING_NB = 6, RING_OUT = 256;   // six 20 KiB buffers
            if (small_need <= RING_LEN && small_syms < RING_OUT && chunk_out >= 4 * (long long)GP.step + 8 && n_chunks >= 8 && !seg &&
                !ctx->tune.gardner_onebuf && !ctx->tune.gardner_noring) {
                const size_t need_bytes = ((size_t)n_chunks + 64 + 15) & ~(size_t)15;
                if ((rc = ctx->gneed.ensure(need_bytes + (size_t)n_chunks * sizeof(CalmEntry<T>)))) return rc;
                CalmEntry<T> *d_calm = (CalmEntry<T> *)((char *)ctx->gneed.p + need_bytes);
                PDT_LAUNCH(256, k_chunk_need<T>, dim3((unsigned)n_chunks), dim3(256), 0, st, (const T *)d_agc, n_out, chunk_out, n_chunks,
                                   (unsigned char *)ctx->gneed.p);
                // chunks without a walk in one stride: where sampling instants stay multiples of 2^(E - p) below 2^E (k_gardner_ring)
                T gran_scale = 0;
                if (!ctx->tune.gardner_nostride) {
                    const double top = (double)chunk_out + 2.0 * (double)GP.step + 2.0;
                    const int E = ilogb(top) + 1, p = sizeof(T) == 8 ? 53 : 24;
                    const T sc = (T)ldexp(1.0, p - E);
                    const T gstep = GP.step * sc;
                    if (E < p && gstep == (T)rint((double)gstep) && (double)gstep < ldexp(1.0, p - 1)) gran_scale = sc;
                }
                PDT_LAUNCH(64 * (RING_NB + 1), (k_gardner_ring<T, RING_LEN, RING_NB, RING_OUT>), dim3(1), dim3(64 * (RING_NB + 1)), 0, st,
                                   (const T *)d_agc, (const T *)d_lock, GP, (const unsigned char *)ctx->gneed.p, d_sym, d_symidx, &d_sc->nsym,
                                   sym_cap, d_calm, gran_scale);
                PDT_LAUNCH(256, k_calm_emit<T>, dim3((unsigned)((n_chunks + 255) / 256)), dim3(256), 0, st, (const unsigned char *)ctx->gneed.p,
                                   (const CalmEntry<T> *)d_calm, GP, d_sym, d_symidx, sym_cap);
            } else if (small_need <= SMALL_LEN && small_syms < SMALL_OUT && !ctx->tune.gardner_onebuf && !seg)
                PDT_LAUNCH(256, (k_gardner_small<T, SMALL_LEN, SMALL_OUT>), dim3(1), dim3(256), 0, st, (const T *)d_agc, (const T *)d_lock, GP,
                                   d_sym, d_symidx, &d_sc->nsym, sym_cap);
            else
                rec_gardner_walk<T>(PL, st, d_agc, d_lock, GP, d_sym, d_symidx, d_sc, sym_cap, carry_in, d_carry_out);
            L.end();
        }

        return PDT_OK;
    }

    // ManchesterDecode, the byte synchroniser, a segment's tail record, the per-chunk reports
    int rec_bits()
    {
        int rc = PDT_OK;
        (void)rc;
        // ---- Manchester
        L.begin("manchester");
        if (ctx->tune.manch_3pass) {
            rec_manch_3pass<T>(PL, st, d_sym, d_sc, manch_thr, d_tiles, n_tiles, sym_pad, clock0, bit0, seg ? &d_tail->clock : (unsigned *)nullptr,
                               d_bits, d_bitsym, bit_cap);
        } else {
            // one pass with look-back; its status words live where the tile summaries of the three passes would
            // (n_tiles records of 32 bytes hold the n_one + 1 <= n_tiles + 1 words)
            constexpr int ONE_NT = ManchOnePass<T>::NT, ONE_TILE = ManchOnePass<T>::TILE;
            const long long n_one = (sym_cap + ONE_TILE - 1) / ONE_TILE;
            unsigned long long *d_mstat = (unsigned long long *)d_tiles;
            PL.memset_async(d_mstat, 0, (size_t)(n_one + 1) * sizeof(unsigned long long), PL.side_of(st));
            PDT_LAUNCH(ONE_NT, k_manch_onepass<T>, dim3((unsigned)n_one), dim3(ONE_NT), 0, st, d_sym, &d_sc->nsym,
                               manch_thr, d_mstat, d_bits, d_bitsym, bit_cap, sym_pad, clock0, bit0, &d_sc->nbits,
                               seg ? &d_tail->clock : (unsigned *)nullptr, sym_cap);
        }
        L.end();

        // ---- byte sync
        L.begin("bytesync");
        launch_bytesync(ctx, PL, st, SP, d_sc, bit_cap, hit_cap, frame_cap, sync_min_pos);
        L.end();
        if (seg) {
            // everything the next segment starts from, in one record
            const long long last_pll = (N > 0) ? (N - 1) / Bp : -1;
            PDT_LAUNCH(256, (k_seg_tail<T, PllSeam<T>, AgcSeam<T>>), dim3(1), dim3(256), 0, st, (const PllSeam<T> *)ctx->seams_pll.p, last_pll,
                       (const T *)d_lock, N, (const AgcSeam<T> *)ctx->seams_agc.p, agc_last_block, (const T *)d_sym, &d_sc->nsym,
                       (const unsigned char *)d_bits, (const unsigned *)d_bitsym, (const long long *)d_symidx, &d_sc->nbits,
                       (long long)bit0, d_tail);
            PL.copy(OP_D2H, spin + 4096, d_tail, sizeof(SegTail<T>));
        }
        ctx->pend_chunks = 0;
        if (inject) {
            // the stage call ends behind the PLL: drop what was recorded for the later stages (their counters stay zero)
            PL.ops.resize(ops_after_pll);
        } else if (quality && n_chunks > 0) {
            // (N > 0 here; a context without a PLL run -- never -- would leave avg_phase 0)
            if (quality_side) {                                  // the averagePhase stream is complete
                PL.simple(OP_JOIN_RECORD);
                PL.simple(OP_JOIN_WAIT);
            }
            PDT_LAUNCH(256, k_chunk_info<T>, dim3((unsigned)((n_chunks + 255) / 256)), dim3(256), 0, st, (const T *)d_avgph, N, chunk, n_chunks,
                               interp, (const long long *)d_symidx, (const unsigned long long *)&d_sc->nsym, (const unsigned *)d_bitsym,
                               (const unsigned long long *)&d_sc->nbits, (ChunkInfo *)ctx->chunkinfo.p);
            // (a segment: the new chunks' records; those of the window's history were reported by the segments before)
            const long long rep_first = seg ? first / chunk : 0;
            PL.copy(OP_D2H, ctx->qual_pin, (const ChunkInfo *)ctx->chunkinfo.p + rep_first, (size_t)(n_chunks - rep_first) * sizeof(ChunkInfo));
            ctx->pend_chunks = (uint64_t)(n_chunks - rep_first);
        }
        PL.simple(OP_EV1);

        return PDT_OK;
    }

    // results back to the host: scalars, lock record, (speculatively) the frame records; RUN_ALL executes the plan
    int rec_readback()
    {
        int rc = PDT_OK;
        (void)rc;
        // ---- results back to the host
        // one synchronisation: the scalars, the lock record and (speculatively, into pinned memory) as many frame
        // records as the previous call of this context produced, plus a margin
        // (the overlapped ingest's segments differ in length: the whole capacity -- about twice what a segment yields, a few MB into
        // pinned memory -- rather than a second, blocking copy between two segments)
        const uint32_t spec_frames = (seg && seg->in_place) ? frame_cap : std::min<uint32_t>(frame_cap, ctx->last_nframes + ctx->last_nframes / 8 + 64);
        if ((size_t)spec_frames * sizeof(FrameRec) > ctx->pinned_cap) {
            if (ctx->pinned) (void)hipHostFree(ctx->pinned);
            ctx->pinned = nullptr;
            ctx->pinned_cap = 0;
            const size_t want = (size_t)spec_frames * sizeof(FrameRec) * 2 + 4096;
            if (timed_host_malloc((void **)&ctx->pinned, want) == hipSuccess) ctx->pinned_cap = want;
            else (void)hipGetLastError();
        }
        const uint32_t got_frames = (ctx->pinned_cap >= (size_t)spec_frames * sizeof(FrameRec)) ? spec_frames : 0u;
        static_assert(sizeof(PllLockInfo<T>) <= 96, "lock record staging");
        PL.copy(OP_D2H, ctx->pend_sc, d_sc, sizeof(DevScalars));
        PL.copy(OP_D2H, ctx->pend_info, d_info, sizeof(PllLockInfo<T>));
        if (got_frames) PL.copy(OP_D2H, ctx->pinned, d_frames, (size_t)got_frames * sizeof(FrameRec));
        ctx->pend_got_frames = got_frames;
        ctx->pend_n = n;
        ctx->pending = true;
        if (phase == RUN_ALL) {
            pdt_ctx *self = ctx;
            if ((rc = execute_plans(&self, 1))) return rc;
        }
        return PDT_OK;
    }

    int run()
    {
        int rc;
        params();
        if ((rc = geometry())) return rc;
        if ((rc = allocate())) return rc;
        if (phase != RUN_FINISH) {
            if ((rc = rec_begin())) return rc;
            if ((rc = rec_pll_walkers())) return rc;
            if ((rc = rec_pll_serial())) return rc;
            ops_after_pll = PL.ops.size();
            ctx->last_pll_block = Bp;
            if ((rc = rec_fir())) return rc;
            if (quality_after_fir) rec_quality_walkers(false);     // behind the kernel that wrote their input (side stream: nothing waits for them)
            if ((rc = rec_agc())) return rc;
            sampler_domain();
            sampler_carry();
            if ((rc = rec_sampler())) return rc;
            if ((rc = rec_bits())) return rc;
            if ((rc = rec_readback())) return rc;
        }
        if (phase == RUN_ENQUEUE) return PDT_OK;
        FinishArgs FA;
        FA.argos = argos; FA.need_lock = need_lock; FA.fuse_mix = fuse_mix;
        FA.N = N; FA.n_out = n_out; FA.chunk = chunk; FA.chunk_out = chunk_out; FA.first = first; FA.first_out = first_out; FA.sym_cap = sym_cap;
        FA.interp = interp; FA.ntaps = ntaps; FA.hit_cap = hit_cap; FA.frame_cap = frame_cap; FA.SP = SP;
        return finish_capture<T>(ctx, n, FA);

    }
};

template <typename T> int run_capture(pdt_ctx *ctx, uint64_t n, int phase)
{
    return Chain<T>(ctx, n, phase).run();
}


// ---------------------------------------------------------------- stage-level entry points (SURVEY 8b)
// One stage of the chain on caller data, the reference function's hidden statics as an explicit state record, so that the
// per-chunk dumps of the reference (or of the oracle) can be replayed stage by stage through the kernels the whole-capture
// path uses.
template <typename T> int stage_manchester(pdt_ctx *ctx, const void *sym_host, uint64_t nsym, double thr_d,
                                                  pdt_manchester_state *state, uint8_t *bits_out, uint32_t *bit_symbol_out,
                                                  uint64_t *nbits_out)
{
    pdt_manchester_state fresh;
    memset(&fresh, 0, sizeof fresh);
    if (!state) state = &fresh;
    // the two symbols the decisions look back on go in front, placed so that local and stream symbol parities agree
    const long long pad = 2 + (long long)(state->even_odd & 1u);
    const long long total = pad + (long long)nsym;
    const long long sym_cap = total + 64, bit_cap = sym_cap;
    const long long n_tiles = (sym_cap + PDT_TILE - 1) / PDT_TILE;
    int rc;
    if ((rc = ctx->sym.ensure((size_t)sym_cap * sizeof(T)))) return rc;
    if ((rc = ctx->bits.ensure((size_t)bit_cap))) return rc;
    if ((rc = ctx->bitsym.ensure((size_t)bit_cap * sizeof(unsigned)))) return rc;
    if ((rc = ctx->hits.ensure((size_t)n_tiles * sizeof(ManchTile)))) return rc;
    if ((rc = ctx->scal.ensure(sizeof(DevScalars)))) return rc;
    T *d_sym = (T *)ctx->sym.p;
    ManchTile *d_tiles = (ManchTile *)ctx->hits.p;
    DevScalars *d_sc = (DevScalars *)ctx->scal.p;
    DevScalars sc;
    memset(&sc, 0, sizeof sc);
    sc.nsym = (unsigned long long)total;
    T hist[4] = { 0, 0, 0, 0 };
    hist[pad - 2] = (T)state->previous;
    hist[pad - 1] = (T)state->current;
    Plan &PL = oneshot_begin(ctx);
    PL.copy(OP_H2D, d_sc, &sc, sizeof sc);
    PL.copy(OP_H2D, d_sym, hist, (size_t)pad * sizeof(T));
    if (nsym) PL.copy(OP_H2D, d_sym + pad, sym_host, (size_t)nsym * sizeof(T));
    rec_manch_3pass<T>(PL, ctx->stream, d_sym, d_sc, (T)thr_d, d_tiles, n_tiles, pad, (unsigned)(state->clockmod & 1u), 0ull, &d_sc->pad0_,
                       (unsigned char *)ctx->bits.p, (unsigned *)ctx->bitsym.p, bit_cap);
    if ((rc = oneshot_run(ctx, d_sc, &sc))) return rc;
    if ((long long)sc.nbits > bit_cap) return PDT_ERR_STATE;
    if (sc.nbits && bits_out) HIP_TRY(hipMemcpy(bits_out, ctx->bits.p, (size_t)sc.nbits, hipMemcpyDeviceToHost));
    if (sc.nbits && bit_symbol_out) {
        HIP_TRY(hipMemcpy(bit_symbol_out, ctx->bitsym.p, (size_t)sc.nbits * sizeof(unsigned), hipMemcpyDeviceToHost));
        for (uint64_t b = 0; b < sc.nbits; b++) bit_symbol_out[b] -= (uint32_t)pad;       // index into this call's symbols
    }
    if (nbits_out) *nbits_out = sc.nbits;
    // ManchesterDecode.c:16-20: the statics after the call
    const T *sy = (const T *)sym_host;
    if (nsym >= 2) { state->previous = (double)sy[nsym - 2]; state->current = (double)sy[nsym - 1]; }
    else if (nsym == 1) { state->previous = state->current; state->current = (double)sy[0]; }
    state->clockmod = sc.pad0_;
    state->even_odd = (uint32_t)((state->even_odd + nsym) & 0xffu);                       // unsigned char evenOddCounter
    memset(ctx->stage_len, 0, sizeof ctx->stage_len);
    return PDT_OK;
}

template <typename T> int stage_fir(pdt_ctx *ctx, const void *in_host, uint64_t n, pdt_fir_state *state, void *out_host)
{
    pdt_fir_state fresh;
    memset(&fresh, 0, sizeof fresh);
    if (!state) state = &fresh;
    const bool argos = ctx->cfg.mode == PDT_MODE_ARGOS;
    const int interp = (int)ctx->interp, ntaps = (int)ctx->ntaps;
    const int K = argos ? ntaps : ntaps / interp;                      // inputs an output looks back on
    if (K < 1 || K > 64) return PDT_ERR_ARG;
    // POES: the reference's ring keeps input m in slot m mod K and sums the slots in ascending order (LowPassFilter.c:43-70),
    // so the local index of every input must equal its stream index modulo K: p zeros, the K last inputs, the new ones
    const long long p = argos ? 0 : (long long)(state->count % (uint64_t)K);
    const long long lead = p + K;
    const long long N = lead + (long long)n;
    int rc;
    if ((rc = ctx->pll.ensure((size_t)(N + 1) * sizeof(T)))) return rc;
    if ((rc = ctx->fir.ensure((size_t)(N * interp + 1) * sizeof(T)))) return rc;
    T *d_in = (T *)ctx->pll.p, *d_out = (T *)ctx->fir.p;
    std::vector<T> head((size_t)lead, (T)0);
    for (int i = 0; i < K; i++) head[(size_t)(p + i)] = (T)state->history[i];
    Plan &PL = oneshot_begin(ctx);
    PL.copy(OP_H2D, d_in, head.data(), (size_t)lead * sizeof(T));
    if (n) PL.copy(OP_H2D, d_in + lead, in_host, (size_t)n * sizeof(T));
    rec_fir_unfused<T>(ctx, PL, ctx->stream, (const T *)d_in, N, d_out, (AgcMap *)nullptr, (T)0);
    if ((rc = oneshot_run(ctx))) return rc;
    if (n && out_host)
        HIP_TRY(hipMemcpy(out_host, d_out + lead * interp, (size_t)n * (size_t)interp * sizeof(T), hipMemcpyDeviceToHost));
    // the ring after the call: the last K inputs, oldest first
    const T *x = (const T *)in_host;
    double nh[64];
    for (int i = 0; i < K; i++) {
        const long long src = (long long)n - K + i;                   // index into the new inputs, negative = older history
        nh[i] = src >= 0 ? (double)x[src] : state->history[K + src];
    }
    memcpy(state->history, nh, sizeof(double) * (size_t)K);
    state->count += n;
    memset(ctx->stage_len, 0, sizeof ctx->stage_len);
    return PDT_OK;
}

template <typename T> int stage_pll(pdt_ctx *ctx, const void *iq_host, uint64_t n, int fmt, pdt_pll_state *state, void *out_host,
                                           void *lock_out_host, double *avg_phase_ret)
{
    const size_t fb = fmt == PDT_FMT_F32 ? 8 : 4;                     // bytes per I,Q pair
    pdt_pll_state fresh;
    memset(&fresh, 0, sizeof fresh);
    if (!state) state = &fresh;
    if (n == 0) {                                                     // the loop body never runs; :277 returns the static
        if (avg_phase_ret) *avg_phase_ret = state->started ? state->avg_phase : 0.0;
        return PDT_OK;
    }
    const bool was_locked = state->started && state->locked;
    const uint64_t lead = was_locked ? 1 : 0;                         // a dummy sample in front stands for "locked before sample 0"
    const uint64_t N = n + lead;
    ctx->pcm_retaken();                                                       // (a search of host memory read this buffer)
    int rc = ctx->pcm.ensure((size_t)N * fb + 16);
    if (rc) return rc;
    HIP_TRY(hipMemset(ctx->pcm.p, 0, 8));
    HIP_TRY(hipMemcpy((char *)ctx->pcm.p + lead * fb, iq_host, (size_t)n * fb, hipMemcpyHostToDevice));
    ctx->pcm_dev = ctx->pcm.p;
    ctx->pcm_fmt = fmt == PDT_FMT_F32 ? 1 : 0;                        // float pairs = `float complex` as they are / int16 pairs, wave.c:127-172
    ctx->inj.active = true;
    ctx->inj.started = state->started != 0;
    ctx->inj.locked = was_locked;
    ctx->inj.phase = state->phase; ctx->inj.freq = state->freq; ctx->inj.avg = state->avg_phase;
    ctx->inj.locksig = state->locksig; ctx->inj.sweep = state->sweep;
    ctx->batch_hint = 1;
    ctx->n_samples = N;
    ctx->n_out = N * ctx->interp;
    rc = run_capture<T>(ctx, N, RUN_ALL);
    ctx->inj.active = false;
    if (rc) return rc;
    // outputs and the statics after the call, from the streams the run left on the device
    if (out_host) HIP_TRY(hipMemcpy(out_host, (const T *)ctx->pll.p + lead, (size_t)n * sizeof(T), hipMemcpyDeviceToHost));
    if (lock_out_host) HIP_TRY(hipMemcpy(lock_out_host, (const T *)ctx->lock.p + lead, (size_t)n * sizeof(T), hipMemcpyDeviceToHost));
    T last_lock = 0, last_avg = 0;
    HIP_TRY(hipMemcpy(&last_lock, (const T *)ctx->lock.p + (N - 1), sizeof(T), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&last_avg, (const T *)ctx->avgph.p + (N - 1), sizeof(T), hipMemcpyDeviceToHost));
    PllLockInfo<T> info;
    HIP_TRY(hipMemcpy(&info, ctx->lockinfo.p, sizeof info, hipMemcpyDeviceToHost));
    state->started = 1;
    if (info.lock_sample < 0) {                                       // still searching: the acquisition's state after the last sample
        state->phase = (double)info.st.phase; state->freq = (double)info.st.freq; state->sweep = (double)info.st.sweep;
    } else {
        if (!was_locked) {
            state->locked = 1;
            state->lock_index = info.lock_sample;
            state->lock_freq_hz = (double)(info.freq_at_lock * (T)ctx->cfg.sample_rate) / (2.0 * M_PI);   // CarrierTrackingPLL.c:269
        }
        state->sweep = (double)info.st.sweep;
        if (info.lock_sample == (long long)N - 1) {                   // locked on the very last sample: nothing walked behind it
            state->phase = (double)info.st.phase; state->freq = (double)info.st.freq;
        } else {
            PllSeam<T> sm;
            const long long Bp = ctx->last_pll_block > 0 ? ctx->last_pll_block : 1;
            HIP_TRY(hipMemcpy(&sm, (const PllSeam<T> *)ctx->seams_pll.p + ((long long)N - 1) / Bp, sizeof sm, hipMemcpyDeviceToHost));
            state->phase = (double)sm.phase1; state->freq = (double)sm.freq1;
        }
    }
    state->locksig = (double)last_lock;
    state->avg_phase = (double)last_avg;
    if (avg_phase_ret) *avg_phase_ret = (double)last_avg;
    memset(ctx->stage_len, 0, sizeof ctx->stage_len);
    ctx->frames_host.clear();
    return PDT_OK;
}

template <typename T> int stage_gardner(pdt_ctx *ctx, const void *in_host, uint64_t n, uint64_t capacity,
                                               const void *neighbour_host, pdt_gardner_state *state, void *out_host,
                                               uint64_t *pick_out, uint64_t *nsym_out)
{
    pdt_gardner_state fresh;
    memset(&fresh, 0, sizeof fresh);
    if (!state) state = &fresh;
    const bool argos = ctx->cfg.mode == PDT_MODE_ARGOS;
    const long long C = (long long)capacity, na = (long long)n;
    // The sampler's reads past the chunk (Q3: the mid-point index is not rolled over with nextSample) see what the caller's
    // buffer still holds behind element n -- for the kernels that is "the previous chunk of the stream": a stream of two
    // chunks of C, the buffer as it stands and then its first n elements, walked from chunk 1 on.
    const long long total = C + na;
    GardnerParams<T> GP = make_gardner_params<T>(ctx, total, C);
    if (argos && neighbour_host && (size_t)C * 8 < 128 * 1024) {              // Q16: the array malloc'd behind this one
        const unsigned long long req = 8ull * (unsigned long long)C;
        GP.argos_heap = 1;
        GP.argos_field_bits = ((req + 8 + 15) & ~15ull) | 1ull;
        GP.argos_even = ((req + 8) % 16) != 0;
    }
    const long long sym_cap = (long long)((double)na / ((double)GP.step - 0.25)) + 64;
    int rc;
    if ((rc = ctx->agc.ensure((size_t)(total + 1) * sizeof(T)))) return rc;
    if ((rc = ctx->lock.ensure((size_t)(total + 1) * sizeof(T)))) return rc;
    if ((rc = ctx->sym.ensure((size_t)sym_cap * sizeof(T)))) return rc;
    if ((rc = ctx->symidx.ensure((size_t)sym_cap * sizeof(long long)))) return rc;
    if ((rc = ctx->scal.ensure(sizeof(DevScalars)))) return rc;
    if ((rc = ctx->seg_dev.ensure(sizeof(SegTail<T>) + 256))) return rc;
    T *d_in = (T *)ctx->agc.p, *d_nb = (T *)ctx->lock.p;
    DevScalars *d_sc = (DevScalars *)ctx->scal.p;
    SegTail<T> *d_tail = (SegTail<T> *)ctx->seg_dev.p;
    SamplerCarry<T> carry_in;
    carry_in.a = (T)state->next_sample; carry_in.b = (T)state->prev_bit; carry_in.c = (T)state->half_sample;
    carry_in.c_first = 1; carry_in.count0 = 0;
    Plan &PL = oneshot_begin(ctx);
    PL.memset_async(d_sc, 0, sizeof(DevScalars));
    PL.copy(OP_H2D, d_in, in_host, (size_t)C * sizeof(T));
    if (na) PL.copy(OP_H2D, d_in + C, in_host, (size_t)na * sizeof(T));
    if (GP.argos_heap) {
        PL.copy(OP_H2D, d_nb, neighbour_host, (size_t)C * sizeof(T));
        if (na) PL.copy(OP_H2D, d_nb + C, neighbour_host, (size_t)na * sizeof(T));
    }
    rec_gardner_walk<T>(PL, ctx->stream, d_in, GP.argos_heap ? d_nb : nullptr, GP, (T *)ctx->sym.p, (long long *)ctx->symidx.p, d_sc, sym_cap, carry_in,
                        &d_tail->sampler);
    DevScalars sc;
    if ((rc = oneshot_run(ctx, d_sc, &sc))) return rc;
    const uint64_t nsym = sc.nsym;
    if ((long long)nsym > sym_cap) return PDT_ERR_STATE;
    if (nsym && out_host) HIP_TRY(hipMemcpy(out_host, ctx->sym.p, (size_t)nsym * sizeof(T), hipMemcpyDeviceToHost));
    if (nsym && pick_out) {
        HIP_TRY(hipMemcpy(pick_out, ctx->symidx.p, (size_t)nsym * sizeof(long long), hipMemcpyDeviceToHost));
        for (uint64_t k = 0; k < nsym; k++) pick_out[k] -= (uint64_t)C;                      // index into this call's samples
    }
    if (nsym_out) *nsym_out = nsym;
    SamplerCarry<T> after;
    HIP_TRY(hipMemcpy(&after, &d_tail->sampler, sizeof after, hipMemcpyDeviceToHost));
    state->next_sample = (double)after.a; state->prev_bit = (double)after.b; state->half_sample = (double)after.c;
    memset(ctx->stage_len, 0, sizeof ctx->stage_len);
    return PDT_OK;
}

template <typename T> int stage_static_gain(pdt_ctx *ctx, const void *iq_host, uint64_t n, int fmt, double level, double *gain_out)
{
    const size_t fb = fmt == PDT_FMT_F32 ? 8 : 4;
    int rc;
    ctx->pcm_retaken();                                                       // (a search of host memory read this buffer)
    if ((rc = ctx->pcm.ensure((size_t)n * fb + 16))) return rc;
    if ((rc = ctx->mag.ensure((size_t)(n + 1) * sizeof(T)))) return rc;
    if ((rc = ctx->scal.ensure(sizeof(DevScalars)))) return rc;
    DevScalars *d_sc = (DevScalars *)ctx->scal.p;
    IqSrc src;
    src.p = ctx->pcm.p;
    src.fmt = fmt == PDT_FMT_F32 ? 1 : 0;
    Plan &PL = oneshot_begin(ctx);
    PL.memset_async(d_sc, 0, sizeof(DevScalars));
    PL.copy(OP_H2D, ctx->pcm.p, iq_host, (size_t)n * fb);
    rec_static_gain<T>(PL, ctx->stream, src, (long long)n, (T *)ctx->mag.p, (T)level, 0.0, (T *)&d_sc->norm);
    DevScalars sc;
    if ((rc = oneshot_run(ctx, d_sc, &sc))) return rc;
    T g;
    memcpy(&g, &sc.norm, sizeof(T));
    if (gain_out) *gain_out = (double)g;
    return PDT_OK;
}

template <typename T> int stage_mm(pdt_ctx *ctx, const void *in_host, uint64_t n, pdt_mm_state *state, void *out_host,
                                          uint64_t *pick_out, uint64_t *nsym_out)
{
    pdt_mm_state fresh;
    memset(&fresh, 0, sizeof fresh);
    if (!state) state = &fresh;
    if (nsym_out) *nsym_out = 0;
    int rc;
    MmParams<T> MP;
    if ((rc = make_mm_params<T>(ctx, (long long)n, (long long)n, &MP))) return rc;         // one call = one chunk
    if (!state->started) { state->started = 1; state->next_sample = 0; state->step_size = (double)MP.step0; state->sample_last = 0; }
    if (n == 0) return PDT_OK;
    const long long sym_cap = (long long)((double)n / ((double)MP.step_min * 0.999)) + 64;
    if ((rc = ctx->agc.ensure((size_t)(n + 1) * sizeof(T)))) return rc;
    if ((rc = ctx->sym.ensure((size_t)sym_cap * sizeof(T)))) return rc;
    if ((rc = ctx->symidx.ensure((size_t)sym_cap * sizeof(long long)))) return rc;
    if ((rc = ctx->scal.ensure(sizeof(DevScalars)))) return rc;
    if ((rc = ctx->seg_dev.ensure(sizeof(SegTail<T>) + 256))) return rc;
    DevScalars *d_sc = (DevScalars *)ctx->scal.p;
    SegTail<T> *d_tail = (SegTail<T> *)ctx->seg_dev.p;
    SamplerCarry<T> carry_in;
    carry_in.a = (T)state->next_sample; carry_in.b = (T)state->step_size; carry_in.c = (T)state->sample_last;
    carry_in.c_first = 0; carry_in.count0 = 0;
    Plan &PL = oneshot_begin(ctx);
    PL.memset_async(d_sc, 0, sizeof(DevScalars));
    PL.copy(OP_H2D, ctx->agc.p, in_host, (size_t)n * sizeof(T));
    rec_mm<T>(PL, ctx->stream, (const T *)ctx->agc.p, MP, (T *)ctx->sym.p, (long long *)ctx->symidx.p, d_sc, sym_cap, carry_in, 1, &d_tail->sampler);
    DevScalars sc;
    if ((rc = oneshot_run(ctx, d_sc, &sc))) return rc;
    const uint64_t nsym = sc.nsym;
    if ((long long)nsym > sym_cap) return PDT_ERR_STATE;
    if (nsym && out_host) HIP_TRY(hipMemcpy(out_host, ctx->sym.p, (size_t)nsym * sizeof(T), hipMemcpyDeviceToHost));
    if (nsym && pick_out) HIP_TRY(hipMemcpy(pick_out, ctx->symidx.p, (size_t)nsym * sizeof(long long), hipMemcpyDeviceToHost));
    if (nsym_out) *nsym_out = nsym;
    SamplerCarry<T> after;
    HIP_TRY(hipMemcpy(&after, &d_tail->sampler, sizeof after, hipMemcpyDeviceToHost));
    state->next_sample = (double)after.a; state->step_size = (double)after.b; state->sample_last = (double)after.c;
    memset(ctx->stage_len, 0, sizeof ctx->stage_len);
    return PDT_OK;
}

template <typename T> int stage_agc(pdt_ctx *ctx, void *data_host, uint64_t n, double initial, double attack, double decay,
                                           pdt_agc_state *state)
{
    pdt_agc_state fresh;
    memset(&fresh, 0, sizeof fresh);
    if (!state) state = &fresh;
    const AgcParams<T> AP = make_agc_params<T>(ctx, attack, decay);
    const T gain0 = state->started ? (T)state->gain : (T)initial;              // AGC.c:91-95: `initial` counts on the first call only
    state->started = 1;
    if (n == 0) { state->gain = (double)gain0; return PDT_OK; }
    // the whole-capture path's block geometry (any values give the same output)
    long long Ba, Wa;
    agc_block_warm(ctx, &Ba, &Wa);
    const long long na = (long long)n, nb = (na + Ba - 1) / Ba;
    int rc;
    if ((rc = ctx->fir.ensure((size_t)(na + 1) * sizeof(T)))) return rc;
    if ((rc = ctx->agc.ensure((size_t)(na + 1) * sizeof(T)))) return rc;
    if ((rc = ctx->seams_agc.ensure((size_t)(nb + 1) * sizeof(AgcSeam<T>)))) return rc;
    if ((rc = ctx->agc_maps.ensure((size_t)(nb + 1) * (sizeof(AgcMap) + sizeof(double))))) return rc;
    if ((rc = ctx->scal.ensure(sizeof(DevScalars)))) return rc;
    const T *a_in = (const T *)ctx->fir.p;
    T *a_out = (T *)ctx->agc.p, *ckpt;
    DevScalars *d_sc = (DevScalars *)ctx->scal.p;
    AgcMap *d_maps = (AgcMap *)ctx->agc_maps.p;
    DevScalars sc;
    memset(&sc, 0, sizeof sc);
    memcpy(&sc.norm, &gain0, sizeof(T));
    Plan &PL = oneshot_begin(ctx);
    PL.copy(OP_H2D, d_sc, &sc, sizeof sc);
    PL.copy(OP_H2D, ctx->fir.p, data_host, (size_t)na * sizeof(T));
    if ((rc = rec_agc_lanes<T>(ctx, PL, ctx->stream, a_in, na, AP, (T *)&d_sc->norm, Ba, Wa, true, d_maps, (double *)(d_maps + nb + 1), (const T *)nullptr, a_out,
                               &ckpt)))
        return rc;
    rec_agc_fix<T>(ctx, PL, ctx->stream, a_in, na, AP, Ba, (const T *)nullptr, a_out, d_sc, ckpt);
    if ((rc = oneshot_run(ctx))) return rc;
    HIP_TRY(hipMemcpy(data_host, a_out, (size_t)na * sizeof(T), hipMemcpyDeviceToHost));      // in place, as the reference
    AgcSeam<T> last;
    HIP_TRY(hipMemcpy(&last, (const AgcSeam<T> *)ctx->seams_agc.p + (nb - 1), sizeof last, hipMemcpyDeviceToHost));
    state->gain = (double)last.g1;
    memset(ctx->stage_len, 0, sizeof ctx->stage_len);
    return PDT_OK;
}

template <typename T> int stage_squelch(pdt_ctx *ctx, void *data_host, const void *lock_host, uint64_t n, double thr)
{
    if (n == 0) return PDT_OK;
    int rc;
    if ((rc = ctx->agc.ensure((size_t)(n + 4) * sizeof(T)))) return rc;
    if ((rc = ctx->lock.ensure((size_t)(n + 4) * sizeof(T)))) return rc;
    Plan &PL = oneshot_begin(ctx);
    PL.copy(OP_H2D, ctx->agc.p, data_host, (size_t)n * sizeof(T));
    PL.copy(OP_H2D, ctx->lock.p, lock_host, (size_t)n * sizeof(T));
    rec_squelch<T>(PL, ctx->stream, (T *)ctx->agc.p, (const T *)ctx->lock.p, (long long)n, (T)thr);
    if ((rc = oneshot_run(ctx))) return rc;
    HIP_TRY(hipMemcpy(data_host, ctx->agc.p, (size_t)n * sizeof(T), hipMemcpyDeviceToHost));
    memset(ctx->stage_len, 0, sizeof ctx->stage_len);
    return PDT_OK;
}
}  // namespace pdtrt
