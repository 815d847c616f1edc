// pdt_bursts.hip -- short transmissions in a wideband capture (pdt_bursts.h): the survey's transform with the time axis kept (the
// waterfall: k_spectra of pdt_survey.hip, one row of power sums per R segments), the peaks of every row (k_row_peaks), and the host
// restatement pdt_host_bursts with the linking of peaks into bursts and of bursts into platforms.  A unit of its own, beside
// pdt_survey.hip.
#include <math.h>
#include <string.h>
#include <algorithm>

#include "../../include/pdt.h"
#include "pdt_bursts.h"

static_assert(sizeof(pdt_burst) == sizeof(pdt::Burst) && sizeof(pdt_burst) == 48, "pdt_burst");
static_assert(sizeof(pdt_row_peak) == sizeof(pdt::BurstPeak) && sizeof(pdt_row_peak) == 16, "pdt_row_peak");

namespace pdt {

// rows of one workgroup of the waterfall's launch: about BURST_BATCH_SEGS segments, so that at small R the window and twiddle traffic
// and the launch are not paid per row
inline int burst_rows_per_group(int rows_per)
{
    return rows_per >= BURST_BATCH_SEGS ? 1 : BURST_BATCH_SEGS / rows_per;
}

constexpr int PEAKS_TB = 256;

// One workgroup per row.  The row's keys (burst_key) go into LDS in natural bin order -- place i of the row is bin survey_rev(i) --,
// N words: 64 KiB at N = 16384.  The places a half-wave loads together are bins N / 16 apart, one bank; bin b is therefore kept at
// peaks_at(b), its low five bits exchanged by the bits those places differ in: a permutation inside every 32 consecutive bins.
// A candidate is (key << 32) | ~bin, so the largest candidate is the strongest bin and of equal ones the lowest; each round reduces
// the lanes' candidates over the wavefront by shuffles and over the four wavefronts through LDS, every lane reads the winner, lane 0
// records it, its neighbourhood is blanked in LDS and the lanes look through the keys again.  No atomics; the result does not
// depend on the order in which anything runs.
template <int LOG4> __device__ __forceinline__ int peaks_at(int b)
{
    return b ^ ((b >> (2 * LOG4 - 8)) & 31);
}

__device__ __forceinline__ unsigned long long peaks_cand(uint32_t key, int bin)
{
    return ((unsigned long long)key << 32) | (unsigned long long)(0xffffffffu - (uint32_t)bin);
}

template <int N>
__global__ void __launch_bounds__(PEAKS_TB) k_row_peaks(const float *__restrict__ rows, float level, int gb, BurstPeak *__restrict__ peaks,
                                                        int *__restrict__ counts)
{
    __shared__ uint32_t key[N];
    __shared__ unsigned long long wbest[PEAKS_TB / 64];
    constexpr int LOG4 = N == 1024 ? 5 : N == 4096 ? 6 : 7;
    const int t = threadIdx.x;
    const float *row = rows + (size_t)blockIdx.x * N;
    unsigned long long best = 0;
    for (int v = t; v < N / 4; v += PEAKS_TB) {
        const float4 w = reinterpret_cast<const float4 *>(row)[v];
        const float we[4] = { w.x, w.y, w.z, w.w };
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int b = (int)survey_rev((uint32_t)(4 * v + e), LOG4);
            const uint32_t k = burst_key(we[e]);
            key[peaks_at<LOG4>(b)] = k;
            best = max(best, peaks_cand(k, b));
        }
    }
    int count = 0;
    for (;;) {
#pragma unroll
        for (int off = 32; off; off >>= 1) best = max(best, __shfl_xor(best, off));
        if ((t & 63) == 0) wbest[t >> 6] = best;
        __syncthreads();
        unsigned long long m = wbest[0];
#pragma unroll
        for (int k = 1; k < PEAKS_TB / 64; k++) m = max(m, wbest[k]);
        const uint32_t mk = (uint32_t)(m >> 32);
        const int b = (int)(0xffffffffu - (uint32_t)m);
        if (!mk || __uint_as_float(mk) < level) break;                     // (the same in every lane)
        if (t == 0) {
            BurstPeak p;
            p.bin = b;
            p.below = row[survey_rev((uint32_t)((b + N - 1) & (N - 1)), LOG4)];
            p.power = __uint_as_float(mk);
            p.above = row[survey_rev((uint32_t)((b + 1) & (N - 1)), LOG4)];
            peaks[(size_t)blockIdx.x * BURST_ROW_PEAKS + count] = p;
        }
        if (++count == BURST_ROW_PEAKS) break;
        for (int k = t; k <= 2 * gb; k += PEAKS_TB) key[peaks_at<LOG4>((b - gb + k + N) & (N - 1))] = 0;
        __syncthreads();                                                   // (also: every lane has read wbest)
        best = 0;
        for (int i = t; i < N; i += PEAKS_TB) best = max(best, peaks_cand(key[peaks_at<LOG4>(i)], i));
    }
    if (t == 0) counts[blockIdx.x] = count;
}

}  // namespace pdt

using namespace pdt;

namespace pdtrt {

// pdt_survey.hip
void survey_host_spectrum(int fmt, const void *x, const SurveyPlan &p, float *spectrum);
hipError_t spectra_launch(hipStream_t st, int fmt, const void *x, uint64_t nseg, int per_row, int per_group, int nfft, const float *win, const float *tw,
                          float *rows);

// the waterfall of nrows rows from x on (x: the first sample of the first of them): rows = nrows x nfft floats in place order, row t's
// place i = the sum of bin survey_rev(i) over its rows_per segments
hipError_t waterfall_launch(hipStream_t st, int fmt, const void *x, uint64_t nrows, int rows_per, int nfft, const float *win, const float *tw, float *rows)
{
    if (rows_per < 1 || rows_per > BURST_MAX_ROWS_PER) return hipErrorInvalidValue;
    return spectra_launch(st, fmt, x, nrows * (uint64_t)rows_per, rows_per, burst_rows_per_group(rows_per) * rows_per, nfft, win, tw, rows);
}

// k_row_peaks over nrows rows of a slab: peaks = nrows x BURST_ROW_PEAKS records, counts = nrows
hipError_t row_peaks_launch(hipStream_t st, const float *rows, uint64_t nrows, int nfft, float level, int gb, void *peaks, int *counts)
{
    if (!nrows || !survey_nfft(nfft) || gb < 0 || gb > nfft / 2) return hipErrorInvalidValue;
    const dim3 grid((unsigned)nrows), block(PEAKS_TB);
    switch (nfft) {
    case 1024: hipLaunchKernelGGL(k_row_peaks<1024>, grid, block, 0, st, rows, level, gb, (BurstPeak *)peaks, counts); break;
    case 4096: hipLaunchKernelGGL(k_row_peaks<4096>, grid, block, 0, st, rows, level, gb, (BurstPeak *)peaks, counts); break;
    default: hipLaunchKernelGGL(k_row_peaks<16384>, grid, block, 0, st, rows, level, gb, (BurstPeak *)peaks, counts); break;
    }
    return hipGetLastError();
}

// cfg (NULL = all defaults) with its defaults filled in, checked against a capture of nframes frames at in_rate
int bursts_plan(const pdt_bursts_cfg *cfg, double mode_range_hz, double channel_rate, double in_rate, uint64_t nframes, int cap, BurstPlan *p)
{
    pdt_bursts_cfg c;
    memset(&c, 0, sizeof c);
    if (cfg) c = *cfg;
    p->nfft = c.nfft ? c.nfft : BURST_DEFAULT_NFFT;
    p->rows_per = c.rows_per ? c.rows_per : BURST_DEFAULT_ROWS_PER;
    p->gap_rows = c.gap_rows ? c.gap_rows : BURST_DEFAULT_GAP_ROWS;
    p->threshold_db = c.threshold_db != 0 ? c.threshold_db : SURVEY_DEFAULT_THRESHOLD_DB;
    p->guard_hz = c.guard_hz != 0 ? c.guard_hz : 0.5 * channel_rate;
    p->merge_hz = c.merge_hz != 0 ? c.merge_hz : mode_range_hz;
    if (!survey_nfft(p->nfft) || p->rows_per < 1 || p->rows_per > BURST_MAX_ROWS_PER || p->gap_rows < 0 || cap < 1) return PDT_ERR_ARG;
    p->min_s = c.min_s != 0 ? c.min_s : 2.0 * (double)p->rows_per * (double)p->nfft / in_rate;
    p->max_s = c.max_s;
    if (!(std::isfinite(p->threshold_db) && std::isfinite(p->guard_hz) && std::isfinite(p->merge_hz) && std::isfinite(p->min_s) && std::isfinite(p->max_s)) ||
        p->guard_hz < 0 || p->merge_hz < 0 || p->min_s < 0 || p->max_s < 0)
        return PDT_ERR_ARG;
    if (c.first_frame > nframes || c.nframes > nframes - c.first_frame) return PDT_ERR_ARG;
    p->first = c.first_frame;
    p->nrows = (c.nframes ? c.nframes : nframes - c.first_frame) / ((uint64_t)p->nfft * (uint64_t)p->rows_per);
    return p->nrows ? PDT_OK : PDT_ERR_ARG;
}

// the survey the floor comes from: the same stretch at the same N, every whole segment of it
SurveyPlan bursts_survey_plan(const BurstPlan &p, const pdt_bursts_cfg *cfg, uint64_t nframes)
{
    SurveyPlan s;
    memset(&s, 0, sizeof s);
    s.nfft = p.nfft;
    s.first = p.first;
    s.nseg = (cfg && cfg->nframes ? cfg->nframes : nframes - p.first) / (uint64_t)p.nfft;
    return s;
}

// the host's share of a burst search: the rows' peaks linked into bursts; the first `cap` of them go to found[]
int bursts_link(const void *peaks, const int *counts, bool compact, const BurstPlan &p, double floor, double in_rate, pdt_burst *found, int cap)
{
    const std::vector<Burst> b = burst_link((const BurstPeak *)peaks, counts, compact, p, floor, in_rate);
    const size_t n = std::min<size_t>(b.size(), (size_t)std::max(cap, 0));
    if (n) memcpy(found, b.data(), n * sizeof(Burst));
    return (int)std::min<size_t>(b.size(), (size_t)INT32_MAX);
}

}  // namespace pdtrt

extern "C" int pdt_host_bursts(uint32_t in_rate, double mode_range_hz, uint32_t channel_rate, int sample_format, const void *x, uint64_t nframes,
                               const pdt_bursts_cfg *cfg, float *rows_out, pdt_row_peak *peaks_out, int *peak_counts_out, pdt_burst *found, int cap,
                               int *count)
{
    if (in_rate == 0 || channel_rate == 0 || !(std::isfinite(mode_range_hz) && mode_range_hz > 0) || !ddc_fmt(sample_format) || !x || !found || !count)
        return PDT_ERR_ARG;
    BurstPlan p;
    const int rc = pdtrt::bursts_plan(cfg, mode_range_hz, (double)channel_rate, (double)in_rate, nframes, cap, &p);
    if (rc) return rc;
    std::vector<float> P((size_t)p.nfft);
    pdtrt::survey_host_spectrum(sample_format, x, pdtrt::bursts_survey_plan(p, cfg, nframes), P.data());
    const double floor = survey_floor(P.data(), p.nfft);
    const float level = burst_level(floor, p.threshold_db, p.rows_per);
    const int gb = burst_guard_bins(p.guard_hz, (double)in_rate, p.nfft);
    std::vector<BurstPeak> peaks((size_t)p.nrows * BURST_ROW_PEAKS);
    std::vector<int> counts((size_t)p.nrows);
    std::vector<float> row((size_t)p.nfft), sum((size_t)p.nfft);
    std::vector<SurveyC> v((size_t)p.nfft);
    const std::vector<float> win = survey_window(p.nfft), tw = survey_twiddles(p.nfft);
    const int log4 = survey_log4(p.nfft);
    const uint64_t row_frames = (uint64_t)p.rows_per * (uint64_t)p.nfft;
    for (uint64_t t = 0; t < p.nrows; t++) {
        float *dst = rows_out ? rows_out + (size_t)t * (size_t)p.nfft : row.data();
        survey_host_sum(sample_format, x, (long long)(p.first + t * row_frames), p.rows_per, win, tw, v, sum.data());
        for (int i = 0; i < p.nfft; i++) dst[survey_rev((uint32_t)i, log4)] = sum[(size_t)i];        // natural bin order
        counts[(size_t)t] = burst_row_peaks(dst, p.nfft, level, gb, &peaks[(size_t)t * BURST_ROW_PEAKS]);
    }
    if (peaks_out) memcpy(peaks_out, peaks.data(), peaks.size() * sizeof(BurstPeak));
    if (peak_counts_out) memcpy(peak_counts_out, counts.data(), counts.size() * sizeof(int));
    *count = pdtrt::bursts_link(peaks.data(), counts.data(), false, p, floor, (double)in_rate, found, cap);
    return PDT_OK;
}

extern "C" int pdt_burst_carriers(const pdt_burst *bursts, int count, double merge_hz, pdt_carrier *carriers, int cap, int *n)
{
    if (count < 0 || (count && !bursts) || !(std::isfinite(merge_hz) && merge_hz >= 0) || !carriers || cap < 1 || !n) return PDT_ERR_ARG;
    const std::vector<SurveyCarrier> c = burst_carriers(reinterpret_cast<const Burst *>(bursts), count, merge_hz);
    *n = (int)c.size();
    memcpy(carriers, c.data(), std::min<size_t>(c.size(), (size_t)cap) * sizeof(SurveyCarrier));
    return PDT_OK;
}

// llround of a time in frames, kept inside what a frame index holds
static long long window_frame(double frames)
{
    return !(frames > 0.0) ? 0LL : frames >= 9.0e18 ? (long long)9.0e18 : llround(frames);
}

// window i of burst i: from skip_s behind the burst's start to tail_s behind its end, cut at the capture's end
extern "C" int pdt_burst_windows(const pdt_burst *bursts, int count, uint32_t in_rate, uint64_t capture_frames, double skip_s, double tail_s,
                                 pdt_window *out)
{
    if (count < 0 || (count && (!bursts || !out)) || in_rate == 0 || !std::isfinite(skip_s) || !std::isfinite(tail_s)) return PDT_ERR_ARG;
    for (int i = 0; i < count; i++)
        if (!(std::isfinite(bursts[i].start_s) && std::isfinite(bursts[i].duration_s) && std::isfinite(bursts[i].offset_hz))) return PDT_ERR_ARG;
    const double rate = (double)in_rate;
    for (int i = 0; i < count; i++) {
        const pdt_burst &b = bursts[i];
        const double skip = skip_s < 0 ? (b.rows ? b.duration_s / (double)b.rows : 0.0) : skip_s;       // the default: one row of the burst
        const double tail = tail_s < 0 ? 0.1 : tail_s;
        const long long first = window_frame((b.start_s + skip) * rate);
        const long long end = std::min<long long>((long long)std::min<uint64_t>(capture_frames, (uint64_t)INT64_MAX),
                                                  window_frame((b.start_s + b.duration_s + tail) * rate));
        out[i].first_frame = (uint64_t)first;
        out[i].nframes = end > first ? (uint64_t)(end - first) : 0;
        out[i].offset_hz = b.offset_hz;
    }
    return PDT_OK;
}
