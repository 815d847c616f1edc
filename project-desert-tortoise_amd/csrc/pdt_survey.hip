// pdt_survey.hip -- the carrier survey of wideband captures (pdt_survey.h): one kernel per input format and NFFT that reads runs of
// segments once, windows and transforms each in LDS and leaves every run's power sums as one row -- the survey's partial rows and,
// with the run length given at launch, the rows of the burst search's waterfall (pdt_bursts.hip) --, a small kernel that adds the
// survey's rows in their fixed order, and the host restatement pdt_host_survey.  A unit of its own: the chain's units do not change.
#include <math.h>
#include <string.h>
#include <algorithm>

#include "../../include/pdt.h"
#include "pdt_survey.h"

static_assert(sizeof(pdt_carrier) == sizeof(pdt::SurveyCarrier) && sizeof(pdt_carrier) == 16, "pdt_carrier");

namespace pdt {

// x: the first sample of segment 0 of this launch; nseg whole segments of N samples follow it.  A workgroup takes per_group consecutive
// segments (per_group a multiple of per_row) and leaves one row of N floats per per_row of them, row r's place i = the sum of bin
// survey_rev(i) over the segments r per_row .. r per_row + per_row - 1; the launch's last row is short when nseg is no multiple of
// per_row.  The survey: per_row = per_group = SURVEY_RUN, the rows are its partial rows.  The waterfall: per_row = R, nseg = rows R
// (pdt_bursts.hip).  One flat loop over the workgroup's segments: the sixteen sums leave and start again at 0 whenever a row is
// complete -- a row loop around a segment loop costs the registers of a second loop state, scratch at N = 16384.
template <int FMT, int N>
__global__ void __launch_bounds__(N / 16) k_spectra(const void *__restrict__ x, long long nseg, int per_row, int per_group, const float *__restrict__ win,
                                                    const float *__restrict__ tw, float *__restrict__ rows)
{
    __shared__ __attribute__((aligned(16))) float2 sv[N];
    constexpr int TB = N / 16;
    const int t = threadIdx.x;
    const long long s0 = (long long)blockIdx.x * per_group, s1 = min(s0 + per_group, nseg);
    float *row = rows + (size_t)(s0 / per_row) * N;
    int left = per_row;
    float acc[4][4];
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int m = 0; m < 4; m++) acc[k][m] = 0.0f;
    for (long long s = s0; s < s1; s++) {
        survey_segment<FMT, N>(sv, x, s, win, tw, t, acc);
        if (--left && s + 1 < s1) continue;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            *reinterpret_cast<float4 *>(row + 4 * (t + TB * k)) = make_float4(acc[k][0], acc[k][1], acc[k][2], acc[k][3]);
#pragma unroll
            for (int m = 0; m < 4; m++) acc[k][m] = 0.0f;
        }
        row += N;
        left = per_row;
    }
}

// P[rev(i)] = (the rows' place i added in ascending order, in double) / nseg
__global__ void __launch_bounds__(256) k_survey_sum(const float *__restrict__ part, int nruns, long long nseg, int n, int log4, float *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int r = 0; r < nruns; r++) s = s + (double)part[(size_t)r * n + i];
    out[survey_rev((uint32_t)i, log4)] = (float)(s / (double)nseg);
}

}  // namespace pdt

using namespace pdt;

namespace pdtrt {

// floats of the partial rows a survey of nseg segments needs
size_t survey_part_floats(uint64_t nseg, int nfft)
{
    return (size_t)((nseg + SURVEY_RUN - 1) / SURVEY_RUN) * (size_t)nfft;
}

// k_spectra over nseg whole segments from x on: rows = ceil(nseg / per_row) x nfft floats in place order (all pointers on the device).
// The one dispatch over format and NFFT.
hipError_t spectra_launch(hipStream_t st, int fmt, const void *x, uint64_t nseg, int per_row, int per_group, int nfft, const float *win, const float *tw,
                          float *rows)
{
    if (!nseg || !survey_nfft(nfft) || !ddc_fmt(fmt) || per_row < 1 || per_group < per_row || per_group % per_row) return hipErrorInvalidValue;
    const unsigned groups = (unsigned)((nseg + (uint64_t)per_group - 1) / (uint64_t)per_group);
#define PDT_SPECTRA_GO(F, N) hipLaunchKernelGGL((k_spectra<F, N>), dim3(groups), dim3(N / 16), 0, st, x, (long long)nseg, per_row, per_group, win, tw, rows)
#define PDT_SPECTRA_FMT(F)                                  \
    switch (nfft) {                                         \
    case 1024: PDT_SPECTRA_GO(F, 1024); break;              \
    case 4096: PDT_SPECTRA_GO(F, 4096); break;              \
    default: PDT_SPECTRA_GO(F, 16384); break;               \
    }
    switch (fmt) {
    case PDT_FMT_WB_PCM16: PDT_SPECTRA_FMT(PDT_FMT_WB_PCM16); break;
    case PDT_FMT_WB_F32: PDT_SPECTRA_FMT(PDT_FMT_WB_F32); break;
    case PDT_FMT_WB_CU8: PDT_SPECTRA_FMT(PDT_FMT_WB_CU8); break;
    default: PDT_SPECTRA_FMT(PDT_FMT_WB_CS8); break;
    }
#undef PDT_SPECTRA_FMT
#undef PDT_SPECTRA_GO
    return hipGetLastError();
}

// the survey over nseg whole segments from x on: the runs' partial rows, then their sum; out = the averaged spectrum, nfft floats
hipError_t survey_launch(hipStream_t st, int fmt, const void *x, uint64_t nseg, int nfft, const float *win, const float *tw, float *part, float *out)
{
    const hipError_t e = spectra_launch(st, fmt, x, nseg, SURVEY_RUN, SURVEY_RUN, nfft, win, tw, part);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_survey_sum, dim3((unsigned)(nfft / 256)), dim3(256), 0, st, (const float *)part, (int)((nseg + SURVEY_RUN - 1) / SURVEY_RUN),
                       (long long)nseg, nfft, survey_log4(nfft), out);
    return hipGetLastError();
}

// cfg (NULL = all defaults) with its defaults filled in, checked against a capture of nframes frames
int survey_plan(const pdt_survey_cfg *cfg, double mode_range_hz, double channel_rate, uint64_t nframes, int cap, SurveyPlan *p)
{
    pdt_survey_cfg c;
    memset(&c, 0, sizeof c);
    if (cfg) c = *cfg;
    p->nfft = c.nfft ? c.nfft : SURVEY_DEFAULT_NFFT;
    p->max_carriers = c.max_carriers ? c.max_carriers : SURVEY_MAX_CARRIERS;
    p->threshold_db = c.threshold_db != 0 ? c.threshold_db : SURVEY_DEFAULT_THRESHOLD_DB;
    p->guard_hz = c.guard_hz != 0 ? c.guard_hz : 0.5 * channel_rate;
    p->merge_hz = c.merge_hz != 0 ? c.merge_hz : mode_range_hz;
    if (!survey_nfft(p->nfft) || p->max_carriers < 0 || cap < 1) return PDT_ERR_ARG;
    if (!(std::isfinite(p->threshold_db) && std::isfinite(p->guard_hz) && std::isfinite(p->merge_hz)) || p->guard_hz < 0 || p->merge_hz < 0) return PDT_ERR_ARG;
    if (c.first_frame > nframes || c.nframes > nframes - c.first_frame) return PDT_ERR_ARG;
    p->max_carriers = std::min(p->max_carriers, cap);
    p->first = c.first_frame;
    p->nseg = (c.nframes ? c.nframes : nframes - c.first_frame) / (uint64_t)p->nfft;
    return p->nseg ? PDT_OK : PDT_ERR_ARG;
}

// the host's share of a survey: the carriers of the averaged spectrum P
int survey_carriers(const float *P, const SurveyPlan &p, double in_rate, pdt_carrier *found)
{
    return survey_detect(P, p.nfft, in_rate, p.threshold_db, p.guard_hz, p.merge_hz, p.max_carriers, reinterpret_cast<SurveyCarrier *>(found));
}

// the averaged spectrum of the plan's stretch as the kernels leave it, on the host (pdt_host_survey, pdt_host_bursts)
void survey_host_spectrum(int fmt, const void *x, const SurveyPlan &p, float *spectrum)
{
    const int N = p.nfft, log4 = survey_log4(N);
    const std::vector<float> win = survey_window(N), tw = survey_twiddles(N);
    std::vector<SurveyC> v((size_t)N);
    std::vector<float> run((size_t)N);
    std::vector<double> total((size_t)N, 0.0);
    for (uint64_t s0 = 0; s0 < p.nseg; s0 += SURVEY_RUN) {
        survey_host_sum(fmt, x, (long long)(p.first + s0 * (uint64_t)N), (int)std::min<uint64_t>(SURVEY_RUN, p.nseg - s0), win, tw, v, run.data());
        for (int i = 0; i < N; i++) total[(size_t)i] = total[(size_t)i] + (double)run[(size_t)i];
    }
    for (int i = 0; i < N; i++) spectrum[survey_rev((uint32_t)i, log4)] = (float)(total[(size_t)i] / (double)p.nseg);
}

}  // namespace pdtrt

extern "C" int pdt_host_survey(uint32_t in_rate, double mode_range_hz, uint32_t channel_rate, int sample_format, const void *x, uint64_t nframes,
                               const pdt_survey_cfg *cfg, float *spectrum_out, pdt_carrier *found, int cap, int *count)
{
    if (in_rate == 0 || channel_rate == 0 || !(std::isfinite(mode_range_hz) && mode_range_hz > 0) || !ddc_fmt(sample_format) || !x || !found || !count)
        return PDT_ERR_ARG;
    SurveyPlan p;
    const int rc = pdtrt::survey_plan(cfg, mode_range_hz, (double)channel_rate, nframes, cap, &p);
    if (rc) return rc;
    std::vector<float> P((size_t)p.nfft);
    pdtrt::survey_host_spectrum(sample_format, x, p, P.data());
    if (spectrum_out) memcpy(spectrum_out, P.data(), P.size() * sizeof(float));
    *count = pdtrt::survey_carriers(P.data(), p, (double)in_rate, found);
    return PDT_OK;
}
