// pdt_survey.hip -- the carrier survey of wideband captures (pdt_survey.h): one kernel per input format and NFFT that reads a run of
// segments once, windows and transforms each in LDS and leaves the run's power sums as one partial row, a small kernel that adds
// the rows in their fixed order, and the host restatement pdt_host_survey.  A unit of its own: the chain's units do not change.
#include <math.h>
#include <string.h>
#include <algorithm>

#include "../../include/pdt.h"
#include "pdt_survey.h"

static_assert(sizeof(pdt_carrier) == sizeof(pdt::SurveyCarrier) && sizeof(pdt_carrier) == 16, "pdt_carrier");

namespace pdt {

// x: the stretch's first sample; nseg whole segments of N samples follow it.  part: ceil(nseg / SURVEY_RUN) rows of N floats.
template <int FMT, int N>
__global__ void __launch_bounds__(N / 16) k_survey(const void *__restrict__ x, long long nseg, const float *__restrict__ win,
                                                   const float *__restrict__ tw, float *__restrict__ part)
{
    __shared__ __attribute__((aligned(16))) float2 sv[N];
    constexpr int TB = N / 16;
    const int t = threadIdx.x;
    const long long s0 = (long long)blockIdx.x * SURVEY_RUN;
    const int ns = (int)min((long long)SURVEY_RUN, nseg - s0);
    float acc[4][4];
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int m = 0; m < 4; m++) acc[k][m] = 0.0f;
    for (int s = 0; s < ns; s++) survey_segment<FMT, N>(sv, x, s0 + s, win, tw, t, acc);
    float *row = part + (size_t)blockIdx.x * N;
#pragma unroll
    for (int k = 0; k < 4; k++)
        *reinterpret_cast<float4 *>(row + 4 * (t + TB * k)) = make_float4(acc[k][0], acc[k][1], acc[k][2], acc[k][3]);
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

// the two kernels over nseg whole segments from x on: out = the averaged spectrum, nfft floats (all pointers on the device)
hipError_t survey_launch(hipStream_t st, int fmt, const void *x, uint64_t nseg, int nfft, const float *win, const float *tw, float *part, float *out)
{
    if (!nseg || !survey_nfft(nfft) || !ddc_fmt(fmt)) return hipErrorInvalidValue;
    const unsigned nruns = (unsigned)((nseg + SURVEY_RUN - 1) / SURVEY_RUN);
#define PDT_SURVEY_GO(F, N) hipLaunchKernelGGL((k_survey<F, N>), dim3(nruns), dim3(N / 16), 0, st, x, (long long)nseg, win, tw, part)
#define PDT_SURVEY_FMT(F)                                   \
    switch (nfft) {                                         \
    case 1024: PDT_SURVEY_GO(F, 1024); break;               \
    case 4096: PDT_SURVEY_GO(F, 4096); break;               \
    default: PDT_SURVEY_GO(F, 16384); break;                \
    }
    switch (fmt) {
    case PDT_FMT_WB_PCM16: PDT_SURVEY_FMT(PDT_FMT_WB_PCM16); break;
    case PDT_FMT_WB_F32: PDT_SURVEY_FMT(PDT_FMT_WB_F32); break;
    case PDT_FMT_WB_CU8: PDT_SURVEY_FMT(PDT_FMT_WB_CU8); break;
    default: PDT_SURVEY_FMT(PDT_FMT_WB_CS8); break;
    }
#undef PDT_SURVEY_FMT
#undef PDT_SURVEY_GO
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_survey_sum, dim3((unsigned)(nfft / 256)), dim3(256), 0, st, (const float *)part, (int)nruns, (long long)nseg, nfft,
                       survey_log4(nfft), out);
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
void survey_host_spectrum(int fmt, const void *x, const SurveyPlan &p, float *spectrum);

int survey_carriers(const float *P, const SurveyPlan &p, double in_rate, pdt_carrier *found)
{
    return survey_detect(P, p.nfft, in_rate, p.threshold_db, p.guard_hz, p.merge_hz, p.max_carriers, reinterpret_cast<SurveyCarrier *>(found));
}

}  // namespace pdtrt

template <int FMT> static void host_survey(const void *x, const SurveyPlan &p, float *spectrum)
{
    const int N = p.nfft, log4 = survey_log4(N);
    const std::vector<float> win = survey_window(N), tw = survey_twiddles(N);
    std::vector<SurveyC> v((size_t)N);
    std::vector<float> run((size_t)N);
    std::vector<double> total((size_t)N, 0.0);
    for (uint64_t s0 = 0; s0 < p.nseg; s0 += SURVEY_RUN) {
        std::fill(run.begin(), run.end(), 0.0f);
        for (uint64_t s = s0; s < std::min<uint64_t>(s0 + SURVEY_RUN, p.nseg); s++) {
            survey_host_segment<FMT>(x, (long long)(p.first + s * (uint64_t)N), win, tw, v);
            for (int i = 0; i < N; i++) run[(size_t)i] = run[(size_t)i] + survey_power(v[(size_t)i]);
        }
        for (int i = 0; i < N; i++) total[(size_t)i] = total[(size_t)i] + (double)run[(size_t)i];
    }
    for (int i = 0; i < N; i++) spectrum[survey_rev((uint32_t)i, log4)] = (float)(total[(size_t)i] / (double)p.nseg);
}

// the averaged spectrum of the plan's stretch as the kernels leave it, on the host (pdt_host_survey, pdt_host_bursts)
void pdtrt::survey_host_spectrum(int fmt, const void *x, const SurveyPlan &p, float *spectrum)
{
    switch (fmt) {
    case PDT_FMT_WB_PCM16: host_survey<PDT_FMT_WB_PCM16>(x, p, spectrum); break;
    case PDT_FMT_WB_F32: host_survey<PDT_FMT_WB_F32>(x, p, spectrum); break;
    case PDT_FMT_WB_CU8: host_survey<PDT_FMT_WB_CU8>(x, p, spectrum); break;
    default: host_survey<PDT_FMT_WB_CS8>(x, p, spectrum); break;
    }
}

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
