// pdt_tone.hip -- the carrier measurement of channel streams (pdt_tone.h): one kernel per NFFT that transforms a segment with the
// survey's own device function, finds the strongest bin of the search set and leaves the raw record of its neighbourhood, the plan
// of a call, and the host restatement pdt_host_tones.  A unit of its own, beside pdt_survey.hip and pdt_bursts.hip.
#include <math.h>
#include <string.h>
#include <algorithm>

#include "../../include/pdt.h"
#include "pdt_tone.h"

static_assert(sizeof(pdt_tone) == sizeof(pdt::Tone) && sizeof(pdt_tone) == 72, "pdt_tone");
static_assert(sizeof(pdt::ToneRaw) == 32 && sizeof(pdt::ToneSeg) == 24, "tone records");

namespace pdt {

// One workgroup of N / 16 lanes per segment of the launch's table.  survey_segment leaves the segment's powers in the lanes' sixteen
// sums (from 0: the powers themselves), place 4 (t + k N / 16) + m, and the LDS image free: the powers go into its first half in place
// order (16-byte stores), while every lane forms the candidates of its own sixteen bins -- bin = survey_rev(place) -- that lie in the
// search set.  The candidates are reduced over the wavefront by shuffles and over the wavefronts through a few words of LDS, as in
// k_row_peaks; every lane reads the winner.  The lanes then gather the noise bins, in the order of the sum, into the image's second half
// (at most N - 2 of them), and lane 0 adds them, reads the neighbours and stores the record.  No atomics; nothing depends on the order in
// which anything runs.
template <int N>
__global__ void __launch_bounds__(N / 16) k_tones(const ToneSeg *__restrict__ segs, int lo, int hi, const float *__restrict__ win,
                                                  const float *__restrict__ tw, ToneRaw *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) float2 sv[N];
    __shared__ unsigned long long wbest[(N / 16 + 63) / 64];
    constexpr int TB = N / 16, LOG4 = N == 1024 ? 5 : N == 4096 ? 6 : 7, NW = (TB + 63) / 64;
    const int t = threadIdx.x;
    const ToneSeg s = segs[blockIdx.x];
    float acc[4][4];
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int m = 0; m < 4; m++) acc[k][m] = 0.0f;
    survey_segment<PDT_FMT_WB_F32, N>(sv, reinterpret_cast<const unsigned char *>(s.x) + s.first * 8, 0, win, tw, t, acc);
    float *pw = reinterpret_cast<float *>(sv), *nz = pw + N;
    unsigned long long best = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int i0 = 4 * (t + TB * k);
        *reinterpret_cast<float4 *>(pw + i0) = make_float4(acc[k][0], acc[k][1], acc[k][2], acc[k][3]);
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const int b = (int)survey_rev((uint32_t)(i0 + m), LOG4);
            if (tone_in_search(b, s.kmax, N)) best = max(best, tone_cand(burst_key(acc[k][m]), b));
        }
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) best = max(best, __shfl_xor(best, off));
    if ((t & 63) == 0) wbest[t >> 6] = best;
    __syncthreads();                                                       // (also: the powers are in LDS)
    unsigned long long w = wbest[0];
#pragma unroll
    for (int k = 1; k < NW; k++) w = max(w, wbest[k]);
    const int bin = (int)(0xffffffffu - (uint32_t)w);                      // (bin 0 is in every search set: there is a winner)
    const int nb = 2 * (hi - lo + 1);
    for (int i = t; i < nb; i += TB) nz[i] = pw[survey_rev((uint32_t)tone_noise_bin(bin, i, lo, hi, N), LOG4)];
    __syncthreads();
    if (t == 0) {
        float sum = 0.0f;
        for (int i = 0; i < nb; i++) sum = sum + nz[i];
        const float below = pw[survey_rev((uint32_t)((bin + N - 1) & (N - 1)), LOG4)], peak = pw[survey_rev((uint32_t)bin, LOG4)];
        const float above = pw[survey_rev((uint32_t)((bin + 1) & (N - 1)), LOG4)];
        int4 *dst = reinterpret_cast<int4 *>(out + s.rec);
        dst[0] = make_int4(bin, __float_as_int(below), __float_as_int(peak), __float_as_int(above));
        dst[1] = make_int4(__float_as_int(sum), nb, 0, 0);
    }
}

}  // namespace pdt

using namespace pdt;

namespace pdtrt {

// k_tones over the nsegs segments of a table that is on the device; win and tw: the survey's tables of nfft points
hipError_t tones_launch(hipStream_t st, int nfft, const void *segs_dev, uint64_t nsegs, int lo, int hi, const float *win, const float *tw, void *out)
{
    if (!nsegs) return hipSuccess;
    if (!survey_nfft(nfft) || nsegs > 0x7fffffffull || lo < 1 || hi < lo || hi >= nfft / 2) return hipErrorInvalidValue;
    const dim3 grid((unsigned)nsegs);
    const ToneSeg *segs = (const ToneSeg *)segs_dev;
    switch (nfft) {
    case 1024: hipLaunchKernelGGL(k_tones<1024>, grid, dim3(64), 0, st, segs, lo, hi, win, tw, (ToneRaw *)out); break;
    case 4096: hipLaunchKernelGGL(k_tones<4096>, grid, dim3(256), 0, st, segs, lo, hi, win, tw, (ToneRaw *)out); break;
    default: hipLaunchKernelGGL(k_tones<16384>, grid, dim3(1024), 0, st, segs, lo, hi, win, tw, (ToneRaw *)out); break;
    }
    return hipGetLastError();
}

// cfg (NULL = all defaults) with its defaults filled in, for a stream of `len` samples at fs.  range_hz: the default of search_hz
// (a context: its mode's PLL range; negative: the widest set, the hook's).
int tone_plan(const pdt_tone_cfg *cfg, double fs, double range_hz, uint64_t len, int cap, TonePlan *p)
{
    pdt_tone_cfg c;
    memset(&c, 0, sizeof c);
    if (cfg) c = *cfg;
    if (!(fs > 0) || cap < 1) return PDT_ERR_ARG;
    p->nfft = c.nfft ? c.nfft : tone_default_nfft(fs);
    if (!survey_nfft(p->nfft)) return PDT_ERR_ARG;
    p->noise_lo = c.noise_lo ? c.noise_lo : TONE_NOISE_LO;
    p->noise_hi = c.noise_hi ? c.noise_hi : TONE_NOISE_HI;
    if (p->noise_lo < 1 || p->noise_lo > p->noise_hi || p->noise_hi >= p->nfft / 2) return PDT_ERR_ARG;
    const double search = c.search_hz != 0 ? c.search_hz : range_hz < 0 ? 0.5 * fs * (1.0 - 1.0 / (double)p->nfft) : range_hz;
    if (!(std::isfinite(search) && search >= 0 && search < 0.5 * fs)) return PDT_ERR_ARG;
    p->kmax = tone_kmax(search, fs, p->nfft);
    p->first = c.first;
    p->stride = c.stride ? c.stride : (uint64_t)p->nfft;
    const uint64_t N = (uint64_t)p->nfft;
    const uint64_t avail = (c.first <= len && len - c.first >= N) ? (len - c.first - N) / p->stride + 1 : 0;
    p->nseg = std::min<uint64_t>(std::min(c.count ? c.count : avail, avail), (uint64_t)cap);
    return PDT_OK;
}

// the sums over the window of nfft points that the derived values need (tone_window_sums)
void tone_sums(int nfft, double *sw, double *sw2)
{
    tone_window_sums(survey_window(nfft), *sw, *sw2);
}

// raw records -> pdt_tone, segment i of the plan at offset_hz; sw, sw2: tone_sums of the plan's nfft
void tones_derive(const void *raw, const TonePlan &p, double fs, double offset_hz, double sw, double sw2, pdt_tone *out)
{
    const ToneRaw *r = (const ToneRaw *)raw;
    for (uint64_t i = 0; i < p.nseg; i++) {
        const Tone t = tone_derive(r[i], p.nfft, fs, offset_hz, p.first + i * p.stride, sw, sw2);
        memcpy(&out[i], &t, sizeof t);
    }
}

}  // namespace pdtrt

extern "C" int pdt_host_tones(uint32_t rate, double offset_hz, const float *iq, uint64_t n, const pdt_tone_cfg *cfg, pdt_tone *out, int cap, int *count)
{
    if (rate == 0 || !std::isfinite(offset_hz) || (!iq && n) || !out || !count) return PDT_ERR_ARG;
    TonePlan p;
    const int rc = pdtrt::tone_plan(cfg, (double)rate, -1.0, n, cap, &p);
    if (rc) return rc;
    const std::vector<float> win = survey_window(p.nfft), tw = survey_twiddles(p.nfft);
    std::vector<SurveyC> v((size_t)p.nfft);
    std::vector<ToneRaw> raw((size_t)p.nseg);
    for (uint64_t i = 0; i < p.nseg; i++)
        raw[(size_t)i] = tone_host_raw(iq, (long long)(p.first + i * p.stride), p.kmax, p.noise_lo, p.noise_hi, win, tw, v);
    double sw, sw2;
    tone_window_sums(win, sw, sw2);
    pdtrt::tones_derive(raw.data(), p, (double)rate, offset_hz, sw, sw2, out);
    *count = (int)p.nseg;
    return PDT_OK;
}
