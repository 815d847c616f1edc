// pdt_survey.h -- the carrier survey of wideband captures: the averaged power spectrum of a stretch of the capture and the carriers
// that stand out of it.  As for the down-converter (pdt_ddc.h) there is no reference to be bit-exact against, so the
// arithmetic is fixed here, once, for the kernels (pdt_survey.hip) and their host restatement (pdt_host_survey) alike:
//   x[n]    = the sample scaled by format, ddc_load<FMT> as it is
//   segment s = samples s N .. s N + N - 1 of the stretch, N = NFFT in {1024, 4096, 16384}; a last incomplete segment is dropped
//   w[n]    = 0.42 - 0.5 cos(2 pi n / (N - 1)) + 0.08 cos(4 pi n / (N - 1)), in double with cos_glibc, rounded to float
//   v[n]    = (xr w[n], xi w[n])
//   X       = the forward DFT of v by log4 N in-place radix-4 decimation-in-frequency passes, span L = N, N / 4, .., 4, q = L / 4:
//             for every block base (a multiple of L) and j < q, (a, b, c, d) = v[base + j + {0, q, 2 q, 3 q}] become
//               t0 = a + c, t1 = a - c, t2 = b + d, t3 = b - d,
//               y0 = t0 + t2, y1 = (t1 - i t3) W^(j N / L), y2 = (t0 - t2) W^(2 j N / L), y3 = (t1 + i t3) W^(3 j N / L)
//             in the same four places; y W^k = (yr c + yi s, yi c - yr s) with (c, s) = tw[k] = (cos, sin)(2 pi k / N) in double from
//             cos_glibc / sin_glibc, rounded to float, every product rounded first; the last pass (L = 4) multiplies by no twiddle.
//             Place i then holds bin survey_rev(i): i's base-4 digits reversed
//   p_s[b]  = re^2 + im^2, both products rounded first
//   P[b]    = the segments in runs of SURVEY_RUN consecutive ones, each run summed in float in ascending order from 0, the runs' sums
//             added in double in ascending order, divided by the number of segments in double, rounded to float
//   carriers: survey_detect below, on the host, over P
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "pdt_ddc.h"

namespace pdt {

constexpr int SURVEY_RUN = 64;                  // R: segments of a run (one workgroup, one partial row)
constexpr int SURVEY_MAX_CARRIERS = 16;         // the channels the host programs take (-t)
constexpr int SURVEY_DEFAULT_NFFT = 16384;
constexpr double SURVEY_DEFAULT_THRESHOLD_DB = 15.0;

inline bool survey_nfft(int n) { return n == 1024 || n == 4096 || n == 16384; }
inline int survey_log4(int n) { return n == 1024 ? 5 : n == 4096 ? 6 : 7; }

inline std::vector<float> survey_window(int n)
{
    std::vector<float> w((size_t)n);
    for (int i = 0; i < n; i++)
        w[(size_t)i] = (float)(0.42 - 0.5 * cos_glibc(2.0 * M_PI * (double)i / (double)(n - 1)) + 0.08 * cos_glibc(4.0 * M_PI * (double)i / (double)(n - 1)));
    return w;
}

// tw[2 k] = cos, tw[2 k + 1] = sin of 2 pi k / n, k < n
inline std::vector<float> survey_twiddles(int n)
{
    std::vector<float> t((size_t)(2 * n));
    for (int k = 0; k < n; k++) {
        const double a = 2.0 * M_PI * (double)k / (double)n;
        t[(size_t)(2 * k)] = (float)cos_glibc(a);
        t[(size_t)(2 * k + 1)] = (float)sin_glibc(a);
    }
    return t;
}

// the base-4 digits of i < 4^log4, reversed
__host__ __device__ __forceinline__ uint32_t survey_rev(uint32_t i, int log4)
{
    uint32_t r = 0;
    for (int d = 0; d < log4; d++) {
        r = (r << 2) | (i & 3u);
        i >>= 2;
    }
    return r;
}

struct SurveyC {
    float r, i;
};

// y (c - j s)
__host__ __device__ __forceinline__ SurveyC survey_twist(float yr, float yi, float c, float s)
{
    SurveyC o;
    o.r = yr * c + yi * s;
    o.i = yi * c - yr * s;
    return o;
}

// one radix-4 butterfly in place; w = tw[k], tw[2 k], tw[3 k] as (c, s) pairs; TW = false: the last pass, w is not read
template <bool TW>
__host__ __device__ __forceinline__ void survey_bfly(SurveyC &a, SurveyC &b, SurveyC &c, SurveyC &d, const float *w1, const float *w2, const float *w3)
{
    const float t0r = a.r + c.r, t0i = a.i + c.i, t1r = a.r - c.r, t1i = a.i - c.i;
    const float t2r = b.r + d.r, t2i = b.i + d.i, t3r = b.r - d.r, t3i = b.i - d.i;
    a.r = t0r + t2r;
    a.i = t0i + t2i;
    const float y1r = t1r + t3i, y1i = t1i - t3r;              // t1 - i t3
    const float y2r = t0r - t2r, y2i = t0i - t2i;
    const float y3r = t1r - t3i, y3i = t1i + t3r;              // t1 + i t3
    if (TW) {
        b = survey_twist(y1r, y1i, w1[0], w1[1]);
        c = survey_twist(y2r, y2i, w2[0], w2[1]);
        d = survey_twist(y3r, y3i, w3[0], w3[1]);
    } else {
        b.r = y1r; b.i = y1i;
        c.r = y2r; c.i = y2i;
        d.r = y3r; d.i = y3i;
    }
}

__host__ __device__ __forceinline__ float survey_power(const SurveyC &y)
{
    const float a = y.r * y.r, b = y.i * y.i;
    return a + b;
}

// One workgroup of N / 16 lanes takes a run of SURVEY_RUN segments.  A segment is converted and windowed on its way into LDS (16-byte
// loads from the first 16-byte boundary on), N float pairs: all of the 128 KiB at N = 16384.  Every pass gives each lane four
// butterflies, u = t + k N / 16: consecutive lanes take consecutive j, so for q >= 64 the 32 lanes of a half-wave read 32
// consecutive pairs, one 256-byte bank row.  In the passes with q = 16, 4 and 1 a half-wave's places are 32 apart in runs of q
// -- without more ado 2, 4 and 4 of them on every bank --, so place i is kept at survey_at(i): the low four bits of i exchanged by
// bits 5-6 (times 5: both bit pairs) and bit 4 by bit 6, a permutation inside each bank row that puts those places on 32 different
// bank pairs and leaves a row's consecutive places a row.  The last pass stays in registers: its four outputs' powers go to the
// lane's sixteen sums, which leave after the run as four 16-byte stores, in place order (k_survey_sum undoes the digit reversal).
__device__ __forceinline__ int survey_at(int i)
{
    return i ^ (((i >> 5) & 3) * 5) ^ (((i >> 6) & 1) << 4);
}

// One segment (number seg of the stretch that starts at x) by the whole workgroup of N / 16 lanes, t = threadIdx.x: converted,
// windowed, transformed in sv (N float pairs of LDS), its bins' powers added to the lane's sixteen sums.  Ends with a barrier: sv
// is free again.  The survey's runs and the waterfall's rows are sums over calls of this one function (k_spectra, pdt_survey.hip).
template <int FMT, int N>
__device__ __forceinline__ void survey_segment(float2 *sv, const void *__restrict__ x, long long seg, const float *__restrict__ win,
                                               const float *__restrict__ tw, int t, float (&acc)[4][4])
{
    constexpr int TB = N / 16, LOG4 = N == 1024 ? 5 : N == 4096 ? 6 : 7;
    constexpr int BPS = DdcFmt<FMT>::BPS, SPV = DdcFmt<FMT>::SPV;
    const long long first = seg * N;
    const unsigned char *src = reinterpret_cast<const unsigned char *>(x) + first * BPS;
    int head = (int)(((16 - ((uintptr_t)src & 15)) & 15) / BPS);      // samples in front of the first 16-byte boundary
    if (((uintptr_t)src & 15) % BPS) head = N;                         // (never aligned: sample by sample)
    const int nvec = (N - head) / SPV;
    for (int j = t; j < head; j += TB) {
        float re, im;
        ddc_load<FMT>(src, j, re, im);
        const float w = win[j];
        sv[survey_at(j)] = make_float2(re * w, im * w);
    }
    for (int v = t; v < nvec; v += TB) {
        const int4 raw = *reinterpret_cast<const int4 *>(src + (size_t)head * BPS + (size_t)v * 16);
#pragma unroll
        for (int e = 0; e < SPV; e++) {
            float re, im;
            ddc_load<FMT>(&raw, e, re, im);
            const int j = head + v * SPV + e;
            const float w = win[j];
            sv[survey_at(j)] = make_float2(re * w, im * w);
        }
    }
    for (int j = head + nvec * SPV + t; j < N; j += TB) {
        float re, im;
        ddc_load<FMT>(src, j, re, im);
        const float w = win[j];
        sv[survey_at(j)] = make_float2(re * w, im * w);
    }
    __syncthreads();
#pragma unroll
    for (int pass = 0; pass < LOG4 - 1; pass++) {
        const int q = N >> (2 * pass + 2), stride = 1 << (2 * pass);       // stride = N / L
#pragma unroll(N == 16384 ? 1 : 4)                                             // (16 wavefronts a workgroup: 128 registers a lane)
        for (int k = 0; k < 4; k++) {
            const int u = t + TB * k, j = u & (q - 1), i0 = ((u - j) << 2) + j;
            const int pa = survey_at(i0), pb = survey_at(i0 + q), pc = survey_at(i0 + 2 * q), pd = survey_at(i0 + 3 * q);
            const float2 fa = sv[pa], fb = sv[pb], fc = sv[pc], fd = sv[pd];
            SurveyC a = { fa.x, fa.y }, b = { fb.x, fb.y }, c = { fc.x, fc.y }, d = { fd.x, fd.y };
            const int k1 = j * stride;
            survey_bfly<true>(a, b, c, d, tw + 2 * k1, tw + 4 * k1, tw + 6 * k1);
            sv[pa] = make_float2(a.r, a.i);
            sv[pb] = make_float2(b.r, b.i);
            sv[pc] = make_float2(c.r, c.i);
            sv[pd] = make_float2(d.r, d.i);
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int i0 = 4 * (t + TB * k);
        const float2 fa = sv[survey_at(i0)], fb = sv[survey_at(i0 + 1)], fc = sv[survey_at(i0 + 2)], fd = sv[survey_at(i0 + 3)];
        SurveyC a = { fa.x, fa.y }, b = { fb.x, fb.y }, c = { fc.x, fc.y }, d = { fd.x, fd.y };
        survey_bfly<false>(a, b, c, d, nullptr, nullptr, nullptr);
        acc[k][0] = acc[k][0] + survey_power(a);
        acc[k][1] = acc[k][1] + survey_power(b);
        acc[k][2] = acc[k][2] + survey_power(c);
        acc[k][3] = acc[k][3] + survey_power(d);
    }
    __syncthreads();                                                   // (the next segment overwrites what this pass read)
}

// the same segment on the host: v[i] = place i of its transform (N = win.size() float pairs), first = its first sample's index in x
template <int FMT>
inline void survey_host_segment(const void *x, long long first, const std::vector<float> &win, const std::vector<float> &tw, std::vector<SurveyC> &v)
{
    const int N = (int)win.size(), log4 = survey_log4(N);
    for (int j = 0; j < N; j++) {
        float re, im;
        ddc_load<FMT>(x, first + j, re, im);
        v[(size_t)j].r = re * win[(size_t)j];
        v[(size_t)j].i = im * win[(size_t)j];
    }
    for (int pass = 0; pass < log4; pass++) {
        const int q = N >> (2 * pass + 2), stride = 1 << (2 * pass);
        for (int u = 0; u < N / 4; u++) {
            const int j = u & (q - 1), i0 = ((u - j) << 2) + j, k1 = j * stride;
            if (pass < log4 - 1)
                survey_bfly<true>(v[(size_t)i0], v[(size_t)(i0 + q)], v[(size_t)(i0 + 2 * q)], v[(size_t)(i0 + 3 * q)], &tw[(size_t)(2 * k1)],
                                  &tw[(size_t)(4 * k1)], &tw[(size_t)(6 * k1)]);
            else
                survey_bfly<false>(v[(size_t)i0], v[(size_t)(i0 + 1)], v[(size_t)(i0 + 2)], v[(size_t)(i0 + 3)], nullptr, nullptr, nullptr);
        }
    }
}

// The sum of `count` consecutive segments on the host, the first of which begins at sample `first` of x: sum[i] = their powers at
// place i, added in float in ascending order from 0 -- a run of the survey, a row of the waterfall (v: room for N = win.size() values)
template <int FMT>
inline void survey_host_sum_of(const void *x, long long first, int count, const std::vector<float> &win, const std::vector<float> &tw,
                               std::vector<SurveyC> &v, float *sum)
{
    const int N = (int)win.size();
    std::fill(sum, sum + N, 0.0f);
    for (int s = 0; s < count; s++) {
        survey_host_segment<FMT>(x, first + (long long)s * N, win, tw, v);
        for (int i = 0; i < N; i++) sum[i] = sum[i] + survey_power(v[(size_t)i]);
    }
}

inline void survey_host_sum(int fmt, const void *x, long long first, int count, const std::vector<float> &win, const std::vector<float> &tw,
                            std::vector<SurveyC> &v, float *sum)
{
    switch (fmt) {
    case PDT_FMT_WB_PCM16: survey_host_sum_of<PDT_FMT_WB_PCM16>(x, first, count, win, tw, v, sum); break;
    case PDT_FMT_WB_F32: survey_host_sum_of<PDT_FMT_WB_F32>(x, first, count, win, tw, v, sum); break;
    case PDT_FMT_WB_CU8: survey_host_sum_of<PDT_FMT_WB_CU8>(x, first, count, win, tw, v, sum); break;
    default: survey_host_sum_of<PDT_FMT_WB_CS8>(x, first, count, win, tw, v, sum); break;
    }
}

// a survey's parameters with the defaults filled in (pdtrt::survey_plan, pdt_survey.hip)
struct SurveyPlan {
    int nfft, max_carriers;
    double threshold_db, guard_hz, merge_hz;
    uint64_t first, nseg;            // the stretch's first frame, its whole segments
};

struct SurveyCarrier {             // (= pdt_carrier of include/pdt.h)
    double offset_hz;
    float peak_db;
    float floor_power;
};

// the median of P[0 .. n), n even: the mean of the two middle values, in double
inline double survey_floor(const float *P, int n)
{
    std::vector<float> s(P, P + n);
    std::sort(s.begin(), s.end());
    return 0.5 * ((double)s[(size_t)(n / 2 - 1)] + (double)s[(size_t)(n / 2)]);
}

// The greedy search over the averaged spectrum P (bin b at b in_rate / n, the upper half negative): the strongest bin not yet
// blanked; stop below floor 10^(threshold_db / 10) or at `max` carriers; its frequency = the centroid of max(P - floor, 0) over the
// bins within merge_hz of it (wrapping at the band's edge); blank the bins within guard_hz of it.  Strongest first.  Returns the count.
inline int survey_detect(const float *P, int n, double in_rate, double threshold_db, double guard_hz, double merge_hz, int max, SurveyCarrier *found)
{
    const double floor = survey_floor(P, n), binw = in_rate / (double)n;
    const double level = floor * pow(10.0, threshold_db / 10.0);
    const int mb = (int)std::min<double>(std::floor(merge_hz / binw), (double)(n / 2 - 1));
    const int gb = (int)std::min<double>(std::floor(guard_hz / binw), (double)(n / 2));
    std::vector<unsigned char> blank((size_t)n, 0);
    int count = 0;
    while (count < max) {
        int b = -1;
        for (int i = 0; i < n; i++)
            if (!blank[(size_t)i] && (b < 0 || P[i] > P[b])) b = i;
        if (b < 0 || !((double)P[b] >= level) || !(P[b] > 0.0f)) break;
        double sw = 0.0, swk = 0.0;
        for (int k = -mb; k <= mb; k++) {
            const double w = std::max((double)P[(b + k + n) % n] - floor, 0.0);
            sw += w;
            swk += w * (double)k;
        }
        double f = ((double)(b < n / 2 ? b : b - n) + (sw > 0.0 ? swk / sw : 0.0)) * binw;
        if (f >= 0.5 * in_rate) f -= in_rate;
        if (f < -0.5 * in_rate) f += in_rate;
        found[count].offset_hz = f;
        found[count].peak_db = (float)(10.0 * log10((double)P[b] / floor));
        found[count].floor_power = (float)floor;
        count++;
        for (int k = -gb; k <= gb; k++) blank[(size_t)((b + k + n) % n)] = 1;
    }
    return count;
}

}  // namespace pdt
