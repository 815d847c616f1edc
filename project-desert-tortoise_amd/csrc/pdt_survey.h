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
constexpr int SURVEY_MAX_CARRIERS = 16;         // what one k_ddc launch takes
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
