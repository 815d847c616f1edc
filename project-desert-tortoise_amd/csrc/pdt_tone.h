// pdt_tone.h -- the carrier of a channel stream as a measurement: frequency, level and C/N0 of the strongest line of a segment
// (DESIGN 4.15).  ARGOS locates platforms from the Doppler shift of their carrier; every burst opens with 160 ms of it, and a POES
// channel carries it all the time.  As for the survey (pdt_survey.h) there is no reference to be bit-exact against, so the arithmetic
// is fixed here, once, for the kernel (pdt_tone.hip) and its host restatement (pdt_host_tones) alike:
//   y         = a float32 I,Q stream at rate Fs (on the device: a context's PDT_ST_CHANNEL)
//   segment i = the N samples from first + i stride on, N in {1024, 4096, 16384}; only segments wholly inside the stream are measured
//   p[b]      = survey_segment<PDT_FMT_WB_F32, N> as it is (Blackman window, radix-4 passes, re^2 + im^2): place j holds bin survey_rev(j)
//   peak      = over the bins with |f_b| <= search_hz (f_b = b Fs / N, the upper half negative: b <= kmax or b >= N - kmax,
//               kmax = tone_kmax): key = burst_key(p[b]) (the bit pattern where p > 0, else 0), the largest key, of equal keys the
//               lowest b -- k_row_peaks' rule
//   raw record (ToneRaw, 32 bytes): the peak's bin, p at bin - 1, bin, bin + 1 (wrapping at N), and
//   noise_sum = the float sum, from 0, of p over the bins at circular distance noise_lo .. noise_hi from the peak, in the order
//               bin - noise_hi, .., bin - noise_lo, bin + noise_lo, .., bin + noise_hi (all mod N); noise_bins = 2 (noise_hi - noise_lo + 1)
//   derived values: tone_derive below, on the host, in double, for the context path and the hook alike
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include "pdt_survey.h"
#include "pdt_bursts.h"

namespace pdt {

constexpr int TONE_NOISE_LO = 8, TONE_NOISE_HI = 71;       // 128 noise bins, clear of the Blackman main lobe and its first side lobes
constexpr double TONE_SEGMENT_S = 0.128;                   // the default segment: inside the 160 ms of carrier an ARGOS burst opens with

struct ToneRaw {                    // what the kernel's one lane stores (two 16-byte stores)
    int32_t bin;
    float below, peak, above;
    float noise_sum;
    int32_t noise_bins;
    int32_t pad_[2];
};

struct Tone {                       // (= pdt_tone of include/pdt.h)
    double time_s, freq_hz, residual_hz, power, cn0_dbhz;
    int32_t valid;
    int32_t bin;
    float below, peak, above, noise_sum;
    int32_t noise_bins;
    int32_t reserved_;
};

struct ToneSeg {                    // one segment of a launch: its stream (device), its first sample, its record, its search set
    const void *x;
    long long first;
    int32_t rec, kmax;
};

// a call's parameters with the defaults filled in (pdtrt::tone_plan, pdt_tone.hip)
struct TonePlan {
    int nfft, kmax, noise_lo, noise_hi;
    uint64_t first, stride, nseg;
};

// the largest bin of the search set: floor(search_hz N / Fs), at most N / 2 - 1
inline int tone_kmax(double search_hz, double fs, int n)
{
    const double k = std::floor(search_hz * (double)n / fs);
    return k >= (double)(n / 2 - 1) ? n / 2 - 1 : k < 0.0 ? 0 : (int)k;
}

// the largest allowed N with N / Fs <= TONE_SEGMENT_S, 0 when there is none
inline int tone_default_nfft(double fs)
{
    for (int n = 16384; n >= 1024; n >>= 2)
        if ((double)n / fs <= TONE_SEGMENT_S) return n;
    return 0;
}

// bin i of the noise sum, i < noise_bins, in the order they are added
__host__ __device__ __forceinline__ int tone_noise_bin(int bin, int i, int lo, int hi, int n)
{
    const int side = hi - lo + 1;
    const int d = i < side ? -(hi - i) : lo + (i - side);
    return (bin + d + n) & (n - 1);
}

// the candidate of the peak search: the largest is the strongest bin, of equal ones the lowest
__host__ __device__ __forceinline__ unsigned long long tone_cand(uint32_t key, int bin)
{
    return ((unsigned long long)key << 32) | (unsigned long long)(0xffffffffu - (uint32_t)bin);
}

__host__ __device__ __forceinline__ bool tone_in_search(int bin, int kmax, int n) { return bin <= kmax || bin >= n - kmax; }

// the raw record of the segment that starts at sample `first` of the float pairs x, on the host (v: room for N = win.size() places)
inline ToneRaw tone_host_raw(const void *x, long long first, int kmax, int lo, int hi, const std::vector<float> &win, const std::vector<float> &tw,
                             std::vector<SurveyC> &v)
{
    const int N = (int)win.size(), log4 = survey_log4(N);
    survey_host_segment<PDT_FMT_WB_F32>(x, first, win, tw, v);
    auto p = [&](int b) { return survey_power(v[(size_t)survey_rev((uint32_t)(b & (N - 1)), log4)]); };
    unsigned long long best = 0;
    for (int b = 0; b < N; b++)
        if (tone_in_search(b, kmax, N)) best = std::max(best, tone_cand(burst_key(p(b)), b));
    ToneRaw r;
    memset(&r, 0, sizeof r);
    r.bin = (int)(0xffffffffu - (uint32_t)best);
    r.below = p(r.bin + N - 1);
    r.peak = p(r.bin);
    r.above = p(r.bin + 1);
    r.noise_bins = 2 * (hi - lo + 1);
    float s = 0.0f;
    for (int i = 0; i < r.noise_bins; i++) s = s + p(tone_noise_bin(r.bin, i, lo, hi, N));
    r.noise_sum = s;
    return r;
}

// the window's sums, in double in ascending order over the float values: sw = sum w, sw2 = sum w^2
inline void tone_window_sums(const std::vector<float> &win, double &sw, double &sw2)
{
    sw = sw2 = 0.0;
    for (float w : win) {
        sw += (double)w;
        sw2 += (double)w * (double)w;
    }
}

// The derived values of a raw record (the one function of the context path and of the hook), with L = ln p:
//   delta = (L- - L+) / (2 (L- - 2 L0 + L+)), residual_hz = (signed bin + delta) Fs / N, freq_hz = offset_hz + residual_hz,
//   peak level = L0 - (L- - L+) delta / 4, power = exp(peak level) / (sum w)^2,
//   cn0_dbhz = 10 log10(power / (noise_sum / noise_bins / sum w^2) Fs), time_s = (start + (N - 1) / 2) / Fs, start = the segment's first sample.
// Not valid -- a neighbour <= 0, a curvature >= 0, a peak that is not > 0 (key 0) --: the bin's centre, the bin's own power, cn0 NaN.
inline Tone tone_derive(const ToneRaw &r, int n, double fs, double offset_hz, uint64_t start, double sw, double sw2)
{
    Tone t;
    memset(&t, 0, sizeof t);
    t.bin = r.bin;
    t.below = r.below;
    t.peak = r.peak;
    t.above = r.above;
    t.noise_sum = r.noise_sum;
    t.noise_bins = r.noise_bins;
    t.time_s = ((double)start + 0.5 * (double)(n - 1)) / fs;
    const double sb = (double)(r.bin < n / 2 ? r.bin : r.bin - n);
    double delta = 0.0, level = r.peak > 0.0f ? log((double)r.peak) : 0.0;
    bool ok = r.peak > 0.0f && r.below > 0.0f && r.above > 0.0f;
    if (ok) {
        const double lm = log((double)r.below), lp = log((double)r.above), curv = lm - 2.0 * level + lp;
        ok = curv < 0.0;
        if (ok) {
            delta = 0.5 * (lm - lp) / curv;
            level = level - 0.25 * (lm - lp) * delta;
        }
    }
    t.valid = ok ? 1 : 0;
    t.residual_hz = (sb + delta) * fs / (double)n;
    t.freq_hz = offset_hz + t.residual_hz;
    t.power = r.peak > 0.0f ? exp(level) / (sw * sw) : 0.0;
    const double n0 = (double)r.noise_sum / (double)r.noise_bins / sw2;
    t.cn0_dbhz = ok && n0 > 0.0 ? 10.0 * log10(t.power / n0 * fs) : (double)NAN;
    return t;
}

}  // namespace pdt
