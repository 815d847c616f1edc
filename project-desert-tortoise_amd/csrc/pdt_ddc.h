// pdt_ddc.h -- the digital down-converter of wideband SDR captures: complex x[n] at Fs_in -> one channel y[m] at Fs_in / D, float32
// I,Q pairs which the chain then takes as a RAW float capture.  As for the Hilbert front end (pdt_analytic.h) there
// is no reference to be bit-exact against, so the arithmetic is fixed here, once, for the kernel (pdt_ddc.hip) and its host
// restatement (pdt_host_ddc) alike:
//   x[n]   = the sample scaled by format: int16 s / 32768, float32 as it is, unsigned 8-bit (u - 127.5) / 128, signed 8-bit s / 128
//   p[n]   = step n mod 2^32 on the GLOBAL sample index, step = round(offset 2^32 / Fs_in) (a negative offset wraps)
//   v[n]   = x[n] e^{-j 2 pi p[n] / 2^32}: (c, s) = analytic_rot(p[n]) with its table, v = (xr c + xi s, xi c - xr s), every product
//            rounded first; v = 0 outside [0, N)
//   h[k]   = sinc(0.8 k / D) blackman_{16 D + 1}[k + 8 D], k = -8 D .. 8 D, in double with cos_glibc / sin_glibc, normalised to unit
//            sum in double, then rounded to float
//   y[m]   = sum_k h[k] v[m D + k], 0 <= m < ceil(N / D): I and Q each an fmaf chain in ascending k from 0
#pragma once
#include <stdint.h>
#include <vector>
#include "pdt_analytic.h"

namespace pdt {

constexpr int DDC_MIN_DECIM = 2, DDC_MAX_DECIM = 64;
constexpr int DDC_SPAN = 8;             // the filter reaches 8 D input samples each way: 16 D + 1 taps

inline bool ddc_fmt(int fmt) { return fmt >= 16 && fmt <= 19; }         // PDT_FMT_WB_PCM16 .. PDT_FMT_WB_CS8
// wideband format FMT (PDT_FMT_WB_*): the bytes of one complex input sample and the samples of one 16-byte load, for every kernel
// that reads a capture (k_ddc, survey_segment of pdt_survey.h)
template <int FMT> struct DdcFmt {
    enum { BPS = FMT == 16 ? 4 : FMT == 17 ? 8 : 2, SPV = 16 / BPS };
};

// h[k + 8 D], 16 D + 1 floats
inline std::vector<float> ddc_taps(int D)
{
    const int n = 2 * DDC_SPAN * D + 1;
    std::vector<double> h((size_t)n);
    double sum = 0.0;
    for (int i = 0; i < n; i++) {
        const int k = i - DDC_SPAN * D;
        const double a = M_PI * 0.8 * (double)k / (double)D;
        const double sinc = k == 0 ? 1.0 : sin_glibc(a) / a;
        const double w = 0.42 - 0.5 * cos_glibc(2.0 * M_PI * (double)i / (double)(n - 1)) + 0.08 * cos_glibc(4.0 * M_PI * (double)i / (double)(n - 1));
        h[(size_t)i] = sinc * w;
        sum += h[(size_t)i];
    }
    std::vector<float> t((size_t)n);
    for (int i = 0; i < n; i++) t[(size_t)i] = (float)(h[(size_t)i] / sum);
    return t;
}

// round(offset 2^32 / Fs_in), modulo 2^32.  The caller has checked |offset| < Fs_in / 2.
inline uint32_t ddc_step(double in_rate, double offset_hz)
{
    return (uint32_t)(int64_t)llrint(offset_hz * 4294967296.0 / in_rate);
}

// sample i of a wideband capture at x, scaled
template <int FMT> __host__ __device__ __forceinline__ void ddc_load(const void *x, long long i, float &re, float &im)
{
    if (FMT == 16) {
        const int16_t *p = reinterpret_cast<const int16_t *>(x) + 2 * i;
        re = (float)p[0] / 32768.0f; im = (float)p[1] / 32768.0f;
    } else if (FMT == 17) {
        const float *p = reinterpret_cast<const float *>(x) + 2 * i;
        re = p[0]; im = p[1];
    } else if (FMT == 18) {
        const uint8_t *p = reinterpret_cast<const uint8_t *>(x) + 2 * i;
        re = ((float)p[0] - 127.5f) / 128.0f; im = ((float)p[1] - 127.5f) / 128.0f;
    } else {
        const int8_t *p = reinterpret_cast<const int8_t *>(x) + 2 * i;
        re = (float)p[0] / 128.0f; im = (float)p[1] / 128.0f;
    }
}

// One conversion of the kernel (k_ddc).  x: the address of input sample 0; the samples lo <= i < hi are
// present, zeros lie elsewhere.  Output m, 0 <= m < n_out, is centred on input m D and goes to out[m]; n_out is the caller's (a
// stream piece asks for fewer outputs than its view holds).  g0: the global index of input 0, modulo 2^32 -- the phase of input i
// is (g0 + i) step mod 2^32.  A whole capture or a window of n frames: lo = 0, hi = n, g0 = 0, n_out = ceil(n / D).  A stream
// piece: lo = -(the left halo kept), g0 = D times the outputs made so far.  tile0: the launch's first tile of this record.  The
// per-call table of a launch of many records, on the device: the records, then one int per tile, the tile's record.
struct DdcWindow {
    const void *x;
    void *out;
    long long lo, hi, n_out;
    uint32_t step, g0;
    int tile0;
};

// v = x e^{-j 2 pi p / 2^32}
__host__ __device__ __forceinline__ void ddc_mix(float xr, float xi, uint32_t p, const float *__restrict__ tab, float &vr, float &vi)
{
    float c, s;
    analytic_rot(p, tab, c, s);
    analytic_mix(xr, xi, c, s, vr, vi);
}

}  // namespace pdt
