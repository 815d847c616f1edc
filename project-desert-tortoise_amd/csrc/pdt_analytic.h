// pdt_analytic.h -- the Hilbert front end of single-channel (real) captures: x[n] -> z[n] = (x[n] + j Q[n]) e^{-j phi[n]}, one
// float32 I,Q pair per real sample, which the chain then takes as a RAW float capture.  There is no reference
// to be bit-exact against, so the arithmetic is fixed here, once, for the kernel (pdt_analytic.hip) and its host restatement
// (pdt_host_analytic) alike:
//   Q[n]   = sum_{k = 1, 3, .., 31} h[k] (x[n - k] - x[n + k]): an fmaf chain in ascending k from 0, each difference rounded first;
//            h[k] = 2 / (pi k) w[k], w the 63-point Blackman window, computed in double and rounded to float; x = 0 outside [0, N)
//   p[n]   = step n mod 2^32 on the GLOBAL sample index (so the phase is the same however a capture is cut), step = round(centre 2^32 / Fs)
//   (c, s) = (cos, sin)(2 pi p / 2^32): quadrant from the top two bits (exact swaps / negations), then a 1024-entry table of the
//            quadrant's coarse angles times the small-angle pair (1 - t^2 / 2, t) of the remaining 20 bits (|t| < 1.6e-3)
//   z[n]   = (x c + Q s, Q c - x s)
#pragma once
#include <stdint.h>
#include "pdt_device_math.h"

namespace pdt {

constexpr int AN_HALF = 31;            // D: the Hilbert branch reaches 31 samples each way (63 taps, centred, no delay)
constexpr int AN_NTAP = 16;            // its non-zero taps on one side: k = 1, 3, .., 31
constexpr int AN_TAB = 1024;           // coarse rotation table: angles 2 pi i / 4096, i < 1024 (one quadrant)

struct AnalyticTaps {
    float h[AN_NTAP];                  // h[i] = h(k = 2 i + 1)
};

inline AnalyticTaps analytic_taps()
{
    AnalyticTaps t;
    for (int i = 0; i < AN_NTAP; i++) {
        const int k = 2 * i + 1, n = k + AN_HALF;
        const double w = 0.42 - 0.5 * cos_glibc(2.0 * M_PI * n / 62.0) + 0.08 * cos_glibc(4.0 * M_PI * n / 62.0);
        t.h[i] = (float)(2.0 / (M_PI * k) * w);
    }
    return t;
}

// tab[2 i] = cos, tab[2 i + 1] = sin of 2 pi i / 4096, in double, rounded to float
inline void analytic_table(float *tab)
{
    for (int i = 0; i < AN_TAB; i++) {
        const double a = 2.0 * M_PI * (double)i / 4096.0;
        tab[2 * i] = (float)cos_glibc(a);
        tab[2 * i + 1] = (float)sin_glibc(a);
    }
}

// 0 = Fs / 4; otherwise round(centre 2^32 / Fs).  The caller has checked 0 < centre < Fs / 2.
inline uint32_t analytic_step(uint32_t fs, double centre_hz)
{
    if (centre_hz == 0.0) return 1u << 30;
    return (uint32_t)llrint(centre_hz * 4294967296.0 / (double)fs);
}

// (cos, sin)(2 pi p / 2^32)
__host__ __device__ __forceinline__ void analytic_rot(uint32_t p, const float *__restrict__ tab, float &c, float &s)
{
    const uint32_t q = p >> 30, r = p & 0x3fffffffu;
    const uint32_t hi = r >> 20, lo = r & 0xfffffu;
    const float ch = tab[2 * hi], sh = tab[2 * hi + 1];
    const float t = (float)lo * 1.46291807926715968e-09f;          // 2 pi / 2^32
    const float cl = 1.0f - (0.5f * t) * t, sl = t;
    const float cr = ch * cl - sh * sl, sr = sh * cl + ch * sl;
    switch (q) {
    case 0: c = cr; s = sr; break;
    case 1: c = -sr; s = cr; break;
    case 2: c = -cr; s = -sr; break;
    default: c = sr; s = -cr; break;
    }
}

// z = (x + j Q) (c - j s)
__host__ __device__ __forceinline__ void analytic_mix(float x, float q, float c, float s, float &zr, float &zi)
{
    zr = x * c + q * s;
    zi = q * c - x * s;
}

}  // namespace pdt
