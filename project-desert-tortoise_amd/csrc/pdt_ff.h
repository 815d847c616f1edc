// pdt_ff.h -- ARGOS bits without a loop: feed-forward bit decisions on one burst's window.  The chain's bits come out of a
// PLL that must pull in, a squelch, a Gardner loop and a Manchester decoder that guesses the symbol pairing.  A burst needs none of
// them: it opens with 160 ms of bare carrier (pdt_tone.h measures it), its modulation is +-1.1 rad Manchester at 400 bit/s, so every
// bit carries its own phase reference -- with half-bit sums h0, h1, Im(h0 conj h1) = Im((h0 - h1) conj (h0 + h1)) and h0 + h1 is the bit's
// residual carrier -- and its bit timing is found by exhaustive search over offset and bit rate.  There is no reference to be bit-exact
// against, so the arithmetic is fixed here, once, for the kernels (pdt_ff.hip) and their host restatement (pdt_host_ff_bits) alike:
//   input   a float32 I,Q stream y of n samples at Fs; 800 divides Fs, H = Fs / 800 samples per half-bit, 4 <= H <= 128.  Only the first
//           L = min(n, 2 Fs) samples are used (a burst lasts at most 0.92 s)
//   v[i]    = ddc_mix(y[i], (uint32)(i step)) with the down-converter's table, step = ddc_step(Fs, residual_hz): the carrier taken out
//   P_r     = llrint(H 65536 (1 + r ppm 1e-6)) in double, r = -R .. R: the half-bit period of rate hypothesis r in 1 / 65536 sample
//   b_k     = (k P_r + 32768) >> 16 in 64-bit integers: half-bit k of offset hypothesis tau = 0 .. 2 H - 1 covers the samples
//           [tau + b_k, tau + b_{k+1}); K = the largest even number with tau + b_K <= L, the hypothesis holds K / 2 bits
//   s_k     = the float sum of v over half-bit k, I and Q each an addition chain from +0 in ascending sample index
//   d_m     = fmaf(s_{2m}.im, s_{2m+1}.re, -(s_{2m}.re s_{2m+1}.im)), the product rounded first: Im(s_{2m} conj s_{2m+1})
//   q_m     = 0 when d_m is not finite, 2^52 when |d_m| >= 2^20, else (uint64)(|d_m| 2^32), truncated
//   M(r, tau) = sum_m q_m in uint64: an integer, so no order of summation can change it
//   winner  the largest M; ties go to the smaller |r|, then the smaller r, then the smaller tau (all zero or too short: r = 0, tau = 0)
//   bit m   = '1' when d_m > 0, else '0'; its soft value is d_m (a NaN, whose sign and payload the hardware leaves open, as the quiet NaN
//           0x7fc00000); its time source the sample index tau + b_{2m+2}
// tau spans both symbol pairings and the message rules (pdt_argos_msg.h) read either polarity: neither needs a rule here.
#pragma once
#include <math.h>
#include <stdint.h>
#include "pdt_ddc.h"

namespace pdt {

constexpr int FF_MIN_H = 4, FF_MAX_H = 128;                // samples per half-bit
constexpr int FF_RATE_STEPS_MAX = 32, FF_RATE_STEPS_DEFAULT = 20;
constexpr double FF_RATE_PPM_DEFAULT = 625.0;
constexpr double FF_RATE_SPAN_MAX = 0.1;                   // R ppm 1e-6 may not exceed this: periods stay within 10 % of H
constexpr int FF_MIX_TILE = 1024;                          // samples a workgroup of k_ff_mix converts
constexpr int FF_SEARCH_BITS = 16;                         // bits of one hypothesis a workgroup of k_ff_search sums

struct FfSync {                     // (= pdt_ff_sync of include/pdt.h)
    double residual_hz;
    int32_t tone_valid;
    uint32_t step;
    int32_t tau, rate;
    int64_t period;
    uint64_t metric;
    uint64_t nbits;
};

// one window of a launch, on the device: its stream, the launch's scratch for it, where its results go
struct FfWin {
    const float *y;                 // I,Q pairs, L of them are read
    float *v;                       // the mixed stream, L pairs (scratch)
    unsigned long long *metric;     // M(r, tau) at [(r + R) 2 H + tau] (scratch; zero before k_ff_search)
    unsigned char *bits;            // '0' / '1'
    float *soft;
    long long *symidx;              // the message kernels' time source: symidx[bitsym[m]] = the sample index of bit m
    unsigned *bitsym;               // = m
    unsigned long long *nbits;
    FfSync *sync;
    long long L;
    double residual_hz;
    uint32_t step;
    int32_t tone_valid;
    int32_t tile0;                  // the window's first workgroup in k_ff_mix's grid
    int32_t group0;                 // ... in k_ff_search's grid
    int32_t segs;                   // segments of FF_SEARCH_BITS bits the search cuts the window into
    int32_t reserved_;
};

inline int64_t ff_period(int H, int r, double ppm) { return (int64_t)llrint((double)H * 65536.0 * (1.0 + (double)r * ppm * 1e-6)); }

__host__ __device__ __forceinline__ long long ff_bound(long long k, long long P) { return (k * P + 32768) >> 16; }

// K: the largest even k with tau + b_k <= L
__host__ __device__ __forceinline__ long long ff_halves(long long L, long long tau, long long P)
{
    const long long X = L - tau;
    if (X < 0) return 0;
    // b_k <= X  <=>  k P + 32768 < (X + 1) 65536
    const long long k = (((X + 1) << 16) - 32769) / P;
    return k & ~1ll;
}

__host__ __device__ __forceinline__ float ff_cross(float ar, float ai, float br, float bi)
{
    const float p = ar * bi;
    return fmaf(ai, br, -p);
}

__host__ __device__ __forceinline__ unsigned long long ff_quant(float d)
{
    const float a = fabsf(d);
    if (!(a <= 3.402823466e+38f)) return 0ull;             // NaN or infinite
    if (a >= 1048576.0f) return 1ull << 52;
    return (unsigned long long)(a * 4294967296.0f);
}

// is hypothesis (m1, r1, t1) in front of (m2, r2, t2) in the winner's order?
__host__ __device__ __forceinline__ bool ff_before(unsigned long long m1, int r1, int t1, unsigned long long m2, int r2, int t2)
{
    if (m1 != m2) return m1 > m2;
    const int a1 = r1 < 0 ? -r1 : r1, a2 = r2 < 0 ? -r2 : r2;
    if (a1 != a2) return a1 < a2;
    if (r1 != r2) return r1 < r2;
    return t1 < t2;
}

// the soft value as it is stored: d, every NaN as 0x7fc00000
__host__ __device__ __forceinline__ float ff_soft(float d)
{
    union { uint32_t u; float f; } q;
    q.u = 0x7fc00000u;
    return d != d ? q.f : d;
}

// the sum of v over [lo, hi): the chain of the rule
__host__ __device__ __forceinline__ void ff_sum(const float *__restrict__ v, long long lo, long long hi, float &sr, float &si)
{
    sr = 0.0f;
    si = 0.0f;
    for (long long i = lo; i < hi; i++) {
        sr += v[2 * i];
        si += v[2 * i + 1];
    }
}

// d_m of hypothesis (P, tau)
__host__ __device__ __forceinline__ float ff_bit(const float *__restrict__ v, long long tau, long long P, long long m)
{
    const long long b0 = tau + ff_bound(2 * m, P), b1 = tau + ff_bound(2 * m + 1, P), b2 = tau + ff_bound(2 * m + 2, P);
    float ar, ai, br, bi;
    ff_sum(v, b0, b1, ar, ai);
    ff_sum(v, b1, b2, br, bi);
    return ff_cross(ar, ai, br, bi);
}

}  // namespace pdt
