// pdt_ffp.h -- POES bits without a loop: feed-forward carrier, clock and bit decisions on a whole stream.  The chain's bits
// come out of a PLL that must pull in, an AGC, a Gardner loop and a Manchester decoder.  A TIP signal needs none of them: it carries a
// residual carrier all the time (pdt_tone.h measures it at a stride), its modulation is +-1.06 rad Manchester at 8320 bit/s, so the
// full-bit sum h0 + h1 of any bit is a piece of bare carrier, the sum of these pieces over a few dozen neighbouring bits is a phase
// reference, Im((h0 - h1) conj ref) is the bit's soft value, and the bit clock is found block by block by exhaustive search.  There is
// no reference to be bit-exact against, so the arithmetic is fixed here, once, for the kernels (pdt_ffp.hip) and their host restatement
// (pdt_host_ffp_bits) alike:
//   input     a float32 I,Q stream y of n samples at Fs, n < 2^36; the half-bit lasts P = Fs / 16640 samples, 3 <= P <= 64: 49920 <= Fs <=
//             1064960.  cfg: B bits per block (208; 64 .. 832), T clock hypotheses (32; 8 .. 64), W bits of reference either side (16;
//             0 .. 64), J blocks of smoothing either side (4; 0 .. 16)
//   time grid every point of the time axis is an integer in Q16, 1 / 65536 sample, int64.  The nominal start of half-bit k is
//             t_k = (k Fs 65536) / 16640, rounded down (= (k Fs 256) / 65); the offset of clock phase f (any integer, in steps of 1 / T bit)
//             is o(f) = (f 2 Fs 65536) / (16640 T), rounded down (towards minus infinity for a negative f).  Under f, bit m >= 0 covers
//             [t_2m + o, t_2m+2 + o), its half-bits meet at t_2m+1 + o.  A bit EXISTS under f when t_2m + o >= 0 and t_2m+2 + o <= n 65536
//   carrier   measured (the default): pdt_tones' arithmetic (k_tones, tone_derive, unchanged) over the segments of nfft samples at stride
//             nfft from sample 0, nfft and the search set that call's defaults; residual_j = the record's residual_hz, derived on the
//             host in double (the call's one round trip).  step_j = ddc_step(Fs, residual_j); a segment with valid = 0 takes the step of
//             the nearest earlier valid one, or 0 when there is none; the tail behind the last whole segment takes the last segment's
//             step; a stream without a whole segment, or a rate without an allowed nfft, has step 0 throughout.  Given
//             (PDT_FFP_RESIDUAL_GIVEN): one step = ddc_step(Fs, residual_hz) for the whole stream.  The mixer's phase is continuous:
//             the start phase of segment j is the uint32 wrap-around sum of step_i nfft over the earlier segments, sample i of segment
//             j (the tail counts to the last segment) has phase(i) = start_j + (i - j nfft) step_j mod 2^32
//   v[i]      = ddc_mix(y[i], phase(i)) with the down-converter's table; v = 0 outside [0, n)
//   sums      the sum over a Q16 interval [a, b), a < b, is the fma chain s = fmaf(v[i], w_i, s) from +0 in ascending i, I and Q each,
//             over the samples i = a >> 16 .. (b - 1) >> 16, w_i = the part of [i, i + 1) inside [a, b) as a float, frac / 65536
//             (exact; a sample wholly inside has w = 1)
//   bit       h0, h1 = the sums of its two half-bits; c = h0 + h1 and e = h0 - h1, component by component
//   ref_m     under f: the float addition chain from +0 of c over the bits m - W .. m + W that exist under f, in ascending order
//   d_m       = fmaf(e.im, ref.re, -(e.re ref.im)), the product rounded first: Im(e conj ref)
//   q(d)      pdt_ff.h's: 0 when d is not finite, 2^52 when |d| >= 2^20, else (uint64)(|d| 2^32), truncated
//   blocks    L = (2 B Fs + 8320) / 16640 samples, B nominal bits rounded to the nearest sample; block b covers the samples [b L, (b + 1) L),
//             nb = ceil(n / L) of them.  M(b, tau), tau = 0 .. T - 1: the uint64 sum of q(d_m) over the bits that exist under tau and
//             start inside block b
//   smoothing Ms(b, tau) = the sum of M(b + j, tau) over |j| <= J, blocks outside the stream left out; tau_b = the arg-max of Ms(b, .),
//             ties to the smaller tau
//   unwrap    phi_0 = tau_0; phi_b = phi_{b-1} + delta_b, delta_b = (tau_b - tau_{b-1}) mod T folded into (-T / 2, T / 2] (2 delta > T:
//             delta - T).  A drifting recorder clock lets phi run on; the bit index m stays the index of one physical bit
//   ownership m_lo(b) = the smallest m >= 0 whose start under phi_b is >= b L 65536; m_end(b) = the largest m that exists under phi_b (-1
//             when none).  Block b decides the bits m_lo(b) <= m < m_hi(b), all of them under phi_b: m_hi(b) = min(m_lo(b + 1), m_end(b)
//             + 1) (the last block: m_end(b) + 1); its count is max(0, m_hi - m_lo).  Output positions are the exclusive scan of the counts
//   decision  bit '1' when d_m > 0, else '0'; the soft value is d_m (every NaN as the quiet NaN 0x7fc00000); the time source is the
//             sample index at which the bit ends, (t_2m+2 + o + 65535) >> 16
// The carrier reference is absolute, so there is no pairing or polarity guess; a mirrored spectrum complements the bits and the
// flywheel (pdt_tip_sync.h) reads either polarity.  Left open by the issue and fixed here: the bound on n, rounding of t_k and o(f)
// (down), which bits exist, that a reference window skips bits that do not exist (adding +0 instead changes no bit of the chain), the
// step of a stream without a whole segment, that m_hi is capped by m_end in every block, and the rounding of the time source (up).
#pragma once
#include <math.h>
#include <stdint.h>
#include "pdt_ddc.h"
#include "pdt_ff.h"

namespace pdt {

constexpr uint32_t FFP_MIN_RATE = 49920, FFP_MAX_RATE = 1064960;
constexpr long long FFP_MAX_SAMPLES = 1ll << 36;
constexpr int FFP_B_DEFAULT = 208, FFP_B_MIN = 64, FFP_B_MAX = 832;
constexpr int FFP_T_DEFAULT = 32, FFP_T_MIN = 8, FFP_T_MAX = 64;
constexpr int FFP_W_DEFAULT = 16, FFP_W_MAX = 64;
constexpr int FFP_J_DEFAULT = 4, FFP_J_MAX = 16;
constexpr int FFP_MIX_TILE = 1024;                         // samples a workgroup of k_ffp_mix converts
constexpr int FFP_PIECE = 2048;                            // samples of v a workgroup stages in LDS at a time
constexpr int FFP_CE_BYTES = 40 * 1024;                    // LDS a workgroup of k_ffp_search spends on the (c, e) pairs of its hypotheses
constexpr int FFP_BITS_CHUNK = 512;                        // bits a workgroup of k_ffp_bits decides per round of its loop

struct FfpSync {                    // (= pdt_ffp_sync of include/pdt.h)
    double residual_hz;             // given: the caller's; measured: that of the first valid segment, 0 when there is none
    uint32_t step;                  // ... and its step
    int32_t nfft;                   // the tone segments' length, 0 when the residual was given or no length is allowed
    uint64_t segs, segs_valid;      // tone segments measured, and how many of them were valid
    uint64_t nblocks, nbits;
    int64_t block_len;              // L
    int32_t B, T, W, J;
};

struct FfpBlock {                   // (= pdt_ffp_block of include/pdt.h)
    int64_t phi;
    int64_t first_bit;              // m_lo(b)
    uint64_t count;
    uint64_t metric;                // Ms(b, tau_b)
    int32_t tau;
    int32_t reserved_;
};

struct FfpOutPtrs {                 // where a call's results go, on the device: the layout the flywheel's kernels read
    unsigned long long *nbits;
    FfpSync *sync;
    FfpBlock *blocks;               // nb records
    unsigned long long *pos;        // nb + 1
    long long *symidx;
    float *soft;
    unsigned *bitsym;
    unsigned char *bits;
};

struct FfpRule {                    // a call's constants
    long long fs, n, L, nb;
    int B, T, W, J;
};

__host__ __device__ __forceinline__ long long ffp_floordiv(long long a, long long b)          // b > 0
{
    const long long q = a / b;
    return (a % b < 0) ? q - 1 : q;
}
__host__ __device__ __forceinline__ long long ffp_ceildiv(long long a, long long b) { return -ffp_floordiv(-a, b); }

// t_k
__host__ __device__ __forceinline__ long long ffp_t(long long k, long long fs) { return (k * fs * 256) / 65; }
// o(f)
__host__ __device__ __forceinline__ long long ffp_off(long long f, long long fs, int T) { return ffp_floordiv(f * fs * 512, 65ll * T); }
// L
inline long long ffp_block_len(int B, long long fs) { return (2ll * B * fs + 8320) / 16640; }

// the smallest m >= 0 with t_2m + off >= x (x, off in Q16): t_2m = floor(m fs 512 / 65) >= X  <=>  m >= ceil(65 X / (512 fs))
__host__ __device__ __forceinline__ long long ffp_first_bit(long long x, long long off, long long fs)
{
    const long long X = x - off;
    return X <= 0 ? 0 : ffp_ceildiv(65 * X, 512 * fs);
}
// the largest m with t_2m+2 + off <= n 65536, -1 when there is none: floor(K fs 256 / 65) <= Y  <=>  K <= ((Y + 1) 65 - 1) / (256 fs), K = 2 m + 2
__host__ __device__ __forceinline__ long long ffp_last_bit(long long n, long long off, long long fs)
{
    const long long Y = (n << 16) - off;
    if (Y < 0) return -1;
    const long long K = ((Y + 1) * 65 - 1) / (256 * fs);
    return (K >> 1) - 1;
}
// the first and last bit that exist under `off`: [lo, hi], hi < lo when none does
__host__ __device__ __forceinline__ void ffp_exist(long long n, long long off, long long fs, long long &lo, long long &hi)
{
    lo = ffp_first_bit(0, off, fs);
    hi = ffp_last_bit(n, off, fs);
}

// the sum of the rule over the Q16 interval [a, b), 0 <= a < b: v = the pairs of sample `base` on (every sample of the interval is there)
__host__ __device__ __forceinline__ void ffp_sum(const float *__restrict__ v, long long base, long long a, long long b, float &sr, float &si)
{
    const long long i0 = a >> 16, i1 = (b - 1) >> 16;
    sr = 0.0f;
    si = 0.0f;
    for (long long i = i0; i <= i1; i++) {
        const long long lo = i == i0 ? a : i << 16, hi = i == i1 ? b : (i + 1) << 16;
        const float w = (float)(int)(hi - lo) * (1.0f / 65536.0f);
        sr = fmaf(v[2 * (i - base)], w, sr);
        si = fmaf(v[2 * (i - base) + 1], w, si);
    }
}

// c and e of bit m under `off`
__host__ __device__ __forceinline__ void ffp_bit(const float *__restrict__ v, long long base, long long m, long long off, long long fs, float &cr, float &ci,
                                                 float &er, float &ei)
{
    const long long a0 = ffp_t(2 * m, fs) + off, a1 = ffp_t(2 * m + 1, fs) + off, a2 = ffp_t(2 * m + 2, fs) + off;
    float ar, ai, br, bi;
    ffp_sum(v, base, a0, a1, ar, ai);
    ffp_sum(v, base, a1, a2, br, bi);
    cr = ar + br;
    ci = ai + bi;
    er = ar - br;
    ei = ai - bi;
}

// delta folded into (-T / 2, T / 2]
__host__ __device__ __forceinline__ int ffp_fold(int tau, int prev, int T)
{
    int d = (tau - prev) % T;
    if (d < 0) d += T;
    return 2 * d > T ? d - T : d;
}

// the sample index at which bit m ends under `off`
__host__ __device__ __forceinline__ long long ffp_end_sample(long long m, long long off, long long fs) { return (ffp_t(2 * m + 2, fs) + off + 65535) >> 16; }

// phase(i) of a table of `nent` >= 1 entries (step, start phase), entry j from sample j nfft on, the last one to the stream's end
__host__ __device__ __forceinline__ uint32_t ffp_phase(const uint32_t *__restrict__ steps, const uint32_t *__restrict__ starts, long long nent, long long nfft,
                                                       long long i)
{
    long long j = i / nfft;
    if (j > nent - 1) j = nent - 1;
    return starts[j] + (uint32_t)(unsigned long long)(i - j * nfft) * steps[j];
}

}  // namespace pdt
