// pdt_ff.hip -- feed-forward ARGOS bits of burst windows (pdt_ff.h): the kernel that takes the measured carrier out (k_ff_mix), the
// exhaustive search over bit offset and bit rate (k_ff_search), the choice of the winner and its bits (k_ff_pick), their launch, and
// the host restatement pdt_host_ff_bits / pdt_host_ff_mix.  A unit of its own, beside pdt_tone.hip and pdt_argos_msg.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../include/pdt.h"
#include "pdt_ff.h"

static_assert(sizeof(pdt_ff_sync) == sizeof(pdt::FfSync) && sizeof(pdt_ff_sync) == 48, "pdt_ff_sync");
static_assert(sizeof(pdt_ff_cfg) == 32, "pdt_ff_cfg");
static_assert(sizeof(pdt::FfWin) == 112, "the launch's table");

namespace pdt {

// the window workgroup `block` of a grid belongs to: the last whose first workgroup in that grid (FIRST) is not behind it
template <int32_t FfWin::*FIRST>
__device__ __forceinline__ int ff_win_of(const FfWin *__restrict__ table, int nwin, int block)
{
    int lo = 0, hi = nwin - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].*FIRST <= block) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// One workgroup per tile of FF_MIX_TILE samples, all windows of a call in one grid: v[i] = y[i] e^{-j 2 pi i step / 2^32}.
__global__ void __launch_bounds__(256) k_ff_mix(const FfWin *__restrict__ table, int nwin, const float *__restrict__ tab)
{
    const FfWin w = table[ff_win_of<&FfWin::tile0>(table, nwin, (int)blockIdx.x)];
    const long long base = ((long long)blockIdx.x - w.tile0) * FF_MIX_TILE;
    const float2 *__restrict__ y = reinterpret_cast<const float2 *>(w.y);
    float2 *__restrict__ v = reinterpret_cast<float2 *>(w.v);
#pragma unroll
    for (int j = 0; j < FF_MIX_TILE / 256; j++) {
        const long long i = base + 256 * j + (int)threadIdx.x;
        if (i < w.L) {
            const float2 a = y[i];
            float2 o;
            ddc_mix(a.x, a.y, (uint32_t)(unsigned long long)i * w.step, tab, o.x, o.y);
            v[i] = o;
        }
    }
}

// The rule's chain over n pairs of LDS from byte address `at` on, n the same in every lane: sr, si = the sums from +0 in ascending index.
// Eight 8-byte reads are issued back to back and waited for once, then added in order.  Written out because the compiler joins
// neighbouring 8-byte reads into ds_read2_b64, which moves half the bytes per LDS cycle; consecutive lanes' single 8-byte reads touch
// every bank once.
__device__ __forceinline__ void ff_lds_sum(unsigned at, int n, float &sr, float &si)
{
    sr = 0.0f;
    si = 0.0f;
    int j = 0;
    for (; j + 8 <= n; j += 8) {
        unsigned long long q0, q1, q2, q3, q4, q5, q6, q7;
        asm volatile("ds_read_b64 %0, %8\n\t"
                     "ds_read_b64 %1, %8 offset:8\n\t"
                     "ds_read_b64 %2, %8 offset:16\n\t"
                     "ds_read_b64 %3, %8 offset:24\n\t"
                     "ds_read_b64 %4, %8 offset:32\n\t"
                     "ds_read_b64 %5, %8 offset:40\n\t"
                     "ds_read_b64 %6, %8 offset:48\n\t"
                     "ds_read_b64 %7, %8 offset:56\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "=&v"(q0), "=&v"(q1), "=&v"(q2), "=&v"(q3), "=&v"(q4), "=&v"(q5), "=&v"(q6), "=&v"(q7)
                     : "v"(at)
                     : "memory");
        const unsigned long long q[8] = { q0, q1, q2, q3, q4, q5, q6, q7 };
#pragma unroll
        for (int k = 0; k < 8; k++) {
            sr += __uint_as_float((unsigned)q[k]);
            si += __uint_as_float((unsigned)(q[k] >> 32));
        }
        at += 64u;
    }
    for (; j < n; j++) {
        unsigned long long q;
        asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(q) : "v"(at) : "memory");
        sr += __uint_as_float((unsigned)q);
        si += __uint_as_float((unsigned)(q >> 32));
        at += 8u;
    }
}

// The hot path.  A workgroup takes one window, one rate hypothesis r and one segment of FF_SEARCH_BITS bits, for ALL 2 H offsets: lane
// tau of the workgroup (64, 128, 192 or 256 lanes) is hypothesis (r, tau).  The half-bit boundaries b_k depend on r alone, so they are
// scalar values, every lane reaches every boundary in the same step and control flow is uniform; lane tau reads sample tau + j of the
// segment, consecutive lanes consecutive 8-byte pairs.  The segment's samples -- from b_{2 m0} on, with a halo of 2 H for the offsets
// -- are staged in LDS once (zeros behind L) and then read by every lane: each sample is loaded from memory once and used 2 H times.
// The two sums of a bit are the rule's chains, in ascending index from +0; q_m is an integer, so the segments of a hypothesis are
// joined by an integer atomic add into M, whatever the order in which the workgroups run.  An offset whose hypothesis ends before a
// bit (its K is smaller) leaves that bit out.
__global__ void __launch_bounds__(256) k_ff_search(const FfWin *__restrict__ table, int nwin, const long long *__restrict__ periods, int H,
                                                  int tile_len)
{
    extern __shared__ __attribute__((aligned(16))) float2 ff_tile[];
    const FfWin w = table[ff_win_of<&FfWin::group0>(table, nwin, (int)blockIdx.x)];
    const int g = (int)blockIdx.x - w.group0, ri = g / w.segs, seg = g - ri * w.segs;
    const long long P = periods[ri];
    const long long m0 = (long long)seg * FF_SEARCH_BITS, most = ff_halves(w.L, 0, P) >> 1;        // (tau = 0 holds the most bits)
    if (m0 >= most) return;
    const long long m1 = m0 + FF_SEARCH_BITS < most ? m0 + FF_SEARCH_BITS : most;
    const long long base = ff_bound(2 * m0, P);
    const float2 *__restrict__ v = reinterpret_cast<const float2 *>(w.v);
    for (int i = (int)threadIdx.x; i < tile_len; i += (int)blockDim.x) {
        const long long idx = base + i;
        ff_tile[i] = idx < w.L ? v[idx] : make_float2(0.0f, 0.0f);
    }
    __syncthreads();
    const bool live = (int)threadIdx.x < 2 * H;
    const int tau = live ? (int)threadIdx.x : 0;
    const long long mine = live ? ff_halves(w.L, tau, P) >> 1 : 0;
    const unsigned t0 = (unsigned)(size_t)(ff_tile + tau);                   // this lane's first pair: its LDS byte address
    unsigned long long acc = 0;
    int lo = 0;
    for (long long m = m0; m < m1; m++) {
        const int mid = (int)(ff_bound(2 * m + 1, P) - base), hi = (int)(ff_bound(2 * m + 2, P) - base);
        float ar, ai, br, bi;
        ff_lds_sum(t0 + 8u * (unsigned)lo, mid - lo, ar, ai);
        ff_lds_sum(t0 + 8u * (unsigned)mid, hi - mid, br, bi);
        const unsigned long long q = ff_quant(ff_cross(ar, ai, br, bi));
        acc += m < mine ? q : 0ull;
        lo = hi;
    }
    if (live && acc) atomicAdd(w.metric + (size_t)ri * (size_t)(2 * H) + (size_t)tau, acc);
}

// One wavefront per window: the arg-max of M in the winner's order -- every lane over its share of the hypotheses, then a butterfly --
// and the winner's bits, a bit per lane and round: d_m recomputed by the rule's chains from v, the character, the soft value and the
// time source in the layout the message kernels read (bitsym[m] = m, symidx[m] = the sample index).  Count and winner stay on the device;
// all: the call's records side by side as well, for one copy to the host.
__global__ void __launch_bounds__(64) k_ff_pick(const FfWin *__restrict__ table, const long long *__restrict__ periods, int R, int H, FfSync *__restrict__ all)
{
    const FfWin w = table[blockIdx.x];
    const int lane = (int)threadIdx.x, nt = 2 * H, total = (2 * R + 1) * nt;
    unsigned long long bm = 0;
    int br = 0, bt = 0;
    bool any = false;
    for (int i = lane; i < total; i += 64) {
        const int r = i / nt - R, tau = i - (r + R) * nt;
        const unsigned long long m = w.metric[i];
        if (!any || ff_before(m, r, tau, bm, br, bt)) {
            bm = m;
            br = r;
            bt = tau;
            any = true;
        }
    }
    if (!any) {                                  // (fewer than 64 hypotheses: a lane without one loses to every real one, |r| = R + 1)
        bm = 0;
        br = R + 1;
        bt = nt;
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const unsigned long long om = __shfl_xor(bm, off);
        const int orr = __shfl_xor(br, off), ot = __shfl_xor(bt, off);
        if (ff_before(om, orr, ot, bm, br, bt)) {
            bm = om;
            br = orr;
            bt = ot;
        }
    }
    const long long P = periods[br + R], nb = ff_halves(w.L, bt, P) >> 1;
    for (long long m = lane; m < nb; m += 64) {
        const float d = ff_bit(w.v, bt, P, m);
        w.bits[m] = d > 0.0f ? '1' : '0';
        w.soft[m] = ff_soft(d);
        w.symidx[m] = bt + ff_bound(2 * m + 2, P);
        w.bitsym[m] = (unsigned)m;
    }
    if (lane == 0) {
        *w.nbits = (unsigned long long)nb;
        FfSync s;
        s.residual_hz = w.residual_hz;
        s.tone_valid = w.tone_valid;
        s.step = w.step;
        s.tau = bt;
        s.rate = br;
        s.period = P;
        s.metric = bm;
        s.nbits = (uint64_t)nb;
        *w.sync = s;
        all[blockIdx.x] = s;
    }
}

}  // namespace pdt

using namespace pdt;

namespace pdtrt {

// LDS pairs of a workgroup of k_ff_search: FF_SEARCH_BITS bits of the longest period, and the offsets' halo
int ff_tile_len(int H, long long pmax) { return (int)((2ll * FF_SEARCH_BITS * pmax + 65535) >> 16) + 2 * H + 1; }

// the three kernels over the nwin records of a table that is on the device.  mix_tiles, groups: the grids of k_ff_mix and k_ff_search
// (the sums over the windows); periods_dev: P_r, r = -R .. R; metric: the windows' M, zeroed here.  inner: NULL, or the two events recorded between
// the kernels (a profiled context times them apart: CallTimer); syncs_dev: room for nwin records, the copy the host reads
hipError_t ff_launch(hipStream_t st, const void *table_dev, int nwin, long long mix_tiles, long long groups, const long long *periods_dev, int R,
                     int H, long long pmax, const float *tab_dev, void *metric_dev, size_t metric_bytes, void *syncs_dev, hipEvent_t *inner)
{
    if (nwin < 1 || mix_tiles < 0 || mix_tiles > 0x7fffffffll || groups < 0 || groups > 0x7fffffffll || R < 0 || R > FF_RATE_STEPS_MAX || H < FF_MIN_H ||
        H > FF_MAX_H)
        return hipErrorInvalidValue;
    const FfWin *table = (const FfWin *)table_dev;
    hipError_t e;
    if (metric_bytes && (e = hipMemsetAsync(metric_dev, 0, metric_bytes, st)) != hipSuccess) return e;
    if (mix_tiles) hipLaunchKernelGGL(k_ff_mix, dim3((unsigned)mix_tiles), dim3(256), 0, st, table, nwin, tab_dev);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (inner && (e = hipEventRecord(inner[0], st)) != hipSuccess) return e;
    const int tile_len = ff_tile_len(H, pmax), lanes = 64 * ((2 * H + 63) / 64);
    if (groups) hipLaunchKernelGGL(k_ff_search, dim3((unsigned)groups), dim3((unsigned)lanes), (size_t)tile_len * sizeof(float2), st, table, nwin, periods_dev, H, tile_len);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (inner && (e = hipEventRecord(inner[1], st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ff_pick, dim3((unsigned)nwin), dim3(64), 0, st, table, periods_dev, R, H, (FfSync *)syncs_dev);
    return hipGetLastError();
}

// cfg (NULL = all defaults) at sample rate `rate`: H, R, ppm, whether the residual is the caller's.  PDT_ERR_ARG for a rate that 800
// does not divide or whose H lies outside 4 .. 128, rate_steps outside 0 .. 32, a step that is not finite, negative or so large that
// R ppm 1e-6 exceeds 0.1, a given residual that is not finite or reaches Fs / 2
int ff_plan(const pdt_ff_cfg *cfg, uint32_t rate, int *H, int *R, double *ppm, int *given, double *residual)
{
    if (rate == 0 || rate % 800u) return PDT_ERR_ARG;
    *H = (int)(rate / 800u);
    if (*H < FF_MIN_H || *H > FF_MAX_H) return PDT_ERR_ARG;
    *R = FF_RATE_STEPS_DEFAULT;
    *ppm = FF_RATE_PPM_DEFAULT;
    *given = 0;
    *residual = 0.0;
    if (!cfg) return PDT_OK;
    if (cfg->rate_steps < 0 || cfg->rate_steps > FF_RATE_STEPS_MAX) return PDT_ERR_ARG;
    if (cfg->rate_steps || (cfg->zero_mask & PDT_FF_ZERO_RATE_STEPS)) *R = cfg->rate_steps;
    if (!(std::isfinite(cfg->rate_step_ppm) && cfg->rate_step_ppm >= 0.0)) return PDT_ERR_ARG;
    if (cfg->rate_step_ppm != 0.0) *ppm = cfg->rate_step_ppm;
    if ((double)*R * *ppm * 1e-6 > FF_RATE_SPAN_MAX) return PDT_ERR_ARG;
    if (cfg->flags & ~(uint32_t)PDT_FF_RESIDUAL_GIVEN) return PDT_ERR_ARG;
    if (cfg->flags & PDT_FF_RESIDUAL_GIVEN) {
        if (!(std::isfinite(cfg->residual_hz) && fabs(cfg->residual_hz) < 0.5 * (double)rate)) return PDT_ERR_ARG;
        *given = 1;
        *residual = cfg->residual_hz;
    }
    return PDT_OK;
}

}  // namespace pdtrt

// the rule on the host: v (L pairs) -> winner, bits, soft values and sample indices (room for ff_halves(L, 0, P_{-R}) / 2 of each)
static void ff_host(const float *v, long long L, int H, int R, double ppm, FfSync *sync, std::vector<unsigned char> &bits, std::vector<float> &soft,
                    std::vector<long long> &index)
{
    unsigned long long bm = 0;
    int br = 0, bt = 0;
    bool any = false;
    for (int r = -R; r <= R; r++) {
        const long long P = ff_period(H, r, ppm);
        for (int tau = 0; tau < 2 * H; tau++) {
            const long long nb = ff_halves(L, tau, P) >> 1;
            unsigned long long M = 0;
            for (long long m = 0; m < nb; m++) M += ff_quant(ff_bit(v, tau, P, m));
            if (!any || ff_before(M, r, tau, bm, br, bt)) {
                bm = M;
                br = r;
                bt = tau;
                any = true;
            }
        }
    }
    const long long P = ff_period(H, br, ppm), nb = ff_halves(L, bt, P) >> 1;
    bits.resize((size_t)nb);
    soft.resize((size_t)nb);
    index.resize((size_t)nb);
    for (long long m = 0; m < nb; m++) {
        const float d = ff_bit(v, bt, P, m);
        bits[(size_t)m] = d > 0.0f ? '1' : '0';
        soft[(size_t)m] = ff_soft(d);
        index[(size_t)m] = bt + ff_bound(2 * m + 2, P);
    }
    sync->tau = bt;
    sync->rate = br;
    sync->period = P;
    sync->metric = bm;
    sync->nbits = (uint64_t)nb;
}

extern "C" {

int pdt_host_ff_mix(uint32_t rate, double residual_hz, const float *iq, uint64_t n, float *out)
{
    if (rate == 0 || ((!iq || !out) && n) || !(std::isfinite(residual_hz) && fabs(residual_hz) < 0.5 * (double)rate)) return PDT_ERR_ARG;
    float tab[2 * AN_TAB];
    analytic_table(tab);
    const uint32_t step = ddc_step((double)rate, residual_hz);
    for (uint64_t i = 0; i < n; i++) ddc_mix(iq[2 * i], iq[2 * i + 1], (uint32_t)i * step, tab, out[2 * i], out[2 * i + 1]);
    return PDT_OK;
}

int pdt_host_ff_bits(uint32_t rate, const float *iq, uint64_t n, const pdt_ff_cfg *cfg, pdt_ff_sync *sync, uint8_t *bits, float *soft, int64_t *index,
                     uint64_t cap, uint64_t *count)
{
    int H, R, given;
    double ppm, residual;
    if ((!iq && n) || !sync || !count || pdtrt::ff_plan(cfg, rate, &H, &R, &ppm, &given, &residual)) return PDT_ERR_ARG;
    try {
        FfSync s;
        memset(&s, 0, sizeof s);
        s.tone_valid = given;
        if (!given) {
            pdt_tone t;
            int got = 0;
            if (pdt_host_tones(rate, 0.0, iq, n, nullptr, &t, 1, &got) == PDT_OK && got == 1 && t.valid) {
                residual = t.residual_hz;
                s.tone_valid = 1;
            }
        }
        const long long L = (long long)std::min<uint64_t>(n, 2ull * rate);
        std::vector<float> v((size_t)(2 * L) + 2);
        const int rc = pdt_host_ff_mix(rate, residual, iq, (uint64_t)L, v.data());
        if (rc) return rc;
        s.residual_hz = residual;
        s.step = ddc_step((double)rate, residual);
        std::vector<unsigned char> b;
        std::vector<float> d;
        std::vector<long long> at;
        ff_host(v.data(), L, H, R, ppm, &s, b, d, at);
        memcpy(sync, &s, sizeof s);
        const size_t k = (size_t)std::min<uint64_t>(cap, b.size());
        if (bits && k) memcpy(bits, b.data(), k);
        if (soft && k) memcpy(soft, d.data(), k * sizeof(float));
        if (index && k) memcpy(index, at.data(), k * sizeof(int64_t));
        *count = b.size();
    } catch (const std::exception &) { return PDT_ERR_NOMEM; }
    return PDT_OK;
}

}  // extern "C"
