// pdt_ddc.hip -- the digital down-converter of wideband captures (pdt_ddc.h): one kernel per input format, which converts what a
// record (DdcWindow) describes -- a whole capture, a window of one, a piece of a stream -- and its host restatement pdt_host_ddc.
// A unit of its own: the chain's units do not change.
#include <math.h>
#include <string.h>
#include <algorithm>

#include "../../include/pdt.h"
#include "pdt_ddc.h"

namespace pdt {

typedef float f2v __attribute__((ext_vector_type(2)));

// One workgroup takes TO = floor(2048 / D) consecutive outputs of one record.  The (TO + 16) D input samples they reach (the tile
// with its +-8 D halo) go from the load through ddc_mix straight into an LDS image laid out by polyphase branch -- input i' at
// [i' mod D][i' / D], rows of ROWP pairs: 16-byte loads where the record's own address allows them and the tile lies inside the
// samples present, sample by sample in front of the first 16-byte boundary and behind the last whole load, and with zeros outside
// [lo, hi) in the tiles that touch the ends (the first and last tiles, stream pieces).  Then the lanes of a wavefront, one output
// each, read consecutive pairs for every tap (ds_read_b64 without bank conflicts), the tap itself is one broadcast read, and I and
// Q advance in one packed FMA.  Outputs leave as consecutive 8-byte pairs.  Up to four outputs per lane (D < 8) share the tap reads.
constexpr int DDC_TILE = 2048;                                           // input samples of a tile without its halo, at most
constexpr int DDC_VS = DDC_TILE + (2 * DDC_SPAN + 1) * DDC_MAX_DECIM;    // 3136: D ROWP <= D (TO + 17)
constexpr int DDC_HS = 2 * DDC_SPAN * DDC_MAX_DECIM + 4;
constexpr int DDC_TB = 256;                                              // lanes of a workgroup, at most

// the SPV samples of one aligned 16-byte load
template <int FMT> __device__ __forceinline__ void ddc_unpack(const void *src, float2 *dst)
{
    if (FMT == PDT_FMT_WB_F32) {
        const float4 a = *reinterpret_cast<const float4 *>(src);
        dst[0] = make_float2(a.x, a.y);
        dst[1] = make_float2(a.z, a.w);
        return;
    }
    const int4 a = *reinterpret_cast<const int4 *>(src);
    const int w[4] = { a.x, a.y, a.z, a.w };
#pragma unroll
    for (int e = 0; e < 4; e++) {
        if (FMT == PDT_FMT_WB_PCM16) {
            dst[e] = make_float2((float)(short)(w[e] & 0xffff) / 32768.0f, (float)(short)(w[e] >> 16) / 32768.0f);
        } else if (FMT == PDT_FMT_WB_CU8) {
            dst[2 * e] = make_float2(((float)(w[e] & 0xff) - 127.5f) / 128.0f, ((float)((w[e] >> 8) & 0xff) - 127.5f) / 128.0f);
            dst[2 * e + 1] = make_float2(((float)((w[e] >> 16) & 0xff) - 127.5f) / 128.0f, ((float)((w[e] >> 24) & 0xff) - 127.5f) / 128.0f);
        } else {
            dst[2 * e] = make_float2((float)(signed char)(w[e] & 0xff) / 128.0f, (float)(signed char)((w[e] >> 8) & 0xff) / 128.0f);
            dst[2 * e + 1] = make_float2((float)(signed char)((w[e] >> 16) & 0xff) / 128.0f, (float)(signed char)((w[e] >> 24) & 0xff) / 128.0f);
        }
    }
}

// outputs m = t + tb b, b < NB, of one channel's tile: the fmaf chains in ascending k
template <int NB>
__device__ __forceinline__ void ddc_fir(const f2v *__restrict__ vs, const float *__restrict__ hs, int D, int TO, int ROWP, int t, int tb,
                                        long long left, float2 *__restrict__ out)
{
    int mb[NB];
    f2v acc[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) {
        mb[b] = min(t + tb * b, TO - 1);           // (a lane without an output of its own reads inside the image and stores nothing)
        acc[b] = (f2v){ 0.0f, 0.0f };
    }
    for (int qo = 0; qo < 2 * DDC_SPAN; qo++) {
        const float *hq = hs + qo * D;
        const f2v *vq = vs + qo;
        for (int r = 0; r < D; r++) {
            const float h = hq[r];
            const f2v h2 = (f2v){ h, h };
#pragma unroll
            for (int b = 0; b < NB; b++) acc[b] = __builtin_elementwise_fma(h2, vq[r * ROWP + mb[b]], acc[b]);
        }
    }
    {
        const float h = hs[2 * DDC_SPAN * D];
        const f2v h2 = (f2v){ h, h };
#pragma unroll
        for (int b = 0; b < NB; b++) acc[b] = __builtin_elementwise_fma(h2, vs[2 * DDC_SPAN + mb[b]], acc[b]);
    }
#pragma unroll
    for (int b = 0; b < NB; b++) {
        const int m = t + tb * b;
        if (m < TO && m < left) out[m] = make_float2(acc[b][0], acc[b][1]);
    }
}

// Input samples first + j, j = j0 + t, j0 + t + tb, ... < j1, of record w, one by one: scaled, mixed with the phase of their global
// index, and put into the polyphase image at [j mod D][j / D].  EDGE: samples outside [lo, hi) are zeros.
template <int FMT, bool EDGE>
__device__ __forceinline__ void ddc_samples(const DdcWindow &w, long long first, int j0, int j1, int t, int tb, int D, int ROWP,
                                            const float *__restrict__ tab, f2v *__restrict__ vs)
{
    int j = j0 + t;
    int r = j % D, q = j / D;
    const int dr = tb % D, dq = tb / D;
    uint32_t p = (w.g0 + (uint32_t)(unsigned long long)(first + j)) * w.step;
    const uint32_t dp = (uint32_t)tb * w.step;
    for (; j < j1; j += tb) {
        const long long i = first + j;
        float vr = 0.0f, vi = 0.0f;
        if (!EDGE || (i >= w.lo && i < w.hi)) {
            float re, im;
            ddc_load<FMT>(w.x, i, re, im);
            ddc_mix(re, im, p, tab, vr, vi);
        }
        vs[r * ROWP + q] = (f2v){ vr, vi };
        p += dp;
        r += dr;
        q += dq;
        if (r >= D) { r -= D; q++; }
    }
}

// The record of a workgroup's tile: `one` when there is no table (tile_win == nullptr: a whole capture or a stream piece, blockIdx.x
// walks its tiles), else wins[tile_win[blockIdx.x]] (the windows of pdt_demod_windows_device: blockIdx.x walks the tiles of all of
// them).  taps: 16 D + 1 floats.  TO = floor(2048 / D), ROWP = (TO + 16) | 1.
template <int FMT>
__global__ void __launch_bounds__(DDC_TB) k_ddc(const DdcWindow one, const DdcWindow *__restrict__ wins, const int *__restrict__ tile_win, int D,
                                                int TO, int ROWP, const float *__restrict__ taps, const float *__restrict__ tab)
{
    __shared__ __attribute__((aligned(16))) f2v vs[DDC_VS];
    __shared__ float hs[DDC_HS];
    const int t = threadIdx.x, tb = blockDim.x;
    const DdcWindow w = tile_win ? wins[tile_win[blockIdx.x]] : one;
    const long long m0 = (long long)((int)blockIdx.x - w.tile0) * TO;
    const long long first = (m0 - DDC_SPAN) * D;                   // the record's input sample at image place 0
    const int len = (TO + 2 * DDC_SPAN) * D;                       // <= 2048 + 16 D; its image D ROWP <= DDC_VS
    constexpr int BPS = DdcFmt<FMT>::BPS, SPV = DdcFmt<FMT>::SPV;
    for (int j = t; j <= 2 * DDC_SPAN * D; j += tb) hs[j] = taps[j];
    if (first >= w.lo && first + len <= w.hi) {
        const unsigned char *src = reinterpret_cast<const unsigned char *>(w.x) + first * BPS;
        int head = (int)(((16 - ((uintptr_t)src & 15)) & 15) / BPS);      // samples in front of the first 16-byte boundary
        if (((uintptr_t)src & 15) % BPS) head = len;                       // (never aligned: sample by sample)
        head = min(head, len);
        const int nvec = (len - head) / SPV;
        ddc_samples<FMT, false>(w, first, 0, head, t, tb, D, ROWP, tab, vs);
        int j = head + t * SPV;
        int r = j % D, q = j / D;
        const int dr = (tb * SPV) % D, dq = (tb * SPV) / D;
        for (int v = t; v < nvec; v += tb) {
            float2 s[SPV];
            ddc_unpack<FMT>(src + (size_t)head * BPS + (size_t)v * 16, s);
            uint32_t p = (w.g0 + (uint32_t)(unsigned long long)(first + j)) * w.step;
            int re = r, qe = q;
#pragma unroll
            for (int e = 0; e < SPV; e++) {
                float vr, vi;
                ddc_mix(s[e].x, s[e].y, p, tab, vr, vi);
                vs[re * ROWP + qe] = (f2v){ vr, vi };
                p += w.step;
                if (++re == D) { re = 0; qe++; }
            }
            j += tb * SPV;
            r += dr;
            q += dq;
            if (r >= D) { r -= D; q++; }
        }
        ddc_samples<FMT, false>(w, first, head + nvec * SPV, len, t, tb, D, ROWP, tab, vs);
    } else {
        ddc_samples<FMT, true>(w, first, 0, len, t, tb, D, ROWP, tab, vs);
    }
    __syncthreads();
    const long long left = w.n_out - m0;
    float2 *out = reinterpret_cast<float2 *>(w.out) + m0;
    if (t < TO) {
        switch ((TO + tb - 1) / tb) {
        case 1: ddc_fir<1>(vs, hs, D, TO, ROWP, t, tb, left, out); break;
        case 2: ddc_fir<2>(vs, hs, D, TO, ROWP, t, tb, left, out); break;
        case 3: ddc_fir<3>(vs, hs, D, TO, ROWP, t, tb, left, out); break;
        default: ddc_fir<4>(vs, hs, D, TO, ROWP, t, tb, left, out); break;
        }
    }
}

}  // namespace pdt

using namespace pdt;

namespace pdtrt {

// k_ddc over `tiles` tiles: of record `one` when table_dev is null, else of the `count` records of the table
static hipError_t ddc_go(hipStream_t st, int fmt, int decim, const float *taps_dev, const float *tab_dev, long long tiles, const DdcWindow &one,
                         const void *table_dev, int count)
{
    if (tiles <= 0) return hipSuccess;
    if (decim < DDC_MIN_DECIM || decim > DDC_MAX_DECIM || !ddc_fmt(fmt)) return hipErrorInvalidValue;
    const int TO = DDC_TILE / decim, ROWP = (TO + 2 * DDC_SPAN) | 1;
    const int tb = std::min(DDC_TB, (TO + 63) / 64 * 64);
    if (tiles > 0xffffffffLL / tb) return hipErrorInvalidValue;        // (a grid's lanes must number less than 2^32)
    const DdcWindow *wins = reinterpret_cast<const DdcWindow *>(table_dev);
    const int *tile_win = table_dev ? reinterpret_cast<const int *>(wins + count) : nullptr;
    const dim3 grid((unsigned)tiles);
#define PDT_DDC_GO(F) hipLaunchKernelGGL(k_ddc<F>, grid, dim3(tb), 0, st, one, wins, tile_win, decim, TO, ROWP, taps_dev, tab_dev)
    switch (fmt) {
    case PDT_FMT_WB_PCM16: PDT_DDC_GO(PDT_FMT_WB_PCM16); break;
    case PDT_FMT_WB_F32: PDT_DDC_GO(PDT_FMT_WB_F32); break;
    case PDT_FMT_WB_CU8: PDT_DDC_GO(PDT_FMT_WB_CU8); break;
    default: PDT_DDC_GO(PDT_FMT_WB_CS8); break;
    }
#undef PDT_DDC_GO
    return hipGetLastError();
}

// The per-call table of many records, as the host builds it: win[i]'s fields are the caller's but .tile0, which is filled in here;
// `table` receives the records and behind them the tiles' records.  Returns the number of tiles, -1 when they are more than a
// launch takes.
long long ddc_windows_table(int decim, DdcWindow *win, int count, std::vector<unsigned char> &table)
{
    const long long TO = DDC_TILE / decim, most = 0xffffffffLL / DDC_TB;
    long long tiles = 0;
    for (int i = 0; i < count; i++) {
        if (tiles > most) return -1;
        win[i].tile0 = (int)tiles;
        tiles += (win[i].n_out + TO - 1) / TO;
    }
    if (tiles > most) return -1;
    table.resize((size_t)count * sizeof(DdcWindow) + (size_t)tiles * sizeof(int));
    if (count) memcpy(table.data(), win, (size_t)count * sizeof(DdcWindow));
    int *tile_win = reinterpret_cast<int *>(table.data() + (size_t)count * sizeof(DdcWindow));
    for (int i = 0; i < count; i++) {
        const long long nt = (win[i].n_out + TO - 1) / TO;
        for (long long k = 0; k < nt; k++) tile_win[win[i].tile0 + k] = i;
    }
    return tiles;
}

// the kernel over a table that is on the device: `count` records, `tiles` tiles, one launch
hipError_t ddc_windows_launch(hipStream_t st, int fmt, int decim, const float *taps_dev, const float *tab_dev, const void *table_dev, int count,
                              long long tiles)
{
    if (count <= 0) return hipSuccess;
    return ddc_go(st, fmt, decim, taps_dev, tab_dev, tiles, DdcWindow(), table_dev, count);
}

// the kernel over one record, passed by value: no table, no copy, nothing waited for
hipError_t ddc_launch(hipStream_t st, int fmt, int decim, const float *taps_dev, const float *tab_dev, DdcWindow w)
{
    const long long TO = DDC_TILE / std::max(decim, 1);
    w.tile0 = 0;
    return ddc_go(st, fmt, decim, taps_dev, tab_dev, (w.n_out + TO - 1) / TO, w, nullptr, 0);
}

}  // namespace pdtrt

template <int FMT> static void host_ddc(const void *x, long long n, int D, uint32_t step, const float *taps, const float *tab, float *out)
{
    std::vector<float> v((size_t)(2 * n));
    for (long long i = 0; i < n; i++) {
        float re, im;
        ddc_load<FMT>(x, i, re, im);
        ddc_mix(re, im, (uint32_t)(unsigned long long)i * step, tab, v[(size_t)(2 * i)], v[(size_t)(2 * i + 1)]);
    }
    const long long n_out = (n + D - 1) / D, span = (long long)DDC_SPAN * D;
    for (long long m = 0; m < n_out; m++) {
        float ar = 0.0f, ai = 0.0f;
        for (long long k = -span; k <= span; k++) {
            const long long i = m * D + k;
            const float h = taps[k + span];
            const float vr = (i >= 0 && i < n) ? v[(size_t)(2 * i)] : 0.0f, vi = (i >= 0 && i < n) ? v[(size_t)(2 * i + 1)] : 0.0f;
            ar = fmaf(h, vr, ar);
            ai = fmaf(h, vi, ai);
        }
        out[2 * m] = ar;
        out[2 * m + 1] = ai;
    }
}

extern "C" int pdt_host_ddc(uint32_t in_rate, int decim, double offset_hz, const void *x, uint64_t n, int sample_format, float *out)
{
    if (in_rate == 0 || decim < DDC_MIN_DECIM || decim > DDC_MAX_DECIM || !ddc_fmt(sample_format) || ((!x || !out) && n)) return PDT_ERR_ARG;
    if (!(isfinite(offset_hz) && fabs(offset_hz) < 0.5 * (double)in_rate)) return PDT_ERR_ARG;
    const std::vector<float> taps = ddc_taps(decim);
    float tab[2 * AN_TAB];
    analytic_table(tab);
    const uint32_t step = ddc_step((double)in_rate, offset_hz);
    switch (sample_format) {
    case PDT_FMT_WB_PCM16: host_ddc<PDT_FMT_WB_PCM16>(x, (long long)n, decim, step, taps.data(), tab, out); break;
    case PDT_FMT_WB_F32: host_ddc<PDT_FMT_WB_F32>(x, (long long)n, decim, step, taps.data(), tab, out); break;
    case PDT_FMT_WB_CU8: host_ddc<PDT_FMT_WB_CU8>(x, (long long)n, decim, step, taps.data(), tab, out); break;
    default: host_ddc<PDT_FMT_WB_CS8>(x, (long long)n, decim, step, taps.data(), tab, out); break;
    }
    return PDT_OK;
}
