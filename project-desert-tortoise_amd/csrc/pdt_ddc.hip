// pdt_ddc.hip -- the digital down-converter of wideband captures (pdt_ddc.h): one kernel per input format that reads a tile of
// the wideband capture once and produces that tile's outputs for every channel of the launch, and its host restatement
// pdt_host_ddc.  A unit of its own: the chain's units do not change.
#include <math.h>
#include <string.h>
#include <algorithm>

#include "../../include/pdt.h"
#include "pdt_ddc.h"

namespace pdt {

typedef float f2v __attribute__((ext_vector_type(2)));

// One workgroup takes TO = floor(2048 / D) consecutive outputs of every channel.  The (TO + 16) D input samples they reach (the
// tile with its +-8 D halo) are converted to float pairs while they are read into LDS, once: 16-byte loads where the tile lies
// inside the samples present, sample by sample with zeros outside elsewhere (the first and last tiles, stream pieces).  Then, per
// channel: every lane rotates its share of the tile into a second LDS image laid out by polyphase branch -- input i' at
// [i' mod D][i' / D], rows of ROWP pairs -- so that the lanes of a wavefront, one output each, read consecutive pairs for every tap
// (ds_read_b64 without bank conflicts), the tap itself is one broadcast read, and I and Q advance in one packed FMA.  Outputs leave
// as consecutive 8-byte pairs.  Up to four outputs per lane (D < 8) share the tap reads.
constexpr int DDC_TILE = 2048;                                           // input samples of a tile without its halo, at most
constexpr int DDC_XS = DDC_TILE + 2 * DDC_SPAN * DDC_MAX_DECIM;          // 3072: (TO + 16) D <= 2048 + 16 D
constexpr int DDC_VS = DDC_TILE + (2 * DDC_SPAN + 1) * DDC_MAX_DECIM;    // 3136: D ROWP <= D (TO + 17)
constexpr int DDC_HS = 2 * DDC_SPAN * DDC_MAX_DECIM + 4;
constexpr int DDC_TB = 256;                                              // lanes of a workgroup, at most
constexpr int DDC_KMAX = 16;                                             // channels of one launch

struct DdcChans {
    float2 *out[DDC_KMAX];
    uint32_t step[DDC_KMAX];
    int k;
};

template <int FMT> struct DdcVec;
template <> struct DdcVec<PDT_FMT_WB_PCM16> { enum { SPV = 4 }; };
template <> struct DdcVec<PDT_FMT_WB_F32> { enum { SPV = 2 }; };
template <> struct DdcVec<PDT_FMT_WB_CU8> { enum { SPV = 8 }; };
template <> struct DdcVec<PDT_FMT_WB_CS8> { enum { SPV = 8 }; };

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

// x: input sample i (relative) is x[i], present for lo <= i < hi, zero elsewhere; output m is centred on input m D.  g0: global
// index of input 0.  Every channel's buffer takes n_out pairs.  taps: 16 D + 1 floats.  TO = floor(2048 / D), ROWP = (TO + 16) | 1.
template <int FMT>
__global__ void __launch_bounds__(DDC_TB) k_ddc(const void *__restrict__ x, long long lo, long long hi, long long n_out, unsigned long long g0,
                                                int D, int TO, int ROWP, const float *__restrict__ taps, const float *__restrict__ tab, DdcChans ch)
{
    __shared__ __attribute__((aligned(16))) float2 xs[DDC_XS];
    __shared__ __attribute__((aligned(16))) f2v vs[DDC_VS];
    __shared__ float hs[DDC_HS];
    const int t = threadIdx.x, tb = blockDim.x;
    const long long m0 = (long long)blockIdx.x * TO;
    const long long first = (m0 - DDC_SPAN) * D;                   // input sample of xs[0]
    const int len = (TO + 2 * DDC_SPAN) * D;                       // <= DDC_XS
    constexpr int BPS = FMT == PDT_FMT_WB_PCM16 ? 4 : FMT == PDT_FMT_WB_F32 ? 8 : 2;
    constexpr int SPV = DdcVec<FMT>::SPV;
    for (int j = t; j <= 2 * DDC_SPAN * D; j += tb) hs[j] = taps[j];
    const bool inner = first >= lo && first + len <= hi;
    if (inner) {
        const unsigned char *src = reinterpret_cast<const unsigned char *>(x) + first * BPS;
        int head = (int)(((16 - ((uintptr_t)src & 15)) & 15) / BPS);      // samples in front of the first 16-byte boundary
        if (((uintptr_t)src & 15) % BPS) head = len;                       // (never aligned: sample by sample)
        head = min(head, len);
        const int nvec = (len - head) / SPV;
        for (int j = t; j < head; j += tb) {
            float re, im;
            ddc_load<FMT>(x, first + j, re, im);
            xs[j] = make_float2(re, im);
        }
        for (int v = t; v < nvec; v += tb) {
            float2 s[SPV];
            ddc_unpack<FMT>(src + (size_t)head * BPS + (size_t)v * 16, s);
#pragma unroll
            for (int e = 0; e < SPV; e++) xs[head + v * SPV + e] = s[e];
        }
        for (int j = head + nvec * SPV + t; j < len; j += tb) {
            float re, im;
            ddc_load<FMT>(x, first + j, re, im);
            xs[j] = make_float2(re, im);
        }
    } else {
        for (int j = t; j < len; j += tb) {
            const long long i = first + j;
            float re = 0.0f, im = 0.0f;
            if (i >= lo && i < hi) ddc_load<FMT>(x, i, re, im);
            xs[j] = make_float2(re, im);
        }
    }
    __syncthreads();
    const long long left = n_out - m0;
    const int nb = (TO + tb - 1) / tb;
    const int dr = tb % D, dq = tb / D;
    for (int c = 0; c < ch.k; c++) {
        const uint32_t step = ch.step[c];
        uint32_t p = (uint32_t)(g0 + (unsigned long long)(first + t)) * step;
        const uint32_t dp = (uint32_t)tb * step;
        int r = t % D, q = t / D;
        for (int j = t; j < len; j += tb) {
            const float2 s = xs[j];
            float vr, vi;
            ddc_mix(s.x, s.y, p, tab, vr, vi);
            vs[r * ROWP + q] = (f2v){ vr, vi };
            p += dp;
            r += dr;
            q += dq;
            if (r >= D) { r -= D; q++; }
        }
        __syncthreads();
        float2 *out = ch.out[c] + m0;
        if (t < TO) {
            switch (nb) {
            case 1: ddc_fir<1>(vs, hs, D, TO, ROWP, t, tb, left, out); break;
            case 2: ddc_fir<2>(vs, hs, D, TO, ROWP, t, tb, left, out); break;
            case 3: ddc_fir<3>(vs, hs, D, TO, ROWP, t, tb, left, out); break;
            default: ddc_fir<4>(vs, hs, D, TO, ROWP, t, tb, left, out); break;
            }
        }
        __syncthreads();
    }
}

// Input samples first + j, j = j0 + t, j0 + t + tb, ... < j1, of window w, one by one: scaled, mixed with the phase counted from the
// window's first sample, and put into the polyphase image at [j mod D][j / D].  EDGE: samples outside [0, n) are zeros.
template <int FMT, bool EDGE>
__device__ __forceinline__ void ddc_win_samples(const DdcWindow &w, long long first, int j0, int j1, int t, int tb, int D, int ROWP,
                                                const float *__restrict__ tab, f2v *__restrict__ vs)
{
    int j = j0 + t;
    int r = j % D, q = j / D;
    const int dr = tb % D, dq = tb / D;
    uint32_t p = (uint32_t)(unsigned long long)(first + j) * w.step;
    const uint32_t dp = (uint32_t)tb * w.step;
    for (; j < j1; j += tb) {
        const long long i = first + j;
        float vr = 0.0f, vi = 0.0f;
        if (!EDGE || (i >= 0 && i < w.n)) {
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

// The windows of one capture, a channel each (pdt_demod_windows_device): blockIdx.x walks the tiles of all windows, tile_win[tile] is
// the tile's window, wins[] its record.  A window is a capture of its own: k_ddc's tile geometry on the window's own sample index,
// zeros outside [0, n) whatever the capture holds there.  One channel, so there is no xs stage: a sample goes from the load through
// ddc_mix straight into the polyphase image, then ddc_fir as it is.  16-byte loads where the window's own address allows them and the
// tile lies inside the window, sample by sample in front of the first 16-byte boundary, behind the last whole load, and in the
// tiles that touch the window's ends.
template <int FMT>
__global__ void __launch_bounds__(DDC_TB) k_ddc_windows(const DdcWindow *__restrict__ wins, const int *__restrict__ tile_win, int D, int TO, int ROWP,
                                                        const float *__restrict__ taps, const float *__restrict__ tab)
{
    __shared__ __attribute__((aligned(16))) f2v vs[DDC_VS];
    __shared__ float hs[DDC_HS];
    const int t = threadIdx.x, tb = blockDim.x;
    const DdcWindow w = wins[tile_win[blockIdx.x]];
    const long long m0 = (long long)((int)blockIdx.x - w.tile0) * TO;
    const long long first = (m0 - DDC_SPAN) * D;                   // the window's input sample at image place 0
    const int len = (TO + 2 * DDC_SPAN) * D;                       // <= DDC_XS
    constexpr int BPS = FMT == PDT_FMT_WB_PCM16 ? 4 : FMT == PDT_FMT_WB_F32 ? 8 : 2;
    constexpr int SPV = DdcVec<FMT>::SPV;
    for (int j = t; j <= 2 * DDC_SPAN * D; j += tb) hs[j] = taps[j];
    if (first >= 0 && first + len <= w.n) {
        const unsigned char *src = reinterpret_cast<const unsigned char *>(w.x) + first * BPS;
        int head = (int)(((16 - ((uintptr_t)src & 15)) & 15) / BPS);      // samples in front of the first 16-byte boundary
        if (((uintptr_t)src & 15) % BPS) head = len;                       // (never aligned: sample by sample)
        head = min(head, len);
        const int nvec = (len - head) / SPV;
        ddc_win_samples<FMT, false>(w, first, 0, head, t, tb, D, ROWP, tab, vs);
        int j = head + t * SPV;
        int r = j % D, q = j / D;
        const int dr = (tb * SPV) % D, dq = (tb * SPV) / D;
        for (int v = t; v < nvec; v += tb) {
            float2 s[SPV];
            ddc_unpack<FMT>(src + (size_t)head * BPS + (size_t)v * 16, s);
            uint32_t p = (uint32_t)(unsigned long long)(first + j) * w.step;
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
        ddc_win_samples<FMT, false>(w, first, head + nvec * SPV, len, t, tb, D, ROWP, tab, vs);
    } else {
        ddc_win_samples<FMT, true>(w, first, 0, len, t, tb, D, ROWP, tab, vs);
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

// The per-call table of the windows kernel, as the host builds it: win[i].x, .out, .n and .step are the caller's, .n_out and .tile0
// are filled in here; `table` receives the records and behind them the tiles' windows.  Returns the number of tiles, -1 when they
// are more than a launch takes: a grid's lanes must number less than 2^32, workgroups of up to DDC_TB lanes.
long long ddc_windows_table(int decim, DdcWindow *win, int count, std::vector<unsigned char> &table)
{
    const long long TO = DDC_TILE / decim, most = 0xffffffffLL / DDC_TB;
    long long tiles = 0;
    for (int i = 0; i < count; i++) {
        win[i].n_out = (win[i].n + decim - 1) / decim;
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

// the windows kernel over a table that is on the device: `count` records, `tiles` tiles, one launch
hipError_t ddc_windows_launch(hipStream_t st, int fmt, int decim, const float *taps_dev, const float *tab_dev, const void *table_dev, int count,
                              long long tiles)
{
    if (tiles <= 0 || count <= 0) return hipSuccess;
    if (decim < DDC_MIN_DECIM || decim > DDC_MAX_DECIM || !ddc_fmt(fmt)) return hipErrorInvalidValue;
    const int TO = DDC_TILE / decim, ROWP = (TO + 2 * DDC_SPAN) | 1;
    const int tb = std::min(DDC_TB, (TO + 63) / 64 * 64);
    const DdcWindow *wins = reinterpret_cast<const DdcWindow *>(table_dev);
    const int *tile_win = reinterpret_cast<const int *>(wins + count);
    const dim3 grid((unsigned)tiles);
#define PDT_DDC_GO(F) hipLaunchKernelGGL(k_ddc_windows<F>, grid, dim3(tb), 0, st, wins, tile_win, decim, TO, ROWP, taps_dev, tab_dev)
    switch (fmt) {
    case PDT_FMT_WB_PCM16: PDT_DDC_GO(PDT_FMT_WB_PCM16); break;
    case PDT_FMT_WB_F32: PDT_DDC_GO(PDT_FMT_WB_F32); break;
    case PDT_FMT_WB_CU8: PDT_DDC_GO(PDT_FMT_WB_CU8); break;
    default: PDT_DDC_GO(PDT_FMT_WB_CS8); break;
    }
#undef PDT_DDC_GO
    return hipGetLastError();
}

// the kernel over outputs [0, n_out) of k channels (host side of pdt_api.hip's channel paths)
hipError_t ddc_launch(hipStream_t st, int fmt, const void *x, long long lo, long long hi, unsigned long long n_out, unsigned long long g0,
                      int decim, const float *taps_dev, const float *tab_dev, const uint32_t *steps, void *const *outs, int k)
{
    if (!n_out || k <= 0) return hipSuccess;
    if (decim < DDC_MIN_DECIM || decim > DDC_MAX_DECIM || !ddc_fmt(fmt)) return hipErrorInvalidValue;
    const int TO = DDC_TILE / decim, ROWP = (TO + 2 * DDC_SPAN) | 1;
    const int tb = std::min(DDC_TB, (TO + 63) / 64 * 64);
    const dim3 grid((unsigned)((n_out + (unsigned long long)TO - 1) / (unsigned long long)TO));
    for (int c0 = 0; c0 < k; c0 += DDC_KMAX) {
        DdcChans ch;
        memset(&ch, 0, sizeof ch);
        ch.k = std::min(DDC_KMAX, k - c0);
        for (int c = 0; c < ch.k; c++) {
            ch.out[c] = (float2 *)outs[c0 + c];
            ch.step[c] = steps[c0 + c];
        }
#define PDT_DDC_GO(F) hipLaunchKernelGGL(k_ddc<F>, grid, dim3(tb), 0, st, x, lo, hi, (long long)n_out, g0, decim, TO, ROWP, taps_dev, tab_dev, ch)
        switch (fmt) {
        case PDT_FMT_WB_PCM16: PDT_DDC_GO(PDT_FMT_WB_PCM16); break;
        case PDT_FMT_WB_F32: PDT_DDC_GO(PDT_FMT_WB_F32); break;
        case PDT_FMT_WB_CU8: PDT_DDC_GO(PDT_FMT_WB_CU8); break;
        default: PDT_DDC_GO(PDT_FMT_WB_CS8); break;
        }
#undef PDT_DDC_GO
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
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
