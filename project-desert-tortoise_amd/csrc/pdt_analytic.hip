// pdt_analytic.hip -- the Hilbert front end of real captures (pdt_analytic.h): one streaming stencil kernel per input format,
// and its host restatement pdt_host_analytic.  A unit of its own: the chain's units do not change.
#include <math.h>
#include <string.h>

#include "../../include/pdt.h"
#include "pdt_analytic.h"

namespace pdt {

typedef float f2v __attribute__((ext_vector_type(2)));

// One workgroup of AN_TB lanes turns AN_PER * AN_TB consecutive samples into I,Q pairs.  The tile of x with its +-31 halo is read
// into LDS (16 samples per lane with 16-byte loads where the tile lies inside [lo, hi) and is aligned; sample by sample, zero
// outside, elsewhere); lane t then takes AN_PER consecutive outputs from a register window of AN_PER + 62 samples, two outputs
// per packed FMA; the pairs leave through LDS (the tile's) so that the stores of a wavefront are consecutive.
constexpr int AN_TB = 256, AN_PER = 16, AN_TILE = AN_TB * AN_PER;
constexpr int AN_WIN = AN_PER + 2 * AN_HALF;                    // 78 samples per lane
constexpr int AN_XS = AN_TILE + 64;                              // tile + halo (62), rounded up to whole float4 reads

template <int FMT> __device__ __forceinline__ float an_load(const void *x, long long i)
{
    if (FMT == PDT_FMT_REAL_PCM16) return (float)reinterpret_cast<const int16_t *>(x)[i] / 32768.0f;
    return reinterpret_cast<const float *>(x)[i];
}

// x: sample i of the output is x[i]; x[i] exists for lo <= i < hi (lo <= 0 < n_out <= hi: a halo on either side), zero elsewhere.
// g0: global index of output 0.  out: n_out pairs.
template <int FMT>
__global__ void __launch_bounds__(AN_TB) k_analytic(const void *__restrict__ x, long long lo, long long hi, long long n_out, unsigned long long g0,
                                                    uint32_t step, AnalyticTaps taps, const float *__restrict__ tab, float2 *__restrict__ out)
{
    // the pairs take the tile's place once every lane holds its window (32 KiB of LDS per workgroup: five of them to a CU)
    __shared__ __attribute__((aligned(16))) float2 zs[AN_TILE];
    float *xs = reinterpret_cast<float *>(zs);
    static_assert(AN_XS <= 2 * AN_TILE, "tile and halo fit the pairs' LDS");
    const int t = threadIdx.x;
    const long long base = (long long)blockIdx.x * AN_TILE;
    const long long first = base - AN_HALF;                       // sample of xs[0]
    constexpr int EB = FMT == PDT_FMT_REAL_PCM16 ? 2 : 4;
    const bool inner = first >= lo && first + AN_TILE + 2 * AN_HALF <= hi &&
                       (((uintptr_t)x + (uintptr_t)(base * EB)) & 15) == 0;
    if (inner) {
        // body: 16 samples per lane at xs[31 + 16 t ..]; halo: lanes 0..61
        const unsigned char *src = reinterpret_cast<const unsigned char *>(x) + (base + (long long)AN_PER * t) * EB;
        float v[AN_PER];
        if (FMT == PDT_FMT_REAL_PCM16) {
            const int4 a = reinterpret_cast<const int4 *>(src)[0], b = reinterpret_cast<const int4 *>(src)[1];
            const int w[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
#pragma unroll
            for (int e = 0; e < 8; e++) {
                v[2 * e] = (float)(short)(w[e] & 0xffff) / 32768.0f;
                v[2 * e + 1] = (float)(short)(w[e] >> 16) / 32768.0f;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const float4 a = reinterpret_cast<const float4 *>(src)[e];
                v[4 * e] = a.x; v[4 * e + 1] = a.y; v[4 * e + 2] = a.z; v[4 * e + 3] = a.w;
            }
        }
#pragma unroll
        for (int e = 0; e < AN_PER; e++) xs[AN_HALF + AN_PER * t + e] = v[e];
        if (t < 2 * AN_HALF) {
            const int j = t < AN_HALF ? t : AN_TILE + t;             // left halo xs[0..31), right halo xs[31 + TILE ..)
            xs[j] = an_load<FMT>(x, first + j);
        }
        if (t < AN_XS - AN_TILE - 2 * AN_HALF) xs[AN_TILE + 2 * AN_HALF + t] = 0.0f;
    } else {
        for (int j = t; j < AN_XS; j += AN_TB) {
            const long long i = first + j;
            xs[j] = (j < AN_TILE + 2 * AN_HALF && i >= lo && i < hi) ? an_load<FMT>(x, i) : 0.0f;
        }
    }
    __syncthreads();

    float w[AN_WIN + 2];
#pragma unroll
    for (int e = 0; e < (AN_WIN + 2) / 4; e++) {
        const float4 a = reinterpret_cast<const float4 *>(xs + AN_PER * t)[e];
        w[4 * e] = a.x; w[4 * e + 1] = a.y; w[4 * e + 2] = a.z; w[4 * e + 3] = a.w;
    }
    __syncthreads();
    // Q of outputs (2 m, 2 m + 1): output j sits at w[j + 31]; x[n - k] = w[j + 31 - k], x[n + k] = w[j + 31 + k]
    f2v acc[AN_PER / 2];
#pragma unroll
    for (int m = 0; m < AN_PER / 2; m++) acc[m] = (f2v){ 0.0f, 0.0f };
#pragma unroll
    for (int i = 0; i < AN_NTAP; i++) {
        const int k = 2 * i + 1;
        const f2v h = (f2v){ taps.h[i], taps.h[i] };
#pragma unroll
        for (int m = 0; m < AN_PER / 2; m++) {
            const int j = 2 * m + AN_HALF;
            const f2v d = (f2v){ w[j - k], w[j + 1 - k] } - (f2v){ w[j + k], w[j + 1 + k] };
            acc[m] = __builtin_elementwise_fma(h, d, acc[m]);
        }
    }
    const uint32_t p0 = (uint32_t)(g0 + (unsigned long long)(base + AN_PER * t)) * step;
#pragma unroll
    for (int j = 0; j < AN_PER; j++) {
        float c, s, zr, zi;
        analytic_rot(p0 + (uint32_t)j * step, tab, c, s);
        analytic_mix(w[j + AN_HALF], acc[j >> 1][j & 1], c, s, zr, zi);
        zs[AN_PER * t + j] = make_float2(zr, zi);
    }
    __syncthreads();
    const long long left = n_out - base;
#pragma unroll
    for (int r = 0; r < AN_PER; r++) {
        const int j = r * AN_TB + t;
        if (j < left) out[base + j] = zs[j];
    }
}

}  // namespace pdt

using namespace pdt;

namespace pdtrt {

// the kernel over outputs [0, n_out) (host side of pdt_api.hip's real-input paths)
hipError_t analytic_launch(hipStream_t st, int fmt, const void *x, long long lo, long long hi, unsigned long long n_out, unsigned long long g0,
                           uint32_t step, const float *tab_dev, void *out)
{
    if (!n_out) return hipSuccess;
    static const AnalyticTaps taps = analytic_taps();
    const dim3 grid((unsigned)((n_out + AN_TILE - 1) / AN_TILE));
    if (fmt == PDT_FMT_REAL_PCM16)
        hipLaunchKernelGGL(k_analytic<PDT_FMT_REAL_PCM16>, grid, dim3(AN_TB), 0, st, x, lo, hi, (long long)n_out, g0, step, taps, tab_dev, (float2 *)out);
    else
        hipLaunchKernelGGL(k_analytic<PDT_FMT_REAL_F32>, grid, dim3(AN_TB), 0, st, x, lo, hi, (long long)n_out, g0, step, taps, tab_dev, (float2 *)out);
    return hipGetLastError();
}

}  // namespace pdtrt

extern "C" int pdt_host_analytic(uint32_t sample_rate, double center_hz, const void *x, uint64_t n, int sample_format, float *out)
{
    if (sample_rate == 0 || (sample_format != PDT_FMT_REAL_PCM16 && sample_format != PDT_FMT_REAL_F32) || ((!x || !out) && n))
        return PDT_ERR_ARG;
    if (!(isfinite(center_hz) && center_hz >= 0.0 && center_hz < 0.5 * (double)sample_rate)) return PDT_ERR_ARG;
    const AnalyticTaps taps = analytic_taps();
    float tab[2 * AN_TAB];
    analytic_table(tab);
    const uint32_t step = analytic_step(sample_rate, center_hz);
    auto xv = [&](long long i) -> float {
        if (i < 0 || i >= (long long)n) return 0.0f;
        if (sample_format == PDT_FMT_REAL_PCM16) return (float)reinterpret_cast<const int16_t *>(x)[i] / 32768.0f;
        return reinterpret_cast<const float *>(x)[i];
    };
    for (uint64_t i = 0; i < n; i++) {
        float q = 0.0f;
        for (int t = 0; t < AN_NTAP; t++) {
            const int k = 2 * t + 1;
            const float d = xv((long long)i - k) - xv((long long)i + k);
            q = fmaf(taps.h[t], d, q);
        }
        float c, s;
        analytic_rot((uint32_t)i * step, tab, c, s);
        analytic_mix(xv((long long)i), q, c, s, out[2 * i], out[2 * i + 1]);
    }
    return PDT_OK;
}
