// pdt_probe.hip -- test hook: the scalar primitives the kernels are made of, each evaluated by itself on the device
// (pdt_device_math, include/pdt.h holds the table of codes and record layouts).  One lane takes one record and calls the very
// function the kernels call -- the inlined code of pdt_device_math.h, the device-only forms of pdt_kernels_front.h /
// pdt_kernels_back.h and the two hand-scheduled blocks acq_vec4_asm / pll_vec4_asm -- so that tests/test_gpu_math.py can compare
// every one of them bit for bit with the reference's expression where it can go wrong.  Nothing of the chain launches these kernels.
#include "pdt_rt.h"

namespace pdtrt {

struct ProbeLayout { int elem, nin, nout; };
constexpr ProbeLayout kProbeLayout[PDT_DEVICE_MATH_FNS] = {
    { 8, 1, 2 }, { 8, 1, 1 }, { 8, 1, 1 }, { 4, 1, 2 }, { 8, 2, 1 }, { 4, 2, 1 }, { 4, 1, 2 }, { 4, 1, 1 }, { 4, 1, 1 },      // 0 - 8
    { 4, 1, 1 }, { 8, 1, 1 }, { 4, 2, 1 }, { 8, 2, 1 }, { 4, 1, 1 },                                                           // 9 - 13
    { 4, 6, 2 }, { 4, 6, 2 }, { 8, 6, 2 }, { 8, 6, 2 },                                                                        // 14 - 17
    { 4, 10, 7 }, { 4, 10, 7 }, { 4, 10, 7 },                                                                                  // 18 - 20
    { 4, 4, 2 }, { 8, 4, 2 }, { 4, 1, 2 }, { 8, 1, 2 }, { 4, 2, 1 }, { 8, 2, 1 }, { 4, 19, 35 },                               // 21 - 27
};
template <int FN> struct ProbeElem { using type = typename std::conditional<kProbeLayout[FN].elem == 4, float, double>::type; };

constexpr int PROBE_TB = 256;

// the launch constants of the four-step blocks (scalar-register operands there, as in the kernels)
struct ProbeUniform { float alpha, beta, maxf; };

template <typename T, bool SLOW> __device__ __forceinline__ void probe_step(const T *r, T *o)
{
    T phase = r[1], freq = r[2];
    pll_phase_step<T, SLOW>(r[0], phase, freq, r[3], r[4], r[5], -r[5]);
    o[0] = phase;
    o[1] = freq;
}
template <typename T> __device__ __forceinline__ void probe_sweep(const T *r, T *o)
{
    T fr = r[0], sw = r[1];
    pll_sweep_sel<T>(fr, sw, r[2], -r[2], r[3] != (T)0);
    o[0] = fr;
    o[1] = sw;
}

// one record; `refill` / `slot` / `slot_addr`: FN 20 only (this lane's 16 bytes to fetch, its wavefront's KiB of LDS)
template <int FN, typename E>
__device__ __forceinline__ void probe_one(const E *r, E *o, const ProbeUniform &U, const unsigned char *refill, unsigned slot_addr)
{
    if constexpr (FN == 0) { double s, c; sincos_glibc(r[0], s, c); o[0] = s; o[1] = c; }
    else if constexpr (FN == 1) o[0] = sin_glibc(r[0]);
    else if constexpr (FN == 2) o[0] = cos_glibc(r[0]);
    else if constexpr (FN == 3) { float s, c; sincosf_glibc(r[0], s, c); o[0] = s; o[1] = c; }
    else if constexpr (FN == 4) o[0] = hypot_glibc(r[0], r[1]);
    else if constexpr (FN == 5) o[0] = hypotf_glibc(r[0], r[1]);
    else if constexpr (FN == 6) { float s, c; sincosf_flat(r[0], s, c); o[0] = s; o[1] = c; }
    else if constexpr (FN == 7) o[0] = pll_wrap_error_f32(r[0]);
    else if constexpr (FN == 8) o[0] = pll_wrap_phase_f32(r[0]);
    else if constexpr (FN == 9 || FN == 10) {                      // the error wrap as the generic step selects it
        const E w = unwrap_2pi<E>(r[0]);
        o[0] = PiAbs<E>::ge_pi(r[0]) ? w : r[0];
    }
    else if constexpr (FN == 11 || FN == 12) o[0] = arctan2_ref(r[0], r[1]);
    else if constexpr (FN == 13) o[0] = q_rsqrt(r[0]);
    else if constexpr (FN == 14) probe_step<float, false>(r, o);
    else if constexpr (FN == 15) probe_step<float, true>(r, o);
    else if constexpr (FN == 16) probe_step<double, false>(r, o);
    else if constexpr (FN == 17) probe_step<double, true>(r, o);
    else if constexpr (FN == 18 || FN == 19) {
        Vec16<float> th;
        th.v[0] = r[0]; th.v[1] = r[1]; th.v[2] = r[2]; th.v[3] = r[3];
        float phase = r[4], freq = r[5], sweep = r[6], pb[4];
        acq_vec4_asm<FN == 19>(th, phase, freq, sweep, pb, U.alpha, U.beta, -U.maxf, U.maxf);
        o[0] = pb[0]; o[1] = pb[1]; o[2] = pb[2]; o[3] = pb[3];
        o[4] = phase; o[5] = freq; o[6] = sweep;
    }
    else if constexpr (FN == 20) {
        Vec16<float> th;
        th.v[0] = r[0]; th.v[1] = r[1]; th.v[2] = r[2]; th.v[3] = r[3];
        float freq = r[5], p[4];
        pll_vec4_asm(th, r[4], freq, p, U.alpha, U.beta, -U.maxf, U.maxf, refill, slot_addr);
        ring_wait<0>();                                            // the refill has landed: the slot may be asked for again
        o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; o[3] = p[3];
        o[4] = p[3]; o[5] = freq; o[6] = r[6];
    }
    else if constexpr (FN == 21 || FN == 22) probe_sweep<E>(r, o);
    else if constexpr (FN == 23) { o[0] = __int_as_float(rint_index(r[0])); o[1] = Real<float>::rint(r[0]); }
    else if constexpr (FN == 24) { o[0] = __longlong_as_double((long long)rint_index(r[0])); o[1] = Real<double>::rint(r[0]); }
    else if constexpr (FN == 25 || FN == 26) o[0] = clip_finite(r[0], r[1]);
    else if constexpr (FN == 27) {
        Vec16<float> b[4];
#pragma unroll
        for (int k = 0; k < 16; k++) b[k >> 2].v[k & 3] = r[k];
        AgcParams<float> P;
        P.attack = r[17]; P.decay = r[18]; P.squelch_thr = 0; P.squelch = 0; P.raw_out = nullptr;
        o[0] = agc_calm<float, 4>(b, r[16], P.decay) ? 1.0f : 0.0f;
        float g = r[16];
#pragma unroll
        for (int k = 0; k < 16; k++) o[1 + k] = agc_step(b[k >> 2].v[k & 3], g, P);
        o[17] = g;
        g = r[16];
#pragma unroll
        for (int k = 0; k < 16; k++) o[18 + k] = agc_step_calm(b[k >> 2].v[k & 3], g, P.decay);
        o[34] = g;
    }
}

// 256 lanes a workgroup, grid-stride over the records.  `src` (FN 20): 16 bytes per lane of the launch.
template <int FN>
__global__ void __launch_bounds__(PROBE_TB) k_probe(const void *__restrict__ in, void *__restrict__ out, unsigned long long n, ProbeUniform U,
                                                    const unsigned char *__restrict__ src)
{
    using E = typename ProbeElem<FN>::type;
    constexpr int NIN = kProbeLayout[FN].nin, NOUT = kProbeLayout[FN].nout;
    const unsigned char *refill = nullptr;
    unsigned slot_addr = 0;
    if constexpr (FN == 20) {
        // what pll_phase_range hands the block: this lane's own aligned 16 bytes of global memory, and its wavefront's slot
        // (64 lanes x 16 bytes) as the LDS byte address M0 takes
        __shared__ __attribute__((aligned(16))) unsigned char ring[(PROBE_TB / 64) * PDT_RING_SLOT];
        unsigned char *slot = ring + (threadIdx.x >> 6) * PDT_RING_SLOT;
        slot_addr = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)slot);
        refill = src + ((size_t)blockIdx.x * PROBE_TB + threadIdx.x) * 16;
    }
    const E *x = (const E *)in;
    E *y = (E *)out;
    for (unsigned long long i = (unsigned long long)blockIdx.x * PROBE_TB + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * PROBE_TB) {
        E r[NIN], o[NOUT];
#pragma unroll
        for (int k = 0; k < NIN; k++) r[k] = x[i * NIN + k];
        probe_one<FN, E>(r, o, U, refill, slot_addr);
#pragma unroll
        for (int k = 0; k < NOUT; k++) y[i * NOUT + k] = o[k];
    }
}

template <int FN> hipError_t probe_launch(hipStream_t st, unsigned groups, const void *in, void *out, uint64_t n, ProbeUniform U, const unsigned char *src)
{
    hipLaunchKernelGGL(k_probe<FN>, dim3(groups), dim3(PROBE_TB), 0, st, in, out, (unsigned long long)n, U, src);
    return hipGetLastError();
}

struct ProbeBufs {
    DevBuf in, out, src;
    ~ProbeBufs() { in.release(); out.release(); src.release(); }
};

}  // namespace pdtrt

extern "C" int pdt_device_math_layout(int fn, int *elem_bytes, int *nin, int *nout)
{
    if (fn < 0 || fn >= PDT_DEVICE_MATH_FNS) return PDT_ERR_ARG;
    if (elem_bytes) *elem_bytes = kProbeLayout[fn].elem;
    if (nin) *nin = kProbeLayout[fn].nin;
    if (nout) *nout = kProbeLayout[fn].nout;
    return PDT_OK;
}

// (a test hook: the device buffers are allocated for the call and freed behind it, nothing is kept in the context)
extern "C" int pdt_device_math(pdt_ctx *ctx, int fn, const void *in, uint64_t n, void *out)
{
    if (!ctx || fn < 0 || fn >= PDT_DEVICE_MATH_FNS || n > (1ull << 31)) return PDT_ERR_ARG;
    if (!n) return PDT_OK;
    if (!in || !out) return PDT_ERR_ARG;
    const ProbeLayout L = kProbeLayout[fn];
    ProbeUniform U = { 0, 0, 0 };
    if (fn >= 18 && fn <= 20) {                                      // scalar operands of the blocks: one value per call
        const float *r = (const float *)in;
        U.alpha = r[7]; U.beta = r[8]; U.maxf = r[9];
        for (uint64_t i = 1; i < n; i++)
            if (memcmp(r + i * 10 + 7, r + 7, 3 * sizeof(float)) != 0) return PDT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(ctx->cfg.device));
    const unsigned groups = (unsigned)std::min<uint64_t>((n + PROBE_TB - 1) / PROBE_TB, 8192);
    const size_t in_bytes = (size_t)n * (size_t)L.nin * (size_t)L.elem, out_bytes = (size_t)n * (size_t)L.nout * (size_t)L.elem;
    const size_t src_bytes = (fn == 20) ? (size_t)groups * PROBE_TB * 16 : 0;
    ProbeBufs B;
    if (B.in.ensure(in_bytes) || B.out.ensure(out_bytes) || (src_bytes && B.src.ensure(src_bytes))) return PDT_ERR_NOMEM;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(B.in.p, in, in_bytes, hipMemcpyHostToDevice, st));
    if (src_bytes) HIP_TRY(hipMemsetAsync(B.src.p, 0, src_bytes, st));
    const unsigned char *src = (const unsigned char *)B.src.p;
    hipError_t e = hipErrorInvalidValue;
    switch (fn) {
#define PDT_PROBE_CASE(F) case F: e = probe_launch<F>(st, groups, B.in.p, B.out.p, n, U, src); break;
        PDT_PROBE_CASE(0) PDT_PROBE_CASE(1) PDT_PROBE_CASE(2) PDT_PROBE_CASE(3) PDT_PROBE_CASE(4) PDT_PROBE_CASE(5) PDT_PROBE_CASE(6)
        PDT_PROBE_CASE(7) PDT_PROBE_CASE(8) PDT_PROBE_CASE(9) PDT_PROBE_CASE(10) PDT_PROBE_CASE(11) PDT_PROBE_CASE(12) PDT_PROBE_CASE(13)
        PDT_PROBE_CASE(14) PDT_PROBE_CASE(15) PDT_PROBE_CASE(16) PDT_PROBE_CASE(17) PDT_PROBE_CASE(18) PDT_PROBE_CASE(19) PDT_PROBE_CASE(20)
        PDT_PROBE_CASE(21) PDT_PROBE_CASE(22) PDT_PROBE_CASE(23) PDT_PROBE_CASE(24) PDT_PROBE_CASE(25) PDT_PROBE_CASE(26) PDT_PROBE_CASE(27)
#undef PDT_PROBE_CASE
    }
    HIP_TRY(e);
    HIP_TRY(hipMemcpyAsync(out, B.out.p, out_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PDT_OK;
}
