"""The oracle's own transcendental restatements against the container's glibc (bit equality)."""
import ctypes as C
import ctypes.util

import numpy as np

libm = C.CDLL(ctypes.util.find_library("m"))
libm.sincosf.argtypes = [C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
libm.sincosf.restype = None
libm.hypotf.argtypes = [C.c_float, C.c_float]
libm.hypotf.restype = C.c_float


def bits(x):
    return np.float32(x).view(np.uint32)


def test_sincosf_matches_glibc_bitwise(orc):
    L = orc.lib()
    rng = np.random.default_rng(0)
    xs = np.concatenate([
        rng.uniform(-2 * np.pi, 2 * np.pi, 200000),
        rng.uniform(-1e-3, 1e-3, 20000),
        np.linspace(-6.2832, 6.2832, 100001),
        np.array([0.0, 0.1, -0.1, 0.785398, 0.7853982, 2.4e-4, 2.5e-4, 6.2831855, -6.2831855, 3.1415927]),
    ]).astype(np.float32)
    s1, c1, s2, c2 = C.c_float(), C.c_float(), C.c_float(), C.c_float()
    bad = 0
    for x in xs:
        L.orc_sincosf(float(x), C.byref(s1), C.byref(c1))
        libm.sincosf(float(x), C.byref(s2), C.byref(c2))
        if bits(s1.value) != bits(s2.value) or bits(c1.value) != bits(c2.value):
            bad += 1
    assert bad == 0, f"{bad} of {len(xs)} arguments differ from this machine's glibc sincosf (FMA ifunc variant expected)"


def test_hypotf_matches_glibc_bitwise(orc):
    L = orc.lib()
    rng = np.random.default_rng(1)
    a = (rng.integers(-32768, 32768, 100000) / 32768.0).astype(np.float32)
    b = (rng.integers(-32768, 32768, 100000) / 32768.0).astype(np.float32)
    for x, y in zip(a, b):
        assert bits(L.orc_hypotf(float(x), float(y))) == bits(libm.hypotf(float(x), float(y)))


def test_q_rsqrt_and_arctan2_known_values(orc):
    """The oracle's Q_rsqrt and arctan2 (oracle_math.c) equal the numpy transcriptions of CarrierTrackingPLL.c:15-52
    (tests/math_models.py) bit for bit, on samples of the sets the GPU tests use (tests/test_gpu_math.py) with all their edge
    inputs: every 9 700th positive float pattern, the coarse int16 grid's a^2 + b^2, +0; the int16 corner grid, the degenerate
    pairs and 60 000 random ones; and, as before, the known values to 1e-6: an anchor that is not a transcription."""
    import math_models as mm
    L = orc.lib()
    # anchors outside the project's own transcriptions: two Newton steps of the 0x5f3759df seed are within 5e-6 relative of
    # 1 / sqrt(x); the rational approximation is exact at the octant centres and odd in y
    assert abs(L.orc_q_rsqrt(4.0) - 0.5) < 1e-5 and abs(L.orc_q_rsqrt(0.25) - 2.0) < 1e-4
    assert abs(L.orc_arctan2_f32(1.0, 1.0) - np.pi / 4) < 1e-6 and abs(L.orc_arctan2_f32(1.0, -1.0) - 3 * np.pi / 4) < 1e-6
    assert L.orc_arctan2_f32(-1.0, 1.0) == -L.orc_arctan2_f32(1.0, 1.0) and abs(L.orc_arctan2_f32(0.0, 1.0)) < 1e-6
    L.orc_arctan2_f64.argtypes = [C.c_double, C.c_double]
    L.orc_arctan2_f64.restype = C.c_double
    x = mm.q_rsqrt_set()
    x = np.concatenate([x[::100], x[-65538::7], np.array([4.0, 0.25, 0.0], np.float32)])
    got = np.array([L.orc_q_rsqrt(float(v)) for v in x], dtype=np.float32)
    assert got.tobytes() == mm.q_rsqrt(x).tobytes()
    for T, f in ((np.float32, L.orc_arctan2_f32), (np.float64, L.orc_arctan2_f64)):
        yx = mm.arctan2_set(T)
        free = np.nonzero(np.arange(len(yx)) % 33 == 0)[0]
        keep = np.concatenate([np.arange(0, 258064, 3), free[free >= 258064][:60000], np.arange(len(yx) - 12000, len(yx))])
        yx = np.concatenate([yx[keep], np.array([[1, 1], [1, -1], [-1, 1], [0, 1]], dtype=T)])
        got = np.array([f(float(y), float(v)) for y, v in yx], dtype=T)
        assert got.tobytes() == mm.arctan2(yx[:, 0], yx[:, 1]).tobytes()


def test_unwrap_f32_exhaustive():
    """The HIP PLL kernels evaluate the reference's (float)((double)x -+ 2*M_PI) wrap
    (CarrierTrackingPLL.c:169-172,183-186) in f32 as (x - hi) + d, hi = (float)(2pi), d = (float)(hi - 2pi).
    Compare the two forms for every float with pi <= |x| <= 13 (the PLL never wraps a larger value)."""
    two_pi = 2.0 * np.pi
    hi = np.float32(two_pi)
    d = np.float32(np.float64(hi) - two_pi)
    assert float(hi) == 6.2831854820251465 and float(d) == 1.7484555314695172e-07
    lo_u = int(np.float32(np.pi).view(np.uint32))
    hi_u = int(np.float32(13.0).view(np.uint32))
    step = 1 << 22
    for u0 in range(lo_u, hi_u + 1, step):
        x = np.arange(u0, min(u0 + step, hi_u + 1), dtype=np.uint32).view(np.float32)
        ref = (x.astype(np.float64) - two_pi).astype(np.float32)
        emu = (x - hi) + d
        assert emu.dtype == np.float32
        assert np.array_equal(ref.view(np.uint32), emu.view(np.uint32))
        xn = -x
        refn = (xn.astype(np.float64) + two_pi).astype(np.float32)
        emun = (xn + hi) - d
        assert np.array_equal(refn.view(np.uint32), emun.view(np.uint32))


def test_agc_calm_batch_needs_no_conditional():
    """The GPU's AGC walkers replace the exact step (AGC.c:98-131: rate select, two range clamps) by
    gain -= (|x*gain| - 1) * decay over 16-sample batches that pass agc_calm (csrc/pdt_kernels_front.h): every |x| <= 1,
    gain in [2.5, 4000] at the start of the batch, decay <= 0.04.  DESIGN 4 gives the argument; this replays both
    forms in float32 on 400 000 random calm batches (edge values included) and demands identical bits, and that no
    conditional of the exact step ever acts."""
    rng = np.random.default_rng(7)
    nb = 400_000
    f32 = np.float32
    gain = np.exp(rng.uniform(np.log(2.5), np.log(4000.0), nb)).astype(f32)
    gain[:2000] = f32(2.5)
    gain[2000:4000] = f32(4000.0)
    decay = np.exp(rng.uniform(np.log(1e-5), np.log(0.04), nb)).astype(f32)
    decay[:1000] = f32(0.04)
    attack = (decay * f32(0.5)).astype(f32)
    x = rng.uniform(-1.0, 1.0, (16, nb)).astype(f32)
    x[:, 4000:6000] = f32(1.0)
    x[:, 6000:8000] = f32(-1.0)
    x[:, 8000:9000] = f32(0.0)
    x[rng.integers(0, 16, 5000), rng.integers(0, nb, 5000)] = f32(1.0)
    g_exact, g_calm = gain.copy(), gain.copy()
    acted = np.zeros(nb, dtype=bool)
    for i in range(16):
        # exact step (float32 at every operation, as the reference compiled for floats)
        y = (x[i] * g_exact).astype(f32)
        err = (np.abs(y) - f32(1.0)).astype(f32)
        att = np.abs(err) > g_exact
        rate = np.where(att, attack, decay).astype(f32)
        g = (g_exact - (err * rate).astype(f32)).astype(f32)
        low, high = g < f32(0), g > f32(5000)
        acted |= att | low | high
        g = np.where(low, f32(10e-5), g)
        g = np.where(high, f32(5000), g).astype(f32)
        g_exact = g
        # calm step
        yc = (x[i] * g_calm).astype(f32)
        ec = (np.abs(yc) - f32(1.0)).astype(f32)
        g_calm = (g_calm - (ec * decay).astype(f32)).astype(f32)
        assert yc.tobytes() == y.tobytes()
    assert not acted.any()
    assert g_calm.tobytes() == g_exact.tobytes()
    assert g_exact.min() >= 1.3 and g_exact.max() <= 4001.0          # the bounds the argument uses


def test_biased_add_rounding_is_rintf():
    """The Gardner kernels round a sampling instant to its sample index as bits(x + 1.5 * 2^23) - 0x4B400000
    (csrc/pdt_kernels_back.h, rint_index and the emission loop) instead of (unsigned)rintf(x): the same round-to-nearest-even
    for every float in [0, 2^22).  Checked on every half-integer and its float neighbours up to 2^22 and on 20 million
    random values; the median clip equals the reference's two-sided select for every non-NaN error."""
    f32 = np.float32
    halves = (np.arange(0, 1 << 22, dtype=np.float64) + 0.5).astype(f32)
    cand = np.concatenate([halves, np.nextafter(halves, f32(0)), np.nextafter(halves, f32(1e9)),
                           np.arange(0, 1 << 22, dtype=np.float64).astype(f32),
                           np.random.default_rng(3).uniform(0, (1 << 22) - 1, 20_000_000).astype(f32)])
    cand = cand[(cand >= 0) & (cand < f32(1 << 22))]
    biased = (cand + f32(12582912.0)).astype(f32)
    idx = biased.view(np.int32) - np.int32(0x4B400000)
    assert np.array_equal(idx, np.rint(cand).astype(np.int32))
    # clip: med3(err, -lim, lim) against (err > lim) ? lim : ((err < -lim) ? -lim : err)
    lim = f32(0.1)
    err = np.concatenate([np.random.default_rng(4).normal(0, 0.2, 1_000_000).astype(f32),
                          np.array([0.0, -0.0, 0.1, -0.1, np.inf, -np.inf, 1e-45, -1e-45], dtype=f32)])
    sel = np.where(err > lim, lim, np.where(err < -lim, -lim, err)).astype(f32)
    med = np.minimum(np.maximum(err, -lim), lim).astype(f32)          # the median of (err, -lim, lim) for ordered bounds
    assert sel.tobytes() == med.tobytes()
