"""The kernels' scalar primitives on the GPU, one at a time and bit for bit (pdt_device_math, csrc/pdt_probe.hip: one record per lane
through the very function -- or machine-code block -- the kernels call).  References: the C library for the libm restatements
(and pdt_host_math, the x86 compilation of the same source, on the large sets); for everything else the numpy transcriptions of
the reference's expressions in tests/math_models.py, which tests/test_math_models.py checks against their host twins on the CPU.
Every comparison is an equality of bytes; every edge grid asserts how many of its records take the branch it was built for."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

import math_models as mm
from math_models import f32, f64

pytestmark = pytest.mark.gpu

libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
libm.sin.restype = libm.cos.restype = libm.hypot.restype = C.c_double
libm.sin.argtypes = libm.cos.argtypes = [C.c_double]
libm.hypot.argtypes = [C.c_double, C.c_double]
libm.sincos.argtypes = [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
libm.sincosf.argtypes = [C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
libm.hypotf.restype = C.c_float
libm.hypotf.argtypes = [C.c_float, C.c_float]


@pytest.fixture(scope="module")
def dem(pdt):
    with pdt.Demodulator(pdt.MODE_POES, 50000) as d:
        yield d


def same(got, want, what=""):
    got, want = mm.canon(np.ascontiguousarray(got)), mm.canon(np.ascontiguousarray(want))
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got.view(np.uint8).reshape(len(got), -1) != want.view(np.uint8).reshape(len(want), -1)).any(axis=1))[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} records differ, first at {bad[0]}: got {got[bad[0]]!r}, want {want[bad[0]]!r}")


def host(pdt, fn, x, T, two=False):
    a, b = pdt.host_math(fn, np.asarray(x, dtype=f64).reshape(-1))
    return np.stack([a, b], axis=1).astype(T) if two else a.astype(T)[:, None]


def libm_sincos(x):
    out = np.zeros((len(x), 2))
    a, b = C.c_double(), C.c_double()
    for i, v in enumerate(x):
        libm.sincos(v, C.byref(a), C.byref(b))
        out[i] = a.value, b.value
    return out


def libm_sincosf(x):
    out = np.zeros((len(x), 2), dtype=f32)
    a, b = C.c_float(), C.c_float()
    for i, v in enumerate(x):
        libm.sincosf(C.c_float(v), C.byref(a), C.byref(b))
        out[i] = a.value, b.value
    return out


# ---------------------------------------------------------------------------------------------------------- libm restatements
@pytest.mark.parametrize("fn", [0, 1, 2])
def test_double_sincos_sin_cos(pdt, dem, fn):
    """sincos_glibc / sin_glibc / cos_glibc: 60 000 arguments per range and the special points against the C library, 2 M per
    range against the host compilation."""
    small = np.concatenate([mm.range_args(lo, hi, 60000, 11) for lo, hi in mm.DOUBLE_RANGES] + [mm.double_special_points()])
    got = dem.device_math(fn, small)
    if fn == 0:
        want = libm_sincos(small)
    else:
        f = libm.sin if fn == 1 else libm.cos
        want = np.array([f(v) for v in small])[:, None]
    same(got, want, f"fn {fn} against the C library")
    big = np.concatenate([mm.range_args(lo, hi, 2_000_000, 13) for lo, hi in mm.DOUBLE_RANGES])
    same(dem.device_math(fn, big), host(pdt, fn, big, f64, two=fn == 0), f"fn {fn} against the host compilation")


@pytest.mark.parametrize("fn", [3, 6])
def test_sincosf_both_forms(pdt, dem, fn):
    x, sub = mm.sincosf_sets()
    assert (np.abs(x) < f32(2.0 ** -126)).sum() > 16000 and np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()          # denormals of both signs, both zeros
    same(dem.device_math(fn, x), host(pdt, fn, x, f32, two=True), f"fn {fn} against the host compilation")
    same(dem.device_math(fn, sub), libm_sincosf(sub), f"fn {fn} against the C library")


@pytest.mark.parametrize("fn", [4, 5])
def test_hypot(pdt, dem, fn):
    T = f64 if fn == 4 else f32
    small, grid = mm.hypot_sets()
    small, grid = small.astype(T), grid.astype(T)
    assert len(grid) == 65536 * 64
    for xy in (small, grid):
        same(dem.device_math(fn, xy), host(pdt, fn, xy, T), f"fn {fn} against the host compilation")
    for xy in (small[:60000], grid[:60000]):
        if fn == 4:
            want = np.array([libm.hypot(a, b) for a, b in xy])[:, None]
        else:
            want = np.array([libm.hypotf(C.c_float(a), C.c_float(b)) for a, b in xy], dtype=f32)[:, None]
        same(dem.device_math(fn, xy), want, f"fn {fn} against the C library")


# ---------------------------------------------------------------------------------------------------------------------- wraps
@pytest.mark.parametrize("fn", [7, 9])
def test_error_wrap_float(dem, fn, record_property):
    """pll_wrap_error_f32 as the device evaluates it (five instructions of inline assembly) and the generic step's
    ge_pi(x) ? unwrap_2pi(x) : x: every float with 3.0 <= |x| <= 9.5 and the range the wrap leaves alone."""
    x = mm.wrap_error_set()
    ref = mm.wrap_error(x)
    assert (ref != x).sum() > 20_000_000 and (ref == x).sum() > 1_000_000
    same(dem.device_math(fn, x), ref[:, None], f"fn {fn}")


def test_phase_wrap_float(dem, record_property):
    x = mm.wrap_phase_set()
    ref = mm.wrap_phase(x)
    assert (ref != x).sum() > 15_000_000 and (ref == x).sum() > 600_000
    same(dem.device_math(8, x), ref[:, None], "pll_wrap_phase_f32")
    # -0: the header argues that a loop state is never -0 and says that the fused form would return +0 for it.  Recorded, not asserted.
    z = np.array([-0.0], dtype=f32)
    got = dem.device_math(8, z)[0, 0]
    record_property("pll_wrap_phase_f32(-0)", f"device {got!r} (sign bit {int(np.signbit(got))}), reference {mm.wrap_phase(z)[0]!r}")
    print(f"pll_wrap_phase_f32(-0): device sign bit {int(np.signbit(got))}, reference sign bit 1 (documented exception)")


def test_error_wrap_double(dem):
    x = mm.wrap_double_set()
    ref = mm.wrap_error(x)
    assert (ref != x).sum() > 1_000_000 and (ref == x).sum() > 400_000
    same(dem.device_math(10, x), ref[:, None], "double error wrap")


# ---------------------------------------------------------------------------------------------------------- reference helpers
@pytest.mark.parametrize("T,fn", [(f32, 11), (f64, 12)])
def test_arctan2(dem, T, fn):
    yx = mm.arctan2_set(T)
    ref = mm.arctan2(yx[:, 0], yx[:, 1])
    assert len(yx) > 2_250_000 and not np.isnan(ref).any()
    same(dem.device_math(fn, yx), ref[:, None], f"arctan2_ref {T.__name__}")


def test_q_rsqrt(dem):
    x = mm.q_rsqrt_set()
    assert len(x) > 22_000_000
    same(dem.device_math(13, x), mm.q_rsqrt(x)[:, None], "q_rsqrt")


# ---------------------------------------------------------------------------------------------------------------- loop filter
def step_records(T, slow):
    recs, refs, counts = [], [], {}
    for g, (alpha, beta, maxf) in enumerate(mm.gain_sets(T, large=slow)):
        large = slow and g == len(mm.gain_sets(T, large=True)) - 1
        th, ph, fr, kinds = mm.step_states(T, 4_000_000 // len(mm.gain_sets(T)) if not large else 500_000, alpha, beta, maxf, 31 + g)
        p2, f2, ew, pw, cl = mm.pll_step(th, ph, fr, T(alpha), T(beta), T(maxf))
        assert not np.isnan(p2).any() and not np.isnan(f2).any()
        for name, flag in (("error_edge", ew), ("phase_edge", pw)):
            k = kinds[name]
            assert flag[k].sum() >= 20000 and (~flag[k]).sum() >= 20000, (name, int(flag[k].sum()))
            counts[name] = counts.get(name, 0) + int(flag[k].sum())
        assert cl[kinds["rail"]].sum() >= 20000 and kinds["zero"].stop - kinds["zero"].start >= 20000
        counts["rail"] = counts.get("rail", 0) + int(cl[kinds["rail"]].sum())
        if not slow and T == f32:
            assert np.abs(ph.astype(f64) + fr + (float(alpha) + float(beta)) * np.pi).max() < 4 * np.pi - 0.05
        one = np.ones(len(th), dtype=T)
        recs.append(np.stack([th, ph, fr, one * T(alpha), one * T(beta), one * T(maxf)], axis=1))
        refs.append(np.stack([p2, f2], axis=1))
    return np.concatenate(recs), np.concatenate(refs), counts


@pytest.fixture(scope="module")
def float_step_sets():
    return {slow: step_records(f32, slow) for slow in (False, True)}


@pytest.mark.parametrize("fn,slow", [(14, False), (15, True)])
def test_one_step_float(dem, float_step_sets, fn, slow):
    recs, ref, counts = float_step_sets[slow]
    print(f"fn {fn}: {len(recs)} records, branch counts {counts}")
    same(dem.device_math(fn, recs), ref, f"pll_phase_step<float, {slow}>")
    if slow:                                    # the two float variants agree wherever both are defined
        plain = float_step_sets[False][0]
        same(dem.device_math(15, plain), dem.device_math(14, plain), "plain against slow-wrap")


@pytest.mark.parametrize("fn,slow", [(16, False), (17, True)])
def test_one_step_double(dem, fn, slow):
    recs, ref, counts = step_records(f64, slow)
    print(f"fn {fn}: {len(recs)} records, branch counts {counts}")
    same(dem.device_math(fn, recs), ref, f"pll_phase_step<double, {slow}>")


@pytest.mark.parametrize("fn", [18, 19, 20])
def test_four_chained_steps(dem, fn):
    """acq_vec4_asm<false>, acq_vec4_asm<true>, pll_vec4_asm against the model step applied four times, every edge built at each of
    the four positions.  The blocks rely on minf = -maxf (the probe passes -maxf) and on a sweep that is not zero; four_case
    asserts both on the inputs, and the branch counts of every grid (tests/test_math_models.py asserts the same without a GPU)."""
    for g in range(len(mm.gain_sets(f32))):
        recs, ref, counts = mm.four_case(fn, g)
        print(f"fn {fn} gains {g}: {len(recs)} records, branch counts {counts}")
        same(dem.device_math(fn, recs), ref, f"fn {fn}, gain set {g}")


@pytest.mark.parametrize("T,fn", [(f32, 21), (f64, 22)])
@pytest.mark.parametrize("on", [True, False])
def test_sweep_select(dem, T, fn, on):
    recs, ref, counts = mm.sweep_case(T, on)
    print(f"fn {fn} on={on}: {len(recs)} records, {counts}")
    same(dem.device_math(fn, recs), ref, f"pll_sweep_sel {T.__name__} on={on}")


# -------------------------------------------------------------------------------------------------------------------- sampler
@pytest.mark.parametrize("T,fn", [(f32, 23), (f64, 24)])
def test_rint_index(dem, T, fn):
    x, r, counts = mm.rint_case(T)
    print(f"fn {fn}: {counts}")
    I = np.int32 if T == f32 else np.int64
    got = dem.device_math(fn, x)
    same(got[:, 0].view(I), r.astype(I), "rint_index")
    same(got[:, 1], r, "Real::rint")


@pytest.mark.parametrize("T,fn", [(f32, 25), (f64, 26)])
def test_clip_finite(dem, T, fn):
    """float: no NaN in the set (v_med3_f32 is claimed for non-NaN errors only); double: NaN included, the select returns it."""
    recs, ref, counts = mm.clip_case(T)
    print(f"fn {fn}: {counts}")
    same(dem.device_math(fn, recs), ref[:, None], f"clip_finite {T.__name__}")


# ------------------------------------------------------------------------------------------------------------------------ AGC
def test_agc_calm_batches(dem):
    x, g, a, d = mm.agc_calm_set()
    y, g1, acted = mm.agc_batch(x, g, a, d)
    assert not acted.any()
    got = dem.device_math(27, mm.agc_records(x, g, a, d))
    assert (got[:, 0] == 1).all()
    same(got[:, 1:17], y.T, "agc_step")
    same(got[:, 17], g1, "agc_step gain")
    same(got[:, 18:35], got[:, 1:18], "agc_step_calm against agc_step")


def test_agc_batches_that_break_one_condition(dem):
    x, g, a, d, which = mm.agc_violating_set()
    assert np.bincount(which).min() > 70_000
    y, g1, _ = mm.agc_batch(x, g, a, d)
    got = dem.device_math(27, mm.agc_records(x, g, a, d))
    assert (got[:, 0] == 0).all(), np.bincount(which[got[:, 0] != 0])
    same(got[:, 1:17], y.T, "agc_step")
    same(got[:, 17], g1, "agc_step gain")


def test_agc_unrestricted_batches(dem):
    x, g, a, d = mm.agc_free_set()
    y, g1, acted = mm.agc_batch(x, g, a, d)
    assert not np.isnan(y).any() and not np.isnan(g1).any()
    assert min((acted & 1 != 0).sum(), (acted & 2 != 0).sum(), (acted & 4 != 0).sum()) > 1000, np.bincount(acted)
    got = dem.device_math(27, mm.agc_records(x, g, a, d))
    same(got[:, 1:17], y.T, "agc_step")
    same(got[:, 17], g1, "agc_step gain")
