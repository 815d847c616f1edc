"""The numpy models of tests/math_models.py (the references of tests/test_gpu_math.py) against their host twins, on the GPU tests' own
input sets and bit for bit: pdt_host_math for the wraps, arctan2 and Q_rsqrt; the oracle's PLL stream for the loop-filter step and
the sweep, iterated.  A wrong model is caught here, without a GPU.  Every set is also checked for what it was built to reach."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

import math_models as mm
from math_models import f32, f64

libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
libm.sincosf.argtypes = [C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
libm.sincosf.restype = None


def same(a, b):
    return a.dtype == b.dtype and mm.canon(a).tobytes() == mm.canon(b).tobytes()


def test_error_wrap_model_equals_the_host_expression(pdt):
    x = mm.wrap_error_set()
    got, _ = pdt.host_math(9, x.astype(f64))
    ref = mm.wrap_error(x)
    assert same(got.astype(f32), ref)
    assert (ref != x).sum() > 20_000_000 and (ref == x).sum() > 1_000_000          # both branches, every float of the wrapped range
    x = mm.wrap_double_set()
    got, _ = pdt.host_math(10, x)
    ref = mm.wrap_error(x)
    assert same(got, ref)
    assert (ref != x).sum() > 1_000_000 and (ref == x).sum() > 400_000
    # the loop form of the phase wrap is the single correction wherever the plain float step is defined
    p = mm.wrap_phase_set()
    pd = p.astype(f64)
    once = np.where(pd > mm.TWO_PI, (pd - mm.TWO_PI).astype(f32), np.where(pd < -mm.TWO_PI, (pd + mm.TWO_PI).astype(f32), p)).astype(f32)
    assert same(mm.wrap_phase(p), once)
    got, _ = pdt.host_math(8, pd)
    assert same(got.astype(f32), once)


@pytest.mark.parametrize("T,fn", [(f32, 11), (f64, 12)])
def test_arctan2_model_equals_the_host_function(pdt, T, fn):
    yx = mm.arctan2_set(T)
    ref = mm.arctan2(yx[:, 0], yx[:, 1])
    assert not np.isnan(ref).any()
    got, _ = pdt.host_math(fn, yx.astype(f64).reshape(-1))
    assert same(got.astype(T), ref)
    assert len(yx) > 2_250_000 and (yx[:, 1] < 0).sum() > 900_000 and (yx[:, 0] < 0).sum() > 900_000


def test_q_rsqrt_model_equals_the_host_function(pdt):
    x = mm.q_rsqrt_set()
    ref = mm.q_rsqrt(x)
    assert len(x) > 22_000_000 and not np.isnan(ref).any()
    got, _ = pdt.host_math(13, x.astype(f64))
    assert same(got.astype(f32), ref)


def test_step_and_sweep_models_iterated_equal_the_oracles_pll(orc, clip):
    """CarrierTrackPLL over the first 2 500 samples of the clip, sample by sample, with the models of arctan2, Q_rsqrt, the
    loop-filter step and the sweep (the C library's sincosf for the mixer): the PLL output -- it depends on every phase -- must
    be the oracle's, bit for bit.  The sweep gate is open from the first sample."""
    rate, iq = clip
    N = 2500
    o = orc.Oracle(orc.POES, rate, iq[:20000])
    x = o.stage(orc.ST_IQ)[:2 * N].reshape(-1, 2)
    want = o.stage(orc.ST_PLL)[:N]
    Fs = f32(rate)
    aa, ba, at, bt, maxf = mm.loop_constants(f32, rate)
    w = 2.0 * np.pi / float(Fs)
    lock_thr, lsa, avg_alpha = f32(0.08), f32(0.3979 * w), f32(0.00005)
    one = lambda v: np.array([v], dtype=f32)
    alpha, beta = aa, ba
    phase, freq, avg, locksig, sw = one(0.1), one(0.0), one(f32(np.pi / 2.0)), one(0.0), one(f32(0.2 * w))
    locked, swept, turned = False, 0, 0
    out = np.zeros(N, dtype=f32)
    s, c = C.c_float(), C.c_float()
    for i in range(N):
        a, b = x[i:i + 1, 0], x[i:i + 1, 1]
        libm.sincosf(C.c_float(phase[0]), C.byref(s), C.byref(c))
        t_imag, t_real = f32(s.value), f32(c.value)
        cc, d = t_real, -t_imag
        o_re = a * cc - b * d
        o_im = a * d + b * cc
        out[i] = o_im[0]
        ph = mm.arctan2(o_im, o_re)
        avg = (avg.astype(f64) * (1.0 - float(avg_alpha)) + (avg_alpha * np.abs(ph)).astype(f64)).astype(f32)
        phase, freq, _, _, _ = mm.pll_step(mm.arctan2(b, a), phase, freq, alpha, beta, maxf)
        inv = mm.q_rsqrt(a * a + b * b)
        re, im = a * inv, b * inv
        locksig = (locksig.astype(f64) * (1.0 - float(lsa)) + (lsa * (re * t_real + im * t_imag)).astype(f64)).astype(f32)
        if float(np.abs((np.pi / 2.0 - avg.astype(f64)).astype(f32))[0]) < 0.05 and not locked:
            freq, sw, t = mm.sweep(freq, sw, maxf)
            swept += 1
            turned += int(t[0])
        if locksig[0] > lock_thr and not locked:
            locked, alpha, beta = True, at, bt
    assert out.tobytes() == want.tobytes()
    assert swept > 1000                        # the sweep model took part


@pytest.mark.parametrize("T", [f32, f64])
def test_step_sets_reach_their_branches(T):
    """the edge grids of the loop-filter step: how many records the model sends through each branch"""
    for alpha, beta, maxf in mm.gain_sets(T):
        th, ph, fr, kinds = mm.step_states(T, 100_000, alpha, beta, maxf, 21)
        p2, f2, ew, pw, cl = mm.pll_step(th, ph, fr, alpha, beta, maxf)
        assert not np.isnan(p2).any() and not np.isnan(f2).any()
        for name, flag in (("error_edge", ew), ("phase_edge", pw)):
            k = kinds[name]
            assert flag[k].sum() >= 20000 and (~flag[k]).sum() >= 20000, (name, int(flag[k].sum()))
        assert cl[kinds["rail"]].sum() >= 20000 and (~cl[kinds["rail"]]).sum() >= 10000
        assert kinds["zero"].stop - kinds["zero"].start >= 20000
        if T == f32:
            pre = np.abs((ph.astype(f64) + fr + (float(alpha) + float(beta)) * np.pi))
            assert pre.max() < 4 * np.pi - 0.05            # where the one-correction float step is defined


def test_agc_sets_reach_their_branches():
    x, g, a, d = mm.agc_calm_set(50_000)
    y, g1, acted = mm.agc_batch(x, g, a, d)
    yc, gc, _ = mm.agc_batch(x, g, a, d, calm=True)
    assert not acted.any() and y.tobytes() == yc.tobytes() and g1.tobytes() == gc.tobytes()
    x, g, a, d = mm.agc_free_set(100_000)
    y, g1, acted = mm.agc_batch(x, g, a, d)
    assert not np.isnan(y).any() and not np.isnan(g1).any()
    assert min((acted & 1 != 0).sum(), (acted & 2 != 0).sum(), (acted & 4 != 0).sum()) > 1000, np.bincount(acted)


@pytest.mark.parametrize("fn", [18, 19, 20])
def test_four_step_sets_reach_their_branches(fn):
    """the edge grids of the four-step blocks at every position and gain set: four_case asserts each grid's branch count -- the
    error and phase wraps, the clamp or the sweep's turn-round, and the frequency crossing zero at position k (with the gate open:
    the sweep re-signed by the sign of the new frequency wherever the loop gain lets an error do that)"""
    reach = 0
    for g in range(len(mm.gain_sets(f32))):
        _, ref, counts = mm.four_case(fn, g)
        assert not np.isnan(ref).any()
        assert len([k for k in counts if k[0] == "zero_freq"]) == 4
        reach += sum(mm.zero_flip_reachable(mm.gain_sets(f32)[g][1], mm.FOUR_SW0[g], k) for k in range(4))
    assert reach >= 10                  # both acquisition gain sets at all four positions, the tracking sets at the first


@pytest.mark.parametrize("T", [f32, f64])
def test_sweep_rint_and_clip_sets_reach_their_branches(T):
    for on in (True, False):
        _, ref, _ = mm.sweep_case(T, on)
        assert not np.isnan(ref).any()
    mm.rint_case(T)
    _, ref, _ = mm.clip_case(T)
    assert np.isnan(ref).sum() == (1 if T == f64 else 0)
