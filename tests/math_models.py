"""Plain numpy transcriptions of the reference's C expressions for the scalar primitives of the PLL, the sampler and the AGC, and the
input sets they are compared on.  Not the code under test: tests/test_math_models.py checks every model against its host twin
(pdt_host_math, the oracle's helpers, the oracle's PLL stream) on the CPU, tests/test_gpu_math.py compares the device with them.

numpy rounds every float32 / float64 operation once and never fuses two: what "gcc -O2 on x86-64, no contraction" evaluates.
Every model takes arrays of one dtype T (float32 = the POES build, float64 = the ARGOS build) and returns arrays of T."""
import numpy as np

f32, f64 = np.float32, np.float64
PI, TWO_PI = np.pi, 2 * np.pi                      # M_PI, 2*M_PI as doubles
PI_F, TWO_PI_F = f32(np.pi), f32(2 * np.pi)        # (float)pi, (float)(2 pi): both lie above the double constants


# ------------------------------------------------------------------------------------------------------------------ the models
def wrap_error(x):
    """CarrierTrackingPLL.c:168-173: if (d > M_PI) d - 2*M_PI; else if (d < -M_PI) d + 2*M_PI -- the comparison and the
    correction in double, the result narrowed to the sample type."""
    T = x.dtype
    xd = x.astype(f64)
    return np.where(xd > PI, (xd - TWO_PI).astype(T), np.where(xd < -PI, (xd + TWO_PI).astype(T), x)).astype(T)


def wrap_phase(p):
    """CarrierTrackingPLL.c:178-182: while (p > 2*M_PI) p = p - 2.0*M_PI; while (p < -2*M_PI) p = p + 2.0*M_PI."""
    T = p.dtype
    p = p.copy()
    while True:
        hi = p.astype(f64) > TWO_PI
        if not hi.any():
            break
        p[hi] = (p[hi].astype(f64) - TWO_PI).astype(T)
    while True:
        lo = p.astype(f64) < -TWO_PI
        if not lo.any():
            break
        p[lo] = (p[lo].astype(f64) + TWO_PI).astype(T)
    return p


def arctan2(y, x):
    """CarrierTrackingPLL.c:15-40: abs_y = fabs(y) + 1e-10 (a double sum, narrowed by the assignment); the quotient in the sample
    type; coeff - coeff_1 * r in double (the coefficients are double constants), narrowed by the assignment to angle."""
    T = y.dtype
    c1, c2 = 0.78539816339744825, 2.35619449019234475
    with np.errstate(all="ignore"):
        abs_y = (np.abs(y).astype(f64) + 1e-10).astype(T)
        pos = x >= 0
        r = np.where(pos, (x - abs_y) / (x + abs_y), (x + abs_y) / (abs_y - x)).astype(T)
        angle = (np.where(pos, c1, c2) - c1 * r.astype(f64)).astype(T)
    return np.where(y < 0, -angle, angle).astype(T)


def q_rsqrt(x):
    """CarrierTrackingPLL.c:43-52 (always float): the shift on the bit pattern, two Newton steps, every product rounded to float."""
    x = x.astype(f32)
    with np.errstate(all="ignore"):
        xhalf = f32(0.5) * x
        i = np.int32(0x5f3759df) - (x.view(np.int32) >> 1)
        y = i.view(f32)
        y = y * (f32(1.5) - (xhalf * y) * y)
        y = y * (f32(1.5) - (xhalf * y) * y)
    return y


def pll_step(th, phase, freq, alpha, beta, maxf):
    """CarrierTrackingPLL.c:165-188 in the sample type, minf = -maxf: the error wrap, d_freq + d_beta * error,
    (d_phase + d_freq) + d_alpha * error with the unclamped new frequency, the two phase-wrap loops, then the clamp.
    Returns (phase', freq', error wrapped?, phase wrapped?, clamped?)."""
    diff = th - phase
    err = wrap_error(diff)
    f1 = freq + beta * err
    ph = (phase + f1) + alpha * err
    phw = wrap_phase(ph)
    fr = np.where(f1 > maxf, maxf, np.where(f1 < -maxf, -maxf, f1)).astype(th.dtype)
    return phw, fr, err != diff, phw != ph, fr != f1


def sweep(fr, sw, maxf, on=True):
    """CarrierTrackingPLL.c:232-246, the four-way if behind d_freq = d_freq + sweep (minf = -maxf).  Returns (fr', sw', turned?)."""
    f2 = fr + sw
    mag = np.abs(sw)
    rail = (f2 >= maxf) | (f2 <= -maxf)
    s2 = np.where(rail, -sw, np.where(f2 >= 0, mag, -mag)).astype(fr.dtype)
    on = np.broadcast_to(np.asarray(on, dtype=bool), fr.shape)
    return np.where(on, f2, fr).astype(fr.dtype), np.where(on, s2, sw).astype(fr.dtype), rail & on


def pll_four(th4, phase, freq, sw, alpha, beta, maxf, open_gate):
    """The step four times (and, with the gate open, the sweep behind each).  Returns (before[4], after[4], phase', freq',
    sweep', flags) -- before[k] / after[k] = the phase in front of / behind step k: acq_vec4_asm's pb[k] and pll_vec4_asm's p[k];
    flags = per position (error wrapped, phase wrapped, clamped, sweep turned at a rail, sweep re-signed by the sign of the new
    frequency, frequency changed sign over the position)."""
    before, after, flags = [], [], []
    for k in range(4):
        before.append(phase)
        f_in = freq
        phase, freq, ew, pw, cl = pll_step(th4[:, k], phase, freq, alpha, beta, maxf)
        turned = flipped = np.zeros(len(phase), dtype=bool)
        if open_gate:
            s_in = sw
            freq, sw, turned = sweep(freq, sw, maxf)
            flipped = ~turned & (sw != s_in)
        after.append(phase)
        flags.append((ew, pw, cl, turned, flipped, np.signbit(freq) != np.signbit(f_in)))
    return before, after, phase, freq, sw, flags


def clip(e, lim):
    """GardenerClockRecovery.c: (e > lim) ? lim : ((e < -lim) ? -lim : e) -- a NaN passes through."""
    return np.where(e > lim, lim, np.where(e < -lim, -lim, e)).astype(e.dtype)


def agc_batch(x, gain, attack, decay, calm=False):
    """AGC.c:98-131 over the rows of x[16, n] (reference 1.0, max_gain 5000): returns (y[16, n], gain', which conditionals acted: 1 attack rate, 2 the clamp at zero, 4 the clamp at max_gain).
    calm = the three conditionals left out (what agc_step_calm evaluates)."""
    T = x.dtype.type
    y = np.empty_like(x)
    g = gain.copy()
    acted = np.zeros(x.shape[1], dtype=np.int32)
    for i in range(x.shape[0]):
        y[i] = x[i] * g
        err = np.abs(y[i]) - T(1.0)
        att = np.abs(err) > g
        rate = decay if calm else np.where(att, attack, decay).astype(x.dtype)
        g2 = g - err * rate
        low, high = g2 < T(0), g2 > T(5000)
        if not calm:
            acted |= att * 1 + low * 2 + high * 4
            g2 = np.where(low, T(10e-5), g2)
            g2 = np.where(high, T(5000), g2)
        g = g2.astype(x.dtype)
    return y, g, acted


def canon(a):
    """NaNs as one bit pattern (the comparisons are on bytes)."""
    return np.where(np.isnan(a), np.nan, a).astype(a.dtype)


# ------------------------------------------------------------------------------------------------------------ the input sets
def every_float(lo, hi):
    a = np.arange(f32(lo).view(np.uint32), f32(hi).view(np.uint32) + 1, dtype=np.uint32).view(f32)
    return np.concatenate([a, -a])


def around(v, n, dtype):
    """the n values below and the n above v (v itself included once), in dtype"""
    U = np.uint32 if dtype == f32 else np.uint64
    c = int(np.abs(dtype(v)).view(U))
    a = np.arange(c - n, c + n + 1, dtype=U).view(dtype)
    return a if v > 0 else -a


def wrap_error_set():
    """every float with 3.0 <= |x| <= 9.5, 200 000 in (-3.2, 3.2), zeros, tiny values, two floats each side of +-(float)pi"""
    rng = np.random.default_rng(5)
    return np.concatenate([every_float(3.0, 9.5), rng.uniform(-3.2, 3.2, 200000).astype(f32), np.array([0.0, -0.0, 1e-30, -1e-30], f32),
                           around(PI_F, 2, f32), around(-PI_F, 2, f32)])


def wrap_phase_set():
    rng = np.random.default_rng(6)
    return np.concatenate([every_float(6.0, 12.5), rng.uniform(-6.3, 6.3, 200000).astype(f32), np.array([0.0, 1e-30, -1e-30], f32),
                           around(TWO_PI_F, 2, f32), around(-TWO_PI_F, 2, f32)])


def wrap_double_set():
    rng = np.random.default_rng(7)
    return np.concatenate([rng.uniform(-13, 13, 2_000_000)] + [around(s * v, 1000, f64) for s in (1, -1) for v in (PI, TWO_PI)] + [np.array([0.0, -0.0])])


def sincosf_sets():
    """(large, small): the sets of test_branch_free_sincosf_equals_the_library_form plus float denormals (every 1021st pattern, both
    signs) for device == host; a 60 000-value subsample of it for the C library"""
    rng = np.random.default_rng(11)
    dense = rng.uniform(-7.0, 7.0, 400000).astype(f32)
    wide = rng.uniform(-119.9, 119.9, 100000).astype(f32)
    tiny = np.arange(1, 0x39800000 + 0x400000, 9973, dtype=np.uint32).view(f32)
    k = np.arange(-80, 81)
    q = (k * (np.pi / 4)).astype(f32)
    edges = np.concatenate([q, np.nextafter(q, f32(-1000.0)), np.nextafter(q, f32(1000.0)), np.array([0.0, -0.0, 0.5, -0.5, 2.0 ** -12, -(2.0 ** -12)], f32)])
    den = np.arange(1, 0x00800000, 1021, dtype=np.uint32).view(f32)
    x = np.concatenate([dense, wide, tiny, -tiny, edges, den, -den])
    sub = np.concatenate([x[:: max(1, len(x) // 58000)], edges, den[::40], -den[::40]])[:60000]
    return x, sub


DOUBLE_RANGES = [(0.0, 2.0 ** -26), (1e-9, 0.13), (0.12, 0.86), (0.85, 2.43), (2.42, 6.3), (6.28, 60.0), (50.0, 1e5), (1e5, 1e8)]


def range_args(lo, hi, n, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(lo, hi, n)
    x[::2] *= -1
    return x


def double_special_points():
    k = np.arange(0, 900)
    return np.concatenate([k / 128.0, k / 128.0 + 2.0 ** -8, np.nextafter(k / 128.0 + 2.0 ** -8, 0), [0.126, 0.855469, 2.426265, 0.0, -0.0],
                           np.arange(1, 400) * (np.pi / 2), np.arange(1, 400) * f64(f32(np.pi))])


def hypot_sets():
    """(small, grid): the three sets of test_hypot_equals_glibc; all 65 536 x 64 pairs (a, b), a = int16 / 32768"""
    rng = np.random.default_rng(9)
    pcm = rng.integers(-32768, 32768, size=(120000, 2)) / 32768.0
    free = rng.uniform(-1, 1, size=(60000, 2))
    edge = np.array([[0, 0], [0, 0.5], [0.25, 0], [1, 1], [-1, 1e-300], [3e-5, 3e-5], [1.0, 2.0 ** -53]])
    a = np.arange(-32768, 32768) / 32768.0
    b = np.linspace(-32768, 32767, 64).round() / 32768.0
    grid = np.stack([np.repeat(a, 64), np.tile(b, 65536)], axis=1)
    return np.concatenate([pcm, free, edge]), grid


def arctan2_set(T):
    """pairs (y, x): the int16 corner grid, 2 M random pairs of [-1, 1]^2, the degenerate inputs of a RAW float capture"""
    rng = np.random.default_rng(12)
    v = np.unique(np.concatenate([[-32768, -32767, -1, 0, 1, 2, 32766, 32767], rng.integers(-32768, 32768, 500)])) / 32768.0
    grid = np.stack([np.repeat(v, len(v)), np.tile(v, len(v))], axis=1)
    free = rng.uniform(-1, 1, (2_000_000, 2)).astype(f32).astype(f64)
    m = np.concatenate([[0.0, 1e-45, 1e-40, 1.2e-38, 1e-30, 1e-12, 9e-11, 1e-10, 1.1e-10, 1e-5, 0.3, 1.0, 7.5, 1e10, 1e30], rng.uniform(0, 1, 40)])
    m = np.concatenate([m, -m, [-0.0]])
    deg = np.stack([np.repeat(m, len(m)), np.tile(m, len(m))], axis=1)                      # every magnitude against every other, signs and zeros
    yy = np.concatenate([m, m, m, m])                                                      # x = +-|y| exactly: r = 0 or the quotient +-1
    diag = np.stack([yy, np.concatenate([np.abs(m), -np.abs(m), np.abs(m) + 1e-10, -(np.abs(m) + 1e-10)])], axis=1)
    return np.concatenate([grid, free, deg, diag]).astype(T)


def q_rsqrt_set():
    """every 97th positive float from the smallest denormal to FLT_MAX, the a^2 + b^2 of a coarse int16 grid, +0"""
    pat = np.arange(1, 0x7f7fffff + 1, 97, dtype=np.uint32).view(f32)
    a = (np.arange(-32768, 32768, 256) / 32768.0).astype(f32)
    aa, bb = np.meshgrid(a, a)
    return np.concatenate([pat, (aa * aa + bb * bb).astype(f32).reshape(-1), np.array([0.0, 3.4028235e38], f32)])


def loop_constants(T, fs, argos=False):
    """(alpha_acq, beta_acq, alpha_trk, beta_trk, maxf) as make_pll_params (csrc/pdt_rt.h) forms them from the mains' constants
    (POESTIPdemod/main.c:32-46,413, ARGOSdemod/main.c:33-44,265; CarrierTrackingPLL.c:90-91 in the sample type, :272-273 in double)."""
    Fs = T(fs)
    w = 2.0 * np.pi / float(Fs)
    bw_acq = T((16.0 if argos else 127.3240) * w)
    bw_trk = T((16.0 if argos else 10.3451) * w)
    damp, four, one, two = T(0.999), T(4), T(1), T(2)
    den = one + two * damp * bw_acq + bw_acq * bw_acq
    a_acq, b_acq = (four * damp * bw_acq) / den, (four * bw_acq * bw_acq) / den
    dd, db = float(damp), float(bw_trk)
    dend = 1.0 + 2.0 * dd * db + float(bw_trk * bw_trk)
    a_trk, b_trk = T((4.0 * dd * db) / dend), T((4.0 * db * db) / dend)
    maxf = T(2.0 * np.pi * float(T(550.0 if argos else 4500.0)) / float(Fs))
    return T(a_acq), T(b_acq), a_trk, b_trk, maxf


def gain_sets(T, large=False):
    """[(alpha, beta, maxf)]: acquisition and tracking gains at 50 and 250 ksps (POES constants for float, ARGOS' too for double);
    large = one set whose |freq| + (alpha + beta) pi passes 2 pi: the slow-wrap variants only"""
    out = []
    for fs in (50000, 250000):
        for argos in ((False, True) if T == f64 else (False,)):
            aa, ba, at, bt, mf = loop_constants(T, fs, argos)
            out += [(aa, ba, mf), (at, bt, mf)]
    if large:
        out.append((T(1.9), T(1.1), T(2.5)))
    return out


def ulps(v, k):
    """v moved by k units in the last place (arrays, float32 / float64, v != 0)"""
    U = np.int32 if v.dtype == f32 else np.int64
    b = v.view(U)
    return (b + np.where(b < 0, -k, k).astype(U)).view(v.dtype)


def step_states(T, n, alpha, beta, maxf, seed, edges=60000):
    """Records (th, phase, freq) of one loop-filter step: n random states (th in [-pi, pi], phase in (-2 pi, 2 pi], freq in
    [-maxf, maxf]) and `edges` records of each edge kind.  Returns (th, phase, freq, kinds): kinds[name] = slice of the records
    built for that edge."""
    rng = np.random.default_rng(seed)
    alpha, beta, maxf = T(alpha), T(beta), T(maxf)
    th = [rng.uniform(-PI, PI, n).astype(T)]
    ph = [(-rng.uniform(-TWO_PI, TWO_PI, n)).astype(T)]
    fr = [rng.uniform(-float(maxf), float(maxf), n).astype(T)]
    kinds, at = {}, n
    eps = float(np.finfo(T).eps)

    def add(name, t, p, f):
        nonlocal at
        th.append(t.astype(T)); ph.append(p.astype(T)); fr.append(f.astype(T))
        kinds[name] = slice(at, at + len(t))
        at += len(t)

    m = edges
    k = rng.integers(-4, 5, m)
    sgn = np.where(rng.integers(0, 2, m) == 1, 1.0, -1.0)
    # th - phase within +-4 ulp of +-pi: phase = th -+ pi (1 + k 2^-23) (float; the double grid steps by its own epsilon)
    t = rng.uniform(-PI, PI, m).astype(T)
    t = np.where(sgn > 0, np.abs(t), -np.abs(t)).astype(T)                                 # th and the error on one side: |phase| < 2 pi
    p = (t.astype(f64) - sgn * PI * (1.0 + k * eps)).astype(T)
    add("error_edge", t, p, rng.uniform(-float(maxf), float(maxf), m))
    # phase + f1 + alpha e within +-4 ulp of +-2 pi: choose th, freq; solve for phase in double, then take the float next to it
    f = rng.uniform(-float(maxf), float(maxf), m).astype(T)
    e = rng.uniform(-0.5, 0.5, m)
    target = sgn * TWO_PI * (1.0 + k * eps)
    p = ((target - f.astype(f64) - (float(alpha) + float(beta)) * e) ).astype(T)
    t = (p.astype(f64) + e).astype(T)
    add("phase_edge", t, p, f)                                                             # (theta = phase + e passes pi here: the step is defined for any)
    # freq at each rail and one ulp inside, the error pushing outwards and inwards
    rail = np.where(sgn > 0, maxf, -maxf).astype(T)
    f = np.where(rng.integers(0, 2, m) == 1, rail, ulps(rail, -1)).astype(T)
    p = rng.uniform(-3.0, 3.0, m).astype(T)
    t = (p.astype(f64) + sgn * rng.uniform(0.0, 0.1, m) * rng.integers(0, 2, m)).astype(T)
    t[:m // 4] = (p[:m // 4].astype(f64) + sgn[:m // 4] * rng.uniform(0.01, 0.1, m // 4)).astype(T)    # outwards for certain
    add("rail", t, p, f)
    # th = +-0, phase = +0
    t = np.where(rng.integers(0, 2, m) == 1, 0.0, -0.0).astype(T)
    add("zero", t, np.zeros(m, T), rng.uniform(-float(maxf), float(maxf), m))
    return np.concatenate(th), np.concatenate(ph), np.concatenate(fr), kinds


def sweep_set(T, maxf, sw0, n, seed):
    """(fr, sw): n random records, then frequencies within a few sweep steps of each rail and around zero, both signs of the sweep"""
    rng = np.random.default_rng(seed)
    maxf, sw0 = T(maxf), T(sw0)
    m = 20000
    sg = np.where(rng.integers(0, 2, n + 3 * m) == 1, sw0, -sw0).astype(T)
    near = lambda c: (c + rng.integers(-6, 7, m) * float(sw0) * rng.choice([1.0, 0.5, 1.0000001], m)).astype(T)
    fr = np.concatenate([rng.uniform(-float(maxf), float(maxf), n).astype(T), np.clip(near(float(maxf)), -maxf, maxf), np.clip(near(-float(maxf)), -maxf, maxf), near(0.0)])
    fr[n:n + 500] = maxf - sw0
    fr[n + m:n + m + 500] = -maxf + sw0
    fr[n + 2 * m:n + 2 * m + 500] = -sw0
    fr[n + 2 * m + 500:n + 2 * m + 1000] = sw0
    kinds = {"rail": slice(n, n + 2 * m), "zero": slice(n + 2 * m, n + 3 * m)}
    return fr, sg, kinds


def rint_set(T):
    rng = np.random.default_rng(3)
    halves = (np.arange(0, 1 << 22, dtype=f64) + 0.5).astype(T)
    if T == f32:
        c = np.concatenate([halves, np.nextafter(halves, f32(0)), np.nextafter(halves, f32(1e9)), np.arange(0, 1 << 22, dtype=f64).astype(f32),
                            rng.uniform(0, (1 << 22) - 1, 4_000_000).astype(f32)])
        return c[(c >= 0) & (c < f32(1 << 22))]
    return np.concatenate([halves, np.nextafter(halves, 0.0), np.nextafter(halves, 1e9), rng.uniform(0, 2.0 ** 31 - 1, 4_000_000)])


def clip_set(T):
    """(e, lim): 1 M normal(0, 0.2) errors with lim = 0.1, +-0, +-lim, +-inf, +-1e-45; the double form also NaN.  (The float form is
    v_med3_f32, which the sampler uses for errors the stager has seen to be finite: a NaN there gives a bound, not a NaN -- the
    identity is claimed for non-NaN errors only, tests/test_oracle_math.py, so the float set holds none.)"""
    e = np.concatenate([np.random.default_rng(4).normal(0, 0.2, 1_000_000).astype(T), np.array([0.0, -0.0, 0.1, -0.1, np.inf, -np.inf, 1e-45, -1e-45], dtype=T)])
    lim = T(0.1)
    e[-6], e[-5] = lim, -lim
    if T == f64:
        e = np.concatenate([e, [np.nan]])
    return e, np.full(len(e), lim, dtype=T)


def agc_calm_set(nb=400_000):
    """the batches of test_agc_calm_batch_needs_no_conditional: (x[16, nb], gain, attack, decay)"""
    rng = np.random.default_rng(7)
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
    return x, gain, attack, decay


def agc_violating_set(nb=400_000):
    """calm batches with exactly one condition broken each; returns (x, gain, attack, decay, which) -- which: 0 one |x| =
    nextafter(1, 2), 1 gain = nextafter(2.5, 0), 2 gain = nextafter(4000, 1e9), 3 decay = nextafter(0.04, 1), 4 decay = 0"""
    x, gain, attack, decay = agc_calm_set(nb)
    rng = np.random.default_rng(8)
    which = rng.integers(0, 5, nb)
    one = np.nextafter(f32(1), f32(2))
    w0 = np.nonzero(which == 0)[0]
    x[rng.integers(0, 16, len(w0)), w0] = np.where(rng.integers(0, 2, len(w0)) == 1, one, -one)
    gain[which == 1] = np.nextafter(f32(2.5), f32(0))
    gain[which == 2] = np.nextafter(f32(4000), f32(1e9))
    decay[which == 3] = np.nextafter(f32(0.04), f32(1))
    decay[which == 4] = f32(0)
    return x, gain, attack, decay, which


def agc_free_set(nb=400_000):
    """unrestricted batches: gain 1e-4 .. 5000, |x| up to 40 (a third of the batches), so that the attack branch and both clamps act"""
    rng = np.random.default_rng(9)
    gain = np.exp(rng.uniform(np.log(1e-4), np.log(5000.0), nb)).astype(f32)
    gain[:1000] = f32(5000)
    gain[1000:2000] = f32(1e-4)
    decay = np.exp(rng.uniform(np.log(1e-5), np.log(0.5), nb)).astype(f32)
    attack = (decay * rng.choice([0.5, 2.0, 30.0], nb)).astype(f32)
    amp = rng.choice([1.0, 1.0, 40.0], nb)
    x = (rng.uniform(-1.0, 1.0, (16, nb)) * amp).astype(f32)
    x[:, :2000] *= f32(1e-5)                               # a faint input under a gain at the limit: the gain grows into max_gain
    gain[1000:2000] = rng.uniform(4990.0, 5000.0, 1000).astype(f32)
    gain[2000:3000] = f32(1e-4)
    decay[:2000] = f32(0.5)
    return x, gain, attack, decay


def agc_records(x, gain, attack, decay):
    return np.concatenate([x.T, gain[:, None], attack[:, None], decay[:, None]], axis=1).astype(f32)


def four_records(n, alpha, beta, maxf, sw0, open_gate, seed, edges=8000):
    """Records (th0..th3, phase, freq, sweep) of the four-step blocks (float): n random ones, then for each position k of the four
    `edges` records of each edge kind built on the state the model reaches in front of step k (the steps before it see theta =
    phase, a zero error; the steps behind it a random theta): the error at +-pi, the new phase at +-2 pi, the frequency at a rail
    -- with the gate open within a few sweep steps of it, so that the sweep turns round at every position -- and the frequency
    carried across zero by the error of step k (zero_freq).
    Returns (th[n, 4], phase, freq, sweep, kinds): kinds[(name, k)] = slice."""
    rng = np.random.default_rng(seed)
    T = f32
    alpha, beta, maxf, sw0 = T(alpha), T(beta), T(maxf), T(sw0)
    eps = float(np.finfo(T).eps)
    TH, PH, FR, SW, kinds = [], [], [], [], {}
    at = 0

    def add(name, th, ph, fr, sw):
        nonlocal at
        TH.append(th.astype(T)); PH.append(ph.astype(T)); FR.append(fr.astype(T)); SW.append(sw.astype(T))
        if name:
            kinds[name] = slice(at, at + len(ph))
        at += len(ph)

    sgn_sw = lambda m: np.where(rng.integers(0, 2, m) == 1, sw0, -sw0).astype(T)
    add(None, rng.uniform(-PI, PI, (n, 4)), -rng.uniform(-TWO_PI, TWO_PI, n), rng.uniform(-float(maxf), float(maxf), n), sgn_sw(n))
    m = edges
    for k in range(4):
        for name in ("error_edge", "phase_edge", "rail", "zero_freq"):
            sgn = np.where(rng.integers(0, 2, m) == 1, 1.0, -1.0)
            j = rng.integers(-4, 5, m)
            sw = sgn_sw(m)
            fr0 = rng.uniform(-float(maxf), float(maxf), m).astype(T)
            ph0 = rng.uniform(-3.0, 3.0, m).astype(T)
            if name == "phase_edge":
                fr0 = (np.abs(fr0) * sgn).astype(T)
                ph0 = (sgn * TWO_PI - (k + 1) * fr0.astype(f64) + rng.uniform(-0.2, 0.2, m) * (float(alpha) + float(beta))).astype(T)
            if name == "rail":
                rail = np.where(sgn > 0, maxf, -maxf).astype(T)
                fr0 = np.clip(rail - sgn * rng.integers(0, 5, m) * float(sw0) * rng.choice([1.0, 0.5], m), -float(maxf), float(maxf)).astype(T)
                if not open_gate:                                 # no sweep to carry it there: at the rail or one ulp inside
                    fr0 = np.where(rng.integers(0, 2, m) == 1, rail, ulps(rail, -1)).astype(T)
            if name == "zero_freq":                              # open: within 2.5 sweep steps of zero; closed: within beta of it
                fr0 = (sgn * float(sw0) * rng.choice([0.5, 1.5, 2.5], m)).astype(T) if open_gate else (sgn * float(beta) * rng.uniform(0.1, 1.0, m)).astype(T)
            th = rng.uniform(-PI, PI, (m, 4)).astype(T)
            ph, fr, s = ph0.copy(), fr0.copy(), sw.copy()
            for q in range(k):                                    # quiet steps: theta = phase
                th[:, q] = ph
                ph, fr, _, _, _ = pll_step(th[:, q], ph, fr, alpha, beta, maxf)
                if open_gate:
                    fr, s, _ = sweep(fr, s, maxf)
            if name == "error_edge":
                th[:, k] = (ph.astype(f64) + sgn * PI * (1.0 + j * eps)).astype(T)
            elif name == "phase_edge":
                e = (sgn * TWO_PI * (1.0 + j * eps) - ph.astype(f64) - fr.astype(f64)) / (float(alpha) + float(beta))
                th[:, k] = (ph.astype(f64) + np.clip(e, -3.0, 3.0)).astype(T)
            elif name == "zero_freq":
                # the crossing at position k itself, by the error of step k: f1 = freq + beta e lands on the other side of zero --
                # open: beyond -sweep (half of them: the sweep is re-signed by the sign of f2), between 0 and -sweep, or on -sweep
                # exactly (f2 = +0); closed: at -u freq.  (|e| <= 3: where beta is too small for that, zero_flip_reachable says so)
                if open_gate:
                    u = np.where(rng.integers(0, 2, m) == 1, rng.uniform(1.2, 2.0, m), np.where(rng.integers(0, 2, m) == 1, rng.uniform(0.05, 0.9, m), 1.0))
                    target = -s.astype(f64) * u
                else:
                    target = -fr.astype(f64) * rng.uniform(0.2, 1.5, m)
                th[:, k] = (ph.astype(f64) + np.clip((target - fr.astype(f64)) / float(beta), -3.0, 3.0)).astype(T)
            elif name == "rail" and not open_gate:               # two in three pushed outwards by an error the smallest beta still shows
                th[:, k] = (ph.astype(f64) + sgn * rng.uniform(0.5, 2.0, m) * (rng.integers(0, 3, m) > 0)).astype(T)
            else:
                th[:, k] = (ph.astype(f64) + sgn * rng.uniform(0.0, 0.1, m) * rng.integers(0, 2, m)).astype(T)
            add((name, k), th, ph0, fr0, sw)
    return np.concatenate(TH), np.concatenate(PH), np.concatenate(FR), np.concatenate(SW), kinds


def zero_flip_reachable(beta, sw0, k):
    """Can the error of step k re-sign the sweep at position k of an open block?  In front of step k >= 1 a sweep step has already
    pointed the sweep away from zero (CarrierTrackingPLL.c:243-246) and the frequency lies up to (2.5 + k) sweep steps out; the
    error is wrapped to [-pi, pi], so f1 = freq + beta e comes back beyond -sweep (two steps more) only if 3 beta >= (4.5 + k) |sweep|
    (the records ask for |e| <= 3).  With the mains' tracking gains beta pi is below one sweep step: the branch does not exist
    there behind position 0, for any input.  At position 0 the block's own sweep sign is free: always reachable."""
    return k == 0 or zero_cross_by_error(beta, sw0, k)


def zero_cross_by_error(beta, sw0, k):
    """the gain condition of zero_flip_reachable alone: the error of step k can carry the frequency across zero and beyond -sweep"""
    return 3.0 * float(beta) >= (4.5 + k) * float(sw0)


FOUR_SW0 = [f32(0.2 * (2.0 * np.pi / float(f32(fs)))) for fs in (50000, 50000, 250000, 250000)]      # as the reference starts the sweep, per gain set


def four_case(fn, g):
    """The records of test_four_chained_steps for one function (18 acq_vec4_asm<false>, 19 <true>, 20 pll_vec4_asm) and gain set,
    the model's result for them, and the number of records of every edge grid that take its branch -- asserted here, for the GPU
    test and for its CPU twin.  Returns (records[n, 10], reference[n, 7], counts)."""
    open_gate = fn == 19
    alpha, beta, maxf = gain_sets(f32)[g]
    sw0 = FOUR_SW0[g]
    th, ph, fr, sw, kinds = four_records(250_000, alpha, beta, maxf, sw0, open_gate, 41 + g)
    assert (sw != 0).all() and maxf > 0                              # the blocks' preconditions (minf = -maxf is how the probe calls them)
    assert np.abs(ph.astype(f64) + fr + (float(alpha) + float(beta)) * np.pi).max() < 4 * np.pi - 0.05     # the plain float step's domain
    before, after, p2, f2, s2, flags = pll_four(th, ph, fr, sw, f32(alpha), f32(beta), f32(maxf), open_gate)
    for a in after + [f2, s2]:
        assert not np.isnan(a).any()
    counts = {}
    for (name, k), sl in kinds.items():
        ew, pw, cl, turned, flipped, crossed = flags[k]
        if name in ("error_edge", "phase_edge"):
            flag = ew if name == "error_edge" else pw
            assert flag[sl].sum() >= 2000 and (~flag[sl]).sum() >= 2000, (name, k, int(flag[sl].sum()))
            counts[(name, k)] = int(flag[sl].sum())
        elif name == "rail":
            hit = turned if open_gate else cl
            assert hit[sl].sum() >= 1000, (name, k, int(hit[sl].sum()))
            counts[(name, k)] = int(hit[sl].sum())
        elif open_gate:                                               # zero_freq: the sign of f2 sets the sweep; where it can, it re-signs it
            assert (~turned[sl]).sum() >= 6000, (name, k, int((~turned[sl]).sum()))
            if zero_flip_reachable(beta, sw0, k):
                assert flipped[sl].sum() >= 1500, (name, g, k, int(flipped[sl].sum()))
                if zero_cross_by_error(beta, sw0, k):
                    assert crossed[sl].sum() >= 1500, (name, g, k, int(crossed[sl].sum()))
            counts[(name, k)] = (int(flipped[sl].sum()), int(crossed[sl].sum()))
        else:
            assert crossed[sl].sum() >= 6000, (name, g, k, int(crossed[sl].sum()))
            counts[(name, k)] = int(crossed[sl].sum())
    one = np.ones(len(ph), dtype=f32)
    recs = np.concatenate([th, np.stack([ph, fr, sw, one * alpha, one * beta, one * maxf], axis=1)], axis=1)
    ref = np.stack((before if fn != 20 else after) + [p2, f2, s2 if open_gate else sw], axis=1)
    return recs, ref, counts


def sweep_case(T, on):
    """pll_sweep_sel: (records[n, 4], reference[n, 2], counts) with the branch counts asserted"""
    _, _, _, _, maxf = loop_constants(T, 50000, argos=T == f64)
    sw0 = T(0.2 * (2.0 * np.pi / float(T(50000))))
    fr, sw, kinds = sweep_set(T, maxf, sw0, 1_000_000, 51)
    f2, s2, turned = sweep(fr, sw, T(maxf), on)
    z = kinds["zero"]
    crossed = (np.sign(fr[z]) != np.sign(f2[z])) | (f2[z] == 0)
    counts = {"turned": int(turned[kinds["rail"]].sum()), "not turned": int((~turned[kinds["rail"]]).sum()), "zero crossed": int(crossed.sum()),
              "re-signed": int((~turned & (s2 != sw)).sum())}
    if on:
        assert counts["turned"] >= 5000 and counts["not turned"] >= 5000 and counts["zero crossed"] >= 2000 and counts["re-signed"] >= 2000, counts
    else:
        assert f2.tobytes() == fr.tobytes() and s2.tobytes() == sw.tobytes()
    one = np.ones(len(fr), dtype=T)
    return np.stack([fr, sw, one * T(maxf), one * T(1.0 if on else 0.0)], axis=1), np.stack([f2, s2], axis=1), counts


def rint_case(T):
    """(x, rint(x)) with the ties counted: every half-integer below 2^22 is there and goes to even"""
    x = rint_set(T)
    r = np.rint(x)
    halves = (x - np.floor(x)) == T(0.5)
    assert halves.sum() >= (1 << 22) and (r[halves] % 2 == 0).all() and len(x) > 16_000_000
    return x, r, {"inputs": len(x), "ties": int(halves.sum())}


def clip_case(T):
    e, lim = clip_set(T)
    assert np.isnan(e).sum() == (1 if T == f64 else 0)
    ref = clip(e, lim)
    counts = {"inputs": len(e), "clipped high": int((e > lim).sum()), "clipped low": int((e < -lim).sum())}
    assert counts["clipped high"] > 250_000 and counts["clipped low"] > 250_000 and (ref == e).sum() > 300_000
    return np.stack([e, lim], axis=1), ref, counts
