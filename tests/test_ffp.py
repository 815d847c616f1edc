"""The feed-forward POES bits without a GPU: pdt_host_ffp_bits against a Python statement of the rule written from the
header's text with float32 arithmetic in the rule's order (tests/ffp_cases.py), byte for byte -- bits, the soft values' bit patterns,
sample indices, the per-block table -- on small streams at every rate and stream length the rule names, a clock fast and slow by
2000 ppm, a block of zeros, Inf and NaN, measured residuals with seams; every bound of the cfg; and the two results the feature exists
for: a weak synthetic capture, where the flywheel places at least as many frames on these bits as on the oracle's, and the real
recording, whose 47 complete frames come out with (seen when this was written) no wrong bit at all, and two more in front of them.

One case the issue asks for cannot exist under the rule: a block BETWEEN signal blocks whose count clamps to 0 through
m_lo(b + 1) < m_lo(b).  Two neighbouring phi differ by at most T / 2 steps, half a bit, and a block is at least 64 bits long, so
m_lo(b + 1) >= m_lo(b) + 62 always.  The clamp is reached at the stream's end instead (a last block shorter than a bit), and the block
of zeros is a case of its own with its expected table written out: it slips one whole bit, as the rule says it may."""
import ctypes as C

import numpy as np
import pytest

import ffp_cases as fc
from test_tip_sync import placed, weak_capture

QNAN = 0x7FC00000


def case(name):
    return [c for c in fc.cases() + fc.tone_cases() if c[0] == name][0]


@pytest.mark.parametrize("name", [c[0] for c in fc.cases()])
def test_host_equals_the_model(pdt, name):
    _, fs, y, cfg = case(name)
    got = pdt.host_ffp_bits(fs, y, **cfg)
    want = fc.model(pdt.host_ffp_mix(fs, y, **cfg), fs, **cfg)
    assert fc.same_as_model(got, want)
    s = got.sync
    B = cfg.get("block_bits", 208)
    assert int(s["block_len"]) == fc.block_len(B, fs) and int(s["nblocks"]) == -(-len(y) // fc.block_len(B, fs))
    assert (int(s["block_bits"]), int(s["clock_steps"])) == (B, cfg.get("clock_steps", 32))
    assert (int(s["ref_bits"]), int(s["smooth_blocks"])) == (cfg.get("ref_bits", 16), cfg.get("smooth_blocks", 4))
    assert s["residual_hz"] == cfg["residual_hz"] and int(s["segs"]) == 0 and int(s["nfft"]) == 0
    assert int(got.blocks["count"].sum()) == len(got.bits) and (np.diff(got.index) > 0).all()
    assert len(got.index) == 0 or got.index[-1] <= len(y)


def test_given_residual_mixes_as_the_burst_rule_does(pdt):
    _, fs, y, cfg = case("rate-50000")
    assert pdt.host_ffp_mix(fs, y, **cfg).tobytes() == pdt.host_ff_mix(fs, cfg["residual_hz"], y).tobytes()


def test_rates_and_lengths(pdt):
    L = pdt.lib()
    y = np.zeros((64, 2), np.float32)
    s, n = np.zeros(1, pdt.FFP_SYNC_DTYPE), C.c_uint64(0)

    def rc(rate, count=64, cfg=None):
        return L.pdt_host_ffp_bits(rate, y.ctypes.data, count, cfg, s.ctypes.data, None, None, None, 0, C.byref(n), None, 0)

    assert rc(49920) == 0 and rc(1064960) == 0 and rc(49919) == -1 and rc(1064961) == -1 and rc(32000) == -1 and rc(18750) == -1
    assert L.pdt_host_ffp_bits(50000, None, 5, None, s.ctypes.data, None, None, None, 0, C.byref(n), None, 0) == -1
    assert L.pdt_host_ffp_bits(50000, y.ctypes.data, 64, None, None, None, None, None, 0, C.byref(n), None, 0) == -1
    assert L.pdt_host_ffp_bits(50000, y.ctypes.data, 64, None, s.ctypes.data, None, None, None, 0, None, None, 0) == -1
    assert L.pdt_host_ffp_bits(50000, None, 0, None, s.ctypes.data, None, None, None, 0, C.byref(n), None, 0) == 0 and n.value == 0
    assert L.pdt_host_ffp_bits(50000, y.ctypes.data, 1 << 36, None, s.ctypes.data, None, None, None, 0, C.byref(n), None, 0) == -1
    # the entries that need a context refuse a missing one before they touch a device
    assert L.pdt_ffp_bits(None, None, s.ctypes.data) == -1 and L.pdt_ffp_read(None, None, None, None, None, 0, C.byref(n)) == -1
    assert L.pdt_ffp_blocks(None, None, 0, C.byref(n)) == -1 and L.pdt_stage_ffp_bits(None, 50000, y.ctypes.data, 64, None, s.ctypes.data) == -1
    k = C.c_int(0)
    assert L.pdt_ffp_frames(None, None, None, None, None, None, 0, C.byref(k)) == -1
    assert L.pdt_stage_ffp_frames(None, 50000, y.ctypes.data, 64, None, None, None, None, None, 0, C.byref(k)) == -1


def test_cfg_bounds(pdt):
    L = pdt.lib()
    y = fc.stream(50000, 900)
    s, n = np.zeros(1, pdt.FFP_SYNC_DTYPE), C.c_uint64(0)

    def rc(**kw):
        c = pdt.FfpCfg(**kw)
        return L.pdt_host_ffp_bits(50000, y.ctypes.data, len(y), C.byref(c), s.ctypes.data, None, None, None, 0, C.byref(n), None, 0)

    assert rc() == 0 and tuple(int(s[0][k]) for k in ("block_bits", "clock_steps", "ref_bits", "smooth_blocks")) == (208, 32, 16, 4)
    assert rc(block_bits=64) == 0 and rc(block_bits=832) == 0 and rc(block_bits=63) == -1 and rc(block_bits=833) == -1 and rc(block_bits=-1) == -1
    assert rc(clock_steps=8) == 0 and rc(clock_steps=64) == 0 and rc(clock_steps=7) == -1 and rc(clock_steps=65) == -1 and rc(clock_steps=-8) == -1
    assert rc(ref_bits=1) == 0 and rc(ref_bits=64) == 0 and rc(ref_bits=65) == -1 and rc(ref_bits=-1) == -1
    assert rc(ref_bits=0, zero_mask=pdt.FFP_ZERO_REF_BITS) == 0 and int(s[0]["ref_bits"]) == 0
    assert rc(ref_bits=0) == 0 and int(s[0]["ref_bits"]) == 16                # a plain 0 is the default
    assert rc(smooth_blocks=1) == 0 and rc(smooth_blocks=16) == 0 and rc(smooth_blocks=17) == -1 and rc(smooth_blocks=-1) == -1
    assert rc(smooth_blocks=0, zero_mask=pdt.FFP_ZERO_SMOOTH) == 0 and int(s[0]["smooth_blocks"]) == 0
    assert rc(smooth_blocks=0) == 0 and int(s[0]["smooth_blocks"]) == 4
    assert rc(zero_mask=4) == -1 and rc(flags=2) == -1
    G = pdt.FFP_RESIDUAL_GIVEN
    assert rc(flags=G, residual_hz=24999.0) == 0 and rc(flags=G, residual_hz=-24999.0) == 0
    assert rc(flags=G, residual_hz=25000.0) == -1 and rc(flags=G, residual_hz=float("nan")) == -1 and rc(flags=G, residual_hz=float("inf")) == -1
    assert rc(residual_hz=float("nan")) == 0                                   # not given: not read


@pytest.mark.parametrize("name,sign", [("clock-fast", -1), ("clock-slow", 1)])
def test_a_clock_off_by_2000_ppm_is_followed(pdt, name, sign):
    """phi passes T (slow) and -T (fast) within the case's 14 blocks of 64 bits, runs on monotonically, and no bit is missing or doubled"""
    _, fs, y, cfg = case(name)
    got = pdt.host_ffp_bits(fs, y, **cfg)
    phi = got.blocks["phi"].astype(np.int64)
    T = cfg["clock_steps"]
    assert (np.diff(phi) * sign >= 0).all() and (phi[-1] - phi[0]) * sign > T and abs(phi).max() > T
    assert fc.aligned(got.bits) == 0
    assert not (np.diff(got.blocks["tau"]) * sign >= 0).all()                 # (tau wrapped; phi did not)


def test_a_block_of_zeros_slips_one_bit_and_the_table_is_as_derived(pdt):
    """49920 sps (P = 3, a bit is 6 samples, a step of T = 8 is 0.75 sample), B = 64 (L = 384), J = 0; the transmitted clock is 3 samples
    = 4 steps late, block 2 and what its bits reach are zeros: every M(2, .) is 0 and the tie goes to tau = 0.  delta folds to +4 twice,
    phi = 4 4 8 12 12 (a whole bit slipped across the gap), o(phi) = 3, 3, 6, 9, 9 samples; m_lo(b) = the smallest m with
    6 m + o >= 384 b: 0, 64, 127, 191, 255; the last block ends with m = 317 (6 318 + 9 <= 1920)."""
    _, fs, y, cfg = case("zero-block")
    got = pdt.host_ffp_bits(fs, y, **cfg)
    assert [b[:4] for b in fc.blocks_of(got)] == [(4, 4, 0, 64), (4, 4, 64, 63), (0, 8, 127, 64), (4, 12, 191, 64), (4, 12, 255, 63)]
    assert int(got.blocks["metric"][2]) == 0 and (got.blocks["metric"][[0, 1, 3, 4]] > 0).all()
    assert (got.soft[127:191] == 0).all() and (got.bits[127:191] == ord("0")).all()
    # the bits in front of the gap are the transmitted ones; behind it they are the transmitted ones one bit on
    bits = got.bits.astype(np.int64) - ord("0")
    sent = fc.sent_bits(400)
    assert np.array_equal(bits[:120], sent[:120]) and np.array_equal(bits[200:], sent[201:201 + len(bits) - 200])


def test_the_count_clamps_at_the_streams_end(pdt):
    """one block and a sample, the clock half a bit late: bit 63 covers the samples [381, 387) and does not exist, so block 0 ends at
    m_end + 1 = 63 and the last block's range, m_lo = 64 up to m_end + 1 = 63, is empty: its count clamps to 0"""
    _, fs, y, cfg = case("one-block-and-a-sample-half-bit-off")
    got = pdt.host_ffp_bits(fs, y, **cfg)
    assert [b[:4] for b in fc.blocks_of(got)] == [(4, 4, 0, 63), (4, 4, 64, 0)]
    assert fc.aligned(got.bits) == 0


def test_inf_and_nan(pdt):
    _, fs, y, cfg = case("inf-nan")
    got = pdt.host_ffp_bits(fs, y, **cfg)
    u = got.soft.view(np.uint32)
    nan = np.isnan(got.soft)
    # sample 200 lies in bit 33 and sample 500 in bit 83: every window that reaches one of them (W = 4) is not a number
    assert set(np.nonzero(nan)[0]) == set(range(29, 38)) | set(range(79, 88))
    assert (u[nan] == QNAN).all() and (got.bits[nan] == ord("0")).all()
    clean = pdt.host_ffp_bits(fs, np.nan_to_num(np.array(y), nan=0.0, posinf=0.0), **cfg)
    assert [b[:4] for b in fc.blocks_of(got)] == [b[:4] for b in fc.blocks_of(clean)]          # q = 0: the clock is found all the same
    assert (got.blocks["metric"] < clean.blocks["metric"]).any()


def expected_mix(pdt, fs, y):
    """the rule's carrier in plain double arithmetic: (steps, start phases, record fields) from pdt_host_tones' records"""
    N = fc.NFFT_50K
    tones = pdt.host_tones(fs, 0.0, y, cap=max(len(y) // N, 1)) if len(y) >= N else []
    steps, starts, cur, phase, valid, first = [], [], 0, 0, 0, None
    for t in tones:
        if t["valid"]:
            cur = int(np.rint(t["residual_hz"] * 4294967296.0 / fs)) & 0xFFFFFFFF
            valid += 1
            first = (float(t["residual_hz"]), cur) if first is None else first
        steps.append(cur)
        starts.append(phase)
        phase = (phase + cur * N) & 0xFFFFFFFF
    return steps or [0], starts or [0], len(tones), valid, first or (0.0, 0)


@pytest.mark.parametrize("name", [c[0] for c in fc.tone_cases()])
def test_measured_residual(pdt, name):
    _, fs, y, cfg = case(name)
    got = pdt.host_ffp_bits(fs, y, **cfg)
    v = pdt.host_ffp_mix(fs, y, **cfg)
    assert fc.same_as_model(got, fc.model(v, fs, **cfg))
    steps, starts, segs, valid, first = expected_mix(pdt, fs, y)
    s = got.sync
    assert (int(s["segs"]), int(s["segs_valid"]), int(s["nfft"])) == (segs, valid, fc.NFFT_50K)
    assert (float(s["residual_hz"]), int(s["step"])) == first
    want = {"shorter-than-nfft": (0, 0), "seam-30hz": (2, 2), "zero-first-segment": (2, 1), "valid-invalid-valid": (3, 2)}[name]
    assert (segs, valid) == want
    # the mixed stream against the same rotation in double: the table's sine is good to a few 1e-7, a wrong step or a phase that is
    # not continuous is off by radians
    i = np.arange(len(y))
    j = np.minimum(i // fc.NFFT_50K, len(steps) - 1)
    phase = (np.array(starts, dtype=np.int64)[j] + (i - j * fc.NFFT_50K) * np.array(steps, dtype=np.int64)[j]) & 0xFFFFFFFF
    z = (y[:, 0].astype(np.float64) + 1j * y[:, 1]) * np.exp(-2j * np.pi * phase / 4294967296.0)
    assert np.abs(z - (v[:, 0] + 1j * v[:, 1])).max() < 2e-6 * max(1.0, float(np.abs(z).max()))
    if name == "zero-first-segment":
        assert steps[0] == 0 and steps[1] != 0
    if name == "valid-invalid-valid":
        assert steps[1] == steps[0] != 0
    if name == "seam-30hz":
        hz = [st * fs / 4294967296.0 - (fs if st >= 1 << 31 else 0) for st in steps]
        assert abs(hz[0] + 3470) < 2 and abs(hz[1] + 3500) < 2
        # the carrier's phase is continuous and so is the mixer's: v's phase runs through the seam, and the bits across it are right
        assert fc.aligned(got.bits) == 0


def test_weak_capture_places_at_least_as_many_frames_as_the_loop(pdt, orc):
    """Synthetic POES, 50 ksps, 30 s, seed 1234, noise x 9, the flywheel at its defaults on both.  Seen when this was written: the
    oracle's bits 295 placed / 3 not, the feed-forward bits at their defaults 299 placed / 0 not."""
    p, x = weak_capture(pdt)
    loop = pdt.host_tip_sync(orc.Oracle(orc.POES, 50000, x).stage(orc.ST_BITS))
    ref = placed(pdt, p, [bytes(v) for v in loop["bytes"]])
    got = pdt.host_ffp_bits(50000, x.astype(np.float32) / np.float32(32768.0))
    ffp = placed(pdt, p, [bytes(v) for v in pdt.host_tip_sync(got.bits.tobytes())["bytes"]])
    print(f"oracle's bits: {ref[0]} placed / {ref[1]} not; feed-forward bits: {ffp[0]} placed / {ffp[1]} not; segments {int(got.sync['segs_valid'])} / "
          f"{int(got.sync['segs'])} valid")
    assert ffp[0] >= ref[0] and ffp[1] <= ref[1]
    assert ref[0] > 100                                                       # (the capture is weak, not dead)


def test_real_recording(pdt, clip):
    """tests/golden/5sec_clip.wav, uncut, the residual measured, the flywheel at its defaults.  Seen when this was written: 49 frames --
    the 47 complete frames of clip.c10000.txt with 0 of their 39 104 bits different, and in front of them two more, at 0.080 and 0.180 s,
    that the loop loses while it pulls in --, a carrier from -3 470 to -3 500 Hz and a clock drift of +71.5 ppm."""
    rate, iq = clip
    got = pdt.host_ffp_bits(rate, iq.astype(np.float32) / np.float32(32768.0))
    fr = pdt.host_tip_sync(got.bits.tobytes())
    assert len(fr) >= 47
    text = open(__file__.replace("test_ffp.py", "golden/clip.c10000.txt")).read().split("\n")
    want = [bytes(int(h, 16) for h in line.split()[1:]) for line in text if len(line.split()) == 105]
    assert len(want) == 47
    mine = np.stack([f["bytes"] for f in fr])
    total, at = 0, -1
    for w in want:
        d = np.unpackbits(mine ^ np.frombuffer(w, dtype=np.uint8), axis=1).sum(axis=1)
        k = int(d.argmin())
        assert d[k] <= 8 and k > at                                           # within 8 of 832 bits, in the same order
        total, at = total + int(d[k]), k
    print(f"{len(fr)} frames, {total} of 39104 bits differ")
    assert total <= 39
    s = got.sync
    assert int(s["segs"]) == len(iq) // 4096 and int(s["segs_valid"]) == int(s["segs"]) and -3520 < s["residual_hz"] < -3450
    # the clock: phi's slope in steps of 1 / T bit per block of B bits
    phi = got.blocks["phi"].astype(np.float64)
    ppm = np.polyfit(np.arange(len(phi)), phi, 1)[0] / (32 * 208) * 1e6
    print(f"clock drift {ppm:.1f} ppm")
    assert 40 < abs(ppm) < 100
    # time stamps are seconds of the stream: the frames lie 0.1 s apart
    t = got.index[fr["bit_index"]] / rate
    assert np.allclose(np.diff(t), 0.1, atol=2e-4)
