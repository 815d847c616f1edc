"""Wideband SDR captures on the GPU: the down-converter's kernel against its host restatement bit for bit, the routing into the
chain (a wideband capture = the RAW float capture of its channel stream), decoded outcomes against what the synthetic generator
transmitted, several channels of one capture, the records of stream pieces, streaming, files and the command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_gpu_real_input import transmitted

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "bin")
FORMATS = ("pcm16", "f32", "cu8", "cs8")


def random_capture(rng, fmt: str, n: int) -> np.ndarray:
    if fmt == "pcm16":
        return rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
    if fmt == "f32":
        return rng.uniform(-1.5, 1.5, (n, 2)).astype(np.float32)
    if fmt == "cu8":
        return rng.integers(0, 256, (n, 2)).astype(np.uint8)
    return rng.integers(-128, 128, (n, 2)).astype(np.int8)


def fmt_code(pdt, x: np.ndarray) -> int:
    return {np.dtype(np.int16): pdt.FMT_WB_PCM16, np.dtype(np.float32): pdt.FMT_WB_F32, np.dtype(np.uint8): pdt.FMT_WB_CU8,
            np.dtype(np.int8): pdt.FMT_WB_CS8}[x.dtype]


def carriers(pdt, kind: int, in_rate: int, secs: float, offsets, seeds, residual: float):
    """Transmissions summed into one int16 capture at in_rate, each at half amplitude, the carrier of channel i at offsets[i] +
    residual.  Returns the capture and each transmission's parameters."""
    n = int(round(secs * in_rate))
    total = np.zeros((n, 2), dtype=np.int32)
    params = []
    for off, seed in zip(offsets, seeds):
        p = pdt.synth_params(kind, in_rate, off + residual, seed)
        p.amplitude //= 2
        p.noise_gain //= 2
        iq = np.zeros((n, 2), dtype="<i2")
        pdt.synth_lib().pdt_synth_fill(C.byref(p), 0, n, iq.ctypes.data)
        total += iq
        params.append(p)
    return np.clip(total, -32768, 32767).astype(np.int16), params


def to_cu8(x16: np.ndarray) -> np.ndarray:
    """The unsigned 8-bit rendering of an int16 capture (what an RTL-SDR would have recorded)."""
    return np.clip(np.floor(x16 / 256.0) + 128, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("D", (2, 4, 16, 64))
def test_kernel_equals_host_restatement(pdt, D, fmt):
    """PDT_ST_CHANNEL is pdt_host_ddc, bit for bit: captures shorter than the halo, around it, around one tile of the kernel and a
    long one; positive and negative offsets; captures in host memory and at unaligned device addresses."""
    rng = np.random.default_rng(1000 * D + FORMATS.index(fmt))
    fs = 250000
    in_rate = fs * D
    tile = 2048 // D * D
    with pdt.Demodulator(pdt.MODE_POES, fs) as d:
        for n in (1, 8 * D - 1, 8 * D + 1, tile - 1, tile + 1, 10 ** 6 + 7):
            x = random_capture(rng, fmt, n)
            for offset in ((0.31 * in_rate, -0.123456 * in_rate) if n < 10 ** 6 else (-0.31 * in_rate,)):
                want = pdt.host_ddc(in_rate, D, offset, x)
                d.set_channel(D, offset).demod_channel(x)
                assert d.stage_len(pdt.ST_CHANNEL) == (n + D - 1) // D
                assert d.stage(pdt.ST_CHANNEL).tobytes() == want.tobytes(), (n, offset)
                assert d.stats().samples == (n + D - 1) // D
        # resident captures whose first sample sits 1, 2 and 3 samples behind a 16-byte boundary
        n = 3 * tile + 5
        x = random_capture(rng, fmt, n + 3)
        dev = torch.from_numpy(x.reshape(-1).copy()).to("cuda:0")
        torch.cuda.synchronize()
        for skip in (1, 2, 3):
            want = pdt.host_ddc(in_rate, D, 77777.0, x[skip: skip + n])
            d.set_channel(D, 77777.0).demod_device_channel(dev.data_ptr() + skip * 2 * x.itemsize, n, fmt_code(pdt, x))
            assert d.stage(pdt.ST_CHANNEL).tobytes() == want.tobytes(), skip


ALL_DECIMS = tuple(range(2, 65))                                        # everything pdt_set_channel and -x accept


def ddc_geometry(D: int):
    """ddc_launch's geometry for decimation D (csrc/pdt_ddc.hip: DDC_TILE = 2048, DDC_TB = 256): outputs of a tile, lanes of a
    workgroup, outputs per lane."""
    TO = 2048 // D
    tb = min(256, (TO + 63) // 64 * 64)
    return TO, tb, (TO + tb - 1) // tb


@pytest.mark.parametrize("D", ALL_DECIMS)
def test_kernel_equals_host_restatement_at_every_decimation(pdt, D):
    """PDT_ST_CHANNEL is pdt_host_ddc, bit for bit, at EVERY decimation and in all four formats.  The kernel's geometry is a function
    of D -- TO = 2048 // D outputs a tile, tb = min(256, TO rounded up to 64) lanes, nb = ceil(TO / tb) outputs a lane -- and the
    powers of two of the test above leave most of it unrun.  From DDC_TILE = 2048 and DDC_TB = 256 (re-derive when either changes):

    * nb, the ddc_fir<NB> instantiation: 4 at D = 2; 3 at D = 3 only (TO = 682); 2 at D = 4 .. 7; 1 from D = 8 on.  The last round has
      lanes clamped by mb[b] = min(.., TO - 1) where tb does not divide TO: D = 3 (nb = 3), D = 5, 6, 7 (nb = 2); for nb = 1 the lanes
      t >= TO take no part: D = 9, 10 (tb = 256), 11 .. 15 (tb = 192), 17 .. 31 (tb = 128), 33 .. 63 (tb = 64; D = 63 and 64 both have
      TO = 32, half a wavefront).
    * the carry of the polyphase rotation (r += tb % D; if (r >= D) { r -= D; q++; }) runs where D does not divide tb: D = 3, 5, 6, 7,
      9, 10 (tb = 256), 11, 13, 14, 15 (tb = 192), 17 .. 31 (tb = 128), 33 .. 63 (tb = 64) -- at no power of two.
    * the head / 16-byte vectors / tail split of an inner tile's load: the tile's first input (m0 - 8) D advances by TO D = 2048 - 2048 %
      D samples a tile, so where D does not divide 2048 the split differs from tile to tile of ONE aligned capture (the lengths of 3
      and of about 20 tiles here), for every format's samples-per-vector (2, 4, 8); the resident captures 1, 2 and 3 samples behind a
      16-byte boundary shift it once more.
    * the worst cases of the LDS image: D ((TO + 16) | 1) <= DDC_VS = 3136 is tightest at D = 64 (3136), 62 (3038), 63 (3087) and 47
      (2773 of the 2048 + 17 D = 2847 the formula allows), where TO + 16 is even and the row is padded.

    Lengths: a single sample, around one output, around the halo (8 D), around one tile (tile = TO D inputs), tile - D + 1 where
    the number of outputs is exactly TO, three tiles and some twenty tiles with an odd remainder; a positive and a negative offset;
    captures from host memory and resident ones at unaligned addresses.  (The 10^6-sample case stays with the test above.)"""
    fs = 250000
    in_rate = fs * D
    TO, tb, nb = ddc_geometry(D)
    tile = TO * D
    print(f"D {D}: TO {TO}, tb {tb}, nb {nb}, tb % D {tb % D}, TO % tb {TO % tb}, tile stride % 8 {tile % 8}")
    with pdt.Demodulator(pdt.MODE_POES, fs) as d:
        for fmt in FORMATS:
            rng = np.random.default_rng(5000 * D + FORMATS.index(fmt))
            for n in (1, D - 1, D, 8 * D - 1, 8 * D + 1, tile - 1, tile, tile + 1, tile - D + 1, 3 * tile + 5, 20 * tile + 2 * D + 777):
                x = random_capture(rng, fmt, n)
                for offset in (0.31 * in_rate, -0.123456 * in_rate):
                    want = pdt.host_ddc(in_rate, D, offset, x)
                    d.set_channel(D, offset).demod_channel(x)
                    assert d.stage_len(pdt.ST_CHANNEL) == (n + D - 1) // D, (fmt, n, offset)
                    assert d.stage(pdt.ST_CHANNEL).tobytes() == want.tobytes(), (fmt, n, offset)
                    assert d.stats().samples == (n + D - 1) // D, (fmt, n, offset)
            # resident captures whose first sample sits 1, 2 and 3 samples behind a 16-byte boundary
            n = 3 * tile + 5
            x = random_capture(rng, fmt, n + 3)
            dev = torch.from_numpy(x.reshape(-1).copy()).to("cuda:0")
            torch.cuda.synchronize()
            for skip in (1, 2, 3):
                want = pdt.host_ddc(in_rate, D, -77777.0, x[skip: skip + n])
                d.set_channel(D, -77777.0).demod_device_channel(dev.data_ptr() + skip * 2 * x.itemsize, n, fmt_code(pdt, x))
                assert d.stage_len(pdt.ST_CHANNEL) == (n + D - 1) // D, (fmt, skip)
                assert d.stage(pdt.ST_CHANNEL).tobytes() == want.tobytes(), (fmt, skip)


PIECE_DECIMS = (2, 3, 7, 16, 64)          # nb = 4, 3, 2, 1 and 1; the rotation's carry (3, 7) and none; the tightest LDS image (64)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("D", PIECE_DECIMS)
def test_a_piece_that_sees_its_neighbours_equals_the_whole_capture(pdt, D, fmt):
    """A stream's converted pairs cannot be read back, and a frame need not notice one wrong ulp or sample at a push seam.  So the
    kernel is run (pdt_dev_ddc) on the records a stream hands it: outputs [k0, k0 + m) of a resident capture of 5 tiles + 3 D + 1
    frames from a view that begins at input k0 D, sees up to 8 D samples to its left (lo < 0) and the rest of the capture to its
    right, with g0 = k0 D -- and must give pdt_host_ddc(whole capture)[k0 : k0 + m], byte for byte.  The tile grid starts at another
    alignment in every piece, as in a stream: the stream's first output and its first tile and a bit (no left halo), one output whose
    view begins exactly 8 D before it (the first tile's inner test at its boundary), two outputs across a tile's end, several
    tiles, and a piece that runs to the capture's end (zeros beyond).
    One further piece is truncated on both sides (lo = -3, hi = (m - 1) D + 2) and must equal the same outputs of the capture with
    every sample outside the view set to zero -- not in cu8, where no byte maps to 0."""
    fs = 250000
    in_rate, offset = fs * D, -0.123456 * fs * D
    TO, _, _ = ddc_geometry(D)
    n = 5 * TO * D + 3 * D + 1
    n_out = (n + D - 1) // D
    rng = np.random.default_rng(9000 * D + FORMATS.index(fmt))
    x = random_capture(rng, fmt, n)
    code, bps = fmt_code(pdt, x), 2 * x.itemsize
    want = pdt.host_ddc(in_rate, D, offset, x)
    dev = torch.from_numpy(x.reshape(-1).copy()).to("cuda:0")
    out = torch.empty((n_out + 1, 2), dtype=torch.float32, device="cuda:0")

    def piece(k0, m, lo, hi):
        out.fill_(float("nan"))
        torch.cuda.synchronize()
        pdt.dev_ddc(in_rate, D, offset, code, dev.data_ptr() + k0 * D * bps, lo, hi, m, k0 * D, out.data_ptr())
        got = out.cpu().numpy()
        assert np.isnan(got[m:]).all(), (k0, m)                          # nothing behind the outputs asked for
        return got[:m]

    for k0, m in ((0, 1), (0, TO + 3), (9, 1), (TO - 1, 2), (TO + 5, 2 * TO + 1), (n_out - TO - 2, TO + 2)):
        got = piece(k0, m, -min(8 * D, k0 * D), n - k0 * D)
        assert got.tobytes() == want[k0: k0 + m].tobytes(), (k0, m)
    if fmt != "cu8":
        k0, m = TO + 5, 2 * TO + 1
        lo, hi = -3, (m - 1) * D + 2
        z = np.zeros_like(x)
        z[k0 * D + lo: k0 * D + hi] = x[k0 * D + lo: k0 * D + hi]
        assert piece(k0, m, lo, hi).tobytes() == pdt.host_ddc(in_rate, D, offset, z)[k0: k0 + m].tobytes()


@pytest.mark.parametrize("fmt", FORMATS)
def test_capture_aligned_to_its_element_but_not_to_its_pair(pdt, fmt):
    """A resident capture may begin half a sample off: at an address that is a multiple of the element's size (2 bytes for int16, 4
    for float, 1 for the 8-bit formats) and not of the I,Q pair's.  No 16-byte boundary then falls between two samples, and k_ddc
    loads every tile sample by sample (head = len); include/pdt.h asks for no more than that, and the result is pdt_host_ddc's of
    the same bytes.  Three tiles and a bit, at a power of two and at an odd decimation; 0, 1 and 3 whole samples further on too."""
    rng = np.random.default_rng(77 + FORMATS.index(fmt))
    fs = 250000
    with pdt.Demodulator(pdt.MODE_POES, fs) as d:
        for D in (4, 7):
            in_rate = fs * D
            n = 3 * (2048 // D * D) + 5
            flat = random_capture(rng, fmt, n + 4).reshape(-1)             # elements: I, Q, I, Q, ...
            dev = torch.from_numpy(flat.view(np.uint8).copy()).to("cuda:0")  # (the bytes; torch allocations are 16-byte aligned)
            torch.cuda.synchronize()
            assert dev.data_ptr() % 16 == 0
            for skip in (0, 1, 3):
                first = 2 * skip + 1                                       # the capture begins with what was a Q
                host = flat[first: first + 2 * n].reshape(n, 2)
                want = pdt.host_ddc(in_rate, D, 0.2 * in_rate, host)
                d.set_channel(D, 0.2 * in_rate).demod_device_channel(dev.data_ptr() + first * flat.itemsize, n, fmt_code(pdt, flat))
                assert d.stage_len(pdt.ST_CHANNEL) == (n + D - 1) // D
                assert d.stage(pdt.ST_CHANNEL).tobytes() == want.tobytes(), (D, skip)


def test_other_captures_have_no_channel_stage(pdt, clip):
    rate, iq = clip
    with pdt.Demodulator(pdt.MODE_POES, rate) as d:
        d.demod(iq[:50000])
        assert d.stage_len(pdt.ST_CHANNEL) == 0


def test_poes_routing_equals_raw_float_path(pdt, orc):
    """demod_channel(x) and demod_raw(host_ddc(x)) at the channel rate are the same capture: frames, text, counts, per-chunk
    reports; and the text is the oracle's for that float capture."""
    fs, D, offset = 250000, 4, 200000.0
    x, _ = carriers(pdt, 0, fs * D, 8.0, (offset,), (31,), 1000.0)
    z = pdt.host_ddc(fs * D, D, offset, x)
    with pdt.Demodulator(pdt.MODE_POES, fs).keep_quality() as d:
        d.set_channel(D, offset).demod_channel(x)
        assert d.stage(pdt.ST_CHANNEL).tobytes() == z.tobytes()
        a = (d.text(), d.frames_array().tobytes(), d.chunk_reports().tobytes())
        sa = d.stats()
    with pdt.Demodulator(pdt.MODE_POES, fs).keep_quality() as d:
        d.demod_raw(z)
        b = (d.text(), d.frames_array().tobytes(), d.chunk_reports().tobytes())
        sb = d.stats()
    assert a == b and len(a[0]) > 10000
    for k in ("samples", "out_samples", "symbols", "bits", "frames", "lock_sample", "lock_freq_hz", "norm_factor", "avg_phase"):
        assert getattr(sa, k) == getattr(sb, k), k
    assert a[0] == orc.Oracle(orc.POES, fs, z).text()


SETUPS = [(1000000, 4, (200000.0, -180000.0)), (2400000, 16, (600000.0, -400000.0)), (2048000, 8, (299500.0, -421700.0))]


def decode_what_was_sent(pdt, in_rate, D, offsets, rendering, seeds):
    fs = in_rate // D
    x, params = carriers(pdt, 0, in_rate, 8.0, offsets, seeds, 1000.0)
    if rendering == "cu8":
        x = to_cu8(x)
    for off, p in zip(offsets, params):
        with pdt.Demodulator(pdt.MODE_POES, fs) as d:
            d.set_channel(D, off).demod_channel(x)
            fr = d.frames_array()
            st = d.stats()
        # the transmission runs on the wideband clock: frame k starts at the same time in seconds of the channel stream
        res = transmitted(pdt, p, fr, len(x), in_rate)
        print(in_rate, D, off, rendering, res, st.lock_freq_hz)
        assert res["ok"], res
        assert st.lock_sample >= 0 and abs(st.lock_freq_hz - 1000.0) < 200.0


@pytest.mark.parametrize("rendering", ["pcm16", "cu8"])
@pytest.mark.parametrize("in_rate,D,offsets", SETUPS)
def test_poes_channels_decode_what_was_sent(pdt, in_rate, D, offsets, rendering):
    """Two POES transmissions (seeds 11 and 12, 8 s, half amplitude each) in one wideband capture: each channel's complete frames
    are frames the generator sent (the `transmitted` criterion of the real-input tests), and its PLL locks on the residual 1 kHz."""
    decode_what_was_sent(pdt, in_rate, D, offsets, rendering, (11, 12))


ODD_SETUPS = [(1750000, 7, (300000.0, -412300.0))]                      # (a list of its own: the survey tests take SETUPS)


@pytest.mark.parametrize("rendering", ["pcm16", "cu8"])
@pytest.mark.parametrize("in_rate,D,offsets", ODD_SETUPS)
def test_poes_channels_decode_what_was_sent_at_an_odd_decimation(pdt, in_rate, D, offsets, rendering):
    """The same criterion at 1.75 Msps / 7 (nb = 2 with clamped lanes, the rotation's carry, a load split that moves from tile to
    tile).  The seeds were tried on the CPU first, as for the ARGOS test below: pdt_host_ddc followed by the oracle's POES chain on
    the float capture (the call of test_poes_routing_equals_raw_float_path).  Seed pairs (11, 12), (21, 22) and (31, 32), both
    offsets, both renderings: all twelve cases decode 79 of the 80 frames sent, every one a sent frame, and lock within 15 Hz of the
    1 kHz residual; (11, 12), the pair of the setups above, is kept."""
    decode_what_was_sent(pdt, in_rate, D, offsets, rendering, (11, 12))


def test_argos_channel_decodes_every_burst_after_the_lock(pdt):
    """ARGOS at 1.024 Msps / 32: the double chain reading the channel's float pairs.  The seeds were chosen on the CPU first: for
    seeds 7, 8 and 9 at both offsets the float64 model of the converter (tests/test_channel_input.py), rendered as int16 -- the
    oracle's ARGOS chain takes no float captures --, and the oracle alone decode every burst after the lock (9 of 10) and nothing
    that was not sent; two of those six cases are kept."""
    in_rate, D, secs = 1024000, 32, 15.0
    fs = in_rate // D
    for offset, seed in ((250000.0, 8), (-333300.0, 9)):
        x, (p,) = carriers(pdt, 1, in_rate, secs, (offset,), (seed,), 120.0)
        with pdt.Demodulator(pdt.MODE_ARGOS, fs) as d:
            d.set_channel(D, offset).demod_channel(x)
            fr = d.frames_array()
            st = d.stats()
        assert st.lock_sample >= 0
        period = in_rate * 3 // 2
        nb = int(len(x) // period)
        sent = [bytes(pdt.synth_argos_payload(p, b)) for b in range(nb)]
        got = [bytes(f["bytes"][:7]) for f in fr if f["complete"]]
        after = [sent[b] for b in range(nb) if b * period >= st.lock_sample * D]
        assert len(after) >= nb // 2
        assert all(s in got for s in after), (len(got), len(after))
        assert all(g in sent for g in got)


def test_several_channels_equal_one_at_a_time(pdt):
    """demod_channels with 2 and with 4 contexts (one of them ARGOS): each context holds, byte for byte, what it gets alone."""
    in_rate, D = 1024000, 4
    fs = in_rate // D
    x, _ = carriers(pdt, 0, in_rate, 6.0, (200000.0, -180000.0, 390000.0), (11, 12, 13), 1000.0)
    xa, _ = carriers(pdt, 1, in_rate, 6.0, (-401000.0,), (8,), 120.0)
    x = np.clip(x.astype(np.int32) + xa, -32768, 32767).astype(np.int16)
    plan = [(pdt.MODE_POES, 200000.0), (pdt.MODE_POES, -180000.0), (pdt.MODE_ARGOS, -401000.0), (pdt.MODE_POES, 390000.0)]
    alone = []
    for mode, off in plan:
        with pdt.Demodulator(mode, fs) as d:
            d.set_channel(D, off).demod_channel(x)
            alone.append((d.text(), d.frames_array().tobytes(), d.stage(pdt.ST_CHANNEL).tobytes()))
    assert all(len(a[0]) > 100 for a in alone[:2])
    dev = torch.from_numpy(x.reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    for count in (2, 4):
        ds = [pdt.Demodulator(mode, fs).set_channel(D, off) for mode, off in plan[:count]]
        try:
            for rep in range(2):
                pdt.demod_channels(ds, dev.data_ptr(), len(x), pdt.FMT_WB_PCM16)
                for d, a in zip(ds, alone):
                    assert (d.text(), d.frames_array().tobytes(), d.stage(pdt.ST_CHANNEL).tobytes()) == a
            pdt.demod_channels(ds, x)                                   # the capture in host memory
            for d, a in zip(ds, alone):
                assert (d.text(), d.frames_array().tobytes()) == a[:2]
            ds[1].set_channel(8, -180000.0)                             # mixed decimations are refused
            with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
                pdt.demod_channels(ds, dev.data_ptr(), len(x), pdt.FMT_WB_PCM16)
            with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
                pdt.demod_channels([ds[0], ds[0]], dev.data_ptr(), len(x), pdt.FMT_WB_PCM16)
        finally:
            for d in ds:
                d.close()


@pytest.mark.parametrize("in_rate,D,tuned", [(1000000, 4, (200000.0, -180000.0, 390000.0)), (1750000, 7, (300000.0, -412300.0, 610000.0))])
def test_seventeen_and_thirty_three_channels(pdt, in_rate, D, tuned):
    """demod_channels with 17 and with 33 contexts (more than the 16 carriers a survey reports): one conversion launch per context, all
    on the first context's stream.  Every context has an offset of its own, except that contexts 15 and 16 share one (a carrier's);
    contexts 0 and 32 sit on carriers too.  Each context's
    channel stream is pdt_host_ddc of ITS offset, and its text and frames are what the same context holds after demod_channel
    alone.  Before every joint call each context converts the capture at another offset, so that no buffer still holds the answer."""
    fs = in_rate // D
    x, _ = carriers(pdt, 0, in_rate, 0.5, tuned, (11, 12, 13), 1000.0)
    offsets = [-0.42 * in_rate + i * (0.84 * in_rate / 32) + 137.0 for i in range(33)]
    offsets[0], offsets[15], offsets[16], offsets[32] = tuned[1], tuned[0], tuned[0], tuned[2]
    assert len(set(offsets)) == 32
    dev = torch.from_numpy(x.reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    ds = [pdt.Demodulator(pdt.MODE_POES, fs) for _ in offsets]
    try:
        alone = []
        for d, off in zip(ds, offsets):
            d.set_channel(D, off).demod_channel(x)
            ch = d.stage(pdt.ST_CHANNEL).tobytes()
            assert ch == pdt.host_ddc(in_rate, D, off, x).tobytes(), off
            alone.append((d.text(), d.frames_array().tobytes(), ch))
        assert all(len(alone[i][0]) > 100 for i in (0, 15, 16, 32))
        assert alone[15] == alone[16] and len({a[2] for a in alone}) == 32

        def scrub(count):
            for d, off in zip(ds[:count], offsets):
                d.set_channel(D, 0.5 * off + 777.0).demod_channel(x)
                d.set_channel(D, off)

        for count in (17, 33):
            for rep in range(2):
                scrub(count)
                pdt.demod_channels(ds[:count], dev.data_ptr(), len(x), pdt.FMT_WB_PCM16)
                for i, (d, a) in enumerate(zip(ds, alone[:count])):
                    assert d.stage_len(pdt.ST_CHANNEL) == (len(x) + D - 1) // D
                    assert d.stage(pdt.ST_CHANNEL).tobytes() == a[2], (count, rep, i)
                    assert (d.text(), d.frames_array().tobytes()) == a[:2], (count, rep, i)
        scrub(33)
        pdt.demod_channels(ds, x)                                       # the capture in host memory
        for i, (d, a) in enumerate(zip(ds, alone)):
            assert (d.text(), d.frames_array().tobytes(), d.stage(pdt.ST_CHANNEL).tobytes()) == a, i
    finally:
        for d in ds:
            d.close()


def test_changing_the_decimation_on_one_context(pdt):
    """The tap table is kept on the context under its decimation: D = 4, then D = 7, then D = 4 again on ONE context, each channel
    stream pdt_host_ddc's and the third call's results the first's; then a stream at D = 3 on the same context, whose frames are
    a fresh context's whole call."""
    fs = 250000
    x4, _ = carriers(pdt, 0, 4 * fs, 1.5, (200000.0,), (41,), 1000.0)
    x7, _ = carriers(pdt, 0, 7 * fs, 1.5, (-412300.0,), (42,), 1000.0)
    x3, _ = carriers(pdt, 0, 3 * fs, 1.5, (150000.0,), (43,), 1000.0)
    with pdt.Demodulator(pdt.MODE_POES, fs) as d:
        d.set_channel(3, 150000.0).demod_channel(x3)
        want3 = (d.text(), d.frames_array())
    assert len(want3[1]) > 3
    with pdt.Demodulator(pdt.MODE_POES, fs) as d:
        d.set_channel(4, 200000.0).demod_channel(x4)
        first = (d.stage(pdt.ST_CHANNEL).tobytes(), d.text(), d.frames_array().tobytes())
        assert first[0] == pdt.host_ddc(4 * fs, 4, 200000.0, x4).tobytes() and len(first[1]) > 100
        d.set_channel(7, -412300.0).demod_channel(x7)
        assert d.stage_len(pdt.ST_CHANNEL) == (len(x7) + 6) // 7
        assert d.stage(pdt.ST_CHANNEL).tobytes() == pdt.host_ddc(7 * fs, 7, -412300.0, x7).tobytes()
        assert len(d.text()) > 100
        d.set_channel(4, 200000.0).demod_channel(x4)
        assert (d.stage(pdt.ST_CHANNEL).tobytes(), d.text(), d.frames_array().tobytes()) == first
        d.set_channel(3, 150000.0)
        got = [d.stream_push_channel(x3[i: i + 100001]) for i in range(0, len(x3), 100001)] + [d.stream_end()]
        assert np.concatenate(got).tobytes() == want3[1].tobytes()
        assert d.text() == want3[0]


@pytest.mark.parametrize("mode,kind,in_rate,D,offset,residual", [(0, 0, 1000000, 4, 200000.0, 1000.0), (1, 1, 1024000, 32, 250000.0, 120.0),
                                                                (0, 0, 2400000, 16, -400000.0, 1000.0),
                                                                # no powers of two: 750 k / 3 and 1.75 M / 7 into 250 ksps contexts,
                                                                # 1.65 M / 33 into a 50 ksps one
                                                                (0, 0, 750000, 3, 150000.0, 1000.0), (0, 0, 1750000, 7, -412300.0, 1000.0),
                                                                (0, 0, 1650000, 33, 400000.0, 1000.0)])
def test_stream_pushes_equal_the_whole_call(pdt, mode, kind, in_rate, D, offset, residual):
    fs = in_rate // D
    x16, _ = carriers(pdt, kind, in_rate, 6.0 if kind == 0 else 12.0, (offset,), (55,), residual)
    rng = np.random.default_rng(D)
    for x in (x16, to_cu8(x16)):
        with pdt.Demodulator(mode, fs) as d:
            d.set_channel(D, offset).demod_channel(x)
            want_text, want = d.text(), d.frames_array()
        assert len(want) > 3
        with pdt.Demodulator(mode, fs) as d:
            d.set_channel(D, offset)
            got, at = [], 0
            sizes = [1, 0, D - 1, D, 1, 8 * D - 1, 0, 3, 8 * D + 1, 2]       # one frame, empty pushes, fewer than the halo (8 D)
            while at < len(x):
                k = sizes.pop(0) if sizes else int(rng.integers(1, 150000 * D))
                got.append(d.stream_push_channel(x[at: at + k]))
                at = min(at + k, len(x))
                held = at if at < 8 * D else 8 * D + at % D
                assert d.stream_retained() >= held
            got.append(d.stream_end())
            assert np.concatenate(got).tobytes() == want.tobytes()
            assert d.text() == want_text


def test_stream_and_context_arguments(pdt):
    fs = 250000
    L = pdt.lib()
    with pdt.Demodulator(pdt.MODE_POES, fs) as d:
        x = np.zeros((1000, 2), dtype=np.int16)
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.demod_channel(x)                                          # no channel yet
        for decim, off in ((1, 0.0), (65, 0.0), (0, 0.0), (4, 500000.0), (4, -500000.0), (4, float("nan")), (4, float("inf"))):
            with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
                d.set_channel(decim, off)
        d.set_channel(64, 7999999.0).set_channel(4, -499999.0).set_channel(4, 200000.0)
        for fmt in (0, 1, 2, 3, 15, 20):
            assert L.pdt_demod_channel(d._h, x.ctypes.data, 1000, fmt) == -1
        d.stream_push_channel(x)
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.set_channel(4, 1000.0)                                    # a stream is open
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            d.stream_push(np.zeros((10, 2), dtype=np.int16))           # I,Q into a wideband stream
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            d.stream_push_real(np.zeros(10, dtype=np.int16))           # real into a wideband stream
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            d.stream_push_channel(np.zeros((10, 2), dtype=np.uint8))   # the other wideband format
        d.stream_end()
        d.stream_push(np.zeros((10, 2), dtype=np.int16))
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            d.stream_push_channel(x)                                    # wideband into an I,Q stream
        d.stream_end()
    with pytest.raises(pdt.PdtError, match=r"\(-5\)"):
        pdt.Demodulator(pdt.MODE_POES, 1000000)                         # a wideband rate is still no context rate


def test_files_equal_the_in_memory_call(pdt, tmp_path):
    in_rate, D, offset = 1000000, 4, 200000.0
    fs = in_rate // D
    x, _ = carriers(pdt, 0, in_rate, 6.0, (offset,), (61,), 1000.0)
    u8 = to_cu8(x)
    s8 = (u8.astype(np.int16) - 128).astype(np.int8)
    wav = str(tmp_path / "wide.wav")
    pdt.write_wav(wav, in_rate, x)
    for path, arr, fmt, off in ((wav, x, pdt.FMT_WB_PCM16, 44), (str(tmp_path / "wide.cu8"), u8, pdt.FMT_WB_CU8, 0),
                                (str(tmp_path / "wide.cs8"), s8, pdt.FMT_WB_CS8, 0)):
        if not off:
            arr.tofile(path)
        with pdt.Demodulator(pdt.MODE_POES, fs) as d:
            d.set_channel(D, offset).demod_channel(arr)
            want = d.text()
        assert len(want) > 10000
        fd = os.open(path, os.O_RDONLY)
        out = str(tmp_path / "out.txt")
        tfd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        try:
            with pdt.Demodulator(pdt.MODE_POES, fs) as d:
                nb = d.set_channel(D, offset).demod_file_text(fd, off, len(arr), tfd, fmt=fmt)
                assert d.stage_len(pdt.ST_CHANNEL) == (len(arr) + D - 1) // D
        finally:
            os.close(fd)
            os.close(tfd)
        text = open(out, "rb").read()
        assert nb == len(text) and text == want


def test_command_line(pdt, tmp_path):
    in_rate, D = 1000000, 4
    fs = in_rate // D
    x, _ = carriers(pdt, 0, in_rate, 6.0, (200000.0, -180000.0), (11, 12), 1000.0)
    wav = str(tmp_path / "two_carriers.wav")
    pdt.write_wav(wav, in_rate, x)
    want = []
    for off in (200000.0, -180000.0):
        with pdt.Demodulator(pdt.MODE_POES, fs) as d:
            d.set_channel(D, off).demod_channel(x)
            want.append(d.text())
    assert all(len(w) > 10000 for w in want)
    exe = os.path.join(BIN, "demodPOES")
    out = str(tmp_path / "frames.txt")
    r = subprocess.run([exe, "-x", "4", "-t", "200", "-t", "-180", "-o", out, wav], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    assert open(out + ".0", "rb").read() == want[0] and open(out + ".1", "rb").read() == want[1]
    # one channel: the usual single output file
    r = subprocess.run([exe, "-x", "4", "-t", "-180", "-o", out, wav], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    assert open(out, "rb").read() == want[1]
    # without -x the same file is refused as before: 1 Msps gives interpolation factor 0
    r = subprocess.run([exe, "-o", out, wav], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "interpolation factor would be 0" in r.stdout
    # a rate the decimation does not divide
    r = subprocess.run([exe, "-x", "7", "-t", "200", "-o", out, wav], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "not divisible" in r.stdout
    # ... and one it does: -x 3 on a 750 ksps file with one carrier
    x3, _ = carriers(pdt, 0, 750000, 6.0, (150000.0,), (13,), 1000.0)
    wav3 = str(tmp_path / "one_carrier_750k.wav")
    pdt.write_wav(wav3, 750000, x3)
    with pdt.Demodulator(pdt.MODE_POES, 250000) as d:
        d.set_channel(3, 150000.0).demod_channel(x3)
        want3 = d.text()
    assert len(want3) > 10000
    r = subprocess.run([exe, "-x", "3", "-t", "150", "-o", out, wav3], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    assert open(out, "rb").read() == want3
    # headerless 8-bit pairs, -s required
    cu8 = str(tmp_path / "two_carriers.cu8")
    u8 = to_cu8(x)
    u8.tofile(cu8)
    with pdt.Demodulator(pdt.MODE_POES, fs) as d:
        d.set_channel(D, 200000.0).demod_channel(u8)
        want8 = d.text()
    r = subprocess.run([exe, "-x", "4", "-t", "200", "-s", "1000", "-o", out, cu8], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    assert open(out, "rb").read() == want8
    r = subprocess.run([exe, "-x", "4", "-t", "200", "-o", out, cu8], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "must be specified" in r.stdout
    # -l -x .. -t .. - : blocks of unsigned 8-bit pairs from a pipe through the stream entry
    with pdt.Demodulator(pdt.MODE_POES, fs, chunk=2400, chain=pdt.CHAIN_LIVE) as d:
        d.set_channel(D, 200000.0)
        fr = [d.stream_push_channel(u8[i: i + 2400 * D]) for i in range(0, len(u8), 2400 * D)] + [d.stream_end()]
        want_live = pdt.format_frames(np.concatenate(fr))
    assert len(want_live) > 100
    r = subprocess.run([exe, "-l", "-x", "4", "-t", "200", "-s", "1000", "-o", out, "-"], input=u8.tobytes(), capture_output=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    assert open(out, "rb").read() == want_live
