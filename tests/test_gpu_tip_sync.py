"""The flywheel frame synchroniser on the GPU: the kernels against the host restatement, byte for byte, on every string
of tests/tip_sync_cases.py -- the hand-derived cases, what sits on the seams of the kernels' tiles, the 200 random strings; after a
real demodulation, with everything else a context holds left as it was; one batch call against four single ones; error codes; the
kernels' names in a profiled context; the validation of a caller's records; and -W on the command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import test_tip_sync as cpu
import tip_sync_cases as tc
from conftest import GOLDEN, ROOT, golden_text

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "bin")
CLIP_WAV = os.path.join(GOLDEN, "5sec_clip.wav")
KERNELS = ("k_tip_cand", "k_tip_heads", "k_tip_pick", "k_tip_scan", "k_tip_pack")


@pytest.fixture(scope="module")
def poes(pdt):
    with pdt.Demodulator(pdt.MODE_POES, 50000) as d:
        yield d


def stage(d, bits, cfg=None, **kw):
    e, w, g = cfg or (None, None, None)
    return d.stage_tip_sync(bits, e, w, g, with_info=True, **kw)


def same(got, want) -> bool:
    return got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def held(pdt, d, alloc: bool = True):
    """what a context holds after a whole-capture call: frames, text, statistics and the bytes of every stage.  alloc = False: the
    statistics without alloc_ms -- the host time this PROCESS has spent allocating device memory so far, which a call that has to
    grow its work buffer moves; a second call of the same size must leave even that alone"""
    stages = tuple(d.stage(st).tobytes() if d.stage_len(st) else b"" for st in range(pdt.ST_CHANNEL + 1))
    s = d.stats()
    stats = bytes(s) if alloc else [(k, bytes(getattr(s, k)) if hasattr(getattr(s, k), "__len__") else getattr(s, k)) for k, _ in s._fields_
                                    if k != "alloc_ms"]
    return d.frames_array().tobytes(), d.text(), stats, stages


def test_stage_equals_host_on_the_case_list(pdt, poes):
    for name, bits, cfg, want in tc.cases():
        got = stage(poes, bits, cfg)
        assert same(got, cpu.host(pdt, bits, cfg)), name
        assert [{k: v for k, v in r.items() if k != "bytes"} for r in cpu.as_dicts(*got)] == want, name


def test_stage_at_tile_seams(pdt, poes):
    T = pdt.tip_sync_tile()
    cases = tc.seam_strings(T)
    assert len(cases) == 19 + 2 + 3 + 20 and max(len(c[1]) for c in cases) <= 6 * T
    for name, bits, cfg in cases:
        want = cpu.host(pdt, bits, cfg)
        assert len(want[0]) >= 2, name
        assert same(stage(poes, bits, cfg), want), name
    by = {c[0]: c for c in cases}
    # the cases hold what their names say: a sync word on every offset across the seam, a flywheel head in a tile of its own, both
    # outcomes of a conflict across the seam and the pair that does not conflict
    for k in range(19):
        assert 2 * T - 1 + k in cpu.host(pdt, by[f"straddle_{k}"][1])[0]["bit_index"]
    fr, info = cpu.host(pdt, by["flywheel_four_tiles"][1], (2, 8, 4))
    assert [int(c) for c in info["candidate"]] == [1, 1, 0, 1, 1] and len({int(p) // T for p in fr["bit_index"]}) == 5
    assert int(cpu.host(pdt, by["flywheel_across_seam"][1])[1]["candidate"].min()) == 0
    g = 2 * T - 400
    assert [int(p) for p in cpu.host(pdt, by["conflict_828_0"][1])[0]["bit_index"]] == [g - tc.F, g, g + 828 + tc.F]
    assert [int(p) for p in cpu.host(pdt, by["conflict_828_1"][1])[0]["bit_index"]] == [g - tc.F, g + 828, g + 828 + tc.F]
    assert [int(p) for p in cpu.host(pdt, by["conflict_829_0"][1])[0]["bit_index"]] == [g - tc.F, g, g + 829, g + 829 + tc.F]


def test_stage_on_random_strings(pdt, poes):
    records = 0
    for i, bits in enumerate(tc.random_strings()):
        got = stage(poes, bits)
        assert same(got, cpu.host(pdt, bits)), i
        records += len(got[0])
    assert records > 300
    for cfg in ((0, 1, 2), (3, 8, 2), (3, 8, 16), (1, 3, 6)):
        for i, bits in enumerate(tc.random_strings(8, seed=7)):
            assert same(stage(poes, bits, cfg), cpu.host(pdt, bits, cfg)), (cfg, i)


def test_stage_capacity_and_what_it_leaves_alone(pdt, poes, clip):
    bits = tc.random_strings(1, seed=3)[0] * 3
    want, found = cpu.host(pdt, bits, with_count=True)
    assert found == len(want[0]) >= 4
    for cap in (0, 1, found - 1):
        got, n = stage(poes, bits, cap=cap, with_count=True)
        assert n == found and same(got, (want[0][:cap], want[1][:cap])), cap
    frames = poes.stage_tip_sync(bits)                                        # without the info array
    assert frames.tobytes() == want[0].tobytes()
    # the stage entry works beside a capture's results, not on them
    poes.demod(clip[1][:60000])
    before = held(pdt, poes)
    stage(poes, bits)
    assert held(pdt, poes) == before                                          # (its buffers were large enough already)
    assert len(poes.tip_sync()) == len([f for f in poes.frames_array() if f["complete"]])


def test_real_recording_and_what_the_call_leaves_alone(pdt, poes, clip):
    rate, iq = clip
    poes.demod(iq)
    before = held(pdt, poes, alloc=False)
    fr, info = poes.tip_sync(with_info=True)
    assert held(pdt, poes, alloc=False) == before
    before = held(pdt, poes)
    again = poes.tip_sync(with_info=True)
    assert held(pdt, poes) == before and same(again, (fr, info))             # byte for byte, the statistics included
    own = poes.frames_array()
    assert len(own) == 48 and len(fr) == 47 and own[-1]["nbytes"] == 26
    assert fr.tobytes() == own[:47].tobytes()                                 # bytes, bit_index, time, time_src, inverted: the reference's frames
    assert (info["sync_errors"] == 0).all() and (info["candidate"] == 1).all()
    want = cpu.host(pdt, poes.stage(pdt.ST_BITS))
    for f in ("bit_index", "inverted", "nbytes", "complete", "bytes"):
        assert (fr[f] == want[0][f]).all(), f
    assert info.tobytes() == want[1].tobytes()
    assert pdt.format_frames(fr) + pdt.format_frames(own[47:]) == poes.text()
    # the validation of a caller's records: the flywheel's frames, against the oracle's restatement of the reference's MATLAB
    from oracle import binding as orc
    held_before = held(pdt, poes, alloc=False)
    summary, per_frame = poes.tip_check_records(fr)
    want_sm, want_rec = orc.tip_check([(round(float(f["time"]) * 1e5) / 1e5, bytes(f["bytes"]), 1) for f in fr])
    assert summary == want_sm and per_frame.tobytes() == want_rec.tobytes() and summary["frames_checked"] == 47
    own_sm, own_rec = poes.tip_check()
    assert summary == own_sm and per_frame.tobytes() == own_rec[:47].tobytes()
    again, _ = poes.tip_check_records(fr[:10])                                # (the context's own validation results stay, too)
    assert again["frames_checked"] == 10 and poes.tip_check()[1].tobytes() == own_rec.tobytes() and held(pdt, poes, alloc=False) == held_before
    assert poes.tip_check_records(fr[:0])[0]["frames_checked"] == 0


def test_weak_capture_equals_host_on_its_bits(pdt, poes):
    p, x = cpu.weak_capture(pdt)
    poes.demod(x)
    before = held(pdt, poes, alloc=False)
    fr, info = poes.tip_sync(with_info=True)
    assert held(pdt, poes, alloc=False) == before
    want = cpu.host(pdt, poes.stage(pdt.ST_BITS))
    for f in ("bit_index", "inverted", "nbytes", "complete", "bytes"):
        assert (fr[f] == want[0][f]).all(), f
    assert info.tobytes() == want[1].tobytes() and len(fr) > 250
    # the time stamp is a frame's: the interpolated sample behind the bit, and through the context's time axis exactly the stamp of
    # the reference's own frame wherever both synchronisers have one at that bit
    bitsym, symidx = poes.stage(pdt.ST_BITSYM), poes.stage(pdt.ST_SYMIDX)
    assert [int(v) for v in fr["time_src"]] == [int(symidx[bitsym[int(p)]]) for p in fr["bit_index"]]
    own = {int(f["bit_index"]): f for f in poes.frames_array() if f["complete"]}
    shared = [r for r in fr if int(r["bit_index"]) in own]
    assert len(shared) > 200 and (np.diff(fr["time"]) > 0).all()
    for r in shared:
        assert r.tobytes() == own[int(r["bit_index"])].tobytes()
    ref = cpu.placed(pdt, p, [bytes(f["bytes"]) for f in poes.frames_array() if f["complete"]])
    fly = cpu.placed(pdt, p, [bytes(v) for v in fr["bytes"]])
    print(f"rule 0: {ref[0]} placed / {ref[1]} not; flywheel: {fly[0]} placed / {fly[1]} not")
    assert fly[0] > ref[0] and fly[1] <= ref[1]
    for cfg in ((1, 2, 3), (2, 2, 2), (2, 3, 3), (3, 2, 3)):
        got = poes.tip_sync(*cfg, with_info=True)
        want = cpu.host(pdt, poes.stage(pdt.ST_BITS), cfg)
        assert (got[0]["bit_index"] == want[0]["bit_index"]).all() and got[0]["bytes"].tobytes() == want[0]["bytes"].tobytes(), cfg
        assert got[1].tobytes() == want[1].tobytes(), cfg


def test_batch_equals_single_calls_in_one_launch(pdt, clip):
    noise_p = pdt.synth_params(0, 50000, 1000.0, 9)
    noise_p.amplitude = 0
    noise = np.zeros((90000, 2), dtype="<i2")
    pdt.synth_lib().pdt_synth_fill(C.byref(noise_p), 0, len(noise), noise.ctypes.data)
    caps = [np.ascontiguousarray(clip[1]), pdt.synth_capture(0, 50000, 6.0, seed=1), noise, cpu.weak_capture(pdt, seconds=9.5)[1]]
    dev = [torch.from_numpy(iq.reshape(-1).copy()).to("cuda:0") for iq in caps]
    torch.cuda.synchronize()
    ds = [pdt.Demodulator(pdt.MODE_POES, 50000, profile=(i == 0)) for i in range(len(caps))]
    try:
        pdt.demod_batch(ds, [t.data_ptr() for t in dev], [len(iq) for iq in caps])
        single = [d.tip_sync(with_info=True) for d in ds]
        counts = [len(s[0]) for s in single]
        assert counts[0] == 47 and counts[1] > 40 and counts[2] <= 2 and counts[3] > 50 and len(set(counts)) == 4
        for d, s in zip(ds, single):
            want = cpu.host(pdt, d.stage(pdt.ST_BITS))
            assert (s[0]["bit_index"] == want[0]["bit_index"]).all() and s[1].tobytes() == want[1].tobytes()
        for cfg in (None, (3, 3, 2)):
            e, w, g = cfg or (None, None, None)
            want = [d.tip_sync(e, w, g, with_info=True) for d in ds]
            got = pdt.tip_sync_batch(ds, e, w, g, with_info=True)
            assert [same(a, b) for a, b in zip(got, want)] == [True] * 4, cfg
            times = ds[0].kernel_times()
            assert all(times[k][0] == 1 for k in KERNELS), times
        small = pdt.tip_sync_batch(ds, cap=3)
        assert [len(s) for s in small] == [min(c, 3) for c in counts] and small[3].tobytes() == single[3][0][:3].tobytes()
        assert pdt.tip_sync_batch([]) == []
        # contexts on the error list are refused before anything runs
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            pdt.tip_sync_batch([ds[0], ds[1], ds[0]])
        with pdt.Demodulator(pdt.MODE_POES, 50000) as fresh:
            with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
                pdt.tip_sync_batch([ds[0], fresh])
        assert [same(d.tip_sync(with_info=True), s) for d, s in zip(ds, single)] == [True] * 4
    finally:
        for d in ds:
            d.close()


def test_error_codes(pdt, poes, clip):
    rate, iq = clip
    poes.demod(iq[:60000])
    n = len(poes.tip_sync())
    assert n >= 5
    for bad in ((-1, None, None), (4, None, None), (None, 9, None), (None, -1, None), (None, None, 1), (None, None, 5), (None, 1, None)):
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            poes.tip_sync(*bad)
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            poes.stage_tip_sync(b"0101", *bad)
    with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
        poes.tip_sync(cap=-1)
    assert len(poes.tip_sync()) == n                                          # a refused call changed nothing
    with pdt.Demodulator(pdt.MODE_ARGOS, 32000) as argos:
        argos.demod(np.zeros((40000, 2), dtype=np.int16))
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            argos.tip_sync()                                                  # an ARGOS context
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            argos.stage_tip_sync(b"0101")
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            argos.tip_check_records(np.zeros(1, dtype=pdt.FRAME_DTYPE))
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            pdt.tip_sync_batch([poes, argos])
    with pdt.Demodulator(pdt.MODE_POES, rate) as d:
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.tip_sync()                                                      # nothing demodulated yet
        d.demod(iq[:60000])
        assert len(d.tip_sync()) == n
        d.stream_begin()
        d.stream_push(iq[:20000])
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.tip_sync()                                                      # an open stream
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.stage_tip_sync(b"0101")
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            pdt.tip_sync_batch([poes, d])
        d.stream_end()
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.tip_sync()                                                      # ... and an ended one
        d.demod(iq[:60000])
        assert len(d.tip_sync()) == n
        d.bytesync(np.frombuffer(b"0101" * 50, dtype=np.uint8))
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.tip_sync()                                                      # a stage-level call took the bit buffer


def test_profiled_context_names_the_kernels(pdt, clip):
    with pdt.Demodulator(pdt.MODE_POES, 50000, profile=True) as d:
        d.demod(clip[1])
        assert not any(k in d.kernel_times() for k in KERNELS)
        assert len(d.tip_sync()) == 47
        times = d.kernel_times()
        assert all(times[k][0] == 1 and times[k][1] >= 0 for k in KERNELS), times
        d.tip_sync()
        assert all(d.kernel_times()[k][0] == 1 for k in KERNELS)


def test_command_line(pdt, poes, clip, tmp_path):
    exe = os.path.join(BIN, "demodPOES")
    out, fly = str(tmp_path / "minor.txt"), str(tmp_path / "fly.txt")
    r = subprocess.run([exe, "-q", "-W", fly, "-o", out, CLIP_WAV], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    assert open(out, "rb").read() == golden_text("clip.c10000.txt")
    poes.demod(clip[1])
    want = poes.frames_array()[:47]
    assert open(fly, "rb").read() == pdt.format_frames(want)
    assert "Flywheel frames: 47 -> " in r.stdout
    sm, _ = poes.tip_check_records(want)
    assert f"Flywheel: {sm['good_frames']} out of 47 Error Free Frames, {sm['good_chunks']} Good Chunks and {sm['bad_chunks']} Bad Chunks" in r.stdout
    # other constants reach the library
    r = subprocess.run([exe, "-W", fly, "-w", "0,1,2", "-o", out, CLIP_WAV], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and open(fly, "rb").read() == pdt.format_frames(poes.tip_sync(0, 1, 2))
    assert open(out, "rb").read() == golden_text("clip.c10000.txt")
    # refusals: demodARGOS, constants out of range, constants without a file
    ra = subprocess.run([os.path.join(BIN, "demodARGOS"), "-W", fly + "x", CLIP_WAV], capture_output=True, text=True, timeout=300)
    assert ra.returncode == 1 and "-W and -w need demodPOES" in ra.stdout and not os.path.exists(fly + "x")
    rw = subprocess.run([exe, "-W", fly + "x", "-w", "2,1,3", "-o", out + "x", CLIP_WAV], capture_output=True, text=True, timeout=300)
    assert rw.returncode == 1 and "-w E,W,G" in rw.stdout and not os.path.exists(fly + "x")
    # ... and a capture taken in pieces (the device pretends to have 64 MB): the message says why
    rp = subprocess.run([exe, "-D", "PDT_HBM_LIMIT_MB=64", "-P", "-W", fly + "x", "-o", out + "x", CLIP_WAV], capture_output=True, text=True, timeout=300)
    assert rp.returncode == 1 and "-W needs a capture taken in one piece" in rp.stdout and not os.path.exists(fly + "x")
    rn = subprocess.run([exe, "-w", "2,2,3", CLIP_WAV], capture_output=True, text=True, timeout=300)
    assert rn.returncode == 1 and "-w sets the constants of -W" in rn.stdout
