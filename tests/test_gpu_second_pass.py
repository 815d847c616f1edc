"""What the second-pass entries share (one kernel timer, one staging path, one delivery of records), seen across
entries on ONE context, where no single entry's test looks: every call of a sequence gives what it gives on a fresh context that did only
its prerequisites (the staging buffers carry nothing over), the kernel times hold every second-pass name at most once with the right
launch count and leave the chain's own entries alone, and a repeated call adds no entry.  Then the edges of the shared delivery through
the batch entries: cap 0 and a cap below the number found, the count returned whole.

Asserted elsewhere and not repeated here: a staged string of length 0 (tip_sync_cases.py:160 through test_gpu_tip_sync.py:50-53,
argos_msg_cases.py:76 through test_gpu_argos_messages.py:35-37; no soft values and no records: the hand cases "no-soft" and "no-records"
through test_gpu_tip_repair.py:40-43); cap 0 and a cap below the number found through the stage entries (test_gpu_tip_sync.py:95-97,
test_gpu_argos_messages.py:59-62)."""
import ctypes as C

import numpy as np
import pytest

import ff_cases as fc
import ffp_cases as pc
import tip_repair_cases as rc

pytestmark = pytest.mark.gpu

TONES = ("k_tones",)
ARGOS = ("k_argos_msgs", "k_argos_finish")
TIP_SYNC = ("k_tip_cand", "k_tip_heads", "k_tip_pick", "k_tip_scan", "k_tip_pack")
FF = ("k_ff_mix", "k_ff_search", "k_ff_pick")
FFP = ("k_ffp_mix", "k_ffp_search", "k_ffp_track", "k_ffp_bits")
REPAIR = ("k_tip_repair",)
SECOND = set(TONES + ARGOS + ("k_argos_heads", "k_argos_pick") + TIP_SYNC + FF + FFP + REPAIR)


def raw_times(pdt, d):
    """pdt_kernel_times entry by entry (Demodulator.kernel_times() is a dict: it could not show a name twice)"""
    L = pdt.lib()
    n = L.pdt_kernel_times(d._h, None, 0)
    arr = (pdt.KernelTime * max(n, 1))()
    L.pdt_kernel_times(d._h, arr, n)
    return [(arr[i].name.decode(), int(arr[i].launches), float(arr[i].total_ms)) for i in range(n)]


def chain_entries(pdt, d):
    return [e for e in raw_times(pdt, d) if e[0] not in SECOND]


def check_times(pdt, d, chain, present, absent=()):
    """every second-pass name at most once, launches 1 (k_ffp_track: 2), the chain's own entries as they were; returns the entry count"""
    t = raw_times(pdt, d)
    names = [e[0] for e in t if e[0] in SECOND]
    assert len(names) == len(set(names)), names
    assert all(e[1] == (2 if e[0] == "k_ffp_track" else 1) and e[2] >= 0 for e in t if e[0] in SECOND), t
    assert [e for e in t if e[0] not in SECOND] == chain
    assert set(present) <= set(names) and not set(absent) & set(names), names
    return len(t)


def same_frames(a, b):
    """(frames, info) pairs, byte for byte"""
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def tip_sync_batch_counts(pdt, ds, cap):
    """pdt_tip_sync_batch with room for `cap` records per context (none at all for cap 0): (frames[len(ds), cap], the counts)"""
    hs = (C.c_void_p * len(ds))(*[d._h for d in ds])
    out, info = np.zeros((len(ds), max(cap, 1)), dtype=pdt.FRAME_DTYPE), np.zeros((len(ds), max(cap, 1)), dtype=pdt.TIP_SYNC_INFO_DTYPE)
    counts = (C.c_int * len(ds))()
    assert pdt.lib().pdt_tip_sync_batch(hs, len(ds), None, out.ctypes.data if cap else None, info.ctypes.data if cap else None, cap, counts) == 0
    return out[:, :cap], info[:, :cap], list(counts)


def test_poes_sequence_on_one_context(pdt):
    p, x = rc.weak_capture(pdt, 3, 9.0, seconds=3.0)                          # 3 s at 50 ksps, frames that carry parity, noise x 9
    xx = np.repeat(x, 2, axis=0)                                              # (the capture at twice its rate: a zero-order hold)
    y = x.astype(np.float32) / np.float32(32768.0)

    def fresh(**kw):
        return pdt.Demodulator(pdt.MODE_POES, 50000, **kw).set_channel(2, 0.0)

    with fresh(profile=True) as d:
        d.demod_channel(xx)
        chain = chain_entries(pdt, d)
        assert len(chain) > 5 and check_times(pdt, d, chain, ()) == len(chain)

        # tones
        tones = d.tones()
        n = check_times(pdt, d, chain, TONES, TIP_SYNC + FFP + REPAIR)
        with fresh() as f:
            assert f.demod_channel(xx).tones().tobytes() == tones.tobytes() and len(tones) > 3
        assert d.tones().tobytes() == tones.tobytes() and check_times(pdt, d, chain, TONES) == n == len(chain) + 1

        # feed-forward bits and their frames, then the repair of those
        frames = d.ffp_frames(with_info=True)
        n = check_times(pdt, d, chain, TONES + FFP + TIP_SYNC, REPAIR)
        fixed = d.tip_repair(frames[0])
        n2 = check_times(pdt, d, chain, TONES + FFP + TIP_SYNC + REPAIR)
        bits = d.ffp_read()
        with fresh() as f:
            f.demod_channel(xx)
            assert same_frames(f.ffp_frames(with_info=True), frames) and len(frames[0]) > 20
            assert pc.same_bits(f.ffp_read(), bits)
            assert rc.same(f.tip_repair(frames[0]), fixed) and fixed[2]["failing"] > 0
        assert same_frames(d.ffp_frames(with_info=True), frames) and rc.same(d.tip_repair(frames[0]), fixed)
        assert check_times(pdt, d, chain, TONES + FFP + TIP_SYNC + REPAIR) == n2 == n + 1 == len(chain) + 11

        # the stage entries, on strings from elsewhere: a shorter string after a longer one, an empty one after that
        string = bits.bits.tobytes()
        want = pdt.host_tip_sync(string, with_info=True)
        for s in (string, string[:5000], b"", string):
            got = d.stage_tip_sync(s, with_info=True)
            with fresh() as f:
                assert same_frames(f.stage_tip_sync(s, with_info=True), got), len(s)
            assert check_times(pdt, d, chain, TONES + FFP + TIP_SYNC + REPAIR) == n2
        assert same_frames(got, want) and len(want[0]) == len(frames[0])
        soft = np.concatenate([bits.soft, bits.soft[::-1]])                   # (other values than the context's own, and more of them)
        for s in (soft, soft[:4000], soft):
            got = d.stage_tip_repair(s, frames[0])
            with fresh() as f:
                assert rc.same(f.stage_tip_repair(s, frames[0]), got), len(s)
            assert check_times(pdt, d, chain, TONES + FFP + TIP_SYNC + REPAIR) == n2
        assert rc.same(got, pdt.host_tip_repair(soft, frames[0]))
        assert pc.same_bits(d.ffp_read(), bits) and rc.same(d.tip_repair(frames[0]), fixed)      # (the context's own bits stayed)

        # a plain demodulation: the chain's entries are new, the second-pass ones are gone; the flywheel on the resident bits
        d.demod(x)
        chain = chain_entries(pdt, d)
        assert check_times(pdt, d, chain, (), SECOND) == len(chain)
        fly = d.tip_sync(with_info=True)
        n = check_times(pdt, d, chain, TIP_SYNC, TONES + FFP + REPAIR)
        with fresh() as f:
            assert same_frames(f.demod(x).tip_sync(with_info=True), fly) and len(fly[0]) > 3
        assert same_frames(d.tip_sync(with_info=True), fly) and check_times(pdt, d, chain, TIP_SYNC) == n == len(chain) + 5

        # the shared delivery through the batch entry: no room at all, and less room than records; the count is whole either way
        found = len(fly[0])
        out, info, counts = tip_sync_batch_counts(pdt, [d], 0)
        assert counts == [found] and out.shape == (1, 0)
        with fresh() as f:
            f.demod(x[:100000])
            short = f.tip_sync(with_info=True)
            out, info, counts = tip_sync_batch_counts(pdt, [d, f], found - 1)
            assert counts == [found, len(short[0])] and 0 < len(short[0]) < found - 1
            assert out[0].tobytes() == fly[0][:found - 1].tobytes() and info[0].tobytes() == fly[1][:found - 1].tobytes()
            assert out[1, :len(short[0])].tobytes() == short[0].tobytes() and info[1, :len(short[0])].tobytes() == short[1].tobytes()
            assert not out[1, len(short[0]):].tobytes().strip(b"\0")          # (nothing is written behind a stream's records)

        # the stage entry of the feed-forward bits: the staged stream shares nothing with the channel stream's results
        got = d.stage_ffp_bits(50000, y[:60000])
        n = check_times(pdt, d, chain, TIP_SYNC + FFP, TONES + REPAIR)
        with fresh() as f:
            assert pc.same_bits(f.stage_ffp_bits(50000, y[:60000]), got)
        assert 9900 < len(got.bits) <= 9984                                   # (60 000 samples at 8 320 bit/s: 9 984 bit times, less the edges)
        assert pc.same_bits(d.stage_ffp_bits(50000, y[:60000]), got) and check_times(pdt, d, chain, TIP_SYNC + FFP) == n == len(chain) + 9
        assert same_frames(d.tip_sync(with_info=True), fly)


def test_argos_sequence_on_one_context(pdt):
    y = fc.burst(0.0)                                                         # one burst, 0.96 s at 16 ksps
    xw = np.ascontiguousarray(np.repeat(y, 2, axis=0))                        # ... as a wideband capture at twice that rate
    window = [pdt.Window(0, len(xw), 0.0)]

    def fresh(**kw):
        return pdt.Demodulator(pdt.MODE_ARGOS, fc.BURST_FS, **kw).set_channel(2, 0.0)

    with fresh(profile=True) as d:
        pdt.demod_windows([d], xw, len(xw), 0, window)
        chain = chain_entries(pdt, d)
        assert len(chain) > 5 and check_times(pdt, d, chain, ()) == len(chain)

        # feed-forward bits and their messages: only pdt_tones* records k_tones, though the carrier is measured here too
        msgs, sync = d.ff_messages(with_sync=True)
        n = check_times(pdt, d, chain, FF + ARGOS, TONES + ("k_argos_heads", "k_argos_pick"))
        assert n == len(chain) + 5 and int(sync["tone_valid"]) == 1 and len(msgs) == 1
        bits = d.ff_read()
        with fresh() as f:
            pdt.demod_windows([f], xw, len(xw), 0, window)
            m2, s2 = f.ff_messages(with_sync=True)
            assert m2.tobytes() == msgs.tobytes() and s2.tobytes() == sync.tobytes() and fc.same_bits(f.ff_read(), bits)
        again = d.ff_messages(with_sync=True)
        assert again[0].tobytes() == msgs.tobytes() and again[1].tobytes() == sync.tobytes() and check_times(pdt, d, chain, FF + ARGOS) == n

        # no room at all through the batch entry: the count is whole
        hs, counts = (C.c_void_p * 1)(d._h), (C.c_int * 1)()
        syncs = np.zeros(1, dtype=pdt.FF_SYNC_DTYPE)
        assert pdt.lib().pdt_ff_messages_batch(hs, 1, None, None, syncs.ctypes.data, None, 0, counts) == 0
        assert list(counts) == [1] and syncs[0].tobytes() == sync.tobytes()

        # the stage entries: a string, then a stream; the channel stream's bits give way to the staged stream's, as documented
        string = bits.bits.tobytes()
        for s in (string, string[:100], string):
            got = d.stage_argos_messages(s)
            with fresh() as f:
                assert f.stage_argos_messages(s).tobytes() == got.tobytes(), len(s)
            assert check_times(pdt, d, chain, FF + ARGOS, TONES) == n
        assert got.tobytes() == pdt.host_argos_messages(string).tobytes() and len(got) == 1
        staged = d.stage_ff_bits(fc.BURST_FS, y)
        assert check_times(pdt, d, chain, FF + ARGOS, TONES) == n
        with fresh() as f:
            assert fc.same_bits(f.stage_ff_bits(fc.BURST_FS, y), staged) and fc.burst_decodes(pdt, staged.bits)
        assert fc.same_bits(d.ff_read(), staged) and fc.same_bits(d.stage_ff_bits(fc.BURST_FS, y[:9000]), pdt.host_ff_bits(fc.BURST_FS, y[:9000]))
        assert check_times(pdt, d, chain, FF + ARGOS, TONES) == n
