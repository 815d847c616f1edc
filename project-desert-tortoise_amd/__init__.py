"""project-desert-tortoise_amd -- MI355X (gfx950) POES-TIP / ARGOS IQ demodulation chain.

Python is only a thin ctypes veneer over ``csrc/libpdt.so`` (hand-written HIP kernels behind the
C ABI of ``include/pdt.h``) and ``synth/libpdtsynth.so`` (integer-only synthetic captures).
There is **no CPU fallback**: if the HIP library is missing, or no GPU is visible when a
context is opened, the call fails loudly.

The directory name contains hyphens, so import it with::

    import importlib; pdt = importlib.import_module("project-desert-tortoise_amd")

Reference behaviour mirrored here (file:line in nebarnix/Project-Desert-Tortoise):
  * ``Demodulator`` == one run of the chunk loop POESTIPdemod/main.c:373-492 or
    ARGOSdemod/main.c:250-306 over a whole capture.
  * ``Demodulator.text()`` == the bytes POESTIPdemod/ByteSync.c:62-69,96-101 /
    ARGOSdemod/ByteSync.c:62-70,99-103 write to minorFrames_*.txt / packets_*.txt.
"""
from __future__ import annotations

import collections
import ctypes as C
import os
import struct

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIBPDT_PATH = os.environ.get("PDT_LIBPDT_PATH") or os.path.join(_HERE, "csrc", "libpdt.so")   # override: tuning experiments only
LIBSYNTH_PATH = os.path.join(_HERE, "synth", "libpdtsynth.so")

MODE_POES, MODE_ARGOS = 0, 1
SAMPLER_GARDNER, SAMPLER_MM = 0, 1
CHAIN_FILE, CHAIN_LIVE = 0, 1          # CHAIN_LIVE: the sound-card twin's constants and stage order (POES)
ST_PLL, ST_LOCK, ST_FIR, ST_AGC, ST_SYM, ST_SYMIDX, ST_BITS, ST_BITSYM, ST_AGC_RAW, ST_ANALYTIC, ST_CHANNEL = range(11)
FMT_PCM16, FMT_F32, FMT_REAL_PCM16, FMT_REAL_F32 = range(4)    # I,Q int16 / I,Q float32 / one int16 / one float32 per frame


# wideband I,Q captures (set_channel): int16 pairs / float32 pairs / unsigned 8-bit pairs / signed 8-bit pairs
FMT_WB_PCM16, FMT_WB_F32, FMT_WB_CU8, FMT_WB_CS8 = range(16, 20)


class PdtError(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [
        ("mode", C.c_int32),
        ("sample_rate", C.c_uint32),
        ("chunk", C.c_uint64),
        ("norm_override", C.c_double),
        ("device", C.c_int32),
        ("profile", C.c_int32),
        ("pll_block", C.c_uint32),
        ("pll_warm", C.c_uint32),
        ("agc_block", C.c_uint32),
        ("agc_warm", C.c_uint32),
        ("gardner_band_pad", C.c_double),
        ("sampler", C.c_int32),
        ("chain", C.c_int32),
        ("mm_step_range", C.c_double),
        ("mm_kp", C.c_double),
    ]


class LoopParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("pll_freq_range_hz", "pll_lock_threshold", "pll_lock_alpha", "pll_loopbw_acq", "pll_loopbw_track",
                                          "agc_attack", "agc_decay", "gardner_baud", "gardner_step_range", "gardner_kp", "manchester_threshold")] \
               + [("zero_mask", C.c_uint32), ("reserved_", C.c_uint32)]


class Frame(C.Structure):
    _fields_ = [
        ("time", C.c_double),
        ("bit_index", C.c_int64),
        ("time_src", C.c_int64),
        ("inverted", C.c_uint8),
        ("nbytes", C.c_uint8),
        ("complete", C.c_uint8),
        ("pad", C.c_uint8),
        ("bytes", C.c_uint8 * 104),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("samples", C.c_uint64),
        ("out_samples", C.c_uint64),
        ("symbols", C.c_uint64),
        ("bits", C.c_uint64),
        ("frames", C.c_uint64),
        ("lock_sample", C.c_int64),
        ("lock_freq_hz", C.c_double),
        ("norm_factor", C.c_double),
        ("avg_phase", C.c_double),
        ("interp", C.c_uint32),
        ("ntaps", C.c_uint32),
        ("pll_blocks", C.c_uint32),
        ("pll_seam_fixes", C.c_uint32),
        ("agc_blocks", C.c_uint32),
        ("agc_seam_fixes", C.c_uint32),
        ("gpu_ms", C.c_double),
        ("gardner_parallel", C.c_uint32),
        ("gardner_walked", C.c_uint32),
        ("gardner_full_domain", C.c_uint32),
        ("sync_overflow", C.c_uint32),
        ("gardner_candidates", C.c_uint64),
        ("ingest_ms", C.c_double),
        ("alloc_ms", C.c_double),
        ("segments", C.c_uint32),
        ("windowed", C.c_uint32),
        ("ingest_direct", C.c_uint32),
        ("ingest_numa_node", C.c_int32),
    ]


class TipSummary(C.Structure):
    _fields_ = [("frames_checked", C.c_uint64), ("good_frames", C.c_uint64), ("good_chunks", C.c_uint64),
                ("bad_chunks", C.c_uint64), ("spacecraft", C.c_int32), ("day", C.c_int32), ("t0_ms", C.c_int64),
                ("time_frames", C.c_uint64)]


PROGRESS_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p)     # == pdt_progress_fn
# == pdt_chunk_report (48 bytes): what the reference's chunk loop knows after every chunk
CHUNK_DTYPE = np.dtype([("samples", "<u8"), ("avg_phase", "<f8"), ("symbols", "<u8"), ("bits", "<u8"), ("frames", "<u8"),
                        ("time0", "<f8")])

TIP_DTYPE = np.dtype([("minor_id", "<u2"), ("spacecraft", "u1"), ("parity", "u1"), ("checked", "u1"), ("has_time", "u1"),
                      ("day", "<u2"), ("day_ms", "<i4")])        # == pdt_tip_frame (12 bytes)


class ManchesterState(C.Structure):
    """pdt_manchester_state: ManchesterDecode's statics (a zeroed record = before the first call)"""
    _fields_ = [("current", C.c_double), ("previous", C.c_double), ("clockmod", C.c_uint32), ("even_odd", C.c_uint32)]


class PllState(C.Structure):
    """pdt_pll_state: CarrierTrackPLL's statics (a zeroed record = before the first call)"""
    _fields_ = [("started", C.c_int32), ("locked", C.c_int32), ("lock_index", C.c_int64), ("lock_freq_hz", C.c_double),
                ("phase", C.c_double), ("freq", C.c_double), ("avg_phase", C.c_double), ("locksig", C.c_double),
                ("sweep", C.c_double)]


class GardnerState(C.Structure):
    """pdt_gardner_state: GardenerClockRecovery's statics (a zeroed record = before the first call)"""
    _fields_ = [("next_sample", C.c_double), ("prev_bit", C.c_double), ("half_sample", C.c_double)]


class MmState(C.Structure):
    """pdt_mm_state: MMClockRecovery's statics (a zeroed record = before the first call)"""
    _fields_ = [("started", C.c_int32), ("pad", C.c_int32), ("next_sample", C.c_double), ("step_size", C.c_double),
                ("sample_last", C.c_double)]


class AgcState(C.Structure):
    """pdt_agc_state: NormalizingAGC's static gain (a zeroed record = before the first call)"""
    _fields_ = [("started", C.c_int32), ("pad", C.c_int32), ("gain", C.c_double)]


class FirState(C.Structure):
    """pdt_fir_state: the low-pass filter's ring (a zeroed record = before the first call)"""
    _fields_ = [("count", C.c_uint64), ("history", C.c_double * 64)]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("launches", C.c_uint32), ("total_ms", C.c_double)]


class SurveyCfg(C.Structure):
    """pdt_survey_cfg: a zero means the default"""
    _fields_ = [("nfft", C.c_int), ("max_carriers", C.c_int), ("threshold_db", C.c_double), ("guard_hz", C.c_double), ("merge_hz", C.c_double),
                ("first_frame", C.c_uint64), ("nframes", C.c_uint64)]


class CarrierRec(C.Structure):
    """pdt_carrier"""
    _fields_ = [("offset_hz", C.c_double), ("peak_db", C.c_float), ("floor_power", C.c_float)]


Carrier = collections.namedtuple("Carrier", "offset_hz peak_db floor_power")


def _survey_cfg(cfg: dict):
    """keyword arguments of a survey -> (pdt_survey_cfg or None, capacity of the result)"""
    unknown = set(cfg) - {f[0] for f in SurveyCfg._fields_}
    if unknown:
        raise TypeError(f"unknown survey parameter(s): {sorted(unknown)}")
    return (SurveyCfg(**cfg) if cfg else None), max(int(cfg.get("max_carriers", 0)) or 16, 1)


class BurstsCfg(C.Structure):
    """pdt_bursts_cfg: a zero means the default"""
    _fields_ = [("nfft", C.c_int), ("rows_per", C.c_int), ("gap_rows", C.c_int), ("threshold_db", C.c_double), ("guard_hz", C.c_double),
                ("merge_hz", C.c_double), ("min_s", C.c_double), ("max_s", C.c_double), ("first_frame", C.c_uint64), ("nframes", C.c_uint64)]


class BurstRec(C.Structure):
    """pdt_burst"""
    _fields_ = [("first_row", C.c_uint64), ("rows", C.c_uint64), ("start_s", C.c_double), ("duration_s", C.c_double), ("offset_hz", C.c_double),
                ("peak_db", C.c_float), ("floor_power", C.c_float)]


Burst = collections.namedtuple("Burst", "first_row rows start_s duration_s offset_hz peak_db floor_power")
ROW_PEAK_DTYPE = np.dtype([("bin", "<i4"), ("below", "<f4"), ("power", "<f4"), ("above", "<f4")])      # pdt_row_peak
BURST_ROW_PEAKS = 8


def _bursts_cfg(cfg: dict):
    """keyword arguments of a burst search -> (pdt_bursts_cfg or None, capacity of the result: `cap`, default 4096)"""
    cfg = dict(cfg)
    cap = int(cfg.pop("cap", 4096))
    unknown = set(cfg) - {f[0] for f in BurstsCfg._fields_}
    if unknown:
        raise TypeError(f"unknown burst search parameter(s): {sorted(unknown)}")
    return (BurstsCfg(**cfg) if cfg else None), cap


def _bursts(rec, count: int, cap: int):
    return [Burst(*(getattr(rec[i], f[0]) for f in BurstRec._fields_)) for i in range(min(count, cap))]


def burst_carriers(bursts, merge_hz: float, cap: int = 16):
    """pdt_burst_carriers: the platforms of a burst list (bursts within merge_hz of each other are one), strongest first, as
    Carrier(offset_hz, peak_db, floor_power) for set_channel."""
    rec = (BurstRec * max(len(bursts), 1))(*[BurstRec(*b) for b in bursts])
    out, n = (CarrierRec * max(cap, 1))(), C.c_int(0)
    _check(lib().pdt_burst_carriers(rec, len(bursts), float(merge_hz), out, cap, C.byref(n)), "pdt_burst_carriers")
    return _carriers(out, min(n.value, cap))


class WindowRec(C.Structure):
    """pdt_window"""
    _fields_ = [("first_frame", C.c_uint64), ("nframes", C.c_uint64), ("offset_hz", C.c_double)]


Window = collections.namedtuple("Window", "first_frame nframes offset_hz")


def _window_recs(windows):
    return (WindowRec * max(len(windows), 1))(*[WindowRec(int(w[0]), int(w[1]), float(w[2])) for w in windows])


def burst_windows(bursts, in_rate: int, capture_frames: int, skip_s: float = -1.0, tail_s: float = -1.0):
    """pdt_burst_windows: window i of burst i, a list of Window(first_frame, nframes, offset_hz) -- from skip_s behind the burst's
    start (negative: one row of the burst, so that the window begins inside the carrier) to tail_s behind its end (negative: 0.1 s),
    cut at the capture's end (host only)."""
    rec = (BurstRec * max(len(bursts), 1))(*[BurstRec(*b) for b in bursts])
    out = (WindowRec * max(len(bursts), 1))()
    _check(lib().pdt_burst_windows(rec, len(bursts), in_rate, capture_frames, float(skip_s), float(tail_s), out), "pdt_burst_windows")
    return [Window(out[i].first_frame, out[i].nframes, out[i].offset_hz) for i in range(len(bursts))]


class ToneCfg(C.Structure):
    """pdt_tone_cfg: a zero means the default"""
    _fields_ = [("nfft", C.c_int32), ("noise_lo", C.c_int32), ("noise_hi", C.c_int32), ("reserved_", C.c_int32), ("search_hz", C.c_double),
                ("first", C.c_uint64), ("stride", C.c_uint64), ("count", C.c_uint64)]


class ToneRec(C.Structure):
    """pdt_tone"""
    _fields_ = [("time_s", C.c_double), ("freq_hz", C.c_double), ("residual_hz", C.c_double), ("power", C.c_double), ("cn0_dbhz", C.c_double),
                ("valid", C.c_int32), ("bin", C.c_int32), ("below", C.c_float), ("peak", C.c_float), ("above", C.c_float), ("noise_sum", C.c_float),
                ("noise_bins", C.c_int32), ("reserved_", C.c_int32)]


# pdt_tone as a numpy record: the derived doubles, the valid flag, then the raw record as the kernel leaves it
TONE_DTYPE = np.dtype([("time_s", "<f8"), ("freq_hz", "<f8"), ("residual_hz", "<f8"), ("power", "<f8"), ("cn0_dbhz", "<f8"), ("valid", "<i4"),
                       ("bin", "<i4"), ("below", "<f4"), ("peak", "<f4"), ("above", "<f4"), ("noise_sum", "<f4"), ("noise_bins", "<i4"),
                       ("reserved_", "<i4")])


def _tone_cfg(cfg: dict):
    """keyword arguments of a carrier measurement -> (pdt_tone_cfg or None, capacity of the result: `cap`, default 4096)"""
    cfg = dict(cfg)
    cap = int(cfg.pop("cap", 4096))
    unknown = set(cfg) - {f[0] for f in ToneCfg._fields_}
    if unknown:
        raise TypeError(f"unknown tone parameter(s): {sorted(unknown)}")
    return (ToneCfg(**cfg) if cfg else None), cap


def host_tones(rate: int, offset_hz: float, iq: np.ndarray, **cfg) -> np.ndarray:
    """pdt_host_tones: the carrier measurement of a float32 I,Q stream at `rate` restated on the host (no GPU), bit for bit what the
    kernel and the host's derivation compute.  offset_hz: what a context's channel offset would be; cfg: fields of pdt_tone_cfg (nfft,
    search_hz, noise_lo, noise_hi, first, stride, count), zero or absent = the default, and cap.  Returns TONE_DTYPE[count]."""
    a = np.ascontiguousarray(iq, dtype="<f4").reshape(-1)
    c, cap = _tone_cfg(cfg)
    out, count = np.zeros(max(cap, 1), dtype=TONE_DTYPE), C.c_int(0)
    _check(lib().pdt_host_tones(rate, float(offset_hz), a.ctypes.data, a.size // 2, C.byref(c) if c else None, out.ctypes.data, cap, C.byref(count)),
           "pdt_host_tones")
    return out[:count.value]


def tones_batch(ds, **cfg):
    """pdt_tones_batch: Demod.tones() of several contexts of one device in ONE launch (the windows of a round of demod_windows_held):
    a list of TONE_DTYPE arrays, one per context."""
    c, cap = _tone_cfg(cfg)
    hs = (C.c_void_p * max(len(ds), 1))(*[d._h for d in ds])
    out, counts = np.zeros((max(len(ds), 1), max(cap, 1)), dtype=TONE_DTYPE), (C.c_int * max(len(ds), 1))()
    _check(lib().pdt_tones_batch(hs, len(ds), C.byref(c) if c else None, out.ctypes.data, cap, counts), "pdt_tones_batch")
    return [out[i, :counts[i]].copy() for i in range(len(ds))]


class ArgosCfg(C.Structure):
    """pdt_argos_cfg: a zero means the default; min_run 0 with ARGOS_ZERO_MIN_RUN in zero_mask asks for no run; rule = ARGOS_RULE_*"""
    _fields_ = [("min_run", C.c_int32), ("zero_mask", C.c_uint32), ("rule", C.c_int32), ("reserved_", C.c_int32)]


class ArgosMsg(C.Structure):
    """pdt_argos_msg"""
    _fields_ = [("time", C.c_double), ("bit_index", C.c_int64), ("time_src", C.c_int64), ("id", C.c_uint32), ("blocks", C.c_uint8),
                ("inverted", C.c_uint8), ("complete", C.c_uint8), ("run_value", C.c_uint8), ("data_bits", C.c_uint32), ("reserved_", C.c_uint32),
                ("data", C.c_uint8 * 32)]


ARGOS_ZERO_MIN_RUN = 1
ARGOS_RULE_FIRST, ARGOS_RULE_BEST = 0, 1         # PDT_ARGOS_RULE_*: the first head in ascending e (the default); the best head of a cluster
# pdt_argos_msg as a numpy record
ARGOS_MSG_DTYPE = np.dtype([("time", "<f8"), ("bit_index", "<i8"), ("time_src", "<i8"), ("id", "<u4"), ("blocks", "u1"), ("inverted", "u1"),
                            ("complete", "u1"), ("run_value", "u1"), ("data_bits", "<u4"), ("reserved_", "<u4"), ("data", "u1", (32,))])
assert ARGOS_MSG_DTYPE.itemsize == C.sizeof(ArgosMsg) == 72


def _argos_cfg(min_run, rule=None):
    """min_run (None = the default, 6) and rule (None = ARGOS_RULE_FIRST) -> pdt_argos_cfg or None; min_run 0 travels with its flag bit"""
    if min_run is None and rule is None:
        return None
    c = ArgosCfg(rule=int(rule or 0))
    if min_run is not None:
        c.min_run, c.zero_mask = int(min_run), ARGOS_ZERO_MIN_RUN if int(min_run) == 0 else 0
    return c


def argos_run_len(msgs):
    """PDT_ARGOS_MSG_RUN_LEN of records of rule ARGOS_RULE_BEST: the length of the run each head was taken with"""
    return np.asarray(msgs["reserved_"]) & 0xFF


def argos_slip(msgs):
    """PDT_ARGOS_MSG_SLIP of records of rule ARGOS_RULE_BEST: 1 where a stray bit stands between run and sync"""
    return (np.asarray(msgs["reserved_"]) >> 8) & 1


def _bit_string(bits) -> np.ndarray:
    """a string of '0'/'1' characters: bytes, or a uint8 array (any byte other than '0' is a one)"""
    if isinstance(bits, (bytes, bytearray)):
        return np.frombuffer(bytes(bits), dtype=np.uint8)
    return np.ascontiguousarray(bits, dtype=np.uint8).reshape(-1)


def argos_msg_tile() -> int:
    """pdt_argos_msg_tile: the bits one workgroup of k_argos_msgs tests"""
    return lib().pdt_argos_msg_tile()


def host_argos_messages(bits, min_run=None, cap: int = 4096, with_count: bool = False, rule=None):
    """pdt_host_argos_messages: the ARGOS messages in a string of '0'/'1' characters, restated on the host (no GPU); the time stamp of
    bit k is k.  rule: ARGOS_RULE_FIRST (None) or ARGOS_RULE_BEST.  Returns ARGOS_MSG_DTYPE[min(found, cap)]; with_count: (that, found)."""
    a, c = _bit_string(bits), _argos_cfg(min_run, rule)
    out, count = np.zeros(max(cap, 1), dtype=ARGOS_MSG_DTYPE), C.c_int(0)
    _check(lib().pdt_host_argos_messages(a.ctypes.data, a.size, C.byref(c) if c else None, out.ctypes.data, cap, C.byref(count)),
           "pdt_host_argos_messages")
    got = out[:min(count.value, cap)]
    return (got, count.value) if with_count else got


def argos_messages_batch(ds, min_run=None, cap: int = 4096, rule=None):
    """pdt_argos_messages_batch: Demodulator.argos_messages() of several contexts of one device with ONE launch of each kernel: a list of
    ARGOS_MSG_DTYPE arrays, one per context."""
    c = _argos_cfg(min_run, rule)
    hs = (C.c_void_p * max(len(ds), 1))(*[d._h for d in ds])
    out, counts = np.zeros((max(len(ds), 1), max(cap, 1)), dtype=ARGOS_MSG_DTYPE), (C.c_int * max(len(ds), 1))()
    _check(lib().pdt_argos_messages_batch(hs, len(ds), C.byref(c) if c else None, out.ctypes.data, cap, counts),
           "pdt_argos_messages_batch")
    return [out[i, :min(counts[i], cap)].copy() for i in range(len(ds))]


class TipSyncCfg(C.Structure):
    """pdt_tip_sync_cfg: a zero means the default; max_errors 0 with TIP_SYNC_ZERO_MAX_ERRORS in zero_mask asks for exact sync words"""
    _fields_ = [("max_errors", C.c_int32), ("window", C.c_int32), ("fly", C.c_int32), ("zero_mask", C.c_uint32)]


TIP_SYNC_ZERO_MAX_ERRORS = 1
# pdt_tip_sync_info as a numpy record: the distance, support and candidate bit of the polarity that stands
TIP_SYNC_INFO_DTYPE = np.dtype([("sync_errors", "u1"), ("support", "u1"), ("candidate", "u1"), ("reserved", "u1")])
assert TIP_SYNC_INFO_DTYPE.itemsize == 4


def _tip_sync_cfg(max_errors=None, window=None, fly=None):
    """the three constants of the flywheel's rule (None = the default: 2, 2, 3) -> pdt_tip_sync_cfg or None; max_errors 0 travels with
    its flag bit"""
    if max_errors is None and window is None and fly is None:
        return None
    c = TipSyncCfg(window=int(window or 0), fly=int(fly or 0))
    if max_errors is not None:
        c.max_errors, c.zero_mask = int(max_errors), TIP_SYNC_ZERO_MAX_ERRORS if int(max_errors) == 0 else 0
    return c


def _tip_sync_result(out, info, found: int, cap: int, with_info: bool, with_count: bool):
    n = min(found, cap)
    got = (out[:n].copy(), info[:n].copy()) if with_info else out[:n].copy()
    return (got, found) if with_count else got


def tip_sync_tile() -> int:
    """pdt_tip_sync_tile: the bits one workgroup of k_tip_cand tests"""
    return lib().pdt_tip_sync_tile()


def host_tip_sync(bits, max_errors=None, window=None, fly=None, cap: int = 65536, with_info: bool = False, with_count: bool = False):
    """pdt_host_tip_sync: the POES minor frames a flywheel synchroniser finds in a string of '0'/'1' characters, restated on the host
    (no GPU); the time stamp of bit k is k.  Returns FRAME_DTYPE[min(found, cap)]; with_info: (that, TIP_SYNC_INFO_DTYPE[..]);
    with_count: (that, found)."""
    a, c = _bit_string(bits), _tip_sync_cfg(max_errors, window, fly)
    out, info, count = np.zeros(max(cap, 1), dtype=FRAME_DTYPE), np.zeros(max(cap, 1), dtype=TIP_SYNC_INFO_DTYPE), C.c_int(0)
    _check(lib().pdt_host_tip_sync(a.ctypes.data, a.size, C.byref(c) if c else None, out.ctypes.data, info.ctypes.data, cap, C.byref(count)),
           "pdt_host_tip_sync")
    return _tip_sync_result(out, info, count.value, cap, with_info, with_count)


def tip_sync_batch(ds, max_errors=None, window=None, fly=None, cap: int = 65536, with_info: bool = False):
    """pdt_tip_sync_batch: Demodulator.tip_sync() of several contexts of one device with ONE launch of each kernel: a list of FRAME_DTYPE
    arrays (with_info: of (frames, info) pairs), one per context."""
    c = _tip_sync_cfg(max_errors, window, fly)
    hs = (C.c_void_p * max(len(ds), 1))(*[d._h for d in ds])
    out, info = np.zeros((max(len(ds), 1), max(cap, 1)), dtype=FRAME_DTYPE), np.zeros((max(len(ds), 1), max(cap, 1)), dtype=TIP_SYNC_INFO_DTYPE)
    counts = (C.c_int * max(len(ds), 1))()
    _check(lib().pdt_tip_sync_batch(hs, len(ds), C.byref(c) if c else None, out.ctypes.data, info.ctypes.data, cap, counts), "pdt_tip_sync_batch")
    return [_tip_sync_result(out[i], info[i], counts[i], cap, with_info, False) for i in range(len(ds))]


# pdt_tip_repair_info as a numpy record, and pdt_tip_repair_summary
TIP_REPAIR_INFO_DTYPE = np.dtype([("status", "u1"), ("failed", "u1"), ("pos", "<u2", (5,)), ("least", "<f4", (5,)), ("next", "<f4", (5,))])
assert TIP_REPAIR_INFO_DTYPE.itemsize == 52
TIP_REPAIR_NONE = 0xFFFF


class TipRepairSummary(C.Structure):
    _fields_ = [("checked", C.c_uint64), ("skipped", C.c_uint64), ("failing", C.c_uint64), ("repaired", C.c_uint64)]


def _tip_repair_result(a, info, sm):
    return a, info[:len(a)], {k: int(getattr(sm, k)) for k, _ in TipRepairSummary._fields_}


def host_tip_repair(soft, frames):
    """pdt_host_tip_repair: the failed parity groups of POES minor frames repaired from the soft bit values, restated on the host (no
    GPU).  soft: float32[n], value k belongs to bit k of the stream the FRAME_DTYPE records were found in.  Returns (the repaired copy of
    the records, TIP_REPAIR_INFO_DTYPE[len], summary dict); `failed` is the parity record to keep -- repaired records pass every check."""
    s = np.ascontiguousarray(soft, dtype="<f4").reshape(-1)
    a = np.array(frames, dtype=FRAME_DTYPE, copy=True).reshape(-1)
    info, sm = np.zeros(max(len(a), 1), dtype=TIP_REPAIR_INFO_DTYPE), TipRepairSummary()
    _check(lib().pdt_host_tip_repair(s.ctypes.data, s.size, a.ctypes.data, len(a), info.ctypes.data, C.byref(sm)), "pdt_host_tip_repair")
    return _tip_repair_result(a, info, sm)


# pdt_dcs_packet as a numpy record, pdt_dcs_cfg and pdt_dcs_summary
DCS_PACKET_DTYPE = np.dtype([("time", "<f8"), ("stream_index", "<i8"), ("frame", "<u4"), ("time_code", "<u4"), ("id", "<u4"), ("doppler_raw", "<i4"),
                             ("slot", "u1"), ("channel", "u1"), ("blocks", "u1"), ("nbytes", "u1"), ("complete", "u1"), ("doppler_ok", "u1"),
                             ("pad", "u1", (2,)), ("bytes", "u1", (44,)), ("_tail", "u1", (4,))])     # the C struct is padded to 88
assert DCS_PACKET_DTYPE.itemsize == 88


class DcsCfg(C.Structure):
    _fields_ = [("channel_max", C.c_uint32), ("reserved", C.c_uint32)]


class DcsSummary(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("used", "skipped", "segments", "stream_bytes", "heads", "shadowed", "bad_code", "packets", "complete",
                                          "doppler_bad")]


def _dcs_result(out, count: int, cap: int, sm):
    return out[:min(count, cap)], count, {k: int(getattr(sm, k)) for k, _ in DcsSummary._fields_}


def tip_dcs_tile() -> int:
    """pdt_tip_dcs_tile: the stream bytes one tile of the DCS kernels covers (tests place packets at its seams)"""
    return int(lib().pdt_tip_dcs_tile())


def host_tip_dcs(frames, channel_max: int = 0, cap: int = 65536):
    """pdt_host_tip_dcs: the DCS-2 platform messages that FRAME_DTYPE records of TIP minor frames relay, restated on the host (no GPU).
    channel_max: the channel byte's bound (0 = 8; 9 for NOAA-19).  Returns (DCS_PACKET_DTYPE[min(found, cap)], found, summary dict)."""
    a = np.ascontiguousarray(frames, dtype=FRAME_DTYPE).reshape(-1)
    c = DcsCfg(channel_max, 0)
    out, count, sm = np.zeros(max(cap, 1), dtype=DCS_PACKET_DTYPE), C.c_int(0), DcsSummary()
    _check(lib().pdt_host_tip_dcs(a.ctypes.data, len(a), C.byref(c), out.ctypes.data if cap else None, cap, C.byref(count), C.byref(sm)), "pdt_host_tip_dcs")
    return _dcs_result(out, count.value, cap, sm)


def format_dcs_packets(packets: np.ndarray) -> bytes:
    """pdt_format_dcs_packets: one line per packet (host-only C, no GPU needed)"""
    a = np.ascontiguousarray(packets, dtype=DCS_PACKET_DTYPE).reshape(-1)
    L = lib()
    n = L.pdt_format_dcs_packets(a.ctypes.data, len(a), None, 0)
    buf = C.create_string_buffer(n + 1)
    L.pdt_format_dcs_packets(a.ctypes.data, len(a), buf, n)
    return buf.raw[:n]


def write_dcs_packets(packets: np.ndarray, fd: int) -> int:
    """pdt_write_dcs_packets: the same text to an open file descriptor; returns the bytes written"""
    a = np.ascontiguousarray(packets, dtype=DCS_PACKET_DTYPE).reshape(-1)
    w = C.c_uint64(0)
    _check(lib().pdt_write_dcs_packets(a.ctypes.data, len(a), fd, C.byref(w)), "pdt_write_dcs_packets")
    return int(w.value)


# pdt_subcom_entry and pdt_subcom_sample as numpy records, pdt_subcom_cfg and pdt_subcom_summary
SUBCOM_ENTRY_DTYPE = np.dtype([("channel", "u1"), ("byte", "u1"), ("period", "<u2"), ("phase", "<u2"), ("mask", "u1"), ("shift", "u1"), ("invert", "u1"),
                               ("pad", "u1")])
SUBCOM_SAMPLE_DTYPE = np.dtype([("time", "<f8"), ("frame", "<u4"), ("minor_id", "<u2"), ("channel", "u1"), ("entry", "u1"), ("value", "u1"), ("raw", "u1"),
                                ("flags", "u1"), ("pad", "u1", (5,))])
assert SUBCOM_ENTRY_DTYPE.itemsize == 10 and SUBCOM_SAMPLE_DTYPE.itemsize == 24
SUBCOM_BYTE_PARITY, SUBCOM_ID_PARITY, SUBCOM_UNCOVERED, SUBCOM_SPIKE = 1, 2, 4, 8
SUBCOM_SEM, SUBCOM_HK, SUBCOM_CUSTOM = 0, 1, -1


class SubcomCfg(C.Structure):
    _fields_ = [("trusted_only", C.c_uint32), ("spike_threshold", C.c_uint32)]


class SubcomSummary(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("used", "skipped", "bad_id", "samples", "dropped", "byte_parity", "id_parity", "spikes", "channels_hit")]


def tip_subcom_tile() -> int:
    """pdt_tip_subcom_tile: the records one tile of the subcommutation kernels covers (tests place samples at its seams)"""
    return int(lib().pdt_tip_subcom_tile())


def subcom_table(which: int) -> np.ndarray:
    """pdt_subcom_table: a built-in table (SUBCOM_SEM, SUBCOM_HK) as SUBCOM_ENTRY_DTYPE records; empty where there is no such table"""
    t = np.zeros(256, dtype=SUBCOM_ENTRY_DTYPE)
    return t[:int(lib().pdt_subcom_table(which, t.ctypes.data, 256))].copy()


def subcom_name(which: int, channel: int):
    """pdt_subcom_name: a built-in table's name of a channel, or None"""
    s = lib().pdt_subcom_name(which, channel)
    return s.decode() if s else None


def _subcom_table(table):
    return subcom_table(table) if isinstance(table, int) else np.ascontiguousarray(table, dtype=SUBCOM_ENTRY_DTYPE).reshape(-1)


def _subcom_call(fn, what, head, table, trusted_only, spike_threshold, cap):
    """what every subcommutation entry shares: (SUBCOM_SAMPLE_DTYPE[min(found, cap)], found, offsets uint64[nchan + 1], summary dict)"""
    t = _subcom_table(table)
    c = SubcomCfg(int(trusted_only), spike_threshold)
    out, count, sm, off = np.zeros(max(cap, 1), dtype=SUBCOM_SAMPLE_DTYPE), C.c_int(0), SubcomSummary(), np.zeros(129, dtype=np.uint64)
    _check(fn(*head, t.ctypes.data, len(t), C.byref(c), out.ctypes.data if cap else None, cap, C.byref(count), off.ctypes.data, C.byref(sm)), what)
    nchan = int(t["channel"].max()) + 1 if len(t) else 0
    return out[:min(count.value, cap)], count.value, off[:nchan + 1].copy(), {k: int(getattr(sm, k)) for k, _ in SubcomSummary._fields_}


def host_tip_subcom(frames, table=SUBCOM_SEM, trusted_only: bool = False, spike_threshold: int = 0, cap: int = 65536):
    """pdt_host_tip_subcom: the subcommutated bytes of FRAME_DTYPE records of TIP minor frames by `table` (SUBCOM_SEM, SUBCOM_HK or
    SUBCOM_ENTRY_DTYPE records), restated on the host (no GPU).  Returns (SUBCOM_SAMPLE_DTYPE[min(found, cap)], found, offsets, summary dict):
    the samples channel-major, offsets[c] .. offsets[c + 1] the samples of channel c."""
    a = np.ascontiguousarray(frames, dtype=FRAME_DTYPE).reshape(-1)
    return _subcom_call(lib().pdt_host_tip_subcom, "pdt_host_tip_subcom", (a.ctypes.data, len(a)), table, trusted_only, spike_threshold, cap)


def format_subcom(samples: np.ndarray, which: int = SUBCOM_CUSTOM) -> bytes:
    """pdt_format_subcom: one line per sample, the channels named as table `which` names them (host-only C, no GPU needed)"""
    a = np.ascontiguousarray(samples, dtype=SUBCOM_SAMPLE_DTYPE).reshape(-1)
    L = lib()
    n = L.pdt_format_subcom(a.ctypes.data, len(a), which, None, 0)
    buf = C.create_string_buffer(n + 1)
    L.pdt_format_subcom(a.ctypes.data, len(a), which, buf, n)
    return buf.raw[:n]


def write_subcom(samples: np.ndarray, fd: int, which: int = SUBCOM_CUSTOM) -> int:
    """pdt_write_subcom: the same text to an open file descriptor; returns the bytes written"""
    a = np.ascontiguousarray(samples, dtype=SUBCOM_SAMPLE_DTYPE).reshape(-1)
    w = C.c_uint64(0)
    _check(lib().pdt_write_subcom(a.ctypes.data, len(a), which, fd, C.byref(w)), "pdt_write_subcom")
    return int(w.value)


class FfCfg(C.Structure):
    """pdt_ff_cfg: a zero means the default; rate_steps 0 with FF_ZERO_RATE_STEPS in zero_mask asks for the nominal rate alone;
    FF_RESIDUAL_GIVEN in flags: residual_hz is the caller's, otherwise the carrier is measured"""
    _fields_ = [("rate_steps", C.c_int32), ("zero_mask", C.c_uint32), ("rate_step_ppm", C.c_double), ("residual_hz", C.c_double),
                ("flags", C.c_uint32), ("reserved_", C.c_uint32)]


class FfSync(C.Structure):
    """pdt_ff_sync"""
    _fields_ = [("residual_hz", C.c_double), ("tone_valid", C.c_int32), ("step", C.c_uint32), ("tau", C.c_int32), ("rate", C.c_int32),
                ("period", C.c_int64), ("metric", C.c_uint64), ("nbits", C.c_uint64)]


FF_ZERO_RATE_STEPS, FF_RESIDUAL_GIVEN = 1, 1
# pdt_ff_sync as a numpy record
FF_SYNC_DTYPE = np.dtype([("residual_hz", "<f8"), ("tone_valid", "<i4"), ("step", "<u4"), ("tau", "<i4"), ("rate", "<i4"), ("period", "<i8"),
                          ("metric", "<u8"), ("nbits", "<u8")])
assert FF_SYNC_DTYPE.itemsize == C.sizeof(FfSync) == 48 and C.sizeof(FfCfg) == 32
FfBits = collections.namedtuple("FfBits", "sync bits soft index")        # FF_SYNC_DTYPE record, '0'/'1' uint8[n], float32[n], int64[n]


def _ff_cfg(rate_steps=None, rate_step_ppm=None, residual_hz=None):
    """rate_steps (None = 20), rate_step_ppm (None = 625) and residual_hz (None = measure the carrier) -> pdt_ff_cfg or None"""
    if rate_steps is None and rate_step_ppm is None and residual_hz is None:
        return None
    c = FfCfg()
    if rate_steps is not None:
        c.rate_steps, c.zero_mask = int(rate_steps), FF_ZERO_RATE_STEPS if int(rate_steps) == 0 else 0
    if rate_step_ppm is not None:
        c.rate_step_ppm = float(rate_step_ppm)
    if residual_hz is not None:
        c.residual_hz, c.flags = float(residual_hz), FF_RESIDUAL_GIVEN
    return c


def ff_max_bits(rate: int, n: int) -> int:
    """room for the bits of any hypothesis of a stream of n samples at `rate` (the shortest allowed period is 0.9 H)"""
    return min(n, 2 * rate) * 800 // (rate * 18 // 10) + 2 if rate >= 800 else 2


def host_ff_mix(rate: int, residual_hz: float, iq: np.ndarray) -> np.ndarray:
    """pdt_host_ff_mix: the stream the feed-forward rule sums -- iq with the carrier at residual_hz taken out by the down-converter's
    mixer -- on the host (no GPU): float32[n, 2]"""
    a = np.ascontiguousarray(iq, dtype="<f4").reshape(-1)
    out = np.zeros(max(a.size, 2), dtype="<f4")
    _check(lib().pdt_host_ff_mix(rate, float(residual_hz), a.ctypes.data, a.size // 2, out.ctypes.data), "pdt_host_ff_mix")
    return out[:a.size // 2 * 2].reshape(-1, 2)


def host_ff_bits(rate: int, iq: np.ndarray, rate_steps=None, rate_step_ppm=None, residual_hz=None) -> FfBits:
    """pdt_host_ff_bits: the feed-forward bits of a float32 I,Q stream at `rate` restated on the host (no GPU), bit for bit what the
    kernels compute: FfBits(sync, bits, soft, index).  residual_hz None: the carrier is measured (pdt_host_tones' first segment)."""
    a = np.ascontiguousarray(iq, dtype="<f4").reshape(-1)
    c, n = _ff_cfg(rate_steps, rate_step_ppm, residual_hz), a.size // 2
    cap = ff_max_bits(rate, n)
    sync, count = np.zeros(1, dtype=FF_SYNC_DTYPE), C.c_uint64(0)
    bits, soft, index = np.zeros(cap, dtype=np.uint8), np.zeros(cap, dtype="<f4"), np.zeros(cap, dtype="<i8")
    _check(lib().pdt_host_ff_bits(rate, a.ctypes.data, n, C.byref(c) if c else None, sync.ctypes.data, bits.ctypes.data, soft.ctypes.data,
                                  index.ctypes.data, cap, C.byref(count)), "pdt_host_ff_bits")
    k = min(count.value, cap)
    return FfBits(sync[0], bits[:k], soft[:k], index[:k])


def ff_bits_batch(ds, rate_steps=None, rate_step_ppm=None, residual_hz=None) -> np.ndarray:
    """pdt_ff_bits_batch: Demodulator.ff_bits() of several contexts of one device and rate with ONE launch of each kernel (the windows of
    a round of demod_windows_held): FF_SYNC_DTYPE[len(ds)]; each context's bits through its ff_read()."""
    c = _ff_cfg(rate_steps, rate_step_ppm, residual_hz)
    hs = (C.c_void_p * max(len(ds), 1))(*[d._h for d in ds])
    syncs = np.zeros(max(len(ds), 1), dtype=FF_SYNC_DTYPE)
    _check(lib().pdt_ff_bits_batch(hs, len(ds), C.byref(c) if c else None, syncs.ctypes.data), "pdt_ff_bits_batch")
    return syncs[:len(ds)]


def ff_messages_batch(ds, min_run=None, cap: int = 64, rule=None, rate_steps=None, rate_step_ppm=None, residual_hz=None, with_sync: bool = False):
    """pdt_ff_messages_batch: feed-forward bits, then the ARGOS messages in them, for several contexts with ONE launch of each kernel: a
    list of ARGOS_MSG_DTYPE arrays, one per context (time = time_src / Fs, time_src = the sample index in the channel stream);
    with_sync: (that, FF_SYNC_DTYPE[len(ds)])."""
    c, a = _ff_cfg(rate_steps, rate_step_ppm, residual_hz), _argos_cfg(min_run, rule)
    hs = (C.c_void_p * max(len(ds), 1))(*[d._h for d in ds])
    syncs = np.zeros(max(len(ds), 1), dtype=FF_SYNC_DTYPE)
    out, counts = np.zeros((max(len(ds), 1), max(cap, 1)), dtype=ARGOS_MSG_DTYPE), (C.c_int * max(len(ds), 1))()
    _check(lib().pdt_ff_messages_batch(hs, len(ds), C.byref(c) if c else None, C.byref(a) if a else None, syncs.ctypes.data, out.ctypes.data, cap,
                                       counts), "pdt_ff_messages_batch")
    got = [out[i, :min(counts[i], cap)].copy() for i in range(len(ds))]
    return (got, syncs[:len(ds)]) if with_sync else got


class FfpCfg(C.Structure):
    """pdt_ffp_cfg: a zero means the default; ref_bits 0 with FFP_ZERO_REF_BITS and smooth_blocks 0 with FFP_ZERO_SMOOTH in zero_mask are
    real zeros; FFP_RESIDUAL_GIVEN in flags: residual_hz is the caller's, otherwise the carrier is measured segment by segment"""
    _fields_ = [("block_bits", C.c_int32), ("clock_steps", C.c_int32), ("ref_bits", C.c_int32), ("smooth_blocks", C.c_int32),
                ("zero_mask", C.c_uint32), ("flags", C.c_uint32), ("residual_hz", C.c_double)]


FFP_ZERO_REF_BITS, FFP_ZERO_SMOOTH, FFP_RESIDUAL_GIVEN = 1, 2, 1
# pdt_ffp_sync and pdt_ffp_block as numpy records
FFP_SYNC_DTYPE = np.dtype([("residual_hz", "<f8"), ("step", "<u4"), ("nfft", "<i4"), ("segs", "<u8"), ("segs_valid", "<u8"), ("nblocks", "<u8"),
                           ("nbits", "<u8"), ("block_len", "<i8"), ("block_bits", "<i4"), ("clock_steps", "<i4"), ("ref_bits", "<i4"),
                           ("smooth_blocks", "<i4")])
FFP_BLOCK_DTYPE = np.dtype([("phi", "<i8"), ("first_bit", "<i8"), ("count", "<u8"), ("metric", "<u8"), ("tau", "<i4"), ("reserved_", "<i4")])
assert FFP_SYNC_DTYPE.itemsize == 72 and FFP_BLOCK_DTYPE.itemsize == 40 and C.sizeof(FfpCfg) == 32
# FFP_SYNC_DTYPE record, '0'/'1' uint8[n], float32[n], int64[n], FFP_BLOCK_DTYPE[nblocks]
FfpBits = collections.namedtuple("FfpBits", "sync bits soft index blocks")


def _ffp_cfg(block_bits=None, clock_steps=None, ref_bits=None, smooth_blocks=None, residual_hz=None):
    """B (None = 208), T (32), W (16), J (4) and residual_hz (None = measure the carrier) -> pdt_ffp_cfg or None"""
    if block_bits is None and clock_steps is None and ref_bits is None and smooth_blocks is None and residual_hz is None:
        return None
    c = FfpCfg(block_bits=int(block_bits or 0), clock_steps=int(clock_steps or 0))
    if ref_bits is not None:
        c.ref_bits = int(ref_bits)
        c.zero_mask |= FFP_ZERO_REF_BITS if int(ref_bits) == 0 else 0
    if smooth_blocks is not None:
        c.smooth_blocks = int(smooth_blocks)
        c.zero_mask |= FFP_ZERO_SMOOTH if int(smooth_blocks) == 0 else 0
    if residual_hz is not None:
        c.residual_hz, c.flags = float(residual_hz), FFP_RESIDUAL_GIVEN
    return c


def ffp_max_bits(rate: int, n: int, block_bits=None) -> int:
    """room for the bits of a stream of n samples at `rate`: every block of B bits decides at most B + 3"""
    B = int(block_bits or 208)
    L = (2 * B * rate + 8320) // 16640
    return ((n + L - 1) // L) * (B + 3) + 1 if rate > 0 else 1


def host_ffp_mix(rate: int, iq: np.ndarray, **cfg) -> np.ndarray:
    """pdt_host_ffp_mix: the stream the feed-forward POES rule sums -- iq with the carrier taken out segment by segment, the phase
    continuous -- on the host (no GPU): float32[n, 2]"""
    a = np.ascontiguousarray(iq, dtype="<f4").reshape(-1)
    c = _ffp_cfg(**cfg)
    out = np.zeros(max(a.size, 2), dtype="<f4")
    _check(lib().pdt_host_ffp_mix(rate, a.ctypes.data, a.size // 2, C.byref(c) if c else None, out.ctypes.data), "pdt_host_ffp_mix")
    return out[:a.size // 2 * 2].reshape(-1, 2)


def host_ffp_bits(rate: int, iq: np.ndarray, **cfg) -> FfpBits:
    """pdt_host_ffp_bits: the feed-forward bits of a float32 I,Q POES stream at `rate` restated on the host (no GPU), bit for bit what
    the kernels compute: FfpBits(sync, bits, soft, index, blocks).  cfg: block_bits, clock_steps, ref_bits, smooth_blocks, residual_hz
    (None = the carrier is measured)."""
    a = np.ascontiguousarray(iq, dtype="<f4").reshape(-1)
    c, n = _ffp_cfg(**cfg), a.size // 2
    cap = ffp_max_bits(rate, n, cfg.get("block_bits"))
    sync, count = np.zeros(1, dtype=FFP_SYNC_DTYPE), C.c_uint64(0)
    bits, soft, index = np.zeros(cap, dtype=np.uint8), np.zeros(cap, dtype="<f4"), np.zeros(cap, dtype="<i8")
    blocks = np.zeros(cap, dtype=FFP_BLOCK_DTYPE)
    _check(lib().pdt_host_ffp_bits(rate, a.ctypes.data, n, C.byref(c) if c else None, sync.ctypes.data, bits.ctypes.data, soft.ctypes.data,
                                   index.ctypes.data, cap, C.byref(count), blocks.ctypes.data, cap), "pdt_host_ffp_bits")
    k = min(count.value, cap)
    return FfpBits(sync[0], bits[:k], soft[:k], index[:k], blocks[:int(sync[0]["nblocks"])])


def format_argos_messages(msgs: np.ndarray) -> bytes:
    """pdt_format_argos_messages: one line per complete message (host-only C, no GPU needed)"""
    a = np.ascontiguousarray(msgs, dtype=ARGOS_MSG_DTYPE)
    L = lib()
    n = L.pdt_format_argos_messages(a.ctypes.data, len(a), None, 0)
    buf = C.create_string_buffer(n + 1)
    L.pdt_format_argos_messages(a.ctypes.data, len(a), buf, n)
    return buf.raw[:n]


def _carriers(rec, count: int):
    return [Carrier(rec[i].offset_hz, rec[i].peak_db, rec[i].floor_power) for i in range(count)]


# every symbol include/pdt.h declares (tests check the library exports all of them)
ABI_SYMBOLS = [
    "pdt_abi_version", "pdt_build_tag", "pdt_strerror", "pdt_device_count", "pdt_open", "pdt_close", "pdt_set_stream",
    "pdt_demod_pcm16", "pdt_demod_device", "pdt_demod_f32", "pdt_demod_device_f32", "pdt_demod_batch_device", "pdt_num_frames", "pdt_frames", "pdt_get_stats",
    "pdt_format_frames", "pdt_read_stage", "pdt_stage_len", "pdt_kernel_times", "pdt_make_lpf",
    "pdt_wav_parse_header", "pdt_time_axis", "pdt_stage_bytesync", "pdt_tip_check", "pdt_tip_frames",
    "pdt_stream_begin", "pdt_stream_push_pcm16", "pdt_stream_push_f32", "pdt_stream_end", "pdt_stream_frames",
    "pdt_keep_quality", "pdt_chunk_reports", "pdt_stage_manchester", "pdt_stage_fir", "pdt_stage_agc", "pdt_stage_squelch", "pdt_stage_pll", "pdt_stage_gardner", "pdt_stage_static_gain", "pdt_stage_mm",
    "pdt_keep_presquelch", "pdt_keep_pll", "pdt_stage_bytesync_from", "pdt_demod_fd", "pdt_format_records", "pdt_stream_retained", "pdt_host_math", "pdt_get_device",
    "pdt_write_frames", "pdt_write_records", "pdt_demod_file", "pdt_set_loop_params", "pdt_set_progress",
    "pdt_set_real_input", "pdt_demod_real", "pdt_demod_device_real", "pdt_stream_push_real", "pdt_host_analytic",
    "pdt_set_channel", "pdt_demod_channel", "pdt_demod_device_channel", "pdt_demod_channels_device", "pdt_demod_channels", "pdt_stream_push_channel", "pdt_host_ddc",
    "pdt_survey", "pdt_survey_device", "pdt_survey_spectrum", "pdt_host_survey",
    "pdt_bursts", "pdt_bursts_device", "pdt_burst_carriers", "pdt_waterfall_rows", "pdt_bursts_shape", "pdt_burst_peaks", "pdt_host_bursts",
    "pdt_device_math", "pdt_device_math_layout",
    "pdt_burst_windows", "pdt_demod_windows_device", "pdt_demod_windows", "pdt_demod_windows_held",
    "pdt_tones", "pdt_tones_batch", "pdt_host_tones",
    "pdt_argos_messages", "pdt_argos_messages_batch", "pdt_stage_argos_messages", "pdt_host_argos_messages", "pdt_argos_msg_tile",
    "pdt_format_argos_messages", "pdt_write_argos_messages",
    "pdt_ff_bits", "pdt_ff_bits_batch", "pdt_ff_read", "pdt_ff_messages", "pdt_ff_messages_batch", "pdt_stage_ff_bits", "pdt_host_ff_bits",
    "pdt_host_ff_mix",
    "pdt_ffp_bits", "pdt_ffp_read", "pdt_ffp_blocks", "pdt_ffp_frames", "pdt_stage_ffp_bits", "pdt_stage_ffp_frames", "pdt_host_ffp_bits",
    "pdt_host_ffp_mix",
    "pdt_tip_sync", "pdt_tip_sync_batch", "pdt_stage_tip_sync", "pdt_host_tip_sync", "pdt_tip_sync_tile", "pdt_tip_check_records",
    "pdt_tip_repair", "pdt_stage_tip_repair", "pdt_host_tip_repair",
    "pdt_tip_dcs", "pdt_tip_dcs_records", "pdt_host_tip_dcs", "pdt_format_dcs_packets", "pdt_write_dcs_packets", "pdt_tip_dcs_tile",
    "pdt_tip_subcom", "pdt_tip_subcom_records", "pdt_host_tip_subcom", "pdt_subcom_table", "pdt_subcom_name", "pdt_tip_subcom_tile", "pdt_format_subcom",
    "pdt_write_subcom",
]
DEV_SYMBOLS = ["pdt_dev_set", "pdt_dev_span_rows", "pdt_dev_span_rekey", "pdt_dev_fir_form", "pdt_dev_ddc"]       # include/pdt_dev.h (test-only)

_lib = None


def _share_torch_hip_runtime():
    """A PyTorch-ROCm wheel carries its own copy of the HIP runtime (torch/lib/libamdhip64.so, same SONAME as /opt/rocm's).
    Loaded after libpdt.so has brought in the system copy, it is a second runtime in the process and finds no GPU ("No HIP
    GPUs are available"); loaded first, libpdt.so's dependency resolves to it and both use one runtime -- the order `import
    torch` before this package always gave.  Make the order irrelevant: when a torch with a bundled runtime is installed
    (found without importing it), load that copy before libpdt.so.  Without torch nothing happens and libpdt.so uses the
    system runtime, as the C programs do."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.submodule_search_locations:
        return
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(path):
        try:
            C.CDLL(path, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    """Load libpdt.so (built in-tree by ``make`` / ``__graft_entry__.build()``); fail loudly if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIBPDT_PATH):
        raise PdtError(
            f"{LIBPDT_PATH} is missing: build it with `make` (hipcc --offload-arch=gfx950). "
            "There is no CPU implementation to fall back to."
        )
    _share_torch_hip_runtime()
    L = C.CDLL(LIBPDT_PATH)
    L.pdt_abi_version.restype = C.c_int
    L.pdt_build_tag.restype = C.c_char_p
    L.pdt_strerror.restype = C.c_char_p
    L.pdt_strerror.argtypes = [C.c_int]
    L.pdt_device_count.restype = C.c_int
    L.pdt_open.argtypes = [C.POINTER(Config), C.POINTER(C.c_void_p)]
    L.pdt_close.argtypes = [C.c_void_p]
    L.pdt_close.restype = None
    L.pdt_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.pdt_demod_pcm16.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.pdt_demod_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.pdt_demod_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.pdt_demod_device_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.pdt_demod_fd.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_int]
    L.pdt_format_records.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint64]
    L.pdt_format_records.restype = C.c_uint64
    L.pdt_num_frames.argtypes = [C.c_void_p]
    L.pdt_num_frames.restype = C.c_uint64
    L.pdt_frames.argtypes = [C.c_void_p, C.POINTER(Frame), C.c_uint64]
    L.pdt_frames.restype = C.c_uint64
    L.pdt_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
    L.pdt_format_frames.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64]
    L.pdt_format_frames.restype = C.c_uint64
    L.pdt_read_stage.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]
    L.pdt_read_stage.restype = C.c_int64
    L.pdt_stage_len.argtypes = [C.c_void_p, C.c_int]
    L.pdt_stage_len.restype = C.c_uint64
    L.pdt_kernel_times.argtypes = [C.c_void_p, C.POINTER(KernelTime), C.c_int]
    L.pdt_make_lpf.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.pdt_wav_parse_header.argtypes = [C.c_char_p] + [C.POINTER(C.c_uint32)] * 5
    L.pdt_time_axis.argtypes = [C.c_int, C.c_uint32, C.c_uint64]
    L.pdt_time_axis.restype = C.c_double
    L.pdt_stage_bytesync.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.pdt_demod_batch_device.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_int]
    L.pdt_stream_begin.argtypes = [C.c_void_p]
    L.pdt_stream_push_pcm16.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.pdt_stream_push_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.pdt_stream_end.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.pdt_stream_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.pdt_stream_frames.restype = C.c_uint64
    L.pdt_host_math.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.pdt_stream_retained.argtypes = [C.c_void_p]
    L.pdt_stream_retained.restype = C.c_uint64
    L.pdt_stage_manchester.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pdt_stage_manchester.restype = C.c_int
    L.pdt_stage_pll.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pdt_stage_pll.restype = C.c_int
    L.pdt_stage_gardner.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]
    L.pdt_stage_gardner.restype = C.c_int
    L.pdt_stage_static_gain.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_double, C.c_void_p]
    L.pdt_stage_static_gain.restype = C.c_int
    L.pdt_stage_mm.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pdt_stage_mm.restype = C.c_int
    L.pdt_stage_agc.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_void_p]
    L.pdt_stage_agc.restype = C.c_int
    L.pdt_stage_squelch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_double]
    L.pdt_stage_squelch.restype = C.c_int
    L.pdt_stage_fir.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.pdt_stage_fir.restype = C.c_int
    L.pdt_keep_quality.argtypes = [C.c_void_p, C.c_int]
    L.pdt_keep_quality.restype = C.c_int
    L.pdt_keep_pll.argtypes = [C.c_void_p, C.c_int]
    L.pdt_keep_pll.restype = C.c_int
    L.pdt_chunk_reports.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.pdt_chunk_reports.restype = C.c_uint64
    L.pdt_set_progress.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.pdt_tip_check.argtypes = [C.c_void_p, C.POINTER(TipSummary)]
    L.pdt_tip_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.pdt_tip_frames.restype = C.c_uint64
    L.pdt_write_frames.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
    L.pdt_write_records.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
    L.pdt_dev_set.argtypes = [C.c_char_p, C.c_char_p]
    L.pdt_dev_fir_form.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
    L.pdt_dev_fir_form.restype = C.c_uint
    L.pdt_set_loop_params.argtypes = [C.c_void_p, C.POINTER(LoopParams)]
    L.pdt_demod_file.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
    L.pdt_set_real_input.argtypes = [C.c_void_p, C.c_double]
    L.pdt_demod_real.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
    L.pdt_demod_device_real.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
    L.pdt_stream_push_real.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
    L.pdt_host_analytic.argtypes = [C.c_uint32, C.c_double, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
    L.pdt_set_channel.argtypes = [C.c_void_p, C.c_int, C.c_double]
    L.pdt_demod_channel.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
    L.pdt_demod_device_channel.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
    L.pdt_demod_channels_device.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_uint64, C.c_int]
    L.pdt_demod_channels.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_uint64, C.c_int]
    L.pdt_stream_push_channel.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
    L.pdt_host_ddc.argtypes = [C.c_uint32, C.c_int, C.c_double, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
    L.pdt_dev_ddc.argtypes = [C.c_int, C.c_uint32, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_longlong, C.c_longlong, C.c_uint64, C.c_uint64, C.c_void_p]
    L.pdt_survey.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(SurveyCfg), C.POINTER(CarrierRec), C.c_int, C.POINTER(C.c_int)]
    L.pdt_survey_device.argtypes = L.pdt_survey.argtypes
    L.pdt_survey_spectrum.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.pdt_bursts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.POINTER(BurstsCfg), C.POINTER(BurstRec), C.c_int, C.POINTER(C.c_int)]
    L.pdt_bursts_device.argtypes = L.pdt_bursts.argtypes
    L.pdt_burst_carriers.argtypes = [C.POINTER(BurstRec), C.c_int, C.c_double, C.POINTER(CarrierRec), C.c_int, C.POINTER(C.c_int)]
    L.pdt_waterfall_rows.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    L.pdt_bursts_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
    L.pdt_burst_peaks.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    L.pdt_host_bursts.argtypes = [C.c_uint32, C.c_double, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(BurstsCfg), C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.POINTER(BurstRec), C.c_int, C.POINTER(C.c_int)]
    L.pdt_host_survey.argtypes = [C.c_uint32, C.c_double, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(SurveyCfg), C.c_void_p,
                                  C.POINTER(CarrierRec), C.c_int, C.POINTER(C.c_int)]
    L.pdt_burst_windows.argtypes = [C.POINTER(BurstRec), C.c_int, C.c_uint32, C.c_uint64, C.c_double, C.c_double, C.POINTER(WindowRec)]
    L.pdt_demod_windows_device.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(WindowRec), C.c_void_p, C.c_uint64, C.c_int]
    L.pdt_demod_windows.argtypes = L.pdt_demod_windows_device.argtypes
    L.pdt_demod_windows_held.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.POINTER(WindowRec)]
    L.pdt_tones.argtypes = [C.c_void_p, C.POINTER(ToneCfg), C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.pdt_tones_batch.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(ToneCfg), C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.pdt_host_tones.argtypes = [C.c_uint32, C.c_double, C.c_void_p, C.c_uint64, C.POINTER(ToneCfg), C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.pdt_argos_messages.argtypes = [C.c_void_p, C.POINTER(ArgosCfg), C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.pdt_argos_messages_batch.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(ArgosCfg), C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.pdt_stage_argos_messages.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(ArgosCfg), C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.pdt_host_argos_messages.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(ArgosCfg), C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.pdt_tip_sync.argtypes = [C.c_void_p, C.POINTER(TipSyncCfg), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.pdt_tip_sync_batch.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(TipSyncCfg), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.pdt_stage_tip_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(TipSyncCfg), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.pdt_host_tip_sync.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(TipSyncCfg), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.pdt_tip_check_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(TipSummary), C.c_void_p]
    L.pdt_tip_repair.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(TipRepairSummary)]
    L.pdt_stage_tip_repair.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(TipRepairSummary)]
    L.pdt_host_tip_repair.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(TipRepairSummary)]
    L.pdt_tip_dcs.argtypes = [C.c_void_p, C.POINTER(DcsCfg), C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(DcsSummary)]
    L.pdt_tip_dcs_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(DcsCfg), C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(DcsSummary)]
    L.pdt_host_tip_dcs.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(DcsCfg), C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(DcsSummary)]
    L.pdt_format_dcs_packets.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint64]
    L.pdt_format_dcs_packets.restype = C.c_uint64
    L.pdt_write_dcs_packets.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
    subcom_tail = [C.c_void_p, C.c_uint64, C.POINTER(SubcomCfg), C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.POINTER(SubcomSummary)]
    L.pdt_tip_subcom.argtypes = [C.c_void_p] + subcom_tail
    L.pdt_tip_subcom_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64] + subcom_tail
    L.pdt_host_tip_subcom.argtypes = [C.c_void_p, C.c_uint64] + subcom_tail
    L.pdt_subcom_table.argtypes = [C.c_int, C.c_void_p, C.c_int]
    L.pdt_subcom_name.argtypes = [C.c_int, C.c_int]
    L.pdt_subcom_name.restype = C.c_char_p
    L.pdt_format_subcom.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_char_p, C.c_uint64]
    L.pdt_format_subcom.restype = C.c_uint64
    L.pdt_write_subcom.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
    L.pdt_format_argos_messages.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint64]
    L.pdt_format_argos_messages.restype = C.c_uint64
    L.pdt_write_argos_messages.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
    L.pdt_ff_bits.argtypes = [C.c_void_p, C.POINTER(FfCfg), C.c_void_p]
    L.pdt_ff_bits_batch.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(FfCfg), C.c_void_p]
    L.pdt_ff_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.pdt_ff_messages.argtypes = [C.c_void_p, C.POINTER(FfCfg), C.POINTER(ArgosCfg), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.pdt_ff_messages_batch.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(FfCfg), C.POINTER(ArgosCfg), C.c_void_p, C.c_void_p, C.c_int,
                                        C.POINTER(C.c_int)]
    L.pdt_stage_ff_bits.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(FfCfg), C.c_void_p]
    L.pdt_host_ff_bits.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(FfCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                   C.POINTER(C.c_uint64)]
    L.pdt_host_ff_mix.argtypes = [C.c_uint32, C.c_double, C.c_void_p, C.c_uint64, C.c_void_p]
    L.pdt_ffp_bits.argtypes = [C.c_void_p, C.POINTER(FfpCfg), C.c_void_p]
    L.pdt_ffp_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.pdt_ffp_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.pdt_ffp_frames.argtypes = [C.c_void_p, C.POINTER(FfpCfg), C.POINTER(TipSyncCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.pdt_stage_ffp_bits.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(FfpCfg), C.c_void_p]
    L.pdt_stage_ffp_frames.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(FfpCfg), C.POINTER(TipSyncCfg), C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.pdt_host_ffp_bits.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(FfpCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                    C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64]
    L.pdt_host_ffp_mix.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(FfpCfg), C.c_void_p]
    L.pdt_device_math.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
    L.pdt_device_math_layout.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    if L.pdt_abi_version() != 4:
        raise PdtError("libpdt.so ABI version mismatch")
    _lib = L
    return L


def _check(rc: int, what: str):
    if rc != 0:
        raise PdtError(f"{what}: {lib().pdt_strerror(rc).decode()} ({rc})")


def build_tag() -> str:
    """pdt_build_tag: which sources the loaded libpdt.so was built from (profiles/ files carry the same tag)"""
    return lib().pdt_build_tag().decode()


def make_lpf(mode: int, sample_rate: int) -> tuple[np.ndarray, int]:
    """MakeLPFIR as the reference's mains call it (LowPassFilter.c:127-175). Returns (taps, interp)."""
    L = lib()
    nt, ip = C.c_int(), C.c_int()
    _check(L.pdt_make_lpf(mode, sample_rate, None, C.byref(nt), C.byref(ip)), "pdt_make_lpf")
    taps = np.zeros(nt.value, dtype=np.float64 if mode == MODE_ARGOS else np.float32)
    _check(L.pdt_make_lpf(mode, sample_rate, taps.ctypes.data, None, None), "pdt_make_lpf")
    return taps, ip.value


def host_math(fn: int, x: np.ndarray):
    """pdt_host_math: the library's own sincos / sin / cos / sincosf / hypot / hypotf, the PLL's wraps, arctan2_ref and q_rsqrt
    evaluated on the host (test hook; include/pdt.h lists the codes).  The two-argument codes take the pairs interleaved."""
    a = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    n = len(a) // 2 if fn in (4, 5, 11, 12) else len(a)
    o0, o1 = np.zeros(n), np.zeros(n)
    _check(lib().pdt_host_math(fn, a.ctypes.data, n, o0.ctypes.data, o1.ctypes.data), "pdt_host_math")
    return o0, o1


def device_math_layout(fn: int) -> tuple[np.dtype, int, int]:
    """pdt_device_math_layout: (element type, elements per record in, elements per record out) of a pdt_device_math code."""
    eb, ni, no = C.c_int(), C.c_int(), C.c_int()
    _check(lib().pdt_device_math_layout(fn, C.byref(eb), C.byref(ni), C.byref(no)), "pdt_device_math_layout")
    return np.dtype(np.float32 if eb.value == 4 else np.float64), ni.value, no.value


def _real_samples(x: np.ndarray) -> tuple[np.ndarray, int]:
    """A single-channel capture as the library takes it: float arrays as little-endian float32 (FMT_REAL_F32), anything else
    as little-endian int16 (FMT_REAL_PCM16)."""
    if np.asarray(x).dtype.kind == "f":
        return np.ascontiguousarray(x, dtype="<f4").reshape(-1), FMT_REAL_F32
    return np.ascontiguousarray(x, dtype="<i2").reshape(-1), FMT_REAL_PCM16


def host_analytic(sample_rate: int, center_hz: float, x: np.ndarray) -> np.ndarray:
    """pdt_host_analytic: the Hilbert front end of real captures restated on the host (no GPU), bit for bit what the kernel
    computes.  Returns float32[n, 2] I,Q pairs."""
    a, fmt = _real_samples(x)
    out = np.zeros((a.size, 2), dtype=np.float32)
    _check(lib().pdt_host_analytic(sample_rate, float(center_hz), a.ctypes.data, a.size, fmt, out.ctypes.data), "pdt_host_analytic")
    return out


def _wb_samples(x: np.ndarray) -> tuple[np.ndarray, int]:
    """A wideband I,Q capture as the library takes it, by dtype: uint8 pairs (FMT_WB_CU8), int8 pairs (FMT_WB_CS8), float pairs as
    little-endian float32 (FMT_WB_F32), anything else as little-endian int16 pairs (FMT_WB_PCM16).  Returns the flat array."""
    dt = np.asarray(x).dtype
    if dt == np.uint8:
        return np.ascontiguousarray(x).reshape(-1), FMT_WB_CU8
    if dt == np.int8:
        return np.ascontiguousarray(x).reshape(-1), FMT_WB_CS8
    if dt.kind == "f":
        return np.ascontiguousarray(x, dtype="<f4").reshape(-1), FMT_WB_F32
    return np.ascontiguousarray(x, dtype="<i2").reshape(-1), FMT_WB_PCM16


def host_ddc(in_rate: int, decim: int, offset_hz: float, x: np.ndarray) -> np.ndarray:
    """pdt_host_ddc: the down-converter of wideband captures restated on the host (no GPU), bit for bit what the kernel computes.
    x: I,Q pairs at in_rate (uint8, int8, int16 or float32).  Returns float32[ceil(n / decim), 2] at in_rate / decim."""
    a, fmt = _wb_samples(x)
    n = a.size // 2
    out = np.zeros(((n + decim - 1) // decim if decim > 0 else 0, 2), dtype=np.float32)
    _check(lib().pdt_host_ddc(in_rate, decim, float(offset_hz), a.ctypes.data, n, fmt, out.ctypes.data), "pdt_host_ddc")
    return out


def dev_ddc(in_rate: int, decim: int, offset_hz: float, fmt: int, x_ptr: int, lo: int, hi: int, n_out: int, g0: int, out_ptr: int, device: int = 0):
    """pdt_dev_ddc (test-only, include/pdt_dev.h): the down-converter's kernel on one record as a stream piece hands it over -- input
    sample 0 at the device address x_ptr, samples lo <= i < hi present, g0 the global index of input 0, n_out float32 pairs to the
    device address out_ptr.  Returns when they are there."""
    _check(lib().pdt_dev_ddc(device, in_rate, decim, float(offset_hz), fmt, C.c_void_p(int(x_ptr)), lo, hi, n_out, g0, C.c_void_p(int(out_ptr))),
           "pdt_dev_ddc")


def host_survey(in_rate: int, mode_range_hz: float, channel_rate: int, x: np.ndarray, **cfg):
    """pdt_host_survey: the carrier survey of a wideband capture restated on the host (no GPU), bit for bit what the kernels and the
    host search compute.  x: I,Q pairs at in_rate; mode_range_hz and channel_rate: what a context would supply as the defaults of
    merge_hz and guard_hz; cfg: fields of pdt_survey_cfg.  Returns (the averaged spectrum float32[nfft], [Carrier, ...])."""
    a, fmt = _wb_samples(x)
    c, cap = _survey_cfg(cfg)
    spec = np.zeros(int(cfg.get("nfft", 0)) or 16384, dtype=np.float32)
    rec, count = (CarrierRec * cap)(), C.c_int(0)
    _check(lib().pdt_host_survey(in_rate, float(mode_range_hz), channel_rate, fmt, a.ctypes.data, a.size // 2, C.byref(c) if c else None,
                                 spec.ctypes.data if spec.size in (1024, 4096, 16384) else None, rec, cap, C.byref(count)), "pdt_host_survey")
    return spec, _carriers(rec, count.value)


def host_bursts(in_rate: int, mode_range_hz: float, channel_rate: int, x: np.ndarray, rows: bool = True, **cfg):
    """pdt_host_bursts: the burst search of a wideband capture restated on the host (no GPU), bit for bit what the kernels and the
    host linking compute.  Arguments as host_survey; cfg: fields of pdt_bursts_cfg, and cap (room for that many bursts).  Returns
    (rows float32[nrows, nfft] or None when rows is False, peaks ROW_PEAK_DTYPE[nrows, 8], counts int32[nrows], [Burst, ...])."""
    a, fmt = _wb_samples(x)
    c, cap = _bursts_cfg(cfg)
    nfft, per = int(cfg.get("nfft", 0)) or 4096, int(cfg.get("rows_per", 0)) or 8
    stretch = int(cfg.get("nframes", 0)) or max(a.size // 2 - int(cfg.get("first_frame", 0)), 0)
    nrows = stretch // (nfft * per) if nfft in (1024, 4096, 16384) and 1 <= per <= 64 else 0
    w = np.zeros((nrows, nfft), dtype=np.float32) if rows else None
    peaks, counts = np.zeros((nrows, BURST_ROW_PEAKS), dtype=ROW_PEAK_DTYPE), np.zeros(nrows, dtype=np.int32)
    rec, count = (BurstRec * max(cap, 1))(), C.c_int(0)
    _check(lib().pdt_host_bursts(in_rate, float(mode_range_hz), channel_rate, fmt, a.ctypes.data, a.size // 2, C.byref(c) if c else None,
                                 w.ctypes.data if rows and nrows else None, peaks.ctypes.data if nrows else None, counts.ctypes.data if nrows else None,
                                 rec, cap, C.byref(count)), "pdt_host_bursts")
    return w, peaks, counts, _bursts(rec, count.value, cap)


def time_axis(mode: int, sample_rate: int, m: int) -> float:
    return lib().pdt_time_axis(mode, sample_rate, m)


def read_wav(path: str) -> tuple[int, np.ndarray]:
    """44-byte canonical header only, like ReadWavHeader (wave.c:303-378); every byte after it is
    sample data (the reference reads to EOF, POESTIPdemod/main.c:373).  Returns (rate, int16[n,2])."""
    with open(path, "rb") as f:
        hdr = f.read(44)
        data = f.read()
    if len(hdr) < 44:
        raise PdtError("short WAV header")
    fmt, ch, rate = struct.unpack_from("<HHI", hdr, 20)
    bits = struct.unpack_from("<H", hdr, 34)[0]
    if fmt != 1 or ch != 2 or bits != 16:
        raise PdtError("need 16-bit PCM with 2 channels (I,Q)")
    n = len(data) // 4
    return rate, np.frombuffer(data, dtype="<i2", count=2 * n).reshape(n, 2)


def sync_dev_switches(L=None):
    """Mirror the process's PDT_* environment variables into the library's developer-switch registry (``pdt_dev_set``,
    include/pdt_dev.h: a TEST-ONLY entry -- the library itself never reads the environment, and the C host programs never
    call this).  Called before every ``pdt_open`` of this binding, so tests and sweeps keep saying
    ``os.environ["PDT_GSPAN"] = "4"`` around the opening of a context."""
    L = L or lib()
    L.pdt_dev_set(None, None)
    for k, v in os.environ.items():
        if k.startswith("PDT_"):
            L.pdt_dev_set(k.encode(), v.encode())


class Demodulator:
    """One capture -> minor frames / packets on one GPU (context of include/pdt.h)."""

    def __init__(self, mode: int, sample_rate: int, chunk: int = 0, norm_override: float = 0.0, device: int = 0,
                 profile: bool = False, pll_block: int = 0, pll_warm: int = 0, agc_block: int = 0, agc_warm: int = 0,
                 gardner_band_pad: float = 0.0, sampler: int = 0, mm_step_range: float = 0.0, mm_kp: float = 0.0, chain: int = 0):
        self._L = lib()
        self.mode = mode
        self.sample_rate = sample_rate
        cfg = Config(mode, sample_rate, chunk, norm_override, device, int(profile), pll_block, pll_warm, agc_block,
                     agc_warm, gardner_band_pad, sampler, chain, mm_step_range, mm_kp)
        self._h = C.c_void_p()
        sync_dev_switches(self._L)
        _check(self._L.pdt_open(C.byref(cfg), C.byref(self._h)), "pdt_open")
        self.chain = chain
        self.dtype = np.float64 if (mode == MODE_ARGOS and not chain) else np.float32      # (the ARGOS twin is the float build)

    def close(self):
        if self._h:
            self._L.pdt_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_loop_params(self, **kw):
        """``pdt_set_loop_params``: loop constants other than the mains' (fields of ``LoopParams``; 0 / absent = default)."""
        lp = LoopParams(**kw)
        # a constant given as 0 where 0 is a meaningful value (lock threshold, timing gain / clip, resync threshold) IS zero
        zero_bits = {"pll_lock_threshold": 1, "gardner_kp": 2, "gardner_step_range": 4, "manchester_threshold": 8}
        if "zero_mask" not in kw:
            lp.zero_mask = sum(b for k, b in zero_bits.items() if k in kw and kw[k] == 0)
        _check(self._L.pdt_set_loop_params(self._h, C.byref(lp)), "pdt_set_loop_params")
        return self

    def keep_presquelch(self, enable: bool = True):
        """Also keep the AGC output before Squelch (stage ST_AGC_RAW): what the reference's -r option dumps."""
        _check(self._L.pdt_keep_presquelch(self._h, int(enable)), "pdt_keep_presquelch")
        return self

    def keep_pll(self, enable: bool = True):
        """Whether the PLL output stream (ST_PLL) is written out where mix and filter run as one kernel (on by default)."""
        _check(self._L.pdt_keep_pll(self._h, int(enable)), "pdt_keep_pll")
        return self

    def keep_quality(self, enable: bool = True):
        """Also keep the per-chunk reports (CarrierTrackPLL's return value = averagePhase, symbol / bit / frame counts):
        what the reference's progress line shows (POESTIPdemod/main.c:457-481)."""
        _check(self._L.pdt_keep_quality(self._h, int(enable)), "pdt_keep_quality")
        return self

    def set_progress(self, fn=None):
        """``pdt_set_progress``: ``fn(first_chunk, reports, stats_so_far)`` is called with the reports (CHUNK_DTYPE array) of the
        chunks that have become final -- once per completed segment of an overlapped ``demod_file`` / ``demod_file_text``
        (from a thread of the library), once at the end of any other whole-capture call.  Needs ``keep_quality``."""
        if fn is None:
            self._progress_cb = None
            _check(self._L.pdt_set_progress(self._h, None, None), "pdt_set_progress")
            return self

        def tramp(_user, first, reports, n, st):
            arr = np.frombuffer(C.string_at(reports, int(n) * CHUNK_DTYPE.itemsize), dtype=CHUNK_DTYPE).copy()
            fn(int(first), arr, Stats.from_buffer_copy(C.string_at(st, C.sizeof(Stats))))

        self._progress_cb = PROGRESS_FN(tramp)                       # (kept alive as long as the context uses it)
        _check(self._L.pdt_set_progress(self._h, C.cast(self._progress_cb, C.c_void_p), None), "pdt_set_progress")
        return self

    def chunk_reports(self) -> np.ndarray:
        n = int(self._L.pdt_chunk_reports(self._h, None, 0))
        out = np.zeros(n, dtype=CHUNK_DTYPE)
        if n:
            got = int(self._L.pdt_chunk_reports(self._h, out.ctypes.data, n))
            out = out[:got]
        return out

    def set_stream(self, stream_handle: int):
        _check(self._L.pdt_set_stream(self._h, C.c_void_p(stream_handle)), "pdt_set_stream")

    def demod(self, iq: np.ndarray):
        """iq: int16 array of shape (n, 2) or flat interleaved I,Q in host memory."""
        a = np.ascontiguousarray(iq, dtype="<i2").reshape(-1)
        _check(self._L.pdt_demod_pcm16(self._h, a.ctypes.data, a.size // 2), "pdt_demod_pcm16")
        return self

    def demod_raw(self, iq: np.ndarray):
        """RAW capture: float32 array of shape (n, 2) or flat interleaved I,Q, used without normalisation."""
        a = np.ascontiguousarray(iq, dtype="<f4").reshape(-1)
        _check(self._L.pdt_demod_f32(self._h, a.ctypes.data, a.size // 2), "pdt_demod_f32")
        return self

    def demod_file(self, fd: int, byte_offset: int, nframes: int, fmt: int = 0):
        """The capture straight from an open file (descriptor `fd`): nframes I,Q pairs from byte_offset (44 after the
        canonical WAV header, 0 for RAW); fmt 0 = int16 pairs, 1 = float32 pairs."""
        _check(self._L.pdt_demod_fd(self._h, fd, byte_offset, nframes, fmt), "pdt_demod_fd")
        return self

    def set_real_input(self, center_hz: float = 0.0):
        """Centre frequency single-channel captures are mixed down from (0 = Fs / 4, the default)."""
        _check(self._L.pdt_set_real_input(self._h, float(center_hz)), "pdt_set_real_input")
        return self

    def demod_real(self, x: np.ndarray):
        """Single-channel capture in host memory: int16 samples (s / 32768) or float32 samples (as they are)."""
        a, fmt = _real_samples(x)
        _check(self._L.pdt_demod_real(self._h, a.ctypes.data, a.size, fmt), "pdt_demod_real")
        return self

    def demod_device_real(self, dev_ptr: int, n: int, fmt: int = FMT_REAL_PCM16):
        """Single-channel capture resident in HBM (n samples of FMT_REAL_PCM16 / FMT_REAL_F32)."""
        _check(self._L.pdt_demod_device_real(self._h, C.c_void_p(dev_ptr), n, fmt), "pdt_demod_device_real")
        return self

    def set_channel(self, decim: int, offset_hz: float):
        """The channel of this context's wideband captures: input at decim x the context's rate, the carrier offset_hz from centre."""
        _check(self._L.pdt_set_channel(self._h, int(decim), float(offset_hz)), "pdt_set_channel")
        return self

    def demod_channel(self, x: np.ndarray):
        """Wideband I,Q capture in host memory: uint8, int8, int16 or float32 pairs at decim x the context's rate."""
        a, fmt = _wb_samples(x)
        _check(self._L.pdt_demod_channel(self._h, a.ctypes.data, a.size // 2, fmt), "pdt_demod_channel")
        return self

    def demod_device_channel(self, dev_ptr: int, nframes: int, fmt: int = FMT_WB_PCM16):
        """Wideband capture resident in HBM (nframes I,Q frames of FMT_WB_*)."""
        _check(self._L.pdt_demod_device_channel(self._h, C.c_void_p(dev_ptr), nframes, fmt), "pdt_demod_device_channel")
        return self

    def survey(self, x: np.ndarray, **cfg):
        """The carriers of a wideband I,Q capture in host memory (after set_channel, whose offset plays no part): a list of
        Carrier(offset_hz, peak_db, floor_power), strongest first.  cfg: fields of pdt_survey_cfg (nfft, max_carriers, threshold_db,
        guard_hz, merge_hz, first_frame, nframes), zero or absent = the default."""
        a, fmt = _wb_samples(x)
        c, cap = _survey_cfg(cfg)
        rec, count = (CarrierRec * cap)(), C.c_int(0)
        _check(self._L.pdt_survey(self._h, a.ctypes.data, a.size // 2, fmt, C.byref(c) if c else None, rec, cap, C.byref(count)), "pdt_survey")
        self._survey_nfft = int(cfg.get("nfft", 0)) or 16384
        return _carriers(rec, count.value)

    def survey_device(self, dev_ptr: int, nframes: int, fmt: int = FMT_WB_PCM16, **cfg):
        """survey() of a capture resident in HBM (nframes I,Q frames of FMT_WB_*), which is only read."""
        c, cap = _survey_cfg(cfg)
        rec, count = (CarrierRec * cap)(), C.c_int(0)
        _check(self._L.pdt_survey_device(self._h, C.c_void_p(dev_ptr), nframes, fmt, C.byref(c) if c else None, rec, cap, C.byref(count)),
               "pdt_survey_device")
        self._survey_nfft = int(cfg.get("nfft", 0)) or 16384
        return _carriers(rec, count.value)

    def survey_spectrum(self) -> np.ndarray:
        """The averaged spectrum of the last survey, float32[nfft]: bin b at b Fs_in / nfft, the upper half the negative frequencies."""
        out = np.zeros(getattr(self, "_survey_nfft", 16384), dtype=np.float32)
        _check(self._L.pdt_survey_spectrum(self._h, out.ctypes.data, out.size), "pdt_survey_spectrum")
        return out

    def bursts(self, x: np.ndarray, **cfg):
        """The short transmissions of a wideband I,Q capture in host memory (after set_channel, whose offset plays no part): a list
        of Burst(first_row, rows, start_s, duration_s, offset_hz, peak_db, floor_power) ordered by start, then offset.  cfg: fields
        of pdt_bursts_cfg (nfft, rows_per, gap_rows, threshold_db, guard_hz, merge_hz, min_s, max_s, first_frame, nframes), zero or
        absent = the default, and cap (room for that many bursts, default 4096)."""
        a, fmt = _wb_samples(x)
        c, cap = _bursts_cfg(cfg)
        rec, count = (BurstRec * max(cap, 1))(), C.c_int(0)
        _check(self._L.pdt_bursts(self._h, a.ctypes.data, a.size // 2, fmt, C.byref(c) if c else None, rec, cap, C.byref(count)), "pdt_bursts")
        return _bursts(rec, count.value, cap)

    def bursts_device(self, dev_ptr: int, nframes: int, fmt: int = FMT_WB_PCM16, **cfg):
        """bursts() of a capture resident in HBM (nframes I,Q frames of FMT_WB_*), which is only read."""
        c, cap = _bursts_cfg(cfg)
        rec, count = (BurstRec * max(cap, 1))(), C.c_int(0)
        _check(self._L.pdt_bursts_device(self._h, C.c_void_p(dev_ptr), nframes, fmt, C.byref(c) if c else None, rec, cap, C.byref(count)),
               "pdt_bursts_device")
        return _bursts(rec, count.value, cap)

    def bursts_shape(self):
        """(nfft, rows_per, rows) of the context's last burst search."""
        nfft, per, nrows = C.c_int(0), C.c_int(0), C.c_uint64(0)
        _check(self._L.pdt_bursts_shape(self._h, C.byref(nfft), C.byref(per), C.byref(nrows)), "pdt_bursts_shape")
        return nfft.value, per.value, nrows.value

    def waterfall_rows(self, first_row: int, nrows: int) -> np.ndarray:
        """Rows of the last burst search, float32[nrows, nfft] (bin b at b Fs_in / nfft), computed again from the capture, which
        must still be where it was."""
        nfft, _, total = self.bursts_shape()
        if nrows < 1 or first_row < 0 or first_row + nrows > total:
            raise PdtError(f"rows {first_row} .. {first_row + nrows - 1} are not rows of the last burst search ({total} rows)")
        out = np.zeros((nrows, nfft), dtype=np.float32)
        _check(self._L.pdt_waterfall_rows(self._h, first_row, nrows, out.ctypes.data), "pdt_waterfall_rows")
        return out

    def burst_peaks(self, first_row: int, nrows: int):
        """The peaks of rows of the last burst search: (ROW_PEAK_DTYPE[nrows, 8], counts int32[nrows])."""
        peaks, counts = np.zeros((max(nrows, 1), BURST_ROW_PEAKS), dtype=ROW_PEAK_DTYPE), np.zeros(max(nrows, 1), dtype=np.int32)
        _check(self._L.pdt_burst_peaks(self._h, first_row, nrows, peaks.ctypes.data, counts.ctypes.data), "pdt_burst_peaks")
        return peaks, counts

    def demod_windows_held(self, ds, windows):
        """pdt_demod_windows_held: demod_windows() on the capture this context's last bursts() or survey() call read (it must still
        be where it was): ds[i] demodulates windows[i].  This context itself may not be among ds; its results are left alone."""
        if len(ds) != len(windows):
            raise ValueError("demod_windows_held: lists of different lengths")
        hs = (C.c_void_p * max(len(ds), 1))(*[d._h for d in ds])
        _check(self._L.pdt_demod_windows_held(self._h, hs, len(ds), _window_recs(windows)), "pdt_demod_windows_held")

    def tones(self, **cfg) -> np.ndarray:
        """pdt_tones: the carrier of this context's channel stream (the last demod_channel / demod_windows call's), segment by segment:
        TONE_DTYPE[count] with time_s, freq_hz, residual_hz, power, cn0_dbhz, valid and the raw record.  cfg: fields of pdt_tone_cfg
        (nfft, search_hz, noise_lo, noise_hi, first, stride, count), zero or absent = the default, and cap (room for that many)."""
        c, cap = _tone_cfg(cfg)
        out, count = np.zeros(max(cap, 1), dtype=TONE_DTYPE), C.c_int(0)
        _check(self._L.pdt_tones(self._h, C.byref(c) if c else None, out.ctypes.data, cap, C.byref(count)), "pdt_tones")
        return out[:count.value]

    def argos_messages(self, min_run=None, cap: int = 4096, with_count: bool = False, rule=None):
        """pdt_argos_messages: the ARGOS messages in the bits of this context's last whole-capture call -- either polarity, 1 .. 8 blocks,
        with the platform ID -- beside frames(), which stay the reference's.  min_run: the equal bits asked for in front of the sync
        (None = 6).  Returns ARGOS_MSG_DTYPE[min(found, cap)]; with_count: (that, found)."""
        c = _argos_cfg(min_run, rule)
        out, count = np.zeros(max(cap, 1), dtype=ARGOS_MSG_DTYPE), C.c_int(0)
        _check(self._L.pdt_argos_messages(self._h, C.byref(c) if c else None, out.ctypes.data, cap, C.byref(count)), "pdt_argos_messages")
        got = out[:min(count.value, cap)]
        return (got, count.value) if with_count else got

    def ff_bits(self, rate_steps=None, rate_step_ppm=None, residual_hz=None):
        """pdt_ff_bits: feed-forward bit decisions on this context's channel stream (one burst's window): the FF_SYNC_DTYPE record; the
        bits stay on the device for ff_read().  residual_hz None: the carrier is measured as tones() measures its first segment."""
        c = _ff_cfg(rate_steps, rate_step_ppm, residual_hz)
        sync = np.zeros(1, dtype=FF_SYNC_DTYPE)
        _check(self._L.pdt_ff_bits(self._h, C.byref(c) if c else None, sync.ctypes.data), "pdt_ff_bits")
        return sync[0]

    def stage_ff_bits(self, rate: int, iq: np.ndarray, rate_steps=None, rate_step_ppm=None, residual_hz=None) -> FfBits:
        """pdt_stage_ff_bits + pdt_ff_read: the feed-forward kernels on a float32 I,Q stream at `rate` (a plain recording of one burst):
        FfBits(sync, bits, soft, index).  Nothing of this context's results changes."""
        a = np.ascontiguousarray(iq, dtype="<f4").reshape(-1)
        c = _ff_cfg(rate_steps, rate_step_ppm, residual_hz)
        sync = np.zeros(1, dtype=FF_SYNC_DTYPE)
        _check(self._L.pdt_stage_ff_bits(self._h, rate, a.ctypes.data, a.size // 2, C.byref(c) if c else None, sync.ctypes.data), "pdt_stage_ff_bits")
        got = self.ff_read()
        return FfBits(sync[0], got.bits, got.soft, got.index)

    def ff_read(self) -> FfBits:
        """pdt_ff_read: the bits of this context's last ff_bits / ff_messages / stage_ff_bits call (or a batch it was part of):
        FfBits(sync, bits, soft, index)"""
        sync, count = np.zeros(1, dtype=FF_SYNC_DTYPE), C.c_uint64(0)
        _check(self._L.pdt_ff_read(self._h, sync.ctypes.data, None, None, None, 0, C.byref(count)), "pdt_ff_read")
        cap = max(count.value, 1)
        bits, soft, index = np.zeros(cap, dtype=np.uint8), np.zeros(cap, dtype="<f4"), np.zeros(cap, dtype="<i8")
        _check(self._L.pdt_ff_read(self._h, sync.ctypes.data, bits.ctypes.data, soft.ctypes.data, index.ctypes.data, cap, C.byref(count)), "pdt_ff_read")
        k = min(count.value, cap)
        return FfBits(sync[0], bits[:k], soft[:k], index[:k])

    def ff_messages(self, min_run=None, cap: int = 64, rule=None, rate_steps=None, rate_step_ppm=None, residual_hz=None, with_sync: bool = False):
        """pdt_ff_messages: ff_bits(), then the ARGOS messages in those bits by argos_messages()' rule, in one call: ARGOS_MSG_DTYPE[found]
        with time_src = the sample index in the channel stream and time = that / Fs; with_sync: (that, the FF_SYNC_DTYPE record)."""
        c, a = _ff_cfg(rate_steps, rate_step_ppm, residual_hz), _argos_cfg(min_run, rule)
        sync = np.zeros(1, dtype=FF_SYNC_DTYPE)
        out, count = np.zeros(max(cap, 1), dtype=ARGOS_MSG_DTYPE), C.c_int(0)
        _check(self._L.pdt_ff_messages(self._h, C.byref(c) if c else None, C.byref(a) if a else None, sync.ctypes.data, out.ctypes.data, cap,
                                       C.byref(count)), "pdt_ff_messages")
        got = out[:min(count.value, cap)]
        return (got, sync[0]) if with_sync else got

    def ffp_bits(self, **cfg):
        """pdt_ffp_bits: feed-forward carrier, clock and bit decisions on this POES context's channel stream: the FFP_SYNC_DTYPE record;
        the bits stay on the device for ffp_read().  cfg: block_bits, clock_steps, ref_bits, smooth_blocks, residual_hz (None = measured)."""
        c = _ffp_cfg(**cfg)
        sync = np.zeros(1, dtype=FFP_SYNC_DTYPE)
        _check(self._L.pdt_ffp_bits(self._h, C.byref(c) if c else None, sync.ctypes.data), "pdt_ffp_bits")
        return sync[0]

    def ffp_read(self) -> FfpBits:
        """pdt_ffp_read + pdt_ffp_blocks: the bits and the per-block table of this context's last ffp_* / stage_ffp_* call:
        FfpBits(sync, bits, soft, index, blocks)"""
        sync, count = np.zeros(1, dtype=FFP_SYNC_DTYPE), C.c_uint64(0)
        _check(self._L.pdt_ffp_read(self._h, sync.ctypes.data, None, None, None, 0, C.byref(count)), "pdt_ffp_read")
        cap = max(count.value, 1)
        bits, soft, index = np.zeros(cap, dtype=np.uint8), np.zeros(cap, dtype="<f4"), np.zeros(cap, dtype="<i8")
        _check(self._L.pdt_ffp_read(self._h, sync.ctypes.data, bits.ctypes.data, soft.ctypes.data, index.ctypes.data, cap, C.byref(count)), "pdt_ffp_read")
        k = min(count.value, cap)
        nb = C.c_uint64(0)
        _check(self._L.pdt_ffp_blocks(self._h, None, 0, C.byref(nb)), "pdt_ffp_blocks")
        blocks = np.zeros(max(nb.value, 1), dtype=FFP_BLOCK_DTYPE)
        _check(self._L.pdt_ffp_blocks(self._h, blocks.ctypes.data, nb.value, C.byref(nb)), "pdt_ffp_blocks")
        return FfpBits(sync[0], bits[:k], soft[:k], index[:k], blocks[:nb.value])

    def stage_ffp_bits(self, rate: int, iq: np.ndarray, **cfg) -> FfpBits:
        """pdt_stage_ffp_bits + ffp_read(): the feed-forward POES kernels on a float32 I,Q stream at `rate` (a plain recording).  Nothing
        of this context's results changes."""
        a = np.ascontiguousarray(iq, dtype="<f4").reshape(-1)
        c = _ffp_cfg(**cfg)
        sync = np.zeros(1, dtype=FFP_SYNC_DTYPE)
        _check(self._L.pdt_stage_ffp_bits(self._h, rate, a.ctypes.data, a.size // 2, C.byref(c) if c else None, sync.ctypes.data), "pdt_stage_ffp_bits")
        got = self.ffp_read()
        return FfpBits(sync[0], got.bits, got.soft, got.index, got.blocks)

    def ffp_frames(self, max_errors=None, window=None, fly=None, cap: int = 65536, with_info: bool = False, with_count: bool = False, **cfg):
        """pdt_ffp_frames: ffp_bits(), then the minor frames the flywheel finds in those bits, in one call: FRAME_DTYPE[found] with
        time_src = the sample index at which the bit ends and time = that / Fs, seconds of the stream"""
        c, t = _ffp_cfg(**cfg), _tip_sync_cfg(max_errors, window, fly)
        out, info, count = np.zeros(max(cap, 1), dtype=FRAME_DTYPE), np.zeros(max(cap, 1), dtype=TIP_SYNC_INFO_DTYPE), C.c_int(0)
        _check(self._L.pdt_ffp_frames(self._h, C.byref(c) if c else None, C.byref(t) if t else None, None, out.ctypes.data, info.ctypes.data, cap,
                                      C.byref(count)), "pdt_ffp_frames")
        return _tip_sync_result(out, info, count.value, cap, with_info, with_count)

    def stage_ffp_frames(self, rate: int, iq: np.ndarray, max_errors=None, window=None, fly=None, cap: int = 65536, with_info: bool = False,
                         with_count: bool = False, **cfg):
        """pdt_stage_ffp_frames: the same on a float32 I,Q stream at `rate`; the bits through ffp_read()"""
        a = np.ascontiguousarray(iq, dtype="<f4").reshape(-1)
        c, t = _ffp_cfg(**cfg), _tip_sync_cfg(max_errors, window, fly)
        out, info, count = np.zeros(max(cap, 1), dtype=FRAME_DTYPE), np.zeros(max(cap, 1), dtype=TIP_SYNC_INFO_DTYPE), C.c_int(0)
        _check(self._L.pdt_stage_ffp_frames(self._h, rate, a.ctypes.data, a.size // 2, C.byref(c) if c else None, C.byref(t) if t else None, None,
                                            out.ctypes.data, info.ctypes.data, cap, C.byref(count)), "pdt_stage_ffp_frames")
        return _tip_sync_result(out, info, count.value, cap, with_info, with_count)

    def stage_argos_messages(self, bits, min_run=None, cap: int = 4096, with_count: bool = False, rule=None):
        """pdt_stage_argos_messages: the message kernels on a string of '0'/'1' characters; the time stamp of bit k is k"""
        a, c = _bit_string(bits), _argos_cfg(min_run, rule)
        out, count = np.zeros(max(cap, 1), dtype=ARGOS_MSG_DTYPE), C.c_int(0)
        _check(self._L.pdt_stage_argos_messages(self._h, a.ctypes.data, a.size, C.byref(c) if c else None, out.ctypes.data, cap, C.byref(count)),
               "pdt_stage_argos_messages")
        got = out[:min(count.value, cap)]
        return (got, count.value) if with_count else got

    def device_math(self, fn: int, records: np.ndarray) -> np.ndarray:
        """pdt_device_math (test hook): the kernels' scalar primitive `fn` evaluated on this context's GPU, one record per lane.
        records: [n, nin] (or [n] where nin is 1) of the code's element type -- it is not converted; returns [n, nout]."""
        dt, nin, nout = device_math_layout(fn)
        a = np.ascontiguousarray(records)
        if a.dtype != dt or a.size % nin:
            raise PdtError(f"pdt_device_math({fn}): records of {nin} x {dt} wanted, got {a.dtype} x {a.shape}")
        n = a.size // nin
        out = np.empty((n, nout), dtype=dt)
        _check(self._L.pdt_device_math(self._h, fn, a.ctypes.data, n, out.ctypes.data), "pdt_device_math")
        return out

    def demod_device(self, dev_ptr: int, nframes: int):
        """Input already resident in HBM (e.g. ``tensor.data_ptr()`` of an int16 torch tensor)."""
        _check(self._L.pdt_demod_device(self._h, C.c_void_p(dev_ptr), nframes), "pdt_demod_device")
        return self

    def bytesync(self, bits: np.ndarray):
        """Stage-level entry: only the sync-word search / frame extraction on a uint8 '0'/'1' array."""
        b = np.ascontiguousarray(bits, dtype=np.uint8)
        _check(self._L.pdt_stage_bytesync(self._h, b.ctypes.data, b.size), "pdt_stage_bytesync")
        return self

    def _dt(self):
        return np.dtype("<f8") if (self.mode == MODE_ARGOS and not self.chain) else np.dtype("<f4")

    def stage_manchester(self, symbols: np.ndarray, resync_threshold: float, state: "ManchesterState | None" = None):
        """ManchesterDecode on these symbols alone (statics in `state`, updated in place): (bits '0'/'1', symbol index per bit)"""
        a = np.ascontiguousarray(symbols, dtype=self._dt())
        bits = np.zeros(a.size + 4, dtype=np.uint8)           # a resynchronisation can make consecutive symbols both end a bit
        bsym = np.zeros(a.size + 4, dtype=np.uint32)
        nb = C.c_uint64(0)
        _check(self._L.pdt_stage_manchester(self._h, a.ctypes.data, a.size, float(resync_threshold),
                                            C.addressof(state) if state is not None else None, bits.ctypes.data, bsym.ctypes.data,
                                            C.addressof(nb)), "pdt_stage_manchester")
        return bits[:nb.value], bsym[:nb.value]

    def stage_fir(self, x: np.ndarray, state: "FirState | None" = None) -> np.ndarray:
        """LowPassFilterInterp (POES) / LowPassFilter (ARGOS) on these inputs alone (ring in `state`, updated in place)"""
        a = np.ascontiguousarray(x, dtype=self._dt())
        out = np.zeros(a.size * self.stats_interp(), dtype=self._dt())
        _check(self._L.pdt_stage_fir(self._h, a.ctypes.data, a.size, C.addressof(state) if state is not None else None,
                                     out.ctypes.data), "pdt_stage_fir")
        return out

    def stage_pll(self, iq: np.ndarray, state: "PllState | None" = None):
        """CarrierTrackPLL on these samples alone (float32[n,2] = `float complex`, or int16[n,2] as the WAV holds them; statics in
        `state`, updated in place): (realDataOut, lockSignalStreamOut, return value)"""
        f32 = np.asarray(iq).dtype.kind == "f"
        a = np.ascontiguousarray(iq, dtype="<f4" if f32 else "<i2").reshape(-1)
        n = a.size // 2
        out = np.zeros(n, dtype=self._dt())
        lock = np.zeros(n, dtype=self._dt())
        ret = C.c_double(0)
        _check(self._L.pdt_stage_pll(self._h, a.ctypes.data, n, 1 if f32 else 0, C.addressof(state) if state is not None else None,
                                     out.ctypes.data, lock.ctypes.data, C.addressof(ret)), "pdt_stage_pll")
        return out, lock, ret.value

    def stage_gardner(self, buf: np.ndarray, n: int, state: "GardnerState | None" = None, neighbour: "np.ndarray | None" = None):
        """GardenerClockRecovery on buf[:n]; `buf` is the caller's whole buffer (what lies behind n is read as it stands);
        returns (symbols, pick index per symbol)"""
        a = np.ascontiguousarray(buf, dtype=self._dt())
        nb = np.ascontiguousarray(neighbour, dtype=self._dt()) if neighbour is not None else None
        cap = int(n / 4) + 64
        sym = np.zeros(cap, dtype=self._dt())
        pick = np.zeros(cap, dtype=np.uint64)
        ns = C.c_uint64(0)
        _check(self._L.pdt_stage_gardner(self._h, a.ctypes.data, int(n), a.size, nb.ctypes.data if nb is not None else None,
                                         C.addressof(state) if state is not None else None, sym.ctypes.data, pick.ctypes.data,
                                         C.addressof(ns)), "pdt_stage_gardner")
        return sym[:ns.value], pick[:ns.value]

    def stage_static_gain(self, iq: np.ndarray, level: float = 1.0) -> float:
        """StaticGain over these samples (int16[n,2] as the WAV holds them, or float32[n,2])"""
        f32 = np.asarray(iq).dtype.kind == "f"
        a = np.ascontiguousarray(iq, dtype="<f4" if f32 else "<i2").reshape(-1)
        g = C.c_double(0)
        _check(self._L.pdt_stage_static_gain(self._h, a.ctypes.data, a.size // 2, 1 if f32 else 0, float(level), C.addressof(g)),
               "pdt_stage_static_gain")
        return g.value

    def stage_mm(self, x: np.ndarray, state: "MmState | None" = None):
        """MMClockRecovery on these samples alone (statics in `state`, updated in place): (symbols, pick index per symbol)"""
        a = np.ascontiguousarray(x, dtype=self._dt())
        cap = int(a.size / 3) + 64
        sym = np.zeros(cap, dtype=self._dt())
        pick = np.zeros(cap, dtype=np.uint64)
        ns = C.c_uint64(0)
        _check(self._L.pdt_stage_mm(self._h, a.ctypes.data, a.size, C.addressof(state) if state is not None else None,
                                    sym.ctypes.data, pick.ctypes.data, C.addressof(ns)), "pdt_stage_mm")
        return sym[:ns.value], pick[:ns.value]

    def stage_agc(self, x: np.ndarray, initial: float, state: "AgcState | None" = None, attack: float = 0.0, decay: float = 0.0):
        """NormalizingAGC on these samples alone (gain in `state`, updated in place); returns the output (the reference works in place)"""
        a = np.array(x, dtype=self._dt(), copy=True)
        _check(self._L.pdt_stage_agc(self._h, a.ctypes.data, a.size, float(initial), float(attack), float(decay),
                                     C.addressof(state) if state is not None else None), "pdt_stage_agc")
        return a

    def stage_squelch(self, x: np.ndarray, lock: np.ndarray, threshold: float) -> np.ndarray:
        a = np.array(x, dtype=self._dt(), copy=True)
        l = np.ascontiguousarray(lock, dtype=self._dt())
        assert a.size == l.size
        _check(self._L.pdt_stage_squelch(self._h, a.ctypes.data, l.ctypes.data, a.size, float(threshold)), "pdt_stage_squelch")
        return a

    def fir_form(self) -> "tuple[int, int]":
        """pdt_dev_fir_form (test-only, include/pdt_dev.h): (the filter kernel the last run took -- 0 none, 1 k_fir_plain, 2 k_mix_fir,
        3 register-tiled, 4 generic --, the AGC tile or run maps it wrote; 0: the AGC built its own)"""
        tiles = C.c_ulonglong(0)
        form = self._L.pdt_dev_fir_form(self._h, C.byref(tiles))
        return int(form), int(tiles.value)

    def stats_interp(self) -> int:
        taps, interp = make_lpf(self.mode, self.sample_rate)
        return int(interp)

    def frames(self) -> list[Frame]:
        n = self._L.pdt_num_frames(self._h)
        arr = (Frame * max(n, 1))()
        got = self._L.pdt_frames(self._h, arr, n)
        return [arr[i] for i in range(got)]

    def frames_array(self) -> np.ndarray:
        """Frames as a structured numpy array (same layout as ``pdt_frame``)."""
        n = self._L.pdt_num_frames(self._h)
        buf = np.zeros(n, dtype=FRAME_DTYPE)
        if n:
            self._L.pdt_frames(self._h, C.cast(buf.ctypes.data, C.POINTER(Frame)), n)
        return buf

    def stats(self) -> Stats:
        s = Stats()
        _check(self._L.pdt_get_stats(self._h, C.byref(s)), "pdt_get_stats")
        return s

    def text(self) -> bytes:
        cap = int(self._L.pdt_num_frames(self._h)) * 352 + 64          # a line is at most 24 + 3 * 104 + 1 characters
        buf = C.create_string_buffer(cap)
        n = self._L.pdt_format_frames(self._h, buf, cap)
        return buf.raw[:n]

    def demod_file_text(self, fd: int, byte_offset: int, nframes: int, text_fd: int, fmt: int = 0) -> int:
        """``pdt_demod_file``: capture file in, frame text out to ``text_fd`` in one call (a large POES file: in overlapped
        segments, each segment's text written while the next one runs); returns the number of text bytes written."""
        nb = C.c_uint64(0)
        _check(self._L.pdt_demod_file(self._h, int(fd), byte_offset, nframes, fmt, int(text_fd), C.byref(nb)), "pdt_demod_file")
        return int(nb.value)

    def write_frames(self, fd: int) -> int:
        """The text of the last run written to an open file descriptor (``pdt_write_frames``: formatted and written in slices
        by a few threads); returns the number of bytes."""
        nb = C.c_uint64(0)
        _check(self._L.pdt_write_frames(self._h, int(fd), C.byref(nb)), "pdt_write_frames")
        return int(nb.value)

    def stage_len(self, st: int) -> int:
        return int(self._L.pdt_stage_len(self._h, st))

    def stage(self, st: int, first: int = 0, count: int | None = None) -> np.ndarray:
        total = self._L.pdt_stage_len(self._h, st)
        if count is None:
            count = max(total - first, 0)
        dt = {ST_SYMIDX: np.int64, ST_BITS: np.uint8, ST_BITSYM: np.uint32}.get(st, self.dtype)
        if st in (ST_ANALYTIC, ST_CHANNEL):
            out = np.zeros((count, 2), dtype=np.float32)
            if count:
                got = self._L.pdt_read_stage(self._h, st, first, count, out.ctypes.data)
                if got < 0:
                    _check(int(got), "pdt_read_stage")
                out = out[:got]
            return out
        out = np.zeros(count, dtype=dt)
        if count:
            got = self._L.pdt_read_stage(self._h, st, first, count, out.ctypes.data)
            if got < 0:
                _check(int(got), "pdt_read_stage")
            out = out[:got]
        return out

    # ---- streaming front end: push blocks, collect frames as they become final
    def stream_begin(self):
        _check(self._L.pdt_stream_begin(self._h), "pdt_stream_begin")
        return self

    def _stream_new(self, n: int) -> np.ndarray:
        buf = np.zeros(n, dtype=FRAME_DTYPE)
        if n:
            self._L.pdt_stream_frames(self._h, buf.ctypes.data, n)
        return buf

    def stream_push(self, iq: np.ndarray) -> np.ndarray:
        """Append a block (int16 or float32 I,Q pairs); returns the frames that became final with it."""
        n = C.c_uint64(0)
        if np.asarray(iq).dtype.kind == "f":
            a = np.ascontiguousarray(iq, dtype="<f4").reshape(-1)
            _check(self._L.pdt_stream_push_f32(self._h, a.ctypes.data, a.size // 2, C.byref(n)), "pdt_stream_push_f32")
        else:
            a = np.ascontiguousarray(iq, dtype="<i2").reshape(-1)
            _check(self._L.pdt_stream_push_pcm16(self._h, a.ctypes.data, a.size // 2, C.byref(n)), "pdt_stream_push_pcm16")
        return self._stream_new(n.value)

    def stream_push_real(self, x: np.ndarray) -> np.ndarray:
        """Append single-channel samples (int16 or float32); returns the frames that became final with them."""
        n = C.c_uint64(0)
        a, fmt = _real_samples(x)
        _check(self._L.pdt_stream_push_real(self._h, a.ctypes.data, a.size, fmt, C.byref(n)), "pdt_stream_push_real")
        return self._stream_new(n.value)

    def stream_push_channel(self, x: np.ndarray) -> np.ndarray:
        """Append wideband I,Q frames (uint8, int8, int16 or float32 pairs); returns the frames that became final with them."""
        n = C.c_uint64(0)
        a, fmt = _wb_samples(x)
        _check(self._L.pdt_stream_push_channel(self._h, a.ctypes.data, a.size // 2, fmt, C.byref(n)), "pdt_stream_push_channel")
        return self._stream_new(n.value)

    def stream_end(self) -> np.ndarray:
        """The capture is over: returns the remaining frames; text()/stats()/frames_array() then describe all of it."""
        n = C.c_uint64(0)
        _check(self._L.pdt_stream_end(self._h, C.byref(n)), "pdt_stream_end")
        return self._stream_new(n.value)

    def stream_retained(self) -> int:
        """Input samples the device currently holds for the stream (history + not yet demodulated): bounded."""
        return int(self._L.pdt_stream_retained(self._h))

    def tip_check(self):
        """Frame validation of the last demodulation (the reference's MATLAB checkParity.m / daytimeDecode.m,
        on the GPU): (summary dict, per-frame structured array)."""
        sm = TipSummary()
        _check(self._L.pdt_tip_check(self._h, C.byref(sm)), "pdt_tip_check")
        n = self._L.pdt_num_frames(self._h)
        rec = np.zeros(n, dtype=TIP_DTYPE)
        if n:
            self._L.pdt_tip_frames(self._h, rec.ctypes.data, n)
        return {k: int(getattr(sm, k)) for k, _ in TipSummary._fields_}, rec

    def tip_check_records(self, frames):
        """pdt_tip_check_records: tip_check()'s validation on a caller's FRAME_DTYPE array (the frames of tip_sync(), say): (summary dict,
        per-frame structured array).  The context's own results stay as they were."""
        a = np.ascontiguousarray(frames, dtype=FRAME_DTYPE)
        sm, rec = TipSummary(), np.zeros(max(len(a), 1), dtype=TIP_DTYPE)
        _check(self._L.pdt_tip_check_records(self._h, a.ctypes.data, len(a), C.byref(sm), rec.ctypes.data), "pdt_tip_check_records")
        return {k: int(getattr(sm, k)) for k, _ in TipSummary._fields_}, rec[:len(a)]

    def tip_repair(self, frames):
        """pdt_tip_repair: the failed parity groups of FRAME_DTYPE records (those of ffp_frames(), say) repaired from the soft values this
        context's last ffp_* / stage_ffp_* call left on the device: (repaired copy, TIP_REPAIR_INFO_DTYPE[len], summary dict).  The
        context's own results stay as they were."""
        a = np.array(frames, dtype=FRAME_DTYPE, copy=True).reshape(-1)
        info, sm = np.zeros(max(len(a), 1), dtype=TIP_REPAIR_INFO_DTYPE), TipRepairSummary()
        _check(self._L.pdt_tip_repair(self._h, a.ctypes.data, len(a), info.ctypes.data, C.byref(sm)), "pdt_tip_repair")
        return _tip_repair_result(a, info, sm)

    def stage_tip_repair(self, soft, frames):
        """pdt_stage_tip_repair: the same kernel on a caller's float32 soft values from any source"""
        s = np.ascontiguousarray(soft, dtype="<f4").reshape(-1)
        a = np.array(frames, dtype=FRAME_DTYPE, copy=True).reshape(-1)
        info, sm = np.zeros(max(len(a), 1), dtype=TIP_REPAIR_INFO_DTYPE), TipRepairSummary()
        _check(self._L.pdt_stage_tip_repair(self._h, s.ctypes.data, s.size, a.ctypes.data, len(a), info.ctypes.data, C.byref(sm)),
               "pdt_stage_tip_repair")
        return _tip_repair_result(a, info, sm)

    def tip_dcs(self, channel_max: int = 0, cap: int = 65536):
        """pdt_tip_dcs: the DCS-2 platform messages in the minor frames of this context's last demodulation, which are still on the device:
        (DCS_PACKET_DTYPE[min(found, cap)], found, summary dict).  The context's own results stay as they were."""
        c = DcsCfg(channel_max, 0)
        out, count, sm = np.zeros(max(cap, 1), dtype=DCS_PACKET_DTYPE), C.c_int(0), DcsSummary()
        _check(self._L.pdt_tip_dcs(self._h, C.byref(c), out.ctypes.data if cap else None, cap, C.byref(count), C.byref(sm)), "pdt_tip_dcs")
        return _dcs_result(out, count.value, cap, sm)

    def tip_dcs_records(self, frames, channel_max: int = 0, cap: int = 65536):
        """pdt_tip_dcs_records: the same kernels on a caller's FRAME_DTYPE records (those of tip_sync() or ffp_frames(), repaired or not)"""
        a = np.ascontiguousarray(frames, dtype=FRAME_DTYPE).reshape(-1)
        c = DcsCfg(channel_max, 0)
        out, count, sm = np.zeros(max(cap, 1), dtype=DCS_PACKET_DTYPE), C.c_int(0), DcsSummary()
        _check(self._L.pdt_tip_dcs_records(self._h, a.ctypes.data, len(a), C.byref(c), out.ctypes.data if cap else None, cap, C.byref(count), C.byref(sm)),
               "pdt_tip_dcs_records")
        return _dcs_result(out, count.value, cap, sm)

    def tip_subcom(self, table=SUBCOM_SEM, trusted_only: bool = False, spike_threshold: int = 0, cap: int = 65536):
        """pdt_tip_subcom: the subcommutated bytes, by `table`, of the minor frames of this context's last demodulation, which are still on the
        device: (SUBCOM_SAMPLE_DTYPE[min(found, cap)], found, offsets, summary dict).  The context's own results stay as they were."""
        return _subcom_call(self._L.pdt_tip_subcom, "pdt_tip_subcom", (self._h,), table, trusted_only, spike_threshold, cap)

    def tip_subcom_records(self, frames, table=SUBCOM_SEM, trusted_only: bool = False, spike_threshold: int = 0, cap: int = 65536):
        """pdt_tip_subcom_records: the same kernels on a caller's FRAME_DTYPE records (those of tip_sync() or ffp_frames(), repaired or not)"""
        a = np.ascontiguousarray(frames, dtype=FRAME_DTYPE).reshape(-1)
        return _subcom_call(self._L.pdt_tip_subcom_records, "pdt_tip_subcom_records", (self._h, a.ctypes.data, len(a)), table, trusted_only, spike_threshold, cap)

    def tip_sync(self, max_errors=None, window=None, fly=None, cap: int = 65536, with_info: bool = False, with_count: bool = False):
        """pdt_tip_sync: the POES minor frames a flywheel synchroniser finds in the bits of this context's last whole-capture call -- a
        sync word with up to max_errors wrong bits (None = 2) counts when a neighbouring slot within `window` frames (None = 2) has one
        too, and a slot with `fly` such neighbours (None = 3) is a frame whatever its own sync word.  Returns FRAME_DTYPE[min(found,
        cap)]; with_info: (that, TIP_SYNC_INFO_DTYPE[..]); with_count: (that, found).  Frames, text and stages stay as they were."""
        c = _tip_sync_cfg(max_errors, window, fly)
        out, info, count = np.zeros(max(cap, 1), dtype=FRAME_DTYPE), np.zeros(max(cap, 1), dtype=TIP_SYNC_INFO_DTYPE), C.c_int(0)
        _check(self._L.pdt_tip_sync(self._h, C.byref(c) if c else None, out.ctypes.data, info.ctypes.data, cap, C.byref(count)), "pdt_tip_sync")
        return _tip_sync_result(out, info, count.value, cap, with_info, with_count)

    def stage_tip_sync(self, bits, max_errors=None, window=None, fly=None, cap: int = 65536, with_info: bool = False, with_count: bool = False):
        """pdt_stage_tip_sync: the flywheel's kernels on a string of '0'/'1' characters; the time stamp of bit k is k"""
        a, c = _bit_string(bits), _tip_sync_cfg(max_errors, window, fly)
        out, info, count = np.zeros(max(cap, 1), dtype=FRAME_DTYPE), np.zeros(max(cap, 1), dtype=TIP_SYNC_INFO_DTYPE), C.c_int(0)
        _check(self._L.pdt_stage_tip_sync(self._h, a.ctypes.data, a.size, C.byref(c) if c else None, out.ctypes.data, info.ctypes.data, cap,
                                          C.byref(count)), "pdt_stage_tip_sync")
        return _tip_sync_result(out, info, count.value, cap, with_info, with_count)

    def kernel_times(self) -> dict[str, tuple[int, float]]:
        n = self._L.pdt_kernel_times(self._h, None, 0)
        arr = (KernelTime * max(n, 1))()
        self._L.pdt_kernel_times(self._h, arr, n)
        return {arr[i].name.decode(): (arr[i].launches, arr[i].total_ms) for i in range(n)}


def demod_batch(demods, dev_ptrs, nframes):
    """Batched many-capture mode: demods[i] demodulates the int16 I/Q capture at device address dev_ptrs[i]
    (nframes[i] pairs); the kernels of all captures overlap on the GPU.  Results are read from each Demodulator."""
    n = len(demods)
    if not (n == len(dev_ptrs) == len(nframes)):
        raise ValueError("demod_batch: lists of different lengths")
    hs = (C.c_void_p * max(n, 1))(*[d._h for d in demods])
    ps = (C.c_void_p * max(n, 1))(*[C.c_void_p(int(p)) for p in dev_ptrs])
    ns = (C.c_uint64 * max(n, 1))(*[int(v) for v in nframes])
    _check(lib().pdt_demod_batch_device(hs, ps, ns, n), "pdt_demod_batch_device")


def demod_channels(demods, dev_ptr, nframes: int = 0, fmt: int = FMT_WB_PCM16):
    """Several channels of ONE wideband capture: demods[i] (each with its set_channel, all of one decim) demodulates its channel;
    the capture is ingested once and converted by one launch per context, then the contexts share the batched chain.  dev_ptr: the address of the
    capture in HBM (nframes I,Q frames of fmt), or a numpy array of I,Q pairs in host memory (pdt_demod_channels)."""
    n = len(demods)
    hs = (C.c_void_p * max(n, 1))(*[d._h for d in demods])
    if isinstance(dev_ptr, np.ndarray):
        a, fmt = _wb_samples(dev_ptr)
        _check(lib().pdt_demod_channels(hs, n, a.ctypes.data, a.size // 2, fmt), "pdt_demod_channels")
        return
    _check(lib().pdt_demod_channels_device(hs, n, C.c_void_p(int(dev_ptr)), int(nframes), fmt), "pdt_demod_channels_device")


def demod_windows(ds, x_or_ptr, nframes: int, fmt: int, windows):
    """Every window of ONE wideband capture on a context of its own: ds[i] (after set_channel, all of one decim) demodulates
    windows[i] = (first_frame, nframes, offset_hz) as a capture of its own at that offset -- what set_channel + demod_device_channel
    on the slice would give -- all windows converted by one launch, then the batched chain.  x_or_ptr: the address of the capture in
    HBM (nframes I,Q frames of fmt), or a numpy array of I,Q pairs in host memory (pdt_demod_windows; nframes and fmt are the array's)."""
    if len(ds) != len(windows):
        raise ValueError("demod_windows: lists of different lengths")
    n = len(ds)
    hs = (C.c_void_p * max(n, 1))(*[d._h for d in ds])
    if isinstance(x_or_ptr, np.ndarray):
        a, fmt = _wb_samples(x_or_ptr)
        _check(lib().pdt_demod_windows(hs, n, _window_recs(windows), a.ctypes.data, a.size // 2, fmt), "pdt_demod_windows")
        return
    _check(lib().pdt_demod_windows_device(hs, n, _window_recs(windows), C.c_void_p(int(x_or_ptr)), int(nframes), fmt), "pdt_demod_windows_device")


FRAME_DTYPE = np.dtype([
    ("time", "<f8"), ("bit_index", "<i8"), ("time_src", "<i8"), ("inverted", "u1"), ("nbytes", "u1"),
    ("complete", "u1"), ("pad", "u1"), ("bytes", "u1", (104,)), ("_tail", "u1", (4,)),   # C struct is padded to 136
])
assert FRAME_DTYPE.itemsize == C.sizeof(Frame)


def format_frames(frames: np.ndarray) -> bytes:
    """Text of a (possibly gathered) frame array: ``pdt_format_records`` (host-only C, no GPU needed)."""
    a = np.ascontiguousarray(frames, dtype=FRAME_DTYPE)
    L = lib()
    n = L.pdt_format_records(a.ctypes.data, len(a), None, 0)
    buf = C.create_string_buffer(n + 1)
    L.pdt_format_records(a.ctypes.data, len(a), buf, n)
    return buf.raw[:n]


def format_frames_py(frames: np.ndarray) -> bytes:
    """The same text through Python's own "%.5f" / "%.2X" (the reference's printf formats); used by the tests."""
    out = []
    for f in frames:
        out.append((b"%.5fi " if f["inverted"] else b"%.5f ") % f["time"])
        out.append(b"".join(b"%.2X " % b for b in f["bytes"][: f["nbytes"]]))
        if f["complete"]:
            out.append(b"\n")
    return b"".join(out)


# ------------------------------------------------------------------ synthetic captures
class SynthParams(C.Structure):
    _fields_ = [
        ("kind", C.c_uint32), ("sample_rate", C.c_uint32), ("carrier_step", C.c_uint32), ("phase0", C.c_uint32),
        ("mod_index", C.c_uint32), ("amplitude", C.c_int32), ("noise_gain", C.c_int32), ("seed", C.c_uint64),
        ("signal_start", C.c_uint64), ("signal_end", C.c_uint64), ("doppler_q32", C.c_int64), ("env_floor_q15", C.c_uint32),
        ("fade_q15", C.c_uint32), ("fade_start", C.c_uint64), ("fade_len", C.c_uint64),
    ]


_synth = None


def synth_lib():
    global _synth
    if _synth is None:
        if not os.path.exists(LIBSYNTH_PATH):
            raise PdtError(f"{LIBSYNTH_PATH} is missing: run `make`")
        S = C.CDLL(LIBSYNTH_PATH)
        S.pdt_synth_default_params.argtypes = [C.POINTER(SynthParams), C.c_int, C.c_uint32, C.c_double, C.c_uint64]
        S.pdt_synth_default_params.restype = None
        S.pdt_synth_set_pass.argtypes = [C.POINTER(SynthParams), C.c_uint64, C.c_uint64, C.c_double, C.c_double, C.c_double]
        S.pdt_synth_set_pass.restype = None
        S.pdt_synth_fill.argtypes = [C.POINTER(SynthParams), C.c_uint64, C.c_uint64, C.c_void_p]
        S.pdt_synth_fill.restype = None
        S.pdt_synth_poes_frame.argtypes = [C.POINTER(SynthParams), C.c_uint64, C.c_void_p]
        S.pdt_synth_poes_frame.restype = None
        S.pdt_synth_argos_payload.argtypes = [C.POINTER(SynthParams), C.c_uint64, C.c_void_p]
        S.pdt_synth_argos_payload.restype = None
        S.pdt_synth_argos_message.argtypes = [C.POINTER(SynthParams), C.c_uint64, C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.c_void_p]
        S.pdt_synth_argos_message.restype = None
        S.pdt_synth_dcs_packet.argtypes = [C.POINTER(SynthParams), C.c_uint64, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        S.pdt_synth_dcs_packet.restype = None
        S.pdt_synth_sine_table.restype = C.POINTER(C.c_int16)
        S.pdt_synth_wav_header.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64]
        S.pdt_synth_wav_header.restype = None
        _synth = S
    return _synth


def synth_params(kind: int, sample_rate: int, f0_hz: float = 1000.0, seed: int = 1234) -> SynthParams:
    p = SynthParams()
    synth_lib().pdt_synth_default_params(C.byref(p), kind, sample_rate, f0_hz, seed)
    return p


def synth_capture(kind: int, sample_rate: int, seconds: float, f0_hz: float | None = None, seed: int = 1234,
                  start: int = 0) -> np.ndarray:
    """int16[n,2] synthetic POES (kind 0) / ARGOS (kind 1; kind 2: messages of 1 .. 8 blocks) capture; bit-reproducible everywhere."""
    if f0_hz is None:
        f0_hz = 1000.0 if kind in (0, 3, 4) else 120.0         # (kind 3: POES frames that carry their parity; kind 4: and a DCS stream)
    p = synth_params(kind, sample_rate, f0_hz, seed)
    n = int(round(seconds * sample_rate))
    out = np.zeros((n, 2), dtype="<i2")
    synth_lib().pdt_synth_fill(C.byref(p), start, n, out.ctypes.data)
    return out


def synth_poes_frame(p: SynthParams, fr: int) -> np.ndarray:
    out = np.zeros(104, dtype=np.uint8)
    synth_lib().pdt_synth_poes_frame(C.byref(p), fr, out.ctypes.data)
    return out


def synth_argos_payload(p: SynthParams, burst: int) -> np.ndarray:
    out = np.zeros(7, dtype=np.uint8)
    synth_lib().pdt_synth_argos_payload(C.byref(p), burst, out.ctypes.data)
    return out


def synth_argos_message(p: SynthParams, burst: int) -> tuple[int, int, np.ndarray]:
    """kind 2: (blocks, id, the 4 * blocks data bytes) of the message burst `burst` carries"""
    blocks, ident, data = C.c_int(0), C.c_uint32(0), np.zeros(32, dtype=np.uint8)
    synth_lib().pdt_synth_argos_message(C.byref(p), burst, C.byref(blocks), C.byref(ident), data.ctypes.data)
    return blocks.value, ident.value, data[:4 * blocks.value]


def synth_dcs_packet(p: SynthParams, s: int, which: int) -> np.ndarray:
    """kind 4: the bytes of DCS packet `which` (0 = A, 1 = B) of slot group s as transmitted"""
    out, n = np.zeros(44, dtype=np.uint8), C.c_int(0)
    synth_lib().pdt_synth_dcs_packet(C.byref(p), s, which, out.ctypes.data, C.byref(n))
    return out[:n.value]


def write_wav(path: str, sample_rate: int, iq: np.ndarray):
    hdr = C.create_string_buffer(44)
    synth_lib().pdt_synth_wav_header(hdr, sample_rate, iq.shape[0])
    with open(path, "wb") as f:
        f.write(hdr.raw)
        f.write(np.ascontiguousarray(iq, dtype="<i2").tobytes())
