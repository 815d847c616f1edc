"""The carrier measurement, three runs:

--mode kernel --nfft N   a random float32 capture of 2 x 2^24 pairs resident in HBM becomes a POES context's channel stream of S N = 2^24
                         pairs (decimation 2); pdt_tones measures its S segments --reps + 1 times (one k_tones launch each).  Beside
                         it the survey's kernel on as many float segments: one pdt_bursts_device call at rows_per = 1 over S N pairs
                         of the capture (two k_spectra launches over S segments: the survey's at 64 segments a row and the
                         waterfall's at one), then --reps pdt_waterfall_rows calls (k_spectra at one segment a row over the S
                         segments, a slab at a time).
--mode windows           the two-platform ARGOS capture of tests/test_gpu_windows.py, its bursts' windows demodulated once on as many
                         contexts, then the whole pdt_tones_batch call for their first segments: wall time, median of --reps.
--mode poes              a channel of --minutes at 250 ksps (noise: the time does not depend on the content) and the whole pdt_tones
                         call at stride N along it.

Run it under `rocprofv3 --kernel-trace --stats -f csv -d DIR -o tones -- python tools/tone_bench.py ...` for the kernels' own time (no
counters); `--stats FILE --mode kernel --nfft N` then turns that file's k_tones and k_spectra rows into time per segment.
"""
import argparse
import csv
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IN_RATE, DECIM = 1024000, 32
OFFSETS, SEEDS, RESIDUAL = (250000.0, -333300.0), (8, 9), 120.0
POES_FS, POES_D = 250000, 2
TOTAL = 1 << 24                                  # channel samples of --mode kernel


def kernel_times(path: str, nfft: int, reps: int) -> dict:
    seg = TOTAL // nfft
    out = {"nfft": nfft, "segments": seg}
    with open(path) as f:
        for r in csv.DictReader(f):
            for k in ("k_tones", "k_spectra"):
                if k in r["Name"]:
                    out[k + "_ms"] = round(out.get(k + "_ms", 0.0) + float(r["TotalDurationNs"]) / 1e6, 3)
                    out[k + "_launches"] = out.get(k + "_launches", 0) + int(r["Calls"])
    if "k_tones_ms" in out:
        out["k_tones_us_per_segment"] = round(1e3 * out["k_tones_ms"] / (out["k_tones_launches"] * seg), 4)     # (every launch measures all segments)
    if "k_spectra_ms" in out:                    # (the search's two passes and the --reps waterfalls: reps + 2 passes over the segments)
        out["k_spectra_us_per_segment"] = round(1e3 * out["k_spectra_ms"] / ((reps + 2) * seg), 4)
    return out


def median_ms(fn, reps: int) -> float:
    ts = []
    for _ in range(reps + 1):                    # (the first call allocates)
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ts[1:])), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("kernel", "windows", "poes"), default="kernel")
    ap.add_argument("--nfft", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--minutes", type=float, default=15.0)
    ap.add_argument("--stats", help="rocprofv3 kernel_stats.csv of an earlier --mode kernel run: the kernels' time per segment")
    a = ap.parse_args()
    if a.stats:
        print(json.dumps(kernel_times(a.stats, a.nfft, a.reps)))
        return
    import torch
    pdt = importlib.import_module("project-desert-tortoise_amd")
    out = {"mode": a.mode, "build": pdt.build_tag()}
    if a.mode == "kernel":
        seg = TOTAL // a.nfft
        dev = torch.rand(2 * POES_D * TOTAL, device="cuda", dtype=torch.float32) * 2.0 - 1.0
        torch.cuda.synchronize()
        with pdt.Demodulator(pdt.MODE_POES, POES_FS) as d:
            d.set_channel(POES_D, 100000.0).demod_device_channel(dev.data_ptr(), POES_D * TOTAL, pdt.FMT_WB_F32)
            out["tones_call_ms"] = median_ms(lambda: d.tones(nfft=a.nfft, cap=seg), a.reps)
            out["segments"] = len(d.tones(nfft=a.nfft, cap=seg))
        with pdt.Demodulator(pdt.MODE_POES, POES_FS) as d:
            d.set_channel(POES_D, 0.0)
            d.bursts_device(dev.data_ptr(), TOTAL, pdt.FMT_WB_F32, nfft=a.nfft, rows_per=1)
            out["waterfall_call_ms"] = median_ms(lambda: d.waterfall_rows(0, seg), a.reps - 1)
        out["nfft"] = a.nfft
    elif a.mode == "windows":
        n = int(15.0 * IN_RATE)
        total = np.zeros((n, 2), dtype=np.int32)
        for off, seed in zip(OFFSETS, SEEDS):
            p = pdt.synth_params(1, IN_RATE, off + RESIDUAL, seed)
            p.amplitude //= 2
            p.noise_gain //= 2
            iq = np.zeros((n, 2), dtype="<i2")
            pdt.synth_lib().pdt_synth_fill(C.byref(p), 0, n, iq.ctypes.data)
            total += iq
        x = np.clip(total, -32768, 32767).astype(np.int16)
        fs = IN_RATE // DECIM
        with pdt.Demodulator(pdt.MODE_ARGOS, fs) as holder:
            holder.set_channel(DECIM, 0.0)
            windows = pdt.burst_windows(holder.bursts(x), IN_RATE, n)
            ds = [pdt.Demodulator(pdt.MODE_ARGOS, fs).set_channel(DECIM, 0.0) for _ in windows]
            try:
                holder.demod_windows_held(ds, windows)
                out["windows"] = len(windows)
                out["batch_call_ms"] = median_ms(lambda: pdt.tones_batch(ds, count=1, cap=1), a.reps)
                rec = np.concatenate(pdt.tones_batch(ds, count=1, cap=1))
                out["cn0_dbhz_mean"] = round(float(rec["cn0_dbhz"].mean()), 2)
            finally:
                for d in ds:
                    d.close()
    else:
        m = int(a.minutes * 60 * POES_FS)
        dev = torch.randint(96, 160, (2 * POES_D * m,), device="cuda", dtype=torch.uint8)
        torch.cuda.synchronize()
        with pdt.Demodulator(pdt.MODE_POES, POES_FS) as d:
            d.keep_pll(False)
            d.set_channel(POES_D, 100000.0).demod_device_channel(dev.data_ptr(), POES_D * m, pdt.FMT_WB_CU8)
            cap = m // 16384 + 1
            out["channel_samples"], out["nfft"] = m, 16384
            out["tones_call_ms"] = median_ms(lambda: d.tones(cap=cap), a.reps)
            out["segments"] = len(d.tones(cap=cap))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
