"""Every burst in a window of its own: the two-platform ARGOS capture of tests/test_gpu_windows.py (1.024 Msps, int16 or
--cu8) resident in HBM, its bursts searched for once, the first --windows of their windows demodulated by one demod_windows call on as
many contexts; wall time of the whole call (one conversion launch and the batched chain), median of --reps.  --single also
demodulates ONE window as long as all of them together through demod_device_channel in the same process: the same kernel over the
same number of input samples, one record by value instead of the table of many.

Run it under `rocprofv3 --kernel-trace --stats -f csv -d DIR -o windows -- python tools/window_bench.py` for the kernel's own time (no
counters); `--stats FILE` then turns that file's k_ddc rows into launches and time.  In a run without --single there must be exactly
one launch per call (reps + 1 of them: the first call allocates); a run with --single has as many launches again, and what it
adds to the time is the single window's.
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


def kernel_times(path: str, calls: int) -> dict:
    out = {"calls": calls}
    with open(path) as f:
        for r in csv.DictReader(f):
            if "k_ddc" in r["Name"]:
                out["k_ddc_ms"] = round(out.get("k_ddc_ms", 0.0) + float(r["TotalDurationNs"]) / 1e6, 3)
                out["k_ddc_launches"] = out.get("k_ddc_launches", 0) + int(r["Calls"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=15.0)
    ap.add_argument("--windows", type=int, default=64, help="at most this many windows (and contexts)")
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--cu8", action="store_true", help="the unsigned 8-bit rendering of the capture")
    ap.add_argument("--single", action="store_true", help="also one window of the same total length through demod_device_channel")
    ap.add_argument("--stats", help="rocprofv3 kernel_stats.csv of an earlier run: print the kernels' launches and total time")
    a = ap.parse_args()
    if a.stats:
        print(json.dumps(kernel_times(a.stats, a.reps + 1)))
        return
    import torch
    pdt = importlib.import_module("project-desert-tortoise_amd")
    n = int(a.seconds * IN_RATE)
    total = np.zeros((n, 2), dtype=np.int32)
    for off, seed in zip(OFFSETS, SEEDS):
        p = pdt.synth_params(1, IN_RATE, off + RESIDUAL, seed)
        p.amplitude //= 2
        p.noise_gain //= 2
        iq = np.zeros((n, 2), dtype="<i2")
        pdt.synth_lib().pdt_synth_fill(C.byref(p), 0, n, iq.ctypes.data)
        total += iq
    x = np.clip(total, -32768, 32767).astype(np.int16)
    if a.cu8:
        x = np.clip(np.floor(x / 256.0) + 128, 0, 255).astype(np.uint8)
    fmt = pdt.FMT_WB_CU8 if a.cu8 else pdt.FMT_WB_PCM16
    dev = torch.from_numpy(x.reshape(-1)).cuda()
    torch.cuda.synchronize()
    fs = IN_RATE // DECIM
    out = {"samples": n, "rate": IN_RATE, "format": "cu8" if a.cu8 else "pcm16"}
    with pdt.Demodulator(pdt.MODE_ARGOS, fs) as holder:
        holder.set_channel(DECIM, 0.0)
        found = holder.bursts_device(dev.data_ptr(), n, fmt)
        windows = pdt.burst_windows(found, IN_RATE, n)[: a.windows]
        out["bursts"], out["windows"] = len(found), len(windows)
        out["window_frames"] = int(sum(w.nframes for w in windows))
        ds = [pdt.Demodulator(pdt.MODE_ARGOS, fs).set_channel(DECIM, 0.0) for _ in windows]
        for d in ds:
            d.keep_pll(False)
        try:
            ts = []
            for _ in range(a.reps + 1):                                                  # (the first call allocates)
                t0 = time.perf_counter()
                pdt.demod_windows(ds, dev.data_ptr(), n, fmt, windows)
                ts.append((time.perf_counter() - t0) * 1e3)
            out["call_ms"] = round(float(np.median(ts[1:])), 2)
            out["packets"] = int(sum(d.stats().frames for d in ds))
            if a.single and windows:
                m = min(out["window_frames"], n)
                ts = []
                for _ in range(a.reps + 1):
                    t0 = time.perf_counter()
                    ds[0].set_channel(DECIM, windows[0].offset_hz).demod_device_channel(dev.data_ptr(), m, fmt)
                    ts.append((time.perf_counter() - t0) * 1e3)
                out["single_frames"], out["single_call_ms"] = m, round(float(np.median(ts[1:])), 2)
        finally:
            for d in ds:
                d.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
