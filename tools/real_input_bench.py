"""The Hilbert front end of single-channel captures: a real PCM16 capture resident in HBM against the I,Q capture of
the same length, through the whole chain (pdt_demod_device_real / pdt_demod_device), wall time per call, median of --reps.

Run it under `rocprofv3 --kernel-trace --stats -d DIR -o real -- python tools/real_input_bench.py` for the conversion kernel's own
time (k_analytic in DIR/.../real_kernel_stats.csv); `--stats FILE` then turns that file's k_analytic row into bytes over time:
2 B in + 8 B out per sample, as a share of 6.3 TB/s (measured copy rate) and 8 TB/s (spec).
"""
import argparse
import csv
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_share(path: str, n: int) -> dict:
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if "k_analytic" in r["Name"]]
    ns = sum(float(r["TotalDurationNs"]) for r in rows)
    calls = sum(int(r["Calls"]) for r in rows)
    per_call_ms = ns / calls / 1e6
    tb_s = 10.0 * n / (per_call_ms * 1e-3) / 1e12
    return {"kernel_ms": round(per_call_ms, 4), "calls": calls, "TB_s": round(tb_s, 3), "of_6.3": round(tb_s / 6.3, 3), "of_8.0": round(tb_s / 8.0, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=900_000_000)
    ap.add_argument("--rate", type=int, default=250000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stats", help="rocprofv3 kernel_stats.csv of an earlier run: print the kernel's share of HBM bandwidth")
    a = ap.parse_args()
    if a.stats:
        print(json.dumps(kernel_share(a.stats, a.samples)))
        return
    import torch
    pdt = importlib.import_module("project-desert-tortoise_amd")
    n, fs = a.samples, a.rate
    iq = pdt.synth_capture(0, fs, n / fs)                                  # carrier at 1 kHz
    d_iq = torch.from_numpy(iq.reshape(-1)).cuda()
    del iq
    x = np.ascontiguousarray(pdt.synth_capture(0, fs, n / fs, f0_hz=fs / 4 + 1000.0)[:, 0])    # the same, real, at Fs / 4 + 1 kHz
    d_x = torch.from_numpy(x).cuda()
    del x
    torch.cuda.synchronize()
    out = {"samples": n, "rate": fs}
    with pdt.Demodulator(pdt.MODE_POES, fs) as d:
        d.keep_pll(False)
        for name, call in (("iq", lambda: d.demod_device(d_iq.data_ptr(), n)),
                           ("real", lambda: d.demod_device_real(d_x.data_ptr(), n, pdt.FMT_REAL_PCM16))):
            call()                                                           # (buffers of this size allocated once)
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                call()
                ts.append((time.perf_counter() - t0) * 1e3)
            out[f"{name}_ms"] = round(float(np.median(ts)), 2)
            out[f"{name}_frames"] = int(d.stats().frames)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
