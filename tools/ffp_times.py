"""The feed-forward POES kernels on the GPU beside the chain's route to the same capture's frames, on two captures:

(a) `bench.py --config pass`'s capture (15 min at 250 ksps, 225 M samples, synthesised as bench does; --pass-seconds shortens it)
(b) 30 s at 50 ksps, the weak capture of the tests (noise x 9)

For each: the chain (pdt_demod_device on the capture in HBM, then pdt_tip_sync) -- wall time of each call and the chain's own gpu_ms --
and pdt_stage_ffp_frames on the same samples as float32 / 32768 from host memory: wall time of the call (it carries the upload of 8
bytes a sample and the tone records' round trip), the four kernels from pdt_kernel_times of the profiled context, and the frames of
both routes.  --reps calls of each, in order; the first carries first-use costs.  One JSON to --out.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = ("k_ffp_mix", "k_ffp_search", "k_ffp_track", "k_ffp_bits")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pass-seconds", type=float, default=900.0)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import torch
    pdt = importlib.import_module("project-desert-tortoise_amd")
    import bench
    import test_tip_sync as cpu
    result = {"build": pdt.build_tag(), "kernels": NAMES}

    def run(name, fs, dev_iq, n):
        host = dev_iq.cpu().numpy().reshape(-1, 2)
        y = host.astype(np.float32) / np.float32(32768.0)
        del host
        row = {"rate": fs, "samples": n, "chain": [], "ffp": []}
        with pdt.Demodulator(pdt.MODE_POES, fs, profile=True) as d:
            for _ in range(args.reps):
                t0 = time.perf_counter()
                d.demod_device(dev_iq.data_ptr(), n)
                t1 = time.perf_counter()
                fly = d.tip_sync()
                t2 = time.perf_counter()
                row["chain"].append({"demod_ms": round(1e3 * (t1 - t0), 2), "gpu_ms": round(d.stats().gpu_ms, 2), "tip_sync_ms": round(1e3 * (t2 - t1), 2),
                                     "rule0_frames": int(d.frames_array()["complete"].sum()), "flywheel_frames": len(fly)})
            for _ in range(args.reps):
                t0 = time.perf_counter()
                fr = d.stage_ffp_frames(fs, y)
                t1 = time.perf_counter()
                times = d.kernel_times()
                sync = d.ffp_read().sync
                row["ffp"].append({"call_ms": round(1e3 * (t1 - t0), 2), "ms_per_kernel": [round(times[k][1], 4) for k in NAMES], "frames": len(fr),
                                   "bits": int(sync["nbits"]), "blocks": int(sync["nblocks"]), "segs_valid": [int(sync["segs_valid"]), int(sync["segs"])]})
        result[name] = row
        print(json.dumps({name: row}), flush=True)

    p = bench.capture_params(pdt, "pass", 1, args.pass_seconds)
    n = int(round(args.pass_seconds * 250000))
    run("pass", 250000, bench.make_capture(pdt, p, n, 8, device="cuda:0"), n)
    torch.cuda.empty_cache()
    _, x = cpu.weak_capture(pdt)
    run("weak_30s", 50000, torch.from_numpy(x.reshape(-1).copy()).to("cuda:0"), len(x))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
