"""k_tip_repair on the GPU behind the feed-forward frames of two captures:

(a) `bench.py --config pass`'s capture (15 min at 250 ksps, 225 M samples, synthesised as bench does; --pass-seconds shortens it)
(b) 30 s at 50 ksps, noise x 9, frames that carry their parity (kind 3): the capture of the tests' survey

For each: pdt_stage_ffp_frames on the samples as float32 / 32768 from host memory, then --reps calls of pdt_tip_repair on its records:
wall time of the call (it carries the records' upload and the way back), the kernel from pdt_kernel_times of the profiled context, the
summary.  The first call carries first-use costs.  One JSON to --out.
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pass-seconds", type=float, default=900.0)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    pdt = importlib.import_module("project-desert-tortoise_amd")
    import bench
    import tip_repair_cases as rc
    result = {"build": pdt.build_tag()}

    def run(name, fs, x):
        y = x.astype(np.float32) / np.float32(32768.0)
        row = {"rate": fs, "samples": len(x), "calls": []}
        with pdt.Demodulator(pdt.MODE_POES, fs, profile=True) as d:
            fr = d.stage_ffp_frames(fs, y)
            row["frames"] = len(fr)
            for _ in range(args.reps):
                t0 = time.perf_counter()
                _, _, sm = d.tip_repair(fr)
                t1 = time.perf_counter()
                row["calls"].append({"call_ms": round(1e3 * (t1 - t0), 3), "k_tip_repair_ms": round(d.kernel_times()["k_tip_repair"][1], 4), "summary": sm})
        result[name] = row
        print(json.dumps({name: row}), flush=True)

    p = bench.capture_params(pdt, "pass", 1, args.pass_seconds)
    n = int(round(args.pass_seconds * 250000))
    run("pass", 250000, bench.make_capture(pdt, p, n, 8, device="cuda:0").cpu().numpy().reshape(-1, 2))
    run("weak_30s_kind3", 50000, rc.weak_capture(pdt, 3, 9.0)[1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
