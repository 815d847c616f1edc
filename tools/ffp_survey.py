"""How many minor frames of weak POES captures the flywheel places on feed-forward bits beside the oracle's, without a GPU.

Synthetic POES captures of --seconds, the noise multiplied as `bench.py --config weak` multiplies it, at every (noise, seed) of --noise x
--seeds -- tools/tip_sync_survey.py's captures.  At 50 ksps the oracle's chain gives the loop's Manchester bits; pdt_host_ffp_bits gives
the feed-forward ones (samples / 32768, the residual measured) at its defaults and at every variant of --grid, one constant moved at a
time.  Both bit streams go through pdt_host_tip_sync under rule 0's nearest relative, the strictest triple 0,1,2, and under the
flywheel's defaults 2,2,3.  A frame is PLACED when its bytes 2 .. 103 differ from those of some transmitted frame in at most 100 of 816
bits, otherwise UNPLACED.  At --more-rates (100 and 250 ksps) only the feed-forward columns exist: the oracle's 30 s run there is the
cell left out.  One JSON: a row per capture and the sums per rate and noise level.

    python tools/ffp_survey.py --out profiles/r22/ffp_survey.json
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

TRIPLES = {"strict": (0, 1, 2), "default": (2, 2, 3)}
GRID = {"W8": dict(ref_bits=8), "W32": dict(ref_bits=32), "W0": dict(ref_bits=0), "J2": dict(smooth_blocks=2), "J8": dict(smooth_blocks=8),
        "T16": dict(clock_steps=16), "T64": dict(clock_steps=64), "B104": dict(block_bits=104), "B416": dict(block_bits=416)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--noise", type=float, nargs="+", default=(6.0, 9.0, 10.5, 12.0))
    ap.add_argument("--seeds", type=int, nargs="+", default=(1234, 77, 5, 2024))
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--more-rates", type=int, nargs="*", default=(100000, 250000))
    ap.add_argument("--grid-noise", type=float, nargs="*", default=(9.0, 12.0), help="the noise levels the grid of constants is walked at (50 ksps)")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    pdt = importlib.import_module("project-desert-tortoise_amd")
    from oracle import binding as orc
    import test_tip_sync as cpu

    def tally(p, bits):
        out = {}
        for name, t in TRIPLES.items():
            fr = pdt.host_tip_sync(bits, *t)
            ok, lost = cpu.placed(pdt, p, [bytes(v) for v in fr["bytes"]], nsent=int(args.seconds * 10) + 40)
            out[name] = {"frames": len(fr), "placed": ok, "unplaced": lost}
        return out

    rows, sums = [], {}

    def add(key, row):
        for col, cell in row.items():
            if not isinstance(cell, dict) or "default" not in cell:
                continue
            for name in TRIPLES:
                tot = sums.setdefault(key, {}).setdefault(col, {}).setdefault(name, {"frames": 0, "placed": 0, "unplaced": 0})
                for k in tot:
                    tot[k] += cell[name][k]

    for fs in (50000,) + tuple(args.more_rates):
        for mult in args.noise:
            for seed in args.seeds:
                p, x = cpu.weak_capture(pdt, mult, seed, args.seconds, fs)
                y = x.astype(np.float32) / np.float32(32768.0)
                row = {"rate": fs, "noise_x": mult, "seed": seed}
                if fs == 50000:
                    bits = orc.Oracle(orc.POES, fs, x).stage(orc.ST_BITS)
                    row["loop"] = tally(p, bits)
                    row["loop_bits"] = len(bits)
                t0 = time.perf_counter()
                got = pdt.host_ffp_bits(fs, y)
                row["host_s"] = round(time.perf_counter() - t0, 2)
                row["ffp"] = tally(p, got.bits.tobytes())
                row["ffp_bits"] = len(got.bits)
                row["segs_valid"] = [int(got.sync["segs_valid"]), int(got.sync["segs"])]
                if fs == 50000 and mult in args.grid_noise:
                    for name, cfg in GRID.items():
                        row[name] = tally(p, pdt.host_ffp_bits(fs, y, **cfg).bits.tobytes())
                add("%d:%g" % (fs, mult), row)
                rows.append(row)
                print(json.dumps(row), flush=True)
    result = {"seconds": args.seconds, "triples": TRIPLES, "grid": GRID, "left_out": "the oracle's bits at 100 and 250 ksps", "captures": rows,
              "per_rate_and_noise": sums}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(sums))


if __name__ == "__main__":
    main()
