"""How many minor frames of weak POES captures the flywheel synchroniser places beside the reference's own, without a GPU.

Synthetic POES captures of --seconds at 50 ksps, the noise multiplied as `bench.py --config weak` multiplies it, at every (noise, seed)
of --noise x --seeds.  The oracle's chain gives the Manchester bits and rule 0's frames (the reference's ByteSyncOnSyncword, complete
frames only); pdt_host_tip_sync gives the flywheel's at its defaults and at the other triples (E, W, G) of --triples.  A frame is PLACED
when its bytes 2 .. 103 differ from those of some transmitted frame in at most 100 of 816 bits (a wrong alignment differs in about
408 +- 14), otherwise UNPLACED; the oracle's restatement of checkParity.m counts the good parity chunks of each frame list.  One JSON:
a row per capture and the sums per noise level.

    python tools/tip_sync_survey.py --out profiles/r21/survey.json
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def triple(text: str):
    e, w, g = (int(v) for v in text.split(","))
    return e, w, g


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--noise", type=float, nargs="+", default=(6.0, 9.0, 10.5, 12.0))
    ap.add_argument("--seeds", type=int, nargs="+", default=(1234, 77, 5, 2024))
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--triples", type=triple, nargs="+", default=((2, 2, 3), (1, 2, 3), (2, 2, 2), (2, 3, 3), (3, 2, 3)))
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    pdt = importlib.import_module("project-desert-tortoise_amd")
    from oracle import binding as orc
    import test_tip_sync as cpu

    def tally(p, frames_bytes, times):
        ok, lost = cpu.placed(pdt, p, frames_bytes, nsent=int(args.seconds * 10) + 40)
        summary, _ = orc.tip_check([(t, b, 1) for t, b in zip(times, frames_bytes)])
        return {"frames": len(frames_bytes), "placed": ok, "unplaced": lost, "good_chunks": summary["good_chunks"], "good_frames": summary["good_frames"]}

    names = ["rule0"] + ["%d,%d,%d" % t for t in args.triples]
    rows, sums = [], {}
    for mult in args.noise:
        total = {name: {"frames": 0, "placed": 0, "unplaced": 0, "good_chunks": 0, "good_frames": 0} for name in names}
        for seed in args.seeds:
            p, x = cpu.weak_capture(pdt, mult, seed, args.seconds)
            o = orc.Oracle(orc.POES, 50000, x)
            bits = o.stage(orc.ST_BITS)
            own = [f for f in o.frames() if f.complete and f.nbytes == 104]
            row = {"noise_x": mult, "seed": seed, "bits": len(bits), "rule0": tally(p, [bytes(f.bytes) for f in own], [f.time for f in own])}
            for t in args.triples:
                fr, info = pdt.host_tip_sync(bits, *t, with_info=True)
                row["%d,%d,%d" % t] = dict(tally(p, [bytes(v) for v in fr["bytes"]], [float(v) for v in fr["time"]]),
                                           flywheel_heads=int((info["candidate"] == 0).sum()), inverted=int(fr["inverted"].sum()))
            for name in names:
                for k in total[name]:
                    total[name][k] += row[name][k]
            rows.append(row)
            print(json.dumps(row), flush=True)
        sums["%g" % mult] = total
    result = {"sample_rate": 50000, "seconds": args.seconds, "defaults": "2,2,3", "captures": rows, "per_noise": sums}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(sums))


if __name__ == "__main__":
    main()
