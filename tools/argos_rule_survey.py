"""How many per-burst windows of a wideband capture yield their ARGOS message under each rule, without a GPU.

Two kind-2 platforms at seeds (a, a + 4) share a capture of --seconds at 1.024 Msps, as tests/test_argos_best.py builds them.  The host
pipeline -- pdt_host_bursts, pdt_burst_windows, pdt_host_ddc of each window's slice, the oracle's chain -- gives a bit string per window,
and pdt_host_argos_messages decodes it under PDT_ARGOS_RULE_FIRST and PDT_ARGOS_RULE_BEST.  Beside the loop's bits, the feed-forward bits
of the same slices (pdt_host_ff_bits at its defaults) under the same two rules: the columns ff_first and ff_best.  A window is RIGHT when its complete messages
are exactly the one sent for its burst, WRONG when it holds a complete message other than that one (a window can be neither: nothing
decoded).  One JSON: per pair the windows, the right and the wrong windows of each rule and the first frames of the windows each rule
does not get right; and the totals.

    python tools/argos_rule_survey.py --first 100 --last 139 --seconds 15 --out profiles/r18/survey_15s.json
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--first", type=int, required=True, help="the first pair's a: seeds (a, a + 4)")
    ap.add_argument("--last", type=int, required=True, help="the last pair's a")
    ap.add_argument("--seconds", type=float, required=True)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    pdt = importlib.import_module("project-desert-tortoise_amd")
    from oracle import binding as orc
    import argos_best_cases as bc
    rules = (("first", pdt.ARGOS_RULE_FIRST), ("best", pdt.ARGOS_RULE_BEST))
    columns = [name for name, _ in rules] + ["ff_" + name for name, _ in rules]
    pairs = []
    total = {"windows": 0, **{name: {"right": 0, "wrong": 0} for name in columns}}
    for a in range(args.first, args.last + 1):
        x, params = bc.kind2_pair(pdt, (a, a + 4), args.seconds)
        win, bits = bc.host_window_bits(pdt, orc, x)
        row = {"seeds": [a, a + 4], "windows": len(win)}
        total["windows"] += len(win)
        ff = [pdt.host_ff_bits(bc.FS, pdt.host_ddc(bc.IN_RATE, bc.D, w.offset_hz, x[w.first_frame: w.first_frame + w.nframes])).bits.tobytes() for w in win]
        for source, strings in (("", bits), ("ff_", ff)):
            for name, rule in rules:
                right, wrong, lost = bc.tally(pdt, params, win, [pdt.host_argos_messages(b, rule=rule) for b in strings])
                row[source + name] = {"right": right, "wrong": wrong, "not_right_at_frame": lost}
                total[source + name]["right"] += right
                total[source + name]["wrong"] += wrong
        pairs.append(row)
        print(json.dumps(row), flush=True)
    result = {"in_rate": bc.IN_RATE, "decimation": bc.D, "seconds": args.seconds, "min_run": 6, "pairs": pairs, "total": total}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(total))


if __name__ == "__main__":
    main()
