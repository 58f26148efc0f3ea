"""Reads the lines of tools/where_mask_bench.py and prints the table of profiles/where_mask/NOTES.md: per grid point gather, mask
and plain search side by side with each route's spread between rounds, the route the automatic rule picks, and whether that
pick is accepted -- not slower than the other route by more than twice the larger of the two spreads.

The pick is recomputed from the cost rule as it stands in csrc/fieldpred.cpp (through the stand-alone sanitizer build of that
file, `make wheredepth_asan`), not taken from the library that ran the benchmark, so the table follows a change of the constants.

usage: python tools/where_mask_report.py profiles/where_mask/where_mask_bench.jsonl [where_mask_min_rows] [i8_sample_m]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "semantic_query_engine_amd", "csrc")
MIN_ROWS = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
SAMPLE_M = int(sys.argv[3]) if len(sys.argv) > 3 else 20


def rule(points):
    subprocess.check_call(["make", "-C", CSRC, "wheredepth_asan"], stdout=subprocess.DEVNULL)
    text = "".join(f"{p['k']} {p['selected']} {p['index_rows']} {p['B']} {max(p['rule_depth'], 1)} {1 if p['rule_depth'] <= SAMPLE_M else 0}\n"
                   for p in points)
    out = subprocess.run([os.path.join(CSRC, "build_san", "wheredepth_asan")], input=text, capture_output=True, text=True, check=True)
    return [int(line.split()[1]) for line in out.stdout.splitlines()]


def main():
    recs = [json.loads(line) for line in open(sys.argv[1])]
    grid = [r for r in recs if r["what"] == "grid"]
    cheaper = rule(grid)
    print("| B | k | selected | d | first pass | gather ms (spread) | mask ms (spread) | plain ms | swept | auto | verdict |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    bad = 0
    for p, ch in zip(grid, cheaper):
        g, m = p["gather"], p["mask"]
        auto_mask = bool(ch) and p["rule_depth"] > 0 and p["selected"] >= MIN_ROWS
        last = p["mask_last"] or {}
        verdict = "-"
        if m is not None:
            tol = 2 * max(g["spread_ms"], m["spread_ms"])
            picked, other = (m, g) if auto_mask else (g, m)
            ok = picked["ms"] <= other["ms"] + tol
            verdict = "ok" if ok else f"MISS by {picked['ms'] - other['ms'] - tol:.2f} ms"
            bad += not ok
        print(f"| {p['B']} | {p['k']} | {100 * p['fraction']:g} % | {p['rule_depth'] or 'none'} | "
              f"{'-' if not last else ('int8' if last['first_pass_i8'] else 'bf16')} | {g['ms']:.2f} ({g['spread_ms']:.2f}) | "
              f"{'-' if m is None else '%.2f (%.2f)' % (m['ms'], m['spread_ms'])} | {p['plain']['ms']:.2f} | {last.get('swept', '-')} | "
              f"{'mask' if auto_mask else 'gather'} | {verdict} |")
    print(f"\n{bad} of {sum(p['mask'] is not None for p in grid)} measured points miss the acceptance rule")
    for p in (r for r in recs if r["what"] == "correlated"):
        print(f"correlated, B = {p['B']}, k = {p['k']}: {p['flagged_queries']} queries lose their 256 nearest rows ({p['refused_rows']} rows refused); "
              f"mask {p['mask']['ms']:.2f} ms (spread {p['mask']['spread_ms']:.2f}), swept {p['mask_last']['swept']}, depth {p['mask_last']['depth']}; "
              f"gather {p['gather']['ms']:.2f} ms (spread {p['gather']['spread_ms']:.2f}); bit-equal {p['bit_equal']}")


if __name__ == "__main__":
    main()
