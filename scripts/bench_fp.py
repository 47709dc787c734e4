#!/usr/bin/env python3
"""Changed rows after a policy edit from kept fingerprints (8 bytes per row) against the kept matrix
(R bytes per row), at the C3 shape (1.25M rows x 204 rules, `exclude` blocks added to three policies)
and the C2 shape (1M rows x 3 rules, the level edited): the edits of scripts/bench_delta.py. One
process; per round and per leg program A is evaluated (untimed), its result kept (timed), program B
evaluated (untimed), and the changed rows asked for (timed):

  (a) matrix: Engine.keep_results, then Engine.changed_rows with the verdict rows, the exact form;
  (b) fp:     Engine.keep_fingerprints, then Engine.changed_rows_fp with the verdict rows and the
              new fingerprints.

Wall times are host clocks around calls followed by a device synchronise: `--warmup` untimed rounds,
then the median and the spread (min, max) of `--reps` rounds, (a) and (b) alternating. Both legs'
rows and verdict rows are compared once. Prints one JSON line per shape.

Kernel durations come from a run of their own under the profiler, which slows the host:

  rocprofv3 --kernel-trace --stats -d DIR -o fp --output-format csv -- \\
      python3 scripts/bench_fp.py --config c3 --fp-only
  python3 scripts/bench_fp.py --config c3 --kernel-stats DIR --changed K [--fail-cells F]

The second command reads the profiler's kernel statistics and prints each kernel's mean duration and
its algorithmic bytes over that time as a fraction of the 8 TB/s HBM peak: the matrix once, 4 bytes
per FAIL cell with --masks and 8 bytes per row out for the fingerprint kernel; 8 + 8 + 1 bytes per
row for the compare; the flag bytes per selection pass; per changed row its index and its row read
and written for the row gather, its index and its fingerprint read and written for the other."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import kyverno_amd as K  # noqa: E402
from bench_delta import HBM_PEAK, shape  # noqa: E402


def alg_bytes(n, R, changed, fail_cells):
    tiles = (n + 4095) // 4096
    return {"kpe_row_fp_kernel": n * R + 4 * fail_cells + 8 * n, "kpe_fp_diff_kernel": 17 * n,
            "kpe_select_count_kernel": n + 4 * tiles, "kpe_select_scan_kernel": 4 * tiles + 8 * (tiles + 1),
            "kpe_select_scatter_kernel": n + 16 * tiles + 8 * changed, "kpe_gather_rows_kernel": changed * (8 + 2 * R),
            "kpe_fp_gather_kernel": changed * 24}


def kernel_stats(directory, n, R, changed, fail_cells):
    want = alg_bytes(n, R, changed, fail_cells)
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for rec in csv.DictReader(open(path)):
            for k in want:
                if k in rec["Name"]:
                    c, tot = rows.get(k, (0, 0.0))
                    rows[k] = (c + int(rec["Calls"]), tot + float(rec["TotalDurationNs"]))
    if not rows:
        raise SystemExit(f"no kernel statistics of the fingerprint kernels under {directory}")
    out = {}
    for k, b in want.items():
        if k in rows:
            calls, tot = rows[k]
            us = tot / calls / 1e3
            out[k] = {"calls": calls, "mean_us": round(us, 2), "alg_bytes": b,
                      "fraction_of_hbm_peak": round(b / (us * 1e-6) / HBM_PEAK, 4)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=("c3", "c2"), default="c3")
    ap.add_argument("--rows", type=int, default=0, help="rows instead of the shape's (a rehearsal)")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--masks", action="store_true", help="evaluate with check masks; FAIL cells' mask words count")
    ap.add_argument("--fp-only", action="store_true", help="only leg (b): the run the profiler traces")
    ap.add_argument("--kernel-stats", metavar="DIR", help="summarise a rocprofv3 --kernel-trace --stats run (no GPU)")
    ap.add_argument("--changed", type=int, default=0, help="with --kernel-stats: changed rows of the traced run")
    ap.add_argument("--fail-cells", type=int, default=0, help="with --kernel-stats: FAIL cells of a --masks run")
    args = ap.parse_args()
    pa, pb, mix, seed, n, docs = shape(args.config, args.rows)
    psa, psb = K.PolicySet(pa), K.PolicySet(pb)
    Ro, Rn = psa.num_rules, psb.num_rules
    if args.kernel_stats:
        print(json.dumps({"config": args.config, "rows": n, "rules": [Ro, Rn], "changed": args.changed,
                          "kernels": kernel_stats(args.kernel_stats, n, Rn, args.changed, args.fail_cells)}))
        return
    eng = K.Engine(ordinal=0)  # raises without a gfx950 device: no fallback
    t0 = time.perf_counter()
    corpus = K.Corpus(K.synth_resources(seed, n, mix=mix), docs=docs).upload(eng.device)
    eng.evaluate_async(psb, corpus, masks=args.masks)
    vb, _, _ = eng.fetch(psb, corpus)
    fail_cells = int((vb == 2).sum())
    del vb
    print(f"[bench_fp] {args.config}: {n} x {Rn}, {fail_cells} FAIL cells, set-up {time.perf_counter() - t0:.1f} s",
          file=sys.stderr, flush=True)

    def leg(keep, changed):
        eng.evaluate_async(psa, corpus, masks=args.masks)
        eng.device.sync()
        t = [time.perf_counter()]
        keep()
        eng.device.sync()
        t.append(time.perf_counter())
        eng.evaluate_async(psb, corpus, masks=args.masks)
        eng.device.sync()
        t.append(time.perf_counter())
        res = changed()
        t.append(time.perf_counter())
        return res[:2], (t[1] - t[0], t[3] - t[2])

    legs = {"matrix": lambda: leg(lambda: eng.keep_results(psa, corpus), lambda: eng.changed_rows(psb, corpus)),
            "fp": lambda: leg(lambda: eng.keep_fingerprints(psa, corpus, masks=args.masks),
                              lambda: eng.changed_rows_fp(psb, corpus, masks=args.masks))}
    if args.fp_only:
        del legs["matrix"]
    times = {k: [] for k in legs}
    res = {}
    for it in range(args.warmup + args.reps):
        for k, f in legs.items():  # alternating, so both see the same neighbours
            res[k], dt = f()
            if it >= args.warmup:
                times[k].append(dt)
    if len(res) == 2 and not args.masks:  # with masks the fingerprint sees what the matrix does not
        assert np.array_equal(res["matrix"][0], res["fp"][0]), "changed rows differ"
        assert np.array_equal(res["matrix"][1], res["fp"][1]), "verdict rows differ"
    changed = int(res["fp"][0].size)
    out = {"config": args.config, "rows": n, "rules": [Ro, Rn], "masks": args.masks, "fail_cells": fail_cells,
           "changed": changed, "hbm_kept_bytes": {"matrix": n * Ro, "fp": n * 8}, "reps": args.reps, "warmup": args.warmup}
    for k, ts in times.items():
        tot = [float(sum(x)) * 1e3 for x in ts]
        out[k] = {"wall_ms_median": round(statistics.median(tot), 3), "wall_ms_min": round(min(tot), 3),
                  "wall_ms_max": round(max(tot), 3),
                  "parts_ms_median": {p: round(statistics.median([x[i] for x in ts]) * 1e3, 3)
                                      for i, p in enumerate(("keep", "changed"))}}
    if len(times) == 2:
        out["fp_over_matrix_median"] = round(out["fp"]["wall_ms_median"] / out["matrix"]["wall_ms_median"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
