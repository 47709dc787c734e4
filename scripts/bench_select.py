#!/usr/bin/env python3
"""Sparse result fetch against the full-matrix read-back, at the C3 shape (1.25M rows x 204
rules) and the C2 shape (1M rows x 3 rules). One process, one evaluation, then per shape:

  (a) full:   kpe_fetch of the N x R matrix + the host selection (np.flatnonzero of the FAIL /
              ERROR cells) + the host summaries (kpe_row_summaries_host), the path without the
              device-side queries;
  (b) sparse: Engine.select_cells(KPE_SEL(FAIL) | KPE_SEL(ERROR)) (a count call, then a call of
              that size) + Engine.row_summaries over all rows.

Wall times are host clocks around calls that end in a stream synchronise: `--warmup` untimed
rounds, then the median and the spread (min, max) of `--reps` rounds, (a) and (b) alternating.
Both paths' results are compared once. Prints one JSON line per shape.

Kernel durations come from a run of their own under the profiler, which slows the host:

  rocprofv3 --kernel-trace --stats -d DIR -o sel --output-format csv -- \\
      python3 scripts/bench_select.py --config c3 --sparse-only
  python3 scripts/bench_select.py --config c3 --kernel-stats DIR

The second command reads the profiler's kernel statistics and prints each new kernel's mean
duration and its algorithmic bytes over that time as a fraction of the 8 TB/s HBM peak: the
matrix once per pass that reads it whole (count, summary), the tile counts and offsets for the
scan, and for the scatter pass the matrix once plus 9 bytes per selected cell (an upper bound:
tiles without a selected cell are skipped)."""
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

import numpy as np  # noqa: E402

import kyverno_amd as K  # noqa: E402
from kyverno_amd._lib import check, load  # noqa: E402

HBM_PEAK = 8.0e12
FAIL, ERROR = 2, 4
SHAPES = {"c3": (1_250_000, 204), "c2": (1_000_000, 3)}


def shape(cfg, rows):
    from tests.policies import c3_policy_set, restricted_latest

    if cfg == "c3":
        return c3_policy_set(), K.SYNTH_C3, 0xC3, rows or SHAPES[cfg][0], True
    return [restricted_latest()], K.SYNTH_PODS, 0xC2, rows or SHAPES[cfg][0], False  # no pattern rules: no tapes


def alg_bytes(n, R, selected):
    cells = n * R
    tiles = (cells + 4095) // 4096
    return {"kpe_select_count_kernel": cells + 4 * tiles, "kpe_select_scan_kernel": 4 * tiles + 8 * (tiles + 1),
            "kpe_select_scatter_kernel": cells + 16 * tiles + 9 * selected, "kpe_row_summary_kernel": cells + 12 * n}


def kernel_stats(directory, n, R, selected):
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for rec in csv.DictReader(open(path)):
            for k in alg_bytes(n, R, selected):
                if k in rec["Name"]:
                    c, tot = rows.get(k, (0, 0.0))
                    rows[k] = (c + int(rec["Calls"]), tot + float(rec["TotalDurationNs"]))
    if not rows:
        raise SystemExit(f"no kernel statistics of the selection kernels under {directory}")
    out = {}
    for k, b in alg_bytes(n, R, selected).items():
        if k in rows:
            calls, tot = rows[k]
            us = tot / calls / 1e3
            out[k] = {"calls": calls, "mean_us": round(us, 2), "alg_bytes": b,
                      "alg_bytes_per_s": b / (us * 1e-6), "fraction_of_hbm_peak": round(b / (us * 1e-6) / HBM_PEAK, 4)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=("c3", "c2"), default="c3")
    ap.add_argument("--rows", type=int, default=0, help="rows instead of the shape's (a rehearsal)")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sparse-only", action="store_true", help="only path (b): the run the profiler traces")
    ap.add_argument("--kernel-stats", metavar="DIR", help="summarise a rocprofv3 --kernel-trace --stats run (no GPU)")
    ap.add_argument("--selected", type=int, default=-1, help="with --kernel-stats: selected cells of the traced run")
    args = ap.parse_args()
    policies, mix, seed, n, docs = shape(args.config, args.rows)
    ps = K.PolicySet(policies)
    R = ps.num_rules
    if args.kernel_stats:
        print(json.dumps({"config": args.config, "rows": n, "rules": R, "selected": max(args.selected, 0),
                          "kernels": kernel_stats(args.kernel_stats, n, R, max(args.selected, 0))}))
        return
    eng = K.Engine(ordinal=0)  # raises without a gfx950 device: no fallback
    t0 = time.perf_counter()
    corpus = K.Corpus(K.synth_resources(seed, n, mix=mix), docs=docs).upload(eng.device)
    eng.evaluate_async(ps, corpus)
    eng.device.sync()
    print(f"[bench_select] {args.config}: {n} x {R} evaluated, set-up {time.perf_counter() - t0:.1f} s",
          file=sys.stderr, flush=True)
    L = load()
    sel = K.SEL(FAIL) | K.SEL(ERROR)
    v = np.zeros((n, R), dtype=np.uint8)

    def full():
        t = [time.perf_counter()]
        check(L.kpe_fetch(eng.device.h, ps.h, corpus.h, v.ctypes.data, None, None))
        t.append(time.perf_counter())
        cells = np.flatnonzero((v == FAIL) | (v == ERROR))
        t.append(time.perf_counter())
        summ = K.row_summaries(ps, v)
        t.append(time.perf_counter())
        return (cells, summ), np.diff(t)

    def sparse():
        t = [time.perf_counter()]
        cells, _, total = eng.select_cells(ps, corpus, sel, with_verdicts=False)
        t.append(time.perf_counter())
        summ = eng.row_summaries(ps, corpus)
        t.append(time.perf_counter())
        return (cells, summ), np.diff(t)

    paths = {"sparse": sparse} if args.sparse_only else {"full": full, "sparse": sparse}
    times = {k: [] for k in paths}
    res = {}
    for it in range(args.warmup + args.reps):
        for k, f in paths.items():  # alternating, so both see the same neighbours
            res[k], dt = f()
            if it >= args.warmup:
                times[k].append(dt)
    if len(res) == 2:
        assert np.array_equal(res["full"][0].astype(np.uint64), res["sparse"][0]), "selected cells differ"
        assert np.array_equal(res["full"][1], res["sparse"][1]), "row summaries differ"
    out = {"config": args.config, "rows": n, "rules": R, "matrix_bytes": n * R, "selected": int(res["sparse"][0].size),
           "sparse_bytes_d2h": int(res["sparse"][0].size) * 8 + n * 12, "reps": args.reps, "warmup": args.warmup}
    parts = {"full": ("fetch", "select", "summaries"), "sparse": ("select_cells", "row_summaries")}
    for k, ts in times.items():
        tot = [float(sum(x)) * 1e3 for x in ts]
        out[k] = {"wall_ms_median": round(statistics.median(tot), 3), "wall_ms_min": round(min(tot), 3),
                  "wall_ms_max": round(max(tot), 3),
                  "parts_ms_median": {p: round(statistics.median([x[i] for x in ts]) * 1e3, 3)
                                      for i, p in enumerate(parts[k])}}
    if len(times) == 2:
        out["speedup_median"] = round(out["full"]["wall_ms_median"] / out["sparse"]["wall_ms_median"], 2)
        out["sparse_below_full_by_more_than_spread"] = bool(
            out["full"]["wall_ms_min"] - out["sparse"]["wall_ms_max"] > 0 and
            out["full"]["wall_ms_median"] - out["sparse"]["wall_ms_median"] >
            out["full"]["wall_ms_max"] - out["full"]["wall_ms_min"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
