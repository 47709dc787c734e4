#!/usr/bin/env python3
"""Changed rows after a policy edit: the device comparison against the full-matrix read-back, at the
C3 shape (1.25M rows x 204 rules, `exclude` blocks added to three policies) and the C2 shape (1M
rows x 3 rules, the level edited). One process: program A is evaluated, fetched and kept, program B
is evaluated, then per round:

  (a) full:  kpe_fetch of B's N x R matrix + kpe_changed_rows_host against A's matrix held on the
             host, the path without a kept result;
  (b) delta: Engine.changed_rows with the verdict rows (a count call, then a call of that size)
             against the result Engine.keep_results kept once (timed once, reported apart).

Wall times are host clocks around calls that end in a stream synchronise: `--warmup` untimed
rounds, then the median and the spread (min, max) of `--reps` rounds, (a) and (b) alternating.
Both paths' results are compared once. Prints one JSON line per shape.

Kernel durations come from a run of their own under the profiler, which slows the host:

  rocprofv3 --kernel-trace --stats -d DIR -o delta --output-format csv -- \\
      python3 scripts/bench_delta.py --config c3 --delta-only
  python3 scripts/bench_delta.py --config c3 --kernel-stats DIR --changed K

The second command reads the profiler's kernel statistics and prints each kernel's mean duration
and its algorithmic bytes over that time as a fraction of the 8 TB/s HBM peak: both matrices and
the flag bytes for the flag pass (N x (Rn + Ro) + N), the flag bytes per selection pass, and per
changed row its index and its row read and written for the gather."""
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
SHAPES = {"c3": 1_250_000, "c2": 1_000_000}


def shape(cfg, rows):
    """(policies A, policies B, synth mix, seed, rows, document tapes)"""
    from tests.policies import c3_policy_set, restricted_latest

    if cfg == "c3":
        b = c3_policy_set()
        for i in (7, 90, 150):
            for rule in b[i]["spec"]["rules"]:
                rule["exclude"] = {"any": [{"resources": {"namespaces": ["team-1*"]}}]}
        return c3_policy_set(), b, K.SYNTH_C3, 0xC3, rows or SHAPES[cfg], True
    b = restricted_latest()
    b["spec"]["rules"][0]["validate"]["podSecurity"]["level"] = "baseline"
    return [restricted_latest()], [b], K.SYNTH_PODS, 0xC2, rows or SHAPES[cfg], False  # no pattern rules: no tapes


def alg_bytes(n, Ro, Rn, changed):
    tiles = (n + 4095) // 4096
    return {"kpe_delta_flags_kernel": n * (Rn + Ro) + n, "kpe_select_count_kernel": n + 4 * tiles,
            "kpe_select_scan_kernel": 4 * tiles + 8 * (tiles + 1), "kpe_select_scatter_kernel": n + 16 * tiles + 8 * changed,
            "kpe_gather_rows_kernel": changed * (8 + 2 * Rn)}


def kernel_stats(directory, n, Ro, Rn, changed):
    want = alg_bytes(n, Ro, Rn, changed)
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for rec in csv.DictReader(open(path)):
            for k in want:
                if k in rec["Name"]:
                    c, tot = rows.get(k, (0, 0.0))
                    rows[k] = (c + int(rec["Calls"]), tot + float(rec["TotalDurationNs"]))
    if not rows:
        raise SystemExit(f"no kernel statistics of the delta kernels under {directory}")
    out = {}
    for k, b in want.items():
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
    ap.add_argument("--delta-only", action="store_true", help="only path (b): the run the profiler traces")
    ap.add_argument("--kernel-stats", metavar="DIR", help="summarise a rocprofv3 --kernel-trace --stats run (no GPU)")
    ap.add_argument("--changed", type=int, default=0, help="with --kernel-stats: changed rows of the traced run")
    args = ap.parse_args()
    pa, pb, mix, seed, n, docs = shape(args.config, args.rows)
    psa, psb = K.PolicySet(pa), K.PolicySet(pb)
    Ro, Rn = psa.num_rules, psb.num_rules
    if args.kernel_stats:
        print(json.dumps({"config": args.config, "rows": n, "rules": [Ro, Rn], "changed": args.changed,
                          "kernels": kernel_stats(args.kernel_stats, n, Ro, Rn, args.changed)}))
        return
    eng = K.Engine(ordinal=0)  # raises without a gfx950 device: no fallback
    L = load()
    t0 = time.perf_counter()
    corpus = K.Corpus(K.synth_resources(seed, n, mix=mix), docs=docs).upload(eng.device)
    eng.evaluate_async(psa, corpus)
    va, _, _ = eng.fetch(psa, corpus)
    t1 = time.perf_counter()
    eng.keep_results(psa, corpus)
    eng.device.sync()
    keep_ms = (time.perf_counter() - t1) * 1e3
    eng.evaluate_async(psb, corpus)
    eng.device.sync()
    print(f"[bench_delta] {args.config}: {n} x {Ro} kept ({keep_ms:.3f} ms), {n} x {Rn} evaluated, "
          f"set-up {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    cmap = K.column_map(psa.rule_names, psb.rule_names)
    vb = np.zeros((n, Rn), dtype=np.uint8)
    rows_a = np.zeros(n, dtype=np.uint64)
    vr_a = np.zeros((n, Rn), dtype=np.uint8)

    def full():
        t = [time.perf_counter()]
        check(L.kpe_fetch(eng.device.h, psb.h, corpus.h, vb.ctypes.data, None, None))
        t.append(time.perf_counter())
        total = L.kpe_changed_rows_host(va.ctypes.data, vb.ctypes.data, n, Ro, Rn, cmap.ctypes.data, None,
                                        rows_a.ctypes.data, vr_a.ctypes.data, n)
        t.append(time.perf_counter())
        return (rows_a[:total].copy(), vr_a[:total].copy()), np.diff(t)

    def delta():
        t = [time.perf_counter()]
        rows, vr, _ = eng.changed_rows(psb, corpus)
        t.append(time.perf_counter())
        return (rows, vr), np.diff(t)

    paths = {"delta": delta} if args.delta_only else {"full": full, "delta": delta}
    times = {k: [] for k in paths}
    res = {}
    for it in range(args.warmup + args.reps):
        for k, f in paths.items():  # alternating, so both see the same neighbours
            res[k], dt = f()
            if it >= args.warmup:
                times[k].append(dt)
    if len(res) == 2:
        assert np.array_equal(res["full"][0], res["delta"][0]), "changed rows differ"
        assert np.array_equal(res["full"][1], res["delta"][1]), "verdict rows differ"
    changed = int(res["delta"][0].size)
    out = {"config": args.config, "rows": n, "rules": [Ro, Rn], "matrix_bytes": n * Rn, "kept_bytes": n * Ro,
           "changed": changed, "delta_bytes_d2h": changed * (8 + Rn) + 16, "keep_results_ms": round(keep_ms, 3),
           "reps": args.reps, "warmup": args.warmup}
    parts = {"full": ("fetch", "changed_rows_host"), "delta": ("changed_rows",)}
    for k, ts in times.items():
        tot = [float(sum(x)) * 1e3 for x in ts]
        out[k] = {"wall_ms_median": round(statistics.median(tot), 3), "wall_ms_min": round(min(tot), 3),
                  "wall_ms_max": round(max(tot), 3),
                  "parts_ms_median": {p: round(statistics.median([x[i] for x in ts]) * 1e3, 3)
                                      for i, p in enumerate(parts[k])}}
    if len(times) == 2:
        out["speedup_median"] = round(out["full"]["wall_ms_median"] / out["delta"]["wall_ms_median"], 2)
        out["delta_below_full_by_more_than_spread"] = bool(
            out["full"]["wall_ms_min"] - out["delta"]["wall_ms_max"] > 0 and
            out["full"]["wall_ms_median"] - out["delta"]["wall_ms_median"] >
            out["full"]["wall_ms_max"] - out["full"]["wall_ms_min"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
