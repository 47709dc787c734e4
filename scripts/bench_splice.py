#!/usr/bin/env python3
"""One policy edited out of the set: the full re-evaluation against the splice, at the C3 shape
(1.25M rows x 204 rules, an `exclude` block added to policy 90) and the C2 shape (1M rows x 3 rules,
the one policy's level edited, so the "partial" evaluation is the whole set). One process: program
A is evaluated and kept, then per round, both paths starting from A kept and A bound:

  (a) full:   evaluate_async(B) + changed_rows(B, always = MESSAGE_CODES on the edited policy) +
              keep_results(B), the path of ResidentScanner.apply;
  (b) splice: evaluate_async(sub) + splice_results(sub) + spliced_rows, the path of
              ResidentScanner.apply_edit (sub: the edited policy compiled alone).

Wall times are host clocks around each path, which ends in a stream synchronise: `--warmup`
untimed rounds, then the median and the spread (min, max) of `--reps` rounds, (a) and (b)
alternating; A is evaluated and kept again, untimed, before each path. The two paths' rows and
verdict rows are compared every round. Both paths start with a rebind (the corpus was bound to A);
what that costs inside (b) is measured apart: evaluate_async(sub) + sync right after A, and once
more with sub already bound. Prints one JSON line.

Kernel durations come from a run of their own under the profiler, which slows the host:

  rocprofv3 --kernel-trace --stats -d DIR -o splice --output-format csv -- \\
      python3 scripts/bench_splice.py --config c3 --splice-only
  python3 scripts/bench_splice.py --config c3 --kernel-stats DIR

The second command reads the profiler's kernel statistics and prints the splice kernel's mean
duration and its algorithmic bytes, N x (Ro + Rs + rn + 1), over that time as a fraction of the
8 TB/s HBM peak."""
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

HBM_PEAK = 8.0e12
SHAPES = {"c3": 1_250_000, "c2": 1_000_000}


def shape(cfg, rows):
    """(policies A, policies B, the edited policies, synth mix, seed, rows, document tapes)"""
    from tests.policies import c3_policy_set, restricted_latest

    if cfg == "c3":
        b = c3_policy_set()
        for rule in b[90]["spec"]["rules"]:
            rule["exclude"] = {"any": [{"resources": {"namespaces": ["team-1*"]}}]}
        return c3_policy_set(), b, [b[90]], K.SYNTH_C3, 0xC3, rows or SHAPES[cfg], True
    b = restricted_latest()
    b["spec"]["rules"][0]["validate"]["podSecurity"]["level"] = "baseline"
    return [restricted_latest()], [b], [b], K.SYNTH_PODS, 0xC2, rows or SHAPES[cfg], False


def kernel_stats(directory, alg):
    calls, tot = 0, 0.0
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for rec in csv.DictReader(open(path)):
            if "kpe_splice_kernel" in rec["Name"]:
                calls, tot = calls + int(rec["Calls"]), tot + float(rec["TotalDurationNs"])
    if not calls:
        raise SystemExit(f"no kernel statistics of kpe_splice_kernel under {directory}")
    us = tot / calls / 1e3
    return {"kpe_splice_kernel": {"calls": calls, "mean_us": round(us, 2), "alg_bytes": alg,
                                  "alg_bytes_per_s": alg / (us * 1e-6),
                                  "fraction_of_hbm_peak": round(alg / (us * 1e-6) / HBM_PEAK, 4)}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=("c3", "c2"), default="c3")
    ap.add_argument("--rows", type=int, default=0, help="rows instead of the shape's (a rehearsal)")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--splice-only", action="store_true", help="only path (b): the run the profiler traces")
    ap.add_argument("--kernel-stats", metavar="DIR", help="summarise a rocprofv3 --kernel-trace --stats run (no GPU)")
    args = ap.parse_args()
    pa, pb, ped, mix, seed, n, docs = shape(args.config, args.rows)
    psa, psb, sub = K.PolicySet(pa), K.PolicySet(pb), K.PolicySet(ped)
    Ro, Rs, rn = psa.num_rules, sub.num_rules, psb.num_rules
    if args.kernel_stats:
        print(json.dumps({"config": args.config, "rows": n, "rules": [Ro, Rs, rn],
                          "kernels": kernel_stats(args.kernel_stats, K.splice_bytes(n, Ro, Rs, rn))}))
        return
    eng = K.Engine(ordinal=0)  # raises without a gfx950 device: no fallback
    t0 = time.perf_counter()
    corpus = K.Corpus(K.synth_resources(seed, n, mix=mix), docs=docs).upload(eng.device)
    edited = {p["metadata"]["name"] for p in ped}
    always_b = np.array([K.MESSAGE_CODES if nm.split("/", 1)[0] in edited else 0 for nm in psb.rule_names], dtype=np.uint8)

    def reset():  # A bound and kept
        eng.evaluate_async(psa, corpus)
        eng.keep_results(psa, corpus)
        eng.device.sync()

    reset()
    print(f"[bench_splice] {args.config}: {n} x {Ro} kept, sub {Rs} rules, new {rn} rules, "
          f"set-up {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)

    def full():
        t = [time.perf_counter()]
        eng.evaluate_async(psb, corpus)
        t.append(time.perf_counter())
        rows, vr, _ = eng.changed_rows(psb, corpus, always=always_b)
        t.append(time.perf_counter())
        eng.keep_results(psb, corpus)
        eng.device.sync()
        t.append(time.perf_counter())
        return (rows, vr), np.diff(t)

    def splice():
        t = [time.perf_counter()]
        eng.evaluate_async(sub, corpus)
        t.append(time.perf_counter())
        total = eng.splice_results(sub, corpus, always=K.MESSAGE_CODES)
        t.append(time.perf_counter())
        rows, vr, _ = eng.spliced_rows(corpus, cap=total)
        eng.device.sync()
        t.append(time.perf_counter())
        return (rows, vr), np.diff(t)

    def timed_eval():
        t = time.perf_counter()
        eng.evaluate_async(sub, corpus)
        eng.device.sync()
        return (time.perf_counter() - t) * 1e3

    paths = {"splice": splice} if args.splice_only else {"full": full, "splice": splice}
    times = {k: [] for k in paths}
    rebind, bound = [], []
    res = {}
    for it in range(args.warmup + args.reps):
        for k, f in paths.items():  # alternating, so both see the same neighbours
            reset()
            res[k], dt = f()
            if it >= args.warmup:
                times[k].append(dt)
        if len(res) == 2:
            assert np.array_equal(res["full"][0], res["splice"][0]), "changed rows differ"
            assert np.array_equal(res["full"][1], res["splice"][1]), "verdict rows differ"
        reset()
        a, b = timed_eval(), timed_eval()
        if it >= args.warmup:
            rebind.append(a)
            bound.append(b)
    changed = int(res["splice"][0].size)
    out = {"config": args.config, "rows": n, "rules": [Ro, Rs, rn], "changed": changed,
           "splice_alg_bytes": K.splice_bytes(n, Ro, Rs, rn), "reps": args.reps, "warmup": args.warmup,
           "eval_sub_after_full_ms_median": round(statistics.median(rebind), 3),
           "eval_sub_bound_ms_median": round(statistics.median(bound), 3),
           "rebind_ms_median": round(statistics.median([x - y for x, y in zip(rebind, bound)]), 3)}
    parts = {"full": ("evaluate_async", "changed_rows", "keep_results+sync"),
             "splice": ("evaluate_async", "splice_results", "spliced_rows+sync")}
    for k, ts in times.items():
        tot = [float(sum(x)) * 1e3 for x in ts]
        out[k] = {"wall_ms_median": round(statistics.median(tot), 3), "wall_ms_min": round(min(tot), 3),
                  "wall_ms_max": round(max(tot), 3),
                  "parts_ms_median": {p: round(statistics.median([x[i] for x in ts]) * 1e3, 3)
                                      for i, p in enumerate(parts[k])}}
    if len(times) == 2:
        out["speedup_median"] = round(out["full"]["wall_ms_median"] / out["splice"]["wall_ms_median"], 2)
        out["splice_below_full_by_more_than_spread"] = bool(
            out["full"]["wall_ms_min"] - out["splice"]["wall_ms_max"] > 0 and
            out["full"]["wall_ms_median"] - out["splice"]["wall_ms_median"] >
            out["full"]["wall_ms_max"] - out["full"]["wall_ms_min"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
