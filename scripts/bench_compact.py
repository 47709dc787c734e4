#!/usr/bin/env python3
"""Compaction of a churned resident corpus: flattening the live NDJSON lines again against gathering
the rows of the segments, at the C2 shape (Pods, restricted:latest, no document tapes) and the C5 mix
(fan-out pods and deployments, the pattern policies, with tapes). The corpus is cut into eight
segments (the first holds 65 % of the rows, seven delta segments 5 % each), 20 % of the physical rows
are retired at random, and the live rows are listed in a logical order in which half of each delta
segment's rows replace rows of the first segment and the other half are appended. One process; the
policy set is evaluated and kept on every segment, then per round

  (a) reflatten: join the live lines, flatten, upload, evaluate, keep_results, sync: what
      ResidentScanner.compact(reflatten=True) does;
  (b) gather:    Corpus.gather, upload, Engine.gather_results (which waits): what compact() does.

Wall times are host clocks around each leg; `--warmup` untimed rounds, then the median and the
spread (min, max) of `--reps` rounds, (a) and (b) alternating, under the same flatten thread count
(KPE_FLATTEN_THREADS, 16 by default). The host parts (join + flatten against gather: no device call
in either) are reported apart. Every round the gathered matrix is compared with the re-evaluated one.

`--apply`: what an `apply` costs over 1, 4 and 16 segments of the same rows (evaluate_batch_async,
then changed_rows and keep_results per segment, as ResidentScanner._apply_segments), for the next
change to max_segments. Prints one JSON line.

Kernel durations come from a run of their own under the profiler, which slows the host:

  rocprofv3 --kernel-trace --stats -d DIR -o compact --output-format csv -- \\
      python3 scripts/bench_compact.py --config c2 --gather-only
  python3 scripts/bench_compact.py --config c2 --kernel-stats DIR"""
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
from kyverno_amd.scan import ndjson_rows  # noqa: E402

HBM_PEAK = 8.0e12
KERNELS = ("kpe_results_gather_kernel", "kpe_fp_gather_pairs_kernel")


def shape(cfg):
    """(policies, synth mix, seed, document tapes)"""
    from tests.policies import c5_policy_set, restricted_latest

    if cfg == "c5":
        return c5_policy_set(), K.SYNTH_FANOUT, 0xC5, True
    return [restricted_latest()], K.SYNTH_PODS, 0xC2, False


def kernel_stats(directory, alg):
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for rec in csv.DictReader(open(path)):
            for k in KERNELS:
                if k in rec["Name"]:
                    calls, tot = int(rec["Calls"]), float(rec["TotalDurationNs"])
                    us = tot / calls / 1e3
                    out[k] = {"calls": calls, "mean_us": round(us, 2), "alg_bytes": alg[k],
                              "fraction_of_hbm_peak": round(alg[k] / (us * 1e-6) / HBM_PEAK, 4)}
    if not out:
        raise SystemExit(f"no kernel statistics of the gather kernels under {directory}")
    return out


def spread(ts):
    ms = [t * 1e3 for t in ts]
    return {"median_ms": round(statistics.median(ms), 2), "min_ms": round(min(ms), 2), "max_ms": round(max(ms), 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=("c2", "c5"), default="c2")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--keep", choices=("matrix", "fingerprints"), default="matrix")
    ap.add_argument("--gather-only", action="store_true", help="only leg (b): the run the profiler traces")
    ap.add_argument("--apply", action="store_true", help="also time an apply over 1, 4 and 16 segments")
    ap.add_argument("--kernel-stats", metavar="DIR", help="summarise a rocprofv3 --kernel-trace --stats run (no GPU)")
    args = ap.parse_args()
    pols, mix, seed, docs = shape(args.config)
    ps = K.PolicySet(pols)
    n, R = args.rows, ps.num_rules
    live_n = n - n // 5
    if args.kernel_stats:
        alg = {KERNELS[0]: 2 * live_n * R + 16 * live_n, KERNELS[1]: 32 * live_n}  # rows read and written, the pairs
        print(json.dumps({"config": args.config, "rows": n, "live": live_n, "rules": R, "kernels": kernel_stats(args.kernel_stats, alg)}))
        return
    eng = K.Engine(ordinal=0)  # raises without a gfx950 device: no fallback
    t0 = time.perf_counter()
    lines = ndjson_rows(K.synth_resources(seed, n, mix=mix))
    assert len(lines) == n
    rng = np.random.default_rng(seed)
    cuts = [0, n - 7 * (n // 20)] + [n - (6 - k) * (n // 20) for k in range(7)]
    segs_lines = [lines[a:b] for a, b in zip(cuts, cuts[1:])]
    segs = [K.Corpus(b"\n".join(s), docs=docs).upload(eng.device) for s in segs_lines]
    dead = np.zeros(n, dtype=bool)
    dead[rng.choice(n, n // 5, replace=False)] = True
    key = np.arange(n, dtype=np.float64)  # logical order: a delta segment's even rows replace rows of segment 0
    delta = np.arange(cuts[1], n)
    key[delta[::2]] = rng.uniform(0, cuts[1], size=len(delta[::2]))
    order = np.argsort(key, kind="stable")
    order = order[~dead[order]]
    seg_of = np.searchsorted(np.array(cuts[1:]), order, side="right")
    pairs = np.stack([seg_of, order - np.array(cuts)[seg_of]], axis=1).astype(np.uint64)
    for t, s in enumerate(segs):
        eng.retire_rows(s, np.flatnonzero(dead[cuts[t]:cuts[t + 1]]))

    def keep(c):
        if args.keep == "matrix":
            eng.keep_results(ps, c)
        else:
            eng.keep_fingerprints(ps, c)

    def kept(c):
        return eng.kept_results(c) if args.keep == "matrix" else eng.kept_fingerprints(c)

    eng.evaluate_batch_async(ps, segs)
    for s in segs:
        keep(s)
    eng.device.sync()
    threads = int(os.environ.get("KPE_FLATTEN_THREADS", "0")) or min(16, os.cpu_count() or 1)
    print(f"[bench_compact] {args.config}: {n} rows in {len(segs)} segments, {len(pairs)} live, {R} rules, "
          f"{threads} flatten threads, set-up {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)

    def reflatten():
        t = [time.perf_counter()]
        nd = b"\n".join(lines[i] for i in order)
        t.append(time.perf_counter())
        c = K.Corpus(nd, docs=docs)
        t.append(time.perf_counter())
        c.upload(eng.device)
        t.append(time.perf_counter())
        eng.evaluate_async(ps, c)
        keep(c)
        eng.device.sync()
        t.append(time.perf_counter())
        return c, np.diff(t)

    def gather():
        t = [time.perf_counter()] * 2
        c = K.Corpus.gather(segs, pairs)
        t.append(time.perf_counter())
        c.upload(eng.device)
        t.append(time.perf_counter())
        eng.gather_results(c, segs, pairs)
        eng.device.sync()
        t.append(time.perf_counter())
        return c, np.diff(t)

    legs = {"gather": gather} if args.gather_only else {"reflatten": reflatten, "gather": gather}
    times = {k: [] for k in legs}
    for it in range(args.warmup + args.reps):
        res = {}
        for k, f in legs.items():  # alternating, so both see the same neighbours
            res[k], dt = f()
            if it >= args.warmup:
                times[k].append(dt)
        if len(res) == 2 and it < 2:  # the same state either way (rows past a limit stay undecided either way)
            assert res["gather"].n == res["reflatten"].n == len(pairs)
            assert np.array_equal(kept(res["gather"]), kept(res["reflatten"])), "the carried results differ from the re-evaluated ones"
        del res
    parts = ("join", "flatten | gather", "upload", "evaluate + keep | gather_results")
    out = {"config": args.config, "rows": n, "segments": len(segs), "live": int(len(pairs)), "rules": R, "keep": args.keep,
           "flatten_threads": threads, "reps": args.reps, "warmup": args.warmup}
    for k, ts in times.items():
        out[k] = {"wall": spread([float(sum(x)) for x in ts]), "host": spread([float(x[0] + x[1]) for x in ts]),
                  "parts_ms_median": {p: round(statistics.median([x[i] for x in ts]) * 1e3, 2) for i, p in enumerate(parts)}}
    if len(times) == 2:
        a, b = out["reflatten"], out["gather"]
        out["speedup_median"] = round(a["wall"]["median_ms"] / b["wall"]["median_ms"], 2)
        out["host_speedup_median"] = round(a["host"]["median_ms"] / b["host"]["median_ms"], 2)
        out["gather_below_reflatten_outside_both_spreads"] = bool(b["wall"]["max_ms"] < a["wall"]["min_ms"])
    if args.apply:
        out["apply_ms"] = {}
        nd_live = [lines[i] for i in order]
        m = len(nd_live)
        for k in (1, 4, 16):
            small = m // 50  # delta segments of 2 % each
            cs = [0, m - (k - 1) * small] + [m - (k - 2 - j) * small for j in range(k - 1)]
            parts_k = [K.Corpus(b"\n".join(nd_live[a:b]), docs=docs).upload(eng.device) for a, b in zip(cs, cs[1:])]
            eng.evaluate_batch_async(ps, parts_k)
            for c in parts_k:
                eng.keep_results(ps, c)
            eng.device.sync()
            ts = []
            for it in range(args.warmup + args.reps):
                t = time.perf_counter()
                eng.evaluate_batch_async(ps, parts_k)
                for c in parts_k:
                    eng.changed_rows(ps, c)
                    eng.keep_results(ps, c)
                eng.device.sync()
                if it >= args.warmup:
                    ts.append(time.perf_counter() - t)
            out["apply_ms"][str(k)] = spread(ts)
            del parts_k
    print(json.dumps(out))


if __name__ == "__main__":
    main()
