#!/usr/bin/env python3
"""Reports of the rows an edit changed: the bulk path (one sparse fetch, one render call) against the
best path built from the per-row calls, at the C3 shape (1.25M rows x 204 rules) and the C2 shape
(1M rows x 3 rules) with the edits of scripts/bench_delta.py. One process: program A is evaluated
and its fingerprints kept, program B is evaluated with check masks, the changed rows are the list.
Per round:

  (a) per-row: kpe_fetch_cv_masks of the whole matrix, kpe_fetch_cond_traces_ex over the range that
      covers the listed rows (when some rule evaluates conditions per resource), a cell list built on
      the host from the policies' text into one kpe_pattern_traces call, then kpe_report_results_ex
      once per listed row. Only calls that exist without the bulk path.
  (b) bulk:    kpe_fetch_report_rows (a count call, then an exact call) and kpe_report_results_rows.

Wall times are host clocks around calls that end in a stream synchronise: `--warmup` untimed rounds,
then the median and the spread (min, max) of `--reps` rounds, (a) and (b) alternating; fetch and
render apart, and the bytes each leg copies back. Both legs' reports are compared once. Prints one
JSON line per shape.

Kernel durations come from a run of their own under the profiler, which slows the host:

  rocprofv3 --kernel-trace --stats -d DIR -o rr --output-format csv -- \\
      python3 scripts/bench_report_rows.py --config c3 --bulk-only
  python3 scripts/bench_report_rows.py --config c3 --kernel-stats DIR --listed K --cells M,C,P

The second command reads the profiler's kernel statistics and prints each kernel's mean duration and
its algorithmic bytes over that time as a fraction of the 8 TB/s HBM peak: the compact matrix once
per pass (and 12 bytes per tile of counts), 12 / 24 / 264 bytes per mask / cond / pattern cell out
(the cell index twice for a pattern cell: compact and absolute) and 8 bytes per listed row in for the
scatter; the row gather reads and writes each listed row."""
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

PASS, FAIL, ERROR = 1, 2, 4
TR = 4 * 16  # words of a pattern record


def alg_bytes(listed, R, cells):
    m, c, p = cells
    compact = listed * R
    tiles = (compact + 4095) // 4096
    return {"kpe_gather_rows_kernel": listed * (8 + 2 * R),
            "kpe_report_need_count_kernel": compact + 12 * tiles,
            "kpe_select_scan_kernel": 12 * tiles + 8 * (3 * tiles + 1),
            "kpe_report_need_scatter_kernel": compact + 24 * tiles + 8 * listed + 12 * m + 24 * c + 16 * p,
            "kpe_pattern_trace_kernel": 264 * p}


def kernel_stats(directory, listed, R, cells):
    want = alg_bytes(listed, R, cells)
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for rec in csv.DictReader(open(path)):
            for k in want:
                if k in rec["Name"]:
                    c, tot = rows.get(k, (0, 0.0))
                    rows[k] = (c + int(rec["Calls"]), tot + float(rec["TotalDurationNs"]))
    if not rows:
        raise SystemExit(f"no kernel statistics of the report kernels under {directory}")
    out = {}
    for k, b in want.items():
        if k in rows:
            calls, tot = rows[k]
            us = tot / calls / 1e3
            out[k] = {"calls": calls, "mean_us": round(us, 2), "alg_bytes": b,
                      "fraction_of_hbm_peak": round(b / (us * 1e-6) / HBM_PEAK, 4)}
    return out


def text_need(pols, ps):
    """Per rule the verdicts whose cell needs a pattern record, and whether any rule evaluates
    conditions per resource, from the policies' text (what a caller knows without the bulk path)."""
    by = {(p["metadata"]["name"], r["name"]): r for p in pols for r in p["spec"]["rules"]}
    pat = np.zeros(ps.num_rules, dtype=np.uint8)
    cond = False
    for j, full in enumerate(ps.rule_names):
        pn, rn = full.split("/", 1)
        r = by[(pn, rn.replace("autogen-cronjob-", "").replace("autogen-", ""))]
        v = r.get("validate", {})
        if "pattern" in v:
            pat[j] = K.SEL(FAIL)
        if "anyPattern" in v:
            pat[j] = K.SEL(FAIL) | K.SEL(PASS)
        if "foreach" in v and "attern" in json.dumps(v["foreach"]):
            pat[j] = K.SEL(FAIL) | K.SEL(ERROR)
        cond = cond or "preconditions" in r or "deny" in v or "foreach" in v
    return pat, cond


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=("c3", "c2"), default="c3")
    ap.add_argument("--rows", type=int, default=0, help="rows instead of the shape's (a rehearsal)")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bulk-only", action="store_true", help="only leg (b): the run the profiler traces")
    ap.add_argument("--kernel-stats", metavar="DIR", help="summarise a rocprofv3 --kernel-trace --stats run (no GPU)")
    ap.add_argument("--listed", type=int, default=0, help="with --kernel-stats: listed rows of the traced run")
    ap.add_argument("--cells", default="0,0,0", help="with --kernel-stats: mask,cond,pattern cells of the traced run")
    args = ap.parse_args()
    pa, pb, mix, seed, n, docs = shape(args.config, args.rows)
    psa, psb = K.PolicySet(pa), K.PolicySet(pb)
    R = psb.num_rules
    if args.kernel_stats:
        cells = tuple(int(x) for x in args.cells.split(","))
        print(json.dumps({"config": args.config, "rows": n, "rules": R, "listed": args.listed, "cells": cells,
                          "kernels": kernel_stats(args.kernel_stats, args.listed, R, cells)}))
        return
    eng = K.Engine(ordinal=0)  # raises without a gfx950 device: no fallback
    t0 = time.perf_counter()
    nd = K.synth_resources(seed, n, mix=mix)
    corpus = K.Corpus(nd, docs=docs).upload(eng.device)
    eng.evaluate_async(psa, corpus)
    eng.keep_fingerprints(psa, corpus)
    eng.evaluate_async(psb, corpus, masks=True)
    rows, vr, _, _ = eng.changed_rows_fp(psb, corpus)
    ri = rows.astype(np.int64)
    lines = K.scan.ndjson_rows(nd)
    res = [lines[i] for i in ri]
    del nd, lines
    pat_need, any_cond = text_need(pb, psb)
    pss = np.array(psb.is_pss)
    print(f"[bench_report_rows] {args.config}: {n} x {R}, {rows.size} listed rows, set-up {time.perf_counter() - t0:.1f} s",
          file=sys.stderr, flush=True)

    def leg_a():
        t = [time.perf_counter()]
        raw = eng.cv_masks(psb, corpus, raw=True)
        lo = int(ri.min()) if ri.size else 0
        cx = eng.cond_traces(psb, corpus, lo, int(ri.max()) - lo + 1, ex=True) if (any_cond and ri.size) else None
        hit = ((pat_need[None, :].astype(np.uint32) >> vr) & 1).astype(bool)
        kk, rr = np.nonzero(hit)
        tr = eng.pattern_traces(psb, corpus, (ri[kk] * R + rr).astype(np.uint64))
        nbytes = raw.nbytes + (cx.nbytes if cx is not None else 0) + tr.nbytes
        t.append(time.perf_counter())
        out = []
        first = np.searchsorted(kk, np.arange(rows.size + 1))
        dense = np.zeros((R, 4, 16), dtype=np.uint32)
        for k, i in enumerate(ri):
            a, b = first[k], first[k + 1]
            dense[rr[a:b]] = tr[a:b]
            out.append(K.report_results(psb, vr[k], cv_mask_row=raw[i] if pss.any() else None, resource=res[k],
                                        traces=dense if b > a else None, corpus=corpus,
                                        cond_traces=None if cx is None else cx[i - lo]))
            dense[rr[a:b]] = 0
        t.append(time.perf_counter())
        return out, (t[1] - t[0], t[2] - t[1]), nbytes

    def leg_b():
        t = [time.perf_counter()]
        sp = eng.fetch_report_rows(psb, corpus, rows)
        nbytes = sum(v.nbytes for v in sp.values() if isinstance(v, np.ndarray))
        t.append(time.perf_counter())
        out = K.render_report_rows(psb, sp, resources=res, corpus=corpus, raw=True)
        t.append(time.perf_counter())
        cells = (sp["mask_total"], sp["cond_total"], sp["pattern_total"])
        return out, (t[1] - t[0], t[2] - t[1]), nbytes, cells

    legs = {"per_row": leg_a, "bulk": leg_b}
    if args.bulk_only:
        del legs["per_row"]
    times = {k: [] for k in legs}
    last = {}
    for it in range(args.warmup + args.reps):
        for k, f in legs.items():  # alternating, so both see the same neighbours
            last[k] = f()
            if it >= args.warmup:
                times[k].append(last[k][1])
    if len(last) == 2:
        bulk = [json.loads(x.decode()) for x in last["bulk"][0]]
        assert bulk == last["per_row"][0], "the two legs' reports differ"
    out = {"config": args.config, "rows": n, "rules": R, "listed": int(rows.size), "cells": list(last["bulk"][3]),
           "reps": args.reps, "warmup": args.warmup}
    for k, ts in times.items():
        out[k] = {"bytes_back": int(last[k][2])}
        for i, part in enumerate(("fetch", "render")):
            x = [a[i] * 1e3 for a in ts]
            out[k][part] = {"ms_median": round(statistics.median(x), 3), "ms_min": round(min(x), 3),
                            "ms_max": round(max(x), 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
