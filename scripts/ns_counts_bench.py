#!/usr/bin/env python3
"""Per-namespace rule counts on the device against what a consumer does without them, at the C2
shape (1M pods x restricted:latest, R = 3, 1000 namespaces) and the C3 shape (1.25M rows x 204
rules). One process, one evaluation per shape, then three legs, alternating:

  device: kpe_fetch_namespace_counts for all groups: wall time including the read-back of the
          G x R x 24-byte table, without the one-time rows-by-namespace index (an untimed first
          call builds it; its build + upload time is reported on its own);
  fetch:  kpe_fetch of the N x R verdict matrix alone;
  host:   kpe_namespace_counts_host over that matrix (the group-by a consumer runs after fetch).

Wall times are host clocks around calls that end in a stream synchronise: `--warmup` untimed
rounds, then the median and the spread (min, max) of `--reps` rounds. The kernel time comes from
HIP events around the launch (kpe_device_set_timing), in a loop of device calls of its own after
the wall-time rounds (which run with the events off). The
achieved rate is the kernel's algorithmic bytes (the matrix once, 4 bytes per row of row ids, 16
bytes per work item, the zeroed and written output window) over the median kernel time, as a
fraction of the 8 TB/s HBM peak. The device table is compared with the host fold once. Prints one
JSON line per shape."""
import argparse
import ctypes
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
CHUNK = 512  # rows per work item (results.hip kNsChunk)
SHAPES = {"c2": 1_000_000, "c3": 1_250_000}


def shape(cfg, rows):
    from tests.policies import c3_policy_set, restricted_latest

    if cfg == "c3":
        return c3_policy_set(), K.SYNTH_C3, 0xC3, rows or SHAPES[cfg], True
    return [restricted_latest()], K.SYNTH_PODS, 0xC2, rows or SHAPES[cfg], False  # no pattern rules: no tapes


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def run(cfg, rows, reps, warmup):
    policies, mix, seed, n, docs = shape(cfg, rows)
    ps = K.PolicySet(policies)
    R = ps.num_rules
    eng = K.Engine(ordinal=0)  # raises without a gfx950 device: no fallback
    L = load()
    t0 = time.perf_counter()
    corpus = K.Corpus(K.synth_resources(seed, n, mix=mix), docs=docs).upload(eng.device)
    eng.evaluate_async(ps, corpus)
    eng.device.sync()
    G = len(corpus.namespaces)
    print(f"[ns_counts_bench] {cfg}: {n} x {R} evaluated, {G} groups, set-up {time.perf_counter() - t0:.1f} s",
          file=sys.stderr, flush=True)
    table = np.zeros((G, R, 6), dtype=np.uint32)
    host = np.zeros((G, R, 6), dtype=np.uint32)
    v = np.zeros((n, R), dtype=np.uint8)
    kms, ims = ctypes.c_double(), ctypes.c_double()

    def device():
        t = time.perf_counter()
        check(L.kpe_fetch_namespace_counts(eng.device.h, ps.h, corpus.h, 0, G, table.ctypes.data))
        return (time.perf_counter() - t) * 1e3

    def fetch():
        t = time.perf_counter()
        check(L.kpe_fetch(eng.device.h, ps.h, corpus.h, v.ctypes.data, None, None))
        return (time.perf_counter() - t) * 1e3

    def fold():
        t = time.perf_counter()
        check(L.kpe_namespace_counts_host(ps.h, corpus.h, v.ctypes.data, 0, G, host.ctypes.data))
        return (time.perf_counter() - t) * 1e3

    eng.device.set_timing(True)
    first_ms = device()  # builds and uploads the index
    check(L.kpe_debug_ns_counts_ms(eng.device.h, None, ctypes.byref(ims)))
    index_ms = ims.value
    eng.device.set_timing(False)
    legs = {"device": device, "fetch": fetch, "host": fold}
    times = {k: [] for k in legs}
    for it in range(warmup + reps):
        for k, f in legs.items():  # alternating, so every leg sees the same neighbours
            dt = f()
            if it >= warmup:
                times[k].append(dt)
    # kernel times in a loop of their own: the events cost the host a little
    eng.device.set_timing(True)
    kernel = []
    for it in range(warmup + reps):
        device()
        check(L.kpe_debug_ns_counts_ms(eng.device.h, ctypes.byref(kms), None))
        if it >= warmup:
            kernel.append(kms.value)
    eng.device.set_timing(False)
    assert np.array_equal(table, host), "device table differs from the host fold"
    rows_per_group = corpus.namespace_rows()
    items = int(((rows_per_group + CHUNK - 1) // CHUNK).sum())
    alg = n * R + 4 * n + 16 * items + 2 * G * R * 24
    kmed = statistics.median(kernel)
    out = {"config": cfg, "rows": n, "rules": R, "groups": G, "work_items": items, "matrix_bytes": n * R,
           "table_bytes": G * R * 24, "reps": reps, "warmup": warmup,
           "device_wall": stats(times["device"]), "fetch_wall": stats(times["fetch"]), "host_fold_wall": stats(times["host"]),
           "kernel": stats(kernel), "kernel_alg_bytes": alg,
           "kernel_fraction_of_hbm_peak": round(alg / (kmed * 1e-3) / HBM_PEAK, 4),
           "index_build_upload_ms": round(index_ms, 3), "first_call_ms": round(first_ms, 3),
           "device_below_fetch": bool(max(times["device"]) < min(times["fetch"])),
           "fetch_over_device_median": round(statistics.median(times["fetch"]) / statistics.median(times["device"]), 2)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=("c2", "c3", "both"), default="both")
    ap.add_argument("--rows", type=int, default=0, help="rows instead of the shape's (a rehearsal)")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    for cfg in (("c2", "c3") if args.config == "both" else (args.config,)):
        run(cfg, args.rows, args.reps, args.warmup)


if __name__ == "__main__":
    main()
