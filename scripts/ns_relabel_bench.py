#!/usr/bin/env python3
"""A namespace label change on a resident corpus: the in-place path (Engine.set_namespace_labels,
then the next evaluation with its full rebinding and Engine.changed_rows against the kept result)
against what a label change cost before it: a new corpus flattened with the new table, its upload,
the evaluation and the fetch of the whole matrix (the first `apply` of a new ResidentScanner).

Shape: the C4 policy set over 625,000 selector-mix rows and 10,000 namespaces; 1, 100 and all
namespaces relabelled. One process. Per size the table alternates between L0 and a table that
differs from it in exactly that many namespaces, so every timed call changes that many entries.

  host:    set_namespace_labels on a twin corpus that is not uploaded (parse, compare, rebuild of
           the table and of the host r_nsl column; no device call)
  set:     the same call on the uploaded corpus (host part + the table's upload + the row remap
           kernel, waited for); KPE_NSL_REUPLOAD=1 for the alternating `set_reupload` calls sends the
           4 N bytes of r_nsl instead of running the kernel
  eval:    evaluate_async + changed_rows with the verdict rows (binds the program again in full)
  keep:    keep_results of the new matrix
  rebuild: Corpus(nd, L1), upload, evaluate_async + fetch, each timed

Host clocks around calls that end in a stream synchronise; `--warmup` untimed rounds, then the
median and the spread (min, max) of `--reps` rounds. The changed rows of the in-place path are
compared once per size with the difference of the two fetched matrices. Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import kyverno_amd as K  # noqa: E402


def relabelled(L0, k):
    """L0 with the labels of k namespaces changed (spread over the table)."""
    names = list(L0)
    step = max(len(names) // k, 1)
    out = dict(L0)
    for i, ns in enumerate(names[::step][:k]):
        lab = dict(L0[ns])
        lab["env"] = ("staging", "dev", "prod")[i % 3] if lab.get("env") != ("staging", "dev", "prod")[i % 3] else "qa"
        lab["team"] = "team-7" if i % 2 else "team-12"
        lab["relabelled"] = f"r{i % 13}"
        out[ns] = lab
    return out


def stats(xs):
    xs = [x * 1e3 for x in xs]
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=625_000)
    ap.add_argument("--namespaces", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rebuild-reps", type=int, default=3)
    args = ap.parse_args()
    from tests.policies import c4_policy_set

    eng = K.Engine(ordinal=0)  # raises without a gfx950 device: no fallback
    ps = K.PolicySet(c4_policy_set())
    R = ps.num_rules
    nd = K.synth_resources(0xC4, args.rows, mix=K.SYNTH_SELECTORS)
    L0 = json.loads(K.synth_ns_labels(0xC4, args.namespaces, mix=K.SYNTH_SELECTORS))
    sync = eng.device.sync
    out = {"rows": args.rows, "rules": R, "namespaces": args.namespaces, "reps": args.reps, "warmup": args.warmup,
           "r_nsl_bytes": 4 * args.rows, "sizes": {}}

    def clock(f):
        t = time.perf_counter()
        r = f()
        return r, time.perf_counter() - t

    corpus = K.Corpus(nd, L0).upload(eng.device)
    twin = K.Corpus(nd, L0)  # never uploaded: its calls touch no device
    eng.evaluate_async(ps, corpus)
    v0, _, _ = eng.fetch(ps, corpus)
    eng.keep_results(ps, corpus)
    sync()
    for k in (1, 100, args.namespaces):
        k = min(k, args.namespaces)
        Lk = relabelled(L0, k)
        patches = [json.dumps({ns: Lk[ns] for ns in Lk if Lk[ns] != L0[ns]}).encode(),
                   json.dumps({ns: L0[ns] for ns in Lk if Lk[ns] != L0[ns]}).encode()]
        t = {x: [] for x in ("host", "set", "set_reupload", "eval", "keep")}
        changed = None
        inplace = []
        for it in range(args.warmup + args.reps):
            for j in (0, 1):  # L0 -> Lk, then back; the kernel and the re-upload alternate and swap directions
                p, reup = patches[j], (it + j) & 1
                n_h, th = clock(lambda: twin.set_namespace_labels(p))
                os.environ["KPE_NSL_REUPLOAD"] = str(reup)
                n_d, ts = clock(lambda: eng.set_namespace_labels(corpus, p))
                assert n_h == n_d == k, (n_h, n_d, k)

                def ev():
                    eng.evaluate_async(ps, corpus)
                    return eng.changed_rows(ps, corpus)

                (rows, vr, total), te = clock(ev)
                _, tk = clock(lambda: (eng.keep_results(ps, corpus), sync()))
                if changed is None:
                    changed = (rows, vr)
                if it >= args.warmup:
                    t["host"].append(th)
                    t["set_reupload" if reup else "set"].append(ts)
                    t["eval"].append(te)
                    t["keep"].append(tk)
                    if not reup:
                        inplace.append(ts + te)
        os.environ.pop("KPE_NSL_REUPLOAD", None)
        # what the same event cost without the in-place call
        tb = {x: [] for x in ("flatten", "upload", "eval_fetch")}
        vk = None
        for it in range(1 + args.rebuild_reps):
            c, tf = clock(lambda: K.Corpus(nd, Lk))
            _, tu = clock(lambda: (c.upload(eng.device), sync()))

            def first_apply():
                eng.evaluate_async(ps, c)
                return eng.fetch(ps, c)[0]

            vk, te = clock(first_apply)
            del c
            if it >= 1:
                tb["flatten"].append(tf), tb["upload"].append(tu), tb["eval_fetch"].append(te)
        want = np.flatnonzero((v0 != vk).any(axis=1))
        assert np.array_equal(changed[0], want.astype(np.uint64)) and np.array_equal(changed[1], vk[want]), "changed rows differ"
        rebuild = [a + b + c_ for a, b, c_ in zip(tb["flatten"], tb["upload"], tb["eval_fetch"])]
        out["sizes"][str(k)] = {
            "changed_rows": int(want.size), "patch_bytes": len(patches[0]),
            "host_part": stats(t["host"]), "set_namespace_labels": stats(t["set"]),
            "set_namespace_labels_reupload": stats(t["set_reupload"]),
            "device_part_median_ms": round(stats(t["set"])["median_ms"] - stats(t["host"])["median_ms"], 3),
            "evaluate_changed_rows": stats(t["eval"]), "keep_results": stats(t["keep"]),
            "in_place_total": stats(inplace),
            "rebuild": {x: stats(v) for x, v in tb.items()}, "rebuild_total": stats(rebuild),
            "speedup_median": round(statistics.median(rebuild) / statistics.median(inplace), 1),
            "remap_kernel_below_reupload_by_more_than_spread": bool(max(t["set"]) < min(t["set_reupload"])),
        }
        print(f"[ns_relabel_bench] {k} namespaces: {json.dumps(out['sizes'][str(k)])}", file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
