"""bench.py --dump-outputs: the last timed step's outputs as .npy files. CPU: the writer (dtypes,
the fixed seeded row sample of a matrix past the size cap). GPU: one small plain run in this
process, whose dumped verdicts and counts are checked against the oracle on the same synthetic
rows, and whose result line holds the headline keys and none of the --full legs."""
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _counts(v):
    return [{"na": int((col == 0).sum()), "pass": int((col == 1).sum()), "fail": int((col == 2).sum()),
             "warn": int((col == 3).sum()), "error": int((col == 4).sum()), "skip": int((col == 5).sum()),
             "undecided": int((col == 7).sum())} for col in v.T]


def test_dump_writes_float_arrays(tmp_path):
    b = _bench()
    v = (np.arange(7 * 3, dtype=np.uint8).reshape(7, 3) % 6)
    b.dump_outputs(str(tmp_path / "d"), v, _counts(v))
    got = np.load(tmp_path / "d" / "verdicts.npy")
    assert got.dtype == np.float32 and np.array_equal(got, v)
    rows = np.load(tmp_path / "d" / "verdict_rows.npy")
    assert rows.dtype == np.float64 and np.array_equal(rows, np.arange(7))
    cnt = np.load(tmp_path / "d" / "counts.npy")
    assert cnt.dtype == np.float64 and cnt.shape == (3, 7)
    assert np.array_equal(cnt.sum(axis=1), [7, 7, 7])


def test_dump_rows_sample_is_fixed_and_within_the_cap():
    b = _bench()
    # a row costs R float32 cells and one float64 index: 10 rows x (3 * 4 + 8) = the cap
    assert np.array_equal(b.dump_rows(10, 3, cap_bytes=200), np.arange(10))
    r1 = b.dump_rows(1000, 3, cap_bytes=2000)
    r2 = b.dump_rows(1000, 3, cap_bytes=2000)
    assert np.array_equal(r1, r2)
    assert r1.size == 100
    assert np.all(np.diff(r1) > 0) and 0 <= r1[0] and r1[-1] < 1000
    # the default cap leaves room for the counts within 64 MB, for few rules and for many
    for n, R in ((20_000_000, 1), (1_250_000, 406)):
        rows = b.dump_rows(n, R)
        assert 0 < rows.size < n and rows.size * R * 4 + rows.size * 8 + R * 7 * 8 <= 64 * 10**6


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(tmp_path, capsys, oracle):
    import kyverno_amd as K
    from tests.policies import restricted_latest

    b = _bench()
    n, replicas, steps = 3001, 3, 5
    b.main(["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--resources", str(n), "--replicas", str(replicas),
            "--dump-outputs", str(tmp_path)])
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(line) == 1
    d = json.loads(line[0])
    assert d["steps"] == steps and d["ms_per_step"] > 0 and d["unit"] == "resource-rule evals/s"
    assert d["higher_is_better"] is True and d["dtype"] == "u32"
    assert d["value"] == pytest.approx(n * d["config"]["rules"] * steps / (d["ms_per_step"] * 1e-3 * steps))
    for k in ("roofline", "cpu_baseline", "gather", "masks_step", "e2e"):
        assert k not in d
    # step i evaluates shard i % replicas; shard k holds rows [k * n, (k + 1) * n) of the corpus
    last = (steps - 1) % replicas
    nd = K.synth_resources(0xC2, n, K.SYNTH_PODS, last * n)
    ref = oracle.validate([restricted_latest()], nd, nthreads=2)
    v = np.load(tmp_path / "verdicts.npy")
    assert v.dtype == np.float32 and np.array_equal(v, ref)
    assert np.array_equal(np.load(tmp_path / "verdict_rows.npy"), np.arange(n))
    want = [[c[f] for f in ("na", "pass", "fail", "warn", "error", "skip", "undecided")] for c in _counts(ref)]
    assert np.array_equal(np.load(tmp_path / "counts.npy"), want)
