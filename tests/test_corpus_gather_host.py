"""kpe_corpus_gather and kpe_corpus_row_digests, the host half of compaction by gather (no GPU): a
corpus built out of chosen rows of other corpora against a whole and a fresh flatten, the row digest's
sensitivity, the argument errors, and the stand-alone sanitizer program (scripts/corpus_gather_check.cpp)
that runs the host gather and the body of the kpe_results_gather kernels under ASan / UBSan."""
import copy
import ctypes
import random
import subprocess

import numpy as np
import pytest

import kyverno_amd as K
from kyverno_amd._lib import KpeError, load
from kyverno_amd.scan import ndjson_rows
from tests.conftest import build_host_tool

SEED = 7
CUTS = [0, 1, 64, 128, 193]  # chunks of 1, 63, 64, 65 rows and the rest


@pytest.fixture(scope="module")
def case():
    nd = K.synth_resources(SEED, 3000, mix=K.SYNTH_EDGE)
    nsl = K.synth_ns_labels(SEED, 40, mix=K.SYNTH_EDGE)
    rows = ndjson_rows(nd)
    assert len(rows) == 3000
    cuts = CUTS + [len(rows)]
    chunks = [rows[a:b] for a, b in zip(cuts, cuts[1:])]
    assert [len(c) for c in chunks[:4]] == [1, 63, 64, 65]
    return nd, nsl, rows, chunks


def _sources(case, docs):
    _, nsl, _, chunks = case
    return [K.Corpus(b"\n".join(c), nsl, docs=docs) for c in chunks]


def _all_pairs(chunks):
    return [(t, r) for t, c in enumerate(chunks) for r in range(len(c))]


def test_symbols_exported():
    L = load()
    assert hasattr(L, "kpe_corpus_gather") and hasattr(L, "kpe_corpus_row_digests") and hasattr(L, "kpe_results_gather")
    assert (K.GATHER_MATRIX, K.GATHER_FINGERPRINTS) == (1, 2)


@pytest.mark.parametrize("docs", [True, False])
def test_every_row_in_order_is_the_whole_flatten(case, docs):
    nd, nsl, _, chunks = case
    whole = K.Corpus(nd, nsl, docs=docs)
    g = K.Corpus.gather(_sources(case, docs), _all_pairs(chunks))
    assert g.n == whole.n == 3000 and g.device is None
    assert g.digest() == whole.digest()
    assert np.array_equal(g.row_digests(), whole.row_digests())


@pytest.mark.parametrize("docs", [True, False])
def test_subset_in_another_order_is_a_fresh_flatten_of_those_lines(case, docs):
    """The list: random.Random(5) drops each pair with probability 0.2 and shuffles the rest."""
    _, nsl, rows, chunks = case
    rng = random.Random(5)
    sel = [p for p in _all_pairs(chunks) if rng.random() >= 0.2]
    rng.shuffle(sel)
    assert 2300 < len(sel) < 2500 and len({t for t, _ in sel}) == 5
    srcs = _sources(case, docs)
    g = K.Corpus.gather(srcs, sel)
    start = np.cumsum([0] + [len(c) for c in chunks])
    fresh = K.Corpus(b"\n".join(rows[start[t] + r] for t, r in sel), nsl, docs=docs)
    assert g.n == fresh.n == len(sel)
    ok = (fresh.row_flags() & 2) == 0  # equality is required of rows not past a limit
    assert ok.sum() > 2000
    dg = g.row_digests()
    assert np.array_equal(dg[ok], fresh.row_digests()[ok])
    assert np.array_equal(g.row_flags(), fresh.row_flags())
    assert [g.namespaces[i] for i in g.row_namespaces()] == [fresh.namespaces[i] for i in fresh.row_namespaces()]
    assert g.namespace_labels() == fresh.namespace_labels() == srcs[0].namespace_labels()
    ds = [s.row_digests() for s in srcs]
    assert np.array_equal(dg, np.array([ds[t][r] for t, r in sel], dtype=np.uint64))
    # the id maps were not the identity: the first namespace of source 1 (its group 0) is not the
    # gathered corpus's group 0, which is the namespace of the first row of the shuffled list
    assert sel[0][0] != 1 and srcs[1].namespaces[0] != g.namespaces[0]
    assert len(set(dg[ok].tolist())) == ok.sum()  # distinct resources, distinct digests


# ---- the digest's sensitivity: one change at a time in one resource ----
def _pod(i, ns):
    return {"apiVersion": "v1", "kind": "Pod",
            "metadata": {"name": f"p{i}", "namespace": ns, "labels": {"app": "a", "tier": f"t{i % 2}"},
                         "annotations": {"note": "n", "container.apparmor.security.beta.kubernetes.io/c": "runtime/default"}},
            "spec": {"securityContext": {"sysctls": [{"name": "kernel.shm_rmid_forced", "value": "0"}]},
                     "volumes": [{"name": "v", "emptyDir": {}}],
                     "containers": [{"name": "c", "image": "nginx:1.25", "ports": [{"containerPort": 80, "hostPort": 8080}],
                                     "securityContext": {"capabilities": {"add": ["NET_BIND_SERVICE"], "drop": ["ALL"]}},
                                     "resources": {"limits": {"cpu": "1", "memory": "1Gi"}}}]}}


def _c0(d):
    return d["spec"]["containers"][0]


def _rename_member(d):
    d["spec"]["containers"][0]["resources"]["limits"] = {"cpu": "1", "mem": "1Gi"}


CHANGES = {
    "image": lambda d: _c0(d).__setitem__("image", "nginx:1.26"),
    "label value": lambda d: d["metadata"]["labels"].__setitem__("app", "b"),
    "annotation key": lambda d: d["metadata"]["annotations"].__setitem__("note2", d["metadata"]["annotations"].pop("note")),
    "added capability": lambda d: _c0(d)["securityContext"]["capabilities"]["add"].append("SYS_TIME"),
    "hostPort": lambda d: _c0(d)["ports"][0].__setitem__("hostPort", 8081),
    "sysctl": lambda d: d["spec"]["securityContext"]["sysctls"][0].__setitem__("name", "net.ipv4.ping_group_range"),
    "volume source": lambda d: d["spec"]["volumes"].__setitem__(0, {"name": "v", "hostPath": {"path": "/x"}}),
    "nested scalar in spec": lambda d: _c0(d)["resources"]["limits"].__setitem__("memory", "2Gi"),
    "member renamed": _rename_member,
}
BASE_LABELS = {"ns-1": {"env": "prod"}, "ns-2": {"env": "dev"}, "ns-3": {"env": "dev"}}


def _digests(pods, labels, docs=True):
    return K.Corpus(pods, labels, docs=docs).row_digests()


@pytest.mark.parametrize("what", list(CHANGES) + ["namespace labels"])
def test_digest_changes_with_one_row_alone(what):
    pods = [_pod(i, f"ns-{i}") for i in range(5)]  # row 2 is alone in ns-2
    base = _digests(pods, BASE_LABELS)
    assert len(set(base.tolist())) == 5
    changed, labels = copy.deepcopy(pods), BASE_LABELS
    if what == "namespace labels":
        labels = {**BASE_LABELS, "ns-2": {"env": "qa"}}
    else:
        CHANGES[what](changed[2])
        assert changed[2] != pods[2]
    d = _digests(changed, labels)
    assert d[2] != base[2], what
    assert np.array_equal(np.delete(d, 2), np.delete(base, 2)), what
    # whatever else the corpus holds: the same resources after unrelated rows, other ids, equal digests
    more = [_pod(10 + i, f"other-{i}") for i in range(3)] + changed
    assert np.array_equal(_digests(more, labels)[3:], d), what
    if what not in ("nested scalar in spec", "member renamed"):  # what the tape alone holds
        nd_base, nd_new = _digests(pods, BASE_LABELS, docs=False), _digests(changed, labels, docs=False)
        assert nd_new[2] != nd_base[2] and np.array_equal(np.delete(nd_new, 2), np.delete(nd_base, 2)), what


# ---- further cases ----
def test_duplicate_pair_empty_list_single_source(case):
    _, nsl, rows, _ = case
    src = K.Corpus(b"\n".join(rows[:50]), nsl)
    d = src.row_digests()
    g = K.Corpus.gather([src], [(0, 7), (0, 3), (0, 7)])
    assert g.n == 3 and np.array_equal(g.row_digests(), d[[7, 3, 7]])
    fresh = K.Corpus(b"\n".join([rows[7], rows[3], rows[7]]), nsl)
    assert np.array_equal(g.row_digests(), fresh.row_digests())
    assert [g.namespaces[i] for i in g.row_namespaces()] == [fresh.namespaces[i] for i in fresh.row_namespaces()]
    assert len(g.namespaces) > len(fresh.namespaces)  # groups without rows: the dropped rows' namespaces stay
    e = K.Corpus.gather([src], [])
    assert e.n == 0 and len(e.row_digests()) == 0 and e.namespace_labels() == src.namespace_labels()
    assert e.row_flags().shape == (0,) and e.namespaces[e.namespaces.index("")] == ""
    same = K.Corpus.gather([src], [(0, r) for r in range(50)])
    assert same.digest() == src.digest()


def _raw_gather(srcs, pairs, out):
    hs = (ctypes.c_void_p * max(len(srcs), 1))(*[s.h if s is not None else None for s in srcs])
    p = np.ascontiguousarray(pairs, dtype=np.uint64).reshape(-1, 2)
    return load().kpe_corpus_gather(hs, len(srcs), p.ctypes.data if p.size else None, len(p), out)


def test_errors_leave_out_untouched(case):
    _, nsl, rows, _ = case
    a, b = K.Corpus(b"\n".join(rows[:10]), nsl), K.Corpus(b"\n".join(rows[10:30]), nsl)
    L = load()
    out = ctypes.c_void_p()
    ok = [(0, 1), (1, 19)]
    assert _raw_gather([a, b], ok, None) == 1  # KPE_E_INVALID: null out
    assert L.kpe_corpus_gather(None, 2, None, 0, ctypes.byref(out)) == 1 and not out.value
    assert _raw_gather([], [], ctypes.byref(out)) == 1 and not out.value  # no source
    assert _raw_gather([a, None], ok, ctypes.byref(out)) == 1 and not out.value
    hs = (ctypes.c_void_p * 2)(a.h, b.h)
    assert L.kpe_corpus_gather(hs, 2, None, 2, ctypes.byref(out)) == 1 and not out.value  # pairs null, npairs > 0
    for bad in ([(2, 0)], [(0, 10)], [(1, 20)], [(0, 1), (1, 2 ** 40)]):
        assert _raw_gather([a, b], bad, ctypes.byref(out)) == 1 and not out.value, bad
    # a retired row (recorded on the host: the corpus is not uploaded)
    check = L.kpe_corpus_retire_rows(None, b.h, np.array([19], dtype=np.uint64).ctypes.data, 1)
    assert check == 0
    assert _raw_gather([a, b], ok, ctypes.byref(out)) == 1 and not out.value
    assert b"retired" in L.kpe_last_error()
    assert _raw_gather([a, b], [(0, 1), (1, 18)], ctypes.byref(out)) == 0 and out.value
    L.kpe_corpus_free(out)
    out = ctypes.c_void_p()
    # sources that differ in documents, or in their label tables (as sets of pairs, by namespace)
    nodocs = K.Corpus(b"\n".join(rows[10:30]), nsl, docs=False)
    assert _raw_gather([a, nodocs], [(0, 1), (1, 18)], ctypes.byref(out)) == 1 and not out.value
    labels = a.namespace_labels()
    first = next(iter(labels))
    other = K.Corpus(b"\n".join(rows[10:30]), {**labels, first: {**labels[first], "extra": "label"}})
    assert _raw_gather([a, other], [(0, 1), (1, 18)], ctypes.byref(out)) == 1 and not out.value
    fewer = K.Corpus(b"\n".join(rows[10:30]), {k: v for k, v in labels.items() if k != first})
    with pytest.raises(KpeError) as e:
        K.Corpus.gather([a, fewer], [(0, 1)])  # a source listed for no row counts too
    assert e.value.status == 1
    # the same table in another order, a label pair twice: equal as sets
    again = K.Corpus(b"\n".join(rows[10:30]), dict(reversed(list(labels.items()))))
    g = K.Corpus.gather([a, again], [(1, 3), (0, 2)])
    assert g.namespace_labels() == labels
    assert np.array_equal(g.row_digests(), K.Corpus(b"\n".join([rows[13], rows[2]]), nsl).row_digests())
    assert L.kpe_corpus_row_digests(None, None) == 1


def test_limit_and_decode_error_rows_keep_their_flags():
    big = _pod(0, "ns-1")
    big["spec"]["containers"] = [{"name": f"c{i}", "image": "x"} for i in range(256)]  # past KPE_MAX_LIST
    broken = _pod(1, "ns-1")
    broken["spec"]["hostNetwork"] = "yes"  # a type error in a modelled field
    cfg = {"apiVersion": "v1", "kind": "ConfigMap", "metadata": {"name": "cm", "namespace": "ns-2"}, "data": {"k": "v"}}
    a = K.Corpus([_pod(2, "ns-2"), big], BASE_LABELS)
    b = K.Corpus([broken, cfg, _pod(3, "ns-3")], BASE_LABELS)
    assert a.row_flags().tolist() == [0, 2] and b.row_flags().tolist() == [1, 4, 0]
    g = K.Corpus.gather([a, b], [(1, 1), (0, 1), (1, 0), (0, 0), (0, 1)])
    assert g.row_flags().tolist() == [4, 2, 1, 0, 2]
    da, db = a.row_digests(), b.row_digests()
    assert g.row_digests().tolist() == [db[1], da[1], db[0], da[0], da[1]]


def test_merged_capability_names_past_64_is_a_limit():
    def pod(i, caps):
        d = _pod(i, "ns-1")
        _c0(d)["securityContext"]["capabilities"] = {"add": caps}
        return d

    names = [f"CAP_{i:02d}" for i in range(65)]
    a = K.Corpus([pod(i, names[4 * i:4 * i + 4]) for i in range(8)], BASE_LABELS)  # 32 names
    b = K.Corpus([pod(i, names[32 + 3 * i:35 + 3 * i]) for i in range(11)], BASE_LABELS)  # 33 more
    assert not a.row_flags().any() and not b.row_flags().any()
    out = ctypes.c_void_p()
    assert _raw_gather([a, b], [(0, 0), (1, 0)], ctypes.byref(out)) == 4 and not out.value  # KPE_E_LIMIT
    with pytest.raises(KpeError) as e:
        K.Corpus.gather([a, b], [(0, 0), (1, 0)])
    assert e.value.status == 4
    assert K.Corpus.gather([a, a], [(1, 2), (0, 0)]).n == 2  # 32 names, twice: no limit


def test_corpus_gather_check_tool(case, tmp_path):
    """The identity and subset cases, and the kpe_results_gather kernels' body lane by lane over
    buffers of exactly N x R and npairs x R bytes (R in 1, 3, 4, 5, 17, 204; npairs in 1, 63, 64, 65,
    1000), under ASan / UBSan."""
    nd, nsl, _, _ = case
    (tmp_path / "rows.ndjson").write_bytes(nd)
    (tmp_path / "nsl.json").write_bytes(nsl)
    tool = build_host_tool("corpus_gather_check")
    r = subprocess.run([tool, str(tmp_path / "rows.ndjson"), str(tmp_path / "nsl.json")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "corpus_gather_check ok" in r.stdout, r.stdout + r.stderr
