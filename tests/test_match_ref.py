"""Pins tests/match_ref.py, the plain reference the placement-regime tests compare the device
with, before a GPU is involved: `glob` against the go-wildcard vectors and the oracle, `matches`
against the oracle on every case of the regime table and against the reference's own
MatchesResourceDescription vectors. CPU only; needs the oracle, not libkpe.so."""
import json
import os
import random

import numpy as np
import pytest

from tests import match_ref as M

GOLD = os.path.join(os.path.dirname(__file__), "golden")
WILD = json.load(open(os.path.join(GOLD, "wildcard_match.json")))
MRD = json.load(open(os.path.join(GOLD, "match_rd_cases.json")))


def test_glob_equals_go_wildcard_vectors():
    assert len(WILD["match"]) == 52
    for c in WILD["match"]:
        assert M.glob(c["pattern"], c["text"]) == c["matched"], c


def test_glob_equals_oracle_on_random_table(oracle):
    """Seeded pattern / text pairs over a small alphabet with 2-, 3- and 4-byte runes, so that
    most pairs come close to matching and both answers occur."""
    rng = random.Random(0x610B)
    alpha = "ab-.é本\U0001F600"
    hits = 0
    for _ in range(20000):
        t = "".join(rng.choice(alpha) for _ in range(rng.randrange(0, 9)))
        p = "".join(rng.choice(alpha + "**??") for _ in range(rng.randrange(0, 7)))
        got = M.glob(p, t)
        hits += got
        assert got == oracle.wildcard(p, t), (p, t)
    assert 1000 < hits < 19000  # both answers are common in the table
    # the retry after `*` steps whole runes: one rune cannot serve two `?`
    assert not M.glob("*??y!", "本y!") and M.glob("*??y!", "a本y!")


@pytest.mark.parametrize("name", list(M.REGIMES))
def test_matches_equals_oracle(oracle, name):
    _, pols, nd, docs, sh = M.regime_case(name)
    ref = oracle.validate(pols, nd, nthreads=8)
    want = np.array(M.match_matrix(pols, docs), dtype=bool)
    assert ref.shape == want.shape
    assert set(np.unique(ref)) <= {0, 1}  # the validate pattern cannot fail: a cell is 0 or pass
    bad = np.argwhere((ref != 0) != want)
    assert bad.size == 0, f"{len(bad)} cells differ, first {bad[:5].tolist()}"
    # no column is decided by nothing: the table as a whole has matched and unmatched cells
    assert want.any() or len(docs) < 3, "no rule matches any row"
    assert not want.all()


def test_regime_table_shapes():
    """The knobs give exactly the dictionaries asked for, and the derived shapes sit on the
    documented edges they are named for."""
    def sh(name):
        return M.regime_case(name)[4]

    for n in (31, 32, 33, 64):
        assert sh(f"fused-{n}")["dict"]["name"] == n and sh(f"fused-{n}")["pairs"] <= M.FUSE_PAIRS
    assert sh("fused-1024-pairs")["pairs"] == M.FUSE_PAIRS
    assert sh("past-1025-pairs")["pairs"] == M.FUSE_PAIRS + 1
    assert sh("fused-4095-byte-string")["max_len"] == M.FUSE_STR
    assert sh("past-4096-byte-string")["max_len"] == M.FUSE_STR + 1
    assert sh("past-4096-records")["records"] > M.FUSE_RECORDS and sh("past-4096-records")["dict"]["name"] == 3
    for n in (63, 64, 65, 255, 256, 257, 2048):
        s = sh(f"local-{n}")
        assert s["dict"]["name"] == n and s["pairs"] > M.FUSE_PAIRS and max(s["dict"].values()) <= M.LOCAL_STRINGS
    assert sh("global-2049")["dict"]["name"] == M.LOCAL_STRINGS + 1
    assert sh("global-2304")["dict"]["name"] == 2304 and sh("global-2304")["dict"]["annv"] == 2561
    assert (sh("patterns-64")["max_list"], sh("patterns-65")["max_list"]) == (64, 65)
    assert sh("patterns-64")["pat_bytes"] <= M.PAT_LDS and sh("patterns-65")["pat_bytes"] <= M.PAT_LDS
    assert sh("patterns-4096-bytes")["pat_bytes"] == M.PAT_LDS and sh("patterns-4096-bytes")["max_list"] == 64
    assert sh("patterns-4097-bytes")["pat_bytes"] == M.PAT_LDS + 1
    docs = M.regime_case("strings-long-names")[3]
    assert min(len(d["metadata"]["name"]) for d in docs) >= 200 and max(len(d["metadata"]["name"]) for d in docs) <= 253
    vb = M.block_bytes([v for d in M.regime_case("strings-long-values")[3] for v in d["metadata"]["annotations"].values()])
    assert vb[0] <= M.STR_LDS < min(vb[1:]) and len(vb) == 3


def test_every_pattern_class_is_in_the_lists():
    """A list of 17 or more patterns holds every record class of patclass.hpp."""
    pl = M.pattern_list(40, M.ann_values_of(50), 0, True)
    cls = set()
    for g in pl:
        stars, q = g.count("*"), "?" in g
        cls.add("any" if g == "*" else "empty" if g == "" else "exact" if not q and not stars else
                "prefix" if not q and stars == 1 and g.endswith("*") else
                "suffix" if not q and stars == 1 and g.startswith("*") else
                "contains" if not q and stars == 2 and g.startswith("*") and g.endswith("*") else
                "nonempty" if g.count("?") == 1 and stars + 1 == len(g) else "glob")
    assert cls == {"any", "empty", "exact", "prefix", "suffix", "contains", "nonempty", "glob"}
    assert {"**", "?*", "*?*", "?", "??"} <= set(pl)
    assert any(ord(c) > 127 for g in pl for c in g)  # non-ASCII in the patterns themselves


def test_matches_reproduces_match_rd_vectors():
    """pkg/engine/utils/utils_test.go MatchesResourceDescription vectors: the ones without a label
    selector are inside the restated subset."""
    inside = [c for c in MRD if M.in_subset({"match": c["match"], "exclude": c["exclude"]})]
    assert len(MRD) == 8 and len(inside) == 5
    for c in inside:
        assert M.matches({"match": c["match"], "exclude": c["exclude"]}, c["resource"]) == c["matched"], c["name"]
