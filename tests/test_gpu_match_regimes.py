"""The match predicates in every placement the binding can choose (kpe_api.cpp ensure_binding):
fused into the scan prologue, an LDS bitset filled by kpe_pred_kernel, a bitset in HBM; and
kpe_pred_kernel's own branches (strings staged in LDS or read from memory, pattern records
staged or not). Each case of tests/match_ref.py REGIMES is built for one regime and asserts
that it reached it; the engine's matrix must equal the oracle's, and (cell != 0) the plain
reference `matches` (pinned on the CPU by tests/test_match_ref.py).

What the `kpe bind:` line of KPE_DEBUG confirms: fused or not (npairs, the pair count itself),
how many predicates went through kpe_pred_kernel and over how many 256-string blocks
(pred_jobs, pred_xblocks), and how many bitset words are LDS-resident (blob), which separates
local from global. What is derived in the test from the documented constants, because the
bind line does not print it: which fuse condition failed, and the kernel's staging branches
(block bytes against 16384, pattern bytes against 4096, list length against 64)."""
import re

import numpy as np
import pytest

import kyverno_amd as K
from tests import match_ref as M


def bind_line(err):
    lines = [ln for ln in err.splitlines() if ln.startswith("kpe bind:")]
    assert lines, err[-2000:]
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", lines[-1])}


def local_words(sh, dicts_local):
    """Bitset words of the predicates over dictionaries of at most 2048 strings, rounded to 4 as
    the blob is (derived: ceil(n / 64) * 2 + 2 words per predicate)."""
    w = sum((sh["dict"][d] + 63) // 64 * 2 + 2 for d, _ in sh["preds"] if d in dicts_local)
    return max(4, (w + 3) & ~3)


def staging(name, sh, docs):
    """The kpe_pred_kernel branches a case is built for, from its own inputs (derived)."""
    pat_lds = sh["pat_bytes"] <= M.PAT_LDS  # and per job: its list has at most 64 records
    if name in ("patterns-64", "patterns-4096-bytes"):
        assert pat_lds and sh["max_list"] == M.PAT_RECORDS
    if name == "patterns-65":
        assert pat_lds and sh["max_list"] == M.PAT_RECORDS + 1  # that job reads its records from memory
    if name == "patterns-4097-bytes":
        assert not pat_lds and sh["max_list"] == M.PAT_RECORDS
    if name == "past-4096-records":
        assert sh["records"] > M.FUSE_RECORDS and not pat_lds
    if name in ("strings-16384-bytes", "strings-16385-bytes"):
        assert M.block_bytes([d["metadata"]["name"] for d in docs]) == [int(name.split("-")[1])]
    if name == "strings-long-names":
        nb = M.block_bytes([d["metadata"]["name"] for d in docs])
        assert nb[0] > M.STR_LDS >= nb[1]  # 256 names of 200 bytes or more, then a short tail block
    if name == "strings-long-values":
        vb = M.block_bytes([v for d in docs for v in d["metadata"]["annotations"].values()])
        assert vb[0] <= M.STR_LDS < min(vb[1:])  # the first block stages, the others do not


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(M.REGIMES))
def test_match_regime(oracle, monkeypatch, capfd, name):
    """The largest annotation value is 4988 bytes and the flattener takes it whole: it has no
    limit on a string's length, so no case here leaves an undecided row."""
    regime, pols, nd, docs, sh = M.regime_case(name)
    monkeypatch.setenv("KPE_DEBUG", "1")
    eng = K.Engine(ordinal=0)
    capfd.readouterr()
    v, _, _ = eng.evaluate(K.PolicySet(pols), K.Corpus(nd))
    b = bind_line(capfd.readouterr().err)
    print(name, b, {k: sh[k] for k in ("dict", "pairs", "records", "pat_bytes", "max_len", "max_list", "fuse_words")})

    ref = oracle.validate(pols, nd, nthreads=8)
    assert v.shape == ref.shape
    bad = np.argwhere(v != ref)
    assert bad.size == 0, f"{len(bad)} cells differ from the oracle, first {bad[:5].tolist()} " \
                          f"gpu={[int(v[i, j]) for i, j in bad[:5]]} ref={[int(ref[i, j]) for i, j in bad[:5]]}"
    want = np.array(M.match_matrix(pols, docs), dtype=bool)
    bad = np.argwhere((v != 0) != want)
    assert bad.size == 0, f"{len(bad)} cells differ from matches(), first {bad[:5].tolist()}"

    # ---- the case reached the regime it was built for ----
    size = sh["dict"]
    used = {d for d, _ in sh["preds"]}
    small = {d for d in used if size[d] <= M.LOCAL_STRINGS}
    # derived: the local predicates are fused when every fuse condition holds
    fusable = (bool(small) and sh["pairs"] <= M.FUSE_PAIRS and sh["max_len"] <= M.FUSE_STR
               and sh["records"] <= M.FUSE_RECORDS and sh["fuse_words"] <= M.FUSE_WORDS)
    # a predicate over an empty dictionary has no job; fused ones have none either
    jobs = [d for d, _ in sh["preds"] if size[d] and not (fusable and d in small)]
    # read from the bind line
    assert b["npairs"] == (sh["pairs"] if fusable else 0)
    assert (b["fuse_words"] > 0) == fusable and b["fuse_words"] <= M.FUSE_WORDS
    assert b["pred_jobs"] == len(jobs)
    assert b["pred_xblocks"] == max(((size[d] + 255) // 256 for d in jobs), default=0)
    assert b["blob"] == local_words(sh, small)  # every small dictionary's bitset is in LDS, no other
    if regime == "fused":
        assert fusable and small == used and not jobs
    elif regime == "local":
        assert not fusable and small == used
    else:
        assert small != used
        # the small dictionaries beside the large one: through the kernel too (2049), or fused (2304)
        assert fusable == (name == "global-2304")
        # domains with different block counts in one launch: the shorter job's blocks past its
        # dictionary return at once
        assert len({(size[d] + 255) // 256 for d in jobs}) >= 2
    staging(name, sh, docs)
