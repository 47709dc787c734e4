"""Row fingerprints on the device: kpe_fetch_row_fingerprints, kpe_fingerprints_keep / _load / _fetch /
_drop and kpe_changed_rows_fp against their host twins over the matrix kpe_fetch returns and the words
kpe_fetch_cv_masks returns. Exact integer comparisons: the matrices themselves are pinned to the
oracle by the parity suites; these tests pin the fingerprints to the matrices.

Shapes: the smallest at which each mechanism can go wrong. A block of the kernel takes groups of
clamp(4096 / R, 1, 1024) whole rows on at most 2048 blocks and reads them with 16-byte loads from the
group's first byte rounded down to 16: N = 63 / 64 / 65 around a wave, 4097 past the groups of R = 1
and R = 3, 20000 rows of 204 rules are 1000 groups; R = 15 / 16+ switches between one and two row
registers per lane; a window starting at row 1 or N - 1 starts off the 16-byte grid. The program
pairs and corpora are those of tests/test_gpu_delta.py."""
import numpy as np
import pytest

import kyverno_amd as K
from kyverno_amd._lib import load
from tests.test_gpu_delta import pair

pytestmark = pytest.mark.gpu

FAIL, ERROR, SKIP = 2, 4, 5
KPE_E_STATE = 5
U = np.uint64
SENTINEL = U(0xDEADBEEFDEADBEEF)


@pytest.fixture(scope="module")
def engine():
    return K.Engine(ordinal=0)


def program(name):
    """R -> a real program with that many rules, its synth seed and mix."""
    cfg, side = {"r1": ("r1-r1", 1), "r3": ("r3-r3", 1), "r6": ("r3-r6", 1), "r15": ("r18-r15", 1),
                 "r18": ("r18-r15", 0), "r204": ("r204-r204", 1)}[name]
    p = pair(cfg)
    ps = p[side]
    assert ps.num_rules == int(name[1:])
    return ps, p[2], p[3]


def salts_of(seed, R):
    return np.random.default_rng(seed).integers(1, 1 << 63, size=R, dtype=np.uint64) * U(2) + U(1)


def evaluated(engine, ps, seed, mix, n, masks=True):
    """(corpus, its matrix, its raw cv mask words or None) after an evaluation of ps."""
    corpus = K.Corpus(K.synth_resources(seed, n, mix=mix)).upload(engine.device)
    assert corpus.n == n
    engine.evaluate_async(ps, corpus, masks=masks)
    v, _, _ = engine.fetch(ps, corpus)
    return corpus, v, (engine.cv_masks(ps, corpus, raw=True) if masks else None)


SIZES = (1, 63, 64, 65, 4097, 20000)
PROGRAMS = ("r1", "r3", "r6", "r15", "r18", "r204")


@pytest.mark.parametrize("name", PROGRAMS)
@pytest.mark.parametrize("n", SIZES)
def test_row_fingerprints_match_the_host_twin(engine, name, n):
    ps, seed, mix = program(name)
    R = ps.num_rules
    corpus, v, cvm = evaluated(engine, ps, seed, mix, n)
    default = K.rule_salts(ps)
    own, own_msg = salts_of(n + R, R), salts_of(n + R + 1, R)
    saw_masks = False
    for salts, msg_salts in ((None, None), (own, own_msg), (None, own_msg)):
        host_salts = default if salts is None else salts
        for msg_codes in [0, K.MESSAGE_CODES] + [1 << b for b in range(8)]:
            for masks in (False, True):
                want = K.row_fingerprints(v, host_salts, msg_salts=msg_salts, msg_codes=msg_codes,
                                          cv_masks=cvm if masks else None)
                got = engine.row_fingerprints(ps, corpus, salts=salts, msg_salts=msg_salts, msg_codes=msg_codes,
                                              masks=masks)
                assert got.dtype == np.uint64 and got.shape == (n,)
                assert np.array_equal(got, want), (msg_codes, masks, np.flatnonzero(got != want)[:8].tolist())
        with_m = K.row_fingerprints(v, host_salts, msg_salts=msg_salts, cv_masks=cvm)
        saw_masks |= not np.array_equal(with_m, K.row_fingerprints(v, host_salts, msg_salts=msg_salts))
        # windows: off the 16-byte grid, the last row, nothing
        for row0 in sorted({0, 1, n - 1} & set(range(n))):
            for nrows in sorted({n - row0, 1}):
                got = engine.row_fingerprints(ps, corpus, salts=salts, msg_salts=msg_salts, masks=True, row0=row0,
                                              nrows=nrows)
                assert np.array_equal(got, with_m[row0:row0 + nrows]), (row0, nrows)
        assert engine.row_fingerprints(ps, corpus, row0=n, nrows=0).shape == (0,)
    assert np.array_equal(engine.row_fingerprints(ps, corpus) == 0, (v == 0).all(axis=1))  # no report: 0
    print(f"{name} n={n}: rows with a response {int((v != 0).any(axis=1).sum())}, "
          f"FAIL cells with a mask word {int(((v == FAIL) & (cvm != 0)).sum())}")
    if n >= 4097 and name in ("r3", "r6", "r15", "r18"):
        assert saw_masks  # podSecurity FAIL cells carry mask words: the flag is not vacuous
    # a caller's buffer past the window is not written
    buf = np.full(n + 4, SENTINEL, dtype=U)
    assert load().kpe_fetch_row_fingerprints(engine.device.h, ps.h, corpus.h, None, None, 0, 0, 0, n, buf.ctypes.data) == 0
    assert np.array_equal(buf[:n], K.row_fingerprints(v, default, msg_codes=0)) and (buf[n:] == SENTINEL).all()


def test_masks_flag_needs_an_evaluation_with_masks(engine):
    ps, seed, mix = program("r3")
    corpus, v, _ = evaluated(engine, ps, seed, mix, 64, masks=False)
    assert np.array_equal(engine.row_fingerprints(ps, corpus), K.row_fingerprints(v, K.rule_salts(ps)))
    for q in (lambda: engine.row_fingerprints(ps, corpus, masks=True),
              lambda: engine.keep_fingerprints(ps, corpus, masks=True)):
        with pytest.raises(K.KpeError) as e:
            q()
        assert e.value.status == KPE_E_STATE
    assert engine.kept_fingerprints(corpus) is None
    engine.keep_fingerprints(ps, corpus)
    with pytest.raises(K.KpeError) as e:
        engine.changed_rows_fp(ps, corpus, masks=True)
    assert e.value.status == KPE_E_STATE
    assert engine.changed_rows_fp(ps, corpus)[3] == 0


EDITS = [("r1-r1", 4097), ("r3-r3", 1366), ("r3-r6", 683), ("r6-r3", 683), ("r18-r15", 228), ("r18-r15", 4096),
         ("r204-r204", 2000), ("r204-r204", 20000)]
# changed rows of the edits, as tests/test_gpu_delta.py knows them from the oracle's matrices
KNOWN = {("r1-r1", 4097): 126, ("r3-r3", 1366): 65, ("r3-r6", 683): 57, ("r6-r3", 683): 57, ("r18-r15", 228): 166,
         ("r18-r15", 4096): 2962, ("r204-r204", 2000): 67}


@pytest.mark.parametrize("masks", (False, True), ids=("verdicts", "masks"))
@pytest.mark.parametrize("cfg,n", EDITS, ids=[f"{c}-{n}" for c, n in EDITS])
def test_changed_rows_fp_after_a_policy_edit(engine, cfg, n, masks):
    psa, psb, seed, mix, (Ro, Rn) = pair(cfg)
    corpus, va, ma = evaluated(engine, psa, seed, mix, n, masks=masks)
    engine.keep_results(psa, corpus)
    engine.keep_fingerprints(psa, corpus, masks=masks)
    engine.evaluate_async(psb, corpus, masks=masks)
    vb, _, _ = engine.fetch(psb, corpus)
    mb = engine.cv_masks(psb, corpus, raw=True) if masks else None
    fpa = K.row_fingerprints(va, K.rule_salts(psa), cv_masks=ma)
    fpb = K.row_fingerprints(vb, K.rule_salts(psb), cv_masks=mb)
    want = K.changed_fingerprints(fpa, fpb)
    rows, vr, fps, total = engine.changed_rows_fp(psb, corpus, masks=masks)
    print(f"changed rows: device {total}, twin {want.size} of {n}")
    assert total == want.size and rows.dtype == np.uint64 and fps.dtype == np.uint64
    assert np.array_equal(rows, want), np.setxor1d(rows, want)[:8].tolist()
    assert vr.shape == (total, Rn) and np.array_equal(vr, vb[want.astype(np.int64)])
    assert np.array_equal(fps, fpb[want.astype(np.int64)])
    if not masks:  # the exact form, from the kept matrix of A on the same corpus
        exact, _, exact_total = engine.changed_rows(psb, corpus)
        assert exact_total == total and np.array_equal(rows, exact)
        if (cfg, n) in KNOWN:
            assert total == KNOWN[(cfg, n)]
    assert 0 < total < n
    assert np.array_equal(engine.kept_fingerprints(corpus), fpa)  # the kept ones are not modified
    # count only, a cap of half the total, a generous cap
    L = load()
    h = (engine.device.h, psb.h, corpus.h, None, None, K.MESSAGE_CODES, K.FP_MASKS if masks else 0)
    assert L.kpe_changed_rows_fp(*h, None, None, None, 0) == total
    cap = total // 2
    r2 = np.full(total + 8, SENTINEL, dtype=U)
    f2 = np.full(total + 8, SENTINEL, dtype=U)
    v2 = np.full((total + 8, Rn), 0xA5, dtype=np.uint8)
    assert L.kpe_changed_rows_fp(*h, r2.ctypes.data, v2.ctypes.data, f2.ctypes.data, cap) == total
    assert np.array_equal(r2[:cap], rows[:cap]) and np.array_equal(v2[:cap], vr[:cap]) and np.array_equal(f2[:cap], fps[:cap])
    assert (r2[cap:] == SENTINEL).all() and (f2[cap:] == SENTINEL).all() and (v2[cap:] == 0xA5).all()
    r2[:] = SENTINEL
    assert L.kpe_changed_rows_fp(*h, r2.ctypes.data, None, None, 1 << 40) == total
    assert np.array_equal(r2[:total], rows) and (r2[total:] == SENTINEL).all()
    r3, v3, f3, t3 = engine.changed_rows_fp(psb, corpus, masks=masks, cap=cap, with_verdicts=False)
    assert t3 == total and np.array_equal(r3, rows[:cap]) and v3.shape == (0, Rn) and np.array_equal(f3, fps[:cap])
    # moving on: keep B's, nothing differs; the kept matrix is still A's
    engine.keep_fingerprints(psb, corpus, masks=masks)
    assert engine.changed_rows_fp(psb, corpus, masks=masks)[3] == 0
    assert np.array_equal(engine.kept_fingerprints(corpus), fpb)
    assert engine.kept_rule_names(corpus) == psa.rule_names


def test_message_salts_do_the_job_of_always(engine):
    """An edited policy under an equal verdict: its rules' msg_salts bumped, the rows with a FAIL /
    ERROR / SKIP cell in its columns change, as `always` makes them for the kept matrix."""
    psa, psb, seed, mix, _ = pair("r18-r15")
    corpus, va, _ = evaluated(engine, psa, seed, mix, 228, masks=False)
    engine.keep_results(psa, corpus)
    engine.keep_fingerprints(psa, corpus)
    engine.evaluate_async(psb, corpus)
    edited = np.array([nm.split("/", 1)[0] == "pol-baseline-v1-22" for nm in psb.rule_names])
    assert edited.any()
    msg = K.rule_salts(psb)
    msg[edited] ^= U(1)
    rows, _, _, total = engine.changed_rows_fp(psb, corpus, msg_salts=msg)
    exact, _, exact_total = engine.changed_rows(psb, corpus, always=np.where(edited, K.MESSAGE_CODES, 0).astype(np.uint8))
    assert total == exact_total and np.array_equal(rows, exact)
    assert total >= engine.changed_rows_fp(psb, corpus)[3] > 0


def test_load_fetch_and_drop(engine):
    ps, seed, mix = program("r18")
    nd = K.synth_resources(seed, 4097, mix=mix)
    corpus = K.Corpus(nd).upload(engine.device)
    engine.evaluate_async(ps, corpus)
    assert engine.kept_fingerprints(corpus) is None and load().kpe_fingerprints_kept(corpus.h) == 0
    with pytest.raises(K.KpeError) as e:
        engine.changed_rows_fp(ps, corpus)
    assert e.value.status == KPE_E_STATE
    engine.keep_fingerprints(ps, corpus)
    stored = engine.kept_fingerprints(corpus)
    assert np.array_equal(stored, engine.row_fingerprints(ps, corpus)) and (stored != 0).any()
    assert np.array_equal(engine.kept_fingerprints(corpus, 1, 4096), stored[1:])
    assert np.array_equal(engine.kept_fingerprints(corpus, 4096, 1), stored[4096:])
    # a freshly uploaded copy of the corpus (a restart): the stored fingerprints, the same program
    fresh = K.Corpus(nd).upload(engine.device)
    assert engine.kept_fingerprints(fresh) is None
    engine.load_fingerprints(fresh, stored)
    assert np.array_equal(engine.kept_fingerprints(fresh), stored)
    engine.evaluate_async(ps, fresh)
    rows, vr, fps, total = engine.changed_rows_fp(ps, fresh)
    assert total == 0 and rows.size == 0 and vr.shape == (0, ps.num_rules) and fps.size == 0
    for i in (0, 1234, 4096):
        altered = stored.copy()
        altered[i] ^= U(1) << U(63)
        engine.load_fingerprints(fresh, altered)
        rows, vr, fps, total = engine.changed_rows_fp(ps, fresh)
        assert total == 1 and rows.tolist() == [i] and fps.tolist() == [int(stored[i])]
        assert np.array_equal(vr[0], engine.fetch(ps, fresh)[0][i])
    with pytest.raises(K.KpeError):
        engine.load_fingerprints(fresh, stored[:-1])  # one per row
    # independent of the kept matrix; drop; a re-upload drops too
    engine.keep_results(ps, fresh)
    engine.drop_results(fresh)
    assert engine.kept_fingerprints(fresh) is not None
    engine.keep_results(ps, fresh)
    engine.drop_fingerprints(fresh)
    assert engine.kept_fingerprints(fresh) is None and engine.kept_rule_names(fresh) == ps.rule_names
    with pytest.raises(K.KpeError) as e:
        engine.changed_rows_fp(ps, fresh)
    assert e.value.status == KPE_E_STATE
    assert engine.kept_fingerprints(corpus) is not None
    corpus.upload(engine.device)
    assert engine.kept_fingerprints(corpus) is None


def same(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[i], b[i]) for i in a)


def test_resident_scanner_with_fingerprints_returns_the_default_scanners_rows(engine):
    psa, psb, seed, mix, _ = pair("r18-r15")
    nd = K.synth_resources(seed, 228, mix=mix)
    edited_pols = {"pol-baseline-v1-22"}  # the policy whose version changed
    by_matrix = K.ResidentScanner(engine, nd)
    by_fp = K.ResidentScanner(engine, nd, keep="fingerprints")
    assert by_fp.fingerprints() is None
    saved = None
    outs = []
    for k, (ps, ed) in enumerate(((psa, ()), (psb, edited_pols), (psb, ()), (psa, ()))):
        want = by_matrix.apply(ps, edited=ed)
        got = by_fp.apply(ps, edited=ed)
        assert same(got, want) and by_fp.last_stats == by_matrix.last_stats, k
        outs.append(want)
        if k == 0:
            saved = (by_fp.fingerprints(), dict(by_fp.edits))
    assert len(outs[0]) > 0 and 0 < len(outs[1]) < 228 and outs[2] == {} and len(outs[3]) > 0
    # restored over a re-uploaded corpus (a new scanner): only the real changes on its first apply
    again = K.ResidentScanner(engine, nd, keep="fingerprints", fingerprints=saved[0], edits=saved[1])
    assert same(again.apply(psb, edited=edited_pols), outs[1])
    assert again.apply(psb) == {}
    unchanged = K.ResidentScanner(engine, nd, keep="fingerprints", fingerprints=saved[0], edits=saved[1])
    assert unchanged.apply(psa) == {} and unchanged.last_stats == {"rows": 228, "changed": 0}
    with pytest.raises(ValueError):
        K.ResidentScanner(engine, nd, fingerprints=saved[0])
    with pytest.raises(ValueError):
        K.ResidentScanner(engine, nd, keep="bytes")
