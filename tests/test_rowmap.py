"""scan.RowMap, the bookkeeping of a resident corpus under resource churn (no GPU, no library): a
scripted sequence of upserts (new, replaced, hash-equal), deletes and compactions against a plain
dict model. Logical rows are stable, a deleted row's index is never reused, compaction is due at
both thresholds, and per-segment row lists translate to logical rows with retired rows dropped."""
import random

import pytest

from kyverno_amd.scan import NO_HASH, RowMap


class Model:
    """key -> (logical row, hash); rows handed out once, in order of first appearance."""

    def __init__(self, keys, hashes):
        self.rows = {k: (i, h) for i, (k, h) in enumerate(zip(keys, hashes))}
        self.next = len(keys)
        self.ever = set(range(len(keys)))

    def update(self, upserts, deletes):
        dele = {self.rows[k][0] for k in deletes if k in self.rows}
        flat, skipped = [], 0
        last = {k: i for i, (k, _) in enumerate(upserts)}
        for i, (k, h) in enumerate(upserts):
            if last[k] != i or (k in self.rows and self.rows[k][0] in dele):
                continue
            if k in self.rows:
                if self.rows[k][1] == h and h != NO_HASH:
                    skipped += 1
                    continue
                self.rows[k] = (self.rows[k][0], h)
            else:
                self.rows[k] = (self.next, h)
                self.ever.add(self.next)
                self.next += 1
            flat.append(self.rows[k][0])
        for k in [k for k, (l, _) in self.rows.items() if l in dele]:
            del self.rows[k]
        return flat, skipped, sorted(dele)


def check(m: RowMap, model: Model):
    live = sorted(l for l, _ in model.rows.values())
    assert m.live() == live
    assert m.n_logical == model.next and m.n_live == len(live)
    for k, (l, h) in model.rows.items():
        assert m.row_of(k) == l and m.hashes[l] == h
        s, r = m.loc[l]
        assert m.back[s][r] == l
    for l in model.ever - set(live):
        assert m.loc[l] is None and m.row_of(l) is None  # never reused
    # the inverse maps hold exactly the live rows, each once
    seen = [l for b in m.back for l in b if l >= 0]
    assert sorted(seen) == live
    assert m.retired == sum(1 for b in m.back for l in b if l < 0) == m.n_physical - m.n_live


def test_scripted_churn_against_a_dict():
    rng = random.Random(5)
    keys = [("uid", f"u{i}") for i in range(50)]
    hashes = [f"h{i}" for i in range(50)]
    m, model = RowMap(keys, hashes, max_segments=1000, max_retired=2.0), Model(keys, hashes)
    check(m, model)
    fresh = 50
    for step in range(60):
        livek = sorted(model.rows)
        ups = []
        for k in rng.sample(livek, min(len(livek), rng.randrange(0, 6))):  # replaced
            ups.append((k, f"h{step}x{k[1]}"))
        for k in rng.sample(livek, min(len(livek), rng.randrange(0, 4))):  # hash-equal
            ups.append((k, model.rows[k][1]))
        for _ in range(rng.randrange(0, 3)):  # new
            ups.append((("uid", f"u{fresh}"), f"h{fresh}"))
            fresh += 1
        if step % 7 == 0 and ups:
            ups.append((ups[0][0], "twice"))  # the same key twice: its last occurrence counts
        rng.shuffle(ups)
        dels = rng.sample(livek, min(len(livek), rng.randrange(0, 3)))
        if step % 5 == 0:
            dels.append(("uid", "never-existed"))
        by_row = step % 2 == 1  # deletes by logical row as well as by key
        plan = m.plan(ups, [model.rows[k][0] if by_row and k in model.rows else k for k in dels])
        before = {k: m.loc[l] for k, (l, _) in model.rows.items()}
        flat, skipped, dele = model.update(ups, dels)
        assert plan["skipped"] == skipped and plan["deletes"] == dele
        nseg = m.segments
        seg, rows, retire = m.commit(plan)
        assert rows == flat
        assert (seg is None) == (not flat) and m.segments == nseg + (1 if flat else 0)
        for j, l in enumerate(rows):
            assert m.loc[l] == (seg, j)
        # what is retired: the old place of every replaced resource, the place of every deleted one
        want = {}
        for i, l in plan["items"]:
            if l is not None:
                want.setdefault(before[ups[i][0]][0], set()).add(before[ups[i][0]][1])
        for k, p in before.items():
            if k not in model.rows:
                want.setdefault(p[0], set()).add(p[1])
        assert {s: set(r) for s, r in retire.items()} == want
        check(m, model)
        if step % 13 == 12:
            live = m.compact()
            assert live == m.live() and m.segments == 1 and m.retired == 0
            assert [m.loc[l] for l in live] == [(0, j) for j in range(len(live))]
            check(m, model)


def test_stable_rows_and_no_reuse():
    m = RowMap(["a", "b", "c"], ["1", "2", "3"])
    seg, rows, retire = m.commit(m.plan([("b", "2x"), ("d", "4")], deletes=["a"]))
    assert (seg, rows, retire) == (1, [1, 3], {0: [1, 0]})
    assert m.loc == [None, (1, 0), (0, 2), (1, 1)]
    # "a" comes back: a new resource, a new row; row 0 stays dead
    seg, rows, _ = m.commit(m.plan([("a", "1")]))
    assert rows == [4] and m.loc[0] is None and m.row_of("a") == 4 and m.row_of(0) is None
    # deleted and offered in one call: deleted
    plan = m.plan([("c", "3x")], deletes=["c"])
    assert plan["items"] == [] and plan["deletes"] == [2]
    # NO_HASH never compares equal: such a row is flattened every time
    m2 = RowMap(["x"], [NO_HASH])
    assert m2.plan([("x", NO_HASH)])["items"] == [(0, 0)]
    with pytest.raises(ValueError):
        RowMap(["a"], [])


def test_compaction_thresholds():
    # past max_segments segments
    m = RowMap([f"k{i}" for i in range(100)], ["h"] * 100, max_segments=3, max_retired=0.9)
    for s in range(2):
        m.commit(m.plan([(f"n{s}", "h")]))
        assert not m.needs_compaction()  # 2, then 3 segments
    m.commit(m.plan([("n2", "h")]))
    assert m.segments == 4 and m.needs_compaction()
    m.compact()
    assert m.segments == 1 and not m.needs_compaction()
    # more than a quarter of the physical rows retired
    m = RowMap([f"k{i}" for i in range(12)], ["h"] * 12, max_segments=16, max_retired=0.25)
    m.commit(m.plan([], deletes=[0, 1, 2]))
    assert m.retired == 3 and m.n_physical == 12 and not m.needs_compaction()  # exactly a quarter
    m.commit(m.plan([], deletes=[3]))
    assert m.needs_compaction()  # 4 of 12
    m.compact()
    assert m.n_physical == 8 and m.live() == list(range(4, 12)) and not m.needs_compaction()
    # replacing retires too: 2 of 6 + 2
    m = RowMap(list("abcdef"), ["h"] * 6, max_retired=0.25)
    m.commit(m.plan([("a", "x"), ("b", "x")]))
    assert m.retired == 2 and m.n_physical == 8 and not m.needs_compaction()
    m.commit(m.plan([("c", "x")]))
    assert m.retired == 3 and m.n_physical == 9 and m.needs_compaction()


def test_translate_and_group():
    m = RowMap(list("abcde"), ["h"] * 5)
    m.commit(m.plan([("b", "x"), ("f", "y")], deletes=["d"]))  # b -> (1, 0), f = row 5 -> (1, 1)
    # segment 0's list with the retired rows 1 (replaced) and 3 (deleted) dropped; positions kept
    assert m.translate(0, [0, 1, 2, 3, 4]) == [(0, 0), (2, 2), (4, 4)]
    assert m.translate(1, [1, 0]) == [(0, 5), (1, 1)]
    assert m.translate(0, []) == []
    assert m.group([5, 0, 1, 3, 4]) == {1: [(5, 1), (1, 0)], 0: [(0, 0), (4, 4)]}
    m.compact()  # live: 0 1 2 4 5
    assert m.translate(0, [0, 1, 2, 3, 4]) == [(0, 0), (1, 1), (2, 2), (3, 4), (4, 5)]
