"""A plain reference for resource matching, and corpus / policy generators with explicit knobs.

`glob` is go-wildcard over Python `str` (code points, so a rune is one element): `*` any run,
`?` exactly one code point, the empty pattern only the empty text. `matches` restates match /
exclude (pkg/engine/utils/match.go:52-300, as oracle/engine.hpp block_errors does) for the
subset the generators use: any / all blocks of resources.{kinds ("*" or an exact kind), name,
names, namespaces, annotations} and exclude with the same fields.

`case(...)` builds (policies, ndjson, docs) whose dictionaries have exactly the sizes asked for
(every name / namespace / annotation key / value carries a counter suffix), so a test chooses
the predicate placement the engine takes at bind time (kpe_api.cpp ensure_binding) instead of
taking what a synthetic corpus happens to give. `shapes(...)` derives, from the documented
constants alone, the numbers that placement depends on. Nothing here imports the engine.
"""
import json

# ---- the reference -----------------------------------------------------------------------


def glob(pattern, text):
    """Rune-wise dynamic programme. After each pattern character the row is the set of j for
    which the pattern so far matches text[:j], kept sparse: a list of such j, or after a `*` the
    least one (`*` makes every later j hold as well)."""
    if pattern == "":
        return text == ""
    n = len(text)
    row, least = [0], None  # exactly one of the two forms is in use: least is None <=> the list is
    for pc in pattern:
        if pc == "*":
            if least is None:
                if not row:
                    return False
                least = min(row)
        elif least is not None:  # every j >= least holds: one more rune from each of them
            row = [j + 1 for j in range(least, n) if pc == "?" or text[j] == pc]
            least = None
        else:
            row = [j + 1 for j in row if j < n and (pc == "?" or text[j] == pc)]
    return least is not None or n in row


_memo = {}


def _glob(p, t):  # the tables repeat a few thousand (pattern, string) pairs over many rows
    k = (p, t)
    r = _memo.get(k)
    if r is None:
        r = _memo[k] = glob(p, t)
    return r


def _kind_ok(kinds, kind):
    return any(k == "*" or k == kind for k in kinds)


def _block(rd, res):
    """One resource description against a resource: every field it names must hold."""
    md = res.get("metadata") or {}
    kind = res.get("kind", "")
    name = md.get("name") or md.get("generateName") or ""
    ns = md.get("name", "") if kind == "Namespace" else md.get("namespace", "")
    if rd.get("kinds") and not _kind_ok(rd["kinds"], kind):
        return False
    if rd.get("name") and not _glob(rd["name"], name):
        return False
    if rd.get("names") and not any(_glob(p, name) for p in rd["names"]):
        return False
    if rd.get("namespaces") and not any(_glob(p, ns) for p in rd["namespaces"]):
        return False
    ann = md.get("annotations") or {}
    for pk, pv in (rd.get("annotations") or {}).items():  # every pair matched by some annotation
        if not any(_glob(pk, k) and _glob(pv, v) for k, v in ann.items()):
            return False
    return True


FIELDS = {"kinds", "name", "names", "namespaces", "annotations"}


def _null_selector(s):
    return s is None or (isinstance(s, dict) and all(v is None for v in s.values()))


def in_subset(rule):
    """Whether `matches` restates this rule's match / exclude (a selector whose members are all
    null selects everything and is read as absent)."""
    def ok_filter(f):
        if set(f) - {"resources"}:
            return False
        rd = f.get("resources") or {}
        rest = {k for k in rd if not (k in ("selector", "namespaceSelector") and _null_selector(rd[k]))}
        if not rest or rest - FIELDS:
            return False
        return all(k == "*" or not set(k) & set("*?/.") for k in rd.get("kinds") or [])

    def ok_block(b):
        if not b:
            return True
        if "any" in b or "all" in b:
            return not set(b) - {"any", "all"} and all(ok_filter(f) for f in (b.get("any") or []) + (b.get("all") or []))
        return ok_filter(b)

    return bool(rule.get("match")) and ok_block(rule["match"]) and ok_block(rule.get("exclude"))


def _filters(block):
    """(any, all) filter lists of a match / exclude block; the legacy form is one `all` filter."""
    if not block:
        return [], []
    if block.get("any"):
        return [f.get("resources") or {} for f in block["any"]], []
    if block.get("all"):
        return [], [f.get("resources") or {} for f in block["all"]]
    return [], [block.get("resources") or {}]


def matches(rule, res):
    many, mall = _filters(rule.get("match"))
    if many:
        hit = any(_block(rd, res) for rd in many)
    else:
        hit = bool(mall) and all(_block(rd, res) for rd in mall)
    if not hit:
        return False
    xany, xall = _filters(rule.get("exclude"))
    if xany:
        return not any(_block(rd, res) for rd in xany)
    if xall:
        return not all(_block(rd, res) for rd in xall)
    return True


def match_matrix(policies, docs):
    """bool [rows][rules] in the column order of single-kind policies (no autogen twin)."""
    rules = [r for p in policies for r in p["spec"]["rules"]]
    return [[matches(r, d) for r in rules] for d in docs]


# ---- generators ----------------------------------------------------------------------------
KIND = "Widget"  # a namespaced kind without autogen rules
WORDS = ["web", "db", "cache", "api", "job"]
# annotation values also carry 2-, 3- and 4-byte runes: `?` must step a rune, `*` must restart on one
RUNES = ["é", "本", "\U0001F600", "aé本", "本\U0001F600é"]


def _len_of(length, i):
    """A length knob: an int, a (lo, hi) range walked through by i, or a function of i."""
    if callable(length):
        return length(i)
    return length if isinstance(length, int) else length[0] + (i * 977) % (length[1] - length[0] + 1)


def _sized(stem, i, length):
    """`stem-xx..x<i>`: unique by the counter, padded to `length` characters when that is longer."""
    tail, length = str(i), _len_of(length, i)
    return stem + "-" + "x" * max(0, length - len(stem) - 1 - len(tail)) + tail


def names_of(n, length=0):
    return [_sized(WORDS[i % len(WORDS)], i, length) for i in range(n)]


def namespaces_of(n):
    return [f"ns-{WORDS[i % len(WORDS)]}-{i}" for i in range(n)]


def ann_keys_of(n):
    return [f"example.io/{WORDS[i % len(WORDS)]}-{i}" for i in range(n)]


def ann_values_of(n, length=0):
    """Values `<word><rune>-xx..x<i>` (every 4th `本<word>-...`), `length` characters or longer."""
    out = []
    for i in range(n):
        ln = _len_of(length, i)
        w, r = WORDS[i % len(WORDS)], RUNES[i % len(RUNES)]
        out.append(_sized("本" + w if i % 4 == 3 else w + r, i, ln))  # every 4th starts with a 3-byte rune
    return out


MATCH_ALL = ("*", "**", "?*", "*?*")


def _q_rune(s):
    k = next((i for i, c in enumerate(s) if ord(c) > 127), 1 if len(s) > 1 else 0)
    return s[:k] + "?" + s[k + 1:]


def pattern_list(k, strings, salt, with_all):
    """k distinct patterns over `strings`, cycling through every record class of patclass.hpp:
    exact, lit*, *lit, *lit*, the match-all forms, true globs, patterns that match nothing and the
    empty string. `with_all` keeps `*`, `**`, `?*` and `*?*` (then the list matches any non-empty
    string; rules with such a list are decided by their other fields)."""
    out = []

    def add(p):
        if p not in out and (with_all or p not in MATCH_ALL):
            out.append(p)

    j = 0
    while len(out) < (k - 1 if k >= 8 else k):
        s = strings[(salt * 7 + j * 13) % len(strings)]
        w = WORDS[(salt + j) % len(WORDS)]
        first = j < 20  # the first round has the broad forms (a fifth of the strings), later rounds narrow ones
        c = [s,                                   # exact
             w + "*" if first else s[:-1] + "*",  # lit*
             "*" + s[-2:],                        # *lit
             "*" + (s[1:-1] if len(s) > 3 else s) + "*",  # *lit*
             "*", "**", "?*", "*?*",
             s[:1] + "?" + s[2:],                 # a?b: one rune replaced by ?
             s[:1] + "*" + s[len(s) // 2] + "*" + s[-1:],  # a*b*c
             "?", "??",
             s[:2] + "?" * (len(s) - 2) if len(s) <= 40 else s[:2] + "*?" + s[-1:],
             _q_rune(s),                          # ? over a multi-byte rune where the string has one
             "*??" + s[1:],                       # two runes wanted before s[1:], one there: the glob's retry
                                                  # after `*` must step whole runes, or `??` eats one rune's bytes
             f"zzz-{salt}-{j}", f"*zzz{j}", f"{w}?zzz*",   # match nothing
             ""]
        add(c[j % len(c)] if j < 4 * len(c) else f"none-{salt}-{j}")
        j += 1
    if k >= 8:  # the last record of a long list decides a string of its own: an exact one no earlier pattern takes
        rest = [s for s in strings[:400] if s not in out and not any(_glob(p, s) for p in out)]
        out.append(rest[salt % len(rest)] if rest else f"last-{salt}")
    return out


def _rule(i, match, exclude=None):
    r = {"name": f"r{i}", "match": match, "validate": {"pattern": {"kind": "?*"}}}  # cannot fail: a cell != 0 <=> matched
    if exclude:
        r["exclude"] = exclude
    return r


def _policy(i, rule):
    return {"apiVersion": "kyverno.io/v1", "kind": "ClusterPolicy", "metadata": {"name": f"p{i}"},
            "spec": {"validationFailureAction": "Audit", "background": True, "rules": [rule]}}


def case(n_names=8, n_ns=3, n_annk=2, n_annv=4, name_len=0, annv_len=0, pats=4, ns_pats=2, n_rules=4,
         fields=("names", "namespaces", "annotations"), rows=None, extra_docs=(), pat_bytes=None, kinds=True,
         match_all=True):
    """(policies, ndjson bytes, docs). Row i takes name i % n_names, namespace i % n_ns and one or two
    annotations (key i % n_annk, value i % n_annv), so `rows` >= every knob gives dictionaries of exactly
    the knob sizes. Rule r uses one of four block shapes by r % 4 over the `fields` asked for; its
    `names` list has `pats` patterns, its `namespaces` list `ns_pats`. `pat_bytes` pads one
    never-matching exact name so that the program's pattern bytes (shapes()) are exactly that. Even rules
    keep the match-all patterns in their `names` list when other fields decide them (`match_all`)."""
    names, nss = names_of(n_names, name_len), namespaces_of(n_ns)
    aks, avs = ann_keys_of(n_annk), ann_values_of(n_annv, annv_len)
    rows = rows if rows is not None else max(n_names, n_ns, n_annk, n_annv)
    docs = []
    for i in range(rows):
        ann = {aks[i % n_annk]: avs[i % n_annv]}
        if i % 3 == 0 and aks[(i // 3 + 1) % n_annk] not in ann:  # values are first seen in index order
            ann[aks[(i // 3 + 1) % n_annk]] = avs[(i + 1) % n_annv]
        docs.append({"apiVersion": "example.io/v1", "kind": KIND,
                     "metadata": {"name": names[i % n_names], "namespace": nss[i % n_ns], "annotations": ann},
                     "spec": {"size": i % 7}})
    docs.extend(extra_docs)
    use = set(fields)
    pols = []
    for r in range(n_rules):
        rd = {}
        if kinds:
            rd["kinds"] = ["*"] if r % 2 else [KIND]
        if "names" in use:
            if r % 4 == 1 and pats == 1:
                rd["name"] = pattern_list(1, names, r, False)[0]
            else:
                rd["names"] = pattern_list(pats, names, r, with_all=match_all and r % 2 == 0 and len(use) > 1)
        rd2 = {}
        if "namespaces" in use:
            rd2["namespaces"] = pattern_list(ns_pats, nss, r + 3, False)
        if "annotations" in use:
            k, v = aks[r % n_annk], avs[(r * 3) % n_annv]
            kp = ["example.io/*", k, "*" + k[-3:], "example.io/?*-*", "*"][r % 5]
            vp = [WORDS[r % len(WORDS)] + "*", "*" + RUNES[r % len(RUNES)] + "-*", "?*", v, _q_rune(v),
                  v[:2] + "*" + v[-1:], ""][r % 7]
            rd2["annotations"] = {kp: vp}
        shape = r % 4
        if shape == 0:  # one `any` filter holding every field
            pol = _rule(r, {"any": [{"resources": {**rd, **rd2}}]})
        elif shape == 1:  # `all` of two filters
            fl = [{"resources": rd}] + ([{"resources": rd2}] if rd2 else [])
            pol = _rule(r, {"all": fl})
        elif shape == 2:  # `any` of two filters, and an `any` exclude
            fl = [{"resources": rd}] + ([{"resources": rd2}] if rd2 else [])
            x = {"any": [{"resources": {"names": pattern_list(2, names, r + 11, False)}}]}
            pol = _rule(r, {"any": fl}, x)
        else:  # the fields matched, an `all` exclude over two filters
            x = {"all": [{"resources": {"names": [WORDS[r % len(WORDS)] + "*"]}},
                         {"resources": {"namespaces": ["ns-*"]} if "namespaces" in use else {"names": ["*1"]}}]}
            pol = _rule(r, {"all": [{"resources": {**rd, **rd2}}]}, x)
        pols.append(_policy(r, pol))
    if "annotations" in use:
        # one rule decided by annotation values alone, over the multi-byte runes: `*??<rest>` against a
        # value that is one rune and <rest> (must not match), `?` in the place of a rune, `??` before one
        v3, v1, v2 = avs[3 % n_annv], avs[1 % n_annv], avs[2 % n_annv]
        fl = [{"resources": {"annotations": {"example.io/*": "*??" + v3[1:]}}},
              {"resources": {"annotations": {"*": _q_rune(v1)}}},
              {"resources": {"annotations": {"*-*": "??" + v2[2:]}}},
              {"resources": {"annotations": {"*": "*" + RUNES[2] + "?" + "*"}}}]
        pols.append(_policy(n_rules, _rule(n_rules, {"any": fl})))
    if pat_bytes is not None:
        have = shapes(pols, docs)["pat_bytes"]
        pad = pat_bytes - have
        assert pad > 0, (have, pat_bytes)
        rd = pols[0]["spec"]["rules"][0]["match"]["any"][0]["resources"]
        rd["names"] = rd["names"] + ["q" * pad]
        assert shapes(pols, docs)["pat_bytes"] == pat_bytes
    return pols, ndjson(docs), docs


def ndjson(docs):
    return "\n".join(json.dumps(d, ensure_ascii=False) for d in docs).encode()


# ---- what the placement depends on, derived from the documented constants ----------------------


def _lit_len(g):
    """Bytes a pattern record stores (patclass.hpp classify_pattern)."""
    b = len(g.encode())
    stars, q = g.count("*"), "?" in g
    if g == "*":
        return 0
    if not q and stars == 1 and (g.endswith("*") or g.startswith("*")):
        return b - 1
    if not q and stars == 2 and len(g) >= 2 and g.startswith("*") and g.endswith("*"):
        return b - 2
    return b


def shapes(policies, docs):
    """The program's distinct predicates (domain, pattern tuple) as the compiler forms them (one per
    distinct list of a domain: name, names -> names; namespaces; annotation keys and values one each;
    kinds), the dictionaries of the corpus, and from them: pattern records, pattern bytes, the
    (string, pattern) pairs over dictionaries, and the longest string of a referenced domain."""
    preds = []

    def pred(dom, globs):
        p = (dom, tuple(globs))
        if p not in preds:
            preds.append(p)

    for pol in policies:
        for rule in pol["spec"]["rules"]:
            for blk in (rule.get("match"), rule.get("exclude")):
                a, b = _filters(blk)
                for rd in a + b:
                    if rd.get("kinds"):
                        pred("kind", rd["kinds"])
                    if rd.get("name"):
                        pred("name", [rd["name"]])
                    if rd.get("names"):
                        pred("name", rd["names"])
                    if rd.get("namespaces"):
                        pred("ns", rd["namespaces"])
                    for k, v in (rd.get("annotations") or {}).items():
                        pred("annk", [k])
                        pred("annv", [v])
    dicts = {"kind": set(), "name": set(), "ns": set(), "annk": set(), "annv": set()}
    for d in docs:
        md = d.get("metadata") or {}
        dicts["kind"].add(d.get("kind", ""))
        dicts["name"].add(md.get("name") or md.get("generateName") or "")
        dicts["ns"].add(md.get("namespace", ""))
        if d.get("kind") == "Namespace":
            dicts["ns"].add(md.get("name", ""))
        for k, v in (md.get("annotations") or {}).items():
            dicts["annk"].add(k)
            dicts["annv"].add(v)
    size = {k: len(v) for k, v in dicts.items()}
    local = [(d, g) for d, g in preds if size[d] <= 2048]  # predicates whose bitset can live in LDS
    records = sum(len(g) for _, g in preds)
    pat_bytes = sum(_lit_len(x) for _, g in preds for x in g)
    pairs = sum(size[d] * len(g) for d, g in local)
    str_bytes = sum(len(s.encode()) for d in {d for d, _ in local} for s in dicts[d])
    return {
        "preds": preds,
        "dict": size,
        "records": records,
        "pat_bytes": pat_bytes,
        # (string, pattern) pairs, the longest string and the fuse image estimate over the local predicates:
        # 2 words per pair, 4 per record, the pattern and string bytes, 16
        "pairs": pairs,
        "max_len": max((len(s.encode()) for d, _ in local for s in dicts[d]), default=0),
        "fuse_words": 2 * pairs + 4 * records + (pat_bytes + str_bytes) // 4 + 16,
        "max_list": max((len(g) for _, g in preds), default=0),
    }


# ---- the regime table ------------------------------------------------------------------------
# The documented constants of the placement (kpe_api.cpp ensure_binding, scan.hip kpe_pred_kernel)
FUSE_PAIRS, FUSE_RECORDS, FUSE_STR, FUSE_WORDS = 1024, 4096, 4095, 4096
LOCAL_STRINGS = 2048
STR_LDS, PAT_LDS, PAT_RECORDS = 16384, 4096, 64


def _long_value_doc(nbytes):
    return {"apiVersion": "example.io/v1", "kind": KIND,
            "metadata": {"name": "long-0", "namespace": "ns-web-0",
                         "annotations": {"example.io/web-0": "web-" + "y" * (nbytes - 4)}}, "spec": {}}


def _degenerate_docs():
    def doc(kind, **md):
        return {"apiVersion": "example.io/v1", "kind": kind, "metadata": md, "spec": {}}

    return [doc(KIND, generateName="web-gen-", namespace="ns-web-0"),           # generateName only
            doc(KIND, name="", generateName="db-gen-", namespace="ns-db-1"),     # an empty name beside it
            doc(KIND, name="cache-cluster"),                                     # cluster-scoped: namespace ""
            doc(KIND, name="api-1", namespace="ns-api-3", annotations={"example.io/web-0": ""}),  # empty value
            doc(KIND, name="job-noann", namespace="ns-job-4", annotations={}),
            doc("Namespace", name="ns-web-0"),                                   # its namespace is its own name
            doc("Namespace", name="web-0", annotations={"example.io/db-1": "dbé-1"})]


def _staged_then_long(i):  # the first 256 values fit one staged block, the rest are 100..5000 bytes
    return 40 if i < 256 else 100 + (i * 977) % 4901


NAMES_ONLY = dict(fields=("names",), kinds=False)
# id -> (regime, knobs). Regimes: "fused" (scan prologue pair table), "local" (every bitset in LDS,
# filled by the dictionary kernel), "global" (some bitset in HBM)
REGIMES = {
    "fused-1": ("fused", dict(n_names=1, n_ns=1, n_annk=1, n_annv=1, n_rules=4, rows=3)),
    "fused-31": ("fused", dict(n_names=31, n_annv=31, n_rules=2)),
    "fused-32": ("fused", dict(n_names=32, n_annv=32, n_rules=2)),
    "fused-33": ("fused", dict(n_names=33, n_annv=33, n_rules=2)),
    "fused-64": ("fused", dict(n_names=64, n_annv=64, n_rules=2)),
    "fused-1024-pairs": ("fused", dict(n_names=64, pats=16, n_rules=1, **NAMES_ONLY)),
    "fused-4095-byte-string": ("fused", dict(n_rules=2, extra_docs=(_long_value_doc(4095),))),
    "past-1025-pairs": ("local", dict(n_names=64, n_ns=1, pats=16, ns_pats=1, n_rules=1,
                                      fields=("names", "namespaces"), kinds=False, match_all=False)),
    "past-4096-byte-string": ("local", dict(n_rules=2, extra_docs=(_long_value_doc(4096),))),
    "past-4096-records": ("local", dict(n_names=3, pats=60, n_rules=70, rows=40, fields=("names",))),
    **{f"local-{n}": ("local", dict(n_names=n, n_annv=max(n // 2, 5), pats=20, n_rules=3))
       for n in (63, 64, 65, 255, 256, 257, 2048)},
    "global-2049": ("global", dict(n_names=2049, n_annv=257, pats=6, n_rules=3)),
    "global-2304": ("global", dict(n_names=2049 + 255, n_annv=2561, pats=6, n_rules=3)),
    "strings-16384-bytes": ("local", dict(n_names=256, name_len=64, pats=8, n_rules=3)),  # one block, staged
    "strings-16385-bytes": ("local", dict(n_names=256, name_len=lambda i: 65 if i == 0 else 64, pats=8, n_rules=3)),
    "strings-long-names": ("local", dict(n_names=300, name_len=(200, 253), pats=8, n_rules=3)),
    "strings-long-values": ("local", dict(n_names=40, n_annv=600, annv_len=_staged_then_long, pats=30, n_rules=4)),
    "patterns-64": ("local", dict(n_names=300, pats=64, n_rules=2, **NAMES_ONLY)),
    "patterns-65": ("local", dict(n_names=300, pats=65, n_rules=2, **NAMES_ONLY)),
    "patterns-4096-bytes": ("local", dict(n_names=300, pats=63, n_rules=2, pat_bytes=4096, **NAMES_ONLY)),
    "patterns-4097-bytes": ("local", dict(n_names=300, pats=63, n_rules=2, pat_bytes=4097, **NAMES_ONLY)),
    "degenerate-one-row": ("fused", dict(n_names=1, n_ns=1, n_annk=1, n_annv=1, n_rules=4, rows=1)),
    "degenerate-documents": ("fused", dict(n_names=6, n_ns=5, ns_pats=18, n_rules=4, extra_docs=tuple(_degenerate_docs()))),
}

_built = {}


def regime_case(name):
    """(regime, policies, ndjson, docs, shapes) of a REGIMES entry, built once."""
    if name not in _built:
        regime, knobs = REGIMES[name]
        pols, nd, docs = case(**knobs)
        _built[name] = (regime, pols, nd, docs, shapes(pols, docs))
    return _built[name]


def block_bytes(strings):
    """Byte totals of the 256-string blocks of a dictionary in interning (first-seen) order."""
    seen = list(dict.fromkeys(strings))
    return [sum(len(s.encode()) for s in seen[i:i + 256]) for i in range(0, len(seen), 256)]
