"""The pattern-leaf table: one single-leaf policy {"spec": {"v": P}} per pattern over documents
{"spec": {"v": V}}, so that cell (document, policy) is pattern.Validate(V, P) and nothing else.

Values and patterns cover what the leaf comparators of patvm.inl decide: quantities (every
suffix, exponents, signs, sub-nano rounding, values past int64 and 2^64, equal values in other
spellings), durations (units, fractional and compound forms, the int64-nanosecond edge), numeric
strings Go parses or refuses, JSON numbers at the float64 / int64 edges, booleans, null, the empty
string, and globs over multi-byte runes. The reference's own vectors (pattern_test.go leaf
validators and ext/wildcard) are added as further (pattern, value) cells whose expected verdict
is the vector's `want`. Every other cell is held engine-to-oracle.
"""
import json
import os
import re

GOLD = os.path.join(os.path.dirname(__file__), "golden")
PLEAF = json.load(open(os.path.join(GOLD, "pattern_leaf_cases.json")))
WILD = json.load(open(os.path.join(GOLD, "wildcard_match.json")))

BIN = ["Ki", "Mi", "Gi", "Ti", "Pi", "Ei"]
DEC = ["n", "u", "m", "", "k", "M", "G", "T", "P", "E"]

QUANTITIES = (
    ["1" + s for s in BIN + DEC if s] + ["3" + s for s in ("Ki", "m", "k", "G")]
    + ["1024", "0.5Gi", "512Mi", "1e3m", "1", "1000m", "1e3", "1E3", "1e-3", "1E-3", "1E", "2E", "1Ee3", "1e3Ki", "1.5e3",
       "12e6", "+1", "-1", "+1Ki", "-1Ki", "-1m", "+1.5Gi", "-0", "0", "0Ki", ".5", "5.", ".5Gi", "1.5Gi", "1536Mi",
       "0.1", "100m", "0.001", "1m", "0.0001", "0.1m", "100u", "1n", "0.1n", "0.5n", "0.9n", "1e-10", "0.0000000005", "1.0000000001",
       "9223372036854775807", "9223372036854775808", "-9223372036854775808", "-9223372036854775809",
       "18446744073709551615", "18446744073709551616", "1e19", "1e30", "9Ei", "8Ei", "7Ei", "16Ei", "9223372036854775807Ei",
       "1000000000000000000000", "123456789012345678901234567890", "0.000000000000000000001",
       "1 Ki", "1ki", "1KI", "Ki", "1K", "1Kii", "1e", "e3", "1ee3", "1e+3", "1e+3Ki", "--1", "+-1", "1..5", "1,5"])

DURATIONS = ["1ns", "1us", "1µs", "1μs", "1ms", "1s", "1h", "60s", "60m", "3600s", "1.5h", "90m", "1h30m", "1h30m0s",
             "-1h", "+1h", "-1.5h", "1m30s", "1.5s", "1500ms", ".5s", "1.s", "0s", "0h", "0", "1d", "1w", "1 h", "h", "1hh",
             "2562047h47m16.854775807s", "2562047h47m16.854775808s", "-2562047h47m16.854775808s",
             "-2562047h47m16.854775809s", "9223372036854775807ns", "9223372036854775808ns", "-9223372036854775808ns",
             "2562048h", "1000000h", "0.000000001s", "0.0000000001s", "1e3s", "1h-30m"]

NUMERIC_STRINGS = ["+1", "1.", ".5", "0x10", "0X10", "0b1", "0o7", "017", "1_000", "Inf", "+Inf", "-Inf", "inf", "NaN", "nan",
                   "Infinity", " 1", "1 ", " 1 ", "\t1", "1\n", "1e400", "-1e400", "1e-400", "-0.0", "-0", "007", "1.0", "1.50",
                   "1.5", "3", "3.0", "4", "5", "7", "7.0000", "7.00001", "10", "2", "0.0", "1e0", "1E0", "1e1",
                   "9007199254740992", "9007199254740993", "9007199254740992.0", "9007199254740993.0",
                   "9223372036854775807.0", "0.1", "0.10", "1e-7", "0.0000001", "1.7976931348623157e308", "4.9e-324", "5e-324"]

STRINGS = ["", " ", "abc", "ABC", "true", "false", "null", "True", "nil", "*", "?", "a|b", "a&b", "a | b", "a & b", "!x", "x",
           ">1", "<1", ">=1", "<=1", "1-5", "1!-5", "5-1", "a-b", "-", "!-", "1-", "-1-1", "é", "本", "\U0001F600", "本y!",
           "a本y!", "é本y!", "naïve", "nai?ve", "á", " ", "日本語", "日本", "x\U0001F600y", "ab" * 40 + "é",
           "s3:GetObject", "leftright", "nginx:latest", "5.10.84-1", "5.16.5-arch1-1"]

JSON_NUMBERS = [0, 1, -1, 2, 3, 4, 5, 7, 10, 1024, 1000, 1536, 2 ** 53, 2 ** 53 + 1, -(2 ** 53) - 1, 2 ** 63 - 1, -(2 ** 63),
                2 ** 31, 2 ** 32, 0.0, -0.0, 1.0, 1.5, 0.1, 0.5, 3.0, 7.00001, 1e19, 1e300, -1e300, 1e-7, 1e-300, 5e-324,
                1.7976931348623157e308, 9007199254740993.0, 1e21, 1e20, 123456789.125, 0.001, 1e3, 18446744073709551616.0]

OTHER = [True, False, None]


def values():
    """JSON texts of the document values, no text twice."""
    out = []
    for v in list(JSON_NUMBERS) + OTHER + QUANTITIES + DURATIONS + NUMERIC_STRINGS + STRINGS:
        t = json.dumps(v, ensure_ascii=False)
        if t not in out:
            out.append(t)
    return out


def _endpoint(s):
    return re.fullmatch(r"[-+|]?[0-9]+(\.[0-9]+)?[A-Za-z]*", s) is not None


def _is_range(s):
    """`lo-hi` or `lo!-hi` with number-and-unit endpoints (operator.go's range forms)."""
    return any(s[k] == "-" and _endpoint(s[:k].removesuffix("!")) and _endpoint(s[k + 1:]) for k in range(1, len(s)))


def _has_operator(s):
    """As a leaf the text means something other than `glob-equal to s`: `|` or `&`, an operator prefix,
    a range form, or blanks at its ends (trimmed away)."""
    return "|" in s or "&" in s or (len(s) >= 2 and s[0] in "<>!") or _is_range(s) or s != s.strip()


def patterns():
    """JSON texts of the patterns."""
    out = []

    def add(p):
        t = json.dumps(p, ensure_ascii=False)
        if t not in out:
            out.append(t)

    plain = [s for s in QUANTITIES + DURATIONS + NUMERIC_STRINGS if s.strip() == s and s]
    for s in plain:  # each string value as equality and under every operator
        for op in ("", ">", "<", ">=", "<=", "!"):
            add(op + s)
    for s in ("1Ki", "1h", "1.5", "1e3", "100m"):  # blanks after the operator are trimmed
        for op in (">", "<=", "!"):
            add(op + " " + s)
    for lo, hi in [("1", "5"), ("0", "2"), ("1.5", "3"), ("-1", "1"), ("100m", "2"), ("1Ki", "1Mi"), ("512Mi", "1Gi"),
                   ("1m", "1"), ("1s", "1h"), ("90m", "2h"), ("1ms", "1s"), ("1e3", "1e4"), ("5", "1"), ("1Gi", "1Ki"),
                   ("0.5", "1Ki"), ("1", "1h"), ("1n", "1E"), ("9223372036854775807", "9223372036854775808"),
                   ("-9223372036854775808", "0"), ("1us", "2562047h47m16.854775807s")]:
        add(f"{lo}-{hi}")
        add(f"{lo}!-{hi}")
    for p in [">1 & <5", ">=1Ki & <=1Mi", ">1h | <1m", "1 | 2 | 3", "abc | 本 | é", ">5 | 1-2", "!1 & !2", "<1 | >1000 & <2000",
              "1-5 | 10-20", "1!-5 & <100", "a* | *b", "a* & *b", "?* & !abc", "| 1", "1 |", "& 1", " 1 ", ">", "<", "!", ">=", "!-", "-",
              "1Ki | 1Mi", "!1Ki & !1024", ">=-1", "<=+1", "!true", "!false", "!null", "true | false", "null"]:
        add(p)
    for p in ["*", "?", "??", "?*", "*?", "**", "*?*", "é", "?本*", "*本*", "本*", "*本", "本??", "*??y!", "?y!", "??y!", "*é*y?",
              "\U0001F600", "?", "x?y", "x*y", "*\U0001F600*", "na?ve", "na??ve", "nai?ve", "a?", "a??", "日?語", "日*", "?本?", "??語",
              "*" + "ab" * 40 + "?", "ab" * 40 + "é", "ab*é", "*abab?", "s3:*", "*Object", "*:Get*", "s3:???Object", "*left*right*",
              "nginx:*", "*:latest", "5.10.84-1", "!5.10.84-1", "abc", "ABC", "", " ", "tru?", "nul*", "1*", "*1", "1?", "?.5", "*Ki", "1?i",
              " ", "* *", "á", "a?"]:
        add(p)
    for p in JSON_NUMBERS + OTHER:
        add(p)
    return out


# ---- the reference's vectors -------------------------------------------------------------------
# Vectors that cannot be one string leaf of a tree, each with its reason. Names are the fixtures' own.
DROPPED = {}


def _drop(name, why):
    DROPPED[name] = why


def golden():
    """[(name, pattern JSON text, value JSON text, want)] of the reference's vectors written as one leaf."""
    out = []
    nvalidate = 0
    for c in PLEAF:
        fn, name = c["fn"], c["name"]
        if fn == "validate":
            p, v = json.loads(c["pattern"]), json.loads(c["value"])
            if isinstance(p, (dict, list)) or isinstance(v, (dict, list)):
                continue  # not scalars: counted by the test (13 of 64)
            nvalidate += 1
            out.append((name, c["pattern"], c["value"], c["want"]))
        elif fn in ("pattern", "patterns"):
            # validateStringPattern takes one condition, validateStringPatterns splits on | and &: as a leaf
            # both go through the split, which changes nothing for a text without | and &
            if fn == "pattern" and ("|" in c["pattern"] or "&" in c["pattern"]):
                _drop(name, "a single-condition vector whose text a leaf would split on | or &")
                continue
            out.append((name, json.dumps(c["pattern"], ensure_ascii=False), c["value"], c["want"]))
        elif fn in ("string", "compare"):
            # validateString / compareString get the operator apart from the operand: the leaf is op + operand
            if _has_operator(c["pattern"]) and not (fn == "compare" and c["op"] == ""):
                _drop(name, "the operand itself reads as an operator or a range once the operator is written before it")
                continue
            if fn == "compare" and c["op"] == "" and _has_operator(c["pattern"]):
                _drop(name, "compareString's glob operand reads as an operator or a range in a leaf")
                continue
            out.append((name, json.dumps(c["op"] + c["pattern"], ensure_ascii=False), c["value"], c["want"]))
    for i, c in enumerate(WILD["match"]):
        name = f'{c["src"]}[{i}]'
        if _has_operator(c["pattern"]):
            _drop(name, "the glob reads as an operator or a range in a leaf")
            continue
        out.append((name, json.dumps(c["pattern"], ensure_ascii=False), json.dumps(c["text"], ensure_ascii=False),
                    c["matched"]))
    return out, nvalidate


def policy(i, pattern_text):
    return ('{"apiVersion":"kyverno.io/v1","kind":"ClusterPolicy","metadata":{"name":"l%d"},"spec":{"rules":[{"name":"r",'
            '"match":{"any":[{"resources":{"kinds":["*"]}}]},"validate":{"pattern":{"spec":{"v":%s}}}}]}}' % (i, pattern_text))


def document(value_text):
    return '{"apiVersion":"v1","kind":"Thing","metadata":{"name":"d"},"spec":{"v":%s}}' % value_text


def table():
    """(pattern texts, value texts, {(pattern index, value index): (vector name, want)})."""
    pats, vals = patterns(), values()
    gold, nvalidate = golden()
    want = {}
    for name, p, v, w in gold:
        if p not in pats:
            pats.append(p)
        if v not in vals:
            vals.append(v)
        key = (pats.index(p), vals.index(v))
        assert want.get(key, (None, w))[1] == w, (name, want[key])  # two vectors on one cell agree
        want[key] = (name, w)
    return pats, vals, want, len(gold), nvalidate


def policies(pattern_texts, first=0):
    return [json.loads(policy(first + i, p)) for i, p in enumerate(pattern_texts)]


def ndjson(value_texts):
    return "\n".join(document(v) for v in value_texts).encode()


# ---- scalar counts and text alignment -----------------------------------------------------------
def simple_head(n):
    """n values whose scalars the test can count: distinct integers and distinct strings without `-`
    (no range form, whose endpoints would be interned too), none of them an envelope string."""
    out = []
    for i in range(n):
        out.append(json.dumps(1000 + 7 * i) if i % 3 == 0 else json.dumps(["%dKi", "w%d", "%dm"][i % 3] % i))
    return out


def scalar_count(value_texts):
    """Interned scalars of a corpus of document(v): null, false, true are fixed entries; the envelope has
    three strings; then one per distinct value text that is none of those (simple_head values only)."""
    fixed = {"null", "false", "true"} | {json.dumps(s) for s in ("v1", "Thing", "d")}
    return 6 + len(set(value_texts) - fixed)


SCALAR_COUNTS = (7, 63, 64, 65, 127, 129)  # 7: the smallest corpus of document(v) (6 of its own + one value)
LONGEST = json.dumps("本" * 3 + "ab" * 60 + "é", ensure_ascii=False)
SHORTEST = json.dumps("é", ensure_ascii=False)


def aligned_tails():
    """Document lists whose last scalar text starts at each of the 8 byte alignments and ends the text
    buffer: a pad string of 1..8 bytes before it moves its start by one byte each time."""
    out = []
    for last in (LONGEST, SHORTEST):
        for k in range(8):
            out.append(simple_head(20) + [json.dumps("p" * (k + 1)), last])
    return out
