"""Policies and edge documents shared by tests/test_jmespath_funcs.py (host VM) and
tests/test_gpu_jmespath_funcs.py (device): the go-jmespath builtins the condition VM evaluates
(contains, starts_with, ends_with, not_null, values(), keys() in function form) in every
argument form the compiler accepts. The literals are what kpe_synth emits (app-1*, team-1,
back*, nginx:*, res-1?) so that every rule's oracle column mixes verdicts."""
import json

OBJ = "request.object"
KINDS = ("Pod", "Deployment", "Service", "ConfigMap")


def c(key, op, value):
    return {"key": key, "operator": op, "value": value}


def q(expr):
    return "{{ " + expr + " }}"


def rule(name, validate, pre=None, kinds=KINDS):
    r = {"name": name, "match": {"any": [{"resources": {"kinds": list(kinds)}}]}, "validate": validate}
    if pre is not None:
        r["preconditions"] = pre
    return r


def deny(*conds, any_block=False):
    return {"message": "m", "deny": {"conditions": {("any" if any_block else "all"): list(conds)}}}


def policy(name, rules):
    return {"apiVersion": "kyverno.io/v1", "kind": "ClusterPolicy", "metadata": {"name": name},
            "spec": {"background": True, "validationFailureAction": "Audit", "rules": rules}}


LABELS = OBJ + ".metadata.labels"
NAME = OBJ + ".metadata.name"
IMG0 = OBJ + ".spec.containers[0].image"

# name -> the deny condition (true => fail, false => pass, an evaluation error => error)
DENY_CONDITIONS = [
    # string subjects
    ("contains-name", c(q(f"contains({NAME}, '1')"), "Equals", True)),
    ("contains-name-empty-needle", c(q(f"contains({OBJ}.metadata.labels.app, '')"), "Equals", True)),
    ("starts-app", c(q(f"starts_with({LABELS}.app, 'app-1')"), "Equals", True)),
    ("starts-json-str", c(q(f'starts_with({NAME}, `"res-1"`)'), "Equals", True)),
    ("ends-image", c(q(f"ends_with({IMG0}, ':latest')"), "Equals", True)),
    ("starts-image", c(q(f"starts_with({IMG0}, 'nginx:')"), "NotEquals", False)),
    ("ends-name-long", c(q(f"ends_with({NAME}, 'res-12')"), "Equals", False)),
    # a needle / suffix that is a chain, alone and with a `||` default inside the argument
    ("ends-chain", c(q(f"ends_with({IMG0}, {LABELS}.tag)"), "Equals", True)),
    ("ends-chain-default", c(q(f"ends_with({IMG0}, {LABELS}.tag || ':latest')"), "Equals", True)),
    ("contains-default-subject", c(q(f"contains({LABELS}.team || 'none', 'team-1')"), "Equals", True)),
    ("contains-chain-needle", c(q(f"contains({NAME}, {LABELS}.part)"), "Equals", True)),
    # list subjects: keys() / values() in function form, `.keys(@)`, `[]`, `[*]`, multi-select,
    # an array of the document, a constant list
    ("contains-keys", c(q(f"contains(keys({LABELS}), 'team')"), "Equals", True)),
    ("contains-keys-step", c(q(f"contains({LABELS}.keys(@), 'team')"), "Equals", True)),
    ("contains-values", c(q(f"contains(values({LABELS}), 'backend')"), "Equals", True)),
    ("contains-values-null", c(q(f"contains(values({LABELS}), `null`)"), "Equals", True)),
    ("contains-flat", c(q(f"contains({OBJ}.spec.containers[].image, 'nginx:latest')"), "Equals", True)),
    ("contains-star", c(q(f"contains({OBJ}.spec.containers[*].name, 'c-1')"), "Equals", True)),
    ("contains-msl", c(q(f"contains({OBJ}.spec.[initContainers, containers][].name, 'init-0')"), "Equals", True)),
    ("contains-ports-num", c(q(f"contains({OBJ}.spec.ports, `80`)"), "Equals", True)),
    ("contains-port-proj", c(q(f"contains({OBJ}.spec.ports[].port, `80`)"), "Equals", True)),
    ("contains-bool", c(q(f"contains({OBJ}.spec.containers[].securityContext.runAsNonRoot, `true`)"), "Equals",
                        True)),
    ("contains-const-list", c(q(f'contains(`["backend", "x"]`, {LABELS}.tier)'), "Equals", True)),
    ("contains-list-chain-needle", c(q(f"contains(values({LABELS}), {NAME})"), "Equals", True)),
    # not_null
    ("not-null-default", c(q(f"not_null({LABELS}.team, 'none')"), "Equals", "none")),
    ("not-null-three", c(q(f"not_null({OBJ}.spec.nothing, {OBJ}.spec.replicas, `1`)"), "Equals", 4)),
    ("not-null-one", c(q(f"not_null({LABELS}.team)"), "Equals", "team-1")),
    ("not-null-keys-error", c(q(f"not_null({NAME}, keys({LABELS}))"), "Equals", "res-1?")),
    # a call as an operand of the top-level `||`, in both positions
    ("or-call-call", c(q(f"contains({NAME}, '7') || starts_with({LABELS}.tier, 'back')"), "Equals", True)),
    ("or-call-literal", c(q(f"starts_with({NAME}, 'res-1') || 'no'"), "Equals", "no")),
    ("or-chain-call", c(q(f"{LABELS}.canary || ends_with({NAME}, '3')"), "Equals", True)),
    # a boolean result substituted into a string, and as the value side
    ("tmpl-bool", c("has-team=" + q(f"contains(keys({LABELS}), 'team')"), "Equals", "has-team=true")),
    ("value-side", c(True, "Equals", q(f"ends_with({LABELS}.app, '7')"))),
]


def deny_rules():
    return [rule(n, deny(cond)) for n, cond in DENY_CONDITIONS]


def foreach_rules():
    return [
        rule("fe-values-list", {"message": "m", "foreach": [{
            "list": f"values({LABELS})",
            "deny": {"conditions": {"all": [c(q("element"), "Equals", "backend")]}}}]}),
        rule("fe-element-ends", {"message": "m", "foreach": [{
            "list": OBJ + ".spec.containers",
            "preconditions": {"all": [c(q("starts_with(element.name, 'c-')"), "Equals", True)]},
            "deny": {"conditions": {"any": [c(q("ends_with(element.image, ':latest')"), "Equals", True)]}}}]}),
        rule("fe-index-const-list", {"message": "m", "foreach": [{
            "list": OBJ + ".spec.containers",
            "deny": {"conditions": {"all": [c(q("contains(`[1, 2]`, elementIndex)"), "Equals", True)]}}}]}),
        rule("pre-contains", deny(c(q(NAME), "Equals", "res-*1")),
             pre={"all": [c(q(f"contains(keys({LABELS}), 'team')"), "Equals", True)]}),
    ]


def func_policy_set():
    """Deny, precondition and foreach rules: the set the host VM and the device evaluate."""
    return [policy("jmesfn", deny_rules() + foreach_rules())]


def needle_list_policy():
    """contains() whose needle is a list on the rows that have spec.ports: a deep comparison the
    device leaves undecided when the subject is an array."""
    return [policy("needle", [rule("needle-list", deny(c(
        q(f"contains(`[80, 443]`, {OBJ}.spec.ports[].port || `80`)"), "Equals", True)))])]


def needle_list_rows(docs):
    """Rows of needle_list_policy whose needle is a (non-empty, so truthy) list."""
    out = []
    for d in docs:
        ports = (d.get("spec") or {}).get("ports") if isinstance(d.get("spec"), dict) else None
        lst = [p["port"] for p in ports if isinstance(p, dict) and p.get("port") is not None] \
            if isinstance(ports, list) else []
        out.append(bool(lst))
    return out


def pattern_and_exception_set():
    """The functions inside a pattern leaf, a pattern template and an exception condition."""
    pols = [policy("fnpat", [
        rule("leaf-not-null", {"message": "m", "pattern": {"metadata": {"labels": {
            "tier": q(f"not_null({LABELS}.wanted, 'backend')")}}}}, kinds=("Pod", "ConfigMap")),
        rule("leaf-tmpl-bool", {"message": "m", "pattern": {"metadata": {"labels": {
            "flag": "is-" + q(f"starts_with({NAME}, 'res-1')")}}}}, kinds=("Pod", "ConfigMap")),
        rule("deny-front", deny(c(q(f"{LABELS}.tier || ''"), "Equals", "frontend")), kinds=("Pod", "Service")),
    ])]
    excs = [{"apiVersion": "kyverno.io/v2beta1", "kind": "PolicyException", "metadata": {"name": "x"},
             "spec": {"exceptions": [{"policyName": "fnpat", "ruleNames": ["deny-front"]}],
                      "match": {"any": [{"resources": {"kinds": ["Pod", "Service"]}}]},
                      "conditions": {"any": [c(q(f"contains(keys({LABELS}), 'team')"), "Equals", True),
                                             c(q(f"ends_with({NAME}, '5')"), "Equals", True)]}}}]
    return pols, excs


def _doc(kind, name, labels=None, spec=None, drop_labels=False):
    meta = {"name": name, "namespace": "edge"}
    if not drop_labels:
        meta["labels"] = labels if labels is not None else {}
    d = {"apiVersion": "v1", "kind": kind, "metadata": meta}
    if spec is not None:
        d["spec"] = spec
    return d


def edge_documents():
    ctr = lambda n, img, **kw: dict({"name": n, "image": img}, **kw)  # noqa: E731
    return [
        _doc("Pod", "no-labels", drop_labels=True, spec={"containers": [ctr("c-0", "nginx:latest")]}),
        _doc("Pod", "empty-labels", {}, {"containers": [ctr("c-1", "redis:7")]}),
        _doc("Pod", "no-containers", {"app": "app-1", "team": "team-1"}, {"containers": []}),
        _doc("Service", "ports-float", {"app": "app-2", "tier": "backend"}, {"ports": [80.0]}),
        _doc("Service", "ports-other", {"app": "app-2", "tier": "frontend"}, {"ports": [81, "80", None, True]}),
        _doc("Service", "ports-objects", {"app": "app-3"}, {"ports": [{"port": 443}, {"port": 80.0}, {"name": "x"}]}),
        _doc("Pod", "tag-suffix", {"app": "app-17", "tag": ":1.2", "part": "suffix"},
             {"containers": [ctr("c-0", "nginx:1.2")]}),
        _doc("Pod", "tag-other", {"app": "app-17", "tag": ":1.3", "part": "zzz"},
             {"containers": [ctr("c-0", "nginx:1.2"), ctr("c-1", "nginx:latest"), ctr("c-2", "x:latest")]}),
        _doc("ConfigMap", "null-label", {"app": None, "tier": "backend", "team": "team-1"}),
        _doc("ConfigMap", "nämé-ünï-1", {"app": "äpp-1", "part": "ünï", "tier": "bäckend"}),
        _doc("ConfigMap", "res-12", {"app": "", "part": "", "team": "", "flag": "is-true"}),
        _doc("ConfigMap", "x", {"app": "app-1", "part": "xres-12-longer-than-the-name", "x": "x", "flag": "is-true"}),
        _doc("ConfigMap", "same", {"app": "same", "part": "same", "canary": "yes"}),
        _doc("Pod", "non-string-args", {"app": 7, "tier": True, "part": 3, "tag": ["a"]},
             {"containers": [ctr("c-1", "nginx:latest", securityContext={"runAsNonRoot": True}),
                             ctr("init-0", "a", securityContext={"runAsNonRoot": False})],
              "initContainers": [ctr("init-0", "b")], "replicas": 4}),
    ]


def edge_ndjson():
    return b"\n".join(json.dumps(d).encode() for d in edge_documents())
