"""Policies and edge documents shared by tests/test_jmespath_filters.py (host VM) and
tests/test_gpu_jmespath_filters.py (device): JMESPath filter steps `[?P]` in every predicate form
the compiler accepts (oracle/conditions.hpp Parser::filter and Interp::eval N_FILTER / N_CMP /
N_AND / N_OR / N_NOT are the specification). The literals are what kpe_synth emits (c-0.., nginx:*,
ports 8080, emptyDir / hostPath volumes) so that every rule's oracle column mixes verdicts."""
import json

from tests.jmespath_func_cases import c, deny, policy, q, rule

OBJ = "request.object"
KINDS = ("Pod", "ConfigMap")
C = OBJ + ".spec.containers"
V = OBJ + ".spec.volumes"

# name -> the deny condition (true => fail, false => pass, an evaluation error => error)
DENY_CONDITIONS = [
    ("truthy-len-pipe", c(q(f"{C}[?securityContext.privileged] | length(@)"), "GreaterThan", 0)),
    ("eq-bool-len-fn", c(q(f"length({C}[?securityContext.privileged == `true`])"), "GreaterThan", 0)),
    ("eq-false", c(q(f"{C}[?securityContext.privileged == `false`].name"), "AnyIn", ["c-0"])),
    ("eq-str-field", c(q(f"{C}[?name == 'c-1'].image"), "AnyIn", ["nginx:latest", "redis:latest"])),
    ("ne-str", c(q(f"{C}[?name != 'c-0'].name | length(@)"), "GreaterThan", 1)),
    ("lit-left", c(q(f"{C}[?'c-2' == name].name | length(@)"), "Equals", 1)),
    ("json-str-lit", c(q(f'{C}[?name == `"c-0"`].securityContext.runAsNonRoot'), "AnyIn", [True])),
    ("and-not", c(q(f"{C}[?name != 'c-0' && !securityContext.runAsNonRoot].name | length(@)"), "GreaterThan", 0)),
    ("or-range", c(q(f"{C}[?ports[0].hostPort > `8050` || ports[0].hostPort < `8010`].name | length(@)"),
                   "GreaterThan", 0)),
    ("ge-le", c(q(f"{C}[?ports[0].containerPort >= `8080` && ports[0].containerPort <= `8080`].name | length(@)"),
                "GreaterThan", 0)),
    ("not-ordering-null", c(q(f"{C}[?!(ports[0].hostPort > `0`)].name | length(@)"), "Equals", 0)),
    ("not-paren-or", c(q(f"{C}[?!(name == 'c-0' || name == 'c-1')].name"), "AnyIn", ["c-2"])),
    ("precedence", c(q(f"{C}[?name == 'c-0' || name == 'c-1' && securityContext.privileged].name | length(@)"),
                     "Equals", 1)),
    ("eq-null", c(q(f"{C}[?ports == `null`].name | length(@)"), "Equals", 0)),
    ("chain-chain", c(q(f"{C}[?securityContext.runAsNonRoot == securityContext.allowPrivilegeEscalation].name"
                        " | length(@)"), "GreaterThan", 0)),
    ("num-eq", c(q(f"{C}[?ports[0].containerPort == `8080`].ports[0].containerPort"), "AnyIn", [8080])),
    ("starts", c(q(f"{C}[?starts_with(image, 'nginx:')].name | length(@)"), "GreaterThan", 0)),
    ("not-ends", c(q(f"{C}[?!ends_with(image, ':latest')].name | length(@)"), "GreaterThan", 0)),
    ("contains-str", c(q(f"{C}[?contains(image, 'a:1.')].name | length(@)"), "GreaterThan", 0)),
    ("has-key", c(q(f"{V}[?contains(keys(@), 'emptyDir')].name | length(@)"), "GreaterThan", 0)),
    ("has-key-chain", c(q(f"{C}[?contains(keys(securityContext), 'privileged')].name | length(@)"),
                        "GreaterThan", 0)),
    ("contains-arr", c(q(f"{C}[?contains(securityContext.capabilities.drop, 'ALL')].name | length(@)"),
                       "GreaterThan", 0)),
    ("at-eq", c(q(f"{C}[0].securityContext.capabilities.add[?@ == 'SYS_ADMIN'] | length(@)"), "GreaterThan", 0)),
    ("flat-after", c(q(f"{C}[?name != 'c-1'].securityContext.capabilities.add[]"), "AnyIn", ["SYS_ADMIN"])),
    ("index-after", c(q(f"{C}[?securityContext.privileged].ports[0].containerPort"), "AnyIn", [8080])),
    ("or-default", c(q(f"{C}[?securityContext.privileged].name || 'none'"), "Equals", "none")),
    ("value-side", c(0, "Equals", q(f"{V}[?hostPath].name | length(@)"))),
    ("tmpl", c("n=" + q(f"{V}[?emptyDir] | length(@)"), "Equals", "n=1")),
    # `!` binds tighter than `.`: `!a.b` is `(!a).b`, a member of a boolean (null), however many `!`
    # stand in front; `!(!a.b)` negates that null; `!a[0].b` is `(!a[0]).b`
    ("not-dotted", c(q(f"{C}[?!securityContext.privileged || name == 'c-1'].name | length(@)"), "GreaterThan", 0)),
    ("not-not-dotted", c(q(f"{C}[?!!securityContext.privileged || name == 'c-1'].name | length(@)"),
                         "GreaterThan", 0)),
    ("not-not-not-dotted", c(q(f"{C}[?!!!securityContext.privileged || name == 'c-2'].name | length(@)"),
                             "GreaterThan", 0)),
    ("not-paren-not-dotted", c(q(f"{C}[?!(!securityContext.privileged)].name | length(@)"), "GreaterThan", 1)),
    ("not-not", c(q(f"{C}[?!!ports].name | length(@)"), "GreaterThan", 1)),
    ("not-index-dotted", c(q(f"{C}[?!ports[0].hostPort || name == 'c-1'].name | length(@)"), "GreaterThan", 0)),
]


def deny_rules():
    return [rule(n, deny(cond), kinds=KINDS) for n, cond in DENY_CONDITIONS]


def foreach_rules():
    return [
        rule("fe-filtered-list", {"message": "m", "foreach": [{
            "list": f"{C}[?securityContext.privileged]",
            "deny": {"conditions": {"all": [c(q("element.name"), "Equals", "c-0")]}}}]}, kinds=KINDS),
        rule("fe-filtered-index", {"message": "m", "foreach": [{  # the index in the filtered list
            "list": f"{C}[?name != 'c-0']",
            "deny": {"conditions": {"all": [c(q("elementIndex"), "Equals", 1)]}}}]}, kinds=KINDS),
        rule("fe-has-key-pattern", {"message": "m", "foreach": [{
            "list": f"{V}[?contains(keys(@), 'emptyDir')]", "elementScope": False,
            "pattern": {"spec": {"containers": [{"name": "c-0 | c-1"}]}}}]}, kinds=KINDS),
        rule("fe-element-filter", {"message": "m", "foreach": [{
            "list": C,
            "deny": {"conditions": {"all": [c(q("element.ports[?containerPort == `8080`] | length(@)"),
                                              "GreaterThan", 0)]}}}]}, kinds=KINDS),
        rule("pre-filter", deny(c(q(OBJ + ".metadata.name"), "Equals", "res-*1")),
             pre={"all": [c(q(f"{V}[?emptyDir].name | length(@)"), "GreaterThan", 0)]}, kinds=KINDS),
    ]


def filter_policy_set():
    """Deny, precondition and foreach rules: the set the host VM and the device evaluate."""
    return [policy("jmesfilt", deny_rules() + foreach_rules())]


# every form that stays KPE_E_UNSUPPORTED, as the whole {{ }} variable of a deny key
REFUSED = [
    f"{C}[?name == 'a']",                               # the filter's own element list as a value
    f"{C}[?name == 'a'] || 'x'",
    f"contains({C}[?name == 'a'].name, 'x')",           # a filter inside a call's argument
    f"{C}[0].name == 'a'",                              # comparators, &&, ! outside a predicate
    f"{C}[0].name && 'a'",
    f"!{C}[0].name",
    f"{C}[].ports[?containerPort == `80`].name",        # a filter inside a projection
    f"{C}[*].ports[?containerPort == `80`].name",
    f"{C}[?name == 'a'].ports[?containerPort == `80`].name",  # a second filter in the chain
    f"{C}[?name == 'a'][?image == 'b'].name",
    f"{C}[?name == 'a'][*].name",                       # `[*]` after a filter (it projects each survivor)
    f"{C}[?name == 'a'].ports[*].containerPort",
    f"{C}[?name == `[1]`].name",                        # array / object literals
    C + '[?securityContext == `{"a": 1}`].name',
    f"{C}[?not_null(name)].name",                       # other calls inside P
    f"{C}[?length(name) > `1`].name",
    f"{C}[?to_string(name) == 'a'].name",
    f"{C}[?ports[?containerPort == `80`]].name",        # a nested filter
    f"{C}[?ports[0:1]].name",                           # slices
    f"{C}[0:1].name",
    f"{C}[?(name || 'x') == 'x'].name",                 # || / && / ! inside a comparison operand
    f"{C}[?!name == `false`].name",
    f"{C}[?contains(name, 'a') == `true`].name",
    f"{C}[?contains(keys(@), name)].name",              # keys() needs a string literal needle
    f"{C}[?contains(name)].name",                       # arity
    f"{C}[?name == 'a'",                                # unclosed
    f"{C}[?name == 'a'].name | [0]",                    # a pipe other than | length(@)
    f"{C}[?name | length(@)].name",                     # a pipe inside P
    f"{C}[?" + " || ".join(f"name == 'c-{i}'" for i in range(17)) + "].name",  # more than 16 leaves
]


def overflow_policy():
    """33 survivors overflow the VM's list (undecided); 2 survivors of 40 elements do not."""
    return [policy("filtcap", [
        rule("all-survive", deny(c(q(f"{C}[?name != 'zz'].name | length(@)"), "GreaterThan", 0)), kinds=KINDS),
        rule("two-survive", deny(c(q(f"{C}[?name == 'c-1' || name == 'c-2'].name | length(@)"), "Equals", 2)),
             kinds=KINDS),
    ])]


def overflow_documents():
    ctr = lambda i: {"name": f"c-{i}", "image": "nginx:1"}  # noqa: E731
    return [_doc("Pod", "ctr-33", {"containers": [ctr(i) for i in range(33)]}),
            _doc("Pod", "ctr-40", {"containers": [ctr(i) for i in range(40)]}),
            _doc("Pod", "ctr-3", {"containers": [ctr(i) for i in range(3)]})]


# (row, rule) cells of overflow_policy over overflow_documents that are KPE_UNDECIDED
OVERFLOW_UNDECIDED = {(0, 0), (1, 0)}


def pattern_and_exception_set():
    """A filter inside a pattern leaf variable and inside an exception's conditions."""
    pols = [policy("filtpat", [
        rule("leaf-whole", {"message": "m", "pattern": {"metadata": {"labels": {
            "=(canary)": q(f"{V}[?hostPath].name | length(@)")}}}}, kinds=KINDS),
        rule("leaf-count", {"message": "m", "pattern": {"metadata": {"labels": {
            "app": "app-" + q(f"{V}[?emptyDir] | length(@)") + "*"}}}}, kinds=KINDS),
        rule("deny-latest", deny(c(q(f"{C}[?ends_with(image, ':latest')].name | length(@)"), "GreaterThan", 0)),
             kinds=KINDS),
    ])]
    excs = [{"apiVersion": "kyverno.io/v2beta1", "kind": "PolicyException", "metadata": {"name": "x"},
             "spec": {"exceptions": [{"policyName": "filtpat", "ruleNames": ["deny-latest"]}],
                      "match": {"any": [{"resources": {"kinds": ["Pod"]}}]},
                      "conditions": {"any": [c(q(f"{V}[?contains(keys(@), 'hostPath')].name | length(@)"),
                                               "GreaterThan", 0)]}}}]
    return pols, excs


def _doc(kind, name, spec=None, labels=None):
    d = {"apiVersion": "v1", "kind": kind, "metadata": {"name": name, "namespace": "edge",
                                                        "labels": labels if labels is not None else {"app": "app-1"}}}
    if spec is not None:
        d["spec"] = spec
    return d


def edge_documents():
    """Malformed shapes as ConfigMaps (a Pod that fails typed decode is a context error in the
    oracle), and one well-formed Pod."""
    def ctr(n, img="nginx:1", **kw):
        return dict({"name": n, "image": img}, **kw)

    def sc(**kw):
        return {"securityContext": kw}
    cm = lambda name, spec=None: _doc("ConfigMap", name, spec)  # noqa: E731
    return [
        cm("no-spec"),
        cm("empty-lists", {"containers": [], "volumes": []}),
        cm("wrong-types", {"containers": "c-0", "volumes": {"name": "v", "emptyDir": {}}}),
        cm("scalar-list", {"containers": ["c-0", 1, None, True, ["c-1"], [{"name": "c-1"}]],
                           "volumes": [None, "emptyDir", 0]}),
        cm("null-members", {"containers": [ctr("c-0", None, securityContext=None, ports=None),
                                           ctr(None, "nginx:latest", ports=[None]),
                                           ctr("c-2", ports=[{"containerPort": None, "hostPort": None}])],
                            "volumes": [{"name": "v0", "emptyDir": None}, {"name": None, "hostPath": None}]}),
        cm("stringly", {"containers": [ctr("c-0", **sc(privileged="true", runAsNonRoot="false"),
                                           ports=[{"containerPort": "8080", "hostPort": "8060"}]),
                                       ctr("c-1", **sc(privileged="false", allowPrivilegeEscalation="false",
                                                       runAsNonRoot="false"),
                                           ports=[{"containerPort": 8080.0, "hostPort": 0}]),
                                       ctr("c-2", **sc(privileged=0), ports=[{"containerPort": 0, "hostPort": 8005.5}])],
                        "volumes": [{"name": "v0", "emptyDir": "x"}, {"name": "v1", "hostPath": 0}]}),
        cm("falsy-privileged", {"containers": [ctr("c-0", **sc(privileged="")), ctr("c-1", **sc(privileged=[])),
                                               ctr("c-2", **sc(privileged={})), ctr("c-3", **sc(privileged=[0]))],
                                "volumes": [{"name": "v0", "emptyDir": {}}, {"name": "v1", "emptyDir": []},
                                            {"name": "v2", "hostPath": ""}]}),
        cm("duplicates", {"containers": [ctr("c-1", "nginx:latest"), ctr("c-1", "redis:latest"), ctr("c-2"),
                                         ctr("c-2", "busybox:latest", **sc(privileged=True))],
                          "volumes": [{"name": "v", "emptyDir": {}}, {"name": "v", "emptyDir": {"medium": "Memory"}}]}),
        cm("non-ascii", {"containers": [ctr("ç-0", "nginx:läte:latest"), ctr("c-1", "ngïnx:1.2a:1.x"),
                                        ctr("c-2", "a:1.", **sc(capabilities={"add": ["SYS_ADMIN", "ÄLL"],
                                                                              "drop": ["ÄLL", "ALL"]}))],
                         "volumes": [{"name": "vö", "emptyDir": {}}]}),
        cm("caps-shapes", {"containers": [ctr("c-0", **sc(capabilities={"add": "SYS_ADMIN", "drop": "ALL"})),
                                          ctr("c-2", **sc(capabilities={"add": [["SYS_ADMIN"]], "drop": [None, 1]}))]}),
        cm("caps-first", {"containers": [ctr("c-0", **sc(capabilities={"add": ["NET_ADMIN", "SYS_ADMIN", "SYS_ADMIN"],
                                                                      "drop": []})),
                                         ctr("c-1", **sc(capabilities={"add": ["SYS_ADMIN"]}))]}),
        cm("drop-not-array", {"containers": [ctr("c-0", **sc(capabilities={"drop": {"ALL": 1}}))]}),
        cm("sc-not-object", {"containers": [ctr("c-0", securityContext="privileged")]}),
        cm("image-not-string", {"containers": [ctr("c-0", 7)]}),
        _doc("Pod", "two-privileged", {
            "containers": [ctr("c-0", "nginx:latest", **sc(privileged=True, runAsNonRoot=True,
                                                           allowPrivilegeEscalation=True),
                               ports=[{"containerPort": 8080, "hostPort": 8060}]),
                           ctr("c-1", "redis:latest", **sc(privileged=True, runAsNonRoot=False),
                               ports=[{"containerPort": 8080}]),
                           ctr("c-2", "busybox:1.36", **sc(privileged=False, capabilities={"add": ["SYS_ADMIN"],
                                                                                           "drop": ["ALL"]}))],
            "volumes": [{"name": "scratch", "emptyDir": {}}, {"name": "host", "hostPath": {"path": "/var"}}]}),
    ]


def edge_ndjson():
    return b"\n".join(json.dumps(d).encode() for d in edge_documents())
