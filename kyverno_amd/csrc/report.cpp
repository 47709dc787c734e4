// C-ABI implementation (include/kpe.h): report rendering and the CLI summaries. String handling
// over the compiled program's report records, caller-supplied resource JSON and the trace words a
// fetch returned; no device call and no HIP header (api_internal.h's host part only), so this file
// also builds for the host sanitizer check (scripts/report_check.cpp).
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <string_view>
#include <thread>
#include <vector>

#include "api_internal.h"
#include "pss_msg.hpp"

using kpe::fail;
using kpe::fe_decider;
using kpe::kCvCheck;
using kpe::ns_groups;
using kpe::report_need_tables;
using kpe::report_rows_args;

// versioned check -> PSA check id (schema.h), and the ids' names
const uint8_t kpe::kCvCheck[KPE_NUM_CV] = KPE_CV_CHECK_TABLE;
static const char* const kCheckIds[KPE_NUM_CHECKS] = {
    "allowPrivilegeEscalation", "appArmorProfile", "capabilities_baseline", "capabilities_restricted",
    "hostNamespaces", "hostPathVolumes", "hostPorts", "privileged", "procMount", "restrictedVolumes",
    "runAsNonRoot", "runAsUser", "seLinuxOptions", "seccompProfile_baseline", "seccompProfile_restricted",
    "sysctls", "windowsHostProcess"};

namespace kpe {
// The foreach entry that decided a FAIL / ERROR cell from its trace words (schema.h FT_*): the
// entry index in Program::fe_reports, or -1 (no valid path)
int64_t fe_decider(const kpe::Program& P, const kpe::RuleReport& rr, uint32_t b) {
  if (!rr.foreach || !(b & FT_VALID) || (b & FT_OVERFLOW)) return -1;
  uint32_t first = rr.fe0, count = rr.nfe;
  int64_t e = -1;
  for (uint32_t l = 0; l <= FT_DEPTH(b); ++l) {
    const uint32_t left = FT_LEFT(b, l);
    if (left == 0 || left > count) return -1;
    e = (int64_t)first + (count - left);
    if ((size_t)e >= P.fe_reports.size()) return -1;
    if (l < FT_DEPTH(b)) {
      const kpe::FeReport& f = P.fe_reports[(size_t)e];
      if (f.kind != FE_NEST) return -1;
      first = f.nested0, count = f.nnested;
    }
  }
  return e;
}

// the argument checks kpe_report_cells_host and kpe_fetch_report_rows share; records: the pattern
// kind needs pattern_traces
kpe_status report_rows_args(uint32_t flags, const kpe_report_rows* io, bool records) {
  if (!io) return fail(KPE_E_INVALID, "null argument");
  if (flags & ~(KPE_RR_MASKS | KPE_RR_COND | KPE_RR_PATTERNS)) return fail(KPE_E_INVALID, "unknown flag");
  if (((flags & KPE_RR_MASKS) && io->mask_cap && (!io->mask_cells || !io->mask_words)) ||
      ((flags & KPE_RR_COND) && io->cond_cap && (!io->cond_cells || !io->cond_words)) ||
      ((flags & KPE_RR_PATTERNS) && io->pattern_cap && (!io->pattern_cells || (records && !io->pattern_traces))))
    return fail(KPE_E_INVALID, "cap > 0 without its arrays");
  return KPE_OK;
}
// the three need tables of a call, [mask][cond][pattern]: a kind whose flag is not set selects nothing
kpe_status report_need_tables(const kpe_program* prog, uint32_t flags, std::vector<uint8_t>& need) {
  const size_t R = prog->p->rules.size();
  need.assign(3 * R + 1, 0);
  const kpe_status st = kpe_report_detail_need(prog, need.data(), need.data() + R, need.data() + 2 * R);
  if (st) return st;
  for (size_t k = 0; k < 3; ++k)
    if (!(flags & (1u << k))) memset(need.data() + k * R, 0, R);
  return KPE_OK;
}
}  // namespace kpe

extern "C" {

const char* kpe_pss_check_id(int k) { return (k >= 0 && k < KPE_NUM_CHECKS) ? kCheckIds[k] : nullptr; }
int kpe_pss_num_checks(void) { return KPE_NUM_CHECKS; }
int kpe_pss_num_cv(void) { return KPE_NUM_CV; }
int kpe_pss_cv_check(int v) { return (v >= 0 && v < KPE_NUM_CV) ? (int)kCvCheck[v] : -1; }

static void json_str(std::string& o, const std::string& s) {  // encoding/json string escaping
  static const char* hx = "0123456789abcdef";
  o += '"';
  for (unsigned char ch : s) {
    if (ch == '"' || ch == '\\') {
      o += '\\';
      o += (char)ch;
    } else if (ch == '\n') {
      o += "\\n";
    } else if (ch == '\r') {
      o += "\\r";
    } else if (ch == '\t') {
      o += "\\t";
    } else if (ch < 0x20 || ch == '<' || ch == '>' || ch == '&') {
      o += "\\u00";
      o += hx[ch >> 4];
      o += hx[ch & 15];
    } else {
      o += (char)ch;
    }
  }
  o += '"';
}

// cmd/cli/kubectl-kyverno/processor/result.go:34-68 (ResultCounts.addEngineResponse): every
// response rule is counted once per validate rule of its policy with the same name; a fail is
// a warn when the policy is unscored, or with --audit-warn when its action is Audit.
kpe_status kpe_cli_summary(const kpe_program* prog, const kpe_counts* counts, int audit_warn, kpe_cli_totals* out) {
  if (!prog || !counts || !out) return fail(KPE_E_INVALID, "null argument");
  const kpe::Program& P = *prog->p;
  *out = kpe_cli_totals{};
  for (size_t r = 0; r < P.rules.size(); ++r) {
    const kpe::RuleReport& rr = P.reports[r];
    const uint64_t m = rr.name_mult;
    if (!m) continue;
    if (audit_warn && rr.overrides && rr.scored && counts[r].fail)
      return fail(KPE_E_UNSUPPORTED, "validationFailureActionOverrides with --audit-warn (per-namespace action)");
    out->pass += m * counts[r].pass;
    out->error += m * counts[r].error;
    out->skip += m * counts[r].skip;
    out->warn += m * counts[r].warn;
    if (!rr.scored || (audit_warn && rr.audit)) out->warn += m * counts[r].fail;
    else out->fail += m * counts[r].fail;
  }
  return KPE_OK;
}

// kpe_cli_summary with the action resolved per namespace group (engineresponse.go:196-225 through
// kpe::vfa_audit): counts is the G x R table of kpe_fetch_namespace_counts / kpe_namespace_counts_host.
kpe_status kpe_cli_summary_ns(const kpe_program* prog, const kpe_corpus* c, const kpe_ns_counts* counts,
                              int audit_warn, kpe_cli_totals* out) {
  if (!prog || !c || !counts || !out) return fail(KPE_E_INVALID, "null argument");
  const kpe::Program& P = *prog->p;
  const kpe::Corpus& C = *c->c;
  const NsGroups& G = ns_groups(c);
  const size_t R = P.rules.size();
  *out = kpe_cli_totals{};
  std::vector<int8_t> audit(P.vfa_overrides.size());  // per policy, for this group: -1 not resolved yet
  std::vector<std::pair<std::string, std::string>> labels;
  for (size_t g = 0; g < G.names.size(); ++g) {
    std::fill(audit.begin(), audit.end(), (int8_t)-1);
    bool have_labels = false;
    for (size_t r = 0; r < R; ++r) {
      const kpe::RuleReport& rr = P.reports[r];
      const uint64_t m = rr.name_mult;
      if (!m) continue;
      const kpe_ns_counts& k = counts[g * R + r];
      out->pass += m * k.pass;
      out->error += m * k.error;
      out->skip += m * k.skip;
      out->warn += m * k.warn;
      if (!k.fail) continue;
      bool warn = !rr.scored;
      if (!warn && audit_warn) {
        if (!rr.overrides || rr.policy >= audit.size()) {
          warn = rr.audit;
        } else {
          if (audit[rr.policy] < 0) {
            if (!have_labels) {  // PolicyContext.NamespaceLabels of the group's name (none: empty)
              labels.clear();
              auto it = C.nsl_index.find(G.names[g]);
              if (it != C.nsl_index.end() && (size_t)it->second + 1 < C.nsl_off.size())
                for (uint32_t j = C.nsl_off[it->second]; j < C.nsl_off[it->second + 1]; ++j)
                  labels.emplace_back(std::string(C.dict[D_LABK].at(C.nsl_k[j])), std::string(C.dict[D_LABV].at(C.nsl_v[j])));
              std::stable_sort(labels.begin(), labels.end(),
                               [](const auto& a, const auto& b) { return a.first < b.first; });
              // a repeated key of the table's JSON object: the last one is the map's value
              for (size_t j = 0; j + 1 < labels.size();)
                if (labels[j].first == labels[j + 1].first) labels.erase(labels.begin() + (long)j);
                else ++j;
              have_labels = true;
            }
            audit[rr.policy] = kpe::vfa_audit(P, rr.policy, rr.audit, G.names[g], labels) ? 1 : 0;
          }
          warn = audit[rr.policy] != 0;
        }
      }
      (warn ? out->warn : out->fail) += m * k.fail;
    }
  }
  return KPE_OK;
}

// The PatternError.Path of a trace record (validate.go: "/" then each key or index followed by
// "/"); false when the record is truncated
static bool trace_path(const kpe::Program& P, const kpe::Corpus* C, const uint32_t* t, std::string* out) {
  if (t[0] & KPE_TR_TRUNC) return false;
  const uint32_t n = t[0] & 0xFFu;
  std::string p = "/";
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t c = t[1 + i];
    if (c & KPE_TC_IDX) {
      p += std::to_string(c & ~KPE_TC_IDX);
    } else if (c & KPE_TC_KEY) {
      if (!C) return false;
      const uint32_t id = c & ~KPE_TC_KEY;
      if (id >= C->dict[D_KEY].size()) return false;
      p += std::string(C->dict[D_KEY].at(id));
    } else {
      if ((size_t)c * 4 + 1 >= P.pat.members.size()) return false;
      if (P.pat.members[(size_t)c * 4] & PMF_VKEY) return false;  // an absent substituted key: no text kept
      const uint32_t ki = P.pat.members[(size_t)c * 4 + 1];
      if (ki >= P.pat.keys.size()) return false;
      p += P.pat.keys[ki];
    }
    p += '/';
  }
  *out = std::move(p);
  return true;
}

// validate_resource.go:316-454: pattern / anyPattern messages from the cell's trace (roots in
// order) of rule `rule` with validate.message `vmsg` (substituted over the resource and, in a
// foreach, the element `el`); empty when the reference's text would need an error string the
// device does not keep (an empty-path PatternError, a skip) or a substituted message
static std::string pattern_msg(const kpe::Program& P, const kpe::Corpus* C, const std::string& rule,
                               const std::string& vmsg, bool any, uint32_t roots, uint8_t v, const uint32_t* tr,
                               const char* json, size_t json_len, const kpe::MsgElem* el) {
  auto root = [&](uint32_t k) { return tr + (size_t)k * KPE_TRACE_WORDS; };
  auto rv = [&](uint32_t k) { return (root(k)[0] & KPE_TR_VALID) ? (root(k)[0] >> 16) & 0xFFu : 0xFFu; };
  if (!any) {
    if (v != KPE_FAIL || rv(0) != KPE_FAIL) return "";
    std::string path;
    if (!trace_path(P, C, root(0), &path)) return "";
    if (vmsg.empty()) return "validation error: rule " + rule + " failed at path " + path;  // buildErrorMessage
    std::string m = vmsg;
    if (vmsg.find("{{") != std::string::npos || vmsg.find("$(") != std::string::npos) {
      // buildErrorMessage: SubstituteAll of the message (a non-string value: no text)
      bool nonstring = false;
      if (!kpe::substitute_message(vmsg, json, json_len, &m, &nonstring, nullptr, el) || nonstring) return "";
    }
    if (m.empty() || m.back() != '.') m += '.';
    return "validation error: " + m + " rule " + rule + " failed at path " + path;
  }
  if (v == KPE_PASS) {
    if (roots == 0) return vmsg;  // no pattern at all: RulePass(rule.Validation.Message)
    for (uint32_t k = 0; k < roots && k < KPE_TRACE_ROOTS; ++k) {
      if (rv(k) == KPE_PASS) return "validation rule '" + rule + "' anyPattern[" + std::to_string(k) + "] passed.";
      if (rv(k) == 0xFFu || rv(k) == KPE_UNDECIDED) return "";
    }
    return "";
  }
  if (v != KPE_FAIL || roots > KPE_TRACE_ROOTS) return "";
  std::string errs;
  for (uint32_t k = 0; k < roots; ++k) {
    const uint32_t x = rv(k);
    if (x == KPE_SKIP) continue;  // skipped patterns are not listed once one failed
    if (x != KPE_FAIL) return "";  // an empty-path failure's message is its error text
    std::string path;
    if (!trace_path(P, C, root(k), &path)) return "";
    errs += (errs.empty() ? "" : " ") + ("rule " + rule + "[" + std::to_string(k) + "] failed at path " + path);
  }
  if (errs.empty()) return "";
  if (vmsg.empty()) return "validation error: " + errs;  // buildAnyPatternErrorMessage
  if (vmsg.back() == '.') return "validation error: " + vmsg + " " + errs;
  return "validation error: " + vmsg + ". " + errs;
}
static std::string pattern_message(const kpe::Program& P, const kpe::Corpus* C, const kpe::RuleReport& rr, uint8_t v,
                                   const uint32_t* tr, const char* json, size_t json_len) {
  return pattern_msg(P, C, rr.rule, rr.vmsg, rr.any_pattern, rr.pat_roots, v, tr, json, json_len, nullptr);
}

// getDenyMessage (validate_resource.go:279-300) of a failing deny block whose condition message is
// `cm`: SubstituteAll of JoinNonEmpty(rule message, cm) over the context (the resource, and the
// foreach element `el`); on a substitution error the condition message as is; a message outside
// the restated variables: none
static std::string deny_msg(const std::string& rule, const std::string& vmsg, const std::string& cm, const char* json,
                            size_t n, const kpe::MsgElem* el) {
  if (vmsg.empty() && cm.empty()) return "validation error: rule " + rule + " failed";
  const std::string j = kpe::join_non_empty({vmsg, cm}, "; ");
  std::string out;
  bool nonstring = false, serr = false;
  if (!kpe::substitute_message(j, json, n, &out, &nonstring, &serr, el)) return serr ? cm : std::string();
  return nonstring ? "the produced message didn't resolve to a string, check your policy definition." : out;
}

// The document of tape entry e as JSON text (the foreach element: a node of the resource's
// document; Go's JSON context holds it with float64 numbers, which the renderers print alike)
static bool tape_json(const kpe::Corpus& C, uint32_t e, std::string& o, int depth = 0) {
  if ((size_t)e * 2 + 1 >= C.doc.size() || depth > 300) return false;
  const uint32_t x = C.doc[(size_t)e * 2], y = C.doc[(size_t)e * 2 + 1];
  auto str = [&](std::string_view t) {
    o += '"';
    for (unsigned char ch : t) {
      if (ch == '"' || ch == '\\') o += '\\', o += (char)ch;
      else if (ch < 0x20) {
        char b[8];
        snprintf(b, sizeof b, "\\u%04x", ch);
        o += b;
      } else o += (char)ch;
    }
    o += '"';
  };
  if (DN_KIND(x) == DN_SCALAR) {
    if (y >= C.scal.size()) return false;
    const KpeScalar& sc = C.scal[y];
    char b[40];
    switch (SC_TYPE(sc.flags)) {
      case SC_T_NULL: o += "null"; break;
      case SC_T_BOOL: o += (y == SC_TRUE_ID || (sc.flags & SC_BTRUE)) ? "true" : "false"; break;
      case SC_T_INT: o += std::to_string(sc.ival); break;
      case SC_T_FLOAT:
        snprintf(b, sizeof b, "%.17g", sc.fval);
        o += b;
        break;
      default: str(C.scal_text_of(y));
    }
    return true;
  }
  if ((size_t)y * 2 + 1 >= C.doc.size()) return false;
  const uint32_t cnt = C.doc[(size_t)y * 2];
  const bool map = DN_KIND(x) == DN_MAP;
  o += map ? '{' : '[';
  for (uint32_t k = 0; k < cnt; ++k) {
    const uint32_t m = y + 1 + k;
    if ((size_t)m * 2 >= C.doc.size()) return false;
    if (k) o += ',';
    if (map) {
      const uint32_t key = DN_KEY(C.doc[(size_t)m * 2]);
      if (key == 0 || key - 1 >= C.dict[D_KEY].size()) return false;
      str(C.dict[D_KEY].at(key - 1));
      o += ':';
    }
    if (!tape_json(C, m, o, depth + 1)) return false;
  }
  o += map ? '}' : ']';
  return true;
}
// %T of a tape entry as the JSON context holds it
static const char* tape_go_type(const kpe::Corpus& C, uint32_t e) {
  if ((size_t)e * 2 + 1 >= C.doc.size()) return nullptr;
  const uint32_t x = C.doc[(size_t)e * 2], y = C.doc[(size_t)e * 2 + 1];
  if (DN_KIND(x) == DN_MAP) return "map[string]interface {}";
  if (DN_KIND(x) == DN_ARR) return "[]interface {}";
  if (y >= C.scal.size()) return nullptr;
  switch (SC_TYPE(C.scal[y].flags)) {
    case SC_T_BOOL: return "bool";
    case SC_T_INT:
    case SC_T_FLOAT: return "float64";
    case SC_T_STR: return "string";
    default: return nullptr;
  }
}

// The message of a validate.foreach cell (validateForEach / validateElements,
// validate_resource.go:186-254) from its condition trace words `w` (schema.h FT_*) and, for an
// entry's pattern, the cell's pattern trace `ptr`
static std::string foreach_message(const kpe::Program& P, const kpe::Corpus* C, const kpe::RuleReport& rr, uint8_t v,
                                   const uint32_t* w, const uint32_t* ptr, const char* json, size_t n) {
  if (v == KPE_PASS) return "rule passed";  // :203
  if ((v != KPE_FAIL && v != KPE_ERROR) || !w) return "";
  const uint32_t b = w[1];
  const int64_t ei = fe_decider(P, rr, b);
  if (ei < 0) return "";
  const kpe::FeReport& f = P.fe_reports[(size_t)ei];
  const uint32_t depth = FT_DEPTH(b), ct = w[0] >> 16;
  kpe::MsgElem me;
  const kpe::MsgElem* el = nullptr;
  if (C && w[2] != 0xFFFFFFFFu && tape_json(*C, w[2], me.json)) {
    me.depth = (int)depth, me.index = FT_IDX(b, depth);
    el = &me;
  }
  std::string leaf, e;
  uint32_t wraps = depth + 1;  // validateElements wraps the response once per level
  switch (FT_KIND(b)) {
    case FT_SCOPE_ERR: {  // AddElementToContext (:218-221, utils/foreach.go:51-54): not wrapped at its level
      const char* t = C && w[2] != 0xFFFFFFFFu ? tape_go_type(*C, w[2]) : nullptr;
      if (!t) return "";
      leaf = std::string("failed to process foreach: cannot use elementScope=true foreach rules for elements that "
                         "are not maps, expected type=map got type=") + t;
      wraps = depth;
      break;
    }
    case FT_PRE_ERR:  // the element's preconditions (:125-128)
      if ((e = kpe::block_error_text(f.pre_json, ct, json, n, el)).empty()) return "";
      leaf = "failed to evaluate preconditions: " + e;
      break;
    case FT_DENY:
      if (CT_IS_ERR(ct)) {  // :269-271
        if ((e = kpe::block_error_text(f.deny_json, ct, json, n, el)).empty()) return "";
        leaf = "failed to check deny conditions: " + e;
      } else if ((ct & (CT_EVAL | CT_TRUE)) == (CT_EVAL | CT_TRUE)) {  // getDenyMessage over the element
        leaf = deny_msg(rr.rule, rr.vmsg, f.deny_msgs.render(CT_ANY(ct), CT_ALL(ct), true), json, n, el);
      }
      break;
    case FT_PVAR_ERR:  // substitutePatterns (:139-141)
      if ((e = kpe::doc_subst_error(f.pattern_json, json, n, el)).empty()) return "";
      leaf = "variable substitution failed: " + e;
      break;
    case FT_PAT:
      if (!f.any_bad_type.empty()) {  // deserializeAnyPattern (:347-350)
        leaf = "failed to deserialize anyPattern, expected type array: json: cannot unmarshal " + f.any_bad_type +
               " into Go value of type []interface {}";
      } else if (ptr) {
        leaf = pattern_msg(P, C, rr.rule, rr.vmsg, f.any, f.nroots, v, ptr, json, n, el);
      }
      break;
    default: break;
  }
  if (leaf.empty()) return "";
  for (uint32_t k = 0; k < wraps; ++k) leaf = "validation failure: " + leaf;
  return leaf;
}

static std::string deny_message(const kpe::RuleReport& rr, const std::string& cm, const char* json, size_t n) {
  return deny_msg(rr.rule, rr.deny_vmsg, cm, json, n, nullptr);
}

// the row's JSON array into o (prog and verdict_row are not null)
static void report_render(const kpe_program* prog, const kpe_corpus* corp, const uint8_t* verdict_row,
                          const uint32_t* cv_mask_row, const uint32_t* traces, const uint32_t* cond_traces,
                          const char* resource_json, size_t resource_len, const uint32_t* cond_traces_ex, std::string& o) {
  // the typed pod view for podSecurity fail messages, decoded on first use
  int pod_state = 0;  // 0 not decoded, 1 ok, -1 getSpec fails
  kpe::PodView pod;
  std::string kind;
  static const char* const kResult[6] = {nullptr, "pass", "fail", "warn", "error", "skip"};
  const kpe::Program& P = *prog->p;
  o = "[";
  bool first = true;
  for (size_t r = 0; r < P.rules.size(); ++r) {
    const uint8_t v = verdict_row[r];
    if (v == KPE_NA || v > KPE_SKIP) continue;  // no RuleResponse (KPE_UNDECIDED: the caller's)
    const kpe::RuleReport& rr = P.reports[r];
    const char* res = kResult[v];
    if (v == KPE_FAIL && !rr.scored) res = "warn";  // results.go:131-133
    o += first ? "{" : ",{";
    first = false;
    o += "\"source\":\"kyverno\",\"policy\":";
    json_str(o, rr.policy_key);
    // the skip's cause: preconditions false (folded at compile time, or the condition trace's
    // preconditions half) or the rule's PolicyException (after preconditions that held)
    const uint32_t* cx = (cond_traces_ex && rr.cond_slot) ? cond_traces_ex + r * (size_t)KPE_CTRACE_WORDS : nullptr;
    const uint32_t ct = cx ? cx[0] : (cond_traces && rr.cond_slot) ? cond_traces[r] : 0u;
    const uint32_t held = CT_EVAL | CT_TRUE;
    const bool pre_skip = v == KPE_SKIP && (rr.pre_const_skip || (ct & held) == CT_EVAL);
    const bool exc_skip = v == KPE_SKIP && !rr.exc_key.empty() && !pre_skip &&
                          (!rr.exc_after_pre || (ct & held) == held);
    if (resource_json) {  // RuleResponse message (validate_pss.go:85,108; validate_resource.go:339)
      std::string msg;
      const kpe::Corpus* C = corp ? corp->c.get() : nullptr;
      const uint32_t* ptr = traces ? traces + r * (size_t)(KPE_TRACE_ROOTS * KPE_TRACE_WORDS) : nullptr;
      std::string e;
      if (v == KPE_ERROR && rr.cond_slot && CT_IS_ERR(ct & 0xFFFFu)) {  // engine.go:279-281
        if (!(e = kpe::block_error_text(rr.pre_json, ct & 0xFFFFu, resource_json, resource_len, nullptr)).empty())
          msg = "failed to evaluate preconditions: " + e;
      } else if (rr.foreach) {
        msg = foreach_message(P, C, rr, v, cx, ptr, resource_json, resource_len);
      } else if (v == KPE_ERROR && rr.msg_deny && rr.cond_slot && CT_IS_ERR(ct >> 16)) {  // :269-271
        if (!(e = kpe::block_error_text(rr.deny_json, ct >> 16, resource_json, resource_len, nullptr)).empty())
          msg = "failed to check deny conditions: " + e;
      } else if (v == KPE_ERROR && !rr.any_bad_type.empty()) {  // :347-350
        msg = "failed to deserialize anyPattern, expected type array: json: cannot unmarshal " + rr.any_bad_type +
              " into Go value of type []interface {}";
      } else if (v == KPE_ERROR && rr.pat_vars &&
                 !(e = kpe::doc_subst_error(rr.pattern_json, resource_json, resource_len, nullptr)).empty()) {
        msg = "variable substitution failed: " + e;  // :139-141
      } else if (rr.pss && v == KPE_PASS) {
        msg = kpe::pss_pass_message(rr.rule);
      } else if (rr.pss && v == KPE_FAIL && !rr.pss_excl && cv_mask_row && (cv_mask_row[r] & KPE_CVM_CHECKS)) {
        if (!pod_state) pod_state = kpe::typed_pod_view(resource_json, resource_len, &pod, &kind) ? 1 : -1;
        if (pod_state > 0)
          msg = kpe::pss_fail_message(rr.rule, rr.pss_level, rr.pss_version, kind, pod, cv_mask_row[r] & KPE_CVM_CHECKS);
      } else if (rr.pss && v == KPE_FAIL && rr.pss_excl && cv_mask_row) {
        // the checks EvaluatePod's exclusions and, when it matched (KPE_CVM_XMATCH), the podSecurity
        // PolicyException's leave (validate_pss.go:76-110)
        if (!pod_state) pod_state = kpe::typed_pod_view(resource_json, resource_len, &pod, &kind) ? 1 : -1;
        const bool xm = rr.pss_has_xexcl && (cv_mask_row[r] & KPE_CVM_XMATCH);
        if (pod_state > 0)
          msg = kpe::pss_fail_message_ex(rr.rule, rr.pss_level, rr.pss_version, kind, pod, rr.pss_cv, &rr.pss_excludes,
                                         xm ? &rr.pss_xexcludes : nullptr);
      } else if (rr.pat_rule && traces && (v == KPE_FAIL || (v == KPE_PASS && rr.any_pattern))) {
        msg = pattern_message(P, corp ? corp->c.get() : nullptr, rr, v,
                              traces + r * (size_t)(KPE_TRACE_ROOTS * KPE_TRACE_WORDS), resource_json, resource_len);
      } else if (rr.msg_pattern && v == KPE_PASS) {
        msg = "validation rule '" + rr.rule + "' passed.";
      } else if (pre_skip) {  // engine.go:282-284
        msg = rr.pre_const_skip
                  ? rr.pre_skip_msg
                  : kpe::join_non_empty({"preconditions not met", rr.pre_msgs.render(CT_ANY(ct), CT_ALL(ct), false)}, "; ");
      } else if (rr.msg_deny && v == KPE_PASS) {
        msg = "validation rule '" + rr.rule + "' passed.";
      } else if (rr.msg_deny && v == KPE_FAIL) {
        const uint32_t dt = ct >> 16;
        if (!rr.cond_deny) msg = deny_message(rr, rr.deny_cm, resource_json, resource_len);
        else if ((dt & held) == held)
          msg = deny_message(rr, rr.deny_msgs.render(CT_ANY(dt), CT_ALL(dt), true), resource_json, resource_len);
      } else if (rr.msg_deny && rr.msg_pre_skip && v == KPE_SKIP && P.rules[r].exc == 0u) {
        msg = "preconditions not met";  // no exception: the skip is the preconditions'
      }
      if (exc_skip) msg = "rule skipped due to policy exception " + rr.exc_key;
      if (!msg.empty()) {
        o += ",\"message\":";
        json_str(o, msg);
      }
    }
    if (!rr.rule.empty()) {
      o += ",\"rule\":";
      json_str(o, rr.rule);
    }
    o += ",\"result\":\"";
    o += res;
    o += '"';
    if (rr.scored) o += ",\"scored\":true";
    // results.go:114-129: failing check ids (one per failing versioned check), sorted
    const uint32_t f = (rr.pss && v == KPE_FAIL && cv_mask_row) ? cv_mask_row[r] & KPE_CVM_CHECKS : 0u;
    if (f) {
      std::vector<std::string> ids;
      for (uint32_t b = f; b; b &= b - 1) ids.push_back(kCheckIds[kCvCheck[__builtin_ctz(b)]]);
      std::sort(ids.begin(), ids.end());
      std::string ctl;
      for (auto& id : ids) ctl += (ctl.empty() ? "" : ",") + id;
      o += ",\"properties\":{\"controls\":";
      json_str(o, ctl);
      o += ",\"standard\":";
      json_str(o, rr.pss_level);
      o += ",\"version\":";
      json_str(o, rr.pss_version);
      o += '}';
    }
    if (exc_skip && !rr.exc_name.empty()) {  // results.go:107-111: the exception's name
      o += ",\"properties\":{\"exception\":";
      json_str(o, rr.exc_name);
      o += '}';
    }
    if (!rr.category.empty()) {
      o += ",\"category\":";
      json_str(o, rr.category);
    }
    if (!rr.severity.empty()) {
      o += ",\"severity\":";
      json_str(o, rr.severity);
    }
    o += '}';
  }
  o += ']';
}

static long report_impl(const kpe_program* prog, const kpe_corpus* corp, const uint8_t* verdict_row,
                        const uint32_t* cv_mask_row, const uint32_t* traces, const uint32_t* cond_traces,
                        const char* resource_json, size_t resource_len, char* buf, size_t cap,
                        const uint32_t* cond_traces_ex) {
  if (!prog || !verdict_row) {
    fail(KPE_E_INVALID, "null argument");
    return -KPE_E_INVALID;
  }
  std::string o;
  report_render(prog, corp, verdict_row, cv_mask_row, traces, cond_traces, resource_json, resource_len, cond_traces_ex, o);
  if (buf && cap > 0) {
    const size_t n = std::min(o.size(), cap - 1);
    memcpy(buf, o.data(), n);
    buf[n] = 0;
  }
  return (long)o.size();
}

// pkg/utils/report/results.go:89-156 (EngineResponseToReportResults) for one resource row,
// over every policy of the program; toPolicyResult results.go:56-71.
long kpe_report_results(const kpe_program* prog, const uint8_t* verdict_row, const uint32_t* cv_mask_row, char* buf,
                        size_t cap) {
  return kpe_report_results_msg(prog, verdict_row, cv_mask_row, nullptr, 0, buf, cap);
}

long kpe_report_results_ex(const kpe_report_args* a, char* buf, size_t cap) {
  if (!a) {
    fail(KPE_E_INVALID, "null argument");
    return -KPE_E_INVALID;
  }
  return report_impl(a->prog, a->corpus, a->verdict_row, a->cv_mask_row, a->pattern_traces, a->cond_traces,
                     a->resource_json, a->resource_len, buf, cap, a->cond_traces_ex);
}

long kpe_report_results_msg(const kpe_program* prog, const uint8_t* verdict_row, const uint32_t* cv_mask_row,
                            const char* resource_json, size_t resource_len, char* buf, size_t cap) {
  return report_impl(prog, nullptr, verdict_row, cv_mask_row, nullptr, nullptr, resource_json, resource_len, buf, cap,
                     nullptr);
}

long kpe_report_results_msg_tr(const kpe_program* prog, const kpe_corpus* corpus, const uint8_t* verdict_row,
                               const uint32_t* cv_mask_row, const uint32_t* traces, const char* resource_json,
                               size_t resource_len, char* buf, size_t cap) {
  return report_impl(prog, corpus, verdict_row, cv_mask_row, traces, nullptr, resource_json, resource_len, buf, cap,
                     nullptr);
}

// ---- reports for a row list: which cells need detail, the bulk renderer (the sparse fetch:
// kpe_fetch_report_rows, api_results.cpp) --------------------------------------------------------
// some entry of a validate.foreach rule (nested ones included) walks a pattern
static bool fe_has_pattern(const kpe::Program& P, uint32_t first, uint32_t count, int depth = 0) {
  for (uint32_t e = first; e - first < count && e < P.fe_reports.size(); ++e) {
    const kpe::FeReport& f = P.fe_reports[e];
    if (f.kind == FE_PAT) return true;
    if (f.kind == FE_NEST && depth < 16 && fe_has_pattern(P, f.nested0, f.nnested, depth + 1)) return true;
  }
  return false;
}

// What report_render and the functions it calls read, per rule and verdict:
//   the mask word   of a FAIL cell of a podSecurity rule (controls, fail messages);
//   the trace words of a FAIL / ERROR / SKIP cell of a rule with a slot (deny messages and foreach
//                   elements, RuleError texts, the skip's cause); PASS and WARN read none;
//   the pattern record of a FAIL cell of a pattern rule, a PASS cell of an anyPattern rule, and a
//                   FAIL / ERROR cell of a foreach rule with a pattern entry.
kpe_status kpe_report_detail_need(const kpe_program* prog, uint8_t* mask_sel, uint8_t* cond_sel, uint8_t* pattern_sel) {
  if (!prog) return fail(KPE_E_INVALID, "null argument");
  const kpe::Program& P = *prog->p;
  const size_t R = P.rules.size();
  if (R && (!mask_sel || !cond_sel || !pattern_sel)) return fail(KPE_E_INVALID, "null argument");
  for (size_t r = 0; r < R; ++r) {
    const kpe::RuleReport& rr = P.reports[r];
    mask_sel[r] = rr.pss ? KPE_SEL(KPE_FAIL) : 0u;
    cond_sel[r] = rr.cond_slot ? KPE_SEL(KPE_FAIL) | KPE_SEL(KPE_ERROR) | KPE_SEL(KPE_SKIP) : 0u;
    uint32_t p = 0;
    if (rr.pat_rule) p |= KPE_SEL(KPE_FAIL) | (rr.any_pattern ? KPE_SEL(KPE_PASS) : 0u);
    if (rr.foreach && fe_has_pattern(P, rr.fe0, rr.nfe)) p |= KPE_SEL(KPE_FAIL) | KPE_SEL(KPE_ERROR);
    pattern_sel[r] = (uint8_t)p;
  }
  return KPE_OK;
}

kpe_status kpe_report_cells_host(const kpe_program* prog, uint64_t nrows, const uint8_t* verdict_rows,
                                 const uint32_t* cv_mask_rows, const uint32_t* cond_ex_rows, uint32_t flags,
                                 kpe_report_rows* io) {
  if (!prog) return fail(KPE_E_INVALID, "null argument");
  kpe_status st = report_rows_args(flags, io, false);
  if (st) return st;
  const size_t R = prog->p->rules.size();
  const uint64_t cells = nrows * R;
  if (cells && (!verdict_rows || ((flags & KPE_RR_MASKS) && !cv_mask_rows) || ((flags & KPE_RR_COND) && !cond_ex_rows)))
    return fail(KPE_E_INVALID, "null argument");
  std::vector<uint8_t> need;
  if ((st = report_need_tables(prog, flags, need))) return st;
  uint64_t nm = 0, nc = 0, np = 0;
  for (uint64_t k = 0; k < nrows; ++k)
    for (size_t r = 0; r < R; ++r) {
      const uint64_t cell = k * R + r;
      const uint32_t v = verdict_rows[cell];
      if (v >= 8u) continue;
      if ((need[r] >> v) & 1u) {
        if (nm < io->mask_cap) io->mask_cells[nm] = cell, io->mask_words[nm] = cv_mask_rows[cell];
        ++nm;
      }
      if ((need[R + r] >> v) & 1u) {
        if (nc < io->cond_cap) {
          io->cond_cells[nc] = cell;
          memcpy(io->cond_words + nc * KPE_CTRACE_WORDS, cond_ex_rows + cell * KPE_CTRACE_WORDS, KPE_CTRACE_WORDS * 4);
        }
        ++nc;
      }
      if ((need[2 * R + r] >> v) & 1u) {
        if (np < io->pattern_cap) io->pattern_cells[np] = cell;
        ++np;
      }
    }
  io->mask_total = nm, io->cond_total = nc, io->pattern_total = np;
  return KPE_OK;
}

// threads of kpe_report_results_rows: up to 16, KPE_REPORT_THREADS lowers it
static unsigned report_threads() {
  unsigned n = 16;
  if (const char* ev = getenv("KPE_REPORT_THREADS")) n = (unsigned)std::max(1, std::min(16, atoi(ev)));
  return n;
}

long kpe_report_results_rows(const kpe_program* prog, const kpe_corpus* corpus, uint64_t nrows, const kpe_report_rows* in,
                             const char* const* resources, const size_t* resource_lens, char* buf, size_t cap,
                             uint64_t* offsets) {
  if (!prog || !in || !offsets || (resources && !resource_lens)) {
    fail(KPE_E_INVALID, "null argument");
    return -KPE_E_INVALID;
  }
  const size_t R = prog->p->rules.size();
  if (nrows && R && !in->verdict_rows) {
    fail(KPE_E_INVALID, "null verdict_rows");
    return -KPE_E_INVALID;
  }
  // a list is its cells and payload, `total` entries of them; a null list has none
  const uint64_t nm = in->mask_cells && in->mask_words ? in->mask_total : 0;
  const uint64_t nc = in->cond_cells && in->cond_words ? in->cond_total : 0;
  const uint64_t np = in->pattern_cells && in->pattern_traces ? in->pattern_total : 0;
  const size_t rec = (size_t)KPE_TRACE_ROOTS * KPE_TRACE_WORDS;
  std::vector<std::string> outs(nrows);
  const unsigned T = (unsigned)std::min<uint64_t>(std::max<uint64_t>(nrows, 1), report_threads());
  std::atomic<uint64_t> next{0};
  std::atomic<bool> bad{false};
  // Rows in blocks of 64, handed out dynamically. A thread expands the row's entries of each list
  // (ascending cells: the entries of row k are one run) into dense rows of its own, renders with the
  // per-row renderer, and clears what it set. A row without an entry in a list renders without that
  // input, as the per-row call with NULL for it does.
  auto work = [&]() {
    std::vector<uint32_t> mrow(nm ? R : 0, 0u), crow(nc ? R * KPE_CTRACE_WORDS : 0, 0u), prow(np ? R * rec : 0, 0u);
    try {
      for (uint64_t b; (b = next.fetch_add(64)) < nrows;)
        for (uint64_t k = b; k < std::min(nrows, b + 64); ++k) {
          const uint64_t c0 = k * R, c1 = c0 + R;
          const uint64_t* m0 = std::lower_bound(in->mask_cells, in->mask_cells + nm, c0);
          const uint64_t* q0 = std::lower_bound(in->cond_cells, in->cond_cells + nc, c0);
          const uint64_t* p0 = std::lower_bound(in->pattern_cells, in->pattern_cells + np, c0);
          const uint64_t *m1 = m0, *q1 = q0, *p1 = p0;
          for (; m1 < in->mask_cells + nm && *m1 >= c0 && *m1 < c1; ++m1)
            mrow[*m1 - c0] = in->mask_words[m1 - in->mask_cells];
          for (; q1 < in->cond_cells + nc && *q1 >= c0 && *q1 < c1; ++q1)
            memcpy(&crow[(*q1 - c0) * KPE_CTRACE_WORDS], in->cond_words + (q1 - in->cond_cells) * KPE_CTRACE_WORDS,
                   KPE_CTRACE_WORDS * 4);
          for (; p1 < in->pattern_cells + np && *p1 >= c0 && *p1 < c1; ++p1)
            memcpy(&prow[(*p1 - c0) * rec], in->pattern_traces + (p1 - in->pattern_cells) * rec, rec * 4);
          const char* res = resources ? resources[k] : nullptr;
          report_render(prog, corpus, in->verdict_rows + c0, m1 != m0 ? mrow.data() : nullptr,
                        p1 != p0 ? prow.data() : nullptr, nullptr, res, res ? resource_lens[k] : 0,
                        q1 != q0 ? crow.data() : nullptr, outs[k]);
          for (const uint64_t* x = m0; x < m1; ++x) mrow[*x - c0] = 0u;
          for (const uint64_t* x = q0; x < q1; ++x) memset(&crow[(*x - c0) * KPE_CTRACE_WORDS], 0, KPE_CTRACE_WORDS * 4);
          for (const uint64_t* x = p0; x < p1; ++x) memset(&prow[(*x - c0) * rec], 0, rec * 4);
        }
    } catch (...) {
      bad = true;
      next = nrows;
    }
  };
  if (T <= 1) {
    work();
  } else {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < T; ++t) th.emplace_back(work);
    for (auto& x : th) x.join();
  }
  if (bad) {
    fail(KPE_E_INVALID, "report rendering failed");
    return -KPE_E_INVALID;
  }
  uint64_t total = 0;
  for (uint64_t k = 0; k < nrows; ++k) offsets[k] = total, total += outs[k].size();
  offsets[nrows] = total;
  if (buf && total < cap) {
    for (uint64_t k = 0; k < nrows; ++k) memcpy(buf + offsets[k], outs[k].data(), outs[k].size());
    buf[total] = 0;
  }
  return (long)total;
}

}  // extern "C"
