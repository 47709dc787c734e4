// Host check of the in-place namespace label change (kyverno_amd/csrc/flatten.cpp set_ns_labels,
// ns_labels_json: the host half of kpe_corpus_set_namespace_labels), for tests/test_ns_relabel_host.py
// without a GPU and under the sanitizers. Not part of libkpe:
//   scripts/build/nsl_check
// Over corpora of 0, 1 and 3000 rows (namespaced rows, a cluster-scoped row and a Namespace object
// among them) flattened with a table L0: a patch that changes, removes and adds entries with label
// strings no dictionary held, then a replace, then an emptied table. After each step the table and
// every row's table row must equal, by namespace name and label strings (ids differ: new strings
// are appended), those of a fresh flatten of the same NDJSON with the resulting table. Prints
// "nsl_check ok" and exits 0, or the first difference and 1.
#include <cstdint>
#include <cstdio>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../kyverno_amd/csrc/corpus.hpp"
#include "../kyverno_amd/csrc/schema.h"

namespace kpe {
void flatten_ndjson(Corpus& C, const char* buf, size_t len, const char* nsl, size_t nsl_len, bool docs);
uint64_t set_ns_labels(Corpus& C, const char* js, size_t len, bool replace, std::vector<uint32_t>* group_map);
std::string ns_labels_json(const Corpus& C);
}  // namespace kpe

using namespace kpe;
using Labels = std::vector<std::pair<std::string, std::string>>;

static int g_bad = 0;
#define CHECK(c, ...)                 \
  do {                                \
    if (!(c)) {                       \
      if (!g_bad) {                   \
        fprintf(stderr, "nsl_check: "); \
        fprintf(stderr, __VA_ARGS__); \
        fprintf(stderr, "\n");        \
      }                               \
      ++g_bad;                        \
    }                                 \
  } while (0)

static std::string ndjson(int n) {
  std::string s;
  for (int i = 0; i < n; ++i) {
    char b[256];
    if (i % 97 == 5)  // cluster-scoped: no metadata.namespace
      snprintf(b, sizeof b, "{\"apiVersion\":\"v1\",\"kind\":\"PersistentVolume\",\"metadata\":{\"name\":\"pv-%d\"}}", i);
    else if (i % 97 == 6 || n == 1)  // a Namespace object, named like a namespace of the table
      snprintf(b, sizeof b, "{\"apiVersion\":\"v1\",\"kind\":\"Namespace\",\"metadata\":{\"name\":\"ns-%d\"}}", i % 40);
    else
      snprintf(b, sizeof b,
               "{\"apiVersion\":\"v1\",\"kind\":\"Pod\",\"metadata\":{\"name\":\"p-%d\",\"namespace\":\"ns-%d\",\"labels\":"
               "{\"app\":\"a%d\"}},\"spec\":{\"containers\":[{\"name\":\"c\",\"image\":\"x\"}]}}",
               i, i % 53, i % 7);
    s += b;
    s += '\n';
  }
  return s;
}

// the table by namespace name
static std::map<std::string, Labels> table_of(const Corpus& C) {
  std::map<std::string, Labels> out;
  for (const auto& kv : C.nsl_index) {
    Labels l;
    for (uint32_t j = C.nsl_off[kv.second]; j < C.nsl_off[kv.second + 1]; ++j)
      l.emplace_back(std::string(C.dict[D_LABK].at(C.nsl_k[j])), std::string(C.dict[D_LABV].at(C.nsl_v[j])));
    out[kv.first] = l;
  }
  return out;
}

// row i's table entry: (has one, its namespace name as the table row says, its labels)
static bool row_entry(const Corpus& C, const std::map<uint32_t, std::string>& name_of_row, size_t i, std::string* ns,
                      Labels* l) {
  const uint32_t row = C.r_nsl[i];
  if (row == KPE_NO_STR) return false;
  *ns = name_of_row.at(row);
  l->clear();
  for (uint32_t j = C.nsl_off[row]; j < C.nsl_off[row + 1]; ++j)
    l->emplace_back(std::string(C.dict[D_LABK].at(C.nsl_k[j])), std::string(C.dict[D_LABV].at(C.nsl_v[j])));
  return true;
}

static void same_as_fresh(const Corpus& C, const std::string& nd, const char* what, int n) {
  const std::string js = ns_labels_json(C);
  Corpus F;
  flatten_ndjson(F, nd.data(), nd.size(), js.data(), js.size(), false);
  CHECK(F.n == C.n && C.r_nsl.size() == (size_t)C.n, "%s n=%d: row counts", what, n);
  CHECK(table_of(F) == table_of(C), "%s n=%d: the table differs from a fresh flatten's", what, n);
  CHECK(F.nsl_off.size() == C.nsl_off.size(), "%s n=%d: table rows %zu, fresh %zu", what, n, C.nsl_off.size() - 1,
        F.nsl_off.size() - 1);
  std::map<uint32_t, std::string> nc, nf;
  for (const auto& kv : C.nsl_index) nc[kv.second] = kv.first;
  for (const auto& kv : F.nsl_index) nf[kv.second] = kv.first;
  for (size_t i = 0; i < (size_t)C.n && i < (size_t)F.n; ++i) {
    std::string a, b;
    Labels la, lb;
    const bool ha = row_entry(C, nc, i, &a, &la), hb = row_entry(F, nf, i, &b, &lb);
    CHECK(ha == hb && a == b && la == lb, "%s n=%d: row %zu has entry %d (%s), fresh %d (%s)", what, n, i, (int)ha,
          a.c_str(), (int)hb, b.c_str());
    // and it is the entry of the row's own namespace
    const std::string own(C.dict[D_NS].at(C.r_nsa[i]));
    CHECK(!ha || a == own, "%s n=%d: row %zu of namespace %s reads the entry of %s", what, n, i, own.c_str(), a.c_str());
    CHECK(ha == (C.nsl_index.count(own) != 0), "%s n=%d: row %zu, namespace %s: entry presence", what, n, i, own.c_str());
  }
  // D_NS and the namespace ids belong to the rows alone
  CHECK(F.dict[D_NS].size() == C.dict[D_NS].size() && F.r_nsa == C.r_nsa, "%s n=%d: D_NS or r_nsa moved", what, n);
}

static uint64_t set(Corpus& C, const std::string& js, bool replace) {
  return set_ns_labels(C, js.data(), js.size(), replace, nullptr);
}

int main() {
  std::string L0 = "{";
  for (int g = 0; g < 45; ++g) {
    char b[160];
    snprintf(b, sizeof b, "%s\"ns-%d\":{\"env\":\"%s\",\"team\":\"team-%d\",\"n\":7}", g ? "," : "", g,
             g % 3 ? "prod" : "dev", g % 5);
    L0 += b;
  }
  L0 += ",\"\":{\"scope\":\"cluster\"}}";  // an entry under the name cluster-scoped rows carry
  for (int n : {0, 1, 3000}) {
    const std::string nd = ndjson(n);
    Corpus C;
    flatten_ndjson(C, nd.data(), nd.size(), L0.data(), L0.size(), false);
    const uint32_t G = C.dict[D_NS].size(), nk = C.dict[D_LABK].size(), nv = C.dict[D_LABV].size();
    same_as_fresh(C, nd, "flattened", n);
    // nothing really changes: same sets in another order, a removal of what is not there
    CHECK(set(C, "{\"ns-1\":{\"team\":\"team-1\",\"env\":\"prod\"},\"nowhere\":null}", false) == 0, "n=%d: equal set", n);
    // patch: changed values, new keys and values (no dictionary holds them), a removed entry, an
    // added one that rows use (ns-50) and one no row uses, a key twice (the last occurrence counts)
    const uint64_t ch = set(C,
                            "{\"ns-0\":{\"env\":\"staging\",\"tier-\\u00e9\":\"gold \\\"q\\\"\"},\"ns-2\":null,"
                            "\"ns-50\":{\"fresh-key\":\"fresh-value\"},\"unused-ns\":{\"a\":\"b\"},"
                            "\"ns-3\":{\"x\":\"1\"},\"ns-3\":{\"env\":\"qa\",\"skipped\":3},\"ns-4\":7}",
                            false);
    CHECK(ch == 6, "n=%d: patch changed %llu entries, expected 6", n, (unsigned long long)ch);
    CHECK(C.dict[D_LABK].size() > nk && C.dict[D_LABV].size() > nv, "n=%d: no new label strings interned", n);
    CHECK(C.dict[D_NS].size() == G, "n=%d: D_NS grew", n);
    same_as_fresh(C, nd, "patched", n);
    {
      const auto t = table_of(C);
      CHECK(!t.count("ns-2") && t.count("unused-ns") && t.count("ns-4") && t.at("ns-4").empty(), "n=%d: patch entries", n);
      const Labels ns3{{"env", "qa"}}, ns1{{"env", "prod"}, {"team", "team-1"}};
      CHECK(t.count("ns-3") && t.at("ns-3") == ns3, "n=%d: duplicate key", n);
      CHECK(t.count("ns-1") && t.at("ns-1") == ns1, "n=%d: untouched entry", n);
    }
    // malformed: nothing changes
    const std::string before = ns_labels_json(C);
    for (const char* bad : {"{\"ns-1\":{\"a\":\"b\"}", "[1]", "{\"ns-1\":{\"a\":}}", "\"x\""}) {
      bool threw = false;
      try {
        set(C, bad, false);
      } catch (const std::invalid_argument&) {
        threw = true;
      }
      CHECK(threw, "n=%d: %s accepted", n, bad);
      CHECK(ns_labels_json(C) == before, "n=%d: %s changed the table", n, bad);
    }
    // replace by the getter's text is the identity; by another table it is that table
    CHECK(set(C, before, true) == 0 && ns_labels_json(C) == before, "n=%d: round trip", n);
    const uint64_t rc = set(C, "{\"ns-7\":{\"only\":\"one\"},\"ns-0\":{\"tier-\\u00e9\":\"gold \\\"q\\\"\",\"env\":\"staging\"}}", true);
    // 47 entries before; ns-0 keeps its set (in another order), ns-7 changes, 45 go
    CHECK(rc == 46, "n=%d: replace changed %llu entries, expected 46", n, (unsigned long long)rc);
    CHECK(table_of(C).size() == 2, "n=%d: replaced table holds %zu entries", n, table_of(C).size());
    same_as_fresh(C, nd, "replaced", n);
    // emptied, then given one again
    CHECK(set(C, "{}", true) == 2 && C.nsl_off.size() == 1 && C.nsl_index.empty(), "n=%d: emptied", n);
    for (size_t i = 0; i < (size_t)C.n; ++i) CHECK(C.r_nsl[i] == KPE_NO_STR, "n=%d: row %zu keeps a table row", n, i);
    same_as_fresh(C, nd, "emptied", n);
    CHECK(set(C, L0, false) == 46, "n=%d: refilled", n);
    same_as_fresh(C, nd, "refilled", n);
  }
  if (g_bad) {
    fprintf(stderr, "nsl_check: %d checks failed\n", g_bad);
    return 1;
  }
  printf("nsl_check ok\n");
  return 0;
}
