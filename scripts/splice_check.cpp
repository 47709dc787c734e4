// Host run of the pass of kpe_results_splice (kyverno_amd/csrc/splice.inl, the text
// kpe_splice_kernel runs) under ASan / UBSan: the 256 lanes of each block in turn, phase by phase
// where the kernel has a barrier, over heap buffers of exactly N x Ro, N x Rs, N x rn and N bytes and
// an "LDS" of exactly the bytes the launcher requests, each carve its own allocation, so a read or
// write past a matrix, a misaligned 16-byte access or an LDS offset past its carve is a sanitizer
// report or a failed check here, before the kernel ever runs on a device.
//
//   splice_check <case> <out>
// case: u64 n, u32 Ro, u32 Rs, u32 rn, u32 grid, i32 plan[rn], i32 partner[Rs], u8 always[Rs],
// u8 kept[n * Ro], u8 sub[n * Rs]. Writes the n x rn bytes of K' and then the n flag bytes; exits
// non-zero when they differ from the rule of include/kpe.h stated directly
// (tests/test_splice_host.py compares them with kpe_results_splice_host).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(x)                                                      \
  do {                                                                \
    if (!(x)) {                                                       \
      fprintf(stderr, "splice_check: %s (line %d)\n", #x, __LINE__);  \
      exit(2);                                                        \
    }                                                                 \
  } while (0)

static uint64_t g_stores16 = 0;
#define KPE_SPLICE_FN static inline
#define KPE_SPLICE_DEV static inline
static inline void splice_load16(const uint8_t* p, uint32_t cnt, uint32_t* w) {
  CHECK(((uintptr_t)p & 15u) == 0 && cnt >= 1 && cnt <= 16);
  w[0] = w[1] = w[2] = w[3] = 0;
  memcpy(w, p, cnt);  // the device reads 16 bytes only when cnt == 16
}
static inline void splice_store16(uint8_t* p, const uint32_t* w) {
  CHECK(((uintptr_t)p & 15u) == 0);
  memcpy(p, w, 16);
  ++g_stores16;
}
static inline void splice_lds_store16(uint8_t* p, const uint32_t* w) {
  CHECK(((uintptr_t)p & 15u) == 0);
  memcpy(p, w, 16);
}
static inline void splice_lds_load16(const uint8_t* p, uint32_t* w) {
  CHECK(((uintptr_t)p & 15u) == 0);
  memcpy(w, p, 16);
}
#include "../kyverno_amd/csrc/splice.inl"

template <class T>
static T* exact(size_t n) {  // exactly n elements, 16-byte aligned like a device allocation
  const size_t bytes = n * sizeof(T);
  T* p = static_cast<T*>(malloc(bytes ? bytes : 1));
  CHECK(p && ((uintptr_t)p & 15u) == 0);
  return p;
}

int main(int argc, char** argv) {
  if (argc != 3) return fprintf(stderr, "usage: splice_check <case> <out>\n"), 2;
  FILE* f = fopen(argv[1], "rb");
  CHECK(f);
  uint64_t n;
  uint32_t hdr[4];
  CHECK(fread(&n, 8, 1, f) == 1 && fread(hdr, 4, 4, f) == 4);
  const uint32_t Ro = hdr[0], Rs = hdr[1], rn = hdr[2], grid = hdr[3];
  CHECK(grid >= 1 && Ro <= kSpliceMaxRules && Rs <= kSpliceMaxRules && rn <= kSpliceMaxRules);
  std::vector<int32_t> plan(rn), partner(Rs);
  std::vector<uint8_t> always(Rs);
  uint8_t* kept = exact<uint8_t>(n * Ro);
  uint8_t* sub = exact<uint8_t>(n * Rs);
  uint8_t* out = exact<uint8_t>(n * rn);
  uint8_t* flags = exact<uint8_t>(n);
  CHECK(fread(plan.data(), 4, rn, f) == rn && fread(partner.data(), 4, Rs, f) == Rs && fread(always.data(), 1, Rs, f) == Rs);
  CHECK(fread(kept, 1, n * Ro, f) == n * Ro && fread(sub, 1, n * Rs, f) == n * Rs);
  fclose(f);
  memset(flags, 0xEE, n);
  memset(out, 0xEE, n * rn);
  std::vector<uint8_t> written(n * rn, 0);  // a cell of K' is written once

  // the tables as api_results.cpp builds them
  std::vector<uint32_t> col(2 * (size_t)rn, 0);
  std::vector<uint8_t> unm(Ro, 1), emitted(Rs, 0);
  for (uint32_t s = 0; s < Rs; ++s) {
    CHECK(partner[s] >= -1 && (partner[s] < 0 || ((uint32_t)partner[s] < Ro && unm[partner[s]])));
    if (partner[s] >= 0) unm[partner[s]] = 0;
  }
  for (uint32_t r = 0; r < rn; ++r) {
    if (plan[r] >= 0) {
      CHECK((uint32_t)plan[r] < Ro && unm[plan[r]] == 1);
      unm[plan[r]] = 2;  // copied
      col[2 * r] = (uint32_t)plan[r];
    } else {
      const uint32_t s = (uint32_t)(-1 - plan[r]);
      CHECK(s < Rs && !emitted[s]);
      emitted[s] = 1;
      col[2 * r] = kSpliceFromSub | s;
      col[2 * r + 1] = (partner[s] < 0 ? kSpliceNone : (uint32_t)partner[s]) | ((uint32_t)always[s] << 16);
    }
  }
  bool any_unm = false;
  for (uint8_t& u : unm) u = u == 1 ? 1 : 0, any_unm |= u != 0;
  for (uint32_t s = 0; s < Rs; ++s) CHECK(emitted[s]);

  const uint32_t rpg = splice_rows_per_group(Ro, Rs, rn);
  const SpliceLds L = splice_lds(Ro, Rs, rn, rpg);
  CHECK(L.total <= 64u * 1024u && L.e_off % 16 == 0 && L.o_off % 16 == 0 && L.flag_off % 16 == 0 && L.col_off % 16 == 0 &&
        L.unm_off % 16 == 0);
  const uint64_t ngroups = n ? (n + rpg - 1) / rpg : 0;
  for (uint32_t b = 0; b < grid && b < ngroups; ++b) {
    // each carve its own exact allocation: an offset past a carve is a heap overflow
    uint8_t* s_k = exact<uint8_t>(L.k_bytes);
    uint8_t* s_e = exact<uint8_t>(L.e_bytes);
    uint8_t* s_o = exact<uint8_t>(L.o_bytes);
    uint32_t* s_flag = exact<uint32_t>(rpg);
    uint32_t* s_col = exact<uint32_t>(2 * (size_t)rn);
    uint8_t* s_unm = exact<uint8_t>(Ro);
    memset(s_k, 0xCC, L.k_bytes), memset(s_e, 0xCC, L.e_bytes), memset(s_o, 0xCC, L.o_bytes);
    if (rn) memcpy(s_col, col.data(), col.size() * 4);
    if (Ro) memcpy(s_unm, unm.data(), Ro);
    for (uint64_t g = b; g < ngroups; g += grid) {
      const SpliceGroup G = splice_group(g, n, Ro, Rs, rn, rpg);
      CHECK(G.r0 + G.rows <= n && G.k.b1 <= n * Ro && G.e.b1 <= n * Rs && G.o.b1 <= n * rn);
      CHECK(G.k.skew < 16 && G.e.skew < 16 && G.o.skew < 16);
      CHECK(G.k.b1 - G.k.b0 <= kSpliceTile && G.e.b1 - G.e.b0 <= kSpliceTile && G.o.b1 - G.o.b0 <= kSpliceTile);
      for (uint32_t t = 0; t < 256; ++t) splice_stage(G, t, kept, sub, s_k, s_e, s_flag);
      for (uint32_t t = 0; t < 256; ++t) {
        splice_build(G, t, Ro, Rs, rn, s_col, s_k, s_e, s_o, s_flag);
        if (any_unm) splice_sweep(G, t, Ro, s_unm, s_k, s_flag);
      }
      for (uint32_t i = 0; i < G.rows; ++i) CHECK(flags[G.r0 + i] == 0xEE);  // a row's byte is written once
      // the group's cells are untouched before its write and only they change in it
      // (the 16-byte lines it shares with its neighbours are what a wide store could spill into)
      const uint64_t lo = G.o.b0 < 16 ? 0 : G.o.b0 - 16, hi = G.o.b1 + 16 < n * rn ? G.o.b1 + 16 : n * rn;
      std::vector<uint8_t> before(out + lo, out + hi);
      for (uint32_t t = 0; t < 256; ++t) splice_write(G, t, s_o, s_flag, out, flags);
      for (uint64_t c = lo; c < hi; ++c) {
        const bool own = c >= G.o.b0 && c < G.o.b1;
        if (own) {
          CHECK(!written[c]);
          written[c] = 1;
        } else {
          CHECK(out[c] == before[c - lo]);
        }
      }
    }
    free(s_k), free(s_e), free(s_o), free(s_flag), free(s_col), free(s_unm);
  }

  // the rule, stated directly
  uint64_t bad = 0, changed = 0;
  for (uint64_t i = 0; i < n; ++i) {
    bool ch = false, cells = true;
    for (uint32_t r = 0; r < rn; ++r) {
      const uint8_t want = plan[r] >= 0 ? kept[i * Ro + plan[r]] : sub[i * Rs + (uint32_t)(-1 - plan[r])];
      cells &= out[i * rn + r] == want && written[i * rn + r];
    }
    for (uint32_t s = 0; s < Rs; ++s) {
      const uint8_t x = sub[i * Rs + s], o = partner[s] >= 0 ? kept[i * Ro + partner[s]] : 0;
      ch |= x != o || (x < 8 && ((always[s] >> x) & 1));
    }
    for (uint32_t o = 0; o < Ro; ++o) ch |= unm[o] && kept[i * Ro + o] != 0;
    changed += ch;
    if ((flags[i] != (ch ? 1 : 0) || !cells) && bad++ < 5)
      fprintf(stderr, "splice_check: row %llu: flag %u, want %d, cells %s\n", (unsigned long long)i, flags[i], (int)ch,
              cells ? "ok" : "differ");
  }
  FILE* o = fopen(argv[2], "wb");
  CHECK(o && fwrite(out, 1, n * rn, o) == n * rn && fwrite(flags, 1, n, o) == n);
  fclose(o);
  printf("n=%llu Ro=%u Rs=%u rn=%u rpg=%u groups=%llu lds=%u stores16=%llu changed=%llu bad=%llu\n", (unsigned long long)n,
         Ro, Rs, rn, rpg, (unsigned long long)ngroups, L.total, (unsigned long long)g_stores16, (unsigned long long)changed,
         (unsigned long long)bad);
  free(kept), free(sub), free(out), free(flags);
  return bad ? 1 : 0;
}
