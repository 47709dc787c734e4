// Host run of the flag pass of kpe_changed_rows (kyverno_amd/csrc/delta.inl, the text
// kpe_delta_flags_kernel runs) under ASan / UBSan: the 256 lanes of each block in turn, phase by
// phase where the kernel has a barrier, over heap buffers of exactly N x Ro and N x Rn bytes and an
// "LDS" of exactly the bytes the launcher requests, so a read past a matrix, a misaligned 16-byte
// access or an LDS offset past its carve is a sanitizer report or a failed check here, before the
// kernel ever runs on a device.
//
//   delta_check <case> <flags-out>
// case: u64 n, u32 Ro, u32 Rn, u32 grid, u32 0, i32 old_of[Rn], u8 always[Rn], u8 old[n * Ro],
// u8 new[n * Rn]. Writes the n flag bytes; exits non-zero when they differ from the rule of
// include/kpe.h stated directly (tests/test_delta_host.py compares them with kpe_changed_rows_host).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(x)                                                      \
  do {                                                                \
    if (!(x)) {                                                       \
      fprintf(stderr, "delta_check: %s (line %d)\n", #x, __LINE__);   \
      exit(2);                                                        \
    }                                                                 \
  } while (0)

#define KPE_DELTA_FN static inline
#define KPE_DELTA_DEV static inline
static inline void delta_load16(const uint8_t* p, uint32_t cnt, uint32_t* w) {
  CHECK(((uintptr_t)p & 15u) == 0 && cnt >= 1 && cnt <= 16);
  w[0] = w[1] = w[2] = w[3] = 0;
  memcpy(w, p, cnt);  // the device reads 16 bytes only when cnt == 16
}
static inline void delta_store16(uint8_t* p, const uint32_t* w) {
  CHECK(((uintptr_t)p & 15u) == 0);
  memcpy(p, w, 16);
}
#include "../kyverno_amd/csrc/delta.inl"

template <class T>
static T* exact(size_t n) {  // exactly n elements, 16-byte aligned like a device allocation
  const size_t bytes = n * sizeof(T);
  T* p = static_cast<T*>(malloc(bytes ? bytes : 1));
  CHECK(p && ((uintptr_t)p & 15u) == 0);
  return p;
}

int main(int argc, char** argv) {
  if (argc != 3) return fprintf(stderr, "usage: delta_check <case> <flags-out>\n"), 2;
  FILE* f = fopen(argv[1], "rb");
  CHECK(f);
  uint64_t n;
  uint32_t hdr[4];
  CHECK(fread(&n, 8, 1, f) == 1 && fread(hdr, 4, 4, f) == 4);
  const uint32_t Ro = hdr[0], Rn = hdr[1], grid = hdr[2];
  CHECK(grid >= 1 && Ro <= kDeltaMaxRules && Rn <= kDeltaMaxRules);
  std::vector<int32_t> old_of(Rn);
  std::vector<uint8_t> always(Rn);
  uint8_t* vold = exact<uint8_t>(n * Ro);
  uint8_t* vnew = exact<uint8_t>(n * Rn);
  uint8_t* flags = exact<uint8_t>(n);
  CHECK(fread(old_of.data(), 4, Rn, f) == Rn && fread(always.data(), 1, Rn, f) == Rn);
  CHECK(fread(vold, 1, n * Ro, f) == n * Ro && fread(vnew, 1, n * Rn, f) == n * Rn);
  fclose(f);
  memset(flags, 0xEE, n);

  // the tables as kpe_api.cpp builds them
  std::vector<uint32_t> tab(Rn);
  std::vector<uint8_t> unm(Ro, 1);
  for (uint32_t r = 0; r < Rn; ++r) {
    CHECK(old_of[r] >= -1 && (old_of[r] < 0 || ((uint32_t)old_of[r] < Ro && unm[old_of[r]])));
    if (old_of[r] >= 0) unm[old_of[r]] = 0;
    tab[r] = (old_of[r] < 0 ? kDeltaNone : (uint32_t)old_of[r]) | ((uint32_t)always[r] << 16);
  }
  bool any_unm = false;
  for (uint8_t u : unm) any_unm |= u != 0;

  const uint32_t rpg = delta_rows_per_group(Rn, Ro);
  const DeltaLds L = delta_lds(Rn, Ro, rpg);
  CHECK(L.total <= 64u * 1024u && L.flag_off % 16 == 0 && L.tab_off % 16 == 0 && L.unm_off % 16 == 0);
  const uint64_t ngroups = n ? (n + rpg - 1) / rpg : 0;
  for (uint32_t b = 0; b < grid && b < ngroups; ++b) {
    // each carve its own exact allocation: an offset past a carve is a heap overflow
    uint8_t* s_old = exact<uint8_t>(L.old_bytes);
    uint32_t* s_flag = exact<uint32_t>(rpg);
    uint32_t* s_tab = exact<uint32_t>(Rn);
    uint8_t* s_unm = exact<uint8_t>(Ro);
    memset(s_old, 0xCC, L.old_bytes);
    if (Rn) memcpy(s_tab, tab.data(), Rn * 4);
    if (Ro) memcpy(s_unm, unm.data(), Ro);
    for (uint64_t g = b; g < ngroups; g += grid) {
      const DeltaGroup G = delta_group(g, n, Rn, Ro, rpg);
      CHECK(G.r0 + G.rn <= n && G.ob1 <= n * Ro && G.nb1 <= n * Rn && G.oskew < 16);
      CHECK(G.ob1 - G.ob0 <= kDeltaTile && G.nb1 - G.nb0 <= kDeltaTile);
      for (uint32_t t = 0; t < 256; ++t) delta_stage(G, t, vold, s_old, s_flag);
      for (uint32_t t = 0; t < 256; ++t) {
        delta_compare(G, t, vnew, Rn, Ro, s_tab, s_old, s_flag);
        if (any_unm) delta_sweep(G, t, Ro, s_unm, s_old, s_flag);
      }
      for (uint32_t i = 0; i < G.rn; ++i) CHECK(flags[G.r0 + i] == 0xEE);  // a row's byte is written once
      for (uint32_t t = 0; t < 256; ++t) delta_write(G, t, s_flag, flags);
    }
    free(s_old), free(s_flag), free(s_tab), free(s_unm);
  }

  // the rule, stated directly
  uint64_t bad = 0, changed = 0;
  for (uint64_t i = 0; i < n; ++i) {
    bool ch = false;
    for (uint32_t r = 0; r < Rn; ++r) {
      const uint8_t x = vnew[i * Rn + r], o = old_of[r] >= 0 ? vold[i * Ro + old_of[r]] : 0;
      ch |= x != o || (x < 8 && ((always[r] >> x) & 1));
    }
    for (uint32_t o = 0; o < Ro; ++o) ch |= unm[o] && vold[i * Ro + o] != 0;
    changed += ch;
    if (flags[i] != (ch ? 1 : 0) && bad++ < 5)
      fprintf(stderr, "delta_check: row %llu: flag %u, want %d\n", (unsigned long long)i, flags[i], (int)ch);
  }
  FILE* o = fopen(argv[2], "wb");
  CHECK(o && fwrite(flags, 1, n, o) == n);
  fclose(o);
  printf("n=%llu Ro=%u Rn=%u rpg=%u groups=%llu lds=%u changed=%llu bad=%llu\n", (unsigned long long)n, Ro, Rn, rpg,
         (unsigned long long)ngroups, L.total, (unsigned long long)changed, (unsigned long long)bad);
  free(vold), free(vnew), free(flags);
  return bad ? 1 : 0;
}
