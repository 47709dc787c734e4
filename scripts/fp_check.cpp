// Host run of the row fingerprint kernel's body (kyverno_amd/csrc/fp.inl, the text
// kpe_row_fp_kernel runs) under ASan / UBSan: the 256 lanes of each block in turn, phase by phase
// where the kernel has a barrier, over heap buffers of exactly N x R bytes (verdicts), N x R x 4
// bytes (mask words) and nrows x 8 bytes (output), row words of exactly one group and salt tables
// of exactly 2 R words, so a read past the matrix, a misaligned 16-byte access or a row word past
// the group is a sanitizer report or a failed check here, before the kernel ever runs on a device.
//
//   fp_check <case> <fingerprints-out>
// case: u64 n, u32 R, u32 grid, u32 flags (1: masks), u32 msg_codes, u64 row0, u64 nrows,
// u64 salts[R], u64 msg_salts[R], u8 v[n * R], and with flags & 1 u32 masks[n * R]. Writes the nrows
// fingerprints; exits non-zero when they differ from the rule of include/kpe.h stated directly
// (tests/test_fp_host.py compares them with kpe_row_fingerprints_host).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(x)                                                 \
  do {                                                           \
    if (!(x)) {                                                  \
      fprintf(stderr, "fp_check: %s (line %d)\n", #x, __LINE__); \
      exit(2);                                                   \
    }                                                            \
  } while (0)

#define KPE_FP_FN static inline
#define KPE_FP_DEV static inline
static inline void fp_load16(const uint8_t* p, uint32_t cnt, uint32_t* w) {
  CHECK(((uintptr_t)p & 15u) == 0 && cnt >= 1 && cnt <= 16);
  w[0] = w[1] = w[2] = w[3] = 0;
  memcpy(w, p, cnt);  // the device reads 16 bytes only when cnt == 16
}
static inline void fp_lds_add(uint64_t* p, uint64_t x) { *p += x; }
#include "../kyverno_amd/csrc/fp.inl"

template <class T>
static T* exact(size_t n) {  // exactly n elements, 16-byte aligned like a device allocation
  const size_t bytes = n * sizeof(T);
  T* p = static_cast<T*>(malloc(bytes ? bytes : 1));
  CHECK(p && ((uintptr_t)p & 15u) == 0);
  return p;
}

int main(int argc, char** argv) {
  if (argc != 3) return fprintf(stderr, "usage: fp_check <case> <fingerprints-out>\n"), 2;
  FILE* f = fopen(argv[1], "rb");
  CHECK(f);
  uint64_t n, win[2];
  uint32_t hdr[4];
  CHECK(fread(&n, 8, 1, f) == 1 && fread(hdr, 4, 4, f) == 4 && fread(win, 8, 2, f) == 2);
  const uint32_t R = hdr[0], grid = hdr[1], flags = hdr[2], msg_codes = hdr[3];
  const uint64_t row0 = win[0], nrows = win[1];
  const bool with_masks = (flags & 1u) != 0;
  CHECK(grid >= 1 && R >= 1 && R <= kFpMaxRules && msg_codes < 256 && row0 <= n && nrows <= n - row0);
  uint64_t* tbl = exact<uint64_t>(2 * (size_t)R);  // [salts][msg_salts], as kpe_api.cpp builds it
  uint8_t* v = exact<uint8_t>(n * R);
  uint32_t* masks = with_masks ? exact<uint32_t>(n * R) : nullptr;
  uint64_t* out = exact<uint64_t>(nrows);
  CHECK(fread(tbl, 8, 2 * (size_t)R, f) == 2 * (size_t)R && fread(v, 1, n * R, f) == n * R);
  if (with_masks) CHECK(fread(masks, 4, n * R, f) == n * R);
  fclose(f);
  memset(out, 0xEE, nrows * 8);
  const uint64_t untouched = 0xEEEEEEEEEEEEEEEEull;

  const uint32_t rpg = fp_rows_per_group(R);
  CHECK(rpg >= 1 && rpg <= kFpMaxRows && ((uint64_t)rpg * R <= kFpTile || rpg == 1));
  const uint64_t ngroups = nrows ? (nrows + rpg - 1) / rpg : 0;
  for (uint32_t b = 0; b < grid && b < ngroups; ++b) {
    for (uint64_t g = b; g < ngroups; g += grid) {
      const FpGroup G = fp_group(g, row0, nrows, R, rpg);
      CHECK(G.r0 + G.rn <= nrows && G.b1 <= n * R && G.b0 - G.a0 < 16 && G.b1 - G.b0 <= kFpTile);
      uint64_t* s_fp = exact<uint64_t>(G.rn);  // exactly the group's rows: a word past them is a heap overflow
      memset(s_fp, 0xCC, (size_t)G.rn * 8);
      for (uint32_t t = 0; t < 256; ++t) fp_clear(G, t, s_fp);
      for (uint32_t t = 0; t < 256; ++t) {
        if (with_masks) fp_accum<true>(G, t, v, masks, R, tbl, msg_codes, s_fp);
        else fp_accum<false>(G, t, v, nullptr, R, tbl, msg_codes, s_fp);
      }
      for (uint32_t i = 0; i < G.rn; ++i) CHECK(out[G.r0 + i] == untouched);  // a row's word is written once
      for (uint32_t t = 0; t < 256; ++t) fp_write(G, t, s_fp, out);
      free(s_fp);
    }
  }

  // the rule, stated directly
  uint64_t bad = 0, nonzero = 0;
  for (uint64_t i = 0; i < nrows; ++i) {
    uint64_t fp = 0;
    for (uint32_t r = 0; r < R; ++r) {
      const uint64_t c = (row0 + i) * R + r;
      const uint32_t x = v[c];
      if (!x) continue;
      const uint64_t s = x < 8 && ((msg_codes >> x) & 1) ? tbl[R + r] : tbl[r];
      const uint64_t m = with_masks && x == 2 ? masks[c] : 0;
      uint64_t z = s + 0x9E3779B97F4A7C15ull * ((uint64_t)x | (m << 8));
      z ^= z >> 30, z *= 0xBF58476D1CE4E5B9ull, z ^= z >> 27, z *= 0x94D049BB133111EBull, z ^= z >> 31;
      fp += z;
    }
    nonzero += fp != 0;
    if (out[i] != fp && bad++ < 5)
      fprintf(stderr, "fp_check: row %llu: %016llx, want %016llx\n", (unsigned long long)(row0 + i),
              (unsigned long long)out[i], (unsigned long long)fp);
  }
  FILE* o = fopen(argv[2], "wb");
  CHECK(o && fwrite(out, 8, nrows, o) == nrows);
  fclose(o);
  printf("n=%llu R=%u rows=[%llu,+%llu) rpg=%u groups=%llu masks=%d nonzero=%llu bad=%llu\n", (unsigned long long)n, R,
         (unsigned long long)row0, (unsigned long long)nrows, rpg, (unsigned long long)ngroups, (int)with_masks,
         (unsigned long long)nonzero, (unsigned long long)bad);
  free(tbl), free(v), free(masks), free(out);
  return bad ? 1 : 0;
}
