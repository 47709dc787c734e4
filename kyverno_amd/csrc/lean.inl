// LEAN evaluation of kind-matched PSS programs (C2: restricted:latest and its autogen columns), the
// PSA dictionary codes it reads, and the general scan's per-pod PSA records. Same verdicts as
// kpe_scan_kernel<PSS, NARROW> (the reference path: pkg/engine/engine.go:87-101 validate ->
// validatePssHandler.Process, validate_pss.go:64-110, pkg/pss/evaluate.go:24-70).
//
// Every PSA check of the v0.29 library is "some container / list item of the pod is in state s"
// for fixed, policy-independent sets s (pss_fixed.hpp). A pod's checks are therefore decided from
// the OR of its containers' state bitmaps and of its list items' codes under those sets. The codes
// belong to the corpus's dictionaries (one byte per distinct capability set, sysctl name and
// annotation key / value: kpe_psa_codes_kernel, once per corpus, like the interned ids
// themselves); everything per pod is read and decided by every evaluation (kpe_lean6_kernel).
// Included by scan.hip (uses its anonymous-namespace helpers).

typedef __amdgpu_buffer_rsrc_t Rsrc;
__device__ __forceinline__ Rsrc make_rsrc(const void* p, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ uint32_t bload1(Rsrc r, uint32_t off) { return __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0); }
__device__ __forceinline__ uint2 bload2(Rsrc r, uint32_t off) {
  auto v = __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0);
  return make_uint2(v[0], v[1]);
}
struct L6Rec {  // what the LEAN evaluation reads of a pod record: pod word, r_gvk, packed list counts
  uint32_t x, y, z;
};
__device__ __forceinline__ L6Rec bload3(Rsrc r, uint32_t off) {
  auto v = __builtin_amdgcn_raw_buffer_load_b96(r, off, 0, 0);
  return L6Rec{v[0], v[1], v[2]};
}
__device__ __forceinline__ uint4 bload4(Rsrc r, uint32_t off) {
  auto v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
  return make_uint4(v[0], v[1], v[2], v[3]);
}

// The kernel arguments, read from the kernarg segment through a laundered pointer (one hop less
// than a device copy before the first load).
__device__ __forceinline__ const __attribute__((address_space(4))) void* kargs() {
  uint64_t v = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(v));
  return (const __attribute__((address_space(4))) void*)v;
}

#ifndef KPE_LEAN6_WAVES
#define KPE_LEAN6_WAVES 6
#endif
// The verdict-only form over the compact columns (CP) holds a container in one register, not two,
// and is compiled for eight resident blocks per CU: 64 VGPRs and, by the rule below, 80 SGPRs
// (gather form <4, true, false, false, true>: 60 VGPRs, no scratch, nine scalars kept in lanes;
// scatter form <..., true>: 50 VGPRs, 77 SGPRs, none). The gather form with the seccomp annotations
// spills 13 VGPRs to scratch at eight and stays at seven; so does the scatter form with them
// (58 VGPRs, 80 SGPRs), which shares the setting and measured no faster at eight.
#ifndef KPE_LEAN6C_WAVES
#define KPE_LEAN6C_WAVES 8
#endif
#ifndef KPE_LEAN6C_SANN_WAVES
#define KPE_LEAN6C_SANN_WAVES 7
#endif
constexpr int l6_waves(bool sann, bool cp) { return !cp ? KPE_LEAN6_WAVES : sann ? KPE_LEAN6C_SANN_WAVES : KPE_LEAN6C_WAVES; }
// Scalar registers of the kernel: a CU holds seven 256-thread blocks up to 96 of them and six
// above (800 per SIMD in blocks of 16, 16 more per wave), and the compiler takes all it may.
// The cap holds for every instantiation: the C2 one (<4, true, false, false>) fits in 94 without
// a spill; <4, true, true, false> (seccomp annotations, verdicts only) spills two scalars into
// lanes under it, the others none.
#ifndef KPE_LEAN6_SGPRS
#define KPE_LEAN6_SGPRS 96
#endif
constexpr uint32_t kLB = 256;
// XCD-aware block order: the dispatcher deals workgroups round-robin to the 8 XCDs (block b on
// XCD b % 8), so block b takes the (b / 8)-th block of XCD b % 8's contiguous share of the tiles:
// neighbouring tiles (whose list items share cache lines) stay on one XCD's L2.
__device__ __forceinline__ uint32_t xcd_block(uint32_t b, uint32_t nb) {
  const uint32_t q = nb >> 3, r = nb & 7u, x = b & 7u;
  return x * q + min(x, r) + (b >> 3);
}

// ---- PSA dictionary codes (once per corpus) -----------------------------------------------------
// Four bytes of s from p on (any alignment): two aligned dword loads and a shift. Dictionary
// buffers carry 128 bytes of slack past their end (kpe_api.cpp upload).
__device__ __forceinline__ uint32_t ld4u(const uint8_t* p) {
  const uintptr_t a = (uintptr_t)p;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
  const uint64_t v = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
  return (uint32_t)(v >> ((a & 3u) * 8u));
}
// Set-hit word of string s (n bytes): bit k = s matches a glob of fixed set k. Exact entries are
// bucketed by length, so a string is compared only with the literals of its own length, then with
// the few prefix entries; literals are compared four bytes per step from the LDS-staged table
// (layout in kernels_abi.h).
__device__ __forceinline__ uint32_t psa_sets(const uint32_t* fx, const uint8_t* s, uint32_t n) {
  auto eq = [&](uint32_t e, uint32_t len) -> bool {
    const uint32_t lit = fx[KPE_PSF_ENT0 + 2u * e + 1u];
    for (uint32_t i = 0; i < len; i += 4u) {
      const uint32_t m = len - i >= 4u ? ~0u : (1u << (8u * (len - i))) - 1u;
      if ((ld4u(s + i) ^ fx[lit + (i >> 2)]) & m) return false;
    }
    return true;
  };
  uint32_t hit = 0;
  if (n < KPE_PSF_MAXLEN) {
    const uint32_t rg = fx[2u + n];
    for (uint32_t e = rg & 0xFFFFu; e < (rg >> 16); ++e)
      if (eq(e, n)) hit |= 1u << (fx[KPE_PSF_ENT0 + 2u * e] & 0x7Fu);
  }
  const uint32_t E = fx[0], X = fx[1];
  for (uint32_t e = E; e < E + X; ++e) {
    const uint32_t h = fx[KPE_PSF_ENT0 + 2u * e], len = h >> 8;
    if (n >= len && eq(e, len)) hit |= 1u << (h & 0x7Fu);
  }
  return hit;
}
#define KPE_PSF_LDS_WORDS 1024u
// One launch: grid y = 0 capability sets (each block first codes the capability names, ids < 64),
// 1 sysctls, 2 annotation keys, 3 annotation values (PSD_*); one thread per entry.
__global__ void __launch_bounds__(256) kpe_psa_codes_kernel(PsaCodeArgs a) {
  __shared__ uint32_t fx[KPE_PSF_LDS_WORDS];
  __shared__ uint32_t s_m[6];
  const uint32_t t = threadIdx.x, y = blockIdx.y;
  for (uint32_t i = t; i < a.fixed_words; i += 256u) fx[i] = a.fixed[i];
  if (t < 6) s_m[t] = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * 256u + t;
  if (y == 0) {
    const uint32_t ncap = min(a.dict_n[PSD_CAP], 64u);
    if (t < ncap) {
      const uint32_t o0 = a.dict_off[PSD_CAP][t], o1 = a.dict_off[PSD_CAP][t + 1];
      const uint32_t h = psa_sets(fx, a.dict_bytes[PSD_CAP] + o0, o1 - o0);
      const uint32_t c = ((h >> PSF_CAPS_OK) & 1u) | (((h >> PSF_CAP_NBS) & 1u) << 1) | (((h >> PSF_CAP_ALL) & 1u) << 2);
      for (uint32_t k = 0; k < 3; ++k)
        if ((c >> k) & 1u) atomicOr(&s_m[2 * k + (t >> 5)], 1u << (t & 31u));
    }
    __syncthreads();
    if (i >= a.L.ncapsets) return;
    const uint64_t ok = s_m[0] | (uint64_t)s_m[1] << 32, nbs = s_m[2] | (uint64_t)s_m[3] << 32,
                   all = s_m[4] | (uint64_t)s_m[5] << 32;
    const uint4 cs = reinterpret_cast<const uint4*>(a.capsets)[i];
    const uint64_t ad = cs.x | (uint64_t)cs.y << 32, dr = cs.z | (uint64_t)cs.w << 32;
    a.codes[i] = (uint8_t)(((ad & ~ok) ? CS_BASE : 0u) | ((dr & all) ? 0u : CS_DROP) | ((ad & ~nbs) ? CS_ADD : 0u));
    return;
  }
  if (i >= a.dict_n[y]) return;
  const uint32_t o0 = a.dict_off[y][i], o1 = a.dict_off[y][i + 1];
  const uint32_t h = psa_sets(fx, a.dict_bytes[y] + o0, o1 - o0);
  uint32_t c, at;
  if (y == PSD_SYSCTL) {
    c = (((h >> PSF_SYSCTL0) & 1u) ^ 1u) | ((((h >> PSF_SYSCTL1) & 1u) ^ 1u) << 1) | ((((h >> PSF_SYSCTL2) & 1u) ^ 1u) << 2);
    at = a.L.o_sys;
  } else if (y == PSD_ANNK) {
    c = ((h >> PSF_APPARMOR_KEY) & 1u) | (((h >> PSF_SECCOMP_POD_KEY) & 1u) << 1);
    at = a.L.o_annk;
  } else {
    c = ((h >> PSF_APPARMOR_OK) & 1u) | (((h >> PSF_SECCOMP_ANN_OK) & 1u) << 1);
    at = a.L.o_annv;
  }
  a.codes[at + i] = (uint8_t)c;
}

// Code of one list item from the corpus's code bytes (`cb`: LDS or global), shared by the LEAN
// evaluation and the general scan's per-pod records. Branch-free: every code byte is read at an
// index clamped into the code table (the part's pad byte stands in for an id past the part) and
// the result selected afterwards, so no lane waits on a divergent load.
struct PsaCoder {
  const PsaCodes& L;
  // capability-set code of a container record (0 for an empty slot: no state bits)
  template <class CB>
  __device__ __forceinline__ uint32_t cap(const CB& cb, uint2 e) const {
    const uint32_t c = cb(CY_CAPSET(e.y)) & 7u;  // a real record's set id is < ncapsets; a zero slot reads set 0
    return e.x ? c : 0u;
  }
  // a container's seccomp annotation value (check_seccompProfile v1.0): 1 when set and not allowed
  template <class CB>
  __device__ __forceinline__ uint32_t sann(const CB& cb, uint32_t cs) const {
    const uint32_t v = cb(L.o_annv + min(cs, L.nannv));
    const uint32_t ok = cs < L.nannv ? (v >> 1) & 1u : 0u;
    return cs == KPE_NO_STR ? 0u : ok ^ 1u;
  }
  template <class CB>
  __device__ __forceinline__ uint32_t sys(const CB& cb, uint32_t id) const {
    const uint32_t v = cb(L.o_sys + min(id, L.nsysd));
    return id < L.nsysd ? v : 7u;
  }
  template <class CB>
  __device__ __forceinline__ uint32_t ann(const CB& cb, uint2 q) const {
    const uint32_t k = cb(L.o_annk + min(q.x, L.nannk)), v = cb(L.o_annv + min(q.y, L.nannv));
    const uint32_t ka = q.x < L.nannk ? k : 0u, va = q.y < L.nannv ? v : 0u;
    return ka & ~va & 3u;  // bit 0 AppArmor key with a disallowed profile, bit 1 pod seccomp key likewise
  }
};
__device__ __forceinline__ uint32_t vol_code(uint32_t v) {
  return ((v >> VS_HOSTPATH) & 1u) | ((v & kAllowedVolumes) ? 0u : 2u);
}

// ---- kpe_psum_kernel: the general scan's per-pod PSA records ----------------------------------
// One wave per 64-pod tile: list offsets from the tile header plus a wave scan of the pod
// records' packed counts, then each lane ORs its own pod's items. Out: {pod word, failing
// versioned checks, kind id << 16} per pod and, when asked (PsumArgs::summ), the summary {OR of
// container states, list codes} (schema.h PS_*). Launched by every evaluation of a podSecurity
// program that takes the general scan, right before it.
__global__ void __launch_bounds__(256) kpe_psum_kernel(PsumArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (tile >= a.ntiles) return;
  const uint32_t r = tile * 64u + lane;
  const bool live = r < (uint32_t)a.n;
  const uint32_t h = a.hdr[tile * 4u + (lane & 3u)];
  const uint4 rc = live ? reinterpret_cast<const uint4*>(a.rec)[r] : make_uint4(0u, 0u, 0u, 0u);
  const uint32_t z = rc.z;
  const uint32_t nc = PRC_CTR(z), nv = PRC_VOL(z), ns = PRC_SYS(z), na = PRC_PANN(z);
  const uint32_t c01 = nc | (nv << 16), c23 = ns | (na << 16);
  const uint32_t e01 = wave_incl_scan(c01) - c01, e23 = wave_incl_scan(c23) - c23;
  const uint32_t oc = hw(h, 0) + (e01 & 0xFFFFu), ov = hw(h, 1) + (e01 >> 16), os = hw(h, 2) + (e23 & 0xFFFFu),
                 oa = hw(h, 3) + (e23 >> 16);
  if (!live) return;
  const PsaCoder K{a.L};
  const uint8_t* codes = a.codes;
  auto cb = [&](uint32_t i) -> uint32_t { return codes[i]; };
  uint32_t xo = 0, co = 0, vc = 0, sc = 0, ac = 0, sa = 0;
  const uint2* crec = reinterpret_cast<const uint2*>(a.crec);
  for (uint32_t k = 0; k < nc; ++k) {
    const uint2 e = crec[oc + k];
    xo |= e.x;
    co |= K.cap(cb, e);
    sa |= K.sann(cb, a.c_sann[oc + k]);
  }
  for (uint32_t k = 0; k < nv; ++k) vc |= vol_code(a.vol_src[ov + k]);
  for (uint32_t k = 0; k < ns; ++k) sc |= K.sys(cb, a.sys_id[os + k]);
  const uint2* kv = reinterpret_cast<const uint2*>(a.pann_kv);
  for (uint32_t k = 0; k < na; ++k) ac |= K.ann(cb, kv[oa + k]);
  const uint32_t y = co | (vc << 3) | (sc << 5) | (ac << 8) | (sa << 10);
  uint32_t* o = a.psum + 3u * r;
  o[0] = rc.x;
  o[1] = cv_fails(rc.x, xo, PS_CAPS(y), PS_SECANN(y), PS_VOL(y) & 1u, PS_VOL(y) & 2u, PS_SYS(y), PS_ANN(y) & 1u,
                  PS_ANN(y) & 2u);
  o[2] = GVK_KIND(rc.y) << 16;
  if (a.summ) a.summ[2u * r] = xo, a.summ[2u * r + 1u] = y;
}

// ---- kpe_lean_pack_kernel: the compact columns of a corpus (once per corpus) --------------------
// Thread i writes words {x, y, z} of pod record i, its pod word (kernels_abi.h kpe_l6_pack_pod;
// a corpus of at most KPE_L6P_MAX_KINDS kinds) and the container word of container record i
// (kernels_abi.h kpe_l6_pack_ctr): a re-packing of the uploaded records, launched where the
// dictionary codes are (first podSecurity binding of the corpus, and a cold evaluation).
__global__ void __launch_bounds__(256) kpe_lean_pack_kernel(LeanPackArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < a.n) {
    const uint4 r = reinterpret_cast<const uint4*>(a.rec)[i];
    uint32_t* const o = a.rec12 + 3u * (size_t)i;
    o[0] = r.x, o[1] = r.y, o[2] = r.z;
    if (a.pw4) a.pw4[i] = kpe_l6_pack_pod(r.x, r.y);
  }
  if (a.cw4 && i < a.nctr) {
    const uint2 e = reinterpret_cast<const uint2*>(a.crec)[i];
    a.cw4[i] = kpe_l6_pack_ctr(e.x, e.y);
  }
}

// ---- kpe_lean_tag_kernel: the owner-tagged columns of a corpus (once per corpus) ---------------
// One wave per 64-pod tile, launched where kpe_lean_pack_kernel is: lane i finds pod i's list
// offsets as kpe_psum_kernel does (tile header plus a wave scan of the packed counts) and writes
// each of its items with owner i and, but for containers, the tile's quarter (kernels_abi.h
// kpe_l6_tag_*). An item outside its column (counts
// and headers that disagree) is not written; the allocation is zeroed before the launch.
__global__ void __launch_bounds__(256) kpe_lean_tag_kernel(LeanTagArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (tile >= a.ntiles) return;
  const uint32_t r = tile * 64u + lane;
  const uint32_t h = a.hdr[tile * 4u + (lane & 3u)];
  const uint32_t z = r < a.n ? a.rec[4u * (size_t)r + 2u] : 0u;
  const uint32_t nc = PRC_CTR(z), nv = PRC_VOL(z), ns = PRC_SYS(z), na = PRC_PANN(z);
  const uint32_t c01 = nc | (nv << 16), c23 = ns | (na << 16);
  const uint32_t e01 = wave_incl_scan(c01) - c01, e23 = wave_incl_scan(c23) - c23;
  const uint32_t oc = hw(h, 0) + (e01 & 0xFFFFu), ov = hw(h, 1) + (e01 >> 16), os = hw(h, 2) + (e23 & 0xFFFFu),
                 oa = hw(h, 3) + (e23 >> 16);
  const KpeL6TagLayout t = kpe_l6_tag_layout(a.nctr, a.nvol, a.nsys, a.npann);
  uint32_t* const tc = a.tag;
  uint32_t* const tv = a.tag + (t.o_vol >> 2);
  uint32_t* const ts = a.tag + (t.o_sys >> 2);
  uint32_t* const ta = a.tag + (t.o_ann >> 2);
  for (uint32_t k = oc; k < oc + nc && k < a.nctr; ++k) {
    const uint2 e = reinterpret_cast<const uint2*>(a.crec)[k];
    tc[k] = kpe_l6_tag_ctr(e.x, e.y, lane);
  }
  const uint32_t qt = tile & 3u;  // the tile's place in its group of four (the group form's word index)
  for (uint32_t k = ov; k < ov + nv && k < a.nvol; ++k) tv[k] = kpe_l6_tagq_vol(a.vol[k], lane, qt);
  for (uint32_t k = os; k < os + ns && k < a.nsys; ++k) ts[k] = kpe_l6_tagq_id(a.sys[k], lane, qt);
  for (uint32_t k = oa; k < oa + na && k < a.npann; ++k) {
    const uint2 q = reinterpret_cast<const uint2*>(a.pann)[k];
    ta[2u * (size_t)k] = kpe_l6_tagq_id(q.x, lane, qt), ta[2u * (size_t)k + 1u] = q.y;
  }
}

// ---- kpe_lean6_kernel: the LEAN evaluation, one or many shards per launch ----------------------
// A wave evaluates T consecutive 64-pod tiles of its block's shard (blocks find their shard by a
// scalar binary search over LeanBatchArgs::blk0). Two dependent memory steps per wave:
//   1. the T + 1 tile headers (one dword per lane) and the T tiles' pod records (16 B per lane;
//      CP: 12 B, one b96 load at a 12-byte stride);
//   2. every tile's list items, cooperatively and coalesced: lane i loads container i and 64 + i
//      of the tile (crec, or CP: cw4; and c_sann in the SANN instantiations: programs with a v1.0
//      seccomp check), volumes i and 64 + i, sysctl i and annotation i, from the tile's first item on.
// Then per tile: lane i codes its staged items (capability-set / sysctl / annotation codes from
// the corpus's code bytes, LDS-staged per block when they fit: LC) into the wave's LDS stage (a
// container as one word: kernels_abi.h KPE_L6_*), each pod ORs its own items from there (its
// offsets: one wave scan of the packed list counts), pods with more items than the clamped reads
// cover (or items past the stage) loop over the rest, the program's version classes are decided
// and the tile's rows are stored as dwords through LDS.
// How a class is decided is the CV parameter. CV: every versioned check (cv_fails), masked by the
// class's checks; needed for the check masks per cell (LeanShard::masks) and taken by programs of
// more than KPE_L6_CLS classes. Otherwise (verdicts only): one AND of the pod's evidence word
// with the class's evidence mask (LeanBatchArgs::cls_ev), the pod word's part of that word read
// from a constant table every block copies to LDS ahead of its kind table (kernels_abi.h
// kpe_l6_pod_table_word). Both give the same verdicts.
// CP (verdicts only): the pod records and containers come from the corpus's compact columns
// (kpe_lean_pack_kernel above) and the evidence word is decided in the packed numbering
// (kernels_abi.h KPE_L6C_*: the host passes the class masks and the pod table permuted by
// kpe_l6_pack_ev). The slow-path loops read cw4 too. The CV forms keep the wide records.
// SC (the default of CP): the scatter form over the owner-tagged columns, l6_scatter_tiles below;
// l6_gather_tiles, CP, is then the gather form, KPE_LEAN6_SHAPE bit 5.
typedef const __attribute__((address_space(4))) LeanBatchArgs CBArgs;
typedef const __attribute__((address_space(4))) LeanShard CShard;
// CT: a loaded container, the wide record (uint2) or the compact word (uint32_t)
template <bool SANN, class CT>
struct L6Items;
template <class CT>
struct L6Items<false, CT> {
  CT c0, c1;
  uint2 q0;
  uint32_t v0, v1, s0;
};
template <class CT>
struct L6Items<true, CT> : L6Items<false, CT> {
  uint32_t a0, a1;
};
// sysctl code (bit v: outside version v's set) at its evidence bits
__device__ __forceinline__ uint32_t l6_sys_evidence(uint32_t c) { return ((c & 3u) << 1) | ((c & 4u) << 2); }

// The body of every form but the scatter form (the kernel itself: end of this file)
template <int T, bool LC, bool SANN, bool CV, bool CP>
__device__ __forceinline__ void l6_gather_tiles() {
  typedef typename std::conditional<CP, uint32_t, uint2>::type CT;
  extern __shared__ __attribute__((aligned(16))) uint32_t dyn[];
  CBArgs& a = *(CBArgs*)kargs();
  const uint32_t t = threadIdx.x, lane = t & 63u;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(t >> 6);  // in a scalar: so are the wave's tile numbers
  const uint32_t gb = xcd_block(blockIdx.x, gridDim.x);
  uint32_t lo = 0, hi = a.nshards;  // blk0[lo] <= gb < blk0[hi]
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a.blk0[mid] <= gb) lo = mid;
    else hi = mid;
  }
  CShard& S = a.sh[lo];
  const uint32_t n = S.n, ntiles = (n + 63u) >> 6;
  const uint32_t tile0 = ((gb - a.blk0[lo]) * 4u + wv) * (uint32_t)T;
  const uint32_t need = a.need;
  // columns a program does not read get zero-length descriptors: their loads return 0 and move
  // no data (so do loads past a column's end)
  const Rsrc REC = CP ? make_rsrc(S.rec12, n * 12u) : make_rsrc(S.rec, n * 16u);
  const Rsrc HDR = make_rsrc(S.hdr, (ntiles + 1u) * 16u);
  const Rsrc CREC = CP ? make_rsrc(S.cw4, S.nctr * 4u) : make_rsrc(S.crec, S.nctr * 8u);
  // container k of the column (past its end: zeros, an empty slot)
  auto ld_ctr = [&](uint32_t k) -> CT {
    if constexpr (CP) return bload1(CREC, k * 4u);
    else return bload2(CREC, k * 8u);
  };
  const Rsrc SAN = make_rsrc(S.sann, SANN && (need & NEED_SANN) ? S.nctr * 4u : 0u);
  const Rsrc VOL = make_rsrc(S.vol, (need & NEED_VOL) ? S.nvol * 4u : 0u);
  const Rsrc SYS = make_rsrc(S.sys, (need & NEED_SYS) ? S.nsys * 4u : 0u);
  const Rsrc ANN = make_rsrc(S.pann, (need & NEED_PANN) ? S.npann * 8u : 0u);
  // ---- step 1: headers (lane k: word k of hdr[tile0 + k / 4]; past the sentinel: 0), records
  const uint32_t hall = bload1(HDR, (tile0 * 4u + min(lane, 4u * T + 3u)) * 4u);
  L6Rec rec[T];
#pragma unroll
  for (int j = 0; j < T; ++j) {  // past n: zeros
    const uint32_t r = (tile0 + j) * 64u + lane;
    if constexpr (CP) {
      rec[j] = bload3(REC, r * 12u);
    } else {
      const uint4 w = bload4(REC, r * 16u);
      rec[j] = L6Rec{w.x, w.y, w.z};
    }
  }
  // the block's kind table and (LC) code bytes, for the LDS below
  const uint32_t nk = S.nkinds;
  const uint32_t k0 = t < nk ? S.kt[t] : 0u;
  const uint32_t ncw = LC ? (S.L.bytes + 3u) >> 2 : 0u;
  const uint32_t* gcw = reinterpret_cast<const uint32_t*>(S.codes);
  const uint32_t cw0 = LC && t < ncw ? gcw[t] : 0u;
  // (verdicts only) the pod-evidence table, ahead of the kind table
  constexpr bool PT = !CV;
  uint32_t pt0 = 0, pt1 = 0;
  if constexpr (PT) {
    const uint32_t* const gpt = a.pod_tab;
    pt0 = gpt[t];
    pt1 = t < KPE_L6_PT_WORDS - kLB ? gpt[t + kLB] : 0u;
  }
  // ---- step 2: the list items of every tile
  L6Items<SANN, CT> it[T];
#pragma unroll
  for (int j = 0; j < T; ++j) {
    if (tile0 + j >= ntiles) break;
    const uint32_t C0 = hw(hall, 4u * j), V0 = hw(hall, 4u * j + 1u), S0 = hw(hall, 4u * j + 2u),
                   A0 = hw(hall, 4u * j + 3u);
    it[j].c0 = ld_ctr(C0 + lane);
    it[j].c1 = ld_ctr(C0 + 64u + lane);
    if constexpr (SANN) {
      it[j].a0 = bload1(SAN, (C0 + lane) * 4u);
      it[j].a1 = bload1(SAN, (C0 + 64u + lane) * 4u);
    }
    it[j].v0 = bload1(VOL, (V0 + lane) * 4u);
    it[j].v1 = bload1(VOL, (V0 + 64u + lane) * 4u);
    it[j].s0 = bload1(SYS, (S0 + lane) * 4u);
    it[j].q0 = bload2(ANN, (A0 + lane) * 8u);
  }
  if constexpr (PT) {
    dyn[t] = pt0;
    if (t < KPE_L6_PT_WORDS - kLB) dyn[t + kLB] = pt1;
  }
  uint32_t* const kt = dyn + KPE_L6_PT_WORDS;
  if (t < nk) kt[t] = k0;
#pragma unroll 1
  for (uint32_t i = t + kLB; i < nk; i += kLB) kt[i] = S.kt[i];
  uint32_t* const cl = kt + a.kt_words;
  if (LC) {
    if (t < ncw) cl[t] = cw0;
#pragma unroll 1
    for (uint32_t i = t + kLB; i < ncw; i += kLB) cl[i] = gcw[i];
  }
  uint32_t cls_cv = 0, cls_rm = 0;
  const uint32_t ncls = a.ncls;
  if (CV && lane < ncls) {
    const uint2 c = reinterpret_cast<const uint2*>(a.narrow_cls)[lane];
    cls_cv = c.x, cls_rm = c.y;
  }
  __syncthreads();
  const uint8_t* const lcodes = reinterpret_cast<const uint8_t*>(cl);
  const uint8_t* const gcodes = S.codes;
  auto cb = [&](uint32_t i) -> uint32_t { return LC ? (uint32_t)lcodes[i] : (uint32_t)gcodes[i]; };
  PsaCodes L;
  L.ncapsets = S.L.ncapsets, L.nsysd = S.L.nsysd, L.nannk = S.L.nannk, L.nannv = S.L.nannv;
  L.o_sys = S.L.o_sys, L.o_annk = S.L.o_annk, L.o_annv = S.L.o_annv, L.bytes = S.L.bytes;
  const PsaCoder K{L};
  const bool nvol = need & NEED_VOL, nsys = need & NEED_SYS, npann = need & NEED_PANN;
  // item counts above which a pod takes the slow path, as scalars: a list the program does not
  // read has a limit no byte count exceeds
  const uint32_t lim_v = nvol ? 4u : 255u, lim_s = nsys ? 2u : 255u, lim_a = npann ? 2u : 255u;
  // a container's stage word. Wide: a real record always has state bits, tested before they are
  // masked. Compact: a real word has KPE_L6C_REAL, which the state mask drops.
  auto ctr_word = [&](CT e, uint32_t cs) -> uint32_t {
    if constexpr (CP) {
      uint32_t w = (e & ((1u << KPE_L6C_STATES) - 1u)) | ((cb(kpe_l6_ctr_capset(e)) & 7u) << KPE_L6C_CAP_SH);
      if constexpr (SANN) w |= K.sann(cb, cs) << KPE_L6C_SANN_SH;
      return e ? w : 0u;
    } else {
      uint32_t w = (e.x & KPE_L6_CX_USED) | ((cb(CY_CAPSET(e.y)) & 7u) << KPE_L6_CAP_SH);
      if constexpr (SANN) w |= K.sann(cb, cs) << KPE_L6_SANN_SH;
      return e.x ? w : 0u;
    }
  };
  // sysctl codes are staged where the pod's word wants them: cv_fails's argument (and the packed
  // evidence word, which takes the code as it is), or in-place evidence bits
  auto sys_code = [&](uint32_t id) -> uint32_t { return CV || CP ? K.sys(cb, id) : l6_sys_evidence(K.sys(cb, id)); };
  // the version classes' evidence masks, in scalars for every tile
  uint32_t cev[KPE_L6_CLS], cev_nw[KPE_L6_CLS], crm[KPE_L6_CLS];
#pragma unroll
  for (uint32_t c = 0; c < KPE_L6_CLS; ++c) {
    cev[c] = CV ? 0u : a.cls_ev[c], cev_nw[c] = CV ? 0u : a.cls_ev_nw[c], crm[c] = CV ? 0u : a.cls_rm[c];
    asm volatile("" : "+s"(cev[c]), "+s"(cev_nw[c]), "+s"(crm[c]));
  }
  const uint32_t R = a.nrules, cv_union = a.cv_union, pss_rules = a.pss_rules;
  const uint32_t ep_rules = a.err_rules | a.pat_rules, pat_rules = a.pat_rules;
  uint8_t* const stg = reinterpret_cast<uint8_t*>(cl + a.code_words + wv * a.wave_words);
  uint32_t* const sc = reinterpret_cast<uint32_t*>(stg);
  uint8_t* const sbv = stg + 4u * KPE_L6_CTR;
  uint8_t* const sbs = sbv + KPE_L6_VOL;
  uint8_t* const sba = sbs + KPE_L6_SMALL;
  uint8_t* const sv = sba + KPE_L6_SMALL;  // the tile's verdict rows (64 x R bytes; 256 at least)
  // Rows of 2 to 4 bytes: a full tile's rows leave as one dword store per lane. Lane i's dword is
  // bytes 4 i .. 4 i + 3 of the tile's rows: they lie in the rows of pod rp_cell and the next one,
  // picked out of those two pods' cell words by the byte selector rp_sel.
  const bool rpack = R - 2u <= 2u;
  uint32_t rp_cell = 0, rp_sel = 0;
  if (rpack) {
    const uint32_t b = 4u * lane, p0 = R == 3u ? (b * 171u) >> 9 : b >> (R >> 1), r0 = b - p0 * R;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      const uint32_t g = r0 + k;
      rp_sel |= (g >= R ? 4u + g - R : g) << (8u * k);
    }
    rp_cell = min(p0, 63u);
  }
#pragma unroll
  for (int j = 0; j < T; ++j) {
    const uint32_t tile = tile0 + j;
    if (tile >= ntiles) break;
    const L6Items<SANN, CT>& d = it[j];
    const uint32_t C0 = hw(hall, 4u * j), V0 = hw(hall, 4u * j + 1u), S0 = hw(hall, 4u * j + 2u),
                   A0 = hw(hall, 4u * j + 3u);
    const uint32_t nct = hw(hall, 4u * j + 4u) - C0, nvt = hw(hall, 4u * j + 5u) - V0,
                   nst = hw(hall, 4u * j + 6u) - S0, nat = hw(hall, 4u * j + 7u) - A0;
    const uint32_t r = tile * 64u + lane;
    const bool live = r < n;
    // the pod's item offsets: exclusive wave scans of its packed counts
    const uint32_t z = rec[j].z;  // 0 for rows past n
    const uint32_t nc = PRC_CTR(z), nv = PRC_VOL(z), ns = PRC_SYS(z), na = PRC_PANN(z);
    uint32_t oc, ov, os, oa;
    if ((nct | nvt | nst | nat) < 256u) {  // one scan of the four packed byte counts (no carries)
      const uint32_t e = wave_incl_scan(z) - z;
      oc = e & 0xFFu, ov = (e >> 8) & 0xFFu, os = (e >> 16) & 0xFFu, oa = e >> 24;
    } else {
      const uint32_t c01 = nc | (nv << 16), c23 = ns | (na << 16);
      const uint32_t e01 = wave_incl_scan(c01) - c01, e23 = wave_incl_scan(c23) - c23;
      oc = e01 & 0xFFFFu, ov = e01 >> 16, os = e23 & 0xFFFFu, oa = e23 >> 16;
    }
    // stage the codes of the loaded slots (slots past the tile's items hold codes of the next
    // tile's items, or of zeros past a column's end, that no pod reads)
    __builtin_amdgcn_wave_barrier();  // the previous tile's stage reads are done
    if constexpr (SANN) {
      sc[lane] = ctr_word(d.c0, d.a0), sc[lane + 64u] = ctr_word(d.c1, d.a1);
    } else {
      sc[lane] = ctr_word(d.c0, 0u), sc[lane + 64u] = ctr_word(d.c1, 0u);
    }
    if (nvol) sbv[lane] = (uint8_t)vol_code(d.v0), sbv[lane + 64u] = (uint8_t)vol_code(d.v1);
    if (nsys && nst) sbs[lane] = (uint8_t)sys_code(d.s0);
    if (npann && nat) sba[lane] = (uint8_t)K.ann(cb, d.q0);
    __builtin_amdgcn_wave_barrier();
    // each pod ORs its first items with clamped reads (a repeated item does not change an OR)
    uint32_t cw, vcode = 0, scode = 0, acode = 0;
    {
      // containers: four words from the pod's first slot on (one address; a pod whose containers
      // reach past the stage is recomputed below, and the reads of slot 127 end in the volume bytes)
      const uint32_t* const p = sc + min(oc, KPE_L6_CTR - 1u);
      cw = kpe_l6_ctr_or(p[0], p[1], p[2], p[3], nc);
    }
    if (nvol) {
      const uint32_t last = min(ov + (nv ? nv - 1u : 0u), KPE_L6_VOL - 1u);
      const uint32_t x = (uint32_t)sbv[min(ov, last)] | sbv[min(ov + 1u, last)] | sbv[min(ov + 2u, last)] |
                         sbv[min(ov + 3u, last)];
      vcode = nv ? x : 0u;
    }
    if (nsys && nst) {
      const uint32_t last = min(os + (ns ? ns - 1u : 0u), KPE_L6_SMALL - 1u);
      const uint32_t x = (uint32_t)sbs[min(os, last)] | sbs[min(os + 1u, last)];
      scode = ns ? x : 0u;
    }
    if (npann && nat) {
      const uint32_t last = min(oa + (na ? na - 1u : 0u), KPE_L6_SMALL - 1u);
      const uint32_t x = (uint32_t)sba[min(oa, last)] | sba[min(oa + 1u, last)];
      acode = na ? x : 0u;
    }
    // pods with more items than that, or items past the stage: recomputed over all their items
    // (staged ones from LDS, the rest loaded)
    const bool tile_over = nct > KPE_L6_CTR || (nvol && nvt > KPE_L6_VOL) || (nsys && nst > KPE_L6_SMALL) ||
                           (npann && nat > KPE_L6_SMALL);
    const bool more_c = nc > 4u, more_v = nv > lim_v, more_s = ns > lim_s, more_a = na > lim_a;
    if (tile_over || __builtin_amdgcn_ballot_w64(more_c || more_v || more_s || more_a)) {
      if (more_c || oc + nc > KPE_L6_CTR) {
        cw = 0;
        for (uint32_t k = oc; k < oc + nc; ++k)
          cw |= k < KPE_L6_CTR ? sc[k]
                               : ctr_word(ld_ctr(C0 + k), SANN ? bload1(SAN, (C0 + k) * 4u) : 0u);
      }
      if (nvol && (more_v || ov + nv > KPE_L6_VOL)) {
        vcode = 0;
        for (uint32_t k = ov; k < ov + nv; ++k)
          vcode |= k < KPE_L6_VOL ? (uint32_t)sbv[k] : vol_code(bload1(VOL, (V0 + k) * 4u));
      }
      if (nsys && (more_s || os + ns > KPE_L6_SMALL)) {
        scode = 0;
        for (uint32_t k = os; k < os + ns; ++k)
          scode |= k < KPE_L6_SMALL ? (uint32_t)sbs[k] : sys_code(bload1(SYS, (S0 + k) * 4u));
      }
      if (npann && (more_a || oa + na > KPE_L6_SMALL)) {
        acode = 0;
        for (uint32_t k = oa; k < oa + na; ++k)
          acode |= k < KPE_L6_SMALL ? (uint32_t)sba[k] : K.ann(cb, bload2(ANN, (A0 + k) * 8u));
      }
    }
    // ---- the PSA checks, the rule match (kind table) and the verdict bytes ----
    const uint32_t pw = rec[j].x;
    uint32_t fails = 0, failr = 0;
    if constexpr (CV) {
      fails = cv_fails(pw, cw & KPE_L6_CX_USED, (cw >> KPE_L6_CAP_SH) & 7u, (cw >> KPE_L6_SANN_SH) & 1u, vcode & 1u,
                       vcode & 2u, scode, acode & 1u, acode & 2u) &
              cv_union;
      if (ncls <= 4u) {  // the usual few version classes: no loop
#pragma unroll
        for (uint32_t c = 0; c < 4u; ++c)
          failr |= (c < ncls && (fails & hw(cls_cv, c))) ? hw(cls_rm, c) : 0u;
      } else {
#pragma unroll 1
        for (uint32_t c = 0; c < ncls; ++c) failr |= (fails & hw(cls_cv, c)) ? hw(cls_rm, c) : 0u;
      }
    } else {
      const uint32_t lists = CP ? (vcode << KPE_L6C_VOL_SH) | (scode << KPE_L6C_SYS_SH) | (acode << KPE_L6C_ANN_SH)
                                : (vcode << KPE_L6_VOL_SH) | scode | (acode << KPE_L6_ANN_SH);
      // the pod word's part from the table: three LDS reads at constant offsets
      const uint32_t tw = kpe_l6_pod_lookup(dyn, pw);
      const uint32_t ev = CP ? kpe_l6c_pod_split(cw, tw, lists) : kpe_l6_pod_split(cw, tw, lists);
      const uint32_t ev_nw = ev & (uint32_t)((int32_t)tw >> 31);  // KPE_L6_PT_NW over the word
#pragma unroll
      for (uint32_t c = 0; c < KPE_L6_CLS; ++c) {
        if (c >= ncls) break;
        const uint32_t hit = (ev & cev[c]) | (ev_nw & cev_nw[c]);
        uint32_t m = hit ? ~0u : 0u;
        // Keeps the select on inline constants: as a select of crm[c] it costs a v_mov more per
        // class. Static VALU of <4, true, false, false> in the build this was measured in: 1,523
        // without the empty asm, 1,511 with it, nothing else changed. Harmless if a
        // later compiler no longer needs it; drop it if those two counts come out equal.
        asm("" : "+v"(m));
        failr |= m & crm[c];
      }
    }
    const uint32_t cls = (pw >> PR_CLASS_SH) & R_CLASS_MASK;
    const bool err = cls == R_CLASS_OTHER || (pw & PR_DECODE_ERR);
    const uint32_t kind = GVK_KIND(rec[j].y);
    const uint32_t matched = live && kind < nk ? kt[kind] : 0u;
    const uint32_t E = matched & ((err ? pss_rules : 0u) | ep_rules);
    const uint32_t F = (matched & pss_rules & failr & ~E) | (matched & pat_rules);  // F|E = PENDING
    const uint32_t P = matched & pss_rules & ~failr & ~E;
    const uint32_t nrows = min(64u, n - tile * 64u);
    bool stored = false;
    if (R <= 4u) {  // (C2: R = 3) the row as one word, byte ri = rule ri's cell: each 4-bit mask spread
      // over the bytes by a 24-bit multiply (bit i to bit 7 i + i) at its cell bit
      constexpr uint32_t kSpread = 0x204081u, kOnes = 0x01010101u;
      const uint32_t cellw = (__umul24(P, kSpread) & kOnes) | (__umul24(F, kSpread << 1) & (kOnes << 1)) |
                             (__umul24(E, kSpread << 2) & (kOnes << 2));
      if (rpack && nrows == 64u) {
        uint32_t* const sw = reinterpret_cast<uint32_t*>(sv);
        sw[lane] = cellw;
        __builtin_amdgcn_wave_barrier();
        const uint32_t w0 = sw[rp_cell], w1 = sw[min(rp_cell + 1u, 63u)];
        if (lane < 16u * R)
          reinterpret_cast<uint32_t*>(S.verdicts + (size_t)tile * (64u * R))[lane] = __builtin_amdgcn_perm(w1, w0, rp_sel);
        stored = true;
      } else {
#pragma unroll
        for (uint32_t ri = 0; ri < 4u; ++ri)
          if (ri < R) sv[lane * R + ri] = (uint8_t)(cellw >> (8u * ri));
      }
    } else {
#pragma unroll 1
      for (uint32_t ri = 0; ri < R; ++ri)
        sv[lane * R + ri] = (uint8_t)(((P >> ri) & 1u) | (((F >> ri) & 1u) << 1) | (((E >> ri) & 1u) << 2));
    }
    if constexpr (CV) {
      if (S.masks && live) {
        uint32_t* mrow = S.masks + (size_t)r * R;
        const uint32_t fm = F & pss_rules;
#pragma unroll 1
        for (uint32_t ri = 0; ri < R; ++ri) {
          uint32_t cv = 0;
          for (uint32_t c = 0; c < ncls; ++c) cv = ((hw(cls_rm, c) >> ri) & 1u) ? hw(cls_cv, c) : cv;
          mrow[ri] = ((fm >> ri) & 1u) ? (fails & cv) : 0u;
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
    if (!stored) store_rows(S.verdicts, sv, tile, R, 0, R, nrows, lane);
  }
}

// ---- kpe_lean6_kernel<T, true, SANN, false, true, true>: the scatter form of the compact
// verdict-only evaluation. The same launch shape, memory steps 1 and 2, class decision and row
// packing as the gather form <T, true, SANN, false, true>, over the corpus's owner-tagged columns
// (kernels_abi.h kpe_l6_tag_*; LeanShard::cw4 is the base of the one allocation that holds the
// four, read through one descriptor plus scalar byte offsets). No pod gathers its items: the lane
// that loaded an item codes it exactly as the gather form does, shifts the code to its place in
// the packed evidence word and ORs it into the word of the item's owner in LDS (one ds_or_b32
// per 64 slots; the packed word is an OR over disjoint bit ranges, and kpe_l6c_pod_split clears
// only container-state bits). A slot whose index is not below the tile's item count ORs 0: it
// holds an item of the next tile, whose owner names a pod of this one, or bytes of the next
// column or the slack. A tile with more items than the loaded slots takes further 64-slot
// batches in a wave-uniform loop. Then pod i reads word i.
// The shard search, the LDS tables, the class decision and the row packing are l6_gather_tiles's,
// restated here and to be kept in step with it: as shared __forceinline__ helpers they cost the
// C2 instantiations scalar spills at eight blocks per CU (gather 9 -> 20-25, scatter 0 -> 8-14;
// DESIGN.md section 9).
// NW (T >= 2: the launches of at least 32,768 tiles, the bandwidth-bound ones): the narrow form.
// The pod record is the corpus's one-word column pw4 (kernels_abi.h kpe_l6_pack_pod;
// LeanShard::rec12 is its base), one dword load per tile at a 4-byte stride, 256 contiguous bytes
// per wave; 8 bytes per pod less than words x and y at rec12's 12-byte stride, whose cache lines
// arrive whole. The T = 1 launches keep rec12.
template <int T, bool SANN, bool NW>
__device__ __forceinline__ void l6_scatter_tiles() {
  extern __shared__ __attribute__((aligned(16))) uint32_t dyn[];
  CBArgs& a = *(CBArgs*)kargs();
  const uint32_t t = threadIdx.x, lane = t & 63u;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const uint32_t gb = xcd_block(blockIdx.x, gridDim.x);
  uint32_t lo = 0, hi = a.nshards;  // blk0[lo] <= gb < blk0[hi]
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a.blk0[mid] <= gb) lo = mid;
    else hi = mid;
  }
  CShard& S = a.sh[lo];
  const uint32_t n = S.n, ntiles = (n + 63u) >> 6;
  const uint32_t tile0 = ((gb - a.blk0[lo]) * 4u + wv) * (uint32_t)T;
  const uint32_t need = a.need;
  const bool nvol = need & NEED_VOL, nsys = need & NEED_SYS, npann = need & NEED_PANN;
  const Rsrc REC = make_rsrc(S.rec12, NW ? n * 4u : n * 12u);
  const Rsrc HDR = make_rsrc(S.hdr, (ntiles + 1u) * 16u);
  // every load of the tagged columns lies inside the allocation (slack included): what a slot
  // past a tile's count holds is dropped by the count, not by the descriptor
  const KpeL6TagLayout lay = kpe_l6_tag_layout(S.nctr, S.nvol, S.nsys, S.npann);
  const Rsrc TAG = make_rsrc(S.cw4, (uint32_t)lay.bytes);
  const uint32_t o_vol = (uint32_t)lay.o_vol, o_sys = (uint32_t)lay.o_sys, o_ann = (uint32_t)lay.o_ann;
  const Rsrc SAN = make_rsrc(S.sann, SANN && (need & NEED_SANN) ? S.nctr * 4u : 0u);
  const uint32_t l4 = lane * 4u;
  auto ldt = [&](uint32_t voff, uint32_t soff) -> uint32_t { return __builtin_amdgcn_raw_buffer_load_b32(TAG, voff, soff, 0); };
  // ---- step 1: headers and records (words x and y, or NW: the pod word; the packed counts are
  // not read)
  const uint32_t hall = bload1(HDR, (tile0 * 4u + min(lane, 4u * T + 3u)) * 4u);
  typename std::conditional<NW, uint32_t, uint2>::type rec[T];
#pragma unroll
  for (int j = 0; j < T; ++j) {  // past n: zeros
    if constexpr (NW) rec[j] = bload1(REC, ((tile0 + j) * 64u + lane) * 4u);
    else rec[j] = bload2(REC, ((tile0 + j) * 64u + lane) * 12u);
  }
  const uint32_t nk = S.nkinds;
  const uint32_t k0 = t < nk ? S.kt[t] : 0u;
  const uint32_t ncw = (S.L.bytes + 3u) >> 2;
  const uint32_t* gcw = reinterpret_cast<const uint32_t*>(S.codes);
  const uint32_t cw0 = t < ncw ? gcw[t] : 0u;
  const uint32_t* const gpt = a.pod_tab;
  const uint32_t pt0 = gpt[t];
  const uint32_t pt1 = t < KPE_L6_PT_WORDS - kLB ? gpt[t + kLB] : 0u;
  // ---- step 2: the list items of every tile
  L6Items<SANN, uint32_t> it[T];
#pragma unroll
  for (int j = 0; j < T; ++j) {
    if (tile0 + j >= ntiles) break;
    const uint32_t C0 = hw(hall, 4u * j), V0 = hw(hall, 4u * j + 1u), S0 = hw(hall, 4u * j + 2u),
                   A0 = hw(hall, 4u * j + 3u);
    it[j].c0 = ldt(l4, C0 * 4u);
    it[j].c1 = ldt(l4 + 256u, C0 * 4u);
    if constexpr (SANN) {
      it[j].a0 = bload1(SAN, (C0 + lane) * 4u);
      it[j].a1 = bload1(SAN, (C0 + 64u + lane) * 4u);
    }
    it[j].v0 = it[j].v1 = it[j].s0 = 0u;
    it[j].q0 = make_uint2(0u, 0u);
    if (nvol) it[j].v0 = ldt(l4, o_vol + V0 * 4u), it[j].v1 = ldt(l4 + 256u, o_vol + V0 * 4u);
    if (nsys) it[j].s0 = ldt(l4, o_sys + S0 * 4u);
    if (npann) {
      const auto q = __builtin_amdgcn_raw_buffer_load_b64(TAG, lane * 8u, o_ann + A0 * 8u, 0);
      it[j].q0 = make_uint2(q[0], q[1]);
    }
  }
  dyn[t] = pt0;
  if (t < KPE_L6_PT_WORDS - kLB) dyn[t + kLB] = pt1;
  uint32_t* const kt = dyn + KPE_L6_PT_WORDS;
  if (t < nk) kt[t] = k0;
#pragma unroll 1
  for (uint32_t i = t + kLB; i < nk; i += kLB) kt[i] = S.kt[i];
  uint32_t* const cl = kt + a.kt_words;
  if (t < ncw) cl[t] = cw0;
#pragma unroll 1
  for (uint32_t i = t + kLB; i < ncw; i += kLB) cl[i] = gcw[i];
  const uint32_t ncls = a.ncls;
  __syncthreads();
  const uint8_t* const lcodes = reinterpret_cast<const uint8_t*>(cl);
  auto cb = [&](uint32_t i) -> uint32_t { return (uint32_t)lcodes[i]; };
  PsaCodes L;
  L.ncapsets = S.L.ncapsets, L.nsysd = S.L.nsysd, L.nannk = S.L.nannk, L.nannv = S.L.nannv;
  L.o_sys = S.L.o_sys, L.o_annk = S.L.o_annk, L.o_annv = S.L.o_annv, L.bytes = S.L.bytes;
  const PsaCoder K{L};
  uint32_t cev[KPE_L6_CLS], cev_nw[KPE_L6_CLS], crm[KPE_L6_CLS];
#pragma unroll
  for (uint32_t c = 0; c < KPE_L6_CLS; ++c) {
    cev[c] = a.cls_ev[c], cev_nw[c] = a.cls_ev_nw[c], crm[c] = a.cls_rm[c];
    asm volatile("" : "+s"(cev[c]), "+s"(cev_nw[c]), "+s"(crm[c]));
  }
  const uint32_t R = a.nrules, pss_rules = a.pss_rules;
  const uint32_t ep_rules = a.err_rules | a.pat_rules, pat_rules = a.pat_rules;
  // the wave's stage (laid out as the gather form's): the 64 evidence words first, the rows last
  uint8_t* const stg = reinterpret_cast<uint8_t*>(cl + a.code_words + wv * a.wave_words);
  uint32_t* const acc = reinterpret_cast<uint32_t*>(stg);
  uint8_t* const sv = stg + KPE_L6_STAGE_BYTES;  // the tile's verdict rows (64 x R bytes; 256 at least)
  const bool rpack = R - 2u <= 2u;  // rows of 2 to 4 bytes leave as one dword store per lane (as in the gather form)
  uint32_t rp_cell = 0, rp_sel = 0;
  if (rpack) {
    const uint32_t b = 4u * lane, p0 = R == 3u ? (b * 171u) >> 9 : b >> (R >> 1), r0 = b - p0 * R;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      const uint32_t g = r0 + k;
      rp_sel |= (g >= R ? 4u + g - R : g) << (8u * k);
    }
    rp_cell = min(p0, 63u);
  }
  // evidence `ev` of the item whose first word is w, into its owner's word; 0 from a slot that is
  // no item of the tile
  auto put = [&](uint32_t w, uint32_t ev, bool valid) {
    __hip_atomic_fetch_or(acc + kpe_l6_tag_owner(w), valid ? ev : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
  };
  auto ctr_ev = [&](uint32_t e, uint32_t cs) -> uint32_t {
    uint32_t w = (e & ((1u << KPE_L6C_STATES) - 1u)) | ((cb(kpe_l6_ctr_capset(e)) & 7u) << KPE_L6C_CAP_SH);
    if constexpr (SANN) w |= K.sann(cb, cs) << KPE_L6C_SANN_SH;
    return w;
  };
#pragma unroll
  for (int j = 0; j < T; ++j) {
    const uint32_t tile = tile0 + j;
    if (tile >= ntiles) break;
    const L6Items<SANN, uint32_t>& d = it[j];
    const uint32_t C0 = hw(hall, 4u * j), V0 = hw(hall, 4u * j + 1u), S0 = hw(hall, 4u * j + 2u),
                   A0 = hw(hall, 4u * j + 3u);
    const uint32_t nct = hw(hall, 4u * j + 4u) - C0, nvt = hw(hall, 4u * j + 5u) - V0,
                   nst = hw(hall, 4u * j + 6u) - S0, nat = hw(hall, 4u * j + 7u) - A0;
    const uint32_t r = tile * 64u + lane;
    const bool live = r < n;
    __builtin_amdgcn_wave_barrier();  // the previous tile's words are read
    acc[lane] = 0u;
    __builtin_amdgcn_wave_barrier();
    {  // containers: slots lane and 64 + lane, then batches of 64
      uint32_t a0 = 0, a1 = 0;
      if constexpr (SANN) a0 = d.a0, a1 = d.a1;
      put(d.c0, ctr_ev(d.c0, a0), lane < nct);
      put(d.c1, ctr_ev(d.c1, a1), lane + 64u < nct);
#pragma unroll 1
      for (uint32_t b = KPE_L6_CTR; b < nct; b += 64u) {
        const uint32_t e = ldt(l4, (C0 + b) * 4u);
        const uint32_t cs = SANN ? bload1(SAN, (C0 + b + lane) * 4u) : 0u;
        put(e, ctr_ev(e, cs), b + lane < nct);
      }
    }
    if (nvol && nvt) {
      // the volume decision; a volume of several sources: vol_code of its original mask
      auto vol_ev = [&](uint32_t w, uint32_t slot) -> uint32_t {
        uint32_t c = kpe_l6_vol_decide(w);
        const bool esc = slot < nvt && (w & KPE_L6T_VOL_ESC);
        if (__builtin_amdgcn_ballot_w64(esc)) {
          if (esc) c = vol_code(S.vol[V0 + slot]);
        }
        return c << KPE_L6C_VOL_SH;
      };
      put(d.v0, vol_ev(d.v0, lane), lane < nvt);
      put(d.v1, vol_ev(d.v1, lane + 64u), lane + 64u < nvt);
#pragma unroll 1
      for (uint32_t b = KPE_L6_VOL; b < nvt; b += 64u) {
        const uint32_t w = ldt(l4, o_vol + (V0 + b) * 4u);
        put(w, vol_ev(w, b + lane), b + lane < nvt);
      }
    }
    if (nsys && nst) {
      put(d.s0, K.sys(cb, kpe_l6_tag_get_id(d.s0)) << KPE_L6C_SYS_SH, lane < nst);
#pragma unroll 1
      for (uint32_t b = KPE_L6_SMALL; b < nst; b += 64u) {
        const uint32_t w = ldt(l4, o_sys + (S0 + b) * 4u);
        put(w, K.sys(cb, kpe_l6_tag_get_id(w)) << KPE_L6C_SYS_SH, b + lane < nst);
      }
    }
    if (npann && nat) {
      put(d.q0.x, K.ann(cb, make_uint2(kpe_l6_tag_get_id(d.q0.x), d.q0.y)) << KPE_L6C_ANN_SH, lane < nat);
#pragma unroll 1
      for (uint32_t b = KPE_L6_SMALL; b < nat; b += 64u) {
        const auto q = __builtin_amdgcn_raw_buffer_load_b64(TAG, lane * 8u, o_ann + (A0 + b) * 8u, 0);
        put(q[0], K.ann(cb, make_uint2(kpe_l6_tag_get_id(q[0]), q[1])) << KPE_L6C_ANN_SH, b + lane < nat);
      }
    }
    __builtin_amdgcn_wave_barrier();
    const uint32_t cw = acc[lane];
    // ---- the version classes, the rule match (kind table) and the verdict bytes: as the gather form
    uint32_t failr = 0, tw, cls, kind;
    bool derr;
    if constexpr (NW) {
      const uint32_t w = rec[j];
      tw = kpe_l6p_pod_lookup(dyn, w), cls = kpe_l6p_class(w), kind = kpe_l6p_kind(w);
      derr = w & KPE_L6P_DECODE_ERR;
    } else {
      const uint32_t pw = rec[j].x;
      tw = kpe_l6_pod_lookup(dyn, pw), cls = (pw >> PR_CLASS_SH) & R_CLASS_MASK, kind = GVK_KIND(rec[j].y);
      derr = pw & PR_DECODE_ERR;
    }
    const uint32_t ev = kpe_l6c_pod_split(cw, tw, 0u);
    const uint32_t ev_nw = ev & (uint32_t)((int32_t)tw >> 31);  // KPE_L6_PT_NW over the word
#pragma unroll
    for (uint32_t c = 0; c < KPE_L6_CLS; ++c) {
      if (c >= ncls) break;
      const uint32_t hit = (ev & cev[c]) | (ev_nw & cev_nw[c]);
      uint32_t m = hit ? ~0u : 0u;
      asm("" : "+v"(m));  // keeps the select on inline constants (see the gather form)
      failr |= m & crm[c];
    }
    const bool err = cls == R_CLASS_OTHER || derr;
    const uint32_t matched = live && kind < nk ? kt[kind] : 0u;
    const uint32_t E = matched & ((err ? pss_rules : 0u) | ep_rules);
    const uint32_t F = (matched & pss_rules & failr & ~E) | (matched & pat_rules);  // F|E = PENDING
    const uint32_t P = matched & pss_rules & ~failr & ~E;
    const uint32_t nrows = min(64u, n - tile * 64u);
    bool stored = false;
    if (R <= 4u) {  // the row as one word, byte ri = rule ri's cell
      constexpr uint32_t kSpread = 0x204081u, kOnes = 0x01010101u;
      const uint32_t cellw = (__umul24(P, kSpread) & kOnes) | (__umul24(F, kSpread << 1) & (kOnes << 1)) |
                             (__umul24(E, kSpread << 2) & (kOnes << 2));
      if (rpack && nrows == 64u) {
        uint32_t* const sw = reinterpret_cast<uint32_t*>(sv);
        sw[lane] = cellw;
        __builtin_amdgcn_wave_barrier();
        const uint32_t w0 = sw[rp_cell], w1 = sw[min(rp_cell + 1u, 63u)];
        if (lane < 16u * R)
          reinterpret_cast<uint32_t*>(S.verdicts + (size_t)tile * (64u * R))[lane] = __builtin_amdgcn_perm(w1, w0, rp_sel);
        stored = true;
      } else {
#pragma unroll
        for (uint32_t ri = 0; ri < 4u; ++ri)
          if (ri < R) sv[lane * R + ri] = (uint8_t)(cellw >> (8u * ri));
      }
    } else {
#pragma unroll 1
      for (uint32_t ri = 0; ri < R; ++ri)
        sv[lane * R + ri] = (uint8_t)(((P >> ri) & 1u) | (((F >> ri) & 1u) << 1) | (((E >> ri) & 1u) << 2));
    }
    __builtin_amdgcn_wave_barrier();
    if (!stored) store_rows(S.verdicts, sv, tile, R, 0, R, nrows, lane);
  }
}

// ---- kpe_lean6_kernel<4, true, SANN, false, true, true, true, true>: the group form of the
// narrow scatter form at four tiles per wave. A wave's four tiles are one 256-pod group, and the
// group's volumes, sysctls and annotations are contiguous in their columns: each column is
// streamed once from the group's first item (hdr[tile0]) to its last (hdr[min(tile0 + 4, ntiles)])
// in 64-slot sets, KPE_L6G_*_SETS of them loaded in step 2 and the rest in a wave-uniform loop,
// where the per-tile form loads, codes and ORs two (one) sets per tile however few items the tile
// has. The item words carry the pod's tile within the group (kernels_abi.h kpe_l6_tag_quarter),
// so byte 3 of a word is the pod's index in the wave's 256 interleaved evidence words: word
// 4 * pod + quarter, cleared once per wave. A slot is an item of the group when its index is
// below the group's count: a slot past it holds an item of the next wave's group, whose quarter
// and owner name a pod of this one, so this is the bound that matters; an item of a later tile of
// the group is that pod's own evidence whenever it is ORed. A set wholly past the count is skipped
// on a scalar branch. Containers (the word has no room for a quarter) stay per tile, into word
// 4 * owner + j. After a wave barrier lane i reads its four pods' words with one 16-byte read and
// the four tails run as in l6_scatter_tiles, restated here as there and to be kept in step.
// A volume with several sources (KPE_L6T_VOL_ESC) is looked for once over the loaded sets; only
// a group that may hold one takes the per-set ballots.
template <bool SANN>
__device__ __forceinline__ void l6_group_tiles() {
  constexpr int T = 4;
  extern __shared__ __attribute__((aligned(16))) uint32_t dyn[];
  CBArgs& a = *(CBArgs*)kargs();
  const uint32_t t = threadIdx.x, lane = t & 63u;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const uint32_t gb = xcd_block(blockIdx.x, gridDim.x);
  uint32_t lo = 0, hi = a.nshards;  // blk0[lo] <= gb < blk0[hi]
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a.blk0[mid] <= gb) lo = mid;
    else hi = mid;
  }
  CShard& S = a.sh[lo];
  const uint32_t n = S.n, ntiles = (n + 63u) >> 6;
  const uint32_t tile0 = ((gb - a.blk0[lo]) * 4u + wv) * (uint32_t)T;
  const uint32_t need = a.need;
  const bool nvol = need & NEED_VOL, nsys = need & NEED_SYS, npann = need & NEED_PANN;
  const Rsrc REC = make_rsrc(S.rec12, n * 4u);
  const Rsrc HDR = make_rsrc(S.hdr, (ntiles + 1u) * 16u);
  // the descriptor ends with the allocation (slack included): what a slot past the group's count
  // holds is dropped by the count
  const KpeL6TagLayout lay = kpe_l6_tag_layout(S.nctr, S.nvol, S.nsys, S.npann);
  const Rsrc TAG = make_rsrc(S.cw4, (uint32_t)lay.bytes);
  const uint32_t o_vol = (uint32_t)lay.o_vol, o_sys = (uint32_t)lay.o_sys, o_ann = (uint32_t)lay.o_ann;
  const Rsrc SAN = make_rsrc(S.sann, SANN && (need & NEED_SANN) ? S.nctr * 4u : 0u);
  const uint32_t l4 = lane * 4u;
  auto ldt = [&](uint32_t voff, uint32_t soff) -> uint32_t { return __builtin_amdgcn_raw_buffer_load_b32(TAG, voff, soff, 0); };
  // ---- step 1: headers and pod words. Lane k: word k & 3 of hdr[min(tile0 + k / 4, ntiles)]: a
  // tile past the shard's end reads the sentinel, so it has no items and the group ends where the
  // columns do
  const uint32_t hl = min(lane, 4u * T + 3u);
  const uint32_t hall = bload1(HDR, (min(tile0 + (hl >> 2), ntiles) * 4u + (hl & 3u)) * 4u);
  uint32_t rec[T];
#pragma unroll
  for (int j = 0; j < T; ++j) rec[j] = bload1(REC, ((tile0 + j) * 64u + lane) * 4u);  // past n: zeros
  const uint32_t nk = S.nkinds;
  const uint32_t k0 = t < nk ? S.kt[t] : 0u;
  const uint32_t ncw = (S.L.bytes + 3u) >> 2;
  const uint32_t* gcw = reinterpret_cast<const uint32_t*>(S.codes);
  const uint32_t cw0 = t < ncw ? gcw[t] : 0u;
  const uint32_t* const gpt = a.pod_tab;
  const uint32_t pt0 = gpt[t];
  const uint32_t pt1 = t < KPE_L6_PT_WORDS - kLB ? gpt[t + kLB] : 0u;
  // ---- step 2: every tile's containers, and the group's first sets of each list
  const uint32_t V0 = hw(hall, 1u), S0 = hw(hall, 2u), A0 = hw(hall, 3u);
  const uint32_t nvg = hw(hall, 4u * T + 1u) - V0, nsg = hw(hall, 4u * T + 2u) - S0, nag = hw(hall, 4u * T + 3u) - A0;
  uint32_t c0[T], c1[T], a0[T], a1[T];
#pragma unroll
  for (int j = 0; j < T; ++j) {
    if (tile0 + j >= ntiles) break;
    const uint32_t C0 = hw(hall, 4u * j);
    c0[j] = ldt(l4, C0 * 4u);
    c1[j] = ldt(l4 + 256u, C0 * 4u);
    if constexpr (SANN) {
      a0[j] = bload1(SAN, (C0 + lane) * 4u);
      a1[j] = bload1(SAN, (C0 + 64u + lane) * 4u);
    }
  }
  uint32_t vw[KPE_L6G_VOL_SETS], sw_[KPE_L6G_SYS_SETS];
  uint2 qw[KPE_L6G_ANN_SETS];
#pragma unroll
  for (uint32_t s = 0; s < KPE_L6G_VOL_SETS; ++s) vw[s] = nvol ? ldt(l4 + 256u * s, o_vol + V0 * 4u) : 0u;
#pragma unroll
  for (uint32_t s = 0; s < KPE_L6G_SYS_SETS; ++s) sw_[s] = nsys ? ldt(l4 + 256u * s, o_sys + S0 * 4u) : 0u;
#pragma unroll
  for (uint32_t s = 0; s < KPE_L6G_ANN_SETS; ++s) {
    qw[s] = make_uint2(0u, 0u);
    if (npann) {
      const auto q = __builtin_amdgcn_raw_buffer_load_b64(TAG, lane * 8u + 512u * s, o_ann + A0 * 8u, 0);
      qw[s] = make_uint2(q[0], q[1]);
    }
  }
  dyn[t] = pt0;
  if (t < KPE_L6_PT_WORDS - kLB) dyn[t + kLB] = pt1;
  uint32_t* const kt = dyn + KPE_L6_PT_WORDS;
  if (t < nk) kt[t] = k0;
#pragma unroll 1
  for (uint32_t i = t + kLB; i < nk; i += kLB) kt[i] = S.kt[i];
  uint32_t* const cl = kt + a.kt_words;
  if (t < ncw) cl[t] = cw0;
#pragma unroll 1
  for (uint32_t i = t + kLB; i < ncw; i += kLB) cl[i] = gcw[i];
  const uint32_t ncls = a.ncls;
  // the wave's 256 evidence words (16 bytes per lane: its four pods'), then the rows
  uint8_t* const stg = reinterpret_cast<uint8_t*>(cl + a.code_words + wv * a.wave_words);
  uint32_t* const acc = reinterpret_cast<uint32_t*>(stg);
  reinterpret_cast<uint4*>(stg)[lane] = make_uint4(0u, 0u, 0u, 0u);
  uint8_t* const sv = stg + KPE_L6G_ACC_BYTES;  // a tile's verdict rows (64 x R bytes; 256 at least)
  __syncthreads();
  const uint8_t* const lcodes = reinterpret_cast<const uint8_t*>(cl);
  auto cb = [&](uint32_t i) -> uint32_t { return (uint32_t)lcodes[i]; };
  PsaCodes L;
  L.ncapsets = S.L.ncapsets, L.nsysd = S.L.nsysd, L.nannk = S.L.nannk, L.nannv = S.L.nannv;
  L.o_sys = S.L.o_sys, L.o_annk = S.L.o_annk, L.o_annv = S.L.o_annv, L.bytes = S.L.bytes;
  const PsaCoder K{L};
  uint32_t cev[KPE_L6_CLS], cev_nw[KPE_L6_CLS], crm[KPE_L6_CLS];
#pragma unroll
  for (uint32_t c = 0; c < KPE_L6_CLS; ++c) {
    cev[c] = a.cls_ev[c], cev_nw[c] = a.cls_ev_nw[c], crm[c] = a.cls_rm[c];
    asm volatile("" : "+s"(cev[c]), "+s"(cev_nw[c]), "+s"(crm[c]));
  }
  const uint32_t R = a.nrules, pss_rules = a.pss_rules;
  const uint32_t ep_rules = a.err_rules | a.pat_rules, pat_rules = a.pat_rules;
  const bool rpack = R - 2u <= 2u;  // rows of 2 to 4 bytes leave as one dword store per lane (as in the gather form)
  uint32_t rp_cell = 0, rp_sel = 0;
  if (rpack) {
    const uint32_t b = 4u * lane, p0 = R == 3u ? (b * 171u) >> 9 : b >> (R >> 1), r0 = b - p0 * R;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      const uint32_t g = r0 + k;
      rp_sel |= (g >= R ? 4u + g - R : g) << (8u * k);
    }
    rp_cell = min(p0, 63u);
  }
  // evidence `ev` of the list item whose first word is w, into its pod's word (byte 3 of w: 4 *
  // owner + quarter); 0 from a slot that is no item of the group
  auto put = [&](uint32_t w, uint32_t ev, bool valid) {
    __hip_atomic_fetch_or(acc + kpe_l6_tag_slot(w), valid ? ev : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
  };
  auto ctr_ev = [&](uint32_t e, uint32_t cs) -> uint32_t {
    uint32_t w = (e & ((1u << KPE_L6C_STATES) - 1u)) | ((cb(kpe_l6_ctr_capset(e)) & 7u) << KPE_L6C_CAP_SH);
    if constexpr (SANN) w |= K.sann(cb, cs) << KPE_L6C_SANN_SH;
    return w;
  };
  // ---- containers, per tile: slots lane and 64 + lane, then batches of 64; tile j's into word 4 * owner + j
#pragma unroll
  for (int j = 0; j < T; ++j) {
    if (tile0 + j >= ntiles) break;
    const uint32_t C0 = hw(hall, 4u * j), nct = hw(hall, 4u * j + 4u) - C0;
    auto putc = [&](uint32_t w, uint32_t ev, bool valid) {
      __hip_atomic_fetch_or(acc + 4u * kpe_l6_tag_owner(w) + (uint32_t)j, valid ? ev : 0u, __ATOMIC_RELAXED,
                            __HIP_MEMORY_SCOPE_WAVEFRONT);
    };
    putc(c0[j], ctr_ev(c0[j], SANN ? a0[j] : 0u), lane < nct);
    putc(c1[j], ctr_ev(c1[j], SANN ? a1[j] : 0u), lane + 64u < nct);
#pragma unroll 1
    for (uint32_t b = KPE_L6_CTR; b < nct; b += 64u) {
      const uint32_t e = ldt(l4, (C0 + b) * 4u);
      const uint32_t cs = SANN ? bload1(SAN, (C0 + b + lane) * 4u) : 0u;
      putc(e, ctr_ev(e, cs), b + lane < nct);
    }
  }
  // ---- the group's lists
  if (nvol && nvg) {
    // the volume decision with the per-set look for a volume of several sources: vol_code of its
    // original mask
    auto vol_ev = [&](uint32_t w, uint32_t slot) -> uint32_t {
      uint32_t c = kpe_l6_vol_decide(w);
      const bool esc = slot < nvg && (w & KPE_L6T_VOL_ESC);
      if (__builtin_amdgcn_ballot_w64(esc)) {
        if (esc) c = vol_code(S.vol[V0 + slot]);
      }
      return c << KPE_L6C_VOL_SH;
    };
    // one look over the loaded sets (a slot past the count may hold the next group's: then the
    // per-set path runs for nothing)
    uint32_t any = 0;
#pragma unroll
    for (uint32_t s = 0; s < KPE_L6G_VOL_SETS; ++s) any |= vw[s];
    if (!__builtin_amdgcn_ballot_w64((any & KPE_L6T_VOL_ESC) != 0u)) {
#pragma unroll
      for (uint32_t s = 0; s < KPE_L6G_VOL_SETS; ++s)
        if (64u * s < nvg) put(vw[s], kpe_l6_vol_decide(vw[s]) << KPE_L6C_VOL_SH, 64u * s + lane < nvg);
    } else {
#pragma unroll
      for (uint32_t s = 0; s < KPE_L6G_VOL_SETS; ++s)
        if (64u * s < nvg) put(vw[s], vol_ev(vw[s], 64u * s + lane), 64u * s + lane < nvg);
    }
#pragma unroll 1
    for (uint32_t b = 64u * KPE_L6G_VOL_SETS; b < nvg; b += 64u) {
      const uint32_t w = ldt(l4, o_vol + (V0 + b) * 4u);
      put(w, vol_ev(w, b + lane), b + lane < nvg);
    }
  }
  if (nsys && nsg) {
#pragma unroll
    for (uint32_t s = 0; s < KPE_L6G_SYS_SETS; ++s)
      if (64u * s < nsg) put(sw_[s], K.sys(cb, kpe_l6_tag_get_id(sw_[s])) << KPE_L6C_SYS_SH, 64u * s + lane < nsg);
#pragma unroll 1
    for (uint32_t b = 64u * KPE_L6G_SYS_SETS; b < nsg; b += 64u) {
      const uint32_t w = ldt(l4, o_sys + (S0 + b) * 4u);
      put(w, K.sys(cb, kpe_l6_tag_get_id(w)) << KPE_L6C_SYS_SH, b + lane < nsg);
    }
  }
  if (npann && nag) {
#pragma unroll
    for (uint32_t s = 0; s < KPE_L6G_ANN_SETS; ++s)
      if (64u * s < nag)
        put(qw[s].x, K.ann(cb, make_uint2(kpe_l6_tag_get_id(qw[s].x), qw[s].y)) << KPE_L6C_ANN_SH, 64u * s + lane < nag);
#pragma unroll 1
    for (uint32_t b = 64u * KPE_L6G_ANN_SETS; b < nag; b += 64u) {
      const auto q = __builtin_amdgcn_raw_buffer_load_b64(TAG, lane * 8u, o_ann + (A0 + b) * 8u, 0);
      put(q[0], K.ann(cb, make_uint2(kpe_l6_tag_get_id(q[0]), q[1])) << KPE_L6C_ANN_SH, b + lane < nag);
    }
  }
  __builtin_amdgcn_wave_barrier();
  const uint4 cw4 = reinterpret_cast<const uint4*>(stg)[lane];
  const uint32_t cws[T] = {cw4.x, cw4.y, cw4.z, cw4.w};
#pragma unroll
  for (int j = 0; j < T; ++j) {
    const uint32_t tile = tile0 + j;
    if (tile >= ntiles) break;
    const uint32_t r = tile * 64u + lane;
    const bool live = r < n;
    const uint32_t cw = cws[j];
    // ---- the version classes, the rule match (kind table) and the verdict bytes: as the gather form
    uint32_t failr = 0;
    const uint32_t w = rec[j];
    const uint32_t tw = kpe_l6p_pod_lookup(dyn, w), cls = kpe_l6p_class(w), kind = kpe_l6p_kind(w);
    const bool derr = w & KPE_L6P_DECODE_ERR;
    const uint32_t ev = kpe_l6c_pod_split(cw, tw, 0u);
    const uint32_t ev_nw = ev & (uint32_t)((int32_t)tw >> 31);  // KPE_L6_PT_NW over the word
#pragma unroll
    for (uint32_t c = 0; c < KPE_L6_CLS; ++c) {
      if (c >= ncls) break;
      const uint32_t hit = (ev & cev[c]) | (ev_nw & cev_nw[c]);
      uint32_t m = hit ? ~0u : 0u;
      asm("" : "+v"(m));  // keeps the select on inline constants (see the gather form)
      failr |= m & crm[c];
    }
    const bool err = cls == R_CLASS_OTHER || derr;
    const uint32_t matched = live && kind < nk ? kt[kind] : 0u;
    const uint32_t E = matched & ((err ? pss_rules : 0u) | ep_rules);
    const uint32_t F = (matched & pss_rules & failr & ~E) | (matched & pat_rules);  // F|E = PENDING
    const uint32_t P = matched & pss_rules & ~failr & ~E;
    const uint32_t nrows = min(64u, n - tile * 64u);
    bool stored = false;
    if (R <= 4u) {  // the row as one word, byte ri = rule ri's cell
      constexpr uint32_t kSpread = 0x204081u, kOnes = 0x01010101u;
      const uint32_t cellw = (__umul24(P, kSpread) & kOnes) | (__umul24(F, kSpread << 1) & (kOnes << 1)) |
                             (__umul24(E, kSpread << 2) & (kOnes << 2));
      if (rpack && nrows == 64u) {
        uint32_t* const sw = reinterpret_cast<uint32_t*>(sv);
        sw[lane] = cellw;
        __builtin_amdgcn_wave_barrier();
        const uint32_t w0 = sw[rp_cell], w1 = sw[min(rp_cell + 1u, 63u)];
        if (lane < 16u * R)
          reinterpret_cast<uint32_t*>(S.verdicts + (size_t)tile * (64u * R))[lane] = __builtin_amdgcn_perm(w1, w0, rp_sel);
        stored = true;
      } else {
#pragma unroll
        for (uint32_t ri = 0; ri < 4u; ++ri)
          if (ri < R) sv[lane * R + ri] = (uint8_t)(cellw >> (8u * ri));
      }
    } else {
#pragma unroll 1
      for (uint32_t ri = 0; ri < R; ++ri)
        sv[lane * R + ri] = (uint8_t)(((P >> ri) & 1u) | (((F >> ri) & 1u) << 1) | (((E >> ri) & 1u) << 2));
    }
    __builtin_amdgcn_wave_barrier();
    if (!stored) store_rows(S.verdicts, sv, tile, R, 0, R, nrows, lane);
    __builtin_amdgcn_wave_barrier();  // the rows are read before the next tile's are written
  }
}

// SC: the scatter form of CP over the corpus's owner-tagged columns (l6_scatter_tiles); each
// instantiation holds the one body it runs.
// NW: its narrow form, over the pod word column (T >= 2). GR: the group form of that (T = 4).
template <int T, bool LC, bool SANN, bool CV, bool CP = false, bool SC = false, bool NW = false, bool GR = false>
__global__ void __launch_bounds__(kLB, l6_waves(SANN, CP)) __attribute__((amdgpu_num_sgpr(KPE_LEAN6_SGPRS)))
kpe_lean6_kernel(LeanBatchArgs) {
  static_assert(!(CP && CV), "the compact columns are read by the verdict-only form");
  static_assert(!SC || (CP && LC), "the scatter form is a compact form with the code bytes in LDS");
  static_assert(!NW || (SC && T >= 2), "the narrow form is a scatter form of two or four tiles per wave");
  static_assert(!GR || (NW && T == 4), "the group form is the narrow form at four tiles per wave");
  if constexpr (GR) l6_group_tiles<SANN>();
  else if constexpr (SC) l6_scatter_tiles<T, SANN, NW>();
  else l6_gather_tiles<T, LC, SANN, CV, CP>();
}
