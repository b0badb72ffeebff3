// gm_match.hip — CDNA4 (gfx950) kernels for batch topic matching, and the
// match call that launches them (MatchCall: run_match / match_submit /
// match_wait, with the knob readers and launch_* that pick the instantiations).
// What consumes the finished rows is in gm_csr.hip, the device side of
// in-place updates in gm_update.hip, the scan in gm_scan.h.
//
// Hot path (replaces emqx_trie:match/1 + emqx_router:match_routes/1,
// apps/emqx/src/emqx_trie.erl:147-333, apps/emqx/src/emqx_router.erl:128-145):
//
//   k_match_fused  main pass: a block stages its 256 topics' text in
//                  LDS; each lane splits its topic into words, hashes them and
//                  resolves them in the word dictionary (verified
//                  byte-for-byte) into registers; then each wave walks its
//                  64-topic tile with the frontier of all 64 topics as ONE
//                  compacted LDS work list (ballot + mbcnt), one entry per
//                  lane per round: an exact probe and a '+' probe per entry,
//                  each one 16-B raw buffer load of a 32-B hot slot (edge probe
//                  and node record in one line).  Matches are staged per tile
//                  as one compact list (or as [slot][lane] columns).
//   k_match_lds    the listed pass: a lane-private walk with the frontier in
//                  LDS (capacity FC) over the topics whose frontier or row
//                  outgrew the main pass (count read on the device, so no
//                  host round trip between the passes).
//   tile sums / scan / k_assemble, k_assemble_c
//                  count -> scan -> write: builds the CSR (row_off u64, ids u32).
//   k_slow_walk / k_slow_emit / k_copy_slow
//                  device slow path: one workgroup per topic the listed pass
//                  could not hold, frontier in HBM (bounded by the node
//                  count), matches as a bitmap over filter ids, emitted in
//                  ascending id order.  No truncation, no CPU fallback.
//   k_d0_refresh   the walk's level-0 record (IndexView::d0_root), rewritten
//                  at build and after each in-place update (refresh_d0).
//
// k_match_fused is the only main pass.  The earlier forms of it as two kernels
// through word ids in HBM, and the two-stream tokenize/walk overlap, are gone;
// DESIGN.md section 4 keeps their measurements against the fused kernel.
//
// Everything here is integer/byte work bound by HBM/L2 latency and bandwidth;
// there is no MFMA.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "gm_internal.h"
#include "gm_scan.h"

namespace gm {

// ---------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------

// Stream accesses (topic text, staging, counts, the CSR)
// touch each byte once; NT = non-temporal, so they do not evict the index
// tables from L2 / the Infinity Cache (GM_NT knob, A/B).
template <bool NT, class T>
__device__ __forceinline__ T ld_s(const T* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}
template <bool NT, class T>
__device__ __forceinline__ void st_s(T* p, T v) {
  if constexpr (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// Diagnostic build only (-DGM_ISSUE_PAD=N, the Makefile's diag target): N
// v_nop and N s_nop 0 per walk round and per tokenized word of the fused
// kernel.  The kernel time against N is the cost of an issued instruction
// (profiles/issue/step0.txt); the product defines nothing.
#ifdef GM_ISSUE_PAD
#define GM_STR_(x) #x
#define GM_STR(x) GM_STR_(x)
#define GM_PAD() asm volatile(".rept " GM_STR(GM_ISSUE_PAD) "\n v_nop\n s_nop 0\n .endr")
#else
#define GM_PAD() \
  do {           \
  } while (0)
#endif

// Byte reader over a lane's topic with an 8-byte cache (aligned 8-B loads;
// topic buffers are padded, emqx_gpu_match.h).
struct ByteReader {
  const uint8_t* base;
  uint64_t cached_addr;
  uint64_t cached;
  __device__ __forceinline__ uint32_t get(uint64_t p) {
    const uint64_t a = p & ~7ull;
    if (a != cached_addr) {
      cached_addr = a;
      cached = *reinterpret_cast<const uint64_t*>(base + a);
    }
    return uint32_t(cached >> ((p & 7) * 8)) & 0xFFu;
  }
};

// One tokenized level word: hash, first 8 bytes, length, first byte.
struct WordTok {
  uint32_t h;  // dict_hash
  uint64_t head;
  uint64_t start;
  uint32_t len;
  uint32_t b0;
};

// Tokenize the word starting at `pos`; leaves `pos` on the '/' (or end).
__device__ __forceinline__ WordTok next_word(ByteReader& rd, uint64_t& pos, uint64_t end) {
  WordTok w;
  w.start = pos;
  w.head = 0;
  uint32_t h = DICT_HASH_SEED;
  uint64_t chunk = 0;
  uint32_t k = 0;
  while (pos < end) {
    const uint32_t b = rd.get(pos);
    if (b == '/') break;
    chunk |= uint64_t(b) << ((k & 7) * 8);
    ++k;
    ++pos;
    if ((k & 7) == 0) {
      if (k == 8) w.head = chunk;
      h = dict_hash_step(h, chunk);
      chunk = 0;
    }
  }
  if (k & 7) {
    if (k < 8) w.head = chunk;
    h = dict_hash_step(h, chunk);
  }
  w.h = dict_hash_final(h, k);
  w.len = k;
  w.b0 = uint32_t(w.head & 0xFF);
  return w;
}

__device__ __noinline__ bool tail_equal(const uint8_t* a, const uint8_t* b, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i)
    if (a[i] != b[i]) return false;
  return true;
}

__device__ __forceinline__ DictSlot dict_at(const IndexView& ix, uint64_t s) { return ix.dict[s]; }
// a depth-1 node's record as the level-0 round takes it: {hot id, sig, hf, end_filter}
constexpr uint4 D1_NONE = {NONE, 0u, HF_NONE, NONE};

// Resolve a word in the dictionary starting from the (prefetched) first slot.
// A hit is exact: length + first 8 bytes compared inline, the rest against
// the arena (only for words longer than 8 bytes).
__device__ __forceinline__ uint32_t dict_resolve(const IndexView& ix, const WordTok& w, DictSlot d,
                                                 const uint8_t* tb) {
  // the common outcomes decided from the prefetched slot with selects
  const bool empty0 = d.len == DICT_EMPTY_LEN;
  const bool hit0 = d.len == w.len && d.head == w.head && w.len <= 8;
  if (empty0 || hit0) return hit0 ? d.word : NONE;
  for (uint64_t s = dict_slot(w.h, ix.dict_mask);;) {
    if (d.len == DICT_EMPTY_LEN) return NONE;
    if (d.len == w.len && d.head == w.head &&
        (w.len <= 8 || tail_equal(ix.arena + d.word + 8, tb + w.start + 8, w.len - 8)))
      return d.word;
    s = (s + 1) & ix.dict_mask;
    d = dict_at(ix, s);
  }
}

__device__ __forceinline__ DictSlot dict_first(const IndexView& ix, const WordTok& w) {
  return dict_at(ix, dict_slot(w.h, ix.dict_mask));
}


__device__ __forceinline__ uint32_t edge_lookup(const IndexView& ix, uint32_t depth, uint32_t parent,
                                                uint32_t word) {
  const int d = edge_depth(depth);
  const EdgeSlot* tab = ix.edges + ix.etab_off[d];
  const uint64_t mask = ix.etab_mask[d];
  const uint64_t key = edge_key(parent, word);
  for (uint64_t s = edge_slot(key, mask);; s = (s + 1) & mask) {
    const EdgeSlot e = tab[s];
    if (e.key == key) return e.child;
    if (e.key == EDGE_EMPTY) return NONE;
  }
}

// Literal lookup of a wildcard topic as a filter string: emqx_router:
// lookup_routes(Topic) for a topic containing '+' / '#' words
// (emqx_router.erl:128-134 with match_trie = []).
__device__ uint32_t literal_lookup(const IndexView& ix, const uint8_t* tb, uint64_t pos, uint64_t end) {
  ByteReader rd{tb, ~0ull, 0};
  uint32_t node = 0;
  for (uint32_t depth = 0;; ++depth) {
    const WordTok w = next_word(rd, pos, end);
    const uint32_t wid = dict_resolve(ix, w, dict_first(ix, w), tb);
    if (wid == NONE) return NONE;
    const uint32_t c = edge_lookup(ix, depth, node, wid);
    if (c == NONE) return NONE;
    node = c & REF_MASK;
    if (pos >= end) break;
    ++pos;
  }
  return ix.nodes[node].end_filter;
}

__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v, uint32_t& total) {
  const int lane = threadIdx.x & 63;
  uint32_t x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  total = __shfl(x, 63, 64);
  return x - v;
}

// ---------------------------------------------------------------------------
// match kernels
// ---------------------------------------------------------------------------
// Staging layout per 64-topic tile: [slot k][lane], FAST_MC slots, so the k-th
// match of every lane is one coalesced 256-B row.
__device__ __forceinline__ uint64_t stage_index(uint64_t tile, uint32_t k, int lane) {
  return tile * (64ull * FAST_MC) + uint64_t(k) * 64u + uint32_t(lane);
}

// A hot slot as the kernel reads it: {key, sig, hf} in one dwordx4; the end
// filter (a second dword of the same line) only on the topic's last level.
struct HotRec {
  uint4 a;      // key lo, key hi, sig, hf (| HOT_PLUS)
  uint32_t ef;  // end_filter (NONE unless loaded)
};
// Hot-table loads go through a buffer resource (raw buffer loads, 32-bit byte
// offset from the table base): at C2 they took 4 % less time and ~10 % fewer
// L2 requests per topic than the same loads as flat global_load (A/B in
// scripts/mem_experiment.sh).  An index with a table of 2 GiB or more
// (IX_HOT_FLAT) uses flat loads.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t hot_rsrc(const HotSlot* tab) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<HotSlot*>(tab), (short)0, 0x7FFFFFFF, 0x00020000);
}
// One table (or one level's part of it) as k_match_fused reads it.  FLAT
// false: through a buffer resource of the table's real byte size,
// built from wave-uniform values only (kernel arguments, a readfirstlane'd
// level), with 32-bit per-lane byte offsets -- no 64-bit address arithmetic per
// lane, and the hardware range check drops the request of a lane that passes
// OOB (it reads zeros), so a load whose lanes do not all want it needs no
// exec-mask branch.  FLAT true (a table of 2 GiB or more, IX_HOT_FLAT): flat
// loads under the predicate.  The caller selects by the predicate, never by
// the loaded value.
constexpr uint32_t OOB = 0x80000000u;  // a byte offset no buffer table reaches
// Which buffer loads every lane issues (the range check drops the lanes that
// pass OOB) instead of sitting under an exec-mask branch: a bit mask per site
// group (-DGM_PRED_LOADS=m for an A/B build).  At C2 against none (8.03 ms):
// the dictionary -0.03 ms, the tails and level 0 -0.03 ms, the MPH / filter
// words +0.11 ms, the hot-slot probes +0.28 ms -- a probe
// most lanes skip costs its address cycles whether or not the range check
// drops it, a branch around it does not.
#ifndef GM_PRED_LOADS
#define GM_PRED_LOADS 9
#endif
constexpr bool PR_DICT = (GM_PRED_LOADS & 1) != 0;  // the tokenizer's first dictionary slots
constexpr bool PR_GATE = (GM_PRED_LOADS & 2) != 0;  // MPH bucket words, exact-edge filter words
constexpr bool PR_HOT = (GM_PRED_LOADS & 4) != 0;   // the hot-slot probes
constexpr bool PR_TAIL = (GM_PRED_LOADS & 8) != 0;  // chain tails, the level-0 probe and its end filter
template <bool FLAT>
struct TabRef {
  const uint8_t* p;
  __amdgpu_buffer_rsrc_t rs;
  __device__ __forceinline__ TabRef(const void* base, uint32_t bytes)
      : p(static_cast<const uint8_t*>(base)),
        rs(__builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, int(FLAT ? 0u : bytes), 0x00020000)) {}
  // element i of ESZ bytes, byte `sub` within it (32-bit byte offsets in the
  // buffer form, 64-bit addresses in the flat form)
  template <uint32_t ESZ>
  __device__ __forceinline__ const uint8_t* at(uint32_t i, uint32_t sub) const {
    return p + uint64_t(i) * ESZ + sub;
  }
  // pol (wave-uniform): hot_load's cache policies; only the A/B instantiations pass one
  template <uint32_t ESZ>
  __device__ __forceinline__ uint4 ld128(uint32_t i, uint32_t sub, bool pred, bool pr, uint32_t pol = 0) const {
    if constexpr (FLAT) {
      return pred ? *reinterpret_cast<const uint4*>(at<ESZ>(i, sub)) : make_uint4(0u, 0u, 0u, 0u);
    } else {
      if (!pr && !pred) return make_uint4(0u, 0u, 0u, 0u);
      const uint32_t o = pred ? i * ESZ + sub : OOB;
      const auto v = pol == 0 ? __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 0)
                     : pol == 1 ? __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 16)
                     : pol == 2 ? __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 17)
                     : pol == 3 ? __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 2)
                                : __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 18);
      return make_uint4(v[0], v[1], v[2], v[3]);
    }
  }
  template <uint32_t ESZ>
  __device__ __forceinline__ uint2 ld64(uint32_t i, bool pred, bool pr) const {
    if constexpr (FLAT) {
      return pred ? *reinterpret_cast<const uint2*>(at<ESZ>(i, 0)) : make_uint2(0u, 0u);
    } else {
      if (!pr && !pred) return make_uint2(0u, 0u);
      const auto v = __builtin_amdgcn_raw_buffer_load_b64(rs, pred ? i * ESZ : OOB, 0, 0);
      return make_uint2(v[0], v[1]);
    }
  }
  template <uint32_t ESZ>
  __device__ __forceinline__ uint32_t ld32(uint32_t i, uint32_t sub, bool pred, bool pr) const {
    if constexpr (FLAT) return pred ? *reinterpret_cast<const uint32_t*>(at<ESZ>(i, sub)) : 0u;
    if (!pr && !pred) return 0u;
    return __builtin_amdgcn_raw_buffer_load_b32(rs, pred ? i * ESZ + sub : OOB, 0, 0);
  }
};
// pol (wave-uniform; 0 = default): the cache policy of a probe of a table
// selected by IndexView::l1_bypass (A/B knobs GM_L1_BYPASS, GM_HOT_POLICY):
// 1 sc1 (no L1 fill), 2 sc0 sc1 (system scope), 3 nt, 4 sc1 nt
__device__ __forceinline__ HotRec hot_load(const HotSlot* tab, uint32_t s, bool with_end, bool flat, uint32_t pol = 0) {
  HotRec r;
  if (!flat) {
    const __amdgpu_buffer_rsrc_t rs = hot_rsrc(tab);
    const auto v = pol == 0 ? __builtin_amdgcn_raw_buffer_load_b128(rs, s * 32u, 0, 0)
                   : pol == 1 ? __builtin_amdgcn_raw_buffer_load_b128(rs, s * 32u, 0, 16)
                   : pol == 2 ? __builtin_amdgcn_raw_buffer_load_b128(rs, s * 32u, 0, 17)
                   : pol == 3 ? __builtin_amdgcn_raw_buffer_load_b128(rs, s * 32u, 0, 2)
                              : __builtin_amdgcn_raw_buffer_load_b128(rs, s * 32u, 0, 18);
    r.a = make_uint4(v[0], v[1], v[2], v[3]);
    r.ef = with_end ? __builtin_amdgcn_raw_buffer_load_b32(rs, s * 32u + 16u, 0, 0) : NONE;
  } else {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(tab + s);
    r.a = *reinterpret_cast<const uint4*>(p);
    r.ef = with_end ? p[4] : NONE;
  }
  return r;
}
__device__ __forceinline__ bool hot_is(const HotRec& r, uint64_t key) {
  return r.a.x == uint32_t(key) && r.a.y == uint32_t(key >> 32);
}
__device__ __forceinline__ bool hot_empty(const HotRec& r) { return r.a.x == 0xFFFFFFFFu && r.a.y == 0xFFFFFFFFu; }
// Linear probing from the home slot s of `key` (whose record r is already
// loaded); returns the slot index of `key` or NONE.  rh: the table is Robin
// Hood ordered (gm_index.cpp), so an absent key is known at the first slot
// whose key lies nearer its own home than this probe is from `key`'s.
__device__ __forceinline__ uint32_t hot_resolve(const HotSlot* tab, uint32_t cap, uint64_t key, uint32_t s,
                                                HotRec& r, bool with_end, bool flat, bool rh) {
  uint32_t dist = 0;
  while (!hot_is(r, key)) {
    if (hot_empty(r)) return NONE;
    if (rh) {
      const uint32_t h = uint32_t(hot_slot((uint64_t(r.a.y) << 32) | r.a.x, cap));
      if ((s >= h ? s - h : s + cap - h) < dist) return NONE;
    }
    s = s + 1 == cap ? 0 : s + 1;
    ++dist;
    r = hot_load(tab, s, with_end, flat);
  }
  return s;
}

// The home slot of `key` in hot table ht (wave-uniform): an MPH table first
// reads the key's bucket displacement (a small array that stays in L2), then
// its one perfect slot; an open-addressing table hashes straight to the home.
__device__ __forceinline__ uint32_t hot_home(const IndexView& ix, int ht, uint64_t key, uint64_t cap) {
  if (const uint32_t mc = ix.mph_cap[ht]) {
    const uint64_t w = ix.mph_word[ix.mph_off[ht] + mph_bucket(key, ix.mph_nb[ht])];
    return mph_slot(key, uint32_t(w) & 0xFFFFu, mc);
  }
  return uint32_t(hot_slot(key, cap));
}
// hot_resolve for either kind of table: an MPH table's key is at its perfect
// slot, or (once an in-place update put keys there) in the overflow region.
__device__ __forceinline__ uint32_t hot_resolve_x(const IndexView& ix, int ht, const HotSlot* tab, uint32_t cap,
                                                  uint64_t key, uint32_t s, HotRec& r, bool with_end, bool flat,
                                                  bool rh) {
  if (const uint32_t mc = ix.mph_cap[ht]) {
    if (hot_is(r, key)) return s;
    if (!((ix.mph_ovf >> ht) & 1u)) return NONE;
    for (s = mph_ovf_home(key, mc, cap);; s = s + 1 == cap ? mc : s + 1) {
      r = hot_load(tab, s, with_end, flat);
      if (hot_is(r, key)) return s;
      if (hot_empty(r)) return NONE;
    }
  }
  return hot_resolve(tab, cap, key, s, r, with_end, flat, rh);
}

// A compact staging list entry (IX_STAGE_SC1, A/B knob GM_STAGE_SC1: an sc1
// store, which leaves the line out of the XCD's L2 instead of keeping it there
// until eviction; the list is read by the next kernel anyway)
template <bool NT>
__device__ __forceinline__ void stage_st(uint32_t* base, uint32_t k, uint32_t v, bool sc1) {
  if (sc1) {
    __builtin_amdgcn_raw_buffer_store_b32(v, __builtin_amdgcn_make_buffer_rsrc(base, (short)0, 0x7FFFFFFF, 0x00020000),
                                          int(k * 4u), 0, 16);
  } else {
    st_s<NT>(base + k, v);
  }
}

// ---- the row, visit and probe steps of the lane-private walk (k_match_lds) ----
// Per-lane match staging: emit one filter id into the topic's row (slot m_n
// of the topic's lane column in its tile, srow = &stage[stage_index(tile, 0,
// lane)]; or of its listed row).
#define GM_EMIT(f)                                \
  do {                                            \
    if (m_n < MC) srow[m_n * sstr] = (f);         \
    ++m_n;                                        \
  } while (0)

// Visit a node reached at this level (its record r, hot id hs): emit
// 'match_#' for it; on the topic's last word also its own filter
// (lookup_topic/3: only wildcard filters in trie mode; the '$X' quirk of
// emqx_trie.erl:275-276 for single-word '$' topics); otherwise push it onto
// the next frontier (GM_PUSH, below).
#define GM_VISIT(hs, r)                                                                 \
  do {                                                                                  \
    if (((r).a.w & HF_MASK) != HF_NONE) GM_EMIT((r).a.w & HF_MASK);                     \
    if (last) {                                                                         \
      if ((r).ef != NONE && (EXACT || ((r).ef & END_WILD) || (dollar && level == 0)))   \
        GM_EMIT((r).ef & ID_MASK);                                                      \
      ++nfinal;                                                                         \
    } else {                                                                            \
      GM_PUSH((hs) | ((r).a.w & FR_PLUS), hot_sig((r).a.w, (r).a.z));                   \
    }                                                                                   \
  } while (0)

// A wildcard publish topic: [] from the trie (emqx_trie.erl:149-158); with
// match_routes semantics the literal route lookup_routes(Topic)
// (emqx_router.erl:128-134).
#define GM_WILD_ROW()                                        \
  do {                                                       \
    m_n = 0;                                                 \
    ovf = false;                                             \
    if (EXACT) {                                             \
      const uint32_t f = literal_lookup(ix, tb, start, end); \
      if (f != NONE) {                                       \
        srow[0] = f;                                         \
        m_n = 1;                                             \
      }                                                      \
    }                                                        \
  } while (0)

// The record of the '+' child held inline by slot `id` of its parent's table
// (gm_common.h): the slot's second 16 bytes, a line this walk read one level
// earlier when it visited the parent.
__device__ __forceinline__ HotRec plus_inline_load(const HotSlot* ptab, uint32_t id, bool flat) {
  uint4 q;
  if (!flat) {
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(hot_rsrc(ptab), (id & SLOT_MASK) * 32u + 16u, 0, 0);
    q = make_uint4(v[0], v[1], v[2], v[3]);
  } else {
    q = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint32_t*>(ptab + (id & SLOT_MASK)) + 4);
  }
  HotRec r;
  r.a = make_uint4(0u, 0u, q.y, q.z);
  r.ef = q.w;
  return r;
}
// Whether the '+' child of frontier entry `id` (a node at depth lvl) is inline.
__device__ __forceinline__ bool plus_is_inline(uint32_t lvl, uint32_t id) { return plus_inline(lvl, !(id & HOT_INLINE)); }

// Issue (load the home slot of) / take (resolve and visit) one probe of a
// frontier entry: the exact edge (word wid) or the '+' edge.  An inline '+'
// child is "issued" as the re-read of its parent's slot (sx = NONE).
#define GM_PROBE_ISSUE(c, e_id, plus, sx, rx)                                           \
  do {                                                                                  \
    if (c) {                                                                            \
      if ((plus) && plus_is_inline(lvl, (e_id))) {                                      \
        sx = NONE;                                                                      \
        rx = plus_inline_load(ptab, (e_id), hflat);                                        \
      } else {                                                                          \
        sx = hot_home(ix, ht, hot_key((e_id), (plus) ? ix.plus_word : wid, lvl), cap);    \
        rx = hot_load(tab, sx, last, hflat);                                            \
      }                                                                                 \
    }                                                                                   \
  } while (0)

#define GM_PROBE_TAKE(c, e_id, plus, sx, rx)                                                              \
  do {                                                                                                    \
    if (c) {                                                                                              \
      if ((plus) && sx == NONE) {                                                                         \
        GM_VISIT((e_id) | HOT_INLINE, rx);                                                                \
      } else {                                                                                            \
        const uint32_t hs_ = hot_resolve_x(ix, ht, tab, capu, hot_key((e_id), (plus) ? ix.plus_word : wid, lvl), sx, rx, last, hflat, hrh); \
        if (hs_ != NONE) GM_VISIT(hs_, rx);                                                               \
      }                                                                                                   \
    }                                                                                                     \
  } while (0)

// ---- k_match_lds: the listed pass -------------------------------------------
// Grid-stride over the topics list_in[0 .. *list_n) (the main pass's overflow
// queue; the count is read on the device), a topic per lane, its frontier
// entries double buffered in LDS, FC per lane.  Overflow here (frontier > FC or
// row > FAST_MC) is queued for k_slow_walk.
#define GM_PUSH(idv, sigv)                                                 \
  do {                                                                     \
    if (nn < FC) s_fr[nb][nn][threadIdx.x] = make_uint2((idv), (sigv));    \
    ++nn;                                                                  \
  } while (0)

// CMP (the main pass staged compactly): the listed rows go to their own
// buffer, row `item` of lstage (FAST_MC ids, stride 1), their length to
// lcnt[item] and cnt[t] = LIST_BIT | item; items past lcap go to the slow path.
// (The topic count and the wildcard counter, the main pass's, are not read
// here -- the main pass has counted a listed wildcard topic, one deeper than
// TOK_LMAX; both keep their places in the argument list.)
template <bool EXACT, int FC, bool CMP>
__global__ __launch_bounds__(256) void k_match_lds(const uint8_t* __restrict__ tb,
                                                   const uint64_t* __restrict__ toff, uint64_t /*n*/, IndexView ix,
                                                   uint32_t* __restrict__ cnt, uint32_t* __restrict__ stage,
                                                   const uint32_t* __restrict__ list_in,
                                                   const uint32_t* __restrict__ list_n,
                                                   uint32_t* __restrict__ ovf_list, uint32_t* __restrict__ ovf_n,
                                                   unsigned long long* __restrict__ probe_ctr,
                                                   unsigned long long* __restrict__ /*wild_ctr*/,
                                                   uint64_t* __restrict__ tsum, uint32_t* __restrict__ lstage,
                                                   uint32_t* __restrict__ lcnt, uint64_t lcap) {
  constexpr int MC = FAST_MC;
  constexpr uint32_t sstr = CMP ? 1u : 64u;
  // frontier entry: {hot id | FR_PLUS, exact-child signature}, double buffered
  __shared__ uint2 s_fr[2][FC][256];
  const int tid = threadIdx.x, lane = tid & 63;
  const uint64_t n_items = *list_n;
  uint32_t probes = 0;

  for (uint64_t item = uint64_t(blockIdx.x) * 256u + tid; item < n_items;
       item += uint64_t(gridDim.x) * 256u) {
    const uint64_t t = list_in[item];
    const uint64_t tile = t >> 6;
    if (CMP && item >= lcap) {  // no listed row left: the slow path
      cnt[t] = OVF_BIT;
      ovf_list[atomicAdd(ovf_n, 1u)] = uint32_t(t);
      continue;
    }
    uint32_t* const srow = CMP ? lstage + item * uint64_t(MC) : stage + stage_index(tile, 0, int(t & 63));
    uint32_t m_n = 0, tprobes = 0;
    bool ovf = false, wild = false;
    uint64_t pos = toff[t];
    const uint64_t end = toff[t + 1];
    const uint64_t start = pos;
    ByteReader rd{tb, ~0ull, 0};
    WordTok w = next_word(rd, pos, end);
    DictSlot d0 = dict_first(ix, w);
    const bool dollar = w.len > 0 && w.b0 == '$';  // emqx_trie.erl:271-278
    if (!dollar && ix.root_hash != NONE) GM_EMIT(ix.root_hash);
    int cur = 0;
    uint32_t cur_n = 1, nfinal = 0;
    s_fr[0][0][tid] = make_uint2((!dollar && (ix.root_flags & HOT_PLUS)) ? FR_PLUS : 0u, ix.root_sig);
    uint32_t level = 0;
    for (;;) {
      const bool last = pos >= end;
      if (w.len == 1 && (w.b0 == '+' || w.b0 == '#')) {
        wild = true;
        break;
      }
      const uint32_t wid = cur_n ? dict_resolve(ix, w, d0, tb) : NONE;
      const uint32_t wbit = sig_bit(wid);
      WordTok wn;
      DictSlot dn;
      if (!last) {
        ++pos;
        wn = next_word(rd, pos, end);
        dn = dict_first(ix, wn);
      }
      if (cur_n) {
        tprobes += 3 * cur_n;
        const int nb = cur ^ 1;
        uint32_t nn = 0;
        const uint32_t lvl = __builtin_amdgcn_readfirstlane(level);  // wave-uniform
        const int ht = hot_table(lvl + 1);
        const HotSlot* tab = ix.hot + ix.hot_off[ht];
        const HotSlot* ptab = ix.hot + ix.hot_off[hot_table(lvl)];  // the frontier nodes' own table
        const bool hflat = (ix.flags & IX_HOT_FLAT) != 0;
        const bool hrh = ((ix.rh_mask >> ht) & 1u) != 0;  // Robin Hood ordered table
        const uint64_t cap = ix.hot_cap[ht];
        const uint32_t capu = uint32_t(cap);
        for (uint32_t i = 0; i < cur_n; ++i) {
          const uint2 e = s_fr[cur][i][tid];
          const uint32_t id = e.x & ID_MASK;
          const bool dx = wid != NONE && (e.y & wbit);
          const bool dp = (e.x & FR_PLUS) != 0;
          uint32_t sx = 0, sp = 0;
          HotRec rx{}, rp{};
          GM_PROBE_ISSUE(dx, id, false, sx, rx);
          GM_PROBE_ISSUE(dp, id, true, sp, rp);
          GM_PROBE_TAKE(dx, id, false, sx, rx);
          GM_PROBE_TAKE(dp, id, true, sp, rp);
        }
        if (nn > FC) {
          ovf = true;
          break;
        }
        cur = nb;
        cur_n = nn;
      }
      if (last) break;
      w = wn;
      d0 = dn;
      ++level;
    }
    if (wild) {
      GM_WILD_ROW();
      tprobes = 0;  // a wildcard publish topic is not walked: P = 0, as the main passes count it
    } else if (!ovf) {
      tprobes += 2 * nfinal + 1;
      if (m_n > MC) ovf = true;
    }
    if (CMP) {
      cnt[t] = ovf ? OVF_BIT : (LIST_BIT | uint32_t(item));
      if (!ovf) lcnt[item] = m_n;
    } else {
      cnt[t] = ovf ? OVF_BIT : m_n;
    }
    if (ovf) ovf_list[atomicAdd(ovf_n, 1u)] = uint32_t(t);
    else atomicAdd(reinterpret_cast<unsigned long long*>(tsum + tile), (unsigned long long)m_n);
    probes += tprobes;
  }
  // the wave's probes (one atomic per wave; an idle listed grid adds nothing:
  // 2,048 same-address atomics cost ~20 us)
  uint32_t ptot;
  wave_excl_scan(probes, ptot);
  if (lane == 0 && ptot) atomicAdd(probe_ctr, (unsigned long long)ptot);
}
#undef GM_PUSH
#undef GM_PROBE_ISSUE
#undef GM_PROBE_TAKE
#undef GM_VISIT
#undef GM_WILD_ROW
#undef GM_EMIT

// ---- the tokenizer (k_match_fused's front end) ----------------------------------
// Per topic: a header = levels | TOK_DOLLAR | TOK_WILD | TOK_DEEP, and the word
// id of each level below TOK_LMAX (NONE for a word no filter uses), which the
// lane keeps in registers (WidsToRegs) for the walk that follows.
constexpr int TOK_LMAX = 8;
// levels scanned, and dictionary slots in flight, at a time (tokenize_grouped)
constexpr int TOK_GROUP = 3;
constexpr uint32_t TOK_DOLLAR = 1u << 8, TOK_WILD = 1u << 9, TOK_DEEP = 1u << 10;

// Word scan over LDS-staged text, 8 bytes per step (SWAR): the next '/' is the
// lowest zero byte of (word ^ 0x2F..2F) at or after the start (an exact
// per-byte test: the usual (y - 0x01..) & ~y trick borrows across bytes and
// can flag a byte just above an earlier '/'); a word's 8-byte
// chunks (from its own first byte, the last one zero padded -- the same
// chunking as the byte reader, so the same hash) are funnel shifts of two
// aligned LDS words.  Needs one staged word of slack past the text.
__device__ __forceinline__ uint64_t funnel8(const uint64_t* lds, uint64_t wi, uint32_t sh) {
  const uint64_t a = lds[wi];
  return sh ? (a >> sh) | (lds[wi + 1] << (64 - sh)) : a;
}

// The scan, in 32-bit offsets relative to the block's staged text (at most
// TOK_STAGE bytes): no 64-bit position arithmetic in the byte scan.
// `w.start` is relative too, so the word's tail is read from `tb + lo`.
__device__ __forceinline__ WordTok next_word_s(const uint64_t* lds, uint32_t& pos, uint32_t end) {
  constexpr uint64_t SL = 0x2F2F2F2F2F2F2F2Full, M7 = 0x7F7F7F7F7F7F7F7Full;
  // exact per-byte zero test (no borrow between bytes): bit 7 of a byte of
  // zbytes(y) is set iff that byte of y is 0
  auto zbytes = [](uint64_t y) { return ~(((y & M7) + M7) | y | M7); };
  WordTok w;
  w.start = pos;
  const uint32_t w0 = pos >> 3;
  const uint32_t sh = (pos & 7u) * 8u;
  // The two staged words that hold any word of up to 8 bytes, loaded
  // unconditionally: the common word is cut and hashed with selects, no
  // divergent loop (the kernels were issue bound on the exec-mask SALU work
  // of those loops as much as on VALU).  Index w0 + 1 stays inside s_txt
  // (staged text <= TOK_STAGE - 8 bytes, one word of slack).
  const uint64_t a0 = lds[w0], a1 = lds[w0 + 1];
  const uint64_t z0 = zbytes(a0 ^ SL) & (~0ull << sh);  // bytes before pos do not count
  const uint64_t z1 = zbytes(a1 ^ SL);
  uint32_t at = z0 ? w0 * 8u + (uint32_t(__builtin_ctzll(z0)) >> 3)
                   : (z1 ? w0 * 8u + 8u + (uint32_t(__builtin_ctzll(z1)) >> 3) : w0 * 8u + 16u);
  if (!z0 && !z1 && (w0 + 2u) * 8u < end) {  // a word reaching past the second staged word
    uint32_t wi = w0 + 2u;
    at = end;
    for (;;) {
      const uint64_t z = zbytes(lds[wi] ^ SL);
      if (z) {
        at = wi * 8u + (uint32_t(__builtin_ctzll(z)) >> 3);
        break;
      }
      if ((wi + 1u) * 8u >= end) break;
      ++wi;
    }
  }
  const uint32_t e = at < end ? at : end;
  const uint32_t len = e - pos;
  uint64_t c = sh ? (a0 >> sh) | (a1 << (64 - sh)) : a0;
  c &= len >= 8 ? ~0ull : (1ull << ((len & 7u) * 8u)) - 1;
  uint32_t h = len ? dict_hash_step(DICT_HASH_SEED, c) : DICT_HASH_SEED;
  for (uint32_t k = 8; k < len; k += 8) {  // words longer than 8 bytes
    uint64_t ck = funnel8(lds, w0 + (k >> 3), sh);
    if (len - k < 8) ck &= (1ull << ((len - k) * 8)) - 1;
    h = dict_hash_step(h, ck);
  }
  w.h = dict_hash_final(h, len);
  w.head = c;
  w.len = len;
  w.b0 = uint32_t(c & 0xFF);
  pos = e;
  return w;
}

// Where the word ids of one topic go: the lane's registers.  Called for levels
// 0, 1, 2, ... in order; the select chain keeps w[] out of scratch.  (The
// tokenizers take it by reference: by value the kernel's registers are
// allocated differently.)
struct WidsToRegs {
  uint32_t (&w)[TOK_LMAX];
  __device__ __forceinline__ void operator()(uint32_t lev, uint32_t v) {
#pragma unroll
    for (int q = 0; q < TOK_LMAX; ++q)
      if (lev == uint32_t(q)) w[q] = v;
  }
};

// Staged text, grouped: the words of TOK_GROUP levels are scanned first and
// their first dictionary slots loaded together, then resolved -- TOK_GROUP L2
// round trips in flight per lane instead of tokenize_topic's one-ahead prefetch
// (the tokenizer waits on the dictionary most of its time).  A word is kept as 4
// VGPRs (head, hash, start | len << 16; staged text is < 64 KiB) until it
// resolves.  Levels past TOK_LMAX are only counted and checked for wildcards.
// DBUF (the buffer form): the words' first dictionary slots are raw buffer
// loads (32-bit offsets from ix.dict) that every lane issues; a lane without
// a word at that level passes an out-of-range offset.
template <bool DBUF>
__device__ __forceinline__ uint32_t tokenize_grouped(const uint64_t* lds, uint32_t pos, uint32_t end,
                                                     const IndexView& ix, const uint8_t* tb_lo, WidsToRegs&& sink) {
  constexpr int G = TOK_GROUP;
  uint32_t lev = 0, fl = 0;
  bool more = true, wild = false;
  const TabRef<!DBUF> DT(ix.dict, uint32_t(ix.dict_mask + 1) * uint32_t(sizeof(DictSlot)));
  while (more && lev < uint32_t(TOK_LMAX)) {
    uint64_t hd[G];
    uint32_t hh[G], sl[G];
    DictSlot d[G];
    bool have[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      have[g] = more && lev + g < uint32_t(TOK_LMAX);
      if constexpr (DBUF) hh[g] = 0u;
      if (have[g]) {
        GM_PAD();
        const WordTok w = next_word_s(lds, pos, end);
        if (g == 0 && lev == 0 && w.len > 0 && w.b0 == '$') fl |= TOK_DOLLAR;  // emqx_trie.erl:271-278
        if (w.len == 1 && (w.b0 == '+' || w.b0 == '#')) {  // emqx_topic:wildcard/1
          wild = true;
          have[g] = more = false;
        } else {
          hd[g] = w.head;
          hh[g] = w.h;
          sl[g] = uint32_t(w.start) | (w.len << 16);
          if constexpr (!DBUF) d[g] = dict_first(ix, w);
          more = pos < end;
          pos += more ? 1u : 0u;
        }
      }
      if constexpr (DBUF) {
        const uint4 q = DT.template ld128<sizeof(DictSlot)>(uint32_t(dict_slot(hh[g], ix.dict_mask)), 0u, have[g], PR_DICT);
        d[g].head = (uint64_t(q.y) << 32) | q.x;
        d[g].len = q.z;
        d[g].word = q.w;
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      if (have[g]) {
        WordTok w;
        w.h = hh[g];
        w.head = hd[g];
        w.start = sl[g] & 0xFFFFu;
        w.len = sl[g] >> 16;
        w.b0 = uint32_t(hd[g] & 0xFF);
        sink(lev, dict_resolve(ix, w, d[g], tb_lo));
        ++lev;
      }
    }
  }
  while (more) {  // deep topic: count the remaining levels
    const WordTok w = next_word_s(lds, pos, end);
    if (w.len == 1 && (w.b0 == '+' || w.b0 == '#')) {
      wild = true;
      break;
    }
    ++lev;
    more = pos < end;
    pos += more ? 1u : 0u;
  }
  if (wild) fl |= TOK_WILD;
  if (lev > uint32_t(TOK_LMAX)) fl |= TOK_DEEP;
  return (lev < 255u ? lev : 255u) | fl;
}

// Unstaged text (a block whose text does not fit TOK_STAGE): one topic from
// global memory, the next word's first dictionary slot loaded while this word
// resolves.
__device__ __forceinline__ uint32_t tokenize_topic(ByteReader& rd, uint64_t pos, uint64_t end, const IndexView& ix,
                                                   const uint8_t* tb, WidsToRegs&& sink) {
  uint32_t lev = 0, fl = 0;
  WordTok w = next_word(rd, pos, end);
  DictSlot d = dict_first(ix, w);
  if (w.len > 0 && w.b0 == '$') fl |= TOK_DOLLAR;  // emqx_trie.erl:271-278
  for (;;) {
    if (w.len == 1 && (w.b0 == '+' || w.b0 == '#')) {  // emqx_topic:wildcard/1
      fl |= TOK_WILD;
      break;
    }
    const bool more = pos < end;
    WordTok wn;
    DictSlot dn;
    if (more) {
      ++pos;
      wn = next_word(rd, pos, end);
      dn = dict_first(ix, wn);
    }
    if (lev < TOK_LMAX) sink(lev, dict_resolve(ix, w, d, tb));
    ++lev;
    if (!more) break;
    w = wn;
    d = dn;
  }
  if (lev > TOK_LMAX) fl |= TOK_DEEP;
  return (lev < 255u ? lev : 255u) | fl;
}

// The block's topic text [toff[t0], toff[t0+256]) is staged in LDS with
// coalesced 8-byte loads when it fits TOK_STAGE bytes (a wave's lanes then
// scan their own topics from LDS instead of issuing dependent global loads
// at every 8-byte boundary); a longer block reads global memory directly.
constexpr int TOK_STAGE = 16384;

// ---- the coop walk: the wave's frontier as one compacted work list ---------
// A lane-private frontier per topic (as k_match_lds keeps one) costs a wave as
// many probe rounds per level as its LONGEST frontier (C2: ~1.6 entries per
// topic on average, but the longest of 64 lanes is 3-4) and the exec-mask
// bookkeeping of those divergent rounds.  Here the frontier entries of all 64
// topics of the tile form one list in LDS, {node | FR_PLUS, signature, topic
// lane}; every round each lane takes the next entry of the list, so a level
// costs ceil(entries / 64) rounds with every lane busy.  Children are
// appended to the next level's list with ballot + mbcnt compaction; matches go
// to the topic's row through an LDS counter per topic (ds_add_rtn).  A topic whose entries do not fit the list, or whose
// row outgrows FAST_MC, is marked (CW_OVF) and queued for the listed pass.
// Frontier entries per wave and level: 9 B each, two lists, so a 4-wave
// block's LDS is 72 * CW_CAP + 3 KB; 236 keeps it under 20 KB, i.e. 8 blocks
// (32 waves) per CU in 160 KB.  (192 -> 236 cut C3's list overflow rows; the
// overflowed topics are re-walked by the listed pass.)
#ifndef GM_CW_CAP
#define GM_CW_CAP 236
#endif
constexpr int CW_CAP = GM_CW_CAP;
constexpr uint32_t CW_OVF = 0x40000000u;   // in a topic's LDS match counter: queued for the listed pass
// compact staging entry: filter id (< 2^22) | lane << 22 | the match's rank in its row << 28
constexpr uint32_t CMP_SHIFT = 22, CMP_RANK = 28;

#ifdef GM_PROBE_STATS
// Diagnostic build only (-DGM_PROBE_STATS): a census of the coop walk's
// probes per level [level][k]: 0 entries, 1 exact candidates (a word), 2 past
// the signature, 3 past the exact-edge filter (= exact probes issued), 4 exact
// children found, 5 '+' slot probes issued, 6 '+' children found (slot), 7
// '+' children taken inline.  Printed by run_match after each call.
__device__ unsigned long long g_pstats[8][8];
#endif
#ifdef GM_PHASE_STATS
// Diagnostic build only (-DGM_PHASE_STATS): per wave of k_match_fused, one
// record of 16 words in g_phase_rec[tile], accumulated in registers and
// written once at the wave's end (no atomics, no read-modify-write in the
// walk): [0] staging, [1] tokenizer, [2+l] walk level l (l < 8) in s_memtime
// ticks, [10] epilogue, [11] rounds of levels 0-3 (8 bits each), [12] rounds of
// levels 4-7, [13] rounds with a chain tail load, [14] the walk in s_memtime
// ticks and [15] in s_memrealtime ticks (100 MHz): their ratio is the
// in-kernel clock.  run_match reduces them after each call.
__device__ uint32_t* g_phase_rec;
struct PhaseRec {
  uint32_t v[32];  // [16 + l] ticks of level l's rounds up to the probes' data, [24 + l] the rest of them
};
#define GM_PHASE_ADD(k, x) (PH.v[k] += uint32_t(x))
// level-indexed adds with constant indices (a dynamic index would put the
// record in scratch memory)
__device__ __forceinline__ void phase_level(PhaseRec& PH, uint32_t level, uint32_t ticks, uint32_t rounds, uint32_t t_data,
                                            uint32_t t_rest) {
  switch (level) {
#define GM_PH_CASE(L)                                          \
  case L:                                                      \
    PH.v[2 + L] += ticks;                                      \
    PH.v[L < 4 ? 11 : 12] += rounds << (8 * (L & 3));          \
    PH.v[16 + L] += t_data;                                    \
    PH.v[24 + L] += t_rest;                                    \
    break;
    GM_PH_CASE(0) GM_PH_CASE(1) GM_PH_CASE(2) GM_PH_CASE(3) GM_PH_CASE(4) GM_PH_CASE(5) GM_PH_CASE(6)
    default:
      PH.v[9] += ticks;
      PH.v[12] += rounds << 24;
      PH.v[23] += t_data;
      PH.v[31] += t_rest;
      break;
#undef GM_PH_CASE
  }
}
#else
struct PhaseRec {};
#define GM_PHASE_ADD(k, x) \
  do {                     \
  } while (0)
#endif

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ uint32_t lane_prefix(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi(uint32_t(mask >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(mask), 0u));
}

// One wave's walk over its 64-topic tile (coop_walk_tile, below).  h = the
// topic's tokenizer header; `words` holds the topic's word ids in the lane's
// registers: of level 0 (first()), of the next level (next()) and of the one
// after it (peek1()); the LDS arrays are the wave's own.
struct CoopLds {
  uint2 e[2][CW_CAP];      // {hot id | FR_PLUS, exact-child signature}
  uint8_t ln[2][CW_CAP];   // the entry's topic (lane of the tile)
  uint2 lw[64];            // per topic: {this level's word id, levels | TOK_DOLLAR}
  uint32_t mc[64];         // per topic: matches emitted | CW_OVF
};
struct WordsFromRegs {
  uint32_t (&w)[TOK_LMAX];
  __device__ __forceinline__ uint32_t peek1() { return w[1]; }  // after next(): the word of level + 2
  __device__ __forceinline__ uint32_t first() { return w[0]; }
  __device__ __forceinline__ uint32_t next() {  // shift the levels down: w[0] = the next level's word
#pragma unroll
    for (int q = 0; q + 1 < TOK_LMAX; ++q) w[q] = w[q + 1];
    return w[0];
  }
};

// CMP (compact staging, k_match_fused): the tile's matches go to ONE list in
// emission order, each entry (filter id | lane | rank in the row), written by
// ballot + mbcnt; tlen[tile] = the list's length.  k_assemble_c sorts them
// into rows.  A tile whose list would pass 64 x FAST_MC entries sends every
// topic to the listed pass.  Otherwise ([slot][lane]): one column per topic.
// IX_D0: a topic's level-0 exact probe, issued by k_match_fused right after
// its tokenizer (the home slot of (root, level-0 word) in the depth-1 table;
// s = NONE: no probe) and resolved in the walk's level-0 round.
struct D0Probe {
  uint4 a;     // the home slot's head {key lo, key hi, sig, hf}
  uint32_t s;  // its slot index, or NONE
};

// ---- the coop walk's table reads through TabRef ----------------------------
// (hot_load, hot_resolve_x, ... above with every lane's request under a
// predicate instead of a branch; a lane with pred false gets zeros)
constexpr uint32_t HS = sizeof(HotSlot);
template <bool FLAT>
__device__ __forceinline__ HotRec hot_load_t(const TabRef<FLAT>& T, uint32_t s, bool with_end, bool pred,
                                             uint32_t pol = 0) {
  HotRec r;
  r.a = T.template ld128<HS>(s, 0u, pred, PR_HOT, pol);
  const uint32_t ef = T.template ld32<HS>(s, 16u, pred && with_end, PR_HOT);
  r.ef = with_end ? ef : NONE;
  return r;
}
template <bool FLAT>
__device__ __forceinline__ HotRec plus_inline_load_t(const TabRef<FLAT>& PT, uint32_t id, bool pred) {
  const uint4 q = PT.template ld128<HS>(id & SLOT_MASK, 16u, pred, PR_HOT);
  HotRec r;
  r.a = make_uint4(0u, 0u, q.y, q.z);
  r.ef = q.w;
  return r;
}
// the levels' tables of one walk level (wave-uniform): the children's hot
// table, its MPH bucket words and its exact-edge filter
template <bool FLAT>
struct LevelTabs {
  TabRef<FLAT> T, MW, FT;
  uint32_t cap, mc, nb, fmask;
  bool rh, ovf;
  __device__ __forceinline__ LevelTabs(const IndexView& ix, int ht)
      : T(ix.hot + ix.hot_off[ht], uint32_t(ix.hot_cap[ht]) * HS),
        MW(ix.mph_word + ix.mph_off[ht], ix.mph_nb[ht] * 8u),
        FT(ix.efilt + ix.efilt_off[ht], ix.efilt_mask[ht] ? (ix.efilt_mask[ht] + 1u) * 4u : 0u),
        cap(uint32_t(ix.hot_cap[ht])),
        mc(ix.mph_cap[ht]),
        nb(ix.mph_nb[ht]),
        fmask(ix.efilt_mask[ht]),
        rh(((ix.rh_mask >> ht) & 1u) != 0),
        ovf(((ix.mph_ovf >> ht) & 1u) != 0) {}
  // an MPH table's bucket word for `key`: its perfect slot, and whether the table may hold it
  __device__ __forceinline__ bool gate(uint64_t key, bool pred, uint32_t& s) const {
    const uint2 w2 = MW.template ld64<8u>(mph_bucket(key, nb), pred, PR_GATE);
    s = mph_slot(key, w2.x & 0xFFFFu, mc);
    return pred && mph_may_hold((uint64_t(w2.y) << 32) | w2.x, key);
  }
  // the exact-edge filter's verdict on `key` (fmask != 0)
  __device__ __forceinline__ bool filter(uint64_t key, bool pred) const {
    const uint32_t fh = edge_filter_hash(key);
    const uint32_t fb = edge_filter_bits(fh);
    return pred && (FT.template ld32<4u>(edge_filter_word(fh, fmask), 0u, pred, PR_GATE) & fb) == fb;
  }
  // hot_resolve_x: the slot of `key` from its loaded home slot (s, r), or NONE
  __device__ __forceinline__ uint32_t resolve(uint64_t key, uint32_t s, HotRec& r, bool with_end) const {
    if (mc) {
      if (hot_is(r, key)) return s;
      if (!ovf) return NONE;
      for (s = mph_ovf_home(key, mc, cap);; s = s + 1 == cap ? mc : s + 1) {
        r = hot_load_t(T, s, with_end, true);
        if (hot_is(r, key)) return s;
        if (hot_empty(r)) return NONE;
      }
    }
    uint32_t dist = 0;
    while (!hot_is(r, key)) {
      if (hot_empty(r)) return NONE;
      if (rh) {
        const uint32_t h = uint32_t(hot_slot((uint64_t(r.a.y) << 32) | r.a.x, cap));
        if ((s >= h ? s - h : s + cap - h) < dist) return NONE;
      }
      s = s + 1 == cap ? 0 : s + 1;
      ++dist;
      r = hot_load_t(T, s, with_end, true);
    }
    return s;
  }
};

template <bool FLAT>
__device__ __forceinline__ D0Probe d0_issue(const IndexView& ix, uint32_t w0, uint32_t h, bool valid) {
  D0Probe p{make_uint4(0u, 0u, 0u, 0u), NONE};
  const bool walk = valid && !(h & (TOK_WILD | TOK_DEEP));
  bool go = walk && w0 != NONE && (ix.root_sig & sig_bit(w0));
  const int ht = hot_table(1);
  const uint64_t key = hot_key(0u, w0, 0u);
  const uint32_t cap = uint32_t(ix.hot_cap[ht]);
  uint32_t s;
  if (const uint32_t mc = ix.mph_cap[ht]) {
    const TabRef<FLAT> MW(ix.mph_word + ix.mph_off[ht], ix.mph_nb[ht] * 8u);
    const uint2 w2 = MW.template ld64<8u>(mph_bucket(key, ix.mph_nb[ht]), go, PR_TAIL);
    s = mph_slot(key, w2.x & 0xFFFFu, mc);
    go = go && mph_may_hold((uint64_t(w2.y) << 32) | w2.x, key);
  } else {
    s = uint32_t(hot_slot(key, cap));
  }
  const TabRef<FLAT> T(ix.hot + ix.hot_off[ht], cap * HS);
  const uint4 a = T.template ld128<HS>(s, 0u, go, PR_TAIL);
  if (go) {
    p.a = a;
    p.s = s;
  }
  return p;
}

// Level 0 under IX_D0 issues no probe of its own.  Each
// walking lane takes its own topic's root entry, resolves the exact probe its
// tokenizer issued (d1; parked in the level-0 list's LDS, which a level-0
// round from registers does not use) and takes the root's '+' child from
// ix.d0_root (one uniform load); the rest of the round -- visits, chains,
// pushes, probe counts -- is the general round's.
// AB false (the default instantiation of k_match_fused): none of the A/B forms
// -- the sc1 staging store (IX_STAGE_SC1), the hot-probe cache policies
// (l1_bypass / hot_policy), level 0 without IX_D0 -- is compiled in;
// launch_match picks AB true whenever the call's view or knobs ask for one.
// FLAT: the tables are read with flat loads (TabRef), chosen per index at launch.
template <bool EXACT, bool NT, bool CMP, bool AB, bool FLAT>
__device__ __forceinline__ void coop_walk_tile(CoopLds& L, uint32_t h, WordsFromRegs& words, bool valid, uint64_t t,
                                               int lane, const uint8_t* __restrict__ tb,
                                               const uint64_t* __restrict__ toff, const IndexView& ix,
                                               uint32_t* __restrict__ cnt, uint32_t* __restrict__ stage,
                                               uint32_t* __restrict__ ovf_list, uint32_t* __restrict__ ovf_n,
                                               unsigned long long* __restrict__ probe_tile,
                                               unsigned long long* __restrict__ wild_ctr,
                                               uint64_t* __restrict__ tsum, uint32_t* __restrict__ tlen,
                                               uint8_t* __restrict__ cnt8, PhaseRec& PH, D0Probe d1) {
  (void)PH;
  constexpr uint32_t MC = FAST_MC;
  constexpr uint32_t TCAP = 64u * FAST_MC;  // a tile's staging entries
  // d0: the lanes' issued level-0 probes wait in the level-0 list's LDS (a
  // level-0 round from registers reads no list), not in VGPRs: stored first
  // thing, before the wildcard topics' literal lookup needs its registers
  uint4* const D1L = reinterpret_cast<uint4*>(L.e[0]);
  uint32_t* const D1S = reinterpret_cast<uint32_t*>(D1L + 64);
  static_assert(sizeof(L.e[0]) >= 64 * (sizeof(uint4) + 4), "the level-0 list holds 64 probes");
  const bool d0 = !AB || (ix.flags & IX_D0);  // (wave-uniform)
  if (d0) {
    D1L[lane] = d1.a;
    D1S[lane] = d1.s;
  }
  const uint64_t tile = t >> 6;
  uint32_t* const MCNT = L.mc;
  uint2* const LW = L.lw;
  uint32_t* const stile = stage + tile * (64ull * MC);
  // CMP: the tile's list, its row bytes and its length through buffer
  // resources whose bases are the wave's own (readfirstlane of the two address
  // halves: the tile offset is out of the 32-bit lane offsets, so a batch's
  // staging may pass 4 GiB) -- one 32-bit offset per store
  auto wave_rsrc = [](const void* q, uint32_t bytes) {
    const uint64_t a = reinterpret_cast<uint64_t>(q);
    // (the builtin returns int: both halves back to unsigned before they are joined)
    const uint64_t u = (uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(uint32_t(a >> 32)))) << 32) |
                       uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(uint32_t(a))));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(u), (short)0, int(bytes), 0x00020000);
  };
  constexpr bool SBUF = CMP && !FLAT;
  const __amdgpu_buffer_rsrc_t srs = wave_rsrc(SBUF ? stile : nullptr, SBUF ? TCAP * 4u : 0u);
  // one entry of the list (k < TCAP); sc1: IX_STAGE_SC1 (A/B)
  auto stage_put = [&](uint32_t k, uint32_t v, bool sc1) {
    if constexpr (SBUF) {
      if (AB && sc1) __builtin_amdgcn_raw_buffer_store_b32(v, srs, int(k * 4u), 0, 16);
      else __builtin_amdgcn_raw_buffer_store_b32(v, srs, int(k * 4u), 0, NT ? 2 : 0);
    } else {
      stage_st<NT>(stile, k, v, AB && sc1);
    }
  };
  const bool sc1st = AB && (ix.flags & IX_STAGE_SC1) != 0;
  const uint32_t nlev = h & 0xFFu;
  const bool dollar = (h & TOK_DOLLAR) != 0, wild = valid && (h & TOK_WILD), deep = valid && (h & TOK_DEEP);
  const bool walk = valid && !wild && !deep;
  uint32_t m0 = deep ? CW_OVF : 0u;  // deep topics: the listed pass tokenizes them itself
  uint32_t f0 = NONE;
  if (wild && EXACT) {  // a wildcard publish topic: the literal route only (emqx_router.erl:128-134)
    f0 = literal_lookup(ix, tb, toff[t], toff[t + 1]);
  }
  if (walk && !dollar && ix.root_hash != NONE) f0 = ix.root_hash;  // '#' at the virtual root ('$' rule: emqx_trie.erl:271-278)
  uint32_t wbase = 0;  // CMP: entries in the tile's list (wave-uniform)
  if (f0 != NONE) m0 = 1;
  if constexpr (CMP) {  // (rank 0 of the lane's row)
    const unsigned long long b0 = __ballot(f0 != NONE);
    if (f0 != NONE) stage_put(lane_prefix(b0), f0 | (uint32_t(lane) << CMP_SHIFT), sc1st);
    wbase = uint32_t(__popcll(b0));
  } else {
    if (f0 != NONE) stile[lane] = f0;
  }
  MCNT[lane] = m0;
  uint32_t probes = walk ? 1u : 0u;  // + the exact-route probe
  // level 0: one root entry per walking topic
  const unsigned long long bw = __ballot(walk);
  uint32_t wnext = walk ? words.first() : NONE;
  if (walk && !d0) {
    const uint32_t p = lane_prefix(bw);
    L.e[0][p] = make_uint2((!dollar && (ix.root_flags & HOT_PLUS)) ? FR_PLUS : 0u, ix.root_sig);
    L.ln[0][p] = uint8_t(lane);
  }
  uint32_t cur_total = uint32_t(__popcll(bw));
  uint4 rq = D1_NONE;                       // the root's '+' child {hot id, sig, hf, end}
  if (d0) rq = *reinterpret_cast<const uint4*>(ix.d0_root);
  int cur = 0;
#ifdef GM_PHASE_STATS
  uint64_t tph = __builtin_amdgcn_s_memtime();
  const uint64_t tw0 = tph, tr0w = __builtin_amdgcn_s_memrealtime();
#endif
  // One level of the walk (a lambda, so that level 0 under IX_D0 -- the round
  // from registers -- is its own instance and its extra live values do not
  // raise the general loop's register pressure)
  auto walk_level = [&](uint32_t level, auto d0r_tag) {
    constexpr bool D0R = decltype(d0r_tag)::value;
#ifdef GM_PHASE_STATS
    const uint32_t ph_rounds = (cur_total + 63) / 64;
    uint32_t ph_data = 0, ph_rest = 0;
#endif
    LW[lane] = make_uint2(wnext, nlev | (dollar ? TOK_DOLLAR : 0u));
    if (walk && level + 1 < nlev) wnext = words.next();  // next level's word
    const uint32_t wnext2 = words.peek1();  // the word after it (chain nodes of two words)
    wave_lds_sync();
    const uint32_t lvl = __builtin_amdgcn_readfirstlane(level);
    const int ht = hot_table(lvl + 1);
    const LevelTabs<FLAT> LT(ix, ht);
    // the frontier nodes' own table (their inline '+' children)
    const TabRef<FLAT> PT(ix.hot + ix.hot_off[hot_table(lvl)], uint32_t(ix.hot_cap[hot_table(lvl)]) * HS);
    // the probes' cache policy (A/B: GM_L1_BYPASS, GM_HOT_POLICY)
    uint32_t nol1 = 0u;
    if constexpr (AB) nol1 = ((ix.l1_bypass >> ht) & 1u) ? ix.hot_policy : 0u;
    const uint2* E = L.e[cur];
    const uint8_t* LNc = L.ln[cur];
    uint2* EN = L.e[cur ^ 1];
    uint8_t* LNn = L.ln[cur ^ 1];
    uint32_t nxt_total = 0;
    for (uint32_t base = 0; base < (D0R ? 1u : cur_total); base += 64) {
#ifdef GM_PHASE_STATS
      const uint64_t tr0 = __builtin_amdgcn_s_memtime();
#endif
      GM_PAD();
      // (d0r: level 0 from registers; every walking lane takes its own root entry)
      constexpr bool d0r = D0R;
      const uint32_t e = base + uint32_t(lane);
      const bool act = d0r ? walk : e < cur_total;
      const uint2 en = d0r ? make_uint2((!dollar && (ix.root_flags & HOT_PLUS)) ? FR_PLUS : 0u, ix.root_sig)
                           : act ? E[e] : make_uint2(0u, 0u);
      const uint32_t tl = d0r ? uint32_t(lane) : act ? LNc[e] : 0u;
      const uint2 lw = LW[tl];
      const uint32_t wid = lw.x, id = en.x & ID_MASK;
      const bool last = act && level + 1 == (lw.y & 0xFFu);
      const bool ldollar = (lw.y & TOK_DOLLAR) != 0;
      bool dx = act && wid != NONE && (en.y & sig_bit(wid));
#ifdef GM_PROBE_STATS
      const bool st_cand = act && wid != NONE, st_sig = dx;
#endif
      bool dp = act && (en.x & FR_PLUS);
      probes += act ? 3u : 0u;
      const bool pin = dp && plus_is_inline(lvl, id);
      const uint64_t kx = hot_key(id, wid, lvl), kp = hot_key(id, ix.plus_word, lvl);
      uint32_t sx = 0, sp = 0;
      HotRec rx{}, rp{};
      uint32_t hx = NONE, hp = NONE;
      if (d0r) {
        const uint32_t s1 = D1S[lane];
        dx = dx && s1 != NONE;  // (NONE: the tokenizer's gates -- root sig, MPH Bloom bits -- ruled it out)
        if (dx) {  // resolve the issued probe; the end filter (a one-level topic) from the found slot
          rx.a = D1L[lane];
          rx.ef = NONE;
          hx = LT.resolve(kx, s1, rx, false);
        }
        // (a one-level topic: the end filter from the found slot)
        const uint32_t ef1 = LT.T.template ld32<HS>(hx, 16u, dx && last && hx != NONE, PR_TAIL);
        if (dx && last && hx != NONE) rx.ef = ef1;
        if (dp) {
          hp = rq.x;
          rp.a = make_uint4(0u, 0u, rq.y, rq.z);
          rp.ef = last ? rq.w : NONE;
        }
      } else {
      if (LT.mc) {
        // an MPH table (wave-uniform): one L2 read of the key's bucket word
        // filters the probe and gives its slot, in place of the exact-edge filter
        dx = LT.gate(kx, dx, sx);
        const bool gp = LT.gate(kp, dp && !pin, sp);
        dp = pin || gp;
      } else {
        // the table's exact-edge filter (an L2 hit) before a random line
        if (LT.fmask) dx = LT.filter(kx, dx);
        sx = uint32_t(hot_slot(kx, LT.cap));
        sp = uint32_t(hot_slot(kp, LT.cap));
      }
      // issue both probes, then resolve
      rx = hot_load_t(LT.T, sx, last, dx, nol1);
      rp = plus_inline_load_t(PT, id, pin);
      {
        const HotRec rs = hot_load_t(LT.T, sp, last, dp && !pin, nol1);
        if (!pin) rp = rs;
      }
      hx = dx ? LT.resolve(kx, sx, rx, last) : NONE;
      hp = pin ? (id | HOT_INLINE) : dp ? LT.resolve(kp, sp, rp, last) : NONE;
      }
#ifdef GM_PHASE_STATS
      __builtin_amdgcn_s_waitcnt(0);  // (diagnostic build: the probes' data is in)
      const uint64_t tr1 = __builtin_amdgcn_s_memtime();
      ph_data += uint32_t(tr1 - tr0);
#endif
      // The topic's next word (its own lane holds it: wnext), for the push
      // filter and the chain nodes below
      const uint32_t w1 = uint32_t(__builtin_amdgcn_ds_bpermute(int(tl) << 2, int(wnext)));
#ifdef GM_PROBE_STATS
      {
        const unsigned long long c[8] = {__ballot(act), __ballot(st_cand), __ballot(st_sig), __ballot(dx),
                                         __ballot(hx != NONE), __ballot(dp && !pin), __ballot(dp && !pin && hp != NONE),
                                         __ballot(pin)};
        if (lane == 0)
          for (int k = 0; k < 8; ++k)
            if (c[k]) atomicAdd(&g_pstats[lvl < 7 ? lvl : 7][k], (unsigned long long)__popcll(c[k]));
      }
#endif
      const bool ex = hx != NONE, ep = hp != NONE;
      // Chain nodes (gm_common.h): the topic must continue with s1 (the head's
      // sig field) and end after the chain's Lc words; the tail {end, s2, -, F}
      // is read (an L2 hit: the head's line was just fetched) only when s1 agrees.
      const bool chx = ex && !last && (rx.a.w & HOT_CHAIN);
      const bool chp = ep && !last && (rp.a.w & HOT_CHAIN);
      const bool tx = chx && w1 == rx.a.z, tp = chp && w1 == rp.a.z;
      const uint32_t rem = (lw.y & 0xFFu) - (level + 1);  // the topic's words after this level (>= 1 when !last)
      uint32_t fx = NONE, fp = NONE, vx = 0, vp = 0;  // the chain's filter on a match; virtual probes
      if (__ballot(tx || tp)) {
        GM_PHASE_ADD(13, 1);
        const uint32_t w2 = uint32_t(__builtin_amdgcn_ds_bpermute(int(tl) << 2, int(wnext2)));
        uint4 qx{}, qp{};
        qx = LT.T.template ld128<HS>(hx, 16u, tx, PR_TAIL);
        qp = LT.T.template ld128<HS>(hp, 16u, tp, PR_TAIL);
        // the probes the reference NFA makes along the chain (SURVEY §8d's P):
        // c1 found at level+1 (+2 there if it is the topic's last level,
        // else +3 for c1's own frontier entry), c2 found at level+2 alike
        auto chain = [&](const uint4& q, uint32_t& f, uint32_t& vpr) {
          const uint32_t lc = q.y == NONE ? 1u : 2u;
          const bool two = lc == 2u && w2 == q.y;
          if (rem == lc && (lc == 1u || two)) f = q.w;
          vpr = rem == 1u ? 2u : 3u + (two ? (rem == 2u ? 2u : 3u) : 0u);
        };
        if (tx) chain(qx, fx, vx);
        if (tp) chain(qp, fp, vp);
      }
      const bool e5 = fx != NONE && (EXACT || (fx & END_WILD));
      const bool e6 = fp != NONE && (EXACT || (fp & END_WILD));
      // a node goes on to the next level only if one of its probes there can
      // find something: a '+' child, or an exact child the next word's
      // signature bit admits.  A node that stays behind (and a chain node) is
      // counted with the probes the reference NFA would make for it there.
      const uint32_t b1 = w1 != NONE ? sig_bit(w1) : 0u;
      const uint32_t yx = ex ? hot_sig(rx.a.w, rx.a.z) : 0u, yp = ep ? hot_sig(rp.a.w, rp.a.z) : 0u;
      const bool cx = ex && !last && !chx && ((rx.a.w & FR_PLUS) || (yx & b1));
      const bool cp = ep && !last && !chp && ((rp.a.w & FR_PLUS) || (yp & b1));
      probes += (ex && !last && !cx ? 3u + vx : 0u) + (ep && !last && !cp ? 3u + vp : 0u);
      // visits: 'match_#', the end filter on the last level, else the next frontier
      if constexpr (CMP) {
        const bool e1 = ex && (rx.a.w & HF_MASK) != HF_NONE;
        const bool e2 = ex && last && rx.ef != NONE && (EXACT || (rx.ef & END_WILD) || (ldollar && level == 0));
        const bool e3 = ep && (rp.a.w & HF_MASK) != HF_NONE;
        const bool e4 = ep && last && rp.ef != NONE && (EXACT || (rp.ef & END_WILD) || (ldollar && level == 0));
        probes += last ? 2u * (uint32_t(ex) + uint32_t(ep)) : 0u;
        // the row's counter hands this lane's matches their ranks in the row
        const uint32_t ne = uint32_t(e1) + uint32_t(e2) + uint32_t(e3) + uint32_t(e4) + uint32_t(e5) + uint32_t(e6);
        uint32_t rk = ne ? atomicAdd(&MCNT[tl], ne) : 0u;
        const uint32_t tag = uint32_t(tl) << CMP_SHIFT;
#define GM_CW_PUT(c, f)                                                                         \
  do {                                                                                          \
    const unsigned long long b_ = __ballot(c);                                                  \
    if (c) {                                                                                    \
      const uint32_t k_ = wbase + lane_prefix(b_);                                              \
      if (k_ < TCAP) stage_put(k_, (f) | tag | ((rk < MC ? rk : MC - 1) << CMP_RANK), sc1st); \
      ++rk;                                                                                     \
    }                                                                                           \
    wbase += uint32_t(__popcll(b_));                                                            \
  } while (0)
        GM_CW_PUT(e1, rx.a.w & HF_MASK);
        GM_CW_PUT(e2, rx.ef & ID_MASK);
        GM_CW_PUT(e3, rp.a.w & HF_MASK);
        GM_CW_PUT(e4, rp.ef & ID_MASK);
        if (__ballot(e5 || e6)) {
          GM_CW_PUT(e5, fx & ID_MASK);
          GM_CW_PUT(e6, fp & ID_MASK);
        }
#undef GM_CW_PUT
      } else {
#define GM_CW_EMIT(f)                                   \
  do {                                                  \
    const uint32_t k_ = atomicAdd(&MCNT[tl], 1u);       \
    if (k_ < MC) st_s<NT>(stile + k_ * 64u + tl, (f));  \
  } while (0)
#define GM_CW_VISIT(r)                                                                          \
  do {                                                                                          \
    if (((r).a.w & HF_MASK) != HF_NONE) GM_CW_EMIT((r).a.w & HF_MASK);                          \
    if (last) {                                                                                 \
      if ((r).ef != NONE && (EXACT || ((r).ef & END_WILD) || (ldollar && level == 0)))          \
        GM_CW_EMIT((r).ef & ID_MASK);                                                           \
      probes += 2u;                                                                             \
    }                                                                                           \
  } while (0)
        if (ex) GM_CW_VISIT(rx);
        if (ep) GM_CW_VISIT(rp);
        if (e5) GM_CW_EMIT(fx & ID_MASK);
        if (e6) GM_CW_EMIT(fp & ID_MASK);
#undef GM_CW_VISIT
#undef GM_CW_EMIT
      }
      const unsigned long long bx = __ballot(cx), bp = __ballot(cp);
      const uint32_t nx = uint32_t(__popcll(bx));
      if (cx) {
        const uint32_t q = nxt_total + lane_prefix(bx);
        if (q < uint32_t(CW_CAP)) {
          EN[q] = make_uint2(hx | (rx.a.w & FR_PLUS), yx);
          LNn[q] = uint8_t(tl);
        } else {
          atomicOr(&MCNT[tl], CW_OVF);
        }
      }
      if (cp) {
        const uint32_t q = nxt_total + nx + lane_prefix(bp);
        if (q < uint32_t(CW_CAP)) {
          EN[q] = make_uint2(hp | (rp.a.w & FR_PLUS), yp);
          LNn[q] = uint8_t(tl);
        } else {
          atomicOr(&MCNT[tl], CW_OVF);
        }
      }
      nxt_total += nx + uint32_t(__popcll(bp));
#ifdef GM_PHASE_STATS
      ph_rest += uint32_t(__builtin_amdgcn_s_memtime() - tr1);
#endif
    }
    cur ^= 1;
    cur_total = nxt_total < uint32_t(CW_CAP) ? nxt_total : uint32_t(CW_CAP);
    wave_lds_sync();
#ifdef GM_PHASE_STATS
    {
      const uint64_t tn = __builtin_amdgcn_s_memtime();
      phase_level(PH, level, uint32_t(tn - tph), ph_rounds, ph_data, ph_rest);
      tph = tn;
    }
#endif
  };
  uint32_t level0 = 0;
  if (d0 && cur_total) {
    walk_level(0u, std::true_type{});
    level0 = 1;
  }
  uint32_t level = level0;
  while (cur_total != 0) walk_level(level++, std::false_type{});  // (each level updates cur_total)
  wave_lds_sync();
  const uint32_t m_n = MCNT[lane];
  // CW_OVF or a row past the staging capacity; CMP: the tile's list past its capacity
  const bool ovf = valid && (m_n > MC || (CMP && wbase > TCAP));
  const __amdgpu_buffer_rsrc_t c8rs = wave_rsrc(SBUF ? cnt8 + tile * 64u : nullptr, SBUF ? 64u : 0u);  // the tile's 64 row bytes
  if (valid) {
    // CMP: one byte per row (0xFF: the listed and slow passes write the row's cnt word)
    if constexpr (CMP) {
      if constexpr (SBUF) __builtin_amdgcn_raw_buffer_store_b8(uint8_t(ovf ? 0xFFu : m_n), c8rs, lane, 0, NT ? 2 : 0);
      else st_s<NT>(cnt8 + t, uint8_t(ovf ? 0xFFu : m_n));
      // (the listed pass writes its rows' cnt words; until it has run -- it is
      // deferred to the host's read-back, MatchCall::finish -- the row reads
      // as a slow row with no ids, so an assembly before it stays in bounds)
      if (ovf) cnt[t] = OVF_BIT;
    } else {
      st_s<NT>(cnt + t, ovf ? OVF_BIT : m_n);
    }
    if (ovf) ovf_list[atomicAdd(ovf_n, 1u)] = uint32_t(t);
  }
  if constexpr (SBUF) {
    if (lane == 0)
      __builtin_amdgcn_raw_buffer_store_b32(wbase < TCAP ? wbase : TCAP, wave_rsrc(tlen + tile, 4u), 0, 0, NT ? 2 : 0);
  } else if (CMP && lane == 0) {
    st_s<NT>(tlen + tile, wbase < TCAP ? wbase : TCAP);
  }
  uint32_t ptot, mtot;
  wave_excl_scan(probes, ptot);
  wave_excl_scan(valid && !ovf ? m_n : 0u, mtot);
  const unsigned long long wb = __ballot(wild);
  if (lane == 0) {
    probe_tile[tile] = ptot;
    tsum[tile] = mtot;
    if (wb) atomicAdd(wild_ctr, (unsigned long long)__popcll(wb));
  }
#ifdef GM_PHASE_STATS
  PH.v[14] = uint32_t(__builtin_amdgcn_s_memtime() - tw0);
  PH.v[15] = uint32_t(__builtin_amdgcn_s_memrealtime() - tr0w);
  GM_PHASE_ADD(10, __builtin_amdgcn_s_memtime() - tph);
  if (lane == 0 && g_phase_rec)
    for (int k = 0; k < 32; ++k) g_phase_rec[tile * 32 + k] = PH.v[k];
#endif
}

// ---- k_match_fused: tokenize + coop walk in one kernel --------------------
// The block stages its topics' text in LDS (stage_text: the offsets' loads
// issued together at entry, then every text load in flight before the first
// LDS write) and each lane tokenizes its topic
// into REGISTERS (word ids of up to TOK_LMAX levels, the header); then each
// wave walks its tile (coop_walk_tile) in the same LDS.  The word ids and
// headers never go through HBM (as two kernels they cost ~48 B per C2 topic,
// written and read back), and the tokenizer's ALU work of one wave overlaps
// the walk's gathers of the others.
constexpr size_t FUSED_LDS = sizeof(CoopLds) * 4 > (TOK_STAGE + 8) ? sizeof(CoopLds) * 4 : (TOK_STAGE + 8);

// Two uniform 8-byte loads issued together, one wait for both (left to the
// compiler, the first is waited for before the second is issued: one more
// round trip at the head of every block)
__device__ __forceinline__ void ld_uniform_pair(const uint64_t* p0, const uint64_t* p1, uint64_t& a, uint64_t& b) {
  asm volatile("s_load_dwordx2 %0, %2, 0x0\n\ts_load_dwordx2 %1, %3, 0x0\n\ts_waitcnt lgkmcnt(0)"
               : "=&s"(a), "=&s"(b)
               : "s"(p0), "s"(p1)
               : "memory");
}

// Text staging with every load in flight before the first LDS write: bytes
// [0, r8) of src (8-byte aligned; r8 a multiple of 8, at most CAP) go to dst,
// 16 bytes per lane and trip, W lanes (id < W) sharing the copy.  The loads go
// through a buffer resource of the text's own size (rounded up to the 16-byte
// access: at most 8 bytes past r8), so a lane past the text issues its load
// like the others and the range check drops it -- no branch around a load, no
// wait between two of them.  The first FIRST trips cover the common text; a
// longer one takes the rest of the trips under one uniform branch.  LDS
// writes are bounded by r8 word by word (dst holds r8 bytes, not the rounding).
template <int W, int CAP, bool NT, int FIRST = 2>
__device__ __forceinline__ void stage_text(uint64_t* dst, const uint8_t* src, uint32_t r8, uint32_t id) {
  constexpr int TRIP = 16 * W, TRIPS = (CAP + TRIP - 1) / TRIP, T0 = FIRST < TRIPS ? FIRST : TRIPS;
  const uint64_t a = reinterpret_cast<uint64_t>(src);
  const uint64_t u = (uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(uint32_t(a >> 32)))) << 32) |
                     uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(uint32_t(a))));
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(u), (short)0, int((r8 + 15u) & ~15u), 0x00020000);
  const uint32_t o = id * 16u;
  auto ld = [&](int k) { return __builtin_amdgcn_raw_buffer_load_b128(rs, int(o + uint32_t(k * TRIP)), 0, NT ? 2 : 0); };
  auto put = [&](int k, const auto& v) {
    const uint32_t b = o + uint32_t(k * TRIP);
    if (b < r8) dst[b >> 3] = (uint64_t(uint32_t(v[1])) << 32) | uint32_t(v[0]);
    if (b + 8u < r8) dst[(b >> 3) + 1] = (uint64_t(uint32_t(v[3])) << 32) | uint32_t(v[2]);
  };
  {
    decltype(ld(0)) v[T0];
#pragma unroll
    for (int k = 0; k < T0; ++k) v[k] = ld(k);
#pragma unroll
    for (int k = 0; k < T0; ++k) put(k, v[k]);
  }
  if constexpr (TRIPS > T0) {
    if (r8 > uint32_t(T0 * TRIP)) {  // uniform
      decltype(ld(0)) v[TRIPS - T0];
#pragma unroll
      for (int k = T0; k < TRIPS; ++k) v[k - T0] = ld(k);
#pragma unroll
      for (int k = T0; k < TRIPS; ++k) put(k, v[k - T0]);
    }
  }
}

// AB, FLAT: coop_walk_tile's (the default instantiation is AB false, FLAT false)
template <bool EXACT, bool NT, bool TOKPRIO, bool CMP, bool AB, bool FLAT>
__global__ __launch_bounds__(256, 8) void k_match_fused(const uint8_t* __restrict__ tb,
                                                        const uint64_t* __restrict__ toff, uint64_t n, IndexView ix,
                                                        uint32_t* __restrict__ cnt, uint32_t* __restrict__ stage,
                                                        uint32_t* __restrict__ ovf_list, uint32_t* __restrict__ ovf_n,
                                                        unsigned long long* __restrict__ probe_tile,
                                                        unsigned long long* __restrict__ wild_ctr,
                                                        uint64_t* __restrict__ tsum, uint32_t* __restrict__ tlen,
                                                        uint8_t* __restrict__ cnt8) {
  __shared__ __align__(16) uint8_t s_raw[FUSED_LDS];  // the staged text, then the walk's lists
  uint64_t* const s_txt = reinterpret_cast<uint64_t*>(s_raw);
  // (wv through readfirstlane: the tile's base and the wave's slice are scalar values, not VGPRs)
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  // TOKPRIO: staging and tokenizing at wave priority 1, the walk at 0.  A block
  // holds its 20 KB of LDS (one of the CU's 8 block slots) through both phases
  // but only the walk keeps lines in flight, so the SIMD's issue arbiter favours
  // the waves that are still getting their block to the walk (C2 9.20 -> 9.10
  // ms, C3 13.68 -> 13.54; raising late walk levels instead was slower:
  // profiles/r02_ab/prio*_c*.txt)
  if constexpr (TOKPRIO) __builtin_amdgcn_s_setprio(1);
#ifdef GM_PHASE_STATS
  const uint64_t tp0 = __builtin_amdgcn_s_memtime();
#endif
  const uint64_t t0 = uint64_t(blockIdx.x) * 256u;
  const uint64_t tw = t0 + uint32_t(wv) * 64u;  // the wave's first topic
  const uint64_t t = tw | uint32_t(lane);
  const bool valid = t < n;
  // the lane's own offsets, issued first (a lane past n reads the last
  // topic's: toff has n + 1 entries)
  const uint64_t tc = valid ? t : n - 1;
  const uint64_t pos = toff[tc], end = toff[tc + 1];
  // the block's text [lo, hi): both bounding offsets in one round trip
  const uint64_t tl = t0 + 256 < n ? t0 + 256 : n;
  uint64_t lo, hi;
  ld_uniform_pair(toff + t0, toff + tl, lo, hi);
  lo &= ~7ull;
  const bool staged = hi - lo <= uint64_t(TOK_STAGE) - 8;  // block-uniform
  // (one word past the text for the funnel shifts: topic buffers are padded by 64 bytes)
  if (staged) stage_text<256, TOK_STAGE, NT>(s_txt, tb + lo, uint32_t(((hi - lo + 7) & ~7ull) + 8), threadIdx.x);
  __syncthreads();
  PhaseRec PH{};
#ifdef GM_PHASE_STATS
  const uint64_t tp1 = __builtin_amdgcn_s_memtime();
  PH.v[0] = uint32_t(tp1 - tp0);
#endif
  uint32_t w[TOK_LMAX];
#pragma unroll
  for (int q = 0; q < TOK_LMAX; ++q) w[q] = NONE;
  uint32_t h = 0;
  if (valid) {
    if (staged) {
      h = tokenize_grouped<!FLAT>(s_txt, uint32_t(pos - lo), uint32_t(end - lo), ix, tb + lo, WidsToRegs{w});
    } else {
      ByteReader rd{tb, ~0ull, 0};
      h = tokenize_topic(rd, pos, end, ix, tb, WidsToRegs{w});
    }
  }
  __syncthreads();  // every lane is done with the staged text: the walk reuses the LDS
#ifdef GM_PHASE_STATS
  PH.v[1] = uint32_t(__builtin_amdgcn_s_memtime() - tp1);
#endif
  if constexpr (TOKPRIO) __builtin_amdgcn_s_setprio(0);
  if ((t >> 6) * 64 >= n) return;  // wave-uniform, after the last workgroup barrier
  // IX_D0: the level-0 exact probe -- the depth-1 node (root, level-0 word) --
  // issued before the walk's setup and resolved in its level-0 round (held
  // across the block barrier it spilled)
  D0Probe d1{make_uint4(0u, 0u, 0u, 0u), NONE};
  if (!AB || (ix.flags & IX_D0)) d1 = d0_issue<FLAT>(ix, w[0], h, valid);
  WordsFromRegs words{w};
  // the walk's topic index, formed again from the wave's scalar base (hidden
  // from value numbering) so that the front end's copy is not held in two
  // VGPRs through the tokenizer
  uint32_t twl = uint32_t(tw), twh = uint32_t(tw >> 32);
  asm volatile("" : "+s"(twl), "+s"(twh));
  const uint64_t t_w = (uint64_t(twh) << 32) | (twl | uint32_t(lane));
  coop_walk_tile<EXACT, NT, CMP, AB, FLAT>(reinterpret_cast<CoopLds*>(s_raw)[wv], h, words, valid, t_w, lane, tb, toff, ix,
                                           cnt, stage, ovf_list, ovf_n, probe_tile, wild_ctr, tsum, tlen, cnt8, PH, d1);
}

// ---- the match call's pass counters; its scan is gm_scan.h's scan_excl -----
__global__ void k_zero16(uint32_t* __restrict__ p) {  // 16 words (64 B)
  if (threadIdx.x < 16) p[threadIdx.x] = 0u;
}

struct LoadCnt {  // masked match counts
  const uint32_t* p;
  __device__ uint64_t operator()(uint64_t i) const { return p[i] & CNT_MASK; }
};

// ---------------------------------------------------------------------------
// assembly
// ---------------------------------------------------------------------------
// Sort a row held in FAST_MC registers (unused slots = 0xFFFFFFFF) with a
// bitonic network over its first N slots; every index is static after
// unrolling.  Valid when every slot at or past N holds the sentinel.
template <int N>
__device__ __forceinline__ void sort_row(uint32_t (&m)[FAST_MC]) {
  static_assert(N <= FAST_MC && (N & (N - 1)) == 0, "bitonic width");
#pragma unroll
  for (int k = 2; k <= N; k <<= 1)
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1)
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const int l = i ^ j;
        if (l > i) {
          const uint32_t a = m[i], b = m[l];
          const bool up = (i & k) == 0;
          const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
          m[i] = up ? lo : hi;
          m[l] = up ? hi : lo;
        }
      }
}

// One tile's rows once the wave's longest row is known to fit W slots (W is
// wave-uniform): W stage loads, the W-wide bitonic network and W stores per
// lane instead of FAST_MC.  At C2 (2.9 matches per topic) most waves take
// W = 8 (24 compare-exchanges instead of 80); k_assemble was bound by that
// VALU work (C2: 1.07 ms -> 0.91 ms with the network sized alone, 0.80 ms
// with loads and stores sized too).
template <int W>
__device__ __forceinline__ void assemble_tile(const uint32_t* __restrict__ stage, uint64_t tile, int lane,
                                              uint32_t cf, bool any_slow, uint64_t base, uint32_t pa,
                                              uint32_t tall, uint32_t* out, uint32_t* __restrict__ ids,
                                              uint64_t tile_base, const uint32_t* __restrict__ gmap) {
  uint32_t m[FAST_MC];
#pragma unroll
  for (int k = 0; k < FAST_MC; ++k)
    m[k] = (k < W && uint32_t(k) < cf) ? stage[stage_index(tile, k, lane)] : 0xFFFFFFFFu;
  if (W > 1) sort_row<W>(m);
  if (any_slow) {
#pragma unroll
    for (int k = 0; k < W; ++k)
      if (uint32_t(k) < cf) ids[base + k] = gmap ? gmap[m[k]] : m[k];  // shard index: global ids (ascending)
    return;
  }
#pragma unroll
  for (int k = 0; k < W; ++k)
    if (uint32_t(k) < cf) out[pa + k] = gmap ? gmap[m[k]] : m[k];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  uint32_t* const dst = ids + tile_base;
  for (uint32_t i = lane; i < tall; i += 64) dst[i] = out[i];
}

// One wave per 64-topic tile: row offsets from the wave's scan, each lane's
// row sorted in registers, then the tile's ids (one contiguous range of the
// output) written through LDS as coalesced 256-B rows.  A tile holding a
// slow-path row (its ids land later, k_copy_slow) stores lane by lane so
// that row's range is left alone.
// cap: the ids buffer's capacity; a tile whose rows would pass it writes no
// ids (the host, seeing a total past cap, assembles again into a larger buffer).
__global__ __launch_bounds__(256) void k_assemble(const uint32_t* __restrict__ cnt, uint64_t n,
                                                  const uint64_t* __restrict__ tile_off,
                                                  const uint32_t* __restrict__ stage,
                                                  uint64_t* __restrict__ row_off, uint32_t* __restrict__ ids,
                                                  const uint32_t* __restrict__ gmap, uint64_t cap) {
  __shared__ uint32_t s_out[4][64 * FAST_MC];
  const int lane = threadIdx.x & 63;
  uint32_t* const out = s_out[threadIdx.x >> 6];
  const uint64_t t = uint64_t(blockIdx.x) * 256u + threadIdx.x;
  const uint64_t tile = t >> 6;
  if (tile * 64 >= n) return;  // wave-uniform; no block barrier below
  const uint32_t c = t < n ? cnt[t] : 0;
  const bool slow = (c & OVF_BIT) != 0;
  const uint32_t call = c & CNT_MASK, cf = slow ? 0 : call;
  uint32_t tall;
  const uint32_t pa = wave_excl_scan(call, tall);
  const uint64_t base = tile_off[tile] + pa;
  if (t < n) row_off[t] = base;
  if (t == n - 1) row_off[n] = base + call;
  const bool any_slow = __ballot(slow) != 0;
  const uint64_t tb0 = tile_off[tile];
  if (tb0 + tall > cap) return;  // wave-uniform
#define GM_ASM(W) assemble_tile<W>(stage, tile, lane, cf, any_slow, base, pa, tall, out, ids, tb0, gmap)
  if (__ballot(cf > 8))
    GM_ASM(FAST_MC);
  else if (__ballot(cf > 4))
    GM_ASM(8);
  else if (__ballot(cf > 2))
    GM_ASM(4);
  else if (__ballot(cf > 1))
    GM_ASM(2);
  else
    GM_ASM(1);
#undef GM_ASM
}

// One lane's row of k_assemble_c once the wave's longest row fits W slots:
// W gathers (LDS, or the listed row), the W-wide network, W writes back (or,
// beside a slow row, straight to the output).
template <int W>
__device__ __forceinline__ void assemble_rows_c(uint32_t* out, const uint32_t* __restrict__ lrow, bool listed,
                                                uint32_t lpa, uint32_t cf, bool any_slow, uint32_t* __restrict__ ids,
                                                uint64_t base, const uint32_t* __restrict__ gmap) {
  uint32_t m[FAST_MC];
#pragma unroll
  for (int k = 0; k < FAST_MC; ++k)
    m[k] = (k < W && uint32_t(k) < cf) ? (listed ? lrow[k] : out[lpa + k]) : 0xFFFFFFFFu;
  if (W > 1) sort_row<W>(m);
  if (any_slow) {  // leave the slow rows' ranges alone: lane by lane
#pragma unroll
    for (int k = 0; k < W; ++k)
      if (uint32_t(k) < cf) ids[base + k] = gmap ? gmap[m[k]] : m[k];
    return;
  }
  wave_lds_sync();
#pragma unroll
  for (int k = 0; k < W; ++k)
    if (uint32_t(k) < cf) out[lpa + k] = gmap ? gmap[m[k]] : m[k];  // (no slow row: lpa == pa)
}

// Compact staging (k_match_fused<CMP>): the tile's list holds its matches in
// emission order as (filter id | lane | rank in its row), tlen[tile] of them, the
// partial rows of topics that went on to the listed pass included.  Each
// wave places its main-pass rows' entries in LDS at the row's offset (one
// LDS counter per row), sorts each row in registers, and writes the tile's
// ids as one coalesced range; a listed row comes from its own lstage row.
// The list is ~11.5 B per C2 topic against the ~20 B of [slot][lane] rows
// k_assemble reads.
struct AsmCLoads {  // one tile's loads of k_assemble_c, issued before any is used
  static constexpr int PRE = 4;
  uint32_t pre[PRE];  // the list's first 256 entries (a C2 tile holds ~184)
  uint32_t len, c;
  uint64_t tb0;
};
// blk_sums: blk holds the split scan's block SUMS (a scan of at most 64
// blocks: the prefix is summed here by the wave, one scan launch fewer), not
// their offsets.
__device__ __forceinline__ uint64_t blk_prefix(const uint64_t* __restrict__ sums, uint32_t j, int lane) {
  uint64_t v = uint32_t(lane) < j ? sums[lane] : 0ull;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ void asm_c_load(AsmCLoads& L, uint64_t tile, uint64_t n, int lane,
                                           const uint8_t* __restrict__ cnt8, const uint64_t* __restrict__ tile_off,
                                           const uint32_t* __restrict__ stage, const uint32_t* __restrict__ tlen,
                                           const uint64_t* __restrict__ blk, bool blk_sums = false) {
  const uint32_t* const lst = stage + tile * (64ull * FAST_MC);
#pragma unroll
  for (int q = 0; q < AsmCLoads::PRE; ++q) L.pre[q] = ld_s<true>(lst + q * 64 + lane);
  L.len = tlen[tile];
  const uint64_t t = tile * 64 + lane;
  L.c = t < n ? ld_s<true>(cnt8 + t) : 0u;  // 0xFF: the row's cnt word (asm_c_tile)
  L.tb0 = tile_off[tile] + (!blk ? 0ull : blk_sums ? blk_prefix(blk, uint32_t(tile / SCAN_B), lane)
                                                   : blk[tile / SCAN_B]);  // blk: a split scan's block offsets
}

// One tile of k_assemble_c from its loads (out, s_pa: the wave's LDS).
__device__ __forceinline__ void asm_c_tile(const AsmCLoads& L, uint64_t tile, uint64_t n, int lane, uint32_t* out,
                                           uint32_t* s_pa, const uint32_t* __restrict__ cnt,
                                           const uint32_t* __restrict__ stage,
                                           const uint32_t* __restrict__ lstage, const uint32_t* __restrict__ lcnt,
                                           uint64_t* __restrict__ row_off, uint32_t* __restrict__ ids,
                                           const uint32_t* __restrict__ gmap, uint64_t cap) {
  const uint64_t t = tile * 64 + lane;
  const uint32_t c = L.c == 0xFFu ? cnt[t] : L.c;  // a listed or slow row: its cnt word
  const bool slow = (c & OVF_BIT) != 0, listed = !slow && (c & LIST_BIT);
  const uint32_t call = slow ? (c & CNT_MASK) : listed ? lcnt[c & ~LIST_BIT] : c;
  const uint32_t cf = slow ? 0 : call;  // rows placed here (a slow row's ids land later, k_copy_slow)
  uint32_t tall, lall;
  const uint32_t pa = wave_excl_scan(call, tall);
  const uint32_t lpa = wave_excl_scan(cf, lall);  // the row's place in LDS (slow rows take none)
  const uint64_t base = L.tb0 + pa;
  if (t < n) row_off[t] = base;
  if (t == n - 1) row_off[n] = base + call;
  if (L.tb0 + tall > cap) return;  // wave-uniform
  const bool any_slow = __ballot(slow) != 0;
  // main-pass rows: scatter the list into LDS at each row's offset + the entry's rank
  s_pa[lane] = (slow || listed || t >= n) ? NONE : lpa;
  wave_lds_sync();
#define GM_PLACE(e)                                                               \
  do {                                                                            \
    const uint32_t rp = s_pa[((e) >> CMP_SHIFT) & 63u];                           \
    if (rp != NONE) out[rp + ((e) >> CMP_RANK)] = (e) & ((1u << CMP_SHIFT) - 1u); \
  } while (0)
#pragma unroll
  for (int q = 0; q < AsmCLoads::PRE; ++q)
    if (uint32_t(q * 64 + lane) < L.len) GM_PLACE(L.pre[q]);
  const uint32_t* const lst = stage + tile * (64ull * FAST_MC);
  for (uint32_t i = AsmCLoads::PRE * 64 + lane; i < L.len; i += 64) {
    const uint32_t e = ld_s<true>(lst + i);
    GM_PLACE(e);
  }
#undef GM_PLACE
  wave_lds_sync();
  // each row sorted in registers (W = the wave's longest row, a power of two)
  const uint32_t* const lrow = listed ? lstage + uint64_t(c & ~LIST_BIT) * FAST_MC : nullptr;
#define GM_ASMC(W) assemble_rows_c<W>(out, lrow, listed, lpa, cf, any_slow, ids, base, gmap)
  if (__ballot(cf > 8)) GM_ASMC(FAST_MC);
  else if (__ballot(cf > 4)) GM_ASMC(8);
  else if (__ballot(cf > 2)) GM_ASMC(4);
  else if (__ballot(cf > 1)) GM_ASMC(2);
  else GM_ASMC(1);
#undef GM_ASMC
  if (any_slow) return;
  wave_lds_sync();
  uint32_t* const dst = ids + L.tb0;
  for (uint32_t i = lane; i < tall; i += 64) st_s<true>(dst + i, out[i]);
}

// ASM_TPW tiles per wave, every tile's loads issued together (one round trip
// for all).  2 was slower at C2: 0.83-0.84 ms against 0.79-0.80 for 1, at 6
// waves/SIMD (74 VGPRs) or at 8 with spills.
constexpr int ASM_TPW = 1;
__global__ __launch_bounds__(256) void k_assemble_c(const uint8_t* __restrict__ cnt8, const uint32_t* __restrict__ cnt,
                                                    uint64_t n,
                                                    const uint64_t* __restrict__ tile_off,
                                                    const uint32_t* __restrict__ stage,
                                                    const uint32_t* __restrict__ tlen,
                                                    const uint32_t* __restrict__ lstage,
                                                    const uint32_t* __restrict__ lcnt,
                                                    uint64_t* __restrict__ row_off, uint32_t* __restrict__ ids,
                                                    const uint32_t* __restrict__ gmap, uint64_t cap,
                                                    const uint64_t* __restrict__ blk,
                                                    const uint32_t* __restrict__ rb_total,
                                                    const uint32_t* __restrict__ rb_ctr, uint32_t* __restrict__ rb_dst,
                                                    uint32_t* __restrict__ zero16, uint32_t blk_sums,
                                                    uint64_t* __restrict__ total_out) {
  __shared__ uint32_t s_out[4][64 * FAST_MC];
  __shared__ uint32_t s_pa[4][64];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // rb_dst (the call's pinned host words): the 40-B read-back -- the match
  // total and the pass counters, final before this kernel -- written by the
  // first wave's lanes (vector stores), so the call needs no copy packet; the
  // host reads it once this launch's stop event has completed
  // blk_sums (= the number of scan blocks): no launch wrote the grand total;
  // the first wave sums the blocks and writes it behind the tile offsets
  uint64_t gtot = 0;
  if (blk_sums && blockIdx.x == 0 && wv == 0) {
    gtot = blk_prefix(blk, blk_sums, lane);
    if (lane == 0) *total_out = gtot;
  }
  if (rb_dst && blockIdx.x == 0 && wv == 0) {
    if (lane < 10)
      rb_dst[lane] = lane < 2 ? (blk_sums ? uint32_t(gtot >> (32 * lane)) : rb_total[lane]) : rb_ctr[lane - 2];
    __threadfence_system();  // (out to host memory before the kernel's end is signalled)
  }
  // zero16: the next call's pass-counter block (the context's ring), zeroed
  // for it here so that call needs no zeroing launch
  if (zero16 && blockIdx.x == 0 && wv == 1 && lane < 16) zero16[lane] = 0u;
  const uint64_t n_tiles = (n + 63) / 64;
  const uint64_t tile0 = (uint64_t(blockIdx.x) * 4 + wv) * ASM_TPW;
  if (tile0 >= n_tiles) return;  // wave-uniform; no block barrier below
  AsmCLoads L[ASM_TPW];
#pragma unroll
  for (int k = 0; k < ASM_TPW; ++k)
    if (tile0 + k < n_tiles) asm_c_load(L[k], tile0 + k, n, lane, cnt8, tile_off, stage, tlen, blk, blk_sums != 0);
#pragma unroll
  for (int k = 0; k < ASM_TPW; ++k) {
    if (tile0 + k >= n_tiles) break;
    if (k) wave_lds_sync();  // the previous tile is done with the wave's LDS
    asm_c_tile(L[k], tile0 + k, n, lane, s_out[wv], s_pa[wv], cnt, stage, lstage, lcnt, row_off, ids, gmap, cap);
  }
}

// ---------------------------------------------------------------------------
// slow path
// ---------------------------------------------------------------------------
template <bool EXACT>
__global__ __launch_bounds__(256) void k_slow_walk(const uint8_t* __restrict__ tb,
                                                   const uint64_t* __restrict__ toff, IndexView ix,
                                                   const uint32_t* __restrict__ list, uint64_t k0, uint64_t kn,
                                                   uint32_t* __restrict__ fr_all, uint64_t fr_cap,
                                                   uint32_t* __restrict__ bm_all, uint64_t bm_words,
                                                   uint32_t* __restrict__ cnt, uint64_t* __restrict__ slow_cnt,
                                                   uint64_t* __restrict__ tsum) {
  const uint64_t k = k0 + blockIdx.x;
  if (k >= kn) return;
  const uint32_t t = list[k];
  uint32_t* fr0 = fr_all + uint64_t(blockIdx.x) * 2 * fr_cap;
  uint32_t* fr1 = fr0 + fr_cap;
  uint32_t* bm = bm_all + uint64_t(blockIdx.x) * bm_words;
  __shared__ uint32_t s_cur_n, s_nxt_n, s_wid, s_flags;  // flags: 1 last, 2 wild, 4 dollar
  __shared__ uint64_t s_pos;
  __shared__ uint32_t s_level;
  __shared__ uint32_t s_red[256];
  const int tid = threadIdx.x;
  for (uint64_t i = tid; i < bm_words; i += 256) bm[i] = 0;
  const uint64_t end = toff[t + 1];
  if (tid == 0) {
    s_pos = toff[t];
    s_cur_n = 1;
    s_nxt_n = 0;
    s_level = 0;
    s_flags = 0;
    fr0[0] = 0;
  }
  __syncthreads();
  uint32_t* cur = fr0;
  uint32_t* nxt = fr1;
  for (;;) {
    if (tid == 0) {
      ByteReader rd{tb, ~0ull, 0};
      uint64_t pos = s_pos;
      const WordTok w = next_word(rd, pos, end);
      uint32_t fl = s_flags & 4u;
      if (pos >= end) fl |= 1u;
      if (w.len == 1 && (w.b0 == '+' || w.b0 == '#')) fl |= 2u;
      if (s_level == 0 && w.len > 0 && w.b0 == '$') fl |= 4u;
      s_flags = fl;
      s_wid = (fl & 2u) ? NONE : dict_resolve(ix, w, dict_first(ix, w), tb);
      s_pos = pos + 1;
    }
    __syncthreads();
    const uint32_t fl = s_flags;
    if (fl & 2u) break;
    const uint32_t wid = s_wid, cn = s_cur_n, lvl = s_level;
    const bool rootskip = (fl & 4u) && lvl == 0;
    for (uint32_t i = tid; i < cn; i += 256) {
      const uint32_t nd = cur[i] & REF_MASK;
      const Node node = ix.nodes[nd];
      if (!rootskip) {
        if (node.hash_filter != NONE) atomicOr(&bm[node.hash_filter >> 5], 1u << (node.hash_filter & 31));
        if (node.plus_child != NONE) nxt[atomicAdd(&s_nxt_n, 1u)] = node.plus_child;
      }
      if (wid != NONE && (node.flags & NF_HAS_EXACT)) {
        const uint32_t c = edge_lookup(ix, lvl, nd, wid);
        if (c != NONE) nxt[atomicAdd(&s_nxt_n, 1u)] = c;
      }
    }
    __syncthreads();
    if (tid == 0) {
      s_cur_n = s_nxt_n;
      s_nxt_n = 0;
      if (!(fl & 1u)) s_level = s_level + 1;
    }
    uint32_t* tmp = cur;
    cur = nxt;
    nxt = tmp;
    __syncthreads();
    if (fl & 1u) break;
  }
  const uint32_t fl = s_flags;
  if (fl & 2u) {  // wildcard topic: [] (trie) or the literal filter (routes)
    __syncthreads();
    for (uint64_t i = tid; i < bm_words; i += 256) atomicAnd(&bm[i], 0u);
    __syncthreads();
    if (EXACT && tid == 0) {
      const uint32_t f = literal_lookup(ix, tb, toff[t], end);
      if (f != NONE) atomicOr(&bm[f >> 5], 1u << (f & 31));
    }
  } else {
    const uint32_t cn = s_cur_n;
    const bool single = s_level == 0 && (fl & 4u);
    for (uint32_t i = tid; i < cn; i += 256) {
      const Node node = ix.nodes[cur[i] & REF_MASK];
      if (node.hash_filter != NONE) atomicOr(&bm[node.hash_filter >> 5], 1u << (node.hash_filter & 31));
      if (node.end_filter != NONE && (EXACT || (node.flags & NF_END_WILD) || single))
        atomicOr(&bm[node.end_filter >> 5], 1u << (node.end_filter & 31));
    }
  }
  __syncthreads();
  uint32_t c = 0;
  for (uint64_t i = tid; i < bm_words; i += 256)
    c += __popc(__hip_atomic_load(&bm[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  s_red[tid] = c;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) s_red[tid] += s_red[tid + s];
    __syncthreads();
  }
  if (tid == 0) {
    slow_cnt[k] = s_red[0];
    cnt[t] = OVF_BIT | s_red[0];
    atomicAdd(reinterpret_cast<unsigned long long*>(tsum + (t >> 6)), (unsigned long long)s_red[0]);
  }
}

__global__ __launch_bounds__(256) void k_slow_emit(uint64_t k0, uint64_t kn, const uint32_t* __restrict__ bm_all,
                                                   uint64_t bm_words, const uint64_t* __restrict__ slow_off,
                                                   uint32_t* __restrict__ slow_ids) {
  const uint64_t k = k0 + blockIdx.x;
  if (k >= kn) return;
  const uint32_t* bm = bm_all + uint64_t(blockIdx.x) * bm_words;
  __shared__ uint32_t s_w[4];
  uint64_t out = slow_off[k];
  for (uint64_t b = 0; b < bm_words; b += 256) {
    const uint64_t i = b + threadIdx.x;
    uint32_t w = i < bm_words ? bm[i] : 0;
    uint32_t tot;
    const uint32_t pre = wave_excl_scan(__popc(w), tot);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_w[wv] = tot;
    __syncthreads();
    uint32_t wpre = 0, all = 0;
    for (int q = 0; q < 4; ++q) {
      if (q < wv) wpre += s_w[q];
      all += s_w[q];
    }
    uint64_t o = out + wpre + pre;
    while (w) {
      const int bit = __ffs(w) - 1;
      slow_ids[o++] = uint32_t(i * 32 + bit);
      w &= w - 1;
    }
    out += all;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_copy_slow(const uint32_t* __restrict__ list, uint64_t kn,
                                                   const uint64_t* __restrict__ row_off,
                                                   const uint64_t* __restrict__ slow_off,
                                                   const uint32_t* __restrict__ slow_ids, uint32_t* __restrict__ ids,
                                                   const uint32_t* __restrict__ gmap) {
  const uint64_t k = blockIdx.x;
  if (k >= kn) return;
  const uint32_t t = list[k];
  const uint64_t dst = row_off[t], src = slow_off[k], len = slow_off[k + 1] - src;
  for (uint64_t i = threadIdx.x; i < len; i += 256) {
    const uint32_t f = slow_ids[src + i];
    ids[dst + i] = gmap ? gmap[f] : f;
  }
}

// ---------------------------------------------------------------------------
// host orchestration
// ---------------------------------------------------------------------------
int finish_csr(emqx_gm_ctx* ctx, uint64_t n, uint64_t nnz, PoolBuf& row_off, PoolBuf& ids, bool device_out,
               emqx_gm_csr* out) {
  out->n_rows = n;
  out->nnz = nnz;
  out->priv = ctx;  // the owning context (emqx_gm_csr_free checks it)
  if (device_out) {
    out->row_off = static_cast<uint64_t*>(row_off.release_ownership());
    out->ids = static_cast<uint32_t*>(ids.release_ownership());
    out->on_device = 1;
    return 0;
  }
  uint64_t* h_off = static_cast<uint64_t*>(ctx->hpool->alloc((n + 1) * 8));
  uint32_t* h_ids = static_cast<uint32_t*>(ctx->hpool->alloc(nnz * 4 + 4));
  if (!h_off || !h_ids) {
    ctx->hpool->release(h_off);
    ctx->hpool->release(h_ids);
    return set_err(ctx, EMQX_GM_ENOMEM, "csr: host allocation");
  }
  GM_HIP(ctx, hipMemcpyAsync(h_off, row_off.p, (n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (nnz) GM_HIP(ctx, hipMemcpyAsync(h_ids, ids.p, nnz * 4, hipMemcpyDeviceToHost, ctx->stream));
  GM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  out->row_off = h_off;
  out->ids = h_ids;
  out->on_device = 0;
  return 0;
}

float ev_ms(hipEvent_t a, hipEvent_t b) {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, a, b) != hipSuccess) {
    (void)hipGetLastError();  // (an event not recorded for this call: no timing, and no sticky error)
    return 0.f;
  }
  return ms;
}

namespace {

constexpr int LISTED_FC = 16;  // frontier capacity of the listed pass

// Non-temporal stream accesses.  GM_NT (A/B knob, read per call): the topic
// text, staging and counts as nt loads / stores (default; C2: 10.45 -> 10.24 ms),
// 0 = plain.
bool nt_streams() {
  const char* e = knob("GM_NT");
  return !e || atoi(e) != 0;
}

// Compact staging of the fused main pass (k_match_fused<CMP> + k_assemble_c).
// GM_STAGE_COMPACT (A/B knob, read per call so tests cover both; default on):
// used when the index's filter ids fit CMP_SHIFT bits.
// The assembly stream (MatchCall::submit) for device-buffer calls of at least
// this many topics; GM_ASM_STREAM (A/B knob, read per call): 0 = never, N =
// from N topics.
// (Off by default: at C2 the overlapped assembly slowed the walk by what it
// hid, 9.16 vs 9.16 ms per step, profiles/r04_ab/asm_stream_c2.txt.)
// GM_SCAN_SUMS (A/B knob, read per call; default on): a split tile scan of at
// most 64 blocks (calls up to ~4M topics: C1) ends after its first launch and
// k_assemble_c sums the block prefixes itself.
bool sums_mode() {
  const char* e = knob("GM_SCAN_SUMS");
  return !e || atoi(e) != 0;
}

uint64_t asm_stream_min() {
  const char* e = knob("GM_ASM_STREAM");
  return e ? strtoull(e, nullptr, 10) : 0;
}

bool stage_compact() {
  const char* e = knob("GM_STAGE_COMPACT");
  return !e || atoi(e) != 0;
}
struct CmpBufs {
  uint8_t* cnt8;     // per topic: its row length, 0xFF = see cnt (listed / slow rows)
  uint32_t* tlen;    // per tile: entries in its list
  uint32_t* lstage;  // listed rows, FAST_MC ids each
  uint32_t* lcnt;    // listed row lengths
  uint64_t lcap;     // listed rows available
};
void launch_assemble(hipStream_t st, uint64_t nblk, const CmpBufs* cb, const uint32_t* cnt, uint64_t n,
                     const uint64_t* toff, const uint32_t* stage, uint64_t* row_off, uint32_t* ids,
                     const uint32_t* gmap, uint64_t cap, const uint64_t* blk = nullptr, uint32_t* rb_dst = nullptr,
                     const uint32_t* rb_ctr = nullptr, hipEvent_t done = nullptr, uint32_t* zero16 = nullptr,
                     uint32_t blk_sums = 0) {
  // blk (compact staging only): toff is a split scan's block-local part, blk its block offsets
  // (blk_sums != 0: blk holds that many block SUMS, and the kernel writes the grand total at toff[n_tiles])
  // rb_dst (compact staging only): the read-back words (the total behind toff, the
  // counters at rb_ctr) written by the kernel, `done` its stop event
  // zero16 (compact staging only): a 64-B counter block the kernel zeroes
  const uint32_t* rb_total = reinterpret_cast<const uint32_t*>(toff + (n + 63) / 64);
  if (cb)
    hipExtLaunchKernelGGL(k_assemble_c, dim3((nblk + ASM_TPW - 1) / ASM_TPW), dim3(256), 0, st, nullptr, done, 0,
                          cb->cnt8, cnt, n, toff, stage, cb->tlen, cb->lstage, cb->lcnt, row_off, ids, gmap, cap, blk,
                          rb_total, rb_ctr, rb_dst, zero16, blk_sums,
                          const_cast<uint64_t*>(toff) + (n + 63) / 64);
  else
    hipLaunchKernelGGL(k_assemble, dim3(nblk), dim3(256), 0, st, cnt, n, toff, stage, row_off, ids, gmap, cap);
}

// The listed pass over the main pass's overflow queue (list1, its count n1 on the device)
template <bool EXACT>
void launch_listed(hipStream_t st, const IndexView& v, const uint8_t* tb, const uint64_t* to, uint64_t n, uint32_t* cnt,
                   uint32_t* stage, uint32_t* list1, uint32_t* n1, uint32_t* list2, uint32_t* n2,
                   unsigned long long* probe_ctr, unsigned long long* wild_ctr, uint64_t* tsum, const CmpBufs* cb) {
  const uint64_t nblk = (n + 255) / 256;
  const uint64_t lblk = std::min<uint64_t>(nblk, 512);
  if (cb)
    hipLaunchKernelGGL((k_match_lds<EXACT, LISTED_FC, true>), dim3(lblk), dim3(256), 0, st, tb, to, n, v, cnt, stage,
                       list1, n1, list2, n2, probe_ctr, wild_ctr, tsum, cb->lstage, cb->lcnt, cb->lcap);
  else
    hipLaunchKernelGGL((k_match_lds<EXACT, LISTED_FC, false>), dim3(lblk), dim3(256), 0, st, tb, to, n, v, cnt, stage,
                       list1, n1, list2, n2, probe_ctr, wild_ctr, tsum, nullptr, nullptr, 0);
}

// f(std::true_type{}) or f(std::false_type{}): a run-time flag as a template argument
template <class F>
void with_flag(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

// Main pass, then the listed pass over its overflow queue (count read on the
// device).  before_main / after_main (both null for an untimed call,
// EMQX_GM_NO_TIMING) take the main pass's own start and stop: the roofline
// times the main pass alone, the same kernel rocprofv3 reports.
template <bool EXACT>
void launch_match(hipStream_t st, const IndexView& v, const uint8_t* tb, const uint64_t* to, uint64_t n,
                  uint32_t* cnt, uint32_t* stage, uint32_t* list1, uint32_t* n1, uint32_t* list2, uint32_t* n2,
                  unsigned long long* probe_ctr, unsigned long long* wild_ctr, unsigned long long* probe_tile,
                  uint64_t* tsum, hipEvent_t before_main, hipEvent_t after_main, const CmpBufs* cb,
                  bool* listed_deferred) {
  const uint64_t nblk = (n + 255) / 256;
  *listed_deferred = false;
#ifdef GM_PHASE_STATS
  uint32_t* phase_rec = nullptr;
  if (n && hipStreamSynchronize(st) == hipSuccess && hipMalloc(&phase_rec, (n + 63) / 64 * 128) == hipSuccess) {
    (void)hipMemset(phase_rec, 0, (n + 63) / 64 * 128);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_phase_rec), &phase_rec, sizeof phase_rec);
  }
#endif
  const bool nt = nt_streams();
  const char* pe = knob("GM_FUSED_PRIO");  // A/B knob (read per call): 0 = every phase at priority 0
  const bool prio = !pe || atoi(pe) != 0;
  const bool flat = view_flat(v);  // a table too large for 32-bit byte offsets: the flat instantiations
  // The kernel's own start / stop timestamps (hipExtLaunchKernel) instead of
  // two event records around it: each record is a barrier packet that costs
  // the stream ~5.5 us of idle GPU (C1 per-call trace, profiles/r03_c1_trace.txt)
  auto launch = [&](auto kernel) {
    hipExtLaunchKernelGGL(kernel, dim3(nblk), dim3(256), 0, st, before_main, after_main, 0, tb, to, n, v, cnt, stage, list1,
                          n1, probe_tile, wild_ctr, tsum, cb ? cb->tlen : nullptr, cb ? cb->cnt8 : nullptr);
  };
  // k_match_fused<EXACT, NT, TOKPRIO, CMP, AB, FLAT>.  The default instantiation
  // (AB false): default knobs, a view that asks for no A/B form and
  // buffer-sized tables.  Everything else runs the general one (AB true).
  const bool plain = nt && prio && !flat && (v.flags & IX_D0) && !(v.flags & IX_STAGE_SC1) && !v.l1_bypass;
  with_flag(cb != nullptr, [&](auto cmp) {
    constexpr bool CMP = decltype(cmp)::value;
    if (plain) {
      launch(k_match_fused<EXACT, true, true, CMP, false, false>);
      return;
    }
    with_flag(nt, [&](auto nt_) {
      with_flag(prio, [&](auto prio_) {
        with_flag(flat, [&](auto flat_) {
          launch(k_match_fused<EXACT, decltype(nt_)::value, decltype(prio_)::value, CMP, true, decltype(flat_)::value>);
        });
      });
    });
  });
#ifdef GM_PROBE_STATS
  {
    unsigned long long h[8][8], z[8][8] = {};
    if (hipStreamSynchronize(st) == hipSuccess && hipMemcpyFromSymbol(h, HIP_SYMBOL(g_pstats), sizeof h) == hipSuccess) {
      (void)hipMemcpyToSymbol(HIP_SYMBOL(g_pstats), z, sizeof z);
      for (int l = 0; l < 8; ++l)
        if (h[l][0])
          fprintf(stderr, "[probe_stats] level %d entries %llu cand %llu sig %llu efilt %llu found %llu plus_slot %llu "
                  "plus_found %llu plus_inline %llu\n", l, h[l][0], h[l][1], h[l][2], h[l][3], h[l][4], h[l][5], h[l][6],
                  h[l][7]);
    }
  }
#endif
#ifdef GM_PHASE_STATS
  if (phase_rec) {
    const uint64_t nt = (n + 63) / 64;
    std::vector<uint32_t> h(nt * 32);
    uint32_t* null_rec = nullptr;
    if (hipStreamSynchronize(st) == hipSuccess &&
        hipMemcpy(h.data(), phase_rec, h.size() * 4, hipMemcpyDeviceToHost) == hipSuccess) {
      double sum[32] = {0}, rounds[8] = {0};
      for (uint64_t i = 0; i < nt; ++i) {
        const uint32_t* r = &h[i * 32];
        for (int k = 0; k < 32; ++k) sum[k] += r[k];
        for (int l = 0; l < 8; ++l) rounds[l] += (r[l < 4 ? 11 : 12] >> (8 * (l & 3))) & 0xFFu;
      }
      const double w = double(nt);
      fprintf(stderr, "[phase_stats] waves %llu; ticks/wave: stage %.0f tok %.0f", (unsigned long long)nt, sum[0] / w,
              sum[1] / w);
      for (int l = 0; l < 8; ++l)
        if (rounds[l] > 0)
          fprintf(stderr, " L%d %.0f (%.2f rounds: to data %.0f, rest %.0f)", l, sum[2 + l] / w, rounds[l] / w,
                  sum[16 + l] / w, sum[24 + l] / w);
      fprintf(stderr, " epi %.0f; chain-tail rounds/wave %.2f; walk %.0f memtime / %.0f memrealtime ticks = %.1f MHz\n",
              sum[10] / w, sum[13] / w, sum[14] / w, sum[15] / w, sum[15] > 0 ? sum[14] / sum[15] * 100.0 : 0.0);
    }
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_phase_rec), &null_rec, sizeof null_rec);
    (void)hipFree(phase_rec);
  }
#endif
  // (probe_tile is summed into the probe counter by the tile scan, MatchCall::submit)
  // With compact staging the listed pass is left to the host's read-back
  // (MatchCall::finish): it launches it only when the main pass queued rows,
  // instead of an (almost always idle) launch per call.
  // GM_LISTED_DEFER=0: launch it here (A/B knob).
  if (cb) {
    const char* le = knob("GM_LISTED_DEFER");
    if (!le || atoi(le) != 0) {
      *listed_deferred = true;
      return;
    }
  }
  launch_listed<EXACT>(st, v, tb, to, n, cnt, stage, list1, n1, list2, n2, probe_ctr, wild_ctr, tsum, cb);
}

}  // namespace

// One match call in two phases (emqx_gm_match = submit then finish at once;
// emqx_gm_match_submit / emqx_gm_match_wait split them, so the next batch's
// launches queue behind this one's before the host has read its total):
//   submit(): every kernel of the call, the speculative assembly and the
//     40-B read-back of the match total + pass counters into the call's own
//     pinned words, then an event -- no host wait;
//   finish(): waits on that event (without the context lock when it was
//     submitted alone), then either hands out the speculative rows or runs
//     the slow path / exact-size assembly and waits again.
// A call owns its workspaces (PoolBufs), events and pinned words until
// finish(), so several can be in flight on one context stream.
struct MatchCall {
  emqx_gm_ctx* ctx;
  const emqx_gm_index* idx = nullptr;
  uint64_t n = 0, n_tiles = 0, nblk = 0, cap_spec = 0;
  bool dev_io = false, exact = false, cmp = false, spec = false, split = false, submitted = false;
  uint32_t split_sums = 0;       // the split scan handed back block sums (k_assemble_c sums them)
  bool listed_deferred = false;  // the listed pass is left to finish() (launched only for queued rows)
  bool timed = true;             // the main pass's start / stop events (EMQX_GM_NO_TIMING: none)
  bool asm_overlap = false;      // scan + speculative assembly on ctx->stream_asm (wanted)
  bool on_asm = false;           // ... and queued there
  int ctr_slot = -1;             // the pass-counter block of the context's ring, or -1 (counters behind toff)
  const uint8_t* tb = nullptr;
  const uint64_t* to = nullptr;
  PoolBuf d_tb_own, d_to_own, row_off, cnt, stage, list1, list2, tsum, toff, probe_tile;
  PoolBuf c_tlen, c_lstage, c_lcnt, c_cnt8, scan_blk, ids;
  CmpBufs cmpb{};
  uint64_t* toff_p = nullptr;
  uint8_t* ctrs_p = nullptr;
  uint64_t* pin = nullptr;  // [0] match total, [1..4] the pass counters
  hipEvent_t ev[3] = {};    // start, after the main pass, done
  emqx_gm_match_stats st_copy{};  // the stats finish() wrote for this call
  explicit MatchCall(emqx_gm_ctx* c) : ctx(c) {}
  MatchCall(const MatchCall&) = delete;
  MatchCall& operator=(const MatchCall&) = delete;
  ~MatchCall() {
    // (caller holds ctx->mu: the pools are not thread safe)
    if (submitted) {  // an abandoned call: its kernels may still use the buffers
      hipStreamSynchronize(ctx->stream);
      if (on_asm) hipStreamSynchronize(ctx->stream_asm);
    }
    for (hipEvent_t& e : ev)
      if (e) ctx->ev_free.push_back(e);
    if (pin) ctx->pin_free.push_back(pin);
    if (ctr_slot >= 0) ctx->ctr_state[ctr_slot] = 2;  // dirty: zeroed before its next use
    if (idx) const_cast<emqx_gm_index*>(idx)->refs.fetch_sub(1) == 1 ? free_index(const_cast<emqx_gm_index*>(idx))
                                                                     : void();
  }
  // the 40-B read-back (match total + pass counters) into the pinned words
  int readback(hipStream_t st) {
    if (ctr_slot < 0) {
      GM_HIP(ctx, hipMemcpyAsync(pin, toff_p + n_tiles, 40, hipMemcpyDeviceToHost, st));
    } else {
      GM_HIP(ctx, hipMemcpyAsync(pin, toff_p + n_tiles, 8, hipMemcpyDeviceToHost, st));
      GM_HIP(ctx, hipMemcpyAsync(pin + 1, ctrs_p, 32, hipMemcpyDeviceToHost, st));
    }
    return 0;
  }
  int take_event(hipEvent_t* e) {
    if (!ctx->ev_free.empty()) {
      *e = ctx->ev_free.back();
      ctx->ev_free.pop_back();
      return 0;
    }
    GM_HIP(ctx, hipEventCreate(e));
    return 0;
  }
  int submit(const emqx_gm_index* index, const uint8_t* tb_in, const uint64_t* to_in, uint64_t n_topics,
             uint32_t flags, MatchTail* tail);
  int finish(emqx_gm_csr* out, MatchTail* tail, bool locked);
};

int MatchCall::submit(const emqx_gm_index* index, const uint8_t* tb_in, const uint64_t* to_in, uint64_t n_topics,
                      uint32_t flags, MatchTail* tail) {
  dev_io = flags & EMQX_GM_DEVICE_IO;
  exact = flags & EMQX_GM_WITH_EXACT;
  timed = !(flags & EMQX_GM_NO_TIMING);
  n = n_topics;
  asm_overlap = dev_io && !tail && asm_stream_min() && n >= asm_stream_min();
  const_cast<emqx_gm_index*>(index)->refs.fetch_add(1);  // the snapshot stays alive until finish (RCU)
  idx = index;
  hipStream_t st = ctx->stream;
  for (hipEvent_t& e : ev)
    if (int rc = take_event(&e)) return rc;
  if (!ctx->pin_free.empty()) {
    pin = static_cast<uint64_t*>(ctx->pin_free.back());
    ctx->pin_free.pop_back();
  } else {
    void* p = nullptr;
    if (hipHostMalloc(&p, 64, hipHostMallocDefault) != hipSuccess)
      return set_err(ctx, EMQX_GM_ENOMEM, "match: pinned read-back words");
    ctx->pin_all.push_back(p);
    pin = static_cast<uint64_t*>(p);
  }

  // ---- inputs on the device
  tb = tb_in;
  to = to_in;
  if (!dev_io) {
    const uint64_t bytes = n ? to_in[n] : 0;
    for (uint64_t i = 0; i < n; ++i)
      if (to_in[i + 1] < to_in[i]) return set_err(ctx, EMQX_GM_EINVAL, "match: topic offsets not monotone");
    d_tb_own = PoolBuf(ctx->pool, bytes + 64);
    d_to_own = PoolBuf(ctx->pool, (n + 1) * 8);
    if (!d_tb_own.p || !d_to_own.p) return set_err(ctx, EMQX_GM_ENOMEM, "match: input workspace");
    submitted = true;
    if (bytes) GM_HIP(ctx, hipMemcpyAsync(d_tb_own.p, tb_in, bytes, hipMemcpyHostToDevice, st));
    GM_HIP(ctx, hipMemsetAsync(static_cast<uint8_t*>(d_tb_own.p) + bytes, 0, 64, st));
    GM_HIP(ctx, hipMemcpyAsync(d_to_own.p, to_in, (n + 1) * 8, hipMemcpyHostToDevice, st));
    tb = d_tb_own.as<uint8_t>();
    to = d_to_own.as<uint64_t>();
  }

  row_off = PoolBuf(ctx->pool, (n + 1) * 8);
  if (!row_off.p) return set_err(ctx, EMQX_GM_ENOMEM, "match: row_off");
  submitted = true;
  if (n == 0) {
    GM_HIP(ctx, hipMemsetAsync(row_off.p, 0, 8, st));
    ids = PoolBuf(ctx->pool, 16);
    GM_HIP(ctx, hipEventRecord(ev[0], st));
    GM_HIP(ctx, hipEventRecord(ev[1], st));
    GM_HIP(ctx, hipEventRecord(ev[2], st));
    pin[0] = pin[1] = pin[2] = pin[3] = pin[4] = 0;
    return 0;
  }

  n_tiles = (n + 63) / 64;
  nblk = (n + 255) / 256;
  cnt = PoolBuf(ctx->pool, n * 4 + 16);
  stage = PoolBuf(ctx->pool, n_tiles * 64ull * FAST_MC * 4);
  list1 = PoolBuf(ctx->pool, n * 4 + 16);
  list2 = PoolBuf(ctx->pool, n * 4 + 16);
  tsum = PoolBuf(ctx->pool, n_tiles * 8 + 8);
  // tile offsets [n_tiles + 1] and, right behind the total, the pass counters:
  // one read-back brings the match total and the counters together
  toff = PoolBuf(ctx->pool, (n_tiles + 1) * 8 + 128);
  if (!cnt.p || !stage.p || !list1.p || !list2.p || !tsum.p || !toff.p)
    return set_err(ctx, EMQX_GM_ENOMEM, "match: workspace");
  // the counters start 64-B aligned, so zeroing them is one fill launch (an
  // unaligned 64-B memset is split into three)
  const uintptr_t ctrs_a = (reinterpret_cast<uintptr_t>(toff.p) + (n_tiles + 1) * 8 + 63) & ~uintptr_t(63);
  ctrs_p = reinterpret_cast<uint8_t*>(ctrs_a);
  toff_p = reinterpret_cast<uint64_t*>(ctrs_p) - (n_tiles + 1);
  // the pass counters: the next block of the context's ring when it is free
  // (zeroed by the previous call's assembly, or here if it is dirty), else the
  // 64-B block behind toff, zeroed here
  bool zero_ctrs = true;
  if (!ctx->ctr_ring) {
    void* r = nullptr;
    if (hipMalloc(&r, emqx_gm_ctx::CTR_RING * 64) == hipSuccess) {
      if (hipMemset(r, 0, emqx_gm_ctx::CTR_RING * 64) == hipSuccess) ctx->ctr_ring = r;
      else hipFree(r);
    }
  }
  if (ctx->ctr_ring && ctx->ctr_state[ctx->ctr_next] != 1) {
    ctr_slot = ctx->ctr_next;
    ctx->ctr_next = (ctx->ctr_next + 1) % emqx_gm_ctx::CTR_RING;
    zero_ctrs = ctx->ctr_state[ctr_slot] == 2;
    ctx->ctr_state[ctr_slot] = 1;
    ctrs_p = static_cast<uint8_t*>(ctx->ctr_ring) + 64 * ctr_slot;
  }
  probe_tile = PoolBuf(ctx->pool, n_tiles * 8 + 8);
  if (!probe_tile.p) return set_err(ctx, EMQX_GM_ENOMEM, "match: probe workspace");
  // counters: u32 n1 @0 (main-pass overflow), u32 n2 @4 (listed-pass
  // overflow), u64 probes @16, u64 wildcard topics @24
  uint32_t* n1 = reinterpret_cast<uint32_t*>(ctrs_p);
  uint32_t* n2 = n1 + 1;
  unsigned long long* probe_ctr = reinterpret_cast<unsigned long long*>(ctrs_p + 16);
  unsigned long long* wild_ctr = reinterpret_cast<unsigned long long*>(ctrs_p + 24);
  // (a one-wave kernel: a 64-B hipMemsetAsync costs 11-26 us of host time
  // before the main pass can be queued, a launch ~6)
  if (zero_ctrs) hipLaunchKernelGGL(k_zero16, dim3(1), dim3(64), 0, st, reinterpret_cast<uint32_t*>(ctrs_p));

  cmp = stage_compact() && uint64_t(idx->view.n_filters) < (1ull << CMP_SHIFT);
  if (cmp) {
    const char* le = knob("GM_LISTED_CAP");  // (tests: listed rows past it go to the slow path)
    cmpb.lcap = std::min<uint64_t>(n, le ? strtoull(le, nullptr, 10) : (1u << 20));
    c_tlen = PoolBuf(ctx->pool, n_tiles * 4 + 16);
    c_cnt8 = PoolBuf(ctx->pool, n + 64);
    c_lstage = PoolBuf(ctx->pool, cmpb.lcap * FAST_MC * 4 + 16);
    c_lcnt = PoolBuf(ctx->pool, cmpb.lcap * 4 + 16);
    if (!c_tlen.p || !c_lstage.p || !c_lcnt.p || !c_cnt8.p) return set_err(ctx, EMQX_GM_ENOMEM, "match: compact staging");
    cmpb.cnt8 = c_cnt8.as<uint8_t>();
    cmpb.tlen = c_tlen.as<uint32_t>();
    cmpb.lstage = c_lstage.as<uint32_t>();
    cmpb.lcnt = c_lcnt.as<uint32_t>();
  }
  // ev[0] / ev[1]: the main pass's start and end (also the call's start: total_device_ms);
  // an untimed call launches it without them
  hipEvent_t main_ev0 = ev[0], main_ev1 = ev[1];
  if (!timed) main_ev0 = main_ev1 = nullptr;
  // GM_D0=0 (A/B knob, read per call): level 0 probed like any other level
  IndexView vcall = idx->view;
  if (const char* de = knob("GM_D0"))
    if (!atoi(de)) vcall.flags &= ~IX_D0;
  if (const char* se = knob("GM_STAGE_SC1"))  // A/B knobs (read per call)
    if (atoi(se)) vcall.flags |= IX_STAGE_SC1;
  if (const char* be = knob("GM_L1_BYPASS")) vcall.l1_bypass = uint32_t(strtoul(be, nullptr, 0));
  if (const char* pe = knob("GM_HOT_POLICY")) vcall.hot_policy = uint32_t(strtoul(pe, nullptr, 0));
  if (knob("GM_HOT_FLAT")) vcall.flags |= IX_HOT_FLAT;  // (test knob, also read per call: the flat instantiation)
  if (exact)
    launch_match<true>(st, vcall, tb, to, n, cnt.as<uint32_t>(), stage.as<uint32_t>(), list1.as<uint32_t>(), n1,
                       list2.as<uint32_t>(), n2, probe_ctr, wild_ctr, probe_tile.as<unsigned long long>(),
                       tsum.as<uint64_t>(), main_ev0, main_ev1, cmp ? &cmpb : nullptr, &listed_deferred);
  else
    launch_match<false>(st, vcall, tb, to, n, cnt.as<uint32_t>(), stage.as<uint32_t>(), list1.as<uint32_t>(), n1,
                        list2.as<uint32_t>(), n2, probe_ctr, wild_ctr, probe_tile.as<unsigned long long>(),
                        tsum.as<uint64_t>(), main_ev0, main_ev1, cmp ? &cmpb : nullptr, &listed_deferred);
  GM_HIP(ctx, hipGetLastError());

  // Assembly stream: a large device-buffer call's scan and speculative
  // assembly go to ctx->stream_asm behind its main pass (an event), so the
  // NEXT call's main pass, queued on the context stream, starts as soon as
  // this one's ends and overlaps this call's latency-bound assembly and the
  // walk's tail.  (Its pass counters were zeroed on the context stream; the
  // assembly then zeroes no ring block for a later call.)
  hipStream_t sa = st;
  if (asm_overlap) {
    if (!ctx->stream_asm && hipStreamCreateWithFlags(&ctx->stream_asm, hipStreamNonBlocking) != hipSuccess)
      ctx->stream_asm = nullptr;
    if (ctx->stream_asm) {
      if (!timed) GM_HIP(ctx, hipEventRecord(ev[1], st));  // (a timed call's main pass records it itself)
      GM_HIP(ctx, hipStreamWaitEvent(ctx->stream_asm, ev[1], 0));
      sa = ctx->stream_asm;
    }
  }
  on_asm = sa != st;

  // count -> scan, then ONE host round trip reads the pass counters and the
  // match total together (the slow path below is rare; it re-scans)
  // (tsum: per-tile match counts, written by the main pass and topped up by the listed and slow passes)
  // (compact staging: a two-level scan is left split, k_assemble_c adds the
  // block offsets -- one launch fewer; GM_SCAN_SPLIT=0 turns it off)
  const char* se = knob("GM_SCAN_SPLIT");
  split = cmp && (!se || atoi(se) != 0);
  // Speculative assembly: the rows are written before the host has read the
  // match total, into an ids buffer sized from this context's recent matches
  // per topic (x1.25), so a call makes ONE host round trip.  The total, the
  // pass counters and the assembly come back together; a batch with a listed-
  // pass overflow (slow-path rows) or more matches than the buffer holds is
  // assembled again in finish(), once the host knows the total.
  // (at most FAST_MC per topic: a longer row is a slow-path row, assembled again anyway)
  cap_spec = 1024 + uint64_t(double(n) * std::min(ctx->ids_per_topic, double(FAST_MC)));
  // (no room for the speculative buffer: skip speculation, the rows are
  // assembled at their exact size once the total is known)
  if (!knob("GM_NO_SPEC_IDS")) ids = PoolBuf(ctx->pool, cap_spec * 4 + 16);  // (test knob: as if it failed)
  spec = ids.p != nullptr;
  // The scan may hand back block SUMS (split_sums) only when the speculative
  // assembly runs: that kernel sums them and writes the grand total to
  // toff[n_tiles], which the read-back below copies.  Without it the total
  // would still be k_scan_local's block-local prefix, so the scan
  // then writes its block offsets and total itself.
  int rc = scan_excl(ctx, LoadU64{tsum.as<uint64_t>()}, n_tiles, toff_p,
                     SideSum{probe_tile.as<unsigned long long>(), n_tiles, probe_ctr}, split ? &scan_blk : nullptr, sa,
                     split && spec && sums_mode() ? &split_sums : nullptr);
  if (rc) return rc;
  // (compact staging with no host copy-out queued behind: the assembly kernel
  // writes the read-back words itself and its stop event is the call's end --
  // a copy and an event record fewer, ~10 us of idle stream per call at C1)
  // (a host copy-out queued behind -- the small host-buffer call's tail -- goes
  // between the assembly and the call's end event, recorded after it)
  uint32_t* pin_dev = nullptr;  // the pinned words as the device addresses them
  const bool tail_q = tail && tail->enqueue;
  const bool rb_kernel =
      spec && cmp && hipHostGetDevicePointer(reinterpret_cast<void**>(&pin_dev), pin, 0) == hipSuccess && pin_dev;
  // (compact staging: the assembly also zeroes the ring's next block for the next call, if it is dirty)
  uint32_t* zero_next = nullptr;
  if (spec && cmp && ctr_slot >= 0 && !on_asm) {
    const int z = (ctr_slot + 1) % emqx_gm_ctx::CTR_RING;
    if (ctx->ctr_state[z] == 2) {
      zero_next = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(ctx->ctr_ring) + 64 * z);
      ctx->ctr_state[z] = 0;  // (a kernel queued before any later call zeroes it)
    }
  }
  if (spec) {
    launch_assemble(sa, nblk, cmp ? &cmpb : nullptr, cnt.as<uint32_t>(), n, toff_p, stage.as<uint32_t>(),
                    row_off.as<uint64_t>(), ids.as<uint32_t>(), idx->view.gmap, cap_spec, scan_blk.as<uint64_t>(),
                    rb_kernel ? pin_dev : nullptr, reinterpret_cast<const uint32_t*>(ctrs_p),
                    rb_kernel && !tail_q ? ev[2] : nullptr, zero_next, split_sums);
    GM_HIP(ctx, hipGetLastError());
    if (tail_q) {
      rc = tail->enqueue(row_off.as<uint64_t>(), ids.as<uint32_t>(), cap_spec);
      if (rc) return rc;
      if (rb_kernel) GM_HIP(ctx, hipEventRecord(ev[2], sa));
    }
  }
  if (!rb_kernel) {
    if (int rc2 = readback(sa)) return rc2;
    GM_HIP(ctx, hipEventRecord(ev[2], sa));
  }
  return 0;
}

int MatchCall::finish(emqx_gm_csr* out, MatchTail* tail, bool locked) {
  // wait for the read-back; a call submitted alone waits without the context
  // lock, so other threads can queue their calls meanwhile
  if (locked) {
    GM_HIP(ctx, hipEventSynchronize(ev[2]));
  } else {
    const hipError_t e = hipEventSynchronize(ev[2]);
    if (e != hipSuccess) return set_err(ctx, EMQX_GM_EDEVICE, std::string("match_wait: ") + hipGetErrorString(e));
  }
  std::unique_lock<std::recursive_mutex> lk(ctx->mu, std::defer_lock);
  if (!locked) lk.lock();
  struct StatsCopy {  // this call's stats, kept with it (destroyed before lk: still under the lock)
    MatchCall* c;
    ~StatsCopy() { c->st_copy = c->ctx->stats; }
  } stats_copy{this};
  hipStream_t st = ctx->stream;
  emqx_gm_match_stats& S = ctx->stats;
  S = emqx_gm_match_stats{};
  S.n_topics = n;
  if (n == 0) {
    submitted = false;
    return finish_csr(ctx, 0, 0, row_off, ids, dev_io, out);
  }
  uint64_t nnz = pin[0];
  uint64_t h_ctr[4] = {pin[1], pin[2], pin[3], pin[4]};
  // (an untimed call's events hold an older call's stamps: no figures)
  const float main_ms = timed ? ev_ms(ev[0], ev[1]) : 0.f, call_ms = timed ? ev_ms(ev[0], ev[2]) : 0.f;
  if (listed_deferred && uint32_t(h_ctr[0])) {
    // the main pass queued rows: the listed pass now, a full scan of the
    // topped-up tile sums, the read-back again; the rows are assembled below
    uint32_t* n1 = reinterpret_cast<uint32_t*>(ctrs_p);
    unsigned long long* probe_ctr = reinterpret_cast<unsigned long long*>(ctrs_p + 16);
    unsigned long long* wild_ctr = reinterpret_cast<unsigned long long*>(ctrs_p + 24);
    if (exact)
      launch_listed<true>(st, idx->view, tb, to, n, cnt.as<uint32_t>(), stage.as<uint32_t>(), list1.as<uint32_t>(), n1,
                          list2.as<uint32_t>(), n1 + 1, probe_ctr, wild_ctr, tsum.as<uint64_t>(), &cmpb);
    else
      launch_listed<false>(st, idx->view, tb, to, n, cnt.as<uint32_t>(), stage.as<uint32_t>(), list1.as<uint32_t>(),
                           n1, list2.as<uint32_t>(), n1 + 1, probe_ctr, wild_ctr, tsum.as<uint64_t>(), &cmpb);
    GM_HIP(ctx, hipGetLastError());
    // (the probe counter already holds the main pass's tiles: the side sum is not repeated)
    int rc = scan_excl(ctx, LoadU64{tsum.as<uint64_t>()}, n_tiles, toff_p);
    if (rc) return rc;
    if (int rc2 = readback(st)) return rc2;
    GM_HIP(ctx, hipStreamSynchronize(st));
    nnz = pin[0];
    for (int k = 0; k < 4; ++k) h_ctr[k] = pin[k + 1];
    spec = false;  // the speculative rows lacked the listed rows
    split = false;  // toff is whole now
  }
  S.probes = h_ctr[2];
  S.n_wildcard_topics = h_ctr[3];
  S.n_overflow = uint32_t(h_ctr[0] >> 32);  // n2: the rows the slow path completes (the low half, n1, is the listed queue)
  if (spec && uint32_t(h_ctr[0] >> 32) == 0 && nnz <= cap_spec) {  // no slow-path row, and the rows fit: done
    ctx->ids_per_topic = std::max(1.0, 1.25 * double(nnz) / double(n));
    S.nnz = nnz;
    S.match_kernel_ms = main_ms;
    S.total_device_ms = call_ms;
    if (tail) tail->used = true;
    submitted = false;
    return finish_csr(ctx, n, nnz, row_off, ids, dev_io, out);
  }
  ids.reset();
  if (nnz > cap_spec) ctx->ids_per_topic = std::max(ctx->ids_per_topic, 1.25 * double(nnz) / double(n));
  const uint64_t n_ovf = uint32_t(h_ctr[0] >> 32);

  // ---- slow path for rows the listed pass could not hold
  PoolBuf slow_off, slow_ids;
  uint32_t* ovf_list = list2.as<uint32_t>();
  if (n_ovf) {
    // a frontier holds the nodes of one depth: the widest depth bounds it
    const uint64_t fr_cap = std::min<uint64_t>(uint64_t(idx->view.n_nodes),
                                               idx->level_nodes ? idx->level_nodes : uint64_t(idx->view.n_nodes)) + 1;
    const uint64_t bm_words = (uint64_t(idx->view.n_filters) + 31) / 32 + 1;
    const uint64_t per_blk = (2 * fr_cap + bm_words) * 4;
    // chunks sized by a 1 GiB workspace, up to 16,384 topics (a workgroup each) per launch
    uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(16384, (1ull << 30) / per_blk));
    chunk = std::min(chunk, n_ovf);
    PoolBuf fr(ctx->pool, chunk * 2 * fr_cap * 4);
    PoolBuf bm(ctx->pool, chunk * bm_words * 4);
    PoolBuf scnt(ctx->pool, n_ovf * 8 + 8);
    std::vector<uint64_t> h_off(n_ovf + 1, 0);
    if (!fr.p || !bm.p || !scnt.p) return set_err(ctx, EMQX_GM_ENOMEM, "match: slow-path workspace");
    slow_off = PoolBuf(ctx->pool, (n_ovf + 1) * 8);
    uint64_t cap_ids = std::max<uint64_t>(1024, n_ovf * 64);
    slow_ids = PoolBuf(ctx->pool, cap_ids * 4);
    if (!slow_off.p || !slow_ids.p) return set_err(ctx, EMQX_GM_ENOMEM, "match: slow-path output");
    for (uint64_t k0 = 0; k0 < n_ovf; k0 += chunk) {
      const uint64_t kn = std::min(n_ovf, k0 + chunk);
      if (exact)
        hipLaunchKernelGGL(k_slow_walk<true>, dim3(kn - k0), dim3(256), 0, st, tb, to, idx->view, ovf_list, k0, kn,
                           fr.as<uint32_t>(), fr_cap, bm.as<uint32_t>(), bm_words, cnt.as<uint32_t>(),
                           scnt.as<uint64_t>(), tsum.as<uint64_t>());
      else
        hipLaunchKernelGGL(k_slow_walk<false>, dim3(kn - k0), dim3(256), 0, st, tb, to, idx->view, ovf_list, k0, kn,
                           fr.as<uint32_t>(), fr_cap, bm.as<uint32_t>(), bm_words, cnt.as<uint32_t>(),
                           scnt.as<uint64_t>(), tsum.as<uint64_t>());
      GM_HIP(ctx, hipGetLastError());
      std::vector<uint64_t> c(kn - k0);
      GM_HIP(ctx, hipMemcpyAsync(c.data(), scnt.as<uint64_t>() + k0, (kn - k0) * 8, hipMemcpyDeviceToHost, st));
      GM_HIP(ctx, hipStreamSynchronize(st));
      for (uint64_t k = k0; k < kn; ++k) h_off[k + 1] = h_off[k] + c[k - k0];
      if (h_off[kn] > cap_ids) {  // grow the slow output buffer
        uint64_t ncap = std::max(h_off[kn], cap_ids * 2);
        PoolBuf nb(ctx->pool, ncap * 4);
        if (!nb.p) return set_err(ctx, EMQX_GM_ENOMEM, "match: slow-path output grow");
        if (h_off[k0]) GM_HIP(ctx, hipMemcpyAsync(nb.p, slow_ids.p, h_off[k0] * 4, hipMemcpyDeviceToDevice, st));
        slow_ids = std::move(nb);
        cap_ids = ncap;
      }
      GM_HIP(ctx, hipMemcpyAsync(slow_off.as<uint64_t>() + k0, h_off.data() + k0, (kn - k0 + 1) * 8,
                                 hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k_slow_emit, dim3(kn - k0), dim3(256), 0, st, k0, kn, bm.as<uint32_t>(), bm_words,
                         slow_off.as<uint64_t>(), slow_ids.as<uint32_t>());
      GM_HIP(ctx, hipGetLastError());
    }
    // the slow path added its rows' counts to tsum: scan again
    int rc = scan_excl(ctx, LoadU64{tsum.as<uint64_t>()}, n_tiles, toff_p);
    if (rc) return rc;
    GM_HIP(ctx, hipMemcpyAsync(&nnz, toff_p + n_tiles, 8, hipMemcpyDeviceToHost, st));
    GM_HIP(ctx, hipStreamSynchronize(st));
  }

  // ---- write the rows (again: the speculative pass did not fit or missed slow-path rows)
  ids = PoolBuf(ctx->pool, nnz * 4 + 16);
  if (!ids.p) return set_err(ctx, EMQX_GM_ENOMEM, "match: ids");
  // (after a slow-path rescan toff is whole; otherwise it is still the split first scan)
  launch_assemble(st, nblk, cmp ? &cmpb : nullptr, cnt.as<uint32_t>(), n, toff_p, stage.as<uint32_t>(),
                  row_off.as<uint64_t>(), ids.as<uint32_t>(), idx->view.gmap, nnz,
                  (n_ovf || !split) ? nullptr : scan_blk.as<uint64_t>(), nullptr, nullptr, nullptr, nullptr,
                  (n_ovf || !split) ? 0u : split_sums);
  GM_HIP(ctx, hipGetLastError());
  if (n_ovf) {
    hipLaunchKernelGGL(k_copy_slow, dim3(n_ovf), dim3(256), 0, st, ovf_list, n_ovf, row_off.as<uint64_t>(),
                       slow_off.as<uint64_t>(), slow_ids.as<uint32_t>(), ids.as<uint32_t>(), idx->view.gmap);
    GM_HIP(ctx, hipGetLastError());
  }
  GM_HIP(ctx, hipEventRecord(ev[2], st));
  GM_HIP(ctx, hipEventSynchronize(ev[2]));
  S.nnz = nnz;
  S.match_kernel_ms = main_ms;
  S.total_device_ms = timed ? ev_ms(ev[0], ev[2]) : 0.f;
  submitted = false;
  return finish_csr(ctx, n, nnz, row_off, ids, dev_io, out);
}

int run_match(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint8_t* tb_in, const uint64_t* to_in, uint64_t n,
              uint32_t flags, emqx_gm_csr* out, MatchTail* tail) {
  MatchCall c(ctx);
  if (int rc = c.submit(idx, tb_in, to_in, n, flags, tail)) return rc;
  return c.finish(out, tail, true);
}

int match_submit(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint8_t* tb, const uint64_t* to, uint64_t n,
                 uint32_t flags, void** ticket, MatchTail* tail) {
  auto* c = new MatchCall(ctx);
  if (int rc = c->submit(idx, tb, to, n, flags, tail)) {
    delete c;
    return rc;
  }
  *ticket = c;
  return 0;
}

// (called without ctx->mu; takes it after the wait)
int match_wait(emqx_gm_ctx* ctx, void* ticket, emqx_gm_csr* out, MatchTail* tail, emqx_gm_match_stats* st_out) {
  auto* c = static_cast<MatchCall*>(ticket);
  const int rc = c->finish(out, tail, false);
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  if (st_out) *st_out = c->st_copy;
  delete c;
  return rc;
}

// ---- IX_D0: the root's '+' child's record (IndexView::d0_root), read from
// the depth-1 hot table (the gm_common.h hot_lookup rules: MPH slot + overflow
// region, or linear probing) by one thread, at build and after each in-place
// update (the update renumbers filter ids and may change its sig / hf).
__device__ __forceinline__ uint32_t hot_find(const IndexView& v, int t, uint64_t key) {
  const uint64_t cap = v.hot_cap[t];
  if (!cap) return NONE;
  const HotSlot* tab = v.hot + v.hot_off[t];
  if (const uint32_t mc = v.mph_cap[t]) {
    const uint64_t w = v.mph_word[v.mph_off[t] + mph_bucket(key, v.mph_nb[t])];
    if (!mph_may_hold(w, key)) return NONE;
    const uint32_t s = mph_slot(key, uint32_t(w & 0xFFFFu), mc);
    if (tab[s].key == key) return s;
    if (!((v.mph_ovf >> t) & 1u)) return NONE;
    for (uint64_t o = mph_ovf_home(key, mc, uint32_t(cap));; o = o + 1 == cap ? mc : o + 1) {
      if (tab[o].key == key) return uint32_t(o);
      if (tab[o].key == EDGE_EMPTY) return NONE;
    }
  }
  for (uint64_t s = hot_slot(key, cap);; s = s + 1 == cap ? 0 : s + 1) {
    if (tab[s].key == key) return uint32_t(s);
    if (tab[s].key == EDGE_EMPTY) return NONE;
  }
}
__global__ void k_d0_refresh(IndexView v, uint4* __restrict__ d0) {
  const int t = hot_table(1);
  const uint32_t s = v.plus_word == NONE ? NONE : hot_find(v, t, hot_key(0u, v.plus_word, 0u));
  if (s == NONE) {
    *d0 = D1_NONE;
  } else {
    const HotSlot& h = v.hot[v.hot_off[t] + s];
    *d0 = make_uint4(s, h.sig, h.hf, h.end_filter);
  }
}

int refresh_d0(emqx_gm_ctx* ctx, const IndexView& v, void* d0) {
  if (const char* e = knob("GM_D0"))  // A/B knob: 0 = the walk probes level 0 like any other
    if (!atoi(e)) return 1;
  hipLaunchKernelGGL(k_d0_refresh, dim3(1), dim3(1), 0, ctx->stream, v, static_cast<uint4*>(d0));
  GM_HIP(ctx, hipGetLastError());
  GM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

}  // namespace gm
