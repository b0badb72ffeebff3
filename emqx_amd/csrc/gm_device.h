// gm_device.h — device helpers shared by the side tables' kernels
// (gm_retained.hip, gm_shared.hip, gm_authz.hip): the wave primitives and the
// device twin of gm_dict.h's lookup.  Included by .hip files only.
#pragma once

#include <hip/hip_runtime.h>

#include "gm_dict.h"

namespace gm {

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ uint32_t uni(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ uint32_t lanes_below(uint64_t m, uint32_t lane) {
  return __popcll(m & ((1ull << lane) - 1ull));
}

__device__ __forceinline__ bool bytes_eq(const uint8_t* a, const uint8_t* b, uint32_t n) {
  uint32_t k = 0;
  while (k < n && a[k] == b[k]) ++k;
  return k == n;
}

// dict_hash of p[0, len) over its 8-byte chunks; *head_out: the first chunk (DictSlot::head)
__device__ __forceinline__ uint32_t dict_hash_bytes(const uint8_t* p, uint32_t len, uint64_t* head_out) {
  uint32_t h = DICT_HASH_SEED;
  uint64_t head = 0;
  for (uint32_t i = 0; i < len; i += 8) {
    uint64_t c = 0;
    for (uint32_t k = 0; k < 8 && i + k < len; ++k) c |= uint64_t(p[i + k]) << (8 * k);
    if (!i) head = c;
    h = dict_hash_step(h, c);
  }
  *head_out = head;
  return dict_hash_final(h, len);
}

// id of the word p[0, len) in the dictionary, or NONE (hits verified by bytes;
// a device table always carries word_off).  One value handed back and no
// forced inlining: see the note at az_key_find (gm_authz.hip) on what out-
// parameters written inside such a probe loop cost on gfx950.
// TAIL_INDEXED picks how the bytes past the head are compared, and nothing
// else: bytes_eq on both pointers + 8 (k_authz_check), or one index running
// from 8 (the retained kernels).  One form for both does not exist on gfx950:
// bytes_eq inlined into k_ret_walk and k_ret_expire costs each 2 VGPRs (28 ->
// 30, 56 -> 58, 48 -> 50), the indexed form inlined into k_authz_check
// reschedules the whole kernel and measured +0.8 % at its 16,384-request
// window (profiles/r10_tables/indexed_tail_in_authz).
template <bool TAIL_INDEXED = false>
static __device__ uint32_t dict_find(const DictView& v, const uint8_t* p, uint32_t len) {
  uint64_t head;
  const uint32_t h = dict_hash_bytes(p, len, &head);
  for (uint64_t s = dict_slot(h, v.dict_mask);; s = (s + 1) & v.dict_mask) {
    const DictSlot e = v.dict[s];
    if (e.len == DICT_EMPTY_LEN) return NONE;
    if (e.len != len || e.head != head) continue;
    if constexpr (TAIL_INDEXED) {
      if (len <= 8) return e.word;
      const uint8_t* a = v.arena + v.word_off[e.word];
      uint32_t k = 8;
      while (k < len && a[k] == p[k]) ++k;
      if (k == len) return e.word;
    } else {
      if (len <= 8 || bytes_eq(v.arena + v.word_off[e.word] + 8, p + 8, len - 8)) return e.word;
    }
  }
}

}  // namespace gm
