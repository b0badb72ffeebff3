// gm_dict.h — the word dictionary's format on the host: the one place that
// builds and probes it outside gm_match.hip (its device twin: gm_device.h).
// Plain host C++, header only.
//
// An open-addressing table of DictSlot (gm_common.h) with linear probing from
// dict_slot(dict_hash(word)).  A slot holds the word's length, its first 8
// bytes and its id; a probe that meets both compares the rest of the word with
// the arena, so only words longer than 8 bytes ever read it.
#pragma once

#include <algorithm>
#include <cstring>

#include "gm_common.h"

namespace gm {

struct DictView {
  const DictSlot* dict;
  const uint32_t* word_off;  // [n_words + 1] id -> byte offset in the arena (words in id order);
                             // nullptr on the host: the id IS the offset (the match index, gm_common.h)
  const uint8_t* arena;
  uint64_t dict_mask;        // slots - 1
};

// A byte string and its order: unsigned bytes, a proper prefix first.
struct WordRef {
  const uint8_t* p;
  uint64_t len;
};
inline bool word_less(const WordRef& a, const WordRef& b) {
  const uint64_t m = std::min(a.len, b.len);
  const int c = m ? std::memcmp(a.p, b.p, m) : 0;
  return c ? c < 0 : a.len < b.len;
}
inline bool word_eq(const WordRef& a, const WordRef& b) {
  return a.len == b.len && (!a.len || !std::memcmp(a.p, b.p, a.len));
}
inline bool operator==(const WordRef& a, const WordRef& b) { return word_eq(a, b); }

// slots of a dictionary of n words: a power of two, load <= 1/2
inline uint64_t dict_capacity(uint64_t n_words) {
  uint64_t cap = 16;
  while (cap < 2 * n_words) cap <<= 1;
  return cap;
}

// The slot of the word p[0, len) with id `word`, and the empty slot it goes to
// (the first of its probe sequence; the caller keeps the load below 1).  An
// insert in two halves for dict_fill below and for the one writer that must
// see the slot before it changes: the in-place update journals its old bytes
// (gm_overlay.cpp, Patcher::word).
inline DictSlot dict_entry_host(const uint8_t* p, uint64_t len, uint32_t word) {
  return DictSlot{word_head_host(p, len), uint32_t(len), word};
}
inline DictSlot& dict_vacancy_host(DictSlot* dict, uint64_t mask, const uint8_t* p, uint64_t len) {
  uint64_t s = dict_slot(dict_hash_host(p, len), mask);
  while (dict[s].len != DICT_EMPTY_LEN) s = (s + 1) & mask;
  return dict[s];
}

// A whole dictionary over words[0, n), a word's id its position: the `cap`
// slots, the words' bytes back to back in the arena, and word_off[0 .. n].
inline void dict_fill(const WordRef* words, uint64_t n, DictSlot* dict, uint64_t cap, uint32_t* word_off,
                      uint8_t* arena) {
  for (uint64_t s = 0; s < cap; ++s) dict[s] = DictSlot{0, DICT_EMPTY_LEN, 0};
  uint64_t ab = 0;
  for (uint64_t w = 0; w < n; ++w) {
    word_off[w] = uint32_t(ab);
    if (words[w].len) std::memcpy(arena + ab, words[w].p, words[w].len);
    ab += words[w].len;
    dict_vacancy_host(dict, cap - 1, words[w].p, words[w].len) = dict_entry_host(words[w].p, words[w].len, uint32_t(w));
  }
  word_off[n] = uint32_t(ab);
}

// id of the word p[0, len), or NONE
inline uint32_t dict_find_host(const DictView& v, const uint8_t* p, uint64_t len) {
  if (len >= DICT_EMPTY_LEN) return NONE;
  const uint64_t head = word_head_host(p, len);
  for (uint64_t s = dict_slot(dict_hash_host(p, len), v.dict_mask);; s = (s + 1) & v.dict_mask) {
    const DictSlot& e = v.dict[s];
    if (e.len == DICT_EMPTY_LEN) return NONE;
    if (e.len != len || e.head != head) continue;
    if (len <= 8) return e.word;
    const uint8_t* w = v.arena + (v.word_off ? v.word_off[e.word] : e.word);
    if (!std::memcmp(w + 8, p + 8, len - 8)) return e.word;
  }
}

}  // namespace gm
