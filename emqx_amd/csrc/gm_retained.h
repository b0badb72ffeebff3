// gm_retained.h — the retained-topic index: layout shared by the host compiler
// and host walk (gm_retained.cpp) and the gfx950 kernels (gm_retained.hip).
//
// It answers the subscribe direction of the broker: which STORED topics does a
// FILTER match (emqx_retainer_mnesia:match_messages/1 + condition/1,
// apps/emqx_retainer/src/emqx_retainer_mnesia.erl:210-244), where the reference
// scans its whole table per subscription.  There is no '$'-rule here: '#' and
// '+/x' do match '$SYS/...' topics (the match-spec pattern is '_'), unlike
// emqx_trie:match/1 on the publish side.
//
// The distinct topics are sorted in word-list order (word by word as unsigned
// bytes, a proper prefix first); a topic's rank is its position there.  A level
// trie over them, all levels in one node array:
//   node 0           the root (prefix of 0 words; topic range [0, n)), node 1 its
//                    level's sentinel;
//   level d (d >= 0) one node per distinct prefix of d+1 words, in sorted order
//                    (siblings adjacent and ascending by word id), then a sentinel.
// A node's children are nodes [child_lo(i), child_lo(i+1)) -- absolute indices,
// monotone within a level; a level's sentinel carries the index of the next
// level's sentinel, so a '+' step maps a node range [a, b) to the one range
// [child_lo(a), child_lo(b)).  topic_lo/topic_hi are explicit: shallower
// topics lie between two subtrees of one level, so a range of nodes is not one
// range of ranks.  Word ids are the rank of the word among the distinct words.
#pragma once

#include "gm_internal.h"

namespace gm {

constexpr uint32_t RET_ENDS = 0x80000000u;     // in RetNode::word: the prefix itself is a stored topic (rank topic_lo)
constexpr uint32_t RET_WORD_MASK = 0x7FFFFFFFu;
constexpr uint32_t RET_PLUS = 0xFFFFFFFEu;     // a filter's '+' among its looked-up word ids
constexpr uint32_t RET_HAS_EXPIRY = 1u;        // RetView::flags: some expiry is non-zero (else the walk reads none)

struct alignas(16) RetNode {
  uint32_t word;      // word id | RET_ENDS
  uint32_t child_lo;  // first child (absolute node index)
  uint32_t topic_lo;  // ranks of the topics carrying this prefix
  uint32_t topic_hi;
};

struct RetView {
  const RetNode* nodes;
  const uint32_t* depth_ends;  // [depth_max + 1]: topics of exactly that many words
  DictView words;              // word -> id (gm_dict.h); DictSlot::word holds the id
  const uint32_t* ids;         // rank -> caller's id
  uint64_t* expiry;            // rank -> expiry in ms, 0 = never; mutated in place by expire
  uint32_t n_topics, n_nodes, n_words, depth_max;
  uint32_t flags;
};

// Per-wave state of k_ret_walk in u32 words: depth_max + 1 frames of 64 (lo, hi)
// items, each frame's count / cursor / offset into the cursor's item, the
// filter's word ids, and 64 words of scan scratch.
inline uint32_t ret_wave_words(uint32_t depth_max) { return (depth_max + 1) * (128 + 4) + 64; }
constexpr uint32_t RET_LDS_WAVE_BYTES = 8192;  // LDS frames while they fit this (4 waves a block: 32 of 160 KiB)
constexpr uint32_t RET_WAVES_PER_BLOCK = 4;
constexpr uint64_t RET_WS_BUDGET = 256ull << 20;  // global-workspace branch: the grid shrinks to keep it under this

}  // namespace gm

struct emqx_gm_retained {
  int device = 0;
  void* dev_base = nullptr;  // one allocation holding every table
  size_t bytes = 0;
  gm::HostBytes blob;        // host copy of the tables (the host walk, info)
  gm::RetView hv{}, dv{};    // views over the host copy / the device allocation
  emqx_gm_retained_info_t info{};
  double last_ms[3] = {0, 0, 0};  // count pass, scan, fill pass of the last timed match
};

namespace gm {
// gm_retained.cpp (host only)
int ret_compile(const uint8_t* tb, const uint64_t* to, uint64_t n, const uint32_t* ids, const uint64_t* expiry,
                emqx_gm_retained** out, std::string* why);
void ret_match_host(const emqx_gm_retained* r, const uint8_t* fb, const uint64_t* fo, uint64_t n, uint64_t now,
                    std::vector<uint64_t>& row_off, std::vector<uint32_t>& ids);
// the end node of a topic walked as an all-literal filter over the host tables (NONE: not stored)
uint32_t ret_find_host(const emqx_gm_retained* r, const uint8_t* p, uint64_t len);
// gm_retained.hip (device)
int ret_upload(emqx_gm_ctx* ctx, emqx_gm_retained* r);
void ret_free_device(emqx_gm_retained* r);
int ret_match_device(emqx_gm_ctx* ctx, emqx_gm_retained* r, const uint8_t* fb, const uint64_t* fo, uint64_t n,
                     uint64_t now, bool timed, emqx_gm_csr* out);
int ret_expire_device(emqx_gm_ctx* ctx, emqx_gm_retained* r, const uint8_t* tb, const uint64_t* to, uint64_t n,
                      const uint64_t* expiry, uint64_t* n_found);
}  // namespace gm
