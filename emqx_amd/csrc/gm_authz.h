// gm_authz.h — the authorization table: layout shared by the host compiler and
// host walk (gm_authz.cpp) and the gfx950 kernel (gm_authz.hip).
//
// It answers emqx_authz:do_authorize/4 (apps/emqx_authz/src/emqx_authz.erl:307-317)
// over a chain of file and built-in-database sources for a window of requests
// (clientinfo, action, topic): the first matching rule in the reference's
// evaluation order (emqx_authz_rule:matches/4, emqx_authz_rule.erl:110-125;
// emqx_authz_mnesia:authorize/4, emqx_authz_mnesia.erl:95-111, 212-218).
//
// The table is an ordered list of segments.  A GLOBAL segment is one rule range
// every client scans; a BY_CLIENTID / BY_USERNAME segment maps a key to a rule
// range and a request scans the range under its own clientid / username only.
// All rules lie in one array in evaluation order per range; rule r's who leaves
// are leaves[rules[r].who_lo, rules[r + 1].who_lo) and its topic filters
// filters[rules[r].filt_lo, rules[r + 1].filt_lo) (a sentinel rule closes the
// array).  A filter is a list of word ids; the distinct filter words are
// interned in a DictSlot dictionary (DictSlot::word holds the id).  Ids 0..4 are
// reserved and always present: '' (the empty word), '+', '#', '${clientid}' and
// '${username}' -- their bytes are in the arena like any word's, so the atoms of
// emqx_topic:words/1 compare by id and, on the byte path, by bytes.
//
// There is NO '$'-rule here: emqx_authz_rule:match_topic/2 calls
// emqx_topic:match/2 on word lists, whose clauses (emqx_topic.erl:74-87) have
// none, so '#' and '+/x' do authorize '$SYS/x'.
#pragma once

#include "gm_internal.h"

namespace gm {

constexpr uint32_t AZ_W_EMPTY = 0, AZ_W_PLUS = 1, AZ_W_HASH = 2, AZ_W_PH_CLIENTID = 3, AZ_W_PH_USERNAME = 4;
constexpr uint32_t AZ_RESERVED_WORDS = 5;
constexpr uint32_t AZ_MAX_SEGS = 64;

// filter kinds (AzFilter::n_kind >> 30)
constexpr uint32_t AZ_F_PLAIN = 0, AZ_F_EQ = 1, AZ_F_PATTERN = 2;
constexpr uint32_t AZ_F_N_MASK = 0x3FFFFFFFu;

// AzRule::meta: verdict (1 allow, 2 deny) | action mask << 2 (1 publish, 2 subscribe, 3 all) | OR << 4
constexpr uint32_t AZ_M_OR = 1u << 4;

struct alignas(16) AzRule {
  uint32_t id;       // the caller's rule id
  uint32_t meta;
  uint32_t who_lo;   // first who leaf
  uint32_t filt_lo;  // first topic filter
};

struct alignas(16) AzLeaf {
  uint32_t kind;  // EMQX_GM_AUTHZ_WHO_USERNAME / _CLIENTID / _IPADDR / _REGEX
  uint32_t a;     // username / clientid: arena offset of the value; ipaddr(s): first CIDR; regex: bit
  uint32_t b;     // username / clientid: its length; ipaddr(s): CIDR count
  uint32_t pad;
};

// A CIDR as esockd_cidr:parse/2 leaves it: a family and an inclusive range,
// each address four big-endian u32 (an IPv4 address in the last one).
struct alignas(16) AzCidr {
  uint32_t lo[4], hi[4];
  uint32_t v6;
  uint32_t pad[3];
};

struct AzFilter {
  uint32_t w_lo;    // first word id in fwords
  uint32_t n_kind;  // words | kind << 30
};

struct alignas(32) AzKeySlot {
  uint64_t head;  // first 8 bytes of the key, little endian, zero padded
  uint32_t len;   // DICT_EMPTY_LEN: an empty slot
  uint32_t hash;
  uint32_t off;   // the whole key in the arena (bytes from 8 on verify a hit)
  uint32_t r_lo, r_hi;
  uint32_t pad;
};

struct alignas(32) AzSeg {
  uint32_t kind;      // EMQX_GM_AUTHZ_GLOBAL / _BY_CLIENTID / _BY_USERNAME
  uint32_t r_lo, r_hi;  // GLOBAL: its rule range
  uint32_t key_lo;    // keyed: first slot of its key table
  uint32_t key_mask;  // ... slots - 1
  uint32_t pad[3];
};

struct AzView {
  const AzSeg* segs;
  const AzRule* rules;  // [n_rules + 1]
  const AzLeaf* leaves;
  const AzCidr* cidrs;
  const AzFilter* filters;
  const uint32_t* fwords;
  const AzKeySlot* keys;
  DictView words;  // filter word -> id (gm_dict.h); its arena: word bytes in id order, then key and leaf-value bytes
  uint32_t n_segs, n_rules, n_words, pad;
};

constexpr uint32_t AZ_LEVELS = 16;  // topic levels whose word ids a lane keeps in LDS; deeper topics compare bytes
constexpr uint32_t AZ_BLOCK = 256;

// the four big-endian u32 of a request's peerhost (16 B; an IPv4 address in its first four)
GM_HD void az_peer_words(const uint8_t* p, bool v6, uint32_t w[4]) {
  auto be = [&](int k) {
    return (uint32_t(p[k]) << 24) | (uint32_t(p[k + 1]) << 16) | (uint32_t(p[k + 2]) << 8) | uint32_t(p[k + 3]);
  };
  if (v6) {
    w[0] = be(0), w[1] = be(4), w[2] = be(8), w[3] = be(12);
  } else {
    w[0] = w[1] = w[2] = 0, w[3] = be(0);
  }
}
GM_HD bool az_le(const uint32_t a[4], const uint32_t b[4]) {
  if (a[0] != b[0]) return a[0] < b[0];
  if (a[1] != b[1]) return a[1] < b[1];
  if (a[2] != b[2]) return a[2] < b[2];
  return a[3] <= b[3];
}
// esockd_cidr:match/2: the families equal and lo <= peerhost <= hi
GM_HD bool az_cidr_match(const AzCidr& c, const uint32_t peer[4], bool v6) {
  return (c.v6 != 0) == v6 && az_le(c.lo, peer) && az_le(peer, c.hi);
}
// a word of emqx_topic:words/1 that stays a binary (not one of the atoms '', '+', '#')
GM_HD bool az_is_binary_word(const uint8_t* p, uint32_t len) {
  return len != 0 && !(len == 1 && (p[0] == '+' || p[0] == '#'));
}

}  // namespace gm

struct emqx_gm_authz {
  int device = 0;
  void* dev_base = nullptr;  // one allocation holding every table
  size_t bytes = 0;
  gm::HostBytes blob;        // host copy of the tables (the host walk, info)
  gm::AzView hv{}, dv{};     // views over the host copy / the device allocation
  emqx_gm_authz_info_t info{};
  double last_kernel_ms = 0;  // of the last EMQX_GM_AUTHZ_TIMED check
};

namespace gm {
// gm_authz.cpp (host only)
int az_compile(const emqx_gm_authz_desc* d, emqx_gm_authz** out, std::string* why);
int az_check_batch(const emqx_gm_authz_batch* b, std::string* why);
void az_check_host(const emqx_gm_authz* t, const emqx_gm_authz_batch* b, uint8_t* verdict, uint32_t* rule);
// gm_authz.hip (device)
int az_upload(emqx_gm_ctx* ctx, emqx_gm_authz* t);
void az_free_device(emqx_gm_authz* t);
int az_check_device(emqx_gm_ctx* ctx, emqx_gm_authz* t, const emqx_gm_authz_batch* b, bool timed, uint8_t* verdict,
                    uint32_t* rule);
}  // namespace gm
