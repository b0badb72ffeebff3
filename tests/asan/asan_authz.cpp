// asan_authz.cpp — the authorization table's host compiler and host walk
// (emqx_amd/csrc/gm_authz.cpp) under AddressSanitizer + UBSan, as a stand-alone
// program: an edge set and a seeded random set are compiled and walked, and
// every answer compared with a plain restatement of emqx_authz_rule:match/4 and
// the list clauses of emqx_topic:match/2 on strings (no tables, no ids).
// Built by `make -C emqx_amd/csrc asan-authz`; nothing is preloaded.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../../emqx_amd/csrc/gm_authz.h"

namespace gm {
int set_err(emqx_gm_ctx*, int code, const std::string&) { return code; }  // gm_api.cpp's, minus the thread-local
// gm_authz.hip's device side: a host-only table never gets there
int az_upload(emqx_gm_ctx*, emqx_gm_authz*) { return EMQX_GM_EDEVICE; }
void az_free_device(emqx_gm_authz*) {}
int az_check_device(emqx_gm_ctx*, emqx_gm_authz*, const emqx_gm_authz_batch*, bool, uint8_t*, uint32_t*) {
  return EMQX_GM_EDEVICE;
}
}

namespace {

struct Leaf {
  uint8_t kind;
  std::string arg;  // value, CIDRs (33 B each) or the regex bit
};
struct Rule {
  uint8_t perm, action, op;
  std::vector<Leaf> who;
  std::vector<std::pair<uint8_t, std::string>> filters;  // kind, text
};
struct Range {
  std::string key;
  std::vector<Rule> rules;
};
struct Segment {
  uint32_t kind;
  std::vector<Range> ranges;
};
struct Client {
  bool has_cid, has_un, has_peer, v6;
  std::string cid, un;
  uint8_t peer[16];
  uint32_t re_mask;
};
struct Request {
  Client c;
  uint8_t action;
  std::string topic;
};

// a word of emqx_topic:words/1: an atom ('', '+', '#') or a binary
struct Word {
  bool atom;
  std::string s;
  bool operator==(const Word& o) const { return atom == o.atom && s == o.s; }
};
std::vector<Word> words(const std::string& t) {
  std::vector<Word> out;
  size_t s = 0;
  for (size_t e = 0; e <= t.size(); ++e)
    if (e == t.size() || t[e] == '/') {
      const std::string w = t.substr(s, e - s);
      out.push_back(Word{w.empty() || w == "+" || w == "#", w});
      s = e + 1;
    }
  return out;
}
bool topic_match(const Word* n, size_t nn, const Word* f, size_t nf) {
  if (!nn && !nf) return true;
  if (nn && nf && n[0] == f[0]) return topic_match(n + 1, nn - 1, f + 1, nf - 1);
  if (nn && nf && f[0].atom && f[0].s == "+") return topic_match(n + 1, nn - 1, f + 1, nf - 1);
  if (nf == 1 && f[0].atom && f[0].s == "#") return true;
  return false;
}
std::string cidr(int fam, std::vector<uint8_t> lo, std::vector<uint8_t> hi) {
  std::string s(33, '\0');
  s[0] = char(fam);
  std::copy(lo.begin(), lo.end(), s.begin() + 1);
  std::copy(hi.begin(), hi.end(), s.begin() + 17);
  return s;
}
bool ref_rule(const Rule& r, const Request& q) {
  if (!(r.action & q.action)) return false;
  bool acc = !r.op;
  for (const Leaf& l : r.who) {
    bool m = false;
    if (l.kind == EMQX_GM_AUTHZ_WHO_USERNAME) m = q.c.has_un && q.c.un == l.arg;
    else if (l.kind == EMQX_GM_AUTHZ_WHO_CLIENTID) m = q.c.has_cid && q.c.cid == l.arg;
    else if (l.kind == EMQX_GM_AUTHZ_WHO_REGEX) m = (q.c.re_mask >> uint8_t(l.arg[0])) & 1;
    else
      for (size_t k = 0; k + 33 <= l.arg.size() && q.c.has_peer; k += 33) {
        const bool v6 = l.arg[k] == 6;
        const size_t nb = v6 ? 16 : 4;
        if (v6 == q.c.v6 && std::memcmp(l.arg.data() + k + 1, q.c.peer, nb) <= 0 &&
            std::memcmp(q.c.peer, l.arg.data() + k + 17, nb) <= 0)
          m = true;
      }
    acc = r.op ? (acc || m) : (acc && m);
  }
  if (!acc) return false;
  const std::vector<Word> name = words(q.topic);
  for (const auto& f : r.filters) {
    std::vector<Word> fw = words(f.second);
    if (f.first == EMQX_GM_AUTHZ_FILTER_EQ) {
      if (name == fw) return true;
      continue;
    }
    for (Word& w : fw) {  // feed_var/3
      if (!w.atom && w.s == "${clientid}" && q.c.has_cid) w = Word{false, q.c.cid};
      else if (!w.atom && w.s == "${username}" && q.c.has_un) w = Word{false, q.c.un};
    }
    if (topic_match(name.data(), name.size(), fw.data(), fw.size())) return true;
  }
  return false;
}

int check_set(const std::vector<Segment>& segs, const std::vector<Request>& reqs) {
  // ---- flatten into the description's arrays
  std::vector<uint32_t> seg_kind, rule_id;
  std::vector<uint64_t> seg_range_off{0}, range_rule_off{0}, key_off{0}, who_off{0}, filt_off{0}, leaf_off{0}, foff{0};
  std::vector<uint8_t> perm, action, op, leaf_kind, filter_kind;
  std::string keys, leaf_bytes, filter_bytes;
  std::vector<const Rule*> flat;
  for (const Segment& s : segs) {
    seg_kind.push_back(s.kind);
    for (const Range& r : s.ranges) {
      keys += r.key;
      key_off.push_back(keys.size());
      for (const Rule& ru : r.rules) {
        rule_id.push_back(uint32_t(1000 + flat.size()));
        flat.push_back(&ru);
        perm.push_back(ru.perm), action.push_back(ru.action), op.push_back(ru.op);
        for (const Leaf& l : ru.who) {
          leaf_kind.push_back(l.kind);
          leaf_bytes += l.arg;
          leaf_off.push_back(leaf_bytes.size());
        }
        for (const auto& f : ru.filters) {
          filter_kind.push_back(f.first);
          filter_bytes += f.second;
          foff.push_back(filter_bytes.size());
        }
        who_off.push_back(leaf_kind.size());
        filt_off.push_back(filter_kind.size());
      }
      range_rule_off.push_back(flat.size());
    }
    seg_range_off.push_back(key_off.size() - 1);
  }
  auto u8 = [](const std::string& s) { return reinterpret_cast<const uint8_t*>(s.data()); };
  emqx_gm_authz_desc d{};
  d.n_segments = uint32_t(segs.size());
  d.seg_kind = seg_kind.data();
  d.seg_range_off = seg_range_off.data();
  d.n_ranges = key_off.size() - 1;
  d.range_rule_off = range_rule_off.data();
  d.key_bytes = u8(keys);
  d.key_off = key_off.data();
  d.n_rules = flat.size();
  d.rule_id = rule_id.data();
  d.rule_perm = perm.data();
  d.rule_action = action.data();
  d.rule_who_op = op.data();
  d.rule_who_off = who_off.data();
  d.rule_filter_off = filt_off.data();
  d.n_leaves = leaf_kind.size();
  d.leaf_kind = leaf_kind.data();
  d.leaf_bytes = u8(leaf_bytes);
  d.leaf_off = leaf_off.data();
  d.n_filters = filter_kind.size();
  d.filter_kind = filter_kind.data();
  d.filter_bytes = u8(filter_bytes);
  d.filter_off = foff.data();
  emqx_gm_authz* t = nullptr;
  std::string why;
  if (int rc = gm::az_compile(&d, &t, &why)) return std::printf("compile: %d %s\n", rc, why.c_str()), 1;
  // ---- the batch
  std::string tb, cb, ub;
  std::vector<uint64_t> to{0}, co{0}, uo{0};
  std::vector<uint8_t> flags, peer, act;
  std::vector<uint32_t> masks;
  for (const Request& q : reqs) {
    tb += q.topic, to.push_back(tb.size());
    cb += q.c.cid, co.push_back(cb.size());
    ub += q.c.un, uo.push_back(ub.size());
    flags.push_back(uint8_t((q.c.has_cid ? 1 : 0) | (q.c.has_un ? 2 : 0) | (q.c.has_peer ? 4 : 0) | (q.c.v6 ? 8 : 0)));
    peer.insert(peer.end(), q.c.peer, q.c.peer + 16);
    act.push_back(q.action);
    masks.push_back(q.c.re_mask);
  }
  emqx_gm_authz_batch b{};
  b.n = reqs.size();
  b.topic_bytes = u8(tb), b.topic_off = to.data();
  b.clientid_bytes = u8(cb), b.clientid_off = co.data();
  b.username_bytes = u8(ub), b.username_off = uo.data();
  b.flags = flags.data(), b.peerhost = peer.data(), b.action = act.data(), b.re_mask = masks.data();
  if (int rc = gm::az_check_batch(&b, &why)) return std::printf("batch: %d %s\n", rc, why.c_str()), 1;
  std::vector<uint8_t> verdict(reqs.size() + 1);
  std::vector<uint32_t> rule(reqs.size() + 1);
  gm::az_check_host(t, &b, verdict.data(), rule.data());
  int bad = 0;
  for (size_t i = 0; i < reqs.size() && bad < 5; ++i) {
    const Request& q = reqs[i];
    uint32_t want_v = 0, want_r = EMQX_GM_AUTHZ_NO_RULE, base = 0;
    for (const Segment& s : segs) {
      for (const Range& r : s.ranges) {
        const bool mine = s.kind == EMQX_GM_AUTHZ_GLOBAL ||
                          (s.kind == EMQX_GM_AUTHZ_BY_CLIENTID ? q.c.has_cid && q.c.cid == r.key
                                                               : q.c.has_un && q.c.un == r.key);
        for (size_t k = 0; k < r.rules.size() && mine && !want_v; ++k)
          if (ref_rule(r.rules[k], q)) want_v = r.rules[k].perm, want_r = 1000 + base + uint32_t(k);
        base += uint32_t(r.rules.size());
      }
    }
    if (verdict[i] != want_v || rule[i] != want_r) {
      std::printf("request %zu ('%s', cid '%s'): got %u/%u, expected %u/%u\n", i, q.topic.c_str(), q.c.cid.c_str(),
                  unsigned(verdict[i]), rule[i], want_v, want_r);
      ++bad;
    }
  }
  emqx_gm_authz_info_t info{};
  emqx_gm_authz_info(t, &info);
  if (info.n_rules != flat.size()) ++bad;
  emqx_gm_authz_release(t);
  return bad;
}

Client client(const char* cid, const char* un, std::vector<uint8_t> peer, uint32_t re_mask = 0) {
  Client c{};
  c.has_cid = cid, c.has_un = un, c.has_peer = !peer.empty(), c.v6 = peer.size() == 16;
  if (cid) c.cid = cid;
  if (un) c.un = un;
  std::copy(peer.begin(), peer.end(), c.peer);
  c.re_mask = re_mask;
  return c;
}

}  // namespace

int main() {
  const uint8_t A = EMQX_GM_AUTHZ_ALLOW, D = EMQX_GM_AUTHZ_DENY, PUB = 1, SUB = 2, ALL = 3, P = 0, EQ = 1;
  auto leaf = [](uint8_t k, std::string a) { return Leaf{k, std::move(a)}; };
  const std::string deep40 = [] {
    std::string s = "d0";
    for (int i = 1; i < 40; ++i) s += "/d" + std::to_string(i);
    return s;
  }();
  const std::string long_word(300, 'w');
  std::vector<uint8_t> ff(16, 0xFF), fe80(16, 0);
  fe80[0] = 0xFE, fe80[1] = 0x80;
  std::vector<uint8_t> fe80_hi = ff;
  fe80_hi[0] = 0xFE, fe80_hi[1] = 0xBF;
  // ---- the edge set
  std::vector<Segment> segs(4);
  segs[0].kind = EMQX_GM_AUTHZ_GLOBAL;
  segs[0].ranges.push_back(Range{"", {
      Rule{D, ALL, 0, {leaf(EMQX_GM_AUTHZ_WHO_USERNAME, "blocked")}, {{P, "#"}}},
      Rule{A, PUB, 0, {leaf(EMQX_GM_AUTHZ_WHO_IPADDR, cidr(4, {10, 1, 2, 0}, {10, 1, 2, 255}))}, {{P, "net/+/x"}}},
      Rule{A, SUB, 0, {leaf(EMQX_GM_AUTHZ_WHO_IPADDR, cidr(4, {192, 168, 0, 1}, {192, 168, 0, 1}) + cidr(6, fe80, fe80_hi))},
           {{P, "v6/#"}}},
      Rule{A, PUB, 0, {}, {{P, "and/none"}}},
      Rule{A, PUB, 1, {}, {{P, "or/none"}}},
      Rule{D, PUB, 0, {leaf(EMQX_GM_AUTHZ_WHO_CLIENTID, "c1"), leaf(EMQX_GM_AUTHZ_WHO_USERNAME, "u1"),
                       leaf(EMQX_GM_AUTHZ_WHO_REGEX, std::string(1, char(31)))}, {{P, "three"}}},
      Rule{A, ALL, 1, {leaf(EMQX_GM_AUTHZ_WHO_REGEX, std::string(1, char(0))), leaf(EMQX_GM_AUTHZ_WHO_CLIENTID, "")},
           {{P, "re/#"}}},
      Rule{A, PUB, 0, {}, {}},
      Rule{A, ALL, 0, {}, {{P, "a/+"}, {P, "a/#/c"}, {P, "#/b"}, {P, "+/b/"}, {P, "/lead"}, {P, "trail/"}, {P, ""}, {P, "x//y"}}},
      Rule{A, SUB, 0, {}, {{EQ, "#"}, {EQ, "a/b"}, {EQ, "e/${clientid}"}}},
      Rule{A, PUB, 0, {}, {{P, "cid/${clientid}/m"}, {P, "${username}/first"}, {P, "last/${username}"},
                           {P, "both/${clientid}/${username}"}}},
      Rule{A, ALL, 0, {}, {{P, long_word + "/+"}, {P, deep40}, {P, "p/" + deep40.substr(0, deep40.size() - 3) + "#"}}},
      Rule{D, SUB, 0, {}, {{P, "$SYS/#"}}},
      Rule{A, ALL, 0, {}, {{P, "+/x"}}}}});
  segs[1].kind = EMQX_GM_AUTHZ_BY_CLIENTID;
  segs[1].ranges = {Range{"c1", {Rule{D, PUB, 0, {}, {{P, "k/c"}}}, Rule{A, ALL, 0, {}, {{P, "k/#"}}}}},
                    Range{"", {Rule{A, ALL, 0, {}, {{P, "empty/key"}}}}},
                    Range{"sameprefix-A", {Rule{A, ALL, 0, {}, {{P, "tail/a"}}}}},
                    Range{"sameprefix-B", {Rule{D, ALL, 0, {}, {{P, "tail/a"}}}}},
                    Range{std::string(300, 'c'), {Rule{A, PUB, 0, {}, {{P, "long/${clientid}"}}}}}};
  segs[2].kind = EMQX_GM_AUTHZ_BY_USERNAME;
  segs[2].ranges = {Range{"u1", {Rule{A, SUB, 0, {}, {{P, "k/c"}}}}}, Range{"c1", {Rule{D, ALL, 0, {}, {{P, "cross"}}}}}};
  segs[3].kind = EMQX_GM_AUTHZ_GLOBAL;
  segs[3].ranges.push_back(Range{"", {Rule{A, ALL, 0, {}, {{P, "k/c"}}}, Rule{D, ALL, 0, {}, {{P, "zz/#"}}}}});
  const std::vector<Client> clients = {
      client("c1", "u1", {10, 1, 2, 3}, 1u << 31), client("c2", "blocked", {10, 1, 2, 3}), client("c2", nullptr, {}),
      client(nullptr, nullptr, fe80, 1), client("", "", {192, 168, 0, 1}), client("+", "#", {10, 1, 3, 0}),
      client("a/b", "adm", {10, 1, 1, 255}), client(std::string(300, 'c').c_str(), "u1", {9, 255, 255, 255}),
      client("sameprefix-A", "c1", ff), client("sameprefix-B", "x", {10, 1, 2, 0}), client("sameprefix-C", "u1", {10, 1, 2, 255})};
  const std::vector<std::string> topics = {
      "#", "+", "a", "a/b", "a/b/", "a/+", "a/#", "a/#/c", "a/x/c", "#/b", "x/b", "q/b/", "/lead", "trail/", "", "/", "x//y",
      "e/${clientid}", "e/c1", "cid/c1/m", "cid/${clientid}/m", "cid/+/m", "cid//m", "cid/a/b/m", "u1/first",
      "${username}/first", "#/first", "last/u1", "last/", "both/c1/u1", "both/${clientid}/${username}", "net/q/x", "v6/z",
      "and/none", "or/none", "three", "re/1", "$SYS/x", "k/c", "k/d", "empty/key", "cross", "tail/a",
      "long/" + std::string(300, 'c'), long_word + "/z", long_word.substr(1) + "/z", "unknown/x", deep40, deep40 + "/e",
      "p/" + deep40, "p/" + deep40.substr(0, deep40.size() - 4), "zz", "zz/1/2"};
  std::vector<Request> reqs;
  for (const Client& c : clients)
    for (uint8_t a : {PUB, SUB})
      for (const std::string& t : topics) reqs.push_back(Request{c, a, t});
  if (int rc = check_set(segs, reqs)) return std::printf("edge set: %d\n", rc), 1;
  if (int rc = check_set({}, reqs)) return std::printf("empty table: %d\n", rc), 1;
  if (int rc = check_set(segs, {})) return std::printf("empty batch: %d\n", rc), 1;
  // ---- a seeded random set: 2,000 rules over 4 segments, 500 keys per keyed segment, 20,000 requests
  std::mt19937 rng(7);
  auto pick = [&](uint32_t n) { return uint32_t(rng() % n); };
  auto word = [&] { return "w" + std::to_string(pick(30)); };
  auto filt = [&] {
    const uint32_t n = 2 + pick(3), r = pick(100);
    std::vector<std::string> ws(n);
    for (auto& w : ws) w = word();
    if (r < 15) ws[1 + pick(n - 1)] = "+";
    else if (r < 25) ws[n - 1] = "#";
    else if (r < 33) ws[pick(n)] = pick(2) ? "${clientid}" : "${username}";
    std::string s = ws[0];
    for (uint32_t k = 1; k < n; ++k) s += "/" + ws[k];
    return std::make_pair(uint8_t(r >= 33 && r < 38 ? EQ : P), s);
  };
  auto rule = [&](bool with_who) {
    Rule ru{uint8_t(1 + pick(2)), uint8_t(1 + pick(3)), 0, {}, {}};
    if (with_who && pick(2)) {
      ru.op = uint8_t(pick(2));
      for (uint32_t k = pick(3); k > 0; --k) {
        const uint32_t kind = pick(4);
        if (kind == EMQX_GM_AUTHZ_WHO_IPADDR) ru.who.push_back(leaf(2, cidr(4, {10, uint8_t(pick(4)), 0, 0}, {10, uint8_t(pick(4)), 255, 255})));
        else if (kind == EMQX_GM_AUTHZ_WHO_REGEX) ru.who.push_back(leaf(3, std::string(1, char(pick(32)))));
        else ru.who.push_back(leaf(uint8_t(kind), (kind ? "client" : "user") + std::to_string(pick(600))));
      }
    }
    for (uint32_t k = 1 + pick(2); k > 0; --k) ru.filters.push_back(filt());
    return ru;
  };
  std::vector<Segment> rs(4);
  rs[0].kind = rs[3].kind = EMQX_GM_AUTHZ_GLOBAL;
  rs[1].kind = EMQX_GM_AUTHZ_BY_CLIENTID, rs[2].kind = EMQX_GM_AUTHZ_BY_USERNAME;
  rs[0].ranges.push_back(Range{"", {}});
  for (int k = 0; k < 40; ++k) rs[0].ranges[0].rules.push_back(rule(true));
  for (int k = 0; k < 500; ++k) rs[1].ranges.push_back(Range{"client" + std::to_string(k), {rule(false), rule(false)}});
  for (int k = 0; k < 500; ++k) rs[2].ranges.push_back(Range{"user" + std::to_string(k), {rule(false)}});
  rs[3].ranges.push_back(Range{"", {}});
  for (int k = 0; k < 460; ++k) rs[3].ranges[0].rules.push_back(rule(false));
  std::vector<const Rule*> all;
  for (const Segment& s : rs)
    for (const Range& r : s.ranges)
      for (const Rule& ru : r.rules) all.push_back(&ru);
  std::vector<Request> rq;
  size_t hits = 0;
  for (int i = 0; i < 20000; ++i) {
    const std::string cid = "client" + std::to_string(pick(700)), un = "user" + std::to_string(pick(700));
    Client c = client(pick(30) ? cid.c_str() : nullptr, pick(10) ? un.c_str() : nullptr,
                      pick(3) ? std::vector<uint8_t>{10, uint8_t(pick(6)), uint8_t(pick(256)), 1} : std::vector<uint8_t>{},
                      uint32_t(rng()));
    // a topic some rule's filter can match: '+' and '#' made words, placeholders the client's values
    std::string t;
    const std::string& f = all[pick(uint32_t(all.size()))]->filters[0].second;
    for (const Word& w : words(f)) {
      std::string x = w.s == "+" ? word() : w.s == "#" ? (pick(2) ? word() + "/" + word() : word())
                      : w.s == "${clientid}" && pick(10) ? c.cid : w.s == "${username}" && pick(10) ? c.un : w.s;
      t += (t.empty() ? "" : "/") + x;
    }
    rq.push_back(Request{c, uint8_t(1 + pick(2)), pick(5) ? t : word() + "/" + word()});
  }
  if (int rc = check_set(rs, rq)) return std::printf("random set: %d\n", rc), 1;
  (void)hits;
  std::printf("asan_authz ok\n");
  return 0;
}
