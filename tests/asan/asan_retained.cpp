// tests/asan/asan_retained.cpp — TEST ONLY: the retained-topic index compiler
// and the host walk (emqx_amd/csrc/gm_retained.cpp) built as host C++ with
// AddressSanitizer + UBSan.  It compiles the edge set and a random set of
// tests/_retained_ref.py's shape, walks filters over them and checks every row
// against a brute-force condition/1 predicate
// (apps/emqx_retainer/src/emqx_retainer_mnesia.erl:225-244); then empty sets,
// NUL and 0xFF bytes, a 5,000-level topic and refused offsets.  Never touches
// a device.  Built by `make -C emqx_amd/csrc asan-retained`, run by
// tests/test_retained_cpu.py::test_compiler_and_host_walk_under_asan.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../../emqx_amd/csrc/gm_retained.h"

namespace gm {
int set_err(emqx_gm_ctx*, int code, const std::string&) { return code; }  // gm_api.cpp's, minus the thread-local
// gm_retained.hip's device side: a host-only index never gets there
int ret_upload(emqx_gm_ctx*, emqx_gm_retained*) { return EMQX_GM_EDEVICE; }
void ret_free_device(emqx_gm_retained*) {}
int ret_match_device(emqx_gm_ctx*, emqx_gm_retained*, const uint8_t*, const uint64_t*, uint64_t, uint64_t, bool,
                     emqx_gm_csr*) {
  return EMQX_GM_EDEVICE;
}
int ret_expire_device(emqx_gm_ctx*, emqx_gm_retained*, const uint8_t*, const uint64_t*, uint64_t, const uint64_t*,
                      uint64_t*) {
  return EMQX_GM_EDEVICE;
}
}  // namespace gm

namespace {
using Words = std::vector<std::string>;

Words split(const std::string& s) {
  Words w;
  size_t a = 0;
  for (size_t i = 0; i <= s.size(); ++i)
    if (i == s.size() || s[i] == '/') {
      w.push_back(s.substr(a, i - a));
      a = i + 1;
    }
  return w;
}

bool cond(Words f, const Words& t) {
  const bool tail = f.back() == "#";
  if (tail) f.erase(std::find(f.begin(), f.end(), "#"));  // Ws1 -- ['#']: the first one
  if (t.size() < f.size() || (!tail && t.size() != f.size())) return false;
  for (size_t k = 0; k < f.size(); ++k)
    if (f[k] != "+" && (f[k] == "#" || f[k] != t[k])) return false;
  return true;
}

struct Packed {
  std::vector<uint8_t> b;
  std::vector<uint64_t> o{0};
  explicit Packed(const std::vector<std::string>& v) {
    for (auto& s : v) {
      b.insert(b.end(), s.begin(), s.end());
      o.push_back(b.size());
    }
    if (b.empty()) b.push_back(0);
  }
};

int check_set(const std::vector<std::string>& topics, const std::vector<std::string>& filters,
              const std::vector<uint64_t>& expiry, uint64_t now) {
  Packed t(topics), f(filters);
  std::vector<uint32_t> ids(topics.size());
  for (size_t i = 0; i < ids.size(); ++i) ids[i] = uint32_t(7 * i + 3);
  emqx_gm_retained* r = nullptr;
  if (emqx_gm_retained_compile_host(t.b.data(), t.o.data(), topics.size(), ids.data(),
                                    expiry.empty() ? nullptr : expiry.data(), &r))
    return 1;
  emqx_gm_csr out;
  if (emqx_gm_retained_match_host(r, f.b.data(), f.o.data(), filters.size(), now, &out)) return 2;
  // the table: the last of equal topics wins; rows in word-list order
  std::map<Words, size_t> tab;
  for (size_t i = 0; i < topics.size(); ++i) tab[split(topics[i])] = i;
  int bad = 0;
  for (size_t k = 0; k < filters.size() && !bad; ++k) {
    std::vector<uint32_t> want;
    const Words fw = split(filters[k]);
    for (auto& kv : tab) {
      const uint64_t e = expiry.empty() ? 0 : expiry[kv.second];
      if (cond(fw, kv.first) && (e == 0 || e > now)) want.push_back(ids[kv.second]);
    }
    const std::vector<uint32_t> got(out.ids + out.row_off[k], out.ids + out.row_off[k + 1]);
    if (got != want) {
      std::printf("row of filter '%s': %zu ids, expected %zu\n", filters[k].c_str(), got.size(), want.size());
      bad = 3;
    }
  }
  emqx_gm_retained_info_t info;
  emqx_gm_retained_info(r, &info);
  if (info.n_topics != tab.size()) bad = 4;
  emqx_gm_retained_csr_free_host(&out);
  emqx_gm_retained_release(r);
  return bad;
}
}  // namespace

int main() {
  const std::vector<std::string> edge_t = {"", "/", "a", "a/", "a//b", "$SYS/x", "a!", "a/b", "longword_0001/x",
                                           "longword_0002/x", "longword_0002", "a/b/c", "+/lit", "a+",
                                           std::string("nul\0in", 6), "\xff\xfe/\xff"};
  const std::vector<std::string> edge_f = {"#", "+", "+/#", "a/#", "#/a", "a/+/#", "a+", "unknown", "a/unknown",
                                           "a/b/c/d", "a/b/c/d/#", "+/+/+/+", "", "/", "+/", "/+", "a/+/b",
                                           "longword_0001/+", "longword_0002/#", "longword_0003/#", "$SYS/+", "+/x",
                                           "#/#", "a/#/#", "+/lit", std::string("nul\0in", 6), "\xff\xfe/+"};
  if (int rc = check_set(edge_t, edge_f, {}, 0)) return std::printf("edge set: %d\n", rc), 1;
  if (int rc = check_set({}, edge_f, {}, 0)) return std::printf("empty index: %d\n", rc), 1;
  if (int rc = check_set(edge_t, {}, {}, 0)) return std::printf("empty batch: %d\n", rc), 1;
  // the random set: 3,000 topics over 12 words, depth 1..6; 2,000 filters, 40 % with a final '#'
  const std::vector<std::string> vocab = {"a", "b", "c", "dd", "", "$SYS", "e!", "longword_over_8_a",
                                          "longword_over_8_b", "f", "g1", "h"};
  std::mt19937 rng(11);
  auto pick = [&](size_t n) { return size_t(rng() % n); };
  std::vector<std::string> topics, filters;
  std::vector<uint64_t> expiry;
  for (int i = 0; i < 3000; ++i) {
    std::string s;
    for (size_t k = 0, n = 1 + pick(6); k < n; ++k) s += (k ? "/" : "") + vocab[pick(vocab.size())];
    topics.push_back(s);
    expiry.push_back(std::vector<uint64_t>{0, 0, 5, 10, 11, 50}[pick(6)]);
  }
  for (int i = 0; i < 2000; ++i) {
    const bool tail = pick(10) < 4;
    std::string s;
    const size_t n = tail ? pick(6) : 1 + pick(6);
    for (size_t k = 0; k < n; ++k) s += (k ? "/" : "") + (pick(10) < 3 ? std::string("+") : vocab[pick(vocab.size())]);
    if (tail) s += n ? "/#" : "#";
    filters.push_back(s);
  }
  if (int rc = check_set(topics, filters, expiry, 10)) return std::printf("random set: %d\n", rc), 1;
  // a 5,000-level topic beside shallow ones; filters of 5,000 '+', 4,999 '+' and '#', 5,001 words
  {
    std::string deep = "w", plus = "+";
    for (int k = 1; k < 5000; ++k) deep += "/w", plus += "/+";
    std::string plus_hash = plus.substr(0, plus.size() - 1) + "#";
    if (int rc = check_set({deep, "w", "w/w", "x"}, {plus, plus_hash, plus + "/+", deep, deep + "/#", "#"}, {}, 0))
      return std::printf("deep set: %d\n", rc), 1;
  }
  // refused inputs
  {
    const uint8_t b[8] = {'a', '/', 'b', 'c', '/', 'd', 0, 0};
    const uint64_t down[4] = {0, 4, 2, 6}, far[3] = {0, 3, uint64_t(1) << 40};
    emqx_gm_retained* r = nullptr;
    if (emqx_gm_retained_compile_host(b, down, 3, nullptr, nullptr, &r) != EMQX_GM_EINVAL || r) return 1;
    if (emqx_gm_retained_compile_host(b, far, 2, nullptr, nullptr, &r) != EMQX_GM_EINVAL || r) return 1;
    if (emqx_gm_retained_compile_host(b, nullptr, 2, nullptr, nullptr, &r) != EMQX_GM_EINVAL || r) return 1;
  }
  std::printf("asan_retained ok\n");
  return 0;
}
