// gm_api.cpp — extern "C" boundary of libemqx_gpu_match.so (include/emqx_gpu_match.h).
// No C++ exception crosses the ABI; every failure is an EMQX_GM_E* code with
// the message in emqx_gm_last_error().
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include <sys/mman.h>

#include "gm_combine.h"
#include "gm_dests.h"
#include "gm_internal.h"
#include "gm_publish.h"
#include "gm_shared.h"
#include "gm_subopts.h"
#include "../../include/emqx_gm_ext.h"

namespace gm {

// The message of the calling thread's last failing call.  Per thread, not per
// context: a context is shared by concurrent callers (e.g. NIF calls on
// several dirty schedulers), and a call runs start to end on one thread, so a
// caller reading emqx_gm_last_error() right after its own failure always gets
// its own message and the pointer stays valid until that thread's next call.
thread_local std::string tl_err;

int set_err(emqx_gm_ctx* ctx, int code, const std::string& msg) {
  (void)ctx;
  tl_err = msg;
  return code;
}

DevPool::~DevPool() {
  hipSetDevice(device_);
  reclaim(true);
  for (auto& kv : free_) hipFree(kv.second);
  for (auto& kv : live_) hipFree(kv.first);
  for (hipEvent_t e : ev_idle_) hipEventDestroy(e);
}

void DevPool::release_after(void* p, hipStream_t s) { release_after(&p, 1, s); }
// (one event for all the buffers: each event record is a marker packet on the
// stream, ~5 us of idle GPU between the kernels around it)
void DevPool::release_after(void* const* ps, int np, hipStream_t s) {
  void* q[4];
  int nq = 0;
  for (int i = 0; i < np && nq < 4; ++i)
    if (ps[i] && live_.count(ps[i])) q[nq++] = ps[i];
  if (!nq) return;
  hipEvent_t e = nullptr;
  if (!ev_idle_.empty()) {
    e = ev_idle_.back();
    ev_idle_.pop_back();
  } else if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
    e = nullptr;
  }
  if (!e || hipEventRecord(e, s) != hipSuccess) {  // no event: the old way, wait for the stream
    if (e) ev_idle_.push_back(e);
    hipStreamSynchronize(s);
    for (int i = 0; i < nq; ++i) release(q[i]);
    return;
  }
  for (int i = 0; i < nq; ++i) deferred_.emplace_back(q[i], i + 1 == nq ? e : nullptr);
}

void DevPool::reclaim(bool wait) {
  // a group of buffers freed together is consecutive, the event on its last
  size_t keep = 0;
  for (size_t i = 0; i < deferred_.size();) {
    size_t j = i;
    while (j < deferred_.size() && !deferred_[j].second) ++j;  // the group's event entry
    if (j == deferred_.size()) {  // (not expected: an unterminated group stays)
      while (i < j) deferred_[keep++] = deferred_[i++];
      break;
    }
    hipEvent_t e = deferred_[j].second;
    const bool done = wait ? (hipEventSynchronize(e), true) : hipEventQuery(e) == hipSuccess;
    if (done) {
      ev_idle_.push_back(e);
      for (size_t k = i; k <= j; ++k) release(deferred_[k].first);
    } else {
      for (size_t k = i; k <= j; ++k) deferred_[keep++] = deferred_[k];
    }
    i = j + 1;
  }
  deferred_.resize(keep);
}

// Buffers still handed out (live_) are NOT freed: a caller may hold a host CSR
// past emqx_gm_close, so they are detached and leak as plain malloc'd memory
// (what the CSRs were before the pool existed).
HostPool::~HostPool() {
  for (int k = 0; k < 2; ++k)
    for (auto& kv : free_[k]) drop(kv.second, k != 0);
}
void HostPool::drop(void* p, bool pinned) {
  if (pinned) (void)hipHostFree(p);
  else free(p);
}
void* HostPool::alloc(size_t bytes, bool pinned) {
  constexpr size_t HUGE_PAGE = 2u << 20;
  const size_t r = bytes < HUGE_PAGE ? ((bytes + 4095) & ~size_t(4095)) : ((bytes + HUGE_PAGE - 1) & ~(HUGE_PAGE - 1));
  auto& fl = free_[pinned ? 1 : 0];
  auto it = fl.lower_bound(r);
  if (it != fl.end() && it->first <= r + r / 4) {
    void* p = it->second;
    cached_ -= it->first;
    live_[p] = Buf{it->first, pinned};
    fl.erase(it);
    return p;
  }
  void* p = nullptr;
  if (pinned) {
    if (hipHostMalloc(&p, r, hipHostMallocPortable) != hipSuccess) return nullptr;
  } else {
    if (posix_memalign(&p, r >= HUGE_PAGE ? HUGE_PAGE : 64, r) != 0) return nullptr;
    if (r >= HUGE_PAGE) (void)madvise(p, r, MADV_HUGEPAGE);
  }
  live_[p] = Buf{r, pinned};  // overwrite: an address freed behind the pool's back may come back
  return p;
}
void HostPool::release(void* p) {
  if (!p) return;
  auto it = live_.find(p);
  if (it == live_.end()) {
    free(p);
    return;
  }
  const size_t r = it->second.bytes;
  const bool pinned = it->second.pinned;
  live_.erase(it);
  for (;;) {  // the largest cached ones go first
    auto* big = &free_[0];
    if (free_[0].empty() || (!free_[1].empty() && std::prev(free_[1].end())->first > std::prev(free_[0].end())->first))
      big = &free_[1];
    if (cached_ + r <= kCap || big->empty()) break;
    auto last = std::prev(big->end());
    cached_ -= last->first;
    drop(last->second, big == &free_[1]);
    big->erase(last);
  }
  if (r > kCap) {
    drop(p, pinned);
    return;
  }
  free_[pinned ? 1 : 0].emplace(r, p);
  cached_ += r;
}

PinPool::~PinPool() {
  for (auto& kv : size_) (void)hipHostFree(kv.first);
}
void* PinPool::get(size_t bytes) {
  size_t r = 64 << 10;  // powers of two from 64 KiB
  while (r < bytes) r <<= 1;
  {
    std::lock_guard<std::mutex> lk(mu_);
    auto it = free_.find(r);
    if (it != free_.end()) {
      void* p = it->second;
      free_.erase(it);
      cached_ -= r;
      return p;
    }
  }
  void* p = nullptr;
  if (hipHostMalloc(&p, r, hipHostMallocPortable) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(mu_);
  size_[p] = r;
  return p;
}
void PinPool::put(void* p) {
  if (!p) return;
  std::lock_guard<std::mutex> lk(mu_);
  auto it = size_.find(p);
  if (it == size_.end()) return;
  if (cached_ + it->second > kCap) {  // (over the cap: freed)
    (void)hipHostFree(p);
    size_.erase(it);
    return;
  }
  free_.emplace(it->second, p);
  cached_ += it->second;
}

namespace {
std::mutex g_pin_mu;
std::map<uintptr_t, size_t> g_pinned;  // emqx_gm_host_alloc buffers: start -> bytes
}  // namespace
bool host_pinned_range(const void* p, size_t bytes) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  std::lock_guard<std::mutex> lk(g_pin_mu);
  auto it = g_pinned.upper_bound(a);
  if (it == g_pinned.begin()) return false;
  --it;
  return a >= it->first && a - it->first <= it->second && bytes <= it->second - (a - it->first);
}
void host_pinned_add(void* p, size_t bytes) {
  std::lock_guard<std::mutex> lk(g_pin_mu);
  g_pinned[reinterpret_cast<uintptr_t>(p)] = bytes;
}
bool host_pinned_remove(void* p) {
  std::lock_guard<std::mutex> lk(g_pin_mu);
  return g_pinned.erase(reinterpret_cast<uintptr_t>(p)) != 0;
}

static size_t round_size(size_t b) {
  if (b < 4096) return 4096;
  if (b < (64u << 20)) {  // powers of two below 64 MiB
    size_t p = 4096;
    while (p < b) p <<= 1;
    return p;
  }
  return (b + (2u << 20) - 1) & ~size_t((2u << 20) - 1);  // 2 MiB granules above
}

void* DevPool::alloc(size_t bytes) {
  if (!deferred_.empty()) reclaim(false);
  size_t r = round_size(bytes);
  auto it = free_.lower_bound(r);
  if (it != free_.end() && it->first <= r + r / 4) {
    void* p = it->second;
    live_[p] = it->first;
    cached_ -= it->first;
    free_.erase(it);
    return p;
  }
  void* p = nullptr;
  hipSetDevice(device_);
  if (hipMalloc(&p, r) != hipSuccess) {
    trim();
    if (!deferred_.empty()) {  // memory is short: wait for the deferred frees, then try once more
      reclaim(true);
      trim();
      if (hipMalloc(&p, r) == hipSuccess) {
        live_[p] = r;
        return p;
      }
    }
    if (hipMalloc(&p, r) != hipSuccess) return nullptr;
  }
  live_[p] = r;
  return p;
}

void DevPool::release(void* p) {
  auto it = live_.find(p);
  if (it == live_.end()) return;
  free_.emplace(it->second, p);
  cached_ += it->second;
  live_.erase(it);
}

void DevPool::trim() {
  hipSetDevice(device_);
  hipDeviceSynchronize();
  reclaim(false);  // (every event has passed now)
  for (auto& kv : free_) hipFree(kv.second);
  free_.clear();
  cached_ = 0;
}

int sum_filter_lengths(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint32_t* d_ids, uint64_t nnz,
                       uint64_t* out);

int table_upload(emqx_gm_ctx* ctx, const HostBytes& blob, size_t bytes, const char* what, void** dev_base) {
  GM_HIP(ctx, hipSetDevice(ctx->device));
  void* d = nullptr;
  if (hipMalloc(&d, bytes) != hipSuccess) return set_err(ctx, EMQX_GM_ENOMEM, std::string(what) + ": device tables");
  hipError_t e = hipMemcpyAsync(d, blob.data(), bytes, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    hipFree(d);
    return set_err(ctx, EMQX_GM_EDEVICE, std::string(what) + ": upload: " + hipGetErrorString(e));
  }
  *dev_base = d;
  return EMQX_GM_OK;
}

void table_free(int device, void* dev_base) {
  hipSetDevice(device);
  hipFree(dev_base);
}

}  // namespace gm

extern "C" {

int emqx_gm_abi_version(void) { return EMQX_GM_ABI_VERSION; }

static int open_one(int dev, uint32_t flags, emqx_gm_ctx** out) {
  if (hipSetDevice(dev) != hipSuccess) return EMQX_GM_EDEVICE;
  auto* ctx = new emqx_gm_ctx;
  ctx->device = dev;
  ctx->open_flags = flags;
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return EMQX_GM_EDEVICE;
  }
  ctx->own_stream = true;
  gm::note_ctx_open(dev);
  ctx->pool = new gm::DevPool(dev);
  ctx->hpool = new gm::HostPool;
  ctx->pins = new gm::PinPool;
  for (auto& e : ctx->ev) {
    if (hipEventCreate(&e) != hipSuccess) {
      emqx_gm_close(ctx);
      return EMQX_GM_EDEVICE;
    }
  }
  *out = ctx;
  return EMQX_GM_OK;
}

int emqx_gm_open(const emqx_gm_opts* opts, emqx_gm_ctx** out) {
  if (!out) return EMQX_GM_EINVAL;
  *out = nullptr;
  GM_GUARD_BEGIN
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return EMQX_GM_EDEVICE;
  if (opts && (opts->flags & ~(EMQX_GM_OPEN_MIRROR_EAGER | EMQX_GM_OPEN_MIRROR_LAZY))) return EMQX_GM_EINVAL;
  if (opts && (opts->flags & EMQX_GM_OPEN_MIRROR_EAGER) && (opts->flags & EMQX_GM_OPEN_MIRROR_LAZY))
    return EMQX_GM_EINVAL;
  std::vector<int> devs;
  if (opts && opts->n_devices) {
    if (opts->n_devices > EMQX_GM_MAX_DEVICES) return EMQX_GM_EINVAL;
    devs.assign(opts->devices, opts->devices + opts->n_devices);
  } else {
    devs.push_back(opts ? opts->device : 0);
  }
  for (int d : devs)
    if (d < 0 || d >= count) return EMQX_GM_EINVAL;
  const uint32_t flags = opts ? opts->flags : 0;
  emqx_gm_ctx* ctx = nullptr;
  if (int rc = open_one(devs[0], flags, &ctx)) return rc;
  for (size_t k = 1; k < devs.size(); ++k) {
    emqx_gm_ctx* m = nullptr;
    if (int rc = open_one(devs[k], flags, &m)) {
      emqx_gm_close(ctx);
      return rc;
    }
    m->parent = ctx;
    ctx->members.push_back(m);
  }
  // replicas are copied GPU to GPU, in a tree (any listed device may be a
  // copy's source): peer access between every pair lets the copy engines go
  // over xGMI directly (already enabled, or unsupported: the runtime stages it)
  for (int a : devs)
    for (int b : devs) {
      int can = 0;
      if (a == b || hipDeviceCanAccessPeer(&can, a, b) != hipSuccess || !can) continue;
      hipSetDevice(a);
      (void)hipDeviceEnablePeerAccess(b, 0);
      (void)hipGetLastError();  // (hipErrorPeerAccessAlreadyEnabled is fine)
    }
  hipSetDevice(devs[0]);
  *out = ctx;
  return EMQX_GM_OK;
  GM_GUARD_END(nullptr)
}

int emqx_gm_devices(const emqx_gm_ctx* ctx, int32_t* devices, uint32_t* n) {
  if (!ctx || !n) return EMQX_GM_EINVAL;
  *n = uint32_t(1 + ctx->members.size());
  if (devices) {
    devices[0] = ctx->device;
    for (size_t k = 0; k < ctx->members.size(); ++k) devices[k + 1] = ctx->members[k]->device;
  }
  return EMQX_GM_OK;
}

int emqx_gm_host_alloc(emqx_gm_ctx* ctx, uint64_t bytes, void** p) {
  if (!ctx || !p) return EMQX_GM_EINVAL;
  *p = nullptr;
  hipSetDevice(ctx->device);
  void* q = nullptr;
  const hipError_t e = hipHostMalloc(&q, bytes ? bytes : 1, hipHostMallocPortable);
  if (e != hipSuccess) return gm::set_err(ctx, EMQX_GM_ENOMEM, std::string("host_alloc: ") + hipGetErrorString(e));
  GM_GUARD_BEGIN
  gm::host_pinned_add(q, bytes);
  *p = q;
  return EMQX_GM_OK;
  GM_GUARD_END(ctx)
}

int emqx_gm_host_free(emqx_gm_ctx* ctx, void* p) {
  if (!ctx) return EMQX_GM_EINVAL;
  if (!p) return EMQX_GM_OK;
  if (!gm::host_pinned_remove(p)) return gm::set_err(ctx, EMQX_GM_EINVAL, "host_free: not an emqx_gm_host_alloc buffer");
  // (a match call in flight on another thread may still read it: the caller's
  // business, as for any input buffer)
  GM_HIP(ctx, hipHostFree(p));
  return EMQX_GM_OK;
}

int emqx_gm_close(emqx_gm_ctx* ctx) {
  if (!ctx) return EMQX_GM_EINVAL;
  gm::free_combiners(ctx);  // (closed first: no group is on the device past here)
  for (emqx_gm_ctx* m : ctx->members) emqx_gm_close(m);
  ctx->members.clear();
  {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    hipSetDevice(ctx->device);
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    gm::note_ctx_close(ctx->device);
    gm::trim_spare_blob(ctx->device);
    gm::free_host_pipe(ctx);
    delete ctx->pool;
    delete ctx->hpool;
    delete ctx->pins;
    for (auto& e : ctx->ev)
      if (e) hipEventDestroy(e);
    if (ctx->own_stream && ctx->stream) hipStreamDestroy(ctx->stream);
    if (ctx->stream_asm) {
      hipStreamSynchronize(ctx->stream_asm);
      hipStreamDestroy(ctx->stream_asm);
    }
    for (hipEvent_t e : ctx->ev_free) hipEventDestroy(e);
    for (void* p : ctx->pin_all) hipHostFree(p);
    if (ctx->ctr_ring) hipFree(ctx->ctr_ring);
  }
  delete ctx;
  return EMQX_GM_OK;
}

const char* emqx_gm_last_error(const emqx_gm_ctx* ctx) {
  (void)ctx;
  return gm::tl_err.c_str();
}

int emqx_gm_set_stream(emqx_gm_ctx* ctx, void* s) {
  if (!ctx) return EMQX_GM_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->stream);
  if (ctx->stream_asm) hipStreamSynchronize(ctx->stream_asm);
  if (s) {
    if (ctx->own_stream) hipStreamDestroy(ctx->stream);
    ctx->stream = static_cast<hipStream_t>(s);
    ctx->own_stream = false;
  } else if (!ctx->own_stream) {
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess)
      return gm::set_err(ctx, EMQX_GM_EDEVICE, "set_stream: hipStreamCreate");
    ctx->own_stream = true;
  }
  return EMQX_GM_OK;
}

int emqx_gm_synchronize(emqx_gm_ctx* ctx) {
  if (!ctx) return EMQX_GM_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  for (emqx_gm_ctx* m : ctx->members) {
    std::lock_guard<std::recursive_mutex> ml(m->mu);
    hipSetDevice(m->device);
    GM_HIP(ctx, hipStreamSynchronize(m->stream));
  }
  hipSetDevice(ctx->device);
  GM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->stream_asm) GM_HIP(ctx, hipStreamSynchronize(ctx->stream_asm));
  return EMQX_GM_OK;
}

// A snapshot made on a multi-device context gets its replicas (gm_multi.cpp)
// unless the update made them itself; the call's update stats are closed.
static int replicated(emqx_gm_ctx* ctx, int rc, emqx_gm_index* prev, emqx_gm_index** out, double t0) {
  if (!rc && !ctx->members.empty() && out && *out) rc = gm::replicate_result(ctx, prev, out);
  gm::tl_ustats.total_ms = gm::now_ms() - t0;
  return rc;
}
static double begin_index_call(uint32_t kind) {
  gm::tl_ustats = emqx_gm_update_stats{};
  gm::tl_ustats.kind = kind;
  return gm::now_ms();
}

int emqx_gm_index_build(emqx_gm_ctx* ctx, const uint8_t* fb, const uint64_t* fo, uint64_t n,
                        const uint64_t* sub_off, const uint32_t* sub_ids, uint32_t* perm_out,
                        emqx_gm_index** out) {
  if (!ctx) return EMQX_GM_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  GM_GUARD_BEGIN
  const double t0 = begin_index_call(EMQX_GM_UPD_BUILD);
  hipSetDevice(ctx->device);
  return replicated(ctx, gm::build_index(ctx, fb, fo, n, sub_off, sub_ids, perm_out, out), nullptr, out, t0);
  GM_GUARD_END(ctx)
}

int emqx_gm_index_build_sharded(emqx_gm_ctx* ctx, const uint8_t* fb, const uint64_t* fo, uint64_t n,
                                const uint64_t* sub_off, const uint32_t* sub_ids, uint32_t* perm_out,
                                emqx_gm_index** out) {
  if (!ctx) return EMQX_GM_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  GM_GUARD_BEGIN
  const double t0 = begin_index_call(EMQX_GM_UPD_BUILD);
  hipSetDevice(ctx->device);
  const int rc = gm::build_sharded(ctx, fb, fo, n, sub_off, sub_ids, perm_out, out);
  gm::tl_ustats.total_ms = gm::now_ms() - t0;
  return rc;
  GM_GUARD_END(ctx)
}

int emqx_gm_index_update(emqx_gm_ctx* ctx, emqx_gm_index* prev, const uint8_t* fb, const uint64_t* fo,
                         const uint8_t* ops, uint64_t n_ops, emqx_gm_index** out) {
  if (!ctx) return EMQX_GM_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  if (prev && prev->device != ctx->device)
    return gm::set_err(ctx, EMQX_GM_EINVAL, "index_update: index lives on another device");
  GM_GUARD_BEGIN
  const double t0 = begin_index_call(EMQX_GM_UPD_NONE);
  hipSetDevice(ctx->device);
  if (prev && prev->route) {  // a sharded index: every shard applies its share at once (gm_shard.cpp)
    const int rc = gm::update_sharded(ctx, prev, fb, fo, ops, n_ops, out);
    gm::tl_ustats.total_ms = gm::now_ms() - t0;
    return rc;
  }
  return replicated(ctx, gm::update_index(ctx, prev, fb, fo, ops, n_ops, out), prev, out, t0);
  GM_GUARD_END(ctx)
}

int emqx_gm_index_update_subs(emqx_gm_ctx* ctx, emqx_gm_index* prev, const uint8_t* fb, const uint64_t* fo,
                              const uint32_t* subs, const uint8_t* ops, uint64_t n_ops, emqx_gm_index** out) {
  if (!ctx) return EMQX_GM_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  if (prev && prev->device != ctx->device)
    return gm::set_err(ctx, EMQX_GM_EINVAL, "index_update_subs: index lives on another device");
  if (prev && prev->route)
    return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "index_update_subs: sharded index (rebuild it)");
  GM_GUARD_BEGIN
  const double t0 = begin_index_call(EMQX_GM_UPD_NONE);
  hipSetDevice(ctx->device);
  return replicated(ctx, gm::update_subs(ctx, prev, fb, fo, subs, ops, n_ops, out), prev, out, t0);
  GM_GUARD_END(ctx)
}

int emqx_gm_index_export(emqx_gm_ctx* ctx, const emqx_gm_index* idx, uint32_t flags, uint8_t* buf, uint64_t* size) {
  if (!ctx) return EMQX_GM_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  if (idx && idx->route) return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "index_export: sharded index");
  GM_GUARD_BEGIN
  return gm::index_export(ctx, idx, flags, buf, size);
  GM_GUARD_END(ctx)
}

int emqx_gm_index_device_blob(const emqx_gm_index* idx, const void** d_blob, uint64_t* bytes) {
  if (!idx || !d_blob || !bytes) return EMQX_GM_EINVAL;
  if (idx->ov || idx->dev_subs || !idx->dev_base) return EMQX_GM_EUNSUPPORTED;
  *d_blob = idx->dev_base;
  *bytes = idx->dev_bytes;
  return EMQX_GM_OK;
}

int emqx_gm_index_import(emqx_gm_ctx* ctx, const uint8_t* image, uint64_t size, const void* d_blob,
                         emqx_gm_index** out) {
  if (!ctx) return EMQX_GM_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  GM_GUARD_BEGIN
  const double t0 = begin_index_call(EMQX_GM_UPD_IMPORT);
  hipSetDevice(ctx->device);
  return replicated(ctx, gm::index_import(ctx, image, size, d_blob, out), nullptr, out, t0);
  GM_GUARD_END(ctx)
}

int emqx_gm_index_retain(emqx_gm_index* idx) {
  if (!idx) return EMQX_GM_EINVAL;
  idx->refs.fetch_add(1);
  return EMQX_GM_OK;
}

int emqx_gm_index_release(emqx_gm_index* idx) {
  if (!idx) return EMQX_GM_EINVAL;
  if (idx->refs.fetch_sub(1) == 1) gm::free_index(idx);
  return EMQX_GM_OK;
}

int emqx_gm_index_info(const emqx_gm_index* idx, emqx_gm_index_info_t* info) {
  if (!idx || !info) return EMQX_GM_EINVAL;
  *info = idx->info;
  return EMQX_GM_OK;
}

int emqx_gm_index_filter(const emqx_gm_index* idx, uint32_t id, const uint8_t** bytes, uint64_t* len) {
  if (!idx || !bytes || !len) return EMQX_GM_EINVAL;
  if (idx->ov) return gm::overlay_filter(idx, id, bytes, len);
  if (!idx->gmap.empty()) {  // shard index: ids are global
    auto it = std::lower_bound(idx->gmap.begin(), idx->gmap.end(), id);
    if (it == idx->gmap.end() || *it != id) return EMQX_GM_EINVAL;
    id = uint32_t(it - idx->gmap.begin());
  }
  if (id >= idx->info.n_filters) return EMQX_GM_EINVAL;
  *bytes = idx->ft.at(id, len);
  return EMQX_GM_OK;
}

int emqx_gm_index_subscriber_count(const emqx_gm_index* idx, uint32_t id, uint64_t* n) {
  if (!idx || !n || idx->ov || !idx->gmap.empty()) return EMQX_GM_EINVAL;
  if (id >= idx->info.n_filters) return EMQX_GM_EINVAL;
  *n = idx->subs.empty() ? 0 : idx->subs.count(id);
  return EMQX_GM_OK;
}

// The stats of the calling thread's last match / fan-out call and the
// context it ran on (emqx_gm_last_stats): concurrent callers of one context
// each read their own call's.
static thread_local emqx_gm_match_stats tl_stats;
static thread_local const emqx_gm_ctx* tl_stats_ctx = nullptr;
static int noted(const emqx_gm_ctx* api_ctx, const emqx_gm_ctx* ran, int rc) {
  if (rc == EMQX_GM_OK) {
    tl_stats = ran->stats;
    tl_stats_ctx = api_ctx;
  }
  return rc;
}

// A host-buffer call of at most one chunk (a publish window): ONE device serves
// it whole -- on a multi-device context the next one round-robin -- and the
// call holds that device's lock only while it queues its work and collects
// its rows (gm_host.cpp run_host_small), so concurrent callers (a NIF's dirty
// schedulers) overlap on one device and run on different GPUs at once, as the
// reference's publishers match in their own processes at once
// (apps/emqx/src/emqx_trie.erl:66-70, emqx_router.erl:128-145).  Larger calls
// are cut into chunks spread over every device (gm_host.cpp run_host_pipe).
static int match_small(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint8_t* tb, const uint64_t* to, uint64_t n,
                       uint32_t flags, emqx_gm_csr* out, gm::SmallFan* fan = nullptr) {
  const size_t K = 1 + (idx->reps.size() == ctx->members.size() ? ctx->members.size() : 0);
  const size_t pick = K > 1 ? ctx->rr.fetch_add(1, std::memory_order_relaxed) % K : 0;
  emqx_gm_ctx* mc = pick ? ctx->members[pick - 1] : ctx;
  const emqx_gm_index* rix = pick ? idx->reps[pick - 1] : idx;
  hipSetDevice(mc->device);
  emqx_gm_match_stats st{};
  const int rc = gm::run_host_small(mc, rix, tb, to, n, flags, out, &st, fan);
  if (rc == EMQX_GM_OK) {
    tl_stats = st;
    tl_stats_ctx = ctx;
  }
  hipSetDevice(ctx->device);
  return rc;
}

// a host-buffer call that runs whole on one device (run_host_small)
static bool small_call(const emqx_gm_index* idx, const uint64_t* to, uint64_t n, uint32_t flags) {
  return !(flags & EMQX_GM_DEVICE_IO) && !idx->ov && !idx->route && n <= gm::host_chunk_topics() &&
         (n == 0 || to[n] - to[0] <= (uint64_t(64) << 20)) && !gm::knob("GM_HOST_SIMPLE") && !gm::knob("GM_HOST_PIPE");
}

int emqx_gm_match(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint8_t* tb, const uint64_t* to,
                  uint64_t n, uint32_t flags, emqx_gm_csr* out) {
  if (!ctx) return EMQX_GM_EINVAL;
  if (!idx || !out || (n && (!tb || !to))) return gm::set_err(ctx, EMQX_GM_EINVAL, "match: NULL argument");
  if (flags & ~(EMQX_GM_WITH_EXACT | EMQX_GM_DEVICE_IO | EMQX_GM_NO_TIMING))
    return gm::set_err(ctx, EMQX_GM_EINVAL, "match: flags");
  if ((flags & EMQX_GM_NO_TIMING) && !(flags & EMQX_GM_DEVICE_IO))
    return gm::set_err(ctx, EMQX_GM_EINVAL, "match: EMQX_GM_NO_TIMING needs EMQX_GM_DEVICE_IO");
  if (n >= 0xFFFFFFF0ull) return gm::set_err(ctx, EMQX_GM_EINVAL, "match: batch too large (>= 2^32 topics)");
  if (idx->device != ctx->device) return gm::set_err(ctx, EMQX_GM_EINVAL, "match: index lives on another device");
  std::memset(out, 0, sizeof(*out));
  GM_GUARD_BEGIN
  if (idx->route) {  // a sharded index: each topic to its one device's shard (gm_shard.cpp)
    if (flags & EMQX_GM_DEVICE_IO)
      return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "match: sharded index takes host buffers");
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    hipSetDevice(ctx->device);
    return noted(ctx, ctx, gm::run_match_sharded(ctx, idx, tb, to, n, flags, out));
  }
  if (small_call(idx, to, n, flags)) return match_small(ctx, idx, tb, to, n, flags, out);
  std::unique_lock<std::recursive_mutex> lk(ctx->mu);
  hipSetDevice(ctx->device);
  if (idx->ov) return noted(ctx, ctx, gm::run_match_overlay(ctx, idx, tb, to, n, flags, out));
  if (!(flags & EMQX_GM_DEVICE_IO) && !gm::knob("GM_HOST_SIMPLE"))  // host buffers: chunked, pipelined
    return noted(ctx, ctx, gm::run_match_host(ctx, idx, tb, to, n, flags, out));
  if (!(flags & EMQX_GM_DEVICE_IO)) return noted(ctx, ctx, gm::run_match(ctx, idx, tb, to, n, flags, out));
  // device buffers: the call is queued under the lock and waited for outside
  // it, so concurrent callers' batches queue behind this one meanwhile
  void* t = nullptr;
  const int rc = gm::match_submit(ctx, idx, tb, to, n, flags, &t);
  if (rc) return rc;
  lk.unlock();
  return noted(ctx, ctx, gm::match_wait(ctx, t, out));
  GM_GUARD_END(ctx)
}

int emqx_gm_match_submit(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint8_t* tb, const uint64_t* to,
                         uint64_t n, uint32_t flags, emqx_gm_call** call) {
  if (!ctx) return EMQX_GM_EINVAL;
  if (!call) return gm::set_err(ctx, EMQX_GM_EINVAL, "match_submit: NULL call");
  *call = nullptr;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  if (!idx || (n && (!tb || !to))) return gm::set_err(ctx, EMQX_GM_EINVAL, "match_submit: NULL argument");
  if (flags & ~(EMQX_GM_WITH_EXACT | EMQX_GM_DEVICE_IO | EMQX_GM_NO_TIMING))
    return gm::set_err(ctx, EMQX_GM_EINVAL, "match_submit: flags");
  if (!(flags & EMQX_GM_DEVICE_IO))
    return gm::set_err(ctx, EMQX_GM_EINVAL, "match_submit: device buffers only (EMQX_GM_DEVICE_IO)");
  if (n >= 0xFFFFFFF0ull) return gm::set_err(ctx, EMQX_GM_EINVAL, "match_submit: batch too large (>= 2^32 topics)");
  if (idx->device != ctx->device) return gm::set_err(ctx, EMQX_GM_EINVAL, "match_submit: index lives on another device");
  if (idx->ov) return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "match_submit: overlay snapshot (use emqx_gm_match)");
  if (idx->route) return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "match_submit: sharded index (use emqx_gm_match)");
  GM_GUARD_BEGIN
  hipSetDevice(ctx->device);
  void* t = nullptr;
  const int rc = gm::match_submit(ctx, idx, tb, to, n, flags, &t);
  if (rc == EMQX_GM_OK) *call = static_cast<emqx_gm_call*>(t);
  return rc;
  GM_GUARD_END(ctx)
}

int emqx_gm_match_wait(emqx_gm_ctx* ctx, emqx_gm_call* call, emqx_gm_csr* out) {
  if (!ctx || !call) return EMQX_GM_EINVAL;
  if (!out) return gm::set_err(ctx, EMQX_GM_EINVAL, "match_wait: NULL out");
  std::memset(out, 0, sizeof(*out));
  GM_GUARD_BEGIN
  hipSetDevice(ctx->device);
  return noted(ctx, ctx, gm::match_wait(ctx, call, out));
  GM_GUARD_END(ctx)
}

// A host-row fan-out of a publish window (fewer than 65,536 rows, at most 16M
// deliveries): like match_small, ONE device serves it whole, round-robin over a
// multi-device context's replicas, holding that device's lock only to queue
// its work (gm_host.cpp run_fanout_small).  1: not small, take the ordinary path.
static int fanout_small(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const emqx_gm_csr* m, emqx_gm_csr* out) {
  const size_t K = 1 + (idx->reps.size() == ctx->members.size() ? ctx->members.size() : 0);
  const size_t pick = K > 1 ? ctx->rr.fetch_add(1, std::memory_order_relaxed) % K : 0;
  emqx_gm_ctx* mc = pick ? ctx->members[pick - 1] : ctx;
  const emqx_gm_index* rix = pick ? idx->reps[pick - 1] : idx;
  hipSetDevice(mc->device);
  emqx_gm_match_stats st{};
  const int rc = gm::run_fanout_small(mc, rix, idx, m, out, &st);
  if (rc == EMQX_GM_OK) {
    tl_stats = st;
    tl_stats_ctx = ctx;
  }
  hipSetDevice(ctx->device);
  return rc;
}

int emqx_gm_fanout(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const emqx_gm_csr* m, uint32_t flags,
                   emqx_gm_csr* out) {
  if (!ctx) return EMQX_GM_EINVAL;
  if (idx && m && out && flags == (flags & EMQX_GM_WITH_EXACT) && !m->on_device && m->row_off && (!m->nnz || m->ids) &&
      m->n_rows < 65536 && !idx->view.gmap && !idx->ov && !idx->route && !idx->subs.empty() &&
      idx->device == ctx->device && !gm::knob("GM_FANOUT_SIMPLE")) {
    std::memset(out, 0, sizeof(*out));
    GM_GUARD_BEGIN
    const int rc = fanout_small(ctx, idx, m, out);
    if (rc != 1) return rc;
    GM_GUARD_END(ctx)
  }
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  if (!idx || !m || !out || (m->nnz && !m->ids) || !m->row_off)
    return gm::set_err(ctx, EMQX_GM_EINVAL, "fanout: NULL argument");
  if (flags & ~(EMQX_GM_WITH_EXACT | EMQX_GM_DEVICE_IO)) return gm::set_err(ctx, EMQX_GM_EINVAL, "fanout: flags");
  if (idx->view.gmap) return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "fanout: shard index (fan out before merging)");
  if (idx->ov) return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "fanout: overlay snapshot (subscribers need a rebuild)");
  std::memset(out, 0, sizeof(*out));
  GM_GUARD_BEGIN
  hipSetDevice(ctx->device);
  if (idx->route) {  // a sharded index: each row on the shard of its filters (gm_shard.cpp)
    if ((flags & EMQX_GM_DEVICE_IO) || m->on_device)
      return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "fanout: sharded index takes host rows");
    // (built without subscriber lists -- the updatable form: no deliveries, as a plain index gives)
    return noted(ctx, ctx, gm::run_fanout_sharded(ctx, idx, m, flags, out));
  }
  if (!ctx->members.empty() && !(flags & EMQX_GM_DEVICE_IO) && !m->on_device)
    return noted(ctx, ctx, gm::run_fanout_multi(ctx, idx, m, flags, out));
  return noted(ctx, ctx, gm::run_fanout(ctx, idx, m, flags, out));
  GM_GUARD_END(ctx)
}

int emqx_gm_match_fanout(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint8_t* tb, const uint64_t* to, uint64_t n,
                         uint32_t flags, emqx_gm_csr* matches, emqx_gm_csr* deliveries) {
  if (!ctx) return EMQX_GM_EINVAL;
  if (!idx || !matches || !deliveries || (n && (!tb || !to)))
    return gm::set_err(ctx, EMQX_GM_EINVAL, "match_fanout: NULL argument");
  if (flags & ~EMQX_GM_WITH_EXACT) return gm::set_err(ctx, EMQX_GM_EINVAL, "match_fanout: flags (host buffers only)");
  if (n >= 0xFFFFFFF0ull) return gm::set_err(ctx, EMQX_GM_EINVAL, "match_fanout: batch too large (>= 2^32 topics)");
  if (idx->device != ctx->device) return gm::set_err(ctx, EMQX_GM_EINVAL, "match_fanout: index lives on another device");
  std::memset(matches, 0, sizeof(*matches));
  std::memset(deliveries, 0, sizeof(*deliveries));
  int rc = EMQX_GM_OK;
  bool fused = false;
  gm::SmallFan fan;
  GM_GUARD_BEGIN
  // a publish window: the fan-out rides the match's one device round trip
  // (gm_host.cpp run_host_small); otherwise, or when its speculation did not
  // hold, the two calls one after the other
  if (small_call(idx, to, n, flags) && !idx->view.gmap && !idx->subs.empty() && !gm::knob("GM_FANOUT_SIMPLE")) {
    rc = match_small(ctx, idx, tb, to, n, flags, matches, &fan);
    if (rc != EMQX_GM_OK) return rc;
    if (fan.ok) {
      *deliveries = fan.out;
      fused = true;
    }
  } else {
    rc = emqx_gm_match(ctx, idx, tb, to, n, flags, matches);
    if (rc != EMQX_GM_OK) return rc;
  }
  GM_GUARD_END(ctx)
  if (fused) return EMQX_GM_OK;
  if (gm::knob("GM_FANOUT_FUSED_ONLY")) {  // (tests: the fused form must have held)
    emqx_gm_csr_free(ctx, matches);
    return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED,
                       "match_fanout: not fused (queued " + std::to_string(fan.queued) + ", speculative rows " +
                           std::to_string(fan.rows_spec) + ", deliveries " + std::to_string(fan.total) + " of " +
                           std::to_string(fan.cap) + ")");
  }
  rc = emqx_gm_fanout(ctx, idx, matches, 0, deliveries);
  if (rc != EMQX_GM_OK) emqx_gm_csr_free(ctx, matches);  // (the error message stays the fan-out's)
  return rc;
}


// ---- a whole publish window in one device round trip (gm_publish.hip) ----
int emqx_gm_publish_result_free(emqx_gm_ctx* ctx, emqx_gm_publish_result* res) {
  if (!ctx || !res) return EMQX_GM_EINVAL;
  for (emqx_gm_csr* c : {&res->matches, &res->deliveries, &res->pick_members, &res->pick_slots})
    if (c->row_off || c->ids) emqx_gm_csr_free(ctx, c);
  if (res->forwards.node_off || res->forwards.rows || res->forwards.filters || res->forwards.row_routes)
    emqx_gm_forwards_free(ctx, &res->forwards);
  std::memset(res, 0, sizeof(*res));
  return EMQX_GM_OK;
}

// every argument of a publish window checked before any device work, no output touched
static int publish_window_check(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint8_t* tb, const uint64_t* to,
                                uint64_t n, const emqx_gm_publish_opts* o, emqx_gm_publish_result* out) {
  if (!idx || !o || !out || (n && (!tb || !to)))
    return gm::set_err(ctx, EMQX_GM_EINVAL, "publish_window: NULL argument");
  if (o->flags & ~EMQX_GM_WITH_EXACT)
    return gm::set_err(ctx, EMQX_GM_EINVAL, "publish_window: flags (host buffers only)");
  if (n >= 0xFFFFFFF0ull) return gm::set_err(ctx, EMQX_GM_EINVAL, "publish_window: batch too large (>= 2^32 topics)");
  if (idx->device != ctx->device)
    return gm::set_err(ctx, EMQX_GM_EINVAL, "publish_window: index lives on another device");
  for (uint64_t i = 0; i < n; ++i)
    if (to[i + 1] < to[i]) return gm::set_err(ctx, EMQX_GM_EINVAL, "publish_window: topic offsets not monotone");
  if (emqx_gm_shared* sh = o->shared) {
    if (o->strategy > EMQX_GM_SHARE_RANDOM) return gm::set_err(ctx, EMQX_GM_EINVAL, "publish_window: strategy");
    if (!sh->dev_base) return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "publish_window: a host-only shared table");
    if (sh->device != ctx->device)
      return gm::set_err(ctx, EMQX_GM_EINVAL, "publish_window: the shared table is on another device");
    if (sh->idx != idx)
      return gm::set_err(ctx, EMQX_GM_EINVAL, "publish_window: the shared table is bound to another snapshot");
    if (o->strategy == EMQX_GM_SHARE_HASH && !o->msg_hash && n)
      return gm::set_err(ctx, EMQX_GM_EINVAL, "publish_window: msg_hash is required for EMQX_GM_SHARE_HASH");
  }
  if (emqx_gm_dests* dt = o->dests) {
    if (!dt->dev_base) return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "publish_window: a host-only dests table");
    if (dt->device != ctx->device)
      return gm::set_err(ctx, EMQX_GM_EINVAL, "publish_window: the dests table is on another device");
    if (dt->idx != idx)
      return gm::set_err(ctx, EMQX_GM_EINVAL, "publish_window: the dests table is bound to another snapshot");
  }
  return EMQX_GM_OK;
}

int emqx_gm_publish_window(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint8_t* tb, const uint64_t* to,
                           uint64_t n, const emqx_gm_publish_opts* o, emqx_gm_publish_result* out,
                           emqx_gm_publish_stats* stats) {
  if (!ctx) return EMQX_GM_EINVAL;
  if (const int crc = publish_window_check(ctx, idx, tb, to, n, o, out)) return crc;
  std::memset(out, 0, sizeof(*out));
  emqx_gm_publish_stats st{};
  int rc = EMQX_GM_OK;
  auto fail = [&](int code) {  // every output zeroed, nothing held (the failing call's message stays)
    emqx_gm_publish_result_free(ctx, out);
    return code;
  };
  GM_GUARD_BEGIN
  if (small_call(idx, to, n, o->flags) && !idx->view.gmap && !idx->subs.empty() && !gm::knob("GM_FANOUT_SIMPLE")) {
    // the window whole on this context's own device (the first listed: it holds the side tables)
    gm::PwArgs a;
    a.sh = o->shared;
    a.strategy = o->strategy;
    a.seed = o->seed;
    a.msg_hash = o->msg_hash;
    a.dt = o->dests;
    a.skip_node = o->skip_node;
    gm::SmallFan fan;
    emqx_gm_match_stats ms{};
    hipSetDevice(ctx->device);
    rc = gm::run_publish_window(ctx, idx, tb, to, n, o->flags, a, out, &st, &ms, &fan);
    if (rc != EMQX_GM_OK) return fail(rc);
    tl_stats = ms;
    tl_stats_ctx = ctx;
    if (fan.ok) {
      out->deliveries = fan.out;
      st.fanout_spec = 1;
    } else {  // (emqx_gm_match_fanout's rule: the fan-out of the returned rows)
      rc = emqx_gm_fanout(ctx, idx, &out->matches, 0, &out->deliveries);
      if (rc != EMQX_GM_OK) return fail(rc);
      st.device_waits += 1;
    }
  } else {  // not a one-round-trip window: the three calls in sequence (their waits are not counted)
    rc = emqx_gm_match_fanout(ctx, idx, tb, to, n, o->flags, &out->matches, &out->deliveries);
    if (rc != EMQX_GM_OK) return fail(rc);
    if (o->shared) {
      rc = emqx_gm_shared_pick(ctx, o->shared, &out->matches, o->strategy, o->msg_hash, o->seed, &out->pick_members,
                               &out->pick_slots);
      if (rc != EMQX_GM_OK) return fail(rc);
      st.n_hits = out->pick_members.nnz;
    }
    if (o->dests) {
      rc = emqx_gm_forward_plan(ctx, o->dests, &out->matches, o->skip_node, &out->forwards);
      if (rc != EMQX_GM_OK) return fail(rc);
      st.n_pairs = out->forwards.n_pairs;
    }
  }
  GM_GUARD_END(ctx)
  if (stats) *stats = st;
  return EMQX_GM_OK;
}

// ---- ... with the deliveries' option bytes as a third speculative part, in
// place of the plain fan-out (gm_publish.hip, gm_subopts.hip so_queue_spec) ----
int emqx_gm_publish_window_deliver(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const uint8_t* tb, const uint64_t* to,
                                   uint64_t n, const emqx_gm_publish_opts* o, const emqx_gm_publish_deliver_opts* d,
                                   emqx_gm_publish_result* out, emqx_gm_deliveries* deliv,
                                   emqx_gm_publish_deliver_stats* stats) {
  if (!ctx) return EMQX_GM_EINVAL;
  if (const int crc = publish_window_check(ctx, idx, tb, to, n, o, out)) return crc;
  if (!d || !deliv || !d->subopts || (n && (!d->msg_flags || !d->msg_from)))
    return gm::set_err(ctx, EMQX_GM_EINVAL, "publish_window_deliver: NULL argument");
  if (d->mode != EMQX_GM_SO_FLAG && d->mode != EMQX_GM_SO_DROP)
    return gm::set_err(ctx, EMQX_GM_EINVAL, "publish_window_deliver: mode");
  emqx_gm_subopts* so = d->subopts;
  if (!so->dev_base) return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "publish_window_deliver: a host-only table");
  if (so->device != ctx->device)
    return gm::set_err(ctx, EMQX_GM_EINVAL, "publish_window_deliver: the table is on another device");
  if (so->idx != idx)
    return gm::set_err(ctx, EMQX_GM_EINVAL, "publish_window_deliver: the table is bound to another snapshot");
  for (uint64_t r = 0; r < n; ++r)
    if (gm::so_bad_msg(d->msg_flags[r]))
      return gm::set_err(ctx, EMQX_GM_EINVAL, "publish_window_deliver: msg_flags[" + std::to_string(r) + "] = " +
                                                  std::to_string(d->msg_flags[r]));
  std::memset(out, 0, sizeof(*out));
  std::memset(deliv, 0, sizeof(*deliv));
  emqx_gm_publish_deliver_stats st{};
  int rc = EMQX_GM_OK;
  auto fail = [&](int code) {  // every output zeroed, nothing held (the failing call's message stays)
    emqx_gm_publish_result_free(ctx, out);
    if (deliv->deliveries.row_off || deliv->deliveries.ids || deliv->dopt || deliv->row_dropped)
      emqx_gm_deliveries_free(ctx, deliv);
    std::memset(deliv, 0, sizeof(*deliv));
    return code;
  };
  GM_GUARD_BEGIN
  if (small_call(idx, to, n, o->flags) && !idx->view.gmap && !idx->subs.empty() && !gm::knob("GM_FANOUT_SIMPLE")) {
    gm::PwArgs a;
    a.sh = o->shared;
    a.strategy = o->strategy;
    a.seed = o->seed;
    a.msg_hash = o->msg_hash;
    a.dt = o->dests;
    a.skip_node = o->skip_node;
    a.so = so;
    a.msg_flags = d->msg_flags;
    a.msg_from = d->msg_from;
    a.so_mode = d->mode;
    gm::PwDeliv dl;
    emqx_gm_match_stats ms{};
    hipSetDevice(ctx->device);
    rc = gm::run_publish_window(ctx, idx, tb, to, n, o->flags, a, out, &st.window, &ms, nullptr, &dl);
    if (rc != EMQX_GM_OK) return fail(rc);
    tl_stats = ms;
    tl_stats_ctx = ctx;
    *deliv = dl.out;
    st.deliveries_spec = dl.spec;
    st.cap_deliveries = dl.cap;
  } else {  // not a one-round-trip window: the calls in sequence (their waits are not counted)
    rc = emqx_gm_match(ctx, idx, tb, to, n, o->flags, &out->matches);
    if (rc != EMQX_GM_OK) return fail(rc);
    if (o->shared) {
      rc = emqx_gm_shared_pick(ctx, o->shared, &out->matches, o->strategy, o->msg_hash, o->seed, &out->pick_members,
                               &out->pick_slots);
      if (rc != EMQX_GM_OK) return fail(rc);
      st.window.n_hits = out->pick_members.nnz;
    }
    if (o->dests) {
      rc = emqx_gm_forward_plan(ctx, o->dests, &out->matches, o->skip_node, &out->forwards);
      if (rc != EMQX_GM_OK) return fail(rc);
      st.window.n_pairs = out->forwards.n_pairs;
    }
    rc = emqx_gm_deliver(ctx, so, &out->matches, d->msg_flags, d->msg_from, d->mode, deliv);
    if (rc != EMQX_GM_OK) return fail(rc);
  }
  st.n_deliveries = deliv->deliveries.nnz;
  st.n_dropped = deliv->n_dropped;
  GM_GUARD_END(ctx)
  if (stats) *stats = st;
  return EMQX_GM_OK;
}

// ---- publish windows coalesced into one device round trip (emqx_gm_match_windows,
// emqx_gm_combiner): every scheduler of a node publishes at once
// (apps/emqx/src/emqx_broker.erl:204-215, 296-322, emqx_trie.erl:66-70), each
// with a window too small to fill the device; a group of them runs as one
// batch (gm_host.cpp run_host_windows, gm_windows.hip k_rows_split) ----
namespace {
constexpr uint32_t kGroupWindows = 64, kGroupWindowsMax = 256;

// 0: offsets not monotone; 1: the window runs alone through the ordinary call
// (not a small call, a topic past 65,535 B, more than the mapped text limit); 2: it may join a group
int window_kind(const emqx_gm_index* idx, const emqx_gm_window& w, uint32_t flags, bool fan) {
  uint64_t lng = 0;
  for (uint64_t i = 0; i < w.n_topics; ++i) {
    if (w.topic_off[i + 1] < w.topic_off[i]) return 0;
    lng |= (w.topic_off[i + 1] - w.topic_off[i]) >> 16;
  }
  if (lng || !small_call(idx, w.topic_off, w.n_topics, flags)) return 1;
  if (w.n_topics && w.topic_off[w.n_topics] - w.topic_off[0] > gm::host_window_text_max()) return 1;
  if (fan && (idx->view.gmap || idx->subs.empty() || gm::knob("GM_FANOUT_SIMPLE"))) return 1;
  return 2;
}

// the windows in order: groups through run_host_windows (one member device
// each, round-robin as match_small picks), the others alone; arguments checked
// by the caller, kind[k] from window_kind.  The calling thread's stats
// (emqx_gm_last_stats) are those of the last group or call.
int match_windows_loop(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const emqx_gm_window* w, uint32_t nw,
                       const std::vector<int>& kind, uint32_t flags, emqx_gm_csr* m, emqx_gm_csr* d,
                       uint32_t max_windows, uint64_t max_topics) {
  int rc = EMQX_GM_OK;
  GM_GUARD_BEGIN
  std::vector<uint8_t> ok;
  for (uint32_t k = 0; k < nw && rc == EMQX_GM_OK;) {
    if (kind[k] != 2) {
      rc = d ? emqx_gm_match_fanout(ctx, idx, w[k].topic_bytes, w[k].topic_off, w[k].n_topics, flags, &m[k], &d[k])
             : emqx_gm_match(ctx, idx, w[k].topic_bytes, w[k].topic_off, w[k].n_topics, flags, &m[k]);
      ++k;
      continue;
    }
    uint32_t e = k;
    uint64_t topics = 0, bytes = 0;
    for (; e < nw && e - k < max_windows && kind[e] == 2; ++e) {
      const uint64_t nb = w[e].n_topics ? w[e].topic_off[w[e].n_topics] - w[e].topic_off[0] : 0;
      if (e > k && (topics + w[e].n_topics > max_topics || bytes + nb > gm::host_window_text_max())) break;
      topics += w[e].n_topics;
      bytes += nb;
    }
    const size_t K = 1 + (idx->reps.size() == ctx->members.size() ? ctx->members.size() : 0);
    const size_t pick = K > 1 ? ctx->rr.fetch_add(1, std::memory_order_relaxed) % K : 0;
    emqx_gm_ctx* mc = pick ? ctx->members[pick - 1] : ctx;
    const emqx_gm_index* rix = pick ? idx->reps[pick - 1] : idx;
    hipSetDevice(mc->device);
    ok.assign(e - k, 0);
    emqx_gm_match_stats st{};
    rc = gm::run_host_windows(mc, rix, w + k, e - k, flags, m + k, d ? d + k : nullptr, ok.data(), &st);
    if (rc == EMQX_GM_OK) {
      tl_stats = st;
      tl_stats_ctx = ctx;
    }
    hipSetDevice(ctx->device);
    // (a window whose deliveries did not hold: today's rule, the fan-out of its rows)
    for (uint32_t j = k; d && j < e && rc == EMQX_GM_OK; ++j)
      if (!ok[j - k]) rc = emqx_gm_fanout(ctx, idx, &m[j], 0, &d[j]);
    k = e;
  }
  return rc;
  GM_GUARD_END(ctx)
}

// ... and on any failure (an exception included: it comes back as a code) nothing is returned or held
int match_windows_run(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const emqx_gm_window* w, uint32_t nw,
                      const std::vector<int>& kind, uint32_t flags, emqx_gm_csr* m, emqx_gm_csr* d,
                      uint32_t max_windows, uint64_t max_topics) {
  for (uint32_t k = 0; k < nw; ++k) {
    std::memset(&m[k], 0, sizeof(m[k]));
    if (d) std::memset(&d[k], 0, sizeof(d[k]));
  }
  const int rc = match_windows_loop(ctx, idx, w, nw, kind, flags, m, d, max_windows, max_topics);
  if (rc != EMQX_GM_OK)  // nothing is returned (the failing call's message stays)
    for (uint32_t k = 0; k < nw; ++k) {
      if (m[k].row_off || m[k].ids) emqx_gm_csr_free(ctx, &m[k]);
      if (d && (d[k].row_off || d[k].ids)) emqx_gm_csr_free(ctx, &d[k]);
      std::memset(&m[k], 0, sizeof(m[k]));
      if (d) std::memset(&d[k], 0, sizeof(d[k]));
    }
  return rc;
}
}  // namespace

int emqx_gm_match_windows(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const emqx_gm_window* w, uint32_t n_windows,
                          uint32_t flags, emqx_gm_csr* matches, emqx_gm_csr* deliveries) {
  if (!ctx) return EMQX_GM_EINVAL;
  if (!idx || (n_windows && (!w || !matches))) return gm::set_err(ctx, EMQX_GM_EINVAL, "match_windows: NULL argument");
  if (flags & ~EMQX_GM_WITH_EXACT) return gm::set_err(ctx, EMQX_GM_EINVAL, "match_windows: flags (host buffers only)");
  if (idx->device != ctx->device) return gm::set_err(ctx, EMQX_GM_EINVAL, "match_windows: index lives on another device");
  std::vector<int> kind;
  GM_GUARD_BEGIN
  kind.resize(n_windows);
  for (uint32_t k = 0; k < n_windows; ++k) {
    if (w[k].n_topics && (!w[k].topic_bytes || !w[k].topic_off))
      return gm::set_err(ctx, EMQX_GM_EINVAL, "match_windows: NULL window");
    if (w[k].n_topics >= 0xFFFFFFF0ull) return gm::set_err(ctx, EMQX_GM_EINVAL, "match_windows: window too large");
    if (!(kind[k] = window_kind(idx, w[k], flags, deliveries != nullptr)))
      return gm::set_err(ctx, EMQX_GM_EINVAL, "match_windows: topic offsets not monotone");
  }
  GM_GUARD_END(ctx)
  return match_windows_run(ctx, idx, w, n_windows, kind, flags, matches, deliveries, kGroupWindows,
                           gm::host_chunk_topics());
}

// One caller's window in the combining queue (gm_combine.h): its arguments,
// its outputs, and what its group's leader leaves for it.
namespace {
struct CombCall {
  emqx_gm_window win{};
  int kind = 2;
  emqx_gm_csr* matches = nullptr;
  emqx_gm_csr* deliveries = nullptr;
  emqx_gm_match_stats stats{};  // the group's
  std::string err;              // the leader's message, on failure
  // a whole publish window (emqx_gm_combiner_publish): its hashes, opts and outputs
  const uint32_t* msg_hash = nullptr;
  emqx_gm_publish_opts popts{};
  emqx_gm_publish_result* pres = nullptr;
  emqx_gm_publish_stats pst{};
  emqx_gm_publish_group_stats pgs{};
};
}  // namespace

struct emqx_gm_combiner {
  emqx_gm_ctx* ctx = nullptr;
  uint32_t max_windows = kGroupWindows;
  uint64_t max_topics = 0;
  gm::Combiner* q = nullptr;
  // publish groups: their sequence numbers, and the lock that makes the numbers
  // of groups with a stateful strategy the order in which they run
  std::atomic<uint64_t> seq{0};
  std::mutex order_mu;
  ~emqx_gm_combiner() { delete q; }
};

static int combiner_run_publish(emqx_gm_combiner* cb, gm::CombWindow* const* g, uint32_t n);

// a group of the queue through match_windows_run: the leader's thread runs it
static int combiner_run(emqx_gm_combiner* cb, gm::CombWindow* const* g, uint32_t n) {
  if (g[0]->kind == 1) return combiner_run_publish(cb, g, n);
  emqx_gm_ctx* ctx = cb->ctx;
  const emqx_gm_index* idx = static_cast<const emqx_gm_index*>(g[0]->index);
  const bool fan = g[0]->want_deliveries;
  std::vector<emqx_gm_window> w(n);
  std::vector<int> kind(n);
  std::vector<emqx_gm_csr> m(n), d(fan ? n : 0);
  for (uint32_t k = 0; k < n; ++k) {
    const CombCall* c = static_cast<const CombCall*>(g[k]->user);
    w[k] = c->win;
    kind[k] = c->kind;
  }
  const int rc = match_windows_run(ctx, idx, w.data(), n, kind, g[0]->flags, m.data(), fan ? d.data() : nullptr,
                                   cb->max_windows, cb->max_topics);
  const char* msg = rc != EMQX_GM_OK ? emqx_gm_last_error(ctx) : nullptr;
  for (uint32_t k = 0; k < n; ++k) {
    CombCall* c = static_cast<CombCall*>(g[k]->user);
    g[k]->rc = rc;
    if (rc == EMQX_GM_OK) {
      *c->matches = m[k];
      if (fan) *c->deliveries = d[k];
      c->stats = tl_stats;
    } else if (msg) {
      c->err = msg;
    }
  }
  return 0;
}

int emqx_gm_combiner_open(emqx_gm_ctx* ctx, const emqx_gm_combiner_opts* opts, emqx_gm_combiner** out) {
  if (!ctx) return EMQX_GM_EINVAL;
  if (!out) return gm::set_err(ctx, EMQX_GM_EINVAL, "combiner_open: NULL out");
  *out = nullptr;
  GM_GUARD_BEGIN
  gm::CombinerLimits lim;
  lim.max_topics = gm::host_chunk_topics();
  lim.max_bytes = gm::host_window_text_max();
  if (opts) {
    if (opts->max_windows > kGroupWindowsMax)
      return gm::set_err(ctx, EMQX_GM_EINVAL, "combiner_open: max_windows (at most 256)");
    if (opts->max_windows) lim.max_windows = opts->max_windows;
    if (opts->max_topics) lim.max_topics = std::min<uint64_t>(opts->max_topics, lim.max_topics);
    if (opts->max_in_flight) lim.max_in_flight = opts->max_in_flight;
    if (opts->min_windows) lim.min_windows = opts->min_windows;
    lim.linger_us = opts->linger_us;
  }
  auto* cb = new emqx_gm_combiner;
  cb->ctx = ctx;
  cb->max_windows = lim.max_windows;
  cb->max_topics = lim.max_topics;
  cb->q = new gm::Combiner(lim, [cb](gm::CombWindow* const* g, uint32_t n) { return combiner_run(cb, g, n); });
  {  // (the context owns it: a closed combiner still answers EMQX_GM_EINVAL until emqx_gm_close)
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    ctx->combiners.push_back(cb);
  }
  *out = cb;
  return EMQX_GM_OK;
  GM_GUARD_END(ctx)
}

int emqx_gm_combiner_match(emqx_gm_combiner* cb, const emqx_gm_index* idx, const uint8_t* tb, const uint64_t* to,
                           uint64_t n, uint32_t flags, emqx_gm_csr* matches, emqx_gm_csr* deliveries) {
  if (!cb) return EMQX_GM_EINVAL;
  emqx_gm_ctx* ctx = cb->ctx;
  if (!idx || !matches || (n && (!tb || !to))) return gm::set_err(ctx, EMQX_GM_EINVAL, "combiner_match: NULL argument");
  if (flags & ~EMQX_GM_WITH_EXACT) return gm::set_err(ctx, EMQX_GM_EINVAL, "combiner_match: flags (host buffers only)");
  if (n >= 0xFFFFFFF0ull) return gm::set_err(ctx, EMQX_GM_EINVAL, "combiner_match: batch too large (>= 2^32 topics)");
  if (idx->device != ctx->device) return gm::set_err(ctx, EMQX_GM_EINVAL, "combiner_match: index lives on another device");
  GM_GUARD_BEGIN
  CombCall c;
  c.win = emqx_gm_window{tb, to, n};
  c.matches = matches;
  c.deliveries = deliveries;
  if (!(c.kind = window_kind(idx, c.win, flags, deliveries != nullptr)))
    return gm::set_err(ctx, EMQX_GM_EINVAL, "combiner_match: topic offsets not monotone");
  std::memset(matches, 0, sizeof(*matches));
  if (deliveries) std::memset(deliveries, 0, sizeof(*deliveries));
  gm::CombWindow qw;
  qw.index = idx;
  qw.flags = flags;
  qw.want_deliveries = deliveries != nullptr;
  qw.n_topics = n;
  qw.n_bytes = n ? to[n] - to[0] : 0;
  qw.user = &c;
  const int rc = cb->q->submit(&qw);
  if (rc == EMQX_GM_OK) {  // the group's figures, for this thread's emqx_gm_last_stats
    tl_stats = c.stats;
    tl_stats_ctx = ctx;
    return rc;
  }
  return gm::set_err(ctx, rc, c.err.empty() ? "combiner_match: the combiner is closed" : c.err);
  GM_GUARD_END(ctx)
}

// ---- whole publish windows coalesced into one device round trip
// (emqx_gm_publish_windows, emqx_gm_combiner_publish; gm_publish.hip's group
// stage): the reference's unit of work, emqx_broker:publish/1 -> route/2 per
// message from many publisher processes at once (apps/emqx/src/emqx_broker.erl:
// 204-215, 245-293, 296-322; emqx_shared_sub.erl:113-130), for a node's whole
// scheduler pool ----
namespace {
// what emqx_gm_publish_window checks of the opts and their tables, before any device work
int publish_opts_check(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const emqx_gm_publish_opts* o, const std::string& who) {
  if (o->flags & ~EMQX_GM_WITH_EXACT) return gm::set_err(ctx, EMQX_GM_EINVAL, who + ": flags (host buffers only)");
  if (idx->device != ctx->device) return gm::set_err(ctx, EMQX_GM_EINVAL, who + ": index lives on another device");
  if (const emqx_gm_shared* sh = o->shared) {
    if (o->strategy > EMQX_GM_SHARE_RANDOM) return gm::set_err(ctx, EMQX_GM_EINVAL, who + ": strategy");
    if (!sh->dev_base) return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, who + ": a host-only shared table");
    if (sh->device != ctx->device)
      return gm::set_err(ctx, EMQX_GM_EINVAL, who + ": the shared table is on another device");
    if (sh->idx != idx)
      return gm::set_err(ctx, EMQX_GM_EINVAL, who + ": the shared table is bound to another snapshot");
  }
  if (const emqx_gm_dests* dt = o->dests) {
    if (!dt->dev_base) return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, who + ": a host-only dests table");
    if (dt->device != ctx->device)
      return gm::set_err(ctx, EMQX_GM_EINVAL, who + ": the dests table is on another device");
    if (dt->idx != idx)
      return gm::set_err(ctx, EMQX_GM_EINVAL, who + ": the dests table is bound to another snapshot");
  }
  return EMQX_GM_OK;
}

// 0: bad (the message set), else window_kind's answer
int publish_window_kind(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const emqx_gm_publish_win& w,
                        const emqx_gm_publish_opts* o, const std::string& who) {
  if (w.w.n_topics && (!w.w.topic_bytes || !w.w.topic_off)) {
    gm::set_err(ctx, EMQX_GM_EINVAL, who + ": NULL window");
    return 0;
  }
  if (w.w.n_topics >= 0xFFFFFFF0ull) {
    gm::set_err(ctx, EMQX_GM_EINVAL, who + ": batch too large (>= 2^32 topics)");
    return 0;
  }
  if (o->shared && o->strategy == EMQX_GM_SHARE_HASH && w.w.n_topics && !w.msg_hash) {
    gm::set_err(ctx, EMQX_GM_EINVAL, who + ": msg_hash is required for EMQX_GM_SHARE_HASH");
    return 0;
  }
  const int kind = window_kind(idx, w.w, o->flags, true);
  if (!kind) gm::set_err(ctx, EMQX_GM_EINVAL, who + ": topic offsets not monotone");
  return kind;
}

// the windows in order: groups through the group stage on this context's own
// device (the first listed: it holds the side tables), the others alone through
// emqx_gm_publish_window, in their place; arguments checked by the caller.
// seq numbers the groups (a window alone is a group of one); with `order` (a
// combiner) a group with a stateful strategy holds it from taking its number
// until it has run, so the numbers are the order of the groups on the table.
int publish_windows_loop(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const emqx_gm_publish_win* w, uint32_t nw,
                         const std::vector<int>& kind, const emqx_gm_publish_opts* o, emqx_gm_publish_result* out,
                         emqx_gm_publish_stats* st, emqx_gm_publish_group_stats* gs, uint32_t max_windows,
                         uint64_t max_topics, std::atomic<uint64_t>* seq, std::mutex* order) {
  int rc = EMQX_GM_OK;
  GM_GUARD_BEGIN
  const bool stateful =
      o->shared && (o->strategy == EMQX_GM_SHARE_ROUND_ROBIN || o->strategy == EMQX_GM_SHARE_STICKY);
  std::vector<uint8_t> ok;
  for (uint32_t k = 0; k < nw && rc == EMQX_GM_OK;) {
    std::unique_lock<std::mutex> ol;
    if (order && stateful) ol = std::unique_lock<std::mutex>(*order);
    const uint64_t sq = seq->fetch_add(1, std::memory_order_relaxed);
    if (kind[k] != 2) {
      emqx_gm_publish_opts o1 = *o;
      o1.msg_hash = w[k].msg_hash;
      rc = emqx_gm_publish_window(ctx, idx, w[k].w.topic_bytes, w[k].w.topic_off, w[k].w.n_topics, &o1, &out[k], &st[k]);
      emqx_gm_publish_group_stats q{};
      q.seq = sq;
      q.n_windows = 1;
      q.device_waits = st[k].device_waits;
      q.rows_spec = st[k].rows_spec;
      q.picks_spec = st[k].picks_spec;
      q.forwards_spec = st[k].forwards_spec;
      q.cap_hits = st[k].cap_hits;
      q.cap_pairs = st[k].cap_pairs;
      q.n_hits = st[k].n_hits;
      q.n_pairs = st[k].n_pairs;
      gs[k] = q;
      ++k;
      continue;
    }
    uint32_t e = k;
    uint64_t topics = 0, bytes = 0;
    for (; e < nw && e - k < max_windows && kind[e] == 2; ++e) {
      const uint64_t nb = w[e].w.n_topics ? w[e].w.topic_off[w[e].w.n_topics] - w[e].w.topic_off[0] : 0;
      if (e > k && (topics + w[e].w.n_topics > max_topics || bytes + nb > gm::host_window_text_max())) break;
      topics += w[e].w.n_topics;
      bytes += nb;
    }
    gm::PwArgs a;
    a.sh = o->shared;
    a.strategy = o->strategy;
    a.seed = o->seed;
    a.dt = o->dests;
    a.skip_node = o->skip_node;
    ok.assign(e - k, 0);
    emqx_gm_match_stats ms{};
    hipSetDevice(ctx->device);
    rc = gm::run_publish_windows(ctx, idx, w + k, e - k, o->flags, a, out + k, st + k, gs + k, ok.data(), &ms);
    if (rc == EMQX_GM_OK) {
      tl_stats = ms;
      tl_stats_ctx = ctx;
    }
    for (uint32_t j = k; j < e && rc == EMQX_GM_OK; ++j) {
      gs[j].seq = sq;
      if (ok[j - k]) continue;
      // (a window whose deliveries did not hold: emqx_gm_match_fanout's rule, the fan-out of its rows)
      rc = emqx_gm_fanout(ctx, idx, &out[j].matches, 0, &out[j].deliveries);
      st[j].device_waits += 1;
    }
    k = e;
  }
  return rc;
  GM_GUARD_END(ctx)
}

// ... and on any failure (an exception included) every output is zeroed and nothing is held
int publish_windows_run(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const emqx_gm_publish_win* w, uint32_t nw,
                        const std::vector<int>& kind, const emqx_gm_publish_opts* o, emqx_gm_publish_result* out,
                        emqx_gm_publish_stats* st, emqx_gm_publish_group_stats* gs, uint32_t max_windows,
                        uint64_t max_topics, std::atomic<uint64_t>* seq, std::mutex* order) {
  for (uint32_t k = 0; k < nw; ++k) {
    std::memset(&out[k], 0, sizeof(out[k]));
    st[k] = emqx_gm_publish_stats{};
    gs[k] = emqx_gm_publish_group_stats{};
  }
  const int rc = publish_windows_loop(ctx, idx, w, nw, kind, o, out, st, gs, max_windows, max_topics, seq, order);
  if (rc != EMQX_GM_OK)
    for (uint32_t k = 0; k < nw; ++k) emqx_gm_publish_result_free(ctx, &out[k]);
  return rc;
}
}  // namespace

int emqx_gm_publish_windows(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const emqx_gm_publish_win* w, uint32_t nw,
                            const emqx_gm_publish_opts* o, emqx_gm_publish_result* out, emqx_gm_publish_stats* stats,
                            emqx_gm_publish_group_stats* gstats) {
  if (!ctx) return EMQX_GM_EINVAL;
  // every argument checked before any device work, no output touched
  if (!idx || !o || (nw && (!w || !out))) return gm::set_err(ctx, EMQX_GM_EINVAL, "publish_windows: NULL argument");
  if (o->msg_hash)
    return gm::set_err(ctx, EMQX_GM_EINVAL, "publish_windows: opts->msg_hash must be NULL (each window brings its own)");
  std::vector<int> kind;
  std::vector<emqx_gm_publish_stats> st;
  std::vector<emqx_gm_publish_group_stats> gs;
  GM_GUARD_BEGIN
  if (const int rc = publish_opts_check(ctx, idx, o, "publish_windows")) return rc;
  kind.resize(nw);
  for (uint32_t k = 0; k < nw; ++k)
    if (!(kind[k] = publish_window_kind(ctx, idx, w[k], o, "publish_windows"))) return EMQX_GM_EINVAL;
  if (!stats) st.resize(nw);
  if (!gstats) gs.resize(nw);
  GM_GUARD_END(ctx)
  std::atomic<uint64_t> seq{0};
  return publish_windows_run(ctx, idx, w, nw, kind, o, out, stats ? stats : st.data(), gstats ? gstats : gs.data(),
                             kGroupWindows, gm::host_chunk_topics(), &seq, nullptr);
}

// a group of publish windows of the queue through publish_windows_run: the leader's thread runs it
static int combiner_run_publish(emqx_gm_combiner* cb, gm::CombWindow* const* g, uint32_t n) {
  emqx_gm_ctx* ctx = cb->ctx;
  const emqx_gm_index* idx = static_cast<const emqx_gm_index*>(g[0]->index);
  std::vector<emqx_gm_publish_win> w(n);
  std::vector<int> kind(n);
  std::vector<emqx_gm_publish_result> res(n);
  std::vector<emqx_gm_publish_stats> st(n);
  std::vector<emqx_gm_publish_group_stats> gs(n);
  for (uint32_t k = 0; k < n; ++k) {
    const CombCall* c = static_cast<const CombCall*>(g[k]->user);
    w[k].w = c->win;
    w[k].msg_hash = c->msg_hash;
    kind[k] = c->kind;
  }
  emqx_gm_publish_opts o = static_cast<const CombCall*>(g[0]->user)->popts;  // (the group's key: every member's are these)
  o.msg_hash = nullptr;
  const int rc = publish_windows_run(ctx, idx, w.data(), n, kind, &o, res.data(), st.data(), gs.data(), cb->max_windows,
                                     cb->max_topics, &cb->seq, &cb->order_mu);
  const char* msg = rc != EMQX_GM_OK ? emqx_gm_last_error(ctx) : nullptr;
  for (uint32_t k = 0; k < n; ++k) {
    CombCall* c = static_cast<CombCall*>(g[k]->user);
    g[k]->rc = rc;
    if (rc == EMQX_GM_OK) {
      *c->pres = res[k];
      c->pst = st[k];
      c->pgs = gs[k];
      c->stats = tl_stats;
    } else if (msg) {
      c->err = msg;
    }
  }
  return 0;
}

int emqx_gm_combiner_publish(emqx_gm_combiner* cb, const emqx_gm_index* idx, const uint8_t* tb, const uint64_t* to,
                             uint64_t n, const emqx_gm_publish_opts* o, emqx_gm_publish_result* out,
                             emqx_gm_publish_stats* stats, emqx_gm_publish_group_stats* where) {
  if (!cb) return EMQX_GM_EINVAL;
  emqx_gm_ctx* ctx = cb->ctx;
  // the caller's own window checked here: a bad one fails this call alone, no output touched
  if (!idx || !o || !out || (n && (!tb || !to)))
    return gm::set_err(ctx, EMQX_GM_EINVAL, "combiner_publish: NULL argument");
  GM_GUARD_BEGIN
  if (const int rc = publish_opts_check(ctx, idx, o, "combiner_publish")) return rc;
  CombCall c;
  c.win = emqx_gm_window{tb, to, n};
  c.msg_hash = o->msg_hash;
  c.popts = *o;
  c.pres = out;
  const emqx_gm_publish_win pw{c.win, c.msg_hash};
  if (!(c.kind = publish_window_kind(ctx, idx, pw, o, "combiner_publish"))) return EMQX_GM_EINVAL;
  std::memset(out, 0, sizeof(*out));
  gm::CombWindow qw;
  qw.index = idx;
  qw.flags = o->flags;
  qw.want_deliveries = true;
  qw.kind = 1;
  qw.shared = o->shared;
  qw.dests = o->dests;
  qw.strategy = o->shared ? o->strategy : 0;
  qw.seed = o->shared ? o->seed : 0;
  qw.skip_node = o->dests ? o->skip_node : 0;
  qw.n_topics = n;
  qw.n_bytes = n ? to[n] - to[0] : 0;
  qw.user = &c;
  const int rc = cb->q->submit(&qw);
  if (rc == EMQX_GM_OK) {
    if (stats) *stats = c.pst;
    if (where) *where = c.pgs;
    tl_stats = c.stats;
    tl_stats_ctx = ctx;
    return rc;
  }
  return gm::set_err(ctx, rc, c.err.empty() ? "combiner_publish: the combiner is closed" : c.err);
  GM_GUARD_END(ctx)
}

int emqx_gm_combiner_stats(const emqx_gm_combiner* cb, emqx_gm_combiner_stats_t* stats) {
  if (!cb || !stats) return EMQX_GM_EINVAL;
  const gm::CombinerCounts c = cb->q->counts();
  stats->windows = c.windows;
  stats->groups = c.groups;
  stats->max_group = c.max_group;
  stats->solo = c.solo;
  return EMQX_GM_OK;
}

int emqx_gm_combiner_close(emqx_gm_combiner* cb) {
  if (!cb) return EMQX_GM_EINVAL;
  cb->q->close();
  return EMQX_GM_OK;
}

}  // extern "C"
namespace gm {
void free_combiners(emqx_gm_ctx* ctx) {
  for (emqx_gm_combiner* cb : ctx->combiners) {
    cb->q->close();
    delete cb;
  }
  ctx->combiners.clear();
}
}  // namespace gm
extern "C" {

int emqx_gm_fanout_part(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const emqx_gm_csr* m, uint32_t part,
                        uint32_t n_parts, uint32_t flags, emqx_gm_csr* out, uint64_t* first) {
  if (!ctx) return EMQX_GM_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  if (!idx || !m || !out || (m->nnz && !m->ids) || !m->row_off)
    return gm::set_err(ctx, EMQX_GM_EINVAL, "fanout_part: NULL argument");
  if (!n_parts || part >= n_parts) return gm::set_err(ctx, EMQX_GM_EINVAL, "fanout_part: part out of range");
  if (flags & ~(EMQX_GM_WITH_EXACT | EMQX_GM_DEVICE_IO))
    return gm::set_err(ctx, EMQX_GM_EINVAL, "fanout_part: flags");
  if (idx->view.gmap) return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "fanout_part: shard index");
  if (idx->ov) return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "fanout_part: overlay snapshot");
  if (idx->route) return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "fanout_part: sharded index");
  std::memset(out, 0, sizeof(*out));
  GM_GUARD_BEGIN
  hipSetDevice(ctx->device);
  return noted(ctx, ctx, gm::run_fanout(ctx, idx, m, flags, out, part, n_parts, first));
  GM_GUARD_END(ctx)
}

int emqx_gm_csr_free(emqx_gm_ctx* ctx, emqx_gm_csr* csr) {
  if (!ctx || !csr) return EMQX_GM_EINVAL;
  // a result CSR records its context (priv): its buffers belong to that
  // context's pools, and handing them to another one would corrupt both; a
  // small call's rows belong to the member device that served it
  if (csr->priv && csr->priv != static_cast<void*>(ctx)) {
    emqx_gm_ctx* owner = nullptr;
    for (emqx_gm_ctx* m : ctx->members)
      if (csr->priv == static_cast<void*>(m)) owner = m;
    if (!owner) return gm::set_err(ctx, EMQX_GM_EINVAL, "csr_free: the CSR belongs to another context");
    ctx = owner;
  }
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  if (csr->on_device) {
    // back to the pool once the work queued so far (which may still read the
    // rows: a fan-out, a later call's inputs) is done -- no wait here, so a
    // caller with the next call in flight keeps it in flight
    hipSetDevice(ctx->device);
    void* const bufs[2] = {csr->row_off, csr->ids};
    ctx->pool->release_after(bufs, 2, ctx->stream);
  } else {
    ctx->hpool->release(csr->row_off);
    ctx->hpool->release(csr->ids);
  }
  std::memset(csr, 0, sizeof(*csr));
  return EMQX_GM_OK;
}

int emqx_gm_last_stats(const emqx_gm_ctx* ctx, emqx_gm_match_stats* stats) {
  if (!ctx || !stats) return EMQX_GM_EINVAL;
  *stats = tl_stats_ctx == ctx ? tl_stats : ctx->stats;
  return EMQX_GM_OK;
}

int emqx_gm_last_update_stats(const emqx_gm_ctx* ctx, emqx_gm_update_stats* stats) {
  if (!ctx || !stats) return EMQX_GM_EINVAL;
  *stats = gm::tl_ustats;
  return EMQX_GM_OK;
}

int emqx_gm_last_shard_update(const emqx_gm_ctx* ctx, uint32_t* kinds, uint32_t* n) {
  if (!ctx || !n) return EMQX_GM_EINVAL;
  const std::vector<uint32_t>& k = gm::last_shard_kinds();
  if (kinds)
    for (uint32_t i = 0; i < *n && i < k.size(); ++i) kinds[i] = k[i];
  *n = uint32_t(k.size());
  return EMQX_GM_OK;
}

int emqx_gm_index_replica_digest(emqx_gm_ctx* ctx, const emqx_gm_index* idx, uint32_t k, uint64_t* tables,
                                 uint64_t* subs) {
  if (!ctx || !idx || !tables || !subs) return EMQX_GM_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  if (k > idx->reps.size()) return gm::set_err(ctx, EMQX_GM_EINVAL, "replica_digest: no such replica");
  const emqx_gm_index* r = k ? idx->reps[k - 1] : idx;
  GM_GUARD_BEGIN
  auto fnv = [](uint64_t h, const std::vector<uint8_t>& b) {
    for (uint8_t x : b) h = (h ^ x) * 0x100000001B3ull;
    return h;
  };
  hipSetDevice(r->device);
  std::vector<uint8_t> b(r->dev_bytes);
  if (!b.empty()) GM_HIP(ctx, hipMemcpy(b.data(), r->dev_base, b.size(), hipMemcpyDeviceToHost));
  *tables = fnv(0xCBF29CE484222325ull, b);
  *subs = 0;
  if (r->view.sub_off) {
    const uint64_t nf = r->info.n_filters;
    std::vector<uint8_t> o((nf + 1) * 8);
    GM_HIP(ctx, hipMemcpy(o.data(), r->view.sub_off, o.size(), hipMemcpyDeviceToHost));
    uint64_t total = 0;
    std::memcpy(&total, o.data() + nf * 8, 8);
    std::vector<uint8_t> ids(total * 4);
    if (total) GM_HIP(ctx, hipMemcpy(ids.data(), r->view.sub_ids, ids.size(), hipMemcpyDeviceToHost));
    *subs = fnv(fnv(0xCBF29CE484222325ull, o), ids);
  }
  hipSetDevice(ctx->device);
  return EMQX_GM_OK;
  GM_GUARD_END(ctx)
}

// ---- extensions used by the bench / Python host layer (emqx_gm_ext.h) ----
int emqx_gm_matched_filter_bytes(emqx_gm_ctx* ctx, const emqx_gm_index* idx, const emqx_gm_csr* csr,
                                 uint64_t* out) {
  if (!ctx || !idx || !csr || !out || !csr->on_device) return EMQX_GM_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  if (idx->ov || idx->route) return gm::set_err(ctx, EMQX_GM_EUNSUPPORTED, "matched_filter_bytes: overlay or sharded");
  GM_GUARD_BEGIN
  hipSetDevice(ctx->device);
  return gm::sum_filter_lengths(ctx, idx, csr->ids, csr->nnz, out);
  GM_GUARD_END(ctx)
}

int emqx_gm_index_compile_host(const uint8_t* fb, const uint64_t* fo, uint64_t n, const uint64_t* sub_off,
                               const uint32_t* sub_ids, uint32_t* perm_out, emqx_gm_index_info_t* info) {
  if (!info) return EMQX_GM_EINVAL;
  GM_GUARD_BEGIN
  return gm::build_index(nullptr, fb, fo, n, sub_off, sub_ids, perm_out, nullptr, info);
  GM_GUARD_END(nullptr)
}

// ---- sharded index ----
int emqx_gm_filter_ranks(const uint8_t* fb, const uint64_t* fo, uint64_t n, uint32_t* rank_out, uint64_t* n_unique) {
  if (n && (!fb || !fo || !rank_out)) return EMQX_GM_EINVAL;
  GM_GUARD_BEGIN
  std::vector<uint32_t> ord(n);
  for (uint64_t i = 0; i < n; ++i) ord[i] = uint32_t(i);
  gm::sort_filters(ord, fb, fo);
  uint32_t r = 0;
  for (uint64_t k = 0; k < n; ++k) {
    const uint32_t i = ord[k];
    if (k) {
      const uint32_t p = ord[k - 1];
      const uint64_t lp = fo[p + 1] - fo[p], li = fo[i + 1] - fo[i];
      if (lp != li || std::memcmp(fb + fo[p], fb + fo[i], li) != 0) ++r;
    }
    rank_out[i] = r;
  }
  if (n_unique) *n_unique = n ? uint64_t(r) + 1 : 0;
  return EMQX_GM_OK;
  GM_GUARD_END(nullptr)
}

int emqx_gm_shard_of(const uint8_t* fb, const uint64_t* fo, uint64_t n, uint32_t n_shards, uint32_t* out) {
  if (!n_shards || (n && (!fb || !fo || !out))) return EMQX_GM_EINVAL;
  for (uint64_t i = 0; i < n; ++i)
    out[i] = uint32_t(gm::fmix64(gm::hash_word_host(fb + fo[i], fo[i + 1] - fo[i]) ^ 0x5BD1E995ull) % n_shards);
  return EMQX_GM_OK;
}

int emqx_gm_select_filters(const uint8_t* fb, const uint64_t* fo, uint64_t n, const uint32_t* shard, uint32_t want,
                           uint8_t* out_b, uint64_t* out_o, uint64_t* n_out, uint64_t* bytes_out) {
  if (!n_out || !bytes_out || (n && (!fb || !fo || !shard))) return EMQX_GM_EINVAL;
  uint64_t k = 0, b = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (shard[i] != want) continue;
    const uint64_t len = fo[i + 1] - fo[i];
    if (out_b && out_o) {
      out_o[k] = b;
      std::memcpy(out_b + b, fb + fo[i], len);
    }
    ++k;
    b += len;
  }
  if (out_o) out_o[k] = b;
  *n_out = k;
  *bytes_out = b;
  return EMQX_GM_OK;
}

int emqx_gm_index_build_shard(emqx_gm_ctx* ctx, const uint8_t* fb, const uint64_t* fo, uint64_t n,
                              const uint32_t* global_ids, const uint64_t* sub_off, const uint32_t* sub_ids,
                              uint32_t* perm_out, emqx_gm_index** out) {
  if (!ctx) return EMQX_GM_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  if (n && !global_ids) return gm::set_err(ctx, EMQX_GM_EINVAL, "index_build_shard: global_ids is NULL");
  GM_GUARD_BEGIN
  const double t0 = begin_index_call(EMQX_GM_UPD_BUILD);
  hipSetDevice(ctx->device);
  return replicated(ctx, gm::build_index(ctx, fb, fo, n, sub_off, sub_ids, perm_out, out, nullptr, global_ids),
                    nullptr, out, t0);
  GM_GUARD_END(ctx)
}

int emqx_gm_csr_row_lengths(emqx_gm_ctx* ctx, const emqx_gm_csr* csr, uint32_t* d_lens) {
  if (!ctx) return EMQX_GM_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  if (!csr || !csr->on_device || !d_lens || !csr->row_off)
    return gm::set_err(ctx, EMQX_GM_EINVAL, "csr_row_lengths: needs a device CSR and a device output");
  GM_GUARD_BEGIN
  hipSetDevice(ctx->device);
  return gm::run_row_lengths(ctx, csr, d_lens);
  GM_GUARD_END(ctx)
}

int emqx_gm_merge_rows(emqx_gm_ctx* ctx, uint64_t n_rows, uint64_t stride, uint32_t n_pieces, const uint32_t* d_lens,
                       const uint32_t* d_ids, uint32_t flags, emqx_gm_csr* out) {
  if (!ctx) return EMQX_GM_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  if (!out || stride < n_rows || !n_pieces || (n_rows && (!d_lens || !d_ids)))
    return gm::set_err(ctx, EMQX_GM_EINVAL, "merge_rows: bad arguments");
  if (flags & ~EMQX_GM_DEVICE_IO) return gm::set_err(ctx, EMQX_GM_EINVAL, "merge_rows: flags");
  std::memset(out, 0, sizeof(*out));
  GM_GUARD_BEGIN
  hipSetDevice(ctx->device);
  return gm::run_merge_rows(ctx, n_rows, stride, n_pieces, d_lens, d_ids, flags, out);
  GM_GUARD_END(ctx)
}

// ---- prefix sharding ----
int emqx_gm_prefix_plan(const uint8_t* fb, const uint64_t* fo, uint64_t n, uint32_t n_shards, uint32_t* shard_out,
                        emqx_gm_route** route) {
  if (!route || !n_shards || (n && (!fb || !fo || !shard_out))) return EMQX_GM_EINVAL;
  *route = nullptr;
  GM_GUARD_BEGIN
  return gm::route_plan(fb, fo, n, n_shards, shard_out, route);
  GM_GUARD_END(nullptr)
}

int emqx_gm_route_topics_host(const emqx_gm_route* route, const uint8_t* tb, const uint64_t* to, uint64_t n,
                              uint32_t* dest) {
  if (!route || (n && (!tb || !to || !dest))) return EMQX_GM_EINVAL;
  return gm::route_topics_host(route, tb, to, n, dest);
}

int emqx_gm_route_filter_shards_host(const emqx_gm_route* route, const uint8_t* fb, const uint64_t* fo, uint64_t n,
                                     uint32_t* shard_out) {
  if (!route || (n && (!fb || !fo || !shard_out))) return EMQX_GM_EINVAL;
  return gm::route_filter_shards_host(route, fb, fo, n, shard_out);
}

int emqx_gm_route_topics(emqx_gm_ctx* ctx, emqx_gm_route* route, const uint8_t* d_tb, const uint64_t* d_to, uint64_t n,
                         uint32_t* d_dest) {
  if (!ctx) return EMQX_GM_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  if (!route || (n && (!d_tb || !d_to || !d_dest))) return gm::set_err(ctx, EMQX_GM_EINVAL, "route_topics: NULL argument");
  if (n >= 0xFFFFFFFFull)  // (u32 batch indices: perm, dest)
    return gm::set_err(ctx, EMQX_GM_EINVAL, "route_topics: batch too large (>= 2^32 topics)");
  GM_GUARD_BEGIN
  hipSetDevice(ctx->device);
  return gm::route_topics_device(ctx, route, d_tb, d_to, n, d_dest);
  GM_GUARD_END(ctx)
}

int emqx_gm_route_partition(emqx_gm_ctx* ctx, emqx_gm_route* route, const uint8_t* d_tb, const uint64_t* d_to,
                            uint64_t n, uint32_t* d_perm, uint32_t* d_plen, uint64_t* d_split) {
  if (!ctx) return EMQX_GM_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  if (!route || !d_split || (n && (!d_tb || !d_to || !d_perm || !d_plen)))
    return gm::set_err(ctx, EMQX_GM_EINVAL, "route_partition: NULL argument");
  if (n >= 0xFFFFFFFFull)  // (u32 batch indices: perm, dest)
    return gm::set_err(ctx, EMQX_GM_EINVAL, "route_partition: batch too large (>= 2^32 topics)");
  GM_GUARD_BEGIN
  hipSetDevice(ctx->device);
  return gm::route_partition(ctx, route, d_tb, d_to, n, d_perm, d_plen, d_split);
  GM_GUARD_END(ctx)
}

int emqx_gm_route_release(emqx_gm_route* route) {
  if (!route) return EMQX_GM_EINVAL;
  gm::free_route(route);
  return EMQX_GM_OK;
}

int emqx_gm_permute_topics(emqx_gm_ctx* ctx, const uint8_t* d_tb, const uint64_t* d_to, uint64_t n,
                           const uint32_t* d_perm, uint8_t* d_out, uint64_t* d_out_off) {
  if (!ctx) return EMQX_GM_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  if (!d_out_off || (n && (!d_tb || !d_to || !d_perm || !d_out)))
    return gm::set_err(ctx, EMQX_GM_EINVAL, "permute_topics: NULL argument");
  if (n >= 0xFFFFFFFFull)  // (u32 batch indices: perm, dest)
    return gm::set_err(ctx, EMQX_GM_EINVAL, "permute_topics: batch too large (>= 2^32 topics)");
  GM_GUARD_BEGIN
  hipSetDevice(ctx->device);
  return gm::permute_topics(ctx, d_tb, d_to, n, d_perm, d_out, d_out_off);
  GM_GUARD_END(ctx)
}

int emqx_gm_unpermute_rows(emqx_gm_ctx* ctx, uint64_t n, const uint32_t* d_perm, const uint32_t* d_lens,
                           const uint32_t* d_ids, uint32_t flags, emqx_gm_csr* out) {
  if (!ctx) return EMQX_GM_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  if (!out || (n && (!d_perm || !d_lens || !d_ids)))
    return gm::set_err(ctx, EMQX_GM_EINVAL, "unpermute_rows: NULL argument");
  if (n >= 0xFFFFFFFFull)  // (u32 batch indices: perm, dest)
    return gm::set_err(ctx, EMQX_GM_EINVAL, "unpermute_rows: batch too large (>= 2^32 topics)");
  if (flags & ~EMQX_GM_DEVICE_IO) return gm::set_err(ctx, EMQX_GM_EINVAL, "unpermute_rows: flags");
  std::memset(out, 0, sizeof(*out));
  GM_GUARD_BEGIN
  hipSetDevice(ctx->device);
  return gm::unpermute_rows(ctx, n, d_perm, d_lens, d_ids, flags, out);
  GM_GUARD_END(ctx)
}

int emqx_gm_pool_trim(emqx_gm_ctx* ctx) {
  if (!ctx) return EMQX_GM_EINVAL;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  ctx->pool->trim();
  gm::trim_spare_blob(ctx->device);
  for (emqx_gm_ctx* m : ctx->members) {
    std::lock_guard<std::recursive_mutex> ml(m->mu);  // (small calls hold only a member's lock)
    m->pool->trim();
    gm::trim_spare_blob(m->device);
  }
  return EMQX_GM_OK;
}

}  // extern "C"
