// devmem.hpp -- move-only owners of the library's device, stream-ordered and pinned memory and
// of its events (host drivers only).
//
// A holder releases what it owns when it goes out of scope or is moved over; a failed allocation
// leaves it empty, and an empty holder releases nothing.  Holders convert to the raw pointer
// kernels and entry points take.  Each one counts in hrf_live_allocations() while it owns.
#pragma once
#include <atomic>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "common.hpp"

namespace hrf {

extern std::atomic<int64_t> g_live_allocations;  // chainops.hip

// P: the raw handle (a pointer); Release: hipError_t operator()(P), copyable
template <class P, class Release>
class Holder {
 public:
  Holder() = default;
  Holder(Holder &&o) noexcept : p_(std::exchange(o.p_, nullptr)), rel_(o.rel_) {}
  Holder &operator=(Holder &&o) noexcept {
    if (this != &o) {
      (void)free();
      p_ = std::exchange(o.p_, nullptr);
      rel_ = o.rel_;
    }
    return *this;
  }
  ~Holder() { (void)free(); }
  operator P() const { return p_; }
  // releases now and reports the release's status (the destructor ignores it)
  hipError_t free() {
    if (!p_) return hipSuccess;
    --g_live_allocations;
    return rel_(std::exchange(p_, nullptr));
  }
  // gives the handle up unreleased (process-lifetime tables)
  P release() {
    if (p_) --g_live_allocations;
    return std::exchange(p_, nullptr);
  }

 protected:
  void adopt(P p, Release rel = Release()) {  // on an empty holder
    p_ = p;
    rel_ = rel;
    ++g_live_allocations;
  }
  P p_ = nullptr;
  Release rel_;
};

struct DevRelease {
  hipError_t operator()(void *p) const { return hipFree(p); }
};
struct StreamRelease {
  hipStream_t s = nullptr;
  hipError_t operator()(void *p) const { return hipFreeAsync(p, s); }
};
struct PinnedRelease {
  hipError_t operator()(void *p) const { return hipHostFree(p); }
};
struct EventRelease {
  hipError_t operator()(hipEvent_t e) const { return hipEventDestroy(e); }
};

// hipMalloc / hipFree; count 0 allocates one element
template <class T>
struct DevBuf : Holder<T *, DevRelease> {
  hrf_status alloc(size_t count) {
    (void)this->free();
    void *p = nullptr;
    HRF_HIP(hipMalloc(&p, sizeof(T) * (count ? count : 1)));
    this->adopt((T *)p);
    return HRF_OK;
  }
};

// hipMallocAsync / hipFreeAsync on the same stream.  The release stays stream-ordered: hipFree
// would synchronise the whole device and stall every other tile's stream.  The destructor covers
// early returns; the normal path ends with HRF_HIP(buf.free()) so a failing release is reported.
template <class T>
struct StreamBuf : Holder<T *, StreamRelease> {
  hipError_t alloc(size_t count, hipStream_t s) {
    const hipError_t fe = this->free();
    if (fe != hipSuccess) return fe;
    void *p = nullptr;
    const hipError_t e = hipMallocAsync(&p, sizeof(T) * count, s);
    if (e == hipSuccess) this->adopt((T *)p, StreamRelease{s});
    return e;
  }
};

// mapped, coherent pinned host words (host_alloc_mapped) with their device address; `who` names
// the caller in the error text
struct PinnedBuf : Holder<int32_t *, PinnedRelease> {
  hrf_status alloc(size_t count, const char *who) {
    (void)free();
    void *p = nullptr;
    if (host_alloc_mapped(&p, sizeof(int32_t) * count) == hipSuccess && p) adopt((int32_t *)p);
    if (!(dev_ = mapped(p_))) {  // (nullptr for a null host pointer)
      (void)free();
      set_error("%s: pinned host allocation failed", who);
      return HRF_EHIP;
    }
    return HRF_OK;
  }
  int32_t *dev() const { return p_ ? dev_ : nullptr; }

 private:
  int32_t *dev_ = nullptr;
};

// an event that orders streams (hipEventDisableTiming)
struct Event : Holder<hipEvent_t, EventRelease> {
  hrf_status create() {
    (void)free();
    hipEvent_t e = nullptr;
    HRF_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    adopt(e);
    return HRF_OK;
  }
};

// Per-(device, key) device tables: built on the host on first use, uploaded synchronously and
// kept for the process (so they leave the live count).  A failed upload releases the allocation
// and caches nothing.
template <class Key, class T>
class DeviceTables {
 public:
  template <class Build>  // void build(std::vector<T> &host)
  hrf_status get(const Key &key, Build build, const T **out) {
    int dev = 0;
    HRF_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu_);
    auto it = tabs_.find({dev, key});
    if (it == tabs_.end()) {
      std::vector<T> h;
      build(h);
      DevBuf<T> d;
      HRF_TRY(d.alloc(h.size()));
      HRF_HIP(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
      it = tabs_.emplace(std::make_pair(dev, key), d.release()).first;
    }
    *out = it->second;
    return HRF_OK;
  }

 private:
  std::mutex mu_;
  std::map<std::pair<int, Key>, const T *> tabs_;
};

}  // namespace hrf
