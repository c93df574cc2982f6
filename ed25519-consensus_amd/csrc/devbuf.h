// Move-only owners of device buffers, pinned host buffers, streams and events, and the two
// grow-only "room" helpers of the host API. Nothing here knows about the project.
//
// The allocator is a template policy A:
//   typedef ... err_t;  static constexpr err_t ok;         (ok must be the zero value of err_t)
//   static err_t dev_alloc(void** p, size_t bytes);   static void dev_free(void* p);
//   static err_t host_alloc(void** p, size_t bytes);  static void host_free(void* p);
// HipAlloc (the default) is defined when compiled by hipcc; tests/native/devbuf_main.cpp compiles
// this header as plain host C++ with a malloc-backed policy that can fail on demand.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <utility>

namespace devbuf {

struct HipAlloc;

// One allocation of `cap` elements of T; Pinned: page-locked host memory instead of device memory.
template <typename T, typename A, bool Pinned>
class Buf {
 public:
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
      cap_ = std::exchange(o.cap_, 0);
    }
    return *this;
  }
  ~Buf() { reset(); }

  // Frees what it holds, then allocates `count` elements (0 -> 1). Empty after a failure.
  typename A::err_t alloc(size_t count) {
    reset();
    if (count == 0) count = 1;
    void* q = nullptr;
    const typename A::err_t e = Pinned ? A::host_alloc(&q, count * sizeof(T)) : A::dev_alloc(&q, count * sizeof(T));
    if (e != A::ok) return e;
    p_ = static_cast<T*>(q);
    cap_ = count;
    return e;
  }
  void reset() {
    if (p_) Pinned ? A::host_free(p_) : A::dev_free(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t cap() const { return cap_; }   // elements held

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

template <typename T, typename A = HipAlloc> using DevBuf = Buf<T, A, false>;
template <typename T, typename A = HipAlloc> using PinnedBuf = Buf<T, A, true>;

// ---- capacity policies: how much to allocate for a need of x ----
inline size_t item_cap(size_t n) { return n < 1024 ? 1024 : n + n / 8; }          // per-item arrays
inline size_t byte_cap(size_t b) { return b < 4096 ? 4096 : b + b / 8; }          // byte arenas
inline size_t off_cap(size_t x) { return x < 1024 ? 1024 : x + (x - 1) / 8; }     // x = m + 1 offsets of m items
inline size_t entry_cap(size_t e) { return e + e / 8 + 1024; }                    // MSM digit entries
inline size_t term_cap(size_t t) { return t + t / 8 + 64; }                       // fallback terms / listed items
inline size_t exact_cap(size_t x) { return x; }
inline size_t next_pow2(size_t x) {
  size_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

// ---- growth helpers ----
// Both are grow-only and call sync() (returns the allocator's err_t) before anything is freed: no
// stream may still touch the old memory.

// Room for `need` elements in one buffer; a new allocation holds cap_of(need).
template <typename B, typename Policy, typename Sync>
auto grow(B& b, size_t need, Policy cap_of, Sync sync) -> decltype(sync()) {
  if (b.get() && need <= b.cap()) return decltype(sync()){};
  const auto e = sync();
  if (e != decltype(e){}) return e;
  return b.alloc(cap_of(need));
}

// A group member and its element count for alloc_all.
template <typename B>
struct Sized {
  B& buf;
  size_t count;
};
template <typename B>
Sized<B> sized(B& b, size_t count) { return Sized<B>{b, count}; }

template <typename... B>
void reset_all(B&... b) { (b.reset(), ...); }

// Frees every member, then allocates each; a failure part-way frees every member again.
template <typename First, typename... Rest>
auto alloc_all(First first, Rest... rest) -> decltype(first.buf.alloc(0)) {
  typedef decltype(first.buf.alloc(0)) err_t;
  reset_all(first.buf, rest.buf...);
  err_t e = first.buf.alloc(first.count);
  ((e == err_t{} ? (void)(e = rest.buf.alloc(rest.count)) : (void)0), ...);
  if (e != err_t{}) reset_all(first.buf, rest.buf...);
  return e;
}

// Room for `need` items in a group of buffers sized from one capacity `cap` (0 = the group is
// empty). fill(c) allocates the group for capacity c = cap_of(need), normally with alloc_all; when
// it fails the capacity stays 0, so the next call starts clean.
template <typename Policy, typename Sync, typename Fill>
auto grow_group(size_t& cap, size_t need, Policy cap_of, Sync sync, Fill fill) -> decltype(sync()) {
  if (cap && need <= cap) return decltype(sync()){};
  auto e = sync();
  if (e != decltype(e){}) return e;
  cap = 0;
  const size_t c = cap_of(need);
  e = fill(c);
  if (e == decltype(e){}) cap = c;
  return e;
}

}  // namespace devbuf

#ifdef __HIPCC__
#include <atomic>
#include <vector>
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

namespace devbuf {

// The HIP policy; it also counts the live allocations made through the owners, process-wide.
struct HipAlloc {
  typedef hipError_t err_t;
  static constexpr hipError_t ok = hipSuccess;
  inline static std::atomic<uint64_t> live_dev{0}, live_host{0};
  static hipError_t dev_alloc(void** p, size_t bytes) {
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) ++live_dev;
    return e;
  }
  static void dev_free(void* p) {
    (void)hipFree(p);
    --live_dev;
  }
  static hipError_t host_alloc(void** p, size_t bytes) {
    const hipError_t e = hipHostMalloc(p, bytes);
    if (e == hipSuccess) ++live_host;
    return e;
  }
  static void host_free(void* p) {
    (void)hipHostFree(p);
    --live_host;
  }
};

// A move-only HIP handle, destroyed by Destroy.
template <typename H, hipError_t (*Destroy)(H)>
class Handle {
 public:
  Handle() = default;
  Handle(Handle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  Handle& operator=(Handle&& o) noexcept {
    if (this != &o) {
      reset();
      h_ = std::exchange(o.h_, nullptr);
    }
    return *this;
  }
  ~Handle() { reset(); }
  void reset() {
    if (h_) (void)Destroy(h_);
    h_ = nullptr;
  }
  operator H() const { return h_; }

 protected:
  H h_ = nullptr;
};

struct Event : Handle<hipEvent_t, hipEventDestroy> {
  hipError_t create(unsigned flags = hipEventDefault) {
    reset();
    return hipEventCreateWithFlags(&h_, flags);
  }
};

struct Stream : Handle<hipStream_t, hipStreamDestroy> {
  hipError_t create(unsigned flags) {
    reset();
    return hipStreamCreateWithFlags(&h_, flags);
  }
  // A stream with an all-CU mask gets a hardware queue of its own instead of one of the runtime's
  // shared pool (GPU_MAX_HW_QUEUES, 4 by default, one of which the default stream already holds).
  hipError_t create_all_cus(int device) {
    reset();
    int cus = 0;
    const hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e != hipSuccess || cus <= 0) return hipStreamCreateWithFlags(&h_, hipStreamNonBlocking);
    std::vector<uint32_t> mask((cus + 31) / 32, 0xFFFFFFFFu);
    if (cus % 32) mask.back() = (1u << (cus % 32)) - 1u;
    return hipExtStreamCreateWithCUMask(&h_, (uint32_t)mask.size(), mask.data());
  }
};

// sync() arguments of the growth helpers
inline auto sync_of(hipStream_t a) {
  return [a] { return hipStreamSynchronize(a); };
}
inline auto sync_of(hipStream_t a, hipStream_t b) {
  return [a, b] {
    const hipError_t e = hipStreamSynchronize(a);
    return e != hipSuccess ? e : hipStreamSynchronize(b);
  };
}

}  // namespace devbuf
#endif  // __HIPCC__
