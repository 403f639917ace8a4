// dev_buf.h — the one owning buffer type of the host side: `cap` elements of T from an allocation policy, freed by its destructor.
// No HIP in here: the two policies of the library (device memory, page-locked host memory) stand in api_context.inc, next to the aliases
// DevBuf<T> / PinBuf<T>; a host test instantiates the template with a policy of its own (tests/host/dev_buf_main.cpp).
//
// A policy is a struct of static members:
//   using Err = ...;  static constexpr Err ok = ...;       the status type of its calls and its "no error"
//   static Err alloc(void **p, size_t bytes);              *p is written on success only
//   static void free(void *p, size_t bytes);               bytes: what alloc was asked for
//   static Err copy(void *dst, const void *src, size_t bytes);   only for reserve(n, keep)
#pragma once
#include <algorithm>
#include <cstddef>

namespace ovg {

template <class T, class Alloc>
struct OwnedBuf {
  using Err = typename Alloc::Err;
  T *p = nullptr;
  size_t cap = 0; // elements

  OwnedBuf() = default;
  ~OwnedBuf() { release(); }
  OwnedBuf(const OwnedBuf &) = delete;
  OwnedBuf &operator=(const OwnedBuf &) = delete;
  // a move leaves the source empty (std::swap of two buffers goes through these three times: nothing is allocated, copied or freed)
  OwnedBuf(OwnedBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  OwnedBuf &operator=(OwnedBuf &&o) noexcept {
    if (this != &o) {
      release();
      p = o.p, cap = o.cap;
      o.p = nullptr, o.cap = 0;
    }
    return *this;
  }

  // room for n elements; the contents do not survive a reallocation.  On failure the buffer is empty.
  Err reserve(size_t n) {
    if (n <= cap) return Alloc::ok;
    release();
    void *q = nullptr;
    const Err e = Alloc::alloc(&q, bytes_of(n));
    if (e == Alloc::ok) p = static_cast<T *>(q), cap = n;
    return e;
  }
  // like reserve, but the first `keep` elements survive a reallocation.  When the allocation fails the buffer is left as it was.
  Err reserve(size_t n, size_t keep) {
    if (n <= cap) return Alloc::ok;
    void *q = nullptr;
    Err e = Alloc::alloc(&q, bytes_of(n));
    if (e != Alloc::ok) return e;
    if (p && keep > 0) e = Alloc::copy(q, p, std::min(keep, cap) * sizeof(T));
    release();
    p = static_cast<T *>(q), cap = n;
    return e;
  }
  void release() {
    if (p) Alloc::free(p, bytes_of(cap));
    p = nullptr, cap = 0;
  }

private:
  static size_t bytes_of(size_t n) { return std::max<size_t>(n, 1) * sizeof(T); } // (reserve(0) on an empty buffer allocates nothing: n <= cap)
};

} // namespace ovg
