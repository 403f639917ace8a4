// OwnedBuf (open_vins_amd/csrc/dev_buf.h) on a counting malloc / free policy: a stand-alone host program, built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_dev_buf_host.py.  After every block the policy's live allocations and live bytes are what the block
// implies; at the end both are zero.  Exit status 0 and the line "dev_buf ok" mean every check held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>

#include "dev_buf.h"

namespace {
struct Counting {
  using Err = int;
  static constexpr Err ok = 0;
  static inline long live = 0, live_bytes = 0, allocs = 0, copies = 0;
  static inline bool fail_next = false;
  static Err alloc(void **p, size_t bytes) {
    if (fail_next) {
      fail_next = false;
      return 1;
    }
    *p = std::malloc(bytes);
    live++, live_bytes += (long)bytes, allocs++;
    return ok;
  }
  static void free(void *p, size_t bytes) {
    std::free(p);
    live--, live_bytes -= (long)bytes;
  }
  static Err copy(void *dst, const void *src, size_t bytes) {
    std::memcpy(dst, src, bytes);
    copies++;
    return ok;
  }
};
using Buf = ovg::OwnedBuf<double, Counting>;
static_assert(!std::is_copy_constructible<Buf>::value && !std::is_copy_assignable<Buf>::value, "an owning buffer must not be copyable");
static_assert(std::is_nothrow_move_constructible<Buf>::value && std::is_nothrow_move_assignable<Buf>::value, "moves must be noexcept");

int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                    \
    }                                                                \
  } while (0)
// the policy holds n allocations of `elems` doubles in all
#define LIVE(n, elems) CHECK(Counting::live == (n) && Counting::live_bytes == (long)((elems) * sizeof(double)))

void fill(Buf &b, size_t n, double base) {
  for (size_t i = 0; i < n; i++) b.p[i] = base + (double)i;
}
bool holds(const Buf &b, size_t n, double base) {
  for (size_t i = 0; i < n; i++)
    if (b.p[i] != base + (double)i) return false;
  return true;
}
} // namespace

int main() {
  { // reserve: growing, not growing, zero elements
    Buf b;
    CHECK(b.p == nullptr && b.cap == 0);
    CHECK(b.reserve(0) == 0 && b.p == nullptr); // nothing to hold: nothing allocated
    LIVE(0, 0);
    CHECK(b.reserve(10) == 0 && b.p && b.cap == 10);
    LIVE(1, 10);
    double *was = b.p;
    fill(b, 10, 1.0);
    CHECK(b.reserve(10) == 0 && b.reserve(3) == 0 && b.p == was && b.cap == 10 && holds(b, 10, 1.0)); // no growth: the same allocation
    LIVE(1, 10);
    CHECK(b.reserve(11) == 0 && b.cap == 11); // growth: the old allocation is freed, the contents are not kept
    LIVE(1, 11);
    fill(b, 11, 2.0);
    Counting::fail_next = true;
    CHECK(b.reserve(100) != 0 && b.p == nullptr && b.cap == 0); // a failed growth leaves the buffer empty
    LIVE(0, 0);
  }
  LIVE(0, 0);
  { // reserve(n, keep): keep below, at and above the old capacity; no growth; from empty; a failed allocation
    for (size_t keep : {(size_t)4, (size_t)8, (size_t)20}) {
      Buf b;
      CHECK(b.reserve(8) == 0);
      fill(b, 8, 5.0);
      const long copies = Counting::copies;
      CHECK(b.reserve(16, keep) == 0 && b.cap == 16);
      CHECK(Counting::copies == copies + 1 && holds(b, keep < 8 ? keep : 8, 5.0)); // min(keep, old capacity) elements survive
      LIVE(1, 16);
      double *was = b.p;
      CHECK(b.reserve(16, keep) == 0 && b.reserve(2, keep) == 0 && b.p == was); // no growth
      LIVE(1, 16);
    }
    LIVE(0, 0);
    Buf b;
    const long copies = Counting::copies;
    CHECK(b.reserve(6, 6) == 0 && b.cap == 6 && Counting::copies == copies); // from empty: nothing to copy
    CHECK(b.reserve(7, 0) == 0 && b.cap == 7 && Counting::copies == copies); // keep = 0: nothing copied
    LIVE(1, 7);
    fill(b, 7, 9.0);
    double *was = b.p;
    Counting::fail_next = true;
    CHECK(b.reserve(50, 7) != 0 && b.p == was && b.cap == 7 && holds(b, 7, 9.0)); // a failed growth leaves the buffer as it was
    LIVE(1, 7);
  }
  LIVE(0, 0);
  { // release, twice; release of an empty buffer; use after release
    Buf b;
    b.release();
    CHECK(b.reserve(5) == 0);
    LIVE(1, 5);
    b.release();
    CHECK(b.p == nullptr && b.cap == 0);
    LIVE(0, 0);
    b.release();
    LIVE(0, 0);
    CHECK(b.reserve(2) == 0 && b.cap == 2);
    LIVE(1, 2);
  }
  LIVE(0, 0);
  { // move construction leaves the source empty and allocates nothing
    Buf a;
    CHECK(a.reserve(12) == 0);
    fill(a, 12, 3.0);
    double *was = a.p;
    const long allocs = Counting::allocs;
    Buf b(std::move(a));
    CHECK(a.p == nullptr && a.cap == 0 && b.p == was && b.cap == 12 && holds(b, 12, 3.0) && Counting::allocs == allocs);
    LIVE(1, 12);
    CHECK(a.reserve(1) == 0); // a moved-from buffer is an empty buffer
    LIVE(2, 13);
  }
  LIVE(0, 0);
  { // move assignment onto a non-empty buffer frees what it held; self-assignment changes nothing
    Buf a, b;
    CHECK(a.reserve(4) == 0 && b.reserve(9) == 0);
    fill(a, 4, 7.0);
    LIVE(2, 13);
    double *was = a.p;
    b = std::move(a);
    CHECK(a.p == nullptr && a.cap == 0 && b.p == was && b.cap == 4 && holds(b, 4, 7.0));
    LIVE(1, 4);
    Buf &same = b;
    b = std::move(same);
    CHECK(b.p == was && b.cap == 4 && holds(b, 4, 7.0));
    LIVE(1, 4);
    Buf empty;
    b = std::move(empty); // an empty source empties the target
    CHECK(b.p == nullptr && b.cap == 0);
    LIVE(0, 0);
  }
  LIVE(0, 0);
  { // std::swap of two buffers, of a buffer and an empty one, and of a buffer with itself: pointers change hands, nothing is allocated or freed
    Buf a, b, e;
    CHECK(a.reserve(3) == 0 && b.reserve(6) == 0);
    fill(a, 3, 1.0), fill(b, 6, 2.0);
    double *pa = a.p, *pb = b.p;
    const long allocs = Counting::allocs;
    std::swap(a, b);
    CHECK(a.p == pb && a.cap == 6 && b.p == pa && b.cap == 3 && holds(a, 6, 2.0) && holds(b, 3, 1.0));
    LIVE(2, 9);
    std::swap(a, a);
    CHECK(a.p == pb && a.cap == 6 && holds(a, 6, 2.0));
    LIVE(2, 9);
    std::swap(a, e);
    CHECK(a.p == nullptr && a.cap == 0 && e.p == pb && e.cap == 6);
    LIVE(2, 9);
    CHECK(Counting::allocs == allocs);
  }
  LIVE(0, 0);
  { // destruction of an empty, a full and a moved-from buffer
    Buf full, from;
    CHECK(full.reserve(32) == 0 && from.reserve(2) == 0);
    {
      Buf empty;
      Buf to(std::move(from));
      LIVE(2, 34);
    }
    LIVE(1, 32); // `to` freed what `from` had held; `from` has nothing left to free
  }
  LIVE(0, 0);
  CHECK(Counting::live == 0 && Counting::live_bytes == 0);
  if (failures) return 1;
  std::printf("dev_buf ok\n");
  return 0;
}
