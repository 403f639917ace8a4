// host_link.h — the two page-locked buffers every frame's bytes cross the bus through, as owning types: Uplink (the upload arena behind
// ovgpu_set_state / ovgpu_set_features) and Landing (the zone the results come back through), with LandLayout for the landing offsets.
// No HIP in here: api_context.inc supplies the HIP port, a host test a port of its own whose copies run late (tests/host/host_link_main.cpp).
//
// A port is a struct of static members:
//   using Err = ...;  static constexpr Err ok = ..., refused = ...;   the status type, its "no error", and "outside the reservation"
//   using Stream = ...;                                               the handle of the context's stream
//   using Pinned = ...;                                               the page-locked allocation policy of OwnedBuf (dev_buf.h)
//   static unsigned char *device_alias(unsigned char *host);          the device's pointer to page-locked host memory, or null
//   static Err h2d(Stream, void *dst, const void *src, size_t bytes); asynchronous copies on the stream
//   static Err d2h(Stream, void *dst, const void *src, size_t bytes);
//   static Err scatter(Stream, const unsigned char *arena, const UpBatch &);   ONE launch: arena + seg.off -> seg.dst, b.n arrays
//   static Err gather(Stream, unsigned char *zone, const UpBatch &);           ONE launch: seg.dst -> zone + seg.off
//   static Err sync(Stream);                                          blocks until the stream is idle
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "dev_buf.h"

// One launch instead of one copy per array.  ovgpu_set_state + ovgpu_set_features hand over ~20 arrays per frame, most of them a few hundred
// bytes.  As one hipMemcpyAsync each they cost the caller's thread ~5 us apiece and the stream a DMA packet with its own completion signal
// apiece.  The arrays are packed into the page-locked arena anyway: ONE kernel reads the arena over PCIe (page-locked host memory is mapped
// into the device's address space) and scatters every array to its own device buffer — the same bytes cross the bus once, the caller pays
// one launch.  (Plain data at global scope: k_upload_scatter and k_download_gather take an UpBatch by value, their symbols carry its name.)
struct UpSeg {
  void *dst;
  uint32_t off, bytes; // offset in the arena (64-byte aligned), length
};
constexpr int UP_MAX_SEG = 28, UP_BLOCKS = 48; // workgroups per array: 48 x 256 lanes x 16 B = 196 KB in flight per pass and array
struct UpBatch {
  UpSeg seg[UP_MAX_SEG];
  int n = 0;
};

namespace ovg {

constexpr size_t LINK_MAX_OFF = 0xffffffffull; // UpSeg's offsets are 32 bits wide

// The uploads of a state / feature batch (25 arrays per update of the drop-in path): a copy from PAGEABLE memory is staged by the runtime
// one call at a time (~20 us apiece, the caller blocked); here the CPU packs the bytes into one page-locked arena and they leave by scatter
// launches, so packing the next array overlaps the transfer of the previous ones.  When put() returns, the bytes are in the arena or on
// the device: the source may die at once.  Stream order is call order: whatever is put is on its way once flush() has returned.
template <class Port>
struct Uplink {
  using Err = typename Port::Err;
  typename Port::Stream stream{}; // the context's stream: set once, before the first call
  bool use_kernel = true;         // false: one asynchronous copy per array out of the arena
  int64_t bypasses = 0;           // arrays that did not fit the arena and went from the caller's memory (rare: the arena grows at the next begin)
  size_t want = 8u << 20;         // capacity asked for at the next begin(); it only grows

  size_t capacity() const { return arena.cap; }

  // At the top of an entry point that uploads.  Copies out of the arena may still be in flight (ovgpu_set_state returns without a
  // synchronisation): keep appending behind them; the offset goes back to 0 once a synchronisation of the stream has been seen (synced()).
  // An arena that must grow while copies are in flight waits for them first.
  Err begin() {
    if (!dirty) off = 0;
    if (want <= arena.cap) return Port::ok;
    if (dirty) {
      if (Err e = flush(); e != Port::ok) return e;
      if (Err e = Port::sync(stream); e != Port::ok) return e;
      dirty = false, off = 0;
    }
    dev = nullptr;
    if (Err e = arena.reserve(want); e != Port::ok) return e;
    dev = Port::device_alias(arena.p);
    return Port::ok;
  }
  // src -> dst (device), with the next flush()
  Err put(void *dst, const void *src, size_t bytes) {
    if (bytes == 0) return Port::ok;
    const size_t o = next();
    if (!deferred_ok(o, bytes)) return staged(dst, src, bytes);
    std::memcpy(arena.p + o, src, bytes);
    off = o + bytes, dirty = true;
    return add(dst, o, bytes);
  }
  // ... with a second destination of the same arena bytes.  `twinned` is cleared when the twin was NOT registered (the array went another
  // way than the scatter launch, or the launch had one free segment left): the caller copies dst -> twin on the device then.
  Err put2(void *dst, void *twin, const void *src, size_t bytes, bool &twinned) {
    const size_t o = next();
    const bool both = bytes > 0 && deferred_ok(o, bytes) && batch.n + 2 <= UP_MAX_SEG;
    if (Err e = put(dst, src, bytes); e != Port::ok) return e;
    if (!both) return twinned = false, Port::ok;
    return add(twin, o, bytes);
  }
  // For an array the caller builds in place: room in the arena, or null when the scatter path is off or the arena full (the caller then
  // builds it elsewhere and uses put()); commit() registers it for the next flush() once its destination is known.
  void *take(size_t bytes) {
    const size_t o = next();
    if (bytes == 0 || !deferred_ok(o, bytes)) return nullptr;
    off = o + bytes, dirty = true;
    return arena.p + o;
  }
  Err commit(void *dst, const void *slot, size_t bytes) { return add(dst, (size_t)(static_cast<const unsigned char *>(slot) - arena.p), bytes); }
  // the arrays registered since the last flush leave by ONE launch
  Err flush() {
    if (batch.n == 0) return Port::ok;
    const Err e = Port::scatter(stream, dev, batch);
    batch.n = 0;
    return e;
  }
  // a synchronisation of the stream has been seen behind the last flush(): nothing reads the arena any more
  void synced() { dirty = false; }

private:
  OwnedBuf<unsigned char, typename Port::Pinned> arena;
  const unsigned char *dev = nullptr; // the arena as the device sees it
  size_t off = 0;
  UpBatch batch;      // arrays packed into the arena since the last scatter launch
  bool dirty = false; // copies out of the arena may be in flight

  size_t next() const { return (off + 63) & ~(size_t)63; }
  bool deferred_ok(size_t o, size_t bytes) const { return use_kernel && dev && o + bytes <= arena.cap && o + bytes <= LINK_MAX_OFF; }
  Err add(void *dst, size_t o, size_t bytes) {
    if (batch.n >= UP_MAX_SEG) {
      if (Err e = flush(); e != Port::ok) return e;
    }
    UpSeg &sg = batch.seg[batch.n++];
    sg.dst = dst, sg.off = (uint32_t)o, sg.bytes = (uint32_t)bytes;
    return Port::ok;
  }
  // one copy for this array, behind what was registered before it
  Err staged(void *dst, const void *src, size_t bytes) {
    if (Err e = flush(); e != Port::ok) return e;
    const size_t o = next();
    if (o + bytes > arena.cap) {
      // The bypass.  No room this time: the copy leaves from the caller's memory, and the stream is idle before this returns, because the
      // source may die then.  The arena grows at the next begin() (bounded: beyond 1 GiB this path serves).
      want = std::min<size_t>(std::max(want, 2 * (o + bytes)), (size_t)1 << 30);
      bypasses++;
      if (Err e = Port::h2d(stream, dst, src, bytes); e != Port::ok) return e;
      return Port::sync(stream); // (dirty stays: a slot taken before this may be committed behind it)
    }
    std::memcpy(arena.p + o, src, bytes);
    off = o + bytes, dirty = true;
    return Port::h2d(stream, dst, arena.p + o, bytes);
  }
};

// Offsets into the landing zone, in the order of the calls: every one 64-byte aligned (the gather kernel stores 16-byte vectors)
struct LandLayout {
  size_t end = 0; // the zone's size so far
  explicit LandLayout(size_t start = 0) : end(start) {}
  size_t add(size_t bytes) {
    const size_t o = (end + 63) & ~(size_t)63;
    end = o + bytes;
    return o;
  }
};

// The way back: the results of an update (status, chi2, p_FinG, flags, dx, P': eight device arrays) land in the page-locked zone by ONE
// launch that writes them over PCIe (as eight hipMemcpyAsync: ~60 us between the last kernel and the caller's memcpy), the caller
// synchronises once and copies them out of at().
template <class Port>
struct Landing {
  using Err = typename Port::Err;
  typename Port::Stream stream{};
  bool use_kernel = true; // false: one asynchronous copy per array

  size_t capacity() const { return zone.cap; }
  // Room for `bytes`, before the first get() of a read-back.  A zone that must move while arrays are on their way into it waits for them
  // first: nothing lands in freed memory.  (Its contents do not survive the move.)
  Err reserve(size_t bytes) {
    if (bytes <= zone.cap) return Port::ok;
    if (busy) {
      if (Err e = flush(); e != Port::ok) return e;
      if (Err e = Port::sync(stream); e != Port::ok) return e;
      busy = false;
    }
    dev = nullptr;
    if (Err e = zone.reserve(bytes); e != Port::ok) return e;
    dev = Port::device_alias(zone.p);
    return Port::ok;
  }
  // device array -> offset `off` of the zone, with the next flush(); Port::refused, and nothing written, beyond what the zone holds
  Err get(size_t off, const void *src, size_t bytes) {
    if (bytes == 0) return Port::ok;
    if (off + bytes > zone.cap) return Port::refused;
    busy = true;
    if (!use_kernel || !dev || (off & 15) || off + bytes > LINK_MAX_OFF) return Port::d2h(stream, zone.p + off, src, bytes);
    if (batch.n >= UP_MAX_SEG) {
      if (Err e = flush(); e != Port::ok) return e;
    }
    UpSeg &sg = batch.seg[batch.n++];
    sg.dst = const_cast<void *>(src), sg.off = (uint32_t)off, sg.bytes = (uint32_t)bytes;
    return Port::ok;
  }
  Err flush() {
    if (batch.n == 0) return Port::ok;
    const Err e = Port::gather(stream, dev, batch);
    batch.n = 0;
    return e;
  }
  void synced() { busy = false; } // a synchronisation of the stream has been seen behind the last flush(): at() holds the results
  const unsigned char *at(size_t off) const { return zone.p + off; }

private:
  OwnedBuf<unsigned char, typename Port::Pinned> zone;
  unsigned char *dev = nullptr; // the zone as the device sees it
  UpBatch batch;                // result arrays registered since the last gather launch
  bool busy = false;            // arrays may be on their way into the zone
};

} // namespace ovg
