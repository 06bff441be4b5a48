// pa_carve.h -- one allocation cut into consecutive typed parts: a layout is a function of a Carve that take()s its
// parts in order, and the same function gives the allocation's size (run on no base) and the parts' addresses (run on
// the allocation).  Byte offsets and their checks only, no HIP runtime, so that a host compiler (and
// tests/tools/sanitize/carve.cpp) can reach them; pa_internal.h's pa_carve is the form over a DevBuf.
#pragma once

#include <cstdint>

enum class CarveVerdict { kOk, kTooLarge, kBadAlignment, kMisaligned, kPassesDisagree };
inline const char *carve_verdict_text(CarveVerdict v) {
  switch (v) {
    case CarveVerdict::kOk: return "ok";
    case CarveVerdict::kTooLarge: return "its size does not fit 64 bits";
    case CarveVerdict::kBadAlignment: return "an alignment that is no power of two or below its type's";
    case CarveVerdict::kMisaligned: return "the allocation's start does not put every part on its alignment";
    case CarveVerdict::kPassesDisagree: return "the layout placed is not the layout measured";
  }
  return "?";
}

class Carve {
 public:
  // Without a base (the measuring pass) every take() is nullptr and only the offsets run.  With one, `room` is the
  // measured size: a layout that goes past it is refused before an address outside the allocation is formed.
  Carve() : base_(nullptr), room_(UINT64_MAX) {}
  Carve(void *base, uint64_t room) : base_(static_cast<char *>(base)), room_(room) {}

  // The next `count` values of T, on alignof(T) or on `align` where that is more.  An empty part has an address too.
  template <typename T>
  T *take(uint64_t count, uint64_t align = alignof(T)) {
    if (align < alignof(T)) fail(CarveVerdict::kBadAlignment);
    align_to(align);
    const uint64_t at = end_;
    if (count > UINT64_MAX / sizeof(T)) fail(CarveVerdict::kTooLarge);
    else advance(count * sizeof(T));
    if (base_ && verdict_ == CarveVerdict::kOk && (reinterpret_cast<uintptr_t>(base_ + at) & (align - 1))) fail(CarveVerdict::kMisaligned);
    return base_ && verdict_ == CarveVerdict::kOk ? reinterpret_cast<T *>(base_ + at) : nullptr;
  }
  // `bytes` that belong to no part: room that wide loads may read past a part, or that a measured layout depends on
  void slack(uint64_t bytes) { advance(bytes); }
  // The next part starts on `align`; returns the bytes this skipped
  uint64_t align_to(uint64_t align) {
    if (align == 0 || (align & (align - 1))) return fail(CarveVerdict::kBadAlignment), 0;
    if (align > max_align_) max_align_ = align;
    const uint64_t skip = (align - (end_ & (align - 1))) & (align - 1);
    advance(skip);
    return skip;
  }

  uint64_t end() const { return end_; }  // the bytes taken so far; after a refusal, where it happened
  uint64_t max_align() const { return max_align_; }
  CarveVerdict verdict() const { return verdict_; }  // the first refusal; nothing is handed out after one

 private:
  void fail(CarveVerdict v) {
    if (verdict_ == CarveVerdict::kOk) verdict_ = v;
  }
  void advance(uint64_t bytes) {
    if (bytes > UINT64_MAX - end_) fail(CarveVerdict::kTooLarge);
    else if (bytes > room_ - end_) fail(CarveVerdict::kPassesDisagree);
    if (verdict_ == CarveVerdict::kOk) end_ += bytes;
  }
  char *base_;
  uint64_t room_;  // end_ <= room_ always
  uint64_t end_ = 0, max_align_ = 1;
  CarveVerdict verdict_ = CarveVerdict::kOk;
};

// The two passes.  carve_measure: the layout's size.  carve_place: the layout on `base`, an allocation of at least the
// `measured` bytes; it must end where the measuring pass ended, on a base that satisfies the largest alignment asked,
// every part on its alignment.  After any verdict but kOk the caller uses none of the pointers.
template <class Layout>
CarveVerdict carve_measure(Layout &&layout, uint64_t *measured) {
  Carve k;
  layout(k);
  *measured = k.end();
  return k.verdict();
}
template <class Layout>
CarveVerdict carve_place(void *base, uint64_t measured, Layout &&layout) {
  Carve k(base, measured);
  layout(k);
  if (k.verdict() != CarveVerdict::kOk) return k.verdict();
  if (k.end() != measured) return CarveVerdict::kPassesDisagree;
  return reinterpret_cast<uintptr_t>(base) & (k.max_align() - 1) ? CarveVerdict::kMisaligned : CarveVerdict::kOk;
}
