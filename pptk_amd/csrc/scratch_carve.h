// scratch_carve.h -- how the batch ops lay their arrays out in the caller's
// scratch (ip_reass.hip, rx_flowlearn.hip, tx_dispatch.hip, tx_frag.hip).  An
// op states its arrays once, as one walk of take() calls: with a null base the
// walk only sizes the scratch (pptk_*_scratch_bytes), with the scratch pointer
// the same walk binds the kernel arguments, so the two cannot disagree.
// Plain C++: a host program can include it (tests/c/carve_check.cc).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace pptk {

class Carve {
 public:
  // align: a power of two; every array starts at a multiple of it from base
  Carve(void *base, size_t align) : base_((uint8_t *)base), align_(align) {}

  // the next array, `count` elements of T; null (but still counted) without a base
  template <typename T>
  T *take(size_t count) {
    T *p = base_ ? (T *)(base_ + at_) : nullptr;
    at_ += (count * sizeof(T) + align_ - 1) & ~(align_ - 1);
    return p;
  }

  size_t total() const { return at_; }

 private:
  uint8_t *base_;
  size_t align_, at_ = 0;
};

}  // namespace pptk
