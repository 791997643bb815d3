// carve_check.cc -- pptk_amd/csrc/scratch_carve.h on a CPU, under ASan + UBSan
// (tests/test_carve.py).  A mixed list of arrays (element sizes 1, 2, 4, 8, 16
// and 32 bytes, zero counts among them) is walked at alignments 16 and 256:
// the sizing walk (no base) and the binding walk must give the same offsets
// and total, every pointer must be aligned, and writing every array in full
// must stay inside a heap block of exactly total() bytes.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "scratch_carve.h"

namespace {

struct E16 {
  uint64_t a, b;
};
struct E32 {
  uint64_t a[4];
};
static_assert(sizeof(E16) == 16 && sizeof(E32) == 32, "element sizes");

constexpr int kArrays = 14;
const size_t kCounts[kArrays] = {1, 0, 3, 17, 0, 255, 256, 257, 1000, 5, 0, 33, 4097, 0};

int fails = 0;
#define CHECK(x)                                              \
  do {                                                        \
    if (!(x)) {                                               \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);     \
      ++fails;                                                \
    }                                                         \
  } while (0)

// array k has elements of 1 << (k % 6) bytes
void *take(pptk::Carve &c, int k, size_t count) {
  switch (k % 6) {
    case 0: return c.take<uint8_t>(count);
    case 1: return c.take<uint16_t>(count);
    case 2: return c.take<uint32_t>(count);
    case 3: return c.take<uint64_t>(count);
    case 4: return c.take<E16>(count);
    default: return c.take<E32>(count);
  }
}

void walk(size_t align) {
  // sizing: no base, every pointer null, the offsets from total()
  size_t off[kArrays], expect = 0;
  pptk::Carve sizing(nullptr, align);
  for (int k = 0; k < kArrays; ++k) {
    off[k] = sizing.total();
    CHECK(off[k] == expect);
    CHECK(take(sizing, k, kCounts[k]) == nullptr);
    expect += ((kCounts[k] << (k % 6)) + align - 1) / align * align;
  }
  const size_t total = sizing.total();
  CHECK(total == expect);

  // binding: a heap block of exactly that size, aligned like a scratch
  uint8_t *block = (uint8_t *)aligned_alloc(align, total);
  CHECK(block != nullptr);
  if (!block) return;
  pptk::Carve bind(block, align);
  for (int k = 0; k < kArrays; ++k) {
    uint8_t *p = (uint8_t *)take(bind, k, kCounts[k]);
    CHECK(p == block + off[k]);
    CHECK(((uintptr_t)p & (align - 1)) == 0);
    memset(p, 0xa5, kCounts[k] << (k % 6));   // past the block: ASan reports it
  }
  CHECK(bind.total() == total);
  free(block);
}

}  // namespace

int main() {
  walk(16);
  walk(256);
  if (fails) return 1;
  printf("carve ok\n");
  return 0;
}
