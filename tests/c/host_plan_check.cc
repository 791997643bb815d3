// host_plan_check.cc -- pptk_amd/csrc/host_plan.h on a CPU, as a program of
// its own (tests/test_host_plan.py builds it under ASan + UBSan and under
// ThreadSanitizer): the chunk description and gather, the fold, the worker
// pool's running totals, and plan_transport's truth table.  The staging
// buffers are exactly-sized heap blocks, so a store past round16 of the last
// frame is an error.  "parent:N" cites line N of rx_capi.hip's enqueue_chunk
// in commit 49adbd1, which the expectations are written from.
#include <stdio.h>
#include <stdlib.h>

#include "host_plan.h"

using namespace pptk;

static int g_fail = 0;
#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);         \
      ++g_fail;                                                   \
    }                                                             \
  } while (0)

static const HostKnobs kDefault = {2u << 20, 0.80, true, true, true};
static size_t r16(size_t n) { return (n + 15) & ~(size_t)15; }

// exactly-sized staging: frame bytes (16-byte aligned), offsets, lengths
struct Stage {
  uint8_t *frames;
  uint64_t *off;
  uint16_t *len;
  size_t bytes, cnt;
  std::vector<PartDesc> parts;
  std::vector<std::atomic<size_t>> run;
  Stage(size_t bytes_, size_t cnt_) : bytes(bytes_), cnt(cnt_) {
    frames = (uint8_t *)aligned_alloc(16, bytes ? bytes : 16);
    off = new uint64_t[cnt];
    len = new uint16_t[cnt];
    memset(frames, 0xAA, bytes);
    for (size_t i = 0; i < cnt; ++i) off[i] = 0xA5A5A5A5A5A5A5A5ull, len[i] = 0xA5A5;
  }
  ~Stage() {
    free(frames);
    delete[] off;
    delete[] len;
  }
  StageView view() { return {frames, off, len, parts, run}; }
  bool untouched() const {
    for (size_t i = 0; i < cnt; ++i)
      if (off[i] != 0xA5A5A5A5A5A5A5A5ull || len[i] != 0xA5A5) return false;
    return true;
  }
};

static uint32_t g_rng = 12345;
static uint8_t rnd() { return (uint8_t)((g_rng = g_rng * 1664525u + 1013904223u) >> 24); }

static void staged_one_part(bool nt) {
  const uint32_t lens[7] = {0, 1, 15, 16, 17, 64, 1500}, maxf = 1500;
  const size_t n = 40;
  std::vector<std::vector<uint8_t>> src(n);
  std::vector<ldp_packet> pk(n);
  std::vector<uint32_t> want(n);
  size_t total = 0;
  for (size_t i = 0; i < n; ++i) {
    uint32_t sz = lens[i % 7];
    if (i == 9) sz = maxf + 1;   // too long: described as length 0
    src[i].resize(sz ? sz : 1);
    for (uint8_t &b : src[i]) b = rnd();
    pk[i].data = i == 5 ? nullptr : src[i].data();   // no data: length 0
    pk[i].sz = sz;
    want[i] = (i == 5 || i == 9) ? 0 : sz;
    total += r16(want[i]);
  }
  Stage st(total, n);
  HostKnobs k = kDefault;
  k.nt_gather = nt;
  const ChunkIn in = {pk.data(), n, maxf, nullptr};
  const ChunkSums s = describe_chunk(st.view(), in, k, nullptr);
  CHECK(st.parts.size() == 1);
  CHECK(s.bytes == total && s.maxlen == 1500 && !s.outside && !s.uni_len);
  size_t pos = 0;
  for (size_t i = 0; i < n; ++i) {
    CHECK(st.len[i] == want[i]);
    CHECK(st.off[i] == pos);
    CHECK(want[i] == 0 || memcmp(st.frames + pos, src[i].data(), want[i]) == 0);
    if (nt)
      for (size_t b = want[i]; b < r16(want[i]); ++b) CHECK(st.frames[pos + b] == 0);
    pos += r16(want[i]);
  }
}

static void staged_over_pool() {
  const size_t n = 8192;
  const uint32_t maxf = 9216;
  std::vector<uint8_t> src(n * 100 + 128);
  for (uint8_t &b : src) b = rnd();
  std::vector<ldp_packet> pk(n);
  size_t total = 0;
  for (size_t i = 0; i < n; ++i) {
    pk[i].data = src.data() + i * 100 + i % 13;
    pk[i].sz = i == 0 ? 60u : (uint32_t)(i * 7 % 97);
    total += r16(pk[i].sz);
  }
  const ChunkIn in = {pk.data(), n, maxf, nullptr};
  Stage one(total, n);
  const ChunkSums s1 = describe_chunk(one.view(), in, kDefault, nullptr);
  CHECK(one.parts.size() == 1 && s1.bytes == total);
  WorkerPool pool(3);
  CHECK(pool.size() == 4 && part_count(in, &pool) > 1);
  for (int rep = 0; rep < 50; ++rep) {
    Stage st(total, n);
    const ChunkSums s = describe_chunk(st.view(), in, kDefault, &pool);
    CHECK(st.parts.size() == part_count(in, &pool));
    CHECK(s.bytes == total && s.maxlen == s1.maxlen && s.uni_len == s1.uni_len);
    CHECK(memcmp(st.off, one.off, n * 8) == 0 && memcmp(st.len, one.len, n * 2) == 0);
    CHECK(memcmp(st.frames, one.frames, total) == 0);
  }
}

// n frames of 1500 bytes in a ring of 2 048-byte slots, frame i in slot
// slot(i); `shift` bytes are added to every third frame's place (irregular
// pitch), frame `odd` (if < n) has another length
struct RingCase {
  std::vector<uint8_t> mem;
  RingView ring;
  std::vector<ldp_packet> pk;
  template <class Slot>
  RingCase(size_t n, size_t slots, Slot slot, size_t shift = 0, size_t odd = SIZE_MAX)
      : mem(slots * 2048), ring{mem.data(), mem.size()}, pk(n) {
    for (size_t i = 0; i < n; ++i) {
      pk[i].data = mem.data() + slot(i) * 2048 + (i % 3 == 2 ? shift : 0);
      pk[i].sz = i == odd ? 700u : 1500u;
    }
  }
  ChunkSums run(Stage &st, WorkerPool *pool, size_t want_parts) {
    const ChunkIn in = {pk.data(), pk.size(), 9216, &ring};
    const ChunkSums s = describe_chunk(st.view(), in, kDefault, pool);
    CHECK(st.parts.size() == want_parts);
    return s;
  }
  // the descriptors of a chunk that is not fixed-stride: the ring offsets
  void check_descriptors(const Stage &st) const {
    for (size_t i = 0; i < pk.size(); ++i) {
      CHECK(st.off[i] == (uint64_t)((const uint8_t *)pk[i].data - ring.host));
      CHECK(st.len[i] == pk[i].sz);
    }
  }
};

static void ring_uniformity(size_t n, WorkerPool *pool, size_t parts) {
  auto fixed = [&](const ChunkSums &s) { return fixed_stride(s, kDefault, true, n); };
  {   // in order, from slot 1: uniform, nothing written
    RingCase rc(n, n + 1, [](size_t i) { return i + 1; });
    Stage st(0, n);
    const ChunkSums s = rc.run(st, pool, parts);
    CHECK(s.uni_len && s.uni_ptr && fixed(s) && !s.outside);
    CHECK(s.stride == 2048 && s.first_off == 2048 && s.ulen == 1500 && s.maxlen == 1500);
    CHECK(s.lo == 2048 && s.hi == n * 2048 + r16(1500) && s.fbytes == n * 1500);
    CHECK(st.untouched());
  }
  {   // two frames swapped
    RingCase rc(n, n, [](size_t i) { return i == 10 ? 11 : i == 11 ? 10 : i; });
    Stage st(0, n);
    const ChunkSums s = rc.run(st, pool, parts);
    CHECK(s.uni_len && !s.uni_ptr && !fixed(s));
    rc.check_descriptors(st);
  }
  {   // equal lengths at an irregular pitch
    RingCase rc(n, n + 1, [](size_t i) { return i; }, 16);
    Stage st(0, n);
    const ChunkSums s = rc.run(st, pool, parts);
    CHECK(s.uni_len && !s.uni_ptr && !fixed(s));
    rc.check_descriptors(st);
  }
  {   // one frame of another length
    RingCase rc(n, n, [](size_t i) { return i; }, 0, n / 2 + 1);
    Stage st(0, n);
    const ChunkSums s = rc.run(st, pool, parts);
    CHECK(!s.uni_len && !s.uni_ptr && !fixed(s));
    rc.check_descriptors(st);
  }
}

static void ring_breaks(WorkerPool *pool) {
  const size_t n = 16384;   // 8 parts of 2 048 frames
  for (size_t at : {(size_t)4096, (size_t)5000}) {   // a part's first frame; mid-part
    RingCase rc(n, n + 1, [at](size_t i) { return i < at ? i : i + 1; });
    Stage st(0, n);
    const ChunkSums s = rc.run(st, pool, 8);
    CHECK(s.uni_len && !s.uni_ptr && !fixed_stride(s, kDefault, true, n));
    // (broken at a part's first frame, every part is uniform in itself:
    // only the fold's p0 == first + i0 * stride sees it)
    if (at == 4096)
      for (const PartDesc &d : st.parts) CHECK(d.uni && d.stride == 2048);
    rc.check_descriptors(st);
  }
  {   // the last part at twice the pitch: where it should start, uniform in itself
    const size_t at = 7 * 2048;
    RingCase rc(n, n + 2048, [at](size_t i) { return i < at ? i : at + 2 * (i - at); });
    Stage st(0, n);
    const ChunkSums s = rc.run(st, pool, 8);
    CHECK(s.uni_len && !s.uni_ptr && !fixed_stride(s, kDefault, true, n));
    CHECK(st.parts[7].uni && st.parts[7].stride == 4096);
    rc.check_descriptors(st);
  }
}

static void ring_single() {
  RingCase rc(1, 1, [](size_t i) { return i; });
  Stage st(0, 1);
  const ChunkSums s = rc.run(st, nullptr, 1);
  CHECK(s.uni_len && !s.uni_ptr && !fixed_stride(s, kDefault, true, 1));
  rc.check_descriptors(st);
}

static void ring_bounds() {
  const size_t R = 8192;
  std::vector<uint8_t> mem(R + 256);
  const RingView ring = {mem.data() + 64, R};
  auto run = [&](const uint8_t *p1, uint32_t sz1) {
    ldp_packet pk[2] = {};
    pk[0].data = (void *)(ring.host + 128);
    pk[0].sz = 100;
    pk[1].data = (void *)p1;
    pk[1].sz = sz1;
    Stage st(0, 2);
    const ChunkIn in = {pk, 2, 9216, &ring};
    const ChunkSums s = describe_chunk(st.view(), in, kDefault, nullptr);
    CHECK(!s.outside || st.untouched());   // the caller stages such a chunk
    return s;
  };
  CHECK(run(ring.host - 16, 64).outside);             // starts before the ring
  ChunkSums s = run(ring.host + R - 64, 64);          // ends exactly at its end
  CHECK(!s.outside && s.hi == R && s.lo == 128);
  s = run(ring.host + R - 64, 65);                    // its 16-rounded end passes it
  CHECK(s.outside && s.hi == R);                      // (hi is clamped)
  CHECK(!run(ring.host + R - 64, 49).outside);        // rounded end == R
}

struct PlanRow {
  const char *name;
  ChunkSums s;
  HostKnobs k;
  bool is_ring;
  size_t cnt;
  bool span_fits;
  FramesSrc src;
  bool pcie, fixed;
  uint32_t fixed_len;
  uint64_t stride;
  size_t first_off;
};

static ChunkSums staged(size_t bytes, bool uni_len = false, uint32_t ulen = 0) {
  ChunkSums s;
  s.bytes = bytes;
  s.uni_len = uni_len;
  s.ulen = ulen;
  return s;
}

static ChunkSums ringed(size_t lo, size_t span, double fill, bool uni_len = false,
                        bool uni_ptr = false, int64_t stride = 0) {
  ChunkSums s;
  s.lo = lo;
  s.hi = lo + span;
  s.fbytes = (size_t)(fill * (double)span);
  s.uni_len = uni_len;
  s.uni_ptr = uni_ptr;
  s.ulen = 1500;
  s.stride = stride;
  s.first_off = lo;
  return s;
}

static void plan_table() {
  const size_t M = 2u << 20;
  HostKnobs nosplit = kDefault, dens70 = kDefault, dm0 = kDefault, nouni = kDefault;
  nosplit.split = false;
  dens70.ring_dma_density = 0.70;
  dm0.direct_max_bytes = 0;
  nouni.uniform = false;
  const FramesSrc InPlace = FramesSrc::RingInPlace, Span = FramesSrc::RingSpanDma,
                  Direct = FramesSrc::StagedDirect, Dma = FramesSrc::StagedDma;
  const PlanRow rows[] = {
      // parent:1616 direct = pos <= direct_max; parent:1619 pcie = direct || split
      {"staged 2 MiB", staged(M), kDefault, false, 4096, true, Direct, true, false, 0, 0, 0},
      // parent:1618 split = !direct && !ring && split_chunks(): frames by DMA, the rest on PCIe
      {"staged 2 MiB + 16", staged(M + 16), kDefault, false, 4096, true, Dma, true, false, 0, 0, 0},
      {"staged 2 MiB, split off", staged(M), nosplit, false, 4096, true, Direct, true, false, 0, 0, 0},
      // parent:1625-1627 !pcie: the descriptor copies return
      {"staged 2 MiB + 16, split off", staged(M + 16), nosplit, false, 4096, true, Dma, false, false, 0, 0, 0},
      // parent:1611 ring_dma needs hi - lo > direct_max; parent:1616 ring: direct = dm > 0 && !ring_dma
      {"ring span 2 MiB, dense", ringed(4096, M, 1.0), kDefault, true, 4096, true, InPlace, true, false, 0, 0, 0},
      {"ring span 2 MiB + 16, dense", ringed(4096, M + 16, 1.0), kDefault, true, 4096, true, Span, true, false, 0, 0, 0},
      // parent:1618 split = !direct && ring_dma && split_chunks()
      {"ring span dense, split off", ringed(4096, 4 * M, 1.0), nosplit, true, 4096, true, Span, false, false, 0, 0, 0},
      // parent:1612 fbytes >= density * (hi - lo)
      {"ring fill 0.5", ringed(0, 4 * M, 0.5), kDefault, true, 4096, true, InPlace, true, false, 0, 0, 0},
      {"ring fill 0.73, density 0.80", ringed(0, 4 * M, 0.73), kDefault, true, 4096, true, InPlace, true, false, 0, 0, 0},
      {"ring fill 0.73, density 0.70", ringed(0, 4 * M, 0.73), dens70, true, 4096, true, Span, true, false, 0, 0, 0},
      // parent:1613 && fit_span(...): a span with no room is read in place, direct
      {"ring dense, span does not fit", ringed(0, 4 * M, 1.0), kDefault, true, 4096, false, InPlace, true, false, 0, 0, 0},
      // parent:1616 direct_max == 0: never direct; parent:1618 no split without ring_dma
      {"ring, direct_max 0", ringed(0, 4 * M, 0.5), dm0, true, 4096, true, InPlace, false, false, 0, 0, 0},
      // parent:1639 uniform && cnt > 1 && uni_len; parent:1649-1650 stride round16(len), 16 for 0
      {"staged uniform 60", staged(6400, true, 60), kDefault, false, 100, true, Direct, true, true, 60, 64, 0},
      {"staged uniform 64", staged(6400, true, 64), kDefault, false, 100, true, Direct, true, true, 64, 64, 0},
      {"staged uniform 0", staged(0, true, 0), kDefault, false, 100, true, Direct, true, true, 0, 16, 0},
      {"staged uniform, by DMA", staged(M + 64, true, 1500), kDefault, false, 1400, true, Dma, true, true, 1500, 1504, 0},
      // parent:1639 ring: uni_ptr && stride > 0; parent:1646-1647 first frame's place, the ring's stride
      {"ring uniform", ringed(4096, M, 0.73, true, true, 2048), kDefault, true, 1024, true, InPlace, true, true, 1500, 2048, 4096},
      {"ring equal lengths, irregular", ringed(4096, M, 0.73, true, false, 2048), kDefault, true, 1024, true, InPlace, true, false, 0, 0, 0},
      {"ring uniform, descending", ringed(4096, M, 0.73, true, true, -2048), kDefault, true, 1024, true, InPlace, true, false, 0, 0, 0},
      // parent:1639 uniform_chunks() off, cnt == 1
      {"uniform knob off", staged(6400, true, 60), nouni, false, 100, true, Direct, true, false, 0, 0, 0},
      {"one frame", staged(64, true, 60), kDefault, false, 1, true, Direct, true, false, 0, 0, 0},
  };
  for (const PlanRow &r : rows) {
    const ChunkPlan p = plan_transport(r.s, r.k, r.is_ring, r.cnt, r.span_fits);
    const bool ok = p.src == r.src && p.pcie == r.pcie && p.fixed == r.fixed &&
                    p.fixed_len == r.fixed_len && p.stride == r.stride && p.first_off == r.first_off;
    if (!ok) printf("plan row \"%s\": src %d pcie %d fixed %d len %u stride %llu first %zu\n", r.name,
                    (int)p.src, p.pcie, p.fixed, p.fixed_len, (unsigned long long)p.stride, p.first_off);
    CHECK(ok);
  }
}

int main() {
  staged_one_part(true);
  staged_one_part(false);
  staged_over_pool();
  ring_uniformity(64, nullptr, 1);
  ring_single();
  ring_bounds();
  {
    WorkerPool pool(3);
    ring_uniformity(16384, &pool, 8);
    ring_breaks(&pool);
  }
  plan_table();
  if (g_fail) return 1;
  printf("host_plan ok\n");
  return 0;
}
