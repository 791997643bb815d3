// host_plan.h -- the host-memory half of the host batch pipeline (rx_host.hip):
// the worker pool, a chunk's description and frame gather, the fold of its
// parts and the choice of its transport.  Plain C++17: no HIP include and no
// HIP type, so it builds with a host compiler alone and its decisions are
// pinned on a CPU (tests/c/host_plan_check.cc, also under ThreadSanitizer).
// Nothing here reads the environment: the knobs come in as a HostKnobs.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <emmintrin.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/ldp_packet.h"

namespace pptk {

// One part of a host chunk's descriptors: the staging bytes its frames take,
// a ring chunk's span and frame bytes, the longest frame.
struct PartDesc {
  size_t bytes = 0;
  size_t lo = SIZE_MAX, hi = 0, fbytes = 0;
  uint32_t maxlen = 0;
  // uniform frames: every frame of the part sz0 bytes (same), and at
  // p0 + k * stride (uni; k = its index in the part); each cleared at the
  // first frame that is not.  A staged chunk needs only `same` (the staging
  // puts equal frames at one stride), a ring chunk both.
  bool same = true, uni = true;
  uint32_t sz0 = 0;
  const uint8_t *p0 = nullptr;
  int64_t stride = 0;
  bool outside = false;   // a frame not (wholly) inside the candidate ring
};

// The context's host worker threads (opts.gather_threads - 1 of them, started
// on the first host batch and kept): parallel_for(n, f) runs f(0..n-1)
// across them and the calling thread and returns when all are done.  The
// staged path's frame gather and record copy-out use it; starting threads
// per chunk instead cost more than the copies for small frames.
class WorkerPool {
 public:
  explicit WorkerPool(size_t nworkers) {
    try {
      for (size_t t = 0; t < nworkers; ++t) th_.emplace_back([this] { loop(); });
    } catch (...) {   // a thread could not be started: stop the others
      shutdown();
      throw;
    }
  }
  ~WorkerPool() { shutdown(); }
  size_t size() const { return th_.size() + 1; }
  void parallel_for(size_t n, const std::function<void(size_t)> &f) {
    if (n == 0) return;
    uint64_t gen;
    {
      std::lock_guard<std::mutex> g(mu_);
      job_ = &f;
      n_ = n;
      next_ = 0;
      left_ = n;
      gen = ++gen_;
    }
    cv_.notify_all();
    work(gen);
    std::unique_lock<std::mutex> g(mu_);
    done_cv_.wait(g, [this] { return left_ == 0; });
    job_ = nullptr;
  }

 private:
  // Items are claimed under the mutex together with the job they belong to:
  // a worker still finishing generation k can never claim an index of
  // generation k + 1 (which starts only after every item of k completed) or
  // run one with a stale job pointer.  Items are ~256 frames or 1 MiB of
  // copying, so a lock per claim costs nothing measurable.
  void work(uint64_t gen) {
    std::unique_lock<std::mutex> g(mu_);
    for (;;) {
      if (gen_ != gen || next_ >= n_) return;
      const size_t i = next_++;
      const std::function<void(size_t)> *job = job_;
      g.unlock();
      (*job)(i);
      g.lock();
      if (--left_ == 0) done_cv_.notify_all();
    }
  }
  void loop() {
    uint64_t seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> g(mu_);
        cv_.wait(g, [&] { return stop_ || gen_ != seen; });
        if (stop_) return;
        seen = gen_;
      }
      work(seen);
    }
  }
  void shutdown() {
    {
      std::lock_guard<std::mutex> g(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    for (std::thread &t : th_) t.join();
    th_.clear();
  }
  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable cv_, done_cv_;
  const std::function<void(size_t)> *job_ = nullptr;
  size_t n_ = 0, left_ = 0, next_ = 0;
  uint64_t gen_ = 0;
  bool stop_ = false;
};

inline size_t pool_size(const WorkerPool *pool) { return pool ? pool->size() : 1; }

// The pipeline's knobs, read once by rx_host.hip (host_knobs) and passed in.
struct HostKnobs {
  size_t direct_max_bytes;   // staged bytes / ring span up to which a chunk runs "direct"
  double ring_dma_density;   // frame bytes / span from which a ring span goes down by DMA
  bool split;                // DMA chunks keep descriptors and records on PCIe
  bool uniform;              // uniform chunks run as fixed-stride batches
  bool nt_gather;            // stage_frame instead of memcpy
};

// A slot's host staging: frame bytes, the 10-byte descriptors, the parts of
// the chunk being described and their running staging totals.
struct StageView {
  uint8_t *h_frames;
  uint64_t *h_off;
  uint16_t *h_len;
  std::vector<PartDesc> &parts;
  std::vector<std::atomic<size_t>> &run;
};

// The registered ring a chunk's frames may be read from in place.
struct RingView {
  const uint8_t *host;
  size_t bytes;
};

// One chunk of a host batch: cnt >= 1 frames; a frame without data or longer
// than maxf is described as length 0.
struct ChunkIn {
  const struct ldp_packet *cp;
  size_t cnt;
  uint32_t maxf;
  const RingView *ring;   // nullptr: staged
};

// Copy one frame into 16-byte-aligned pinned staging with non-temporal
// stores: the lines go to memory without being read for ownership first
// and without staying dirty in the host caches, where the copy engine's
// reads of the staging would have to snoop them.  The bytes past the frame
// up to the next 16-byte boundary are zero (the kernel never uses them).
inline void stage_frame(uint8_t *dst, const uint8_t *src, size_t n) {
  size_t k = 0;
  for (; k + 16 <= n; k += 16)
    _mm_stream_si128((__m128i *)(dst + k), _mm_loadu_si128((const __m128i *)(src + k)));
  if (k < n) {
    alignas(16) uint8_t t[16] = {0};
    memcpy(t, src + k, n - k);
    _mm_stream_si128((__m128i *)(dst + k), _mm_load_si128((const __m128i *)t));
  }
}

// One part, frames [i0, i1): lengths (+ ring offsets / span) and the staging
// bytes it needs from `base` on; with `gather`, also the staging offsets and
// the frames.  write = false: a ring chunk's first pass -- the span, the
// checks, the uniformity -- with nothing written.
inline void describe_part(const StageView &v, const ChunkIn &c, bool nt, size_t i0, size_t i1,
                          size_t base, bool gather, bool write, PartDesc &d) {
  const struct ldp_packet *cp = c.cp;
  const RingView *ring = c.ring;
  size_t pos = base;
  if (i1 > i0) {
    d.p0 = (const uint8_t *)cp[i0].data;
    d.sz0 = cp[i0].sz;
    d.stride = i1 - i0 > 1 ? (const uint8_t *)cp[i0 + 1].data - d.p0 : 0;
    d.same = d.p0 != nullptr && d.sz0 <= c.maxf;
    d.uni = d.same;
  }
  for (size_t i = i0; i < i1; ++i) {
    const struct ldp_packet &pk = cp[i];
    const bool ok = pk.data && pk.sz <= c.maxf;
    const uint32_t sz = ok ? pk.sz : 0u;
    d.same = d.same && ok && pk.sz == d.sz0;
    d.uni = d.uni && d.same && (const uint8_t *)pk.data == d.p0 + (int64_t)(i - i0) * d.stride;
    if (write) v.h_len[i] = (uint16_t)sz;
    if (ring) {
      const uint8_t *pd = (const uint8_t *)pk.data;
      // (every frame's chunk-rounded end inside the registered region)
      d.outside = d.outside || (pd && (pd < ring->host ||
                                       (((size_t)(pd - ring->host) + pk.sz + 15) & ~(size_t)15) >
                                           ring->bytes));
      const uint64_t o = pd ? (uint64_t)(pd - ring->host) : 0u;
      if (write) v.h_off[i] = o;
      d.lo = std::min<size_t>(d.lo, o);
      // (the frame's chunk-rounded END, clamped to the region: a span
      // copy must not read past the registered memory; the kernel's reads
      // past a frame's end stay inside the span's 16-byte slack)
      d.hi = std::max<size_t>(d.hi, std::min<size_t>((o + sz + 15) & ~(size_t)15, ring->bytes));
      d.fbytes += sz;
    } else if (gather) {
      v.h_off[i] = pos;
      if (sz && nt) stage_frame(v.h_frames + pos, (const uint8_t *)pk.data, sz);
      else if (sz) memcpy(v.h_frames + pos, pk.data, sz);
    }
    pos += (sz + 15) & ~(size_t)15;
    d.maxlen = std::max(d.maxlen, sz);
  }
  d.bytes = pos - base;
  // this thread's streaming stores, before the copy is queued
  if (gather && nt) _mm_sfence();
}

// Parts a chunk is described in.  The pool only for big chunks: waking it
// costs ~20-40 us, more than a 256-frame or even a 1.5 MB gather saves
// (DESIGN.md "End-to-end").  Staged chunks: parts of ~1024 frames or ~256 KB
// of frame bytes (estimated from the first frame); ring chunks (no gather):
// parts of ~2048 frames; at most 8 per thread.
inline size_t part_count(const ChunkIn &c, const WorkerPool *pool) {
  const size_t cnt = c.cnt, est = cnt * (size_t)std::min<uint32_t>(c.cp[0].sz, c.maxf);
  size_t nparts = 1;
  if (pool && !c.ring && (cnt >= 8192 || est >= (4u << 20)))
    nparts = std::max(cnt / 1024, est >> 18);
  else if (pool && c.ring && cnt >= 16384)
    nparts = cnt / 2048;
  return std::max<size_t>(1, std::min<size_t>(nparts, std::min<size_t>(8 * pool_size(pool), cnt)));
}

// What a chunk's parts add up to.
struct ChunkSums {
  size_t bytes = 0;                            // staging bytes (16-byte-rounded frames)
  size_t lo = SIZE_MAX, hi = 0, fbytes = 0;    // ring: the span and the frame bytes in it
  uint32_t maxlen = 0;
  bool outside = false;                        // ring: a frame not wholly inside it
  // every frame ulen bytes (uni_len) and, from the first, `stride` apart
  // (uni_ptr); first_off = the first frame's place in the ring (staged: 0)
  bool uni_len = false, uni_ptr = false;
  uint32_t ulen = 0;
  int64_t stride = 0;
  size_t first_off = 0;
};

// The one fold over the parts (part t holds frames [cnt * t / n, cnt * (t + 1) / n)).
inline ChunkSums fold_parts(const std::vector<PartDesc> &parts, const ChunkIn &c) {
  ChunkSums s;
  const PartDesc &f = parts[0];
  const size_t n = parts.size();
  s.uni_len = s.uni_ptr = true;
  s.ulen = f.sz0;
  s.stride = f.stride;
  s.first_off = c.ring && f.p0 ? (size_t)(f.p0 - c.ring->host) : 0;
  for (size_t t = 0; t < n; ++t) {
    const PartDesc &d = parts[t];
    s.bytes += d.bytes;
    s.lo = std::min(s.lo, d.lo);
    s.hi = std::max(s.hi, d.hi);
    s.fbytes += d.fbytes;
    s.maxlen = std::max(s.maxlen, d.maxlen);
    s.outside = s.outside || d.outside;
    const size_t i0 = c.cnt * t / n;
    s.uni_len = s.uni_len && d.same && d.sz0 == f.sz0;
    // (each part's own stride, and its first frame where the first part's
    // stride puts it; one-frame parts have no stride of their own)
    s.uni_ptr = s.uni_ptr && s.uni_len && d.uni &&
                (d.stride == s.stride || c.cnt * (t + 1) / n - i0 == 1) &&
                d.p0 == f.p0 + (int64_t)i0 * s.stride;
  }
  if (c.cnt == 1) s.uni_ptr = false;
  return s;
}

// Uniform chunk: every frame the same length (and, in a registered ring, at
// one fixed stride from the first): it runs as a fixed-stride batch -- no
// descriptor is read by the kernel (in a staged chunk the frames sit at
// 16-byte-rounded offsets, i.e. at a fixed stride already), and frames of at
// most 64 bytes take the lane kernel.  A C64 chunk then moves its frames and
// its records over PCIe and nothing else.
inline bool fixed_stride(const ChunkSums &s, const HostKnobs &k, bool is_ring, size_t cnt) {
  return k.uniform && cnt > 1 && s.uni_len && (!is_ring || (s.uni_ptr && s.stride > 0));
}

// Describe the chunk into the staging and, staged, gather its frames.  On one
// thread (no pool, or a small chunk) in one pass.  Ring chunks: a first pass
// with nothing written; a chunk with a frame outside the ring is returned as
// such (the caller stages it), a uniform one needs no descriptors at all,
// any other gets them in a second pass.  Staged chunks over the pool: ONE
// pass -- each part sums its staging bytes, takes its base from the previous
// part's published running total (parts are claimed in order, so that one is
// done or in progress), publishes its own, then writes its offsets and
// gathers (a serial descriptor pass had cost a 65 536-frame C64 chunk as much
// as the whole parallel gather, DESIGN.md "End-to-end").
inline ChunkSums describe_chunk(const StageView &v, const ChunkIn &c, const HostKnobs &k,
                                WorkerPool *pool) {
  const size_t cnt = c.cnt, nparts = part_count(c, pool);
  const bool nt = k.nt_gather;
  std::vector<PartDesc> &parts = v.parts;
  parts.assign(nparts, PartDesc{});
  if (c.ring) {
    auto pass = [&](bool write) {
      auto part = [&](size_t t) {
        parts[t] = PartDesc{};
        describe_part(v, c, nt, cnt * t / nparts, cnt * (t + 1) / nparts, 0, false, write, parts[t]);
      };
      if (nparts == 1) part(0);
      else pool->parallel_for(nparts, part);
    };
    pass(false);
    const ChunkSums s = fold_parts(parts, c);
    if (!s.outside && !fixed_stride(s, k, true, cnt)) pass(true);   // (the same sums again)
    return s;
  }
  if (nparts == 1) {
    describe_part(v, c, nt, 0, cnt, 0, true, true, parts[0]);
    return fold_parts(parts, c);
  }
  if (v.run.size() < nparts) v.run = std::vector<std::atomic<size_t>>(nparts);
  std::atomic<size_t> *run = v.run.data();
  for (size_t t = 0; t < nparts; ++t) run[t].store(SIZE_MAX, std::memory_order_relaxed);
  pool->parallel_for(nparts, [&](size_t t) {
    const size_t i0 = cnt * t / nparts, i1 = cnt * (t + 1) / nparts;
    describe_part(v, c, nt, i0, i1, 0, false, true, parts[t]);   // lengths, this part's bytes
    size_t base = 0;
    if (t > 0)
      while ((base = run[t - 1].load(std::memory_order_acquire)) == SIZE_MAX) _mm_pause();
    run[t].store(base + parts[t].bytes, std::memory_order_release);
    PartDesc d2{};
    describe_part(v, c, nt, i0, i1, base, true, true, d2);   // offsets + gather
  });
  return fold_parts(parts, c);
}

// Where the kernel reads the chunk's frames.
enum class FramesSrc {
  RingInPlace,    // the registered ring, over PCIe
  RingSpanDma,    // the ring's span [lo, hi) copied down as one piece
  StagedDirect,   // the pinned staging, over PCIe ("direct")
  StagedDma,      // the staging copied down
};

struct ChunkPlan {
  FramesSrc src;
  bool pcie;    // descriptors read from, records written to pinned memory over PCIe
  bool fixed;   // fixed-stride batch, no descriptors: fixed_len, stride, first_off
  uint32_t fixed_len;
  uint64_t stride;
  size_t first_off;
};

// The chunk's transport.  Chunks run "direct" -- one kernel launch instead
// of three host-to-device copies, the launch and a device-to-host copy --
// when the frames come from a registered ring (the kernel reads them over
// PCIe anyway) or the staged frame bytes are at most direct_max_bytes.  A
// ring chunk whose frames lie densely in a span above that goes down as one
// span by DMA (span_fits: the device buffer has room).  Chunks that go down
// by DMA keep descriptors and records on PCIe ("split"): the copy engine
// then runs nothing but frame copies back to back.
inline ChunkPlan plan_transport(const ChunkSums &s, const HostKnobs &k, bool is_ring, size_t cnt,
                                bool span_fits) {
  const bool ring_dma = is_ring && s.hi > s.lo && s.hi - s.lo > k.direct_max_bytes &&
                        (double)s.fbytes >= k.ring_dma_density * (double)(s.hi - s.lo) && span_fits;
  const bool direct = is_ring ? k.direct_max_bytes > 0 && !ring_dma : s.bytes <= k.direct_max_bytes;
  const bool split = !direct && (ring_dma || !is_ring) && k.split;
  ChunkPlan p{};
  p.src = is_ring ? (ring_dma ? FramesSrc::RingSpanDma : FramesSrc::RingInPlace)
                  : (direct ? FramesSrc::StagedDirect : FramesSrc::StagedDma);
  p.pcie = direct || split;
  p.fixed = fixed_stride(s, k, is_ring, cnt);
  if (p.fixed) {
    // staged frames at i * round16(len); ring frames at the first frame's
    // place + i * stride
    p.fixed_len = s.ulen;
    p.stride = is_ring ? (uint64_t)s.stride : std::max<uint64_t>((s.ulen + 15u) & ~15u, 16);
    p.first_off = s.first_off;
  }
  return p;
}

}  // namespace pptk
