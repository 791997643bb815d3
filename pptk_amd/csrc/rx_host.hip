// rx_host.hip -- the host-buffer batch pipeline of libpptkrx.so: the entry
// points an LDP rx loop calls between ldp_in_nextpkts() and
// ldp_in_deallocate_some() (reference ldp/ldprecv.c:60-70), and the ring
// registration.  A call is cut into chunks; each is described and planned by
// plain host code (host_plan.h) and issued here on a slot's stream: the
// copies, pptk_rx_batch_device, the record copy.  Errors: 0 or -errno.
#include <errno.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "host_plan.h"
#include "rx_internal.h"

using namespace pptk;

// One slot of the host-batch pipeline: pinned staging, device copies, and
// the chunk currently in flight on its stream.
struct RxSlot {
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  size_t cap_pkts = 0, cap_bytes = 0;
  size_t dev_cap = 0;   // d_frames bytes (grown for registered-ring spans)
  uint8_t *h_frames = nullptr, *d_frames = nullptr;
  uint64_t *h_off = nullptr, *d_off = nullptr;
  uint16_t *h_len = nullptr, *d_len = nullptr;
  pptk_rx_rec *h_recs = nullptr, *d_recs = nullptr;
  // device addresses of the pinned h_* buffers (direct small chunks)
  uint8_t *hd_frames = nullptr;
  uint64_t *hd_off = nullptr;
  uint16_t *hd_len = nullptr;
  pptk_rx_rec *hd_recs = nullptr;
  void *out = nullptr;   // caller's records of the chunk in flight
  size_t count = 0;
  size_t rec_bytes = 64;   // of the chunk in flight: 64 (pptk_rx_rec) or 32 (pptk_rx_rec32)
  bool busy = false;
  std::vector<PartDesc> parts;             // describe_chunk's per-part sums
  std::vector<std::atomic<size_t>> run;    // and the parts' running staging totals
};

// A host rx ring registered for zero-copy reads (hipHostRegister, mapped).
struct RxRing {
  uint8_t *host;
  size_t bytes;
  const uint8_t *dev;
};

// The pipeline's state in a context: pptk_rx_batch rotates over the first
// sync_slots() slots, pptk_rx_batch_submit over all of them (allocated on
// first use).
struct pptk::HostPipe {
  RxSlot slot[PPTK_RX_MAX_INFLIGHT];
  int async_head = 0;  // slot of the oldest outstanding submission
  int async_n = 0;     // outstanding submissions (0..PPTK_RX_MAX_INFLIGHT)
  std::vector<RxRing> rings;
  WorkerPool *pool = nullptr;   // started by the first host batch
};

static void free_slot(RxSlot &sl) {
  if (sl.stream) (void)hipStreamSynchronize(sl.stream);
  if (sl.done) (void)hipEventDestroy(sl.done);
  if (sl.stream) (void)hipStreamDestroy(sl.stream);
  (void)hipHostFree(sl.h_frames);
  (void)hipHostFree(sl.h_off);
  (void)hipHostFree(sl.h_len);
  (void)hipHostFree(sl.h_recs);
  (void)hipFree(sl.d_frames);
  (void)hipFree(sl.d_off);
  (void)hipFree(sl.d_len);
  (void)hipFree(sl.d_recs);
  sl = RxSlot();
}

namespace pptk {
HostPipe *host_pipe_create() { return new (std::nothrow) HostPipe(); }
void host_pipe_release(HostPipe *hp) {
  for (RxSlot &sl : hp->slot) free_slot(sl);
  delete hp->pool;
  hp->pool = nullptr;
}
void host_pipe_destroy(HostPipe *hp) {
  for (const RxRing &r : hp->rings) (void)hipHostUnregister(r.host);
  delete hp;
}
}  // namespace pptk

static int ensure_slot(const pptk_rx_opts &o, RxSlot &sl, size_t pkts, size_t bytes) {
  if (sl.stream && pkts <= sl.cap_pkts && bytes <= sl.cap_bytes) return 0;
  free_slot(sl);
  pkts = std::max(pkts, (size_t)o.max_batch);
  bytes = std::max(bytes, (size_t)o.max_batch * ((o.max_frame + 15) & ~15u)) + 64;
  if (hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&sl.done, hipEventDisableTiming) != hipSuccess ||
      hipHostMalloc((void **)&sl.h_frames, bytes, hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc((void **)&sl.h_off, pkts * 8, hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc((void **)&sl.h_len, pkts * 2, hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc((void **)&sl.h_recs, pkts * 64, hipHostMallocDefault) != hipSuccess ||
      hipMalloc((void **)&sl.d_frames, bytes) != hipSuccess ||
      hipMalloc((void **)&sl.d_off, pkts * 8) != hipSuccess ||
      hipMalloc((void **)&sl.d_len, pkts * 2) != hipSuccess ||
      hipMalloc((void **)&sl.d_recs, pkts * 64) != hipSuccess) {
    free_slot(sl);
    return -ENOMEM;
  }
  if (hipHostGetDevicePointer((void **)&sl.hd_frames, sl.h_frames, 0) != hipSuccess ||
      hipHostGetDevicePointer((void **)&sl.hd_off, sl.h_off, 0) != hipSuccess ||
      hipHostGetDevicePointer((void **)&sl.hd_len, sl.h_len, 0) != hipSuccess ||
      hipHostGetDevicePointer((void **)&sl.hd_recs, sl.h_recs, 0) != hipSuccess) {
    free_slot(sl);
    return -EIO;
  }
  sl.cap_pkts = pkts;
  sl.cap_bytes = bytes;
  sl.dev_cap = bytes;
  return 0;
}

// Room for a registered-ring span of `bytes` in the slot's device frame
// buffer (the slot is idle: its last chunk was retired).  Sparse rings
// (e.g. 2 KB netmap slots) have spans longer than max_batch * max_frame;
// grown up to 4x the staging size, once.
static bool fit_span(RxSlot &sl, size_t bytes) {
  if (bytes <= sl.dev_cap) return true;
  if (bytes > 4 * sl.cap_bytes) return false;
  uint8_t *p = nullptr;
  if (hipMalloc((void **)&p, bytes) != hipSuccess) return false;
  (void)hipFree(sl.d_frames);
  sl.d_frames = p;
  sl.dev_cap = bytes;
  return true;
}

// The knobs of host_plan.h's decisions, read once (DESIGN.md "End-to-end").
// PPTK_RX_DIRECT_MAX_BYTES, 2 MiB: with four chunks in flight the DMA copy
// beats the kernel's PCIe reads from there on (1 M-frame C64 calls 375 -> 449
// Mpkt/s staged, ring spans 325 -> 408; 4 096-frame C1500 calls 278 -> 238
// us), while calls of up to ~1 400 1500-byte frames keep the single launch.
// PPTK_RX_RING_DMA_PCT (percent; 0 = always, > 100 = never): a dense span
// moves ~48 GB/s of frames by DMA, the kernel's own reads of host memory
// ~37-38, so the break-even is near 80 % (1500-byte frames in 2 KB netmap
// slots, 73 %, measured 37 GB/s by DMA against 38 in place).
// split, uniform and nt_gather are always on: without the split the
// descriptor and record copies cost ~0.18 ms of copy-engine time per
// 65 536-frame chunk beside its 2.2 ms frame copy.
static const HostKnobs &host_knobs() {
  static const HostKnobs k = {
      (size_t)std::max(0l, env_long("PPTK_RX_DIRECT_MAX_BYTES", 2l << 20)),
      env_long("PPTK_RX_RING_DMA_PCT", 80) / 100.0,
      true,   // split
      true,   // uniform
      true,   // nt_gather
  };
  return k;
}

// The context's worker pool (nullptr with gather_threads <= 1).  If the
// threads cannot be started the batch runs on the calling thread alone (and
// later batches try again): no exception leaves the C ABI.
static WorkerPool *pool_of(HostPipe *hp, const pptk_rx_opts &o) {
  const size_t nth = std::max<size_t>(1, std::min<size_t>(o.gather_threads, 64));
  if (nth > 1 && !hp->pool) {
    try {
      hp->pool = new WorkerPool(nth - 1);
    } catch (...) {
      hp->pool = nullptr;
    }
  }
  return hp->pool;
}

// Copy n bytes, split over the pool when it pays (a few MB and up; 256 KB
// pieces measured slower than 1 MB ones on C64 chunks: the pool's per-item
// cost).
static void copy_out(WorkerPool *pool, void *dst, const void *src, size_t n) {
  constexpr size_t kPiece = 1u << 20;
  if (!pool || n < 2 * kPiece) {
    memcpy(dst, src, n);
    return;
  }
  const size_t parts = (n + kPiece - 1) / kPiece;
  pool->parallel_for(parts, [&](size_t i) {
    const size_t lo = i * kPiece, hi = std::min(n, lo + kPiece);
    memcpy((uint8_t *)dst + lo, (const uint8_t *)src + lo, hi - lo);
  });
}

// Wait for the slot's chunk and hand its records to the caller.
static int retire(RxSlot &sl, WorkerPool *pool) {
  if (!sl.busy) return 0;
  sl.busy = false;
  // (HIP spins before it blocks: polling hipEventQuery instead measured
  // equal on 32-frame chunks)
  if (hipEventSynchronize(sl.done) != hipSuccess) return -EIO;
  if (sl.out) copy_out(pool, sl.out, sl.h_recs, sl.count * sl.rec_bytes);
  return 0;
}

// The registered ring holding the call's first frame, the candidate for
// reading the frames in place; every chunk checks its own frames against it
// in its descriptor pass (describe_chunk) and is staged instead when one lies
// outside.  (A serial pass over all frames here, before the first chunk,
// had cost a 4 M-frame C64 call as much as its frame copies.)
static const RxRing *ring_of(const HostPipe *hp, const struct ldp_packet *pkts, int num) {
  if (hp->rings.empty() || num <= 0) return nullptr;
  const uint8_t *p0 = (const uint8_t *)pkts[0].data;
  for (const RxRing &r : hp->rings)
    if (p0 >= r.host && p0 < r.host + r.bytes) return &r;
  return nullptr;
}

// The registered region holding the caller's whole record array, so that
// the kernel writes the records there in place over PCIe (no record copy
// from the staging); NULL otherwise.
static const RxRing *records_region(const HostPipe *hp, const void *recs, size_t bytes) {
  const uint8_t *p = (const uint8_t *)recs;
  for (const RxRing &r : hp->rings)
    if (p >= r.host && bytes <= r.bytes && (size_t)(p - r.host) <= r.bytes - bytes) return &r;
  return nullptr;
}

// A chunk that failed part-way: nothing it queued may still run (it may
// read the caller's frames or write the slot) when the error is returned.
static int chunk_failed(RxSlot &sl, int rc) {
  (void)hipStreamSynchronize(sl.stream);
  sl.busy = false;
  return rc;
}

// Staging bytes a slot needs for one chunk of this context's batches.
static size_t chunk_bytes(const pptk_rx_opts &o) {
  const uint32_t maxf = o.max_frame ? o.max_frame : 65535u;
  return std::max<size_t>(o.max_batch, 1) * ((maxf + 15) & ~15u);
}

// One chunk of a host batch (cnt <= opts.max_batch frames) into slot `sl`,
// idle and sized by ensure_slot: described, planned, then its copies, the
// launch and the record copy-back queued on the slot's stream, nothing
// waited for.  retire() waits for it and hands the records to `out`.  In a
// registered ring the kernel reads the frames in place over PCIe (or the
// span goes down by DMA) and only the 10-byte descriptors are written.
static int enqueue_chunk(pptk_rx_ctx *c, RxSlot &sl, const struct ldp_packet *cp, size_t cnt,
                         void *out, size_t rec_bytes, const RxRing *ring, const RxRing *rreg,
                         WorkerPool *pool) {
  const pptk_rx_opts &o = ctx_opts(c);
  const HostKnobs &k = host_knobs();
  // 1. describe (and gather)
  const RingView rv = {ring ? ring->host : nullptr, ring ? ring->bytes : 0};
  ChunkIn in = {cp, cnt, o.max_frame ? o.max_frame : 65535u, ring ? &rv : nullptr};
  ChunkSums sums = describe_chunk({sl.h_frames, sl.h_off, sl.h_len, sl.parts, sl.run}, in, k, pool);
  if (sums.outside) {   // staged instead (the slot is idle: size its staging)
    const int rc = ensure_slot(o, sl, std::max<size_t>(o.max_batch, 1), chunk_bytes(o));
    if (rc != 0) return rc;
    ring = nullptr;
    in.ring = nullptr;
    sums = describe_chunk({sl.h_frames, sl.h_off, sl.h_len, sl.parts, sl.run}, in, k, pool);
  }
  // 2. plan (a span the device buffer cannot take is read in place)
  ChunkPlan p = plan_transport(sums, k, ring != nullptr, cnt, true);
  const size_t lo = sums.lo, span = sums.hi - sums.lo;
  if (p.src == FramesSrc::RingSpanDma && !fit_span(sl, span + 16))
    p = plan_transport(sums, k, true, cnt, false);
  // 3. the batch; a span's buffer is seen shifted down by `lo`, so the ring
  // offsets stay as they are
  pptk_rx_dev_batch b;
  memset(&b, 0, sizeof(b));
  switch (p.src) {
    case FramesSrc::RingInPlace: b.d_frames = ring->dev; break;
    case FramesSrc::RingSpanDma: b.d_frames = (const uint8_t *)((uintptr_t)sl.d_frames - lo); break;
    case FramesSrc::StagedDirect: b.d_frames = sl.hd_frames; break;
    case FramesSrc::StagedDma: b.d_frames = sl.d_frames; break;
  }
  b.max_len = sums.maxlen;
  b.n = cnt;
  if (p.fixed) {
    b.d_frames += p.first_off;
    b.fixed_len = p.fixed_len;
    b.stride = p.stride;
  } else {
    b.d_off = p.pcie ? sl.hd_off : sl.d_off;
    b.d_len = p.pcie ? sl.hd_len : sl.d_len;
  }
  // records: into the caller's array itself when it is registered
  void *d_out = rreg     ? (void *)(rreg->dev + ((const uint8_t *)out - rreg->host))
                : p.pcie ? (void *)sl.hd_recs
                         : (void *)sl.d_recs;
  if (rec_bytes == 32) b.d_recs32 = (pptk_rx_rec32 *)d_out;   // compact records
  else b.d_recs = (pptk_rx_rec *)d_out;
  // 4. queue
  hipStream_t s = sl.stream;
  if ((p.src == FramesSrc::StagedDma &&
       hipMemcpyAsync(sl.d_frames, sl.h_frames, std::max<size_t>(sums.bytes, 16),
                      hipMemcpyHostToDevice, s) != hipSuccess) ||
      (p.src == FramesSrc::RingSpanDma &&
       hipMemcpyAsync(sl.d_frames, ring->host + lo, span, hipMemcpyHostToDevice, s) != hipSuccess) ||
      (!p.pcie &&
       (hipMemcpyAsync(sl.d_off, sl.h_off, cnt * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(sl.d_len, sl.h_len, cnt * 2, hipMemcpyHostToDevice, s) != hipSuccess)))
    return chunk_failed(sl, -EIO);
  const int rc = pptk_rx_batch_device(c, &b, s);
  if (rc != 0) return chunk_failed(sl, rc);
  if ((!p.pcie && !rreg &&
       hipMemcpyAsync(sl.h_recs, sl.d_recs, cnt * rec_bytes, hipMemcpyDeviceToHost, s) !=
           hipSuccess) ||
      hipEventRecord(sl.done, s) != hipSuccess)
    return chunk_failed(sl, -EIO);
  sl.out = rreg ? nullptr : out;   // (retire copies only staged records)
  sl.rec_bytes = rec_bytes;
  sl.count = cnt;
  sl.busy = true;
  return 0;
}

// Slots a synchronous pptk_rx_batch rotates over (chunks in flight; a slot
// is allocated when a call first has that many chunks): four measured
// +17-24 % on 1 M-frame C64 calls against two, C1500 +1-2 % (at the PCIe
// ceiling either way; DESIGN.md "End-to-end").  PPTK_RX_SYNC_SLOTS (2 ..
// PPTK_RX_MAX_INFLIGHT) overrides.
static size_t sync_slots() {
  static const long v = env_long("PPTK_RX_SYNC_SLOTS", PPTK_RX_MAX_INFLIGHT);
  return (size_t)std::min<long>(std::max<long>(v, 2), PPTK_RX_MAX_INFLIGHT);
}

static bool host_args_ok(const pptk_rx_ctx *c, const struct ldp_packet *pkts, int num,
                         const void *recs) {
  return c && num >= 0 && (num == 0 || (pkts && recs));
}

// pptk_rx_batch / pptk_rx_batch32: records of rec_bytes (64 or 32) each.
static int host_batch(struct pptk_rx_ctx *c, const struct ldp_packet *pkts, int num, void *recs,
                      size_t rec_bytes) {
  if (!host_args_ok(c, pkts, num, recs)) return -EINVAL;
  if (num == 0) return 0;
  HostPipe *hp = ctx_host_pipe(c);
  const pptk_rx_opts &o = ctx_opts(c);
  if (hp->async_n) return -EBUSY;   // the submissions own the slots
  DeviceScope dg(ctx_device(c));
  if (!dg.ok) return -EIO;
  WorkerPool *pool = pool_of(hp, o);
  const RxRing *ring = ring_of(hp, pkts, num);
  const RxRing *rreg = records_region(hp, recs, (size_t)num * rec_bytes);
  const size_t chunk = std::max<size_t>(o.max_batch, 1);
  int rc = 0;
  // Multi-buffered: while chunk k runs on one slot's stream (H2D, kernel,
  // D2H), the host gathers the next chunks into the other slots.
  const size_t nslots = sync_slots();
  size_t k = 0, cnt = 0;
  for (size_t first = 0; first < (size_t)num && rc == 0; first += cnt, ++k) {
    RxSlot &sl = hp->slot[k % nslots];
    if ((rc = retire(sl, pool)) != 0) break;
    cnt = std::min(chunk, (size_t)num - first);
    if ((rc = ensure_slot(o, sl, chunk, ring ? 64 : chunk_bytes(o))) != 0) break;
    rc = enqueue_chunk(c, sl, pkts + first, cnt, (uint8_t *)recs + first * rec_bytes, rec_bytes,
                       ring, rreg, pool);
  }
  // drain (also on error: nothing may still read the caller's buffers)
  for (RxSlot &sl : hp->slot) {
    const int r2 = retire(sl, pool);
    if (rc == 0) rc = r2;
  }
  return rc;
}

static int host_submit(struct pptk_rx_ctx *c, const struct ldp_packet *pkts, int num, void *recs,
                       size_t rec_bytes) {
  if (!host_args_ok(c, pkts, num, recs)) return -EINVAL;
  if (num == 0) return 0;
  HostPipe *hp = ctx_host_pipe(c);
  const pptk_rx_opts &o = ctx_opts(c);
  if ((size_t)num > std::max<size_t>(o.max_batch, 1)) return -EINVAL;
  if (hp->async_n >= PPTK_RX_MAX_INFLIGHT) return -EBUSY;
  DeviceScope dg(ctx_device(c));
  if (!dg.ok) return -EIO;
  const RxRing *ring = ring_of(hp, pkts, num);
  const RxRing *rreg = records_region(hp, recs, (size_t)num * rec_bytes);
  // the slots rotate in submission order (FIFO), so consecutive
  // submissions run on different streams and may overlap on the GPU
  RxSlot &sl = hp->slot[(hp->async_head + hp->async_n) % PPTK_RX_MAX_INFLIGHT];
  int rc = ensure_slot(o, sl, std::max<size_t>(o.max_batch, 1), ring ? 64 : chunk_bytes(o));
  if (rc == 0)
    rc = enqueue_chunk(c, sl, pkts, (size_t)num, recs, rec_bytes, ring, rreg, pool_of(hp, o));
  if (rc != 0) return rc;
  ++hp->async_n;
  return 0;
}

extern "C" {

int pptk_rx_register_ring(struct pptk_rx_ctx *c, void *base, size_t bytes) {
  if (!c || !base || bytes == 0) return -EINVAL;
  DeviceScope dg(ctx_device(c));
  if (!dg.ok) return -EIO;
  if (hipHostRegister(base, bytes, hipHostRegisterMapped) != hipSuccess) return -EIO;
  void *dev = nullptr;
  if (hipHostGetDevicePointer(&dev, base, 0) != hipSuccess) {
    (void)hipHostUnregister(base);
    return -EIO;
  }
  ctx_host_pipe(c)->rings.push_back(RxRing{(uint8_t *)base, bytes, (const uint8_t *)dev});
  return 0;
}

int pptk_rx_unregister_ring(struct pptk_rx_ctx *c, void *base) {
  if (!c || !base) return -EINVAL;
  HostPipe *hp = ctx_host_pipe(c);
  for (size_t i = 0; i < hp->rings.size(); ++i) {
    if (hp->rings[i].host == (uint8_t *)base) {
      DeviceScope dg(ctx_device(c));
      if (!dg.ok) return -EIO;
      for (RxSlot &sl : hp->slot)   // no chunk may still read the ring
        if (sl.stream) (void)hipStreamSynchronize(sl.stream);
      (void)hipHostUnregister(base);
      hp->rings.erase(hp->rings.begin() + (long)i);
      return 0;
    }
  }
  return -EINVAL;
}

int pptk_rx_batch(struct pptk_rx_ctx *c, const struct ldp_packet *pkts, int num,
                  struct pptk_rx_rec *recs) {
  return host_batch(c, pkts, num, recs, sizeof(pptk_rx_rec));
}

int pptk_rx_batch32(struct pptk_rx_ctx *c, const struct ldp_packet *pkts, int num,
                    struct pptk_rx_rec32 *recs) {
  return host_batch(c, pkts, num, recs, sizeof(pptk_rx_rec32));
}

int pptk_rx_batch_submit(struct pptk_rx_ctx *c, const struct ldp_packet *pkts, int num,
                         struct pptk_rx_rec *recs) {
  return host_submit(c, pkts, num, recs, sizeof(pptk_rx_rec));
}

int pptk_rx_batch_submit32(struct pptk_rx_ctx *c, const struct ldp_packet *pkts, int num,
                           struct pptk_rx_rec32 *recs) {
  return host_submit(c, pkts, num, recs, sizeof(pptk_rx_rec32));
}

int pptk_rx_batch_complete(struct pptk_rx_ctx *c) {
  if (!c) return -EINVAL;
  HostPipe *hp = ctx_host_pipe(c);
  if (hp->async_n == 0) return -ENOENT;
  DeviceScope dg(ctx_device(c));
  if (!dg.ok) return -EIO;
  RxSlot &sl = hp->slot[hp->async_head];
  const int cnt = (int)sl.count;
  const int rc = retire(sl, hp->pool);
  // (dropped from the queue even on an error: its slot is idle again)
  hp->async_head = (hp->async_head + 1) % PPTK_RX_MAX_INFLIGHT;
  --hp->async_n;
  return rc ? rc : cnt;
}

int pptk_rx_batch_pending(const struct pptk_rx_ctx *c) {
  return c ? ctx_host_pipe(c)->async_n : -EINVAL;
}

}  // extern "C"
