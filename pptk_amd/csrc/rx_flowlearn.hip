// rx_flowlearn.hip -- the device half of "Flow learning" (include/pptk_rx.h):
// pptk_flow_learn_device, which turns the status bytes of a lookup into the
// report of the batch's new flows -- one entry per flow, the record of its
// first frame, that frame's index and the flow's packet count, in ascending
// frame order.  host/flowlearn.c holds the CPU statement
// (pptk_flow_learn_host); the device call equals it byte for byte.
//
// The status array (1 B per frame) is the only thing read for all n frames;
// records are read for considered candidates only.  Two ordered compactions
// around a hash set, eight launches on the caller's stream:
//   clear    the set's slots = {tag empty, first 0xffffffff, count 0}
//   count    candidates per block of kFrames frames (16-byte status loads in
//            the aligned numbering j = i + phase, bytewise head and tail)
//   scan     one workgroup turns the block counts into exclusive prefixes,
//            kScan counts per round; writes hdr.candidates / .considered
//   compact  cand[rank] = i for rank < max_candidates
//   insert   lane r < considered puts flow_hash of recs[cand[r]] into the
//            set: an open-addressed array of {u64 tag, u32 first, u32 count}
//            slots, home = low hash word & (slots - 1), linear probing; a
//            slot is claimed by a 64-bit compare-and-swap on the tag and
//            first = min(first, r).  A hash that equals the empty tag lives
//            in one spare slot behind the array.
//   resolve  lane r finds its slot, L = first, and compares its 37 key bytes
//            with those of recs[cand[L]]: equal -> count += 1, a leader iff
//            r == L; different -> a leader of its own with count 1.  Writes
//            lead[r] and the leaders per block of kBlock lanes.
//   scan     the leader counts; writes hdr.flows / .written
//   emit     leaders write record, first and packets at their rank < cap
// The passes are ordered by kernel boundaries only: no lane ever waits for
// another lane's store.  Every loop's trip count is a kernel argument (the
// probe loops: the slot count) or a device value clamped by one; a probe also
// ends at the first empty slot, and since at most slots / 2 distinct hashes
// enter, one always exists.  Tags never change once claimed, so a plain load
// ahead of the compare-and-swap is a safe hint; the swap's returned value
// decides.  All sums are integer and the set's content (first = a minimum,
// count = a sum) does not depend on arrival order: the report is the same for
// any grid and any interleaving.
#include <errno.h>

#include "block_scan.h"
#include "copy16.h"
#include "rx_internal.h"
#include "scratch_carve.h"

namespace pptk {
namespace {

constexpr int kBlock = 256;
constexpr uint32_t kFrames = 16 * kBlock;   // frames per block of count / compact: one 16-byte load per lane
constexpr int kScan = 1024;                 // counts per round of the scan's one workgroup
constexpr uint32_t kMaxGrid = 1u << 16;
constexpr uint64_t kEmptyTag = ~0ull;
constexpr uint32_t kNotLeader = 0xffffffffu;
constexpr uint32_t kAlone = 0xfffffffeu;    // a leader outside the set: count 1
constexpr uint64_t kMaxCand = 1ull << 30;

struct Slot {
  uint64_t tag;
  uint32_t first;   // smallest candidate rank that carried the tag
  uint32_t count;   // frames whose key equals that candidate's
};
static_assert(sizeof(Slot) == 16, "a slot is 16 bytes");

struct LearnArgs {
  const uint8_t *status;
  const pptk_rx_rec *recs;
  uint64_t n;
  uint32_t phase;     // address of status & 15: frame i is 16-byte aligned when (i + phase) % 16 == 0
  uint32_t maxc;      // min(max_candidates, n)
  uint32_t *blk;      // candidates per block, then their exclusive prefix
  uint32_t *cand;     // maxc frame indices
  uint32_t *lead;     // maxc codes: slot index, kAlone or kNotLeader
  uint32_t *lcnt;     // leaders per kBlock ranks, then their exclusive prefix
  Slot *slots;        // nslots + 1 (the spare)
  uint32_t nslots;    // a power of two >= 2 * maxc
  pptk_rx_rec *new_recs;
  uint32_t *first;    // nullable
  uint32_t *packets;  // nullable
  uint64_t cap;
  pptk_flow_learn_hdr *hdr;
};

__device__ __forceinline__ uint32_t cand_bits(uint32_t w) {
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) m |= (uint32_t)(((w >> (8 * k)) & 0xffu) == PPTK_FLOW_ST_SUBJECT) << k;
  return m;
}

// bit k: frame j0 + k - phase of this lane's 16 is a candidate
__device__ __forceinline__ uint32_t lane_candidates(const LearnArgs &a, uint64_t j0) {
  const uint64_t jend = a.n + a.phase;   // frames are j in [phase, jend)
  uint32_t m = 0;
  if (j0 >= a.phase && j0 + 16 <= jend) {
    const u32x4 w = *(const u32x4 *)(a.status + (j0 - a.phase));
    m = cand_bits(w.x) | cand_bits(w.y) << 4 | cand_bits(w.z) << 8 | cand_bits(w.w) << 12;
  } else if (j0 < jend) {
#pragma unroll 1
    for (uint32_t k = 0; k < 16; ++k) {
      const uint64_t j = j0 + k;
      if (j >= a.phase && j < jend)
        m |= (uint32_t)(a.status[j - a.phase] == PPTK_FLOW_ST_SUBJECT) << k;
    }
  }
  return m;
}

__global__ __launch_bounds__(kBlock) void learn_clear_kernel(Slot *slots, uint32_t count) {
  const uint32_t stride = gridDim.x * kBlock;
  for (uint32_t k = blockIdx.x * kBlock + threadIdx.x; k < count; k += stride)
    *(u32x4 *)(slots + k) = (u32x4){0xffffffffu, 0xffffffffu, 0xffffffffu, 0u};
}

__global__ __launch_bounds__(kBlock) void learn_count_kernel(LearnArgs a) {
  __shared__ uint32_t lds[kBlock / 64];
  const uint64_t j0 = (uint64_t)blockIdx.x * kFrames + 16u * threadIdx.x;
  uint32_t total;
  (void)block_excl_scan<kBlock / 64, uint32_t>(__popc(lane_candidates(a, j0)), lds, &total);
  if (threadIdx.x == 0) a.blk[blockIdx.x] = total;
}

// cnt[0 .. nb) -> exclusive prefixes; *out_total = the sum, *out_min = min(sum, limit).
// nb = nb_arg, or where `items` is given ceil(*items / per) if that is smaller.
__global__ __launch_bounds__(kScan) void learn_scan_kernel(uint32_t *cnt, uint32_t nb_arg,
                                                          const uint64_t *items, uint32_t per,
                                                          uint64_t limit, uint64_t *out_total,
                                                          uint64_t *out_min) {
  __shared__ uint32_t lds[kScan / 64];
  // the sum is at most n < 2^32, so every prefix fits the word
  const uint64_t running =
      scan_counts<kScan, uint32_t>(cnt, scan_extent(nb_arg, items, per), true, lds);
  if (threadIdx.x == 0) {
    *out_total = running;
    *out_min = running < limit ? running : limit;
  }
}

__global__ __launch_bounds__(kBlock) void learn_compact_kernel(LearnArgs a) {
  __shared__ uint32_t lds[kBlock / 64];
  const uint32_t base = a.blk[blockIdx.x];
  if (base >= a.maxc) return;   // (the whole workgroup) every rank here is past the bound
  const uint64_t j0 = (uint64_t)blockIdx.x * kFrames + 16u * threadIdx.x;
  uint32_t m = lane_candidates(a, j0);
  uint32_t total;
  // base + the block's count <= candidates < 2^32
  uint32_t rank = base + block_excl_scan<kBlock / 64, uint32_t>(__popc(m), lds, &total);
  while (m && rank < a.maxc) {   // at most 16 rounds: a bit leaves m in each
    const uint32_t k = __builtin_ctz(m);
    m &= m - 1;
    a.cand[rank++] = (uint32_t)(j0 + k - a.phase);
  }
}

__global__ __launch_bounds__(kBlock) void learn_insert_kernel(LearnArgs a) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= clamped_count(&a.hdr->considered, a.maxc)) return;
  const uint64_t h = a.recs[a.cand[r]].flow_hash;
  const uint32_t mask = a.nslots - 1;
  uint32_t s = (uint32_t)h & mask;
  if (h == kEmptyTag) {
    s = a.nslots;   // the spare slot: no tag to claim
  } else {
    bool found = false;
#pragma unroll 1
    for (uint32_t p = 0; p < a.nslots; ++p, s = (s + 1) & mask) {
      uint64_t cur = __hip_atomic_load(&a.slots[s].tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == kEmptyTag) {
        uint64_t expect = kEmptyTag;
        if (__hip_atomic_compare_exchange_strong(&a.slots[s].tag, &expect, h, __ATOMIC_RELAXED,
                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
          cur = h;
        else
          cur = expect;   // another lane claimed it, maybe for h
      }
      if (cur == h) {
        found = true;
        break;
      }
    }
    if (!found) return;   // not reached: at most nslots / 2 tags enter
  }
  (void)__hip_atomic_fetch_min(&a.slots[s].first, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kBlock) void learn_resolve_kernel(LearnArgs a) {
  __shared__ uint32_t lds[kBlock / 64];
  const uint32_t cons = clamped_count(&a.hdr->considered, a.maxc);
  if (blockIdx.x * kBlock >= cons) return;   // the whole workgroup
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  uint32_t code = kNotLeader;
  if (r < cons) {
    const u32x4 *me = (const u32x4 *)(a.recs + a.cand[r]);
    const u32x4 r0 = me[0], r1 = me[1], r2 = me[2], r3 = me[3];
    const uint64_t h = (uint64_t)r0.x | (uint64_t)r0.y << 32;
    const uint32_t mask = a.nslots - 1;
    uint32_t s = r0.x & mask;
    bool found = false;
    u32x4 sl = {0, 0, 0, 0};
    if (h == kEmptyTag) {
      s = a.nslots;
      sl = *(const u32x4 *)(a.slots + s);
      found = true;
    } else {
#pragma unroll 1
      for (uint32_t p = 0; p < a.nslots; ++p, s = (s + 1) & mask) {
        sl = *(const u32x4 *)(a.slots + s);
        const uint64_t tag = (uint64_t)sl.x | (uint64_t)sl.y << 32;
        if (tag == h) {
          found = true;
          break;
        }
        if (tag == kEmptyTag) break;
      }
    }
    code = kAlone;   // (a hash the insert pass did not leave cannot occur; it would report alone)
    if (found) {
      const uint32_t L = sl.z;
      bool same = L == r;
      if (!same && L < cons) {
        // 37 key bytes: record bytes 8..43 and proto (byte 53); the hashes are equal
        const u32x4 *q = (const u32x4 *)(a.recs + a.cand[L]);
        const u32x4 q0 = q[0], q1 = q[1], q2 = q[2];
        const uint32_t qp = q[3].y;
        same = q0.z == r0.z && q0.w == r0.w && q1.x == r1.x && q1.y == r1.y && q1.z == r1.z &&
               q1.w == r1.w && q2.x == r2.x && q2.y == r2.y && q2.z == r2.z &&
               ((qp ^ r3.y) & 0xff00u) == 0;
      }
      if (same) {
        (void)__hip_atomic_fetch_add(&a.slots[s].count, 1u, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
        code = L == r ? s : kNotLeader;
      }
    }
    a.lead[r] = code;
  }
  uint32_t total;
  (void)block_excl_scan<kBlock / 64, uint32_t>(code != kNotLeader, lds, &total);
  if (threadIdx.x == 0) a.lcnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void learn_emit_kernel(LearnArgs a) {
  __shared__ uint32_t lds[kBlock / 64];
  const uint32_t cons = clamped_count(&a.hdr->considered, a.maxc);
  if (blockIdx.x * kBlock >= cons) return;   // the whole workgroup
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t code = r < cons ? a.lead[r] : kNotLeader;
  uint32_t total;
  const uint64_t rank = (uint64_t)a.lcnt[blockIdx.x] +
                        block_excl_scan<kBlock / 64, uint32_t>(code != kNotLeader, lds, &total);
  if (code == kNotLeader || rank >= a.cap) return;
  const uint32_t i = a.cand[r];
  const u32x4 *src = (const u32x4 *)(a.recs + i);
  u32x4 *dst = (u32x4 *)(a.new_recs + rank);
  const u32x4 c0 = src[0], c1 = src[1], c2 = src[2], c3 = src[3];
  dst[0] = c0, dst[1] = c1, dst[2] = c2, dst[3] = c3;
  if (a.first) a.first[rank] = i;
  if (a.packets) a.packets[rank] = code == kAlone ? 1u : a.slots[code].count;
}

// the derived counts of a call
struct Layout {
  uint32_t maxc, nslots, nblk, nlblk;
};

bool layout_of(uint64_t n, uint64_t max_candidates, Layout *l) {
  if (n == 0 || n >= (1ull << 32) || max_candidates == 0 || max_candidates > kMaxCand)
    return false;
  l->maxc = (uint32_t)(max_candidates < n ? max_candidates : n);
  l->nslots = 2;
  while (l->nslots < 2ull * l->maxc) l->nslots <<= 1;
  l->nblk = (uint32_t)((n + 15 + kFrames - 1) / kFrames);   // whatever the phase of d_status
  l->nlblk = (l->maxc + kBlock - 1) / kBlock;
  return true;
}

// the scratch's arrays, in order: without a base the walk sizes the scratch,
// with the scratch pointer it binds the arguments
size_t carve(const Layout &l, void *base, LearnArgs *a) {
  Carve c(base, 256);
  a->blk = c.take<uint32_t>(l.nblk);
  a->cand = c.take<uint32_t>(l.maxc);
  a->lead = c.take<uint32_t>(l.maxc);
  a->lcnt = c.take<uint32_t>(l.nlblk);
  a->slots = c.take<Slot>((size_t)l.nslots + 1);
  return c.total();
}

}  // namespace
}  // namespace pptk

using namespace pptk;

extern "C" void pptk_flow_learn_shape(uint32_t *block_frames, uint32_t *scan_width) {
  if (block_frames) *block_frames = kFrames;
  if (scan_width) *scan_width = (uint32_t)kScan;
}

extern "C" size_t pptk_flow_learn_scratch_bytes(uint64_t n, uint64_t max_candidates) {
  Layout l;
  LearnArgs a;
  return layout_of(n, max_candidates, &l) ? carve(l, nullptr, &a) : 0;
}

extern "C" int pptk_flow_learn_device(struct pptk_rx_ctx *c, const struct pptk_rx_rec *d_recs,
                                      const uint8_t *d_status, uint64_t n,
                                      uint64_t max_candidates, struct pptk_rx_rec *d_new_recs,
                                      uint32_t *d_first, uint32_t *d_packets, uint64_t cap,
                                      struct pptk_flow_learn_hdr *d_hdr, void *d_scratch,
                                      size_t scratch_bytes, void *stream) {
  static_assert(sizeof(pptk_flow_learn_hdr) == 32, "the header is 32 bytes");
  static_assert(sizeof(pptk_rx_rec) == 64, "a record is 64 bytes");
  if (!c || n >= (1ull << 32) || max_candidates == 0 || max_candidates > kMaxCand) return -EINVAL;
  if (n && (!d_recs || !d_status || !d_hdr)) return -EINVAL;
  if (cap && !d_new_recs) return -EINVAL;
  if (((uintptr_t)d_recs & 15u) || ((uintptr_t)d_new_recs & 15u) || ((uintptr_t)d_hdr & 7u) ||
      ((uintptr_t)d_first & 3u) || ((uintptr_t)d_packets & 3u) || ((uintptr_t)d_scratch & 255u))
    return -EINVAL;
  Layout l;
  LearnArgs a;
  if (n) {
    if (!layout_of(n, max_candidates, &l) || !d_scratch ||
        scratch_bytes < carve(l, d_scratch, &a))
      return -EINVAL;
  }
  DeviceScope dg(ctx_device(c));
  if (!dg.ok) return -EIO;
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    if (!d_hdr) return 0;
    return hip_rc(hipMemsetAsync(d_hdr, 0, sizeof(*d_hdr), s));
  }
  a.status = d_status;
  a.recs = d_recs;
  a.n = n;
  a.phase = (uint32_t)((uintptr_t)d_status & 15u);
  a.maxc = l.maxc;
  a.nslots = l.nslots;
  a.new_recs = d_new_recs;
  a.first = d_first;
  a.packets = d_packets;
  a.cap = cap;
  a.hdr = d_hdr;
  const uint32_t nblk = (uint32_t)((n + a.phase + kFrames - 1) / kFrames);   // <= l.nblk
  const dim3 blk(kBlock);
  hipLaunchKernelGGL(learn_clear_kernel, dim3(capped_grid(l.nslots + 1, kBlock, kMaxGrid)), blk, 0,
                     s, a.slots, l.nslots + 1);
  hipLaunchKernelGGL(learn_count_kernel, dim3(nblk), blk, 0, s, a);
  hipLaunchKernelGGL(learn_scan_kernel, dim3(1), dim3(kScan), 0, s, a.blk, nblk,
                     (const uint64_t *)nullptr, 1u, (uint64_t)l.maxc, &d_hdr->candidates,
                     &d_hdr->considered);
  hipLaunchKernelGGL(learn_compact_kernel, dim3(nblk), blk, 0, s, a);
  // the grids of the passes over the candidates come from the argument; lanes
  // past the device-side `considered` leave at once
  hipLaunchKernelGGL(learn_insert_kernel, dim3(l.nlblk), blk, 0, s, a);
  hipLaunchKernelGGL(learn_resolve_kernel, dim3(l.nlblk), blk, 0, s, a);
  hipLaunchKernelGGL(learn_scan_kernel, dim3(1), dim3(kScan), 0, s, a.lcnt, l.nlblk,
                     (const uint64_t *)&d_hdr->considered, (uint32_t)kBlock, cap, &d_hdr->flows,
                     &d_hdr->written);
  hipLaunchKernelGGL(learn_emit_kernel, dim3(l.nlblk), blk, 0, s, a);
  return hip_rc(hipGetLastError());
}
