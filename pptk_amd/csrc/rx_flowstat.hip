// rx_flowstat.hip -- the device half of "Flow state" (include/pptk_rx.h):
// pptk_flow_account_device, which adds a batch's frames to the per-flow
// packet / byte counters and last-seen stamps, and
// pptk_flow_stats_reset_device.  host/flowtab.c holds the CPU statement
// (pptk_flow_account_host) and the expiry that reads the stamps.
//
// The input is 6 bytes per frame; the work is the read-modify-writes: two
// 64-bit adds and a 64-bit max per frame, all no-return agent-scope atomics
// that execute at the memory side.  Two shapes, one compile-time switch:
//   direct      (PPTK_FLOWSTAT_DIRECT) one lane per frame issues the three
//               atomics into stats[v] or *unmatched.
//   aggregated  (default) a workgroup owns a segment of kSeg consecutive
//               frames and sums it in LDS first: an open-addressed table of
//               kSlots {index, packets u32, bytes u32} slots, claimed with a
//               compare-and-swap on the index word and updated with LDS
//               adds, plus one unmatched pair.  kSeg * 65535 < 2^32, so a
//               slot's byte sum cannot wrap.  The probe visits kProbe slots
//               at most; a frame that finds none takes the direct path.  At
//               segment end every used slot is flushed with two adds and one
//               max: last_seen costs one atomic per distinct flow per
//               segment, unmatched three per workgroup.
//               Before LDS, equal indices are merged: the four consecutive
//               frames a lane loads in registers, and lanes whose four
//               frames are one flow across neighbouring lanes (a ballot
//               finds the runs, a wave prefix sum their bytes; waves without
//               such neighbours skip it).
// Every loop's trip count is a function of n and compile-time constants, or
// bounded by kProbe: table content never keeps a loop going.  The sums are
// integer and commutative, so both shapes, any grid and any stream order give
// the host statement's result bit for bit.
//   make abvariant NAME=flowstat_direct DEFS=-DPPTK_FLOWSTAT_DIRECT=1
#include <errno.h>

#include "copy16.h"
#include "rx_internal.h"

namespace pptk {
namespace {

constexpr int kBlock = 256;
constexpr uint32_t kSeg = 4096;      // frames per segment: 4 rounds of 256 lanes x 4 frames
constexpr uint32_t kSlots = 2048;    // LDS table slots (24 KB)
constexpr uint32_t kSlotBits = 11;
constexpr uint32_t kProbe = 8;
constexpr uint32_t kEmpty = 0xffffffffu;
constexpr uint32_t kMaxGrid = 1u << 16;   // beyond it the workgroups stride over the segments
static_assert(kSlots == 1u << kSlotBits, "kSlots is a power of two");
static_assert((uint64_t)kSeg * 65535u < (1ull << 32), "a segment's byte sum fits 32 bits");
static_assert(kSeg % (4 * kBlock) == 0, "whole rounds of 4 frames per lane");

#ifdef PPTK_FLOWSTAT_DIRECT
constexpr bool kDirect = PPTK_FLOWSTAT_DIRECT != 0;
#else
constexpr bool kDirect = false;
#endif

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

struct StatArgs {
  const uint32_t *idx;
  const uint16_t *len;      // nullable -> fixed_len
  pptk_flow_stats *stats;
  pptk_flow_stats *um;      // nullable
  uint64_t n;
  uint64_t stats_count;     // 1 .. 2^32
  uint64_t now;
  uint32_t fixed_len;
  uint32_t phase;           // (address of idx / 4) & 3: frame i is 16-byte aligned when (i + phase) % 4 == 0
};

// the three no-return atomics of one entry
__device__ __forceinline__ void entry_add(pptk_flow_stats *e, uint64_t packets, uint64_t bytes,
                                          uint64_t now) {
  (void)__hip_atomic_fetch_add(&e->packets, packets, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  (void)__hip_atomic_fetch_add(&e->bytes, bytes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  (void)__hip_atomic_fetch_max(&e->last_seen, now, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void direct_add(const StatArgs &a, uint32_t v, uint32_t packets,
                                           uint32_t bytes) {
  pptk_flow_stats *e = v < a.stats_count ? a.stats + v : a.um;
  if (e) entry_add(e, packets, bytes, a.now);
}

__global__ __launch_bounds__(kBlock) void flow_account_direct_kernel(StatArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += stride)
    direct_add(a, a.idx[i], 1u, a.len ? (uint32_t)a.len[i] : a.fixed_len);
}

// four lengths from p, which is 2-byte aligned: the widest loads its address allows
__device__ __forceinline__ void load_len4(const uint16_t *p, uint32_t L[4]) {
  const uint32_t m = (uint32_t)(uintptr_t)p & 7u;
  uint32_t lo, hi;
  if (m == 0) {
    const u32x2 w = *(const u32x2 *)p;
    lo = w.x;
    hi = w.y;
  } else if (m == 4) {
    lo = ((const uint32_t *)p)[0];
    hi = ((const uint32_t *)p)[1];
  } else {   // 2 or 6: a 4-byte aligned pair in the middle
    const uint32_t mid = *(const uint32_t *)(p + 1);
    lo = (uint32_t)p[0] | (mid << 16);
    hi = (mid >> 16) | ((uint32_t)p[3] << 16);
  }
  L[0] = lo & 0xffffu;
  L[1] = lo >> 16;
  L[2] = hi & 0xffffu;
  L[3] = hi >> 16;
}

struct SegTable {
  uint32_t key[kSlots];
  uint32_t packets[kSlots];
  uint32_t bytes[kSlots];
  uint32_t um_packets, um_bytes;
};

// `packets` frames of flow v with `bytes` bytes in all, into the segment's table
__device__ __forceinline__ void seg_add(const StatArgs &a, SegTable &t, uint32_t v,
                                        uint32_t packets, uint32_t bytes) {
  if (v >= a.stats_count) {
    if (a.um) {
      (void)__hip_atomic_fetch_add(&t.um_packets, packets, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);
      (void)__hip_atomic_fetch_add(&t.um_bytes, bytes, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    return;
  }
  if (v != kEmpty) {   // (a flow value only when stats_count is 2^32; it is the empty mark here)
    // multiplicative hash: indices that are multiples of a power of two
    // still spread over the slots
    const uint32_t h = (v * 0x9E3779B1u) >> (32 - kSlotBits);
#pragma unroll 1
    for (uint32_t p = 0; p < kProbe; ++p) {
      const uint32_t s = (h + p) & (kSlots - 1);
      uint32_t cur = __hip_atomic_load(&t.key[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (cur == kEmpty) {
        uint32_t expect = kEmpty;
        if (__hip_atomic_compare_exchange_strong(&t.key[s], &expect, v, __ATOMIC_RELAXED,
                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
          cur = v;
        else
          cur = expect;   // another lane claimed it, maybe for v
      }
      if (cur == v) {
        (void)__hip_atomic_fetch_add(&t.packets[s], packets, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_WORKGROUP);
        (void)__hip_atomic_fetch_add(&t.bytes[s], bytes, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_WORKGROUP);
        return;
      }
    }
  }
  entry_add(a.stats + v, packets, bytes, a.now);   // no slot within the bound
}

// Segments are cut in the aligned numbering j = i + phase, so that every group
// of four frames a lane takes is one aligned 16-byte load of d_idx; the first
// group of the batch and the last may be partial and are loaded frame by
// frame (the scalar head and tail).  A segment holds at most kSeg frames.
__global__ __launch_bounds__(kBlock) void flow_account_seg_kernel(StatArgs a) {
  __shared__ SegTable t;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t jend = a.n + a.phase;                       // frames are j in [phase, jend)
  const uint64_t nseg = (jend + kSeg - 1) / kSeg;
  for (uint64_t seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
    for (uint32_t k = threadIdx.x; k < kSlots; k += kBlock) {
      t.key[k] = kEmpty;
      t.packets[k] = 0;
      t.bytes[k] = 0;
    }
    if (threadIdx.x == 0) t.um_packets = t.um_bytes = 0;
    __syncthreads();
#pragma unroll 1
    for (uint32_t r = 0; r < kSeg / (4 * kBlock); ++r) {
      const uint64_t j0 = seg * kSeg + 4ull * (r * kBlock + threadIdx.x);
      uint32_t v[4] = {0, 0, 0, 0}, L[4] = {0, 0, 0, 0};
      uint32_t ok = 0;   // bit k: frame j0 + k exists
      if (j0 >= a.phase && j0 + 4 <= jend) {
        const uint64_t i0 = j0 - a.phase;
        const u32x4 w = *(const u32x4 *)(a.idx + i0);
        v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
        if (a.len)
          load_len4(a.len + i0, L);
        else
          L[0] = L[1] = L[2] = L[3] = a.fixed_len;
        ok = 0xfu;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint64_t j = j0 + k;
          if (j >= a.phase && j < jend) {
            v[k] = a.idx[j - a.phase];
            L[k] = a.len ? (uint32_t)a.len[j - a.phase] : a.fixed_len;
            ok |= 1u << k;
          }
        }
      }
      // a lane whose four frames are one flow joins its left neighbour's run
      // when that lane is such a lane of the same flow
      const bool uni = ok == 0xfu && v[0] == v[1] && v[1] == v[2] && v[2] == v[3];
      uint32_t cnt = 4, sum = L[0] + L[1] + L[2] + L[3];
      const uint32_t pv = __shfl_up(v[0], 1);
      const int puni = __shfl_up((int)uni, 1);
      const bool join = uni && puni && pv == v[0] && lane > 0;
      const uint64_t joined = __ballot(join);
      if (joined) {   // wave-uniform
        // the run of head lane l ends before the next lane that does not join
        uint32_t x = uni ? sum : 0u;   // inclusive prefix sum over the wave (< 2^24)
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const uint32_t y = __shfl_up(x, d);
          if ((int)lane >= d) x += y;
        }
        const uint64_t after = lane == 63 ? 0ull : (~joined) >> (lane + 1);
        const uint32_t lanes = after ? (uint32_t)__builtin_ctzll(after) + 1u : 64u - lane;
        const uint32_t xe = __shfl(x, (int)(lane + lanes - 1));
        if (uni && !join) {
          cnt = 4 * lanes;
          sum = xe - (x - sum);
        }
      }
      if (uni) {
        if (!join) seg_add(a, t, v[0], cnt, sum);
      } else {
        // the lane's own frames, equal neighbours merged in registers
        uint32_t rv = 0, rc = 0, rb = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!(ok & (1u << k))) continue;
          if (rc && v[k] == rv) {
            rc++;
            rb += L[k];
          } else {
            if (rc) seg_add(a, t, rv, rc, rb);
            rv = v[k];
            rc = 1;
            rb = L[k];
          }
        }
        if (rc) seg_add(a, t, rv, rc, rb);
      }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < kSlots; k += kBlock) {
      const uint32_t v = t.key[k];
      if (v != kEmpty) entry_add(a.stats + v, t.packets[k], t.bytes[k], a.now);
    }
    if (threadIdx.x == 0 && t.um_packets) entry_add(a.um, t.um_packets, t.um_bytes, a.now);
    __syncthreads();   // the table is reused by the workgroup's next segment
  }
}

struct ResetArgs {
  pptk_flow_stats *stats;
  const uint32_t *values;
  uint64_t stats_count, count, now;
};

// stats[v] = {0, 0, now}: one 16-byte and one 8-byte plain store, `reserved` left alone
__global__ __launch_bounds__(kBlock) void flow_stats_reset_kernel(ResetArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < a.count; k += stride) {
    const uint32_t v = a.values[k];
    if (v >= a.stats_count) continue;
    pptk_flow_stats *e = a.stats + v;
    *(u32x4 *)e = (u32x4){0, 0, 0, 0};
    e->last_seen = a.now;
  }
}

bool stats_ok(const void *stats, uint64_t stats_count) {
  return stats_count != 0 && stats_count <= (1ull << 32) && !((uintptr_t)stats & 31u);
}

}  // namespace
}  // namespace pptk

using namespace pptk;

extern "C" void pptk_flow_account_shape(uint32_t *segment_frames, uint32_t *lds_slots) {
  // a direct build has no segments: its unit is the 256 frames of a workgroup's round
  if (segment_frames) *segment_frames = kDirect ? (uint32_t)kBlock : kSeg;
  if (lds_slots) *lds_slots = kDirect ? 0u : kSlots;
}

extern "C" int pptk_flow_account_device(struct pptk_rx_ctx *c, const uint32_t *d_idx,
                                        const uint16_t *d_len, uint32_t fixed_len, uint64_t n,
                                        struct pptk_flow_stats *d_stats, uint64_t stats_count,
                                        struct pptk_flow_stats *d_unmatched, uint64_t now,
                                        void *stream) {
  static_assert(sizeof(pptk_flow_stats) == 32, "an entry is 32 bytes");
  if (!c || !stats_ok(d_stats, stats_count) || fixed_len > 65535u) return -EINVAL;
  if (((uintptr_t)d_idx & 3u) || ((uintptr_t)d_len & 1u) || ((uintptr_t)d_unmatched & 31u))
    return -EINVAL;
  if (n && (!d_idx || !d_stats)) return -EINVAL;
  DeviceScope dg(ctx_device(c));
  if (!dg.ok) return -EIO;
  if (n == 0) return 0;
  StatArgs a;
  a.idx = d_idx;
  a.len = d_len;
  a.stats = d_stats;
  a.um = d_unmatched;
  a.n = n;
  a.stats_count = stats_count;
  a.now = now;
  a.fixed_len = fixed_len;
  a.phase = (uint32_t)((uintptr_t)d_idx >> 2) & 3u;
  if (kDirect) {
    const dim3 grid(capped_grid(n, kBlock, kMaxGrid));
    hipLaunchKernelGGL(flow_account_direct_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, a);
  } else {
    // one workgroup per segment: many more workgroups than CUs, so the
    // dispatcher balances segments of uneven cost
    const dim3 grid(capped_grid(n + a.phase, kSeg, kMaxGrid));
    hipLaunchKernelGGL(flow_account_seg_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, a);
  }
  return hip_rc(hipGetLastError());
}

extern "C" int pptk_flow_stats_reset_device(struct pptk_rx_ctx *c, struct pptk_flow_stats *d_stats,
                                            uint64_t stats_count, const uint32_t *d_values,
                                            uint64_t count, uint64_t now, void *stream) {
  if (!c || !stats_ok(d_stats, stats_count) || ((uintptr_t)d_values & 3u)) return -EINVAL;
  if (count && (!d_values || !d_stats)) return -EINVAL;
  DeviceScope dg(ctx_device(c));
  if (!dg.ok) return -EIO;
  if (count == 0) return 0;
  const ResetArgs a = {d_stats, d_values, stats_count, count, now};
  const dim3 grid(capped_grid(count, kBlock, kMaxGrid));
  hipLaunchKernelGGL(flow_stats_reset_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, a);
  return hip_rc(hipGetLastError());
}
