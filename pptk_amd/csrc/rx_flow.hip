// rx_flow.hip -- the device half of the flow table (include/pptk_rx.h "Flow
// table"): the hipMalloc mirror of the host image (host/flowtab.c),
// pptk_flow_table_sync, which uploads its dirty 4 KB pages, and
// pptk_flow_lookup_device, one launch that turns a batch of receive records
// into d_idx.
//   lookup  a team of T lanes per record.  A slot's first 44 bytes are laid
//           out as the record's (flowtab.h), so a probe compares 16-byte
//           chunks as they lie in memory.  T = 1: the lane loads the four
//           chunks of its record and of each slot it probes.  T = 4: lane j
//           of the team loads chunk j of both (the record read of a wave is
//           then one contiguous 1 KB, a probe one 64-byte segment per team)
//           and the verdicts are combined with a ballot.
//           The probe loop runs at most `limit` times -- a kernel argument
//           from the host's bookkeeping, never above the slot count -- and
//           stops at the first unused slot: table content alone never keeps
//           it going.  No atomics; every store is a plain vector store.
#include <errno.h>

#include "copy16.h"
#include "flowtab.h"
#include "rx_internal.h"

namespace pptk {
namespace {

constexpr int kBlock = 256;
constexpr uint32_t kMaxGrid = 1u << 16;   // beyond it the teams stride over the batch

// Lanes per record, by measurement (tools/flow_perf.py: 16 M records, hit rate
// 0.9).  Lookup ms with 1 / 4 lanes, tables of 2^16,
// 2^21 and 2^24 slots:
//     load 0.25   0.413 / 0.392   0.485 / 0.471   0.618 / 0.588
//     load 0.5    0.536 / 0.608   0.633 / 0.674   0.809 / 0.831
// Four lanes win by 3-5 % where probes are short, one lane by 3-12 % where
// they are long, and over all six cases.  PPTK_FLOW_TEAM builds the other
// shape (A/B):
//   make abvariant NAME=flow4 DEFS=-DPPTK_FLOW_TEAM=4
#ifdef PPTK_FLOW_TEAM
constexpr int kTeam = PPTK_FLOW_TEAM;
#else
constexpr int kTeam = 1;
#endif
static_assert(kTeam == 1 || kTeam == 4, "PPTK_FLOW_TEAM is 1 or 4");

struct FlowArgs {
  const pptk_flow_slot *img;
  const pptk_rx_rec *recs;
  const uint8_t *subject;   // nullable
  uint32_t *idx;
  uint8_t *status;          // nullable
  uint64_t n;
  uint32_t mask;            // slots - 1
  uint32_t limit;           // probes per record at most (<= slots)
};

constexpr uint32_t kSubjMask = (PPTK_RX_F_PARSED | PPTK_RX_F_MALFORMED) << 16;
constexpr uint32_t kSubjWant = PPTK_RX_F_PARSED << 16;

__device__ __forceinline__ bool eq4(u32x4 a, u32x4 b) {
  return ((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) == 0;
}

// One lane per record.  Record chunk 3 holds l3_off | proto << 8 | flags << 16
// in its second word; slot chunk 2 ends in proto | used << 8, chunk 3 starts
// with the value.
__global__ __launch_bounds__(kBlock) void flow_lookup_kernel_1(FlowArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += stride) {
    const u32x4 *r = (const u32x4 *)(a.recs + i);
    const u32x4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
    uint32_t val = PPTK_FLOW_NONE, st = 0;
    if ((r3.y & kSubjMask) == kSubjWant && (!a.subject || a.subject[i])) {
      st = PPTK_FLOW_ST_SUBJECT;
      const uint32_t want = ((r3.y >> 8) & 0xffu) | 0x100u;   // proto, used = 1, pad 0
      uint32_t s = r0.x & a.mask;
      for (uint32_t p = 0; p < a.limit; ++p, s = (s + 1) & a.mask) {
        const u32x4 *q = (const u32x4 *)(a.img + s);
        const u32x4 s0 = q[0], s1 = q[1], s2 = q[2], s3 = q[3];
        if (!((s2.w >> 8) & 0xffu)) break;   // unused: the probe ends
        if (eq4(s0, r0) && eq4(s1, r1) && s2.x == r2.x && s2.y == r2.y && s2.z == r2.z &&
            s2.w == want) {
          val = s3.x;
          st |= PPTK_FLOW_ST_HIT;
          break;
        }
      }
      if (!(st & PPTK_FLOW_ST_HIT)) val = PPTK_FLOW_NONE;
    }
    a.idx[i] = val;
    if (a.status) a.status[i] = (uint8_t)st;
  }
}

// Four lanes per record: lane j holds chunk j of the record and loads chunk j
// of every slot.  Every lane of a wave runs the same number of loop rounds
// (the rounds end when no team is still probing), so the ballots are taken
// with the whole wave converged.
__global__ __launch_bounds__(kBlock) void flow_lookup_kernel_4(FlowArgs a) {
  const uint32_t lane = threadIdx.x & 63u, j = lane & 3u;
  const uint32_t tshift = lane & ~3u;   // the team's first lane
  const uint64_t per_round = (uint64_t)gridDim.x * (kBlock / 4);
  // first record of this wave (wave-uniform) and this lane's own
  uint64_t w0 = ((uint64_t)blockIdx.x * kBlock + (threadIdx.x & ~63u)) / 4;
  for (; w0 < a.n; w0 += per_round) {
    const uint64_t i = w0 + (lane >> 2);
    const bool in = i < a.n;
    u32x4 rc = {0, 0, 0, 0};
    if (in) rc = ((const u32x4 *)(a.recs + i))[j];
    // the words the whole team needs: the hash's low half (chunk 0) and
    // proto | flags (chunk 3)
    const uint32_t h = __shfl(rc.x, 0, 4);
    const uint32_t pf = __shfl(rc.y, 3, 4);
    bool probing = in && (pf & kSubjMask) == kSubjWant && (!a.subject || a.subject[i]);
    uint32_t st = probing ? PPTK_FLOW_ST_SUBJECT : 0u;
    uint32_t val = PPTK_FLOW_NONE;
    const uint32_t want = ((pf >> 8) & 0xffu) | 0x100u;
    uint32_t s = h & a.mask;
    for (uint32_t p = 0; p < a.limit; ++p, s = (s + 1) & a.mask) {
      if (!__any(probing)) break;
      u32x4 sc = {0, 0, 0, 0};
      if (probing) sc = ((const u32x4 *)(a.img + s))[j];
      // chunk 2 carries `used` and compares its last word with proto | used;
      // chunk 3 (the value) takes no part in the match
      bool ok = j == 3 || (sc.x == rc.x && sc.y == rc.y && sc.z == rc.z &&
                           (j == 2 ? sc.w == want : sc.w == rc.w));
      const bool empty = j == 2 && !((sc.w >> 8) & 0xffu);
      const uint32_t okb = (uint32_t)(__ballot(ok && probing) >> tshift) & 0xfu;
      const uint32_t emb = (uint32_t)(__ballot(empty && probing) >> tshift) & 0xfu;
      if (probing) {
        if (emb) {
          probing = false;
        } else if (okb == 0xfu) {
          val = sc.x;   // meaningful in lane 3
          st |= PPTK_FLOW_ST_HIT;
          probing = false;
        }
      }
    }
    // lane 3 holds the value; the team's first lane writes
    const uint32_t v = __shfl(val, 3, 4);
    if (in && j == 0) {
      a.idx[i] = (st & PPTK_FLOW_ST_HIT) ? v : PPTK_FLOW_NONE;
      if (a.status) a.status[i] = (uint8_t)st;
    }
  }
}

}  // namespace
}  // namespace pptk

using namespace pptk;

extern "C" int pptk_flowtab_dev_attach(struct pptk_flow_table *t, struct pptk_rx_ctx *c) {
  static_assert(sizeof(pptk_flow_slot) == 64, "a slot is 64 bytes");
  DeviceScope dg(ctx_device(c));
  if (!dg.ok) return -EIO;
  void *p = nullptr;
  if (hipMalloc(&p, (size_t)t->slots * sizeof(pptk_flow_slot)) != hipSuccess) {
    (void)hipGetLastError();
    return -ENOMEM;
  }
  t->ctx = c;
  t->device = ctx_device(c);
  t->d_img = p;
  t->synced = 0;
  t->d_probe_limit = 0;
  return 0;
}

extern "C" void pptk_flowtab_dev_release(struct pptk_flow_table *t) {
  DeviceScope dg(t->device);
  if (dg.ok) (void)hipFree(t->d_img);   // (waits for work that still reads the image)
  t->d_img = nullptr;
  t->synced = 0;
}

extern "C" int pptk_flow_table_sync(struct pptk_flow_table *t, void *stream,
                                    uint64_t *uploaded_bytes) {
  if (uploaded_bytes) *uploaded_bytes = 0;
  if (!t || !t->d_img) return -EINVAL;
  DeviceScope dg(t->device);
  if (!dg.ok) return -EIO;
  hipStream_t s = (hipStream_t)stream;
  const size_t total = (size_t)t->slots * sizeof(pptk_flow_slot);
  const size_t page = (size_t)PPTK_FLOW_PAGE_SLOTS * sizeof(pptk_flow_slot);
  uint64_t bytes = 0;
  auto dirty = [&](uint32_t p) { return (t->dirty[p >> 6] >> (p & 63)) & 1u; };
  // runs of dirty pages go up as one copy each
  for (uint32_t p = 0; p < t->pages;) {
    if (!dirty(p)) {
      ++p;
      continue;
    }
    uint32_t e = p + 1;
    while (e < t->pages && dirty(e)) ++e;
    const size_t lo = p * page, hi = e * page < total ? e * page : total;
    if (hipMemcpyAsync((uint8_t *)t->d_img + lo, (const uint8_t *)t->img + lo, hi - lo,
                       hipMemcpyHostToDevice, s) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipStreamSynchronize(s);
      return -EIO;   // the pages stay dirty: the next sync repeats them
    }
    bytes += hi - lo;
    p = e;
  }
  if (hipStreamSynchronize(s) != hipSuccess) return -EIO;
  for (uint32_t w = 0; w < (t->pages + 63) / 64; ++w) t->dirty[w] = 0;
  t->d_probe_limit = t->probe_limit;
  t->synced = 1;
  if (uploaded_bytes) *uploaded_bytes = bytes;
  return 0;
}

extern "C" int pptk_flow_lookup_device(struct pptk_rx_ctx *c, const struct pptk_flow_table *t,
                                       const struct pptk_rx_rec *d_recs, uint64_t n,
                                       const uint8_t *d_subject, uint32_t *d_idx,
                                       uint8_t *d_status, void *stream) {
  if (!c || !t || !t->d_img || !t->synced || t->device != ctx_device(c)) return -EINVAL;
  if (((uintptr_t)d_recs & 15u) || ((uintptr_t)d_idx & 3u)) return -EINVAL;
  if (n && (!d_recs || !d_idx)) return -EINVAL;
  DeviceScope dg(ctx_device(c));
  if (!dg.ok) return -EIO;
  if (n == 0) return 0;
  FlowArgs a;
  a.img = (const pptk_flow_slot *)t->d_img;
  a.recs = d_recs;
  a.subject = d_subject;
  a.idx = d_idx;
  a.status = d_status;
  a.n = n;
  a.mask = t->slots - 1;
  a.limit = t->d_probe_limit < t->slots ? t->d_probe_limit : t->slots;
  const dim3 grid(capped_grid(n, kBlock / kTeam, kMaxGrid));
  if (kTeam == 4)
    hipLaunchKernelGGL(flow_lookup_kernel_4, grid, dim3(kBlock), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(flow_lookup_kernel_1, grid, dim3(kBlock), 0, (hipStream_t)stream, a);
  return hip_rc(hipGetLastError());
}
