// ip_reass.hip -- pptk_ip_reass_device: batch-local IPv4 reassembly, the
// receiving half of tx_frag.hip (include/pptk_rx.h "IPv4 reassembly";
// reference ipfrag/ipreass.c).  host/ipreass.c holds the CPU statement
// (pptk_ip_reass_host); the device call equals it byte for byte.
//
// Fifteen launches on the caller's stream:
//   clear     the set's slots = {owner empty, first 0xffffffff, count 0, cursor 0}
//   classify  one lane per frame: fragment / rejected / candidate from the
//             record, the side record and one frame byte (the IHL); writes
//             fstatus, dgram = 0xffffffff and the candidates per 256 frames
//   scan      one workgroup: exclusive prefixes; hdr.candidates / .considered
//   compact   cand[rank] = i, key[rank] = {src, dst, proto | ident << 8,
//             off | dl << 16}, meta[rank] = l2 | ihl << 8 | MF << 16 for rank <
//             max_candidates; the other candidates get SKIPPED
//   insert    lane r < considered enters its key into an open-addressed set:
//             a slot is claimed by a compare-and-swap of its owner word (empty
//             -> r) and belongs to the owner's key from then on; a lane that
//             meets an owned slot compares its 88 key bits with the owner's
//             and moves on when they differ.  Every lane of a key walks the
//             same probe sequence over slots that never change hands, so all
//             of them end in the same slot.  first = min(r), count += 1.
//   resolve   leaders (r == first) and the members of runs (count <= 64) per
//             256 candidates
//   scan      both; hdr.dgrams / .reported
//   assign    leaders write their datagram's report index and run base into
//             the slot, and lead[index] = r
//   append    every member of a datagram of <= 64 takes the next place of its
//             run with one atomic add (the order does not matter: the next
//             pass sorts)
//   decide    one wave per datagram, one member per lane: rank sort by (off,
//             candidate number) with shuffles, the run rewritten in that
//             order, neighbours compared, status and length decided
//   count     COMPLETE datagrams and those that take a slot, per 256
//   scan      both; hdr.complete / .written
//   finish    slots, WRITTEN / NOROOM, the report entries, out_len; then the
//             per-frame words of the members (a launch of its own)
//   emit      a team of 16 lanes per written datagram: the member table and
//             the patched header chunks parked in LDS, then one aligned
//             16-byte store per lane and chunk, each chunk funnelled from the
//             one to three members (and the header) that meet in it
// The passes are ordered by kernel boundaries only: no lane waits for another
// lane's store.  Every loop's trip count is a kernel argument or a device
// value clamped by one (probe loops: the slot count; member loops: 64).  The
// set is at most half full, so a probe always meets an empty slot.  first is
// a minimum and count a sum, the runs are sorted before use, and which slot a
// key lands in never reaches an output: the result is the same for any grid
// and any interleaving.
#include <errno.h>

#include "block_scan.h"
#include "copy16.h"
#include "rx_internal.h"
#include "scratch_carve.h"

namespace pptk {
namespace {

constexpr int kBlock = 256;
constexpr int kScan = 1024;
constexpr int kTeam = 16;
constexpr uint32_t kMaxFrags = 64;
constexpr uint64_t kMaxFrames = 1ull << 24;
constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kMaxGrid = 1u << 14;

struct Slot {
  uint32_t owner;    // a candidate that carries the slot's key; kNone = empty
  uint32_t first;    // the leader: the smallest candidate number of the key
  uint32_t count;    // members
  uint32_t cursor;   // places of the run handed out
  uint32_t dg;       // report index
  uint32_t base;     // start of the run in mem[]
  uint32_t pad[2];
};
static_assert(sizeof(Slot) == 32, "a slot is 32 bytes");

struct ReassArgs {
  FrameBatch fb;
  uint32_t maxc;         // min(max_candidates, n)
  const u32x4 *recs;     // 4 chunks per record
  const u32x4 *frag;
  uint8_t *out;
  uint64_t out_stride;
  uint64_t out_cap;
  uint16_t *out_len;
  uint32_t *report;      // 4 words per entry
  uint64_t report_cap;
  uint32_t *dgram;
  uint8_t *fstatus;
  pptk_reass_hdr *hdr;
  // scratch
  uint32_t *blk;         // candidates per block of frames, then their prefix
  uint32_t *cand;        // frame index
  u32x4 *key;            // src, dst, proto | ident << 8, off | dl << 16
  uint32_t *meta;        // l2 | ihl << 8 | MF << 16
  uint32_t *cslot;       // the candidate's slot
  uint32_t *mem;         // the runs: candidate numbers
  uint32_t *cnt_a;       // per block of candidates / datagrams, two counts
  uint32_t *cnt_b;
  uint32_t *lead;        // per datagram: the leader's candidate number
  uint32_t *dstat;       // per datagram: status
  uint32_t *dlen;        // per datagram: l2 + ihl + total where COMPLETE
  uint32_t *dslot;       // per datagram: output slot or kNone
  uint64_t *junk;        // totals nobody reads
  Slot *slots;
  uint32_t nslots;       // a power of two >= 2 * maxc
};

__global__ __launch_bounds__(kBlock) void reass_clear_kernel(Slot *slots, uint32_t count) {
  const uint32_t stride = gridDim.x * kBlock;
  for (uint32_t k = blockIdx.x * kBlock + threadIdx.x; k < count; k += stride) {
    u32x4 *p = (u32x4 *)(slots + k);
    p[0] = (u32x4){kNone, kNone, 0u, 0u};
    p[1] = (u32x4){0u, 0u, 0u, 0u};
  }
}

// What one frame's records say: its status bits and, for a fragment that
// passes, the words of the compact pass.  Reads record bytes 32..63, the side
// record and, where l3 < len, the frame byte at l3.
struct Parsed {
  uint32_t st, src, dst, pi, ol, meta;
};

__device__ __forceinline__ Parsed parse_one(const ReassArgs &a, uint64_t i, bool full) {
  Parsed p = {0, 0, 0, 0, 0, 0};
  const u32x4 c2 = a.recs[4 * i + 2], c3 = a.recs[4 * i + 3];
  const uint32_t fl = c3.y >> 16;
  if ((fl & (PPTK_RX_F_PARSED | PPTK_RX_F_FRAGMENT | PPTK_RX_F_MALFORMED | PPTK_RX_F_IPV6)) !=
      (PPTK_RX_F_PARSED | PPTK_RX_F_FRAGMENT))
    return p;
  const u32x4 fr = a.frag[i];
  const uint32_t l3 = c3.y & 0xffu, fo = fr.y & 0xffffu, dl = fr.y >> 16;
  const uint32_t mf = (fr.w >> 8) & PPTK_RX_FRAG_MF ? 1u : 0u;
  const uint32_t len = a.fb.len_at(i);
  uint32_t st = PPTK_REASS_FST_FRAG, ihl = 0;
  if (c2.w & 0xffffu) st |= PPTK_REASS_FST_BADCKSUM;
  if ((l3 != 14 && l3 != 18) || len <= l3) {
    st |= PPTK_REASS_FST_BADFRAG;
  } else {
    ihl = (ld_u8(a.fb.addr(i) + l3) & 15u) * 4u;
    if (ihl < 20 || dl == 0 || fo + dl > 65535 || (mf && (dl & 7u)) || l3 + ihl + dl > len)
      st |= PPTK_REASS_FST_BADFRAG;
  }
  p.st = st;
  if (full && st == PPTK_REASS_FST_FRAG) {
    const u32x4 c0 = a.recs[4 * i], c1 = a.recs[4 * i + 1];
    p.src = c0.z;   // record bytes 8..11
    p.dst = c1.z;   // record bytes 24..27
    p.pi = ((c3.y >> 8) & 0xffu) | (fr.x & 0xffffu) << 8;
    p.ol = fr.y;
    p.meta = l3 | ihl << 8 | mf << 16;
  }
  return p;
}

__global__ __launch_bounds__(kBlock) void reass_classify_kernel(ReassArgs a) {
  __shared__ uint32_t lds[kBlock / 64];
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  uint32_t st = 0;
  if (i < a.fb.n) {
    st = parse_one(a, i, false).st;
    a.fstatus[i] = (uint8_t)st;
    a.dgram[i] = kNone;
  }
  uint32_t total;
  (void)block_excl_scan<kBlock / 64, uint32_t>(st == PPTK_REASS_FST_FRAG, lds, &total);
  if (threadIdx.x == 0) a.blk[blockIdx.x] = total;
}

// cnt_a[0 .. nb) (and cnt_b where given) -> exclusive prefixes; the sums and
// min(sum of a, limit) go where the pointers say.  nb = nb_arg, or where
// `items` is given ceil(*items / per) if that is smaller.
__global__ __launch_bounds__(kScan) void reass_scan_kernel(uint32_t *cnt_a, uint32_t *cnt_b,
                                                          uint32_t nb_arg, const uint64_t *items,
                                                          uint32_t per, uint64_t limit,
                                                          uint64_t *total_a, uint64_t *min_a,
                                                          uint64_t *total_b) {
  __shared__ uint32_t lds[kScan / 64];
  const uint32_t nb = scan_extent(nb_arg, items, per);
  // every sum is at most 2^24
  const uint64_t run_a = scan_counts<kScan, uint32_t>(cnt_a, nb, true, lds);
  const uint64_t run_b = cnt_b ? scan_counts<kScan, uint32_t>(cnt_b, nb, true, lds) : 0;
  if (threadIdx.x == 0) {
    *total_a = run_a;
    *min_a = run_a < limit ? run_a : limit;
    *total_b = run_b;
  }
}

__global__ __launch_bounds__(kBlock) void reass_compact_kernel(ReassArgs a) {
  __shared__ uint32_t lds[kBlock / 64];
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool is = i < a.fb.n && a.fstatus[i] == PPTK_REASS_FST_FRAG;
  uint32_t total;
  // blk + the block's count <= candidates <= 2^24
  const uint32_t rank = a.blk[blockIdx.x] + block_excl_scan<kBlock / 64, uint32_t>(is, lds, &total);
  if (!is) return;
  if (rank >= a.maxc) {
    a.fstatus[i] = PPTK_REASS_FST_FRAG | PPTK_REASS_FST_SKIPPED;
    return;
  }
  const Parsed p = parse_one(a, i, true);
  a.cand[rank] = (uint32_t)i;
  a.key[rank] = (u32x4){p.src, p.dst, p.pi, p.ol};
  a.meta[rank] = p.meta;
}

__global__ __launch_bounds__(kBlock) void reass_insert_kernel(ReassArgs a) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= clamped_count(&a.hdr->considered, a.maxc)) return;
  const u32x4 me = a.key[r];
  const uint32_t mask = a.nslots - 1;
  uint32_t h = me.x * 0x9e3779b1u ^ me.y * 0x85ebca6bu ^ me.z * 0xc2b2ae35u;
  uint32_t s = (h ^ h >> 15) & mask;
  bool found = false;
#pragma unroll 1
  for (uint32_t p = 0; p < a.nslots; ++p, s = (s + 1) & mask) {
    uint32_t cur = __hip_atomic_load(&a.slots[s].owner, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kNone) {
      uint32_t expect = kNone;
      if (__hip_atomic_compare_exchange_strong(&a.slots[s].owner, &expect, r, __ATOMIC_RELAXED,
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        cur = r;
      else
        cur = expect;   // another lane claimed it, maybe for this key
    }
    if (cur == r) {
      found = true;
    } else if (cur < a.maxc) {   // (always: owners are candidate numbers)
      const u32x4 o = a.key[cur];   // written by the compact pass: never changes here
      found = o.x == me.x && o.y == me.y && o.z == me.z;
    }
    if (found) break;
  }
  if (!found) {   // not reached: at most nslots / 2 keys enter
    a.cslot[r] = kNone;
    return;
  }
  (void)__hip_atomic_fetch_min(&a.slots[s].first, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  (void)__hip_atomic_fetch_add(&a.slots[s].count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  a.cslot[r] = s;
}

// leader or not, and the places its datagram's run takes
__device__ __forceinline__ void leader_of(const ReassArgs &a, uint32_t r, uint32_t cons,
                                          uint32_t *is_lead, uint32_t *run) {
  *is_lead = 0, *run = 0;
  if (r >= cons) return;
  const uint32_t s = a.cslot[r];
  if (s >= a.nslots) return;
  const uint32_t first = a.slots[s].first, count = a.slots[s].count;
  if (first != r) return;
  *is_lead = 1;
  *run = count <= kMaxFrags ? count : 0u;
}

__global__ __launch_bounds__(kBlock) void reass_resolve_kernel(ReassArgs a) {
  __shared__ uint32_t lds[kBlock / 64];
  const uint32_t cons = clamped_count(&a.hdr->considered, a.maxc);
  if (blockIdx.x * kBlock >= cons) return;   // the whole workgroup
  uint32_t is_lead, run, ta, tb;
  leader_of(a, blockIdx.x * kBlock + threadIdx.x, cons, &is_lead, &run);
  (void)block_excl_scan<kBlock / 64>(is_lead, lds, &ta);
  (void)block_excl_scan<kBlock / 64>(run, lds, &tb);
  if (threadIdx.x == 0) a.cnt_a[blockIdx.x] = ta, a.cnt_b[blockIdx.x] = tb;
}

__global__ __launch_bounds__(kBlock) void reass_assign_kernel(ReassArgs a) {
  __shared__ uint32_t lds[kBlock / 64];
  const uint32_t cons = clamped_count(&a.hdr->considered, a.maxc);
  if (blockIdx.x * kBlock >= cons) return;   // the whole workgroup
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  uint32_t is_lead, run, ta, tb;
  leader_of(a, r, cons, &is_lead, &run);
  const uint32_t k = a.cnt_a[blockIdx.x] + block_excl_scan<kBlock / 64>(is_lead, lds, &ta);
  const uint32_t base = a.cnt_b[blockIdx.x] + block_excl_scan<kBlock / 64>(run, lds, &tb);
  if (!is_lead || k >= a.maxc) return;
  Slot *sl = a.slots + a.cslot[r];
  sl->dg = k;
  sl->base = base;
  a.lead[k] = r;
}

__global__ __launch_bounds__(kBlock) void reass_append_kernel(ReassArgs a) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= clamped_count(&a.hdr->considered, a.maxc)) return;
  const uint32_t s = a.cslot[r];
  if (s >= a.nslots) return;
  Slot *sl = a.slots + s;
  if (sl->count > kMaxFrags) return;
  const uint32_t at = sl->base + __hip_atomic_fetch_add(&sl->cursor, 1u, __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT);
  if (at < a.maxc) a.mem[at] = r;   // (always: the runs tile [0, members))
}

__global__ __launch_bounds__(kBlock) void reass_decide_kernel(ReassArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (blockIdx.x * kBlock + threadIdx.x) >> 6;
  const uint32_t nwaves = gridDim.x * (kBlock / 64);
  const uint32_t ndg = clamped_count(&a.hdr->dgrams, a.maxc);
  for (uint32_t k = wave; k < ndg; k += nwaves) {
    const uint32_t r0 = a.lead[k];
    const Slot sl = a.slots[a.cslot[r0]];
    const uint32_t cnt = sl.count;
    uint32_t st, flen = 0;
    if (cnt > kMaxFrags) {
      st = PPTK_REASS_DG_TOOMANY;
    } else {
      // one member per lane; idle lanes carry the largest key
      uint32_t m = 0x00ffffffu, ol = 0xffffu, mf = 1;
      if (lane < cnt) {
        m = a.mem[sl.base + lane];
        ol = a.key[m].w;
        mf = (a.meta[m] >> 16) & 1u;
      }
      const uint32_t skey = lane < cnt ? (ol & 0xffffu) : 0x10000u;   // (off, candidate number)
      uint32_t pos = 0;
#pragma unroll 1
      for (uint32_t j = 0; j < cnt; ++j) {   // cnt <= 64, the same in every lane
        const uint32_t kj = __shfl(skey, j), mj = __shfl(m, j);
        pos += kj < skey || (kj == skey && mj < m);
      }
      // lane p takes the member whose position is p
      uint32_t s_ol = 0, s_mm = 0;
#pragma unroll 1
      for (uint32_t j = 0; j < cnt; ++j) {
        const uint32_t pj = __shfl(pos, j), olj = __shfl(ol, j), mmj = __shfl(m | mf << 31, j);
        if (pj == lane) s_ol = olj, s_mm = mmj;
      }
      const uint32_t off = s_ol & 0xffffu, end = off + (s_ol >> 16), last = !(s_mm >> 31);
      const uint32_t next = __shfl_down(off, 1);
      const bool in = lane < cnt, inner = lane + 1 < cnt;
      if (in) a.mem[sl.base + lane] = s_mm & 0x00ffffffu;
      const bool overlap = __ballot(inner && (end > next || last)) != 0;
      const bool gap = __ballot(inner && end < next) != 0;
      const uint32_t lasts = __popcll(__ballot(in && last));
      const uint32_t off0 = __shfl(off, 0), total = __shfl(end, cnt ? cnt - 1 : 0);
      if (overlap || lasts > 1) {
        st = PPTK_REASS_DG_OVERLAP;
      } else if (lasts == 0 || off0 != 0 || gap) {
        st = PPTK_REASS_DG_INCOMPLETE;
      } else {
        st = PPTK_REASS_DG_COMPLETE;
        const uint32_t mt = a.meta[r0];
        flen = (mt & 0xffu) + ((mt >> 8) & 0xffu) + total;
        if (flen > 65535 || (((uint64_t)flen + 15u) & ~15ull) > a.out_stride)
          st |= PPTK_REASS_DG_TOOBIG;
        if (flen > 65535) flen = 0;
      }
    }
    if (lane == 0) a.dstat[k] = st, a.dlen[k] = flen;
  }
}

__device__ __forceinline__ void dg_kind(const ReassArgs &a, uint32_t k, uint32_t ndg,
                                        uint32_t *st, uint32_t *elig, uint32_t *comp) {
  *st = k < ndg ? a.dstat[k] : 0u;
  *comp = (*st & PPTK_REASS_DG_COMPLETE) != 0;
  *elig = *comp && !(*st & PPTK_REASS_DG_TOOBIG);
}

__global__ __launch_bounds__(kBlock) void reass_count_kernel(ReassArgs a) {
  __shared__ uint32_t lds[kBlock / 64];
  const uint32_t ndg = clamped_count(&a.hdr->dgrams, a.maxc);
  if (blockIdx.x * kBlock >= ndg) return;   // the whole workgroup
  uint32_t st, elig, comp, ta, tb;
  dg_kind(a, blockIdx.x * kBlock + threadIdx.x, ndg, &st, &elig, &comp);
  (void)block_excl_scan<kBlock / 64>(elig, lds, &ta);
  (void)block_excl_scan<kBlock / 64>(comp, lds, &tb);
  if (threadIdx.x == 0) a.cnt_a[blockIdx.x] = ta, a.cnt_b[blockIdx.x] = tb;
}

__global__ __launch_bounds__(kBlock) void reass_finish_kernel(ReassArgs a) {
  __shared__ uint32_t lds[kBlock / 64];
  const uint32_t ndg = clamped_count(&a.hdr->dgrams, a.maxc);
  if (blockIdx.x * kBlock >= ndg) return;   // the whole workgroup
  const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
  uint32_t st, elig, comp, ta;
  dg_kind(a, k, ndg, &st, &elig, &comp);
  const uint64_t slot = (uint64_t)a.cnt_a[blockIdx.x] + block_excl_scan<kBlock / 64>(elig, lds, &ta);
  if (k >= ndg) return;
  const bool written = elig && slot < a.out_cap;
  if (elig) st |= written ? PPTK_REASS_DG_WRITTEN : PPTK_REASS_DG_NOROOM;
  const uint32_t flen = a.dlen[k];
  a.dstat[k] = st;
  a.dslot[k] = written ? (uint32_t)slot : kNone;
  if (written) a.out_len[slot] = (uint16_t)flen;
  if (k < a.report_cap) {
    const uint32_t r0 = a.lead[k];
    uint32_t *e = a.report + 4ull * k;
    e[0] = a.cand[r0];
    e[1] = written ? (uint32_t)slot : kNone;
    e[2] = a.slots[a.cslot[r0]].count;
    e[3] = flen | st << 16;
  }
}

__global__ __launch_bounds__(kBlock) void reass_frames_kernel(ReassArgs a) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= clamped_count(&a.hdr->considered, a.maxc)) return;
  const uint32_t s = a.cslot[r];
  if (s >= a.nslots) return;
  const uint32_t k = a.slots[s].dg, i = a.cand[r];
  const bool done = k < a.maxc && (a.dstat[k] & PPTK_REASS_DG_WRITTEN);
  a.fstatus[i] = PPTK_REASS_FST_FRAG | PPTK_REASS_FST_MEMBER | (done ? PPTK_REASS_FST_DONE : 0u);
  a.dgram[i] = k;
}

// ---- emit ------------------------------------------------------------------
// (the re-aligning chunk loads and the field helpers: copy16.h)
struct TeamLds {
  u32x4 hd[5];                // the header chunks, patched (l2 + ihl <= 78)
  uint64_t src[kMaxFrags];    // address of the member's payload
  uint32_t ol[kMaxFrags];     // off | dl << 16, in datagram order
};

__device__ __forceinline__ void emit_dgram(const ReassArgs &a, uint32_t k, uint32_t t,
                                           TeamLds *L) {
  const uint32_t r0 = a.lead[k];
  const Slot sl = a.slots[a.cslot[r0]];
  const uint32_t cnt = sl.count < kMaxFrags ? sl.count : kMaxFrags;
  const uint32_t mt0 = a.meta[r0], l2 = mt0 & 0xffu, ihl = (mt0 >> 8) & 0xffu, H = l2 + ihl;
  const uint32_t flen = a.dlen[k], total = flen - H;
  const uintptr_t F = a.fb.addr(a.cand[r0]);
  uint8_t *slot = a.out + (uint64_t)a.dslot[k] * a.out_stride;

  // The team's lanes are in one wave, whose LDS accesses keep their order.
  __builtin_amdgcn_wave_barrier();
  for (uint32_t p = t; p < cnt; p += kTeam) {
    const uint32_t m = a.mem[sl.base + p], mt = a.meta[m];
    L->ol[p] = a.key[m].w;
    L->src[p] = a.fb.addr(a.cand[m]) + (mt & 0xffu) + ((mt >> 8) & 0xffu);
  }
  // the header: the leader's, offset and MF cleared (DF and the reserved bit
  // stay), the new total length, the checksum over the patched bytes
  {
    const uint32_t o = 16 * t;
    const uint32_t fkeep = (ld_u8(F + l2 + 6) & 0xc0u) << 8;
    u32x4 v = {0, 0, 0, 0};
    uint32_t sum = 0;
    if (o < H) {
      v = load16(F + o, F + H);
#pragma unroll
      for (int d = 0; d < 4; ++d) v[d] &= low_bytes((int)H - (int)o - 4 * d);
      put16(v, o, l2 + 2, ihl + total);
      put16(v, o, l2 + 6, fkeep);
      put16(v, o, l2 + 10, 0);
#pragma unroll
      for (int d = 0; d < 4; ++d) sum += halves(v[d] & ~low_bytes((int)l2 - (int)o - 4 * d));
    }
#pragma unroll
    for (int d = kTeam / 2; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, kTeam);
    // the stored little-endian half is the complement of the little-endian sum
    put16(v, o, l2 + 10, bswap16(~fold16(sum) & 0xffffu));
    if (o < H) L->hd[t] = v;
  }
  __builtin_amdgcn_wave_barrier();

  const uint32_t nchunks = (flen + 15) >> 4;
  uint32_t p = 0;
  for (uint32_t q = t; q < nchunks; q += kTeam) {
    const uint32_t o = 16 * q;
    u32x4 v = {0, 0, 0, 0};
    if (o + 16 > H) {
      // payload bytes [pa, pb) of the datagram fall into this chunk
      const uint32_t pa = o > H ? o - H : 0u, pb = o + 16 - H < total ? o + 16 - H : total;
      while (p < cnt) {   // at most cnt steps over the whole loop
        const uint32_t w = L->ol[p];
        if ((w & 0xffffu) + (w >> 16) > pa) break;
        ++p;
      }
      for (uint32_t pp = p; pp < cnt; ++pp) {   // at most three meet in a chunk
        const uint32_t w = L->ol[pp], mo = w & 0xffffu, ml = w >> 16;
        if (mo >= pb) break;
        const uintptr_t D = (uintptr_t)L->src[pp];
        // slot byte o is member byte o - H - mo: up to 15 bytes before the
        // payload, which is still inside the frame (its headers)
        const uintptr_t A = D + o - H - mo;
        const u32x4 x = load16(A, D + ml);
        const int lo = (int)(H + mo) - (int)o, hi = lo + (int)ml;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const uint32_t msk = low_bytes(hi - 4 * d) & ~low_bytes(lo - 4 * d);
          v[d] = (v[d] & ~msk) | (x[d] & msk);
        }
      }
    }
    if (o < H) {
      const u32x4 hd = L->hd[q];
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const uint32_t msk = low_bytes((int)H - (int)o - 4 * d);
        v[d] = (hd[d] & msk) | (v[d] & ~msk);
      }
    }
    if (flen - o < 16) {   // zeros up to the next 16-byte boundary
#pragma unroll
      for (int d = 0; d < 4; ++d) v[d] &= low_bytes((int)(flen - o) - 4 * d);
    }
    *(u32x4 *)(slot + o) = v;
  }
}

__global__ __launch_bounds__(kBlock) void reass_emit_kernel(ReassArgs a) {
  __shared__ TeamLds lds[kBlock / kTeam];
  TeamLds *L = &lds[threadIdx.x / kTeam];
  const uint32_t t = threadIdx.x & (kTeam - 1);
  const uint32_t team = (blockIdx.x * kBlock + threadIdx.x) / kTeam;
  const uint32_t nteams = gridDim.x * (kBlock / kTeam);
  const uint32_t ndg = clamped_count(&a.hdr->dgrams, a.maxc);
  for (uint32_t k = team; k < ndg; k += nteams)
    if (a.dstat[k] & PPTK_REASS_DG_WRITTEN) emit_dgram(a, k, t, L);
}

// the derived counts of a call
struct Layout {
  uint32_t maxc, nslots, nblk, ncblk;
};

bool layout_of(uint64_t n, uint64_t max_candidates, Layout *l) {
  if (n == 0 || n > kMaxFrames || max_candidates == 0 || max_candidates > kMaxFrames) return false;
  l->maxc = (uint32_t)(max_candidates < n ? max_candidates : n);
  l->nslots = 2;
  while (l->nslots < 2ull * l->maxc) l->nslots <<= 1;
  l->nblk = (uint32_t)((n + kBlock - 1) / kBlock);
  l->ncblk = (l->maxc + kBlock - 1) / kBlock;
  return true;
}

// the scratch's arrays, in order: without a base the walk sizes the scratch,
// with the scratch pointer it binds the arguments
size_t carve(const Layout &l, void *base, ReassArgs *a) {
  Carve c(base, 256);
  a->blk = c.take<uint32_t>(l.nblk);
  a->cand = c.take<uint32_t>(l.maxc);
  a->key = c.take<u32x4>(l.maxc);
  a->meta = c.take<uint32_t>(l.maxc);
  a->cslot = c.take<uint32_t>(l.maxc);
  a->mem = c.take<uint32_t>(l.maxc);
  a->cnt_a = c.take<uint32_t>(l.ncblk);
  a->cnt_b = c.take<uint32_t>(l.ncblk);
  a->lead = c.take<uint32_t>(l.maxc);
  a->dstat = c.take<uint32_t>(l.maxc);
  a->dlen = c.take<uint32_t>(l.maxc);
  a->dslot = c.take<uint32_t>(l.maxc);
  a->junk = c.take<uint64_t>(2);
  a->slots = c.take<Slot>(l.nslots);
  return c.total();
}

}  // namespace
}  // namespace pptk

using namespace pptk;

extern "C" void pptk_ip_reass_shape(uint32_t *max_frags, uint32_t *block_frames) {
  if (max_frags) *max_frags = kMaxFrags;
  if (block_frames) *block_frames = (uint32_t)kBlock;
}

extern "C" size_t pptk_ip_reass_scratch_bytes(uint64_t n, uint64_t max_candidates) {
  Layout l;
  ReassArgs a;
  return layout_of(n, max_candidates, &l) ? carve(l, nullptr, &a) : 0;
}

extern "C" int pptk_ip_reass_device(struct pptk_rx_ctx *c, const uint8_t *d_frames,
                                    const uint64_t *d_off, const uint16_t *d_len, uint64_t stride,
                                    uint32_t fixed_len, uint64_t n,
                                    const struct pptk_rx_rec *d_recs,
                                    const struct pptk_rx_frag *d_frag, uint64_t max_candidates,
                                    uint8_t *d_out, uint64_t out_stride, uint64_t out_cap,
                                    uint16_t *d_out_len, struct pptk_reass_dgram *d_report,
                                    uint64_t report_cap, uint32_t *d_dgram, uint8_t *d_fstatus,
                                    struct pptk_reass_hdr *d_hdr, void *d_scratch,
                                    size_t scratch_bytes, void *stream) {
  static_assert(sizeof(pptk_reass_hdr) == 48, "the header is 48 bytes");
  static_assert(sizeof(pptk_reass_dgram) == 16, "a report entry is 16 bytes");
  static_assert(sizeof(pptk_rx_rec) == 64 && sizeof(pptk_rx_frag) == 16, "record sizes");
  if (!c || !d_hdr || ((uintptr_t)d_hdr & 7u) || n > kMaxFrames || max_candidates == 0 ||
      max_candidates > kMaxFrames || (out_stride & 15u) || ((uintptr_t)d_out & 15u) ||
      out_cap > 0xffffffffull || report_cap > 0xffffffffull || ((uintptr_t)d_report & 3u) ||
      ((uintptr_t)d_dgram & 3u) || ((uintptr_t)d_recs & 15u) || ((uintptr_t)d_frag & 15u) ||
      ((uintptr_t)d_scratch & 255u))
    return -EINVAL;
  if ((out_cap && (!d_out || !d_out_len)) || (report_cap && !d_report)) return -EINVAL;
  Layout l;
  ReassArgs a;
  if (n) {
    if (!frame_batch_ok(d_frames, d_off, d_len, stride, fixed_len, n) || !d_recs || !d_frag ||
        !d_dgram || !d_fstatus)
      return -EINVAL;
    if (!layout_of(n, max_candidates, &l) || !d_scratch ||
        scratch_bytes < carve(l, d_scratch, &a))
      return -EINVAL;
  }
  DeviceScope dg(ctx_device(c));
  if (!dg.ok) return -EIO;
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return hip_rc(hipMemsetAsync(d_hdr, 0, sizeof(*d_hdr), s));

  a.fb = {d_frames, d_off, d_len, stride, n, fixed_len};
  a.maxc = l.maxc;
  a.recs = (const u32x4 *)d_recs;
  a.frag = (const u32x4 *)d_frag;
  a.out = d_out;
  a.out_stride = out_stride;
  a.out_cap = out_cap;
  a.out_len = d_out_len;
  a.report = (uint32_t *)d_report;
  a.report_cap = report_cap;
  a.dgram = d_dgram;
  a.fstatus = d_fstatus;
  a.hdr = d_hdr;
  a.nslots = l.nslots;
  const dim3 blk(kBlock), frames(l.nblk), cands(l.ncblk);
  const uint64_t *none = nullptr;
  hipLaunchKernelGGL(reass_clear_kernel, dim3(capped_grid(l.nslots, kBlock, kMaxGrid)), blk, 0, s,
                     a.slots, l.nslots);
  hipLaunchKernelGGL(reass_classify_kernel, frames, blk, 0, s, a);
  hipLaunchKernelGGL(reass_scan_kernel, dim3(1), dim3(kScan), 0, s, a.blk, (uint32_t *)nullptr,
                     l.nblk, none, 1u, (uint64_t)l.maxc, &d_hdr->candidates, &d_hdr->considered,
                     a.junk);
  hipLaunchKernelGGL(reass_compact_kernel, frames, blk, 0, s, a);
  // the grids of the passes over candidates and datagrams come from the
  // arguments; lanes past the device-side counts leave at once
  hipLaunchKernelGGL(reass_insert_kernel, cands, blk, 0, s, a);
  hipLaunchKernelGGL(reass_resolve_kernel, cands, blk, 0, s, a);
  hipLaunchKernelGGL(reass_scan_kernel, dim3(1), dim3(kScan), 0, s, a.cnt_a, a.cnt_b, l.ncblk,
                     (const uint64_t *)&d_hdr->considered, (uint32_t)kBlock, report_cap,
                     &d_hdr->dgrams, &d_hdr->reported, a.junk);
  hipLaunchKernelGGL(reass_assign_kernel, cands, blk, 0, s, a);
  hipLaunchKernelGGL(reass_append_kernel, cands, blk, 0, s, a);
  hipLaunchKernelGGL(reass_decide_kernel, dim3(capped_grid(l.maxc, kBlock / 64, kMaxGrid)), blk,
                     0, s, a);
  hipLaunchKernelGGL(reass_count_kernel, cands, blk, 0, s, a);
  hipLaunchKernelGGL(reass_scan_kernel, dim3(1), dim3(kScan), 0, s, a.cnt_a, a.cnt_b, l.ncblk,
                     (const uint64_t *)&d_hdr->dgrams, (uint32_t)kBlock, out_cap, a.junk + 1,
                     &d_hdr->written, &d_hdr->complete);
  hipLaunchKernelGGL(reass_finish_kernel, cands, blk, 0, s, a);
  hipLaunchKernelGGL(reass_frames_kernel, cands, blk, 0, s, a);
  hipLaunchKernelGGL(reass_emit_kernel, dim3(capped_grid(l.maxc, kBlock / kTeam, kMaxGrid)), blk,
                     0, s, a);
  return hip_rc(hipGetLastError());
}
