// tx_gather.hip -- the device half of "Egress gather" (include/pptk_rx.h):
// pptk_tx_gather_device, which copies the frames a packed tx list names back
// to back into one region of `out` per egress port, every frame in a slot of
// whole 16-byte chunks.  host/gather.c holds the CPU statement
// (pptk_tx_gather_host); the device call equals it byte for byte.
//
// The place of entry e is start_p + C(e) - C(first_p): the slot bytes of all
// entries before e, less those before its run's first entry, from its
// region's start.  C is a prefix sum over the entries in list order, kept per
// block of kEntries entries.  Five launches on the caller's stream:
//   count    per block: the slot bytes, frame bytes and bad entries of its
//            entries; list by aligned 16-byte loads, len per lane
//   scan     one workgroup per column: the block sums (32-bit) become 64-bit
//            exclusive prefixes, kScan sums per round, and the column's total
//   bounds   one workgroup per run boundary: C at the run's first entry
//   ports    one wave: the runs checked, the region starts, where the packed
//            prefix ends (a search over the block prefixes, then inside one
//            block), the ports and the header
//   copy     per block: the offsets again from the block prefix, pk_off and
//            pk_len, then the frame bytes -- a team of lanes per entry, the
//            source at any byte phase, the destination chunk 16-byte aligned,
//            kUnroll rounds of loads in flight before the first funnel shift
//            (tx_tunnel.hip's encap), the slot's zero tail folded into the
//            last chunk's store
// The considered count is device data (d_entries): every pass clamps it by
// max_entries, which sizes the grids and the scratch.  The call uses no atomic
// operation, no workgroup waits for another's store -- the passes are ordered
// by kernel boundaries only -- and every loop's trip count is a constant, a
// kernel argument or a value clamped by one.  The result is the same for any
// grid.
#include "block_scan.h"
#include "copy16.h"
#include "gather_check.h"
#include "rx_internal.h"
#include "scratch_carve.h"

namespace pptk {
namespace {

constexpr int kBlock = 256;
constexpr uint32_t kPer = 4;                    // entries per lane: one 16-byte load of list
constexpr uint32_t kEntries = kPer * kBlock;    // entries per block
constexpr int kScan = 1024;                     // block sums per round of a scan workgroup
constexpr int kUnroll = 4;                      // team rounds whose loads are in flight together
constexpr uint32_t kSlot = PPTK_GATHER_SLOT_ALIGN, kRegion = PPTK_GATHER_REGION_ALIGN;
enum Col : uint32_t { kColSlot = 0, kColLen = 1, kColBad = 2, kCols = 3, kPrefixed = 2 };

// Lanes per entry.  The starting point is the tunnel's measured table
// (tx_tunnel.hip: 4 / 8 / 16 / 32 lanes with switch points 96 / 320 / 896
// bytes at one fixed length, 16 lanes with a length array); DESIGN.md "Egress
// gather" holds what was measured for this kernel.
constexpr uint32_t kLen4 = 96, kLen8 = 320, kLen16 = 896;   // longest fixed length per width
constexpr int kTeamAny = 16;

struct GatherArgs {
  FrameBatch fb;
  pptk_gather g;
  uint32_t nblk;
  uint32_t *cnt;    // [kCols][nblk]: the block sums
  uint64_t *pre;    // [kPrefixed][nblk + 1]: their exclusive prefixes, the total last
  uint64_t *tot;    // [kCols]
  uint64_t *bnd;    // [nports + 1]: C at each run's first considered entry, C(E) last
  uint64_t *ctl;    // [2]: considered and packed entries, as the ports pass decided (0 for bad runs)
};

__device__ __forceinline__ uint64_t round_up(uint64_t x, uint64_t a) { return (x + a - 1) & ~(a - 1); }

// E of the contract, whatever the runs look like: never above max_entries
__device__ __forceinline__ uint64_t considered(const pptk_gather &g) {
  uint64_t e = g.max_entries;
  if (g.d_entries) {
    const uint64_t d = *g.d_entries;
    if (d < e) e = d;
  }
  if (g.runs) {
    const uint64_t s = g.runs[g.nports - 1].start, end = s + g.runs[g.nports - 1].count;
    if (end >= s && end < e) e = end;
  }
  return e;
}

// the first considered entry of run p (p < nports)
__device__ __forceinline__ uint64_t run_first(const pptk_gather &g, uint32_t p, uint64_t E) {
  if (!g.runs) return 0;
  const uint64_t s = g.runs[p].start;
  return s < E ? s : E;
}

// A lane's kPer consecutive entries e0 .. e0 + kPer - 1, those below `lim`:
// the frame and its length (0 for a bad entry and at or above lim), and how
// many of them are bad.  list is read as one aligned 16-byte load where the
// four entries are whole and the array's phase allows it.
struct Four {
  uint32_t idx[kPer], len[kPer];
  uint32_t bad;
};

__device__ __forceinline__ Four load_four(const GatherArgs &a, uint64_t e0, uint64_t lim) {
  Four f;
  f.bad = 0;
  const uint32_t *lp = a.g.list ? a.g.list + e0 : nullptr;
  if (lp && e0 + kPer <= lim && ((uintptr_t)lp & 15u) == 0) {
    const u32x4 v = *(const u32x4 *)lp;
    f.idx[0] = v.x, f.idx[1] = v.y, f.idx[2] = v.z, f.idx[3] = v.w;
  } else {
#pragma unroll
    for (uint32_t j = 0; j < kPer; ++j)
      f.idx[j] = e0 + j < lim ? (lp ? lp[j] : (uint32_t)(e0 + j)) : 0u;
  }
#pragma unroll
  for (uint32_t j = 0; j < kPer; ++j) {
    const bool live = e0 + j < lim, ok = live && f.idx[j] < a.fb.n;
    f.len[j] = ok ? (a.fb.len_at(f.idx[j]) & 0xffffu) : 0u;
    f.bad += live && !ok;
  }
  return f;
}

__device__ __forceinline__ uint32_t slot_of(uint32_t len) { return (len + kSlot - 1) & ~(kSlot - 1); }

__global__ __launch_bounds__(kBlock) void gather_count_kernel(GatherArgs a) {
  __shared__ uint32_t lds[kBlock / 64];
  const uint64_t E = considered(a.g);
  const Four f = load_four(a, (uint64_t)blockIdx.x * kEntries + kPer * threadIdx.x, E);
  uint32_t slots = 0, lens = 0;
#pragma unroll
  for (uint32_t j = 0; j < kPer; ++j) slots += slot_of(f.len[j]), lens += f.len[j];
  uint32_t ts, tl, tb;   // a block's sums fit the word: kEntries * 65536 < 2^32
  block_excl_scan<kBlock / 64, uint32_t>(slots, lds, &ts);
  block_excl_scan<kBlock / 64, uint32_t>(lens, lds, &tl);
  block_excl_scan<kBlock / 64, uint32_t>(f.bad, lds, &tb);
  if (threadIdx.x == 0) {
    a.cnt[(size_t)kColSlot * a.nblk + blockIdx.x] = ts;
    a.cnt[(size_t)kColLen * a.nblk + blockIdx.x] = tl;
    a.cnt[(size_t)kColBad * a.nblk + blockIdx.x] = tb;
  }
}

// Workgroup c: column c's nblk block sums -> their total in tot[c] and, for
// the prefixed columns, their 64-bit exclusive prefixes in pre (the total as
// entry nblk): a batch's slot bytes pass 2^32.
__global__ __launch_bounds__(kScan) void gather_scan_kernel(GatherArgs a) {
  __shared__ uint64_t lds[kScan / 64];
  const uint32_t c = blockIdx.x;
  const uint32_t *col = a.cnt + (size_t)c * a.nblk;
  uint64_t *out = c < kPrefixed ? a.pre + (size_t)c * (a.nblk + 1) : nullptr;
  uint64_t running = 0;
  for (uint32_t base = 0; base < a.nblk; base += kScan) {
    const uint32_t k = base + threadIdx.x;
    const uint64_t v = k < a.nblk ? col[k] : 0u;
    uint64_t total;
    const uint64_t ex = block_excl_scan<kScan / 64, uint64_t>(v, lds, &total);
    if (out && k < a.nblk) out[k] = running + ex;
    running += total;
  }
  if (threadIdx.x == 0) {
    a.tot[c] = running;
    if (out) out[a.nblk] = running;
  }
}

// Workgroup p: bnd[p] = C(first entry of run p), bnd[nports] = C(E): the
// prefix of the block the entry lies in plus the block's entries before it.
__global__ __launch_bounds__(kBlock) void gather_bounds_kernel(GatherArgs a) {
  __shared__ uint32_t lds[kBlock / 64];
  const uint64_t E = considered(a.g);
  const uint32_t p = blockIdx.x;
  const uint64_t r = p < a.g.nports ? run_first(a.g, p, E) : E;
  const uint32_t b = (uint32_t)(r / kEntries);   // <= nblk: r <= E <= max_entries
  const Four f = load_four(a, (uint64_t)b * kEntries + kPer * threadIdx.x, r);
  uint32_t slots = 0, part;
#pragma unroll
  for (uint32_t j = 0; j < kPer; ++j) slots += slot_of(f.len[j]);
  block_excl_scan<kBlock / 64, uint32_t>(slots, lds, &part);
  if (threadIdx.x == 0) a.bnd[p] = a.pre[b] + part;
}

// one wave: lane p < nports writes ports[p], lane 0 the header and ctl
__global__ __launch_bounds__(64) void gather_ports_kernel(GatherArgs a) {
  __shared__ uint64_t sl[64];
  const pptk_gather &g = a.g;
  const uint32_t p = threadIdx.x, np = g.nports;
  bool badrun = false;
  if (g.runs && p < np) {   // pptk_gather_run_ok
    const uint64_t s = g.runs[p].start, c = g.runs[p].count;
    const uint64_t prev = p ? g.runs[p - 1].start + g.runs[p - 1].count : 0;
    badrun = s + c < s || s != prev;
  }
  if (__ballot(badrun)) {   // (the whole wave)
    if (p < np) g.ports[p] = pptk_gather_port{0, 0, 0, 0};
    if (p == 0) {
      *g.hdr = pptk_gather_hdr{0, 0, 0, 0, 0, 0, PPTK_GATHER_ST_BADRUNS, 0};
      a.ctl[0] = 0;
      a.ctl[1] = 0;
    }
    return;
  }
  const uint64_t E = considered(g);
  const uint64_t lo = p < np ? run_first(g, p, E) : E;
  const uint64_t hi = p + 1 < np ? run_first(g, p + 1, E) : E;
  const uint64_t S = p < np ? a.bnd[p + 1] - a.bnd[p] : 0;
  sl[p] = S;
  __syncthreads();
  uint64_t start = 0, mystart = 0, need = 0;
  for (uint32_t q = 0; q < np; ++q) {
    if (q == p) mystart = start;
    need = start + sl[q];
    start = round_up(need, kRegion);
  }
  // The first region that does not fit whole holds the cut; every region
  // before it is packed whole, none after it holds a packed entry.
  const uint64_t nofit = __ballot(p < np && mystart + S > g.out_cap);
  uint64_t P = E, CP = a.tot[kColSlot], CLP = a.tot[kColLen];   // packed entries, their slot and frame bytes
  uint32_t q = np;
  if (nofit) {
    q = (uint32_t)__ffsll((long long)nofit) - 1;
    const uint64_t rq = __shfl(lo, (int)q), startq = __shfl(mystart, (int)q), bq = a.bnd[q];
    const bool capok = g.out_cap >= startq;
    const uint64_t T = capok ? g.out_cap - startq + bq : 0;   // entry e of run q is packed iff C(e + 1) <= T
    uint32_t b = (uint32_t)(rq / kEntries);
    if (capok) {   // the blocks that end at or below T are packed whole
      uint32_t bl = 0, bh = a.nblk;
      for (int it = 0; it < 32; ++it) {
        if (bl < bh) {
          const uint32_t mid = bl + (bh - bl) / 2;
          if (a.pre[mid + 1] <= T) bl = mid + 1; else bh = mid;
        }
      }
      if (bl > b) b = bl;
    }
    if (b < a.nblk) {   // the cut lies in block b: walk it, 64 entries a round
      uint64_t run = a.pre[b], cnt = 0;
      CP = run;
      CLP = a.pre[(size_t)a.nblk + 1 + b];
#pragma unroll 1
      for (uint32_t r = 0; r < kEntries / 64; ++r) {
        const uint64_t e = (uint64_t)b * kEntries + 64u * r + p;
        const bool live = e < E;
        const uint32_t i = !live ? 0u : g.list ? g.list[e] : (uint32_t)e;
        const uint32_t len = live && i < a.fb.n ? (a.fb.len_at(i) & 0xffffu) : 0u;
        const uint32_t is = wave_incl_scan<uint32_t>(slot_of(len), p);
        const uint32_t il = wave_incl_scan<uint32_t>(len, p);
        const bool ok = live && (e < rq || (capok && run + is <= T));
        const uint32_t c = (uint32_t)__popcll(__ballot(ok));   // the ok lanes are the round's first c
        const uint32_t as = __shfl(is, c ? (int)c - 1 : 0), al = __shfl(il, c ? (int)c - 1 : 0);
        if (c) CP += as, CLP += al, cnt += c;
        run += __shfl(is, 63);
      }
      P = (uint64_t)b * kEntries + cnt;
    }
  }
  if (p < np) {
    const uint64_t cut = P < lo ? lo : P > hi ? hi : P;
    const uint64_t bytes = p < q ? S : p == q ? CP - a.bnd[q] : 0;
    g.ports[p] = pptk_gather_port{mystart, bytes, hi - lo, cut - lo};
  }
  if (p == 0) {
    *g.hdr = pptk_gather_hdr{E, P, need, CP, CLP, a.tot[kColBad], 0, 0};
    a.ctl[0] = E;
    a.ctl[1] = P;
  }
}

template <int T>
__global__ __launch_bounds__(kBlock) void gather_copy_kernel(GatherArgs a) {
  __shared__ uint64_t s_first[PPTK_PORT_MAX], s_base[PPTK_PORT_MAX];
  __shared__ uint64_t s_dst[kEntries], s_src[kEntries];
  __shared__ uint32_t s_len[kEntries];
  __shared__ uint32_t lds[kBlock / 64];
  const pptk_gather &g = a.g;
  const uint64_t E = a.ctl[0] < g.max_entries ? a.ctl[0] : g.max_entries;
  const uint64_t eb = (uint64_t)blockIdx.x * kEntries;
  if (eb >= E) return;   // (the whole workgroup)
  const uint32_t np = g.nports;
  if (threadIdx.x < np) {
    // run p's first entry; its region's start less the slot bytes before the run (modulo 2^64)
    s_first[threadIdx.x] = run_first(g, threadIdx.x, E);
    s_base[threadIdx.x] = g.ports[threadIdx.x].start - a.bnd[threadIdx.x];
  }
  const uint64_t e0 = eb + kPer * threadIdx.x;
  const Four f = load_four(a, e0, E);
  uint32_t slots = 0, total;
#pragma unroll
  for (uint32_t j = 0; j < kPer; ++j) slots += slot_of(f.len[j]);
  uint64_t C = a.pre[blockIdx.x] + block_excl_scan<kBlock / 64, uint32_t>(slots, lds, &total);
#pragma unroll
  for (uint32_t j = 0; j < kPer; ++j) {
    const uint64_t e = e0 + j;
    const uint32_t k = kPer * threadIdx.x + j;
    uint32_t copy = 0;
    if (e < E) {
      uint32_t p = 0;   // the last run that starts at or below e
#pragma unroll
      for (uint32_t step = PPTK_PORT_MAX / 2; step; step >>= 1)
        if (p + step < np && s_first[p + step] <= e) p += step;
      const uint64_t at = s_base[p] + C;
      if (g.pk_off) g.pk_off[e] = at;
      if (g.pk_len) g.pk_len[e] = (uint16_t)f.len[j];
      if (f.len[j] && at + slot_of(f.len[j]) <= g.out_cap) {   // packed: the contract's own test
        copy = f.len[j];
        s_dst[k] = at;
        s_src[k] = a.fb.addr(f.idx[j]);
      }
    }
    s_len[k] = copy;
    C += slot_of(f.len[j]);
  }
  __syncthreads();

  // the frames: team `team` takes the block's entries team, team + nteams, ...
  const uint32_t t = threadIdx.x & (T - 1), team = threadIdx.x / T;
  for (uint32_t k = team; k < kEntries; k += kBlock / T) {
    const uint32_t len = s_len[k];
    if (!len) continue;
    const uintptr_t F = (uintptr_t)s_src[k], lim = F + len;
    uint8_t *slot = g.out + s_dst[k];
    const uint32_t nchunks = (len + 15u) >> 4;
    for (uint32_t q0 = t; q0 < nchunks; q0 += T * kUnroll) {
      Raw16 raw[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const uint32_t q = q0 + T * u;
        if (q < nchunks) raw[u] = load16_raw(F + 16u * q, lim);
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const uint32_t q = q0 + T * u;
        if (q < nchunks) {
          const uint32_t o = 16u * q;
          u32x4 v = funnel16(raw[u], F + o);
          if (len - o < 16) {   // zeros up to the slot's end
#pragma unroll
            for (int d = 0; d < 4; ++d) v[d] &= low_bytes((int)(len - o) - 4 * d);
          }
          *(u32x4 *)(slot + o) = v;
        }
      }
    }
  }
}

// the derived counts of a call
struct Layout {
  uint32_t nblk, nports;
};

bool layout_of(uint64_t max_entries, uint32_t nports, Layout *l) {
  if (max_entries == 0 || max_entries >= (1ull << 32) || nports == 0 || nports > PPTK_PORT_MAX)
    return false;
  l->nblk = (uint32_t)((max_entries + kEntries - 1) / kEntries);
  l->nports = nports;
  return true;
}

// the scratch's arrays, in order: without a base the walk sizes the scratch,
// with the scratch pointer it binds the arguments
size_t carve(const Layout &l, void *base, GatherArgs *a) {
  Carve c(base, 256);
  a->cnt = c.take<uint32_t>((size_t)kCols * l.nblk);
  a->pre = c.take<uint64_t>((size_t)kPrefixed * (l.nblk + 1));
  a->tot = c.take<uint64_t>(kCols);
  a->bnd = c.take<uint64_t>(l.nports + 1);
  a->ctl = c.take<uint64_t>(2);
  return c.total();
}

template <int T>
void launch_copy(const GatherArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(gather_copy_kernel<T>, dim3(a.nblk), dim3(kBlock), 0, s, a);
}

}  // namespace
}  // namespace pptk

using namespace pptk;

extern "C" void pptk_tx_gather_shape(uint32_t *block_entries, uint32_t *scan_width) {
  if (block_entries) *block_entries = kEntries;
  if (scan_width) *scan_width = (uint32_t)kScan;
}

extern "C" size_t pptk_tx_gather_scratch_bytes(uint64_t max_entries, uint32_t nports) {
  Layout l;
  GatherArgs a;
  return layout_of(max_entries, nports, &l) ? carve(l, nullptr, &a) : 0;
}

extern "C" int pptk_tx_gather_device(struct pptk_rx_ctx *c, const struct pptk_gather *g,
                                     void *d_scratch, size_t scratch_bytes, void *stream) {
  static_assert(sizeof(pptk_gather_port) == 32, "a port entry is 32 bytes");
  static_assert(sizeof(pptk_gather_hdr) == 64, "the header is 64 bytes");
  static_assert(sizeof(pptk_gather) == 136, "the argument block is 136 bytes");
  static_assert(kEntries * 65536ull < (1ull << 32), "a block's slot bytes fit a word");
  if (!c) return -EINVAL;
  const int rc = pptk_gather_check(g);
  if (rc) return rc;
  Layout l;
  GatherArgs a;
  if (g->max_entries) {
    if (!layout_of(g->max_entries, g->nports, &l) || !d_scratch || ((uintptr_t)d_scratch & 255u) ||
        scratch_bytes < carve(l, d_scratch, &a))
      return -EINVAL;
  }
  DeviceScope dg(ctx_device(c));
  if (!dg.ok) return -EIO;
  hipStream_t s = (hipStream_t)stream;
  if (g->max_entries == 0) {
    hipError_t e = hipMemsetAsync(g->hdr, 0, sizeof(*g->hdr), s);
    if (e == hipSuccess) e = hipMemsetAsync(g->ports, 0, g->nports * sizeof(*g->ports), s);
    return hip_rc(e);
  }
  a.fb = {g->frames, g->off, g->len, g->stride, g->n, g->fixed_len};
  a.g = *g;
  a.nblk = l.nblk;
  const dim3 blk(kBlock);
  hipLaunchKernelGGL(gather_count_kernel, dim3(l.nblk), blk, 0, s, a);
  hipLaunchKernelGGL(gather_scan_kernel, dim3(kCols), dim3(kScan), 0, s, a);
  hipLaunchKernelGGL(gather_bounds_kernel, dim3(g->nports + 1), blk, 0, s, a);
  hipLaunchKernelGGL(gather_ports_kernel, dim3(1), dim3(64), 0, s, a);
  if (g->out_cap || g->pk_off || g->pk_len) {
    if (g->len)
      launch_copy<kTeamAny>(a, s);
    else if (g->fixed_len <= kLen4)
      launch_copy<4>(a, s);
    else if (g->fixed_len <= kLen8)
      launch_copy<8>(a, s);
    else if (g->fixed_len <= kLen16)
      launch_copy<16>(a, s);
    else
      launch_copy<32>(a, s);
  }
  return hip_rc(hipGetLastError());
}
