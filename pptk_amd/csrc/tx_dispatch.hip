// tx_dispatch.hip -- the device half of "Egress dispatch" (include/pptk_rx.h):
// pptk_tx_dispatch_device, which turns a per-frame port code (or a flow index
// and a code per flow) into one packed list of frame indices with a run per
// egress port, flood frames copied into every run but their ingress port's.
// host/dispatch.c holds the CPU statement (pptk_tx_dispatch_host); the device
// call equals it byte for byte.
//
// A stable multi-way partition with multicast.  The place of frame i in port
// p's run is U_p(i) + F(i) - Fin_p(i): the unicast frames to p before i, plus
// the flood frames before i, less those of them that came in through p.  So
// two per-port histograms and one scalar, kept per block of kFrames frames,
// give every place.  Four launches on the caller's stream:
//   count    per block: U[p], Fin[p], F, the class counts and, where lengths
//            are per frame, the byte sums; one row of the count table each
//   scan     one workgroup per column of the table turns the block counts
//            into exclusive prefixes, kScan counts per round, and writes the
//            column's total (64-bit)
//   ports    one wave: count, start, bytes, flooded of every port and the header
//   scatter  per block: the counts of its waves again, then every frame's
//            entries at start_p + place, predicated on g < cap and i < n
// A workgroup stages its frames' bytes in LDS with aligned 16-byte loads, each
// array in its own aligned numbering (bytewise where a 16-byte chunk crosses
// the array's first or last byte), and every wave then walks its 1024 frames
// in 16 rounds of 64 consecutive frames, one per lane.  Within a round frames
// are matched by ballots over the six bits of the port code and of the ingress
// port; lane p of a wave holds the running place of port p, so a lane ranks
// its frame with one cross-lane read and two popcounts.  The byte sums come
// from the same masks and a ballot per bit of the length.  The call uses no
// atomic operation at all, no workgroup waits for another's store -- the
// passes are ordered by kernel boundaries only -- and every loop's trip count
// is a constant or a kernel argument.  The result is the same for any grid.
// Only the byte arrays and idx are staged; off and len are read per lane (8
// and 2 bytes, consecutive frames in consecutive lanes) where a live frame
// needs them.
#include "block_scan.h"
#include "copy16.h"
#include "dispatch_check.h"
#include "rx_internal.h"
#include "scratch_carve.h"

namespace pptk {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr uint32_t kFrames = 16 * kBlock;       // frames per block: one 16-byte load per lane and byte array
constexpr uint32_t kWaveFrames = kFrames / kWaves;
constexpr int kRounds = kWaveFrames / 64;
constexpr int kScan = 1024;                     // counts per round of a scan workgroup
constexpr uint32_t kChunks = kFrames / 16 + 1;  // 16-byte chunks a block's bytes can touch
constexpr uint32_t kStage = kChunks * 16;
constexpr uint32_t kNoPort = 64;                // an ingress port at or above nports
constexpr uint32_t kBadCode = 0xfdu;            // never a port, FLOOD or DROP
enum Kind : uint32_t { kUni = 0, kFlood = 1, kDrop = 2, kBad = 3, kNone = 4 };

// the count table's columns, for nports = np
struct Cols {
  uint32_t np;
  __host__ __device__ uint32_t u(uint32_t p) const { return p; }
  __host__ __device__ uint32_t fin(uint32_t p) const { return np + p; }
  __host__ __device__ uint32_t f() const { return 2 * np; }
  __host__ __device__ uint32_t prefixed() const { return 2 * np + 1; }   // columns the scatter reads back
  __host__ __device__ uint32_t uni() const { return 2 * np + 1; }
  __host__ __device__ uint32_t drop() const { return 2 * np + 2; }
  __host__ __device__ uint32_t bad() const { return 2 * np + 3; }
  __host__ __device__ uint32_t hair() const { return 2 * np + 4; }
  __host__ __device__ uint32_t ub(uint32_t p) const { return 2 * np + 5 + p; }
  __host__ __device__ uint32_t finb(uint32_t p) const { return 3 * np + 5 + p; }
  __host__ __device__ uint32_t fb() const { return 4 * np + 5; }
  __host__ __device__ uint32_t count(bool bytes) const { return bytes ? 4 * np + 6 : 2 * np + 5; }
};

struct DispArgs {
  pptk_dispatch d;
  uint32_t nblk;
  uint32_t *cnt;    // [column][block]: counts, then (first `prefixed` columns) exclusive prefixes
  uint64_t *tot;    // the column totals
};

struct Stage {
  alignas(16) uint8_t code[kStage];
  alignas(16) uint8_t subj[kStage];
  alignas(16) uint8_t inp[kStage];
};

// x[i0 .. i0 + kFrames) within [0, n) into dst, in the array's own aligned
// 16-byte chunks: frame i0 + k is dst[shift + k], the shift returned
__device__ __forceinline__ uint32_t stage_bytes(const uint8_t *x, uint64_t i0, uint64_t n,
                                                uint8_t *dst) {
  const uintptr_t first = (uintptr_t)x + i0, lo = (uintptr_t)x, hi = (uintptr_t)x + n;
  const uint32_t shift = (uint32_t)(first & 15u);
  const uintptr_t base = first - shift;
  for (uint32_t c = threadIdx.x; c < kChunks; c += kBlock) {
    const uintptr_t a = base + 16u * c;
    u32x4 v = {0, 0, 0, 0};
    if (a >= lo && a + 16 <= hi) {
      if (c + 1 < kChunks || shift) v = *(const u32x4 *)a;   // the last chunk: only a shifted block reaches it
    } else if (a + 16 > lo && a < hi) {
      uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
      for (uint32_t k = 0; k < 16; ++k)
        if (a + k >= lo && a + k < hi) w[k >> 2] |= (uint32_t)(*(const uint8_t *)(a + k)) << (8 * (k & 3));
      v = (u32x4){w[0], w[1], w[2], w[3]};
    }
    *(u32x4 *)(dst + 16u * c) = v;
  }
  return shift;
}

__device__ __forceinline__ uint32_t code_of_idx(const pptk_dispatch &d, uint32_t v) {
  if (v == PPTK_FLOW_NONE) return d.miss_code;
  if (v >= d.flows) return kBadCode;
  return d.flow_port[v];
}

// the idx form: 16-byte chunks of four flow indices become four code bytes
__device__ __forceinline__ uint32_t stage_idx(const pptk_dispatch &d, uint64_t i0, uint8_t *dst) {
  const uintptr_t first = (uintptr_t)(d.idx + i0), lo = (uintptr_t)d.idx,
                  hi = (uintptr_t)(d.idx + d.n);
  const uint32_t shift = (uint32_t)(first & 15u) >> 2;
  const uintptr_t base = first - 4u * shift;
  constexpr uint32_t kIdxChunks = kFrames / 4 + 1;
  static_assert(kIdxChunks * 4 <= kStage, "the code bytes of a block fit the stage");
  for (uint32_t c = threadIdx.x; c < kIdxChunks; c += kBlock) {
    const uintptr_t a = base + 16u * c;
    uint32_t codes = 0;
    if (a >= lo && a + 16 <= hi) {
      if (c + 1 < kIdxChunks || shift) {
        const u32x4 v = *(const u32x4 *)a;
        codes = code_of_idx(d, v.x) | code_of_idx(d, v.y) << 8 | code_of_idx(d, v.z) << 16 |
                code_of_idx(d, v.w) << 24;
      }
    } else if (a + 16 > lo && a < hi) {
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k)
        if (a + 4 * k >= lo && a + 4 * k < hi)
          codes |= code_of_idx(d, *(const uint32_t *)(a + 4 * k)) << (8 * k);
    }
    *(uint32_t *)(dst + 4u * c) = codes;
  }
  return shift;
}

// where the staged bytes of frame i0 + k lie
struct Shifts {
  uint32_t code, subj, inp;
};

__device__ __forceinline__ Shifts stage_block(const pptk_dispatch &d, uint64_t i0, Stage &st) {
  Shifts s = {0, 0, 0};
  s.code = d.port ? stage_bytes(d.port, i0, d.n, st.code) : stage_idx(d, i0, st.code);
  if (d.subject) s.subj = stage_bytes(d.subject, i0, d.n, st.subj);
  if (d.in_port) s.inp = stage_bytes(d.in_port, i0, d.n, st.inp);
  __syncthreads();
  return s;
}

// one lane's frame of a round
struct Frame {
  uint32_t kind;   // Kind
  uint32_t port;   // kUni: the egress port; otherwise 0
  uint32_t in;     // the ingress port, kNoPort when none
};

__device__ __forceinline__ Frame classify(const pptk_dispatch &d, const Stage &st, const Shifts &s,
                                          uint64_t i0, uint32_t k) {
  Frame f = {kNone, 0, kNoPort};
  if (i0 + k >= d.n) return f;
  const uint32_t in = d.in_port ? st.inp[s.inp + k] : d.in_port_all;
  f.in = in < d.nports ? in : kNoPort;
  const uint32_t code = st.code[s.code + k];
  if (d.subject && st.subj[s.subj + k] == 0) {
    f.kind = kDrop;
  } else if (code < d.nports) {
    f.kind = kUni;
    f.port = code;
  } else {
    f.kind = code == PPTK_PORT_FLOOD ? kFlood : code == PPTK_PORT_DROP ? kDrop : kBad;
  }
  return f;
}

// the lanes of a round by what they hold: ballots over the kinds and over the
// six bits of the egress port and of the ingress port
struct Round {
  uint64_t uni, flood, drop, bad;
  uint64_t pb[6];   // bit k of the unicast lanes' port
  uint64_t ib[6];   // bit k of the flood lanes' ingress port
  uint64_t fin;     // flood lanes that have an ingress port

  __device__ __forceinline__ explicit Round(const Frame &f) {
    uni = __ballot(f.kind == kUni);
    flood = __ballot(f.kind == kFlood);
    drop = __ballot(f.kind == kDrop);
    bad = __ballot(f.kind == kBad);
    fin = __ballot(f.kind == kFlood && f.in != kNoPort);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      pb[k] = __ballot((f.port >> k) & 1u);
      ib[k] = __ballot((f.in >> k) & 1u);
    }
  }
  // unicast lanes whose port is v / flood lanes whose ingress port is v (v < 64)
  __device__ __forceinline__ uint64_t to(uint32_t v) const {
    uint64_t m = uni;
#pragma unroll
    for (int k = 0; k < 6; ++k) m &= (v >> k) & 1u ? pb[k] : ~pb[k];
    return m;
  }
  __device__ __forceinline__ uint64_t from(uint32_t v) const {
    uint64_t m = fin;
#pragma unroll
    for (int k = 0; k < 6; ++k) m &= (v >> k) & 1u ? ib[k] : ~ib[k];
    return m;
  }
};

// what a wave's kWaveFrames frames add: u and fin of port `lane` in each lane,
// the rest the same in every lane
struct WaveCount {
  uint32_t u, fin, f, uni, drop, bad, hair;
  uint32_t ub, finb, fb;   // with per-frame lengths: the byte sums beside u, fin, f
};

// frames i0 + wave * kWaveFrames ..; with BYTES the frame lengths are summed
// beside the counts, bit by bit: a ballot per bit of the length, and the lanes
// of a match mask that have the bit set count 2^bit each
template <bool BYTES>
__device__ __forceinline__ WaveCount count_wave(const pptk_dispatch &d, const Stage &st,
                                                const Shifts &s, uint64_t i0) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  WaveCount c = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 1
  for (int r = 0; r < kRounds; ++r) {
    const uint32_t k = wave * kWaveFrames + 64u * r + lane;
    const Frame f = classify(d, st, s, i0, k);
    const Round rd(f);
    c.u += __popcll(rd.to(lane));
    c.fin += __popcll(rd.from(lane));
    c.f += __popcll(rd.flood);
    c.uni += __popcll(rd.uni);
    c.drop += __popcll(rd.drop);
    c.bad += __popcll(rd.bad);
    c.hair += __popcll(__ballot(f.kind == kUni && f.in == f.port));
    if (BYTES) {
      const uint32_t len = f.kind == kUni || f.kind == kFlood ? d.len[i0 + k] : 0u;
      const uint64_t to = rd.to(lane), from = rd.from(lane);
#pragma unroll
      for (int b = 0; b < 16; ++b) {
        const uint64_t set = __ballot((len >> b) & 1u);
        c.ub += (uint32_t)__popcll(to & set) << b;
        c.finb += (uint32_t)__popcll(from & set) << b;
        c.fb += (uint32_t)__popcll(rd.flood & set) << b;
      }
    }
  }
  return c;
}

struct WaveTable {
  uint32_t u[kWaves][64], fin[kWaves][64];
  uint32_t f[kWaves], uni[kWaves], drop[kWaves], bad[kWaves], hair[kWaves];
};

struct ByteTable {
  uint32_t ub[kWaves][64], finb[kWaves][64], fb[kWaves];
};

__device__ __forceinline__ void put_wave(WaveTable &t, const WaveCount &c) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  t.u[wave][lane] = c.u;
  t.fin[wave][lane] = c.fin;
  if (lane == 0) {
    t.f[wave] = c.f;
    t.uni[wave] = c.uni;
    t.drop[wave] = c.drop;
    t.bad[wave] = c.bad;
    t.hair[wave] = c.hair;
  }
}

template <bool BYTES>
__global__ __launch_bounds__(kBlock) void dispatch_count_kernel(DispArgs a) {
  __shared__ Stage st;
  __shared__ WaveTable t;
  __shared__ ByteTable bt;
  const pptk_dispatch &d = a.d;
  const uint64_t i0 = (uint64_t)blockIdx.x * kFrames;
  const Shifts s = stage_block(d, i0, st);
  const WaveCount wc = count_wave<BYTES>(d, st, s, i0);
  put_wave(t, wc);
  if (BYTES) {
    bt.ub[threadIdx.x >> 6][threadIdx.x & 63u] = wc.ub;
    bt.finb[threadIdx.x >> 6][threadIdx.x & 63u] = wc.finb;
    if ((threadIdx.x & 63u) == 0) bt.fb[threadIdx.x >> 6] = wc.fb;
  }
  __syncthreads();
  const Cols col = {d.nports};
  uint32_t *row = a.cnt + blockIdx.x;        // column c of this block: row[c * nblk]
  const uint32_t p = threadIdx.x;
  if (p < d.nports) {
    uint32_t u = 0, fin = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) u += t.u[w][p], fin += t.fin[w][p];
    row[(size_t)col.u(p) * a.nblk] = u;
    row[(size_t)col.fin(p) * a.nblk] = fin;
    if (BYTES) {
      uint32_t ub = 0, finb = 0;   // a block's byte sum fits the word: kFrames * 65535 < 2^32
#pragma unroll
      for (int w = 0; w < kWaves; ++w) ub += bt.ub[w][p], finb += bt.finb[w][p];
      row[(size_t)col.ub(p) * a.nblk] = ub;
      row[(size_t)col.finb(p) * a.nblk] = finb;
    }
  }
  if (p == 64) {
    uint32_t f = 0, uni = 0, drop = 0, bad = 0, hair = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w)
      f += t.f[w], uni += t.uni[w], drop += t.drop[w], bad += t.bad[w], hair += t.hair[w];
    row[(size_t)col.f() * a.nblk] = f;
    row[(size_t)col.uni() * a.nblk] = uni;
    row[(size_t)col.drop() * a.nblk] = drop;
    row[(size_t)col.bad() * a.nblk] = bad;
    row[(size_t)col.hair() * a.nblk] = hair;
    if (BYTES) {
      uint32_t fb = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) fb += bt.fb[w];
      row[(size_t)col.fb() * a.nblk] = fb;
    }
  }
}

// Workgroup c: column c's nblk counts -> their total in tot[c] and, for the
// first `prefixed` columns, their exclusive prefixes in place.  A prefixed
// column sums frames of one kind, at most n < 2^32, so its prefixes fit the
// word; the byte sums need 64 bits and are not prefixed.
__global__ __launch_bounds__(kScan) void dispatch_scan_kernel(uint32_t *cnt, uint32_t nblk,
                                                             uint32_t prefixed, uint64_t *tot) {
  __shared__ uint64_t lds[kScan / 64];
  uint32_t *colp = cnt + (size_t)blockIdx.x * nblk;
  const uint64_t total = scan_counts<kScan, uint64_t>(colp, nblk, blockIdx.x < prefixed, lds);
  if (threadIdx.x == 0) tot[blockIdx.x] = total;
}

// one wave: lane p < nports writes ports[p], lane 0 the header
__global__ __launch_bounds__(64) void dispatch_ports_kernel(DispArgs a, bool bytes) {
  __shared__ uint64_t cnt[64];
  const pptk_dispatch &d = a.d;
  const Cols col = {d.nports};
  const uint32_t p = threadIdx.x;
  const uint64_t f = a.tot[col.f()];
  uint64_t count = 0, flooded = 0, nbytes = 0;
  if (p < d.nports) {
    flooded = f - a.tot[col.fin(p)];
    count = a.tot[col.u(p)] + flooded;
    nbytes = bytes ? a.tot[col.ub(p)] + a.tot[col.fb()] - a.tot[col.finb(p)]
                   : count * (uint64_t)d.fixed_len;
  }
  cnt[p] = count;
  __syncthreads();
  uint64_t start = 0, total = 0;
  for (uint32_t q = 0; q < d.nports; ++q) {
    if (q < p) start += cnt[q];
    total += cnt[q];
  }
  if (p < d.nports) {
    pptk_dispatch_port e = {start, count, nbytes, flooded};
    d.ports[p] = e;
  }
  if (p == 0) {
    pptk_dispatch_hdr h = {total, total < d.cap ? total : d.cap, a.tot[col.uni()], f,
                           a.tot[col.drop()], a.tot[col.bad()], a.tot[col.hair()], 0};
    *d.hdr = h;
  }
}

__device__ __forceinline__ uint64_t below(uint32_t lane) { return (1ull << lane) - 1; }

__device__ __forceinline__ void put_entry(const pptk_dispatch &d, uint64_t g, uint64_t i,
                                          uint64_t off, uint16_t len) {
  if (g >= d.cap || i >= d.n) return;
  d.list[g] = (uint32_t)i;
  if (d.out_off) d.out_off[g] = off;
  if (d.out_len) d.out_len[g] = len;
}

__global__ __launch_bounds__(kBlock) void dispatch_scatter_kernel(DispArgs a) {
  __shared__ Stage st;
  __shared__ WaveTable t;
  const pptk_dispatch &d = a.d;
  const Cols col = {d.nports};
  const uint32_t *row = a.cnt + blockIdx.x;
  const uint32_t fpre = row[(size_t)col.f() * a.nblk];
  // port 0's run comes first and every later port starts behind it, so no
  // entry of this block lies below port 0's place at the block's first frame
  if ((uint64_t)row[(size_t)col.u(0) * a.nblk] + fpre - row[(size_t)col.fin(0) * a.nblk] >= d.cap)
    return;   // (the whole workgroup)
  const uint64_t i0 = (uint64_t)blockIdx.x * kFrames;
  const Shifts s = stage_block(d, i0, st);
  put_wave(t, count_wave<false>(d, st, s, i0));
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  // lane p: start_p + U_p - Fin_p at the wave's first frame (modulo 2^64; with
  // the flood count added it is a place); the flood count, the same in every lane
  uint64_t place = 0, floods = fpre;
  if (lane < d.nports)
    place = d.ports[lane].start + row[(size_t)col.u(lane) * a.nblk] -
            row[(size_t)col.fin(lane) * a.nblk];
#pragma unroll
  for (uint32_t w = 0; w + 1 < kWaves; ++w) {
    if (w < wave) {
      place += t.u[w][lane];
      place -= t.fin[w][lane];
      floods += t.f[w];
    }
  }
#pragma unroll 1
  for (int r = 0; r < kRounds; ++r) {
    const uint32_t k = wave * kWaveFrames + 64u * r + lane;
    const uint64_t i = i0 + k;
    const Frame f = classify(d, st, s, i0, k);
    const Round rd(f);
    const bool live = f.kind == kUni || f.kind == kFlood;
    const uint64_t off = !live ? 0 : d.off ? d.off[i] : i * d.stride;
    const uint16_t len = !live ? 0 : d.len ? d.len[i] : (uint16_t)d.fixed_len;
    const uint64_t fl = floods + __popcll(rd.flood & below(lane));   // F(i)
    const uint64_t mine = __shfl(place, (int)f.port);
    if (f.kind == kUni)
      put_entry(d, mine + __popcll(rd.to(f.port) & below(lane)) + fl -
                       __popcll(rd.from(f.port) & below(lane)), i, off, len);
    if (rd.flood) {
      for (uint32_t q = 0; q < d.nports; ++q) {   // the same q in every lane
        const uint64_t at = __shfl(place, (int)q) + __popcll(rd.to(q) & below(lane)) + fl -
                            __popcll(rd.from(q) & below(lane));
        if (f.kind == kFlood && f.in != q) put_entry(d, at, i, off, len);
      }
    }
    place += __popcll(rd.to(lane));
    place -= __popcll(rd.from(lane));
    floods += __popcll(rd.flood);
  }
}

// the derived counts of a call
struct Layout {
  uint32_t nblk, cols;
};

bool layout_of(uint64_t n, uint32_t nports, Layout *l) {
  if (n == 0 || n >= (1ull << 32) || nports == 0 || nports > PPTK_PORT_MAX) return false;
  const Cols col = {nports};
  l->nblk = (uint32_t)((n + kFrames - 1) / kFrames);
  l->cols = col.count(true);   // whether or not the call has per-frame lengths
  return true;
}

// the scratch's arrays, in order: without a base the walk sizes the scratch,
// with the scratch pointer it binds the arguments
size_t carve(const Layout &l, void *base, DispArgs *a) {
  Carve c(base, 256);
  a->cnt = c.take<uint32_t>((size_t)l.cols * l.nblk);
  a->tot = c.take<uint64_t>(l.cols);
  return c.total();
}

}  // namespace
}  // namespace pptk

using namespace pptk;

extern "C" void pptk_tx_dispatch_shape(uint32_t *block_frames, uint32_t *scan_width) {
  if (block_frames) *block_frames = kFrames;
  if (scan_width) *scan_width = (uint32_t)kScan;
}

extern "C" size_t pptk_tx_dispatch_scratch_bytes(uint64_t n, uint32_t nports) {
  Layout l;
  DispArgs a;
  return layout_of(n, nports, &l) ? carve(l, nullptr, &a) : 0;
}

extern "C" int pptk_tx_dispatch_device(struct pptk_rx_ctx *c, const struct pptk_dispatch *d,
                                       void *d_scratch, size_t scratch_bytes, void *stream) {
  static_assert(sizeof(pptk_dispatch_port) == 32, "a port entry is 32 bytes");
  static_assert(sizeof(pptk_dispatch_hdr) == 64, "the header is 64 bytes");
  static_assert(sizeof(pptk_dispatch) == 152, "the argument block is 152 bytes");
  static_assert(kFrames * 65535ull < (1ull << 32), "a block's byte sum fits a word");
  if (!c) return -EINVAL;
  const int rc = pptk_dispatch_check(d);
  if (rc) return rc;
  Layout l;
  DispArgs a;
  if (d->n) {
    if (!layout_of(d->n, d->nports, &l) || !d_scratch || ((uintptr_t)d_scratch & 255u) ||
        scratch_bytes < carve(l, d_scratch, &a))
      return -EINVAL;
  }
  DeviceScope dg(ctx_device(c));
  if (!dg.ok) return -EIO;
  hipStream_t s = (hipStream_t)stream;
  if (d->n == 0) {
    hipError_t e = hipMemsetAsync(d->hdr, 0, sizeof(*d->hdr), s);
    if (e == hipSuccess) e = hipMemsetAsync(d->ports, 0, d->nports * sizeof(*d->ports), s);
    return hip_rc(e);
  }
  a.d = *d;
  a.nblk = l.nblk;
  const bool bytes = d->len != nullptr;
  const Cols col = {d->nports};
  const dim3 blk(kBlock);
  if (bytes)
    hipLaunchKernelGGL(dispatch_count_kernel<true>, dim3(l.nblk), blk, 0, s, a);
  else
    hipLaunchKernelGGL(dispatch_count_kernel<false>, dim3(l.nblk), blk, 0, s, a);
  hipLaunchKernelGGL(dispatch_scan_kernel, dim3(col.count(bytes)), dim3(kScan), 0, s, a.cnt, l.nblk,
                     col.prefixed(), a.tot);
  hipLaunchKernelGGL(dispatch_ports_kernel, dim3(1), dim3(64), 0, s, a, bytes);
  if (d->cap) hipLaunchKernelGGL(dispatch_scatter_kernel, dim3(l.nblk), blk, 0, s, a);
  return hip_rc(hipGetLastError());
}
