// tx_frag.hip -- pptk_ip_fragment_device: batched IPv4 fragmentation to an
// egress MTU (include/pptk_rx.h; reference ipfrag/ipfrag.c:11-123,
// fragment4).  Unlike the receive kernels the output size depends on the
// data, so the call runs in four launches:
//   plan   one lane per frame: the receive transform's structural IPv4
//          parse, the header checksum, status and fragment count; a block
//          scan leaves each frame's prefix inside its 256-frame tile
//   scan   one block: exclusive prefix of the tile sums, totals[0]
//   apply  one lane per frame: first[i], NOROOM, the caller's per-frame
//          arrays, totals[1]
//   emit   a team of 16 lanes per 16 frames walks the DONE frames among
//          them and copies each one's fragments, 16-byte chunk by chunk: a
//          re-aligning copy, the source at any byte offset, the destination
//          slot 16-byte aligned
// The scan is the classic three-launch one: nothing waits on another
// workgroup.
#include <errno.h>

#include "block_scan.h"
#include "frame_view.h"
#include "rx_internal.h"
#include "scratch_carve.h"

namespace pptk {
namespace {

constexpr int kTile = 256;                  // frames per plan / apply block = scan tile
constexpr int kScanThreads = 1024;
constexpr uint64_t kMaxFrames = 1ull << 24; // 65536 tiles: one scan block
constexpr int kTeam = 16;                   // lanes per source frame in the emit kernel
constexpr int kUnroll = 4;                  // team rounds whose loads are in flight together

struct FragArgs {
  FrameBatch fb;
  uint32_t mtu;
  uint8_t *out;
  uint64_t out_stride;
  uint64_t out_cap;
  uint16_t *out_len;     // nullable
  uint32_t *out_src;     // nullable
  uint32_t *first;       // nullable
  uint32_t *count;       // nullable
  uint8_t *status;       // nullable
  uint64_t *totals;
  // scratch
  uint64_t *s_info;      // DONE frames: S0 | tl << 16 | ihl << 32 | l2 << 40 | kept flag bits << 48
  uint64_t *s_tile;      // tile sums, then their exclusive prefix
  uint32_t *s_cnt;
  uint32_t *s_first;     // prefix inside the tile, then the global one
  uint8_t *s_st;
};

// the scratch's arrays, in order: without a base the walk sizes the scratch,
// with the scratch pointer it binds the arguments
size_t carve(uint64_t n, void *base, FragArgs *a) {
  Carve c(base, 16);
  a->s_info = c.take<uint64_t>(n);
  a->s_tile = c.take<uint64_t>((n + kTile - 1) / kTile);
  a->s_cnt = c.take<uint32_t>(n);
  a->s_first = c.take<uint32_t>(n);
  a->s_st = c.take<uint8_t>(n);
  return c.total();
}

// ---- plan ------------------------------------------------------------------
// The subject test is outer_ipv4 (copy16.h).
__global__ __launch_bounds__(kTile) void frag_plan_kernel(FragArgs a) {
  __shared__ uint32_t wsum[kTile / 64];
  const uint64_t i = (uint64_t)blockIdx.x * kTile + threadIdx.x;
  uint32_t st = 0, cnt = 0;
  if (i < a.fb.n) {
    const uintptr_t F = a.fb.addr(i);
    OuterIpv4 o;
    if (outer_ipv4(F, a.fb.len_at(i), &o)) {
      const uint32_t l2 = o.l2, ihl = o.ihl, tl = o.tl, w0 = o.w0, w1 = o.w1, w2 = o.w2;
      const uintptr_t ip = F + l2;
      st = PPTK_FRAG_ST_IPV4;
      if (tl <= a.mtu) {
        st |= PPTK_FRAG_ST_FITS;
      } else {
        // the header's one's-complement sum over little-endian halves
        // (byte order does not matter to the fold); s0 leaves out the
        // three fields every fragment rewrites: total length, flags +
        // offset, checksum
        uint32_t s0 = (w0 & 0xffffu) + (w1 & 0xffffu) + (w2 & 0xffffu) +
                      halves(ld_le32(ip + 12)) + halves(ld_le32(ip + 16));
        for (uint32_t k = 20; k < ihl; k += 4) s0 += halves(ld_le32(ip + k));
        const uint32_t all = s0 + (w0 >> 16) + (w1 >> 16) + (w2 >> 16);
        const uint32_t fw = bswap16(w1 >> 16);
        if (fw & 0x4000u) st |= PPTK_FRAG_ST_DF;
        if (fw & 0x3fffu) st |= PPTK_FRAG_ST_ISFRAG;
        if (fold16(all) != 0xffffu) st |= PPTK_FRAG_ST_BADCKSUM;
        if (st == PPTK_FRAG_ST_IPV4) {
          st |= PPTK_FRAG_ST_DONE;
          const uint32_t per = (a.mtu - ihl) & ~7u;
          cnt = (tl - ihl + per - 1) / per;
          // s0 holds the version byte, so its fold is 1..0xffff
          a.s_info[i] = (uint64_t)bswap16(fold16(s0)) | ((uint64_t)tl << 16) |
                        ((uint64_t)ihl << 32) | ((uint64_t)l2 << 40) |
                        ((uint64_t)(fw & 0xc000u) << 48);
        }
      }
    }
    a.s_cnt[i] = cnt;
    a.s_st[i] = (uint8_t)st;
  }
  // exclusive prefix inside the tile (at most 256 * 8190 slots: 32 bits)
  uint32_t total;
  const uint32_t before = block_excl_scan<kTile / 64, uint32_t>(cnt, wsum, &total);
  if (i < a.fb.n) a.s_first[i] = before;
  if (threadIdx.x == 0) a.s_tile[blockIdx.x] = total;
}

// ---- scan ------------------------------------------------------------------
__global__ __launch_bounds__(kScanThreads) void frag_scan_kernel(FragArgs a, uint32_t ntiles) {
  __shared__ uint64_t wsum[kScanThreads / 64];
  const uint32_t per = (ntiles + kScanThreads - 1) / kScanThreads;
  const uint32_t lo = min(threadIdx.x * per, ntiles), hi = min(lo + per, ntiles);
  uint64_t s = 0;
  for (uint32_t t = lo; t < hi; ++t) s += a.s_tile[t];
  // each thread sums a contiguous range and one scan runs over the threads'
  // sums, 64-bit: not the rounds of scan_counts
  uint64_t total;
  uint64_t run = block_excl_scan<kScanThreads / 64, uint64_t>(s, wsum, &total);
  for (uint32_t t = lo; t < hi; ++t) {
    const uint64_t v = a.s_tile[t];
    a.s_tile[t] = run;
    run += v;
  }
  if (threadIdx.x == 0) {
    a.totals[0] = total;
    // otherwise the one frame that straddles out_cap writes it (apply)
    if (total <= a.out_cap) a.totals[1] = total;
  }
}

// ---- apply -----------------------------------------------------------------
__global__ __launch_bounds__(kTile) void frag_apply_kernel(FragArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kTile + threadIdx.x;
  if (i >= a.fb.n) return;
  const uint64_t first = a.s_tile[blockIdx.x] + a.s_first[i];
  const uint32_t cnt = a.s_cnt[i];
  uint32_t st = a.s_st[i];
  if (cnt && first + cnt > a.out_cap) {
    st |= PPTK_FRAG_ST_NOROOM;
    a.s_st[i] = (uint8_t)st;
    // the slot intervals of the DONE frames are disjoint and ascending:
    // exactly one of them holds out_cap when the batch does not fit
    if (first <= a.out_cap) a.totals[1] = first;
  }
  a.s_first[i] = (uint32_t)first;
  if (a.first) a.first[i] = (uint32_t)first;
  if (a.count) a.count[i] = cnt;
  if (a.status) a.status[i] = (uint8_t)st;
}

// ---- emit ------------------------------------------------------------------
// (the re-aligning chunk loads and the field helpers: copy16.h)
__device__ __forceinline__ void emit_frame(const FragArgs &a, uint64_t i, uint32_t t,
                                           LDS_AS u32x4 *hds) {
  const uint64_t base = a.fb.base(i);
  const uint64_t info = a.s_info[i];
  const uint32_t first = a.s_first[i], count = a.s_cnt[i];
  const uint32_t s0 = (uint32_t)info & 0xffffu, tl = (uint32_t)(info >> 16) & 0xffffu;
  const uint32_t ihl = (uint32_t)(info >> 32) & 0xffu, l2 = (uint32_t)(info >> 40) & 0xffu;
  const uint32_t fkeep = (uint32_t)(info >> 48);   // the reserved bit (DF is clear)
  const uint32_t H = l2 + ihl, datamax = tl - ihl, per = (a.mtu - ihl) & ~7u;
  const uintptr_t F = (uintptr_t)a.fb.frames + base;

  // lengths and source indices of the frame's slots, a run of `count`
  for (uint32_t j = t; j < count; j += kTeam) {
    const uint32_t left = datamax - j * per;
    if (a.out_len) a.out_len[first + j] = (uint16_t)(H + (left < per ? left : per));
    if (a.out_src) a.out_src[first + j] = (uint32_t)i;
  }

  // the header chunks, once per frame, parked in the team's LDS slot: chunk c
  // = slot bytes [16c, 16c + 16) as far as they are header (at most five:
  // H <= 78).  The team's lanes are in one wave, whose LDS accesses keep
  // their order.
  __builtin_amdgcn_wave_barrier();
  if (16 * t < H) hds[t] = load16(F + 16 * t, F + H);
  __builtin_amdgcn_wave_barrier();

  // The frame's chunks as one index space across its fragments: c0 chunks for
  // every fragment but the last.  The team takes kTeam * kUnroll of them per
  // pass, whatever fragment they fall into, and issues all their loads before
  // the first chunk is shifted and stored.
  const uint32_t c0 = (H + per + 15) >> 4, last = count - 1;
  const uint32_t nchunks = last * c0 + ((H + datamax - last * per + 15) >> 4);
  for (uint32_t q0 = t; q0 < nchunks; q0 += kTeam * kUnroll) {
    Raw16 raw[kUnroll];
    uint32_t fj[kUnroll], fo[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const uint32_t q = q0 + kTeam * u;
      if (q < nchunks) {
        const uint32_t j = min(q / c0, last), o = (q - j * c0) * 16u;
        const uint32_t ds = j * per, left = datamax - ds, flen = H + (left < per ? left : per);
        fj[u] = j;
        fo[u] = o;
        // slot byte o >= H is frame byte o + ds
        if (o + 16 > H) raw[u] = load16_raw(F + ds + o, F + ds + flen);
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      if (q0 + kTeam * u < nchunks) {
        const uint32_t j = fj[u], o = fo[u];
        const uint32_t ds = j * per, left = datamax - ds, dl = left < per ? left : per;
        const uint32_t flen = H + dl;
        u32x4 v = {0, 0, 0, 0};
        if (o + 16 > H) v = funnel16(raw[u], F + ds + o);
        if (o < H) {   // a header chunk, the last one mixed with payload
          const uint32_t ntl = ihl + dl;                                   // ip_set_total_len
          const uint32_t nfw = fkeep | (ds + dl < datamax ? 0x2000u : 0u) | (ds >> 3);
          const uint32_t ck = ~fold16(s0 + ntl + nfw) & 0xffffu;            // ip_set_hdr_cksum_calc
          const u32x4 hd = hds[o >> 4];
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            const uint32_t m = low_bytes((int)H - (int)o - 4 * d);
            v[d] = (hd[d] & m) | (v[d] & ~m);
          }
          put16(v, o, l2 + 2, ntl);
          put16(v, o, l2 + 6, nfw);
          put16(v, o, l2 + 10, ck);
        }
        if (flen - o < 16) {   // zeros up to the next 16-byte boundary
#pragma unroll
          for (int d = 0; d < 4; ++d) v[d] &= low_bytes((int)(flen - o) - 4 * d);
        }
        *(u32x4 *)(a.out + (uint64_t)(first + j) * a.out_stride + o) = v;
      }
    }
  }
}

__global__ __launch_bounds__(256) void frag_emit_kernel(FragArgs a) {
  __shared__ u32x4 hdr_lds[256 / kTeam][5];
  LDS_AS u32x4 *hds = (LDS_AS u32x4 *)&hdr_lds[threadIdx.x / kTeam][0];
  const uint32_t t = threadIdx.x & (kTeam - 1);
  const uint64_t team = ((uint64_t)blockIdx.x * 256u + threadIdx.x) / kTeam;
  const uint64_t step = (uint64_t)gridDim.x * 256u;
  for (uint64_t g = team * kTeam; g < a.fb.n; g += step) {
    // each lane looks at one of the team's 16 frames; the team then walks
    // those that are to be written
    const uint32_t st = g + t < a.fb.n ? a.s_st[g + t] : 0u;
    const bool go = (st & (PPTK_FRAG_ST_DONE | PPTK_FRAG_ST_NOROOM)) == PPTK_FRAG_ST_DONE;
    uint32_t mask = (uint32_t)(__ballot(go) >> (threadIdx.x & 48u)) & 0xffffu;
    while (mask) {
      const uint32_t k = (uint32_t)__builtin_ctz(mask);
      mask &= mask - 1;
      emit_frame(a, g + k, t, hds);
    }
  }
}

}  // namespace
}  // namespace pptk

using namespace pptk;

extern "C" size_t pptk_ip_fragment_scratch_bytes(uint64_t n) {
  FragArgs a;
  return carve(n, nullptr, &a) + 64;
}

extern "C" int pptk_ip_fragment_device(struct pptk_rx_ctx *c, const uint8_t *d_frames,
                                       const uint64_t *d_off, const uint16_t *d_len,
                                       uint64_t stride, uint32_t fixed_len, uint64_t n,
                                       uint32_t mtu, uint8_t *d_out, uint64_t out_stride,
                                       uint64_t out_cap, uint16_t *d_out_len, uint32_t *d_out_src,
                                       uint32_t *d_first, uint32_t *d_count, uint8_t *d_status,
                                       uint64_t *d_totals, void *d_scratch, void *stream) {
  if (!c || !d_totals || n > kMaxFrames || mtu < 68 || mtu > 65535) return -EINVAL;
  if (((uintptr_t)d_out & 15u) || (out_stride & 15u) ||
      out_stride < ((18u + (uint64_t)mtu + 15u) & ~15ull) || out_cap > 0xffffffffull ||
      (!d_out && out_cap))
    return -EINVAL;
  if (n && (!d_scratch || ((uintptr_t)d_scratch & 15u))) return -EINVAL;
  if (!frame_batch_ok(d_frames, d_off, d_len, stride, fixed_len, n)) return -EINVAL;
  DeviceScope dg(ctx_device(c));
  if (!dg.ok) return -EIO;
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return hip_rc(hipMemsetAsync(d_totals, 0, 2 * sizeof(uint64_t), s));

  FragArgs a;
  a.fb = {d_frames, d_off, d_len, stride, n, fixed_len};
  a.mtu = mtu;
  a.out = d_out;
  a.out_stride = out_stride;
  a.out_cap = out_cap;
  a.out_len = d_out_len;
  a.out_src = d_out_src;
  a.first = d_first;
  a.count = d_count;
  a.status = d_status;
  a.totals = d_totals;
  (void)carve(n, d_scratch, &a);
  const uint32_t ntiles = (uint32_t)((n + kTile - 1) / kTile);
  hipLaunchKernelGGL(frag_plan_kernel, dim3(ntiles), dim3(kTile), 0, s, a);
  hipLaunchKernelGGL(frag_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, a, ntiles);
  hipLaunchKernelGGL(frag_apply_kernel, dim3(ntiles), dim3(kTile), 0, s, a);
  hipLaunchKernelGGL(frag_emit_kernel, dim3(ntiles), dim3(256), 0, s, a);
  return hip_rc(hipGetLastError());
}
