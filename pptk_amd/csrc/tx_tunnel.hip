// tx_tunnel.hip -- pptk_tunnel_encap_device / pptk_tunnel_decap_device: the
// GRE tunnel gateway of the reference's ldp/ldptunnel.c on batches in device
// memory (include/pptk_rx.h).
//   encap  one launch, a team of lanes per frame: a re-aligning copy with a
//          38-byte prepend.  Slot i belongs to frame i, so nothing is scanned.
//          The header's two whole chunks are built from the tunnel entry by
//          the team's first two lanes; the frame follows chunk by chunk, the
//          source at any byte offset (slot byte o is frame byte o - 38), the
//          destination chunk 16-byte aligned, several rounds of loads in
//          flight before the first funnel shift (tx_frag.hip's emit).
//   decap  one lane per frame over the outer header; writes descriptors only.
#include <errno.h>

#include "copy16.h"
#include "rx_internal.h"

namespace pptk {
namespace {

constexpr int kBlock = 256;
constexpr int kUnroll = 4;        // team rounds whose loads are in flight together
constexpr uint32_t kHdr = PPTK_TUN_HDR_LEN;
constexpr uint32_t kMaxGrid = 1u << 14;   // beyond it the teams stride over the batch

// Lanes per frame, by measurement (tools/tunnel_perf.py --sweep: 16 M frames,
// A/B builds with -DPPTK_TUN_TEAM=T, this grid cap; DESIGN.md "GRE tunnel
// gateway").  Encap ms with 4 / 8 / 16 / 32 lanes at one fixed length:
//     64 B   1.01   1.31   2.21   3.96        384 B   6.23   4.11   3.40   5.23
//    128 B   2.13   1.75   2.51   4.17        768 B  10.99   7.72   6.36   6.69
//    256 B   4.12   2.77   3.06   4.77       1024 B  16.30  11.47   8.84   8.50
//                                            1500 B  21.18  15.49  12.08  10.56
// The switch points lie between the measured lengths that disagree (they are
// not measured themselves).  With a length array the lengths are device data:
// 16 lanes were fastest on both mixed-length batches of harness/synth.py
// (IMIX 6.12 / 5.18 / 5.00 / 6.80 ms, CMIX 13.27 / 10.45 / 9.04 / 9.07 ms).
// PPTK_TUN_TEAM builds one width for every case (A/B).
constexpr uint32_t kLen4 = 96, kLen8 = 320, kLen16 = 896;   // longest fixed length per width
#ifdef PPTK_TUN_TEAM
constexpr int kTeamAny = PPTK_TUN_TEAM;
#else
constexpr int kTeamAny = 16;
#endif

struct EncapArgs {
  FrameBatch fb;
  const pptk_tunnel *tun;
  uint64_t tun_count;
  const uint32_t *idx;   // nullable -> tun[tun_one ? 0 : i]
  uint8_t *out;
  uint64_t out_stride;
  uint16_t *out_len;     // nullable
  uint8_t *status;       // nullable
  uint32_t tun_one;
  uint32_t id_base;
};

struct DecapArgs {
  FrameBatch fb;
  uint64_t *in_off;      // nullable
  uint16_t *in_len;      // nullable
  uint8_t *status;       // nullable
};

__device__ __forceinline__ uint32_t bswap32(uint32_t x) { return __builtin_bswap32(x); }

// The chunks of [F, F + len) that hold the 16 bytes from A = F + o - 38 on.
// For the first payload chunk (o = 32) A lies 6 bytes before the frame: when
// A's aligned chunk is not the frame's first one it is not loaded (its bytes
// land in the header part of the slot chunk, which the caller overwrites).
__device__ __forceinline__ Raw16 load_payload(uintptr_t F, uintptr_t A, uintptr_t lim) {
  if ((A & ~(uintptr_t)15) >= (F & ~(uintptr_t)15)) return load16_raw(A, lim);
  const uintptr_t end = A + 16 < lim ? A + 16 : lim;   // > F: len >= 14
  Raw16 r;
  r.lo = u32x4{0, 0, 0, 0};
  r.hi = __builtin_nontemporal_load((const u32x4 *)((end - 1) & ~(uintptr_t)15));
  return r;
}

template <int T>
__global__ __launch_bounds__(kBlock) void tunnel_encap_kernel(EncapArgs a) {
  const uint32_t t = threadIdx.x & (T - 1);
  const uint64_t team = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) / T;
  const uint64_t nteams = (uint64_t)gridDim.x * (kBlock / T);
  for (uint64_t i = team; i < a.fb.n; i += nteams) {
    const uint64_t ti = a.idx ? (uint64_t)a.idx[i] : (a.tun_one ? 0 : i);
    uint32_t st = 0, len = 0;
    u32x4 ta = {0, 0, 0, 0}, tb = {0, 0, 0, 0};
    if (ti >= a.tun_count) {
      st = PPTK_TUN_ST_NOFLOW;
    } else {
      // the tunnel entry: eth_dst, eth_src | src, dst, id + ttl + tos, flags, reserved
      const u32x4 *tp = (const u32x4 *)(a.tun + ti);
      ta = tp[0];
      tb = tp[1];
      if ((tb.z & ~(PPTK_TUN_DF | PPTK_TUN_ID_SEQ)) || tb.w) {
        st = PPTK_TUN_ST_BADTUN;
      } else {
        len = a.fb.len_at(i);
        if (len < 14) {
          st = PPTK_TUN_ST_RUNT;
        } else {
          if (kHdr + len > 65535u) st |= PPTK_TUN_ST_TOOBIG;
          if ((uint64_t)kHdr + len > a.out_stride) st |= PPTK_TUN_ST_NOROOM;
          if (!st) st = PPTK_TUN_ST_DONE;
        }
      }
    }
    const uint32_t tot = kHdr + len;
    if (t == 0) {
      if (a.status) a.status[i] = (uint8_t)st;
      if (a.out_len) a.out_len[i] = (uint16_t)(st == PPTK_TUN_ST_DONE ? tot : 0u);
    }
    if (st != PPTK_TUN_ST_DONE) continue;

    const uintptr_t F = a.fb.addr(i);
    uint8_t *slot = a.out + i * a.out_stride;
    const uint32_t src_be = bswap32(ta.w), dst_be = bswap32(tb.x);

    // slot bytes [0, 32): Ethernet and the IPv4 header up to the first half of
    // the destination address
    if (t == 0) {
      const uint32_t tos = tb.y >> 24;
      *(u32x4 *)slot = u32x4{ta.x, ta.y, ta.z, 0x00450008u | (tos << 24)};
    } else if (t == 1) {
      const uint32_t tos = tb.y >> 24, ttl = (tb.y >> 16) & 0xffu;
      const uint32_t seq = (tb.z & PPTK_TUN_ID_SEQ) ? a.id_base + (uint32_t)i : 0u;
      const uint32_t id = (tb.y + seq) & 0xffffu, tl = len + 24u;
      const uint32_t fw = (tb.z & PPTK_TUN_DF) ? 0x4000u : 0u;
      // the template's sum (everything but total length and id), then
      // ip_set_hdr_cksum_calc as ~fold16(S0 + tl + id)
      const uint32_t s0 = (0x4500u | tos) + fw + ((ttl << 8) | 47u) + halves(ta.w) + halves(tb.x);
      const uint32_t ck = ~fold16(s0 + tl + id) & 0xffffu;
      u32x4 v;
      v.x = bswap16(tl) | (bswap16(id) << 16);
      v.y = bswap16(fw) | (ttl << 16) | (47u << 24);
      v.z = bswap16(ck) | (src_be << 16);
      v.w = (src_be >> 16) | (dst_be << 16);
      *(u32x4 *)(slot + 16) = v;
    }

    // slot chunks 2 .. nchunks - 1: the frame, shifted by 38 bytes
    const uint32_t nchunks = (tot + 15u) >> 4;
    const uintptr_t lim = F + len;
    for (uint32_t q0 = 2 + t; q0 < nchunks; q0 += T * kUnroll) {
      Raw16 raw[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const uint32_t q = q0 + T * u;
        if (q < nchunks) raw[u] = load_payload(F, F + 16u * q - kHdr, lim);
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const uint32_t q = q0 + T * u;
        if (q < nchunks) {
          const uint32_t o = 16u * q;
          u32x4 v = funnel16(raw[u], F + o - kHdr);
          if (q == 2) {   // bytes 32..37: the address's second half, GRE 00 00 65 58
            v.x = dst_be >> 16;
            v.y = (v.y & 0xffff0000u) | 0x5865u;
          }
          if (tot - o < 16) {   // zeros up to the next 16-byte boundary
#pragma unroll
            for (int d = 0; d < 4; ++d) v[d] &= low_bytes((int)(tot - o) - 4 * d);
          }
          *(u32x4 *)(slot + o) = v;
        }
      }
    }
  }
}

// The outer subject test is outer_ipv4 (copy16.h).
__global__ __launch_bounds__(kBlock) void tunnel_decap_kernel(DecapArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.fb.n) return;
  const uint64_t base = a.fb.base(i);
  const uint32_t len = a.fb.len_at(i);
  const uintptr_t F = (uintptr_t)a.fb.frames + base;
  uint32_t st = 0, in_len = 0;
  uint64_t in_off = base;
  OuterIpv4 o;
  if (outer_ipv4(F, len, &o)) {
    const uint32_t l2 = o.l2, ihl = o.ihl, tl = o.tl, w0 = o.w0, w1 = o.w1, w2 = o.w2;
    const uintptr_t ip = F + l2;
    st = PPTK_DECAP_ST_IPV4;
    if (((w2 >> 8) & 0xffu) == 47u) {
      uint32_t sum = halves(w0) + halves(w1) + halves(w2) + halves(ld_le32(ip + 12)) +
                     halves(ld_le32(ip + 16));
      for (uint32_t k = 20; k < ihl; k += 4) sum += halves(ld_le32(ip + k));
      if (fold16(sum) != 0xffffu) st |= PPTK_DECAP_ST_BADCKSUM;
      if (bswap16(w1 >> 16) & 0x3fffu) {
        st |= PPTK_DECAP_ST_ISFRAG;
      } else if (tl - ihl < 4) {
        st |= PPTK_DECAP_ST_SHORT;
      } else {
        st |= PPTK_DECAP_ST_GRE;
        const uint32_t g = ld_le32(ip + ihl);
        if (g & 0xffffu) st |= PPTK_DECAP_ST_GREOPT;
        if ((g >> 16) != 0x5865u) st |= PPTK_DECAP_ST_PTYPE;
        if (st == (PPTK_DECAP_ST_IPV4 | PPTK_DECAP_ST_GRE)) {
          st |= PPTK_DECAP_ST_OK;
          in_off = base + l2 + ihl + 4;
          in_len = tl - ihl - 4;
        }
      }
    }
  }
  if (a.in_off) a.in_off[i] = in_off;
  if (a.in_len) a.in_len[i] = (uint16_t)in_len;
  if (a.status) a.status[i] = (uint8_t)st;
}

template <int T>
void launch_encap(const EncapArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(tunnel_encap_kernel<T>, dim3(capped_grid(a.fb.n, kBlock / T, kMaxGrid)),
                     dim3(kBlock), 0, s, a);
}

}  // namespace
}  // namespace pptk

using namespace pptk;

extern "C" int pptk_tunnel_encap_device(struct pptk_rx_ctx *c, const uint8_t *d_frames,
                                        const uint64_t *d_off, const uint16_t *d_len,
                                        uint64_t stride, uint32_t fixed_len, uint64_t n,
                                        const struct pptk_tunnel *d_tun, uint64_t tun_count,
                                        const uint32_t *d_idx, uint32_t id_base, uint8_t *d_out,
                                        uint64_t out_stride, uint16_t *d_out_len,
                                        uint8_t *d_status, void *stream) {
  static_assert(sizeof(struct pptk_tunnel) == 32, "struct pptk_tunnel is 32 bytes");
  if (!c || !d_tun || ((uintptr_t)d_tun & 15u) || tun_count == 0 ||
      (!d_idx && tun_count != 1 && tun_count != n))
    return -EINVAL;
  if (((uintptr_t)d_out & 15u) || (out_stride & 15u) || (n && !d_out)) return -EINVAL;
  if (!frame_batch_ok(d_frames, d_off, d_len, stride, fixed_len, n)) return -EINVAL;
  DeviceScope dg(ctx_device(c));
  if (!dg.ok) return -EIO;
  if (n == 0) return 0;
  EncapArgs a;
  a.fb = {d_frames, d_off, d_len, stride, n, fixed_len};
  a.tun = d_tun;
  a.tun_count = tun_count;
  a.idx = d_idx;
  a.out = d_out;
  a.out_stride = out_stride;
  a.out_len = d_out_len;
  a.status = d_status;
  a.tun_one = tun_count == 1;
  a.id_base = id_base;
  hipStream_t s = (hipStream_t)stream;
#ifdef PPTK_TUN_TEAM
  launch_encap<kTeamAny>(a, s);
#else
  if (d_len)
    launch_encap<kTeamAny>(a, s);
  else if (fixed_len <= kLen4)
    launch_encap<4>(a, s);
  else if (fixed_len <= kLen8)
    launch_encap<8>(a, s);
  else if (fixed_len <= kLen16)
    launch_encap<16>(a, s);
  else
    launch_encap<32>(a, s);
#endif
  return hip_rc(hipGetLastError());
}

extern "C" int pptk_tunnel_decap_device(struct pptk_rx_ctx *c, const uint8_t *d_frames,
                                        const uint64_t *d_off, const uint16_t *d_len,
                                        uint64_t stride, uint32_t fixed_len, uint64_t n,
                                        uint64_t *d_in_off, uint16_t *d_in_len,
                                        uint8_t *d_status, void *stream) {
  if (!c || !frame_batch_ok(d_frames, d_off, d_len, stride, fixed_len, n)) return -EINVAL;
  const uint64_t blocks = (n + kBlock - 1) / kBlock;
  if (blocks > 0x7fffffffull) return -EINVAL;
  DeviceScope dg(ctx_device(c));
  if (!dg.ok) return -EIO;
  if (n == 0) return 0;
  DecapArgs a;
  a.fb = {d_frames, d_off, d_len, stride, n, fixed_len};
  a.in_off = d_in_off;
  a.in_len = d_in_len;
  a.status = d_status;
  hipLaunchKernelGGL(tunnel_decap_kernel, dim3((uint32_t)blocks), dim3(kBlock), 0,
                     (hipStream_t)stream, a);
  return hip_rc(hipGetLastError());
}
