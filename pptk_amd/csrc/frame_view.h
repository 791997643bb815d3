// frame_view.h -- a frame as a lane sees it and its structural parse, shared
// by the receive transform (rx_kernel.hip), the in-place header kernels
// (tx_hdr.hip) and whatever else restates the parse (tx_frag.hip plan).
#pragma once
#include "../../include/pptk_rx.h"
#include "copy16.h"

// Explicit address spaces for every pointer the per-frame code dereferences:
// a pointer the compiler cannot place becomes a FLAT access, which counts in
// both vmcnt and lgkmcnt and may complete out of order, so every later wait
// on the streaming loads degrades to vmcnt(0) -- a drain of the prefetch.
#define LDS_AS __attribute__((address_space(3)))
#define GLB_AS __attribute__((address_space(1)))

namespace pptk {

// A value loaded from global memory on a rare path, made ready before the
// paths join: the empty asm consumes it, so its vmcnt wait sits inside the
// rare branch.  Consumed after the join instead, the wait would be a
// vmcnt(0) on the common path -- a drain of the prefetched rounds.
__device__ __forceinline__ uint32_t settle(uint32_t x) {
  asm volatile("" : "+v"(x));
  return x;
}

// A frame as seen by a lane: bytes [0, lim) from the LDS image (frame byte k
// at img[m + k], image = aligned 16-byte chunks from floor16(frame start)),
// everything else straight from global memory.
struct FrameView {
  const LDS_AS uint8_t *img;
  const GLB_AS uint8_t *g;
  int m;
  int lim;

  __device__ __forceinline__ uint32_t u8(int k) const {
    if (k < lim) return (uint32_t)img[m + k];
    return settle((uint32_t)g[k]);
  }
  __device__ __forceinline__ uint32_t be16(int k) const {
    return (u8(k) << 8) | u8(k + 1);
  }
  // 4 frame bytes at offset k as a little-endian dword (hdr_get32h).
  __device__ __forceinline__ uint32_t le32(int k) const {
    if (k + 4 <= lim) {
      const int a = m + k;
      const LDS_AS uint32_t *p = (const LDS_AS uint32_t *)(img + (a & ~3));
      return __builtin_amdgcn_alignbyte(p[1], p[0], (uint32_t)(a & 3));
    }
    return settle((uint32_t)g[k] | ((uint32_t)g[k + 1] << 8) | ((uint32_t)g[k + 2] << 16) |
                  ((uint32_t)g[k + 3] << 24));
  }
};

// Structural parse of one frame (the branchy part of DESIGN.md "Record
// semantics"): where L3/L4 are, what they are, and whether the L4 sum
// applies.  IP_OK / L4_OK / UDP_ZERO are decided later by the owning lane.
struct Parse {
  uint32_t flags, l3, ver, et, proto, rs, re;
  uint32_t fho;   // IPv6: offset of the last fragment header from L3 (0: none)
};

__device__ __forceinline__ bool is_v6_ext(uint32_t nh) {
  // is_ipv6_nexthdr, iphdr/iphdr.h:717-727
  return nh == 0 || nh == 60 || nh == 43 || nh == 44 || nh == 51;
}

__device__ __forceinline__ Parse parse_frame(const FrameView &v, uint32_t len) {
  Parse p = {0, 0, 0, 0, 0, 0, 0, 0};
  if (len < 14 || len > 65535) {
    p.flags = PPTK_RX_F_MALFORMED;
    return p;
  }
  uint32_t et = v.be16(12), l3 = 14;             // ether_type, iphdr.h:403
  if (et == 0x8100) {
    p.flags = PPTK_RX_F_VLAN;
    if (len < 18) {
      p.flags |= PPTK_RX_F_MALFORMED;
      return p;
    }
    et = v.be16(16);
    l3 = 18;
  }
  p.et = et;
  p.l3 = l3;
  uint32_t frag = 0;
  if (et == 0x0800) {
    if (len < l3 + 20) {
      p.flags |= PPTK_RX_F_MALFORMED;
      return p;
    }
    const uint32_t b0 = v.u8(l3);
    p.ver = b0 >> 4;                              // ip_version, :435
    const uint32_t ihl = (b0 & 15u) * 4u;         // ip_hdr_len, :876
    const uint32_t tl = v.be16(l3 + 2);           // ip_total_len, :943
    if (p.ver != 4 || ihl < 20 || tl < ihl || l3 + tl > len) {
      p.flags |= PPTK_RX_F_MALFORMED;
      return p;
    }
    p.flags |= PPTK_RX_F_PARSED;
    p.proto = v.u8(l3 + 9);                       // ip_proto, :1171
    frag = (v.be16(l3 + 6) & 0x3fffu) != 0;       // ip_frag_off/ip_more_frags
    p.rs = l3 + ihl;
    p.re = l3 + tl;
  } else if (et == 0x86dd) {
    p.flags |= PPTK_RX_F_IPV6;
    if (len < l3 + 40) {
      p.flags |= PPTK_RX_F_MALFORMED;
      return p;
    }
    p.ver = v.u8(l3) >> 4;
    const uint32_t tlen = v.be16(l3 + 4) + 40u;   // ipv6_payload_len + 40
    if (p.ver != 6 || l3 + tlen > len) {
      p.flags |= PPTK_RX_F_MALFORMED;
      return p;
    }
    // ipv6_const_proto_hdr_2, iphdr/iphdr.h:804-860, restated literally
    // (the length of the header at `off` is derived from the NEXT header's
    // type, as in the reference).
    uint32_t off = 40, nh = v.u8(l3 + 6);
    bool walked = false;
    while (is_v6_ext(nh)) {
      walked = true;
      if (off + 8u > tlen) {
        p.flags |= PPTK_RX_F_MALFORMED;
        p.fho = 0;
        return p;
      }
      if (nh == 44) {
        frag = 1;
        p.fho = off;
        if ((v.be16(l3 + off + 2) & 0xfff8u) > 0)
          break;
      }
      nh = v.u8(l3 + off);
      const uint32_t lf = v.u8(l3 + off + 1);
      const uint32_t extlen = nh == 44 ? 8u : (nh == 51 ? lf * 4u + 8u : lf * 8u + 8u);
      if (off + extlen > tlen) {
        p.flags |= PPTK_RX_F_MALFORMED;
        p.fho = 0;
        return p;
      }
      off = (off + extlen) & 0xffffu;
    }
    if (walked)
      p.flags |= PPTK_RX_F_V6_EXT;
    p.flags |= PPTK_RX_F_PARSED | PPTK_RX_F_IP_OK;
    p.proto = nh;
    p.rs = l3 + off;
    p.re = l3 + tlen;
  } else {
    return p;
  }
  if (frag)
    p.flags |= PPTK_RX_F_FRAGMENT;
  const uint32_t l4len = p.re - p.rs;
  if (!frag && ((p.proto == 6 && l4len >= 20) || (p.proto == 17 && l4len >= 8)))
    p.flags |= PPTK_RX_F_L4;
  return p;
}

}  // namespace pptk
