// copy16.h -- the device helpers of the re-aligning 16-byte-chunk copies
// (tx_frag.hip emit, tx_tunnel.hip encap) and of their header parses: the
// source at any byte address, the destination chunk 16-byte aligned, and
// nothing outside the aligned chunks of the source range is read.  The chunk
// type and the 16-bit sum helpers also serve rx_kernel.hip and tx_hdr.hip,
// through frame_view.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pptk {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t bswap16(uint32_t x) {
  return ((x & 0xffu) << 8) | ((x >> 8) & 0xffu);
}

// end-around-carry fold, as the reference's loop (iphdr/ipcksum.h:17-25)
__device__ __forceinline__ uint32_t fold16(uint32_t s) {
  s = (s & 0xffffu) + (s >> 16);
  s = (s & 0xffffu) + (s >> 16);
  return s;
}

__device__ __forceinline__ uint32_t halves(uint32_t w) { return (w & 0xffffu) + (w >> 16); }

__device__ __forceinline__ uint32_t ld_u8(uintptr_t A) { return *(const uint8_t *)A; }

// Four bytes at any byte address as a little-endian dword, from the one or
// two aligned dwords that hold them (both inside the frame when the four
// bytes are).
__device__ __forceinline__ uint32_t ld_le32(uintptr_t A) {
  const uint32_t *w = (const uint32_t *)(A & ~(uintptr_t)3);
  const uint32_t r = (uint32_t)(A & 3);
  const uint32_t lo = w[0], hi = w[r ? 1 : 0];
  return __builtin_amdgcn_alignbyte(hi, lo, r);
}

// The outer IPv4 subject test of the ops that take whole frames (tx_frag.hip
// plan, tx_tunnel.hip decap; host/outer_ipv4.h is its CPU statement): the
// IPv4 branch of the receive transform's parse (frame_view.h parse_frame) --
// one optional 802.1Q tag, ethertype 0x0800, version 4, 20 <= ihl <= tl,
// l2 + tl <= len.  A frame shorter than 14 bytes is not read at all; every
// other read lies inside the frame.
struct OuterIpv4 {
  uint32_t l2, ihl, tl;
  uint32_t w0, w1, w2;   // the header's first three words, little-endian
};

__device__ __forceinline__ bool outer_ipv4(uintptr_t F, uint32_t len, OuterIpv4 *o) {
  if (len < 14 || len > 65535) return false;
  uint32_t et = (ld_u8(F + 12) << 8) | ld_u8(F + 13), l2 = 14;
  if (et == 0x8100 && len >= 18) {
    et = (ld_u8(F + 16) << 8) | ld_u8(F + 17);
    l2 = 18;
  }
  if (et != 0x0800 || len < l2 + 20) return false;
  const uintptr_t ip = F + l2;
  const uint32_t w0 = ld_le32(ip), w1 = ld_le32(ip + 4), w2 = ld_le32(ip + 8);
  const uint32_t b0 = w0 & 0xffu, ihl = (b0 & 15u) * 4u;
  const uint32_t tl = bswap16(w0 >> 16);
  *o = {l2, ihl, tl, w0, w1, w2};
  return (b0 >> 4) == 4 && ihl >= 20 && tl >= ihl && l2 + tl <= len;
}

// 16 bytes from any byte address A, of which only those below `lim` (> A)
// are meaningful: the aligned chunk holding A and the aligned chunk holding
// the last needed byte (the same or the next one), funnelled to A's
// alignment.  Nothing outside the aligned chunks of [A, lim) is read.  The
// loads and the funnel are separate so that a lane can have the chunks of
// several rounds in flight before it shifts the first.
struct Raw16 {
  u32x4 lo, hi;
};

__device__ __forceinline__ Raw16 load16_raw(uintptr_t A, uintptr_t lim) {
  const uintptr_t end = A + 16 < lim ? A + 16 : lim;
  Raw16 r;
  r.lo = __builtin_nontemporal_load((const u32x4 *)(A & ~(uintptr_t)15));
  r.hi = __builtin_nontemporal_load((const u32x4 *)((end - 1) & ~(uintptr_t)15));
  return r;
}

__device__ __forceinline__ u32x4 funnel16(const Raw16 &c, uintptr_t A) {
  const uint32_t sh = (uint32_t)(A & 15), r = sh & 3u;
  // dword select in two steps (by 2, by 1), then the byte funnel
  const bool s2 = sh & 8u, s1 = sh & 4u;
  const uint32_t f0 = s2 ? c.lo.z : c.lo.x, f1 = s2 ? c.lo.w : c.lo.y, f2 = s2 ? c.hi.x : c.lo.z;
  const uint32_t f3 = s2 ? c.hi.y : c.lo.w, f4 = s2 ? c.hi.z : c.hi.x, f5 = s2 ? c.hi.w : c.hi.y;
  const uint32_t e0 = s1 ? f1 : f0, e1 = s1 ? f2 : f1, e2 = s1 ? f3 : f2, e3 = s1 ? f4 : f3;
  const uint32_t e4 = s1 ? f5 : f4;
  u32x4 o;
  o.x = __builtin_amdgcn_alignbyte(e1, e0, r);
  o.y = __builtin_amdgcn_alignbyte(e2, e1, r);
  o.z = __builtin_amdgcn_alignbyte(e3, e2, r);
  o.w = __builtin_amdgcn_alignbyte(e4, e3, r);
  return o;
}

__device__ __forceinline__ u32x4 load16(uintptr_t A, uintptr_t lim) {
  return funnel16(load16_raw(A, lim), A);
}

// mask of the first nb bytes of a dword (nb may be <= 0 or >= 4)
__device__ __forceinline__ uint32_t low_bytes(int nb) {
  return nb <= 0 ? 0u : (nb >= 4 ? 0xffffffffu : (1u << (8 * nb)) - 1u);
}

// the big-endian 16-bit field at slot offset pos (even) := val, if it lies in
// the chunk at slot offset o
__device__ __forceinline__ void put16(u32x4 &v, uint32_t o, uint32_t pos, uint32_t val) {
  const uint32_t rel = pos - o;
  if (rel >= 16) return;
  const uint32_t sh = (rel & 3u) * 8u, le = bswap16(val) << sh, keep = ~(0xffffu << sh);
#pragma unroll
  for (int d = 0; d < 4; ++d)
    if ((rel >> 2) == (uint32_t)d) v[d] = (v[d] & keep) | le;
}

}  // namespace pptk
