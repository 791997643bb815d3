// tx_hdr.hip -- the kernels that edit frame headers in place: header rewrite
// (pptk_tx_rewrite_device), TCP MSS clamping (pptk_tcp_mss_clamp_device),
// TCP sequence-space translation (pptk_tcp_seq_translate_device) and the
// second pass of the two-pass tx checksums (launch_tx_apply).
//
// The three header kernels share one lane scaffold: one lane per frame, the
// frame's first aligned 16-byte chunks in the lane's LDS slot (load_frame),
// the receive transform's parse on that image (frame_view.h), the edit in
// the image, and the changed chunks written back by one rule (write_back).
#include <algorithm>

#include "frame_view.h"
#include "rx_internal.h"

namespace pptk {

namespace {

// RFC 1624 incremental checksum updates, as the reference composes them
__device__ __forceinline__ uint32_t upd16(uint32_t ck, uint32_t o, uint32_t nw) {
  // ip_update_cksum16 (iphdr/ipcksum.h:213-226)
  uint32_t s = (~ck & 0xffffu) + (~o & 0xffffu) + nw;
  s = fold16(s);
  return ~s & 0xffffu;
}
__device__ __forceinline__ uint32_t upd32(uint32_t ck, uint32_t o, uint32_t nw) {
  // ip_update_cksum32 (:228-236): high halves, then low halves
  return upd16(upd16(ck, o >> 16, nw >> 16), o & 0xffffu, nw & 0xffffu);
}

// Lane slots of the header kernels sit an odd number of dwords apart (slot
// + 4 bytes): the per-frame parse reads the same frame offset in every
// lane's slot, which at a 64- or 128-byte pitch falls into one or two LDS
// banks (a 32- to 64-way conflict on every byte read: SQ_ACTIVE_INST_LDS
// ~15x SQ_INSTS_LDS); at an odd dword pitch the lanes spread over all 32
// banks.  The slots are then only 4-byte aligned, so chunks are parked and
// read back as dwords.
template <int SLOT>
__device__ __forceinline__ LDS_AS uint8_t *lane_slot() {
  __shared__ __attribute__((aligned(16))) uint8_t lds[256 * (SLOT + 4)];
  return (LDS_AS uint8_t *)lds + threadIdx.x * (SLOT + 4);
}

template <int SLOT>
__device__ __forceinline__ void park_chunks(LDS_AS uint8_t *slot, const u32x4 *c0, int nch) {
  LDS_AS uint32_t *w = (LDS_AS uint32_t *)slot;
#pragma unroll
  for (int c = 0; c < SLOT / 16; ++c) {
    const u32x4 v = c0[min(c, nch - 1)];
    w[4 * c] = v.x;
    w[4 * c + 1] = v.y;
    w[4 * c + 2] = v.z;
    w[4 * c + 3] = v.w;
  }
}

// Frame i of the batch in the lane's slot: its first SLOT / 16 aligned
// chunks (clamped to the frame's own chunks) parked, SLOT - m frame bytes
// readable from the image and the rest through the FrameView rare path.
struct LaneFrame {
  uint64_t base;   // byte offset of the frame in the batch
  uint32_t len;
  int m;           // the frame's start inside its first chunk
  FrameView v;
};

template <int SLOT>
__device__ __forceinline__ LaneFrame load_frame(const HdrBatch &b, uint64_t i,
                                                LDS_AS uint8_t *slot) {
  const uint64_t base = b.fb.base(i);
  const uint32_t len = b.fb.len_at(i);
  const int m = (int)(base & 15);
  const int nch = max((m + (int)len + 15) >> 4, 1);
  park_chunks<SLOT>(slot, (const u32x4 *)(b.fb.frames + (base - (uint64_t)m)), nch);
  return {base, len, m, {slot, (const GLB_AS uint8_t *)b.fb.frames + base, m, SLOT - m}};
}

// The write-back of one chunk of a patched slot.  `row` is the frame's first
// aligned chunk in the writable batch (frame start - m) and `changed` the
// 16-bit mask of the bytes of slot chunk c that the edit changed.  A chunk
// that lies inside the frame goes back whole; of a chunk that reaches
// outside it only the changed bytes do, one by one (the others may be a
// neighbour's).  A chunk without a changed byte is not written (writing
// those back as well cost the rewrite C64 0.526 vs 0.463 ms, C1500 1.300 vs
// 1.220 ms).
__device__ __forceinline__ void write_back(const LDS_AS uint8_t *slot, GLB_AS uint8_t *row, int c,
                                           int m, uint32_t len, uint32_t changed) {
  if (!changed) return;
  const int fo = 16 * c - m;   // frame offset of the chunk
  if (fo >= 0 && fo + 16 <= (int)len) {
    const LDS_AS uint32_t *w = (const LDS_AS uint32_t *)slot + 4 * c;
    *(GLB_AS u32x4 *)(row + 16 * c) = (u32x4){w[0], w[1], w[2], w[3]};
  } else {
    while (changed) {
      const int b = __builtin_ctz(changed);
      row[16 * c + b] = slot[16 * c + b];
      changed &= changed - 1;
    }
  }
}

// Field writes of one frame: patched into the lane's LDS image (and marked
// in `touched`) where the image holds the byte, stored directly otherwise;
// flush() then writes the touched image chunks back (write_back) -- whole
// 16-byte chunks instead of a dozen scattered byte stores per frame: C64
// 0.77 -> 0.58 ms, C1500 1.47 -> 1.24 ms, CMIX 1.28 -> 1.15 ms (in-process
// A/B, tools/ab_rewrite.py).
template <int SLOT>
struct FieldWriter {
  LDS_AS uint8_t *img;
  GLB_AS uint8_t *f;     // frame start
  int m;
  uint64_t touched = 0;  // image byte positions patched

  __device__ __forceinline__ void put(int k, uint32_t v, int nbytes) {
    for (int b = 0; b < nbytes; ++b) {
      const uint8_t x = (uint8_t)(v >> (8 * (nbytes - 1 - b)));
      const int pos = m + k + b;
      if (pos < SLOT) {
        img[pos] = x;
        touched |= 1ull << pos;
      } else {
        f[k + b] = x;
      }
    }
  }
  __device__ __forceinline__ void flush(uint32_t len) {
    if (!touched) return;
#pragma unroll
    for (int c = 0; c < SLOT / 16; ++c)   // masked by slot position
      write_back(img, f - m, c, m, len, (uint32_t)(touched >> (16 * c)) & 0xffffu);
  }
};

// Header rewrite with incremental checksum updates (pptk_tx_rewrite_device,
// reference iphdr/ipcksum.h:213-393): the lane parses its frame exactly as
// the receive transform does, folds the requested changes into the
// transmitted checksums with RFC 1624 updates, and stores the changed
// fields.  The lane's image holds the frame's first four aligned chunks, 64
// - m frame bytes: every field of an IPv4 frame with a 20-byte header lies
// in the first 52 bytes (56 behind a VLAN tag), so the image covers it when
// the frame starts at most 12 (8) bytes into its chunk; fields past the
// image come from global memory through the FrameView rare path.
constexpr int RW_SLOT = 64;

__global__ __launch_bounds__(256) void rx_rewrite_kernel(RewriteKArgs a) {
  LDS_AS uint8_t *slot = lane_slot<RW_SLOT>();
  const uint64_t step = (uint64_t)gridDim.x * 256u;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < a.b.fb.n; i += step) {
    const uint64_t j = a.idx ? (uint64_t)a.idx[i] : (a.rw_one ? 0u : i);
    if (a.idx && j >= a.rw_count) {   // no flow: the frame is not even read
      if (a.b.status) a.b.status[i] = (uint8_t)PPTK_RW_ST_NOFLOW;
      continue;
    }
    const LaneFrame fr = load_frame<RW_SLOT>(a.b, i, slot);
    const uint64_t base = fr.base;
    const uint32_t len = fr.len;
    const int m = fr.m;
    const FrameView &v = fr.v;
    const Parse p = parse_frame(v, len);
    uint32_t st = 0;
    if ((p.flags & (PPTK_RX_F_PARSED | PPTK_RX_F_MALFORMED | PPTK_RX_F_IPV6)) == PPTK_RX_F_PARSED) {
      const pptk_rewrite w = a.rw[j];
      const int l3 = (int)p.l3, l4 = (int)p.rs;
      const bool l4ok = p.flags & PPTK_RX_F_L4;
      const uint32_t proto = p.proto;
      uint32_t ttl = v.u8(l3 + 8);
      if ((w.ops & PPTK_RW_DECR_TTL) && ttl == 0) {
        st = PPTK_RW_ST_TTL_ZERO;   // the reference abort()s (:382-385)
      } else {
        st = PPTK_RW_ST_IP | (l4ok ? PPTK_RW_ST_L4 : 0u);
        FieldWriter<RW_SLOT> fw{slot, (GLB_AS uint8_t *)a.b.frames_w + base, m};
        const int cko = proto == 6 ? 16 : 6;          // TCP / UDP checksum field
        uint32_t ipc = v.be16(l3 + 10);
        uint32_t l4c = l4ok ? v.be16(l4 + cko) : 0u;
        bool l4c_w = false;
        if (w.ops & PPTK_RW_DECR_TTL) {   // ip_decr_ttl_cksum_update (:374-393)
          ipc = upd16(ipc, (ttl << 8) | proto, ((ttl - 1) << 8) | proto);
          ttl -= 1;
          fw.put(l3 + 8, ttl, 1);
          if (ttl == 0) st |= PPTK_RW_ST_EXPIRED;
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {    // ip_set_src/dst_cksum_update (:238-261, :349-372)
          const uint32_t op = k == 0 ? PPTK_RW_SRC : PPTK_RW_DST;
          if (!(w.ops & op)) continue;
          const uint32_t nw = k == 0 ? w.src : w.dst;
          const uint32_t old = __builtin_bswap32(v.le32(l3 + 12 + 4 * k));
          ipc = upd32(ipc, old, nw);
          if (l4ok && (proto == 6 || l4c != 0)) {   // UDP: a 0 checksum stays 0
            l4c = upd32(l4c, old, nw);
            l4c_w = true;
          }
          fw.put(l3 + 12 + 4 * k, nw, 4);
        }
        if (l4ok) {
#pragma unroll
          for (int k = 0; k < 2; ++k) {  // tcp/udp_set_src/dst_port_cksum_update (:263-347)
            const uint32_t op = k == 0 ? PPTK_RW_SPORT : PPTK_RW_DPORT;
            if (!(w.ops & op)) continue;
            const uint32_t nw = k == 0 ? w.sport : w.dport;
            if (proto == 6 || l4c != 0) {
              l4c = upd16(l4c, v.be16(l4 + 2 * k), nw);
              l4c_w = true;
            }
            fw.put(l4 + 2 * k, nw, 2);
          }
        }
        if ((w.ops & PPTK_RW_ICMP_ID) && proto == 1 && !(p.flags & PPTK_RX_F_FRAGMENT) &&
            p.re - p.rs >= 8u) {
          // icmp_set_echo_identifier_cksum_update (:283-291) on an echo
          // request / reply; the ICMP checksum has no pseudo-header, so the
          // address changes above leave it alone
          const uint32_t type = v.u8(l4);
          if (type == 8 || type == 0) {
            fw.put(l4 + 2, upd16(v.be16(l4 + 2), v.be16(l4 + 4), w.sport), 2);
            fw.put(l4 + 4, w.sport, 2);
            st |= PPTK_RW_ST_ICMP;
          }
        }
        if (w.ops & (PPTK_RW_DECR_TTL | PPTK_RW_SRC | PPTK_RW_DST))
          fw.put(l3 + 10, ipc, 2);
        if (l4c_w)
          fw.put(l4 + cko, l4c, 2);
        fw.flush(len);
      }
    }
    if (a.b.status) a.b.status[i] = (uint8_t)st;
  }
}

// TCP MSS clamping (pptk_tcp_mss_clamp_device): one lane per frame, the
// frame's first eight aligned chunks in the lane's LDS slot (Ethernet, IPv4
// or IPv6 with a VLAN tag and a 20-byte IP header leave the TCP options in
// it; longer headers reach the rest through the FrameView rare path), the
// receive transform's parse, tcp_parse_options (iphdr/iphdr.c:4-132) over
// the options, and tcp_set_mss_cksum_update (iphdr/ipcksum.h:466-489) when
// the MSS option exceeds the clamp.  Only clamped frames are written (four
// bytes: the option value and the checksum).
constexpr int MSS_SLOT = 128;

__global__ __launch_bounds__(256) void rx_mss_kernel(MssKArgs a) {
  LDS_AS uint8_t *slot = lane_slot<MSS_SLOT>();
  const uint64_t step = (uint64_t)gridDim.x * 256u;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < a.b.fb.n; i += step) {
    const LaneFrame fr = load_frame<MSS_SLOT>(a.b, i, slot);
    const uint64_t base = fr.base;
    const uint32_t len = fr.len;
    const int m = fr.m;
    const FrameView &v = fr.v;
    const Parse p = parse_frame(v, len);
    uint32_t st = 0;
    if ((p.flags & (PPTK_RX_F_PARSED | PPTK_RX_F_MALFORMED | PPTK_RX_F_L4)) ==
            (PPTK_RX_F_PARSED | PPTK_RX_F_L4) &&
        p.proto == 6) {
      const int t = (int)p.rs;   // TCP header
      if (!(a.flags & PPTK_MSS_SYN_ONLY) || (v.u8(t + 13) & 2u)) {
        st = PPTK_MSS_ST_TCP;
        const int end = (int)(v.u8(t + 12) >> 4) * 4;   // tcp_data_offset
        if (t + end > (int)p.re) {
          st |= PPTK_MSS_ST_BADOPT;   // options past the segment
        } else {
          // tcp_parse_options: kind 0 ends the list, kind 1 is a NOP, any
          // other option is min(length byte, bytes left) long (the bytes
          // left when its length byte is past the options) and the list is
          // malformed below 2; the last 4-byte MSS option counts
          int off = 20, mssoff = 0;
          uint32_t mssv = 536u;
          bool valid = true;
          // one exit branch per option: the kind, length and MSS bytes are
          // read unconditionally (a length byte past the options is not
          // used) and combined arithmetically
          auto walk = [&](auto rd) __attribute__((always_inline)) {
            while (off < end) {
              const uint32_t kind = rd(t + off), lb = rd(t + off + 1);
              const uint32_t mv = (rd(t + off + 2) << 8) | rd(t + off + 3);
              int L = off + 1 < end ? min(end - off, (int)lb) : 1;
              L = kind == 1 ? 1 : L;
              const bool bad = kind > 1 && L < 2;
              const bool is_mss = kind == 2 && L == 4;
              mssv = is_mss ? mv : mssv;
              mssoff = is_mss ? off : mssoff;
              if (kind == 0 || bad) {
                valid = !bad;
                break;
              }
              off += L;
            }
          };
          if (m + t + end <= MSS_SLOT) {
            // the whole option list (and 3 bytes past it, in the slot or
            // its 4 pad bytes) is in the LDS image: plain LDS reads
            const LDS_AS uint8_t *img = v.img + m;
            walk([&](int k) __attribute__((always_inline)) { return (uint32_t)img[k]; });
          } else {
            // long headers (IPv6 extension chains): reads past the image
            // come from global memory, clamped to the frame
            walk([&](int k) __attribute__((always_inline)) {
              return v.u8(min(k, (int)len - 1));
            });
          }
          if (!valid) {
            st |= PPTK_MSS_ST_BADOPT;
          } else if (mssoff) {
            st |= PPTK_MSS_ST_FOUND;
            if (mssv > a.mss) {
              // tcp_set_mss_cksum_update: a value at an even TCP offset is
              // one checksum word; at an odd offset it straddles two, each
              // updated with its other byte unchanged (that byte cancels in
              // the RFC 1624 sum, so a byte past the frame is taken as 0)
              const int f = t + mssoff + 2;
              uint32_t ck = v.be16(t + 16);
              if (!(mssoff & 1)) {
                ck = upd16(ck, mssv, a.mss);
              } else {
                const uint32_t x1 = v.u8(f - 1);
                const uint32_t x2 = f + 2 < (int)len ? v.u8(f + 2) : 0u;
                ck = upd16(ck, (x1 << 8) | (mssv >> 8), (x1 << 8) | (a.mss >> 8));
                ck = upd16(ck, ((mssv & 0xffu) << 8) | x2, ((a.mss & 0xffu) << 8) | x2);
              }
              GLB_AS uint8_t *fw = (GLB_AS uint8_t *)a.b.frames_w + base;
              // each field as one 16-bit store where its address is even.
              // The stores dominate this kernel: loading, parking, parsing
              // and walking 16 M SYNs takes 0.29 ms, the four byte stores
              // per frame added 0.35 ms; two 16-bit stores cut the total
              // 0.639 -> 0.577 ms; writing back the patched 16-byte image
              // chunks instead measured the same (0.575), non-temporal
              // 16-bit stores 2 % slower (tools/ab_mss.py, one box each)
              const uintptr_t fa = (uintptr_t)(fw + f), ca = (uintptr_t)(fw + t + 16);
              if (!(fa & 1)) {
                *(GLB_AS uint16_t *)(fw + f) = (uint16_t)bswap16(a.mss);
              } else {
                fw[f] = (uint8_t)(a.mss >> 8);
                fw[f + 1] = (uint8_t)a.mss;
              }
              if (!(ca & 1)) {
                *(GLB_AS uint16_t *)(fw + t + 16) = (uint16_t)bswap16(ck);
              } else {
                fw[t + 16] = (uint8_t)(ck >> 8);
                fw[t + 17] = (uint8_t)ck;
              }
              st |= PPTK_MSS_ST_CLAMPED;
            }
          }
        }
      }
    }
    if (a.b.status) a.b.status[i] = (uint8_t)st;
  }
}

// TCP sequence-space translation (pptk_tcp_seq_translate_device): one lane
// per frame, the frame's first eight aligned chunks in the lane's LDS slot
// and the receive transform's parse, as rx_mss_kernel.  The ops of the
// frame's translation are then applied to the TCP header where it lies in
// LDS -- in the slot itself when the whole header [t, t + end) is in the
// image, else in a copy gathered at the slot's start through the FrameView
// rare path (IPv6 extension chains, IHL 15 behind a VLAN tag) -- with the
// checksum carried in a register through the kept functions' exact sequence
// of ip_update_cksum16/32 steps (include/ipcksum.h: steps that leave the
// value alone are kept too, they can turn 0xffff into 0).  A frame changes
// up to ~50 bytes (seq, ack, checksum, four SACK blocks, the timestamps), so
// the patched image goes back through write_back, as the rewrite's does,
// with the changed bytes kept as a mask over the header's 60 bytes instead
// of the slot's 128.
struct SeqPatch {
  LDS_AS uint8_t *h;     // TCP header bytes [0, end) in LDS
  int end;
  uint32_t ck;
  uint64_t touched = 0;  // header byte positions written

  // a byte past the options is taken as 0: it only ever is the far half of
  // a straddling checksum word, where it cancels (and is never written)
  __device__ __forceinline__ uint32_t u8(int k) const { return k < end ? (uint32_t)h[k] : 0u; }
  __device__ __forceinline__ uint32_t be16(int k) const { return (u8(k) << 8) | u8(k + 1); }
  __device__ __forceinline__ uint32_t be32(int k) const { return (be16(k) << 16) | be16(k + 2); }
  __device__ __forceinline__ void put(int k, uint32_t v, int nbytes) {
    for (int b = 0; b < nbytes; ++b) {
      h[k + b] = (uint8_t)(v >> (8 * (nbytes - 1 - b)));
      touched |= 1ull << (k + b);
    }
  }
  // tcp_set_seq/ack_number_cksum_update (ipcksum.h): fields at offsets 4, 8
  __device__ __forceinline__ void add_aligned32(int k, uint32_t add) {
    const uint32_t o = be32(k), nw = o + add;
    ck = upd32(ck, o, nw);
    put(k, nw, 4);
  }
  // pptk_tcp_adjust_ts32: a 32-bit field at any offset; at an odd one the
  // three words that straddle it, old values read before the write
  __device__ __forceinline__ void add_ts32(int f, uint32_t add) {
    const uint32_t o = be32(f), nw = o + add;
    if (!(f & 1)) {
      ck = upd32(ck, o, nw);
    } else {
      const uint32_t x0 = u8(f - 1), x1 = u8(f + 4);
      ck = upd16(ck, (x0 << 8) | (o >> 24), (x0 << 8) | (nw >> 24));
      ck = upd16(ck, (o >> 8) & 0xffffu, (nw >> 8) & 0xffffu);
      ck = upd16(ck, ((o & 0xffu) << 8) | x1, ((nw & 0xffu) << 8) | x1);
    }
    put(f, nw, 4);
  }
  // tcp_adjust_sack_cksum_update: every 8-byte block from option offset 2,
  // each adjusted once (at most 4: sacklen <= 40)
  __device__ __forceinline__ void adjust_sack(int so, int sl, uint32_t add) {
    for (int k = 2; k + 8 <= sl; k += 8) {
      const int p = so + k;
      const uint32_t s0 = be32(p), e0 = be32(p + 4), s1 = s0 + add, e1 = e0 + add;
      if (!(so & 1)) {
        ck = upd32(ck, s0, s1);
        ck = upd32(ck, e0, e1);
      } else {
        const uint32_t x0 = u8(p - 1), x1 = u8(p + 8);
        ck = upd16(ck, (x0 << 8) | (s0 >> 24), (x0 << 8) | (s1 >> 24));
        ck = upd32(ck, (s0 << 8) | (e0 >> 24), (s1 << 8) | (e1 >> 24));
        ck = upd32(ck, (e0 << 8) | x1, (e1 << 8) | x1);
      }
      put(p, s1, 4);
      put(p + 4, e1, 4);
    }
  }
  // tcp_disable_sack_cksum_update: NOPs pair by pair (at most 20 pairs); an
  // odd last byte shares its word with the byte behind the option, which
  // stays
  __device__ __forceinline__ void disable_sack(int so, int sl) {
    for (int k = 0; k + 1 <= sl; k += 2) {
      const bool whole = k + 2 <= sl;
      const int p = so + k;
      const uint32_t o = be16(p);
      const uint32_t nw = whole ? 0x0101u : ((o & 0xffu) | 0x0100u);
      if (!(so & 1)) {
        ck = upd16(ck, o, nw);
      } else {
        const uint32_t x0 = u8(p - 1), x1 = u8(p + 2);
        ck = upd16(ck, (x0 << 8) | (o >> 8), (x0 << 8) | (nw >> 8));
        ck = upd16(ck, ((o & 0xffu) << 8) | x1, ((nw & 0xffu) << 8) | x1);
      }
      put(p, nw >> (whole ? 0 : 8), whole ? 2 : 1);
      if (!whole) break;
    }
  }
};

constexpr int SEQ_SLOT = 128;

__global__ __launch_bounds__(256) void rx_seq_kernel(SeqKArgs a) {
  LDS_AS uint8_t *slot = lane_slot<SEQ_SLOT>();
  const uint64_t step = (uint64_t)gridDim.x * 256u;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < a.b.fb.n; i += step) {
    const uint64_t j = a.idx ? (uint64_t)a.idx[i] : (a.xl_one ? 0u : i);
    if (j >= a.xl_count) {   // no flow: the frame is not even read
      if (a.b.status) a.b.status[i] = (uint8_t)PPTK_SEQ_ST_NOFLOW;
      continue;
    }
    const LaneFrame fr = load_frame<SEQ_SLOT>(a.b, i, slot);
    const uint64_t base = fr.base;
    const uint32_t len = fr.len;
    const int m = fr.m;
    const FrameView &v = fr.v;
    const Parse p = parse_frame(v, len);
    uint32_t st = 0;
    if ((p.flags & (PPTK_RX_F_PARSED | PPTK_RX_F_MALFORMED | PPTK_RX_F_L4)) ==
            (PPTK_RX_F_PARSED | PPTK_RX_F_L4) &&
        p.proto == 6) {
      const int t = (int)p.rs;   // TCP header
      const int end = (int)(v.u8(t + 12) >> 4) * 4;   // tcp_data_offset
      if (end < 20 || t + end > (int)p.re) {
        st = PPTK_SEQ_ST_BADOPT;
      } else {
        st = PPTK_SEQ_ST_TCP;
        const pptk_seqxlate x = a.xl[j];
        const bool fast = m + t + end <= SEQ_SLOT;
        if (!fast) {
          // gather the header at the slot's start: byte k comes from image
          // position m + t + k > k or from global memory, so the ascending
          // copy never overwrites a byte it has yet to read
          for (int k = 0; k < end; ++k) slot[k] = (uint8_t)v.u8(t + k);
        }
        SeqPatch s{fast ? slot + m + t : slot, end, 0u};
        const uint32_t ck0 = s.be16(16);
        s.ck = ck0;
        if (x.ops & PPTK_SEQ_SEQ) {
          s.add_aligned32(4, x.seq_add);
          st |= PPTK_SEQ_ST_SEQ;
        }
        if ((x.ops & PPTK_SEQ_ACK) && (s.u8(13) & 0x10u)) {
          s.add_aligned32(8, x.ack_add);
          st |= PPTK_SEQ_ST_ACK;
        }
        if (x.ops & (PPTK_SEQ_SACK | PPTK_SEQ_TSVAL | PPTK_SEQ_TSECHO | PPTK_SEQ_SACK_OFF)) {
          // tcp_find_sack_ts_headers (last SACK, last 10-byte timestamp) and
          // tcp_find_sack_header (first SACK) in one pass: the two walks step
          // through the same offsets until the second one ends -- at the
          // first SACK option, or where a timestamp option has a length
          // below 2, which only the first walk steps over (`first_done`);
          // kind 0, and any other kind with a length below 2, end both.
          // The offset grows by at least 1 per step from 20 to at most 60:
          // 40 steps bound the loop whatever the bytes are.  No op writes a
          // byte a walk reads (kinds and lengths stay), so walking once
          // before the ops equals the kept functions' walks between them.
          int off = 20, sackoff = 0, sacklen = 0, tsoff = 0, first = 0, firstlen = 0;
          bool first_done = false;
          for (int n = 0; n < 40 && off < end; ++n) {
            const uint32_t kind = s.u8(off);
            if (kind == 0) break;
            if (kind == 1) {
              off++;
              continue;
            }
            const int left = end - off;
            const int lb = (int)s.u8(off + 1);
            const int L = (off + 1 < end && lb < left) ? lb : left;
            if (kind == 5) {
              sackoff = off;
              sacklen = L;
              if (!first_done) {
                first = off;
                firstlen = L;
                first_done = true;
              }
            } else if (kind == 8) {
              if (L == 10) tsoff = off;
              if (L < 2) first_done = true;
            } else if (L < 2) {
              break;
            }
            if (L == 0) break;
            off += L;
          }
          if ((x.ops & PPTK_SEQ_SACK) && sackoff) {
            s.adjust_sack(sackoff, sacklen, x.sack_add);
            st |= PPTK_SEQ_ST_SACK;
          }
          if (tsoff) {
            if (x.ops & PPTK_SEQ_TSVAL) s.add_ts32(tsoff + 2, x.tsval_add);
            if (x.ops & PPTK_SEQ_TSECHO) s.add_ts32(tsoff + 6, x.tsecho_add);
            if (x.ops & (PPTK_SEQ_TSVAL | PPTK_SEQ_TSECHO)) st |= PPTK_SEQ_ST_TS;
          }
          if ((x.ops & PPTK_SEQ_SACK_OFF) && first) {
            s.disable_sack(first, firstlen);
            st |= PPTK_SEQ_ST_SACK_OFF;
          }
        }
        if (s.ck != ck0) s.put(16, s.ck, 2);
        if (s.touched) {
          GLB_AS uint8_t *fw = (GLB_AS uint8_t *)a.b.frames_w + base;
          if (fast) {
            const int hp = m + t;   // the header's place in the slot
#pragma unroll
            for (int c = 0; c < SEQ_SLOT / 16; ++c) {
              // the changed bytes of chunk c: header bytes [16c - hp, +16)
              const int lo = 16 * c - hp;
              const uint32_t tb = lo >= 64 || lo <= -16 ? 0u
                                  : (uint32_t)(lo >= 0 ? s.touched >> lo : s.touched << -lo) & 0xffffu;
              write_back(slot, fw - m, c, m, len, tb);
            }
          } else {
            uint64_t tb = s.touched;   // bits below `end` only: inside the frame
            while (tb) {
              const int b = __builtin_ctzll(tb);
              fw[t + b] = slot[b];
              tb &= tb - 1;
            }
          }
        }
      }
    }
    if (a.b.status) a.b.status[i] = (uint8_t)st;
  }
}

}  // namespace

// Two-pass tx, second pass: one thread per frame writes the (at most two)
// checksum fields the streaming pass left in txside -- the only writes of
// the operation, issued without a read stream beside them.
__global__ __launch_bounds__(256) void tx_apply_kernel(const uint64_t *__restrict__ side,
                                                       uint8_t *__restrict__ frames,
                                                       const uint64_t *__restrict__ off,
                                                       uint64_t stride, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t e = side[i];
    const uint64_t base = off ? off[i] : i * stride;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const uint32_t f = (uint32_t)(e >> (32 * k));
      const uint32_t o = f & 0xffffu;
      if (o == 0xffffu) continue;
      uint8_t *p = frames + base + o;
      if (((uintptr_t)p & 1u) == 0) {
        *(uint16_t *)p = (uint16_t)bswap16(f >> 16);   // network order
      } else {
        p[0] = (uint8_t)(f >> 24);
        p[1] = (uint8_t)(f >> 16);
      }
    }
  }
}

hipError_t launch_tx_apply(const uint64_t *txside, uint8_t *frames, const uint64_t *off,
                           uint64_t stride, uint64_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const uint64_t blocks = std::min<uint64_t>((n + 255) / 256, 8192);
  hipLaunchKernelGGL(tx_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, s, txside, frames,
                     off, stride, n);
  return hipGetLastError();
}

hipError_t launch_rewrite(const RewriteKArgs &a, int grid, hipStream_t s) {
  hipLaunchKernelGGL(rx_rewrite_kernel, dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_mss_clamp(const MssKArgs &a, int grid, hipStream_t s) {
  hipLaunchKernelGGL(rx_mss_kernel, dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_seq_translate(const SeqKArgs &a, int grid, hipStream_t s) {
  hipLaunchKernelGGL(rx_seq_kernel, dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace pptk
