/*
 * pptk_rx.h -- C-ABI of the MI355X batch receive transform.
 *
 * One call turns a batch of Ethernet frames into one 64-byte record per
 * frame: IPv4 header checksum, TCP/UDP (v4/v6) checksum, fixed-format
 * L2/L3/L4 field extraction and a SipHash-2-4 flow hash of the 5-tuple.
 *
 * Where it plugs in: between ldp_in_nextpkts() and ldp_in_deallocate_some()
 * of an LDP rx loop (reference ldp/ldprecv.c:60-70, ldp/ldprecvmt.c:54-64,
 * ldp/ldpfwdmt.c:72-89).  The reference has no batch entry point: its rx
 * loops call the per-packet primitives below, one packet at a time:
 *   ip_hdr_cksum_calc      iphdr/ipcksum.c:39-49
 *   tcp_cksum_calc         iphdr/ipcksum.c:51-68
 *   tcp6_cksum_calc        iphdr/ipcksum.c:74-115
 *   udp_cksum_calc         iphdr/ipcksum.c:117-134
 *   udp6_cksum_calc        iphdr/ipcksum.c:140-181
 *   ipv6_const_proto_hdr_2 iphdr/iphdr.h:804-860
 *   siphash_buf            misc/siphash.h:214-229
 *   ip_permitted hashing   iphash/iphash.c:157-162 (v4), :108-120 (v6)
 * pptk_rx_batch() replaces that per-packet loop; its record carries exactly
 * the values those functions return for the same frame.
 *
 * Plain C types only: no HIP, torch or RCCL types appear in signatures.
 * Every function returns 0 or a negative errno (-EINVAL, -ENOMEM, -EIO for
 * HIP/RCCL failures; the multi-GPU calls also -ETIMEDOUT, -ECANCELED and
 * -ENOSYS, see there).  Nothing aborts on packet content: per-packet problems
 * are reported in pptk_rx_rec.flags.
 */
#ifndef PPTK_RX_H
#define PPTK_RX_H

#include <stddef.h>
#include <stdint.h>

#include "ldp_packet.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- per-packet record (64 bytes, one per frame, written at the frame's
 * index).  Multi-byte integers are host (little-endian) order unless noted. */
struct pptk_rx_rec {
  uint64_t flow_hash;  /*  0 siphash_buf(key, tuple, 40); 0 if !PARSED      */
  uint8_t src[16];     /*  8 network-order address; IPv4 uses bytes 0..3    */
  uint8_t dst[16];     /* 24 idem                                           */
  uint16_t sport;      /* 40 host order (tcp_src_port / udp_src_port)       */
  uint16_t dport;      /* 42                                                */
  uint16_t ip_cksum;   /* 44 ip_hdr_cksum_calc(ip, ihl); 0 == valid; 0 v6   */
  uint16_t l4_cksum;   /* 46 tcp/udp(6)_cksum_calc(...); 0 == valid         */
  uint16_t l4_off;     /* 48 frame offset of the L4 header                  */
  uint16_t l4_len;     /* 50 L4 length = ip_total_len - ihl (v6: tlen - off)*/
  uint8_t l3_off;      /* 52 14, or 18 behind an 802.1Q tag                 */
  uint8_t proto;       /* 53 ip_proto / final IPv6 next header              */
  uint16_t flags;      /* 54 PPTK_RX_F_*                                    */
  uint32_t src_bucket; /* 56 ip_permitted/ipv6_permitted bucket, 0 if off   */
  uint16_t ethertype;  /* 60 (inner) ethertype, host order                  */
  uint8_t ip_version;  /* 62 version nibble of the L3 header (0 if none)    */
  uint8_t reserved;    /* 63 always 0                                       */
};

/* ---- compact record (32 bytes): the same values minus the raw checksum
 * words, ethertype, version and the IPv6 addresses (IPv6 frames carry 0 in
 * src4/dst4; the addresses are at frame + l3_off + 8 / + 24).  Written
 * instead of pptk_rx_rec when pptk_rx_dev_batch.d_recs32 is set: half the
 * record bytes, which is what bounds small frames. */
struct pptk_rx_rec32 {
  uint64_t flow_hash;  /*  0 as pptk_rx_rec.flow_hash                       */
  uint32_t src4;       /*  8 IPv4 source, network byte order; 0 for IPv6    */
  uint32_t dst4;       /* 12 IPv4 destination; 0 for IPv6                   */
  uint16_t sport;      /* 16 host order                                     */
  uint16_t dport;      /* 18                                                */
  uint16_t flags;      /* 20 PPTK_RX_F_*                                    */
  uint8_t proto;       /* 22                                                */
  uint8_t l3_off;      /* 23                                                */
  uint16_t l4_off;     /* 24                                                */
  uint16_t l4_len;     /* 26                                                */
  uint32_t src_bucket; /* 28                                                */
};

/* ---- fragment side record (16 bytes, one per frame, written at the
 * frame's index when pptk_rx_dev_batch.d_frag is set): what an IP
 * reassembler needs -- reference ipfrag/ipreass.c:118-124 and
 * ipfrag/rfc815.c:145-151 key on ip_frag_off, ip_more_frags, ip_total_len
 * and ip_hdr_len -- so fragments can be handed on without parsing the frame
 * a second time.  All zero for frames that are not PARSED, are MALFORMED,
 * or are IPv6 without a fragment header.  Fields are host order. */
struct pptk_rx_frag {
  uint32_t ident;        /*  0 IPv4 ip_id (iphdr/iphdr.h:1093-1097); IPv6 the
                                fragment header's 32-bit Identification     */
  uint16_t frag_off;     /*  4 data offset in bytes: ip_frag_off (:1124-1128)
                                / ipv6_frag_off (:727-731)                  */
  uint16_t data_len;     /*  6 fragment data bytes: IPv4 ip_total_len - ihl;
                                IPv6 40 + payload_len - (frag_hdr_off + 8)  */
  uint16_t frag_hdr_off; /*  8 IPv6: *frag_hdr_off_ptr of
                                ipv6_const_proto_hdr_2 (:804-860), counted
                                from the IPv6 header (the last fragment
                                header of the chain); IPv4: 0               */
  uint16_t proto_hdr_off_from_frag; /* 10 IPv6: its *proto_hdr_off_from_frag
                                (0 for a non-first fragment); IPv4: 0       */
  uint8_t next_hdr;      /* 12 IPv4 ip_proto; IPv6 the fragment header's
                                Next Header byte                            */
  uint8_t flags;         /* 13 PPTK_RX_FRAG_*                               */
  uint16_t reserved;     /* 14 always 0                                     */
};

#define PPTK_RX_FRAG_IS 0x01u   /* a fragment: PPTK_RX_F_FRAGMENT            */
#define PPTK_RX_FRAG_MF 0x02u   /* ip_more_frags (:1023-1027) /
                                   ipv6_more_frags (:733-737)               */
#define PPTK_RX_FRAG_DF 0x04u   /* ip_dont_frag (:1040-1044), IPv4 only      */
#define PPTK_RX_FRAG_V6 0x08u   /* fields taken from an IPv6 fragment header */

#define PPTK_RX_F_PARSED 0x0001u      /* IPv4/IPv6 header parsed            */
#define PPTK_RX_F_IP_OK 0x0002u       /* ip_cksum == 0 (always for IPv6)    */
#define PPTK_RX_F_L4_OK 0x0004u       /* L4 present and l4_cksum == 0       */
#define PPTK_RX_F_L4 0x0008u          /* TCP/UDP header present             */
#define PPTK_RX_F_IPV6 0x0010u        /* L3 is IPv6                         */
#define PPTK_RX_F_VLAN 0x0020u        /* one 802.1Q tag was skipped         */
#define PPTK_RX_F_FRAGMENT 0x0040u    /* IPv4 MF/offset or IPv6 frag header */
#define PPTK_RX_F_UDP_ZERO 0x0080u    /* UDP checksum field transmitted 0   */
#define PPTK_RX_F_MALFORMED 0x0100u   /* lengths/IHL/ext chain inconsistent */
#define PPTK_RX_F_V6_EXT 0x0200u      /* IPv6 extension headers walked      */

/* ---- context ------------------------------------------------------------ */
struct pptk_rx_ctx;

struct pptk_rx_opts {
  int device;           /* HIP device ordinal                              */
  uint8_t key[16];      /* SipHash key (hash_seed in the reference)        */
  uint8_t iphash_bits4; /* ip_permitted prefix bits, 1..32; 0 = no bucket  */
  uint8_t iphash_bits6; /* ipv6_permitted prefix bits, 1..128; 0 = off     */
  uint16_t gather_threads; /* host threads gathering staged frames (0 = 1) */
  uint32_t iphash_size; /* struct ip_hash.hash_size (power of two)         */
  uint32_t max_batch;   /* pptk_rx_batch chunk (frames per staged transfer) */
  uint32_t max_frame;   /* largest frame accepted by pptk_rx_batch (<=65535)*/
  uint32_t comm_timeout_ms; /* bound on every multi-GPU wait (communicator
                           creation, a gather's enqueue, pptk_rx_comm_sync,
                           teardown); 0 = PPTK_RX_COMM_TIMEOUT_MS          */
};

#define PPTK_RX_COMM_TIMEOUT_MS 60000u

void pptk_rx_opts_default(struct pptk_rx_opts *opts);

int pptk_rx_ctx_create(struct pptk_rx_ctx **ctx, const struct pptk_rx_opts *opts);
void pptk_rx_ctx_destroy(struct pptk_rx_ctx *ctx);

/* Host in -> host out.  Gathers the borrowed ldp_packet frames into pinned
 * staging (or reads them in place from a registered ring, see below), copies
 * them to HBM, runs the transform and copies the records back, in chunks of
 * opts.max_batch frames, up to four in flight on their own streams (each
 * with its own staging, allocated when a call first has that many chunks);
 * synchronous: on
 * return recs[0..num) are final and no pointer in pkts is retained.
 * ancillary fields are neither read nor written.  Frames longer than
 * opts.max_frame get PPTK_RX_F_MALFORMED only. */
int pptk_rx_batch(struct pptk_rx_ctx *ctx, const struct ldp_packet *pkts,
                  int num, struct pptk_rx_rec *recs);

/* The same with compact 32-byte records (struct pptk_rx_rec32, the values
 * of pptk_rx_rec minus the raw checksum words, ethertype, version and the
 * IPv6 addresses): half the record bytes back over PCIe, which is what
 * bounds small frames host to host (a 64-byte frame's 64-byte record moves
 * as many bytes up as the frame moved down).  Same rules as pptk_rx_batch,
 * including records written in place into a registered region. */
int pptk_rx_batch32(struct pptk_rx_ctx *ctx, const struct ldp_packet *pkts,
                    int num, struct pptk_rx_rec32 *recs);

/* pptk_rx_batch split in two, so that an rx loop overlaps one batch's GPU
 * round trip with fetching and submitting the next (the synchronous call
 * leaves the host idle for the whole launch-to-completion latency, which
 * dominates LDP-sized batches; DESIGN.md "Pipelined host batches"):
 *
 *   ldp_in_nextpkts(q, pkts[k], ...);  pptk_rx_batch_submit(ctx, pkts[k], n, recs[k]);
 *   if (pptk_rx_batch_pending(ctx) == DEPTH) {   -- DEPTH <= PPTK_RX_MAX_INFLIGHT
 *     pptk_rx_batch_complete(ctx);      -- batch k-DEPTH+1: recs final, frames free
 *     ... use its recs ...;  ldp_in_deallocate_some(q, its pkts, ...);
 *   }
 *
 * submit gathers and enqueues one batch of 1..opts.max_batch frames (one
 * chunk) and returns without waiting; the frames and recs[0, num) must stay
 * valid and untouched until the batch is completed.  complete waits for the
 * OLDEST outstanding submission (FIFO) and returns its frame count (> 0):
 * after it its records are final and none of its pointers is retained.
 * Results are those of pptk_rx_batch.  At most PPTK_RX_MAX_INFLIGHT
 * submissions are outstanding per context (submit returns -EBUSY beyond;
 * each depth in use keeps its own staging buffers, allocated on first use);
 * pptk_rx_batch returns -EBUSY while any is; num == 0 submits nothing and
 * returns 0; num > opts.max_batch is -EINVAL (use pptk_rx_batch);
 * complete with nothing outstanding returns -ENOENT.  A failed submit
 * leaves nothing outstanding.  pptk_rx_ctx_destroy waits for (and drops)
 * outstanding submissions. */
#define PPTK_RX_MAX_INFLIGHT 4
int pptk_rx_batch_submit(struct pptk_rx_ctx *ctx, const struct ldp_packet *pkts, int num,
                         struct pptk_rx_rec *recs);
/* pptk_rx_batch_submit with compact records (as pptk_rx_batch32); completed
 * by pptk_rx_batch_complete like any other submission. */
int pptk_rx_batch_submit32(struct pptk_rx_ctx *ctx, const struct ldp_packet *pkts, int num,
                           struct pptk_rx_rec32 *recs);
int pptk_rx_batch_complete(struct pptk_rx_ctx *ctx);
int pptk_rx_batch_pending(const struct pptk_rx_ctx *ctx);

/* Zero-copy rx rings: register a host region (e.g. a netmap ring's buffer
 * area or a socket ring) once; pptk_rx_batch() calls whose frames all lie in
 * one registered ring skip the host gather into staging: a chunk whose
 * frames fill >= 80 % of the ring span they cover (and that span > 2 MiB)
 * is copied down by DMA as one span, any other chunk is read by the GPU in
 * place over PCIe (PPTK_RX_RING_DMA_PCT sets the fraction).  Every frame's
 * end rounded up to 16 bytes must lie inside the region.  A registered
 * region that holds a call's whole record array (recs[0, num)) receives the
 * records in place: the kernel writes them there over PCIe and the host
 * copies nothing back -- register the rx loop's record array once.
 * Unregister before freeing the memory. */
int pptk_rx_register_ring(struct pptk_rx_ctx *ctx, void *base, size_t bytes);
int pptk_rx_unregister_ring(struct pptk_rx_ctx *ctx, void *base);

/* Device-resident batch (asynchronous on `stream`, a hipStream_t or NULL).
 * Frame i starts at d_frames + (d_off ? d_off[i] : i * stride) and is
 * (d_len ? d_len[i] : fixed_len) bytes long.  d_perm (nullable) gives the
 * processing order (a permutation of 0..n-1, e.g. from
 * pptk_rx_bin_device); records always land at d_recs[i] (or d_recs32[i]
 * when that is set: compact records, d_recs unused) for frame i.
 * d_hash (nullable) additionally receives flow_hash[i] as a dense u64 array,
 * the send buffer of the multi-GPU all-gather; d_frag (nullable) receives
 * the fragment side record of every frame (struct pptk_rx_frag).
 * The frame buffer must stay readable up to the next 16-byte boundary past
 * the last frame (any hipMalloc allocation is); the 16-byte chunk holding
 * the start of an empty (0-byte) frame is read too.  The kernels of every
 * device entry point that takes this layout (this one, pptk_tx_cksum_device,
 * pptk_tx_rewrite_device, pptk_tcp_mss_clamp_device) lay their 16-byte
 * chunks out from d_frames, not from address 0: the boundary meant is the
 * next multiple of 16 bytes counted from d_frames, which for a d_frames
 * that is not itself 16-byte aligned lies up to 15 bytes past the next
 * aligned address (a d_frames inside a hipMalloc allocation with 16 bytes
 * of slack behind the last frame is always fine). */
struct pptk_rx_dev_batch {
  const uint8_t *d_frames;
  const uint64_t *d_off;  /* nullable: fixed stride                       */
  const uint16_t *d_len;  /* nullable: fixed_len                          */
  const uint32_t *d_perm; /* nullable: identity order                     */
  uint64_t stride;
  uint32_t fixed_len;
  uint32_t max_len;       /* upper bound of frame lengths (tuning only)   */
  uint64_t n;
  struct pptk_rx_rec *d_recs;     /* nullable when d_recs32 is set     */
  uint64_t *d_hash;       /* nullable                                     */
  struct pptk_rx_rec32 *d_recs32; /* nullable: compact records instead */
  struct pptk_rx_frag *d_frag;    /* nullable: fragment side records    */
  uint32_t *d_key;        /* nullable: dense rate-limiter key per frame:
                             src_bucket of a PARSED IPv4 frame, src_bucket |
                             0x80000000 of a PARSED IPv6 frame, 0xffffffff
                             otherwise (pptk_rx_permit_keys_device)      */
};

int pptk_rx_batch_device(struct pptk_rx_ctx *ctx,
                         const struct pptk_rx_dev_batch *b, void *stream);

/* Length binning for mixed-size batches: writes into d_perm a stable
 * permutation of 0..n-1 ordered by length group (the groups of
 * pptk_rx_batch_device_mixed), so the lanes of one wavefront sum frames of
 * similar length.  d_scratch must hold
 * pptk_rx_bin_scratch_bytes(n) bytes.  Asynchronous on `stream`. */
size_t pptk_rx_bin_scratch_bytes(uint64_t n);
int pptk_rx_bin_device(struct pptk_rx_ctx *ctx, const uint16_t *d_len,
                       uint64_t n, uint32_t *d_perm, void *d_scratch,
                       void *stream);

/* Mixed-size batch in one call.  Length binning pays on MI355X only when a
 * batch mixes jumbo frames (> 1521 bytes, which batch order would stream
 * with the 64-lane jumbo shape) with shorter ones; every split of 64..1521 B
 * frames into groups measured slower than batch order (DESIGN.md "Binned
 * order").  So: with b->max_len (a hint) at most 1521 the call runs the
 * batch in batch order, as pptk_rx_batch_device; otherwise a device pass
 * counts the length groups (..113, ..1521 bytes, longer) and, when the
 * batch holds frames of the last group and shorter ones, bins it
 * (pptk_rx_bin_device into the permutation) and runs one launch per group,
 * each streamed by the kernel shape sized for it; else batch order by the
 * launch of the highest non-empty group.  Results are identical either way.
 * Requires d_len; b->d_perm is ignored.  d_perm (nullable) receives the
 * processing order: the binned permutation, or the identity.  d_scratch:
 * pptk_rx_bin_scratch_bytes(n) bytes (counters, group table, the binned
 * descriptors the group launches stream, and the permutation when d_perm
 * is NULL); both stay in use until the stream reaches the end of the call.
 * Records land at d_recs[i] for frame i. */
int pptk_rx_batch_device_mixed(struct pptk_rx_ctx *ctx,
                               const struct pptk_rx_dev_batch *b, uint32_t *d_perm,
                               void *d_scratch, void *stream);

/* Batched rate limiting: ip_permitted / ipv6_permitted (reference
 * iphash/iphash.c:108-197) for a device batch, with the result the
 * reference gives when called once per frame in frame order.  The subject
 * frames are the PARSED frames of `family` (4 or 6; the context must have
 * that family's iphash_bits set, so the records carry its bucket) for which
 * d_subject[i] != 0 (d_subject nullable = all of them).  d_tokens holds
 * opts.iphash_size u32 counters (the entries of struct ip_hash, widened to
 * u32); verdict[i] = 1 permitted (a token was consumed), 0 denied, 2 not a
 * subject.  Reads one of d_recs / d_recs32 (the other NULL).  d_scratch:
 * pptk_rx_permit_scratch_bytes(n, opts.iphash_size) bytes.  Asynchronous. */
size_t pptk_rx_permit_scratch_bytes(uint64_t n, uint32_t hash_size);
int pptk_rx_permit_device(struct pptk_rx_ctx *ctx, const struct pptk_rx_rec *d_recs,
                          const struct pptk_rx_rec32 *d_recs32, uint64_t n, int family,
                          const uint8_t *d_subject, uint32_t *d_tokens,
                          uint8_t *d_verdict, void *d_scratch, void *stream);

/* The same from the dense keys the receive transform wrote into
 * pptk_rx_dev_batch.d_key (4 bytes per frame instead of a 16-byte slice of
 * each record).  Results are those of pptk_rx_permit_device on the
 * records of the same batch; same scratch size.  A key whose bucket (bits
 * 0..30) is >= opts.iphash_size -- only caller-made keys can be -- is not a
 * subject (verdict 2, no token touched).  Up to 2^16 buckets and 16 M
 * frames (65 536 per CU) this runs as one persistent launch that reads the
 * keys once (DESIGN.md section 5 "Rate limiter"); beyond, or with
 * PPTK_RX_TUNE_PERMIT_PASSES set (pptk_rx_set_tuning, or the PPTK_RX_TUNE
 * environment word), as four launches.  The persistent launch needs all its
 * workgroups resident at once: the library orders every such launch of a
 * device behind the previous one, whatever stream or context issued it, so
 * concurrent calls never starve each other; calls that share one scratch
 * buffer must still be ordered on one stream.  Should the workgroups not
 * all become resident within 2 s (e.g. another process's kernels hold the
 * CUs), the launch aborts and fails closed: every subject frame's verdict
 * is 0 (denied, as the reference denies a frame it has no token for), the
 * others 2, the token counts are left as they were before the call (nothing
 * half-updated: all workgroups act on one commit-or-abort decision), and
 * pptk_rx_permit_status reports -ETIMEDOUT; never a hang.  The scratch
 * needs no initialisation. */
int pptk_rx_permit_keys_device(struct pptk_rx_ctx *ctx, const uint32_t *d_keys, uint64_t n,
                               int family, const uint8_t *d_subject, uint32_t *d_tokens,
                               uint8_t *d_verdict, void *d_scratch, void *stream);

/* Whether every pptk_rx_permit_keys_device call on d_scratch since the last
 * status query completed: 0, or -ETIMEDOUT if one aborted (its subject
 * frames were denied and its tokens left unchanged: repeat it, e.g. with
 * PPTK_RX_TUNE_PERMIT_PASSES, to get the verdicts the tokens allow).
 * Synchronises `stream` (the stream those calls ran on).  -EIO on a HIP
 * error.  The library tracks up to 1024 scratch buffers; a buffer not
 * queried while 1024 others were used since reports 0. */
int pptk_rx_permit_status(struct pptk_rx_ctx *ctx, const void *d_scratch, void *stream);

/* The token refill timer (batch_timer_fn, reference iphash/iphash.c:
 * 290-350) for buckets [start, end): tokens = min(tokens + add, initial).
 * Asynchronous; order it with pptk_rx_permit_device on one stream. */
int pptk_rx_tokens_refill_device(struct pptk_rx_ctx *ctx, uint32_t *d_tokens,
                                 uint32_t start, uint32_t end, uint32_t add,
                                 uint32_t initial_tokens, void *stream);

/* Tx side (reference iphdr/ipcksum.h:101-211, callers ldp/ldpsend.c:
 * 162-167): set, in place, the checksums of every frame of a device batch as
 * ip46_set_hdr_cksum_calc + tcp/udp(6)_set_cksum_calc would -- the IPv4
 * header checksum of every parsed IPv4 frame, the TCP/UDP checksum of every
 * frame with an L4 header (PPTK_RX_F_L4: not a fragment, long enough),
 * located exactly as pptk_rx_batch_device parses.  Frames the receive
 * transform would not parse are left untouched.  After it, the receive
 * transform verifies every such frame (IP_OK / L4_OK).  Layout arguments as
 * in pptk_rx_dev_batch; max_len is a tuning hint.  Asynchronous.
 * Fixed-stride batches run in two passes (checksums into a side array of 8
 * bytes per frame, then the field writes).  The side array is allocated and
 * freed on `stream` from a stream-ordered pool the context owns, so tx calls
 * of one context may run concurrently on different streams. */
int pptk_tx_cksum_device(struct pptk_rx_ctx *ctx, uint8_t *d_frames, const uint64_t *d_off,
                         const uint16_t *d_len, uint64_t stride, uint32_t fixed_len,
                         uint64_t n, uint32_t max_len, void *stream);

/* The two-pass side array from the caller: `frames` * 8 bytes of device
 * memory (8-byte aligned) that the context uses instead of its pool, e.g. a
 * buffer placed like a record ring (its writes beside the frame reads cost
 * what record writes cost: pptk_rx_place_records).  Every tx call of the
 * context that fits uses this ONE buffer: such calls must not overlap (use
 * one stream, or order the streams).  The buffer must stay valid until the
 * context is destroyed or another buffer (or NULL: back to the pool) is
 * set; batches larger than `frames` use the pool. */
int pptk_tx_set_side_buffer(struct pptk_rx_ctx *ctx, void *d_side, uint64_t frames);

/* Header rewrite with incremental checksum update (NAT / forwarding),
 * reference iphdr/ipcksum.h:213-393: per frame, in this order,
 *   PPTK_RW_DECR_TTL  ip_decr_ttl_cksum_update          (:374-393)
 *   PPTK_RW_SRC       ip_set_src_cksum_update(src)      (:238-261)
 *   PPTK_RW_DST       ip_set_dst_cksum_update(dst)      (:349-372)
 *   PPTK_RW_SPORT     tcp/udp_set_src_port_cksum_update (:263-271, :323-334)
 *   PPTK_RW_DPORT     tcp/udp_set_dst_port_cksum_update (:273-281, :336-347)
 *   PPTK_RW_ICMP_ID   icmp_set_echo_identifier_cksum_update (:283-291), with
 *                     the new identifier in `sport`
 * each computing the new checksum from the old one with ip_update_cksum16/32
 * (:213-236), results identical to calling those functions in that order.
 * Applies to every frame the receive transform parses as IPv4; the TCP/UDP
 * parts (the L4 checksum follow-up of an address change, the port writes)
 * only when its record has PPTK_RX_F_L4 (an L4 header, not a fragment), and
 * a UDP checksum of 0 stays 0 as in the reference; the ICMP identifier
 * only on an echo request or reply (type 8 / 0) that is not a fragment and
 * has its 8-byte header inside the packet.  A frame whose TTL is 0
 * under PPTK_RW_DECR_TTL (the reference abort()s) is left untouched.
 * Addresses and ports are host order, as the reference's setters take them.
 * d_rw holds rw_count = 1 (one rewrite for every frame) or n entries.
 * d_status (nullable) receives per frame PPTK_RW_ST_* bits.  Layout
 * arguments as in pptk_tx_cksum_device.  Asynchronous on `stream`. */
struct pptk_rewrite {
  uint32_t ops;    /* PPTK_RW_* */
  uint32_t src;    /* new IPv4 source (host order) */
  uint32_t dst;    /* new IPv4 destination (host order) */
  uint16_t sport;  /* new TCP/UDP source port (host order) */
  uint16_t dport;  /* new TCP/UDP destination port (host order) */
};
#define PPTK_RW_DECR_TTL 0x1u
#define PPTK_RW_SRC 0x2u
#define PPTK_RW_DST 0x4u
#define PPTK_RW_SPORT 0x8u
#define PPTK_RW_DPORT 0x10u
#define PPTK_RW_ICMP_ID 0x20u
#define PPTK_RW_ST_IP 0x1u         /* parsed IPv4: the IP-level ops applied */
#define PPTK_RW_ST_L4 0x2u         /* L4 header present: the L4 ops applied */
#define PPTK_RW_ST_TTL_ZERO 0x4u   /* TTL was 0: frame left untouched      */
#define PPTK_RW_ST_EXPIRED 0x8u    /* TTL reached 0 (reference returns 0)  */
#define PPTK_RW_ST_ICMP 0x10u      /* ICMP echo: the identifier op applied  */
int pptk_tx_rewrite_device(struct pptk_rx_ctx *ctx, uint8_t *d_frames, const uint64_t *d_off,
                           const uint16_t *d_len, uint64_t stride, uint32_t fixed_len,
                           uint64_t n, const struct pptk_rewrite *d_rw, uint64_t rw_count,
                           uint8_t *d_status, void *stream);

/* TCP MSS clamping with incremental checksum update (middlebox / tunnel
 * ingress), reference iphdr/iphdr.c:4-132 (tcp_parse_options) and
 * iphdr/ipcksum.h:466-489 (tcp_set_mss_cksum_update): per frame with a TCP
 * header (the receive transform's record: PPTK_RX_F_L4 and proto 6, IPv4 or
 * IPv6, with or without a VLAN tag; with PPTK_MSS_SYN_ONLY also the SYN flag
 * set), whose options lie inside the segment (l4_off + data offset <= L4
 * end), tcp_parse_options is applied to the TCP header; if the option list
 * is valid and holds an MSS option whose value exceeds `mss`, the value
 * becomes `mss` through tcp_set_mss_cksum_update -- results identical to
 * those two calls.  Everything else is left untouched.  d_status (nullable)
 * receives per frame PPTK_MSS_ST_* bits.  Layout arguments as in
 * pptk_tx_cksum_device.  Asynchronous on `stream`. */
#define PPTK_MSS_SYN_ONLY 0x1u
#define PPTK_MSS_ST_TCP 0x1u       /* TCP header present (and SYN if asked) */
#define PPTK_MSS_ST_FOUND 0x2u     /* valid options with an MSS option      */
#define PPTK_MSS_ST_CLAMPED 0x4u   /* MSS lowered to `mss`                  */
#define PPTK_MSS_ST_BADOPT 0x8u    /* options past the segment or malformed */
int pptk_tcp_mss_clamp_device(struct pptk_rx_ctx *ctx, uint8_t *d_frames, const uint64_t *d_off,
                              const uint16_t *d_len, uint64_t stride, uint32_t fixed_len,
                              uint64_t n, uint16_t mss, uint32_t flags, uint8_t *d_status,
                              void *stream);

/* TCP sequence-space translation (SYN proxy / TCP splice): the rewrite a
 * stateful middlebox does on every packet of an established flow, reference
 * iphdr/ipcksum.h:395-623 and iphdr/iphdr.c:134-246.  Frame i takes the
 * translation d_xl[0] or d_xl[i] (d_idx NULL: xl_count must be 1 or n, as
 * pptk_tx_rewrite_device) or d_xl[d_idx[i]] (the result of a flow-table
 * lookup, pptk_flow_lookup_device below); an index >= xl_count (use 0xffffffff) means "no flow": the frame
 * is neither read nor written and its status is PPTK_SEQ_ST_NOFLOW.
 * Subjects are the frames whose receive record would be PPTK_RX_F_PARSED,
 * not MALFORMED, PPTK_RX_F_L4 and proto 6 (IPv4 or IPv6, with or without a
 * VLAN tag, never a fragment); everything else is left untouched with status
 * 0.  With end = tcp_data_offset, a subject with end < 20 or l4_off + end
 * past the L4 end is left untouched with status BADOPT, whatever the ops.
 * Otherwise the status gets TCP and the requested ops are applied in this
 * fixed order, byte for byte as the kept functions (include/ipcksum.h,
 * include/iphdr.h) called in this order on the TCP header:
 *   1 SEQ      tcp_set_seq_number_cksum_update(seq + seq_add)
 *   2 ACK      tcp_set_ack_number_cksum_update(ack + ack_add), only when the
 *              header's ACK flag is set (this API's own guard: the ack field
 *              of a segment without ACK carries nothing)
 *   3 SACK     tcp_find_sack_ts_headers, tcp_adjust_sack_cksum_update_2
 *              (sack_add): the LAST SACK option of that walk
 *   4 TSVAL    tcp_adjust_tsval_cksum_update(tsval_add)   (the same walk)
 *   5 TSECHO   tcp_adjust_tsecho_cksum_update(tsecho_add)
 *   6 SACK_OFF tcp_find_sack_header, tcp_disable_sack_cksum_update: the
 *              FIRST SACK option of that other walk becomes NOPs
 * with the checksum updated in exactly that sequence of ip_update_cksum16/32
 * steps.  Where the reference never returns, the kept functions decide: a
 * SACK or timestamp option with length byte 0 stops the walk, which keeps
 * what it recorded, and a SACK option of 10 or more bytes at an odd TCP
 * offset has each block adjusted once.  A checksum word that straddles the
 * end of the options takes the byte past them as 0 (it cancels in the
 * update) and never reads or writes it.  d_status (nullable) receives per
 * frame PPTK_SEQ_ST_* bits.  Layout arguments, asynchrony and error returns
 * as for pptk_tcp_mss_clamp_device; -EINVAL also for a null d_xl, xl_count
 * 0, or (without d_idx) xl_count neither 1 nor n. */
struct pptk_seqxlate {          /* 24 bytes, one per flow or per frame */
  uint32_t ops;                 /* PPTK_SEQ_* */
  uint32_t seq_add;             /* added to the sequence number        */
  uint32_t ack_add;             /* added to the acknowledgement number */
  uint32_t sack_add;            /* added to every SACK block edge      */
  uint32_t tsval_add;           /* added to the timestamp value        */
  uint32_t tsecho_add;          /* added to the timestamp echo reply   */
};
#define PPTK_SEQ_SEQ      0x01u
#define PPTK_SEQ_ACK      0x02u
#define PPTK_SEQ_SACK     0x04u
#define PPTK_SEQ_TSVAL    0x08u
#define PPTK_SEQ_TSECHO   0x10u
#define PPTK_SEQ_SACK_OFF 0x20u

#define PPTK_SEQ_ST_TCP      0x01u  /* TCP header and option area inside the segment       */
#define PPTK_SEQ_ST_SEQ      0x02u  /* sequence number rewritten                           */
#define PPTK_SEQ_ST_ACK      0x04u  /* acknowledgement number rewritten                    */
#define PPTK_SEQ_ST_SACK     0x08u  /* a SACK option was found and its blocks adjusted     */
#define PPTK_SEQ_ST_TS       0x10u  /* a timestamp option was found and adjusted           */
#define PPTK_SEQ_ST_SACK_OFF 0x20u  /* a SACK option was overwritten with NOPs             */
#define PPTK_SEQ_ST_BADOPT   0x40u  /* data offset < 20 or past the segment: untouched     */
#define PPTK_SEQ_ST_NOFLOW   0x80u  /* d_idx[i] >= xl_count: untouched                     */

int pptk_tcp_seq_translate_device(struct pptk_rx_ctx *ctx, uint8_t *d_frames,
                                  const uint64_t *d_off, const uint16_t *d_len, uint64_t stride,
                                  uint32_t fixed_len, uint64_t n,
                                  const struct pptk_seqxlate *d_xl, uint64_t xl_count,
                                  const uint32_t *d_idx, uint8_t *d_status, void *stream);

/* The same rules on one TCP segment the caller has located (host, per
 * packet): bytes [0, seglen) of tcphdr must be readable and writable, no
 * byte at or past seglen is read.  Does the end < 20 || end > seglen check
 * and the ACK-flag guard; returns the PPTK_SEQ_ST_* bits (TCP, SEQ, ACK,
 * SACK, TS, SACK_OFF or BADOPT). */
uint32_t pptk_tcp_seq_translate_hdr(void *tcphdr, uint32_t seglen,
                                    const struct pptk_seqxlate *x);

/* IPv4 fragmentation to an egress MTU (forwarder / tunnel ingress), the
 * batch form of the reference's fragment4() (ipfrag/ipfrag.c:11-123) with
 * the plan "as few fragments as possible".  `mtu` (68..65535) counts the IP
 * packet without L2.  Per frame, parsed exactly as pptk_rx_batch_device
 * parses: a frame whose record would be PARSED, not MALFORMED and not IPV6
 * is a subject (status PPTK_FRAG_ST_IPV4); everything else gets status 0 and
 * count 0.  With l2 = l3_off, ihl = ip_hdr_len, tl = ip_total_len and
 * datamax = tl - ihl (Ethernet padding past l2 + tl is ignored, as calling
 * fragment4 with sz = 14 + tl ignores it):
 *   tl <= mtu    PPTK_FRAG_ST_FITS, count 0: the caller sends the original.
 *   otherwise    PPTK_FRAG_ST_DF if ip_dont_frag, PPTK_FRAG_ST_ISFRAG if
 *                ip_more_frags or ip_frag_off != 0, PPTK_FRAG_ST_BADCKSUM if
 *                ip_hdr_cksum_calc(ip, ihl) != 0 -- the conditions under
 *                which fragment4 abort()s (:42-61); with any of them count
 *                is 0 and nothing is emitted (DF: answer with ICMP).
 *   else         PPTK_FRAG_ST_DONE: per = (mtu - ihl) & ~7, count =
 *                ceil(datamax / per); fragment j carries datastart = j * per
 *                and datalen = min(per, datamax - datastart).
 * A fragment is what fragment4 writes (:106-121): the frame's first l2 + ihl
 * bytes (every IP option goes into every fragment, as in the reference),
 * ip_set_frag_off(datastart), ip_set_more_frags(datastart + datalen <
 * datamax) -- the reserved and DF bits stay --, ip_set_total_len(ihl +
 * datalen), ip_set_hdr_cksum_calc(ip, ihl), then datalen payload bytes from
 * frame + l2 + ihl + datastart; its length is l2 + ihl + datalen.
 *
 * Output: first[i] = the exclusive prefix sum of the counts; the fragments
 * of frame i fill slots first[i] .. first[i] + count[i] - 1 in ascending
 * offset, slot s at d_out + s * out_stride: bytes [0, len) the fragment,
 * bytes [len, round_up(len, 16)) zero, the rest of the slot untouched.  A
 * DONE frame with first[i] + count[i] > out_cap also gets
 * PPTK_FRAG_ST_NOROOM and none of its slots is written (so every later DONE
 * frame has it too; earlier frames are complete).  d_out_len[s] / d_out_src[s]
 * (nullable) receive the length and the source frame index of every written
 * slot; d_first / d_count / d_status (nullable) the per-frame words (d_first
 * holds the low 32 bits); d_totals[0] the slots the batch needs, d_totals[1]
 * the slots written.  The slots can go straight back into
 * pptk_rx_batch_device (stride = out_stride, d_len = d_out_len) or
 * pptk_tx_cksum_device.
 *
 * d_out must be 16-byte aligned, out_stride a multiple of 16 and >=
 * round_up(18 + mtu, 16), n <= 2^24 and out_cap < 2^32 (-EINVAL otherwise).  Layout arguments
 * and the frame read bounds are those of pptk_tx_cksum_device /
 * pptk_rx_dev_batch (no frame shorter than 14 bytes is read at all).  n = 0
 * writes d_totals = {0, 0}.  d_scratch: pptk_ip_fragment_scratch_bytes(n)
 * bytes, 16-byte aligned, no initialisation needed, in use until the stream
 * reaches the end of the call.  Asynchronous on `stream`.
 *
 * Out of scope: re-fragmenting fragments (ISFRAG), IPv6, the "copied" flag
 * of IP options (the reference copies all of them), and a host
 * ldp_packet[] in -> host out batch path (pptk_ip_fragment_host is per
 * packet). */
#define PPTK_FRAG_ST_IPV4 0x01u      /* a subject: parsed IPv4                */
#define PPTK_FRAG_ST_FITS 0x02u      /* tl <= mtu: send the original          */
#define PPTK_FRAG_ST_DONE 0x04u      /* fragmented into count slots           */
#define PPTK_FRAG_ST_DF 0x08u        /* too big and DF set                    */
#define PPTK_FRAG_ST_ISFRAG 0x10u    /* too big and already a fragment        */
#define PPTK_FRAG_ST_BADCKSUM 0x20u  /* too big and a bad header checksum     */
#define PPTK_FRAG_ST_NOROOM 0x40u    /* DONE but past out_cap: not written    */
size_t pptk_ip_fragment_scratch_bytes(uint64_t n);
int pptk_ip_fragment_device(struct pptk_rx_ctx *ctx, const uint8_t *d_frames,
                            const uint64_t *d_off, const uint16_t *d_len, uint64_t stride,
                            uint32_t fixed_len, uint64_t n, uint32_t mtu, uint8_t *d_out,
                            uint64_t out_stride, uint64_t out_cap, uint16_t *d_out_len,
                            uint32_t *d_out_src, uint32_t *d_first, uint32_t *d_count,
                            uint8_t *d_status, uint64_t *d_totals, void *d_scratch,
                            void *stream);

/* The per-packet host form, and the CPU statement of the contract above
 * (plain C over iphdr.h / ipcksum.h, pptk_amd/csrc/host/ipfrag.c): the same
 * rules and the same slot layout for one frame.  Returns the fragment count
 * (0 unless *status has DONE) or -EINVAL (a null frame with len > 0, a null
 * out, out_len or status, an mtu outside 68..65535, an out_stride that is
 * not a multiple of 16 or is below round_up(18 + mtu, 16); *status is then
 * not written).  With count > out_cap the status gets NOROOM,
 * nothing is written and the count is still returned.  `out` needs no
 * alignment. */
int pptk_ip_fragment_host(const void *frame, uint32_t len, uint32_t mtu, uint8_t *out,
                          uint64_t out_stride, uint32_t out_cap, uint16_t *out_len,
                          uint8_t *status);

/* IPv4 reassembly, the receiving half of the reference's ipfrag/
 * (ipfrag/ipreass.c reassctx_add / reassctx_reassemble) as a stateless,
 * batch-local call: it rebuilds the datagrams whose fragments are all in the
 * batch and reports the rest.  The loop is
 *   pptk_rx_batch_device (d_recs + d_frag) -> pptk_ip_reass_device
 *      -> pptk_rx_batch_device on the slots -> pptk_tunnel_decap_device ...
 * and carrying the members of INCOMPLETE datagrams over to the next batch is
 * the caller's job, done with descriptors (keep their d_off / d_len entries
 * and put them in front of the next batch's; the frames stay where they
 * are).  pptk_ip_reass_host (pptk_amd/csrc/host/ipreass.c, plain C over
 * iphdr.h / ipcksum.h) is the statement of this contract; the device call
 * equals it byte for byte, in every output array and in every byte it must
 * not touch.
 *
 * Inputs.  Frame layout and read bounds are those of pptk_ip_fragment_device;
 * recs[i] and frag[i] are what pptk_rx_batch_device wrote for the same
 * frames.  The records are trusted for meaning, never for memory safety:
 * whatever they say, no byte outside a frame's own 16-byte chunks is read and
 * nothing outside the output arrays is written.
 *
 * Per frame (fstatus[i], dgram[i]).  Frame i is a fragment
 * (PPTK_REASS_FST_FRAG) when recs[i].flags has PARSED and FRAGMENT and has
 * neither MALFORMED nor IPV6; every other frame gets status 0 and dgram[i] =
 * 0xffffffff.  With l3 = recs[i].l3_off, off = frag[i].frag_off, dl =
 * frag[i].data_len, MF = frag[i].flags & PPTK_RX_FRAG_MF and ihl_i = 4 *
 * (frame[l3] & 15), a fragment is rejected (dgram[i] = 0xffffffff) with
 *   PPTK_REASS_FST_BADCKSUM  recs[i].ip_cksum != 0
 *   PPTK_REASS_FST_BADFRAG   l3 is not 14 or 18; len <= l3 (then frame[l3] is
 *                            not read); ihl_i < 20; dl == 0; off + dl > 65535
 *                            (ipreass.c:119-122); MF and dl % 8 != 0; l3 +
 *                            ihl_i + dl > len
 * (both bits when both hold).  The remaining fragments are the candidates,
 * numbered in index order; only the first max_candidates are considered, the
 * rest get PPTK_REASS_FST_SKIPPED (dgram[i] = 0xffffffff) and count in
 * hdr.candidates and nowhere else, which bounds work and scratch under a
 * flood.  A considered candidate gets PPTK_REASS_FST_MEMBER and dgram[i] =
 * its datagram's report index, and PPTK_REASS_FST_DONE too when that datagram
 * is WRITTEN: the frame is consumed.
 *
 * Datagrams.  The key is (src[0..3], dst[0..3], proto of the record, ident &
 * 0xffff), compared exactly (a hash only finds the bucket); L2 is not part of
 * it.  The leader is the key's lowest-indexed considered candidate; report
 * entries are the datagrams in ascending leader index, entry k written only
 * when k < report_cap.  Order a datagram's members by (off, frame index);
 * its status is the first that applies of
 *   PPTK_REASS_DG_TOOMANY     more than 64 members (nothing else is examined)
 *   PPTK_REASS_DG_OVERLAP     two neighbours with off[k] + dl[k] > off[k+1];
 *                             more than one member without MF; a member
 *                             without MF that is not the last in this order
 *   PPTK_REASS_DG_INCOMPLETE  no member without MF; off[0] != 0; a gap
 *                             between neighbours
 *   PPTK_REASS_DG_COMPLETE    otherwise; total = off[last] + dl[last]
 * For a COMPLETE datagram l2 is the leader's l3 and ihl the leader's ihl_i
 * (the reference takes the header of the first packet added, ipreass.c:47-50),
 * len = l2 + ihl + total, and it also gets, the first that applies of
 *   PPTK_REASS_DG_TOOBIG   len > 65535 (lengths are 16 bits here, as d_len;
 *                          this includes ihl + total > 65535) or
 *                          round_up(len, 16) > out_stride
 *   PPTK_REASS_DG_NOROOM   the datagram takes the next slot in report order
 *                          (TOOBIG ones take none) and that slot is >= out_cap
 *   PPTK_REASS_DG_WRITTEN  otherwise
 * A written slot is what reassctx_reassemble writes (ipreass.c:61-86): the
 * leader's first l2 + ihl bytes, ip_set_frag_off(0) and ip_set_more_frags(0)
 * (the DF and reserved bits stay), ip_set_total_len(ihl + total),
 * ip_set_hdr_cksum_calc(ip, ihl), then each member's dl payload bytes from
 * frame + l3 + ihl_i at l2 + ihl + off.  Bytes [len, round_up(len, 16)) are
 * zero, the rest of the slot is untouched, out_len[slot] = len.  The slots go
 * straight back into pptk_rx_batch_device (stride = out_stride, d_len =
 * d_out_len) and pptk_tunnel_decap_device.
 *
 * Deviation from the reference, stated: it accepts overlapping fragments
 * (the later copy wins, the smallest last end is taken); here such a datagram
 * is reported as OVERLAP and not built, as current IP stacks do, and the
 * host decides (dropping is the sane policy).
 *
 * -EINVAL: a null ctx (device call) or hdr; with n > 0 a null frames, recs,
 * frag, dgram or fstatus, a scratch (device call) that is null, not 256-byte
 * aligned or below pptk_ip_reass_scratch_bytes(n, max_candidates), no layout
 * (no off, stride 0, n > 1) or a fixed_len above 65535 without len; a null out
 * or out_len with out_cap > 0, a null report with report_cap > 0; out not
 * 16-byte, recs or frag not 16-byte (device call), report or dgram not 4-byte,
 * hdr not 8-byte aligned; out_stride not a multiple of 16; n > 2^24;
 * max_candidates 0 or above 2^24; out_cap or report_cap >= 2^32.  n = 0
 * writes a zero header and nothing else.  The host call returns -ENOMEM when
 * its tables cannot be allocated.
 *
 * The device call is asynchronous on `stream`: a fixed sequence of launches
 * ordered by kernel boundaries only (no grid barrier, no spin, no lane waits
 * for another workgroup's store), every loop bound a kernel argument or a
 * device value clamped by one, all arithmetic integer, the result the same
 * for any grid and interleaving.  It clears what it needs of the scratch and
 * must not share a scratch with a call in flight on another stream.
 * pptk_ip_reass_shape reports the member limit (64) and the frames of one
 * workgroup of the per-frame passes; results do not depend on the latter.
 *
 * Out of scope: IPv6 fragments, pptk_rx_rec32 input, state across batches
 * and timeouts, datagrams of more than 64 fragments, and merging overlaps. */
#define PPTK_REASS_FST_FRAG 0x01u      /* PARSED | FRAGMENT IPv4, not MALFORMED   */
#define PPTK_REASS_FST_BADCKSUM 0x02u  /* rejected: bad header checksum           */
#define PPTK_REASS_FST_BADFRAG 0x04u   /* rejected: inconsistent fragment fields  */
#define PPTK_REASS_FST_SKIPPED 0x08u   /* a candidate past max_candidates         */
#define PPTK_REASS_FST_MEMBER 0x10u    /* considered: dgram[i] is its datagram    */
#define PPTK_REASS_FST_DONE 0x20u      /* its datagram was WRITTEN: consumed      */
#define PPTK_REASS_DG_COMPLETE 0x01u   /* every byte of the datagram is there     */
#define PPTK_REASS_DG_WRITTEN 0x02u    /* COMPLETE and built in `slot`            */
#define PPTK_REASS_DG_INCOMPLETE 0x04u /* a hole, or the last fragment is missing */
#define PPTK_REASS_DG_OVERLAP 0x08u    /* overlapping or contradictory fragments  */
#define PPTK_REASS_DG_TOOMANY 0x10u    /* more than 64 members                    */
#define PPTK_REASS_DG_TOOBIG 0x20u     /* COMPLETE, does not fit a slot           */
#define PPTK_REASS_DG_NOROOM 0x40u     /* COMPLETE, slot >= out_cap               */
struct pptk_reass_dgram {  /* 16 bytes, one report entry per datagram */
  uint32_t first;          /*  0 frame index of its leader                       */
  uint32_t slot;           /*  4 output slot, 0xffffffff unless WRITTEN          */
  uint32_t frags;          /*  8 considered fragments carrying its key           */
  uint16_t out_len;        /* 12 l2 + ihl + total; 0 unless COMPLETE and <= 65535 */
  uint8_t status;          /* 14 PPTK_REASS_DG_*                                 */
  uint8_t reserved;        /* 15 always 0                                        */
};
struct pptk_reass_hdr {    /* 48 bytes, 8-byte aligned */
  uint64_t candidates;     /* fragments that passed the per-frame checks         */
  uint64_t considered;     /* min(candidates, max_candidates)                    */
  uint64_t dgrams;         /* datagrams among the considered                     */
  uint64_t reported;       /* min(dgrams, report_cap)                            */
  uint64_t complete;       /* datagrams with PPTK_REASS_DG_COMPLETE              */
  uint64_t written;        /* slots written                                      */
};
size_t pptk_ip_reass_scratch_bytes(uint64_t n, uint64_t max_candidates);
int pptk_ip_reass_device(struct pptk_rx_ctx *ctx, const uint8_t *d_frames,
                         const uint64_t *d_off, const uint16_t *d_len, uint64_t stride,
                         uint32_t fixed_len, uint64_t n, const struct pptk_rx_rec *d_recs,
                         const struct pptk_rx_frag *d_frag, uint64_t max_candidates,
                         uint8_t *d_out, uint64_t out_stride, uint64_t out_cap,
                         uint16_t *d_out_len, struct pptk_reass_dgram *d_report,
                         uint64_t report_cap, uint32_t *d_dgram, uint8_t *d_fstatus,
                         struct pptk_reass_hdr *d_hdr, void *d_scratch, size_t scratch_bytes,
                         void *stream);
int pptk_ip_reass_host(const uint8_t *frames, const uint64_t *off, const uint16_t *len,
                       uint64_t stride, uint32_t fixed_len, uint64_t n,
                       const struct pptk_rx_rec *recs, const struct pptk_rx_frag *frag,
                       uint64_t max_candidates, uint8_t *out, uint64_t out_stride,
                       uint64_t out_cap, uint16_t *out_len, struct pptk_reass_dgram *report,
                       uint64_t report_cap, uint32_t *dgram, uint8_t *fstatus,
                       struct pptk_reass_hdr *hdr);
void pptk_ip_reass_shape(uint32_t *max_frags, uint32_t *block_frames);

/* GRE tunnel gateway (tunnel ingress and egress), the batch form of the
 * reference's ldp/ldptunnel.c: encap puts the fixed 38-byte header Ethernet +
 * IPv4 + GRE with protocol type 0x6558 (transparent Ethernet bridging) in
 * front of every frame (template :29-46, per packet :126-128), decap finds
 * the inner frame of such a packet (:155-158).  With them a tunnel endpoint
 * runs  decap -> pptk_rx_batch_device on the inner frames  and
 * pptk_tcp_mss_clamp_device -> encap -> pptk_ip_fragment_device  on batches
 * that stay in device memory.
 *
 * Encap.  Frame i takes the tunnel d_tun[0] or d_tun[i] (d_idx NULL:
 * tun_count must be 1 or n) or d_tun[d_idx[i]]; an index >= tun_count (use
 * 0xffffffff) means "no tunnel": status PPTK_TUN_ST_NOFLOW, the frame is not
 * read and its slot is not written.  A tunnel whose `reserved` is not 0 or
 * whose `flags` hold an unknown bit is malformed and gives its frames
 * PPTK_TUN_ST_BADTUN, likewise unread and unwritten: the device call cannot
 * look into d_tun without waiting for the stream, so that check is per frame
 * and not an error return (a caller that builds the table on the host checks
 * it there; the Python binding does).  Slot i, at d_out +
 * i * out_stride, belongs to frame i: no compaction, one launch.  Per frame,
 * with len its length:
 *   len < 14                PPTK_TUN_ST_RUNT: nothing is read
 *   38 + len > 65535        PPTK_TUN_ST_TOOBIG (the 16-bit frame length of the
 *                           batch layout; so len + 24 <= 65535 always holds)
 *   38 + len > out_stride   PPTK_TUN_ST_NOROOM (host form: > out_cap); TOOBIG
 *                           and NOROOM are independent of each other
 *   else                    PPTK_TUN_ST_DONE: slot bytes [0, 38 + len) are
 *                           written, bytes [38 + len, round_up(38 + len, 16))
 *                           are zero, the rest of the slot is untouched
 * A frame without DONE has no byte of its slot written.  d_out_len[i]
 * (nullable) is 38 + len with DONE, else 0; d_status[i] (nullable) the
 * PPTK_TUN_ST_* bits.  The header is what ldptunnel.c writes through the kept
 * setters of include/iphdr.h:
 *   Ethernet  ether_dst, ether_src, ether_set_type(0x0800)
 *   IPv4      ip_set_version(4), ip_set_hdr_len(20), tos, ip_set_total_len(
 *             len + 24), ip_set_id(id), ip_set_dont_frag(PPTK_TUN_DF) with MF
 *             and offset 0, ip_set_ttl, ip_set_proto(47), ip_set_src,
 *             ip_set_dst, ip_set_hdr_cksum_calc(ip, 20)
 *   GRE       00 00 65 58 (no checksum, key or sequence number, version 0)
 * followed by the len frame bytes unchanged.  id is t.id, or with
 * PPTK_TUN_ID_SEQ (uint16_t)(t.id + id_base + i) (host form: seq in place of
 * id_base + i), which wraps 0xffff -> 0.
 *
 * d_out must be 16-byte aligned, out_stride a multiple of 16, d_tun 16-byte
 * aligned (-EINVAL otherwise); -EINVAL also for a null d_tun, tun_count 0 or
 * (without d_idx) tun_count neither 1 nor n, as
 * pptk_tcp_seq_translate_device.  Layout arguments, read bounds (nothing
 * outside the aligned 16-byte chunks of [frame, frame + len) is read, no
 * frame shorter than 14 bytes is read at all), asynchrony and the other
 * error returns are those of pptk_ip_fragment_device; there is no scratch
 * and no limit on n.  The slots go straight into pptk_ip_fragment_device,
 * pptk_rx_batch_device or pptk_tx_cksum_device (stride = out_stride, d_len =
 * d_out_len).
 *
 * Decap is zero-copy: it writes descriptors, never frames.  The outer subject
 * test is pptk_ip_fragment_device's: one optional 802.1Q tag, ethertype
 * 0x0800, version 4, 20 <= ihl <= tl, l2 + tl <= len; a subject gets
 * PPTK_DECAP_ST_IPV4.  A subject with ip_proto 47 is checked further, each
 * bit on its own:
 *   ISFRAG    ip_more_frags or ip_frag_off != 0
 *   BADCKSUM  ip_hdr_cksum_calc(ip, ihl) != 0
 *   GRE       not ISFRAG and tl - ihl >= 4
 *   SHORT     not ISFRAG and tl - ihl < 4
 *   GREOPT    with GRE: the first 16-bit GRE word != 0 (C, K or S flag, a
 *             reserved bit or a version)
 *   PTYPE     with GRE: the second GRE word != 0x6558
 *   OK        GRE with none of BADCKSUM, GREOPT, PTYPE
 * With OK d_in_off[i] = base + l2 + ihl + 4, an absolute byte offset into
 * d_frames (base = d_off[i] or i * stride), and d_in_len[i] = tl - ihl - 4:
 * Ethernet padding after the outer packet is excluded.  Otherwise d_in_off[i]
 * = base and d_in_len[i] = 0.  The pair goes straight into
 * pptk_rx_batch_device as d_off / d_len.  All three outputs are nullable.
 *
 * Out of scope: the GRE key, sequence and checksum fields (GREOPT: the caller
 * decides), IPv6 or IP-in-IP outers, a match of the outer addresses against
 * an endpoint (the caller has them from the outer frames' receive records),
 * the ICMP answer to a DF packet that does not fit, and a host ldp_packet[]
 * batch path (the host forms are per packet). */
struct pptk_tunnel {            /* 32 bytes, one per tunnel */
  uint8_t eth_dst[6], eth_src[6];
  uint32_t src, dst;            /* outer IPv4, host order (ip_set_src/dst) */
  uint16_t id;                  /* ip_set_id */
  uint8_t ttl, tos;
  uint32_t flags;               /* PPTK_TUN_DF | PPTK_TUN_ID_SEQ */
  uint32_t reserved;            /* must be 0 */
};
#define PPTK_TUN_DF     0x1u    /* ip_set_dont_frag(ip, 1)                 */
#define PPTK_TUN_ID_SEQ 0x2u    /* id counts up with the frame index       */
#define PPTK_TUN_HDR_LEN 38u    /* 14 + 20 + 4 */

#define PPTK_TUN_ST_DONE   0x01u  /* slot written                             */
#define PPTK_TUN_ST_RUNT   0x02u  /* len < 14: nothing read, nothing written  */
#define PPTK_TUN_ST_TOOBIG 0x04u  /* 38 + len > 65535                         */
#define PPTK_TUN_ST_NOROOM 0x08u  /* 38 + len > out_stride (host: out_cap)    */
#define PPTK_TUN_ST_NOFLOW 0x10u  /* tunnel index >= tun_count: frame not read */
#define PPTK_TUN_ST_BADTUN 0x20u  /* malformed tunnel entry: frame not read    */

#define PPTK_DECAP_ST_IPV4     0x01u  /* a subject: parsed IPv4                */
#define PPTK_DECAP_ST_GRE      0x02u  /* proto 47, whole, a GRE header fits    */
#define PPTK_DECAP_ST_OK       0x04u  /* descriptor points at the inner frame  */
#define PPTK_DECAP_ST_ISFRAG   0x08u  /* proto 47 and a fragment               */
#define PPTK_DECAP_ST_BADCKSUM 0x10u  /* proto 47 and a bad header checksum    */
#define PPTK_DECAP_ST_SHORT    0x20u  /* proto 47, whole, tl - ihl < 4         */
#define PPTK_DECAP_ST_GREOPT   0x40u  /* GRE flags or version not 0            */
#define PPTK_DECAP_ST_PTYPE    0x80u  /* GRE protocol type not 0x6558          */

int pptk_tunnel_encap_device(struct pptk_rx_ctx *ctx, const uint8_t *d_frames,
                             const uint64_t *d_off, const uint16_t *d_len, uint64_t stride,
                             uint32_t fixed_len, uint64_t n, const struct pptk_tunnel *d_tun,
                             uint64_t tun_count, const uint32_t *d_idx, uint32_t id_base,
                             uint8_t *d_out, uint64_t out_stride, uint16_t *d_out_len,
                             uint8_t *d_status, void *stream);
int pptk_tunnel_decap_device(struct pptk_rx_ctx *ctx, const uint8_t *d_frames,
                             const uint64_t *d_off, const uint16_t *d_len, uint64_t stride,
                             uint32_t fixed_len, uint64_t n, uint64_t *d_in_off,
                             uint16_t *d_in_len, uint8_t *d_status, void *stream);

/* The per-packet host forms, and the CPU statement of the contract above
 * (plain C over iphdr.h / ipcksum.h, pptk_amd/csrc/host/tunnel.c).  Both
 * return the status bits.  Encap takes the tunnel itself (no index) and seq
 * in place of id_base + i; out_cap is the size of `out` in bytes: NOROOM is
 * 38 + len > out_cap, and with DONE out[0, min(round_up(38 + len, 16),
 * out_cap)) is written.  *out_len (nullable) = 38 + len or 0.  A null t or
 * out, or a null frame with len >= 14, gives NOFLOW, a malformed t
 * BADTUN.  `out` needs no
 * alignment.  Decap sets *in_off (relative to frame) and *in_len, both
 * nullable. */
uint32_t pptk_tunnel_encap_host(const void *frame, uint32_t len, const struct pptk_tunnel *t,
                                uint32_t seq, uint8_t *out, uint64_t out_cap,
                                uint16_t *out_len);
uint32_t pptk_tunnel_decap_host(const void *frame, uint32_t len, uint32_t *in_off,
                                uint16_t *in_len);

/* Flow table: the step between the receive transform and the per-flow
 * header edits.  pptk_tcp_seq_translate_device and pptk_tunnel_encap_device
 * take a d_idx, "the flow of frame i"; this is what produces it:
 *   rx -> pptk_flow_lookup_device -> seq-translate / rewrite / encap -> fragment
 * all on batches that stay in device memory.  The structure is the
 * reference's hashtable/hashtable.h: a power-of-two array addressed by
 * bucket = hashval & (bucketcnt - 1) with hashval the SipHash of the key
 * truncated to 32 bits, candidates compared key by key, never growing
 * (hash_table_add_nogrow).  The table is managed on the host -- it is the
 * control plane, as the reference's is -- and mirrored in device memory; one
 * kernel turns a batch of records into d_idx.
 *
 * Shape.  `slots` is a power of two, 16 .. 2^26 (-EINVAL otherwise); the
 * table holds at most slots / 2 flows and never grows (insert beyond:
 * -ENOSPC).  ctx == NULL gives a host-only table: find and lookup_host work
 * on it, sync and lookup_device return -EINVAL.  One writer at a time, no
 * locking, as the reference's table.
 *
 * Hashing.  The table never hashes: the caller passes the flow_hash the
 * receive transform wrote into the record, or, for a flow no frame of which
 * it has seen yet, pptk_flow_key_hash(opts.key, &key): siphash_buf over
 * src | dst | be16 sport | be16 dport | proto | 0 0 0, the 40 bytes the
 * receive transform hashes, so that for every parsed frame it equals
 * rec.flow_hash.  pptk_flow_key_from_rec copies a record's tuple into a key.
 * A key whose zero[] is not 0 is -EINVAL everywhere.
 *
 * Probing.  The home slot is (uint32_t)flow_hash & (slots - 1), the
 * reference's bucket; collisions resolve by linear probing with wrap-around.
 * A slot matches when it is in use, its stored 64-bit hash equals the hash
 * given and all 37 key bytes (src, dst, sport, dport, proto) are equal: a
 * 64-bit hash match alone is never a hit.
 *
 * insert   0; -EEXIST for a key that is present (its value is left alone);
 *          -ENOSPC at slots / 2 flows; -EINVAL for value PPTK_FLOW_NONE.
 * update   sets the value of a present key; -ENOENT if absent.
 * delete   backward-shift deletion: the image never holds tombstones and an
 *          empty slot always ends a probe; -ENOENT if absent.
 * find     0 and *value (nullable), or -ENOENT.
 * insert_recs  inserts the key of every record that is a subject (below,
 *          with d_subject NULL) with values[i]; results[i] (nullable) = 0,
 *          -EEXIST, -ENOSPC, or -EINVAL for a non-subject or a bad value.
 *          Returns the number inserted, or -EINVAL for null arguments.
 * clear    empties the table.
 * stats    slots, count and probe_limit (each nullable): probe_limit is 0 for
 *          an empty table that has held nothing since the last clear, else
 *          1 + the largest displacement from its home slot any entry has had
 *          since then; it may stay high after deletes.
 *
 * sync uploads the slots that changed since the last sync, tracked at a
 * granularity of 4 KB of image (a first sync uploads everything), on
 * `stream`, and waits for the upload: on return the device image equals the
 * host image.  *uploaded_bytes (nullable) is what it copied.  Device lookups
 * see the table as of the last sync; ordering a sync against lookups in
 * flight on other streams is the caller's duty.
 *
 * lookup.  A record is a subject when it has PPTK_RX_F_PARSED, lacks
 * PPTK_RX_F_MALFORMED and d_subject[i] != 0 (or d_subject is NULL).  Its key
 * is record bytes 8..43 plus proto, its hash flow_hash.  A subject found gets
 * d_idx[i] = value and status SUBJECT | HIT; one not found PPTK_FLOW_NONE and
 * SUBJECT; a non-subject PPTK_FLOW_NONE and 0.  PPTK_FLOW_NONE is the "no
 * flow" index of pptk_tcp_seq_translate_device and pptk_tunnel_encap_device.
 * Nothing is written past entry n - 1; n = 0 launches nothing.  The probe of
 * a record ends at the first unused slot and after probe_limit slots at the
 * latest (a kernel argument from the host's bookkeeping, never above
 * `slots`), whatever the image holds.  d_recs must be 16-byte and d_idx 4-byte
 * aligned; -EINVAL for that, for a null ctx, t, d_recs or d_idx (with n > 0),
 * a host-only table, a table of another context's device or one never
 * synced.  d_status is nullable.  Asynchronous on `stream`.
 * pptk_flow_lookup_host is the same rule over the host image (idx required,
 * subject and status nullable) and the CPU statement of this contract.
 *
 * Last-seen stamps, per-flow counters and idle expiry are the next section,
 * "Flow state".
 *
 * Out of scope: inserts or deletes performed by a kernel (the device only
 * reports the new flows of a batch, "Flow learning" below; the host inserts),
 * growth, a
 * direction-symmetric key (the caller inserts both directions),
 * pptk_rx_rec32 input (it lacks the IPv6 addresses), and locking. */
struct pptk_flow_key {            /* 40 bytes: the tuple the flow hash covers */
  uint8_t src[16], dst[16];       /* as pptk_rx_rec.src / .dst                */
  uint16_t sport, dport;          /* host order, as the record                */
  uint8_t proto;                  /* pptk_rx_rec.proto                        */
  uint8_t zero[3];                /* must be 0 (-EINVAL otherwise)            */
};
#define PPTK_FLOW_NONE 0xffffffffu  /* d_idx value "no flow"; not a legal value to insert */
#define PPTK_FLOW_ST_SUBJECT 0x1u
#define PPTK_FLOW_ST_HIT     0x2u

struct pptk_flow_table;
int pptk_flow_table_create(struct pptk_rx_ctx *ctx, uint32_t slots, struct pptk_flow_table **t);
void pptk_flow_table_destroy(struct pptk_flow_table *t);
void pptk_flow_key_from_rec(const struct pptk_rx_rec *rec, struct pptk_flow_key *key);
uint64_t pptk_flow_key_hash(const uint8_t key16[16], const struct pptk_flow_key *key);
int pptk_flow_table_insert(struct pptk_flow_table *t, const struct pptk_flow_key *key,
                           uint64_t flow_hash, uint32_t value);
int pptk_flow_table_update(struct pptk_flow_table *t, const struct pptk_flow_key *key,
                           uint64_t flow_hash, uint32_t value);
int pptk_flow_table_delete(struct pptk_flow_table *t, const struct pptk_flow_key *key,
                           uint64_t flow_hash);
int pptk_flow_table_find(const struct pptk_flow_table *t, const struct pptk_flow_key *key,
                         uint64_t flow_hash, uint32_t *value);
int pptk_flow_table_insert_recs(struct pptk_flow_table *t, const struct pptk_rx_rec *recs,
                                uint64_t n, const uint32_t *values, int32_t *results);
void pptk_flow_table_clear(struct pptk_flow_table *t);
void pptk_flow_table_stats(const struct pptk_flow_table *t, uint32_t *slots, uint32_t *count,
                           uint32_t *probe_limit);
int pptk_flow_table_sync(struct pptk_flow_table *t, void *stream, uint64_t *uploaded_bytes);
int pptk_flow_lookup_device(struct pptk_rx_ctx *ctx, const struct pptk_flow_table *t,
                            const struct pptk_rx_rec *d_recs, uint64_t n,
                            const uint8_t *d_subject, uint32_t *d_idx, uint8_t *d_status,
                            void *stream);
int pptk_flow_lookup_host(const struct pptk_flow_table *t, const struct pptk_rx_rec *recs,
                          uint64_t n, const uint8_t *subject, uint32_t *idx, uint8_t *status);

/* Flow state: what the frames of a batch leave behind per flow, and what the
 * host does with it.  The batches never leave device memory, so the host
 * sees no traffic; a kernel leaves per flow value a packet counter, a byte
 * counter and a last-seen stamp, the host downloads that small array now and
 * then and deletes the flows that have been idle -- the work the reference
 * does in its table users (ldp/ldpswitch.c:88-123 time_out(): every entry
 * with e->time64 + TIMEOUT < time64, the stamp refreshed per packet at :139;
 * arp/arp.c:30-31,107-120: a 30 s entry timer).  The gateway loop is
 *   insert + stats_reset, then per batch
 *   rx -> pptk_flow_lookup_device -> pptk_flow_account_device
 *      -> pptk_tx_rewrite_flow_device / seq-translate / encap -> fragment,
 *   and every T seconds: download stats -> pptk_flow_table_expire
 *      -> stats_reset of the recycled values -> pptk_flow_table_sync.
 *
 * Accounting.  Entry v of the stats array belongs to flow value v (the value
 * given at insert, d_idx[i] of the lookup).  pptk_flow_account_host is the
 * CPU statement of the contract: for frame i, v = idx[i], L = len ? len[i] :
 * fixed_len, e = v < stats_count ? &stats[v] : unmatched; if e is not NULL,
 *   e->packets += 1; e->bytes += L; e->last_seen = max(e->last_seen, now).
 * The arrays accumulate (the caller zeroes them once); PPTK_FLOW_NONE is an
 * index >= stats_count like any other, so the lookup's non-subjects and
 * misses land in `unmatched` (nullable), the drop counter.  `reserved` and
 * every entry at or past stats_count are never touched; n = 0 changes nothing
 * and launches nothing.  The sums are integer arithmetic mod 2^64 and
 * independent of order: the device call equals the host call bit for bit,
 * whatever streams or kernel shapes ran it.  `now` is the caller's clock in
 * the caller's unit.  -EINVAL: a null ctx (device call); null idx or stats
 * with n > 0; stats_count 0 or above 2^32; idx not 4-byte, len not 2-byte,
 * stats or unmatched not 32-byte aligned; fixed_len > 65535 (with or without
 * len).  The device call is asynchronous on `stream`; calls on several
 * streams may add into one array.
 *
 * pptk_flow_stats_reset_device sets stats[v] = {0, 0, now, reserved
 * unchanged} for every v = d_values[k] < stats_count (values past the array
 * are skipped, duplicates are allowed) with plain stores in one launch: how a
 * flow value is recycled, and how a flow inserted before its first frame gets
 * a stamp, so that it does not expire at once.  It must not run beside an
 * accounting call that counts the same values.  -EINVAL as above, d_values
 * 4-byte aligned and non-null with count > 0.
 *
 * pptk_flow_account_shape reports the accounting kernel of the built
 * library: the frames a workgroup sums in LDS before it touches the array
 * (segment_frames) and the slots of its LDS table (lds_slots; 0 for a build
 * whose lanes add to the array directly, make abvariant NAME=flowstat_direct
 * DEFS=-DPPTK_FLOWSTAT_DIRECT=1).  Results do not depend on it.
 *
 * pptk_flow_table_expire (host; works on host-only tables) deletes from the
 * host image every flow whose value v < stats_count and whose
 * stats[v].last_seen + idle < now -- strictly, as ldpswitch.c:100, and without
 * 64-bit wrap: a sum past 2^64 is "not idle".  `stats` is the host copy the
 * caller downloaded.  Flows whose value lies past stats_count never expire.
 * At most `cap` flows are deleted per call, their values written to
 * expired_values (nullable when cap is 0, and then nothing is deleted); the
 * return value is the number deleted, and the caller calls again while it
 * equals cap.  Deletion is the table's backward-shift delete and marks the
 * same dirty pages, so the next sync uploads them; probe_limit stays a valid
 * bound.  -EINVAL for a null t or stats, or a null expired_values with cap > 0.
 *
 * pptk_tx_rewrite_flow_device is pptk_tx_rewrite_device with the lookup's
 * result: with d_idx non-null frame i takes d_rw[d_idx[i]], and an index >=
 * rw_count means no flow -- the frame is neither read nor written and its
 * status is exactly PPTK_RW_ST_NOFLOW (pptk_tcp_seq_translate_device's rule);
 * rw_count must not be 0 and d_idx must be 4-byte aligned.  With d_idx NULL
 * it is pptk_tx_rewrite_device itself (rw_count 1 or n).  Everything else is
 * that call's contract.
 *
 * Out of scope: TCP-state tracking (FIN / RST), per-flow rate limiting, an
 * LRU list, IPv6 address rewrite (the reference has no such setter),
 * pptk_rx_rec32 input, and locking. */
struct pptk_flow_stats {     /* 32 bytes, 32-byte aligned; entry v belongs to flow value v */
  uint64_t packets;          /* frames counted, mod 2^64                      */
  uint64_t bytes;            /* sum of their descriptor lengths, mod 2^64     */
  uint64_t last_seen;        /* max of `now` over the calls that counted or reset it */
  uint64_t reserved;         /* never read, never written                     */
};
#define PPTK_RW_ST_NOFLOW 0x80u    /* d_idx[i] >= rw_count: frame left untouched */

int pptk_flow_account_device(struct pptk_rx_ctx *ctx, const uint32_t *d_idx,
                             const uint16_t *d_len, uint32_t fixed_len, uint64_t n,
                             struct pptk_flow_stats *d_stats, uint64_t stats_count,
                             struct pptk_flow_stats *d_unmatched, uint64_t now, void *stream);
int pptk_flow_account_host(const uint32_t *idx, const uint16_t *len, uint32_t fixed_len,
                           uint64_t n, struct pptk_flow_stats *stats, uint64_t stats_count,
                           struct pptk_flow_stats *unmatched, uint64_t now);
int pptk_flow_stats_reset_device(struct pptk_rx_ctx *ctx, struct pptk_flow_stats *d_stats,
                                 uint64_t stats_count, const uint32_t *d_values, uint64_t count,
                                 uint64_t now, void *stream);
void pptk_flow_account_shape(uint32_t *segment_frames, uint32_t *lds_slots);
int pptk_flow_table_expire(struct pptk_flow_table *t, const struct pptk_flow_stats *stats,
                           uint64_t stats_count, uint64_t now, uint64_t idle,
                           uint32_t *expired_values, uint32_t cap);
int pptk_tx_rewrite_flow_device(struct pptk_rx_ctx *ctx, uint8_t *d_frames, const uint64_t *d_off,
                                const uint16_t *d_len, uint64_t stride, uint32_t fixed_len,
                                uint64_t n, const struct pptk_rewrite *d_rw, uint64_t rw_count,
                                const uint32_t *d_idx, uint8_t *d_status, void *stream);

/* Flow learning: a device report of the new flows in a batch.  The host
 * inserts flows and expires them, but the batches never leave device memory,
 * so it does not see the frame of an unknown flow arrive: the lookup gives it
 * PPTK_FLOW_NONE and status SUBJECT without HIT, and accounting adds it to
 * `unmatched`.  The reference learns per packet -- ldp/ldpswitch.c:125-208
 * port_put() adds an entry when its probe found none (:153-203) -- and a NAT
 * or SYN proxy on hashtable/ does the same for a first packet.  Here a kernel
 * turns the lookup's status bytes into a small array: one entry per new flow,
 * free of duplicates, in frame order, ready for pptk_flow_table_insert_recs.
 * No kernel inserts into the table or deletes from it: the device reports,
 * the host decides policy and inserts, sync uploads.  The gateway loop is
 *   rx -> pptk_flow_lookup_device -> pptk_flow_learn_device
 *      -> download hdr + `written` entries -> policy
 *      -> pptk_flow_table_insert_recs + stats_reset -> pptk_flow_table_sync.
 *
 * pptk_flow_learn_host is the CPU statement; the device call equals it byte
 * for byte.  Walk i = 0 .. n - 1.  Frame i is a candidate when status[i] ==
 * PPTK_FLOW_ST_SUBJECT exactly (a subject that did not hit); the status byte
 * is trusted, the record's flags are not re-tested.  Candidates are numbered
 * in index order and only the first max_candidates are considered; the rest
 * count in hdr.candidates and nowhere else, which bounds work and scratch
 * under a flood of new flows.  A map from flow_hash to the first considered
 * frame L that carried it decides the rest: a considered frame whose hash is
 * new is a leader; one whose hash is known and whose 37 key bytes (record
 * bytes 8..43 plus proto) equal L's adds 1 to L's packet count; one whose hash
 * is known but whose key differs is a leader of its own with count 1 and does
 * not enter the map (a true 64-bit collision: a hash match alone is never a
 * hit, as in the table).  The entries are the leaders in ascending frame
 * index; entry k is written only for k < cap: new_recs[k] = the leader's
 * record, all 64 bytes verbatim, first[k] = its frame index, packets[k] = its
 * count.  Entries at and past `written` are untouched and nothing is written
 * outside the arrays; hdr gets all four words.  Every value of flow_hash, 0
 * and 2^64 - 1 included, is an ordinary hash.  n = 0 writes a zero header
 * (where hdr is given) and launches no more than that; cap = 0 with null
 * outputs is legal, the call then only counts; first and packets are
 * nullable.
 *
 * -EINVAL: a null ctx (device call); null recs, status or hdr with n > 0;
 * null new_recs with cap > 0; n >= 2^32; max_candidates 0 or above 2^30; recs
 * or new_recs not 16-byte, hdr not 8-byte, first or packets not 4-byte
 * aligned; and, on the device call with n > 0, a scratch that is null, not
 * 256-byte aligned or smaller than pptk_flow_learn_scratch_bytes(n,
 * max_candidates) (0 for n = 0 or arguments the call would reject).  status
 * may have any alignment.  The host call returns -ENOMEM when its map cannot
 * be allocated.
 *
 * The device call clears what it needs of the scratch itself, is
 * asynchronous on `stream` (eight small launches ordered by the stream alone,
 * no host synchronisation) and must not share a scratch with a call in
 * flight on another stream.  Its cost follows n only through the status bytes
 * (1 B per frame); records are read for considered candidates only.
 * pptk_flow_learn_shape reports the built kernels: the frames of one
 * workgroup of the counting passes (block_frames) and the block counts the
 * scan's single workgroup takes per round (scan_width).  Results do not
 * depend on it.
 *
 * Out of scope: a policy (which new flows to admit), inserts by a kernel,
 * pptk_rx_rec32 input, and a report across batches (a flow learned from
 * batch b is unknown to the lookup until the host has inserted and synced). */
struct pptk_flow_learn_hdr {   /* 32 bytes, 8-byte aligned, in device memory */
  uint64_t candidates;         /* frames with status == SUBJECT (no HIT)            */
  uint64_t considered;         /* min(candidates, max_candidates)                   */
  uint64_t flows;              /* report entries the considered frames give         */
  uint64_t written;            /* min(flows, cap)                                   */
};
size_t pptk_flow_learn_scratch_bytes(uint64_t n, uint64_t max_candidates);
int pptk_flow_learn_device(struct pptk_rx_ctx *ctx, const struct pptk_rx_rec *d_recs,
                           const uint8_t *d_status, uint64_t n, uint64_t max_candidates,
                           struct pptk_rx_rec *d_new_recs, uint32_t *d_first,
                           uint32_t *d_packets, uint64_t cap,
                           struct pptk_flow_learn_hdr *d_hdr,
                           void *d_scratch, size_t scratch_bytes, void *stream);
int pptk_flow_learn_host(const struct pptk_rx_rec *recs, const uint8_t *status, uint64_t n,
                         uint64_t max_candidates, struct pptk_rx_rec *new_recs,
                         uint32_t *first, uint32_t *packets, uint64_t cap,
                         struct pptk_flow_learn_hdr *hdr);
void pptk_flow_learn_shape(uint32_t *block_frames, uint32_t *scan_width);

/* Egress dispatch: per-port tx lists from a batch in device memory.  Every
 * stage above ends with per-frame results in frame order; a forwarder finally
 * needs which frames leave through which port.  The reference ends its loop
 * with that step -- ldp/ldpswitch.c:276-318 appends a packet to the output
 * table of its port for a known destination, to every port's but the ingress
 * port's for an unknown one (:296-305), then calls ldp_out_inject once per port
 * (:311-318); ldpfwd.c and ldptunnel.c do the two-port form.  Here one call
 * turns a per-frame port code, or the flow index of pptk_flow_lookup_device
 * and a code per flow value, into one packed list of frame indices (and,
 * where asked for, their offsets and lengths) with a run per port:
 *   rx -> pptk_flow_lookup_device -> pptk_tx_dispatch_device(idx, flow_port,
 *      miss_code = PPTK_PORT_FLOOD) -> download ports -> per port p: inject
 *      out_off / out_len[start .. start + count).
 *
 * pptk_tx_dispatch_host is the CPU statement; the device call equals it byte
 * for byte.  Frame i is classified in this order.  (1) subject given and
 * subject[i] == 0: dropped.  (2) Its code: port[i] with `port` set; with
 * `idx` set miss_code where idx[i] == PPTK_FLOW_NONE, otherwise the frame is
 * bad where idx[i] >= flows (flow_port is not read for it), otherwise
 * flow_port[idx[i]].  (3) A code below nports is unicast to that port -- also
 * when that port is the frame's ingress port, as in the reference; such a
 * frame counts in hdr.hairpin.  PPTK_PORT_FLOOD makes a flood frame,
 * PPTK_PORT_DROP drops, any other code makes the frame bad.  Bad frames go
 * nowhere and count in hdr.bad, not in hdr.dropped.  The ingress port of
 * frame i is in_port ? in_port[i] : in_port_all; a value at or above nports
 * means "none", and a flood then reaches all nports ports.
 *
 * Port p's run is every i, ascending, that is unicast to p or is a flood
 * frame whose ingress port is not p: the order in which the reference's loop
 * fills port p's output table.  The runs lie back to back in port order:
 * ports[0].start == 0, ports[p + 1].start == ports[p].start + ports[p].count.
 * Entry g of the packed list is written only for g < cap: list[g] = i,
 * out_off[g] = off ? off[i] : i * stride, out_len[g] = len ? len[i] :
 * fixed_len (its low 16 bits).  With a cap below hdr.total every port before
 * the cut is complete and the cut port holds a prefix of its run; ports and
 * hdr are always complete, and `bytes` sums the frame lengths (len[i] or
 * fixed_len) of the whole run whatever cap is.  Nothing is written outside
 * the arrays or past `written`.  cap == 0 with a null list is legal, the call
 * then only counts; out_off and out_len are nullable.  n == 0 writes a zero
 * header and nports zero entries and launches no more than that.  A flood
 * with nports == 1 from port 0 reaches nobody and still counts in hdr.flood.
 * The padding members are ignored.
 *
 * -EINVAL: a null ctx (device call); a null d, ports or hdr; both or neither
 * of port / idx set with n > 0; idx without flow_port while flows > 0; a
 * miss_code that is not below nports, FLOOD or DROP; nports 0 or above
 * PPTK_PORT_MAX; n >= 2^32; a null list with cap > 0; idx or list not 4-byte,
 * off, out_off, ports or hdr not 8-byte, len or out_len not 2-byte aligned
 * (port, subject, in_port and flow_port may have any alignment); and, on the
 * device call with n > 0, a scratch that is null, not 256-byte aligned or
 * smaller than pptk_tx_dispatch_scratch_bytes(n, nports) (0 for n = 0 or
 * arguments the call would reject).
 *
 * The device call reads `d` before it returns (the struct itself is host
 * memory, its arrays device memory), clears what it needs of the scratch
 * itself, is asynchronous on `stream` (at most four launches ordered by the
 * stream alone, no host synchronisation) and must not share a scratch with a
 * call in flight on another stream.  The order of a run never depends on the
 * grid or on arrival: no atomic operation takes part in a position.
 * pptk_tx_dispatch_shape reports the built kernels: the frames of one
 * workgroup of the count and scatter passes (block_frames) and the block
 * counts a scan workgroup takes per round (scan_width).  Results do not
 * depend on it.
 *
 * Out of scope: a MAC-keyed table and MAC learning (the caller supplies the
 * code per frame, or per flow through the 5-tuple table); copying frame bytes
 * into per-port buffers (the lists describe frames in place; "Egress gather"
 * below packs them); VLAN-scoped
 * flooding or multicast groups beyond "all but ingress"; more than 64 ports;
 * carrying the fragmenter's d_out_src through (the caller dispatches the
 * slots as a batch of their own); a host ldp_packet[] form. */
#define PPTK_PORT_MAX   64u
#define PPTK_PORT_FLOOD 0xffu   /* every port but the frame's ingress port (ldpswitch.c:296-305) */
#define PPTK_PORT_DROP  0xfeu   /* no port */

struct pptk_dispatch_port {   /* 32 bytes, one per port, device memory */
  uint64_t start;             /* first entry of this port's run in the list      */
  uint64_t count;             /* entries of the run, whatever cap is             */
  uint64_t bytes;             /* sum of the frame lengths of the run             */
  uint64_t flooded;           /* entries of the run that come from flood frames  */
};
struct pptk_dispatch_hdr {    /* 64 bytes, 8-byte aligned */
  uint64_t total;             /* sum of count over the ports                     */
  uint64_t written;           /* min(total, cap)                                 */
  uint64_t unicast, flood, dropped, bad;   /* frames by class, sum == n          */
  uint64_t hairpin;           /* unicast frames whose port is their ingress port */
  uint64_t reserved;          /* 0 */
};
struct pptk_dispatch {        /* arguments, host and device call alike; 152 bytes */
  uint64_t n;
  const uint8_t *port;        /* per-frame code; exactly one of port / idx set   */
  const uint32_t *idx;        /* per-frame flow index (pptk_flow_lookup_device)  */
  const uint8_t *flow_port;   /* with idx: code per flow value, `flows` entries  */
  uint64_t flows;
  const uint8_t *subject;     /* nullable; 0 = frame is dropped                  */
  const uint8_t *in_port;     /* nullable per-frame ingress port                 */
  uint32_t in_port_all;       /* ingress port of every frame when in_port NULL   */
  uint32_t nports;            /* 1 .. PPTK_PORT_MAX                              */
  uint8_t miss_code;          /* with idx: code of a PPTK_FLOW_NONE frame        */
  uint8_t pad0[7];
  const uint64_t *off;        /* nullable: frame i lies at i * stride            */
  const uint16_t *len;        /* nullable: every frame is fixed_len long         */
  uint64_t stride;
  uint32_t fixed_len;
  uint32_t pad1;
  uint32_t *list;             /* frame indices, `cap` entries                    */
  uint64_t *out_off;          /* nullable: off of list[g]'s frame                */
  uint16_t *out_len;          /* nullable: len of list[g]'s frame                */
  uint64_t cap;
  struct pptk_dispatch_port *ports;   /* nports entries */
  struct pptk_dispatch_hdr *hdr;
};
size_t pptk_tx_dispatch_scratch_bytes(uint64_t n, uint32_t nports);
int pptk_tx_dispatch_device(struct pptk_rx_ctx *ctx, const struct pptk_dispatch *d,
                            void *d_scratch, size_t scratch_bytes, void *stream);
int pptk_tx_dispatch_host(const struct pptk_dispatch *d);
void pptk_tx_dispatch_shape(uint32_t *block_frames, uint32_t *scan_width);

/* Egress gather: each port's tx list packed into contiguous buffers.  The
 * dispatch above says which frames leave through which port, as entries that
 * name frames in place -- scattered over the whole batch, a flood frame named
 * by several runs.  The reference ends the same loop with the copy: per port,
 * ldp_out_inject copies every packet of the port's output table into the next
 * tx slot (ldp/ldpnetmap.c:68, ldp/ldpdpdk.c:256, called from
 * ldp/ldpswitch.c:311-318).  Here one call copies the frames of every run back
 * to back into `out`, one region per port, so that a caller whose NIC sits
 * behind the host downloads one range per port:
 *   rx -> pptk_flow_lookup_device -> pptk_tx_dispatch_device ->
 *      pptk_tx_gather_device(list, d_entries = &dispatch hdr.written, runs =
 *      dispatch ports) -> download ports -> per port p: one download of
 *      out[start, start + bytes) -> inject pk_off / pk_len of the run.
 *
 * pptk_tx_gather_host is the CPU statement; the device call equals it byte for
 * byte.  Considered entries: E = max_entries, or min(max_entries, *d_entries)
 * where d_entries is given (a device word on the device call, read on the
 * device: the call never synchronises with the host); with `runs` E is also
 * cut at the end of the last run, so every considered entry lies in a run.
 * Port p's entries are [runs[p].start, runs[p].start + runs[p].count) cut at
 * E; runs[].bytes and runs[].flooded are not read.  The runs must lie back to
 * back from 0, as dispatch writes them (runs[0].start == 0, runs[p + 1].start
 * == runs[p].start + runs[p].count, no sum wrapping); otherwise hdr.status =
 * PPTK_GATHER_ST_BADRUNS, every other word of hdr and of ports is 0, and
 * nothing else is written.  Null runs (nports == 1) make one region of every
 * entry.
 *
 * Entry g names frame i = list ? list[g] : g.  Its length is L = len ? len[i]
 * : fixed_len, its slot round_up(L, 16) bytes.  A bad entry (i >= n) has L = 0
 * and counts in hdr.bad; nothing of the source is read for it.  Region 0
 * starts at 0, region p + 1 at round_up(start_p + the slot bytes of all
 * considered entries of p, 256), whether or not they fit.  pk_off[g] is the
 * region start plus the slots of the run's earlier entries, pk_len[g] is L;
 * both are written for every considered entry and for no other.  hdr.need is
 * the end of the last region's slots.  Entry g is packed iff pk_off[g] + slot
 * <= out_cap; offsets never decrease in g, so the packed entries are a prefix
 * of hdr.packed entries, and ports[p].packed / ports[p].bytes count that
 * prefix inside each run.  For a packed entry out[pk_off, pk_off + L) holds
 * the frame's bytes and [L, slot) zeros.  No other byte of out is written:
 * not the padding between regions, nothing from an unpacked entry on, nothing
 * past out_cap.  Of the source nothing outside the aligned 16-byte chunks of
 * [frame, frame + L) is read.  A flood frame named by several entries is
 * copied once per entry.  out must not overlap the source batch (not
 * checked).  out null with out_cap 0 is legal, the call then only counts;
 * pk_off and pk_len are nullable.  max_entries == 0 writes a zero header and
 * nports zero port entries and launches no more than that (the runs are not
 * looked at).  The padding members are ignored.
 *
 * -EINVAL: a null ctx (device call), g, ports or hdr; nports 0 or above
 * PPTK_PORT_MAX, or runs null with nports != 1; a source batch no batch op
 * accepts (n > 0 with null frames, neither off nor stride while n > 1, or
 * fixed_len > 65535 without len); max_entries >= 2^32 or n >= 2^32; out null
 * with out_cap > 0, or out not 256-byte aligned; list not 4-byte, off,
 * pk_off, runs, ports, hdr or d_entries not 8-byte, len or pk_len not 2-byte
 * aligned; and, on the device call with max_entries > 0, a scratch that is
 * null, not 256-byte aligned or smaller than
 * pptk_tx_gather_scratch_bytes(max_entries, nports) (0 for max_entries = 0 or
 * arguments the call would reject).
 *
 * The device call reads `g` before it returns (the struct itself is host
 * memory, its arrays device memory), clears what it needs of the scratch
 * itself, is asynchronous on `stream` (launches ordered by the stream alone)
 * and must not share a scratch with a call in flight on another stream.  The
 * result is the same for any grid: no atomic operation takes part in an
 * offset, and every loop's trip count is a constant, a kernel argument or a
 * device value clamped by one.  pptk_tx_gather_shape reports the built
 * kernels: the entries of one workgroup of the count and copy passes
 * (block_entries) and the block sums a scan workgroup takes per round
 * (scan_width).  Results do not depend on it.
 *
 * Out of scope: headroom or a per-frame prepend in the slot; slot alignments
 * other than 16; a host ldp_packet[] form, or the download itself; writing
 * into netmap or DPDK rings; a MAC-keyed table; a gather straight from the
 * fragmenter's d_out_src. */
#define PPTK_GATHER_SLOT_ALIGN   16u    /* every packed frame starts at a multiple */
#define PPTK_GATHER_REGION_ALIGN 256u   /* every port's region starts at a multiple */
#define PPTK_GATHER_ST_BADRUNS   1u     /* hdr.status: runs not back to back from 0 */

struct pptk_gather_port {     /* 32 bytes, one per port, device memory */
  uint64_t start;             /* byte offset of the region in out, multiple of 256 */
  uint64_t bytes;             /* slot bytes of the run's packed entries            */
  uint64_t entries;           /* considered entries of the run                     */
  uint64_t packed;            /* of them packed (a prefix of the run)              */
};
struct pptk_gather_hdr {      /* 64 bytes, 8-byte aligned */
  uint64_t entries;           /* considered entries                                */
  uint64_t packed;            /* entries g < packed lie in out                     */
  uint64_t need;              /* out_cap at which every considered entry is packed */
  uint64_t bytes;             /* sum of ports[p].bytes                             */
  uint64_t frame_bytes;       /* sum of the frame lengths of the packed entries    */
  uint64_t bad;               /* considered entries with list[g] >= n              */
  uint64_t status;            /* 0 or PPTK_GATHER_ST_BADRUNS                       */
  uint64_t reserved;          /* 0 */
};
struct pptk_gather {          /* arguments, host and device call alike; 136 bytes */
  const uint8_t *frames;      /* the source batch, as every batch op takes it      */
  const uint64_t *off;        /* nullable: frame i lies at i * stride              */
  const uint16_t *len;        /* nullable: every frame is fixed_len long           */
  uint64_t stride;
  uint32_t fixed_len;
  uint32_t pad0;
  uint64_t n;                 /* frames of the batch                               */
  const uint32_t *list;       /* nullable: entry g is frame g                      */
  uint64_t max_entries;       /* host bound: sizes grids and scratch               */
  const uint64_t *d_entries;  /* nullable word, e.g. &dispatch hdr.written         */
  const struct pptk_dispatch_port *runs;   /* nullable: one region, nports == 1    */
  uint32_t nports;            /* 1 .. PPTK_PORT_MAX                                */
  uint32_t pad1;
  uint8_t *out;               /* nullable with out_cap 0: count only               */
  uint64_t out_cap;
  uint64_t *pk_off;           /* nullable, max_entries each                        */
  uint16_t *pk_len;
  struct pptk_gather_port *ports;   /* nports entries */
  struct pptk_gather_hdr *hdr;
};
size_t pptk_tx_gather_scratch_bytes(uint64_t max_entries, uint32_t nports);
int pptk_tx_gather_device(struct pptk_rx_ctx *ctx, const struct pptk_gather *g,
                          void *d_scratch, size_t scratch_bytes, void *stream);
int pptk_tx_gather_host(const struct pptk_gather *g);
void pptk_tx_gather_shape(uint32_t *block_entries, uint32_t *scan_width);

/* Tuning: force kernel variant `variant` (0 .. pptk_rx_variant_count()-1)
 * and/or memory-policy flags for every later batch of this context; -1
 * restores the automatic choice (variant by frame length and alignment).
 * flags: PPTK_RX_TUNE_NT_LOADS (non-temporal frame loads),
 * PPTK_RX_TUNE_NO_STAGING (store records per lane, not via LDS),
 * PPTK_RX_TUNE_NT_STORES (non-temporal record stores),
 * PPTK_RX_TUNE_SC1_STORES (write-through record stores),
 * PPTK_RX_TUNE_BLOCKED (each wavefront takes a contiguous block of tiles
 * instead of every nwaves-th tile), PPTK_RX_TUNE_PERMIT_PASSES (the rate
 * limiter's four-launch path instead of its fused one-launch path; a flags
 * word holding only this bit leaves the receive transform's memory policy
 * automatic).
 * Variants and flags change speed only: results are identical for every
 * setting on every input.  Any other flag bit is rejected with -EINVAL
 * (PPTK_RX_TUNE in the environment is masked to these bits). */
#define PPTK_RX_TUNE_NT_LOADS 0x1
#define PPTK_RX_TUNE_NO_STAGING 0x2
#define PPTK_RX_TUNE_NT_STORES 0x20
#define PPTK_RX_TUNE_SC1_STORES 0x40
#define PPTK_RX_TUNE_BLOCKED 0x100   /* contiguous tiles per wavefront */
#define PPTK_RX_TUNE_PERMIT_PASSES 0x400   /* rate limiter: four launches, not one */
int pptk_rx_set_tuning(struct pptk_rx_ctx *ctx, int variant, int flags);
int pptk_rx_variant_count(void);
/* The kernel variant the last device batch of this context launched (the
 * automatic or forced choice after eligibility checks; -1 before the first
 * batch).  Diagnostics for tests and benchmarks. */
int pptk_rx_last_variant(const struct pptk_rx_ctx *ctx);

/* Autotuning: run the batch (records are written, as by
 * pptk_rx_batch_device) with the automatic kernel variant and the shapes
 * interchangeable with it -- two warm-up rounds, then reps timed rounds of
 * one launch per shape, interleaved so that clock drift falls on all alike
 * -- and let later device batches of the same automatic variant and layout
 * (fixed-stride or offset-described) use the fastest median (another shape
 * must beat the automatic one by 1 % to replace it).  The best shape
 * depends on how expensive the record writes are (which follows where the
 * record buffer sits, see pptk_rx_place_records) and, for
 * offset-described batches, on the length mix (the candidates include the
 * kernel that bins each tile's frames by length into 4-, 8- and 16-lane
 * rounds, fastest on IMIX-like streams of mostly small frames);
 * results never change.  Synchronous; reps 1..100.
 * pptk_rx_set_tuning's forced variant still takes precedence. */
int pptk_rx_autotune(struct pptk_rx_ctx *ctx, const struct pptk_rx_dev_batch *batch, int reps,
                     void *stream);

/* ---- Multi-GPU (RCCL over xGMI) ------------------------------------------
 * Batches shard embarrassingly: GPU r of R runs pptk_rx_batch_device on its
 * own contiguous range of the batch (pptk_rx_shard_range) with d_hash set,
 * and pptk_rx_allgather_hash then gives every GPU the flow hash of every
 * frame (ncclAllGather of u64 over one communicator).  The reference scales
 * with one rx thread per queue (ldp/ldprecvmt.c:174-182); here one context
 * per GPU, driven by one process per GPU (pptk_rx_comm_uid +
 * pptk_rx_comm_create) or by one thread per GPU of a single process
 * (pptk_rx_comm_create_all).  The communicator belongs to its context and is
 * destroyed with it (or by pptk_rx_comm_destroy).
 *
 * Failure containment: the reference's queue threads share nothing, so one
 * failing thread never stalls the others; ranks of a collective do wait for
 * each other.  So no call here waits without a bound: creation gives up
 * after opts.comm_timeout_ms (-ETIMEDOUT, e.g. a rank that never joins),
 * pptk_rx_comm_sync waits for a stream with a deadline and surfaces RCCL's
 * asynchronous errors (a dead peer: -EIO), and pptk_rx_comm_abort lets any
 * thread cancel a communicator other threads are waiting on.  After
 * -ETIMEDOUT / -EIO from a gather or a sync, or an abort, the communicator
 * is dead (calls on it return -ECANCELED): destroy it and create a new one.
 * RCCL is loaded on first use; without it these calls return -ENOSYS. */
#define PPTK_RX_COMM_UID_BYTES 128

/* Number of visible GPUs (>= 0), or -EIO. */
int pptk_rx_device_count(void);

/* A new communicator id: made once by one rank and handed to every rank
 * through the application's own channel (a file, a socket, MPI). */
int pptk_rx_comm_uid(uint8_t uid[PPTK_RX_COMM_UID_BYTES]);

/* Join `ctx` (one context per GPU) to communicator `uid` as rank `rank` of
 * `nranks`.  Collective: blocks until every rank has called it, at most
 * opts.comm_timeout_ms (then -ETIMEDOUT and the context has no
 * communicator, so it may try again with a new uid).  -ECANCELED if
 * pptk_rx_comm_abort was called on the context while this ran, or before
 * it (a pending abort, consumed by this call).  -EAGAIN if kMaxAbandoned
 * (4) earlier creations of this process that gave up are still stuck inside
 * RCCL (a rank that never joined).  -EINVAL if the context already has a
 * communicator or a creation in progress. */
int pptk_rx_comm_create(struct pptk_rx_ctx *ctx, int nranks, int rank,
                        const uint8_t uid[PPTK_RX_COMM_UID_BYTES]);

/* Single process, one thread per GPU: one communicator over ctxs[0..n)
 * (each on a different device), rank i = ctxs[i].  Call from one thread;
 * afterwards each rx thread uses its own context concurrently.  Bounded by
 * ctxs[0]'s opts.comm_timeout_ms; an abort of any of the contexts cancels
 * it (-ECANCELED, as pptk_rx_comm_create); on any failure no context keeps
 * one. */
int pptk_rx_comm_create_all(struct pptk_rx_ctx *const *ctxs, int n);

/* Orderly teardown (flushes enqueued gathers, bounded; an abort if the
 * flush does not finish).  Also drops a pending abort.  The context may then
 * create a new one.  -EBUSY while the context's creation is in progress. */
int pptk_rx_comm_destroy(struct pptk_rx_ctx *ctx);

/* Cancel the context's communicator now, from any thread: RCCL's kernels
 * of pending gathers return (so their streams drain, with wrong gathered
 * data), waits in pptk_rx_comm_sync / pptk_rx_allgather_hash on it return
 * -ECANCELED, and so does every later call on it until
 * pptk_rx_comm_destroy.  A creation still in progress on the context
 * (pptk_rx_comm_create / _create_all) returns -ECANCELED promptly and keeps
 * nothing; on a context with no communicator yet the abort is kept pending
 * and cancels its next creation.  An rx thread that fails calls this on
 * every context of the job, so no sibling waits for a gather -- or a
 * creation -- it will never join (examples/rx_multigpu.c).  0 in every
 * case.  It must not race with pptk_rx_comm_destroy or pptk_rx_ctx_destroy
 * of the same context. */
int pptk_rx_comm_abort(struct pptk_rx_ctx *ctx);

/* Wait until everything enqueued on `stream` (gathers included) is done,
 * for at most timeout_ms (0 = opts.comm_timeout_ms), watching the
 * communicator for RCCL's asynchronous errors.  0: done.  -ETIMEDOUT: the
 * deadline passed (a peer never issued its part); -EIO: RCCL reported an
 * error (a peer died); in both cases the communicator is aborted, so the
 * stream drains.  -ECANCELED: it was aborted (pptk_rx_comm_abort).  Use it
 * instead of hipStreamSynchronize on a stream that carries gathers.
 * Without a communicator: a bounded stream wait (-ETIMEDOUT). */
int pptk_rx_comm_sync(struct pptk_rx_ctx *ctx, void *stream, uint32_t timeout_ms);

/* The context's communicator size and rank; -EINVAL without one. */
int pptk_rx_comm_info(const struct pptk_rx_ctx *ctx, int *nranks, int *rank);

/* Equal-shard policy for a batch of n frames over nranks GPUs: per_rank =
 * ceil(n / nranks); rank r owns frames [first, first + count) with first =
 * min(r * per_rank, n).  Every rank all-gathers per_rank hashes (the last
 * ranks' shards are padded), so the gathered array holds the flow hash of
 * global frame i at index i for every i < n. */
void pptk_rx_shard_range(uint64_t n, int nranks, int rank, uint64_t *first, uint64_t *count,
                         uint64_t *per_rank);

/* d_out[r * n + i] = d_hash[i] of rank r, for every rank r (n u64 per rank,
 * the same n on every rank; d_hash may be d_out + rank * n).  Asynchronous
 * on `stream`; collective: every rank calls it, in the same order relative
 * to its other collectives.  -EIO if an earlier gather failed
 * asynchronously, -ECANCELED on an aborted communicator, -ETIMEDOUT (and
 * the communicator aborted) if RCCL's enqueue -- the connection setup with
 * the peers at the first gather -- does not finish in opts.comm_timeout_ms.
 * Completion: pptk_rx_comm_sync. */
int pptk_rx_allgather_hash(struct pptk_rx_ctx *ctx, const uint64_t *d_hash, uint64_t n,
                           uint64_t *d_out, void *stream);

/* Two streams that split the chip's CUs between the batches and the
 * gather that overlaps them (no reference counterpart: the reference has no
 * device; this belongs with the collective above).  RCCL's all-gather
 * kernel needs a whole CU per block on gfx950 (512 threads, 37 KB of LDS,
 * 248 VGPRs), and the receive grid fills every CU (persistent for
 * fixed-stride batches, oversubscribed for offset-described ones and the
 * small-frame kernel), so at each batch boundary one kernel takes CUs the
 * other was sized for and the two run one after the other (DESIGN.md
 * section 8).  *coll_stream (for
 * pptk_rx_allgather_hash) may use `coll_cus` CUs -- the same number in
 * every shader engine of every XCC -- and *rx_stream (for the batches) the
 * rest; the context sizes its receive grids for the rest from now on, on
 * any stream, and the rate limiter's one-launch path
 * (pptk_rx_permit_keys_device) its grid too; launch only the collective on
 * *coll_stream.  coll_cus: a multiple of 4 x the device's XCC count (32 on an
 * MI355X), below its CU count; -EINVAL otherwise.
 *
 * Order: split first, then create the communicator.  A communicator created
 * on a split context runs at most coll_cus RCCL blocks (channels) per
 * collective (ncclConfig_t.maxCTAs), so that all of them are resident on the
 * CUs left to it at once; that cap is fixed at creation, so a split to a
 * different CU count while the context has a communicator (or a creation in
 * progress) returns -EBUSY.  A split to the count the context already holds
 * returns the same two streams.  coll_cus 0 (streams NULL allowed) gives the
 * context's grids the whole chip again; the streams stay valid.
 *
 * The streams belong to the context: pptk_rx_ctx_destroy destroys them,
 * after its communicator (a gather stream destroyed before the communicator
 * made later device-wide waits or the teardown hang).
 * pptk_rx_stream_destroy returns -EBUSY for a stream its context still holds,
 * 0 (and does nothing) for one its context has destroyed, and destroys any
 * other stream. */
int pptk_rx_stream_split(struct pptk_rx_ctx *ctx, int coll_cus, void **rx_stream,
                         void **coll_stream);
int pptk_rx_stream_destroy(void *stream);

/* Buffer placement.  What the memory charges for the record writes beside
 * the frame-read stream depends on where the frame buffer and the record
 * buffer sit physically: the same C1500 launch, same kernel, same bytes,
 * takes 4.15-4.3 ms or 4.5-5.1 ms depending on the frame buffer, the record
 * buffer, or the pair.  For long-lived rings, set up
 * once: allocate a few candidate buffers (any allocator; spread apart, e.g.
 * with a few GB allocated between them), frame candidates each holding the
 * same representative batch, and let this run the batch on every (frames,
 * records) pair -- `reps` timed launches after one warm-up, pairs
 * interleaved -- and return the fastest pair in *best_frames / *best_recs;
 * keep those, free the others.  The frame candidates replace b->d_frames
 * (offsets in b->d_off are relative to it, so one descriptor array serves
 * all), the record candidates b->d_recs (b->d_recs32 for a compact batch)
 * and receive the batch's records; the rest of `b` is used as given.
 * Synchronous; nframes 1..16, nrecs 1..64, nframes * nrecs <= 256, reps
 * 1..100.  ms (nullable) receives nframes * nrecs median launch times,
 * frames-major.  Freeing the candidates not kept makes the driver scrub that
 * memory in the background (~30 GB/s measured); batches beside the scrub
 * run up to 9 % slower, so a latency-sensitive ring starts after it. */
int pptk_rx_place_buffers(struct pptk_rx_ctx *ctx, const struct pptk_rx_dev_batch *b,
                          const uint8_t *const *d_frames, int nframes, void *const *d_recs,
                          int nrecs, int reps, int *best_frames, int *best_recs, float *ms,
                          void *stream);

/* The record buffer alone (the frames as given in b->d_frames): as
 * pptk_rx_place_buffers with one frame candidate; *best = the record
 * candidate's index, ms = ncand median times. */
int pptk_rx_place_records(struct pptk_rx_ctx *ctx, const struct pptk_rx_dev_batch *b,
                          void *const *d_cands, int ncand, int reps, int *best, float *ms,
                          void *stream);

/* ---- Device rings owned by the library -----------------------------------
 * The default way to get the device frame ring and record ring of a
 * long-lived rx queue (an LDP/netmap ring lives for the process, reference
 * ldp/ldpnetmap.c:163-185): the library allocates frame and record
 * candidates spread apart in HBM, fills every frame candidate with a
 * synthetic batch of the ring's geometry (fixed-stride IPv4/TCP frames of
 * probe_len bytes, as many as fit, at most nrec), runs the receive
 * transform on every (frames, records) pair as pptk_rx_place_buffers does,
 * keeps the fastest pair and frees everything else -- so an application
 * that takes its rings from here gets the placed pair without managing
 * candidates (placement measured: C1500 4.03 ms placed against 4.80 ms on a
 * plain allocation of the same box).  The frame ring's
 * contents after the call are the probe batch: the application writes its
 * frames over it.  Synchronous (uses `stream` for the probe).
 * frame_cands 1..8 (0 = 3), rec_cands 1..16 (0 = 8), reps 1..20 (0 = 3),
 * probe_len 64..1536 (0 = 1500); candidates beyond the first pair are
 * allocated only as far as budget_bytes (0: 60 % of the free device memory)
 * allows.  Calls for one device run one at a time (several rx queues of a
 * GPU, a context each, setting up their rings together: each probe runs
 * alone and sizes its candidates from what the earlier calls kept; give
 * each queue a budget so the first ones do not take the memory the later
 * ones need for their candidates).  Freeing the
 * candidates not kept makes the driver scrub that memory in the background
 * (~20-30 GB/s; batches beside it run up to 9 % slower): with
 * PPTK_RX_RING_SETTLE the call sleeps until it is over (settle_ms), else
 * freed_bytes says how much was freed.  -EINVAL for a bad spec, -ENOMEM if
 * not even one pair fits.  Release with pptk_rx_ring_free. */
#define PPTK_RX_RING_SETTLE 0x1
/* The queue's batches will also write the dense flow hashes (d_hash, the
 * multi-GPU gather's send slice): the probe batches write them too (into a
 * scratch buffer freed with the candidates), so the pair kept is the best
 * for all three write streams, not for the records alone. */
#define PPTK_RX_RING_PROBE_HASH 0x2
struct pptk_rx_ring_spec {
  uint64_t frame_bytes;   /* frame ring bytes (the ring stays readable 64 B past it) */
  uint64_t nrec;          /* records the record ring holds (<= 2^32 - 1) */
  uint32_t rec_bytes;     /* 64 (struct pptk_rx_rec) or 32 (struct pptk_rx_rec32) */
  uint32_t probe_len;     /* probe frame length, 0 = 1500 */
  uint32_t frame_cands;   /* 0 = 3 */
  uint32_t rec_cands;     /* 0 = 8 */
  uint32_t reps;          /* timed probe launches per pair, 0 = 3 */
  uint32_t flags;         /* PPTK_RX_RING_SETTLE | PPTK_RX_RING_PROBE_HASH */
  uint64_t budget_bytes;  /* device memory the call may hold at once (candidates
                             and spacers included), 0 = 60 % of the free memory */
  uint64_t reserved;      /* 0 */
};
struct pptk_rx_ring {
  uint8_t *d_frames;      /* frame_bytes (+ 64 readable) */
  void *d_recs;           /* nrec * rec_bytes */
  uint64_t frame_bytes;
  uint64_t nrec;
  uint32_t rec_bytes;
  int32_t device;         /* the context's device */
  uint32_t frame_cands;   /* candidates actually probed */
  uint32_t rec_cands;
  int32_t chosen_frames;  /* the pair kept (candidate indices) */
  int32_t chosen_recs;
  float chosen_ms;        /* probe median launch time on the pair kept */
  float first_ms;         /* ... on candidate pair (0, 0): a plain allocation */
  uint64_t probe_frames;  /* frames in the probe batch */
  uint64_t freed_bytes;   /* candidates and spacers freed */
  uint32_t settle_ms;     /* slept for the scrub (PPTK_RX_RING_SETTLE) */
  uint32_t reserved;
};
int pptk_rx_ring_alloc(struct pptk_rx_ctx *ctx, const struct pptk_rx_ring_spec *spec,
                       struct pptk_rx_ring *ring, void *stream);
/* Frees both rings (on ring->device; the context need not exist any more)
 * and zeroes *ring.  Every batch using them must have completed. */
int pptk_rx_ring_free(struct pptk_rx_ring *ring);

/* The multi-GPU gather buffers, placed by the library like the rings: the
 * two (double-buffered) destinations of pptk_rx_allgather_hash for this
 * rank, nranks * per_rank u64 each, zeroed.  Where they sit decides what the
 * gather's writes -- the kernel's own hashes into the rank's slice and the
 * (nranks - 1) shards the collective lands while the next batch streams --
 * cost beside the frame stream.  Candidate regions
 * (each holding both buffers) are allocated apart; `b` (this rank's batch:
 * frames, records, geometry; b->d_hash is replaced by each buffer's slice in
 * turn) runs ~300 ms to warm the clocks, then `reps` rounds over the
 * candidates, each launch followed, on a second stream, by a device copy of
 * the bytes the gather would land (beside the next launch, as in an rx loop);
 * the region whose launches have the lowest median kernel time is kept,
 * everything else freed.  Synchronous; uses
 * `stream`.  Call after the rings are placed (the probe runs on them) and
 * after the scrub of what their placement freed is over
 * (PPTK_RX_RING_SETTLE): batches beside the scrub run up to 20 % slower on
 * every candidate alike, which hides the differences the probe looks for.
 * cands 1..16 (0 = 8), reps 1..20 (0 = 5); candidates as far as
 * budget_bytes (0: 50 % of the free memory) allows.  b->n <= per_rank.
 * Release with pptk_rx_gather_free. */
struct pptk_rx_gather_spec {
  uint64_t per_rank;      /* hashes each rank gathers (pptk_rx_shard_range) */
  int32_t nranks;
  int32_t rank;
  uint32_t cands;         /* candidate regions, 0 = 8 */
  uint32_t reps;          /* rounds over the candidates (two timed batches each), 0 = 5 */
  uint32_t flags;         /* PPTK_RX_RING_SETTLE */
  uint32_t reserved;      /* 0 */
  uint64_t budget_bytes;  /* 0 = 50 % of the free memory */
};
struct pptk_rx_gather {
  uint64_t *d_out[2];     /* the two gather buffers; rank r's slice of each
                             starts at d_out[k] + r * per_rank */
  uint64_t per_rank;
  int32_t nranks;
  int32_t rank;
  int32_t device;
  uint32_t cands;         /* candidate regions probed */
  int32_t chosen;         /* the region kept */
  float chosen_ms;        /* median probe kernel ms on the region kept */
  float first_ms;         /* ... on candidate 0: a plain allocation */
  uint32_t settle_ms;
  uint64_t freed_bytes;
  float cand_ms[16];      /* median probe kernel ms of every candidate probed */
};
int pptk_rx_gather_alloc(struct pptk_rx_ctx *ctx, const struct pptk_rx_dev_batch *b,
                         const struct pptk_rx_gather_spec *spec, struct pptk_rx_gather *gather,
                         void *stream);
int pptk_rx_gather_free(struct pptk_rx_gather *gather);

/* Library / build identification for the loaders. */
const char *pptk_rx_version(void);

/* The layout revision of the structs in this header (pptk_rx_opts,
 * pptk_rx_dev_batch, pptk_rx_ring_spec, ...).  It changes whenever one of
 * them changes size or meaning (round 5 added pptk_rx_ring_spec.budget_bytes
 * and .reserved; round 6 is the first revision with this check): a caller
 * compares pptk_rx_abi() with the PPTK_RX_ABI it was compiled against before
 * passing any struct, so a caller built against an older header is detected
 * instead of read past its structs' end. */
#define PPTK_RX_ABI 6
int pptk_rx_abi(void);

#ifdef __cplusplus
}
#endif

#endif /* PPTK_RX_H */
