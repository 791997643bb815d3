/*
 * tunnel.c -- pptk_tunnel_encap_host / pptk_tunnel_decap_host: the GRE
 * tunnel gateway of the reference's ldp/ldptunnel.c on one frame.  Encap is
 * the reference's sequence of iphdr.h / ipcksum.h calls (template :29-46, per
 * packet :126-128) with verdicts for the frames it cannot take; decap is the
 * strip of :155-158 behind the checks a receiver needs.  Both are the CPU
 * statement of the device calls' contract (include/pptk_rx.h).
 */
#include <string.h>

#include "ipcksum.h"
#include "iphdr.h"
#include "outer_ipv4.h"
#include "pptk_rx.h"

#define GRE_HDR_LEN 4u
#define GRE_PTYPE_TEB 0x6558u
#define IP_PROTO_GRE 47u

uint32_t pptk_tunnel_encap_host(const void *frame, uint32_t len, const struct pptk_tunnel *t,
                                uint32_t seq, uint8_t *out, uint64_t out_cap,
                                uint16_t *out_len)
{
  uint32_t st = 0, tot;
  uint64_t end;
  void *ip, *gre;

  if (out_len)
    *out_len = 0;
  if (!t || !out || (!frame && len >= ETHER_HDR_LEN))
    return PPTK_TUN_ST_NOFLOW;
  if (t->reserved || (t->flags & ~(PPTK_TUN_DF | PPTK_TUN_ID_SEQ)))
    return PPTK_TUN_ST_BADTUN;
  if (len < ETHER_HDR_LEN)
    return PPTK_TUN_ST_RUNT;
  if (len > 65535u - PPTK_TUN_HDR_LEN)
    st |= PPTK_TUN_ST_TOOBIG;
  if ((uint64_t)PPTK_TUN_HDR_LEN + len > out_cap)
    st |= PPTK_TUN_ST_NOROOM;
  if (st)
    return st;
  tot = PPTK_TUN_HDR_LEN + len;

  /* ldptunnel.c:29-46 */
  memset(out, 0, PPTK_TUN_HDR_LEN);
  memcpy(ether_dst(out), t->eth_dst, 6);
  memcpy(ether_src(out), t->eth_src, 6);
  ether_set_type(out, ETHER_TYPE_IP);
  ip = ether_payload(out);
  ip_set_version(ip, 4);
  ip_set_hdr_len(ip, IP_HDR_MINLEN);
  ((unsigned char *)ip)[1] = t->tos;
  ip_set_dont_frag(ip, (t->flags & PPTK_TUN_DF) != 0);
  ip_set_id(ip, (uint16_t)(t->id + ((t->flags & PPTK_TUN_ID_SEQ) ? seq : 0u)));
  ip_set_ttl(ip, t->ttl);
  ip_set_proto(ip, IP_PROTO_GRE);
  ip_set_src(ip, t->src);
  ip_set_dst(ip, t->dst);
  gre = ip_payload(ip);
  hdr_set16n((unsigned char *)gre + 2, GRE_PTYPE_TEB);
  /* :126-128 */
  ip_set_total_len(ip, (uint16_t)(len + GRE_HDR_LEN + IP_HDR_MINLEN));
  ip_set_hdr_cksum_calc(ip, IP_HDR_MINLEN);

  memcpy(out + PPTK_TUN_HDR_LEN, frame, len);
  end = ((uint64_t)tot + 15u) & ~(uint64_t)15u;
  if (end > out_cap)
    end = out_cap;
  memset(out + tot, 0, (size_t)(end - tot));
  if (out_len)
    *out_len = (uint16_t)tot;
  return PPTK_TUN_ST_DONE;
}

uint32_t pptk_tunnel_decap_host(const void *frame, uint32_t len, uint32_t *in_off,
                                uint16_t *in_len)
{
  const unsigned char *f = (const unsigned char *)frame;
  const unsigned char *ip, *gre;
  uint32_t l2, ihl, tl, st;

  if (in_off)
    *in_off = 0;
  if (in_len)
    *in_len = 0;
  if (!f || !pptk_outer_ipv4(f, len, &l2, &ihl, &tl))
    return 0;
  ip = f + l2;
  st = PPTK_DECAP_ST_IPV4;
  if (ip_proto(ip) != IP_PROTO_GRE)
    return st;

  if (ip_more_frags(ip) || ip_frag_off(ip))
    st |= PPTK_DECAP_ST_ISFRAG;
  if (ip_hdr_cksum_calc(ip, (uint16_t)ihl) != 0)
    st |= PPTK_DECAP_ST_BADCKSUM;
  if (st & PPTK_DECAP_ST_ISFRAG)
    return st;
  if (tl - ihl < GRE_HDR_LEN)
    return st | PPTK_DECAP_ST_SHORT;
  st |= PPTK_DECAP_ST_GRE;
  gre = (const unsigned char *)ip_const_payload(ip);
  if (hdr_get16n(gre) != 0)
    st |= PPTK_DECAP_ST_GREOPT;
  if (hdr_get16n(gre + 2) != GRE_PTYPE_TEB)
    st |= PPTK_DECAP_ST_PTYPE;
  if (st & (PPTK_DECAP_ST_BADCKSUM | PPTK_DECAP_ST_GREOPT | PPTK_DECAP_ST_PTYPE))
    return st;
  if (in_off)
    *in_off = l2 + ihl + GRE_HDR_LEN;
  if (in_len)
    *in_len = (uint16_t)(tl - ihl - GRE_HDR_LEN);
  return st | PPTK_DECAP_ST_OK;
}
