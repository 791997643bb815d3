/*
 * outer_ipv4.h -- the outer IPv4 subject test of the host statements that take
 * a whole frame (ipfrag.c, tunnel.c); copy16.h outer_ipv4 is its device form.
 * It is the receive transform's structural parse: one optional 802.1Q tag,
 * IPv4, version, header and total length consistent with the frame.
 */
#pragma once
#include <stdint.h>

#include "iphdr.h"

/* 1 and *l2, *ihl, *tl when the len bytes at f are a subject, else 0 */
static inline int pptk_outer_ipv4(const unsigned char *f, uint32_t len, uint32_t *l2,
                                  uint32_t *ihl, uint32_t *tl)
{
  const void *ip;
  uint16_t et;

  *l2 = ETHER_HDR_LEN;
  if (len < ETHER_HDR_LEN || len > 65535)
    return 0;
  et = ether_type(f);
  if (et == 0x8100) {
    if (len < 18)
      return 0;
    et = hdr_get16n(f + 16);
    *l2 = 18;
  }
  if (et != ETHER_TYPE_IP || len < *l2 + IP_HDR_MINLEN)
    return 0;
  ip = f + *l2;
  *ihl = ip_hdr_len(ip);
  *tl = ip_total_len(ip);
  return ip_version(ip) == 4 && *ihl >= IP_HDR_MINLEN && *tl >= *ihl && *l2 + *tl <= len;
}
