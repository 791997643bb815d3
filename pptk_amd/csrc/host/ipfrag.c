/*
 * ipfrag.c -- pptk_ip_fragment_host: IPv4 fragmentation of one frame to an
 * egress MTU, the reference's fragment4() (ipfrag/ipfrag.c:11-123) with the
 * plan "as few fragments as possible" and verdicts instead of abort()s.  It
 * is also the CPU statement of pptk_ip_fragment_device's contract
 * (include/pptk_rx.h): the subject test repeats the receive transform's
 * structural IPv4 parse, everything after it is the reference's sequence of
 * iphdr.h / ipcksum.h calls.
 */
#include <errno.h>
#include <string.h>

#include "ipcksum.h"
#include "iphdr.h"
#include "outer_ipv4.h"
#include "pptk_rx.h"

int pptk_ip_fragment_host(const void *frame, uint32_t len, uint32_t mtu, uint8_t *out,
                          uint64_t out_stride, uint32_t out_cap, uint16_t *out_len,
                          uint8_t *status)
{
  const unsigned char *f = (const unsigned char *)frame;
  const void *ip;
  uint32_t l2, ihl, tl, datamax, per, count, j;
  uint8_t st;

  if ((!frame && len) || !out || !out_len || !status || mtu < 68 || mtu > 65535 ||
      out_stride % 16 != 0 || out_stride < ((18u + mtu + 15u) & ~15u))
    return -EINVAL;
  *status = 0;
  if (!pptk_outer_ipv4(f, len, &l2, &ihl, &tl))
    return 0;
  ip = f + l2;

  st = PPTK_FRAG_ST_IPV4;
  if (tl <= mtu) {
    *status = st | PPTK_FRAG_ST_FITS;
    return 0;
  }
  /* fragment4's abort conditions, ipfrag.c:42-61 */
  if (ip_dont_frag(ip))
    st |= PPTK_FRAG_ST_DF;
  if (ip_more_frags(ip) || ip_frag_off(ip))
    st |= PPTK_FRAG_ST_ISFRAG;
  if (ip_hdr_cksum_calc(ip, (uint16_t)ihl) != 0)
    st |= PPTK_FRAG_ST_BADCKSUM;
  if (st != PPTK_FRAG_ST_IPV4) {
    *status = st;
    return 0;
  }
  st |= PPTK_FRAG_ST_DONE;
  datamax = tl - ihl;
  per = (mtu - ihl) & ~7u;
  count = (datamax + per - 1) / per;
  if (count > out_cap) {
    *status = st | PPTK_FRAG_ST_NOROOM;
    return (int)count;
  }
  for (j = 0; j < count; ++j) {
    /* ipfrag.c:106-121 */
    const uint32_t datastart = j * per;
    const uint32_t datalen = datamax - datastart < per ? datamax - datastart : per;
    const uint32_t flen = l2 + ihl + datalen;
    unsigned char *slot = out + (uint64_t)j * out_stride;
    void *ip2 = slot + l2;
    memcpy(slot, f, l2 + ihl);
    ip_set_frag_off(ip2, (uint16_t)datastart);
    ip_set_more_frags(ip2, datastart + datalen < datamax);
    ip_set_total_len(ip2, (uint16_t)(ihl + datalen));
    ip_set_hdr_cksum_calc(ip2, (uint16_t)ihl);
    memcpy(ip_payload(ip2), (const unsigned char *)ip_const_payload(ip) + datastart, datalen);
    memset(slot + flen, 0, (16u - flen % 16u) % 16u);
    out_len[j] = (uint16_t)flen;
  }
  *status = st;
  return (int)count;
}
