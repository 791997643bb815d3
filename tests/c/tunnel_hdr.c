/*
 * tunnel_hdr.c -- builds a GRE tunnel's 38-byte outer header with nothing but
 * the kept setters of include/iphdr.h, the way an application that keeps a
 * header template per tunnel does: the constant fields once (make_template),
 * total length and checksum for every packet (finish_for).  Prints the header
 * in hex; tests/test_tunnel.py compares it with pptk_tunnel_encap_host's and
 * with the NumPy restatement's.
 *
 *   tunnel_hdr <inner frame length> <df 0|1> <id>
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ipcksum.h"
#include "iphdr.h"

#define GRE_HDR_LEN 4u
#define GRE_PTYPE_TEB 0x6558u
#define IP_PROTO_GRE 47u
#define OUTER_LEN (ETHER_HDR_LEN + IP_HDR_MINLEN + GRE_HDR_LEN)

struct endpoint {
  unsigned char mac[6];
  uint32_t addr;   /* host order */
};

/* the same endpoints as the tunnel entry the test hands to the host function */
static const struct endpoint local = {{0x02, 0x10, 0x20, 0x30, 0x40, 0x50}, 0x0a000001u};
static const struct endpoint remote = {{0x02, 0xaa, 0xbb, 0xcc, 0xdd, 0xee}, 0x0a000002u};

static void make_template(unsigned char *hdr, int df, uint16_t ident)
{
  unsigned char *outer_ip = ether_payload(hdr), *gre_words;

  memset(hdr, 0, OUTER_LEN);
  memcpy(ether_src(hdr), local.mac, sizeof(local.mac));
  memcpy(ether_dst(hdr), remote.mac, sizeof(remote.mac));
  ether_set_type(hdr, ETHER_TYPE_IP);

  ip_set_version(outer_ip, 4);
  ip_set_hdr_len(outer_ip, IP_HDR_MINLEN);
  ip_set_proto(outer_ip, IP_PROTO_GRE);
  ip_set_ttl(outer_ip, 64);
  ip_set_src(outer_ip, local.addr);
  ip_set_dst(outer_ip, remote.addr);
  ip_set_id(outer_ip, ident);
  ip_set_dont_frag(outer_ip, df);

  /* flags and version word stays 0; the protocol type follows it */
  gre_words = ip_payload(outer_ip);
  hdr_set16n(gre_words + 2, GRE_PTYPE_TEB);
}

static void finish_for(unsigned char *hdr, unsigned long inner_len)
{
  void *outer_ip = ether_payload(hdr);
  ip_set_total_len(outer_ip, (uint16_t)(IP_HDR_MINLEN + GRE_HDR_LEN + inner_len));
  ip_set_hdr_cksum_calc(outer_ip, IP_HDR_MINLEN);
}

int main(int argc, char **argv)
{
  unsigned char hdr[OUTER_LEN];
  unsigned k;

  if (argc != 4)
    return 2;
  make_template(hdr, atoi(argv[2]) != 0, (uint16_t)strtoul(argv[3], NULL, 0));
  finish_for(hdr, strtoul(argv[1], NULL, 0));
  for (k = 0; k < OUTER_LEN; ++k)
    printf("%02x", hdr[k]);
  printf("\n");
  return 0;
}
