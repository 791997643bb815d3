/*
 * tunnel_asan.c -- pptk_tunnel_encap_host / pptk_tunnel_decap_host and the
 * header-construction setters of include/iphdr.h under
 * -fsanitize=address,undefined (tests/test_tunnel.py builds this file with
 * pptk_amd/csrc/host/tunnel.c and ipcksum.c and runs it as a program).  Every
 * frame and every output buffer is a heap block of exactly the size the
 * contract allows the function to touch, so a read past the frame or a write
 * past out_cap is reported.  The checks do not repeat the function's
 * arithmetic: the outer header verifies (ip_hdr_cksum_calc == 0), its fields
 * read back through the getters, the payload is the frame, and decap of the
 * result points back at it.  Exit status 0 = clean.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/wait.h>
#include <unistd.h>

#include "ipcksum.h"
#include "iphdr.h"
#include "pptk_rx.h"

static int failures;
#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      printf("%s:%d: %s\n", __FILE__, __LINE__, #c);                    \
      failures++;                                                       \
    }                                                                   \
  } while (0)

static uint32_t rnd_state = 4711;
static unsigned rnd(void)
{
  rnd_state = rnd_state * 1664525u + 1013904223u;
  return rnd_state >> 24;
}

static unsigned char *heap_copy(const unsigned char *p, size_t n)
{
  unsigned char *q = malloc(n ? n : 1);
  if (n)
    memcpy(q, p, n);
  return q;
}

static struct pptk_tunnel tunnel(unsigned k)
{
  struct pptk_tunnel t;
  unsigned i;
  memset(&t, 0, sizeof(t));
  for (i = 0; i < 6; ++i) {
    t.eth_dst[i] = (uint8_t)rnd();
    t.eth_src[i] = (uint8_t)rnd();
  }
  t.src = (rnd() << 24) | (rnd() << 16) | (rnd() << 8) | rnd();
  t.dst = k == 2 ? 0xffffffffu : ((rnd() << 24) | (rnd() << 8) | rnd());
  t.id = (uint16_t)(k == 2 ? 0xfffe : rnd() * 257u);
  t.ttl = (uint8_t)rnd();
  t.tos = (uint8_t)rnd();
  t.flags = k & 3u;
  return t;
}

static uint32_t up16(uint32_t x) { return (x + 15u) & ~15u; }

static void encap_case(uint32_t len, unsigned k, uint32_t seq, int exact_cap)
{
  const struct pptk_tunnel t = tunnel(k);
  const uint32_t tot = 38 + len, cap = exact_cap ? tot : up16(tot);
  unsigned char *f = malloc(len ? len : 1), *out = malloc(cap);
  uint16_t olen = 0xeeee;
  uint32_t st, i, in_off = 77;
  uint16_t in_len = 77;
  const unsigned char *ip = out + 14;

  for (i = 0; i < len; ++i)
    f[i] = (unsigned char)rnd();
  memset(out, 0xee, cap);
  st = pptk_tunnel_encap_host(f, len, &t, seq, out, cap, &olen);
  if (len < 14) {
    CHECK(st == PPTK_TUN_ST_RUNT && olen == 0 && out[0] == 0xee);
  } else if (tot > 65535) {
    CHECK(st == PPTK_TUN_ST_TOOBIG && olen == 0 && out[0] == 0xee && out[cap - 1] == 0xee);
  } else {
    CHECK(st == PPTK_TUN_ST_DONE && olen == tot);
    CHECK(memcmp(ether_const_dst(out), t.eth_dst, 6) == 0);
    CHECK(memcmp(ether_const_src(out), t.eth_src, 6) == 0);
    CHECK(ether_type(out) == ETHER_TYPE_IP);
    CHECK(ip_version(ip) == 4 && ip_hdr_len(ip) == 20 && ip[1] == t.tos);
    CHECK(ip_total_len(ip) == len + 24);
    CHECK(ip_id(ip) == (uint16_t)(t.id + ((t.flags & PPTK_TUN_ID_SEQ) ? seq : 0)));
    CHECK(!ip_dont_frag(ip) == !(t.flags & PPTK_TUN_DF));
    CHECK(!ip_more_frags(ip) && ip_frag_off(ip) == 0 && !ip_rsvd_bit(ip));
    CHECK(ip_ttl(ip) == t.ttl && ip_proto(ip) == 47);
    CHECK(ip_src(ip) == t.src && ip_dst(ip) == t.dst);
    CHECK(ip_hdr_cksum_calc(ip, 20) == 0);
    CHECK(out[34] == 0 && out[35] == 0 && out[36] == 0x65 && out[37] == 0x58);
    CHECK(memcmp(out + 38, f, len) == 0);
    for (i = tot; i < cap; ++i)
      CHECK(out[i] == 0);
    /* and back: an exact-size copy of the packet */
    {
      unsigned char *pkt = heap_copy(out, tot);
      st = pptk_tunnel_decap_host(pkt, tot, &in_off, &in_len);
      CHECK(st == (PPTK_DECAP_ST_IPV4 | PPTK_DECAP_ST_GRE | PPTK_DECAP_ST_OK));
      CHECK(in_off == 38 && in_len == len);
      free(pkt);
    }
    /* one byte short: NOROOM, nothing written */
    memset(out, 0xee, cap);
    olen = 0xeeee;
    st = pptk_tunnel_encap_host(f, len, &t, seq, out, tot - 1, &olen);
    CHECK(st == PPTK_TUN_ST_NOROOM && olen == 0);
    for (i = 0; i < cap; ++i)
      CHECK(out[i] == 0xee);
  }
  free(out);
  free(f);
}

static void encap_cases(void)
{
  static const uint32_t lens[] = {0, 1, 13, 14, 15, 16, 17, 25, 26, 27, 41, 42, 43, 60, 64,
                                  89, 90, 91, 1500, 1514, 9000, 65496, 65497, 65498, 65535};
  unsigned i, k;
  struct pptk_tunnel t = tunnel(0);
  unsigned char f[64] = {0}, out[112];
  uint16_t olen = 7;
  for (i = 0; i < sizeof(lens) / sizeof(*lens); ++i)
    for (k = 0; k < 4; ++k)
      encap_case(lens[i], k, k == 3 ? 0xffffffffu : 0x10000u * k + i, (int)((i + k) & 1));
  /* no tunnel or a malformed one: nothing read, nothing written; null out_len is fine */
  memset(out, 0xee, sizeof(out));
  CHECK(pptk_tunnel_encap_host(f, 64, NULL, 0, out, sizeof(out), &olen) == PPTK_TUN_ST_NOFLOW);
  CHECK(olen == 0);
  t.reserved = 1;
  CHECK(pptk_tunnel_encap_host(f, 64, &t, 0, out, sizeof(out), NULL) == PPTK_TUN_ST_BADTUN);
  t.reserved = 0;
  t.flags = 4;
  CHECK(pptk_tunnel_encap_host(f, 64, &t, 0, out, sizeof(out), NULL) == PPTK_TUN_ST_BADTUN);
  t.flags = 0;
  CHECK(pptk_tunnel_encap_host(NULL, 64, &t, 0, out, sizeof(out), NULL) == PPTK_TUN_ST_NOFLOW);
  CHECK(pptk_tunnel_encap_host(f, 64, &t, 0, NULL, sizeof(out), NULL) == PPTK_TUN_ST_NOFLOW);
  CHECK(pptk_tunnel_encap_host(NULL, 0, &t, 0, out, sizeof(out), NULL) == PPTK_TUN_ST_RUNT);
  CHECK(out[0] == 0xee && out[sizeof(out) - 1] == 0xee);
  CHECK(pptk_tunnel_encap_host(f, 64, &t, 0, out, sizeof(out), NULL) == PPTK_TUN_ST_DONE);
}

/* an outer packet around `inner_len` bytes, in a heap block of its length */
static unsigned char *make_outer(uint32_t inner_len, uint32_t ihl, int vlan, uint32_t pad,
                                 uint32_t *len)
{
  const uint32_t l2 = vlan ? 18 : 14, tl = ihl + 4 + inner_len;
  unsigned char *f = malloc(l2 + tl + pad), *ip = f + l2;
  uint32_t k;
  for (k = 0; k < l2 + tl + pad; ++k)
    f[k] = (unsigned char)rnd();
  if (vlan) {
    f[12] = 0x81; f[13] = 0x00;
    ether_set_type(f + 4, ETHER_TYPE_IP);
  } else {
    ether_set_type(f, ETHER_TYPE_IP);
  }
  ip_set_version(ip, 4);
  ip_set_hdr_len(ip, (uint8_t)ihl);
  ip_set_total_len(ip, (uint16_t)tl);
  ip[6] = 0; ip[7] = 0;
  ip_set_proto(ip, 47);
  ip_set_hdr_cksum_calc(ip, (uint16_t)ihl);
  memset(ip + ihl, 0, 2);
  hdr_set16n(ip + ihl + 2, 0x6558);
  *len = l2 + tl + pad;
  return f;
}

static void decap_cases(void)
{
  static const uint32_t inner[] = {0, 1, 14, 64, 1500, 65000};
  const uint32_t ok = PPTK_DECAP_ST_IPV4 | PPTK_DECAP_ST_GRE | PPTK_DECAP_ST_OK;
  unsigned i, v;
  uint32_t ihl, len, off, n;
  uint16_t il;
  for (i = 0; i < 6; ++i)
    for (ihl = 20; ihl <= 60; ihl += 20)
      for (v = 0; v < 2; ++v) {
        const uint32_t l2 = v ? 18 : 14;
        unsigned char *f = make_outer(inner[i], ihl, (int)v, (i * 5 + v) % 16, &len), *ip = f + l2;
        CHECK(pptk_tunnel_decap_host(f, len, &off, &il) == ok);
        CHECK(off == l2 + ihl + 4 && il == inner[i]);
        CHECK(pptk_tunnel_decap_host(f, len, NULL, NULL) == ok);
        /* every truncation below the outer packet's end: not a subject */
        for (n = 0; n < l2 + ihl + 4 + inner[i]; n += n < 80 ? 1 : 977) {
          unsigned char *g = heap_copy(f, n);
          off = il = 5;
          CHECK(pptk_tunnel_decap_host(g, n, &off, &il) == 0 && off == 0 && il == 0);
          free(g);
        }
        ip[ihl] = 0x20;   /* K flag */
        CHECK(pptk_tunnel_decap_host(f, len, &off, &il) ==
              (PPTK_DECAP_ST_IPV4 | PPTK_DECAP_ST_GRE | PPTK_DECAP_ST_GREOPT));
        CHECK(off == 0 && il == 0);
        ip[ihl + 3] = 0x59;
        ip[10] ^= 1;
        CHECK(pptk_tunnel_decap_host(f, len, &off, &il) ==
              (PPTK_DECAP_ST_IPV4 | PPTK_DECAP_ST_GRE | PPTK_DECAP_ST_GREOPT |
               PPTK_DECAP_ST_PTYPE | PPTK_DECAP_ST_BADCKSUM));
        ip[6] = 0x20;     /* MF */
        CHECK(pptk_tunnel_decap_host(f, len, &off, &il) ==
              (PPTK_DECAP_ST_IPV4 | PPTK_DECAP_ST_ISFRAG | PPTK_DECAP_ST_BADCKSUM));
        ip_set_proto(ip, 6);
        CHECK(pptk_tunnel_decap_host(f, len, &off, &il) == PPTK_DECAP_ST_IPV4);
        free(f);
      }
  /* tl - ihl = 3: the frame ends where the three bytes end */
  {
    unsigned char *f = make_outer(0, 24, 0, 0, &len), *ip = f + 14, *g;
    ip_set_total_len(ip, 27);
    ip_set_hdr_cksum_calc(ip, 24);
    g = heap_copy(f, 14 + 27);
    CHECK(pptk_tunnel_decap_host(g, 14 + 27, &off, &il) ==
          (PPTK_DECAP_ST_IPV4 | PPTK_DECAP_ST_SHORT));
    free(g);
    free(f);
  }
  CHECK(pptk_tunnel_decap_host(NULL, 0, &off, &il) == 0);
  CHECK(pptk_tunnel_decap_host(NULL, 64, &off, &il) == 0);
}

static int aborts(uint8_t hl)
{
  int ws = 0;
  const pid_t pid = fork();
  if (pid == 0) {
    unsigned char h[20] = {0x45};
    ip_set_hdr_len(h, hl);
    _exit(0);
  }
  return pid > 0 && waitpid(pid, &ws, 0) == pid && WIFSIGNALED(ws) && WTERMSIG(ws) == SIGABRT;
}

/* the six setters, on every value of the bytes they share */
static void setter_cases(void)
{
  unsigned b, v, k;
  for (b = 0; b < 256; ++b) {
    unsigned char h[34], ref[34];
    for (k = 0; k < 34; ++k)
      ref[k] = (unsigned char)(b + 13 * k);
    ref[14] = (unsigned char)b;
    for (v = 0; v < 256; v += 5) {
      memcpy(h, ref, 34);
      ip_set_version(h + 14, (uint8_t)v);   /* only the low four bits count */
      CHECK(h[14] == ((b & 0x0f) | ((v & 0xf) << 4)) && ip_version(h + 14) == (v & 0xf));
      h[14] = ref[14];
      CHECK(memcmp(h, ref, 34) == 0);
      ip_set_proto(h + 14, (uint8_t)v);
      CHECK(ip_proto(h + 14) == v);
      h[23] = ref[23];
      ether_set_type(h, (uint16_t)(v * 257u + b));
      CHECK(ether_type(h) == (uint16_t)(v * 257u + b));
      h[12] = ref[12]; h[13] = ref[13];
      CHECK(memcmp(h, ref, 34) == 0);
    }
    for (v = 0; v < 256; v += 4) {
      memcpy(h, ref, 34);
      ip_set_hdr_len(h + 14, (uint8_t)v);   /* (v / 4) & 15, as the reference */
      CHECK(h[14] == ((b & 0xf0) | ((v / 4) & 0xf)));
      h[14] = ref[14];
      CHECK(memcmp(h, ref, 34) == 0);
    }
    CHECK((unsigned char *)ether_dst(ref) == ref && (unsigned char *)ether_src(ref) == ref + 6);
  }
  CHECK(aborts(21) && aborts(22) && aborts(23) && aborts(255) && !aborts(20) && !aborts(60));
}

int main(void)
{
  encap_cases();
  decap_cases();
  setter_cases();
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("tunnel ok\n");
  return 0;
}
