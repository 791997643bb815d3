/*
 * ipfrag_asan.c -- pptk_ip_fragment_host and the fragmentation setters of
 * include/iphdr.h under -fsanitize=address,undefined (tests/test_fragment.py
 * builds this file with pptk_amd/csrc/host/ipfrag.c and ipcksum.c and runs
 * it as a program).  Every frame and every output buffer is a heap block of
 * exactly the size the contract allows the function to touch, so a read past
 * the frame or a write past a slot's rounded-up length is reported.  The
 * checks are independent of the function's own arithmetic: every fragment
 * verifies (ip_hdr_cksum_calc == 0), carries the frame's header bytes
 * outside the rewritten fields, the offsets tile the payload and the
 * payloads concatenate to the original.  Exit status 0 = clean.
 */
#include <errno.h>
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

static uint32_t rnd_state = 12345;
static unsigned rnd(void)
{
  rnd_state = rnd_state * 1664525u + 1013904223u;
  return rnd_state >> 24;
}

/* Ethernet (+ tag) + IPv4 with ihl bytes of header + payload + padding, in a
 * heap block of exactly its length */
static unsigned char *make_frame(uint32_t tl, uint32_t ihl, int vlan, unsigned flags6,
                                 uint32_t pad, int badck, uint32_t *len)
{
  const uint32_t l2 = vlan ? 18 : 14;
  unsigned char *f = malloc(l2 + tl + pad ? l2 + tl + pad : 1), *ip = f + l2;
  uint32_t k;
  for (k = 0; k < l2 + tl + pad; ++k)
    f[k] = (unsigned char)rnd();
  if (vlan) {
    f[12] = 0x81; f[13] = 0x00; f[16] = 0x08; f[17] = 0x00;
  } else {
    f[12] = 0x08; f[13] = 0x00;
  }
  ip[0] = (unsigned char)(0x40 | (ihl / 4));
  ip_set_total_len(ip, (uint16_t)tl);
  ip[6] = (unsigned char)flags6;
  ip[7] = 0;
  ip_set_hdr_cksum_calc(ip, (uint16_t)ihl);
  if (badck)
    ip[10] ^= 0x40;
  *len = l2 + tl + pad;
  return f;
}

static uint32_t up16(uint32_t x) { return (x + 15u) & ~15u; }

/* one frame, one mtu: run, then check what came out */
static void run_case(uint32_t tl, uint32_t ihl, int vlan, unsigned flags6, uint32_t pad,
                     int badck, uint32_t mtu, unsigned want_status)
{
  const uint32_t l2 = vlan ? 18 : 14, stride = up16(18 + mtu);
  uint32_t len, j, pos = 0;
  unsigned char *f = make_frame(tl, ihl, vlan, flags6, pad, badck, &len);
  const uint32_t per = (mtu - ihl) & ~7u, datamax = tl - ihl;
  const uint32_t want = (want_status & PPTK_FRAG_ST_DONE) ? (datamax + per - 1) / per : 0;
  uint8_t st = 0xee;
  /* the last slot may be written up to its length rounded up to 16 only */
  const uint32_t lastlen = want ? l2 + ihl + datamax - (want - 1) * per : 0;
  const size_t outsz = want ? (size_t)(want - 1) * stride + up16(lastlen) : 1;
  unsigned char *out = malloc(outsz);
  uint16_t *olen = malloc(sizeof(uint16_t) * (want ? want : 1));
  int rc;
  memset(out, 0xee, outsz);
  rc = pptk_ip_fragment_host(f, len, mtu, out, stride, want, olen, &st);
  CHECK(rc == (int)want);
  CHECK(st == want_status);
  for (j = 0; j < want; ++j) {
    const unsigned char *s = out + (size_t)j * stride, *ip = s + l2;
    const uint32_t dl = datamax - pos < per ? datamax - pos : per, flen = l2 + ihl + dl;
    uint32_t k;
    CHECK(olen[j] == flen);
    CHECK(memcmp(s, f, l2 + 2) == 0);                       /* L2, version, tos */
    CHECK(memcmp(ip + 4, f + l2 + 4, 2) == 0);              /* id */
    CHECK(memcmp(ip + 8, f + l2 + 8, 2) == 0);              /* ttl, proto */
    CHECK(memcmp(ip + 12, f + l2 + 12, ihl - 12) == 0);     /* addresses, options */
    CHECK(ip_total_len(ip) == ihl + dl);
    CHECK(ip_frag_off(ip) == pos);
    CHECK(!ip_more_frags(ip) == (pos + dl == datamax));
    CHECK(!ip_dont_frag(ip));
    CHECK(ip_rsvd_bit(ip) == (int)(flags6 & 0x80));
    CHECK(ip_hdr_cksum_calc(ip, (uint16_t)ihl) == 0);
    CHECK(memcmp(ip + ihl, f + l2 + ihl + pos, dl) == 0);
    for (k = flen; k < up16(flen); ++k)
      CHECK(s[k] == 0);
    if (j + 1 < want)
      for (k = up16(flen); k < stride; ++k)
        CHECK(s[k] == 0xee);
    pos += dl;
  }
  CHECK(want == 0 || pos == datamax);
  if (want > 1) {   /* one slot short: NOROOM, nothing written */
    unsigned char guard[1] = {0xee};
    st = 0;
    rc = pptk_ip_fragment_host(f, len, mtu, guard, stride, want - 1, olen, &st);
    CHECK(rc == (int)want && st == (want_status | PPTK_FRAG_ST_NOROOM) && guard[0] == 0xee);
  }
  free(olen);
  free(out);
  free(f);
}

static void fragment_cases(void)
{
  static const uint32_t mtus[] = {68, 576, 1280, 1500};
  static const uint32_t ihls[] = {20, 24, 40, 60};
  const unsigned done = PPTK_FRAG_ST_IPV4 | PPTK_FRAG_ST_DONE;
  unsigned m, h, e;
  for (m = 0; m < 4; ++m)
    for (h = 0; h < 4; ++h) {
      const uint32_t mtu = mtus[m], ihl = ihls[h], per = (mtu - ihl) & ~7u;
      static const uint32_t extra[] = {0, 1, 7, 8};
      run_case(mtu, ihl, h & 1, 0, h, 0, mtu, PPTK_FRAG_ST_IPV4 | PPTK_FRAG_ST_FITS);
      run_case(mtu + 1, ihl, h & 1, 0, 0, 0, mtu, done);
      for (e = 0; e < 4; ++e) {
        run_case(ihl + per + extra[e], ihl, (int)(e & 1), 0, 2 * e + 1, 0, mtu,
                 ihl + per + extra[e] <= mtu ? PPTK_FRAG_ST_IPV4 | PPTK_FRAG_ST_FITS : done);
        run_case(ihl + 2 * per + extra[e], ihl, (int)(~e & 1), 0x80, 15 - e, 0, mtu, done);
      }
    }
  run_case(1500, 60, 0, 0, 0, 0, 68, done);      /* 180 fragments of 8 bytes */
  run_case(9000, 20, 1, 0, 3, 0, 1500, done);
  run_case(65521, 20, 0, 0, 0, 0, 576, done);
  /* the conditions under which fragment4 aborts, alone and together */
  run_case(1600, 20, 0, 0x40, 0, 0, 1500, PPTK_FRAG_ST_IPV4 | PPTK_FRAG_ST_DF);
  run_case(1600, 20, 0, 0x20, 0, 0, 1500, PPTK_FRAG_ST_IPV4 | PPTK_FRAG_ST_ISFRAG);
  run_case(1600, 24, 1, 0x01, 0, 0, 1500, PPTK_FRAG_ST_IPV4 | PPTK_FRAG_ST_ISFRAG);
  run_case(1600, 20, 0, 0, 0, 1, 1500, PPTK_FRAG_ST_IPV4 | PPTK_FRAG_ST_BADCKSUM);
  run_case(1600, 20, 0, 0x60, 0, 1, 1500,
           PPTK_FRAG_ST_IPV4 | PPTK_FRAG_ST_DF | PPTK_FRAG_ST_ISFRAG | PPTK_FRAG_ST_BADCKSUM);
  run_case(600, 20, 0, 0x40, 0, 1, 1500, PPTK_FRAG_ST_IPV4 | PPTK_FRAG_ST_FITS);
}

static void non_subjects_and_einval(void)
{
  uint32_t len, n;
  unsigned char *f = make_frame(1400, 20, 0, 0, 0, 0, &len);
  unsigned char out[1] = {0xee};
  uint16_t olen[1];
  uint8_t st;
  /* every truncation of a frame is MALFORMED or a runt: status 0, no write;
   * each runs on its own exact-size copy */
  for (n = 0; n < len; n += n < 64 ? 1 : 97) {
    unsigned char *g = malloc(n ? n : 1);
    memcpy(g, f, n);
    st = 0xee;
    CHECK(pptk_ip_fragment_host(g, n, 576, out, 608, 0, olen, &st) == 0 && st == 0);
    free(g);
  }
  f[12] = 0x86; f[13] = 0xdd;   /* IPv6 ethertype */
  st = 0xee;
  CHECK(pptk_ip_fragment_host(f, len, 576, out, 608, 0, olen, &st) == 0 && st == 0);
  f[12] = 0x08; f[13] = 0x06;   /* ARP */
  CHECK(pptk_ip_fragment_host(f, len, 576, out, 608, 0, olen, &st) == 0 && st == 0);
  f[12] = 0x08; f[13] = 0x00;
  f[14] = 0x55;                 /* version 5 */
  CHECK(pptk_ip_fragment_host(f, len, 576, out, 608, 0, olen, &st) == 0 && st == 0);
  f[14] = 0x44;                 /* ihl 16 */
  CHECK(pptk_ip_fragment_host(f, len, 576, out, 608, 0, olen, &st) == 0 && st == 0);
  f[14] = 0x45;
  CHECK(pptk_ip_fragment_host(NULL, 0, 576, out, 608, 0, olen, &st) == 0 && st == 0);
  st = 0xee;
  CHECK(pptk_ip_fragment_host(NULL, 64, 576, out, 608, 0, olen, &st) == -EINVAL);
  CHECK(pptk_ip_fragment_host(f, len, 67, out, 608, 0, olen, &st) == -EINVAL);
  CHECK(pptk_ip_fragment_host(f, len, 65536, out, 65568, 0, olen, &st) == -EINVAL);
  CHECK(pptk_ip_fragment_host(f, len, 576, out, 592, 0, olen, &st) == -EINVAL);   /* < 608 */
  CHECK(pptk_ip_fragment_host(f, len, 576, out, 609, 0, olen, &st) == -EINVAL);   /* % 16 */
  CHECK(pptk_ip_fragment_host(f, len, 576, NULL, 608, 0, olen, &st) == -EINVAL);
  CHECK(pptk_ip_fragment_host(f, len, 576, out, 608, 0, NULL, &st) == -EINVAL);
  CHECK(pptk_ip_fragment_host(f, len, 576, out, 608, 0, olen, NULL) == -EINVAL);
  CHECK(st == 0xee && out[0] == 0xee);
  free(f);
}

static int aborts(uint16_t off)
{
  int ws = 0;
  const pid_t pid = fork();
  if (pid == 0) {
    unsigned char h[20] = {0x45};
    ip_set_frag_off(h, off);
    _exit(0);
  }
  return pid > 0 && waitpid(pid, &ws, 0) == pid && WIFSIGNALED(ws) && WTERMSIG(ws) == SIGABRT;
}

/* the setters, on every value of byte 6 (three flag bits, five offset bits) */
static void setter_cases(void)
{
  unsigned b6, bit, off;
  for (b6 = 0; b6 < 256; ++b6) {
    unsigned char h[24], ref[24];
    unsigned k;
    for (k = 0; k < 24; ++k)
      ref[k] = (unsigned char)(0x45 + 7 * k);
    ref[6] = (unsigned char)b6;
    CHECK(!!ip_rsvd_bit(ref) == !!(b6 & 0x80) && !!ip_dont_frag(ref) == !!(b6 & 0x40) &&
          !!ip_more_frags(ref) == !!(b6 & 0x20));
    for (bit = 0; bit < 3; ++bit) {   /* 0 and any non-zero int */
      const int v = bit == 2 ? 0x100 : (int)bit;
      memcpy(h, ref, 24);
      ip_set_more_frags(h, v);
      CHECK(h[6] == ((b6 & ~0x20u) | (v ? 0x20u : 0u)));
      h[6] = ref[6];
      ip_set_dont_frag(h, v);
      CHECK(h[6] == ((b6 & ~0x40u) | (v ? 0x40u : 0u)));
      h[6] = ref[6];
      ip_set_rsvd_bit(h, v);
      CHECK(h[6] == ((b6 & ~0x80u) | (v ? 0x80u : 0u)));
      h[6] = ref[6];
      CHECK(memcmp(h, ref, 24) == 0);
    }
    for (off = 0; off < 65536; off += 8 * 251) {
      memcpy(h, ref, 24);
      ip_set_frag_off(h, (uint16_t)off);
      CHECK(ip_frag_off(h) == off && (h[6] & 0xe0) == (b6 & 0xe0));
      h[6] = ref[6]; h[7] = ref[7];
      CHECK(memcmp(h, ref, 24) == 0);
    }
    memcpy(h, ref, 24);
    ip_set_frag_off(h, 65528);
    CHECK(ip_frag_off(h) == 65528 && h[7] == 0xff && (h[6] & 0x1f) == 0x1f);
    memcpy(h, ref, 24);
    ip_set_total_len(h, (uint16_t)(b6 * 257u));
    ip_set_id(h, (uint16_t)(b6 * 255u + 1));
    CHECK(ip_total_len(h) == (uint16_t)(b6 * 257u) && ip_id(h) == (uint16_t)(b6 * 255u + 1));
    h[2] = ref[2]; h[3] = ref[3]; h[4] = ref[4]; h[5] = ref[5];
    CHECK(memcmp(h, ref, 24) == 0);
    ref[0] = (unsigned char)(0x40 | (5 + b6 % 11));
    CHECK((unsigned char *)ip_payload(ref) == ref + 4 * (5 + b6 % 11));
  }
  CHECK(aborts(4) && aborts(12) && aborts(65535) && !aborts(8));
}

int main(void)
{
  fragment_cases();
  non_subjects_and_einval();
  setter_cases();
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("ipfrag ok\n");
  return 0;
}
