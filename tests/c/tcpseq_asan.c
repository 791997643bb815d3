/*
 * tcpseq_asan.c -- pptk_tcp_seq_translate_hdr under
 * -fsanitize=address,undefined (tests/test_seqxlate.py builds this file with
 * pptk_amd/csrc/host/tcpseq.c and tcpopt.c and runs it as a program).  Every
 * segment is a heap block of exactly seglen bytes, so a read or write at or
 * past seglen is reported.  The expected bytes come from the kept functions
 * of include/ipcksum.h called one by one, in the contract's order, on a
 * padded copy whose bytes behind the options are random: the results must
 * not depend on them.  Exit status 0 = clean.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ipcksum.h"
#include "iphdr.h"
#include "pptk_rx.h"

static int failures;
#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      printf("%s:%d: %s (case %d)\n", __FILE__, __LINE__, #c, cur);     \
      failures++;                                                       \
    }                                                                   \
  } while (0)

static int cur;
static uint32_t rnd_state = 4242;
static unsigned rnd(void)
{
  rnd_state = rnd_state * 1664525u + 1013904223u;
  return rnd_state >> 24;
}
static uint32_t rnd32(void)
{
  return (uint32_t)rnd() << 24 | (uint32_t)rnd() << 16 | (uint32_t)rnd() << 8 | rnd();
}

/* a random option list of at most 40 bytes: NOPs, timestamps, SACK options
 * with 0-4 blocks, length bytes 0 / 1 / too long, unknown kinds, EOL */
static size_t make_opts(unsigned char *o)
{
  size_t n = 0, want = 4 * (rnd() % 11), k;
  while (n < want) {
    const unsigned c = rnd() % 100;
    unsigned char tmp[40];
    size_t l = 0;
    if (c < 30) {
      tmp[l++] = 1;
    } else if (c < 50) {
      tmp[l++] = 8;
      tmp[l++] = 10;
      for (k = 0; k < 8; k++)
        tmp[l++] = (unsigned char)rnd();
    } else if (c < 80) {
      const unsigned blocks = rnd() % 5;
      tmp[l++] = 5;
      tmp[l++] = (unsigned char)(2 + 8 * blocks);
      for (k = 0; k < 8 * blocks; k++)
        tmp[l++] = (unsigned char)rnd();
    } else if (c < 88) {
      tmp[l++] = (rnd() & 1) ? 5 : 8;
      tmp[l++] = (unsigned char)(rnd() % 3 == 0 ? 40 + rnd() % 20 : rnd() % 2);
    } else if (c < 95) {
      tmp[l++] = (unsigned char)(2 + rnd() % 250);
      tmp[l++] = (unsigned char)(rnd() % 6);
    } else {
      tmp[l++] = 0;
    }
    for (k = 0; k < l && n < want; k++)   /* the last option may be cut */
      o[n++] = tmp[k];
  }
  return n;
}

/* the contract, from the kept functions one by one */
static uint32_t expected(unsigned char *w, uint32_t seglen, const struct pptk_seqxlate *x)
{
  struct sack_ts_headers h;
  uint32_t st = PPTK_SEQ_ST_TCP;
  size_t end;
  if (seglen < 20)
    return PPTK_SEQ_ST_BADOPT;
  end = tcp_data_offset(w);
  if (end < 20 || end > seglen)
    return PPTK_SEQ_ST_BADOPT;
  if (x->ops & PPTK_SEQ_SEQ) {
    tcp_set_seq_number_cksum_update(w, 0, tcp_seq_number(w) + x->seq_add);
    st |= PPTK_SEQ_ST_SEQ;
  }
  if ((x->ops & PPTK_SEQ_ACK) && (w[13] & 0x10)) {
    tcp_set_ack_number_cksum_update(w, 0, tcp_ack_number(w) + x->ack_add);
    st |= PPTK_SEQ_ST_ACK;
  }
  if (x->ops & PPTK_SEQ_SACK) {
    tcp_find_sack_ts_headers(w, &h);
    tcp_adjust_sack_cksum_update_2(w, &h, x->sack_add);
    if (h.sackoff)
      st |= PPTK_SEQ_ST_SACK;
  }
  if (x->ops & PPTK_SEQ_TSVAL) {
    tcp_find_sack_ts_headers(w, &h);
    tcp_adjust_tsval_cksum_update(w, &h, x->tsval_add);
    if (h.tsoff)
      st |= PPTK_SEQ_ST_TS;
  }
  if (x->ops & PPTK_SEQ_TSECHO) {
    tcp_find_sack_ts_headers(w, &h);
    tcp_adjust_tsecho_cksum_update(w, &h, x->tsecho_add);
    if (h.tsoff)
      st |= PPTK_SEQ_ST_TS;
  }
  if (x->ops & PPTK_SEQ_SACK_OFF) {
    size_t sl = 0;
    int al = 0;
    void *s = tcp_find_sack_header(w, &sl, &al);
    if (s) {
      tcp_disable_sack_cksum_update(w, s, sl, al);
      st |= PPTK_SEQ_ST_SACK_OFF;
    }
  }
  return st;
}

int main(void)
{
  int written = 0, bad = 0, tight = 0;
  for (cur = 0; cur < 200000; cur++) {
    unsigned char hdr[64], pad[128], *seg;
    struct pptk_seqxlate x;
    const size_t no = make_opts(hdr + 20);
    size_t end = 20 + no, k;
    uint32_t seglen, st, want;
    for (k = 0; k < 20; k++)
      hdr[k] = (unsigned char)rnd();
    hdr[12] = (unsigned char)((end / 4) << 4 | (rnd() & 15));
    if (rnd() % 16 == 0)   /* any data offset, below 5 words and past the segment too */
      hdr[12] = (unsigned char)rnd();
    /* half of the segments end with their options */
    seglen = (uint32_t)end + ((rnd() & 1) ? 0 : rnd() % 8);
    if (rnd() % 32 == 0)
      seglen = rnd() % 24;   /* short segments, 0 included */
    if (seglen > sizeof(hdr))
      seglen = sizeof(hdr);
    x.ops = rnd() % 4 == 0 ? 0x3f : rnd() & 0x3f;
    x.seq_add = rnd32();
    x.ack_add = rnd32();
    x.sack_add = rnd() % 8 ? rnd32() : 0;
    x.tsval_add = rnd() % 8 ? rnd32() : 0xffffffffu;
    x.tsecho_add = rnd32();
    /* the segment, exactly seglen bytes on the heap */
    seg = malloc(seglen ? seglen : 1);
    for (k = end; k < sizeof(hdr); k++)
      hdr[k] = (unsigned char)rnd();
    memcpy(seg, hdr, seglen);
    /* the padded copy: the segment, then random bytes */
    memcpy(pad, hdr, seglen);
    for (k = seglen; k < sizeof(pad); k++)
      pad[k] = (unsigned char)rnd();
    want = expected(pad, seglen, &x);
    st = pptk_tcp_seq_translate_hdr(seg, seglen, &x);
    CHECK(st == want);
    if (st & PPTK_SEQ_ST_BADOPT) {
      CHECK(st == PPTK_SEQ_ST_BADOPT);
      CHECK(memcmp(seg, hdr, seglen) == 0);
      bad++;
    } else {
      end = tcp_data_offset(hdr);
      CHECK(memcmp(seg, pad, end) == 0);
      CHECK(memcmp(seg + end, hdr + end, seglen - end) == 0);   /* payload stays */
      written += memcmp(seg, hdr, end) != 0;
      tight += end == seglen;
    }
    free(seg);
  }
  CHECK(written > 50000 && bad > 5000 && tight > 50000);
  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("tcpseq ok: %d written, %d bad option areas, %d ending with the options\n", written, bad,
         tight);
  return 0;
}
