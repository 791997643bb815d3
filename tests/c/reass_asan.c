/*
 * reass_asan.c -- pptk_ip_reass_host under -fsanitize=address,undefined
 * (tests/test_reass.py builds this file with pptk_amd/csrc/host/ipreass.c and
 * ipcksum.c and runs it as a program).  The frames of a case lie back to back
 * in a heap block of exactly their size and the slots in a block that ends
 * where the contract lets the last write end, so a read past the last frame
 * or a write past a slot's rounded-up length is reported.  The checks are
 * independent of the function's own arithmetic: every slot verifies
 * (ip_hdr_cksum_calc == 0), carries the leader's header bytes outside the
 * rewritten fields, offset 0 and MF clear, and the original payload.  The
 * records are made here, as the receive transform would make them, and then
 * made to lie.  Exit status 0 = clean.
 */
#include <errno.h>
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
      printf("%s:%d: %s\n", __FILE__, __LINE__, #c);                    \
      failures++;                                                       \
    }                                                                   \
  } while (0)

static uint32_t rnd_state = 4242;
static unsigned rnd(void)
{
  rnd_state = rnd_state * 1664525u + 1013904223u;
  return rnd_state >> 24;
}

#define MAXF 80
struct batch {
  unsigned char *buf;
  size_t size;
  uint64_t off[MAXF];
  uint16_t len[MAXF];
  struct pptk_rx_rec recs[MAXF];
  struct pptk_rx_frag frag[MAXF];
  uint32_t n;
};

static uint32_t up16(uint32_t x) { return (x + 15u) & ~15u; }

/* append one fragment: Ethernet (+ tag) + ihl header bytes + dl payload bytes
 * taken from data + off, and the records the receive transform would write */
static void add_frag(struct batch *b, int vlan, uint32_t ihl, uint16_t ident, uint32_t off,
                     uint32_t dl, int mf, const unsigned char *data)
{
  const uint32_t l2 = vlan ? 18 : 14, len = l2 + ihl + dl, i = b->n++;
  unsigned char *f, *ip;
  uint32_t k;
  b->buf = realloc(b->buf, b->size + len);
  f = b->buf + b->size;
  ip = f + l2;
  for (k = 0; k < l2 + ihl; ++k)
    f[k] = (unsigned char)rnd();
  if (vlan) {
    f[12] = 0x81; f[13] = 0x00; f[16] = 0x08; f[17] = 0x00;
  } else {
    f[12] = 0x08; f[13] = 0x00;
  }
  ip[0] = (unsigned char)(0x40 | (ihl / 4));
  ip_set_total_len(ip, (uint16_t)(ihl + dl));
  ip_set_id(ip, ident);
  ip[6] = 0x40; ip[7] = 0;   /* DF stays through the rewrite */
  ip_set_frag_off(ip, (uint16_t)off);
  ip_set_more_frags(ip, mf);
  ip[9] = 17;
  memcpy(ip + 12, "\x0a\x00\x00\x01\xc0\xa8\x00\x01", 8);
  ip_set_hdr_cksum_calc(ip, (uint16_t)ihl);
  memcpy(ip + ihl, data + off, dl);
  b->off[i] = b->size;
  b->len[i] = (uint16_t)len;
  b->size += len;
  memset(&b->recs[i], 0, sizeof(b->recs[i]));
  memset(&b->frag[i], 0, sizeof(b->frag[i]));
  memcpy(b->recs[i].src, ip + 12, 4);
  memcpy(b->recs[i].dst, ip + 16, 4);
  b->recs[i].l3_off = (uint8_t)l2;
  b->recs[i].proto = 17;
  b->recs[i].flags = PPTK_RX_F_PARSED | PPTK_RX_F_IP_OK | PPTK_RX_F_FRAGMENT;
  b->frag[i].ident = ident;
  b->frag[i].frag_off = (uint16_t)off;
  b->frag[i].data_len = (uint16_t)dl;
  b->frag[i].next_hdr = 17;
  b->frag[i].flags = (uint8_t)(PPTK_RX_FRAG_IS | (mf ? PPTK_RX_FRAG_MF : 0));
}

struct result {
  unsigned char *out;
  uint16_t out_len[MAXF];
  struct pptk_reass_dgram rep[MAXF];
  uint32_t dgram[MAXF];
  uint8_t fstatus[MAXF];
  struct pptk_reass_hdr hdr;
  int rc;
};

/* run with an output block of exactly `outsz` bytes */
static void run(const struct batch *b, struct result *r, uint64_t stride, uint64_t cap,
                size_t outsz)
{
  r->out = aligned_alloc(16, up16((uint32_t)(outsz ? outsz : 16)));
  memset(r->out, 0xee, outsz);
  memset(r->rep, 0xee, sizeof(r->rep));
  r->rc = pptk_ip_reass_host(b->buf, b->off, b->len, 0, 0, b->n, b->recs, b->frag, MAXF, r->out,
                             stride, cap, r->out_len, r->rep, MAXF, r->dgram, r->fstatus,
                             &r->hdr);
}

static const unsigned perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1},
                                     {2, 1, 0}};

/* three fragments in every order, every l2 / ihl mix, an odd last payload */
static void complete_cases(void)
{
  static const uint32_t ihls[] = {20, 24, 60};
  unsigned p, h, v, k;
  unsigned char data[200];
  for (k = 0; k < sizeof(data); ++k)
    data[k] = (unsigned char)rnd();
  for (p = 0; p < 6; ++p)
    for (h = 0; h < 3; ++h)
      for (v = 0; v < 2; ++v) {
        const uint32_t offs[3] = {0, 64, 128}, dls[3] = {64, 64, 37 + p};
        const uint32_t total = 128 + dls[2];
        struct batch b = {0};
        struct result r;
        uint32_t l2, ihl, flen;
        const unsigned char *lead, *s, *ip;
        for (k = 0; k < 3; ++k) {
          const unsigned j = perms[p][k];
          add_frag(&b, (int)((v + k) & 1), ihls[(h + k) % 3], 77, offs[j], dls[j], j < 2, data);
        }
        l2 = b.recs[0].l3_off;
        ihl = ihls[h % 3];
        flen = l2 + ihl + total;
        run(&b, &r, 512, 1, up16(flen));
        CHECK(r.rc == 0 && r.hdr.candidates == 3 && r.hdr.dgrams == 1 && r.hdr.written == 1);
        CHECK(r.rep[0].status == (PPTK_REASS_DG_COMPLETE | PPTK_REASS_DG_WRITTEN));
        CHECK(r.rep[0].first == 0 && r.rep[0].slot == 0 && r.rep[0].frags == 3);
        CHECK(r.rep[0].out_len == flen && r.out_len[0] == flen);
        for (k = 0; k < 3; ++k)
          CHECK(r.dgram[k] == 0 && r.fstatus[k] == (PPTK_REASS_FST_FRAG | PPTK_REASS_FST_MEMBER |
                                                    PPTK_REASS_FST_DONE));
        lead = b.buf;
        s = r.out;
        ip = s + l2;
        CHECK(memcmp(s, lead, l2 + 2) == 0 && memcmp(ip + 4, lead + l2 + 4, 2) == 0);
        CHECK(memcmp(ip + 8, lead + l2 + 8, 2) == 0);
        CHECK(memcmp(ip + 12, lead + l2 + 12, ihl - 12) == 0);
        CHECK(ip_total_len(ip) == ihl + total && ip_frag_off(ip) == 0 && !ip_more_frags(ip));
        CHECK(ip_dont_frag(ip) && ip_hdr_cksum_calc(ip, (uint16_t)ihl) == 0);
        CHECK(memcmp(ip + ihl, data, total) == 0);
        for (k = flen; k < up16(flen); ++k)
          CHECK(s[k] == 0);
        free(r.out);
        /* no slot: NOROOM, nothing written */
        run(&b, &r, 512, 0, 0);
        CHECK(r.rc == 0 && r.hdr.written == 0 && r.hdr.complete == 1);
        CHECK(r.rep[0].status == (PPTK_REASS_DG_COMPLETE | PPTK_REASS_DG_NOROOM));
        CHECK(r.fstatus[0] == (PPTK_REASS_FST_FRAG | PPTK_REASS_FST_MEMBER));
        free(r.out);
        /* a stride one chunk too small: TOOBIG */
        run(&b, &r, up16(flen) - 16, 1, 0);
        CHECK(r.rep[0].status == (PPTK_REASS_DG_COMPLETE | PPTK_REASS_DG_TOOBIG));
        CHECK(r.rep[0].out_len == flen && r.rep[0].slot == 0xffffffffu);
        free(r.out);
        free(b.buf);
      }
}

static void verdict_cases(void)
{
  unsigned char data[1024];
  struct batch b = {0};
  struct result r;
  unsigned k;
  for (k = 0; k < sizeof(data); ++k)
    data[k] = (unsigned char)rnd();
  /* 65 fragments of 8 bytes */
  for (k = 0; k < 65; ++k)
    add_frag(&b, 0, 20, 1, 8 * k, 8, k < 64, data);
  run(&b, &r, 608, 1, 0);
  CHECK(r.rep[0].status == PPTK_REASS_DG_TOOMANY && r.rep[0].frags == 65 && r.hdr.written == 0);
  free(r.out);
  b.n = 64;   /* without the last one: INCOMPLETE */
  run(&b, &r, 608, 1, 0);
  CHECK(r.rep[0].status == PPTK_REASS_DG_INCOMPLETE && r.rep[0].frags == 64);
  free(r.out);
  free(b.buf);
  /* a hole, a duplicate, a partial overlap, two lasts: four datagrams */
  memset(&b, 0, sizeof(b));
  add_frag(&b, 0, 20, 10, 0, 16, 1, data);
  add_frag(&b, 0, 20, 10, 32, 16, 0, data);
  add_frag(&b, 0, 20, 11, 0, 16, 1, data);
  add_frag(&b, 0, 20, 11, 0, 16, 1, data);
  add_frag(&b, 0, 20, 11, 16, 5, 0, data);
  add_frag(&b, 1, 24, 12, 0, 24, 1, data);
  add_frag(&b, 0, 20, 12, 16, 16, 0, data);
  add_frag(&b, 0, 20, 13, 0, 16, 1, data);
  add_frag(&b, 0, 20, 13, 16, 8, 0, data);
  add_frag(&b, 0, 20, 13, 16, 9, 0, data);
  run(&b, &r, 608, 4, 0);
  CHECK(r.rc == 0 && r.hdr.dgrams == 4 && r.hdr.complete == 0 && r.hdr.written == 0);
  CHECK(r.rep[0].status == PPTK_REASS_DG_INCOMPLETE && r.rep[1].status == PPTK_REASS_DG_OVERLAP);
  CHECK(r.rep[2].status == PPTK_REASS_DG_OVERLAP && r.rep[3].status == PPTK_REASS_DG_OVERLAP);
  CHECK(r.rep[1].first == 2 && r.rep[2].first == 5 && r.rep[3].first == 7);
  free(r.out);
  free(b.buf);
}

/* records that lie about a frame at the very end of the block */
static void lying_records(void)
{
  unsigned char data[64] = {0};
  struct batch b = {0};
  struct result r;
  add_frag(&b, 0, 20, 5, 0, 16, 1, data);
  add_frag(&b, 0, 20, 5, 16, 16, 0, data);
  b.frag[1].data_len = 17;               /* one byte past the frame */
  run(&b, &r, 608, 1, 0);
  CHECK(r.fstatus[1] == (PPTK_REASS_FST_FRAG | PPTK_REASS_FST_BADFRAG) && r.hdr.candidates == 1);
  CHECK(r.rep[0].status == PPTK_REASS_DG_INCOMPLETE && r.dgram[1] == 0xffffffffu);
  free(r.out);
  b.frag[1].data_len = 16;
  b.recs[1].l3_off = 200;                /* not 14 or 18: frame[200] is not read */
  run(&b, &r, 608, 1, 0);
  CHECK(r.fstatus[1] == (PPTK_REASS_FST_FRAG | PPTK_REASS_FST_BADFRAG));
  free(r.out);
  b.recs[1].l3_off = 18;                 /* the header reaches two bytes further */
  run(&b, &r, 608, 1, 0);
  CHECK(r.fstatus[1] & PPTK_REASS_FST_BADFRAG);
  free(r.out);
  b.recs[1].l3_off = 14;
  b.len[1] = 14;                         /* len <= l3: frame[l3] is outside */
  b.buf = realloc(b.buf, b.off[1] + 14);
  run(&b, &r, 608, 1, 0);
  CHECK(r.fstatus[1] == (PPTK_REASS_FST_FRAG | PPTK_REASS_FST_BADFRAG));
  free(r.out);
  b.recs[0].ip_cksum = 0x1234;
  b.frag[0].frag_off = 65528;
  run(&b, &r, 608, 1, 0);
  CHECK(r.fstatus[0] == (PPTK_REASS_FST_FRAG | PPTK_REASS_FST_BADCKSUM | PPTK_REASS_FST_BADFRAG));
  CHECK(r.hdr.candidates == 0 && r.hdr.dgrams == 0);
  free(r.out);
  free(b.buf);
}

static void einval(void)
{
  unsigned char data[32] = {0};
  struct batch b = {0};
  struct result r;
  add_frag(&b, 0, 20, 5, 0, 16, 1, data);
  run(&b, &r, 608, 1, 0);
  CHECK(r.rc == 0);
#define CALL(frames, n, maxc, out, stride, cap, hdr)                                        \
  pptk_ip_reass_host(frames, b.off, b.len, 0, 0, n, b.recs, b.frag, maxc, out, stride, cap, \
                     r.out_len, r.rep, MAXF, r.dgram, r.fstatus, hdr)
  CHECK(CALL(NULL, 1, 1, r.out, 608, 1, &r.hdr) == -EINVAL);
  CHECK(CALL(b.buf, 1, 0, r.out, 608, 1, &r.hdr) == -EINVAL);
  CHECK(CALL(b.buf, 1, (1u << 24) + 1, r.out, 608, 1, &r.hdr) == -EINVAL);
  CHECK(CALL(b.buf, (1u << 24) + 1, 1, r.out, 608, 1, &r.hdr) == -EINVAL);
  CHECK(CALL(b.buf, 1, 1, r.out + 4, 608, 1, &r.hdr) == -EINVAL);
  CHECK(CALL(b.buf, 1, 1, r.out, 600, 1, &r.hdr) == -EINVAL);
  CHECK(CALL(b.buf, 1, 1, NULL, 608, 1, &r.hdr) == -EINVAL);
  CHECK(CALL(b.buf, 1, 1, r.out, 608, 1, NULL) == -EINVAL);
  r.hdr.candidates = 9;
  CHECK(CALL(NULL, 0, 1, NULL, 608, 0, &r.hdr) == 0 && r.hdr.candidates == 0);
  free(r.out);
  free(b.buf);
}

int main(void)
{
  complete_cases();
  verdict_cases();
  lying_records();
  einval();
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("reass ok\n");
  return 0;
}
