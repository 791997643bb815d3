/*
 * flow_learn_asan.c -- pptk_flow_learn_host (pptk_amd/csrc/host/flowlearn.c)
 * as a program of its own, for -fsanitize=address,undefined: every array is
 * a heap block of exactly the size the contract allows the call to touch, so
 * that a write past `written` entries or a read past n is a sanitizer report,
 * and every result is compared with a quadratic restatement of the contract
 * that uses no map.  tests/test_flow_learn.py builds and runs it.
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pptk_rx.h"

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);     \
      exit(1);                                                    \
    }                                                             \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;

static uint64_t rnd(void)
{
  uint64_t x = rng_state;
  x ^= x << 13;
  x ^= x >> 7;
  x ^= x << 17;
  return rng_state = x;
}

/* record i of flow f: the key bytes follow f alone, the rest is noise */
static void make_rec(struct pptk_rx_rec *r, uint32_t f, uint64_t hash)
{
  uint32_t k;
  memset(r, 0, sizeof(*r));
  r->flow_hash = hash;
  for (k = 0; k < 16; k++) {
    r->src[k] = (uint8_t)(f * 7 + k);
    r->dst[k] = (uint8_t)(f * 13 + 3 * k);
  }
  r->src[0] = (uint8_t)f;
  r->src[1] = (uint8_t)(f >> 8);
  r->sport = (uint16_t)(f * 31);
  r->dport = (uint16_t)(f >> 3);
  r->proto = (f & 1) ? 6 : 17;
  r->flags = PPTK_RX_F_PARSED;
  r->l4_len = (uint16_t)rnd();
  r->ip_cksum = (uint16_t)rnd();
  r->src_bucket = (uint32_t)rnd();
}

static int key_same(const struct pptk_rx_rec *a, const struct pptk_rx_rec *b)
{
  return !memcmp((const uint8_t *)a + 8, (const uint8_t *)b + 8, 36) && a->proto == b->proto;
}

/* The contract without a map: frame i's hash leader is the first considered
 * frame with its hash. */
static void restate(const struct pptk_rx_rec *recs, const uint8_t *st, uint64_t n, uint64_t maxc,
                    uint32_t *lead_frame, uint32_t *lead_count, struct pptk_flow_learn_hdr *h)
{
  uint64_t i, j, taken = 0;
  uint32_t *cons = malloc((n + 1) * sizeof(*cons));
  uint32_t *entry_of = malloc((n + 1) * sizeof(*entry_of));
  CHECK(cons && entry_of);
  memset(h, 0, sizeof(*h));
  for (i = 0; i < n; i++) {
    if (st[i] != PPTK_FLOW_ST_SUBJECT)
      continue;
    h->candidates++;
    if (taken == maxc)
      continue;
    for (j = 0; j < taken; j++)
      if (recs[cons[j]].flow_hash == recs[i].flow_hash)
        break;
    cons[taken] = (uint32_t)i;
    if (j < taken && key_same(&recs[cons[j]], &recs[i])) {
      lead_count[entry_of[j]]++;
      entry_of[taken] = 0xffffffffu;
    } else {
      entry_of[taken] = (uint32_t)h->flows;
      lead_frame[h->flows] = (uint32_t)i;
      lead_count[h->flows] = 1;
      h->flows++;
    }
    taken++;
  }
  h->considered = taken;
  free(cons);
  free(entry_of);
}

/* one call with exactly-sized outputs against the restatement */
static void run(const struct pptk_rx_rec *src, const uint8_t *st_src, uint64_t n, uint64_t maxc,
                uint64_t cap, int with_first, int with_packets)
{
  /* exactly n records and n status bytes, the latter at an odd address */
  struct pptk_rx_rec *recs = n ? aligned_alloc(16, n * sizeof(*recs)) : NULL;
  uint8_t *stbuf = malloc(n + 1), *st = stbuf + 1;
  uint32_t *lf = malloc((n + 1) * sizeof(*lf)), *lc = malloc((n + 1) * sizeof(*lc));
  struct pptk_flow_learn_hdr want, *hdr = malloc(sizeof(*hdr));
  struct pptk_rx_rec *out;
  uint32_t *first, *packets;
  uint64_t w, k;
  CHECK(stbuf && lf && lc && hdr && (recs || !n));
  if (n) {
    memcpy(recs, src, n * sizeof(*recs));
    memcpy(st, st_src, n);
  }
  restate(recs, st, n, maxc, lf, lc, &want);
  want.written = want.flows < cap ? want.flows : cap;
  w = want.written;
  /* the outputs hold `written` entries and not one more */
  out = w ? aligned_alloc(16, w * sizeof(*out)) : NULL;
  first = with_first && w ? malloc(w * sizeof(*first)) : NULL;
  packets = with_packets && w ? malloc(w * sizeof(*packets)) : NULL;
  CHECK(pptk_flow_learn_host(recs, st, n, maxc, cap && !out ? (void *)16 : out, first, packets,
                             cap, hdr) == 0);
  CHECK(!memcmp(hdr, &want, sizeof(want)));
  for (k = 0; k < w; k++) {
    CHECK(!memcmp(&out[k], &recs[lf[k]], sizeof(*out)));
    CHECK(!first || first[k] == lf[k]);
    CHECK(!packets || packets[k] == lc[k]);
  }
  free(recs);
  free(stbuf);
  free(lf);
  free(lc);
  free(hdr);
  free(out);
  free(first);
  free(packets);
}

static void sweep(const struct pptk_rx_rec *recs, const uint8_t *st, uint64_t n)
{
  struct pptk_flow_learn_hdr h;
  uint32_t *lf = malloc((n + 1) * sizeof(*lf)), *lc = malloc((n + 1) * sizeof(*lc));
  uint64_t c, f, maxcs[6], caps[5], a, b;
  CHECK(lf && lc);
  restate(recs, st, n, 1ull << 30, lf, lc, &h);
  free(lf);
  free(lc);
  c = h.candidates;
  f = h.flows;
  maxcs[0] = 1, maxcs[1] = c > 1 ? c - 1 : 1, maxcs[2] = c ? c : 1, maxcs[3] = c + 1;
  maxcs[4] = 1ull << 30, maxcs[5] = 3;
  caps[0] = 0, caps[1] = f > 1 ? f - 1 : 0, caps[2] = f, caps[3] = f + 7, caps[4] = 1;
  for (a = 0; a < 6; a++)
    for (b = 0; b < 5; b++) {
      run(recs, st, n, maxcs[a], caps[b], 1, 1);
      run(recs, st, n, maxcs[a], caps[b], (int)(a & 1), (int)(b & 1));
    }
}

int main(void)
{
  enum { N = 3000 };
  struct pptk_rx_rec *recs = aligned_alloc(16, N * sizeof(*recs));
  uint8_t *st = malloc(N);
  struct pptk_flow_learn_hdr h;
  uint64_t i;
  CHECK(recs && st);

  /* a mix: 200 flows, a third candidates, hits and non-subjects between */
  for (i = 0; i < N; i++) {
    const uint32_t f = (uint32_t)(rnd() % 200);
    const uint64_t r = rnd() % 6;
    make_rec(&recs[i], f, 0x1000003ull * f + 77);
    st[i] = r < 2 ? PPTK_FLOW_ST_SUBJECT : r < 4 ? (PPTK_FLOW_ST_SUBJECT | PPTK_FLOW_ST_HIT)
                                                 : r == 4 ? 0 : 0xff;
  }
  sweep(recs, st, N);
  sweep(recs, st, 1);
  sweep(recs, st, 0);
  /* one flow; all distinct; no candidates */
  for (i = 0; i < N; i++) {
    make_rec(&recs[i], 5, 99);
    st[i] = PPTK_FLOW_ST_SUBJECT;
  }
  sweep(recs, st, 700);
  for (i = 0; i < N; i++)
    make_rec(&recs[i], (uint32_t)i, rnd());
  sweep(recs, st, 900);
  memset(st, PPTK_FLOW_ST_SUBJECT | PPTK_FLOW_ST_HIT, N);
  sweep(recs, st, 500);
  /* hashes 0 and 2^64 - 1, two keys under each; three keys under one hash;
   * 300 hashes with one low word */
  for (i = 0; i < N; i++) {
    const uint32_t f = (uint32_t)(rnd() % 12);
    make_rec(&recs[i], f, f < 2 ? 0 : f < 4 ? ~0ull : f < 7 ? 0xABCDEF0123456789ull : f);
    st[i] = PPTK_FLOW_ST_SUBJECT;
  }
  sweep(recs, st, 400);
  for (i = 0; i < N; i++) {
    const uint32_t f = (uint32_t)(rnd() % 300);
    make_rec(&recs[i], f, ((uint64_t)(f + 1) << 32) | 0xfffffff0u);
  }
  sweep(recs, st, 1200);

  /* the argument checks: nothing is read or written */
  CHECK(pptk_flow_learn_host(NULL, st, 4, 4, NULL, NULL, NULL, 0, &h) == -EINVAL);
  CHECK(pptk_flow_learn_host(recs, NULL, 4, 4, NULL, NULL, NULL, 0, &h) == -EINVAL);
  CHECK(pptk_flow_learn_host(recs, st, 4, 4, NULL, NULL, NULL, 0, NULL) == -EINVAL);
  CHECK(pptk_flow_learn_host(recs, st, 4, 4, NULL, NULL, NULL, 1, &h) == -EINVAL);
  CHECK(pptk_flow_learn_host(recs, st, 1ull << 32, 4, NULL, NULL, NULL, 0, &h) == -EINVAL);
  CHECK(pptk_flow_learn_host(recs, st, 4, 0, NULL, NULL, NULL, 0, &h) == -EINVAL);
  CHECK(pptk_flow_learn_host(recs, st, 4, (1ull << 30) + 1, NULL, NULL, NULL, 0, &h) == -EINVAL);
  CHECK(pptk_flow_learn_host((void *)((uintptr_t)recs + 8), st, 4, 4, NULL, NULL, NULL, 0, &h) ==
        -EINVAL);
  CHECK(pptk_flow_learn_host(recs, st, 4, 4, (void *)((uintptr_t)recs + 4), NULL, NULL, 1, &h) ==
        -EINVAL);
  CHECK(pptk_flow_learn_host(recs, st, 4, 4, NULL, NULL, NULL, 0,
                             (void *)((uintptr_t)&h + 4)) == -EINVAL);
  CHECK(pptk_flow_learn_host(recs, st, 4, 4, NULL, (void *)((uintptr_t)st + 2), NULL, 0, &h) ==
        -EINVAL);
  CHECK(pptk_flow_learn_host(recs, st, 4, 4, NULL, NULL, (void *)((uintptr_t)st + 1), 0, &h) ==
        -EINVAL);
  CHECK(pptk_flow_learn_host(NULL, NULL, 0, 1, NULL, NULL, NULL, 0, NULL) == 0);
  free(recs);
  free(st);
  puts("flow learn ok");
  return 0;
}
