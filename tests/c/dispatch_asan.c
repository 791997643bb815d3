/*
 * dispatch_asan.c -- pptk_tx_dispatch_host (pptk_amd/csrc/host/dispatch.c)
 * driven from a program of its own, built with -fsanitize=address,undefined:
 * every array is a heap block of exactly the size the contract gives it, so a
 * read or write one element outside is reported.  Random batches in both
 * forms, with and without each nullable array, caps below, at and above the
 * total; the results are checked against a plain recount (per port: the
 * entries ascend, their number, bytes and flood share add up).
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pptk_rx.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;

static uint32_t rnd(void)
{
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}

#define CHECK(x)                                                         \
  do {                                                                   \
    if (!(x)) {                                                          \
      printf("dispatch_asan: %s failed at line %d\n", #x, __LINE__);     \
      exit(1);                                                           \
    }                                                                    \
  } while (0)

static void *block(size_t bytes)
{
  void *p = malloc(bytes ? bytes : 1);
  CHECK(p);
  return p;
}

static uint8_t rand_code(uint32_t nports)
{
  uint32_t r = rnd() % 20;
  if (r == 0)
    return PPTK_PORT_FLOOD;
  if (r == 1)
    return PPTK_PORT_DROP;
  if (r == 2)
    return (uint8_t)(nports + rnd() % (PPTK_PORT_DROP - nports));   /* a bad code */
  return (uint8_t)(rnd() % nports);
}

/* one batch; variant bits: 1 idx form, 2 subject, 4 in_port, 8 off / len, 16 out_off, 32 out_len */
static void one(uint64_t n, uint32_t nports, unsigned variant, int cap_mode)
{
  struct pptk_dispatch d;
  struct pptk_dispatch_port *ports = block(nports * sizeof(*ports));
  struct pptk_dispatch_hdr *hdr = block(sizeof(*hdr));
  uint64_t i, g, flows = 37, total, cap, classes;
  uint32_t p;
  memset(&d, 0, sizeof(d));
  d.n = n;
  d.nports = nports;
  d.miss_code = (variant & 64) ? PPTK_PORT_FLOOD : PPTK_PORT_DROP;
  d.in_port_all = rnd() % (nports + 2);
  d.stride = 2048;
  d.fixed_len = 60;
  d.ports = ports;
  d.hdr = hdr;
  if (variant & 1) {
    uint32_t *idx = block(n * sizeof(*idx));
    uint8_t *fp = block(flows);
    for (i = 0; i < flows; i++)
      fp[i] = rand_code(nports);
    for (i = 0; i < n; i++) {
      uint32_t r = rnd() % 10;
      idx[i] = r == 0 ? PPTK_FLOW_NONE : r == 1 ? (uint32_t)flows + rnd() % 3 : rnd() % flows;
    }
    d.idx = idx;
    d.flow_port = fp;
    d.flows = flows;
  } else {
    uint8_t *port = block(n);
    for (i = 0; i < n; i++)
      port[i] = rand_code(nports);
    d.port = port;
  }
  if (variant & 2) {
    uint8_t *s = block(n);
    for (i = 0; i < n; i++)
      s[i] = rnd() % 8 ? (uint8_t)(1 + rnd() % 255) : 0;
    d.subject = s;
  }
  if (variant & 4) {
    uint8_t *in = block(n);
    for (i = 0; i < n; i++)
      in[i] = (uint8_t)(rnd() % (nports + 3));
    d.in_port = in;
  }
  if (variant & 8) {
    uint64_t *off = block(n * sizeof(*off));
    uint16_t *len = block(n * sizeof(*len));
    for (i = 0; i < n; i++) {
      off[i] = (uint64_t)rnd() << 8;
      len[i] = (uint16_t)rnd();
    }
    d.off = off;
    d.len = len;
  }
  /* first a count-only call: cap 0, null list */
  CHECK(pptk_tx_dispatch_host(&d) == 0);
  total = hdr->total;
  CHECK(hdr->written == 0);
  cap = cap_mode == 0 ? total : cap_mode == 1 ? total / 2 : total + 3;
  d.cap = cap;
  d.list = block(cap * sizeof(*d.list));
  if (variant & 16)
    d.out_off = block(cap * sizeof(*d.out_off));
  if (variant & 32)
    d.out_len = block(cap * sizeof(*d.out_len));
  CHECK(pptk_tx_dispatch_host(&d) == 0);
  CHECK(hdr->total == total && hdr->written == (total < cap ? total : cap) && hdr->reserved == 0);
  classes = hdr->unicast + hdr->flood + hdr->dropped + hdr->bad;
  CHECK(classes == n && hdr->hairpin <= hdr->unicast);
  g = 0;
  for (p = 0; p < nports; p++) {
    uint64_t k, bytes = 0, prev = 0;
    CHECK(ports[p].start == g && ports[p].flooded <= ports[p].count &&
          ports[p].flooded <= hdr->flood);
    for (k = 0; k < ports[p].count && g + k < hdr->written; k++) {
      const uint64_t f = d.list[g + k];
      CHECK(f < n && (k == 0 || f > prev));
      prev = f;
      if (d.out_off)
        CHECK(d.out_off[g + k] == (d.off ? d.off[f] : f * d.stride));
      if (d.out_len)
        CHECK(d.out_len[g + k] == (d.len ? d.len[f] : d.fixed_len));
      bytes += d.len ? d.len[f] : d.fixed_len;
    }
    if (g + ports[p].count <= hdr->written)
      CHECK(bytes == ports[p].bytes);
    g += ports[p].count;
  }
  CHECK(g == total);
  free((void *)d.port);
  free((void *)d.idx);
  free((void *)d.flow_port);
  free((void *)d.subject);
  free((void *)d.in_port);
  free((void *)d.off);
  free((void *)d.len);
  free(d.list);
  free(d.out_off);
  free(d.out_len);
  free(ports);
  free(hdr);
}

int main(void)
{
  static const uint32_t nports[] = {1, 2, 3, 32, 33, 63, 64};
  static const uint64_t sizes[] = {0, 1, 2, 63, 64, 65, 500, 3000};
  struct pptk_dispatch bad;
  unsigned variant, np, s;
  for (variant = 0; variant < 128; variant++)
    for (np = 0; np < sizeof(nports) / sizeof(nports[0]); np++) {
      s = (variant + np) % (sizeof(sizes) / sizeof(sizes[0]));
      /* n == 0 runs too, in either form: its arrays are one-byte blocks never read */
      one(sizes[s], nports[np], variant, (int)((variant + np) % 3));
    }
  memset(&bad, 0, sizeof(bad));
  CHECK(pptk_tx_dispatch_host(NULL) == -EINVAL);
  CHECK(pptk_tx_dispatch_host(&bad) == -EINVAL);
  printf("dispatch ok\n");
  return 0;
}
