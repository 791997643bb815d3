/*
 * gather_asan.c -- pptk_tx_gather_host (pptk_amd/csrc/host/gather.c) driven
 * from a program of its own, built with -fsanitize=address,undefined: every
 * array is a heap block of exactly the size the contract gives it -- the
 * source batch ends with its last frame's last byte, `out` is out_cap bytes --
 * so a read or write one byte outside is reported.  Random batches in every
 * form, with and without each nullable array, caps below, at and above need;
 * the results are checked against a plain recount (per port: the offsets
 * ascend from the region start, every packed slot holds its frame and zeros).
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

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      printf("gather_asan: %s failed at line %d\n", #x, __LINE__);     \
      exit(1);                                                         \
    }                                                                  \
  } while (0)

static void *block(size_t bytes)
{
  void *p = malloc(bytes ? bytes : 1);
  CHECK(p);
  return p;
}

static uint32_t rand_len(void)
{
  static const uint32_t edge[] = {0, 1, 15, 16, 17, 60, 64, 1500, 1514, 9000, 65535};
  uint32_t r = rnd() % 16;
  return r < 11 ? edge[r] : rnd() % 300;
}

/* one batch; variant bits: 1 off / len arrays, 2 list, 4 runs, 8 d_entries, 16 pk_off, 32 pk_len */
static void one(uint64_t n, uint64_t entries, uint32_t nports, unsigned variant, int cap_mode)
{
  struct pptk_gather g;
  struct pptk_dispatch_port *runs = NULL;
  struct pptk_gather_port *ports;
  struct pptk_gather_hdr *hdr = block(sizeof(*hdr));
  uint64_t *off = NULL, i, e, total = 0, need, word, at, packed = 0;
  uint16_t *len = NULL;
  uint32_t *list = NULL, p, fixed = rand_len() % 2000;
  uint8_t *frames, *out = NULL;
  void *outraw = NULL;
  memset(&g, 0, sizeof(g));
  if (!(variant & 4))
    nports = 1;
  ports = block(nports * sizeof(*ports));
  g.n = n;
  g.nports = nports;
  g.ports = ports;
  g.hdr = hdr;
  if (variant & 1) {
    off = block(n * sizeof(*off));
    len = block(n * sizeof(*len));
    for (i = 0; i < n; i++) {
      len[i] = (uint16_t)rand_len();
      off[i] = total + rnd() % 5;
      total = off[i] + len[i];
    }
    g.off = off;
    g.len = len;
  } else {
    g.stride = fixed + rnd() % 9 + (fixed == 0);
    g.fixed_len = fixed;
    total = n ? (n - 1) * g.stride + fixed : 0;
  }
  frames = block(total);
  for (i = 0; i < total; i++)
    frames[i] = (uint8_t)rnd();
  g.frames = frames;
  if (variant & 2) {
    list = block(entries * sizeof(*list));
    for (e = 0; e < entries; e++)
      list[e] = rnd() % 10 ? (uint32_t)(rnd() % (n ? n : 1)) : (uint32_t)(n + rnd() % 3);
    g.list = list;
  } else if (entries > n + 2) {
    entries = n + 2;          /* the identity list: two bad entries at the most */
  }
  g.max_entries = entries;
  if (variant & 4) {
    uint64_t left = entries + (variant & 64 ? 3 : 0), s = 0;
    runs = block(nports * sizeof(*runs));
    for (p = 0; p < nports; p++) {
      uint64_t c = p + 1 == nports ? left : rnd() % 3 ? rnd() % (left + 1) : 0;
      runs[p].start = s;
      runs[p].count = c;
      runs[p].bytes = runs[p].flooded = ~0ull;
      s += c;
      left -= c;
    }
    g.runs = runs;
  }
  if (variant & 8) {
    word = rnd() % 4 == 0 ? entries + 5 : rnd() % (entries + 1);
    g.d_entries = &word;
  }
  if (variant & 16)
    g.pk_off = block(entries * sizeof(*g.pk_off));
  if (variant & 32)
    g.pk_len = block(entries * sizeof(*g.pk_len));
  /* first a count-only call: a null out */
  CHECK(pptk_tx_gather_host(&g) == 0);
  need = hdr->need;
  CHECK(hdr->status == 0 && hdr->entries <= entries && hdr->reserved == 0);
  g.out_cap = cap_mode == 0 ? need : cap_mode == 1 ? need / 2 : need + 3;
  if (g.out_cap) {            /* out_cap bytes exactly, 256-byte aligned */
    CHECK(posix_memalign(&outraw, PPTK_GATHER_REGION_ALIGN, g.out_cap) == 0);
    out = outraw;
    memset(out, 0xEE, g.out_cap);
    g.out = out;
  }
  CHECK(pptk_tx_gather_host(&g) == 0);
  CHECK(hdr->need == need && hdr->packed <= hdr->entries);
  e = 0;
  at = 0;
  for (p = 0; p < nports; p++) {
    uint64_t k, bytes = 0, pk = 0;
    CHECK(ports[p].start == at && ports[p].start % PPTK_GATHER_REGION_ALIGN == 0);
    for (k = 0; k < ports[p].entries; k++, e++) {
      const uint64_t f = list ? list[e] : e;
      const uint32_t l = f >= n ? 0 : len ? len[f] : g.fixed_len;
      const uint64_t slot = (l + 15ull) & ~15ull;
      if (g.pk_off)
        CHECK(g.pk_off[e] == at);
      if (g.pk_len)
        CHECK(g.pk_len[e] == l);
      if (at + slot <= g.out_cap) {
        CHECK(packed == e);
        packed++;
        pk++;
        bytes += slot;
        if (l)
          CHECK(memcmp(out + at, frames + (off ? off[f] : f * g.stride), l) == 0);
        for (i = l; i < slot; i++)
          CHECK(out[at + i] == 0);
      }
      at += slot;
    }
    CHECK(ports[p].packed == pk && ports[p].bytes == bytes);
    if (p + 1 == nports)
      CHECK(at == need);
    for (i = at; i < ((at + 255) & ~255ull) && i < g.out_cap; i++)
      CHECK(out[i] == 0xEE);   /* the padding between regions is not written */
    at = (at + 255) & ~255ull;
  }
  CHECK(e == hdr->entries && packed == hdr->packed);
  free(frames);
  free(off);
  free(len);
  free(list);
  free(runs);
  free(g.pk_off);
  free(g.pk_len);
  free(outraw);
  free(ports);
  free(hdr);
}

int main(void)
{
  static const uint32_t nports[] = {1, 2, 3, 64};
  static const uint64_t sizes[] = {0, 1, 2, 63, 64, 65, 300};
  struct pptk_gather bad;
  struct pptk_gather_port port;
  struct pptk_gather_hdr hdr;
  struct pptk_dispatch_port runs[1] = {{0, 4, 0, 0}};
  unsigned variant, np, s;
  for (variant = 0; variant < 128; variant++)
    for (np = 0; np < sizeof(nports) / sizeof(nports[0]); np++) {
      s = (variant + np) % (sizeof(sizes) / sizeof(sizes[0]));
      one(sizes[s], sizes[(s + variant / 7) % 7] + variant % 3, nports[np], variant,
          (int)((variant + np) % 3));
    }
  memset(&bad, 0, sizeof(bad));
  CHECK(pptk_tx_gather_host(NULL) == -EINVAL);
  CHECK(pptk_tx_gather_host(&bad) == -EINVAL);
  /* runs that are not back to back: a status, nothing else */
  bad.runs = runs;
  bad.max_entries = 8;
  bad.ports = &port;
  bad.hdr = &hdr;
  bad.nports = 1;
  runs[0].start = 1;
  CHECK(pptk_tx_gather_host(&bad) == 0 && hdr.status == PPTK_GATHER_ST_BADRUNS && hdr.entries == 0);
  printf("gather ok\n");
  return 0;
}
