/*
 * flowlearn.c -- pptk_flow_learn_host, the CPU statement of "Flow learning"
 * (include/pptk_rx.h): the report of the new flows in a batch, which the
 * device call (rx_flowlearn.hip) must equal byte for byte.  It is the step
 * the reference takes per packet when its probe finds no entry
 * (ldp/ldpswitch.c port_put(), "adding entry ... due to learning"), stated
 * over a batch: the first frame of every unknown flow, in frame order, with
 * the number of frames that followed it.  Plain C with an open-addressed map
 * of its own; no HIP, no recursion: a program may link this file alone.
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "pptk_rx.h"

_Static_assert(sizeof(struct pptk_flow_learn_hdr) == 32, "the header is 32 bytes");
_Static_assert(sizeof(struct pptk_rx_rec) == 64, "struct pptk_rx_rec is 64 bytes");

struct learn_ent {
  uint64_t hash;
  uint32_t frame;   /* the first considered frame that carried the hash */
  uint32_t k1;      /* 1 + its entry number; 0 = unused */
};

/* record bytes 8..43 plus proto */
static int key_eq(const struct pptk_rx_rec *a, const struct pptk_rx_rec *b)
{
  return !memcmp(a->src, b->src, 16) && !memcmp(a->dst, b->dst, 16) && a->sport == b->sport &&
         a->dport == b->dport && a->proto == b->proto;
}

int pptk_flow_learn_host(const struct pptk_rx_rec *recs, const uint8_t *status, uint64_t n,
                         uint64_t max_candidates, struct pptk_rx_rec *new_recs, uint32_t *first,
                         uint32_t *packets, uint64_t cap, struct pptk_flow_learn_hdr *hdr)
{
  struct learn_ent *map;
  uint64_t i, candidates = 0, considered = 0, flows = 0, size, left;
  if (n >= (1ull << 32) || max_candidates == 0 || max_candidates > (1ull << 30))
    return -EINVAL;
  if (n && (!recs || !status || !hdr))
    return -EINVAL;
  if (cap && !new_recs)
    return -EINVAL;
  if (((uintptr_t)recs & 15u) || ((uintptr_t)new_recs & 15u) || ((uintptr_t)hdr & 7u) ||
      ((uintptr_t)first & 3u) || ((uintptr_t)packets & 3u))
    return -EINVAL;
  if (n == 0) {
    if (hdr)
      memset(hdr, 0, sizeof(*hdr));
    return 0;
  }
  for (i = 0; i < n; i++)
    candidates += status[i] == PPTK_FLOW_ST_SUBJECT;
  considered = candidates < max_candidates ? candidates : max_candidates;
  /* at most half full, so a probe always ends on an unused entry */
  for (size = 16; size < 2 * considered; size <<= 1)
    ;
  map = calloc(size, sizeof(*map));
  if (!map)
    return -ENOMEM;
  left = considered;
  for (i = 0; i < n && left; i++) {
    const struct pptk_rx_rec *r = &recs[i];
    struct learn_ent *e = NULL;
    uint64_t s, d;
    int known = 0;
    if (status[i] != PPTK_FLOW_ST_SUBJECT)
      continue;
    left--;
    s = (uint32_t)r->flow_hash & (size - 1);
    for (d = 0; d < size; d++, s = (s + 1) & (size - 1)) {
      e = &map[s];
      if (!e->k1)
        break;
      if (e->hash == r->flow_hash) {
        known = 1;
        break;
      }
    }
    if (known && key_eq(r, &recs[e->frame])) {
      if (e->k1 - 1 < cap && packets)
        packets[e->k1 - 1]++;
      continue;
    }
    /* a leader: the first frame of its hash, or another key under a known
     * hash (a true 64-bit collision), which stays outside the map */
    if (!known && e && !e->k1) {
      e->hash = r->flow_hash;
      e->frame = (uint32_t)i;
      e->k1 = (uint32_t)flows + 1;
    }
    if (flows < cap) {
      memcpy(&new_recs[flows], r, sizeof(*r));
      if (first)
        first[flows] = (uint32_t)i;
      if (packets)
        packets[flows] = 1;
    }
    flows++;
  }
  free(map);
  hdr->candidates = candidates;
  hdr->considered = considered;
  hdr->flows = flows;
  hdr->written = flows < cap ? flows : cap;
  return 0;
}
