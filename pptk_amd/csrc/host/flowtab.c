/*
 * flowtab.c -- the host half of the flow table (include/pptk_rx.h "Flow
 * table"): the slot image and its insert, update, delete, find, clear and
 * stats, the dirty-page bitmap pptk_flow_table_sync uploads from, and
 * pptk_flow_lookup_host, the CPU statement of the device lookup; and the
 * host half of "Flow state": pptk_flow_table_expire, which deletes idle flows
 * by a downloaded stats array, and pptk_flow_account_host, the CPU statement
 * of the accounting kernel (rx_flowstat.hip).  The
 * structure is the reference's hashtable/hashtable.h -- a power-of-two array
 * addressed by hashval & (bucketcnt - 1), never growing -- with the bucket's
 * candidate list laid out in the array itself (linear probing), so that the
 * device walks it with aligned 64-byte reads.  No HIP here: the device half
 * (rx_flow.hip) is referenced weakly and a program may link this file alone.
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "pptk_rx.h"
#include "siphash.h"
#include "../flowtab.h"

#pragma weak pptk_flowtab_dev_attach
#pragma weak pptk_flowtab_dev_release

_Static_assert(sizeof(struct pptk_flow_slot) == 64, "a slot is 64 bytes");
_Static_assert(sizeof(struct pptk_flow_key) == 40, "struct pptk_flow_key is 40 bytes");
_Static_assert(sizeof(struct pptk_rx_rec) == 64, "struct pptk_rx_rec is 64 bytes");

static inline uint32_t home_of(const struct pptk_flow_table *t, uint64_t hash)
{
  return (uint32_t)hash & (t->slots - 1);
}

static inline void mark(struct pptk_flow_table *t, uint32_t s)
{
  const uint32_t p = s / PPTK_FLOW_PAGE_SLOTS;
  t->dirty[p >> 6] |= 1ull << (p & 63);
}

static void mark_all(struct pptk_flow_table *t)
{
  uint32_t p;
  memset(t->dirty, 0, ((size_t)t->pages + 63) / 64 * sizeof(uint64_t));
  for (p = 0; p < t->pages; p++)
    t->dirty[p >> 6] |= 1ull << (p & 63);
}

static int key_ok(const struct pptk_flow_key *k)
{
  return k && !(k->zero[0] | k->zero[1] | k->zero[2]);
}

/* in use, the same 64-bit hash and all 37 key bytes */
static int slot_is(const struct pptk_flow_slot *s, const struct pptk_flow_key *k, uint64_t hash)
{
  return s->used && s->hash == hash && !memcmp(s->src, k->src, 16) &&
         !memcmp(s->dst, k->dst, 16) && s->sport == k->sport && s->dport == k->dport &&
         s->proto == k->proto;
}

/* The slot of the key, or, where the probe ends on an unused slot, that slot
 * with *found = 0.  The table is never more than half full, so it ends. */
static uint32_t probe(const struct pptk_flow_table *t, const struct pptk_flow_key *k,
                      uint64_t hash, int *found)
{
  const uint32_t mask = t->slots - 1;
  uint32_t s = home_of(t, hash), d;
  for (d = 0; d < t->slots; d++, s = (s + 1) & mask) {
    if (!t->img[s].used) {
      *found = 0;
      return s;
    }
    if (slot_is(&t->img[s], k, hash)) {
      *found = 1;
      return s;
    }
  }
  *found = 0;
  return t->slots;   /* not reached while count <= slots / 2 */
}

int pptk_flow_table_create(struct pptk_rx_ctx *ctx, uint32_t slots, struct pptk_flow_table **out)
{
  struct pptk_flow_table *t;
  int rc;
  if (!out)
    return -EINVAL;
  *out = NULL;
  if (slots < PPTK_FLOW_MIN_SLOTS || slots > PPTK_FLOW_MAX_SLOTS || (slots & (slots - 1)))
    return -EINVAL;
  if (ctx && !pptk_flowtab_dev_attach)
    return -ENOSYS;
  t = calloc(1, sizeof(*t));
  if (!t)
    return -ENOMEM;
  t->slots = slots;
  t->pages = (slots + PPTK_FLOW_PAGE_SLOTS - 1) / PPTK_FLOW_PAGE_SLOTS;
  t->img = aligned_alloc(64, (size_t)slots * sizeof(struct pptk_flow_slot));
  t->dirty = calloc(((size_t)t->pages + 63) / 64, sizeof(uint64_t));
  if (!t->img || !t->dirty) {
    pptk_flow_table_destroy(t);
    return -ENOMEM;
  }
  memset(t->img, 0, (size_t)slots * sizeof(struct pptk_flow_slot));
  mark_all(t);   /* a first sync uploads everything */
  if (ctx) {
    rc = pptk_flowtab_dev_attach(t, ctx);
    if (rc) {
      pptk_flow_table_destroy(t);
      return rc;
    }
  }
  *out = t;
  return 0;
}

void pptk_flow_table_destroy(struct pptk_flow_table *t)
{
  if (!t)
    return;
  if (t->d_img && pptk_flowtab_dev_release)
    pptk_flowtab_dev_release(t);
  free(t->img);
  free(t->dirty);
  free(t);
}

void pptk_flow_key_from_rec(const struct pptk_rx_rec *rec, struct pptk_flow_key *key)
{
  memcpy(key->src, rec->src, 16);
  memcpy(key->dst, rec->dst, 16);
  key->sport = rec->sport;
  key->dport = rec->dport;
  key->proto = rec->proto;
  key->zero[0] = key->zero[1] = key->zero[2] = 0;
}

uint64_t pptk_flow_key_hash(const uint8_t key16[16], const struct pptk_flow_key *key)
{
  uint8_t tuple[40];
  memcpy(tuple, key->src, 16);
  memcpy(tuple + 16, key->dst, 16);
  tuple[32] = (uint8_t)(key->sport >> 8);
  tuple[33] = (uint8_t)key->sport;
  tuple[34] = (uint8_t)(key->dport >> 8);
  tuple[35] = (uint8_t)key->dport;
  tuple[36] = key->proto;
  tuple[37] = tuple[38] = tuple[39] = 0;
  return siphash_buf(key16, tuple, sizeof(tuple));
}

int pptk_flow_table_insert(struct pptk_flow_table *t, const struct pptk_flow_key *key,
                           uint64_t flow_hash, uint32_t value)
{
  struct pptk_flow_slot *s;
  uint32_t at, disp;
  int found;
  if (!t || !key_ok(key) || value == PPTK_FLOW_NONE)
    return -EINVAL;
  at = probe(t, key, flow_hash, &found);
  if (found)
    return -EEXIST;
  if (t->count >= t->slots / 2 || at >= t->slots)
    return -ENOSPC;
  s = &t->img[at];
  memset(s, 0, sizeof(*s));
  s->hash = flow_hash;
  memcpy(s->src, key->src, 16);
  memcpy(s->dst, key->dst, 16);
  s->sport = key->sport;
  s->dport = key->dport;
  s->proto = key->proto;
  s->used = 1;
  s->value = value;
  mark(t, at);
  t->count++;
  disp = (at - home_of(t, flow_hash)) & (t->slots - 1);
  if (disp + 1 > t->probe_limit)
    t->probe_limit = disp + 1;
  return 0;
}

int pptk_flow_table_update(struct pptk_flow_table *t, const struct pptk_flow_key *key,
                           uint64_t flow_hash, uint32_t value)
{
  uint32_t at;
  int found;
  if (!t || !key_ok(key) || value == PPTK_FLOW_NONE)
    return -EINVAL;
  at = probe(t, key, flow_hash, &found);
  if (!found)
    return -ENOENT;
  if (t->img[at].value != value) {
    t->img[at].value = value;
    mark(t, at);
  }
  return 0;
}

static void delete_at(struct pptk_flow_table *t, uint32_t hole);

int pptk_flow_table_delete(struct pptk_flow_table *t, const struct pptk_flow_key *key,
                           uint64_t flow_hash)
{
  uint32_t hole;
  int found;
  if (!t || !key_ok(key))
    return -EINVAL;
  hole = probe(t, key, flow_hash, &found);
  if (!found)
    return -ENOENT;
  delete_at(t, hole);
  return 0;
}

/* Empties the used slot `hole`.  Backward shift: every entry of the cluster
 * behind the hole whose home slot does not lie in (hole, j] moves into the
 * hole, so that no probe meets an unused slot before its key. */
static void delete_at(struct pptk_flow_table *t, uint32_t hole)
{
  const uint32_t mask = t->slots - 1;
  uint32_t j;
  for (j = (hole + 1) & mask; t->img[j].used; j = (j + 1) & mask) {
    const uint32_t from_home = (j - home_of(t, t->img[j].hash)) & mask;
    if (from_home >= ((j - hole) & mask)) {
      t->img[hole] = t->img[j];
      mark(t, hole);
      hole = j;
    }
  }
  memset(&t->img[hole], 0, sizeof(t->img[hole]));
  mark(t, hole);
  t->count--;
}

/* Idle expiry (include/pptk_rx.h "Flow state").  The walk visits the slots
 * in array order and stays on a slot while it deletes there: the backward
 * shift may have put another entry into it.  An entry the walk has not yet
 * seen lies in a slot after the walk's, and a shift only ever moves it back
 * as far as the slot being emptied -- the walk's own; the slots a cluster
 * that wraps round the end of the array shifts within [0, walk) hold entries
 * the walk has already kept.  So one pass sees every entry. */
int pptk_flow_table_expire(struct pptk_flow_table *t, const struct pptk_flow_stats *stats,
                           uint64_t stats_count, uint64_t now, uint64_t idle,
                           uint32_t *expired_values, uint32_t cap)
{
  uint32_t s, done = 0;
  if (!t || !stats || (cap && !expired_values))
    return -EINVAL;
  if (cap > 0x7fffffffu)
    cap = 0x7fffffffu;   /* the count is returned as an int */
  for (s = 0; s < t->slots && done < cap; s++) {
    while (t->img[s].used && done < cap) {
      const uint32_t v = t->img[s].value;
      uint64_t seen;
      if (v >= stats_count)
        break;
      seen = stats[v].last_seen;
      /* seen + idle < now, without the sum */
      if (!(now > seen && now - seen > idle))
        break;
      expired_values[done++] = v;
      delete_at(t, s);
    }
  }
  return (int)done;
}

int pptk_flow_account_host(const uint32_t *idx, const uint16_t *len, uint32_t fixed_len,
                           uint64_t n, struct pptk_flow_stats *stats, uint64_t stats_count,
                           struct pptk_flow_stats *unmatched, uint64_t now)
{
  uint64_t i;
  if (stats_count == 0 || stats_count > (1ull << 32) || fixed_len > 65535u)
    return -EINVAL;
  if (((uintptr_t)idx & 3u) || ((uintptr_t)len & 1u) || ((uintptr_t)stats & 31u) ||
      ((uintptr_t)unmatched & 31u))
    return -EINVAL;
  if (n && (!idx || !stats))
    return -EINVAL;
  for (i = 0; i < n; i++) {
    const uint32_t v = idx[i];
    struct pptk_flow_stats *e = v < stats_count ? &stats[v] : unmatched;
    if (!e)
      continue;
    e->packets += 1;
    e->bytes += len ? len[i] : fixed_len;
    if (e->last_seen < now)
      e->last_seen = now;
  }
  return 0;
}

int pptk_flow_table_find(const struct pptk_flow_table *t, const struct pptk_flow_key *key,
                         uint64_t flow_hash, uint32_t *value)
{
  uint32_t at;
  int found;
  if (!t || !key_ok(key))
    return -EINVAL;
  at = probe(t, key, flow_hash, &found);
  if (!found)
    return -ENOENT;
  if (value)
    *value = t->img[at].value;
  return 0;
}

static int rec_subject(const struct pptk_rx_rec *r)
{
  return (r->flags & (PPTK_RX_F_PARSED | PPTK_RX_F_MALFORMED)) == PPTK_RX_F_PARSED;
}

int pptk_flow_table_insert_recs(struct pptk_flow_table *t, const struct pptk_rx_rec *recs,
                                uint64_t n, const uint32_t *values, int32_t *results)
{
  struct pptk_flow_key k;
  uint64_t i;
  int done = 0, rc;
  if (!t || (n && (!recs || !values)) || n > 0x7fffffffu)
    return -EINVAL;
  for (i = 0; i < n; i++) {
    if (!rec_subject(&recs[i])) {
      rc = -EINVAL;
    } else {
      pptk_flow_key_from_rec(&recs[i], &k);
      rc = pptk_flow_table_insert(t, &k, recs[i].flow_hash, values[i]);
    }
    if (results)
      results[i] = rc;
    done += rc == 0;
  }
  return done;
}

void pptk_flow_table_clear(struct pptk_flow_table *t)
{
  if (!t)
    return;
  memset(t->img, 0, (size_t)t->slots * sizeof(struct pptk_flow_slot));
  mark_all(t);
  t->count = 0;
  t->probe_limit = 0;
}

void pptk_flow_table_stats(const struct pptk_flow_table *t, uint32_t *slots, uint32_t *count,
                           uint32_t *probe_limit)
{
  if (slots)
    *slots = t ? t->slots : 0;
  if (count)
    *count = t ? t->count : 0;
  if (probe_limit)
    *probe_limit = t ? t->probe_limit : 0;
}

int pptk_flow_lookup_host(const struct pptk_flow_table *t, const struct pptk_rx_rec *recs,
                          uint64_t n, const uint8_t *subject, uint32_t *idx, uint8_t *status)
{
  struct pptk_flow_key k;
  uint64_t i;
  if (!t || (n && (!recs || !idx)))
    return -EINVAL;
  for (i = 0; i < n; i++) {
    uint32_t v = PPTK_FLOW_NONE;
    uint8_t st = 0;
    if (rec_subject(&recs[i]) && (!subject || subject[i])) {
      st = PPTK_FLOW_ST_SUBJECT;
      pptk_flow_key_from_rec(&recs[i], &k);
      if (pptk_flow_table_find(t, &k, recs[i].flow_hash, &v) == 0)
        st |= PPTK_FLOW_ST_HIT;
      else
        v = PPTK_FLOW_NONE;
    }
    idx[i] = v;
    if (status)
      status[i] = st;
  }
  return 0;
}
