/*
 * flowtab_asan.c -- the host half of the flow table under
 * -fsanitize=address,undefined (tests/test_flowtab.py builds this file with
 * pptk_amd/csrc/host/flowtab.c alone and runs it as a program: no HIP, so
 * every table is host-only).  100 000 random inserts, updates, deletes, finds
 * and record lookups on a 64-slot and on a 1024-slot table against a naive
 * model in this file -- an unordered array of (hash, key, value) searched
 * from the front, which knows nothing of slots or probing -- with the hashes
 * drawn from a small range so that clusters form, wrap around the end of the
 * array and fill the table to its limit; then the wrap and -ENOSPC cases with
 * forged hashes.  Exit status 0 = clean.
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pptk_rx.h"

static int failures;
#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      printf("%s:%d: %s\n", __FILE__, __LINE__, #c);                    \
      failures++;                                                       \
    }                                                                   \
  } while (0)

static uint64_t rnd_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(void)
{
  rnd_state = rnd_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rnd_state >> 33);
}

struct ent {
  uint64_t hash;
  struct pptk_flow_key key;
  uint32_t value;
};

static struct ent *model;
static uint32_t model_n;

static int key_eq(const struct pptk_flow_key *a, const struct pptk_flow_key *b)
{
  return !memcmp(a->src, b->src, 16) && !memcmp(a->dst, b->dst, 16) && a->sport == b->sport &&
         a->dport == b->dport && a->proto == b->proto;
}

static int model_find(const struct pptk_flow_key *k, uint64_t h)
{
  uint32_t i;
  for (i = 0; i < model_n; i++)
    if (model[i].hash == h && key_eq(&model[i].key, k))
      return (int)i;
  return -1;
}

/* key number id of a small universe; its hash falls into `spread` home slots
 * near the end of the array (so clusters wrap), and several ids share one
 * 64-bit hash */
static void make_key(uint32_t id, uint32_t slots, uint32_t spread, struct pptk_flow_key *k,
                     uint64_t *h)
{
  memset(k, 0, sizeof(*k));
  k->src[0] = (uint8_t)id;
  k->src[15] = (uint8_t)(id >> 8);
  k->dst[7] = (uint8_t)(id * 7u);
  k->sport = (uint16_t)(id * 31u);
  k->dport = (uint16_t)(id >> 3);
  k->proto = (id & 1) ? 6 : 17;
  *h = ((uint64_t)(id % 5u) << 40) | ((slots - spread / 2 + (id / 3u) % spread) & 0xffffffffu);
}

static void run_random(uint32_t slots, uint32_t universe, uint32_t spread, uint32_t ops)
{
  struct pptk_flow_table *t = NULL;
  struct pptk_flow_key k;
  struct pptk_rx_rec *rec;
  uint64_t h;
  uint32_t op, v, got, cnt, lim, sl, idx;
  uint8_t st, subj;
  int at, rc;

  CHECK(pptk_flow_table_create(NULL, slots, &t) == 0 && t);
  if (!t)
    return;
  model = calloc(slots, sizeof(*model));
  model_n = 0;
  for (op = 0; op < ops; op++) {
    make_key(rnd() % universe, slots, spread, &k, &h);
    at = model_find(&k, h);
    v = rnd() % 4 ? rnd() : (rnd() & 1 ? 0u : 0xfffffffeu);
    switch (rnd() % 8) {
    case 0:
    case 1:
    case 2:
      rc = pptk_flow_table_insert(t, &k, h, v);
      if (at >= 0) {
        CHECK(rc == -EEXIST);
      } else if (model_n >= slots / 2) {
        CHECK(rc == -ENOSPC);
      } else {
        CHECK(rc == 0);
        model[model_n].hash = h;
        model[model_n].key = k;
        model[model_n].value = v;
        model_n++;
      }
      break;
    case 3:
      rc = pptk_flow_table_update(t, &k, h, v);
      CHECK(rc == (at >= 0 ? 0 : -ENOENT));
      if (at >= 0)
        model[at].value = v;
      break;
    case 4:
    case 5:
      rc = pptk_flow_table_delete(t, &k, h);
      CHECK(rc == (at >= 0 ? 0 : -ENOENT));
      if (at >= 0)
        model[at] = model[--model_n];
      break;
    case 6:
      got = 0x5a5a5a5au;
      rc = pptk_flow_table_find(t, &k, h, &got);
      CHECK(rc == (at >= 0 ? 0 : -ENOENT));
      CHECK(at >= 0 ? got == model[at].value : got == 0x5a5a5a5au);
      break;
    default:
      /* the record form, one heap record of exactly 64 bytes; every fourth
       * is no subject */
      rec = calloc(1, sizeof(*rec));
      rec->flow_hash = h;
      memcpy(rec->src, k.src, 16);
      memcpy(rec->dst, k.dst, 16);
      rec->sport = k.sport;
      rec->dport = k.dport;
      rec->proto = k.proto;
      subj = rnd() % 4 != 0;
      rec->flags = subj ? PPTK_RX_F_PARSED : (rnd() & 1 ? 0 : PPTK_RX_F_PARSED | PPTK_RX_F_MALFORMED);
      idx = 0x5a5a5a5au;
      st = 0x5a;
      CHECK(pptk_flow_lookup_host(t, rec, 1, NULL, &idx, &st) == 0);
      if (!subj)
        CHECK(idx == PPTK_FLOW_NONE && st == 0);
      else if (at >= 0)
        CHECK(idx == model[at].value && st == (PPTK_FLOW_ST_SUBJECT | PPTK_FLOW_ST_HIT));
      else
        CHECK(idx == PPTK_FLOW_NONE && st == PPTK_FLOW_ST_SUBJECT);
      free(rec);
      break;
    }
    pptk_flow_table_stats(t, &sl, &cnt, &lim);
    CHECK(sl == slots && cnt == model_n && lim <= slots);
    if (failures > 20)
      break;
  }
  /* everything the model holds is found, then cleared away */
  for (op = 0; op < model_n; op++) {
    got = 0;
    CHECK(pptk_flow_table_find(t, &model[op].key, model[op].hash, &got) == 0 &&
          got == model[op].value);
  }
  pptk_flow_table_clear(t);
  pptk_flow_table_stats(t, NULL, &cnt, &lim);
  CHECK(cnt == 0 && lim == 0);
  for (op = 0; op < model_n; op++)
    CHECK(pptk_flow_table_find(t, &model[op].key, model[op].hash, NULL) == -ENOENT);
  free(model);
  pptk_flow_table_destroy(t);
}

static void run_wrap(void)
{
  struct pptk_flow_table *t = NULL;
  struct pptk_flow_key k[9];
  uint32_t i, j, lim, cnt, got;
  const uint64_t h = 0xabcdef000000000full;   /* home slot 15 of 16 */

  CHECK(pptk_flow_table_create(NULL, 16, &t) == 0 && t);
  if (!t)
    return;
  for (i = 0; i < 9; i++) {
    memset(&k[i], 0, sizeof(k[i]));
    k[i].src[3] = (uint8_t)(i + 1);
    k[i].proto = 6;
  }
  for (i = 0; i < 8; i++)
    CHECK(pptk_flow_table_insert(t, &k[i], h, i) == 0);
  CHECK(pptk_flow_table_insert(t, &k[8], h, 8) == -ENOSPC);
  CHECK(pptk_flow_table_insert(t, &k[3], h, 99) == -EEXIST);
  pptk_flow_table_stats(t, NULL, &cnt, &lim);
  CHECK(cnt == 8 && lim == 8);
  /* delete from the middle outwards; the rest stays findable */
  for (i = 0; i < 8; i++) {
    const uint32_t d = (i * 3 + 4) % 8;
    CHECK(pptk_flow_table_delete(t, &k[d], h) == 0);
    CHECK(pptk_flow_table_delete(t, &k[d], h) == -ENOENT);
    for (j = i + 1; j < 8; j++) {
      const uint32_t r = (j * 3 + 4) % 8;
      got = 77;
      CHECK(pptk_flow_table_find(t, &k[r], h, &got) == 0 && got == r);
    }
  }
  pptk_flow_table_stats(t, NULL, &cnt, &lim);
  CHECK(cnt == 0 && lim == 8);   /* the limit may stay high after deletes */

  /* bad arguments */
  k[0].zero[1] = 1;
  CHECK(pptk_flow_table_insert(t, &k[0], h, 1) == -EINVAL);
  CHECK(pptk_flow_table_find(t, &k[0], h, NULL) == -EINVAL);
  k[0].zero[1] = 0;
  CHECK(pptk_flow_table_insert(t, &k[0], h, PPTK_FLOW_NONE) == -EINVAL);
  pptk_flow_table_destroy(t);
  t = (struct pptk_flow_table *)&k;
  CHECK(pptk_flow_table_create(NULL, 24, &t) == -EINVAL && t == NULL);
  CHECK(pptk_flow_table_create(NULL, 8, &t) == -EINVAL);
  CHECK(pptk_flow_table_create(NULL, 0, &t) == -EINVAL);
  CHECK(pptk_flow_table_create(NULL, 1u << 27, &t) == -EINVAL);
}

int main(void)
{
  run_random(64, 60, 12, 100000);
  run_random(1024, 900, 200, 100000);
  run_wrap();
  if (failures) {
    printf("flowtab: %d failures\n", failures);
    return 1;
  }
  printf("flowtab ok\n");
  return 0;
}
