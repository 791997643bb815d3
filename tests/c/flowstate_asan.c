/*
 * flowstate_asan.c -- the host half of "Flow state" under
 * -fsanitize=address,undefined (tests/test_flowstats.py builds this file with
 * pptk_amd/csrc/host/flowtab.c alone and runs it as a program: no HIP, so
 * every table is host-only).  pptk_flow_account_host on heap arrays of
 * exactly the sizes named, against a naive loop in this file, with indices on
 * both sides of the array's end, lengths 0 and 65535, a null unmatched, a
 * counter that wraps and the -EINVAL cases; pptk_flow_table_expire in a
 * random run against an unordered array model with hashes drawn from a small
 * range near the end of the array (clusters form and wrap), with caps, the
 * strict boundary, a stamp near 2^64, values past the array, and every
 * subset of a cluster that wraps round the end of a 16-slot table.  Exit
 * status 0 = clean.
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

static uint64_t rnd_state = 0x2545f4914f6cdd1dull;
static uint32_t rnd(void)
{
  rnd_state = rnd_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rnd_state >> 33);
}

#define SENT 0xa5a5a5a5a5a5a5a5ull

static struct pptk_flow_stats *stats_new(uint64_t count)
{
  struct pptk_flow_stats *s = aligned_alloc(32, count * sizeof(*s));
  uint64_t i;
  for (i = 0; i < count; i++) {
    s[i].packets = s[i].bytes = s[i].last_seen = 0;
    s[i].reserved = SENT;
  }
  return s;
}

static void run_account(void)
{
  enum { COUNT = 37, N = 4000 };
  uint32_t *idx = malloc(N * sizeof(*idx));
  uint16_t *len = malloc(N * sizeof(*len));
  struct pptk_flow_stats *st = stats_new(COUNT), *want = stats_new(COUNT);
  struct pptk_flow_stats *um = stats_new(1), *wum = stats_new(1);
  uint64_t now;
  uint32_t i, pass;

  for (i = 0; i < N; i++) {
    idx[i] = rnd() % 8 == 0 ? PPTK_FLOW_NONE : rnd() % (COUNT + 5);
    len[i] = rnd() % 16 == 0 ? 65535 : rnd() % 16 == 1 ? 0 : (uint16_t)rnd();
  }
  idx[0] = COUNT - 1;
  idx[1] = COUNT;
  for (pass = 0; pass < 4; pass++) {
    /* len and unmatched each present and absent; the clock goes back once */
    const uint16_t *l = pass & 1 ? NULL : len;
    struct pptk_flow_stats *u = pass & 2 ? NULL : um;
    now = pass == 2 ? 10 : 1000 + pass;
    CHECK(pptk_flow_account_host(idx, l, 1514, N, st, COUNT, u, now) == 0);
    for (i = 0; i < N; i++) {
      struct pptk_flow_stats *e = idx[i] < COUNT ? &want[idx[i]] : (u ? wum : NULL);
      if (!e)
        continue;
      e->packets++;
      e->bytes += l ? l[i] : 1514;
      if (e->last_seen < now)
        e->last_seen = now;
    }
    CHECK(!memcmp(st, want, COUNT * sizeof(*st)) && !memcmp(um, wum, sizeof(*um)));
  }
  CHECK(want[COUNT - 1].packets >= 4 && wum->packets > 100 && wum->reserved == SENT);
  CHECK(want[3].last_seen == 1003);

  /* a counter that wraps; n = 0 */
  st[5].packets = ~0ull;
  st[5].bytes = ~0ull - 9;
  idx[0] = 5;
  CHECK(pptk_flow_account_host(idx, NULL, 65535, 1, st, COUNT, NULL, 7) == 0);
  CHECK(st[5].packets == 0 && st[5].bytes == 65535 - 10);
  memcpy(want, st, COUNT * sizeof(*st));
  CHECK(pptk_flow_account_host(NULL, NULL, 0, 0, st, COUNT, NULL, 1u << 30) == 0);
  CHECK(pptk_flow_account_host(idx, len, 0, 0, st, COUNT, um, 1u << 30) == 0);
  CHECK(!memcmp(st, want, COUNT * sizeof(*st)));

  /* -EINVAL, nothing written */
  CHECK(pptk_flow_account_host(NULL, len, 0, 4, st, COUNT, um, 1) == -EINVAL);
  CHECK(pptk_flow_account_host(idx, len, 0, 4, NULL, COUNT, um, 1) == -EINVAL);
  CHECK(pptk_flow_account_host(idx, len, 0, 4, st, 0, um, 1) == -EINVAL);
  CHECK(pptk_flow_account_host(idx, len, 0, 4, st, (1ull << 32) + 1, um, 1) == -EINVAL);
  CHECK(pptk_flow_account_host((const uint32_t *)((const char *)idx + 2), len, 0, 4, st, COUNT, um,
                               1) == -EINVAL);
  CHECK(pptk_flow_account_host(idx, (const uint16_t *)((const char *)len + 1), 0, 4, st, COUNT, um,
                               1) == -EINVAL);
  CHECK(pptk_flow_account_host(idx, len, 0, 4, (struct pptk_flow_stats *)((char *)st + 8), COUNT,
                               um, 1) == -EINVAL);
  CHECK(pptk_flow_account_host(idx, len, 0, 4, st, COUNT,
                               (struct pptk_flow_stats *)((char *)um + 16), 1) == -EINVAL);
  CHECK(pptk_flow_account_host(idx, NULL, 65536, 4, st, COUNT, um, 1) == -EINVAL);
  CHECK(!memcmp(st, want, COUNT * sizeof(*st)));
  free(idx);
  free(len);
  free(st);
  free(want);
  free(um);
  free(wum);
}

struct ent {
  uint64_t hash;
  struct pptk_flow_key key;
  uint32_t value;
};

static void make_key(uint32_t id, uint32_t slots, uint32_t spread, struct pptk_flow_key *k,
                     uint64_t *h)
{
  memset(k, 0, sizeof(*k));
  k->src[0] = (uint8_t)id;
  k->src[15] = (uint8_t)(id >> 8);
  k->dst[7] = (uint8_t)(id * 7u);
  k->sport = (uint16_t)(id * 31u);
  k->proto = (id & 1) ? 6 : 17;
  *h = ((uint64_t)(id % 5u) << 40) | ((slots - spread / 2 + (id / 3u) % spread) & 0xffffffffu);
}

static int idle_rule(uint64_t seen, uint64_t idle, uint64_t now)
{
  /* seen + idle < now in 128 bits */
  return (unsigned __int128)seen + idle < now;
}

/* rounds of inserts, deletes, stamps and a (sometimes capped) expire; the
 * model is an unordered array that knows nothing of slots */
static void run_expire(uint32_t slots, uint32_t universe, uint32_t spread, uint32_t rounds)
{
  struct pptk_flow_table *t = NULL;
  struct ent *model = calloc(slots, sizeof(*model));
  const uint32_t count = universe - universe / 4;   /* the top quarter of values lies past the array */
  struct pptk_flow_stats *st = stats_new(count);
  uint32_t *out = malloc(slots * sizeof(*out));
  uint32_t model_n = 0, r, i, j, k, cnt, total = 0;

  CHECK(pptk_flow_table_create(NULL, slots, &t) == 0 && t);
  for (r = 0; r < rounds && t && failures < 20; r++) {
    const uint64_t now = 5000 + 10ull * r, idle = rnd() % 80;
    uint32_t cap, want_n = 0, got_n = 0;
    int rc;
    for (i = 0; i < 10; i++) {
      struct pptk_flow_key key;
      uint64_t h;
      const uint32_t id = rnd() % universe;
      int at = -1;
      make_key(id, slots, spread, &key, &h);
      for (j = 0; j < model_n; j++)
        if (model[j].value == id)
          at = (int)j;
      if (rnd() % 4) {
        rc = pptk_flow_table_insert(t, &key, h, id);
        if (at >= 0) {
          CHECK(rc == -EEXIST);
        } else if (model_n >= slots / 2) {
          CHECK(rc == -ENOSPC);
        } else {
          CHECK(rc == 0);
          model[model_n].hash = h;
          model[model_n].key = key;
          model[model_n++].value = id;
          if (id < count)
            st[id].last_seen = now;
        }
      } else {
        rc = pptk_flow_table_delete(t, &key, h);
        CHECK(rc == (at >= 0 ? 0 : -ENOENT));
        if (at >= 0)
          model[at] = model[--model_n];
      }
    }
    for (i = 0; i < 20; i++) {   /* traffic */
      const uint32_t id = rnd() % universe;
      if (id < count && st[id].last_seen < now)
        st[id].last_seen = now;
    }
    for (j = 0; j < model_n; j++)
      want_n += model[j].value < count && idle_rule(st[model[j].value].last_seen, idle, now);
    cap = rnd() % 3 ? slots : rnd() % 4;
    /* call until a call returns less than cap (cap 0: once) */
    do {
      rc = pptk_flow_table_expire(t, st, count, now, idle, out + got_n, cap);
      CHECK(rc >= 0 && (uint32_t)rc <= cap);
      if (rc < 0)
        break;
      for (k = 0; k < (uint32_t)rc; k++) {
        const uint32_t v = out[got_n + k];
        int at = -1;
        for (j = 0; j < model_n; j++)
          if (model[j].value == v)
            at = (int)j;
        CHECK(at >= 0 && v < count && idle_rule(st[v].last_seen, idle, now));
        if (at >= 0) {
          CHECK(pptk_flow_table_find(t, &model[at].key, model[at].hash, NULL) == -ENOENT);
          model[at] = model[--model_n];
        }
      }
      got_n += (uint32_t)rc;
    } while (cap && (uint32_t)rc == cap);
    CHECK(got_n == (cap ? want_n : 0));
    total += got_n;
    pptk_flow_table_stats(t, NULL, &cnt, NULL);
    CHECK(cnt == model_n);
    for (j = 0; j < model_n; j++) {
      uint32_t got = ~0u;
      CHECK(pptk_flow_table_find(t, &model[j].key, model[j].hash, &got) == 0 &&
            got == model[j].value);
    }
  }
  CHECK(total > rounds / 4);
  pptk_flow_table_destroy(t);
  free(model);
  free(st);
  free(out);
}

static void run_wrap_subsets(void)
{
  struct pptk_flow_key k[6];
  const uint64_t h = 0xabcdef000000000eull;   /* home slot 14 of 16: slots 14, 15, 0, 1, 2 */
  uint32_t sub, i, out[8], got;

  for (i = 0; i < 6; i++) {
    memset(&k[i], 0, sizeof(k[i]));
    k[i].dst[2] = (uint8_t)(i + 1);
    k[i].proto = 17;
  }
  for (sub = 0; sub < 32; sub++) {
    struct pptk_flow_table *t = NULL;
    struct pptk_flow_stats *st = stats_new(5);   /* value 5 lies past it */
    int rc, n = 0;
    CHECK(pptk_flow_table_create(NULL, 16, &t) == 0 && t);
    if (!t)
      return;
    for (i = 0; i < 5; i++) {
      CHECK(pptk_flow_table_insert(t, &k[i], h, i) == 0);
      st[i].last_seen = (sub >> i) & 1 ? 10 : 100;
      n += (sub >> i) & 1;
    }
    CHECK(pptk_flow_table_insert(t, &k[5], 0x10, 5) == 0);   /* home slot 0, pushed to 3 */
    rc = pptk_flow_table_expire(t, st, 5, 111, 100, out, 8);
    CHECK(rc == n);
    for (i = 0; i < 5; i++) {
      got = 77;
      rc = pptk_flow_table_find(t, &k[i], h, &got);
      CHECK((sub >> i) & 1 ? rc == -ENOENT : (rc == 0 && got == i));
    }
    CHECK(pptk_flow_table_find(t, &k[5], 0x10, &got) == 0 && got == 5);
    CHECK(pptk_flow_table_expire(t, st, 5, 111, 100, out, 8) == 0);
    pptk_flow_table_destroy(t);
    free(st);
  }
}

static void run_boundaries(void)
{
  struct pptk_flow_table *t = NULL;
  struct pptk_flow_key k[3];
  struct pptk_flow_stats *st = stats_new(2);
  uint32_t i, out[4];

  CHECK(pptk_flow_table_create(NULL, 16, &t) == 0 && t);
  if (!t)
    return;
  for (i = 0; i < 3; i++) {
    memset(&k[i], 0, sizeof(k[i]));
    k[i].src[5] = (uint8_t)(i + 1);
    k[i].proto = 6;
    CHECK(pptk_flow_table_insert(t, &k[i], 0x40 + i, i) == 0);   /* value 2 lies past the array */
  }
  st[0].last_seen = 5000000;
  st[1].last_seen = ~0ull - 4;
  CHECK(pptk_flow_table_expire(t, st, 2, 35000000, 30000000, out, 4) == 0);   /* == : stays */
  CHECK(pptk_flow_table_expire(t, st, 2, 35000001, 30000000, NULL, 0) == 0);  /* cap 0 */
  CHECK(pptk_flow_table_expire(t, st, 2, 35000001, 30000000, out, 4) == 1 && out[0] == 0);
  CHECK(pptk_flow_table_expire(t, st, 2, ~0ull, 100, out, 4) == 0);           /* the sum wraps */
  CHECK(pptk_flow_table_expire(t, st, 2, 3, 100, out, 4) == 0);
  st[1].last_seen = 0;
  CHECK(pptk_flow_table_expire(t, st, 2, ~0ull, 1, out, 4) == 1 && out[0] == 1);
  CHECK(pptk_flow_table_find(t, &k[2], 0x42, NULL) == 0);                     /* never expires */
  CHECK(pptk_flow_table_expire(NULL, st, 2, 1, 1, out, 4) == -EINVAL);
  CHECK(pptk_flow_table_expire(t, NULL, 2, 1, 1, out, 4) == -EINVAL);
  CHECK(pptk_flow_table_expire(t, st, 2, 1, 1, NULL, 4) == -EINVAL);
  pptk_flow_table_destroy(t);
  free(st);
}

int main(void)
{
  run_account();
  run_expire(64, 60, 12, 3000);
  run_expire(256, 200, 40, 3000);
  run_wrap_subsets();
  run_boundaries();
  if (failures) {
    printf("flowstate: %d failures\n", failures);
    return 1;
  }
  printf("flowstate ok\n");
  return 0;
}
