/*
 * ipreass.c -- pptk_ip_reass_host: batch-local IPv4 reassembly, the CPU
 * statement of pptk_ip_reass_device's contract (include/pptk_rx.h "IPv4
 * reassembly"); the device call (ip_reass.hip) must equal it byte for byte.
 * The slot it builds is what the reference's reassctx_reassemble writes
 * (ipfrag/ipreass.c:61-86) through the same iphdr.h / ipcksum.h calls; what
 * differs from the reference is stated in the header: no state across
 * batches, at most 64 fragments per datagram, and overlapping fragments are
 * reported, never merged.  Plain C; a program may link this file with
 * ipcksum.c alone.
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "ipcksum.h"
#include "iphdr.h"
#include "pptk_rx.h"

_Static_assert(sizeof(struct pptk_reass_dgram) == 16, "a report entry is 16 bytes");
_Static_assert(sizeof(struct pptk_reass_hdr) == 48, "the header is 48 bytes");
_Static_assert(sizeof(struct pptk_rx_frag) == 16, "struct pptk_rx_frag is 16 bytes");

#define REASS_MAX_FRAGS 64u
#define REASS_NONE 0xffffffffu

struct reass_cand {
  uint32_t frame;   /* frame index */
  uint32_t src, dst, pi;   /* the key: addresses as stored, proto | ident << 8 */
  uint32_t dg;      /* its datagram */
  uint16_t off, dl;
  uint8_t l2, ihl, mf;
};

struct reass_dg {
  uint32_t lead;    /* candidate number of the leader */
  uint32_t count;   /* members */
  uint32_t start;   /* of its run in the member array */
  uint32_t fill;
};

static const uint8_t *frame_at(const uint8_t *frames, const uint64_t *off, uint64_t stride,
                               uint64_t i)
{
  return frames + (off ? off[i] : i * stride);
}

int pptk_ip_reass_host(const uint8_t *frames, const uint64_t *off, const uint16_t *len,
                       uint64_t stride, uint32_t fixed_len, uint64_t n,
                       const struct pptk_rx_rec *recs, const struct pptk_rx_frag *frag,
                       uint64_t max_candidates, uint8_t *out, uint64_t out_stride,
                       uint64_t out_cap, uint16_t *out_len, struct pptk_reass_dgram *report,
                       uint64_t report_cap, uint32_t *dgram, uint8_t *fstatus,
                       struct pptk_reass_hdr *hdr)
{
  struct reass_cand *cand = NULL;
  struct reass_dg *dg = NULL;
  uint32_t *map = NULL, *mem = NULL;
  uint64_t i, candidates = 0, considered, ndg = 0, size, complete = 0, slots = 0;
  uint32_t r, k;
  int rc = -ENOMEM;

  if (!hdr || ((uintptr_t)hdr & 7u) || n > (1ull << 24) || max_candidates == 0 ||
      max_candidates > (1ull << 24) || (out_stride & 15u) || ((uintptr_t)out & 15u) ||
      out_cap > 0xffffffffull || report_cap > 0xffffffffull || ((uintptr_t)report & 3u) ||
      ((uintptr_t)dgram & 3u))
    return -EINVAL;
  if (n && (!frames || !recs || !frag || !dgram || !fstatus || (!off && stride == 0 && n > 1) ||
            (!len && fixed_len > 65535)))
    return -EINVAL;
  if ((out_cap && (!out || !out_len)) || (report_cap && !report))
    return -EINVAL;
  memset(hdr, 0, sizeof(*hdr));
  if (n == 0)
    return 0;

  /* per frame: fragment, rejected, candidate */
  for (i = 0; i < n; i++) {
    const uint32_t fl = recs[i].flags, flen = len ? len[i] : fixed_len;
    const uint32_t l3 = recs[i].l3_off, fo = frag[i].frag_off, dl = frag[i].data_len;
    uint8_t st = 0;
    dgram[i] = REASS_NONE;
    if ((fl & (PPTK_RX_F_PARSED | PPTK_RX_F_FRAGMENT | PPTK_RX_F_MALFORMED | PPTK_RX_F_IPV6)) ==
        (PPTK_RX_F_PARSED | PPTK_RX_F_FRAGMENT)) {
      st = PPTK_REASS_FST_FRAG;
      if (recs[i].ip_cksum != 0)
        st |= PPTK_REASS_FST_BADCKSUM;
      if ((l3 != 14 && l3 != 18) || flen <= l3) {
        st |= PPTK_REASS_FST_BADFRAG;
      } else {
        const uint32_t ihl = ip_hdr_len(frame_at(frames, off, stride, i) + l3);
        if (ihl < 20 || dl == 0 || fo + dl > 65535 ||
            ((frag[i].flags & PPTK_RX_FRAG_MF) && dl % 8 != 0) || l3 + ihl + dl > flen)
          st |= PPTK_REASS_FST_BADFRAG;
      }
      if (st == PPTK_REASS_FST_FRAG)
        candidates++;
    }
    fstatus[i] = st;
  }
  considered = candidates < max_candidates ? candidates : max_candidates;
  hdr->candidates = candidates;
  hdr->considered = considered;

  /* the map is at most half full, so a probe always ends */
  for (size = 16; size < 2 * considered; size <<= 1)
    ;
  cand = malloc((considered ? considered : 1) * sizeof(*cand));
  dg = malloc((considered ? considered : 1) * sizeof(*dg));
  mem = malloc((considered ? considered : 1) * sizeof(*mem));
  map = calloc(size, sizeof(*map));   /* 1 + datagram number, 0 = unused */
  if (!cand || !dg || !mem || !map)
    goto done;

  /* the considered candidates and their datagrams, in first-appearance =
   * ascending leader order */
  r = 0;
  for (i = 0; i < n; i++) {
    struct reass_cand *c;
    uint64_t s, d;
    if (fstatus[i] != PPTK_REASS_FST_FRAG)
      continue;
    if (r >= considered) {
      fstatus[i] |= PPTK_REASS_FST_SKIPPED;
      continue;
    }
    c = &cand[r];
    c->frame = (uint32_t)i;
    memcpy(&c->src, recs[i].src, 4);
    memcpy(&c->dst, recs[i].dst, 4);
    c->pi = recs[i].proto | (frag[i].ident & 0xffffu) << 8;
    c->off = frag[i].frag_off;
    c->dl = frag[i].data_len;
    c->l2 = recs[i].l3_off;
    c->ihl = (uint8_t)ip_hdr_len(frame_at(frames, off, stride, i) + c->l2);
    c->mf = (frag[i].flags & PPTK_RX_FRAG_MF) != 0;
    s = (c->src * 0x9e3779b1u ^ c->dst * 0x85ebca6bu ^ c->pi * 0xc2b2ae35u) & (size - 1);
    for (d = 0; d < size; d++, s = (s + 1) & (size - 1)) {
      const struct reass_cand *l;
      if (!map[s])
        break;
      l = &cand[dg[map[s] - 1].lead];
      if (l->src == c->src && l->dst == c->dst && l->pi == c->pi)
        break;
    }
    if (!map[s]) {
      map[s] = (uint32_t)ndg + 1;
      dg[ndg].lead = r;
      dg[ndg].count = 0;
      ndg++;
    }
    c->dg = map[s] - 1;
    dg[c->dg].count++;
    fstatus[i] |= PPTK_REASS_FST_MEMBER;
    dgram[i] = c->dg;
    r++;
  }
  hdr->dgrams = ndg;
  hdr->reported = ndg < report_cap ? ndg : report_cap;

  /* members of each datagram, in candidate order */
  for (k = 0, r = 0; k < ndg; k++) {
    dg[k].start = r;
    dg[k].fill = 0;
    r += dg[k].count;
  }
  for (r = 0; r < considered; r++) {
    struct reass_dg *g = &dg[cand[r].dg];
    mem[g->start + g->fill++] = r;
  }

  for (k = 0; k < ndg; k++) {
    const struct reass_dg *g = &dg[k];
    const struct reass_cand *lead = &cand[g->lead];
    uint32_t m[REASS_MAX_FRAGS] = {0}, a, b, total = 0, olen = 0, slot = REASS_NONE;
    uint8_t st;
    if (g->count > REASS_MAX_FRAGS) {
      st = PPTK_REASS_DG_TOOMANY;
    } else {
      uint32_t nolast = 0;
      int overlap = 0, gap = 0;
      /* order by (off, frame index); the run is in index order already */
      for (a = 0; a < g->count; a++) {
        const uint32_t x = mem[g->start + a];
        for (b = a; b > 0 && cand[m[b - 1]].off > cand[x].off; b--)
          m[b] = m[b - 1];
        m[b] = x;
      }
      for (a = 0; a < g->count; a++) {
        const struct reass_cand *c = &cand[m[a]];
        if (!c->mf) {
          nolast++;
          if (a + 1 < g->count)
            overlap = 1;
        }
        if (a + 1 < g->count) {
          const uint32_t end = (uint32_t)c->off + c->dl, next = cand[m[a + 1]].off;
          if (end > next)
            overlap = 1;
          if (end < next)
            gap = 1;
        }
      }
      if (overlap || nolast > 1)
        st = PPTK_REASS_DG_OVERLAP;
      else if (nolast == 0 || cand[m[0]].off != 0 || gap)
        st = PPTK_REASS_DG_INCOMPLETE;
      else
        st = PPTK_REASS_DG_COMPLETE;
    }
    if (st == PPTK_REASS_DG_COMPLETE) {
      const uint32_t l2 = lead->l2, ihl = lead->ihl;
      uint32_t flen;
      complete++;
      total = (uint32_t)cand[m[g->count - 1]].off + cand[m[g->count - 1]].dl;
      flen = l2 + ihl + total;
      if (flen <= 65535)
        olen = flen;
      if (flen > 65535 || (((uint64_t)flen + 15u) & ~15ull) > out_stride) {
        st |= PPTK_REASS_DG_TOOBIG;
      } else if (slots >= out_cap) {
        st |= PPTK_REASS_DG_NOROOM;
        slots++;
      } else {
        /* ipreass.c:61-86 */
        unsigned char *s = out + slots * out_stride;
        void *ip2 = s + l2;
        slot = (uint32_t)slots++;
        st |= PPTK_REASS_DG_WRITTEN;
        memcpy(s, frame_at(frames, off, stride, lead->frame), l2 + ihl);
        ip_set_frag_off(ip2, 0);
        ip_set_more_frags(ip2, 0);
        ip_set_total_len(ip2, (uint16_t)(ihl + total));
        ip_set_hdr_cksum_calc(ip2, (uint16_t)ihl);
        for (a = 0; a < g->count; a++) {
          const struct reass_cand *c = &cand[m[a]];
          memcpy(s + l2 + ihl + c->off,
                 frame_at(frames, off, stride, c->frame) + c->l2 + c->ihl, c->dl);
        }
        memset(s + flen, 0, (16u - flen % 16u) % 16u);
        out_len[slot] = (uint16_t)flen;
        for (a = 0; a < g->count; a++)
          fstatus[cand[m[a]].frame] |= PPTK_REASS_FST_DONE;
      }
    }
    if (k < report_cap) {
      report[k].first = lead->frame;
      report[k].slot = slot;
      report[k].frags = g->count;
      report[k].out_len = (uint16_t)olen;
      report[k].status = st;
      report[k].reserved = 0;
    }
  }
  hdr->complete = complete;
  hdr->written = slots < out_cap ? slots : out_cap;
  rc = 0;
done:
  free(map);
  free(mem);
  free(dg);
  free(cand);
  return rc;
}
