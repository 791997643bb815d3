/*
 * gather.c -- pptk_tx_gather_host, the CPU statement of "Egress gather"
 * (include/pptk_rx.h): each port's tx list packed into one region of `out`,
 * which the device call (tx_gather.hip) must equal byte for byte.  It is the
 * reference's per-port copy (ldp_out_inject, ldp/ldpnetmap.c:68 and
 * ldp/ldpdpdk.c:256, called once per port from ldp/ldpswitch.c:311-318)
 * stated over a batch: a loop over ports and entries with memcpy and memset.
 * Two passes -- size the regions, then place and copy -- and nothing
 * allocated beyond the stack.  Plain C; no HIP, no recursion: a program may
 * link this file alone.
 */
#include <string.h>

#include "../gather_check.h"

_Static_assert(sizeof(struct pptk_gather_port) == 32, "a port entry is 32 bytes");
_Static_assert(sizeof(struct pptk_gather_hdr) == 64, "the header is 64 bytes");
_Static_assert(sizeof(struct pptk_gather) == 136, "the argument block is 136 bytes");

/* the frame of entry e: its length (0 for a bad entry) and where it lies */
static uint32_t entry_len(const struct pptk_gather *g, uint64_t e, const uint8_t **src)
{
  const uint64_t i = g->list ? g->list[e] : e;
  *src = NULL;
  if (i >= g->n)
    return 0;
  *src = g->frames + (g->off ? g->off[i] : i * g->stride);
  return g->len ? g->len[i] : g->fixed_len;
}

static uint64_t round_up(uint64_t x, uint64_t a)
{
  return (x + a - 1) & ~(a - 1);
}

int pptk_tx_gather_host(const struct pptk_gather *g)
{
  struct pptk_gather_port port[PPTK_PORT_MAX];
  struct pptk_gather_hdr hdr;
  uint64_t first[PPTK_PORT_MAX + 1];   /* port p's considered entries: [first[p], first[p + 1]) */
  uint64_t entries, e, at = 0;
  uint32_t p, np;
  int rc = pptk_gather_check(g);
  if (rc)
    return rc;
  np = g->nports;
  memset(port, 0, sizeof(port));
  memset(&hdr, 0, sizeof(hdr));
  if (g->max_entries == 0)
    goto done;
  entries = g->max_entries;
  if (g->d_entries && *g->d_entries < entries)
    entries = *g->d_entries;
  if (g->runs) {
    for (p = 0; p < np; p++) {
      if (!pptk_gather_run_ok(g->runs, p)) {
        hdr.status = PPTK_GATHER_ST_BADRUNS;
        goto done;
      }
    }
    if (g->runs[np - 1].start + g->runs[np - 1].count < entries)
      entries = g->runs[np - 1].start + g->runs[np - 1].count;
  }
  for (p = 0; p < np; p++)
    first[p] = g->runs && g->runs[p].start < entries ? g->runs[p].start : g->runs ? entries : 0;
  first[np] = entries;
  /* the regions: every considered entry counts, whether or not it fits */
  for (p = 0; p < np; p++) {
    const uint8_t *src;
    port[p].start = at;
    port[p].entries = first[p + 1] - first[p];
    for (e = first[p]; e < first[p + 1]; e++)
      at += round_up(entry_len(g, e, &src), PPTK_GATHER_SLOT_ALIGN);
    hdr.need = at;
    at = round_up(at, PPTK_GATHER_REGION_ALIGN);
  }
  hdr.entries = entries;
  for (p = 0; p < np; p++) {
    at = port[p].start;
    for (e = first[p]; e < first[p + 1]; e++) {
      const uint8_t *src;
      const uint32_t len = entry_len(g, e, &src);
      const uint64_t slot = round_up(len, PPTK_GATHER_SLOT_ALIGN);
      hdr.bad += src == NULL;
      if (g->pk_off)
        g->pk_off[e] = at;
      if (g->pk_len)
        g->pk_len[e] = (uint16_t)len;
      /* at + slot never decreases, so the entries that fit are a prefix */
      if (at + slot <= g->out_cap) {
        if (len) {
          memcpy(g->out + at, src, len);
          memset(g->out + at + len, 0, slot - len);
        }
        hdr.packed++;
        hdr.frame_bytes += len;
        port[p].packed++;
        port[p].bytes += slot;
      }
      at += slot;
    }
    hdr.bytes += port[p].bytes;
  }
done:
  memcpy(g->ports, port, np * sizeof(port[0]));
  memcpy(g->hdr, &hdr, sizeof(hdr));
  return 0;
}
