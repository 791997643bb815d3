/*
 * dispatch.c -- pptk_tx_dispatch_host, the CPU statement of "Egress dispatch"
 * (include/pptk_rx.h): the per-port tx lists of a batch, which the device
 * call (tx_dispatch.hip) must equal byte for byte.  It is the tail of the
 * reference's switch loop (ldp/ldpswitch.c:296-318: a known destination goes
 * to its port, an unknown one to every port but the ingress port) stated
 * over a batch, with the per-port tables laid back to back in one list.  Two
 * passes -- count, then place -- and nothing allocated beyond the stack.
 * Plain C; no HIP, no recursion: a program may link this file alone.
 */
#include <string.h>

#include "../dispatch_check.h"

_Static_assert(sizeof(struct pptk_dispatch_port) == 32, "a port entry is 32 bytes");
_Static_assert(sizeof(struct pptk_dispatch_hdr) == 64, "the header is 64 bytes");
_Static_assert(sizeof(struct pptk_dispatch) == 152, "the argument block is 152 bytes");

enum { DROPPED = 0x100, BAD = 0x101, FLOOD = 0x102 };

/* the port of a unicast frame, or DROPPED / BAD / FLOOD */
static uint32_t classify(const struct pptk_dispatch *d, uint64_t i)
{
  uint32_t code;
  if (d->subject && d->subject[i] == 0)
    return DROPPED;
  if (d->port)
    code = d->port[i];
  else if (d->idx[i] == PPTK_FLOW_NONE)
    code = d->miss_code;
  else if (d->idx[i] >= d->flows)
    return BAD;
  else
    code = d->flow_port[d->idx[i]];
  if (code < d->nports)
    return code;
  if (code == PPTK_PORT_FLOOD)
    return FLOOD;
  return code == PPTK_PORT_DROP ? DROPPED : BAD;
}

int pptk_tx_dispatch_host(const struct pptk_dispatch *d)
{
  struct pptk_dispatch_port port[PPTK_PORT_MAX];
  struct pptk_dispatch_hdr hdr;
  uint64_t at[PPTK_PORT_MAX];   /* where the next entry of each run goes */
  uint64_t i, total = 0;
  uint32_t p, np;
  int rc = pptk_dispatch_check(d);
  if (rc)
    return rc;
  np = d->nports;
  memset(port, 0, sizeof(port));
  memset(&hdr, 0, sizeof(hdr));
  for (i = 0; i < d->n; i++) {
    const uint32_t c = classify(d, i);
    const uint32_t in = d->in_port ? d->in_port[i] : d->in_port_all;
    const uint64_t len = d->len ? d->len[i] : d->fixed_len;
    if (c == DROPPED) {
      hdr.dropped++;
    } else if (c == BAD) {
      hdr.bad++;
    } else if (c == FLOOD) {
      hdr.flood++;
      for (p = 0; p < np; p++) {
        if (p != in) {
          port[p].count++;
          port[p].bytes += len;
          port[p].flooded++;
        }
      }
    } else {
      hdr.unicast++;
      hdr.hairpin += c == in;
      port[c].count++;
      port[c].bytes += len;
    }
  }
  for (p = 0; p < np; p++) {
    port[p].start = at[p] = total;
    total += port[p].count;
  }
  hdr.total = total;
  hdr.written = total < d->cap ? total : d->cap;
  for (i = 0; i < d->n && d->cap; i++) {
    const uint32_t c = classify(d, i);
    const uint32_t in = d->in_port ? d->in_port[i] : d->in_port_all;
    uint32_t first = c, last = c + 1;   /* the ports frame i goes to: [first, last) less `in` */
    if (c == DROPPED || c == BAD)
      continue;
    if (c == FLOOD)
      first = 0, last = np;
    for (p = first; p < last; p++) {
      uint64_t g;
      if (c == FLOOD && p == in)
        continue;
      g = at[p]++;
      if (g >= d->cap)
        continue;
      d->list[g] = (uint32_t)i;
      if (d->out_off)
        d->out_off[g] = d->off ? d->off[i] : i * d->stride;
      if (d->out_len)
        d->out_len[g] = d->len ? d->len[i] : (uint16_t)d->fixed_len;
    }
  }
  memcpy(d->ports, port, np * sizeof(port[0]));
  memcpy(d->hdr, &hdr, sizeof(hdr));
  return 0;
}
