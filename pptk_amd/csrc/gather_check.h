/*
 * gather_check.h -- the argument rules and the two small statements of "Egress
 * gather" (include/pptk_rx.h) that the host call (host/gather.c) and the
 * device call (tx_gather.hip) share: one statement, so the two cannot drift
 * apart.  Plain C, no HIP.
 */
#ifndef PPTK_GATHER_CHECK_H
#define PPTK_GATHER_CHECK_H

#include <errno.h>
#include <stdint.h>

#include "pptk_rx.h"

/* 0, or -EINVAL for everything the contract rejects on both calls */
static inline int pptk_gather_check(const struct pptk_gather *g)
{
  if (!g || !g->ports || !g->hdr)
    return -EINVAL;
  if (g->nports == 0 || g->nports > PPTK_PORT_MAX || (!g->runs && g->nports != 1))
    return -EINVAL;
  if (g->max_entries >= (1ull << 32) || g->n >= (1ull << 32))
    return -EINVAL;
  /* the source batch, as every batch op takes it (rx_internal.h frame_batch_ok) */
  if (g->n && !(g->frames && (g->off || g->stride || g->n == 1) && (g->len || g->fixed_len <= 65535)))
    return -EINVAL;
  if ((!g->out && g->out_cap) || ((uintptr_t)g->out & (PPTK_GATHER_REGION_ALIGN - 1)))
    return -EINVAL;
  if (((uintptr_t)g->list & 3u) || ((uintptr_t)g->off & 7u) || ((uintptr_t)g->pk_off & 7u) ||
      ((uintptr_t)g->runs & 7u) || ((uintptr_t)g->ports & 7u) || ((uintptr_t)g->hdr & 7u) ||
      ((uintptr_t)g->d_entries & 7u) || ((uintptr_t)g->len & 1u) || ((uintptr_t)g->pk_len & 1u))
    return -EINVAL;
  return 0;
}

/* whether run p follows the runs before it: back to back from 0, no sum wrapping */
static inline int pptk_gather_run_ok(const struct pptk_dispatch_port *runs, uint32_t p)
{
  if (runs[p].start + runs[p].count < runs[p].start)
    return 0;
  return runs[p].start == (p ? runs[p - 1].start + runs[p - 1].count : 0);
}

#endif
