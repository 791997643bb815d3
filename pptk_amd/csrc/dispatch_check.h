/*
 * dispatch_check.h -- the argument rules of "Egress dispatch"
 * (include/pptk_rx.h) that the host call (host/dispatch.c) and the device call
 * (tx_dispatch.hip) share: one statement, so the two cannot drift apart.
 */
#ifndef PPTK_DISPATCH_CHECK_H
#define PPTK_DISPATCH_CHECK_H

#include <errno.h>
#include <stdint.h>

#include "pptk_rx.h"

static inline int pptk_dispatch_code_ok(uint32_t code, uint32_t nports)
{
  return code < nports || code == PPTK_PORT_FLOOD || code == PPTK_PORT_DROP;
}

/* 0, or -EINVAL for everything the contract rejects on both calls */
static inline int pptk_dispatch_check(const struct pptk_dispatch *d)
{
  if (!d || !d->ports || !d->hdr)
    return -EINVAL;
  if (d->nports == 0 || d->nports > PPTK_PORT_MAX || d->n >= (1ull << 32))
    return -EINVAL;
  if (d->n && !d->port == !d->idx)
    return -EINVAL;
  if (d->idx && !d->flow_port && d->flows)
    return -EINVAL;
  if (!pptk_dispatch_code_ok(d->miss_code, d->nports))
    return -EINVAL;
  if (d->cap && !d->list)
    return -EINVAL;
  if (((uintptr_t)d->idx & 3u) || ((uintptr_t)d->list & 3u) || ((uintptr_t)d->off & 7u) ||
      ((uintptr_t)d->out_off & 7u) || ((uintptr_t)d->ports & 7u) || ((uintptr_t)d->hdr & 7u) ||
      ((uintptr_t)d->len & 1u) || ((uintptr_t)d->out_len & 1u))
    return -EINVAL;
  return 0;
}

#endif
