/* flowtab.h -- the flow table's private layout, shared between its host half
 * (host/flowtab.c, plain C) and its device half (rx_flow.hip). */
#ifndef PPTK_FLOWTAB_H
#define PPTK_FLOWTAB_H

#include <stdint.h>

#include "../../include/pptk_rx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One slot: 64 bytes, 64-byte aligned, so a probe is one aligned 64-byte
 * read.  Its first 44 bytes are laid out as bytes 0..43 of struct
 * pptk_rx_rec (flow_hash, src, dst, sport, dport): a lookup compares them
 * 16 bytes at a time with the record as it lies in memory. */
struct pptk_flow_slot {
  uint64_t hash;        /*  0 the flow_hash given at insert                 */
  uint8_t src[16];      /*  8                                               */
  uint8_t dst[16];      /* 24                                               */
  uint16_t sport;       /* 40                                               */
  uint16_t dport;       /* 42                                               */
  uint8_t proto;        /* 44                                               */
  uint8_t used;         /* 45 1 = in use; an unused slot is all zero        */
  uint8_t pad[2];       /* 46 zero                                          */
  uint32_t value;       /* 48                                               */
  uint8_t fill[12];     /* 52 zero                                          */
};

#define PPTK_FLOW_MIN_SLOTS 16u
#define PPTK_FLOW_MAX_SLOTS (1u << 26)
#define PPTK_FLOW_PAGE_SLOTS 64u   /* dirty tracking: 4 KB of image */

struct pptk_flow_table {
  struct pptk_flow_slot *img;   /* slots entries, 64-byte aligned */
  uint32_t slots, count;
  uint32_t probe_limit;         /* 0, or 1 + the largest displacement since clear */
  uint64_t *dirty;              /* one bit per page of PPTK_FLOW_PAGE_SLOTS slots */
  uint32_t pages;
  /* device half (all zero for a host-only table) */
  struct pptk_rx_ctx *ctx;
  int device;
  void *d_img;                  /* hipMalloc image of slots entries */
  int synced;                   /* a sync has completed */
  uint32_t d_probe_limit;       /* probe_limit of the image as of the last sync */
};

/* The device half, defined in rx_flow.hip and referenced weakly by
 * host/flowtab.c: a program that links that file alone has neither, and a
 * table with a context is then -ENOSYS. */
int pptk_flowtab_dev_attach(struct pptk_flow_table *t, struct pptk_rx_ctx *ctx);
void pptk_flowtab_dev_release(struct pptk_flow_table *t);

#ifdef __cplusplus
}
#endif
#endif
