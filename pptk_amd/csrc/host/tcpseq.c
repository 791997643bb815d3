/*
 * tcpseq.c -- pptk_tcp_seq_translate_hdr: the per-packet host form of
 * pptk_tcp_seq_translate_device (include/pptk_rx.h), composed from the kept
 * per-packet functions of include/ipcksum.h and the walks of tcpopt.c in the
 * contract's fixed order.
 *
 * The kept functions fold a field at an odd TCP offset into the checksum
 * through the words that straddle it, and the last of those words may reach
 * one byte past the options -- past the segment when the segment has no
 * payload.  That byte cancels exactly in the RFC 1624 sum (~old + new with
 * the same low byte does not depend on it), so the header is worked on in a
 * zero-padded copy and only bytes [0, data offset) go back: no byte at or
 * past seglen is read, none at or past the data offset is written.
 */
#include <stdint.h>
#include <string.h>

#include "iphdr.h"
#include "ipcksum.h"
#include "pptk_rx.h"

uint32_t pptk_tcp_seq_translate_hdr(void *tcphdr, uint32_t seglen, const struct pptk_seqxlate *x)
{
  unsigned char w[64];   /* data offset <= 60, and the straddling byte */
  struct sack_ts_headers h;
  uint32_t st = PPTK_SEQ_ST_TCP;
  size_t end;
  if (seglen < 20)       /* no room for the data offset byte's header */
    return PPTK_SEQ_ST_BADOPT;
  end = tcp_data_offset(tcphdr);
  if (end < 20 || end > seglen)
    return PPTK_SEQ_ST_BADOPT;
  memcpy(w, tcphdr, end);
  memset(w + end, 0, sizeof(w) - end);
  if (x->ops & PPTK_SEQ_SEQ) {
    tcp_set_seq_number_cksum_update(w, 0, tcp_seq_number(w) + x->seq_add);
    st |= PPTK_SEQ_ST_SEQ;
  }
  if ((x->ops & PPTK_SEQ_ACK) && (w[13] & 0x10)) {
    tcp_set_ack_number_cksum_update(w, 0, tcp_ack_number(w) + x->ack_add);
    st |= PPTK_SEQ_ST_ACK;
  }
  if (x->ops & (PPTK_SEQ_SACK | PPTK_SEQ_TSVAL | PPTK_SEQ_TSECHO)) {
    tcp_find_sack_ts_headers(w, &h);
    if (x->ops & PPTK_SEQ_SACK) {
      tcp_adjust_sack_cksum_update_2(w, &h, x->sack_add);
      if (h.sackoff != 0)
        st |= PPTK_SEQ_ST_SACK;
    }
    if (x->ops & PPTK_SEQ_TSVAL)
      tcp_adjust_tsval_cksum_update(w, &h, x->tsval_add);
    if (x->ops & PPTK_SEQ_TSECHO)
      tcp_adjust_tsecho_cksum_update(w, &h, x->tsecho_add);
    if ((x->ops & (PPTK_SEQ_TSVAL | PPTK_SEQ_TSECHO)) && h.tsoff != 0)
      st |= PPTK_SEQ_ST_TS;
  }
  if (x->ops & PPTK_SEQ_SACK_OFF) {
    size_t sacklen = 0;
    int aligned = 0;
    void *sack = tcp_find_sack_header(w, &sacklen, &aligned);
    if (sack) {
      tcp_disable_sack_cksum_update(w, sack, sacklen, aligned);
      st |= PPTK_SEQ_ST_SACK_OFF;
    }
  }
  memcpy(tcphdr, w, end);
  return st;
}
