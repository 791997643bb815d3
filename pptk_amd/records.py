"""Record formats of the rx transform: numpy views of ``struct pptk_rx_rec``
(64 bytes per frame) and ``struct pptk_rx_rec32`` (32 bytes), little-endian
(include/pptk_rx.h)."""
import numpy as np

REC_DTYPE = np.dtype([
    ("flow_hash", "<u8"),
    ("src", "u1", 16),
    ("dst", "u1", 16),
    ("sport", "<u2"),
    ("dport", "<u2"),
    ("ip_cksum", "<u2"),
    ("l4_cksum", "<u2"),
    ("l4_off", "<u2"),
    ("l4_len", "<u2"),
    ("l3_off", "u1"),
    ("proto", "u1"),
    ("flags", "<u2"),
    ("src_bucket", "<u4"),
    ("ethertype", "<u2"),
    ("ip_version", "u1"),
    ("reserved", "u1"),
])
assert REC_DTYPE.itemsize == 64

# struct pptk_rewrite (pptk_tx_rewrite_device): ops, new src/dst (host
# order), new ports (host order)
REWRITE_DTYPE = np.dtype([("ops", "<u4"), ("src", "<u4"), ("dst", "<u4"),
                          ("sport", "<u2"), ("dport", "<u2")])
assert REWRITE_DTYPE.itemsize == 16
RW_DECR_TTL, RW_SRC, RW_DST, RW_SPORT, RW_DPORT = 0x1, 0x2, 0x4, 0x8, 0x10
RW_ST_IP, RW_ST_L4, RW_ST_TTL_ZERO, RW_ST_EXPIRED, RW_ST_ICMP = 0x1, 0x2, 0x4, 0x8, 0x10
RW_ST_NOFLOW = 0x80   # pptk_tx_rewrite_flow_device: idx[i] >= rw_count, frame untouched
RW_ICMP_ID = 0x20
MSS_SYN_ONLY = 0x1
MSS_ST_TCP, MSS_ST_FOUND, MSS_ST_CLAMPED, MSS_ST_BADOPT = 0x1, 0x2, 0x4, 0x8
# struct pptk_seqxlate (pptk_tcp_seq_translate_device / _hdr): ops and the
# per-flow offsets added to seq, ack, the SACK block edges and the timestamps
seqxlate_dtype = np.dtype([("ops", "<u4"), ("seq_add", "<u4"), ("ack_add", "<u4"),
                           ("sack_add", "<u4"), ("tsval_add", "<u4"), ("tsecho_add", "<u4")])
assert seqxlate_dtype.itemsize == 24
SEQ_SEQ, SEQ_ACK, SEQ_SACK, SEQ_TSVAL, SEQ_TSECHO, SEQ_SACK_OFF = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
(SEQ_ST_TCP, SEQ_ST_SEQ, SEQ_ST_ACK, SEQ_ST_SACK, SEQ_ST_TS, SEQ_ST_SACK_OFF, SEQ_ST_BADOPT,
 SEQ_ST_NOFLOW) = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80
SEQ_NOFLOW = 0xFFFFFFFF   # d_idx entry meaning "no flow"
# PPTK_FRAG_ST_*: per-frame status of pptk_ip_fragment_device / _host
(FRAG_ST_IPV4, FRAG_ST_FITS, FRAG_ST_DONE, FRAG_ST_DF, FRAG_ST_ISFRAG, FRAG_ST_BADCKSUM,
 FRAG_ST_NOROOM) = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40
# pptk_ip_reass_device / _host: per-frame status bits, per-datagram status bits,
# struct pptk_reass_dgram (one report entry) and struct pptk_reass_hdr
(REASS_FST_FRAG, REASS_FST_BADCKSUM, REASS_FST_BADFRAG, REASS_FST_SKIPPED, REASS_FST_MEMBER,
 REASS_FST_DONE) = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
(REASS_DG_COMPLETE, REASS_DG_WRITTEN, REASS_DG_INCOMPLETE, REASS_DG_OVERLAP, REASS_DG_TOOMANY,
 REASS_DG_TOOBIG, REASS_DG_NOROOM) = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40
REASS_NONE, REASS_MAX_FRAGS = 0xFFFFFFFF, 64
REASS_DGRAM_DTYPE = np.dtype([("first", "<u4"), ("slot", "<u4"), ("frags", "<u4"),
                              ("out_len", "<u2"), ("status", "u1"), ("reserved", "u1")])
assert REASS_DGRAM_DTYPE.itemsize == 16
REASS_HDR_DTYPE = np.dtype([("candidates", "<u8"), ("considered", "<u8"), ("dgrams", "<u8"),
                            ("reported", "<u8"), ("complete", "<u8"), ("written", "<u8")])
assert REASS_HDR_DTYPE.itemsize == 48
# struct pptk_tunnel and the status bits of pptk_tunnel_encap_* / _decap_*
TUNNEL_DTYPE = np.dtype([("eth_dst", "u1", 6), ("eth_src", "u1", 6), ("src", "<u4"),
                         ("dst", "<u4"), ("id", "<u2"), ("ttl", "u1"), ("tos", "u1"),
                         ("flags", "<u4"), ("reserved", "<u4")])
assert TUNNEL_DTYPE.itemsize == 32
TUN_DF, TUN_ID_SEQ, TUN_HDR_LEN = 0x1, 0x2, 38
(TUN_ST_DONE, TUN_ST_RUNT, TUN_ST_TOOBIG, TUN_ST_NOROOM, TUN_ST_NOFLOW,
 TUN_ST_BADTUN) = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
(DECAP_ST_IPV4, DECAP_ST_GRE, DECAP_ST_OK, DECAP_ST_ISFRAG, DECAP_ST_BADCKSUM, DECAP_ST_SHORT,
 DECAP_ST_GREOPT, DECAP_ST_PTYPE) = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80
# struct pptk_flow_key (the flow table's key: the tuple the flow hash covers),
# the "no flow" index and the status bits of pptk_flow_lookup_device / _host
FLOW_KEY_DTYPE = np.dtype([("src", "u1", 16), ("dst", "u1", 16), ("sport", "<u2"),
                           ("dport", "<u2"), ("proto", "u1"), ("zero", "u1", 3)])
assert FLOW_KEY_DTYPE.itemsize == 40
FLOW_NONE = 0xFFFFFFFF
FLOW_ST_SUBJECT, FLOW_ST_HIT = 0x1, 0x2
# struct pptk_flow_stats (include/pptk_rx.h "Flow state"): entry v belongs to flow value v
FLOW_STATS_DTYPE = np.dtype([("packets", "<u8"), ("bytes", "<u8"), ("last_seen", "<u8"),
                             ("reserved", "<u8")])
assert FLOW_STATS_DTYPE.itemsize == 32
# struct pptk_flow_learn_hdr (include/pptk_rx.h "Flow learning")
FLOW_LEARN_HDR_DTYPE = np.dtype([("candidates", "<u8"), ("considered", "<u8"), ("flows", "<u8"),
                                 ("written", "<u8")])
assert FLOW_LEARN_HDR_DTYPE.itemsize == 32
# struct pptk_dispatch_port / pptk_dispatch_hdr and the port codes
# (include/pptk_rx.h "Egress dispatch")
DISPATCH_PORT_DTYPE = np.dtype([("start", "<u8"), ("count", "<u8"), ("bytes", "<u8"),
                                ("flooded", "<u8")])
DISPATCH_HDR_DTYPE = np.dtype([("total", "<u8"), ("written", "<u8"), ("unicast", "<u8"),
                               ("flood", "<u8"), ("dropped", "<u8"), ("bad", "<u8"),
                               ("hairpin", "<u8"), ("reserved", "<u8")])
assert DISPATCH_PORT_DTYPE.itemsize == 32 and DISPATCH_HDR_DTYPE.itemsize == 64
PORT_MAX, PORT_FLOOD, PORT_DROP = 64, 0xFF, 0xFE
# struct pptk_gather_port / pptk_gather_hdr (include/pptk_rx.h "Egress gather")
GATHER_PORT_DTYPE = np.dtype([("start", "<u8"), ("bytes", "<u8"), ("entries", "<u8"),
                              ("packed", "<u8")])
GATHER_HDR_DTYPE = np.dtype([("entries", "<u8"), ("packed", "<u8"), ("need", "<u8"),
                             ("bytes", "<u8"), ("frame_bytes", "<u8"), ("bad", "<u8"),
                             ("status", "<u8"), ("reserved", "<u8")])
assert GATHER_PORT_DTYPE.itemsize == 32 and GATHER_HDR_DTYPE.itemsize == 64
GATHER_SLOT_ALIGN, GATHER_REGION_ALIGN, GATHER_ST_BADRUNS = 16, 256, 1

REC32_DTYPE = np.dtype([
    ("flow_hash", "<u8"),
    ("src4", "u1", 4),
    ("dst4", "u1", 4),
    ("sport", "<u2"),
    ("dport", "<u2"),
    ("flags", "<u2"),
    ("proto", "u1"),
    ("l3_off", "u1"),
    ("l4_off", "<u2"),
    ("l4_len", "<u2"),
    ("src_bucket", "<u4"),
])
assert REC32_DTYPE.itemsize == 32

# struct pptk_rx_frag: the fragment side record (pptk_rx_dev_batch.d_frag)
FRAG_DTYPE = np.dtype([
    ("ident", "<u4"),
    ("frag_off", "<u2"),
    ("data_len", "<u2"),
    ("frag_hdr_off", "<u2"),
    ("proto_hdr_off_from_frag", "<u2"),
    ("next_hdr", "u1"),
    ("flags", "u1"),
    ("reserved", "<u2"),
])
assert FRAG_DTYPE.itemsize == 16
FRAG_IS, FRAG_MF, FRAG_DF, FRAG_V6 = 0x01, 0x02, 0x04, 0x08

F_PARSED = 0x0001
F_IP_OK = 0x0002
F_L4_OK = 0x0004
F_L4 = 0x0008
F_IPV6 = 0x0010
F_VLAN = 0x0020
F_FRAGMENT = 0x0040
F_UDP_ZERO = 0x0080
F_MALFORMED = 0x0100
F_V6_EXT = 0x0200


def as_records(raw):
    """View a uint8 buffer (n*64 bytes) as records."""
    raw = np.ascontiguousarray(raw)
    return raw.view(np.uint8).reshape(-1).view(REC_DTYPE)


def to_rec32(recs):
    """The compact record the kernel writes for each full record: the same
    values, IPv6 addresses left out (src4/dst4 = 0)."""
    r = as_records(recs)
    out = np.zeros(len(r), dtype=REC32_DTYPE)
    v4 = (r["flags"] & F_IPV6) == 0
    for f in ("flow_hash", "sport", "dport", "flags", "proto", "l3_off", "l4_off", "l4_len",
              "src_bucket"):
        out[f] = r[f]
    out["src4"] = np.where(v4[:, None], r["src"][:, :4], 0)
    out["dst4"] = np.where(v4[:, None], r["dst"][:, :4], 0)
    return out


def diff_records(got, want, limit=5, dtype=REC_DTYPE):
    """Return a human-readable description of the first mismatching records
    (empty string when identical byte for byte)."""
    rb = dtype.itemsize
    g = np.ascontiguousarray(got).view(np.uint8).reshape(-1, rb)
    w = np.ascontiguousarray(want).view(np.uint8).reshape(-1, rb)
    if g.shape != w.shape:
        return f"shape mismatch {g.shape} vs {w.shape}"
    bad = np.nonzero((g != w).any(axis=1))[0]
    if bad.size == 0:
        return ""
    lines = [f"{bad.size} of {g.shape[0]} records differ"]
    gr, wr = g.view(dtype).reshape(-1), w.view(dtype).reshape(-1)
    for i in bad[:limit]:
        fields = [n for n in dtype.names
                  if not np.array_equal(gr[i][n], wr[i][n])]
        lines.append(f"  rec {i}: fields {fields}: got "
                     + ", ".join(f"{n}={gr[i][n]}" for n in fields)
                     + " want " + ", ".join(f"{n}={wr[i][n]}" for n in fields))
    return "\n".join(lines)
