"""Deterministic geometry sweeps for the two in-place header kernels
(pptk_tx_rewrite_device, pptk_tcp_mss_clamp_device).

Both kernels keep a per-lane image of the frame's first aligned 16-byte
chunks: frame bytes [0, SLOT - m) with m = (frame offset from d_frames) & 15,
RW_SLOT = 64, MSS_SLOT = 128.  A written field lies wholly in the image,
straddles its last byte, or lies past it; image chunks are written back
whole only where they lie inside the frame.  The batches here put a small
set of base frames (built once with framegen's builders) at every m, with
0..15 filler bytes between neighbours and guards on both sides, and in
fixed-stride layouts whose stride walks m through all 16 values; coverage()
says which of those cases a batch reaches.  numpy and framegen only: no GPU,
no oracle.

A Batch is compared whole: `buf` (guards, gaps and all) against the
oracle's output for the same layout, the frames pointer being
buf[origin:].
"""
import functools
import struct

import numpy as np

import framegen

RW_SLOT, MSS_SLOT = 64, 128
FILL = 0xA5
GUARD = 4096          # bytes of FILL on both sides of the frames (a multiple of 16)
ST_GUARD = 8          # status entries past n that must keep their fill
VLAN_TAG = 0x123

# rewrite ops and the fields they write (records.RW_*)
OP_TTL, OP_SRC, OP_DST, OP_SPORT, OP_DPORT, OP_ICMP = 1, 2, 4, 8, 16, 32

(K_TCP, K_UDP, K_UDP0, K_ICMP8, K_ICMP0, K_ICMPX, K_ICMPCUT, K_P47, K_FRAG, K_TTL0,
 K_TTL1) = range(11)
_L4OK = (K_TCP, K_UDP, K_UDP0, K_TTL0, K_TTL1)
_TCPLIKE = (K_TCP, K_TTL0, K_TTL1)

RW_FIELDS = ("ttl", "ipck", "src", "dst", "sport", "dport", "tcpck", "udpck", "icmpck", "icmpid")
IP_FIELDS = ("ttl", "ipck", "src", "dst")


class Batch:
    """One batch: buf (whole buffer), origin (frames pointer = buf[origin:]),
    either off/lens (offsets from the frames pointer) or stride/fixed_len,
    n, rewrite entries rw (n) and rw_one (1) where it is a rewrite batch, and
    per-frame metadata arrays in meta (m, l3, l4, kind, vlan, ...)."""

    def __init__(self, buf, origin, n, off=None, lens=None, stride=0, fixed_len=0, rw=None,
                 rw_one=None, meta=None, tags=None):
        self.buf, self.origin, self.n = buf, origin, n
        self.off, self.lens, self.stride, self.fixed_len = off, lens, stride, fixed_len
        self.rw, self.rw_one, self.meta, self.tags = rw, rw_one, meta or {}, tags

    def layout(self):
        if self.off is not None:
            return dict(off=self.off, lens=self.lens)
        return dict(stride=self.stride, fixed_len=self.fixed_len, n=self.n)

    def starts(self):
        """Frame offsets from the frames pointer."""
        if self.off is not None:
            return self.off.astype(np.int64)
        return np.arange(self.n, dtype=np.int64) * self.stride

    def frame_lens(self):
        if self.lens is not None:
            return self.lens.astype(np.int64)
        return np.full(self.n, self.fixed_len, np.int64)


# --------------------------------------------------------------- placement
def _scatter(buf, frames, fidx, pos):
    order = np.argsort(fidx, kind="stable")
    cuts = np.searchsorted(fidx[order], np.arange(len(frames) + 1))
    for j, fr in enumerate(frames):
        idx = order[cuts[j]:cuts[j + 1]]
        if len(idx):
            buf[pos[idx][:, None] + np.arange(len(fr))] = fr


def place(frames, fidx, m):
    """Frame k is a copy of frames[fidx[k]] starting at an offset = m[k] mod
    16, as close behind its predecessor as that allows: gaps of 0..15 FILL
    bytes.  Returns (buf, off, lens); offsets are from buf[0] and include
    the leading guard."""
    fidx, m = np.asarray(fidx, np.int64), np.asarray(m, np.int64)
    lens = np.array([len(f) for f in frames], np.int64)[fidx]
    step = np.empty(len(fidx), np.int64)
    step[0] = m[0]
    step[1:] = lens[:-1] + ((m[1:] - m[:-1] - lens[:-1]) & 15)
    off = GUARD + np.cumsum(step)
    end = int(off[-1] + lens[-1])
    buf = np.full((end + 15) // 16 * 16 + GUARD, FILL, np.uint8)
    _scatter(buf, frames, fidx, off)
    assert ((off & 15) == m).all()
    return buf, off.astype(np.uint64), lens.astype(np.uint16)


def place_fixed(frames, fidx, stride):
    """Fixed-stride layout of equally long frames behind a guard; the frames
    pointer is buf[GUARD:]."""
    fidx = np.asarray(fidx, np.int64)
    L = len(frames[0])
    assert all(len(f) == L for f in frames) and stride >= L
    n = len(fidx)
    buf = np.full(GUARD + (n * stride + 15) // 16 * 16 + GUARD, FILL, np.uint8)
    _scatter(buf, frames, fidx, GUARD + np.arange(n, dtype=np.int64) * stride)
    return buf


def _pad(fr, L):
    out = np.zeros(L, np.uint8)      # Ethernet padding behind the IP packet
    out[:len(fr)] = fr
    return out


def fixed_strides(L):
    return (L, L + 1, L + 3, (L + 15) // 16 * 16 + 16)


def rewrites(n, seed, ops=None):
    """n rewrite entries (records.REWRITE_DTYPE's layout) from a fixed seed."""
    rng = np.random.default_rng(seed)
    rw = np.zeros(n, np.dtype([("ops", "<u4"), ("src", "<u4"), ("dst", "<u4"),
                               ("sport", "<u2"), ("dport", "<u2")]))
    rw["src"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    rw["dst"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    rw["sport"] = rng.integers(0, 65536, n)
    rw["dport"] = rng.integers(0, 65536, n)
    rw["ops"] = rng.integers(0, 64, n) if ops is None else ops
    return rw


# ------------------------------------------------------ rewrite base frames
def _set_ttl(f, l3, ihl, ttl):
    f = bytearray(f)
    f[l3 + 8] = ttl
    f[l3 + 10:l3 + 12] = b"\0\0"
    struct.pack_into(">H", f, l3 + 10, framegen.csum(bytes(f[l3:l3 + 4 * ihl])))
    return bytes(f)


def _rw_frame(rng, kind, vlan, ihl, extra):
    """One base frame whose L4 is at its minimum plus `extra` bytes."""
    l3 = 18 if vlan is not None else 14
    hdr = l3 + 4 * ihl
    if kind in _TCPLIKE:
        f = framegen.frame_v4(rng, 6, hdr + 20 + extra, vlan, ihl)
        if kind != K_TCP:
            f = _set_ttl(f, l3, ihl, 0 if kind == K_TTL0 else 1)
    elif kind in (K_UDP, K_UDP0):
        f = framegen.frame_v4(rng, 17, hdr + 8 + extra, vlan, ihl, udp_zero=kind == K_UDP0)
    elif kind == K_FRAG:          # a non-first fragment: no L4 header to rewrite
        f = framegen.frame_v4(rng, 17, hdr + 8 + extra, vlan, ihl, frag_off=3)
    elif kind == K_ICMPCUT:       # echo header cut by ip_total_len: 7 bytes inside
        f = framegen.frame_icmp4(rng, 8, 0, vlan, ihl, l4_len=7) + bytes(extra)
    elif kind == K_P47:           # GRE: IP-level ops only; no payload at all when short
        opts = bytes(rng.integers(0, 256, (ihl - 5) * 4, dtype=np.uint8))
        ip = framegen.ipv4_hdr(bytes(rng.integers(0, 256, 4, dtype=np.uint8)),
                               bytes(rng.integers(0, 256, 4, dtype=np.uint8)), 47, extra, opts)
        f = framegen.eth(framegen.ETH_IP, vlan) + ip + bytes(rng.integers(0, 256, extra,
                                                                         dtype=np.uint8))
    else:
        f = framegen.frame_icmp4(rng, {K_ICMP8: 8, K_ICMP0: 0, K_ICMPX: 3}[kind], extra, vlan, ihl)
    return f


@functools.lru_cache(None)
def rewrite_bases():
    """Every kind at every IHL with and without a VLAN tag, all with L4 at
    its minimum (the frame ends in the chunk of its last rewritten field),
    plus TCP / UDP / echo with 37 bytes behind L4: 260 frames.  Returns
    (frames, table) with table fields kind, vlan, ihl, l3, l4, len."""
    rng = np.random.default_rng(0x5EE9)
    spec = []
    for vlan in (None, VLAN_TAG):
        for ihl in range(5, 16):
            for kind in range(11):
                spec.append((kind, vlan, ihl, 0))
        for ihl in (5, 10, 15):
            for kind in (K_TCP, K_UDP, K_ICMP8):
                spec.append((kind, vlan, ihl, 37))
    frames = [np.frombuffer(_rw_frame(rng, *s), np.uint8) for s in spec]
    tab = np.zeros(len(spec), np.dtype([("kind", "i4"), ("vlan", "i4"), ("ihl", "i4"),
                                        ("l3", "i4"), ("l4", "i4"), ("len", "i4")]))
    for i, (kind, vlan, ihl, _) in enumerate(spec):
        l3 = 18 if vlan is not None else 14
        tab[i] = (kind, vlan is not None, ihl, l3, l3 + 4 * ihl, len(frames[i]))
    return frames, tab


def _rw_meta(tab, fidx, m, ops):
    t = tab[fidx]
    return dict(m=np.asarray(m, np.int64), ops=np.asarray(ops, np.int64), kind=t["kind"],
                vlan=t["vlan"], l3=t["l3"].astype(np.int64), l4=t["l4"].astype(np.int64),
                fidx=np.asarray(fidx, np.int64))


@functools.lru_cache(None)
def rewrite_placed():
    """Every base frame at every m in 0..15 with every ops mask 0..63, one
    rewrite entry per frame, in a fixed shuffled order."""
    frames, tab = rewrite_bases()
    nb = len(frames)
    fidx, m, ops = (a.reshape(-1) for a in np.meshgrid(np.arange(nb), np.arange(16),
                                                       np.arange(64), indexing="ij"))
    perm = np.random.default_rng(0x91ACE).permutation(len(fidx))
    fidx, m, ops = fidx[perm], m[perm], ops[perm]
    buf, off, lens = place(frames, fidx, m)
    return Batch(buf, 0, len(fidx), off=off, lens=lens, rw=rewrites(len(fidx), 0xA11, ops),
                 meta=_rw_meta(tab, fidx, m, ops))


@functools.lru_cache(None)
def rewrite_fixed():
    """Fixed-stride rewrite batches, (name, Batch) each: frames of one length
    L (shorter bases carry Ethernet padding) at strides L, L + 1, L + 3 and
    round_up(L, 16) + 16, for L = 42 (the UDP / echo frames end with their
    last field's chunk) and L = 98 (every short base), and 2048 frames of
    1500 bytes at stride 1501."""
    frames, tab = rewrite_bases()
    rng = np.random.default_rng(0xF1C5)
    out = []
    for L in (42, 98):
        sel = np.nonzero(tab["len"] <= L)[0]
        padded = [_pad(frames[j], L) for j in sel]
        for stride in fixed_strides(L):
            n = 4096
            pick = rng.integers(0, len(sel), n)
            ops = rng.integers(0, 64, n)
            buf = place_fixed(padded, pick, stride)
            m = (np.arange(n) * stride) & 15
            out.append((f"L{L}_s{stride}", Batch(
                buf, GUARD, n, stride=stride, fixed_len=L, rw=rewrites(n, 0xA12 + stride, ops),
                rw_one=rewrites(1, 0xA13, 0x3F), meta=_rw_meta(tab, sel[pick], m, ops))))
    big, btab = [], []
    for kind in (K_TCP, K_UDP, K_ICMP8):
        for vlan, ihl in ((None, 5), (VLAN_TAG, 15), (None, 12)):
            l3 = 18 if vlan is not None else 14
            f = _rw_frame(rng, kind, vlan, ihl, 1500 - l3 - 4 * ihl - (20 if kind == K_TCP else 8))
            assert len(f) == 1500
            big.append(np.frombuffer(f, np.uint8))
            btab.append((kind, vlan is not None, ihl, l3, l3 + 4 * ihl, 1500))
    btab = np.array(btab, tab.dtype)
    n = 2048
    pick, ops = rng.integers(0, len(big), n), rng.integers(0, 64, n)
    out.append(("L1500_s1501", Batch(
        place_fixed(big, pick, 1501), GUARD, n, stride=1501, fixed_len=1500,
        rw=rewrites(n, 0xA14, ops), rw_one=rewrites(1, 0xA15, 0x3F),
        meta=_rw_meta(btab, pick, (np.arange(n) * 1501) & 15, ops))))
    return out


# -------------------------------------------------------- checksum corners
def upd16(c, o, n):
    """ip_update_cksum16 (RFC 1624 eqn. 3) restated; c may be an array."""
    s = (~np.asarray(c, np.int64) & 0xFFFF) + (~int(o) & 0xFFFF) + int(n)
    s = (s & 0xFFFF) + (s >> 16)
    s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


CORNER_VALUES = (0x0000, 0x0001, 0x7FFF, 0x8000, 0xFFFE, 0xFFFF)
# the documented op order as 16-bit checksum updates
UPDATES = ("ttl", "src_hi", "src_lo", "dst_hi", "dst_lo", "sport", "dport", "icmp_id")
_UPTO = (OP_TTL, OP_TTL | OP_SRC, OP_TTL | OP_SRC, 7, 7, 0xF, 0x1F, 0x3F)
TAG_DTYPE = np.dtype([("field", "u1"), ("k", "i1"), ("target", "<u2"), ("predict", "u1"),
                      ("udp", "u1")])
F_IP, F_L4, F_SET = 0, 1, 2


def _pairs(f, l3, l4, kind, w, ops):
    """(update index, old word, new word) of each 16-bit checksum update the
    rewrite `w` with `ops` makes, for the IP and for the L4 checksum."""
    be16 = lambda k: (int(f[k]) << 8) | int(f[k + 1])
    ip, l4u = [], []
    if ops & OP_TTL:
        ip.append((0, be16(l3 + 8), be16(l3 + 8) - 0x100))
    for bit, at, new, k in ((OP_SRC, 12, int(w["src"]), 1), (OP_DST, 16, int(w["dst"]), 3)):
        if ops & bit:
            for h in (0, 1):
                p = (k + h, be16(l3 + at + 2 * h), (new >> (16 * (1 - h))) & 0xFFFF)
                ip.append(p)
                if kind != K_ICMP8:
                    l4u.append(p)
    if kind != K_ICMP8:
        for bit, at, new, k in ((OP_SPORT, 0, int(w["sport"]), 5), (OP_DPORT, 2, int(w["dport"]), 6)):
            if ops & bit:
                l4u.append((k, be16(l4 + at), new))
    elif ops & OP_ICMP:
        l4u.append((7, be16(l4 + 4), int(w["sport"])))
    return ip, l4u


def run_updates(c0, pairs, udp):
    """Running checksum after each update from start value(s) c0, and
    whether the update was skipped: two lists of arrays.  udp: an address
    or port update (both halves of an address together) is skipped while
    the running value is 0."""
    run, runs, skips = np.asarray(c0, np.int64), [], []
    skip = np.zeros(run.shape, bool)
    for k, o, n in pairs:
        if udp:
            skip = skip if k in (2, 4) else run == 0
            run = np.where(skip, run, upd16(run, o, n))
        else:
            run = upd16(run, o, n)
        runs.append(run)
        skips.append(skip)
    return runs, skips


def find_start(pairs, k, target, udp):
    """Checksum start values for which the running value is `target` right
    after update k, no update up to k having been skipped."""
    ks = [p[0] for p in pairs]
    if k not in ks:
        return []
    j = ks.index(k)
    runs, skips = run_updates(np.arange(65536, dtype=np.int64), pairs[:j + 1], udp)
    ok = runs[j] == target
    for sk in skips:
        ok &= ~sk
    return [int(x) for x in np.nonzero(ok)[0]]


@functools.lru_cache(None)
def corners():
    """Checksum-corner batch over TCP, UDP and ICMP-echo base frames (IHL 5
    and 7, with and without a VLAN tag), every variant at all 16 m:
      * IP and L4 checksum fields set to each pair of CORNER_VALUES, all ops;
      * for every update k and target 0x0000 / 0xffff, start values (found
        with find_start) that make the running checksum the target right
        after update k, once with the ops stopping at k's op and once with
        all ops.  0xffff results from RFC 1624's eqn. 3 only as ~(0 + 0 + 0):
        old checksum 0xffff, old word 0xffff, new word 0; those variants
        carry all-ones addresses / ports / identifier and a rewrite to 0
        without the TTL op, and a TTL update can never give 0xffff.
    tags (TAG_DTYPE) per frame: field F_IP / F_L4 (F_SET for the plain
    value pairs), update k, target, predict (the final field must equal the
    target: k is the last update of its checksum, or a UDP checksum that
    became 0 at the end of an op and so stays 0), udp.
    Returns (Batch, unreachable) with unreachable = {(field, k, target)}
    for which no start value exists."""
    frames, tab = rewrite_bases()
    sel = [j for j in range(len(frames)) if tab["kind"][j] in (K_TCP, K_UDP, K_ICMP8)
           and tab["ihl"][j] in (5, 7) and tab["len"][j] - tab["l4"][j] <= 20]
    w_all, w_zero = rewrites(1, 0xC0A, 0x3F)[0], rewrites(1, 0xC0A, 0x3F)[0]
    for name in ("src", "dst", "sport", "dport"):
        w_zero[name] = 0
    var, vtab, vrw, tags, unreachable = [], [], [], [], set()

    def emit(f, j, w, ops, tag):
        var.append(f.copy())
        vtab.append(tab[j])
        e = w.copy()
        e["ops"] = ops
        vrw.append(e)
        tags.append(tag)

    for j in sel:
        kind, l3, l4 = int(tab["kind"][j]), int(tab["l3"][j]), int(tab["l4"][j])
        udp = kind == K_UDP
        cko = {K_TCP: 16, K_UDP: 6, K_ICMP8: 2}[kind]
        base = frames[j].copy()
        ones = base.copy()
        ones[l3 + 12:l3 + 20] = 0xFF
        ones[l4 + 4 if kind == K_ICMP8 else l4:(l4 + 6 if kind == K_ICMP8 else l4 + 4)] = 0xFF

        def with_ck(f, ipck, l4ck):
            g = f.copy()
            if ipck is not None:
                g[l3 + 10], g[l3 + 11] = ipck >> 8, ipck & 0xFF
            if l4ck is not None:
                g[l4 + cko], g[l4 + cko + 1] = l4ck >> 8, l4ck & 0xFF
            return g

        for a in CORNER_VALUES:
            for b in CORNER_VALUES:
                emit(with_ck(base, a, b), j, w_all, 0x3F, (F_SET, -1, 0, 0, udp))
        if not find_start(_pairs(base, l3, l4, kind, w_all, OP_TTL)[0], 0, 0xFFFF, False):
            unreachable.add((F_IP, 0, 0xFFFF))
        for k in range(8):
            for target in (0x0000, 0xFFFF):
                src, w = (base, w_all) if target == 0 else (ones, w_zero)
                drop = 0 if target == 0 else OP_TTL
                for ops in sorted({_UPTO[k] & ~drop, 0x3F & ~drop}):
                    ip, l4u = _pairs(src, l3, l4, kind, w, ops)
                    for field, pairs, isudp in ((F_IP, ip, False), (F_L4, l4u, udp)):
                        if k not in [p[0] for p in pairs]:
                            continue
                        starts = find_start(pairs, k, target, isudp)
                        if not starts:
                            unreachable.add((field, k, target))
                            continue
                        last = pairs[-1][0] == k
                        for c in starts:
                            stuck = isudp and target == 0 and k not in (1, 3)
                            g = with_ck(src, c if field == F_IP else None,
                                        c if field == F_L4 else None)
                            emit(g, j, w, ops, (field, k, target, last or stuck, isudp))
    nv = len(var)
    fidx, m = (a.reshape(-1) for a in np.meshgrid(np.arange(nv), np.arange(16), indexing="ij"))
    perm = np.random.default_rng(0xC02).permutation(len(fidx))
    fidx, m = fidx[perm], m[perm]
    buf, off, lens = place(var, fidx, m)
    rw = np.array(vrw)[fidx]
    meta = _rw_meta(np.array(vtab), fidx, m, rw["ops"])
    meta["cko"] = np.array([{K_TCP: 16, K_UDP: 6, K_ICMP8: 2}[int(k)] for k in meta["kind"]],
                           np.int64)
    return (Batch(buf, 0, len(fidx), off=off, lens=lens, rw=rw, meta=meta,
                  tags=np.array(tags, TAG_DTYPE)[fidx]), unreachable)


# ------------------------------------------------------------ MSS batches
MSS_PRESENT = 1460
MSS_CLAMPS = (0, 536, MSS_PRESENT - 1, MSS_PRESENT, 65535)


def _mss_lists():
    """(name, option bytes, payload bytes, data-offset override)."""
    M = struct.pack(">BBH", 2, 4, MSS_PRESENT)
    big = struct.pack(">BBH", 2, 4, 9000)
    nop = b"\x01"

    def upto(o, doff):
        return o + nop * (4 * (doff - 5) - len(o))

    L = [("none", b"", b"", None),
         ("first", M, b"", None),                       # even offset, value ends at the frame end
         ("first_pl", M, bytes(range(9)), None),
         ("nop1", upto(nop + M, 7), b"", None),
         ("nop1_d10", upto(nop + M, 10), b"", None),
         ("nop1_d13", upto(nop + M, 13), bytes(5), None),
         ("nop2", upto(nop * 2 + M, 7), b"", None),
         # odd offset, value ends one byte before the frame end.  (It cannot
         # end AT the end: the options' length is a multiple of 4, so a
         # 4-byte option at an odd offset leaves at least one byte.)
         ("nop3", nop * 3 + M + b"\x00", b"", None),
         ("nop3_pl", nop * 3 + M + nop, bytes(range(7)), None),
         ("two", big + M, b"", None),                   # the last one counts
         ("two_odd", upto(nop + big + nop * 2 + M, 9), b"", None),
         ("k2l3", b"\x02\x03\x05\x01", b"", None),      # kind 2 but not an MSS
         ("k2l5", b"\x02\x05\x05\xb4\x00\x01\x01\x01", b"", None),
         ("lenlast", M + nop * 2 + b"\x08\x0a", b"", None),   # length byte = last option byte
         ("kindlast", M + nop * 3 + b"\x08", b"\x0a\x00", None),  # length byte past the options
         ("len0", M + b"\x03\x00\x01\x01", b"", None),
         ("len1", M + b"\x03\x01\x01\x01", b"", None),
         ("k2len0", b"\x02\x00\x05\xb4", b"", None),
         ("toolong", b"\x08\x0a\x01\x01", b"", None),  # longer than the bytes left: clipped
         ("toolong_mss", nop * 4 + b"\x02\x0a\x05\xb4", b"", None),   # clipped to 4: an MSS
         ("eol", b"\x00\x00\x00\x00" + M, b"", None),
         ("past", M, b"", 15),                          # options run past the segment
         ("past1", M + nop * 4, b"", 8)]
    for doff in (8, 11, 12, 14, 15):                            # MSS as the last four option bytes
        L.append((f"last_d{doff}", nop * (4 * (doff - 6)) + M, b"", None))
    return L


def _mss_frame(rng, v6ext, ihl, vlan, opts, payload, syn, doff):
    seg = bytearray(framegen.tcp_hdr(*(int(x) for x in rng.integers(0, 65536, 2)),
                                     int(rng.integers(0, 2 ** 32)), 0,
                                     flags=0x02 if syn else 0x10, opts=opts) + payload)
    if doff is not None:
        seg[12] = (doff << 4) | (seg[12] & 0x0F)
    if v6ext is None:
        src, dst = (bytes(rng.integers(0, 256, 4, dtype=np.uint8)) for _ in range(2))
        seg = framegen.fill_l4(seg, 6, framegen.pseudo4(src, dst, 6, len(seg)))
        ipo = bytes(rng.integers(0, 256, (ihl - 5) * 4, dtype=np.uint8))
        ip = framegen.ipv4_hdr(src, dst, 6, len(seg), ipo)
        return framegen.eth(framegen.ETH_IP, vlan) + ip + seg
    src, dst = (bytes(rng.integers(0, 256, 16, dtype=np.uint8)) for _ in range(2))
    seg = framegen.fill_l4(seg, 6, framegen.pseudo6(src, dst, 6, len(seg)))
    types = [0] + [60] * (v6ext - 1) if v6ext else []
    exth = b"".join(bytes([(types + [6])[i + 1]]) + framegen.hbh(1)[1:] for i in range(v6ext))
    ip = framegen.ipv6_hdr(src, dst, (types + [6])[0], len(exth) + len(seg))
    return framegen.eth(framegen.ETH_IP6, vlan) + ip + exth + seg


@functools.lru_cache(None)
def mss_bases():
    """IPv4 IHL 5..15 and IPv6 with 0..6 eight-byte extension headers, each
    with and without a VLAN tag, crossed with the option lists; one frame in
    four is not a SYN.  Returns (frames, table) with t (TCP header offset),
    end (data offset in bytes, as transmitted), inseg (options inside the
    segment), len."""
    rng = np.random.default_rng(0x3557)
    geoms = [(None, ihl) for ihl in range(5, 16)] + [(e, 0) for e in range(7)]
    frames, rows = [], []
    for gi, (v6ext, ihl) in enumerate(geoms):
        for vlan in (None, VLAN_TAG):
            for li, (_, opts, payload, doff) in enumerate(_mss_lists()):
                syn = (gi + li + (vlan is not None)) % 4 != 0
                f = _mss_frame(rng, v6ext, ihl, vlan, opts, payload, syn, doff)
                l3 = 18 if vlan is not None else 14
                t = l3 + (4 * ihl if v6ext is None else 40 + 8 * v6ext)
                end = (f[t + 12] >> 4) * 4
                frames.append(np.frombuffer(f, np.uint8))
                rows.append((t, end, t + end <= len(f), len(f), li, syn))
    return frames, np.array(rows, np.dtype([("t", "i4"), ("end", "i4"), ("inseg", "i4"),
                                            ("len", "i4"), ("list", "i4"), ("syn", "i4")]))


def _mss_meta(tab, fidx, m):
    t = tab[fidx]
    return dict(m=np.asarray(m, np.int64), t=t["t"].astype(np.int64),
                end=t["end"].astype(np.int64), inseg=t["inseg"], list=t["list"], syn=t["syn"],
                fidx=np.asarray(fidx, np.int64))


@functools.lru_cache(None)
def mss_placed():
    frames, tab = mss_bases()
    fidx, m = (a.reshape(-1) for a in np.meshgrid(np.arange(len(frames)), np.arange(16),
                                                  indexing="ij"))
    perm = np.random.default_rng(0x355A).permutation(len(fidx))
    fidx, m = fidx[perm], m[perm]
    buf, off, lens = place(frames, fidx, m)
    return Batch(buf, 0, len(fidx), off=off, lens=lens, meta=_mss_meta(tab, fidx, m))


@functools.lru_cache(None)
def mss_fixed():
    """Every MSS base frame, padded to the longest one's length L, at strides
    L, L + 1, L + 3 and round_up(L, 16) + 16; (name, Batch) each."""
    frames, tab = mss_bases()
    L = int(tab["len"].max())
    padded = [_pad(f, L) for f in frames]
    rng = np.random.default_rng(0x355B)
    out = []
    for stride in fixed_strides(L):
        n = 4096
        pick = rng.integers(0, len(frames), n)
        out.append((f"L{L}_s{stride}", Batch(
            place_fixed(padded, pick, stride), GUARD, n, stride=stride, fixed_len=L,
            meta=_mss_meta(tab, pick, (np.arange(n) * stride) & 15))))
    return out


def tile(b, n):
    """The placed batch b repeated until it holds n frames (the body is a
    multiple of 16 bytes long, so every copy keeps its m); the frames of the
    last copy past n stay in the buffer, outside the batch."""
    body = b.buf[GUARD:b.buf.size - GUARD]
    assert body.size % 16 == 0 and b.origin == 0
    reps = -(-n // b.n)
    buf = np.concatenate([b.buf[:GUARD]] + [body] * reps + [b.buf[-GUARD:]])
    off = np.concatenate([b.off + np.uint64(r * body.size) for r in range(reps)])[:n]
    lens = np.concatenate([b.lens] * reps)[:n]
    rw = None if b.rw is None else np.concatenate([b.rw] * reps)[:n]
    return Batch(buf, 0, n, off=off, lens=lens, rw=rw)


# ---------------------------------------------------------------- coverage
def _written(meta):
    """Per rewritten field: (frame offset, bytes, mask of frames whose
    rewrite writes it)."""
    kind, ops, l3, l4 = meta["kind"], meta["ops"], meta["l3"], meta["l4"]
    live = ~((kind == K_TTL0) & ((ops & OP_TTL) != 0))     # TTL 0: left untouched
    l4ok, tcp = np.isin(kind, _L4OK), np.isin(kind, _TCPLIKE)
    echo = np.isin(kind, (K_ICMP8, K_ICMP0)) & ((ops & OP_ICMP) != 0)
    return {
        "ttl": (l3 + 8, 1, live & ((ops & OP_TTL) != 0)),
        "ipck": (l3 + 10, 2, live & ((ops & 7) != 0)),
        "src": (l3 + 12, 4, live & ((ops & OP_SRC) != 0)),
        "dst": (l3 + 16, 4, live & ((ops & OP_DST) != 0)),
        "sport": (l4, 2, live & l4ok & ((ops & OP_SPORT) != 0)),
        "dport": (l4 + 2, 2, live & l4ok & ((ops & OP_DPORT) != 0)),
        "tcpck": (l4 + 16, 2, live & tcp & ((ops & 0x1E) != 0)),
        "udpck": (l4 + 6, 2, live & (kind == K_UDP) & ((ops & 0x1E) != 0)),
        "icmpck": (l4 + 2, 2, live & echo),
        "icmpid": (l4 + 4, 2, live & echo),
    }


def coverage(b):
    """What a batch reaches.  For a rewrite batch (meta has ops), per field
    of RW_FIELDS the sets of m at which a frame's written field lies "in"
    the image, "straddle"s its last byte or lies "past" it, the m of
    straddles with ("straddle_vlan") and without ("straddle_plain") a VLAN
    tag, and "chunk_out": the m at which an image chunk holding a written
    byte of the field reaches outside its frame.  For an MSS batch (meta has
    t), "mss_dist": the values of m + t + end - MSS_SLOT within -4..+4 over
    frames whose options lie inside the segment.  Always "m": the m seen."""
    meta = b.meta
    m = meta["m"]
    out = {"m": set(np.unique(m).tolist())}
    if "ops" in meta:
        flen = b.frame_lens()
        for name, (k, nb, on) in _written(meta).items():
            lo, hi = m + k, m + k + nb
            cls = {"in": on & (hi <= RW_SLOT), "past": on & (lo >= RW_SLOT),
                   "straddle": on & (lo < RW_SLOT) & (hi > RW_SLOT)}
            cls["straddle_vlan"] = cls["straddle"] & (meta["vlan"] != 0)
            cls["straddle_plain"] = cls["straddle"] & (meta["vlan"] == 0)
            reach = np.zeros(len(m), bool)
            for byte in range(nb):
                pos = lo + byte
                fo = (pos & ~15) - m                 # frame offset of the byte's chunk
                reach |= on & (pos < RW_SLOT) & ((fo < 0) | (fo + 16 > flen))
            cls["chunk_out"] = reach
            out[name] = {c: set(np.unique(m[v]).tolist()) for c, v in cls.items()}
    if "t" in meta:
        d = m + meta["t"] + meta["end"] - MSS_SLOT
        ok = (meta["inseg"] != 0) & (np.abs(d) <= 4)
        out["mss_dist"] = set(np.unique(d[ok]).tolist())
    return out
