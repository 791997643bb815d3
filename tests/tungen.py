"""NumPy restatement of the GRE tunnel contracts (include/pptk_rx.h,
pptk_tunnel_encap_* / pptk_tunnel_decap_*) and the frames their tests run on.

The restatement is independent of the library: the 38-byte header is packed
field by field with struct, its checksum is framegen's own one's-complement
sum, the decap checks are written out.  tests/golden/gen_tunnel_golden.py
pins it to the reference through the reference's ip_hdr_cksum_calc,
ip_set_hdr_cksum_calc and receive parse (check_with below).
"""
import struct

import numpy as np

import fraggen
import framegen
from pptk_amd.records import REC_DTYPE, TUNNEL_DTYPE

HDR = 38
TUN_DF, TUN_ID_SEQ = 0x1, 0x2
ST_DONE, ST_RUNT, ST_TOOBIG, ST_NOROOM, ST_NOFLOW, ST_BADTUN = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
(D_IPV4, D_GRE, D_OK, D_ISFRAG, D_BADCKSUM, D_SHORT, D_GREOPT,
 D_PTYPE) = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80
NOFLOW = 0xFFFFFFFF

ID_BASE = 0x10005          # with tunnel 1's id 0xfff0: ids 0xfff5 + i, wrapping at i = 11
FULL_STRIDE = 65536        # every frame that is not TOOBIG fits
NR_STRIDE = 1552           # 38 + 1514 fits exactly; the 9000-byte frame and up NOROOM


def up16(x):
    return (x + 15) & ~15


# ------------------------------------------------------------------- encap
def header(t, length, seq):
    """The 38 bytes in front of a frame of `length` bytes in tunnel t (one
    TUNNEL_DTYPE entry)."""
    flags = int(t["flags"])
    ident = (int(t["id"]) + (seq if flags & TUN_ID_SEQ else 0)) & 0xFFFF
    ip = bytearray(struct.pack(">BBHHHBBHII", 0x45, int(t["tos"]), length + 24, ident,
                               0x4000 if flags & TUN_DF else 0, int(t["ttl"]), 47, 0,
                               int(t["src"]), int(t["dst"])))
    struct.pack_into(">H", ip, 10, framegen.csum(ip))
    return (bytes(t["eth_dst"]) + bytes(t["eth_src"]) + b"\x08\x00" + bytes(ip)
            + b"\x00\x00\x65\x58")


def encap(f, t, seq, room):
    """(status, slot bytes or None) of one frame; t None = no tunnel."""
    if t is None:
        return ST_NOFLOW, None
    if int(t["reserved"]) or int(t["flags"]) & ~(TUN_DF | TUN_ID_SEQ):
        return ST_BADTUN, None
    n = len(f)
    if n < 14:
        return ST_RUNT, None
    st = (ST_TOOBIG if HDR + n > 65535 else 0) | (ST_NOROOM if HDR + n > room else 0)
    if st:
        return st, None
    return ST_DONE, header(t, n, seq) + bytes(f)


def encap_batch(frames, tun, idx=None, id_base=0, out_stride=FULL_STRIDE):
    """The whole contract for a list of frames: dict with slots (bytes or
    None per frame), out_len, status.  tun: TUNNEL_DTYPE array of 1 or n
    entries, or a table indexed by idx."""
    n = len(frames)
    assert idx is not None or len(tun) in (1, n)
    slots, status = [], np.zeros(n, np.uint8)
    for i, f in enumerate(frames):
        k = int(idx[i]) if idx is not None else (0 if len(tun) == 1 else i)
        st, s = encap(f, tun[k] if k < len(tun) else None, (id_base + i) & 0xFFFFFFFF, out_stride)
        slots.append(s)
        status[i] = st
    return dict(slots=slots, status=status,
                out_len=np.array([len(s) if s else 0 for s in slots], np.uint16))


def slot_buffer(slots, out_stride, fill=0xEE):
    """What a call leaves in len(slots) slots pre-filled with `fill`: the
    packet, zeros to the next 16-byte boundary, the rest untouched."""
    out = np.full((len(slots), out_stride), fill, np.uint8)
    for i, s in enumerate(slots):
        if s is not None:
            out[i, :len(s)] = np.frombuffer(s, np.uint8)
            out[i, len(s):up16(len(s))] = 0
    return out.reshape(-1)


# ------------------------------------------------------------------- decap
def decap(f):
    """(status, in_off relative to the frame, in_len) of one frame."""
    s = fraggen.subject(f)
    if s is None:
        return 0, 0, 0
    l2, ihl, tl = s
    st = D_IPV4
    if f[l2 + 9] != 47:
        return st, 0, 0
    fw = (f[l2 + 6] << 8) | f[l2 + 7]
    if fw & 0x3FFF:
        st |= D_ISFRAG
    if framegen.csum(f[l2:l2 + ihl]) != 0:
        st |= D_BADCKSUM
    if st & D_ISFRAG:
        return st, 0, 0
    if tl - ihl < 4:
        return st | D_SHORT, 0, 0
    st |= D_GRE
    g = l2 + ihl
    if f[g] or f[g + 1]:
        st |= D_GREOPT
    if (f[g + 2], f[g + 3]) != (0x65, 0x58):
        st |= D_PTYPE
    if st & (D_BADCKSUM | D_GREOPT | D_PTYPE):
        return st, 0, 0
    return st | D_OK, g + 4, tl - ihl - 4


def decap_batch(frames, off):
    """status, absolute in_off (off = the frames' byte offsets), in_len."""
    r = [decap(f) for f in frames]
    return dict(status=np.array([x[0] for x in r], np.uint8),
                in_off=np.asarray(off, np.uint64) + np.array([x[1] for x in r], np.uint64),
                in_len=np.array([x[2] for x in r], np.uint16))


# ------------------------------------------------------------------ frames
def tunnels():
    """The fixture's tunnel table: DF with a fixed id; no DF with ids that
    count up and wrap; another tos / ttl / addresses."""
    t = np.zeros(3, TUNNEL_DTYPE)
    t[0] = ([2, 0, 0, 0, 0, 0x11], [2, 0, 0, 0, 0, 0x22], (10 << 24) | 1, (10 << 24) | 2,
            0, 64, 0, TUN_DF, 0)
    t[1] = ([0x02, 0xAA, 0xBB, 0xCC, 0xDD, 0xEE], [0x02, 0x10, 0x20, 0x30, 0x40, 0x50],
            0xC0A80101, 0xC633640A, 0xFFF0, 255, 0xB8, TUN_ID_SEQ, 0)
    t[2] = ([0xFF] * 6, [0x06, 5, 4, 3, 2, 1], 0xFFFFFFFF, 0x01020304, 0x1234, 1, 0x03,
            TUN_DF | TUN_ID_SEQ, 0)
    return t


def inner_frame(rng, n, pattern=False):
    """A frame of exactly n bytes: Ethernet + IPv4 + payload where that fits
    (n >= 42), else random bytes."""
    if n < 42:
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    return fraggen.frame4(rng, n - 14, proto=17, pattern=pattern)


ENCAP_LENS = ([0, 13, 14, 15, 16, 17]
              + [m + d - HDR for m in range(48, 129, 16) for d in (-1, 0, 1)]
              + [60, 64, 1500, 1514, 9000, 65497, 65498, 65535])


def encap_frames(seed=0x6558):
    rng = np.random.default_rng(seed)
    return [inner_frame(rng, n, pattern=n >= 9000) for n in ENCAP_LENS]


def encap_idx(n):
    """Tunnels 0, 1, 2 in turn, every seventh frame without one."""
    idx = np.arange(n, dtype=np.uint32) % 3
    idx[5::7] = NOFLOW
    return idx


def modes(n):
    """name -> (tunnel array, idx or None): the three ways a frame finds its
    tunnel.  'idx': the table through encap_idx; 'one': tunnel 1 for every
    frame (its ids wrap at frame 11); 'per': one entry per frame."""
    t = tunnels()
    return {"idx": (t, encap_idx(n)), "one": (t[1:2].copy(), None),
            "per": (t[(np.arange(n) + 1) % 3].copy(), None)}


def mode_idx(name, n):
    """The table index of every frame's tunnel in modes(n)[name]."""
    return {"idx": encap_idx(n), "one": np.zeros(n, np.uint32),
            "per": np.arange(n, dtype=np.uint32)}[name]


def outer(inner, ihl=20, vlan=None, pad=0, proto=47, mf=False, frag_off=0, gre0=0,
          ptype=0x6558, badck=False, tl=None, rng=None):
    """Ethernet (+ tag) + IPv4 with ihl bytes of header + GRE + inner + pad."""
    rng = rng or np.random.default_rng(len(inner))
    opts = rng.integers(0, 256, ihl - 20, dtype=np.uint8).tobytes()
    body = struct.pack(">HH", gre0, ptype) + bytes(inner)
    h = bytearray(framegen.ipv4_hdr(bytes([10, 0, 0, 1]), bytes([10, 0, 0, 2]), proto, len(body),
                                    opts, df=False, mf=mf, frag_off=frag_off, ident=7, fix=False))
    if tl is not None:
        struct.pack_into(">H", h, 2, tl)
    struct.pack_into(">H", h, 10, framegen.csum(h))
    if badck:
        h[10] ^= 0x40
    return framegen.eth(framegen.ETH_IP, vlan) + bytes(h) + body + bytes(pad)


def decap_frames(seed=0x2F):
    """The shapes listed in tests/test_tunnel.py's docstring, in that order."""
    rng = np.random.default_rng(seed)
    a, b = inner_frame(rng, 64), inner_frame(rng, 1500)
    v6 = framegen.frame_v6(rng, 17, 120)
    return [
        outer(a), outer(b), outer(a, vlan=5), outer(b, vlan=0xFFF),
        outer(a, ihl=24), outer(b, ihl=24, vlan=9),
        outer(a, pad=7), outer(inner_frame(rng, 61), pad=15),
        outer(b""), outer(b"", ihl=24),
        outer(a, badck=True),
        outer(a, proto=6), outer(a, proto=17),
        v6,
        outer(a, mf=True), outer(a, frag_off=3), outer(a, mf=True, frag_off=100),
        outer(b"", pad=3), outer(b"", tl=23)[:14 + 23], outer(b"", ihl=24, tl=27)[:14 + 27],
        outer(a)[:-1], outer(a, vlan=2)[:-1],
        outer(a)[:13], outer(a)[:37], outer(a)[:33], b"",
        outer(a, gre0=0x8000), outer(a, gre0=0x2000), outer(a, gre0=0x1000), outer(a, gre0=0x0001),
        outer(a, ptype=0x0800),
        outer(a, badck=True, ptype=0x0800), outer(a, gre0=0xB001, ptype=0x88BE),
        outer(a, mf=True, badck=True), outer(b"", tl=22, badck=True)[:14 + 22],
        outer(a, gre0=0x2000, badck=True),
    ]


# ------------------------------------------------------------ reference pin
def check_with(lib, frames, res, tun, idx):
    """Pin the restated DONE slots to a per-packet implementation (`lib`: the
    Reference or the Oracle of oracle/oracle.py).  Returns how many were
    checked."""
    from oracle.oracle import make_opts
    from pptk_amd.records import F_IP_OK, F_IPV6, F_MALFORMED, F_PARSED
    done = [i for i, s in enumerate(res["slots"]) if s is not None]
    slots = [res["slots"][i] for i in done]
    buf, off, lens = framegen.pack(slots)
    opts = make_opts(bytes(range(1, 17)))
    hck = getattr(lib.lib, "ref_ip_hdr_cksum_calc", None)
    if hck is not None:
        assert all(hck(s[14:34], 20) == 0 for s in slots)
    else:
        assert all(lib.cksum(s[14:34]) == 0 for s in slots)
    # its ip_set_hdr_cksum_calc (and no L4 setter: proto 47) changes no byte
    assert np.array_equal(lib.tx_batch(buf, off=off, lens=lens), buf)
    rec = lib.rx_batch(buf, off=off, lens=lens, opts=opts)
    assert np.all(rec["flags"] & (F_PARSED | F_IP_OK | F_IPV6 | F_MALFORMED) == F_PARSED | F_IP_OK)
    assert np.all(rec["proto"] == 47) and np.all(rec["l3_off"] == 14)
    for r, i in zip(rec, done):
        t = tun[int(idx[i])]
        assert bytes(r["src"][:4]) == struct.pack(">I", int(t["src"]))
        assert bytes(r["dst"][:4]) == struct.pack(">I", int(t["dst"]))
    # the inner frame behind the header is the original, to the receive parse
    inner = lib.rx_batch(buf, off=off + np.uint64(HDR), lens=lens - np.uint16(HDR), opts=opts)
    fbuf, foff, flen = framegen.pack([frames[i] for i in done])
    orig = lib.rx_batch(fbuf, off=foff, lens=flen, opts=opts)
    assert inner.dtype == REC_DTYPE and np.array_equal(inner, orig)
    return len(done)
