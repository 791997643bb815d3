"""NumPy restatement of the IPv4 fragmentation contract (include/pptk_rx.h,
pptk_ip_fragment_device / pptk_ip_fragment_host) and the frames its tests
run on.

The restatement is independent of the library: the subject test, the plan
(per = (mtu - ihl) & ~7, as few fragments as possible) and the fragment bytes
(header copied, offset / MF / total length rewritten, checksum recomputed
with framegen's own one's-complement sum, payload slice) are written out
here.  tests/golden/gen_fragment_golden.py pins it to the reference through
the reference's own getters and ip_set_hdr_cksum_calc.
"""
import struct

import numpy as np

import framegen

ST_IPV4, ST_FITS, ST_DONE, ST_DF, ST_ISFRAG, ST_BADCKSUM, ST_NOROOM = (
    0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40)
MTUS = (68, 576, 1280, 1500)


def up16(x):
    return (x + 15) & ~15


def subject(f):
    """(l2, ihl, tl) of a frame the receive transform parses as IPv4 (PARSED,
    not MALFORMED), else None."""
    n = len(f)
    if n < 14 or n > 65535:
        return None
    et, l2 = (f[12] << 8) | f[13], 14
    if et == 0x8100:
        if n < 18:
            return None
        et, l2 = (f[16] << 8) | f[17], 18
    if et != 0x0800 or n < l2 + 20:
        return None
    ihl, tl = (f[l2] & 15) * 4, (f[l2 + 2] << 8) | f[l2 + 3]
    if f[l2] >> 4 != 4 or ihl < 20 or tl < ihl or l2 + tl > n:
        return None
    return l2, ihl, tl


def plan(f, mtu):
    """(status, [(datastart, datalen), ...]) of one frame."""
    s = subject(f)
    if s is None:
        return 0, []
    l2, ihl, tl = s
    if tl <= mtu:
        return ST_IPV4 | ST_FITS, []
    st = ST_IPV4
    fw = (f[l2 + 6] << 8) | f[l2 + 7]
    if fw & 0x4000:
        st |= ST_DF
    if fw & 0x3FFF:
        st |= ST_ISFRAG
    if framegen.csum(f[l2:l2 + ihl]) != 0:
        st |= ST_BADCKSUM
    if st != ST_IPV4:
        return st, []
    datamax, per = tl - ihl, (mtu - ihl) & ~7
    return st | ST_DONE, [(ds, min(per, datamax - ds)) for ds in range(0, datamax, per)]


def fragments(f, mtu):
    """(status, [fragment bytes, ...]) of one frame."""
    st, pl = plan(f, mtu)
    if not pl:
        return st, []
    l2, ihl, tl = subject(f)
    datamax, out = tl - ihl, []
    for ds, dl in pl:
        h = bytearray(f[:l2 + ihl])
        fw = (h[l2 + 6] << 8) | h[l2 + 7]
        fw = (fw & 0xC000) | (0x2000 if ds + dl < datamax else 0) | (ds >> 3)
        struct.pack_into(">H", h, l2 + 2, ihl + dl)
        struct.pack_into(">H", h, l2 + 6, fw)
        struct.pack_into(">H", h, l2 + 10, 0)
        struct.pack_into(">H", h, l2 + 10, framegen.csum(h[l2:]))
        out.append(bytes(h) + bytes(f[l2 + ihl + ds:l2 + ihl + ds + dl]))
    return st, out


def fragment_batch(frames, mtu, out_cap=None):
    """The whole contract for a list of frames (bytes each): dict with frags
    (the written fragments, in slot order), out_len, out_src, first, count,
    status, totals = [needed, written]."""
    n = len(frames)
    first, count = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    status = np.zeros(n, np.uint8)
    frags, src, pos, written = [], [], 0, None
    for i, f in enumerate(frames):
        st, fr = fragments(f, mtu)
        first[i], count[i] = pos & 0xFFFFFFFF, len(fr)
        if fr and out_cap is not None and pos + len(fr) > out_cap:
            st |= ST_NOROOM
            if written is None:
                written = pos
        elif fr:
            frags += fr
            src += [i] * len(fr)
        status[i] = st
        pos += len(fr)
    if written is None:
        written = pos
    assert len(frags) == written
    return dict(mtu=mtu, frags=frags, out_len=np.array([len(x) for x in frags], np.uint16),
                out_src=np.array(src, np.uint32), first=first, count=count, status=status,
                totals=np.array([pos, written], np.uint64))


def slots(frags, out_stride, nslots, fill=0xEE):
    """The slot buffer a call leaves behind in `nslots` slots pre-filled with
    `fill`: the fragment, zeros to the next 16-byte boundary, the rest
    untouched."""
    out = np.full((nslots, out_stride), fill, np.uint8)
    for s, fr in enumerate(frags):
        out[s, :len(fr)] = np.frombuffer(fr, np.uint8)
        out[s, len(fr):up16(len(fr))] = 0
    return out.reshape(-1)


def check_with(lib, frames, res):
    """Pin the restated fragments to a per-packet implementation (`lib`: the
    Reference or the Oracle of oracle/oracle.py): its ip_set_hdr_cksum_calc
    (tx_batch) changes no byte of them, and its getters (frag_batch: ip_id,
    ip_frag_off, ip_more_frags, ip_dont_frag, ip_total_len) return the plan.
    Returns the number of fragments checked."""
    from pptk_amd.records import FRAG_DF, FRAG_IS, FRAG_MF
    if not res["frags"]:
        return 0
    buf, off, lens = framegen.pack(res["frags"])
    assert np.array_equal(lib.tx_batch(buf, off=off, lens=lens), buf)
    side = lib.frag_batch(buf, off=off, lens=lens)
    want = []
    for i, f in enumerate(frames):
        if res["status"][i] & ST_NOROOM:
            continue
        st, pl = plan(f, int(res["mtu"]))
        if not pl:
            continue
        l2, ihl, tl = subject(f)
        for ds, dl in pl:
            want.append(((f[l2 + 4] << 8) | f[l2 + 5], ds, dl, f[l2 + 9],
                         FRAG_IS | (FRAG_MF if ds + dl < tl - ihl else 0)))
    w = np.array(want, np.int64)
    assert len(w) == len(side)
    for k, name in enumerate(("ident", "frag_off", "data_len", "next_hdr", "flags")):
        assert np.array_equal(side[name].astype(np.int64), w[:, k]), name
    assert not (side["flags"] & FRAG_DF).any()
    return len(w)


# ------------------------------------------------------------------ frames
def _payload(rng, n, pattern=False):
    if pattern:   # compressible (the fixture's two big frames), period 251
        return (np.arange(n) % 251).astype(np.uint8).tobytes()
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def frame4(rng, tl, ihl=20, vlan=None, df=False, mf=False, frag_off=0, rsvd=False,
           badck=False, pad=0, proto=17, pattern=False):
    """Ethernet + IPv4 (ihl bytes of header, random options) + payload, the
    IP packet exactly `tl` bytes, `pad` bytes of Ethernet padding after it."""
    opts = rng.integers(0, 256, ihl - 20, dtype=np.uint8).tobytes()
    src = bytes([10]) + rng.integers(0, 256, 3, dtype=np.uint8).tobytes()
    dst = bytes([192, 168]) + rng.integers(0, 256, 2, dtype=np.uint8).tobytes()
    h = bytearray(framegen.ipv4_hdr(src, dst, proto, tl - ihl, opts, df=df, mf=mf,
                                    frag_off=frag_off, ident=int(rng.integers(0, 65536)),
                                    fix=False))
    if rsvd:
        h[6] |= 0x80
    struct.pack_into(">H", h, 10, framegen.csum(h))
    if badck:
        h[10] ^= 0x40
    return (framegen.eth(framegen.ETH_IP, vlan) + bytes(h) + _payload(rng, tl - ihl, pattern)
            + _payload(rng, pad))


def other_frames(rng):
    """Non-subjects: IPv6, ARP, a truncated IPv4 frame, runts, an empty frame."""
    trunc = frame4(rng, 1400)[:700]
    return [framegen.frame_v6(rng, 17, 1400), framegen.frame_v6(rng, 6, 90),
            framegen.eth(0x0806) + _payload(rng, 46),
            trunc, _payload(rng, 13), frame4(rng, 1400)[:33], b""]


def fixture_frames(seed=0xF4A6):
    """The smallest shapes where fragmentation can go wrong, for every mtu of
    MTUS (listed in tests/test_fragment.py's docstring)."""
    rng = np.random.default_rng(seed)
    fr = []
    for mtu in MTUS:
        per = (mtu - 20) & ~7
        fr += [frame4(rng, mtu), frame4(rng, mtu + 1)]
        for k in (1, 2):
            for extra in (0, 1, 7, 8):
                fr.append(frame4(rng, 20 + k * per + extra, pad=(k * 5 + extra) % 16))
        for ihl in (24, 40, 60):
            p = (mtu - ihl) & ~7
            fr += [frame4(rng, mtu, ihl), frame4(rng, mtu + 1, ihl, vlan=ihl),
                   frame4(rng, ihl + 2 * p + 1, ihl, pad=ihl % 16 + 1)]
    # mtu 68 with ihl 60: 8 bytes per fragment, 180 fragments
    fr.append(frame4(rng, 1500, 60))
    fr += [frame4(rng, 9000 - 14, pattern=True), frame4(rng, 65521, pattern=True)]
    # padding of 1..15 bytes, odd and even lengths, with and without a tag
    for pad in range(1, 16):
        fr.append(frame4(rng, 1501 + 3 * pad, (20, 24, 40, 60)[pad % 4], pad=pad,
                         vlan=5 if pad % 3 == 0 else None))
    # fragment4's abort conditions (too big for every mtu) and the kept bits
    fr += [frame4(rng, 1600, df=True), frame4(rng, 1600, mf=True),
           frame4(rng, 1600, frag_off=100), frame4(rng, 1600, df=True, mf=True, badck=True),
           frame4(rng, 1600, badck=True), frame4(rng, 1600, rsvd=True),
           frame4(rng, 60, df=True), frame4(rng, 60, badck=True)]
    return fr + other_frames(rng)


def random_frames(n, seed):
    """n frames of 64..1600 bytes, about half longer than both 576 + 14 and
    1280 + 14, mixing the fixture's shapes."""
    rng = np.random.default_rng(seed)
    u = rng.random(n)
    big = rng.random(n) < 0.5
    ln = np.where(big, rng.integers(1300, 1601, n), rng.integers(64, 571, n))
    ihls = rng.choice([20, 20, 20, 24, 40, 60], n)
    fr = []
    for i in range(n):
        L, ihl, x = int(ln[i]), int(ihls[i]), u[i]
        vlan = 9 if (i % 11) == 0 else None
        l2 = 18 if vlan is not None else 14
        pad = int(i % 16) if (i % 7) == 0 else 0
        tl = max(L - l2 - pad, ihl + 8)
        if x < 0.05:
            fr.append(framegen.frame_v6(rng, 17, max(L, 70)))
        elif x < 0.08:
            fr.append(b"\xff" * 6 + b"\x02\0\0\0\0\x02\x08\x06" + _payload(rng, L - 14))
        elif x < 0.10:
            fr.append(frame4(rng, tl, ihl, vlan)[:l2 + tl - 5])      # truncated
        elif x < 0.11:
            fr.append(_payload(rng, i % 14))                          # runt / empty
        elif x < 0.16:
            fr.append(frame4(rng, tl, ihl, vlan, df=True, pad=pad))
        elif x < 0.19:
            fr.append(frame4(rng, tl, ihl, vlan, mf=bool(i & 1), frag_off=(i & 2) * 50, pad=pad))
        elif x < 0.21:
            fr.append(frame4(rng, tl, ihl, vlan, badck=True, pad=pad))
        else:
            fr.append(frame4(rng, tl, ihl, vlan, rsvd=(i % 13) == 0, pad=pad))
    return fr
