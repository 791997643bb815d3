"""NumPy restatement of the IPv4 reassembly contract (include/pptk_rx.h,
pptk_ip_reass_device / pptk_ip_reass_host) and the frames its tests run on.

The restatement is independent of the library: the per-frame tests, the
grouping by (src, dst, proto, ident), the ordering, the status precedence and
the slot bytes (leader's header, offset / MF cleared, total length rewritten,
checksum recomputed with framegen's own one's-complement sum, payloads placed
at their offsets) are written out here.  Honest inputs come from the
fragmenter's restatement (fraggen.fragments), which is pinned to the
reference's fragment4.
"""
import struct

import numpy as np

import fraggen
import framegen
from pptk_amd.records import (F_FRAGMENT, F_IPV6, F_MALFORMED, F_PARSED, FRAG_MF,
                              REASS_DGRAM_DTYPE, REASS_HDR_DTYPE)

(FST_FRAG, FST_BADCKSUM, FST_BADFRAG, FST_SKIPPED, FST_MEMBER, FST_DONE) = (
    0x01, 0x02, 0x04, 0x08, 0x10, 0x20)
(DG_COMPLETE, DG_WRITTEN, DG_INCOMPLETE, DG_OVERLAP, DG_TOOMANY, DG_TOOBIG, DG_NOROOM) = (
    0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40)
NONE, MAX_FRAGS = 0xFFFFFFFF, 64
KEY = bytes(range(1, 17))


def up16(x):
    return (x + 15) & ~15


def decide(members):
    """(status, total) of one datagram from its (off, dl, mf) triples in
    (off, frame index) order."""
    if len(members) > MAX_FRAGS:
        return DG_TOOMANY, 0
    lasts = [k for k, m in enumerate(members) if not m[2]]
    pairs = list(zip(members, members[1:]))
    if (any(a[0] + a[1] > b[0] for a, b in pairs) or len(lasts) > 1
            or (lasts and lasts[0] != len(members) - 1)):
        return DG_OVERLAP, 0
    if not lasts or members[0][0] != 0 or any(a[0] + a[1] < b[0] for a, b in pairs):
        return DG_INCOMPLETE, 0
    return DG_COMPLETE, members[-1][0] + members[-1][1]


def reassemble(frames, recs, frag, max_candidates, out_cap, out_stride, report_cap=None):
    """The whole contract for a list of frames (bytes each) with their records
    and fragment side records: dict with fstatus, dgram, report (every
    datagram, not cut to report_cap), hdr, slots (the written slots' bytes, in
    slot order) and out_len."""
    n = len(frames)
    report_cap = n if report_cap is None else report_cap
    fst, dgram = np.zeros(n, np.uint8), np.full(n, NONE, np.uint32)
    cands, info = [], {}
    for i, f in enumerate(frames):
        fl = int(recs[i]["flags"])
        if not (fl & F_PARSED and fl & F_FRAGMENT) or fl & (F_MALFORMED | F_IPV6):
            continue
        st = FST_FRAG
        l3, off, dl = int(recs[i]["l3_off"]), int(frag[i]["frag_off"]), int(frag[i]["data_len"])
        mf = bool(int(frag[i]["flags"]) & FRAG_MF)
        if int(recs[i]["ip_cksum"]) != 0:
            st |= FST_BADCKSUM
        bad, ihl = l3 not in (14, 18) or len(f) <= l3, 0
        if not bad:
            ihl = (f[l3] & 15) * 4
            bad = (ihl < 20 or dl == 0 or off + dl > 65535 or (mf and dl % 8 != 0)
                   or l3 + ihl + dl > len(f))
        if bad:
            st |= FST_BADFRAG
        fst[i] = st
        if st == FST_FRAG:
            cands.append(i)
            info[i] = (off, dl, mf, l3, ihl)
    for i in cands[max_candidates:]:
        fst[i] |= FST_SKIPPED
    groups = {}   # insertion order = ascending leader index
    for i in cands[:max_candidates]:
        key = (bytes(recs[i]["src"][:4]), bytes(recs[i]["dst"][:4]), int(recs[i]["proto"]),
               int(frag[i]["ident"]) & 0xFFFF)
        groups.setdefault(key, []).append(i)
    report = np.zeros(len(groups), REASS_DGRAM_DTYPE)
    slots, taken, complete = [], 0, 0
    for k, idx in enumerate(groups.values()):
        fst[idx] |= FST_MEMBER
        dgram[idx] = k
        order = sorted(idx, key=lambda i: (info[i][0], i))
        st, total = decide([info[i][:3] for i in order])
        slot, olen = NONE, 0
        if st == DG_COMPLETE:
            complete += 1
            lead = idx[0]
            l2, ihl = info[lead][3], info[lead][4]
            flen = l2 + ihl + total
            olen = flen if flen <= 65535 else 0
            if flen > 65535 or up16(flen) > out_stride:
                st |= DG_TOOBIG
            elif taken >= out_cap:
                st |= DG_NOROOM
                taken += 1
            else:
                st |= DG_WRITTEN
                slot, taken = taken, taken + 1
                h = bytearray(frames[lead][:l2 + ihl])
                fw = ((h[l2 + 6] << 8) | h[l2 + 7]) & 0xC000
                struct.pack_into(">H", h, l2 + 2, ihl + total)
                struct.pack_into(">H", h, l2 + 6, fw)
                struct.pack_into(">H", h, l2 + 10, 0)
                struct.pack_into(">H", h, l2 + 10, framegen.csum(h[l2:]))
                pay = bytearray(total)
                for i in order:
                    off, dl, _, l3, hl = info[i]
                    pay[off:off + dl] = frames[i][l3 + hl:l3 + hl + dl]
                slots.append(bytes(h) + bytes(pay))
                fst[idx] |= FST_DONE
        report[k] = (idx[0], slot, len(idx), olen, st, 0)
    hdr = np.zeros(1, REASS_HDR_DTYPE)[0]
    hdr["candidates"], hdr["considered"] = len(cands), min(len(cands), max_candidates)
    hdr["dgrams"], hdr["reported"] = len(groups), min(len(groups), report_cap)
    hdr["complete"], hdr["written"] = complete, len(slots)
    return dict(fstatus=fst, dgram=dgram, report=report, hdr=hdr, slots=slots,
                out_len=np.array([len(s) for s in slots], np.uint16))


def records(lib, frames, align=1, key=KEY):
    """Pack `frames` and run them through the receive transform of `lib` (the
    Oracle or the Reference of oracle/oracle.py): (buf, off, lens, recs,
    frag)."""
    from oracle.oracle import make_opts
    buf, off, lens = framegen.pack(frames, align=align)
    recs = lib.rx_batch(buf, off, lens, opts=make_opts(key, 24, 48, 4096))
    side = lib.frag_batch(buf, off=off, lens=lens)
    return buf, off, lens, recs, side


def check_with(lib, slots):
    """Pin reassembled slots to a per-packet implementation (`lib`: the
    Reference or the Oracle of oracle/oracle.py): its ip_hdr_cksum_calc over
    every header is 0 (rx_batch), its ip_set_hdr_cksum_calc (tx_batch) changes
    no header byte, and its getters (frag_batch) return offset 0, MF clear and
    the data length the total length gives.  Returns the number checked."""
    from oracle.oracle import make_opts
    if not slots:
        return 0
    buf, off, lens = framegen.pack(slots)
    recs = lib.rx_batch(buf, off, lens, opts=make_opts(KEY, 24, 48, 4096))
    assert np.all(recs["flags"] & F_PARSED) and not np.any(recs["flags"] & (F_FRAGMENT | F_MALFORMED))
    assert not recs["ip_cksum"].any()
    sent = lib.tx_batch(buf, off=off, lens=lens)
    side = lib.frag_batch(buf, off=off, lens=lens)
    assert not side["frag_off"].any() and not (side["flags"] & 0x03).any()
    for s, o, d in zip(slots, off, side):
        l2 = 14 if s[12:14] == b"\x08\x00" else 18
        H = l2 + (s[l2] & 15) * 4
        assert np.array_equal(sent[int(o):int(o) + H], buf[int(o):int(o) + H])
        assert int(d["data_len"]) == len(s) - H
    return len(slots)


# ------------------------------------------------------------------ frames
def frag4(src, dst, ident, off, payload, mf, proto=17, ihl=20, vlan=None, df=False, rsvd=False,
          badck=False, pad=0, opts=None, ttl=64):
    """One IPv4 fragment: Ethernet (+ tag) + ihl bytes of header + payload."""
    assert off % 8 == 0
    opts = bytes((7 * k + ihl) & 0xFF for k in range(ihl - 20)) if opts is None else opts
    h = bytearray(framegen.ipv4_hdr(bytes(src), bytes(dst), proto, len(payload), opts, df=df,
                                    mf=mf, frag_off=off >> 3, ident=ident, ttl=ttl, fix=False))
    if rsvd:
        h[6] |= 0x80
    struct.pack_into(">H", h, 10, framegen.csum(h))
    if badck:
        h[10] ^= 0x40
    return framegen.eth(framegen.ETH_IP, vlan) + bytes(h) + bytes(payload) + bytes(pad)


def split(rng, ident, sizes, src=(10, 0, 0, 1), dst=(192, 168, 0, 1), proto=17, last_mf=False,
          **kw):
    """A datagram cut into len(sizes) fragments of those payload sizes."""
    out, off = [], 0
    for j, sz in enumerate(sizes):
        pay = rng.integers(0, 256, sz, dtype=np.uint8).tobytes()
        out.append(frag4(src, dst, ident, off, pay, j + 1 < len(sizes) or last_mf, proto, **kw))
        off += sz
    return out


def honest(rng, tl, mtu, ihl=20, vlan=None, **kw):
    """The fragments the fragmenter's restatement makes of one whole frame,
    and the frame (its Ethernet padding cut)."""
    f = fraggen.frame4(rng, tl, ihl, vlan, **kw)
    st, fr = fraggen.fragments(f, mtu)
    assert st & fraggen.ST_DONE
    return fr, f[:(18 if vlan is not None else 14) + tl]


def fixture_frames(seed=0x4EA5):
    """The smallest shapes where reassembly can go wrong (the list is in
    tests/test_reass.py's docstring), a few hundred frames."""
    rng = np.random.default_rng(seed)
    F = []
    # honest datagrams, in order, reversed and interleaved
    a, _ = honest(rng, 1500, 576)
    b, _ = honest(rng, 1501, 576, ihl=24, vlan=7)
    c, _ = honest(rng, 3000, 1500, ihl=60, rsvd=True)
    F += a + b[::-1] + [x for pair in zip(c, honest(rng, 2999, 1500)[0]) for x in pair]
    # the 65535-byte datagram: l2 + ihl + total = 65535
    big, _ = honest(rng, 65535 - 14, 1500, pattern=True)
    order = rng.permutation(len(big))
    F += [big[j] for j in order]
    # ihl + total = 65535: complete, but 65549 bytes do not fit a length word
    F += split(rng, 150, [8184] * 8 + [43])
    # keys that differ in one field only, interleaved
    k1 = split(rng, 100, [16, 16, 8])
    k2 = split(rng, 101, [16, 16, 8])
    k3 = split(rng, 100, [16, 16, 8], proto=6)
    k4 = split(rng, 100, [16, 16, 8], dst=(192, 168, 0, 2))
    k5 = split(rng, 100, [16, 16, 8], src=(10, 0, 0, 2))
    F += [x for grp in zip(k1, k2, k3, k4, k5) for x in grp]
    # 64 and 65 eight-byte fragments
    F += split(rng, 200, [8] * 64)[::-1] + split(rng, 201, [8] * 65)
    # holes: first, middle, last missing; MF on the last
    for ident, drop in ((300, 0), (301, 1), (302, 2)):
        s = split(rng, ident, [24, 24, 24])
        F += s[:drop] + s[drop + 1:]
    F += split(rng, 303, [8, 8], last_mf=True)
    # overlaps: exact duplicate, partial, data past the last, two lasts
    s = split(rng, 400, [16, 16, 8])
    F += s + [s[1]]
    s = split(rng, 401, [16, 16, 8])
    F += [s[0], frag4((10, 0, 0, 1), (192, 168, 0, 1), 401, 8, bytes(16), True), s[1], s[2]]
    s = split(rng, 402, [16, 8])
    F += s + [frag4((10, 0, 0, 1), (192, 168, 0, 1), 402, 32, bytes(8), True)]
    s = split(rng, 403, [16, 8])
    F += s + [frag4((10, 0, 0, 1), (192, 168, 0, 1), 403, 16, bytes(16), False)]
    # leader and members with different l2 and ihl, odd payload on the last
    F += [frag4((10, 1, 1, 1), (10, 2, 2, 2), 500, 0, rng.bytes(24), True, ihl=24, vlan=3),
          frag4((10, 1, 1, 1), (10, 2, 2, 2), 500, 24, rng.bytes(13), False, ihl=60),
          frag4((10, 1, 1, 1), (10, 2, 2, 2), 501, 8, rng.bytes(7), False, ihl=20, pad=5),
          frag4((10, 1, 1, 1), (10, 2, 2, 2), 501, 0, rng.bytes(8), True, ihl=40, vlan=9)]
    # rejected fragments: bad checksum, MF with an odd length, beyond 65535
    F += [frag4((10, 3, 3, 3), (10, 2, 2, 2), 600, 0, rng.bytes(16), True, badck=True),
          frag4((10, 3, 3, 3), (10, 2, 2, 2), 600, 16, rng.bytes(8), False),
          frag4((10, 3, 3, 3), (10, 2, 2, 2), 601, 0, rng.bytes(12), True),
          frag4((10, 3, 3, 3), (10, 2, 2, 2), 602, 65528, rng.bytes(16), False)]
    # non-fragments: whole packets, IPv6 (with a fragment header too), ARP, runts
    v6f = framegen.frame_v6(rng, 17, 200, ext=[(44, bytes([0, 0, 0, 1, 0, 0, 0, 9]))])
    F += [frag4((10, 4, 4, 4), (10, 2, 2, 2), 700, 0, rng.bytes(40), False), v6f]
    F += fraggen.other_frames(rng)
    return F


def random_mix(nframes, ndg, seed):
    """About `nframes` frames: the shuffled fragments of `ndg` datagrams with
    bad checksums, duplicates, holes and partial overlaps among them, plus
    non-fragments, IPv6 fragments and malformed frames."""
    rng = np.random.default_rng(seed)
    F = []
    for d in range(ndg):
        u = rng.random()
        src, dst = (10, int(rng.integers(0, 4)), 0, 1), (192, 168, int(rng.integers(0, 4)), 1)
        ident = d if d % 9 else d - 1   # some keys collide
        if u < 0.04:
            fr = split(rng, ident, [8] * int(rng.integers(60, 70)), src, dst)
        else:
            tl = int(rng.integers(700, 4000))
            ihl = int(rng.choice([20, 20, 24, 60]))
            fr = honest(rng, tl, int(rng.choice([576, 1280, 1500])), ihl,
                        vlan=5 if d % 7 == 0 else None)[0] if tl > 1520 else \
                split(rng, ident, [int(8 * rng.integers(1, 40)) for _ in range(int(rng.integers(2, 5)))],
                      src, dst, ihl=ihl)
        fr = list(fr)
        if 0.04 <= u < 0.14 and len(fr) > 1:
            del fr[int(rng.integers(0, len(fr)))]                       # a hole
        elif u < 0.22:
            fr.append(fr[int(rng.integers(0, len(fr)))])                # a duplicate
        elif u < 0.30 and len(fr) > 1:
            g = bytearray(fr[0])                                        # a partial overlap
            l2 = 14 if g[12:14] == b"\x08\x00" else 18
            hl = (g[l2] & 15) * 4
            struct.pack_into(">H", g, l2 + 6, (((g[l2 + 6] << 8) | g[l2 + 7]) & 0xE000) | 1)
            struct.pack_into(">H", g, l2 + 10, 0)
            struct.pack_into(">H", g, l2 + 10, framegen.csum(g[l2:l2 + hl]))
            fr.append(bytes(g))
        elif u < 0.36:
            g = bytearray(fr[-1])                                       # a bad checksum
            g[(14 if g[12:14] == b"\x08\x00" else 18) + 10] ^= 0x11
            fr[-1] = bytes(g)
        F += fr
    for _ in range(max(nframes - len(F), nframes // 8)):
        u = rng.random()
        if u < 0.1:                                                     # MF and an odd length
            F.append(frag4((10, 9, 9, 9), (10, 8, 8, 8), int(rng.integers(0, 65536)), 0,
                           rng.bytes(int(rng.integers(1, 8))), True))
        elif u < 0.5:
            F.append(framegen.frame_v4(rng, 17, int(rng.integers(64, 1500))))
        elif u < 0.7:
            F.append(framegen.frame_v6(rng, 17, 200, ext=[(44, bytes([0, 0, 0, 1, 0, 0, 0, 9]))]))
        elif u < 0.85:
            F.append(fraggen.frame4(rng, 400, mf=True)[:200])           # truncated: malformed
        else:
            F.append(rng.bytes(int(rng.integers(0, 40))))
    order = rng.permutation(len(F))
    return [F[j] for j in order]
