"""The independent model of the flow table (include/pptk_rx.h "Flow table")
and the frames, flows and values behind tests/golden/flow.npz.

Model is the reference's table (hashtable/hashtable.h) in Python: bucketcnt
buckets addressed by hashval & (bucketcnt - 1) with hashval the low 32 bits of
the 64-bit hash, each bucket a list of candidates walked in order, the first
whose hash and key match wins -- plus this API's own rules: -EEXIST, -ENOSPC
at slots / 2 entries, -EINVAL for a bad key or value, the subject rule and
PPTK_FLOW_NONE.  It knows nothing of linear probing, displacement or
backward-shift deletion: whatever the library does with its slots, its answers
must be these.

siphash24 is SipHash-2-4 written out from its specification; tuple40 the 40
bytes the receive transform hashes (oracle/rx_oracle.c:384-394).

fixture_frames() builds, with framegen's header builders, about 200 frames
whose tuples are known by construction: IPv4 and IPv6 TCP and UDP flows with
and without a VLAN tag, several frames per flow and both directions of some,
ICMP, a first fragment and its follow-up, IPv6 behind one hop-by-hop header, a
TCP segment too short for its header, and malformed, runt and non-IP frames.
fixture_flows() picks the flows the fixture table holds.
"""
import errno
import struct

import numpy as np

import framegen
from pptk_amd.records import (F_MALFORMED, F_PARSED, FLOW_KEY_DTYPE, FLOW_NONE, FLOW_ST_HIT,
                              FLOW_ST_SUBJECT)

KEY = bytes(range(1, 17))
SLOTS = 64
NFLOWS = 24
M64 = (1 << 64) - 1


# ------------------------------------------------------------------- hashing
def _rotl(x, b):
    return ((x << b) | (x >> (64 - b))) & M64


def siphash24(key, data):
    """SipHash-2-4 of `data` under the 16-byte `key` (64-bit result)."""
    k0, k1 = struct.unpack("<QQ", bytes(key))
    v = [k0 ^ 0x736F6D6570736575, k1 ^ 0x646F72616E646F6D,
         k0 ^ 0x6C7967656E657261, k1 ^ 0x7465646279746573]

    def rounds(n):
        for _ in range(n):
            v[0] = (v[0] + v[1]) & M64
            v[1] = _rotl(v[1], 13) ^ v[0]
            v[0] = _rotl(v[0], 32)
            v[2] = (v[2] + v[3]) & M64
            v[3] = _rotl(v[3], 16) ^ v[2]
            v[0] = (v[0] + v[3]) & M64
            v[3] = _rotl(v[3], 21) ^ v[0]
            v[2] = (v[2] + v[1]) & M64
            v[1] = _rotl(v[1], 17) ^ v[2]
            v[2] = _rotl(v[2], 32)

    data = bytes(data)
    tail = len(data) % 8
    for (m,) in struct.iter_unpack("<Q", data[:len(data) - tail]):
        v[3] ^= m
        rounds(2)
        v[0] ^= m
    m = int.from_bytes(data[len(data) - tail:], "little") | ((len(data) & 0xFF) << 56)
    v[3] ^= m
    rounds(2)
    v[0] ^= m
    v[2] ^= 0xFF
    rounds(4)
    return v[0] ^ v[1] ^ v[2] ^ v[3]


def pad16(addr):
    """An address as the record holds it: 16 bytes, IPv4 in bytes 0..3."""
    return bytes(addr) + bytes(16 - len(addr))


def tuple40(src, dst, sport, dport, proto):
    return pad16(src) + pad16(dst) + struct.pack(">HHB", sport, dport, proto) + bytes(3)


def flow_key(src, dst, sport, dport, proto):
    """One struct pptk_flow_key (records.FLOW_KEY_DTYPE)."""
    k = np.zeros(1, FLOW_KEY_DTYPE)
    k["src"], k["dst"] = list(pad16(src)), list(pad16(dst))
    k["sport"], k["dport"], k["proto"] = sport, dport, proto
    return k[0]


def flow_hash(tup, key=KEY):
    return siphash24(key, tuple40(*tup))


def keys_of_records(recs):
    """The FLOW_KEY_DTYPE array of a record array (every record, subject or
    not) and the subject mask of the lookup rule without d_subject."""
    k = np.zeros(len(recs), FLOW_KEY_DTYPE)
    for f in ("src", "dst", "sport", "dport", "proto"):
        k[f] = recs[f]
    return k, (recs["flags"] & (F_PARSED | F_MALFORMED)) == F_PARSED


# --------------------------------------------------------------------- model
class Model:
    """The table as the reference builds it: buckets of candidates."""

    def __init__(self, slots):
        if slots < 16 or slots > 1 << 26 or slots & (slots - 1):
            raise ValueError("slots")
        self.slots = slots
        self.buckets = {}
        self.count = 0

    @staticmethod
    def _key(key):
        b = key.tobytes() if hasattr(key, "tobytes") else bytes(key)
        assert len(b) == 40
        return b[:37], b[37:] == bytes(3)

    def _bucket(self, h):
        return self.buckets.setdefault((h & 0xFFFFFFFF) & (self.slots - 1), [])

    def _cand(self, k37, h):
        for e in self._bucket(h):
            if e[0] == h and e[1] == k37:
                return e
        return None

    def insert(self, key, h, value):
        k37, ok = self._key(key)
        if not ok or value == FLOW_NONE:
            return -errno.EINVAL
        if self._cand(k37, h) is not None:
            return -errno.EEXIST
        if self.count >= self.slots // 2:
            return -errno.ENOSPC
        self._bucket(h).append([h, k37, value])
        self.count += 1
        return 0

    def update(self, key, h, value):
        k37, ok = self._key(key)
        if not ok or value == FLOW_NONE:
            return -errno.EINVAL
        e = self._cand(k37, h)
        if e is None:
            return -errno.ENOENT
        e[2] = value
        return 0

    def delete(self, key, h):
        k37, ok = self._key(key)
        if not ok:
            return -errno.EINVAL
        e = self._cand(k37, h)
        if e is None:
            return -errno.ENOENT
        self._bucket(h).remove(e)
        self.count -= 1
        return 0

    def find(self, key, h):
        k37, ok = self._key(key)
        assert ok
        e = self._cand(k37, h)
        return None if e is None else e[2]

    def clear(self):
        self.buckets = {}
        self.count = 0

    def lookup(self, keys, hashes, subject):
        """(idx uint32, status uint8) of the lookup rule for the subjects."""
        n = len(keys)
        idx = np.full(n, FLOW_NONE, np.uint32)
        st = np.zeros(n, np.uint8)
        kb = np.ascontiguousarray(keys).view(np.uint8).reshape(n, 40)
        for i in range(n):
            if not subject[i]:
                continue
            st[i] = FLOW_ST_SUBJECT
            e = self._cand(kb[i, :37].tobytes(), int(hashes[i]))
            if e is not None:
                idx[i] = e[2]
                st[i] |= FLOW_ST_HIT
        return idx, st

    def lookup_recs(self, recs, subject=None):
        keys, sub = keys_of_records(recs)
        if subject is not None:
            sub = sub & (np.asarray(subject) != 0)
        return self.lookup(keys, recs["flow_hash"], sub)

    def max_bucket(self):
        return max((len(b) for b in self.buckets.values()), default=0)


def linear_probe_limit(slots, hashes):
    """1 + the largest displacement when entries with these hashes are put,
    in this order and with nothing deleted, into the first free slot at or
    after hash & (slots - 1) -- the bound a test may assert about a table
    built that way (0 for none)."""
    used = np.zeros(slots, bool)
    worst = 0
    for h in hashes:
        d = 0
        s = (int(h) & 0xFFFFFFFF) & (slots - 1)
        while used[s]:
            s = (s + 1) & (slots - 1)
            d += 1
        used[s] = True
        worst = max(worst, d + 1)
    return worst


# ---------------------------------------------------- forged keys and records
def rand_key(rng):
    """A random struct pptk_flow_key (every byte of the 37 in use)."""
    k = np.zeros(1, FLOW_KEY_DTYPE)
    k["src"], k["dst"] = rng.integers(0, 256, 16), rng.integers(0, 256, 16)
    k["sport"], k["dport"] = rng.integers(0, 65536, 2)
    k["proto"] = rng.integers(0, 256)
    return k[0]


def forged_cases(rng):
    """(keys, hashes, values) to insert and (keys, hashes, expected value or
    None) to look up: two keys under one 64-bit hash, and for each of the 37
    key bytes a key that differs from an inserted one in that byte only,
    under the same hash."""
    a, b, base = rand_key(rng), rand_key(rng), rand_key(rng)
    h2, hb = 0xDEADBEEFCAFEF00D, 0x0F1E2D3C4B5A6978
    ins = [(a, h2, 11), (b, h2, 0xFFFFFFFE), (base, hb, 0)]
    look = [(a, h2, 11), (b, h2, 0xFFFFFFFE), (base, hb, 0), (a, hb, None), (base, h2, None),
            (base, hb ^ (1 << 63), None), (base, hb ^ (1 << 32), None)]
    for pos in range(37):
        raw = bytearray(base.tobytes())
        raw[pos] ^= 1 << (pos % 8)
        look.append((np.frombuffer(bytes(raw), FLOW_KEY_DTYPE)[0], hb, None))
    return ins, look


def records_of(keys, hashes, flags=F_PARSED):
    """Receive records (records.REC_DTYPE) that carry these keys and hashes;
    flags: one value or one per record."""
    from pptk_amd.records import REC_DTYPE
    keys = np.asarray(keys, FLOW_KEY_DTYPE).reshape(-1)
    r = np.zeros(len(keys), REC_DTYPE)
    for f in ("src", "dst", "sport", "dport", "proto"):
        r[f] = keys[f]
    r["flow_hash"] = np.asarray(hashes, np.uint64)
    r["flags"] = flags
    return r


# -------------------------------------------------------------------- frames
def _ip4(src, dst, proto, l4, vlan=None, mf=False, frag_off=0, ident=7):
    ip = framegen.ipv4_hdr(src, dst, proto, len(l4), df=False, mf=mf, frag_off=frag_off,
                           ident=ident)
    return framegen.eth(framegen.ETH_IP, vlan) + ip + l4


def _ip6(src, dst, nexthdr, body, vlan=None):
    return framegen.eth(framegen.ETH_IP6, vlan) + framegen.ipv6_hdr(src, dst, nexthdr,
                                                                    len(body)) + body


def _l4(rng, proto, sport, dport, pseudo, src, dst, n):
    payload = bytes(rng.integers(0, 256, n, dtype=np.uint8))
    if proto == 6:
        seg = framegen.tcp_hdr(sport, dport, int(rng.integers(0, 2**32)), 1) + payload
    else:
        seg = framegen.udp_hdr(sport, dport, 8 + n) + payload
    return framegen.fill_l4(seg, proto, pseudo(src, dst, proto, len(seg)))


def frame_of(rng, tup, vlan=None, n=None):
    """A TCP or UDP frame of the tuple (4- or 16-byte addresses)."""
    src, dst, sport, dport, proto = tup
    n = int(rng.integers(0, 40)) if n is None else n
    if len(src) == 4:
        return _ip4(src, dst, proto, _l4(rng, proto, sport, dport, framegen.pseudo4, src, dst, n),
                    vlan)
    return _ip6(src, dst, proto, _l4(rng, proto, sport, dport, framegen.pseudo6, src, dst, n), vlan)


def reverse(tup):
    src, dst, sport, dport, proto = tup
    return dst, src, dport, sport, proto


def base_flows():
    """The TCP / UDP tuples of the fixture, IPv4 then IPv6."""
    rng = np.random.default_rng(0xF10)
    out = []
    for i in range(26):
        out.append((bytes([10, 0, i // 8, 1 + i]), bytes([192, 168, 1 + i % 5, 200 - i]),
                    int(rng.integers(1024, 65536)), (80, 443, 53, 8080)[i % 4], (6, 17)[i % 2]))
    for i in range(12):
        src = bytes([0x20, 0x01, 0x0D, 0xB8]) + bytes(rng.integers(0, 256, 12, dtype=np.uint8))
        dst = bytes([0xFD]) + bytes(rng.integers(0, 256, 15, dtype=np.uint8))
        out.append((src, dst, int(rng.integers(1024, 65536)), (443, 53)[i % 2], (6, 17)[i % 2]))
    return out


def fixture_frames():
    """[(frame bytes, tuple or None)]: the tuple of the key a lookup uses, None
    for a frame that is no subject (malformed, runt, not IP)."""
    rng = np.random.default_rng(0xF70)
    out = []
    flows = base_flows()
    for j, t in enumerate(flows):
        for r in range(3 + j % 3):                  # several frames per flow
            out.append((frame_of(rng, t, vlan=(100 + j) if (j + r) % 3 == 0 else None), t))
        if j % 2 == 0:                              # the other direction of every second flow
            out.append((frame_of(rng, reverse(t)), reverse(t)))
            out.append((frame_of(rng, reverse(t), vlan=9), reverse(t)))
    # ICMP: ports 0, proto 1
    for i in range(6):
        src, dst = bytes([10, 9, 0, i]), bytes([192, 168, 9, 9])
        msg = bytearray(struct.pack(">BBHHH", 8 if i % 2 else 0, 0, 0, 0x1234 + i, i) + bytes(8 * i))
        struct.pack_into(">H", msg, 2, framegen.csum(bytes(msg)))
        out.append((_ip4(src, dst, 1, bytes(msg), vlan=5 if i == 3 else None), (src, dst, 0, 0, 1)))
    # a first fragment and its follow-up: no L4 header is read from either
    t = flows[0]
    seg = _l4(rng, 6, t[2], t[3], framegen.pseudo4, t[0], t[1], 44)
    out.append((_ip4(t[0], t[1], 6, seg[:40], mf=True, ident=99), (t[0], t[1], 0, 0, 6)))
    out.append((_ip4(t[0], t[1], 6, seg[40:], frag_off=5, ident=99), (t[0], t[1], 0, 0, 6)))
    # IPv6 behind one hop-by-hop header: the final next header and its ports
    for t in flows[26:29]:
        seg = _l4(rng, t[4], t[2], t[3], framegen.pseudo6, t[0], t[1], 12)
        h = bytearray(framegen.hbh(1))
        h[0] = t[4]
        out.append((_ip6(t[0], t[1], 0, bytes(h) + seg, vlan=None), t))
    # a TCP segment of 12 bytes: parsed, but no L4 header, so ports 0
    src, dst = bytes([10, 7, 7, 7]), bytes([192, 168, 7, 7])
    out.append((_ip4(src, dst, 6, bytes(rng.integers(0, 256, 12, dtype=np.uint8))),
                (src, dst, 0, 0, 6)))
    # malformed: total length past the frame, IHL below 5, IPv6 payload past the frame
    good = frame_of(rng, flows[1], n=30)
    out.append((good[:-9], None))
    bad = bytearray(frame_of(rng, flows[2], n=8))
    bad[14] = 0x44
    out.append((bytes(bad), None))
    out.append((frame_of(rng, flows[27], n=30)[:-5], None))
    # runts and non-IP
    out.append((good[:10], None))
    out.append((good[:14], None))
    out.append((good[:33], None))
    out.append((b"", None))
    out.append((framegen.eth(0x0806) + bytes(rng.integers(0, 256, 28, dtype=np.uint8)), None))
    out.append((framegen.eth(0x88CC, vlan=3) + bytes(rng.integers(0, 256, 50, dtype=np.uint8)),
                None))
    return out


def fixture_tuples():
    """The distinct tuples of the fixture's subjects, in order of appearance."""
    seen, out = set(), []
    for _, t in fixture_frames():
        if t is not None and t not in seen:
            seen.add(t)
            out.append(t)
    return out


def fixture_flows():
    """[(tuple, value)]: the NFLOWS flows the fixture table holds -- first the
    tuples that share a home slot at SLOTS slots with an earlier one (each
    with that partner), then the rest in order of appearance.  The values
    include 0 and 0xfffffffe."""
    tuples = fixture_tuples()
    home = {}
    for t in tuples:
        home.setdefault(flow_hash(t) & (SLOTS - 1), []).append(t)
    picked = []
    for t in tuples:   # colliding groups first, four of them
        g = home[flow_hash(t) & (SLOTS - 1)]
        if len(g) >= 2 and t == g[0] and len(picked) < 8:
            picked += g[:2]
    for t in tuples:
        if len(picked) < NFLOWS and t not in picked:
            picked.append(t)
    values = [0, 0xFFFFFFFE] + [(0x9E3779B1 * (j + 1)) & 0x7FFFFFFF for j in range(2, NFLOWS)]
    return list(zip(picked, values))


def shared_home_pairs(flows, slots=SLOTS):
    homes = [flow_hash(t) & (slots - 1) for t, _ in flows]
    return sum(homes.count(h) * (homes.count(h) - 1) // 2 for h in set(homes))


def fixture():
    """Everything tests/golden/flow.npz holds, computed by this module alone
    (keys, hashes and the lookup answer from the model)."""
    ff = fixture_frames()
    frames = [f for f, _ in ff]
    n = len(frames)
    buf, off, lens = framegen.pack(frames)
    keys = np.zeros(n, FLOW_KEY_DTYPE)
    hashes = np.zeros(n, np.uint64)
    subject = np.zeros(n, np.uint8)
    for i, (_, t) in enumerate(ff):
        if t is not None:
            keys[i], hashes[i], subject[i] = flow_key(*t), flow_hash(t), 1
    flows = fixture_flows()
    m = Model(SLOTS)
    fk = np.zeros(len(flows), FLOW_KEY_DTYPE)
    fh = np.zeros(len(flows), np.uint64)
    fv = np.zeros(len(flows), np.uint32)
    for j, (t, v) in enumerate(flows):
        fk[j], fh[j], fv[j] = flow_key(*t), flow_hash(t), v
        assert m.insert(fk[j], int(fh[j]), v) == 0
    idx, status = m.lookup(keys, hashes, subject)
    return dict(frames=buf, off=off, len=lens, keys=keys.view(np.uint8).reshape(n, 40),
                hashes=hashes, subject=subject, flow_keys=fk.view(np.uint8).reshape(-1, 40),
                flow_hashes=fh, flow_values=fv, idx=idx, status=status,
                slots=np.array([SLOTS], np.uint32), key=np.frombuffer(KEY, np.uint8))
