"""The independent model of flow learning (include/pptk_rx.h "Flow
learning") and the batches its tests run.

model() is the contract as a Python dict: candidates are the frames whose
status byte is exactly FLOW_ST_SUBJECT, the first max_candidates of them are
considered, a dict from flow_hash to the first considered frame that carried
it decides leader / repeat / collision.  It knows nothing of open addressing,
blocks, scans or scratch.

Outputs is the set of output arrays of one call between sentinel entries --
PAD entries of 0xA5 bytes before and after each array, and `cap` such entries
inside -- so that "entries at and past written are untouched and nothing is
written outside the arrays" is one whole-buffer comparison.  expected() fills
one from the model; host_call() fills one through pptk_flow_learn_host.

The builders return (recs, status): records.REC_DTYPE records made with
flowgen.records_of from flowgen.rand_key keys, their hashes SipHash-2-4 of the
tuple (flowgen.flow_hash) unless forged, every other record field random per
frame so that "the leader's record, verbatim" is told from any other frame of
its flow.
"""
import numpy as np

import flowgen
from pptk_amd.records import FLOW_LEARN_HDR_DTYPE, FLOW_ST_HIT, FLOW_ST_SUBJECT, REC_DTYPE

PAD = 2
SENT = 0xA5
SENT32 = 0xA5A5A5A5
M64 = (1 << 64) - 1
NOISE_FIELDS = ("ip_cksum", "l4_cksum", "l4_off", "l4_len", "src_bucket")


# --------------------------------------------------------------------- model
def model(recs, status, max_candidates):
    """(hdr dict without `written`, [[leader frame, packets], ...])."""
    rb = np.ascontiguousarray(recs).view(np.uint8).reshape(-1, 64)
    cand = np.nonzero(np.asarray(status) == FLOW_ST_SUBJECT)[0]
    seen, entries = {}, []
    for i in cand[:max_candidates]:
        i = int(i)
        key = rb[i, 8:44].tobytes() + rb[i, 53:54].tobytes()
        e = seen.get(int(recs["flow_hash"][i]))
        if e is None:
            ent = [i, 1]
            entries.append(ent)
            seen[int(recs["flow_hash"][i])] = (key, ent)
        elif e[0] == key:
            e[1][1] += 1
        else:
            entries.append([i, 1])        # another key under a known hash: alone, not in the dict
    return dict(candidates=len(cand), considered=min(len(cand), max_candidates),
                flows=len(entries)), entries


class Outputs:
    """Sentinel-framed output arrays for a call with this cap."""

    def __init__(self, cap, pad=PAD):
        self.cap, self.pad = cap, pad
        rows = cap + 2 * pad
        self.new = aligned_bytes(rows * 64)
        self.new[:] = SENT
        self.first = np.full(rows, SENT32, np.uint32)
        self.packets = np.full(rows, SENT32, np.uint32)
        self.hdr = aligned_bytes(3 * 32)
        self.hdr[:] = SENT

    def pointers(self):
        """Addresses of entry 0 of new_recs, first, packets and of the header."""
        p = self.pad
        return (self.new.ctypes.data + 64 * p, self.first.ctypes.data + 4 * p,
                self.packets.ctypes.data + 4 * p, self.hdr.ctypes.data + 32)

    def header(self):
        return self.hdr[32:64].view(FLOW_LEARN_HDR_DTYPE)[0]

    def written(self):
        """(records, first, packets) cut to hdr.written."""
        w, p = int(self.header()["written"]), self.pad
        return (self.new[64 * p:64 * (p + w)].view(REC_DTYPE), self.first[p:p + w],
                self.packets[p:p + w])

    def same(self, other, first=True, packets=True):
        return (np.array_equal(self.new, other.new) and np.array_equal(self.hdr, other.hdr)
                and (not first or np.array_equal(self.first, other.first))
                and (not packets or np.array_equal(self.packets, other.packets)))

    def untouched(self, first=True, packets=True, hdr=False):
        """The arrays named hold sentinels only."""
        return ((self.new == SENT).all() and (not first or (self.first == SENT32).all())
                and (not packets or (self.packets == SENT32).all())
                and (not hdr or (self.hdr == SENT).all()))


def aligned_bytes(nbytes, align=64):
    raw = np.zeros(nbytes + align, np.uint8)
    skip = -raw.ctypes.data & (align - 1)
    return raw[skip:skip + nbytes]


def expected(recs, status, max_candidates, cap, first=True, packets=True):
    """The Outputs the contract asks of a call, from the model."""
    hdr, entries = model(recs, status, max_candidates)
    o = Outputs(cap)
    rb = np.ascontiguousarray(recs).view(np.uint8).reshape(-1, 64)
    p = o.pad
    for k, (frame, count) in enumerate(entries[:cap]):
        o.new[64 * (p + k):64 * (p + k + 1)] = rb[frame]
        if first:
            o.first[p + k] = frame
        if packets:
            o.packets[p + k] = count
    h = o.hdr[32:64].view(FLOW_LEARN_HDR_DTYPE)
    h["candidates"], h["considered"], h["flows"] = hdr["candidates"], hdr["considered"], hdr["flows"]
    h["written"] = min(hdr["flows"], cap)
    return o


def aligned_records(recs):
    """The records' bytes at a 16-byte aligned address (their own where it is one)."""
    raw = np.ascontiguousarray(recs).view(np.uint8).reshape(-1)
    if raw.size and raw.ctypes.data % 16 == 0:
        return raw
    a = aligned_bytes(max(raw.size, 64))
    a[:raw.size] = raw
    return a[:raw.size]


def host_call(L, recs, status, max_candidates, cap, first=True, packets=True, null_new=False):
    """pptk_flow_learn_host into fresh Outputs: (rc, Outputs)."""
    r = aligned_records(recs)
    st = np.ascontiguousarray(status, dtype=np.uint8)
    o = Outputs(cap)
    pn, pf, pp, ph = o.pointers()
    rc = L.pptk_flow_learn_host(r.ctypes.data, st.ctypes.data, len(st), max_candidates,
                                None if null_new else pn, pf if first else None,
                                pp if packets else None, cap, ph)
    return rc, o


# ------------------------------------------------------------------ builders
def hash_of_key(k):
    return flowgen.flow_hash((bytes(k["src"]), bytes(k["dst"]), int(k["sport"]), int(k["dport"]),
                              int(k["proto"])))


def flows(count, rng):
    """(keys, SipHash hashes) of `count` random flows."""
    keys = np.array([flowgen.rand_key(rng) for _ in range(count)])
    return keys, np.array([hash_of_key(k) for k in keys], np.uint64)


def frames_of(keys, hashes, pick, rng):
    """One record per entry of `pick` (flow numbers), noise in the other fields."""
    pick = np.asarray(pick, np.int64)
    r = flowgen.records_of(keys[pick], np.asarray(hashes, np.uint64)[pick])
    for f in NOISE_FIELDS:
        r[f] = rng.integers(0, 1 << (8 * r.dtype[f].itemsize), len(r), dtype=np.uint64)
    return r


def other_status(count, rng):
    """Status bytes that are no candidates: non-subjects, hits, and values the
    lookup never writes but `== SUBJECT exactly` must reject."""
    return rng.choice(np.array([0, FLOW_ST_SUBJECT | FLOW_ST_HIT, FLOW_ST_HIT, 0x81, 0xFF, 5],
                               np.uint8), count, p=[0.4, 0.5, 0.025, 0.025, 0.025, 0.025])


def mix(n, nflows, share, rng, keys=None, hashes=None):
    """n frames over nflows flows, about `share` of them candidates, the rest
    non-subjects and hits in between."""
    if keys is None:
        keys, hashes = flows(nflows, rng)
    recs = frames_of(keys, hashes, rng.integers(0, len(keys), n), rng)
    status = other_status(n, rng)
    status[rng.random(n) < share] = FLOW_ST_SUBJECT
    return recs, status


def one_flow(n, rng):
    keys, hashes = flows(1, rng)
    return frames_of(keys, hashes, np.zeros(n, np.int64), rng), np.full(n, FLOW_ST_SUBJECT, np.uint8)


def all_distinct(n, rng):
    """n candidates of n flows (random 64-bit hashes: the table never hashes)."""
    keys = np.array([flowgen.rand_key(rng) for _ in range(n)])
    hashes = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    assert np.unique(hashes).size == n
    return frames_of(keys, hashes, np.arange(n), rng), np.full(n, FLOW_ST_SUBJECT, np.uint8)


def no_candidates(n, rng):
    recs, _ = mix(n, 20, 0.0, rng)
    return recs, other_status(n, rng)


def edge_hashes(rng, repeats=5):
    """Flows forged under flow_hash 0 and 2^64 - 1 (two keys under each, so
    both also collide), among ordinary ones, each flow `repeats` times."""
    keys, hashes = flows(8, rng)
    hashes[0] = hashes[1] = 0
    hashes[2] = hashes[3] = M64
    pick = rng.permutation(np.repeat(np.arange(8), repeats))
    return frames_of(keys, hashes, pick, rng), np.full(len(pick), FLOW_ST_SUBJECT, np.uint8)


def three_under_one_hash(rng, repeats=4):
    """Keys A, B, C under one forged hash, interleaved with repeats of each,
    plus two ordinary flows."""
    keys, hashes = flows(5, rng)
    hashes[:3] = 0x1234567890ABCDEF
    pick = np.concatenate([[1, 0, 2], rng.permutation(np.repeat(np.arange(5), repeats))])
    return frames_of(keys, hashes, pick, rng), np.full(len(pick), FLOW_ST_SUBJECT, np.uint8)


def cluster(count, rng, repeats=3, low=0xFFFFFFF0):
    """`count` keys whose forged hashes share the low 32 bits -- one probe
    cluster under every mask -- each `repeats` times, shuffled."""
    keys = np.array([flowgen.rand_key(rng) for _ in range(count)])
    hashes = ((np.arange(1, count + 1, dtype=np.uint64) * np.uint64(0x9E3779B1)) << np.uint64(32)) \
        | np.uint64(low)
    assert np.unique(hashes).size == count
    pick = rng.permutation(np.repeat(np.arange(count), repeats))
    return frames_of(keys, hashes, pick, rng), np.full(len(pick), FLOW_ST_SUBJECT, np.uint8)
