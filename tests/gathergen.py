"""The yardstick of egress gather (include/pptk_rx.h "Egress gather") and the
batches its tests run.

expected() is a NumPy model of the contract that shares no code with either C
implementation: the considered entries, their slots, the offsets by cumsum per
run, the bytes by slicing.  replay_regions() is the reference's per-port copy
loop (ldp_out_inject, ldp/ldpnetmap.c:68: one memcpy of every packet of the
port's output table into the next tx slot) taken literally over Python lists.

Case holds the inputs of one call.  Outputs is the set of output arrays of one
call between sentinels of 0xA5 bytes -- PAD entries before and after pk_off,
pk_len, ports and hdr, GUARD bytes before `out` and behind out_cap -- so that
"nothing else is written" is one whole-buffer comparison.  host_call() fills
one through pptk_tx_gather_host; arguments() builds struct pptk_gather from
addresses, for host and device memory alike.
"""
import ctypes

import numpy as np

from pptk_amd.records import (DISPATCH_PORT_DTYPE, GATHER_HDR_DTYPE, GATHER_PORT_DTYPE,
                              GATHER_ST_BADRUNS)
from pptk_amd.rx import Gather

PAD = 2
SENT = 0xA5
GUARD = 256          # sentinel bytes before out and behind out_cap
LENGTHS = (0, 1, 15, 16, 17, 60, 64, 1500, 1514, 9000, 65535)
INPUTS = ("frames", "off", "lens", "list", "runs", "d_entries")
DTYPES = dict(frames=np.uint8, off=np.uint64, lens=np.uint16, list=np.uint32,
              runs=DISPATCH_PORT_DTYPE, d_entries=np.uint64)


class Case:
    """The inputs of one call: NumPy arrays or None, and the scalars."""

    def __init__(self, frames, n, off=None, lens=None, stride=0, fixed_len=0, list=None,
                 max_entries=None, d_entries=None, runs=None, nports=1):
        self.n, self.stride, self.fixed_len, self.nports = n, stride, fixed_len, nports
        if runs is not None and getattr(runs, "dtype", None) != DISPATCH_PORT_DTYPE:
            runs = make_runs(runs)
        if d_entries is not None:
            d_entries = [d_entries]
        for name, a in zip(INPUTS, (frames, off, lens, list, runs, d_entries)):
            setattr(self, name, None if a is None else np.ascontiguousarray(a, dtype=DTYPES[name]))
        if max_entries is None:
            max_entries = n if self.list is None else len(self.list)
        self.max_entries = max_entries

    def addresses(self):
        return {k: None if getattr(self, k) is None else getattr(self, k).ctypes.data
                for k in INPUTS}


def make_runs(counts, first=0):
    """Dispatch port entries with these counts, back to back from `first`;
    bytes and flooded hold junk (the gather does not read them)."""
    r = np.zeros(len(counts), DISPATCH_PORT_DTYPE)
    r["count"] = counts
    r["start"] = first + np.cumsum(r["count"]) - r["count"]
    r["bytes"], r["flooded"] = 0xDEAD, 0xBEEF
    return r


class Outputs:
    """Sentinel-framed output arrays of a call."""

    ARRAYS = ("out", "pk_off", "pk_len", "ports", "hdr")

    def __init__(self, max_entries, nports, out_cap, pad=PAD):
        self.max_entries, self.nports, self.out_cap, self.pad = max_entries, nports, out_cap, pad
        rows = max_entries + 2 * pad
        # out lies 256-byte aligned inside a larger block; `out` is the view
        # GUARD + out_cap + GUARD around it
        self._raw = np.full(out_cap + 2 * GUARD + 256, SENT, np.uint8)
        shift = -(self._raw.ctypes.data + GUARD) % 256
        self.out = self._raw[shift:shift + out_cap + 2 * GUARD]
        self.pk_off = np.frombuffer(bytes([SENT]) * (8 * rows), np.uint64).copy()
        self.pk_len = np.frombuffer(bytes([SENT]) * (2 * rows), np.uint16).copy()
        self.ports = np.full(32 * (nports + 2 * pad), SENT, np.uint8)
        self.hdr = np.full(3 * 64, SENT, np.uint8)

    def offsets(self):
        """Byte offset of entry 0 of each array within its buffer."""
        p = self.pad
        return dict(out=GUARD, pk_off=8 * p, pk_len=2 * p, ports=32 * p, hdr=64)

    def addresses(self):
        return {k: getattr(self, k).ctypes.data + o for k, o in self.offsets().items()}

    def header(self):
        return self.hdr[64:128].view(GATHER_HDR_DTYPE)[0]

    def port_entries(self):
        p = self.pad
        return self.ports[32 * p:32 * (p + self.nports)].view(GATHER_PORT_DTYPE)

    def packed_bytes(self):
        return self.out[GUARD:GUARD + self.out_cap]

    def considered(self):
        """(pk_off, pk_len) cut to hdr.entries."""
        e, p = int(self.header()["entries"]), self.pad
        return self.pk_off[p:p + e], self.pk_len[p:p + e]

    def same(self, other):
        return all(np.array_equal(getattr(self, k), getattr(other, k)) for k in self.ARRAYS)

    def differing(self, other):
        return [k for k in self.ARRAYS if not np.array_equal(getattr(self, k), getattr(other, k))]

    def untouched(self, names=("out", "pk_off", "pk_len")):
        return all((getattr(self, k).view(np.uint8) == SENT).all() for k in names)


# --------------------------------------------------------------------- model
def entry_lengths(c, idx):
    """The frame length of each entry (0 for a bad one) and which are bad."""
    idx = idx.astype(np.int64)
    ok = idx < c.n
    safe = np.where(ok, idx, 0)
    if c.n == 0:
        return np.zeros(len(idx), np.int64), ~ok
    L = c.lens[safe].astype(np.int64) if c.lens is not None else np.full(len(idx), c.fixed_len, np.int64)
    return np.where(ok, L, 0), ~ok


def expected(c, out_cap, pk_off=True, pk_len=True):
    """The Outputs the contract asks of a call."""
    o = Outputs(c.max_entries, c.nports, out_cap)
    pe, h = o.port_entries(), o.hdr[64:128].view(GATHER_HDR_DTYPE)
    pe[:] = 0
    h[:] = 0
    if c.max_entries == 0:
        return o
    E = c.max_entries if c.d_entries is None else min(c.max_entries, int(c.d_entries[0]))
    if c.runs is not None:
        at = 0
        for s, k in zip(c.runs["start"].tolist(), c.runs["count"].tolist()):
            if s != at or s + k >= 1 << 64:
                h["status"] = GATHER_ST_BADRUNS
                return o
            at = s + k
        E = min(E, at)
        first = [min(int(s), E) for s in c.runs["start"]] + [E]
    else:
        first = [0, E]
    idx = c.list[:E] if c.list is not None else np.arange(E)
    L, bad = entry_lengths(c, idx)
    slot = (L + 15) // 16 * 16
    start, offs = 0, np.zeros(E, np.int64)
    for p in range(c.nports):
        a, b = first[p], first[p + 1]
        offs[a:b] = start + np.cumsum(slot[a:b]) - slot[a:b]
        pe[p]["start"], pe[p]["entries"] = start, b - a
        need = start + int(slot[a:b].sum())
        start = (need + 255) // 256 * 256
    packed = offs + slot <= out_cap
    npk = int(packed.sum())
    assert packed[:npk].all()                       # a prefix
    for p in range(c.nports):
        a, b = first[p], first[p + 1]
        pe[p]["packed"], pe[p]["bytes"] = packed[a:b].sum(), slot[a:b][packed[a:b]].sum()
    h["entries"], h["packed"], h["need"], h["bytes"] = E, npk, need, pe["bytes"].sum()
    h["frame_bytes"], h["bad"] = L[:npk].sum(), bad.sum()
    if pk_off:
        o.pk_off[o.pad:o.pad + E] = offs
    if pk_len:
        o.pk_len[o.pad:o.pad + E] = L
    body = o.packed_bytes()
    for g in range(npk):
        if L[g]:
            i = int(idx[g])
            base = int(c.off[i]) if c.off is not None else i * c.stride
            body[offs[g]:offs[g] + L[g]] = c.frames[base:base + L[g]]
            body[offs[g] + L[g]:offs[g] + slot[g]] = 0
    return o


def replay_regions(c, tables):
    """Per port, the bytes the reference's copy loop leaves in that port's tx
    slots, laid back to back at this library's slot rounding: for each packet
    of pktout_tbl[k] one memcpy of its sz bytes."""
    regions = []
    for tbl in tables:
        buf = bytearray()
        for j in tbl:
            base = int(c.off[j]) if c.off is not None else j * c.stride
            sz = int(c.lens[j]) if c.lens is not None else c.fixed_len
            buf += bytes(c.frames[base:base + sz]) + bytes(-sz % 16)
        regions.append(bytes(buf))
    return regions


def arguments(c, inputs, outputs, out_cap, pk_off=True, pk_len=True):
    """struct pptk_gather of case c from the addresses of its inputs ({name:
    address or None}) and of entry 0 of its outputs."""
    return Gather(frames=inputs["frames"], off=inputs["off"], len=inputs["lens"], stride=c.stride,
                  fixed_len=c.fixed_len, n=c.n, list=inputs["list"], max_entries=c.max_entries,
                  d_entries=inputs["d_entries"], runs=inputs["runs"], nports=c.nports,
                  out=outputs["out"] if out_cap else None, out_cap=out_cap,
                  pk_off=outputs["pk_off"] if pk_off else None,
                  pk_len=outputs["pk_len"] if pk_len else None, ports=outputs["ports"],
                  hdr=outputs["hdr"])


def host_call(L, c, out_cap, pk_off=True, pk_len=True):
    """pptk_tx_gather_host into fresh Outputs: (rc, Outputs)."""
    o = Outputs(c.max_entries, c.nports, out_cap)
    g = arguments(c, c.addresses(), o.addresses(), out_cap, pk_off, pk_len)
    return L.pptk_tx_gather_host(ctypes.byref(g)), o


# ------------------------------------------------------------------ builders
def batch(lengths, rng, form="off", phases=None):
    """A source batch of frames with these lengths, random bytes: form "off"
    (offset-described, frame i at byte phase phases[i] or a random one, junk
    between the frames), "stride" (lens array, one stride) or "fixed" (one
    length, lengths[0]).  Returns dict(frames, n, off / lens / stride /
    fixed_len)."""
    lengths = np.asarray(lengths, np.int64)
    n = len(lengths)
    if form == "fixed":
        assert (lengths == lengths[0]).all()
        stride = int(lengths[0]) + int(rng.integers(0, 40))
        stride = max(stride, 1)
        frames = rng.integers(0, 256, n * stride + 16, dtype=np.uint8)
        return dict(frames=frames, n=n, stride=stride, fixed_len=int(lengths[0]))
    if form == "stride":
        stride = int(lengths.max()) + 7 if n else 8
        frames = rng.integers(0, 256, n * stride + 16, dtype=np.uint8)
        return dict(frames=frames, n=n, stride=stride, lens=lengths.astype(np.uint16))
    off, at = np.zeros(n, np.uint64), 0
    for i, ln in enumerate(lengths.tolist()):
        ph = int(phases[i]) if phases is not None else int(rng.integers(0, 16))
        at = (at + 15) // 16 * 16 + ph
        off[i] = at
        at += ln
    frames = rng.integers(0, 256, at + 32, dtype=np.uint8)
    return dict(frames=frames, n=n, off=off, lens=lengths.astype(np.uint16))


def mixed_lengths(n, rng, top=1600):
    """n lengths: the edge lengths that fit below `top` first, then random."""
    edge = [x for x in LENGTHS if x <= top]
    a = rng.integers(0, top + 1, n)
    a[:min(n, len(edge))] = edge[:n]
    return rng.permutation(a)


def entry_list(kind, n, count, rng):
    """An entry list over n frames: "permuted", "flood" (repeats) or "bad"
    (indices at and above n in between)."""
    if kind == "permuted":
        return rng.permutation(n)[:count].astype(np.uint32) if count <= n else \
            rng.integers(0, n, count).astype(np.uint32)
    a = rng.integers(0, max(n, 1), count).astype(np.uint32)
    if kind == "flood":
        a[1::3] = a[0::3][:len(a[1::3])]
        return a
    assert kind == "bad", kind
    k = rng.random(count) < 0.2
    a[k] = rng.choice(np.array([n, n + 1, 0x7FFFFFFF, 0xFFFFFFFF], np.uint32), int(k.sum()))
    return a


def split_runs(total, nports, rng, empty=True):
    """Counts of nports runs that add up to `total`, some empty."""
    cuts = np.sort(rng.integers(0, total + 1, nports - 1))
    counts = np.diff(np.concatenate([[0], cuts, [total]]))
    if empty and nports > 2:
        counts[1] += counts[0]
        counts[0] = 0
    return counts.astype(np.uint64)
