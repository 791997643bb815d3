"""The yardstick of egress dispatch (include/pptk_rx.h "Egress dispatch") and
the batches its tests run.

replay() is the tail of the reference's switch loop, ldp/ldpswitch.c:276-318,
taken literally: one Python list per port (pktout_tbl[k]), walked once in
frame order; a frame with a known port is appended to that port's list, a
frame without one (port == -1) to the list of every port k != i, the ingress
port.  What stands where port_get() stands is the contract's classification
of the frame's code.  It shares no code with either C implementation and
knows nothing of counts, prefixes, blocks or scratch.

Case holds the inputs of one call.  Outputs is the set of output arrays of one
call between sentinel entries -- PAD entries of 0xA5 bytes before and after
each array and `cap` such entries inside -- so that "nothing is written
outside the arrays or past written" is one whole-buffer comparison.
expected() fills one from the replay; host_call() fills one through
pptk_tx_dispatch_host; arguments() builds struct pptk_dispatch from addresses,
for host and device memory alike.
"""
import numpy as np

from pptk_amd.records import (DISPATCH_HDR_DTYPE, DISPATCH_PORT_DTYPE, FLOW_NONE, PORT_DROP,
                              PORT_FLOOD, PORT_MAX)
from pptk_amd.rx import Dispatch

PAD = 2
SENT = 0xA5
INPUTS = ("port", "idx", "flow_port", "subject", "in_port", "off", "lens")
DTYPES = dict(port=np.uint8, idx=np.uint32, flow_port=np.uint8, subject=np.uint8,
              in_port=np.uint8, off=np.uint64, lens=np.uint16)


class Case:
    """The inputs of one call: NumPy arrays or None, and the scalars."""

    def __init__(self, nports, port=None, idx=None, flow_port=None, miss_code=PORT_DROP,
                 subject=None, in_port=None, in_port_all=PORT_MAX, off=None, lens=None, stride=0,
                 fixed_len=0):
        self.nports, self.miss_code, self.in_port_all = nports, miss_code, in_port_all
        self.stride, self.fixed_len = stride, fixed_len
        for name, a in zip(INPUTS, (port, idx, flow_port, subject, in_port, off, lens)):
            setattr(self, name, None if a is None else np.ascontiguousarray(a, dtype=DTYPES[name]))
        self.n = len(self.port if self.port is not None else self.idx)
        self.flows = 0 if self.flow_port is None else len(self.flow_port)

    def addresses(self):
        return {k: None if getattr(self, k) is None else getattr(self, k).ctypes.data
                for k in INPUTS}

    def length(self, i):
        return int(self.lens[i]) if self.lens is not None else self.fixed_len

    def offset(self, i):
        return int(self.off[i]) if self.off is not None else i * self.stride


# -------------------------------------------------------------------- replay
def replay(c):
    """(pktout_tbl, classes): the per-port lists of frame indices and the
    frames by class, dict(unicast, flood, dropped, bad, hairpin, floods = the
    set of flood frames)."""
    num_intfs = c.nports
    pktout_tbl = [[] for _ in range(num_intfs)]
    cls = dict(unicast=0, flood=0, dropped=0, bad=0, hairpin=0, floods=set())
    lst = {k: None if getattr(c, k) is None else getattr(c, k).tolist() for k in INPUTS}
    for j in range(c.n):
        i = lst["in_port"][j] if lst["in_port"] is not None else c.in_port_all
        if lst["subject"] is not None and lst["subject"][j] == 0:
            cls["dropped"] += 1
            continue
        if lst["port"] is not None:
            code = lst["port"][j]
        elif lst["idx"][j] == FLOW_NONE:
            code = c.miss_code
        elif lst["idx"][j] >= c.flows:
            cls["bad"] += 1
            continue
        else:
            code = lst["flow_port"][lst["idx"][j]]
        if code == PORT_DROP:
            cls["dropped"] += 1
            continue
        if code != PORT_FLOOD and code >= num_intfs:
            cls["bad"] += 1
            continue
        port = -1 if code == PORT_FLOOD else code
        if port == -1:
            cls["flood"] += 1
            cls["floods"].add(j)
            for k in range(num_intfs):
                if k != i:
                    pktout_tbl[k].append(j)
        else:
            cls["unicast"] += 1
            cls["hairpin"] += port == i
            pktout_tbl[port].append(j)
    return pktout_tbl, cls


class Outputs:
    """Sentinel-framed output arrays of a call with this cap and port count."""

    def __init__(self, cap, nports, pad=PAD):
        self.cap, self.nports, self.pad = cap, nports, pad
        rows = cap + 2 * pad
        self.list = np.frombuffer(bytes([SENT]) * (4 * rows), np.uint32).copy()
        self.out_off = np.frombuffer(bytes([SENT]) * (8 * rows), np.uint64).copy()
        self.out_len = np.frombuffer(bytes([SENT]) * (2 * rows), np.uint16).copy()
        self.ports = np.full(32 * (nports + 2 * pad), SENT, np.uint8)
        self.hdr = np.full(3 * 64, SENT, np.uint8)

    ARRAYS = ("list", "out_off", "out_len", "ports", "hdr")

    def offsets(self):
        """Byte offset of entry 0 of each array within its buffer."""
        p = self.pad
        return dict(list=4 * p, out_off=8 * p, out_len=2 * p, ports=32 * p, hdr=64)

    def addresses(self):
        return {k: getattr(self, k).ctypes.data + o for k, o in self.offsets().items()}

    def header(self):
        return self.hdr[64:128].view(DISPATCH_HDR_DTYPE)[0]

    def port_entries(self):
        p = self.pad
        return self.ports[32 * p:32 * (p + self.nports)].view(DISPATCH_PORT_DTYPE)

    def written(self):
        """(list, out_off, out_len) cut to hdr.written."""
        w, p = int(self.header()["written"]), self.pad
        return self.list[p:p + w], self.out_off[p:p + w], self.out_len[p:p + w]

    def same(self, other):
        return all(np.array_equal(getattr(self, k), getattr(other, k)) for k in self.ARRAYS)

    def differing(self, other):
        return [k for k in self.ARRAYS if not np.array_equal(getattr(self, k), getattr(other, k))]

    def untouched(self, names=("list", "out_off", "out_len")):
        return all((getattr(self, k).view(np.uint8) == SENT).all() for k in names)


def expected(c, cap, out_off=True, out_len=True):
    """The Outputs the contract asks of a call, from the replay."""
    pktout_tbl, cls = replay(c)
    o = Outputs(cap, c.nports)
    pe, h, g = o.port_entries(), o.hdr[64:128].view(DISPATCH_HDR_DTYPE), 0
    for k, tbl in enumerate(pktout_tbl):
        pe[k]["start"], pe[k]["count"] = g, len(tbl)
        pe[k]["bytes"] = sum(c.length(j) for j in tbl)
        pe[k]["flooded"] = sum(j in cls["floods"] for j in tbl)
        for j in tbl:             # ldp_out_inject(outq k, pktout_tbl[k], numout[k])
            if g < cap:
                o.list[o.pad + g] = j
                if out_off:
                    o.out_off[o.pad + g] = c.offset(j)
                if out_len:
                    o.out_len[o.pad + g] = c.length(j) & 0xFFFF
            g += 1
    h["total"], h["written"], h["reserved"] = g, min(g, cap), 0
    for k in ("unicast", "flood", "dropped", "bad", "hairpin"):
        h[k] = cls[k]
    return o


def arguments(c, inputs, outputs, cap, out_off=True, out_len=True, null_list=False):
    """struct pptk_dispatch of case c from the addresses of its inputs
    ({name: address or None}) and of entry 0 of its outputs."""
    return Dispatch(n=c.n, port=inputs["port"], idx=inputs["idx"], flow_port=inputs["flow_port"],
                    flows=c.flows, subject=inputs["subject"], in_port=inputs["in_port"],
                    in_port_all=c.in_port_all, nports=c.nports, miss_code=c.miss_code,
                    off=inputs["off"], len=inputs["lens"], stride=c.stride, fixed_len=c.fixed_len,
                    list=None if null_list else outputs["list"],
                    out_off=outputs["out_off"] if out_off else None,
                    out_len=outputs["out_len"] if out_len else None, cap=cap,
                    ports=outputs["ports"], hdr=outputs["hdr"])


def host_call(L, c, cap, out_off=True, out_len=True, null_list=False):
    """pptk_tx_dispatch_host into fresh Outputs: (rc, Outputs)."""
    import ctypes
    o = Outputs(cap, c.nports)
    d = arguments(c, c.addresses(), o.addresses(), cap, out_off, out_len, null_list)
    return L.pptk_tx_dispatch_host(ctypes.byref(d)), o


# ------------------------------------------------------------------ builders
def describe(n, rng, lens=True):
    """off / lens of n frames (or the stride form)."""
    if lens:
        return dict(off=rng.integers(0, 1 << 40, n, dtype=np.uint64) * np.uint64(8),
                    lens=rng.integers(0, 1 << 16, n, dtype=np.uint64).astype(np.uint16))
    return dict(stride=2048, fixed_len=1514)


def bad_codes(nports, count, rng):
    """Codes that are no port, FLOOD or DROP."""
    return rng.integers(nports, PORT_DROP, count).astype(np.uint8)


def codes(name, n, nports, rng, block=4096):
    """The per-frame code array of distribution `name`."""
    if name == "one_port":
        return np.full(n, nports - 1, np.uint8)
    if name == "round_robin":
        return (np.arange(n) % nports).astype(np.uint8)
    if name == "all_flood":
        return np.full(n, PORT_FLOOD, np.uint8)
    if name == "no_flood" or name == "hairpin":
        return rng.integers(0, nports, n).astype(np.uint8)
    if name == "alternating":
        a = rng.integers(0, nports, n).astype(np.uint8)
        a[::2] = PORT_FLOOD
        return a
    if name == "flood_at_block_edges":
        a = rng.integers(0, nports, n).astype(np.uint8)
        for e in range(0, n + block, block):
            for i in (e - 65, e - 64, e - 1, e, e + 63, e + 64):
                if 0 <= i < n:
                    a[i] = PORT_FLOOD
        return a
    if name == "all_dropped":
        return np.full(n, PORT_DROP, np.uint8)
    if name == "all_bad":
        return bad_codes(nports, n, rng)
    assert name == "random", name
    a = rng.integers(0, nports, n).astype(np.uint8)
    r = rng.random(n)
    a[r < 0.10] = PORT_FLOOD
    a[(r >= 0.10) & (r < 0.15)] = PORT_DROP
    k = (r >= 0.15) & (r < 0.20)
    a[k] = bad_codes(nports, int(k.sum()), rng)
    return a


DISTRIBUTIONS = ("one_port", "round_robin", "random", "all_flood", "no_flood", "alternating",
                 "flood_at_block_edges", "all_dropped", "all_bad", "hairpin")


def ingress(n, nports, rng, none_share=0.1):
    """Per-frame ingress ports, some at or above nports ("none")."""
    a = rng.integers(0, nports, n).astype(np.uint8)
    k = rng.random(n) < none_share
    a[k] = rng.integers(nports, 256, int(k.sum())).astype(np.uint8)
    return a


def case(name, n, nports, rng, block=4096, subject=False, per_frame_in=True, lens=True):
    """A port-form case of distribution `name`."""
    port = codes(name, n, nports, rng, block)
    kw = describe(n, rng, lens)
    if name == "hairpin":
        kw["in_port"] = port.copy()
    elif per_frame_in:
        kw["in_port"] = ingress(n, nports, rng)
    else:
        kw["in_port_all"] = int(rng.integers(0, nports))
    if subject:
        kw["subject"] = (rng.random(n) < 0.9).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)
    return Case(nports, port=port, **kw)


def idx_case(n, nports, flows, miss_code, rng, none_share=0.2, beyond_share=0.05, lens=True):
    """An idx-form case: a flow_port table of `flows` codes (ports, some
    FLOOD, DROP and bad), indices into it, PPTK_FLOW_NONE and indices at or
    above `flows` in between."""
    flow_port = codes("random", flows, nports, rng) if flows else None
    idx = rng.integers(0, max(flows, 1), n).astype(np.uint32)
    r = rng.random(n)
    idx[r < none_share] = FLOW_NONE
    k = (r >= none_share) & (r < none_share + beyond_share)
    idx[k] = rng.choice(np.array([flows, flows + 1, 0x7FFFFFFF, FLOW_NONE - 1], np.uint32), int(k.sum()))
    if flows == 0:
        idx[r >= none_share] = rng.integers(0, 1 << 31, int((r >= none_share).sum()))
    return Case(nports, idx=idx, flow_port=flow_port, miss_code=miss_code,
                in_port=ingress(n, nports, rng), subject=(rng.random(n) < 0.9).astype(np.uint8),
                **describe(n, rng, lens))
