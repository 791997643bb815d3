"""Egress dispatch on the GPU (include/pptk_rx.h "Egress dispatch"):
pptk_tx_dispatch_device against pptk_tx_dispatch_host byte for byte -- the
header, the ports, the `written` entries of list / out_off / out_len and
sentinel entries around each, a guard behind the scratch, no tolerance -- over
batch sizes around the wave and the block (pptk_tx_dispatch_shape), one batch
of a full scan round plus a block, port counts 1, 2, 3, 32, 33, 63 and 64,
every 16-byte phase of port, subject and in_port, every distribution of
tests/dispatchgen.py, scalar and per-frame ingress ports, caps around the
total and inside runs, null outputs, the stride form, the idx form under
every kind of miss_code, a scratch reused without clearing, two contexts on
two streams, the chain rx -> lookup -> dispatch on tests/golden/flow.npz
against the replay of the reference's loop, and the argument checks.  Needs an
MI355X."""
import ctypes

import numpy as np
import pytest

import dispatchgen as dg
import flowgen
from conftest import load_golden
from pptk_amd.records import (DISPATCH_HDR_DTYPE, DISPATCH_PORT_DTYPE, FLOW_KEY_DTYPE, FLOW_NONE,
                              PORT_DROP, PORT_FLOOD, as_records)
from pptk_amd.rx import _dp, _stream, lib, tx_dispatch_scratch_bytes, tx_dispatch_shape

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B, W = tx_dispatch_shape()
GUARD = 256          # sentinel bytes behind the scratch
EINVAL = -22


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ctx():
    from pptk_amd.rx import RxContext
    c = RxContext(0, flowgen.KEY)
    yield c
    c.close()


def upload(dev, a, byte_off=0):
    """The array's bytes `byte_off` bytes into a device allocation (uint8)."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    big = torch.zeros(byte_off + raw.size + 16, dtype=torch.uint8, device=dev)
    if raw.size:
        big[byte_off:byte_off + raw.size] = torch.from_numpy(raw.copy()).to(dev)
    return big[byte_off:byte_off + raw.size]


class DevCase:
    """A dispatchgen.Case in device memory, each array at its phase."""

    def __init__(self, dev, c, phases=None):
        phases = phases or {}
        self.t = {k: None if getattr(c, k) is None else upload(dev, getattr(c, k), phases.get(k, 0))
                  for k in dg.INPUTS}
        for k, ph in phases.items():
            assert self.t[k] is None or c.n == 0 or self.t[k].data_ptr() % 16 == ph % 16

    def addresses(self):
        return {k: None if t is None else t.data_ptr() for k, t in self.t.items()}


class DevOutputs:
    """dispatchgen.Outputs in device memory: the same sentinel-framed arrays."""

    def __init__(self, dev, cap, nports):
        self.host = dg.Outputs(cap, nports)
        self.t = {k: upload(dev, getattr(self.host, k)) for k in dg.Outputs.ARRAYS}

    def addresses(self):
        return {k: self.t[k].data_ptr() + o for k, o in self.host.offsets().items()}

    def download(self):
        o = dg.Outputs(self.host.cap, self.host.nports)
        for k in dg.Outputs.ARRAYS:
            getattr(o, k).view(np.uint8)[:] = self.t[k].cpu().numpy()
        return o


def scratch_for(dev, n, nports):
    need = tx_dispatch_scratch_bytes(n, nports)
    buf = torch.full((need + GUARD,), dg.SENT, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 256 == 0 and need % 256 == 0
    return buf


def launch(ctx, dev, c, dc, cap, out_off=True, out_len=True, null_list=False, scratch=None,
           out=None, stream=None):
    """One device call into sentinel-framed outputs (fresh ones unless given):
    (DevOutputs, scratch)."""
    out = DevOutputs(dev, cap, c.nports) if out is None else out
    scratch = scratch_for(dev, c.n, c.nports) if scratch is None else scratch
    d = dg.arguments(c, dc.addresses(), out.addresses(), cap, out_off, out_len, null_list)
    rc = ctx._L.pptk_tx_dispatch_device(ctx._ctx, ctypes.byref(d), _dp(scratch),
                                        tx_dispatch_scratch_bytes(c.n, c.nports),
                                        _stream(stream, dev))
    assert rc == 0, rc
    return out, scratch


def settle(out, scratch, c, want):
    """After the stream is done: the device outputs equal the host's."""
    got = out.download()
    assert tuple(got.header()) == tuple(want.header()), (got.header(), want.header())
    assert np.array_equal(got.port_entries(), want.port_entries()), (got.port_entries(),
                                                                      want.port_entries())
    assert got.same(want), got.differing(want)
    need = tx_dispatch_scratch_bytes(c.n, c.nports)
    assert (scratch[need:].cpu().numpy() == dg.SENT).all()
    return got.header()


def both(ctx, dev, c, cap, phases=None, out_off=True, out_len=True, null_list=False, dc=None):
    """The device call and the host call on one batch, compared; the header."""
    dc = DevCase(dev, c, phases) if dc is None else dc
    out, scratch = launch(ctx, dev, c, dc, cap, out_off, out_len, null_list)
    rc, want = dg.host_call(lib(), c, cap, out_off, out_len, null_list)
    assert rc == 0
    torch.cuda.synchronize()
    return settle(out, scratch, c, want)


# ------------------------------------------------------ sizes and alignments
@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 17))
def test_sizes(ctx, dev, n):
    rng = np.random.default_rng(7000 + n)
    c = dg.case("random", n, 5, rng, block=B, subject=True)
    h = both(ctx, dev, c, 2 * n + 1, phases=dict(port=3, subject=7, in_port=11))
    assert h["written"] == h["total"] and h["unicast"] + h["flood"] + h["dropped"] + h["bad"] == n
    assert n < 1000 or min(h["unicast"], h["flood"], h["dropped"], h["bad"]) > 10
    # and aligned, 64 ports from one ingress port, the stride form, a small cap
    c = dg.case("random", n, 64, rng, block=B, per_frame_in=False, lens=False)
    h = both(ctx, dev, c, 100)
    assert h["written"] == min(100, h["total"])


def test_scan_round_plus_block(ctx, dev):
    """n = W * B + B: a full round of the scan plus a block, per-frame lengths
    (the byte columns are summed too), floods and drops throughout."""
    rng = np.random.default_rng(0xD15)
    n = W * B + B
    c = dg.case("random", n, 3, rng, block=B, subject=True)
    h = both(ctx, dev, c, n + n // 2, phases=dict(port=5, subject=9, in_port=2))
    assert h["total"] == h["written"] > n // 2 and h["flood"] > n // 20


@pytest.mark.parametrize("nports", (1, 2, 3, 32, 33, 63, 64))
def test_port_counts(ctx, dev, nports):
    rng = np.random.default_rng(7100 + nports)
    c = dg.case("random", 2 * B + 17, nports, rng, block=B)
    h = both(ctx, dev, c, (2 * B + 17) * (1 + nports), phases=dict(port=1))
    assert h["total"] == h["written"]
    # the last port, and floods that skip it or port 0
    port = np.full(500, nports - 1, np.uint8)
    port[::3] = PORT_FLOOD
    inp = np.where(np.arange(500) % 2, nports - 1, 0).astype(np.uint8)
    h = both(ctx, dev, dg.Case(nports, port=port, in_port=inp, **dg.describe(500, rng)),
             500 * nports)
    assert h["flood"] == 167 and h["total"] == h["written"] == 333 + 167 * (nports - 1)


@pytest.mark.parametrize("phase", range(16))
def test_phases(ctx, dev, phase):
    rng = np.random.default_rng(78)           # one batch at every phase of each byte array
    c = dg.case("random", 2 * B + 3, 6, rng, block=B, subject=True)
    c.port[[0, 1, 15, 16, -17, -16, -2, -1]] = [0, 5, PORT_FLOOD, 1, 2, PORT_FLOOD, 5, 3]
    c.subject[[0, 1, 15, 16, -17, -16, -2, -1]] = 1
    h = both(ctx, dev, c, 3 * B, phases=dict(port=phase, subject=(phase + 5) % 16,
                                             in_port=(3 * phase + 1) % 16))
    assert h["total"] == h["written"] > B


# ------------------------------------------------------------- distributions
@pytest.mark.parametrize("name", dg.DISTRIBUTIONS)
def test_distributions(ctx, dev, name):
    rng = np.random.default_rng(sum(name.encode()) + 2)
    n = 2 * B + 17
    c = dg.case(name, n, 7, rng, block=B)
    h = both(ctx, dev, c, 7 * n, phases=dict(port=9))
    want = dict(one_port=(n, 0), round_robin=(n, 0), all_flood=(0, n), no_flood=(n, 0),
                hairpin=(n, 0), all_dropped=(0, 0), all_bad=(0, 0))
    if name in want:
        assert (h["unicast"], h["flood"]) == want[name]
    if name == "hairpin":
        assert h["hairpin"] == n
    if name == "alternating":
        assert h["flood"] == (n + 1) // 2
    if name == "flood_at_block_edges":
        assert 10 <= h["flood"] <= 18
    if name == "all_dropped":
        assert h["dropped"] == n
    if name == "all_bad":
        assert h["bad"] == n


def test_ingress(ctx, dev):
    rng = np.random.default_rng(81)
    n = B + 100
    port = dg.codes("alternating", n, 4, rng)
    dc = None
    for in_all in (0, 3, 4, 64, 255, 2**32 - 1):          # at or above nports: "none"
        c = dg.Case(4, port=port, in_port_all=in_all, stride=64, fixed_len=60)
        dc = DevCase(dev, c) if dc is None else dc
        h = both(ctx, dev, c, 4 * n, dc=dc)
        assert h["total"] == n // 2 + (n // 2) * (3 if in_all < 4 else 4)
    c = dg.Case(4, port=port, in_port=dg.ingress(n, 4, rng, 0.3), in_port_all=1, stride=64,
                fixed_len=60)
    both(ctx, dev, c, 4 * n, phases=dict(in_port=13))
    # nports == 1 flooding from port 0: reaches nobody, still counts
    flood = np.full(300, PORT_FLOOD, np.uint8)
    h = both(ctx, dev, dg.Case(1, port=flood, in_port_all=0, fixed_len=9), 300)
    assert tuple(h) == (0, 0, 0, 300, 0, 0, 0, 0)
    h = both(ctx, dev, dg.Case(1, port=flood, in_port_all=1, fixed_len=9), 300)
    assert h["total"] == 300


def test_cap_and_nullable_outputs(ctx, dev):
    rng = np.random.default_rng(82)
    n = 2 * B + 17
    c = dg.case("random", n, 6, rng, block=B)
    dc = DevCase(dev, c, dict(port=4, in_port=6))
    rc, full = dg.host_call(lib(), c, 8 * n)
    total, pe = int(full.header()["total"]), full.port_entries()
    inside = int(pe["start"][2] + pe["count"][2] // 2)               # a cut inside port 2's run
    between = int(pe["start"][3])
    assert rc == 0 and total > n and 0 < inside < between < total
    for cap in (1, total - 1, total, total + 5, inside, between):
        h = both(ctx, dev, c, cap, dc=dc)
        assert h["written"] == min(cap, total) and h["total"] == total
    h = both(ctx, dev, c, 0, null_list=True, dc=dc)                  # the call only counts
    assert h["written"] == 0 and h["total"] == total
    for oo, ol in ((False, True), (True, False), (False, False)):
        both(ctx, dev, c, inside, out_off=oo, out_len=ol, dc=dc)
    # a cut between the entries of one flood frame: its entry in port 0's run
    # is written, the one in port 1's run is not
    f = dg.Case(3, port=[0, PORT_FLOOD, 1, 2], in_port_all=2, stride=1, fixed_len=1)
    assert both(ctx, dev, f, 3)["total"] == 5
    both(ctx, dev, f, 2)
    # off / len given against stride / fixed_len
    both(ctx, dev, dg.case("random", n, 6, rng, block=B, lens=False), 8 * n)
    c2 = dg.Case(6, port=c.port, in_port=c.in_port, off=c.off, stride=64, fixed_len=70000)
    both(ctx, dev, c2, 8 * n)
    c3 = dg.Case(6, port=c.port, in_port=c.in_port, lens=c.lens, stride=64)
    both(ctx, dev, c3, 8 * n)


@pytest.mark.parametrize("miss", (0, 2, PORT_FLOOD, PORT_DROP))
def test_idx_form(ctx, dev, miss):
    rng = np.random.default_rng(83 + miss)
    n = 2 * B + 17
    c = dg.idx_case(n, 3, 40, miss, rng)
    assert (c.idx == FLOW_NONE).sum() > 1000 and ((c.idx >= 40) & (c.idx != FLOW_NONE)).sum() > 100
    for ph in (0, 4, 8, 12):
        h = both(ctx, dev, c, 3 * n, phases=dict(idx=ph, flow_port=3, subject=1, in_port=2))
    assert h["bad"] > 100 and h["total"] == h["written"]
    c0 = dg.idx_case(B + 5, 3, 0, miss, rng)                        # flows == 0, no table
    h = both(ctx, dev, c0, 3 * B, phases=dict(idx=4))
    assert h["bad"] == ((c0.subject != 0) & (c0.idx != FLOW_NONE)).sum() > 1000
    # every index at or above `flows`
    c1 = dg.Case(3, idx=np.full(200, 40, np.uint32), flow_port=c.flow_port, miss_code=miss, fixed_len=1)
    assert both(ctx, dev, c1, 200)["bad"] == 200


# ------------------------------------------------------ streams and scratch
def test_two_contexts_two_streams(ctx, dev):
    from pptk_amd.rx import RxContext
    rng = np.random.default_rng(84)
    ca = dg.case("random", 2 * B + 3, 9, rng, block=B, subject=True)
    cb = dg.case("alternating", 3 * B + 1, 33, rng, block=B)
    other = RxContext(0, flowgen.KEY)
    da, db = DevCase(dev, ca, dict(port=7)), DevCase(dev, cb, dict(port=2))
    oa, xa = DevOutputs(dev, 4 * B, 9), scratch_for(dev, ca.n, 9)
    ob, xb = DevOutputs(dev, 60 * B, 33), scratch_for(dev, cb.n, 33)
    torch.cuda.synchronize()             # the uploads above ran on the current stream
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    launch(ctx, dev, ca, da, 4 * B, scratch=xa, out=oa, stream=s1)
    launch(other, dev, cb, db, 60 * B, scratch=xb, out=ob, stream=s2)
    s1.synchronize()
    s2.synchronize()
    settle(oa, xa, ca, dg.host_call(lib(), ca, 4 * B)[1])
    hb = settle(ob, xb, cb, dg.host_call(lib(), cb, 60 * B)[1])
    assert hb["total"] == hb["written"] > 40 * B
    other.close()


def test_scratch_is_reused_without_clearing(ctx, dev):
    """A, B, A into one scratch on one stream: each equals the host, so nothing
    of the call before is left in the counts."""
    rng = np.random.default_rng(85)
    n = 3 * B
    ca = dg.case("all_flood", n, 5, rng, block=B)
    cb = dg.case("random", n, 5, rng, block=B, lens=False)
    scratch = scratch_for(dev, n, 5)
    da, db = DevCase(dev, ca), DevCase(dev, cb)
    outs = [launch(ctx, dev, ca, da, 5 * n, scratch=scratch)[0],
            launch(ctx, dev, cb, db, 5 * n, scratch=scratch)[0],
            launch(ctx, dev, ca, da, 5 * n, scratch=scratch)[0]]
    torch.cuda.synchronize()
    wa, wb = dg.host_call(lib(), ca, 5 * n)[1], dg.host_call(lib(), cb, 5 * n)[1]
    assert settle(outs[0], scratch, ca, wa)["flood"] == n
    assert settle(outs[1], scratch, cb, wb)["flood"] < n // 5
    settle(outs[2], scratch, ca, wa)


# --------------------------------------------------------------------- chain
def test_chain_lookup_dispatch(ctx, dev):
    """rx -> pptk_flow_lookup_device -> dispatch(idx, flow_port, FLOOD for an
    unknown flow) against the replay of the reference's loop run over the host
    lookup's idx."""
    z = load_golden("flow")
    n, nports = len(z["off"]), 4
    fk = np.ascontiguousarray(z["flow_keys"]).view(FLOW_KEY_DTYPE).reshape(-1)
    recs = ctx.batch_device(torch.from_numpy(z["frames"]).to(dev), n,
                            off=torch.from_numpy(z["off"].view(np.int64)).to(dev),
                            lens=torch.from_numpy(z["len"].view(np.int16)).to(dev),
                            max_len=int(z["len"].max()))
    t = ctx.flow_table(int(z["slots"][0]))
    flows = len(fk)                                                  # flow v of the fixture gets value v
    for v, (k, h) in enumerate(zip(fk, z["flow_hashes"])):
        t.insert(k, int(h), v)
    assert t.sync() > 0
    idx, status = ctx.flow_lookup_device(t, recs)
    rng = np.random.default_rng(86)
    flow_port = rng.integers(0, nports, flows).astype(np.uint8)      # a learned flow's value is its port
    flow_port[::9] = PORT_DROP
    subject = torch.from_numpy(np.ascontiguousarray(z["subject"])).to(dev)
    r = ctx.tx_dispatch_device(n, nports, idx=idx, flow_port=torch.from_numpy(flow_port).to(dev),
                               miss_code=PORT_FLOOD, subject=subject, in_port_all=1,
                               off=torch.from_numpy(z["off"].view(np.int64)).to(dev),
                               lens=torch.from_numpy(z["len"].view(np.int16)).to(dev),
                               cap=nports * n)
    torch.cuda.synchronize()
    hrecs = as_records(recs.cpu().numpy().reshape(-1))
    hidx, _ = t.lookup_host(hrecs)
    assert np.array_equal(hidx, idx.cpu().numpy().view(np.uint32))
    c = dg.Case(nports, idx=hidx, flow_port=flow_port, miss_code=PORT_FLOOD, subject=z["subject"],
                in_port_all=1, off=z["off"], lens=z["len"])
    pktout_tbl, cls = dg.replay(c)
    hdr = r["hdr"].cpu().numpy().view(DISPATCH_HDR_DTYPE)[0]
    ports = r["ports"].cpu().numpy().view(DISPATCH_PORT_DTYPE)
    flat = [j for tbl in pktout_tbl for j in tbl]
    assert hdr["total"] == hdr["written"] == len(flat) > 100
    assert (hdr["unicast"], hdr["flood"], hdr["dropped"], hdr["bad"], hdr["hairpin"]) == tuple(
        cls[k] for k in ("unicast", "flood", "dropped", "bad", "hairpin"))
    assert cls["flood"] > 40 and cls["unicast"] > 40 and cls["dropped"] > 0 and cls["bad"] == 0
    assert ports["count"].tolist() == [len(tbl) for tbl in pktout_tbl] and ports["count"][1] > 0
    w = len(flat)
    assert r["list"][:w].cpu().numpy().view(np.uint32).tolist() == flat
    # per port: inject out_off / out_len[start .. start + count)
    assert r["out_off"][:w].cpu().numpy().view(np.uint64).tolist() == [int(z["off"][j]) for j in flat]
    assert r["out_len"][:w].cpu().numpy().view(np.uint16).tolist() == [int(z["len"][j]) for j in flat]
    assert ports["bytes"].tolist() == [sum(int(z["len"][j]) for j in tbl) for tbl in pktout_tbl]
    t.close()


# ---------------------------------------------------------------- arguments
def test_argument_checks(ctx, dev):
    call = ctx._L.pptk_tx_dispatch_device
    rng = np.random.default_rng(87)
    c = dg.case("random", 64, 4, rng)
    dc, out = DevCase(dev, c), DevOutputs(dev, 256, 4)
    need = tx_dispatch_scratch_bytes(64, 4)
    scratch = scratch_for(dev, 64, 4)
    d = dg.arguments(c, dc.addresses(), out.addresses(), 256)
    sp = scratch.data_ptr()
    assert call(None, ctypes.byref(d), sp, need, None) == EINVAL           # a null ctx
    assert call(ctx._ctx, None, sp, need, None) == EINVAL                  # a null d
    for s, size in ((None, need), (sp + 128, need), (sp, need - 1), (sp, 0)):
        assert call(ctx._ctx, ctypes.byref(d), s, size, None) == EINVAL, (s, size)

    def changed(**kw):
        e = dg.arguments(c, dc.addresses(), out.addresses(), 256)
        for k, v in kw.items():
            setattr(e, k, v)
        return call(ctx._ctx, ctypes.byref(e), sp, need, None)

    for kw in (dict(ports=None), dict(hdr=None), dict(idx=dc.t["off"].data_ptr()), dict(port=None),
               dict(miss_code=4), dict(nports=0), dict(nports=65), dict(n=2**32), dict(list=None),
               dict(list=d.list + 2), dict(off=d.off + 4), dict(out_off=d.out_off + 4),
               dict(ports=d.ports + 4), dict(hdr=d.hdr + 4), dict(len=d.len + 1),
               dict(out_len=d.out_len + 1)):
        assert changed(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert out.download().untouched(dg.Outputs.ARRAYS)
    assert (scratch.cpu().numpy() == dg.SENT).all()
    # n = 0: a zero header and zero port entries, no scratch needed
    assert changed(n=0) == 0
    e = dg.arguments(c, dc.addresses(), out.addresses(), 256)
    e.n = 0
    assert call(ctx._ctx, ctypes.byref(e), None, 0, None) == 0
    torch.cuda.synchronize()
    got = out.download()
    assert got.untouched() and not got.hdr[64:128].any() and not got.ports[64:192].any()
    assert (got.hdr[:64] == dg.SENT).all() and (got.hdr[128:] == dg.SENT).all()
    assert (got.ports[:64] == dg.SENT).all() and (got.ports[192:] == dg.SENT).all()
    assert (scratch.cpu().numpy() == dg.SENT).all()
    # and the good call
    assert call(ctx._ctx, ctypes.byref(d), sp, need, None) == 0
    torch.cuda.synchronize()
    rc, want = dg.host_call(lib(), c, 256)
    assert rc == 0 and out.download().same(want)
