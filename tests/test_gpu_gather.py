"""Egress gather on the GPU (include/pptk_rx.h "Egress gather"):
pptk_tx_gather_device against pptk_tx_gather_host byte for byte -- the header,
the ports, pk_off / pk_len over the considered entries, the whole `out` buffer
with the sentinels between the regions and behind out_cap, sentinel entries
around every array, a guard behind the scratch, no tolerance -- over entry
counts around the wave and the block (pptk_tx_gather_shape), one scan round
plus a block, every source byte phase against every length class and the
lengths around a team round of every team width built, list and len at every
16-byte phase of their own arrays, repeats, bad indices, port counts, caps and
d_entries (one of them the header word a dispatch call on the same stream
wrote just before), null pk_off / pk_len, the count-only call, a scratch
reused without clearing, two contexts on two streams, the chain rx -> lookup
-> dispatch -> gather on tests/golden/flow.npz, and the argument checks.
Needs an MI355X."""
import ctypes

import numpy as np
import pytest

import dispatchgen as dg
import flowgen
import gathergen as gg
from conftest import load_golden
from pptk_amd.records import (DISPATCH_HDR_DTYPE, DISPATCH_PORT_DTYPE, FLOW_KEY_DTYPE,
                              GATHER_HDR_DTYPE, GATHER_PORT_DTYPE, GATHER_ST_BADRUNS, PORT_DROP,
                              PORT_FLOOD)
from pptk_amd.rx import (_dp, _stream, lib, tx_dispatch_host, tx_gather_scratch_bytes,
                         tx_gather_shape)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B, W = tx_gather_shape()
GUARD = 256          # sentinel bytes behind the scratch
EINVAL = -22
UNROLL = 4           # rounds of a team's loads in flight (tx_gather.hip kUnroll)
TEAMS = (4, 8, 16, 32)   # the team widths built


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
    """A gathergen.Case in device memory, each array at its phase."""

    def __init__(self, dev, c, phases=None):
        phases = phases or {}
        self.t = {k: None if getattr(c, k) is None else upload(dev, getattr(c, k), phases.get(k, 0))
                  for k in gg.INPUTS}
        for k, ph in phases.items():
            assert self.t[k] is None or self.t[k].numel() == 0 or self.t[k].data_ptr() % 16 == ph % 16

    def addresses(self):
        return {k: None if t is None else t.data_ptr() for k, t in self.t.items()}


class DevOutputs:
    """gathergen.Outputs in device memory: the same sentinel-framed arrays."""

    def __init__(self, dev, max_entries, nports, out_cap):
        self.host = gg.Outputs(max_entries, nports, out_cap)
        self.t = {k: upload(dev, getattr(self.host, k)) for k in gg.Outputs.ARRAYS}
        assert (self.t["out"].data_ptr() + gg.GUARD) % 256 == 0

    def addresses(self):
        return {k: self.t[k].data_ptr() + o for k, o in self.host.offsets().items()}

    def download(self):
        h = self.host
        o = gg.Outputs(h.max_entries, h.nports, h.out_cap)
        for k in gg.Outputs.ARRAYS:
            getattr(o, k).view(np.uint8)[:] = self.t[k].cpu().numpy()
        return o


def scratch_for(dev, max_entries, nports):
    need = tx_gather_scratch_bytes(max_entries, nports)
    buf = torch.full((need + GUARD,), gg.SENT, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 256 == 0 and need % 256 == 0
    return buf


def launch(ctx, dev, c, dc, out_cap, pk_off=True, pk_len=True, scratch=None, out=None, stream=None,
           d_entries=None):
    """One device call into sentinel-framed outputs (fresh ones unless given):
    (DevOutputs, scratch)."""
    out = DevOutputs(dev, c.max_entries, c.nports, out_cap) if out is None else out
    scratch = scratch_for(dev, c.max_entries, c.nports) if scratch is None else scratch
    g = gg.arguments(c, dc.addresses(), out.addresses(), out_cap, pk_off, pk_len)
    if d_entries is not None:
        g.d_entries = d_entries
    rc = ctx._L.pptk_tx_gather_device(ctx._ctx, ctypes.byref(g), _dp(scratch),
                                      tx_gather_scratch_bytes(c.max_entries, c.nports),
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
    need = tx_gather_scratch_bytes(c.max_entries, c.nports)
    assert (scratch[need:].cpu().numpy() == gg.SENT).all()
    return got.header()


def both(ctx, dev, c, out_cap, phases=None, pk_off=True, pk_len=True, dc=None):
    """The device call and the host call on one case, compared; the header."""
    dc = DevCase(dev, c, phases) if dc is None else dc
    out, scratch = launch(ctx, dev, c, dc, out_cap, pk_off, pk_len)
    rc, want = gg.host_call(lib(), c, out_cap, pk_off, pk_len)
    assert rc == 0
    torch.cuda.synchronize()
    return settle(out, scratch, c, want)


def room(lengths):
    """An out_cap that holds these frames in any number of regions below 64."""
    return int(sum((int(x) + 15) // 16 * 16 for x in lengths)) + 64 * 256


# ------------------------------------------------------ sizes and alignments
@pytest.mark.parametrize("count", (1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 17))
def test_entry_counts(ctx, dev, count):
    rng = np.random.default_rng(9000 + count)
    n = max(count // 2, 1)
    lengths = gg.mixed_lengths(n, rng, top=400)
    b = gg.batch(lengths, rng, "off")
    lst = gg.entry_list("flood", n, count, rng)
    c = gg.Case(**b, list=lst, runs=gg.split_runs(count, 3, rng), nports=3)
    h = both(ctx, dev, c, room(lengths[lst]), phases=dict(frames=5, list=4, lens=6))
    assert h["packed"] == h["entries"] == count and h["status"] == 0
    # the identity list, one region, the stride form
    b = gg.batch(gg.mixed_lengths(count, rng, top=120), rng, "stride")
    h = both(ctx, dev, gg.Case(**b), room(b["lens"]))
    assert h["packed"] == count and h["bad"] == 0


def test_scan_round_plus_block(ctx, dev):
    """W * B + B entries: a full round of the scan plus a block; short frames,
    four ports, a flood list."""
    rng = np.random.default_rng(0x6A7)
    count, n = W * B + B, 50000
    lengths = rng.integers(0, 41, n)
    b = gg.batch(lengths, rng, "stride")
    lst = rng.integers(0, n, count).astype(np.uint32)
    c = gg.Case(**b, list=lst, runs=gg.split_runs(count, 4, rng, empty=False), nports=4)
    h = both(ctx, dev, c, room(lengths[lst]), phases=dict(list=8, lens=2))
    assert h["packed"] == h["entries"] == count
    assert both(ctx, dev, c, int(h["need"]) // 2)["packed"] < count


@pytest.mark.parametrize("phase", range(16))
def test_source_phases(ctx, dev, phase):
    """Every length class at source byte phase `phase`, in both length-array
    forms and with list and len at that phase of their own arrays."""
    rng = np.random.default_rng(9100 + phase)
    lengths = np.array(list(gg.LENGTHS) + [31, 32, 33, 255, 256, 257], np.int64)
    b = gg.batch(lengths, rng, "off", phases=np.full(len(lengths), phase))
    assert ((b["off"] % 16) == phase).all()
    lst = rng.permutation(np.arange(2 * len(lengths)) % len(lengths)).astype(np.uint32)
    c = gg.Case(**b, list=lst, runs=[len(lengths), len(lengths)], nports=2)
    h = both(ctx, dev, c, room(lengths[lst]), phases=dict(list=phase & ~3, lens=phase & ~1,
                                                          off=8 * (phase & 1)))
    assert h["packed"] == 2 * len(lengths)
    # the batch as a whole shifted by the phase too
    both(ctx, dev, gg.Case(**b), room(lengths), phases=dict(frames=phase))


@pytest.mark.parametrize("length", (1, 96, 97, 320, 321, 896, 897, 2047, 2048, 2049, 4113))
def test_team_widths_fixed(ctx, dev, length):
    """One fixed length selects the team width: both sides of every switch
    point (96 / 320 / 896 bytes), and for the widest team -- the only one whose
    fixed lengths pass one round of team * 16 * UNROLL bytes -- the lengths
    just under, at and over one and two rounds.  A stride coprime to 16 walks
    the frames over every source phase."""
    rng = np.random.default_rng(9200 + length)
    stride = length + 3
    frames = rng.integers(0, 256, 17 * stride + 16, dtype=np.uint8)
    c = gg.Case(frames, 17, stride=stride, fixed_len=length)
    h = both(ctx, dev, c, 17 * (length + 16))
    assert h["packed"] == 17 and h["frame_bytes"] == 17 * length
    c = gg.Case(frames, 17, stride=stride, fixed_len=length, list=gg.entry_list("bad", 17, 40, rng))
    h = both(ctx, dev, c, 40 * (length + 16), phases=dict(frames=length % 16))
    assert h["packed"] == 40 and h["bad"] > 0


def test_team_rounds_length_array(ctx, dev):
    """The same lengths around every width's team round with a length array
    (the width built for device lengths), at every source phase."""
    rng = np.random.default_rng(9300)
    lengths = []
    for team in TEAMS:
        rnd = team * 16 * UNROLL
        lengths += [rnd - 1, rnd, rnd + 1, 2 * rnd + 1]
    lengths = np.array(lengths * 16, np.int64)
    ph = np.repeat(np.arange(16), len(lengths) // 16)
    b = gg.batch(lengths, rng, "off", phases=ph)
    h = both(ctx, dev, gg.Case(**b), room(lengths))
    assert h["packed"] == len(lengths)


@pytest.mark.parametrize("phase", (0, 4, 8, 12))
def test_list_and_len_phases(ctx, dev, phase):
    rng = np.random.default_rng(9400 + phase)
    n, count = 700, 2 * B + 9
    lengths = gg.mixed_lengths(n, rng, top=300)
    b = gg.batch(lengths, rng, "stride")
    lst = gg.entry_list("bad", n, count, rng)
    c = gg.Case(**b, list=lst, runs=gg.split_runs(count, 5, rng), nports=5)
    for lp in (phase, phase + 2, phase + 14):
        h = both(ctx, dev, c, room(lengths) * 4, phases=dict(list=phase, lens=lp % 16))
    assert h["bad"] > 100 and h["packed"] == count


# ------------------------------------------------- ports, caps and d_entries
@pytest.mark.parametrize("nports", (1, 2, 3, 64))
def test_port_counts(ctx, dev, nports):
    rng = np.random.default_rng(9500 + nports)
    n, count = 500, 2 * B + 17
    lengths = gg.mixed_lengths(n, rng, top=200)
    b = gg.batch(lengths, rng, "off")
    lst = gg.entry_list("flood", n, count, rng)
    for runs in ([None] if nports == 1 else []) + [gg.split_runs(count, nports, rng)]:
        c = gg.Case(**b, list=lst, runs=runs, nports=nports)
        h = both(ctx, dev, c, room(lengths[lst]), phases=dict(frames=3))
        assert h["packed"] == h["entries"] == count
    # every run but the last empty, and every run but the first
    for counts in ([0] * (nports - 1) + [count], [count] + [0] * (nports - 1)):
        c = gg.Case(**b, list=lst, runs=counts[:nports], nports=nports)
        assert both(ctx, dev, c, room(lengths[lst]))["packed"] == count


def test_caps_and_nullable_outputs(ctx, dev):
    rng = np.random.default_rng(9600)
    n, count = 400, 2 * B + 50
    lengths = gg.mixed_lengths(n, rng, top=200)
    b = gg.batch(lengths, rng, "off")
    lst = gg.entry_list("flood", n, count, rng)
    c = gg.Case(**b, list=lst, runs=[B - 10, 0, B + 30, 30], nports=4)
    dc = DevCase(dev, c, dict(frames=9, list=4))
    rc, full = gg.host_call(lib(), c, room(lengths[lst]))
    need, pe = int(full.header()["need"]), full.port_entries()
    off, ln = full.considered()
    g = B + 40                                                    # an entry of port 2, past a block edge
    while ln[g] < 40:
        g += 1
    inside, slot_end, region = int(off[g]) + 20, int(off[g]) + (int(ln[g]) + 15) // 16 * 16, int(pe["start"][2])
    assert rc == 0 and 0 < region < inside < slot_end < need
    edge = int(off[B])                                            # a cut at a block's first entry
    for cap in (inside, slot_end, slot_end - 1, region, region - 1, edge, need - 1, need, need + 300,
                16, 0):
        h = both(ctx, dev, c, cap, dc=dc)
        assert h["need"] == need and (h["packed"] == count) == (cap >= need)
    for po, pl in ((False, True), (True, False), (False, False)):
        both(ctx, dev, c, inside, pk_off=po, pk_len=pl, dc=dc)
        both(ctx, dev, c, 0, pk_off=po, pk_len=pl, dc=dc)         # the count-only call
    # a cap that ends in the padding between two regions
    assert both(ctx, dev, c, int(pe["start"][3]) - 1, dc=dc)["packed"] <= 2 * B + 20


def test_d_entries(ctx, dev):
    rng = np.random.default_rng(9700)
    n, count = 300, B + 200
    lengths = gg.mixed_lengths(n, rng, top=150)
    b = gg.batch(lengths, rng, "stride")
    lst = gg.entry_list("permuted", n, count, rng)
    for d in (0, 1, 100, B, B + 1, count, count + 1, 2**40):
        c = gg.Case(**b, list=lst, d_entries=d, runs=[100, B, 100], nports=3)
        h = both(ctx, dev, c, room(lengths) * 8)
        assert h["entries"] == min(d, count) == h["packed"]
        c1 = gg.Case(**b, list=lst, d_entries=d)                  # null runs
        assert both(ctx, dev, c1, room(lengths) * 8)["entries"] == min(d, count)
    c = gg.Case(**b, list=lst, runs=[10, 20], nports=2)          # runs that end below max_entries
    assert both(ctx, dev, c, room(lengths) * 8)["entries"] == 30


def test_bad_runs(ctx, dev):
    rng = np.random.default_rng(9800)
    b = gg.batch(gg.mixed_lengths(50, rng, top=100), rng, "off")
    for runs in (gg.make_runs([10, 20, 20], first=1),
                 np.array([(0, 10, 0, 0), (11, 20, 0, 0)], DISPATCH_PORT_DTYPE),
                 np.array([(0, 2**64 - 1, 0, 0), (2**64 - 1, 5, 0, 0)], DISPATCH_PORT_DTYPE)):
        c = gg.Case(**b, runs=runs, nports=len(runs))
        dc = DevCase(dev, c)
        out, scratch = launch(ctx, dev, c, dc, 1 << 16)
        torch.cuda.synchronize()
        got = out.download()
        assert tuple(got.header()) == (0, 0, 0, 0, 0, 0, GATHER_ST_BADRUNS, 0)
        assert got.untouched() and got.same(gg.host_call(lib(), c, 1 << 16)[1])


# ------------------------------------------------------ streams and scratch
def test_two_contexts_two_streams(ctx, dev):
    from pptk_amd.rx import RxContext
    rng = np.random.default_rng(9900)
    la, lb = gg.mixed_lengths(600, rng, top=300), gg.mixed_lengths(900, rng, top=90)
    ca = gg.Case(**gg.batch(la, rng, "off"), list=gg.entry_list("flood", 600, 2 * B + 3, rng),
                 runs=gg.split_runs(2 * B + 3, 9, rng), nports=9)
    cb = gg.Case(**gg.batch(lb, rng, "stride"), list=gg.entry_list("bad", 900, 3 * B + 1, rng),
                 runs=gg.split_runs(3 * B + 1, 33, rng), nports=33)
    other = RxContext(0, flowgen.KEY)
    da, db = DevCase(dev, ca, dict(frames=7)), DevCase(dev, cb, dict(list=12))
    capa, capb = room(la) * 8, room(lb) * 8
    oa, xa = DevOutputs(dev, ca.max_entries, 9, capa), scratch_for(dev, ca.max_entries, 9)
    ob, xb = DevOutputs(dev, cb.max_entries, 33, capb), scratch_for(dev, cb.max_entries, 33)
    torch.cuda.synchronize()             # the uploads above ran on the current stream
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    launch(ctx, dev, ca, da, capa, scratch=xa, out=oa, stream=s1)
    launch(other, dev, cb, db, capb, scratch=xb, out=ob, stream=s2)
    s1.synchronize()
    s2.synchronize()
    settle(oa, xa, ca, gg.host_call(lib(), ca, capa)[1])
    hb = settle(ob, xb, cb, gg.host_call(lib(), cb, capb)[1])
    assert hb["packed"] == 3 * B + 1 and hb["bad"] > 100
    other.close()


def test_scratch_is_reused_without_clearing(ctx, dev):
    """A, B, A into one scratch on one stream: each equals the host, so nothing
    of the call before is left in the sums."""
    rng = np.random.default_rng(9950)
    count = 3 * B
    la, lb = gg.mixed_lengths(500, rng, top=500), gg.mixed_lengths(500, rng, top=40)
    ca = gg.Case(**gg.batch(la, rng, "off"), list=gg.entry_list("flood", 500, count, rng),
                 runs=gg.split_runs(count, 5, rng), nports=5)
    cb = gg.Case(**gg.batch(lb, rng, "stride"), list=gg.entry_list("bad", 500, count, rng),
                 d_entries=B + 7, runs=gg.split_runs(count, 5, rng), nports=5)
    scratch = scratch_for(dev, count, 5)
    da, db = DevCase(dev, ca), DevCase(dev, cb)
    cap = room(la) * 8
    outs = [launch(ctx, dev, ca, da, cap, scratch=scratch)[0],
            launch(ctx, dev, cb, db, cap, scratch=scratch)[0],
            launch(ctx, dev, ca, da, cap, scratch=scratch)[0]]
    torch.cuda.synchronize()
    wa, wb = gg.host_call(lib(), ca, cap)[1], gg.host_call(lib(), cb, cap)[1]
    assert settle(outs[0], scratch, ca, wa)["entries"] == count
    assert settle(outs[1], scratch, cb, wb)["entries"] == B + 7
    settle(outs[2], scratch, ca, wa)


# --------------------------------------------------------------------- chain
def test_dispatch_header_feeds_gather(ctx, dev):
    """d_entries points into the header a dispatch call on the same stream
    wrote just before, runs at its ports: no download in between."""
    rng = np.random.default_rng(9960)
    n, nports = B + 300, 4
    lengths = gg.mixed_lengths(n, rng, top=250)
    b = gg.batch(lengths, rng, "off")
    port = dg.codes("random", n, nports, rng)
    cap = 2 * n                                                   # below the total: the list is cut
    t = {k: upload(dev, b[k]) for k in ("frames", "off", "lens")}
    r = ctx.tx_dispatch_device(n, nports, port=upload(dev, port), in_port_all=1,
                               off=t["off"].view(torch.int64), lens=t["lens"].view(torch.int16),
                               cap=cap)
    hdr_written = r["hdr"].data_ptr() + DISPATCH_HDR_DTYPE.fields["written"][1]
    out_cap = room(lengths) * nports
    g = ctx.tx_gather_device(t["frames"], n, cap, out_cap, nports=nports,
                             off=t["off"].view(torch.int64), lens=t["lens"].view(torch.int16),
                             entries=r["list"], d_entries=hdr_written, runs=r["ports"])
    torch.cuda.synchronize()
    dh, runs, lst, _, _ = tx_dispatch_host(nports, port=port, in_port_all=1, off=b["off"],
                                           lens=b["lens"], cap=cap)
    assert np.array_equal(r["list"][:len(lst)].cpu().numpy().view(np.uint32), lst)
    c = gg.Case(**b, list=lst, max_entries=cap, d_entries=int(dh["written"]), runs=runs, nports=nports)
    want = gg.expected(c, out_cap)
    assert tuple(g["hdr"].cpu().numpy().view(GATHER_HDR_DTYPE)[0]) == tuple(want.header())
    assert np.array_equal(g["ports"].cpu().numpy().view(GATHER_PORT_DTYPE), want.port_entries())
    e = int(want.header()["entries"])
    assert e == int(dh["written"]) > n
    assert np.array_equal(g["pk_off"][:e].cpu().numpy().view(np.uint64), want.considered()[0])
    assert np.array_equal(g["pk_len"][:e].cpu().numpy().view(np.uint16), want.considered()[1])
    body, got = want.packed_bytes(), g["out"].cpu().numpy()
    assert np.array_equal(got[body != gg.SENT], body[body != gg.SENT])


def test_chain_lookup_dispatch_gather(ctx, dev):
    """rx -> pptk_flow_lookup_device -> dispatch -> gather on the flow
    fixture: every port's region equals what a replay of the reference's
    per-port copy loop over the replayed output tables leaves."""
    z = load_golden("flow")
    n, nports = len(z["off"]), 4
    fk = np.ascontiguousarray(z["flow_keys"]).view(FLOW_KEY_DTYPE).reshape(-1)
    frames = torch.from_numpy(z["frames"]).to(dev)
    off = torch.from_numpy(z["off"].view(np.int64)).to(dev)
    lens = torch.from_numpy(z["len"].view(np.int16)).to(dev)
    recs = ctx.batch_device(frames, n, off=off, lens=lens, max_len=int(z["len"].max()))
    t = ctx.flow_table(int(z["slots"][0]))
    for v, (k, h) in enumerate(zip(fk, z["flow_hashes"])):
        t.insert(k, int(h), v)
    assert t.sync() > 0
    idx, status = ctx.flow_lookup_device(t, recs)
    rng = np.random.default_rng(86)
    flow_port = rng.integers(0, nports, len(fk)).astype(np.uint8)
    flow_port[::9] = PORT_DROP
    subject = torch.from_numpy(np.ascontiguousarray(z["subject"])).to(dev)
    r = ctx.tx_dispatch_device(n, nports, idx=idx, flow_port=torch.from_numpy(flow_port).to(dev),
                               miss_code=PORT_FLOOD, subject=subject, in_port_all=1, off=off,
                               lens=lens, cap=nports * n)
    out_cap = nports * int(((z["len"].astype(np.int64) + 15) // 16 * 16).sum()) + 1024
    g = ctx.tx_gather_device(frames, n, nports * n, out_cap, nports=nports, off=off, lens=lens,
                             entries=r["list"],
                             d_entries=r["hdr"].data_ptr() + DISPATCH_HDR_DTYPE.fields["written"][1],
                             runs=r["ports"])
    torch.cuda.synchronize()
    c = dg.Case(nports, idx=idx.cpu().numpy().view(np.uint32), flow_port=flow_port,
                miss_code=PORT_FLOOD, subject=z["subject"], in_port_all=1, off=z["off"], lens=z["len"])
    tables, cls = dg.replay(c)
    assert cls["flood"] > 40 and cls["unicast"] > 40
    src = gg.Case(z["frames"], n, off=z["off"], lens=z["len"])
    regions = gg.replay_regions(src, tables)
    hdr = g["hdr"].cpu().numpy().view(GATHER_HDR_DTYPE)[0]
    pe, body = g["ports"].cpu().numpy().view(GATHER_PORT_DTYPE), g["out"].cpu().numpy()
    assert hdr["packed"] == hdr["entries"] == sum(len(tb) for tb in tables) and hdr["bad"] == 0
    assert pe["entries"].tolist() == [len(tb) for tb in tables]
    for p in range(nports):
        s, nb = int(pe["start"][p]), int(pe["bytes"][p])
        assert nb == len(regions[p]) > 0 and bytes(body[s:s + nb]) == regions[p], p
    t.close()


# ---------------------------------------------------------------- arguments
def test_argument_checks(ctx, dev):
    call = ctx._L.pptk_tx_gather_device
    rng = np.random.default_rng(9970)
    b = gg.batch(gg.mixed_lengths(64, rng, top=100), rng, "off")
    c = gg.Case(**b, list=gg.entry_list("permuted", 64, 64, rng), d_entries=50, runs=[32, 32],
                nports=2)
    dc, out = DevCase(dev, c), DevOutputs(dev, 64, 2, 16384)
    need = tx_gather_scratch_bytes(64, 2)
    scratch = scratch_for(dev, 64, 2)
    g = gg.arguments(c, dc.addresses(), out.addresses(), 16384)
    sp = scratch.data_ptr()
    assert call(None, ctypes.byref(g), sp, need, None) == EINVAL           # a null ctx
    assert call(ctx._ctx, None, sp, need, None) == EINVAL                  # a null g
    for s, size in ((None, need), (sp + 128, need), (sp, need - 1), (sp, 0)):
        assert call(ctx._ctx, ctypes.byref(g), s, size, None) == EINVAL, (s, size)

    def changed(**kw):
        e = gg.arguments(c, dc.addresses(), out.addresses(), 16384)
        for k, v in kw.items():
            setattr(e, k, v)
        return call(ctx._ctx, ctypes.byref(e), sp, need, None)

    for kw in (dict(ports=None), dict(hdr=None), dict(nports=0), dict(nports=65), dict(runs=None),
               dict(frames=None), dict(off=None, stride=0), dict(len=None, fixed_len=65536),
               dict(max_entries=2**32), dict(n=2**32), dict(out=None), dict(out=g.out + 128),
               dict(list=g.list + 2), dict(off=g.off + 4), dict(pk_off=g.pk_off + 4),
               dict(runs=g.runs + 4), dict(ports=g.ports + 4), dict(hdr=g.hdr + 4),
               dict(d_entries=g.d_entries + 4), dict(len=g.len + 1), dict(pk_len=g.pk_len + 1)):
        assert changed(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert out.download().untouched(gg.Outputs.ARRAYS)
    assert (scratch.cpu().numpy() == gg.SENT).all()
    # max_entries = 0: a zero header and zero port entries, no scratch needed
    e = gg.arguments(c, dc.addresses(), out.addresses(), 16384)
    e.max_entries = 0
    assert call(ctx._ctx, ctypes.byref(e), None, 0, None) == 0
    torch.cuda.synchronize()
    got = out.download()
    assert got.untouched() and not got.hdr[64:128].any() and not got.ports[64:128].any()
    assert (got.hdr[:64] == gg.SENT).all() and (got.hdr[128:] == gg.SENT).all()
    assert (got.ports[:64] == gg.SENT).all() and (got.ports[128:] == gg.SENT).all()
    assert (scratch.cpu().numpy() == gg.SENT).all()
    # and the good call
    assert call(ctx._ctx, ctypes.byref(g), sp, need, None) == 0
    torch.cuda.synchronize()
    rc, want = gg.host_call(lib(), c, 16384)
    assert rc == 0 and out.download().same(want) and want.header()["entries"] == 50
