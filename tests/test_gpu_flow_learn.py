"""Flow learning on the GPU (include/pptk_rx.h "Flow learning"):
pptk_flow_learn_device against pptk_flow_learn_host byte for byte -- the
header, the `written` entries of all three arrays and sentinel entries around
each, no tolerance -- over batch sizes around the wave and the counting block
(pptk_flow_learn_shape), every 16-byte phase of d_status, one batch of a full
round of the block-count scan plus a block, the distributions the hash set is
aimed at (one flow, all distinct, none, 300 hashes in one probe cluster,
hashes 0 and 2^64 - 1, three keys under one hash), max_candidates and cap
around their thresholds, null first / packets, two contexts on two streams, a
scratch reused without clearing, the chain rx -> lookup -> learn -> insert_recs
-> sync -> lookup -> learn on tests/golden/flow.npz, and the argument checks.
Needs an MI355X."""
import numpy as np
import pytest

import flowgen
import learngen as lg
from conftest import load_golden
from pptk_amd.records import FLOW_NONE, FLOW_ST_HIT, FLOW_ST_SUBJECT, REC_DTYPE
from pptk_amd.rx import flow_learn_scratch_bytes, flow_learn_shape, lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B, W = flow_learn_shape()
BIG = 1 << 30
GUARD = 256          # sentinel bytes behind the scratch


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


class DevOutputs:
    """learngen.Outputs in device memory: the same sentinel-framed arrays."""

    def __init__(self, dev, cap):
        self.host = lg.Outputs(cap)
        o = self.host
        self.new, self.hdr = upload(dev, o.new), upload(dev, o.hdr)
        self.first = upload(dev, o.first).view(torch.int32)
        self.packets = upload(dev, o.packets).view(torch.int32)

    def args(self, first=True, packets=True, null_new=False):
        p, cap = self.host.pad, self.host.cap
        assert self.new.data_ptr() % 16 == 0 and self.hdr.data_ptr() % 8 == 0
        return dict(new_recs=None if null_new else self.new[64 * p:64 * (p + max(cap, 1))],
                    first=self.first[p:] if first else False,
                    packets=self.packets[p:] if packets else False, hdr=self.hdr[32:64])

    def download(self):
        o = lg.Outputs(self.host.cap)
        o.new[:] = self.new.cpu().numpy()
        o.hdr[:] = self.hdr.cpu().numpy()
        o.first[:] = self.first.cpu().numpy().view(np.uint32)
        o.packets[:] = self.packets.cpu().numpy().view(np.uint32)
        return o


def scratch_for(dev, n, maxc):
    need = flow_learn_scratch_bytes(n, maxc)
    buf = torch.full((need + GUARD,), lg.SENT, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 256 == 0 and need % 256 == 0
    return buf


def launch(ctx, dev, d_recs, d_status, n, maxc, cap, first=True, packets=True, null_new=False,
           scratch=None, out=None, stream=None):
    """One device call into sentinel-framed outputs (fresh ones unless given):
    (DevOutputs, scratch)."""
    out = DevOutputs(dev, cap) if out is None else out
    scratch = scratch_for(dev, n, maxc) if scratch is None else scratch
    need = flow_learn_scratch_bytes(n, maxc)
    ctx.flow_learn_device(d_recs, d_status, maxc, cap, n=n, scratch=scratch[:max(need, 1)],
                          stream=stream, **out.args(first, packets, null_new))
    return out, scratch


def settle(out, scratch, n, maxc, want, first=True, packets=True):
    """After the stream is done: the device outputs equal the host's."""
    got = out.download()
    assert tuple(got.header()) == tuple(want.header()), (got.header(), want.header())
    assert got.same(want, first=first, packets=packets)
    assert (first or (got.first == lg.SENT32).all()) and (packets or (got.packets == lg.SENT32).all())
    need = flow_learn_scratch_bytes(n, maxc)
    assert (scratch[need:].cpu().numpy() == lg.SENT).all()
    return got.header()


def learn_both(ctx, dev, recs, status, maxc, cap, phase=0, first=True, packets=True,
               null_new=False, d_recs=None):
    """The device call and the host call on one batch, compared; the header."""
    n = len(status)
    d_recs = upload(dev, recs) if d_recs is None else d_recs
    d_status = upload(dev, status, phase)
    assert n == 0 or d_status.data_ptr() % 16 == phase % 16
    out, scratch = launch(ctx, dev, d_recs, d_status, n, maxc, cap, first, packets, null_new)
    rc, want = lg.host_call(lib(), recs, status, maxc, cap, first=first, packets=packets,
                            null_new=null_new)
    assert rc == 0
    torch.cuda.synchronize()
    return settle(out, scratch, n, maxc, want, first, packets)


# ------------------------------------------------------ sizes and alignments
@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, B - 1, B, B + 1, 1000, 2 * B + 3))
def test_sizes(ctx, dev, n):
    rng = np.random.default_rng(4000 + n)
    recs, status = lg.mix(n, 40, 1 / 3, rng)
    h = learn_both(ctx, dev, recs, status, BIG, max(n, 1), phase=3)
    assert h["candidates"] == (status == FLOW_ST_SUBJECT).sum() and h["flows"] <= 40
    assert n < 2000 or (h["flows"] == 40 and h["candidates"] > n // 4)
    # and with an aligned status, a small bound and a small cap
    h = learn_both(ctx, dev, recs, status, 17, 5)
    assert h["considered"] == min(17, h["candidates"]) and h["written"] == min(5, h["flows"])


@pytest.mark.parametrize("phase", range(16))
def test_status_phases(ctx, dev, phase):
    rng = np.random.default_rng(77)           # one batch at every phase
    recs, status = lg.mix(2 * B + 3, 40, 1 / 3, rng)
    status[[0, 1, 15, 16, -17, -16, -2, -1]] = FLOW_ST_SUBJECT      # the head and the tail count
    h = learn_both(ctx, dev, recs, status, BIG, 64, phase=phase)
    assert h["flows"] == 40 == h["written"] and h["candidates"] > 2000


def test_scan_round_plus_block(ctx, dev):
    """n = B * W + B + 3: one full round of the block-count scan plus a block;
    1500 candidates of 200 flows with some in the first and the last block.
    Only the candidates' records exist; the rest of d_recs is zeros."""
    rng = np.random.default_rng(0xB16)
    n = B * W + B + 3
    forced = np.unique(np.concatenate([rng.integers(0, B, 5), rng.integers(n - 40, n, 5),
                                       [0, n - 1]]))
    rest = np.setdiff1d(np.unique(rng.integers(0, n, 1600)), forced)
    pos = np.sort(np.concatenate([forced, rng.permutation(rest)[:1500 - len(forced)]]))
    keys, hashes = lg.flows(200, rng)
    rows = lg.frames_of(keys, hashes, rng.integers(0, 200, len(pos)), rng)
    recs = np.zeros(n, REC_DTYPE)
    recs[pos] = rows
    status = lg.other_status(n, rng)
    status[pos] = FLOW_ST_SUBJECT
    d_recs = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    d_recs.view(n, 64)[torch.from_numpy(pos).to(dev)] = torch.from_numpy(
        rows.view(np.uint8).reshape(-1, 64).copy()).to(dev)
    assert (pos < B).sum() >= 3 and (pos >= n - 40).sum() >= 3 and len(pos) == 1500
    h = learn_both(ctx, dev, recs, status, BIG, 256, phase=5, d_recs=d_recs)
    assert h["candidates"] == len(pos) and 195 <= h["flows"] <= 200
    h = learn_both(ctx, dev, recs, status, 1000, 100, d_recs=d_recs)
    assert h["considered"] == 1000 and h["written"] == 100


# ------------------------------------------------------------- distributions
@pytest.mark.parametrize("name", ["one_flow", "all_distinct", "no_candidates", "cluster",
                                  "edge_hashes", "three_under_one_hash"])
def test_distributions(ctx, dev, name):
    rng = np.random.default_rng(sum(name.encode()) + 1)
    if name == "one_flow":
        recs, status = lg.one_flow(4096, rng)        # every lane meets one slot
    elif name == "all_distinct":
        recs, status = lg.all_distinct(4096, rng)
    elif name == "no_candidates":
        recs, status = lg.no_candidates(4096, rng)
    elif name == "cluster":
        recs, status = lg.cluster(300, rng)          # one probe cluster under every mask
    elif name == "edge_hashes":
        recs, status = lg.edge_hashes(rng, repeats=40)
    else:
        recs, status = lg.three_under_one_hash(rng, repeats=30)
    n = len(status)
    h = learn_both(ctx, dev, recs, status, BIG, n, phase=9)
    want = dict(one_flow=1, all_distinct=4096, no_candidates=0, cluster=300,
                edge_hashes=2 + 2 * 40 + 4, three_under_one_hash=1 + 2 * 31 + 2)[name]
    assert h["flows"] == want == h["written"]
    if name in ("edge_hashes", "three_under_one_hash"):
        assert name != "edge_hashes" or set(recs["flow_hash"].tolist()) >= {0, lg.M64}
        h = learn_both(ctx, dev, recs, status, n // 2, 7)       # and bounded
        assert h["considered"] == n // 2 and h["written"] == 7


def test_max_candidates_and_cap(ctx, dev):
    rng = np.random.default_rng(0xCA9)
    recs, status = lg.mix(3000, 120, 0.4, rng)
    d_recs = upload(dev, recs)
    c = int((status == FLOW_ST_SUBJECT).sum())
    for maxc in (c - 1, c, c + 1):                   # the scratch is sized for each
        h = learn_both(ctx, dev, recs, status, maxc, 3000, phase=1, d_recs=d_recs)
        assert h["candidates"] == c and h["considered"] == min(c, maxc)
    f = int(h["flows"])
    assert f > 100
    for cap in (f - 1, f):
        h = learn_both(ctx, dev, recs, status, c, cap, d_recs=d_recs)
        assert h["written"] == cap and h["flows"] == f
    h = learn_both(ctx, dev, recs, status, c, 0, first=False, packets=False, null_new=True,
                   d_recs=d_recs)                    # cap 0 with nulls: the call only counts
    assert tuple(h) == (c, c, f, 0)
    for fp in ((False, True), (True, False), (False, False)):
        h = learn_both(ctx, dev, recs, status, BIG, f, first=fp[0], packets=fp[1], d_recs=d_recs)
        assert h["written"] == f


# ------------------------------------------------------ streams and scratch
def test_two_contexts_two_streams(ctx, dev):
    from pptk_amd.rx import RxContext
    rng = np.random.default_rng(31)
    ra, sa = lg.mix(2 * B + 3, 500, 0.5, rng)
    rb, sb = lg.mix(3 * B + 1, 60, 0.2, rng)
    other = RxContext(0, flowgen.KEY)
    d = [(upload(dev, ra), upload(dev, sa, 7)), (upload(dev, rb), upload(dev, sb, 2))]
    oa, xa = DevOutputs(dev, 600), scratch_for(dev, len(sa), BIG)
    ob, xb = DevOutputs(dev, 50), scratch_for(dev, len(sb), 4000)
    torch.cuda.synchronize()             # the uploads above ran on the current stream
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    launch(ctx, dev, d[0][0], d[0][1], len(sa), BIG, 600, scratch=xa, out=oa, stream=s1)
    launch(other, dev, d[1][0], d[1][1], len(sb), 4000, 50, scratch=xb, out=ob, stream=s2)
    s1.synchronize()
    s2.synchronize()
    ha = settle(oa, xa, len(sa), BIG, lg.host_call(lib(), ra, sa, BIG, 600)[1])
    hb = settle(ob, xb, len(sb), 4000, lg.host_call(lib(), rb, sb, 4000, 50)[1])
    assert ha["flows"] == 500 and hb["flows"] == 60 and hb["written"] == 50
    other.close()


def test_scratch_is_cleared_by_the_call(ctx, dev):
    """A, B, A into one scratch on one stream: each equals the host, so nothing
    of the call before is left in the set, the lists or the counts."""
    rng = np.random.default_rng(32)
    ra, sa = lg.all_distinct(3000, rng)
    rb, sb = lg.mix(3000, 50, 0.6, rng)
    n, maxc = 3000, 3000
    scratch = scratch_for(dev, n, maxc)
    da, db = (upload(dev, ra), upload(dev, sa)), (upload(dev, rb), upload(dev, sb))
    outs = [launch(ctx, dev, da[0], da[1], n, maxc, n, scratch=scratch)[0],
            launch(ctx, dev, db[0], db[1], n, maxc, n, scratch=scratch)[0],
            launch(ctx, dev, da[0], da[1], n, maxc, n, scratch=scratch)[0]]
    torch.cuda.synchronize()
    wa, wb = lg.host_call(lib(), ra, sa, maxc, n)[1], lg.host_call(lib(), rb, sb, maxc, n)[1]
    assert settle(outs[0], scratch, n, maxc, wa)["flows"] == 3000
    assert settle(outs[1], scratch, n, maxc, wb)["flows"] == 50
    assert settle(outs[2], scratch, n, maxc, wa)["flows"] == 3000


# --------------------------------------------------------------------- chain
def test_chain_lookup_learn_insert(ctx, dev):
    z = load_golden("flow")
    n = len(z["off"])
    recs = ctx.batch_device(torch.from_numpy(z["frames"]).to(dev), n,
                            off=torch.from_numpy(z["off"].view(np.int64)).to(dev),
                            lens=torch.from_numpy(z["len"].view(np.int16)).to(dev),
                            max_len=int(z["len"].max()))
    t = ctx.flow_table(1024)
    assert t.sync() > 0                               # empty, but synced
    idx, status = ctx.flow_lookup_device(t, recs)
    r = ctx.flow_learn_device(recs, status, BIG, n)
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert np.array_equal(st, z["subject"] * FLOW_ST_SUBJECT)
    h = r["hdr"].cpu().numpy()
    cand, flows, written = int(h[0]), int(h[2]), int(h[3])
    assert cand == int(z["subject"].sum()) > 100 and written == flows > 40 and int(h[1]) == cand
    # the download: `written` entries, not n records
    nr = r["new_recs"][:64 * written].cpu().numpy().view(REC_DTYPE)
    first = r["first"][:written].cpu().numpy().view(np.uint32)
    packets = r["packets"][:written].cpu().numpy().view(np.uint32)
    hrecs = recs.cpu().numpy().view(np.uint8).reshape(-1).view(REC_DTYPE)
    rc, want = lg.host_call(lib(), hrecs, st, BIG, n)
    wr, wf, wp = want.written()
    assert rc == 0 and np.array_equal(nr.view(np.uint8), wr.view(np.uint8))
    assert np.array_equal(first, wf) and np.array_equal(packets, wp) and packets.sum() == cand
    done, res = t.insert_recs(nr, np.arange(written, dtype=np.uint32))
    assert done == written and not res.any()
    assert t.sync() > 0
    idx2, status2 = ctx.flow_lookup_device(t, recs)
    r2 = ctx.flow_learn_device(recs, status2, BIG, n)
    torch.cuda.synchronize()
    st2, was = status2.cpu().numpy(), st == FLOW_ST_SUBJECT
    assert (st2[was] == (FLOW_ST_SUBJECT | FLOW_ST_HIT)).all() and (st2[~was] == 0).all()
    i2 = idx2.cpu().numpy().view(np.uint32)
    assert (i2[~was] == FLOW_NONE).all()
    assert np.array_equal(np.bincount(i2[was], minlength=written), packets)
    assert r2["hdr"].cpu().numpy().tolist() == [0, 0, 0, 0]
    t.close()


# ---------------------------------------------------------------- arguments
def test_argument_checks(ctx, dev):
    from pptk_amd.rx import _dp
    call = ctx._L.pptk_flow_learn_device
    rng = np.random.default_rng(5)
    recs, status = lg.mix(64, 8, 0.5, rng)
    d_recs, d_status = upload(dev, recs), upload(dev, status)
    out = DevOutputs(dev, 16)
    a = out.args()
    need = flow_learn_scratch_bytes(64, 100)
    scratch = scratch_for(dev, 64, 100)
    good = [_dp(d_recs), _dp(d_status), 64, 100, _dp(a["new_recs"]), _dp(a["first"]),
            _dp(a["packets"]), 16, _dp(a["hdr"]), _dp(scratch), need, None]

    def bad(pos, val):
        b = list(good)
        b[pos] = val
        return b

    def off(t, k):
        return _dp(t.view(torch.uint8)[k:])

    assert call(None, *good) == -22
    for b in (bad(0, None), bad(1, None), bad(8, None), bad(4, None),
              bad(2, 2**32), bad(3, 0), bad(3, BIG + 1),
              bad(0, off(d_recs, 8)), bad(4, off(a["new_recs"], 8)), bad(8, off(a["hdr"], 4)),
              bad(5, off(a["first"], 2)), bad(6, off(a["packets"], 1)),
              bad(9, off(scratch, 128)), bad(9, None), bad(10, need - 1), bad(10, 0)):
        assert call(ctx._ctx, *b) == -22, b
    torch.cuda.synchronize()
    assert out.download().untouched(hdr=True)
    assert (scratch.cpu().numpy() == lg.SENT).all()
    # n = 0: a zero header and no more; no arrays, no scratch needed
    assert call(ctx._ctx, None, None, 0, 100, None, None, None, 0, _dp(a["hdr"]), None, 0, None) == 0
    assert call(ctx._ctx, None, None, 0, 100, None, None, None, 0, None, None, 0, None) == 0
    torch.cuda.synchronize()
    got = out.download()
    assert tuple(got.header()) == (0, 0, 0, 0) and got.untouched()
    assert (got.hdr[:32] == lg.SENT).all() and (got.hdr[64:] == lg.SENT).all()
    # and the good call, with a status at an odd address
    odd = upload(dev, status, 1)
    good[1] = _dp(odd)
    assert call(ctx._ctx, *good) == 0
    torch.cuda.synchronize()
    rc, want = lg.host_call(lib(), recs, status, 100, 16)
    assert rc == 0 and out.download().same(want)
