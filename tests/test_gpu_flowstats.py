"""Flow state on the GPU (include/pptk_rx.h "Flow state"):
pptk_flow_account_device against pptk_flow_account_host -- all four words of
every entry and sentinel entries on both sides of the array, no tolerance --
over batch sizes around the block and the kernel's segment
(pptk_flow_account_shape), every 16-byte phase of d_idx and 8-byte phase of
d_len, the distributions the LDS stage is aimed at (one flow, all unmatched,
more distinct flows in a segment than its table holds, indices that collide
under any power-of-two mask, runs of equal indices, a mix), both length
forms, a null d_unmatched and two streams into one array;
pptk_flow_stats_reset_device; pptk_tx_rewrite_flow_device on the rewrite
fixtures of tests/golden/rewrite.npz; the chain rx -> lookup -> account ->
download -> expire -> sync -> lookup on tests/golden/flow.npz; and the
argument checks.  Needs an MI355X."""
import numpy as np
import pytest

import flowgen
import flowstatgen as fs
from conftest import load_golden
from pptk_amd.records import (FLOW_KEY_DTYPE, FLOW_NONE, FLOW_STATS_DTYPE, RW_ST_NOFLOW,
                              as_records)
from pptk_amd.rx import flow_account_host, flow_account_shape, flow_stats_array
from test_oracle import REWRITE_CASES, rewrite_case

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PAD = 2
S, K = flow_account_shape()
NS = (0, 1, 63, 64, 65, 255, 256, 257, 1000, S - 1, S, S + 1, 2 * S + 3)
BIG = 2 * S + 3
OVER = min(S, 4 * K) if K else S         # distinct flows per segment: past the LDS table
WIDE = 6 * 65536 + 1                     # an array with several multiples of 65536


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


def at_offset(dev, a, byte_off, tdtype):
    """The array's bytes `byte_off` bytes into a device allocation, as a
    tensor of tdtype (None for None)."""
    if a is None:
        return None
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    big = torch.zeros(byte_off + raw.size + 32, dtype=torch.uint8, device=dev)
    big[byte_off:byte_off + raw.size] = torch.from_numpy(raw.copy()).to(dev)
    return big[byte_off:byte_off + raw.size].view(tdtype)


class DevStats:
    """`count` entries 32 bytes into a device allocation, between PAD
    sentinel entries on each side, and the host array they started as."""

    def __init__(self, dev, count, pad=PAD):
        self.whole, self.st = fs.stats_array(count, pad)
        self.pad, self.count = pad, count
        raw = self.whole.view(np.uint8)
        self.buf = torch.zeros(32 + raw.size, dtype=torch.uint8, device=dev)
        self.buf[32:] = torch.from_numpy(raw.copy()).to(dev)
        self.d = self.buf[32 + 32 * pad:32 + 32 * (pad + count)]
        assert self.d.data_ptr() % 32 == 0 and self.d.numel() == 32 * count

    def download(self):
        torch.cuda.synchronize()
        return self.buf[32:].cpu().numpy().view(FLOW_STATS_DTYPE)

    def check(self):
        """The device array equals the host array, sentinels included."""
        got = self.download()
        for f in FLOW_STATS_DTYPE.names:
            bad = np.nonzero(got[f] != self.whole[f])[0]
            assert bad.size == 0, (f, bad[:6] - self.pad, got[f][bad[:6]], self.whole[f][bad[:6]])
        for f in FLOW_STATS_DTYPE.names:
            assert (got[f][:self.pad] == fs.SENT).all() and (got[f][-self.pad:] == fs.SENT).all()
        assert (got["reserved"] == fs.SENT).all()


def account_both(ctx, dev, ds, idx, now, lens=None, fixed_len=0, um=None, io=0, lo=0, stream=None):
    """One device call and the host call on the mirrored arrays."""
    n = len(idx)
    d_idx = at_offset(dev, idx, io, torch.int32)
    d_len = at_offset(dev, lens, lo, torch.int16)
    if d_idx is not None and n:
        assert d_idx.data_ptr() % 16 == io % 16
    if stream is not None:
        torch.cuda.synchronize()         # the uploads above ran on the current stream
    ctx.flow_account_device(d_idx, ds.d, now, lens=d_len, fixed_len=fixed_len,
                            unmatched=None if um is None else um.d, n=n, stream=stream)
    flow_account_host(idx, ds.st, now, lens=lens, fixed_len=fixed_len,
                      unmatched=None if um is None else um.st)
    return d_idx, d_len


# ------------------------------------------------------ sizes and alignments
@pytest.mark.parametrize("n", NS)
def test_sizes_and_alignments(ctx, dev, n):
    rng = np.random.default_rng(1000 + n)
    count = 3000
    idx = fs.mix(max(n, 1), count, min(OVER, count), rng)[:n]
    lens = fs.lengths(max(n, 1), rng)[:n]
    ds, um = DevStats(dev, count), DevStats(dev, 1)
    keep = []
    now = 10
    for io in (0, 4, 8, 12):
        for lo in (0, 2, 14):
            now += 7
            keep.append(account_both(ctx, dev, ds, idx, now, lens=lens, um=um, io=io, lo=lo))
    keep.append(account_both(ctx, dev, ds, idx, 5, fixed_len=1514, um=um, io=4))   # an older clock
    ds.check()
    um.check()
    assert int(ds.st["packets"].sum() + um.st["packets"][0]) == 13 * n
    if n:
        assert max(int(ds.st["last_seen"].max()), int(um.st["last_seen"][0])) == now


# ------------------------------------------------------------- distributions
def _dist(name, rng):
    """(idx, stats_count) of a distribution at n = 2S + 3."""
    if name == "one_flow":
        return fs.one_flow(BIG, 3000, rng), 3000
    if name == "unmatched":
        return fs.all_unmatched(BIG, 3000, rng), 3000
    if name == "overflow":
        return fs.distinct(BIG, 2 * OVER + 5, OVER, rng), 2 * OVER + 5
    if name == "step4096":
        return fs.strided(BIG, WIDE, 4096, rng), WIDE
    if name == "step65536":
        return fs.strided(BIG, WIDE, 65536, rng), WIDE
    if name == "runs":
        return fs.runs(BIG, 3000, rng), 3000
    if name == "mix":
        return fs.mix(BIG, WIDE, OVER, rng), WIDE
    raise KeyError(name)


@pytest.mark.parametrize("name", ["one_flow", "unmatched", "overflow", "step4096", "step65536",
                                  "runs", "mix"])
def test_distributions(ctx, dev, name):
    rng = np.random.default_rng(sum(name.encode()))
    idx, count = _dist(name, rng)
    lens = fs.lengths(BIG, rng)
    ds, um = DevStats(dev, count), DevStats(dev, 1)
    keep = [account_both(ctx, dev, ds, idx, 100, lens=lens, um=um),
            account_both(ctx, dev, ds, idx, 200, fixed_len=65535, um=um),
            account_both(ctx, dev, ds, idx, 300, lens=lens, um=None, io=8, lo=2),     # no drop counter
            account_both(ctx, dev, ds, idx, 250, fixed_len=0, um=None)]
    ds.check()
    um.check()
    hit = idx < count
    assert int(ds.st["packets"].sum()) == 4 * int(hit.sum())
    assert int(um.st["packets"][0]) == 2 * int((~hit).sum())
    if name == "one_flow":
        assert int(ds.st["packets"][3000 // 3]) == 4 * BIG
    if name == "unmatched":
        assert not ds.st["packets"].any() and not ds.st["last_seen"].any()
        assert um.st["last_seen"][0] == 200
    if name == "overflow":
        assert np.unique(idx[:OVER]).size == OVER and (K == 0 or OVER > K)
    if name in ("step4096", "step65536"):
        step = int(name[4:])
        assert not (idx % step).any() and np.unique(idx).size >= 5
    assert len(keep) == 4


def test_two_streams(ctx, dev):
    """Two calls on two streams, different `now`, one array: sums add and
    last_seen is the max."""
    rng = np.random.default_rng(22)
    count, n = 500, max(BIG, 6000)       # enough frames for the two calls to share flows
    a = fs.mix(n, count, min(OVER, count), rng)
    b = np.concatenate([fs.runs(n // 2, count, rng),
                        rng.integers(0, count + 20, n - n // 2).astype(np.uint32)])
    la = fs.lengths(n, rng)
    ds, um = DevStats(dev, count), DevStats(dev, 1)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    keep = [account_both(ctx, dev, ds, a, 900, lens=la, um=um, stream=s1),
            account_both(ctx, dev, ds, b, 700, fixed_len=60, um=um, stream=s2)]
    s1.synchronize()
    s2.synchronize()
    ds.check()
    um.check()
    both = np.intersect1d(a[a < count], b[b < count])
    assert both.size > 50 and (ds.st["last_seen"][both] == 900).all()
    only_b = np.setdiff1d(b[b < count], a)
    assert (ds.st["last_seen"][only_b] == 700).all()
    assert len(keep) == 2


# --------------------------------------------------------------------- reset
def test_reset(ctx, dev):
    rng = np.random.default_rng(5)
    count = 400
    ds = DevStats(dev, count)
    idx = rng.integers(0, count, 3000).astype(np.uint32)
    keep = account_both(ctx, dev, ds, idx, 50, fixed_len=100)
    vals = np.concatenate([rng.integers(0, count, 120), [7, 7, 7, count - 1, count, count + 1,
                                                         FLOW_NONE, 0]]).astype(np.uint32)
    d_vals = at_offset(dev, vals, 4, torch.int32)
    ctx.flow_stats_reset_device(ds.d, d_vals, 77)
    inside = np.unique(vals[vals < count])
    for f, x in (("packets", 0), ("bytes", 0), ("last_seen", 77)):
        ds.st[f][inside] = x
    ds.check()
    untouched = np.setdiff1d(np.arange(count), inside)
    assert untouched.size > 200 and ds.st["packets"][untouched].sum() > 1000
    assert ds.st["last_seen"][count - 1] == 77 and ds.st["packets"][7] == 0
    # a reset stamp is a stamp like any other: accounting keeps the max
    keep2 = account_both(ctx, dev, ds, idx[:500], 60, fixed_len=1)
    ds.check()
    ctx.flow_stats_reset_device(ds.d, d_vals[:0], 99)                 # count = 0: nothing
    ds.check()
    assert keep and keep2


# ------------------------------------------------------------ rewrite by flow
def _flow_rewrite(ctx, dev, z, buf, rw_rows, idx, shift, stride=None, use_flow=True):
    big = torch.zeros(buf.size + shift + 64, dtype=torch.uint8, device=dev)
    big[shift:shift + buf.size] = torch.from_numpy(buf).to(dev)
    frames = big[shift:]
    n = len(z["off"])
    rw_t = torch.from_numpy(np.ascontiguousarray(rw_rows).view(np.uint8).reshape(-1).copy()).to(dev)
    st = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    d_idx = None if idx is None else torch.from_numpy(idx.view(np.int32).copy()).to(dev)
    kw = (dict(off=torch.from_numpy(z["off"].view(np.int64)).to(dev),
               lens=torch.from_numpy(z["len"].view(np.int16)).to(dev)) if stride is None
          else dict(stride=stride, fixed_len=int(z["len"][0])))
    if use_flow:
        ctx.tx_rewrite_flow_device(frames, n, rw_t, idx=d_idx, status=st, **kw)
    else:
        ctx.tx_rewrite_device(frames, n, rw_t, status=st, **kw)
    torch.cuda.synchronize()
    return big.cpu().numpy(), st.cpu().numpy()


def _flow_case(tag, name, stride=None):
    """The golden case as a table of its distinct rewrites and an idx; every
    seventh frame has no flow (PPTK_FLOW_NONE or rw_count in turn)."""
    z, buf_in, buf_out, rw, status = rewrite_case(tag, name)
    n = len(z["off"])
    rows, inv = np.unique(rw.view(np.uint8).reshape(-1, 16), axis=0, return_inverse=True)
    idx = (np.zeros(n, np.int64) if len(rw) == 1 else inv.reshape(-1)).astype(np.uint32)
    none = np.arange(n) % 7 == 3
    idx[none] = np.where(np.arange(n) % 14 == 3, FLOW_NONE, len(rows))[none]
    want, wst = buf_out.copy(), status.copy()
    for i in np.nonzero(none)[0]:
        o = i * stride if stride is not None else int(z["off"][i])
        want[o:o + int(z["len"][i])] = buf_in[o:o + int(z["len"][i])]
    wst[none] = RW_ST_NOFLOW
    return z, buf_in, rows, idx, want, wst


@pytest.mark.parametrize("tag,name", REWRITE_CASES)
@pytest.mark.parametrize("shift", [0, 5, 64])
def test_rewrite_by_flow(ctx, dev, tag, name, shift):
    z, buf_in, rows, idx, want, wst = _flow_case(tag, name)
    big, st = _flow_rewrite(ctx, dev, z, buf_in, rows, idx, shift)
    assert np.array_equal(st, wst), np.nonzero(st != wst)[0][:8]
    got = big[shift:shift + buf_in.size]
    assert np.array_equal(got, want), int((got != want).sum())
    assert not big[:shift].any() and not big[shift + buf_in.size:].any()
    assert (wst == RW_ST_NOFLOW).sum() >= len(wst) // 7 and (want != buf_in).any()


def test_rewrite_by_flow_fixed_stride(ctx, dev):
    z, buf_in, rows, idx, want, wst = _flow_case("c64", "c64", stride=64)
    big, st = _flow_rewrite(ctx, dev, z, buf_in, rows, idx, 3, stride=64)
    assert np.array_equal(st, wst)
    assert np.array_equal(big[3:3 + buf_in.size], want)


@pytest.mark.parametrize("tag,name", [("fuzz", "fuzz"), ("c64_one", "c64")])
def test_rewrite_flow_without_idx_is_rewrite(ctx, dev, tag, name):
    z, buf_in, buf_out, rw, status = rewrite_case(tag, name)
    a, sa = _flow_rewrite(ctx, dev, z, buf_in, rw, None, 5)
    b, sb = _flow_rewrite(ctx, dev, z, buf_in, rw, None, 5, use_flow=False)
    assert np.array_equal(a, b) and np.array_equal(sa, sb) and np.array_equal(sa, status)
    assert np.array_equal(a[5:5 + buf_in.size], buf_out)


# --------------------------------------------------------------------- chain
def test_chain_account_expire(ctx, dev):
    z = load_golden("flow")
    fk = np.ascontiguousarray(z["flow_keys"]).view(FLOW_KEY_DTYPE).reshape(-1)
    nf = len(fk)
    # this test's own flow values 0 .. nf - 1, in the fixture's order
    of_value = {int(v): j for j, v in enumerate(z["flow_values"])}
    assert len(of_value) == nf
    want = np.array([FLOW_NONE if v == FLOW_NONE else of_value[int(v)] for v in z["idx"]], np.uint32)
    t = ctx.flow_table(int(z["slots"][0]))
    for j in range(nf):
        t.insert(fk[j], int(z["flow_hashes"][j]), j)
    assert t.sync() > 0
    n = len(z["off"])
    d_len = torch.from_numpy(z["len"].view(np.int16)).to(dev)
    recs = ctx.batch_device(torch.from_numpy(z["frames"]).to(dev), n,
                            off=torch.from_numpy(z["off"].view(np.int64)).to(dev), lens=d_len,
                            max_len=int(z["len"].max()))
    ds, um = DevStats(dev, nf), DevStats(dev, 1)
    all_vals = torch.arange(nf, dtype=torch.int32, device=dev)
    ctx.flow_stats_reset_device(ds.d, all_vals, 500)          # inserted: stamped before any frame
    ds.st["last_seen"] = 500
    idx, _ = ctx.flow_lookup_device(t, recs)
    ctx.flow_account_device(idx, ds.d, 1000, lens=d_len, unmatched=um.d)
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy().view(np.uint32), want)
    fs.account(ds.st, want, 1000, lens=z["len"], unmatched=um.st)
    ds.check()
    um.check()
    hit = want != FLOW_NONE
    assert np.array_equal(ds.st["packets"], np.bincount(want[hit], minlength=nf).astype(np.uint64))
    assert np.array_equal(ds.st["bytes"], np.bincount(want[hit], weights=z["len"][hit],
                                                      minlength=nf).astype(np.uint64))
    assert um.st["packets"][0] == (~hit).sum() > 60 and um.st["bytes"][0] == z["len"][~hit].sum()
    # a later batch in which only the even flows send
    even = (hit & (want % 2 == 0)).astype(np.uint8)
    idx2, _ = ctx.flow_lookup_device(t, recs, subject=torch.from_numpy(even).to(dev))
    um2 = DevStats(dev, 1)
    ctx.flow_account_device(idx2, ds.d, 2000, lens=d_len, unmatched=um2.d)
    fs.account(ds.st, np.where(even != 0, want, FLOW_NONE).astype(np.uint32), 2000, lens=z["len"],
               unmatched=um2.st)
    ds.check()
    um2.check()
    # the host: download, expire, sync
    host = flow_stats_array(nf)
    host[:] = ds.download()[PAD:PAD + nf]
    gone = t.expire(host, 2500, 1000)
    idle = [j for j in range(nf) if fs.is_idle(j, ds.st, 2500, 1000)]
    assert sorted(gone.tolist()) == idle and nf // 3 <= len(idle) <= nf - nf // 3
    assert all(j % 2 == 1 or ds.st["packets"][j] == 0 for j in idle)
    assert t.sync() > 0
    idx3, _ = ctx.flow_lookup_device(t, recs)
    torch.cuda.synchronize()
    after = np.where(np.isin(want, np.array(idle, np.uint32)), FLOW_NONE, want).astype(np.uint32)
    assert np.array_equal(idx3.cpu().numpy().view(np.uint32), after)
    assert (after != FLOW_NONE).sum() > 20 and (after != want).sum() > 20
    t.close()


# ---------------------------------------------------------------- arguments
def test_argument_checks(ctx, dev):
    from pptk_amd.rx import _dp
    L = ctx._L
    ds, um = DevStats(dev, 16), DevStats(dev, 1)
    idx = at_offset(dev, np.arange(16, dtype=np.uint32), 0, torch.int32)
    lens = at_offset(dev, np.full(16, 64, np.uint16), 0, torch.int16)
    i8, l8, s8, u8 = (x.view(torch.uint8) for x in (idx, lens, ds.d, um.d))
    acc = L.pptk_flow_account_device
    good = (_dp(idx), _dp(lens), 0, 16, _dp(ds.d), 16, _dp(um.d), 9, None)

    def bad(pos, val):
        a = list(good)
        a[pos] = val
        return a

    assert acc(None, *good) == -22
    for a in (bad(0, None), bad(4, None), bad(5, 0), bad(5, 2**32 + 1), bad(0, _dp(i8[2:])),
              bad(1, _dp(l8[1:])), bad(4, _dp(s8[16:])), bad(6, _dp(u8[8:])), bad(2, 65536),
              bad(1, None)[:2] + [65536] + bad(1, None)[3:]):
        assert acc(ctx._ctx, *a) == -22, a
    rst = L.pptk_flow_stats_reset_device
    assert rst(None, _dp(ds.d), 16, _dp(idx), 16, 9, None) == -22
    assert rst(ctx._ctx, None, 16, _dp(idx), 16, 9, None) == -22
    assert rst(ctx._ctx, _dp(ds.d), 0, _dp(idx), 16, 9, None) == -22
    assert rst(ctx._ctx, _dp(ds.d), 2**32 + 1, _dp(idx), 16, 9, None) == -22
    assert rst(ctx._ctx, _dp(s8[8:]), 15, _dp(idx), 16, 9, None) == -22
    assert rst(ctx._ctx, _dp(ds.d), 16, None, 16, 9, None) == -22
    assert rst(ctx._ctx, _dp(ds.d), 16, _dp(i8[1:]), 15, 9, None) == -22
    rwf = L.pptk_tx_rewrite_flow_device
    frames = torch.zeros(16 * 64, dtype=torch.uint8, device=dev)
    rw = torch.zeros(3 * 16, dtype=torch.uint8, device=dev)
    st = torch.full((16,), 0xEE, dtype=torch.uint8, device=dev)
    tail = (_dp(st), None)
    assert rwf(None, _dp(frames), None, None, 64, 64, 16, _dp(rw), 3, _dp(idx), *tail) == -22
    assert rwf(ctx._ctx, _dp(frames), None, None, 64, 64, 16, _dp(rw), 0, _dp(idx), *tail) == -22
    assert rwf(ctx._ctx, _dp(frames), None, None, 64, 64, 16, None, 3, _dp(idx), *tail) == -22
    assert rwf(ctx._ctx, _dp(frames), None, None, 64, 64, 16, _dp(rw), 3, _dp(i8[2:]), *tail) == -22
    assert rwf(ctx._ctx, _dp(frames), None, None, 64, 64, 16, _dp(rw), 3, None, *tail) == -22
    assert rwf(ctx._ctx, None, None, None, 64, 64, 16, _dp(rw), 3, _dp(idx), *tail) == -22
    assert rwf(ctx._ctx, _dp(frames), None, None, 64, 65536, 16, _dp(rw), 3, _dp(idx), *tail) == -22
    ds.check()
    um.check()
    assert (st.cpu().numpy() == 0xEE).all() and not frames.cpu().numpy().any()
    # n = 0 launches nothing and needs no arrays
    assert acc(ctx._ctx, None, None, 0, 0, _dp(ds.d), 16, None, 9, None) == 0
    assert rst(ctx._ctx, _dp(ds.d), 16, None, 0, 9, None) == 0
    assert rwf(ctx._ctx, None, None, None, 0, 0, 0, None, 0, None, None, None) == 0
    ds.check()
    # and the good call counts: zeroed all-zero frames are no IPv4, status 0 / NOFLOW
    assert acc(ctx._ctx, *good) == 0
    flow_account_host(np.arange(16, dtype=np.uint32), ds.st, 9, lens=np.full(16, 64, np.uint16))
    ds.check()
    assert rwf(ctx._ctx, _dp(frames), None, None, 64, 64, 16, _dp(rw), 3, _dp(idx), *tail) == 0
    torch.cuda.synchronize()
    assert st.cpu().numpy().tolist() == [0] * 3 + [RW_ST_NOFLOW] * 13
