"""IPv4 fragmentation on the GPU (pptk_ip_fragment_device) against the
committed fixture (tests/golden/fragment.npz) and the NumPy restatement of
the contract (tests/fraggen.py): every output byte, every per-slot and
per-frame word, and everything the call must not touch (slot tails, slots
past the written ones, guard regions) -- no tolerance.  Needs an MI355X."""
import functools

import numpy as np
import pytest

import fraggen
import framegen
from conftest import load_golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 4096          # bytes of 0xEE before and after the slots
SPARE = 3             # slots past the needed ones
FILL16, FILL32 = -4370, -286331154   # 0xEEEE, 0xEEEEEEEE


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ctx():
    from pptk_amd.rx import RxContext
    c = RxContext(0, bytes(range(1, 17)))
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def fixture():
    z = load_golden("fragment")
    frames = [bytes(z["frames"][int(o):int(o) + int(l)]) for o, l in zip(z["off"], z["len"])]
    return z, frames


FIX_STRIDE, FIX_LEN = 65541, 65535   # odd stride: frame starts at every alignment


@functools.lru_cache(maxsize=None)
def fixture_fixed():
    """The fixture frames at a fixed stride with one fixed_len: what follows
    a frame inside its slot is Ethernet padding (zeros), so the truncated
    frames become whole ones."""
    _, frames = fixture()
    buf = np.zeros(len(frames) * FIX_STRIDE + 64, np.uint8)
    for i, f in enumerate(frames):
        buf[i * FIX_STRIDE:i * FIX_STRIDE + len(f)] = np.frombuffer(f, np.uint8)
    padded = [bytes(buf[i * FIX_STRIDE:i * FIX_STRIDE + FIX_LEN]) for i in range(len(frames))]
    return buf, padded


@functools.lru_cache(maxsize=None)
def restated_fixed(mtu):
    return fraggen.fragment_batch(fixture_fixed()[1], mtu)


def run(ctx, dev, buf, n, mtu, out_cap, off=None, lens=None, stride=0, fixed_len=0, shift=0,
        out_stride=0):
    """One call on a 0xEE-filled output with guards; everything as numpy."""
    big = torch.zeros(buf.size + shift + 64, dtype=torch.uint8, device=dev)
    big[shift:shift + buf.size] = torch.from_numpy(buf).to(dev)
    out_stride = out_stride or fraggen.up16(18 + mtu)
    raw = torch.full((2 * GUARD + out_cap * out_stride,), 0xEE, dtype=torch.uint8, device=dev)
    r = ctx.ip_fragment_device(
        big[shift:], n, mtu, out_cap,
        off=None if off is None else torch.from_numpy(off.view(np.int64)).to(dev),
        lens=None if lens is None else torch.from_numpy(lens.view(np.int16)).to(dev),
        stride=stride, fixed_len=fixed_len,
        out=raw[GUARD:GUARD + out_cap * out_stride], out_stride=out_stride,
        out_len=torch.full((out_cap + 8,), FILL16, dtype=torch.int16, device=dev),
        out_src=torch.full((out_cap + 8,), FILL32, dtype=torch.int32, device=dev),
        first=torch.full((n + 8,), FILL32, dtype=torch.int32, device=dev),
        count=torch.full((n + 8,), FILL32, dtype=torch.int32, device=dev),
        status=torch.full((n + 8,), 0xEE, dtype=torch.uint8, device=dev),
        totals=torch.full((2,), -1, dtype=torch.int64, device=dev))
    torch.cuda.synchronize()
    g = {k: r[k].cpu().numpy() for k in ("out_len", "out_src", "first", "count", "status", "totals")}
    g["out_len"], g["out_src"] = g["out_len"].view(np.uint16), g["out_src"].view(np.uint32)
    g["first"], g["count"] = g["first"].view(np.uint32), g["count"].view(np.uint32)
    g["totals"] = g["totals"].view(np.uint64)
    g["raw"], g["out_stride"], g["dev"] = raw.cpu().numpy(), out_stride, r
    return g


def check(g, want, n, out_cap):
    """Everything the call defines equals `want` (a fraggen.fragment_batch
    result) and everything else still holds the fill."""
    w = int(want["totals"][1])
    assert np.array_equal(g["totals"], want["totals"]), (g["totals"], want["totals"])
    for k in ("first", "count", "status"):
        assert np.array_equal(g[k][:n], want[k]), k
        assert np.all(g[k][n:] == g[k][-1]) and g[k][-1] in (0xEE, 0xEEEEEEEE), k
    assert np.array_equal(g["out_len"][:w], want["out_len"])
    assert np.array_equal(g["out_src"][:w], want["out_src"])
    assert np.all(g["out_len"][w:] == 0xEEEE) and np.all(g["out_src"][w:] == 0xEEEEEEEE)
    raw = g["raw"]
    assert np.all(raw[:GUARD] == 0xEE) and np.all(raw[-GUARD:] == 0xEE)
    exp = fraggen.slots(want["frags"], g["out_stride"], out_cap)
    got = raw[GUARD:-GUARD]
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:8]


@pytest.mark.parametrize("layout", ["offsets", "fixed"])
@pytest.mark.parametrize("shift", [0, 3, 64])
@pytest.mark.parametrize("mtu", fraggen.MTUS)
def test_fixture_parity(ctx, dev, mtu, shift, layout):
    z, frames = fixture()
    n = len(frames)
    if layout == "offsets":
        want = {k: z[f"m{mtu}_{k}"] for k in ("out_len", "out_src", "first", "count", "status",
                                             "totals")}
        pos = np.concatenate([[0], np.cumsum(want["out_len"].astype(np.int64))])
        want["frags"] = [bytes(z[f"m{mtu}_out"][pos[s]:pos[s + 1]]) for s in range(len(pos) - 1)]
        cap = int(want["totals"][0]) + SPARE
        g = run(ctx, dev, z["frames"], n, mtu, cap, off=z["off"], lens=z["len"], shift=shift)
    else:
        want = restated_fixed(mtu)
        cap = int(want["totals"][0]) + SPARE
        g = run(ctx, dev, fixture_fixed()[0], n, mtu, cap, stride=FIX_STRIDE, fixed_len=FIX_LEN,
                shift=shift)
    check(g, want, n, cap)


@functools.lru_cache(maxsize=None)
def random_case(seed):
    frames = fraggen.random_frames(20000, 0xF00 + seed)
    return frames, framegen.pack(frames, align=1)


@pytest.mark.parametrize("mtu", [576, 1280])
@pytest.mark.parametrize("seed", range(2))
def test_random_batches_match_restatement(ctx, dev, seed, mtu):
    frames, (buf, off, lens) = random_case(seed)
    want = fraggen.fragment_batch(frames, mtu)
    assert 0.3 < ((want["status"] & fraggen.ST_DONE) != 0).mean() < 0.6
    cap = int(want["totals"][0]) + SPARE
    check(run(ctx, dev, buf, len(frames), mtu, cap, off=off, lens=lens, shift=seed), want,
          len(frames), cap)


def test_scan_boundaries(ctx, dev):
    """n spans 2051 scan tiles of 256 frames (so every thread of the tile
    scan sums several) and a ragged tail; 64-byte ARP frames except big
    frames at the first and last index of tiles 0, 1, 2, 1023, 1024, the last
    whole tile, and in the tail: first, count and totals exact, slots too."""
    T, mtu = 256, 576
    n = 2051 * T + 77
    rng = np.random.default_rng(5)
    arp = framegen.eth(0x0806) + bytes(50)
    idx = sorted({t * T + k for t in (0, 1, 2, 1023, 1024, 2050) for k in (0, T - 1)}
                 | {2051 * T, 2051 * T + 40, n - 1})
    bigs = [fraggen.frame4(rng, 600 + 37 * j, (20, 24, 60)[j % 3], vlan=j if j % 4 == 0 else None,
                           pad=j % 5) for j in range(len(idx))]
    bbuf, boff, blen = framegen.pack(bigs, align=1)
    buf = np.concatenate([np.tile(np.frombuffer(arp, np.uint8), n), bbuf])
    off = np.arange(n, dtype=np.uint64) * 64
    lens = np.full(n, 64, np.uint16)
    off[idx], lens[idx] = boff + np.uint64(64 * n), blen
    r = fraggen.fragment_batch(bigs, mtu)
    assert np.all(r["count"] >= 2)
    want = dict(frags=r["frags"], out_len=r["out_len"], totals=r["totals"],
                out_src=np.array(idx, np.uint32)[r["out_src"]],
                count=np.zeros(n, np.uint32), status=np.zeros(n, np.uint8))
    want["count"][idx], want["status"][idx] = r["count"], r["status"]
    want["first"] = (np.cumsum(want["count"], dtype=np.uint64) - want["count"]).astype(np.uint32)
    cap = int(r["totals"][0]) + SPARE
    check(run(ctx, dev, buf, n, mtu, cap, off=off, lens=lens), want, n, cap)


@pytest.mark.parametrize("where", ["inside", "boundary", "zero"])
def test_out_cap_too_small(ctx, dev, where):
    """Frames before the cut complete, the straddling frame and every later
    DONE frame NOROOM, totals = {needed, written}, nothing past slot
    `written` touched (check() compares all out_cap slots and the arrays)."""
    z, frames = fixture()
    mtu = 576
    full = fraggen.fragment_batch(frames, mtu)
    k = int(np.nonzero((full["count"] >= 3) & (full["first"] > 100))[0][0])
    cap = {"inside": int(full["first"][k]) + 2, "boundary": int(full["first"][k]), "zero": 0}[where]
    want = fraggen.fragment_batch(frames, mtu, out_cap=cap)
    assert want["totals"][1] == (0 if where == "zero" else full["first"][k]) < want["totals"][0]
    later = (full["status"] & fraggen.ST_DONE != 0) & (np.arange(len(frames)) >= k)
    assert np.all(want["status"][later] & fraggen.ST_NOROOM) and later.sum() > 5
    check(run(ctx, dev, z["frames"], len(frames), mtu, cap, off=z["off"], lens=z["len"]), want,
          len(frames), cap)


def test_n_zero_and_one(ctx, dev):
    g = run(ctx, dev, np.zeros(64, np.uint8), 0, 576, 4, stride=64, fixed_len=64)
    assert tuple(g["totals"]) == (0, 0) and np.all(g["raw"] == 0xEE)
    assert np.all(g["status"] == 0xEE) and np.all(g["out_len"] == 0xEEEE)
    f = fraggen.frame4(np.random.default_rng(9), 1501, 24, vlan=3, pad=5)
    buf, off, lens = framegen.pack([f])
    for layout in ({"off": off, "lens": lens}, {"stride": 0, "fixed_len": len(f)}):
        want = fraggen.fragment_batch([f], 576)
        check(run(ctx, dev, buf, 1, 576, 5, shift=7, **layout), want, 1, 5)


def test_round_trip_through_receive_transform(ctx, dev):
    """The slots go straight back into pptk_rx_batch_device: every one parses
    as a valid IPv4 fragment and its side record is the plan."""
    from pptk_amd.records import (F_FRAGMENT, F_IP_OK, F_MALFORMED, F_PARSED, FRAG_DTYPE, FRAG_IS,
                                  FRAG_MF, as_records)
    z, frames = fixture()
    for mtu in (68, 576):
        want = fraggen.fragment_batch(frames, mtu)
        w = int(want["totals"][1])
        g = run(ctx, dev, z["frames"], len(frames), mtu, w, off=z["off"], lens=z["len"])
        r = g["dev"]
        side = torch.empty((w, 16), dtype=torch.uint8, device=dev)
        recs = ctx.batch_device(r["out"], w, lens=r["out_len"], stride=g["out_stride"],
                                max_len=18 + mtu, frag_out=side)
        torch.cuda.synchronize()
        fl = as_records(recs.cpu().numpy().reshape(-1))["flags"]
        assert np.all(fl & (F_PARSED | F_IP_OK | F_FRAGMENT) == F_PARSED | F_IP_OK | F_FRAGMENT)
        assert not np.any(fl & F_MALFORMED)
        s = side.cpu().numpy().reshape(-1).view(FRAG_DTYPE)
        plan = []
        for i, f in enumerate(frames):
            st, pl = fraggen.plan(f, mtu)
            if pl:
                l2, ihl, tl = fraggen.subject(f)
                plan += [((f[l2 + 4] << 8) | f[l2 + 5], ds, dl,
                          FRAG_IS | (FRAG_MF if ds + dl < tl - ihl else 0)) for ds, dl in pl]
        p = np.array(plan, np.int64)
        assert len(p) == w
        for k, name in enumerate(("ident", "frag_off", "data_len", "flags")):
            assert np.array_equal(s[name].astype(np.int64), p[:, k]), name


def test_rejects_bad_arguments(ctx, dev):
    from pptk_amd.rx import _dp
    L = ctx._L
    fr = torch.zeros(4096, dtype=torch.uint8, device=dev)
    out = torch.zeros(8192, dtype=torch.uint8, device=dev)
    tot = torch.full((2,), -1, dtype=torch.int64, device=dev)
    sc = torch.zeros(L.pptk_ip_fragment_scratch_bytes(4), dtype=torch.uint8, device=dev)

    def call(mtu=576, o=out, stride=608, cap=4, n=4, totals=tot, scratch=sc, fstride=64, c=ctx._ctx):
        return L.pptk_ip_fragment_device(c, _dp(fr), None, None, fstride, 64, n, mtu, _dp(o), stride,
                                         cap, None, None, None, None, None, _dp(totals),
                                         _dp(scratch), None)
    assert call() == 0
    torch.cuda.synchronize()
    assert tuple(tot.cpu().numpy()) == (0, 0)      # four zero frames: no subject
    assert call(mtu=67) == -22 and call(mtu=65536) == -22
    assert call(o=out[8:]) == -22                  # d_out not 16-byte aligned
    assert call(stride=600) == -22 and call(stride=592) == -22
    assert call(totals=None) == -22 and call(scratch=None) == -22 and call(c=None) == -22
    assert call(fstride=0) == -22                  # no layout
    assert call(n=(1 << 24) + 1) == -22 and call(cap=1 << 32) == -22
    assert call(n=0, scratch=None) == 0            # n = 0 needs no scratch
