"""GRE tunnel encapsulation and decapsulation on the GPU
(pptk_tunnel_encap_device / pptk_tunnel_decap_device) against the committed
fixture (tests/golden/tunnel.npz) and the NumPy restatement of the contracts
(tests/tungen.py): every output byte, length, status and descriptor, and
everything the calls must not touch (slot tails, slots without DONE, guard
regions, the frames) -- no tolerance -- and the three chains a tunnel
endpoint runs with the receive transform and fragmentation.  Needs an
MI355X."""
import functools

import numpy as np
import pytest

import fraggen
import framegen
import tungen
from conftest import load_golden
from pptk_amd.records import TUNNEL_DTYPE

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 4096          # bytes of 0xEE before and after the slots
PAD = 8               # entries of fill past the per-frame arrays
FILL16 = -4370        # 0xEEEE


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
    z = load_golden("tunnel")
    frames = [bytes(z["frames"][int(o):int(o) + int(l)]) for o, l in zip(z["off"], z["len"])]
    dframes = [bytes(z["dframes"][int(o):int(o) + int(l)]) for o, l in zip(z["doff"], z["dlen"])]
    return z, frames, dframes


@functools.lru_cache(maxsize=None)
def want_fixture(name):
    """The fixture's expectation of one mode as an encap_batch result."""
    z, _, _ = fixture()
    olen = z[f"{name}_out_len"].astype(np.int64)
    pos = np.concatenate([[0], np.cumsum(olen)])
    slots = [bytes(z[f"{name}_out"][pos[i]:pos[i + 1]]) if olen[i] else None
             for i in range(len(olen))]
    return dict(slots=slots, out_len=z[f"{name}_out_len"], status=z[f"{name}_status"])


def put(dev, buf, shift):
    """buf on the device, starting `shift` bytes into an allocation."""
    big = torch.zeros(buf.size + shift + 64, dtype=torch.uint8, device=dev)
    big[shift:shift + buf.size] = torch.from_numpy(buf).to(dev)
    return big[shift:]


def i64(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)


def i16(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(dev)


def i32(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)


def run_encap(ctx, dev, buf, n, tun, idx=None, id_base=0, off=None, lens=None, stride=0,
              fixed_len=0, shift=0, out_stride=tungen.FULL_STRIDE):
    """One call on 0xEE-filled outputs with guards; everything as numpy."""
    raw = torch.full((2 * GUARD + n * out_stride,), 0xEE, dtype=torch.uint8, device=dev)
    r = ctx.tunnel_encap_device(
        put(dev, buf, shift), n, tun, idx=i32(idx, dev), id_base=id_base, off=i64(off, dev),
        lens=i16(lens, dev), stride=stride, fixed_len=fixed_len,
        out=raw[GUARD:GUARD + n * out_stride], out_stride=out_stride,
        out_len=torch.full((n + PAD,), FILL16, dtype=torch.int16, device=dev),
        status=torch.full((n + PAD,), 0xEE, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    return dict(raw=raw.cpu().numpy(), out_len=r["out_len"].cpu().numpy().view(np.uint16),
                status=r["status"].cpu().numpy(), out_stride=out_stride, dev=r)


def check_encap(g, want, n):
    """Everything the call defines equals `want` (a tungen.encap_batch
    result) and everything else still holds the fill."""
    assert np.array_equal(g["status"][:n], want["status"]), np.nonzero(g["status"][:n] != want["status"])
    assert np.array_equal(g["out_len"][:n], want["out_len"])
    assert np.all(g["status"][n:] == 0xEE) and np.all(g["out_len"][n:] == 0xEEEE)
    raw = g["raw"]
    assert np.all(raw[:GUARD] == 0xEE) and np.all(raw[-GUARD:] == 0xEE)
    exp = tungen.slot_buffer(want["slots"], g["out_stride"])
    got = raw[GUARD:-GUARD]
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:8]


# ---------------------------------------------------------------------- encap
@pytest.mark.parametrize("shift", range(16))
@pytest.mark.parametrize("name", ["idx", "one", "per"])
def test_encap_fixture_parity(ctx, dev, name, shift):
    z, frames, _ = fixture()
    n = len(frames)
    tun, idx = tungen.modes(n)[name]
    g = run_encap(ctx, dev, z["frames"], n, tun, idx, tungen.ID_BASE, off=z["off"], lens=z["len"],
                  shift=shift)
    check_encap(g, want_fixture(name), n)


def test_encap_noroom_stride(ctx, dev):
    """out_stride 1552: the frames above 1514 bytes get NOROOM (with TOOBIG
    where that holds too) and their slots stay untouched; the others are the
    fixture's."""
    z, frames, _ = fixture()
    n = len(frames)
    tun, idx = tungen.modes(n)["idx"]
    want = dict(want_fixture("idx"), status=z["nr_status"], out_len=z["nr_out_len"])
    want["slots"] = [s if l else None for s, l in zip(want["slots"], z["nr_out_len"])]
    assert sum(s is not None for s in want["slots"]) > 15
    g = run_encap(ctx, dev, z["frames"], n, tun, idx, tungen.ID_BASE, off=z["off"], lens=z["len"],
                  shift=3, out_stride=tungen.NR_STRIDE)
    check_encap(g, want, n)


@functools.lru_cache(maxsize=None)
def fixed_case(flen):
    """The fixture's bytes cut into frames of flen bytes at an odd stride:
    every start alignment, one length."""
    z, _, _ = fixture()
    stride = flen + 3 if flen % 2 == 0 else flen + 2
    src = z["frames"][:min(z["frames"].size, 40 * stride)]
    n = src.size // stride - 1
    frames = [bytes(src[i * stride:i * stride + flen]) for i in range(n)]
    return src, stride, frames


# 13: all RUNT; 14: the shortest; then both sides of every length at which a
# fixed-length call takes the next team width (4, 8, 16, 32 lanes; a length
# array, as in the fixture tests, always takes 16)
@pytest.mark.parametrize("name", ["one", "per"])
@pytest.mark.parametrize("shift", [0, 5, 11])
@pytest.mark.parametrize("flen", [13, 14, 64, 96, 97, 320, 321, 896, 897, 1500])
def test_encap_fixed_stride(ctx, dev, flen, shift, name):
    src, stride, frames = fixed_case(flen)
    n = len(frames)
    assert n >= 16
    tun, idx = tungen.modes(n)[name]
    want = tungen.encap_batch(frames, tun, idx, 0xFFFFFFF0)
    ostr = tungen.up16(38 + flen) + 16
    g = run_encap(ctx, dev, src, n, tun, idx, 0xFFFFFFF0, stride=stride, fixed_len=flen,
                  shift=shift, out_stride=ostr)
    check_encap(g, want, n)


def test_encap_bad_tunnel_entries(ctx, dev):
    """A table entry with a non-zero `reserved` or an unknown flag bit is
    malformed: its frames get BADTUN and are left alone, beside the NOFLOW of
    the frames without an entry (the table goes in as a device tensor: the
    binding's host-side check does not see it)."""
    z, frames, _ = fixture()
    n = len(frames)
    tun, idx = tungen.modes(n)["idx"]
    tun = tun.copy()
    tun["reserved"][0], tun["flags"][2] = 1, 0x10 | tungen.TUN_DF
    want = tungen.encap_batch(frames, tun, idx, 7)
    assert (want["status"] == tungen.ST_BADTUN).sum() > 15 and (want["status"] == tungen.ST_NOFLOW).sum() >= 4
    d_tun = torch.from_numpy(tun.view(np.uint8).copy()).to(dev)
    g = run_encap(ctx, dev, z["frames"], n, d_tun, idx, 7, off=z["off"], lens=z["len"])
    check_encap(g, want, n)


def test_encap_nullable_outputs_and_n_zero(ctx, dev):
    from pptk_amd.rx import _dp
    z, frames, _ = fixture()
    n, L = len(frames), ctx._L
    tun, _ = tungen.modes(n)["one"]
    d_tun = torch.from_numpy(tun.view(np.uint8).copy()).to(dev)
    fr, off, lens = put(dev, z["frames"], 0), i64(z["off"], dev), i16(z["len"], dev)
    ostr = tungen.FULL_STRIDE
    raw = torch.full((2 * GUARD + n * ostr,), 0xEE, dtype=torch.uint8, device=dev)
    out = raw[GUARD:GUARD + n * ostr]
    assert L.pptk_tunnel_encap_device(ctx._ctx, _dp(fr), _dp(off), _dp(lens), 0, 0, 0, _dp(d_tun),
                                      1, None, 0, _dp(out), ostr, None, None, None) == 0
    assert L.pptk_tunnel_encap_device(ctx._ctx, None, None, None, 0, 0, 0, _dp(d_tun), 1, None, 0,
                                      None, 0, None, None, None) == 0
    torch.cuda.synchronize()
    assert bool((raw == 0xEE).all())                       # n = 0 writes nothing
    assert L.pptk_tunnel_encap_device(ctx._ctx, _dp(fr), _dp(off), _dp(lens), 0, 0, n, _dp(d_tun),
                                      1, None, tungen.ID_BASE, _dp(out), ostr, None, None,
                                      None) == 0
    torch.cuda.synchronize()
    exp = tungen.slot_buffer(want_fixture("one")["slots"], ostr)
    got = raw.cpu().numpy()
    assert np.array_equal(got[GUARD:-GUARD], exp)
    assert np.all(got[:GUARD] == 0xEE) and np.all(got[-GUARD:] == 0xEE)
    r = ctx.tunnel_decap_device(fr, 0, off=off, lens=lens)
    assert r["status"].numel() == 0
    assert L.pptk_tunnel_decap_device(ctx._ctx, _dp(fr), _dp(off), _dp(lens), 0, 0, n, None, None,
                                      None, None) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("flen,with_lens,n", [(64, False, (1 << 20) + 77), (128, False, (1 << 19) + 77),
                                             (64, True, (1 << 18) + 77), (400, False, (1 << 18) + 77),
                                             (900, False, (1 << 17) + 77)])
def test_encap_more_frames_than_teams(ctx, dev, flen, with_lens, n):
    """More frames than one pass of the grid takes (2^14 blocks of 256 lanes),
    for every team width: 4 lanes (above 2^20 frames), 8 (2^19), 16 (2^18,
    through a length array and through a fixed length) and 32 (2^17), ids
    counting through several wraps.  Checked on the device."""
    tot = 38 + flen
    ostr = tungen.up16(tot) + 16
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    fr = torch.randint(0, 256, (n * flen + 64,), dtype=torch.uint8, device=dev, generator=g)
    tun = tungen.tunnels()[1:2]
    lens = torch.full((n,), flen, dtype=torch.int16, device=dev) if with_lens else None
    out = torch.full((n, ostr), 0xEE, dtype=torch.uint8, device=dev)
    r = ctx.tunnel_encap_device(fr, n, tun, id_base=5, lens=lens, stride=flen, fixed_len=flen,
                                out=out, out_stride=ostr)
    torch.cuda.synchronize()
    assert bool((r["status"] == tungen.ST_DONE).all()) and bool((r["out_len"] == tot).all())
    assert torch.equal(out[:, 38:tot], fr[:n * flen].view(n, flen))
    assert bool((out[:, tot:tungen.up16(tot)] == 0).all())
    assert bool((out[:, tungen.up16(tot):] == 0xEE).all())
    hdr = np.frombuffer(tungen.header(tun[0], flen, 0), np.uint8).copy()
    fixed = [k for k in range(38) if k not in (18, 19, 24, 25)]
    assert torch.equal(out[:, fixed], torch.from_numpy(hdr[fixed]).to(dev).expand(n, -1))
    ids = (int(tun[0]["id"]) + 5 + torch.arange(n, device=dev)) & 0xFFFF
    assert torch.equal(out[:, 18].long() * 256 + out[:, 19].long(), ids)
    # the header checksum verifies: the ten big-endian words sum to 0xffff
    w = out[:, 14:34].long()
    s = (w[:, 0::2] * 256 + w[:, 1::2]).sum(1)
    s = (s & 0xFFFF) + (s >> 16)
    s = (s & 0xFFFF) + (s >> 16)
    assert bool((s == 0xFFFF).all())


# ---------------------------------------------------------------------- decap
@pytest.mark.parametrize("shift", [0, 1, 2, 3, 7, 13])
def test_decap_fixture_parity(ctx, dev, shift):
    z, _, dframes = fixture()
    n = len(dframes)
    fr = put(dev, z["dframes"], shift)
    before = fr.clone()
    r = ctx.tunnel_decap_device(
        fr, n, off=i64(z["doff"], dev), lens=i16(z["dlen"], dev),
        in_off=torch.full((n + PAD,), -1, dtype=torch.int64, device=dev),
        in_len=torch.full((n + PAD,), FILL16, dtype=torch.int16, device=dev),
        status=torch.full((n + PAD,), 0xEE, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    st, io = r["status"].cpu().numpy(), r["in_off"].cpu().numpy().view(np.uint64)
    il = r["in_len"].cpu().numpy().view(np.uint16)
    assert np.array_equal(st[:n], z["d_status"]), np.nonzero(st[:n] != z["d_status"])
    assert np.array_equal(io[:n], z["d_in_off"]) and np.array_equal(il[:n], z["d_in_len"])
    assert np.all(st[n:] == 0xEE) and np.all(il[n:] == 0xEEEE) and np.all(io[n:] == 2**64 - 1)
    assert torch.equal(fr, before)


def test_decap_fixed_stride(ctx, dev):
    """One outer packet per 128-byte slot at fixed_len 102 / 109 (padding)."""
    a = tungen.inner_frame(np.random.default_rng(4), 64)
    frames = [tungen.outer(a, pad=7), tungen.outer(a, gre0=0x2000, pad=7), tungen.outer(a, vlan=3, pad=3),
              tungen.outer(a, proto=17, pad=7), tungen.outer(a, badck=True, pad=7)] * 60
    n, stride = len(frames), 131
    buf = np.zeros(n * stride + 64, np.uint8)
    for i, f in enumerate(frames):
        buf[i * stride:i * stride + 109] = np.frombuffer(f, np.uint8)
    want = tungen.decap_batch(frames, np.arange(n, dtype=np.uint64) * stride)
    r = ctx.tunnel_decap_device(put(dev, buf, 5), n, stride=stride, fixed_len=109)
    torch.cuda.synchronize()
    assert np.array_equal(r["status"].cpu().numpy(), want["status"])
    assert np.array_equal(r["in_off"].cpu().numpy().view(np.uint64), want["in_off"])
    assert np.array_equal(r["in_len"].cpu().numpy().view(np.uint16), want["in_len"])


# --------------------------------------------------------------------- chains
def test_chain_encap_then_receive_transform(ctx, dev):
    """encap -> pptk_rx_batch_device on the slots with d_out_len: every DONE
    slot is a valid IPv4 packet of protocol 47 between the tunnel's
    addresses."""
    from pptk_amd.records import F_IP_OK, F_MALFORMED, F_PARSED, as_records
    z, frames, _ = fixture()
    n = len(frames)
    tun, idx = tungen.modes(n)["per"]
    g = run_encap(ctx, dev, z["frames"], n, tun, None, 3, off=z["off"], lens=z["len"])
    r = g["dev"]
    recs = ctx.batch_device(r["out"], n, lens=r["out_len"], stride=g["out_stride"], max_len=65535)
    torch.cuda.synchronize()
    rec = as_records(recs.cpu().numpy().reshape(-1))
    done = g["status"][:n] == tungen.ST_DONE
    assert done.sum() > 20
    assert np.all(rec["flags"][done] & (F_PARSED | F_IP_OK | F_MALFORMED) == F_PARSED | F_IP_OK)
    assert np.all(rec["proto"][done] == 47) and np.all(rec["l3_off"][done] == 14)
    assert np.array_equal(rec["src"][done][:, :4],
                          tun["src"][done].astype(">u4").view(np.uint8).reshape(-1, 4))
    assert np.all(rec["flags"][~done] & F_PARSED == 0)


def test_chain_decap_then_receive_transform(ctx, dev):
    """decap -> pptk_rx_batch_device with the descriptors: the records are
    byte-equal to the records of the inner frames on their own."""
    z, _, dframes = fixture()
    n = len(dframes)
    fr = put(dev, z["dframes"], 9)
    r = ctx.tunnel_decap_device(fr, n, off=i64(z["doff"], dev), lens=i16(z["dlen"], dev))
    got = ctx.batch_device(fr, n, off=r["in_off"], lens=r["in_len"], max_len=1500)
    inner = []
    for f in dframes:
        st, o, l = tungen.decap(f)
        inner.append(f[o:o + l] if st & tungen.D_OK else b"")
    assert sum(len(x) > 0 for x in inner) >= 8
    buf, off, lens = framegen.pack(inner)
    want = ctx.batch_device(put(dev, buf, 0), n, off=i64(off, dev), lens=i16(lens, dev), max_len=1500)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_chain_encap_then_fragment(ctx, dev):
    """encap (DF clear) -> pptk_ip_fragment_device at mtu 576: the fragments'
    payloads put together are the unfragmented slots' payloads."""
    z, frames, _ = fixture()
    n, mtu = len(frames), 576
    tun, _ = tungen.modes(n)["one"]
    g = run_encap(ctx, dev, z["frames"], n, tun, None, tungen.ID_BASE, off=z["off"], lens=z["len"])
    r = g["dev"]
    slots = want_fixture("one")["slots"]
    want = fraggen.fragment_batch([s or b"" for s in slots], mtu)
    cap = int(want["totals"][0])
    fr = ctx.ip_fragment_device(r["out"], n, mtu, cap, lens=r["out_len"], stride=g["out_stride"])
    torch.cuda.synchronize()
    assert tuple(fr["totals"].cpu().numpy()) == (cap, cap) and cap >= 119 + 17
    first, count = fr["first"].cpu().numpy(), fr["count"].cpu().numpy()
    out, olen = fr["out"].cpu().numpy(), fr["out_len"].cpu().numpy().view(np.uint16)
    st = fr["status"].cpu().numpy()
    assert np.array_equal(st, want["status"]) and np.array_equal(count.view(np.uint32), want["count"])
    big = 0
    for i, s in enumerate(slots):
        if s is None:
            assert st[i] == 0
        elif len(s) - 14 <= mtu:
            assert st[i] == fraggen.ST_IPV4 | fraggen.ST_FITS
        else:
            assert st[i] == fraggen.ST_IPV4 | fraggen.ST_DONE and count[i] >= 2
            parts = [bytes(out[k, 34:olen[k]]) for k in range(first[i], first[i] + count[i])]
            assert b"".join(parts) == s[34:]
            big += 1
    assert big >= 4


# ------------------------------------------------------------------ arguments
def test_rejects_bad_arguments(ctx, dev):
    from pptk_amd.rx import _dp
    L = ctx._L
    fr = torch.zeros(4096, dtype=torch.uint8, device=dev)
    out = torch.zeros(8192, dtype=torch.uint8, device=dev)
    tun = torch.from_numpy(tungen.tunnels().view(np.uint8).copy()).to(dev)
    idx = torch.zeros(4, dtype=torch.int32, device=dev)

    def call(o=out, ostr=112, t=tun, count=1, ix=None, n=4, fstride=64, flen=64, c=ctx._ctx, f=fr):
        return L.pptk_tunnel_encap_device(c, _dp(f), None, None, fstride, flen, n, _dp(t), count,
                                          _dp(ix), 0, _dp(o), ostr, None, None, None)
    assert call() == 0
    assert call(count=3, ix=idx) == 0 and call(count=3, n=3) == 0
    assert call(o=out[8:]) == -22                  # d_out not 16-byte aligned
    assert call(ostr=120) == -22                   # out_stride not a multiple of 16
    assert call(t=None) == -22 and call(count=0) == -22
    assert call(count=2) == -22 and call(count=3) == -22   # neither 1 nor n without d_idx
    assert call(t=tun[8:]) == -22                  # d_tun not 16-byte aligned
    assert call(c=None) == -22 and call(f=None) == -22 and call(o=None) == -22
    assert call(fstride=0) == -22 and call(flen=65536) == -22
    torch.cuda.synchronize()

    def dcall(n=4, fstride=128, flen=102, c=ctx._ctx, f=fr):
        return L.pptk_tunnel_decap_device(c, _dp(f), None, None, fstride, flen, n, None, None,
                                          None, None)
    assert dcall() == 0
    assert dcall(c=None) == -22 and dcall(f=None) == -22 and dcall(fstride=0) == -22
    assert dcall(flen=65536) == -22
    torch.cuda.synchronize()
    # a table built on the host is checked there: reserved and unknown flag bits
    for field, v in (("reserved", 1), ("flags", 4)):
        bad = tungen.tunnels()
        bad[field][1] = v
        with pytest.raises(OSError) as e:
            ctx.tunnel_encap_device(fr, 4, bad, idx=idx, stride=64, fixed_len=64)
        assert e.value.errno == 22
    assert tungen.tunnels().dtype == TUNNEL_DTYPE
