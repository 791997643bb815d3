"""IPv4 reassembly on the GPU (pptk_ip_reass_device) against the committed
fixture (tests/golden/reass.npz), the host statement pptk_ip_reass_host and
the NumPy restatement (tests/reassgen.py): every output byte, every per-slot,
per-datagram and per-frame word, and everything the call must not touch
(slot tails, slots past the written ones, report entries past the reported
ones, guard regions) -- no tolerance.  The records every call consumes are
the ones pptk_rx_batch_device wrote for the same frames.  Needs an MI355X."""
import functools
import itertools

import numpy as np
import pytest

import fraggen
import framegen
import reassgen
from conftest import load_golden
from pptk_amd.records import REASS_DGRAM_DTYPE, REASS_HDR_DTYPE

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 4096          # bytes of 0xEE before and after the slots
FILL16, FILL32 = -4370, -286331154   # 0xEEEE, 0xEEEEEEEE
A, B = (10, 0, 0, 1), (192, 168, 0, 1)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ctx():
    from pptk_amd.rx import RxContext
    c = RxContext(0, reassgen.KEY, max_frame=65535)
    yield c
    c.close()


def place(frames, starts=None, fixed=None):
    """(buf, off, lens, layout): the frames back to back, or frame i at a
    16-byte boundary + starts[i], or (fixed = (stride, fixed_len)) at a fixed
    stride with zero padding up to fixed_len."""
    if fixed:
        stride, flen = fixed
        buf = np.zeros(len(frames) * stride + flen + 64, np.uint8)
        for i, f in enumerate(frames):
            buf[i * stride:i * stride + len(f)] = np.frombuffer(f, np.uint8)
        return buf, None, None, dict(stride=stride, fixed_len=flen)
    if starts is None:
        buf, off, lens = framegen.pack(frames)
        return buf, off, lens, {}
    off, pos = [], 0
    for f, a in zip(frames, starts):
        pos = fraggen.up16(pos) + a
        off.append(pos)
        pos += len(f)
    buf = np.zeros(pos + 64, np.uint8)
    for o, f in zip(off, frames):
        buf[o:o + len(f)] = np.frombuffer(f, np.uint8)
    return buf, np.array(off, np.uint64), np.array([len(f) for f in frames], np.uint16), {}


class Batch:
    """Frames on the device with the records the receive transform wrote."""

    def __init__(self, ctx, dev, frames, starts=None, fixed=None, shift=0, packed=None):
        if packed:   # (buf, n, fixed layout) made elsewhere
            self.buf, n, self.layout = packed
            self.off = self.lens = None
        else:
            n = len(frames)
            self.buf, self.off, self.lens, self.layout = place(frames, starts, fixed)
        self.n = n
        big = torch.zeros(self.buf.size + shift, dtype=torch.uint8, device=dev)
        big[shift:] = torch.from_numpy(self.buf).to(dev)
        self.d_buf = big[shift:]
        self.d_off = None if self.off is None else torch.from_numpy(self.off.view(np.int64)).to(dev)
        self.d_len = None if self.lens is None else torch.from_numpy(self.lens.view(np.int16)).to(dev)
        self.d_side = torch.zeros((max(n, 1), 16), dtype=torch.uint8, device=dev)
        if n:
            maxlen = int(self.lens.max()) if self.lens is not None else self.layout["fixed_len"]
            self.d_recs = ctx.batch_device(self.d_buf, n, off=self.d_off, lens=self.d_len,
                                           max_len=maxlen, frag_out=self.d_side, **self.layout)
        else:
            self.d_recs = torch.zeros((1, 64), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

    def host(self, maxc, out_cap, out_stride, report_cap, recs=None, side=None):
        from pptk_amd.rx import ip_reass_host
        recs = self.d_recs.cpu().numpy() if recs is None else recs
        side = self.d_side.cpu().numpy() if side is None else side
        return ip_reass_host(self.buf, recs, side, maxc, out_cap, out_stride, report_cap,
                             off=self.off, lens=self.lens, n=self.n, **self.layout)


def run(ctx, dev, b, maxc, out_cap, out_stride, report_cap, stream=None, d_recs=None, d_side=None):
    """One device call on 0xEE-filled outputs with guards; everything as numpy."""
    n = b.n
    torch.cuda.synchronize()   # the fills below and a caller's stream do not order themselves
    raw = torch.full((2 * GUARD + max(out_cap, 1) * out_stride,), 0xEE, dtype=torch.uint8, device=dev)
    r = ctx.ip_reass_device(
        b.d_buf, n, b.d_recs if d_recs is None else d_recs, b.d_side if d_side is None else d_side,
        maxc, out_cap, out_stride, report_cap, off=b.d_off, lens=b.d_len,
        out=raw[GUARD:GUARD + max(out_cap, 1) * out_stride],
        out_len=torch.full((out_cap + 8,), FILL16, dtype=torch.int16, device=dev),
        report=torch.full(((report_cap + 8) * 16,), 0xEE, dtype=torch.uint8, device=dev),
        dgram=torch.full((n + 8,), FILL32, dtype=torch.int32, device=dev),
        fstatus=torch.full((n + 8,), 0xEE, dtype=torch.uint8, device=dev),
        hdr=torch.full((6,), -1, dtype=torch.int64, device=dev), stream=stream,
        scratch=torch.empty(max(ctx.ip_reass_scratch_bytes(n, maxc), 256), dtype=torch.uint8,
                            device=dev), **b.layout)
    torch.cuda.synchronize()
    g = {k: r[k].cpu().numpy() for k in ("out_len", "report", "dgram", "fstatus", "hdr")}
    g["out_len"], g["dgram"] = g["out_len"].view(np.uint16), g["dgram"].view(np.uint32)
    g["hdr"] = g["hdr"].view(REASS_HDR_DTYPE)[0]
    g["raw"], g["dev"] = raw.cpu().numpy(), r
    return g


def check(g, want, n, out_cap, out_stride, report_cap):
    """Everything the call defines equals `want` (an ip_reass_host result on
    0xEE-filled arrays) and everything else still holds the fill."""
    for k in REASS_HDR_DTYPE.names:
        assert int(g["hdr"][k]) == int(want["hdr"][k]), (k, g["hdr"], want["hdr"])
    for k, fill in (("fstatus", 0xEE), ("dgram", 0xEEEEEEEE)):
        assert np.array_equal(g[k][:n], want[k]), (k, np.nonzero(g[k][:n] != want[k])[0][:8])
        assert np.all(g[k][n:] == fill), k
    assert np.array_equal(g["report"][:report_cap * 16], want["report"].view(np.uint8))
    assert np.all(g["report"][report_cap * 16:] == 0xEE)
    assert np.array_equal(g["out_len"][:out_cap], want["out_len"]) and np.all(g["out_len"][out_cap:] == 0xEEEE)
    raw = g["raw"]
    assert np.all(raw[:GUARD] == 0xEE) and np.all(raw[-GUARD:] == 0xEE)
    got, exp = raw[GUARD:GUARD + out_cap * out_stride], want["out"].reshape(-1)
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:8]


def parity(ctx, dev, frames, maxc=None, out_cap=None, out_stride=2048, report_cap=None, **kw):
    """Device against host on one batch; returns the host result."""
    b = Batch(ctx, dev, frames, **kw)
    n = b.n
    maxc, out_cap = maxc or max(n, 1), n if out_cap is None else out_cap
    report_cap = n if report_cap is None else report_cap
    want = b.host(maxc, out_cap, out_stride, report_cap)
    check(run(ctx, dev, b, maxc, out_cap, out_stride, report_cap), want, n, out_cap, out_stride,
          report_cap)
    want["rep"] = want["report"][:int(want["hdr"]["reported"])]   # the entries that were written
    want["lens"] = want["out_len"][:int(want["hdr"]["written"])]
    return want


@functools.lru_cache(maxsize=None)
def fixture():
    z = load_golden("reass")
    frames = [bytes(z["frames"][int(o):int(o) + int(l)]) for o, l in zip(z["off"], z["len"])]
    return z, frames


@pytest.mark.parametrize("shift", [0, 3])
def test_fixture_parity(ctx, dev, shift):
    """The golden, byte for byte, and the host statement on the same records."""
    z, frames = fixture()
    n = len(frames)
    b = Batch(ctx, dev, frames, shift=shift)
    cap = len(z["out_len"]) + 2
    g = run(ctx, dev, b, n, cap, 65536, n)
    check(g, b.host(n, cap, 65536, n), n, cap, 65536, n)
    assert np.array_equal(g["hdr"].reshape(1).view(np.uint64), z["hdr"])
    assert np.array_equal(g["fstatus"][:n], z["fstatus"]) and np.array_equal(g["dgram"][:n], z["dgram"])
    assert np.array_equal(g["report"][:len(z["report"])], z["report"])
    assert np.array_equal(g["out_len"][:cap - 2], z["out_len"])
    pos = np.concatenate([[0], np.cumsum(z["out_len"].astype(np.int64))])
    slots = [bytes(z["out"][pos[s]:pos[s + 1]]) for s in range(len(pos) - 1)]
    assert np.array_equal(g["raw"][GUARD:-GUARD], fraggen.slots(slots, 65536, cap))


def test_fixture_fixed_stride(ctx, dev):
    """The fixture's frames of at most 1600 bytes at an odd fixed stride (every
    start alignment) with one fixed_len: what follows a frame is padding."""
    _, frames = fixture()
    small = [f for f in frames if len(f) <= 1600]
    want = parity(ctx, dev, small, fixed=(1621, 1600), out_stride=4096)
    assert int(want["hdr"]["written"]) >= 8


def test_n_zero_and_lone_fragment(ctx, dev):
    b = Batch(ctx, dev, [])
    g = run(ctx, dev, b, 1, 2, 64, 2)
    assert not any(int(g["hdr"][k]) for k in REASS_HDR_DTYPE.names)
    assert np.all(g["raw"] == 0xEE) and np.all(g["report"] == 0xEE) and np.all(g["out_len"] == 0xEEEE)
    rng = np.random.default_rng(1)
    lone = reassgen.split(rng, 9, [24, 8])[:1]
    want = parity(ctx, dev, lone, out_stride=64)
    assert want["rep"]["status"][0] == reassgen.DG_INCOMPLETE and want["fstatus"][0] == 0x11
    whole = [reassgen.frag4(A, B, 9, 0, rng.bytes(24), False)]   # MF clear, offset 0: no fragment
    want = parity(ctx, dev, whole, out_stride=64)
    assert want["fstatus"][0] == 0 and int(want["hdr"]["dgrams"]) == 0


def test_arrival_orders(ctx, dev):
    """Two fragments in both orders and three in all six, one batch."""
    rng = np.random.default_rng(2)
    frames, ident = [], 1
    for perm in list(itertools.permutations(range(2))) + list(itertools.permutations(range(3))):
        s = reassgen.split(rng, ident, [24, 16, 13][-len(perm):], ihl=(20, 24, 60)[ident % 3])
        frames += [s[j] for j in perm]
        ident += 1
    want = parity(ctx, dev, frames, out_stride=128)
    assert np.all(want["rep"]["status"] == 0x03) and len(want["rep"]) == 8
    # the same datagrams again, every fragment of one before the next: the same slots
    again = parity(ctx, dev, sorted(frames, key=lambda f: (f[18:20], f[20:22])), out_stride=128)
    assert np.array_equal(again["out"], want["out"])


@pytest.mark.parametrize("field", ["ident", "proto", "dst"])
def test_keys_differing_in_one_field(ctx, dev, field):
    rng = np.random.default_rng(3)
    kw = {"ident": {}, "proto": dict(proto=6), "dst": dict(dst=(192, 168, 0, 2))}[field]
    one = reassgen.split(rng, 50, [16, 16, 8])
    two = reassgen.split(rng, 51 if field == "ident" else 50, [16, 16, 8], **kw)
    want = parity(ctx, dev, [x for pair in zip(one, two[::-1]) for x in pair], out_stride=96)
    assert list(want["rep"]["status"]) == [0x03, 0x03] and list(want["rep"]["frags"]) == [3, 3]


def test_64_and_65_fragments(ctx, dev):
    rng = np.random.default_rng(4)
    a, b = reassgen.split(rng, 1, [8] * 64), reassgen.split(rng, 2, [8] * 65)
    frames = [x for pair in zip(a[::-1], b) for x in pair] + [b[64]]
    want = parity(ctx, dev, frames, out_stride=560)
    assert list(want["rep"]["status"]) == [0x03, 0x10] and list(want["rep"]["frags"]) == [64, 65]
    assert want["lens"][0] == 34 + 512


def test_holes_and_overlaps(ctx, dev):
    rng = np.random.default_rng(5)
    frames = []
    for ident, drop in ((1, 0), (2, 1), (3, 2)):
        s = reassgen.split(rng, ident, [24, 24, 24])
        frames += s[:drop] + s[drop + 1:]
    s = reassgen.split(rng, 4, [16, 16, 8])
    frames += s + [s[1]]                                                   # exact duplicate
    s = reassgen.split(rng, 5, [16, 16, 8])
    frames += [s[0], reassgen.frag4(A, B, 5, 8, bytes(16), True), s[1], s[2]]   # partial overlap
    s = reassgen.split(rng, 6, [16, 8])
    frames += s + [reassgen.frag4(A, B, 6, 32, bytes(8), True)]           # data past the last
    s = reassgen.split(rng, 7, [16, 8])
    frames += s + [reassgen.frag4(A, B, 7, 16, bytes(16), False)]          # two lasts
    frames += reassgen.split(rng, 8, [16, 8])                              # and one that is fine
    want = parity(ctx, dev, frames, out_stride=128)
    assert list(want["rep"]["status"]) == [4, 4, 4, 8, 8, 8, 8, 3]


def sweep_frames():
    """start 0..15 x l2 14/18 x ihl 20/24/60 (the leader's and the others'
    differ) x payload 8/16/24/1480: one 3-fragment datagram each."""
    rng = np.random.default_rng(6)
    frames, starts, ident = [], [], 0
    for a in range(16):
        for vlan in (None, 5):
            for h, ihl in enumerate((20, 24, 60)):
                for pay in (8, 16, 24, 1480):
                    ident += 1
                    off = 0
                    for j in range(3):
                        dl = pay if j < 2 else pay - 3
                        frames.append(reassgen.frag4(
                            A, B, ident, off, rng.bytes(dl), j < 2, ihl=(20, 24, 60)[(h + j) % 3],
                            vlan=vlan if j != 1 else (None if vlan else 7)))
                        starts.append((a + 5 * j) % 16)
                        off += dl
    order = np.random.default_rng(7).permutation(len(frames))
    return [frames[j] for j in order], [starts[j] for j in order]


@pytest.mark.parametrize("layout", ["offsets", "fixed"])
def test_alignment_sweep(ctx, dev, layout):
    frames, starts = sweep_frames()
    kw = dict(starts=starts) if layout == "offsets" else dict(fixed=(1573, 1560))
    want = parity(ctx, dev, frames, out_stride=4560, **kw)
    assert len(want["rep"]) == 384 and np.all(want["rep"]["status"] == 0x03)
    assert len(set(want["lens"])) >= 12 and int(want["lens"].max()) == 18 + 60 + 4437


@pytest.mark.parametrize("maxc,out_cap,out_stride,report_cap", [
    (1 << 24, 0, 65536, 0), (100, 3, 65536, 5), (236, 13, 1536, 1000), (237, 11, 3024, 24),
    (238, 12, 3024, 24), (237, 14, 3008, 23), (1, 1, 64, 1)])
def test_bounds(ctx, dev, maxc, out_cap, out_stride, report_cap):
    """max_candidates below, at and above the fixture's candidate count (237);
    out_cap 0, one short (11) and exact (12) at stride 3024; out_stride exact
    for the 3014-byte datagram and one chunk short; report_cap 0, short, exact
    and above."""
    z, frames = fixture()
    want = parity(ctx, dev, frames, maxc, out_cap, out_stride, report_cap)
    st = want["rep"]["status"]
    assert bool((st & reassgen.DG_NOROOM).any()) == (out_cap in (0, 3, 11) and report_cap > 0)
    if maxc == 236:
        assert ((want["fstatus"] & reassgen.FST_SKIPPED) != 0).sum() == 1
    if out_stride == 3008:
        assert st[want["rep"]["out_len"] == 3014][0] == 0x21
    if out_stride == 3024:
        assert st[want["rep"]["out_len"] == 3014][0] & 0x01 and not st[want["rep"]["out_len"] == 3014][0] & 0x20


def test_fixture_candidate_count():
    assert int(fixture()[0]["hdr"][0]) == 237


def test_lying_record_is_badfrag(ctx, dev):
    """A side record whose data_len points past the frame, on the last frame
    of the buffer: BADFRAG, and the datagram stays INCOMPLETE."""
    rng = np.random.default_rng(8)
    frames = reassgen.split(rng, 1, [16, 16]) + reassgen.split(rng, 2, [24, 9])
    b = Batch(ctx, dev, frames)
    side = b.d_side.cpu().numpy().copy()
    side.view(np.uint16).reshape(-1, 8)[3, 3] = 60000
    recs = b.d_recs.cpu().numpy().copy()
    recs.reshape(-1, 64)[1, 52] = 200
    want = b.host(4, 4, 128, 4, recs=recs, side=side)
    assert list(want["fstatus"]) == [0x11, 0x05, 0x11, 0x05]
    g = run(ctx, dev, b, 4, 4, 128, 4, d_recs=torch.from_numpy(recs).to(dev),
            d_side=torch.from_numpy(side).to(dev))
    check(g, want, 4, 4, 128, 4)


def test_determinism_and_second_stream(ctx, dev):
    frames = reassgen.random_mix(2000, 300, 0x5EA5)
    b = Batch(ctx, dev, frames)
    n = b.n
    want = b.host(2020, 60, 2048, 150)
    first = run(ctx, dev, b, 2020, 60, 2048, 150)
    check(first, want, n, 60, 2048, 150)
    second = run(ctx, dev, b, 2020, 60, 2048, 150)
    other = run(ctx, dev, b, 2020, 60, 2048, 150, stream=torch.cuda.Stream(dev))
    for g in (second, other):
        for k in ("raw", "out_len", "report", "dgram", "fstatus"):
            assert np.array_equal(g[k], first[k]), k
        assert g["hdr"] == first["hdr"]
    assert other["dev"]["scratch"].data_ptr() != first["dev"]["scratch"].data_ptr()


def tiny_fragments(ndg, seed):
    """ndg datagrams of 64 eight-byte fragments, built with NumPy, shuffled
    over the whole batch, about one frame in a hundred dropped."""
    rng = np.random.default_rng(seed)
    n = ndg * 64
    d, j = np.repeat(np.arange(ndg), 64), np.tile(np.arange(64), ndg)
    f = np.zeros((n, 42), np.uint8)
    f[:, 0], f[:, 6], f[:, 5], f[:, 11] = 2, 2, 1, 2
    f[:, 12], f[:, 14], f[:, 17], f[:, 22], f[:, 23] = 8, 0x45, 28, 64, 17
    f[:, 18], f[:, 19] = d >> 8, d & 255
    fw = j | np.where(j < 63, 0x2000, 0)
    f[:, 20], f[:, 21] = fw >> 8, fw & 255
    f[:, 26:34] = (10, 0, 0, 1, 192, 168, 0, 1)
    f[:, 34:] = rng.integers(0, 256, (n, 8), dtype=np.uint8)
    s = (f[:, 14:34:2].astype(np.uint32) << 8 | f[:, 15:34:2]).sum(axis=1)
    s = (s & 0xFFFF) + (s >> 16)
    s = ~((s & 0xFFFF) + (s >> 16)) & 0xFFFF
    f[:, 24], f[:, 25] = s >> 8, s & 255
    keep = rng.permutation(n)[:n - n // 100]
    return f[keep]


def test_more_than_one_scan_round(ctx, dev):
    """About 270 000 candidates of 4250 datagrams: the frame blocks and the
    candidate blocks exceed one round (1024 counts) of the single-workgroup
    scans, the datagrams fill several blocks, and the members of a datagram
    lie far apart."""
    f = tiny_fragments(4250, 9)
    n = len(f)
    assert n > 1024 * 256
    b = Batch(ctx, dev, None, packed=(np.concatenate([f.reshape(-1), np.zeros(64, np.uint8)]), n,
                                      dict(stride=42, fixed_len=42)))
    cap = 2300
    want = b.host(n - 1000, cap, 560, 4250)
    assert int(want["hdr"]["considered"]) == n - 1000 and 1500 < int(want["hdr"]["written"]) < cap
    check(run(ctx, dev, b, n - 1000, cap, 560, 4250), want, n, cap, 560, 4250)


def test_round_trip_on_the_device(ctx, dev):
    """frames -> encap -> fragment (mtu 576) -> a fixed shuffle -> rx with
    d_frag -> reassembly -> rx on the slots -> decap: the original frames,
    and every inner record equals the direct one."""
    from pptk_amd.records import DECAP_ST_OK, TUNNEL_DTYPE, as_records
    rng = np.random.default_rng(10)
    frames = [framegen.frame_v4(rng, (6, 17)[i & 1], 800 + 13 * i, vlan=3 if i % 5 == 0 else None)
              for i in range(48)]
    n = len(frames)
    buf, off, lens = framegen.pack(frames)
    d_buf = torch.from_numpy(buf).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    d_len = torch.from_numpy(lens.view(np.int16)).to(dev)
    direct = ctx.batch_device(d_buf, n, off=d_off, lens=d_len, max_len=int(lens.max()))
    tun = np.zeros(1, TUNNEL_DTYPE)
    tun["eth_dst"], tun["eth_src"] = (2, 0, 0, 0, 0, 9), (2, 0, 0, 0, 0, 8)
    tun["src"], tun["dst"], tun["ttl"], tun["id"], tun["flags"] = 0x0A000001, 0x0A000002, 64, 100, 2
    e = ctx.tunnel_encap_device(d_buf, n, tun, off=d_off, lens=d_len, out_stride=1536)
    fr = ctx.ip_fragment_device(e["out"], n, 576, 4 * n, lens=e["out_len"], stride=1536)
    torch.cuda.synchronize()
    total = int(fr["totals"][1].item())
    assert int(fr["totals"][0].item()) == total and total >= 2 * n
    perm = torch.from_numpy(np.random.default_rng(11).permutation(total)).to(dev)
    s_off = (perm * fr["out_stride"]).to(torch.int64)
    s_len = fr["out_len"][:total][perm].contiguous()
    side = torch.zeros((total, 16), dtype=torch.uint8, device=dev)
    recs = ctx.batch_device(fr["out"], total, off=s_off, lens=s_len, max_len=608, frag_out=side)
    r = ctx.ip_reass_device(fr["out"], total, recs, side, total, n, 1536, off=s_off, lens=s_len)
    torch.cuda.synchronize()
    hdr = r["hdr"].cpu().numpy().view(REASS_HDR_DTYPE)[0]
    assert int(hdr["dgrams"]) == int(hdr["written"]) == n
    rep = r["report"].cpu().numpy().view(REASS_DGRAM_DTYPE)[:n]
    assert np.all(rep["status"] == 0x03)
    assert np.all(r["fstatus"].cpu().numpy()[:total] == 0x31)
    outer = ctx.batch_device(r["out"], n, lens=r["out_len"], stride=1536, max_len=1536)
    d = ctx.tunnel_decap_device(r["out"], n, lens=r["out_len"], stride=1536)
    inner = ctx.batch_device(r["out"], n, off=d["in_off"], lens=d["in_len"], max_len=1536)
    torch.cuda.synchronize()
    assert np.all(d["status"].cpu().numpy() & DECAP_ST_OK)
    o = as_records(outer.cpu().numpy().reshape(-1))
    assert np.all(o["flags"] & 0x3 == 0x3) and not np.any(o["flags"] & 0x140)
    # slot k holds the datagram whose first fragment came first: tunnel id 100 + frame
    out = r["out"].cpu().numpy()
    in_off, in_len = d["in_off"].cpu().numpy(), d["in_len"].cpu().numpy().view(np.uint16)
    src = (out[:, 18].astype(int) << 8 | out[:, 19]) - 100
    assert sorted(src) == list(range(n))
    got, want = as_records(inner.cpu().numpy().reshape(-1)), as_records(direct.cpu().numpy().reshape(-1))
    for k in range(n):
        i = int(src[k])
        assert in_len[k] == lens[i]
        assert bytes(out.reshape(-1)[int(in_off[k]):int(in_off[k]) + int(in_len[k])]) == frames[i], i
        assert got[k].tobytes() == want[i].tobytes(), i


def test_rejects_bad_arguments(ctx, dev):
    from pptk_amd.rx import _dp
    L = ctx._L
    fr = torch.zeros(4096, dtype=torch.uint8, device=dev)
    recs = torch.zeros(4 * 64, dtype=torch.uint8, device=dev)
    side = torch.zeros(4 * 16, dtype=torch.uint8, device=dev)
    out = torch.zeros(4 * 256, dtype=torch.uint8, device=dev)
    olen = torch.zeros(4, dtype=torch.int16, device=dev)
    rep = torch.zeros(64, dtype=torch.uint8, device=dev)
    dg = torch.zeros(4, dtype=torch.int32, device=dev)
    fst = torch.zeros(4, dtype=torch.uint8, device=dev)
    hdr = torch.full((6,), -1, dtype=torch.int64, device=dev)
    need = L.pptk_ip_reass_scratch_bytes(4, 4)
    sc = torch.zeros(need + 256, dtype=torch.uint8, device=dev)

    def call(c=ctx._ctx, frames=fr, n=4, r=recs, s=side, maxc=4, o=out, stride=256, cap=4,
             ol=olen, rp=rep, rcap=4, d=dg, f=fst, h=hdr, scratch=sc, sb=need, fstride=64):
        return L.pptk_ip_reass_device(c, _dp(frames), None, None, fstride, 64, n, _dp(r), _dp(s),
                                      maxc, _dp(o), stride, cap, _dp(ol), _dp(rp), rcap, _dp(d),
                                      _dp(f), _dp(h), _dp(scratch), sb, None)
    assert call() == 0
    torch.cuda.synchronize()
    assert not hdr.cpu().numpy().any()             # four zero records: no fragment
    for bad in (dict(c=None), dict(h=None), dict(frames=None), dict(r=None), dict(s=None),
                dict(d=None), dict(f=None), dict(o=None), dict(ol=None), dict(rp=None),
                dict(o=out[8:]), dict(stride=250), dict(n=(1 << 24) + 1), dict(maxc=0),
                dict(maxc=(1 << 24) + 1), dict(scratch=None), dict(scratch=sc[16:]),
                dict(sb=need - 1), dict(fstride=0), dict(h=hdr.view(torch.uint8)[4:]),
                dict(r=recs[8:]), dict(cap=1 << 32), dict(rcap=1 << 32)):
        assert call(**bad) == -22, list(bad)
    hdr.fill_(-1)
    assert call(n=0, frames=None, r=None, s=None, d=None, f=None, scratch=None, sb=0) == 0
    torch.cuda.synchronize()
    assert not hdr.cpu().numpy().any()
    assert call(o=None, ol=None, cap=0, rp=None, rcap=0) == 0   # counting only
    torch.cuda.synchronize()
