"""TCP sequence-space translation on the GPU (pptk_tcp_seq_translate_device)
against the reference's functions (tests/golden/seqxlate.npz) on the frames
where the reference returns, and against the per-packet host form
pptk_tcp_seq_translate_hdr on every frame -- whole buffer and status -- at
several buffer misalignments, through a flow table with "no flow" entries, in
the fixed-stride layout, on larger random batches, and, on 2^20 frames, the
property that translation keeps every TCP checksum verdict of the receive
transform.  Needs an MI355X."""
import numpy as np
import pytest

import framegen
import seqgen
from conftest import load_golden
from oracle.oracle import make_opts
from pptk_amd.records import (F_L4_OK, SEQ_ST_ACK, SEQ_ST_NOFLOW, SEQ_ST_SACK, SEQ_ST_SACK_OFF,
                              SEQ_ST_SEQ, SEQ_ST_TCP, SEQ_ST_TS, seqxlate_dtype)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KEY = bytes(range(1, 17))
WRITTEN = SEQ_ST_SEQ | SEQ_ST_ACK | SEQ_ST_SACK | SEQ_ST_TS | SEQ_ST_SACK_OFF


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ctx():
    from pptk_amd.rx import RxContext
    c = RxContext(0, KEY)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gold():
    z = load_golden("seqxlate")
    z["table"] = np.ascontiguousarray(z["table"]).view(seqxlate_dtype).reshape(-1)
    want = z["buf"].copy()
    want[z["pos"]] = z["val"]
    z["want"] = want
    return z


@pytest.fixture(scope="module")
def gold_host(ctx, gold):
    """The host form over the golden batch, once: (bytes, status)."""
    return seqgen.host_translate(ctx._L, gold["buf"], gold["off"], gold, gold["table"],
                                 gold["idx"])


def _dev_bytes(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


def _translate(ctx, buf, dev, xl, idx=None, off=None, lens=None, stride=0, fixed_len=0, shift=0,
               n=None):
    """Run the device entry on a copy of buf placed `shift` bytes into a
    zeroed allocation: (the allocation, the bytes afterwards, status)."""
    big = torch.zeros(buf.size + shift + 64, dtype=torch.uint8, device=dev)
    big[shift:shift + buf.size] = torch.from_numpy(buf).to(dev)
    frames = big[shift:]
    if n is None:
        n = len(off) if off is not None else buf.size // stride
    st = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device=dev)
    ctx.seq_translate_device(
        frames, n, _dev_bytes(xl, dev),
        idx=None if idx is None else _dev_bytes(idx.astype(np.uint32), dev),
        off=None if off is None else torch.from_numpy(off.view(np.int64)).to(dev),
        lens=None if lens is None else torch.from_numpy(lens.view(np.int16)).to(dev),
        stride=stride, fixed_len=fixed_len, status=st)
    torch.cuda.synchronize()
    return big, frames[:buf.size].cpu().numpy(), st.cpu().numpy()[:n]


def _frame_mask(z, sel):
    """Byte mask of the frames selected by the boolean array sel."""
    m = np.zeros(z["buf"].size, bool)
    for o, l in zip(z["off"][sel], z["len"][sel]):
        m[int(o):int(o) + int(l)] = True
    return m


@pytest.mark.parametrize("shift", [0, 3, 64])
def test_seq_translate_matches_golden_and_host(ctx, gold, gold_host, shift, dev):
    """Per-frame translations (xl_count = n).  The frames lie back to back
    (align 1): every chunk offset, both TCP-header address parities, and
    every frame's last chunk shared with its neighbour."""
    z = gold
    hb, hs = gold_host
    big, got, st = _translate(ctx, z["buf"], dev, z["table"][z["idx"]], off=z["off"],
                              lens=z["len"], shift=shift)
    pin = z["pinned"]
    assert np.array_equal(st[pin], z["status"][pin])
    pm = _frame_mask(z, pin)
    assert np.array_equal(got[pm], z["want"][pm]), int((got[pm] != z["want"][pm]).sum())
    assert np.array_equal(st, hs)
    assert np.array_equal(got, hb), int((got != hb).sum())
    assert int(big[:shift].sum()) == 0 and int(big[shift + z["buf"].size:].sum()) == 0


def test_seq_translate_table_mode(ctx, gold, gold_host, dev):
    """d_idx into the 16-entry table, some entries "no flow"."""
    z = gold
    hb, hs = gold_host
    idx = z["idx"].copy()
    idx[::5] = 0xFFFFFFFF
    idx[2::13] = 16            # any index >= xl_count
    none = idx >= 16
    _, got, st = _translate(ctx, z["buf"], dev, z["table"], idx=idx, off=z["off"], lens=z["len"])
    assert none.sum() > 800 and (st[none] == SEQ_ST_NOFLOW).all()
    assert np.array_equal(st[~none], hs[~none])
    nm = _frame_mask(z, none)
    assert np.array_equal(got[nm], z["buf"][nm])
    assert np.array_equal(got[~nm], hb[~nm])
    # and the whole table-mode run is the host form's
    wb, ws = seqgen.host_translate(ctx._L, z["buf"], z["off"], z, z["table"], idx)
    assert np.array_equal(st, ws) and np.array_equal(got, wb)


def test_seq_translate_fixed_stride(ctx, oracle_lib, dev):
    """128-byte slots of NOP NOP TS + SACK(2) segments, IPv4 and IPv6, one
    translation for every frame (xl_count = 1)."""
    rng = np.random.default_rng(99)
    stride, n = 128, 4096
    buf = np.zeros(n * stride, np.uint8)
    L = 0
    for i in range(n):
        opts = b"\x01\x01" + seqgen._ts(rng) + seqgen._sack(rng, 2) + b"\x01\x01"
        f = framegen.frame_tcp_opts(rng, v6=bool(i & 1), syn=False, opts=opts, payload=b"")
        buf[i * stride:i * stride + len(f)] = np.frombuffer(f, np.uint8)
        L = max(L, len(f))   # shorter frames: Ethernet padding behind the IP packet
    assert L <= stride
    recs = oracle_lib.rx_batch(buf, stride=stride, fixed_len=L, opts=make_opts(KEY))
    off = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    for xl in (seqgen.XL_TABLE[7:8], seqgen.XL_TABLE[9:10]):
        want, sw = seqgen.host_translate(ctx._L, buf, off, recs, xl)
        _, got, st = _translate(ctx, buf, dev, xl, stride=stride, fixed_len=L)
        assert (sw == (SEQ_ST_TCP | WRITTEN)).all()
        assert np.array_equal(st, sw) and np.array_equal(got, want), int((got != want).sum())


@pytest.fixture(scope="module")
def random_batch():
    return seqgen.gen(20000, seed=0xB0B)


def test_seq_translate_random_offsets(ctx, oracle_lib, random_batch, dev):
    frames, idx = random_batch
    idx = idx.copy()
    idx[::9] = 0xFFFFFFFF
    buf, off, lens = framegen.pack(frames, align=1)
    recs = oracle_lib.rx_batch(buf, off, lens, opts=make_opts(KEY))
    want, sw = seqgen.host_translate(ctx._L, buf, off, recs, seqgen.XL_TABLE, idx)
    _, got, st = _translate(ctx, buf, dev, seqgen.XL_TABLE, idx=idx, off=off, lens=lens)
    assert ((sw & WRITTEN) != 0).sum() > 8000
    assert np.array_equal(st, sw) and np.array_equal(got, want), int((got != want).sum())


def test_seq_translate_random_fixed_stride(ctx, oracle_lib, random_batch, dev):
    frames, idx = random_batch
    stride = 192
    assert max(len(f) for f in frames) <= stride
    buf = np.zeros(len(frames) * stride, np.uint8)
    for i, f in enumerate(frames):
        buf[i * stride:i * stride + len(f)] = np.frombuffer(f, np.uint8)
    recs = oracle_lib.rx_batch(buf, stride=stride, fixed_len=stride, opts=make_opts(KEY))
    off = np.arange(len(frames), dtype=np.uint64) * np.uint64(stride)
    xl = seqgen.XL_TABLE[idx]
    want, sw = seqgen.host_translate(ctx._L, buf, off, recs, xl)
    _, got, st = _translate(ctx, buf, dev, xl, stride=stride, fixed_len=stride)
    assert ((sw & WRITTEN) != 0).sum() > 8000
    assert np.array_equal(st, sw) and np.array_equal(got, want), int((got != want).sum())


def test_seq_translate_empty_and_single(ctx, oracle_lib, dev):
    rng = np.random.default_rng(3)
    f = framegen.frame_tcp_opts(rng, syn=False, opts=b"\x01\x01" + seqgen._ts(rng), payload=b"ab")
    buf, off, lens = framegen.pack([f], align=1)
    recs = oracle_lib.rx_batch(buf, off, lens, opts=make_opts(KEY))
    xl = seqgen.XL_TABLE[7:8]
    _, got, st = _translate(ctx, buf, dev, xl, off=off, lens=lens, n=0)
    assert np.array_equal(got, buf) and st.size == 0
    want, sw = seqgen.host_translate(ctx._L, buf, off, recs, xl)
    _, got, st = _translate(ctx, buf, dev, xl, stride=0, fixed_len=len(f), n=1)   # n = 1: no stride
    assert sw[0] == SEQ_ST_TCP | SEQ_ST_SEQ | SEQ_ST_ACK | SEQ_ST_TS
    assert np.array_equal(st, sw) and np.array_equal(got, want)


def test_seq_translate_keeps_verdicts_large(ctx, dev):
    """2^20 frames (a 2^16 set tiled 16 times, more than one pass of the
    grid): the receive transform's records before and after differ only on
    frames whose status reports a write, and no L4 verdict changes."""
    from pptk_amd.records import as_records
    frames, idx = seqgen.gen(1 << 16, seed=0x5151)
    buf, off, lens = framegen.pack(frames, align=1)
    rep = 16
    big = np.concatenate([buf] * rep)
    offs = np.concatenate([off + np.uint64(r * buf.size) for r in range(rep)])
    ln = np.concatenate([lens] * rep)
    ix = np.concatenate([idx] * rep)
    ix[::17] = 0xFFFFFFFF
    d = torch.from_numpy(big).to(dev)
    o = torch.from_numpy(offs.view(np.int64)).to(dev)
    l = torch.from_numpy(ln.view(np.int16)).to(dev)
    n = len(offs)

    def records():
        return as_records(ctx.batch_device(d, n, off=o, lens=l, max_len=int(ln.max()))
                          .cpu().numpy().reshape(-1))

    before = records()
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    ctx.seq_translate_device(d, n, _dev_bytes(seqgen.XL_TABLE, dev), idx=_dev_bytes(ix, dev),
                             off=o, lens=l, status=st)
    after = records()
    s = st.cpu().numpy()
    wr = (s & WRITTEN) != 0
    assert wr.sum() > 400000 and (s == SEQ_ST_NOFLOW).sum() > 60000
    assert (before["flags"] & F_L4_OK).any()
    assert np.array_equal(before["flags"], after["flags"])
    assert np.array_equal(before[~wr], after[~wr])


def test_seq_translate_rejects_bad_args(ctx, dev):
    from pptk_amd.rx import _dp
    frames = torch.zeros(256, dtype=torch.uint8, device=dev)
    xl = _dev_bytes(seqgen.XL_TABLE, dev)
    call = ctx._L.pptk_tcp_seq_translate_device
    with pytest.raises(OSError):
        ctx.seq_translate_device(frames, 2, xl[:24], stride=0)                  # no layout
    assert call(ctx._ctx, _dp(frames), None, None, 0, 64, 2, _dp(xl), 1, None, None, None) == -22
    assert call(ctx._ctx, _dp(frames), None, None, 64, 64, 2, None, 1, None, None, None) == -22
    assert call(ctx._ctx, _dp(frames), None, None, 64, 64, 2, _dp(xl), 0, None, None, None) == -22
    with pytest.raises(OSError):
        ctx.seq_translate_device(frames, 2, xl[:72], stride=64, fixed_len=64)   # 3 entries, n = 2
    assert call(ctx._ctx, _dp(frames), None, None, 64, 64, 2, _dp(xl), 16, None, None, None) == -22
    idx = torch.zeros(2, dtype=torch.int32, device=dev)
    assert call(ctx._ctx, _dp(frames), None, None, 64, 64, 2, _dp(xl), 16, _dp(idx), None,
                None) == 0                                                      # a table needs d_idx
    torch.cuda.synchronize()
