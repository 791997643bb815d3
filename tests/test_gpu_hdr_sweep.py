"""The two in-place header kernels (pptk_tx_rewrite_device,
pptk_tcp_mss_clamp_device) over the deterministic geometry sweeps of
tests/hdrsweep.py: every base frame at every offset m within its 16-byte
chunk, crossed with absolute buffer misalignment, in offset-described and
fixed-stride layouts, with checksum corner values, without a status array,
and on a grid that takes a second grid-stride pass.  Every comparison is of
the whole buffer (gaps and guards included) and the status, byte for byte
against the oracle, which test_hdr_sweep.py checks against the live
reference on the same batches.  Needs an MI355X."""
import numpy as np
import pytest

import framegen
import hdrsweep as H

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SHIFTS = (0, 1, 8, 15)


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


_want = {}


def _expect(key, b, fn):
    """(whole expected buffer, status) of batch b under the oracle call fn,
    computed once per key."""
    if key not in _want:
        out, st = fn(b.buf[b.origin:])
        whole = b.buf.copy()
        whole[b.origin:] = out
        _want[key] = (whole, st)
    return _want[key]


def _run(b, dev, shift, launch, status=True):
    """Upload b.buf at `shift` bytes into a zeroed allocation, launch on the
    frames pointer, and return (buffer as left by the kernel, status incl.
    its guard entries); checks that nothing around the buffer was written."""
    size = b.buf.size
    big = torch.zeros(size + shift + 64, dtype=torch.uint8, device=dev)
    big[shift:shift + size] = torch.from_numpy(b.buf).to(dev)
    st = torch.full((b.n + H.ST_GUARD,), 0xEE, dtype=torch.uint8, device=dev) if status else None
    kw = dict(status=st)
    if b.off is not None:
        kw.update(off=torch.from_numpy(b.off.view(np.int64)).to(dev),
                  lens=torch.from_numpy(b.lens.view(np.int16)).to(dev))
    else:
        kw.update(stride=b.stride, fixed_len=b.fixed_len)
    launch(big[shift + b.origin:], b.n, kw)
    torch.cuda.synchronize()
    assert int(big[:shift].sum()) == 0 and int(big[shift + size:].sum()) == 0
    return big[shift:shift + size].cpu().numpy(), (st.cpu().numpy() if status else None)


def _check(got, st, want, st_want, n, what):
    if st is not None:
        assert np.array_equal(st[:n], st_want), what
        assert (st[n:] == 0xEE).all(), what
    assert np.array_equal(got, want), (what, int((got != want).sum()), np.nonzero(got != want)[0][:8])
    g = H.GUARD
    assert (got[:g] == H.FILL).all() and (got[-g:] == H.FILL).all(), what


def _rewrite(ctx, b, rw, dev, shift=0, status=True):
    rw_t = torch.from_numpy(np.ascontiguousarray(rw).view(np.uint8).copy()).to(dev)
    return _run(b, dev, shift,
                lambda fr, n, kw: ctx.tx_rewrite_device(fr, n, rw_t, **kw), status)


def _clamp(ctx, b, mss, flags, dev, shift=0):
    return _run(b, dev, shift,
                lambda fr, n, kw: ctx.mss_clamp_device(fr, n, mss, syn_only=bool(flags & 1), **kw))


# ------------------------------------------------------------------ rewrite
@pytest.mark.parametrize("shift", SHIFTS)
def test_rewrite_placed(ctx, oracle_lib, dev, shift):
    """Every base frame x m x ops; the shift moves the absolute store
    alignment and leaves m (taken from the offset) as placed."""
    b = H.rewrite_placed()
    want, sw = _expect("rw_placed", b, lambda fr: oracle_lib.rewrite_batch(fr, b.rw, **b.layout()))
    got, st = _rewrite(ctx, b, b.rw, dev, shift)
    _check(got, st, want, sw, b.n, shift)


@pytest.mark.parametrize("entries", ["one", "n"])
def test_rewrite_fixed_stride(ctx, oracle_lib, dev, entries):
    for name, b in H.rewrite_fixed():
        rw = b.rw_one if entries == "one" else b.rw
        want, sw = _expect(("rw_fixed", name, entries), b,
                           lambda fr: oracle_lib.rewrite_batch(fr, rw, **b.layout()))
        got, st = _rewrite(ctx, b, rw, dev, shift=3)
        _check(got, st, want, sw, b.n, name)


def test_rewrite_checksum_corners(ctx, oracle_lib, dev):
    b, _ = H.corners()
    want, sw = _expect("rw_corners", b, lambda fr: oracle_lib.rewrite_batch(fr, b.rw, **b.layout()))
    got, st = _rewrite(ctx, b, b.rw, dev, shift=5)
    bad = np.nonzero(st[:b.n] != sw)[0]
    assert not len(bad), b.tags[bad[:8]]
    _check(got, st, want, sw, b.n, "corners")


def test_rewrite_without_status(ctx, oracle_lib, dev):
    b = H.rewrite_placed()
    want, sw = _expect("rw_placed", b, lambda fr: oracle_lib.rewrite_batch(fr, b.rw, **b.layout()))
    got, _ = _rewrite(ctx, b, b.rw, dev, status=False)
    _check(got, None, want, sw, b.n, "d_status == NULL")


def _two_pass_n(dev):
    # the launch uses min(blocks, ncu * 8) blocks of 256 lanes: one full grid
    # and a ragged last block, so every lane's slot is used a second time
    return torch.cuda.get_device_properties(dev).multi_processor_count * 8 * 256 + 300


def test_rewrite_second_grid_pass(ctx, oracle_lib, dev):
    b = H.tile(H.rewrite_placed(), _two_pass_n(dev))
    out, sw = oracle_lib.rewrite_batch(b.buf, b.rw, **b.layout())
    got, st = _rewrite(ctx, b, b.rw, dev, shift=1)
    _check(got, st, out, sw, b.n, "second pass")


@pytest.mark.parametrize("seed", range(2))
def test_rewrite_matches_oracle_random(ctx, oracle_lib, dev, seed):
    """20 000 random frames (fuzzed headers and the CMIX mix) packed back to
    back with a random rewrite each, all six ops."""
    from tests.golden.gen_golden import random_rewrites
    b1, o1, l1 = framegen.gen_fuzz(10000, seed=0x7100 + seed)
    b2, o2, l2 = framegen.gen_cmix(10000, seed=0x7200 + seed)
    buf = np.concatenate([b1, b2])
    off = np.concatenate([o1, o2 + np.uint64(b1.size)])
    lens = np.concatenate([l1, l2])
    rw = random_rewrites(len(off), np.random.default_rng(0x7300 + seed), nops=64)
    b = H.Batch(buf, 0, len(off), off=off, lens=lens, rw=rw)
    want, sw = oracle_lib.rewrite_batch(buf, rw, off, lens)
    assert ((sw & 3) == 3).sum() > 5000
    got, st = _rewrite(ctx, b, rw, dev, shift=(0, 7)[seed])
    assert np.array_equal(st[:b.n], sw) and (st[b.n:] == 0xEE).all()
    assert np.array_equal(got, want), int((got != want).sum())


# ---------------------------------------------------------------------- MSS
def _clamp_cases():
    return [(mss, flags) for mss in H.MSS_CLAMPS for flags in (0, 1)]


@pytest.mark.parametrize("shift", SHIFTS)
def test_mss_placed(ctx, oracle_lib, dev, shift):
    b = H.mss_placed()
    for mss, flags in _clamp_cases():
        want, sw = _expect(("mss_placed", mss, flags), b,
                           lambda fr: oracle_lib.mss_clamp_batch(fr, mss, flags, **b.layout()))
        got, st = _clamp(ctx, b, mss, flags, dev, shift)
        _check(got, st, want, sw, b.n, (shift, mss, flags))


def test_mss_fixed_stride(ctx, oracle_lib, dev):
    for name, b in H.mss_fixed():
        for mss, flags in _clamp_cases():
            want, sw = _expect(("mss_fixed", name, mss, flags), b,
                               lambda fr: oracle_lib.mss_clamp_batch(fr, mss, flags, **b.layout()))
            got, st = _clamp(ctx, b, mss, flags, dev, shift=3)
            _check(got, st, want, sw, b.n, (name, mss, flags))


def test_mss_second_grid_pass(ctx, oracle_lib, dev):
    b = H.tile(H.mss_placed(), _two_pass_n(dev))
    want, sw = oracle_lib.mss_clamp_batch(b.buf, 536, 0, **b.layout())
    assert (sw & 4).sum() > b.n // 4
    got, st = _clamp(ctx, b, 536, 0, dev, shift=1)
    _check(got, st, want, sw, b.n, "second pass")
