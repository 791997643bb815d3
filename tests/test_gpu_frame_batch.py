"""The frame-batch arguments (d_frames, d_off, d_len, stride, fixed_len, n) of
the nine entry points that take one, checked alike: header rewrite, rewrite
by flow, MSS clamp, sequence translation, fragmentation, GRE encap and decap,
reassembly and pptk_rx_batch_device.  All of them share one predicate
(rx_internal.h frame_batch_ok); this file keeps them from drifting apart.
Two 64-byte frames and otherwise valid arguments.  Needs an MI355X."""
import ctypes

import numpy as np
import pytest

import framegen

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EINVAL = -22
OPS = ("rewrite", "rewrite_flow", "mss_clamp", "seq_translate", "fragment", "encap", "decap",
       "reass", "rx_batch")


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


@pytest.fixture(scope="module")
def callers(ctx, dev):
    """op name -> call(frames, stride, fixed_len, n) with no d_off and no d_len;
    `frames` is a device tensor or None.  Everything else is valid for n <= 2."""
    from pptk_amd.rx import RxDevBatch, _dp
    L, c = ctx._L, ctx._ctx

    def z(nbytes, dtype=torch.uint8):
        return torch.zeros(nbytes, dtype=dtype, device=dev)

    status, idx = z(2), z(2, torch.int32)
    rw, xl, tun = z(16), z(24), z(32)
    out, out_len, words = z(4 * 608), z(4, torch.int16), [z(4, torch.int32) for _ in range(3)]
    totals, in_off = z(2, torch.int64), z(2, torch.int64)
    frag_sc = z(L.pptk_ip_fragment_scratch_bytes(2))
    recs, side, report, hdr = z(2 * 64), z(2 * 16), z(2 * 16), z(6, torch.int64)
    reass_need = L.pptk_ip_reass_scratch_bytes(2, 2)
    reass_sc = z(reass_need)
    keep = [status, idx, rw, xl, tun, out, out_len, words, totals, in_off, frag_sc, recs, side,
            report, hdr, reass_sc]

    def rx_batch(f, stride, fixed_len, n):
        b = RxDevBatch(d_frames=_dp(f), stride=stride, fixed_len=fixed_len, n=n,
                       d_recs=_dp(recs))
        return L.pptk_rx_batch_device(c, ctypes.byref(b), None)

    calls = {
        "rewrite": lambda f, stride, fixed_len, n: L.pptk_tx_rewrite_device(
            c, _dp(f), None, None, stride, fixed_len, n, _dp(rw), 1, _dp(status), None),
        "rewrite_flow": lambda f, stride, fixed_len, n: L.pptk_tx_rewrite_flow_device(
            c, _dp(f), None, None, stride, fixed_len, n, _dp(rw), 1, _dp(idx), _dp(status), None),
        "mss_clamp": lambda f, stride, fixed_len, n: L.pptk_tcp_mss_clamp_device(
            c, _dp(f), None, None, stride, fixed_len, n, 1400, 0, _dp(status), None),
        "seq_translate": lambda f, stride, fixed_len, n: L.pptk_tcp_seq_translate_device(
            c, _dp(f), None, None, stride, fixed_len, n, _dp(xl), 1, None, _dp(status), None),
        "fragment": lambda f, stride, fixed_len, n: L.pptk_ip_fragment_device(
            c, _dp(f), None, None, stride, fixed_len, n, 576, _dp(out), 608, 4, _dp(out_len),
            _dp(words[0]), _dp(words[1]), _dp(words[2]), _dp(status), _dp(totals), _dp(frag_sc),
            None),
        "encap": lambda f, stride, fixed_len, n: L.pptk_tunnel_encap_device(
            c, _dp(f), None, None, stride, fixed_len, n, _dp(tun), 1, None, 0, _dp(out), 112,
            _dp(out_len), _dp(status), None),
        "decap": lambda f, stride, fixed_len, n: L.pptk_tunnel_decap_device(
            c, _dp(f), None, None, stride, fixed_len, n, _dp(in_off), _dp(out_len), _dp(status),
            None),
        "reass": lambda f, stride, fixed_len, n: L.pptk_ip_reass_device(
            c, _dp(f), None, None, stride, fixed_len, n, _dp(recs), _dp(side), 2, _dp(out), 608,
            2, _dp(out_len), _dp(report), 2, _dp(words[0]), _dp(status), _dp(hdr), _dp(reass_sc),
            reass_need, None),
        "rx_batch": rx_batch,
    }
    assert set(calls) == set(OPS)
    yield calls
    del keep


@pytest.fixture(scope="module")
def frames(dev):
    two = [framegen.frame_v4(np.random.default_rng(k), 6, 64) for k in range(2)]
    buf = np.zeros(4096, np.uint8)   # room behind the frames for whole-chunk reads
    buf[:128] = np.frombuffer(b"".join(two), np.uint8)
    return torch.from_numpy(buf).to(dev)


@pytest.mark.parametrize("op", OPS)
def test_frame_batch_arguments(callers, frames, op):
    call = callers[op]
    assert call(frames, 64, 64, 2) == 0                 # the valid call the others vary
    torch.cuda.synchronize()
    assert call(None, 64, 64, 2) == EINVAL              # no frames
    assert call(frames, 0, 64, 2) == EINVAL             # two frames, no d_off, no stride
    assert call(frames, 64, 65536, 2) == EINVAL         # no d_len and a length past 16 bits
    assert call(frames, 0, 64, 1) == 0                  # one frame needs no stride
    torch.cuda.synchronize()
    assert call(frames, 64, 64, 0) == 0                 # an empty batch
    torch.cuda.synchronize()
