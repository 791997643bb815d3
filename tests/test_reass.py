"""Batch-local IPv4 reassembly, CPU side: the NumPy restatement of the
contract (tests/reassgen.py) against the committed fixture
(tests/golden/reass.npz), the host function pptk_ip_reass_host byte for byte
against the fixture and the restatement (bounds and -EINVAL included), the
three pins to the reference, a random mix, and a stand-alone C program that
runs the host function under -fsanitize=address,undefined.

The reference's reassctx_* cannot be run from here (the reference library of
oracle/ does not hold ipfrag/), so the restatement is pinned three ways:
(a) the records it consumes are the reference's own, (b) every reassembled
header passes the reference's ip_hdr_cksum_calc / ip_set_hdr_cksum_calc and
getters, (c) reassembly inverts the fragmenter, which is pinned to fragment4.

Fixture frames (reassgen.fixture_frames): honest fragments of the
fragmenter's restatement in order, reversed and interleaved (ihl 20 / 24 / 60,
a VLAN tag, the reserved bit); the datagram with l2 + ihl + total = 65535 in
45 shuffled fragments and one with ihl + total = 65535 (complete, TOOBIG: its
65549 bytes have no 16-bit length); five interleaved datagrams whose keys
differ only in ident, proto, dst or src; 64 and 65 eight-byte fragments; a
missing first, middle and last fragment and MF on the last; an exact
duplicate, a partial overlap, data past the last fragment and two last
fragments; leader and members with different l2 and ihl and an odd last
payload; a bad header checksum, MF with a length that is no multiple of 8, an
offset beyond 65535; whole packets, IPv6 (one with a fragment header), ARP,
a truncated frame and runts as non-fragments."""
import os
import subprocess

import numpy as np
import pytest

import fraggen
import reassgen
from conftest import ROOT, load_golden
from pptk_amd.records import REASS_DGRAM_DTYPE, REASS_HDR_DTYPE

STRIDE = 65536


@pytest.fixture(scope="module")
def fixture(oracle_lib):
    z = load_golden("reass")
    frames = [bytes(z["frames"][int(o):int(o) + int(l)]) for o, l in zip(z["off"], z["len"])]
    from oracle.oracle import make_opts
    recs = oracle_lib.rx_batch(z["frames"], z["off"], z["len"],
                               opts=make_opts(reassgen.KEY, 24, 48, 4096))
    side = oracle_lib.frag_batch(z["frames"], off=z["off"], lens=z["len"])
    return z, frames, recs, side


def slots_of(z):
    pos = np.concatenate([[0], np.cumsum(z["out_len"].astype(np.int64))])
    return [bytes(z["out"][pos[s]:pos[s + 1]]) for s in range(len(pos) - 1)]


def assert_same(got, want, n, out_cap, out_stride, report_cap):
    """A pptk_amd.rx.ip_reass_host result (0xEE-filled arrays) against a
    reassgen.reassemble result: every defined byte and every untouched one."""
    h, w = got["hdr"], want["hdr"]
    for k in REASS_HDR_DTYPE.names:
        assert int(h[k]) == int(w[k]), (k, int(h[k]), int(w[k]))
    assert np.array_equal(got["fstatus"], want["fstatus"])
    assert np.array_equal(got["dgram"], want["dgram"])
    rep = int(w["reported"])
    assert np.array_equal(got["report"][:rep].view(np.uint8),
                          want["report"][:rep].view(np.uint8))
    assert np.all(got["report"][rep:].view(np.uint8) == 0xEE)
    nw = int(w["written"])
    assert np.array_equal(got["out_len"][:nw], want["out_len"]) and np.all(got["out_len"][nw:] == 0xEEEE)
    exp = fraggen.slots(want["slots"], out_stride, out_cap)
    assert np.array_equal(got["out"].reshape(-1), exp)


def test_fixture_frames_are_the_generators(fixture):
    z, frames, _, _ = fixture
    assert frames == reassgen.fixture_frames()
    assert 200 < len(frames) < 400 and 65535 in z["out_len"]


def test_restatement_matches_fixture(fixture):
    z, frames, recs, side = fixture
    n = len(frames)
    r = reassgen.reassemble(frames, recs, side, n, n, STRIDE)
    assert r["slots"] == slots_of(z)
    assert np.array_equal(r["out_len"], z["out_len"])
    assert np.array_equal(r["report"].view(np.uint8), z["report"])
    assert np.array_equal(r["dgram"], z["dgram"]) and np.array_equal(r["fstatus"], z["fstatus"])
    assert np.array_equal(np.array([r["hdr"]]).view(np.uint64), z["hdr"])


def test_fixture_covers_the_shapes(fixture):
    """Every per-frame and per-datagram status occurs, the 64-fragment
    datagram is built and the 65-fragment one is not."""
    z, _, _, _ = fixture
    rep = z["report"].view(REASS_DGRAM_DTYPE)
    for want in (0, 0x01 | 0x02, 0x01 | 0x04, 0x01 | 0x10, 0x01 | 0x10 | 0x20):
        assert (z["fstatus"] == want).any(), hex(want)
    for want in (0x03, 0x04, 0x08, 0x10, 0x21):
        assert (rep["status"] == want).any(), hex(want)
    assert rep["status"][rep["frags"] == 64] == 0x03 and rep["status"][rep["frags"] == 65] == 0x10
    assert (rep["status"] == 0x04).sum() >= 4 and (rep["status"] == 0x08).sum() >= 4
    big = rep[rep["status"] == 0x21]
    assert len(big) == 1 and big["out_len"][0] == 0 and big["slot"][0] == reassgen.NONE


def test_host_function_matches_fixture(fixture):
    """pptk_ip_reass_host against the golden with no tolerance, records from
    the oracle's receive transform."""
    from pptk_amd.rx import ip_reass_host
    z, frames, recs, side = fixture
    n = len(frames)
    want = dict(hdr=z["hdr"].view(REASS_HDR_DTYPE)[0], fstatus=z["fstatus"], dgram=z["dgram"],
                report=z["report"].view(REASS_DGRAM_DTYPE), out_len=z["out_len"], slots=slots_of(z))
    cap = int(want["hdr"]["written"]) + 2
    got = ip_reass_host(z["frames"], recs, side, n, cap, STRIDE, off=z["off"], lens=z["len"])
    assert_same(got, want, n, cap, STRIDE, n)


@pytest.mark.parametrize("maxc,out_cap,out_stride,report_cap", [
    (1 << 24, 0, STRIDE, 0), (100, 3, STRIDE, 5), (101, 13, 1536, 1000), (1, 1, 64, 1),
    (150, 12, 3040, 24), (151, 100, 3024, 23)])
def test_host_function_matches_restatement_at_the_bounds(fixture, maxc, out_cap, out_stride,
                                                         report_cap):
    """max_candidates, out_cap, out_stride and report_cap below, at and above
    what the fixture needs: SKIPPED, NOROOM, TOOBIG and the cut report."""
    from pptk_amd.rx import ip_reass_host
    z, frames, recs, side = fixture
    n = len(frames)
    want = reassgen.reassemble(frames, recs, side, maxc, out_cap, out_stride, report_cap)
    got = ip_reass_host(z["frames"], recs, side, maxc, out_cap, out_stride, report_cap,
                        off=z["off"], lens=z["len"])
    assert_same(got, want, n, out_cap, out_stride, report_cap)


def test_bounds_cases_reach_their_statuses(fixture):
    z, frames, recs, side = fixture
    n = len(frames)
    r = reassgen.reassemble(frames, recs, side, 100, 3, 3040, 5)
    assert (r["fstatus"] & reassgen.FST_SKIPPED).any()
    assert (r["report"]["status"] & reassgen.DG_NOROOM).any()
    assert (r["report"]["status"] & reassgen.DG_TOOBIG).sum() >= 2
    assert int(r["hdr"]["written"]) == 3 and int(r["hdr"]["reported"]) == 5
    # 3000 bytes with ihl 60: round_up(14 + 3000, 16) = 3024 fits exactly, 3008 is one chunk short
    full = reassgen.reassemble(frames, recs, side, n, n, 3024)
    short = reassgen.reassemble(frames, recs, side, n, n, 3008)
    k = int(np.nonzero(full["report"]["out_len"] == 3014)[0][0])
    assert full["report"]["status"][k] == 0x03 and short["report"]["status"][k] == 0x21


def test_records_are_the_references_own(fixture, reference_lib):
    """Pin (a): the records and side records the fixture's expectations were
    made from are the reference's, and the oracle's equal them."""
    z, frames, recs, side = fixture
    _, _, _, rrecs, rside = reassgen.records(reference_lib, frames)
    assert np.array_equal(rside.view(np.uint8), side.view(np.uint8))
    for k in ("src", "dst", "proto", "flags", "ip_cksum", "l3_off"):
        assert np.array_equal(rrecs[k], recs[k]), k
    n = len(frames)
    r = reassgen.reassemble(frames, rrecs, rside, n, n, STRIDE)
    assert r["slots"] == slots_of(z)


def test_headers_pinned_to_reference(fixture, reference_lib):
    """Pin (b) with the reference's own functions."""
    assert reassgen.check_with(reference_lib, slots_of(fixture[0])) == len(fixture[0]["out_len"])


def test_headers_pinned_to_oracle(fixture, oracle_lib):
    """Pin (b) where the reference tree is absent."""
    assert reassgen.check_with(oracle_lib, slots_of(fixture[0])) == len(fixture[0]["out_len"])


@pytest.mark.parametrize("mtu", fraggen.MTUS)
def test_round_trip_inverts_the_fragmenter(oracle_lib, mtu):
    """Pin (c): for every DONE frame of fragment.npz that yields at most 64
    fragments, its fragments in a shuffled order reassemble -- restatement and
    host function -- to the first l2 + tl bytes of the frame."""
    from pptk_amd.rx import ip_reass_host
    z = load_golden("fragment")
    rng = np.random.default_rng(mtu)
    frags, want, seen = [], [], set()
    for o, l in zip(z["off"], z["len"]):
        f = bytes(z["frames"][int(o):int(o) + int(l)])
        st, fr = fraggen.fragments(f, mtu)
        if not fr or len(fr) > 64:
            continue
        l2, ihl, tl = fraggen.subject(f)
        key = (f[l2 + 12:l2 + 20], f[l2 + 9], f[l2 + 4:l2 + 6])
        if key in seen:
            continue
        seen.add(key)
        start = len(frags)
        frags += [fr[j] for j in rng.permutation(len(fr))]
        want.append((start, f[:l2 + tl]))
    assert len(want) > 30
    n = len(frags)
    buf, off, lens, recs, side = reassgen.records(oracle_lib, frags)
    r = reassgen.reassemble(frags, recs, side, n, n, STRIDE)
    assert np.all(r["report"]["status"] == 0x03) and len(r["slots"]) == len(want)
    assert [int(x) for x in r["report"]["first"]] == [s for s, _ in want]
    assert r["slots"] == [w for _, w in want]
    got = ip_reass_host(buf, recs, side, n, len(want), STRIDE, off=off, lens=lens)
    assert_same(got, r, n, len(want), STRIDE, n)


MIX_MAXC = 2020   # a few dozen of the mix's candidates are SKIPPED


@pytest.fixture(scope="module")
def mix(oracle_lib):
    frames = reassgen.random_mix(2000, 300, 0x5EA5)
    return (frames,) + reassgen.records(oracle_lib, frames)


def test_random_mix_holds_every_status(mix):
    frames, buf, off, lens, recs, side = mix
    n = len(frames)
    assert 1900 <= n <= 2400
    r = reassgen.reassemble(frames, recs, side, MIX_MAXC, 60, 2048, 150)
    st = r["report"]["status"]
    done = ((st & reassgen.DG_COMPLETE) != 0).mean()
    print("datagrams", len(st), "complete", done)
    assert 250 <= len(st) <= 330 and 0.3 <= done <= 0.7
    for bit in (reassgen.DG_COMPLETE, reassgen.DG_WRITTEN, reassgen.DG_INCOMPLETE,
                reassgen.DG_OVERLAP, reassgen.DG_TOOMANY, reassgen.DG_TOOBIG, reassgen.DG_NOROOM):
        assert (st & bit).any(), hex(bit)
    for bit in (reassgen.FST_FRAG, reassgen.FST_BADCKSUM, reassgen.FST_BADFRAG,
                reassgen.FST_SKIPPED, reassgen.FST_MEMBER, reassgen.FST_DONE):
        assert (r["fstatus"] & bit).any(), hex(bit)
    assert (r["fstatus"] == 0).any()


def test_host_function_matches_restatement_on_the_mix(mix):
    from pptk_amd.rx import ip_reass_host
    frames, buf, off, lens, recs, side = mix
    n = len(frames)
    for maxc, cap, stride, rcap in ((MIX_MAXC, 60, 2048, 150), (n, n, 4096, n)):
        want = reassgen.reassemble(frames, recs, side, maxc, cap, stride, rcap)
        got = ip_reass_host(buf, recs, side, maxc, cap, stride, rcap, off=off, lens=lens)
        assert_same(got, want, n, cap, stride, rcap)


def test_records_are_not_trusted_for_memory_safety(fixture):
    """Records that lie -- a data_len past the frame, an l3_off of 200, an
    l3_off at the frame's end -- give BADFRAG and the call reads nothing it
    must not (the sanitized program repeats this on exact-size blocks)."""
    from pptk_amd.rx import ip_reass_host
    z, frames, recs, side = fixture
    recs, side = recs.copy(), side.copy()
    idx = np.nonzero(z["fstatus"] & reassgen.FST_MEMBER)[0][:3]
    side["data_len"][idx[0]] = 60000
    recs["l3_off"][idx[1]] = 200
    n = len(frames)
    want = reassgen.reassemble(frames, recs, side, n, n, STRIDE)
    assert np.all(want["fstatus"][idx[:2]] == (reassgen.FST_FRAG | reassgen.FST_BADFRAG))
    got = ip_reass_host(z["frames"], recs, side, n, n, STRIDE, off=z["off"], lens=z["len"])
    assert_same(got, want, n, n, STRIDE, n)


def test_host_function_rejects_bad_arguments(fixture):
    from pptk_amd.rx import lib
    z, frames, recs, side = fixture
    L, n = lib(), 8
    buf = np.ascontiguousarray(z["frames"])
    off, ln = np.ascontiguousarray(z["off"]), np.ascontiguousarray(z["len"])
    r, s = np.ascontiguousarray(recs[:n]), np.ascontiguousarray(side[:n])
    raw = np.zeros(4 * 2048 + 64, np.uint8)
    out = raw[-raw.ctypes.data & 15:][:4 * 2048]
    olen, rep = np.zeros(4, np.uint16), np.zeros(8 * 16, np.uint8)
    dg, fst, hdr = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.full(6, 7, np.uint64)

    def call(**kw):
        a = dict(frames=buf.ctypes.data, off=off.ctypes.data, len=ln.ctypes.data, stride=0,
                 fixed=0, n=n, recs=r.ctypes.data, frag=s.ctypes.data, maxc=8, out=out.ctypes.data,
                 ostride=2048, ocap=4, olen=olen.ctypes.data, rep=rep.ctypes.data, rcap=8,
                 dg=dg.ctypes.data, fst=fst.ctypes.data, hdr=hdr.ctypes.data)
        a.update(kw)
        return L.pptk_ip_reass_host(*a.values())
    assert call() == 0 and hdr[0] <= 8
    for bad in (dict(hdr=None), dict(hdr=hdr.ctypes.data + 4), dict(frames=None), dict(recs=None),
                dict(frag=None), dict(dg=None), dict(fst=None), dict(out=None), dict(olen=None),
                dict(rep=None), dict(out=out.ctypes.data + 8), dict(ostride=2040),
                dict(n=(1 << 24) + 1), dict(maxc=0), dict(maxc=(1 << 24) + 1),
                dict(off=None, stride=0), dict(len=None, fixed=65536), dict(ocap=1 << 32),
                dict(rcap=1 << 32), dict(dg=dg.ctypes.data + 2)):
        assert call(**bad) == -22, bad
    hdr[:] = 7
    assert call(n=0, frames=None, recs=None, frag=None, dg=None, fst=None) == 0
    assert not hdr.any()
    assert call(out=None, olen=None, ocap=0, rep=None, rcap=0) == 0   # counting only


def test_shape_and_scratch():
    from pptk_amd.rx import ip_reass_scratch_bytes, ip_reass_shape
    assert ip_reass_shape()[0] == 64
    assert ip_reass_scratch_bytes(0, 1) == 0 and ip_reass_scratch_bytes(10, 0) == 0
    assert ip_reass_scratch_bytes((1 << 24) + 1, 1) == 0
    a, b = ip_reass_scratch_bytes(1000, 1000), ip_reass_scratch_bytes(1000, 1 << 24)
    assert a == b and a % 256 == 0 and 0 < ip_reass_scratch_bytes(1000, 10) < a


def test_sanitized_host_program(tmp_path):
    """tests/c/reass_asan.c with host/ipreass.c and host/ipcksum.c under
    ASan + UBSan, run as a program of its own."""
    exe = str(tmp_path / "reass_asan")
    src = [os.path.join(ROOT, "tests", "c", "reass_asan.c"),
           os.path.join(ROOT, "pptk_amd", "csrc", "host", "ipreass.c"),
           os.path.join(ROOT, "pptk_amd", "csrc", "host", "ipcksum.c")]
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include")] + src + ["-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "reass ok" in out.stdout, out.stdout + out.stderr
