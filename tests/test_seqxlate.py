"""TCP sequence-space translation, CPU side: the per-packet host form
pptk_tcp_seq_translate_hdr against the reference's functions
(tests/golden/seqxlate.npz, made by tests/golden/gen_seqxlate_golden.py), the
fixture's coverage stated as counts, the frames on which the reference never
returns (the checksum verdict is kept, nothing outside the TCP header
changes), a fresh batch against the live reference where it is built, and
the host form under ASan + UBSan as a program of its own."""
import os
import subprocess

import numpy as np
import pytest

import framegen
import seqgen
from conftest import ROOT, load_golden
from oracle.oracle import make_opts
from pptk_amd.records import (F_L4_OK, SEQ_ACK, SEQ_SACK, SEQ_SACK_OFF, SEQ_SEQ, SEQ_ST_ACK,
                              SEQ_ST_BADOPT, SEQ_ST_NOFLOW, SEQ_ST_SACK, SEQ_ST_SACK_OFF,
                              SEQ_ST_SEQ, SEQ_ST_TCP, SEQ_ST_TS, SEQ_TSECHO, SEQ_TSVAL,
                              seqxlate_dtype)

KEY = bytes(range(1, 17))


@pytest.fixture(scope="module")
def lib():
    from pptk_amd import rx
    return rx.lib()


@pytest.fixture(scope="module")
def gold():
    z = load_golden("seqxlate")
    z["table"] = np.ascontiguousarray(z["table"]).view(seqxlate_dtype).reshape(-1)
    want = z["buf"].copy()
    want[z["pos"]] = z["val"]
    z["want"] = want
    return z


@pytest.fixture(scope="module")
def host(lib, gold):
    """The host form over the whole golden batch, once: (bytes, status)."""
    return seqgen.host_translate(lib, gold["buf"], gold["off"], gold, gold["table"], gold["idx"])


def _frame_ranges(z):
    off = z["off"].astype(np.int64)
    return off, off + z["len"].astype(np.int64)


def _changed_frames(a, b, z):
    """Mask of the frames in which buffers a and b differ."""
    lo, hi = _frame_ranges(z)
    c = np.concatenate([[0], np.cumsum(a != b)])
    return c[hi] - c[lo] > 0


def test_fixture_is_the_generators(gold):
    frames, idx = seqgen.fixture()
    buf, off, lens = framegen.pack(frames, align=1)
    assert np.array_equal(buf, gold["buf"]) and np.array_equal(off, gold["off"])
    assert np.array_equal(lens, gold["len"]) and np.array_equal(idx, gold["idx"])
    assert np.array_equal(seqgen.XL_TABLE, gold["table"])


def test_host_matches_golden(gold, host, oracle_lib):
    got, st = host
    pin = gold["pinned"]
    assert np.array_equal(st[pin], gold["status"][pin])
    bad = _changed_frames(got, gold["want"], gold) & pin
    assert not bad.any(), np.nonzero(bad)[0][:10]
    # nothing between or behind the frames
    lo, hi = _frame_ranges(gold)
    inside = np.zeros(gold["buf"].size + 1, np.int64)
    np.add.at(inside, lo, 1)
    np.add.at(inside, hi, -1)
    outside = np.cumsum(inside)[:-1] == 0
    assert np.array_equal(got[outside], gold["buf"][outside])
    # the golden's frame geometry is the restated oracle's too
    recs = oracle_lib.rx_batch(gold["buf"], gold["off"], gold["len"], opts=make_opts(KEY))
    subj = seqgen.is_subject(recs)
    assert np.array_equal(subj, gold["subject"])
    assert np.array_equal(recs["l4_off"][subj], gold["l4_off"][subj])
    assert np.array_equal(recs["l4_len"][subj], gold["l4_len"][subj])


def test_fixture_coverage(gold, host):
    """What the fixture exercises, as counts (lower bounds asserted)."""
    _, st = host
    z = gold
    n = len(z["off"])
    ops = z["table"]["ops"][z["idx"]]
    counts = {}
    for name, bit in (("TCP", SEQ_ST_TCP), ("SEQ", SEQ_ST_SEQ), ("ACK", SEQ_ST_ACK),
                      ("SACK", SEQ_ST_SACK), ("TS", SEQ_ST_TS), ("SACK_OFF", SEQ_ST_SACK_OFF),
                      ("BADOPT", SEQ_ST_BADOPT)):
        counts["st_" + name] = int(((st & bit) != 0).sum())
    assert counts["st_TCP"] > 2500 and counts["st_BADOPT"] >= 40
    assert min(counts["st_" + k] for k in ("SEQ", "ACK", "SACK", "TS", "SACK_OFF")) > 300
    assert int((st == 0).sum()) >= 200            # UDP, fragments, not IP: not subjects
    assert not (st & SEQ_ST_NOFLOW).any()         # (table mode: test_no_flow_entries)
    tcp = (st & SEQ_ST_TCP) != 0
    for name, bit in (("SEQ", SEQ_SEQ), ("ACK", SEQ_ACK), ("SACK", SEQ_SACK), ("TSVAL", SEQ_TSVAL),
                      ("TSECHO", SEQ_TSECHO), ("SACK_OFF", SEQ_SACK_OFF)):
        counts["op_" + name] = int((tcp & ((ops & bit) != 0)).sum())
        assert counts["op_" + name] > 800, counts
    assert int((tcp & (ops == 0)).sum()) > 100
    # the ACK guard: ACK asked for on a segment without the flag
    assert int((tcp & ((ops & SEQ_ACK) != 0) & ((st & SEQ_ST_ACK) == 0)).sum()) >= 30
    sack = np.zeros((2, 5), int)      # [odd offset][blocks], SACK op applied
    ts = np.zeros(4, int)             # timestamp option offset mod 4, a TS op applied
    two = rare_any = rare_here = past = 0
    for i in np.nonzero(tcp)[0]:
        t0 = int(z["off"][i]) + int(z["l4_off"][i])
        end = (int(z["buf"][t0 + 12]) >> 4) * 4
        t = bytes(z["buf"][t0:t0 + end])
        _, sackoff, sacklen, tsoff = framegen.sack_ts_walk(t)
        first, firstlen = seqgen.first_sack(t)
        o = int(ops[i])
        if (o & SEQ_SACK) and sackoff and (sacklen - 2) % 8 == 0 and 2 <= sacklen <= 34:
            sack[sackoff & 1][(sacklen - 2) // 8] += 1
        if (o & (SEQ_TSVAL | SEQ_TSECHO)) and tsoff:
            ts[tsoff & 3] += 1
        if (o & SEQ_SACK) and (o & SEQ_SACK_OFF) and first and first != sackoff:
            two += 1
        rare_any += 15 + int(z["l4_off"][i]) + end > 128
        rare_here += int(z["off"][i]) % 16 + int(z["l4_off"][i]) + end > 128
        # tcp_disable_sack_cksum_update on an odd-length option at an odd
        # offset that ends with the header, in a segment without payload: the
        # straddling word's far byte is past the frame
        if (o & SEQ_SACK_OFF) and first & 1 and firstlen & 1 and first + firstlen == end \
                and int(z["l4_off"][i]) + end == int(z["len"][i]):
            past += 1
    counts.update(sack_even=sack[0].tolist(), sack_odd=sack[1].tolist(), ts_align=ts.tolist(),
                  first_ne_last=two, rare_any=rare_any, rare_here=rare_here, straddle_past=past,
                  unpinned=int((~z["pinned"]).sum()), frames=n)
    print(counts)
    # by construction: one shape per (parity, blocks) / alignment, 5 frame
    # variants, 5 translations with SACK and 9 with a timestamp op
    assert sack.min() >= 25, counts
    assert ts.min() >= 45, counts
    assert two >= 30 and rare_any >= 300 and rare_here >= 100 and past >= 5, counts
    assert 0 < counts["unpinned"] <= 0.10 * n, counts
    # the pinned mask is seqgen.pinned's
    for i in np.nonzero(~z["pinned"])[0]:
        t0 = int(z["off"][i]) + int(z["l4_off"][i])
        assert not seqgen.pinned(bytes(z["buf"][t0:t0 + 60]), int(ops[i]))


def test_unpinned_frames_keep_verdict(gold, host, oracle_lib):
    """Where the reference never returns, the host form still leaves a
    segment whose checksum verdict is the one it had, and changes nothing
    outside [l4_off, l4_off + data offset) -- on every frame."""
    got, st = host
    o = make_opts(KEY)
    before = oracle_lib.rx_batch(gold["buf"], gold["off"], gold["len"], opts=o)
    after = oracle_lib.rx_batch(got, gold["off"], gold["len"], opts=o)
    assert np.array_equal(before["flags"], after["flags"])
    assert ((before["flags"][~gold["pinned"]] & F_L4_OK) != 0).all()
    keep = np.ones(got.size, bool)
    for i in np.nonzero((st & SEQ_ST_TCP) != 0)[0]:
        t0 = int(gold["off"][i]) + int(gold["l4_off"][i])
        keep[t0:t0 + (int(gold["buf"][t0 + 12]) >> 4) * 4] = False
    assert np.array_equal(got[keep], gold["buf"][keep])
    changed = _changed_frames(got, gold["buf"], gold)
    assert (changed & ~gold["pinned"]).sum() > 100


def test_no_flow_entries(lib, gold):
    idx = gold["idx"].copy()
    idx[::7] = 0xFFFFFFFF
    idx[3::11] = 16
    got, st = seqgen.host_translate(lib, gold["buf"], gold["off"], gold, gold["table"], idx)
    none = idx >= 16
    assert (st[none] == SEQ_ST_NOFLOW).all() and not (st[~none] & SEQ_ST_NOFLOW).any()
    assert not (_changed_frames(got, gold["buf"], gold) & none).any()


def test_python_wrapper(lib):
    from pptk_amd import rx
    rng = np.random.default_rng(5)
    opts = b"\x01\x01" + b"\x08\x0a" + bytes(range(8))
    seg = bytearray(framegen.tcp_hdr(1, 2, 0xFFFFFFFF, 7, flags=0x10, opts=opts) + b"xy")
    seg[16:18] = bytes(rng.integers(0, 256, 2, dtype=np.uint8))
    x = seqgen.XL_TABLE[7:8]
    st, out = rx.tcp_seq_translate_hdr(bytes(seg), x)
    assert st == SEQ_ST_TCP | SEQ_ST_SEQ | SEQ_ST_ACK | SEQ_ST_TS
    assert int.from_bytes(out[4:8], "big") == (0xFFFFFFFF + 0xDEADBEEF) & 0xFFFFFFFF
    assert int.from_bytes(out[8:12], "big") == 7 + 0x01020304
    assert out[32:] == b"xy" and len(out) == len(seg)
    # the segment must hold the data offset; shorter ones are BADOPT, untouched
    for cut in (0, 12, 19, 31):
        st, out = rx.tcp_seq_translate_hdr(bytes(seg[:cut]), x)
        assert st == SEQ_ST_BADOPT and out == bytes(seg[:cut])
    with pytest.raises(ValueError):
        rx.tcp_seq_translate_hdr(bytes(seg), b"\0" * 23)


def test_fresh_batch_matches_live_reference(lib, reference_lib):
    frames, idx = seqgen.gen(3000, seed=0xA11CE)
    buf, off, lens = framegen.pack(frames, align=1)
    recs = reference_lib.rx_batch(buf, off, lens, opts=make_opts(KEY))
    want, sw, pin = seqgen.reference_translate(reference_lib, buf, off, recs, seqgen.XL_TABLE, idx)
    got, st = seqgen.host_translate(lib, buf, off, recs, seqgen.XL_TABLE, idx)
    assert pin.mean() > 0.85 and (~pin).any()
    assert np.array_equal(st[pin], sw[pin])
    z = dict(off=off, len=lens)
    assert not (_changed_frames(got, want, z) & pin).any()
    assert _changed_frames(got, buf, z).sum() > 1500


def test_sanitized_host_program(tmp_path):
    """tests/c/tcpseq_asan.c with host/tcpseq.c and host/tcpopt.c under ASan
    + UBSan, run as a program of its own: segments of exactly seglen heap
    bytes."""
    exe = str(tmp_path / "tcpseq_asan")
    src = [os.path.join(ROOT, "tests", "c", "tcpseq_asan.c"),
           os.path.join(ROOT, "pptk_amd", "csrc", "host", "tcpseq.c"),
           os.path.join(ROOT, "pptk_amd", "csrc", "host", "tcpopt.c")]
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include")] + src + ["-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "tcpseq ok" in out.stdout, out.stdout + out.stderr
