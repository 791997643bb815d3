"""GRE tunnel encapsulation and decapsulation, CPU side: the NumPy
restatement of the contracts (tests/tungen.py) against the committed fixture
(tests/golden/tunnel.npz), the restatement pinned to the reference and to the
oracle, the per-packet host functions pptk_tunnel_encap_host /
pptk_tunnel_decap_host byte for byte against the fixture, a round trip, the
header of a C program that writes the ldptunnel.c template with the kept
setters, and a stand-alone C program that runs the host functions and the new
iphdr.h setters under -fsanitize=address,undefined.

Encap frames (tungen.encap_frames), packed back to back so that their starts
fall on every alignment: lengths 0, 13, 14, 15, 16, 17; 38 + len at every
multiple of 16 from 48 to 128, one below and one above; 60, 64, 1500, 1514,
9000; 65497 (the last that fits 16 bits), 65498 and 65535 (TOOBIG).  Three
tunnels through idx with 0xffffffff entries, one tunnel for all, one per
frame; DF set and clear; ids that count up from id_base and wrap 0xffff -> 0
between frames 10 and 11; an out_stride of 1552 that gives NOROOM to the
frames above 1514 bytes only.

Decap frames (tungen.decap_frames): valid ones plain and VLAN-tagged, ihl 24,
Ethernet padding after the outer packet, inner length 0, a bad header
checksum, proto 6 and 17 (IPV4 only), an IPv6 outer (0), MF set, offset != 0,
tl - ihl = 4 with padding and = 3 (ihl 20 and 24), l2 + tl = len + 1 (plain
and tagged), lengths 13, 37, 33 and 0, GRE with C, K, S or version 1, ptype
0x0800, and two or three faults at once."""
import os
import subprocess

import numpy as np
import pytest

import tungen
from conftest import ROOT, load_golden
from pptk_amd.records import TUNNEL_DTYPE


@pytest.fixture(scope="module")
def fixture():
    z = load_golden("tunnel")
    frames = [bytes(z["frames"][int(o):int(o) + int(l)]) for o, l in zip(z["off"], z["len"])]
    dframes = [bytes(z["dframes"][int(o):int(o) + int(l)]) for o, l in zip(z["doff"], z["dlen"])]
    return z, frames, dframes


def want_slots(z, name):
    """The fixture's slots of one mode: bytes, or None without DONE."""
    olen = z[f"{name}_out_len"].astype(np.int64)
    pos = np.concatenate([[0], np.cumsum(olen)])
    return [bytes(z[f"{name}_out"][pos[i]:pos[i + 1]]) if olen[i] else None
            for i in range(len(olen))]


def test_fixture_frames_are_the_generators(fixture):
    z, frames, dframes = fixture
    assert frames == tungen.encap_frames() and dframes == tungen.decap_frames()
    assert [len(f) for f in frames] == tungen.ENCAP_LENS
    assert np.array_equal(z["tun"].view(TUNNEL_DTYPE), tungen.tunnels())
    assert np.array_equal(z["idx"], tungen.encap_idx(len(frames)))
    assert int(z["id_base"][0]) == tungen.ID_BASE
    assert sorted({int(o) % 16 for o, l in zip(z["off"], z["len"]) if l >= 14}) == list(range(16))


@pytest.mark.parametrize("name", ["idx", "one", "per"])
def test_restatement_matches_fixture(fixture, name):
    z, frames, _ = fixture
    tun, idx = tungen.modes(len(frames))[name]
    r = tungen.encap_batch(frames, tun, idx, tungen.ID_BASE)
    assert r["slots"] == want_slots(z, name)
    for k in ("out_len", "status"):
        assert r[k].dtype == z[f"{name}_{k}"].dtype and np.array_equal(r[k], z[f"{name}_{k}"]), k
    if name == "idx":
        r = tungen.encap_batch(frames, tun, idx, tungen.ID_BASE, tungen.NR_STRIDE)
        assert np.array_equal(r["out_len"], z["nr_out_len"])
        assert np.array_equal(r["status"], z["nr_status"])
    d = tungen.decap_batch(fixture[2], z["doff"])
    for k in ("status", "in_off", "in_len"):
        assert d[k].dtype == z[f"d_{k}"].dtype and np.array_equal(d[k], z[f"d_{k}"]), k


def test_fixture_covers_the_shapes(fixture):
    z, frames, _ = fixture
    st = z["idx_status"]
    for bit in (tungen.ST_DONE, tungen.ST_RUNT, tungen.ST_TOOBIG, tungen.ST_NOFLOW):
        assert (st == bit).any(), bit
    nr = z["nr_status"]
    assert (nr == tungen.ST_NOROOM).any() and (nr == tungen.ST_NOROOM | tungen.ST_TOOBIG).any()
    assert (nr == tungen.ST_DONE).sum() > 15 and nr[tungen.ENCAP_LENS.index(1514)] == tungen.ST_DONE
    assert z["idx_out_len"].max() == 65535
    # the ids count through 0xffff -> 0 (mode 'one': frames 10 and 11)
    s = want_slots(z, "one")
    assert (s[10][18:20], s[11][18:20]) == (b"\xff\xff", b"\x00\x00")
    # DF set and clear
    assert {x[20] for x in want_slots(z, "idx") if x} == {0x40, 0x00}
    ds = set(int(x) for x in z["d_status"])
    assert {0, 0x01, 0x07, 0x09, 0x13, 0x19, 0x21, 0x31, 0x43, 0x53, 0x83, 0x93, 0xC3} <= ds


@pytest.mark.parametrize("name", ["idx", "one", "per"])
def test_restatement_pinned_to_reference(fixture, reference_lib, name):
    _check_pinned(fixture, reference_lib, name)


@pytest.mark.parametrize("name", ["idx", "one", "per"])
def test_restatement_pinned_to_oracle(fixture, oracle_lib, name):
    _check_pinned(fixture, oracle_lib, name)


def _check_pinned(fixture, lib, name):
    z, frames, _ = fixture
    n = len(frames)
    tun, idx = tungen.modes(n)[name]
    r = dict(slots=want_slots(z, name))
    want = int((z[f"{name}_status"] == tungen.ST_DONE).sum())
    assert tungen.check_with(lib, frames, r, tun, tungen.mode_idx(name, n)) == want > 15


@pytest.mark.parametrize("name", ["idx", "one", "per"])
def test_encap_host_matches_fixture(fixture, name):
    """pptk_tunnel_encap_host, frame by frame: status, length and every byte
    of an 0xEE-filled out (zeros up to the 16-byte boundary, the fill after
    it); with one byte too few NOROOM and nothing written."""
    from pptk_amd.rx import tunnel_encap_host
    z, frames, _ = fixture
    tun, idx = tungen.modes(len(frames))[name]
    slots = want_slots(z, name)
    ti = tungen.mode_idx(name, len(frames))
    for i, f in enumerate(frames):
        seq = (tungen.ID_BASE + i) & 0xFFFFFFFF
        if ti[i] == tungen.NOFLOW:
            continue   # the device call's index check; the host form takes the tunnel itself
        cap = tungen.FULL_STRIDE
        st, out, olen = tunnel_encap_host(f, tun[int(ti[i])], seq, out_cap=cap)
        assert (st, olen) == (int(z[f"{name}_status"][i]), int(z[f"{name}_out_len"][i])), i
        assert np.array_equal(out, tungen.slot_buffer([slots[i]], cap)), i
        if slots[i] is not None:
            n = len(slots[i])
            st, out, olen = tunnel_encap_host(f, tun[int(ti[i])], seq, out_cap=n - 1)
            assert (st, olen) == (tungen.ST_NOROOM, 0) and np.all(out == 0xEE)
            # out_cap = the packet's length exactly: written, no zero byte past it
            st, out, olen = tunnel_encap_host(f, tun[int(ti[i])], seq, out_cap=n)
            assert (st, olen) == (tungen.ST_DONE, n) and out.tobytes() == slots[i]


def test_encap_host_noroom_and_bad_tunnels(fixture):
    from pptk_amd.rx import tunnel_encap_host
    z, frames, _ = fixture
    t = tungen.tunnels()
    for i, f in enumerate(frames):   # the fixture's NOROOM stride as out_cap
        st, out, olen = tunnel_encap_host(f, t[0], 0, out_cap=tungen.NR_STRIDE)
        want = tungen.encap(f, t[0], 0, tungen.NR_STRIDE)
        assert st == want[0] and olen == (len(want[1]) if want[1] else 0)
        if st & tungen.ST_NOROOM:
            assert np.all(out == 0xEE)
    f = frames[tungen.ENCAP_LENS.index(64)]
    for field, v in (("reserved", 1), ("reserved", 0x80000000), ("flags", 4), ("flags", 0x103)):
        bad = t[1:2].copy()
        bad[field] = v
        st, out, olen = tunnel_encap_host(f, bad[0], 0)
        assert (st, olen) == (tungen.ST_BADTUN, 0) and np.all(out == 0xEE)
    with pytest.raises(ValueError):
        tunnel_encap_host(f, bytes(31))


def test_decap_host_matches_fixture(fixture):
    from pptk_amd.rx import tunnel_decap_host
    z, _, dframes = fixture
    for i, f in enumerate(dframes):
        st, off, ln = tunnel_decap_host(f)
        assert (st, off + int(z["doff"][i]), ln) == (int(z["d_status"][i]), int(z["d_in_off"][i]),
                                                     int(z["d_in_len"][i])), i


def test_round_trip(fixture):
    """decap(encap(f)) is f for every DONE frame of every mode; an encap of
    an encap decaps one level at a time."""
    from pptk_amd.rx import tunnel_decap_host, tunnel_encap_host
    z, frames, _ = fixture
    ok = tungen.D_IPV4 | tungen.D_GRE | tungen.D_OK
    for name in ("idx", "one", "per"):
        for f, s in zip(frames, want_slots(z, name)):
            if s is not None:
                st, off, ln = tunnel_decap_host(s)
                assert (st, off, ln) == (ok, 38, len(f)) and s[off:off + ln] == f
    t = tungen.tunnels()
    f = frames[tungen.ENCAP_LENS.index(1500)]
    st, once, n1 = tunnel_encap_host(f, t[0], 0)
    st, twice, n2 = tunnel_encap_host(once[:n1].tobytes(), t[2], 9)
    assert (st, n2) == (tungen.ST_DONE, len(f) + 76)
    st, off, ln = tunnel_decap_host(twice[:n2].tobytes())
    assert (st, off, ln) == (ok, 38, n1) and twice[off:off + ln].tobytes() == once[:n1].tobytes()
    assert tungen.decap(twice[:n2].tobytes()) == (ok, 38, n1)


def _cc(tmp_path, name, extra, flags):
    exe = str(tmp_path / name)
    src = [os.path.join(ROOT, "tests", "c", name + ".c")] + [
        os.path.join(ROOT, "pptk_amd", "csrc", "host", x) for x in extra]
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror"] + flags +
                          ["-I", os.path.join(ROOT, "include")] + src + ["-o", exe])
    return exe


def test_setter_sequence_gives_the_encap_header(tmp_path):
    """tests/c/tunnel_hdr.c writes the reference application's template with
    the kept setters; its 38 bytes are the header of pptk_tunnel_encap_host
    (and of the restatement) for the same tunnel."""
    from pptk_amd.rx import tunnel_encap_host
    exe = _cc(tmp_path, "tunnel_hdr", ["ipcksum.c"], ["-O2"])
    t = np.zeros(1, TUNNEL_DTYPE)
    t[0] = ([0x02, 0xAA, 0xBB, 0xCC, 0xDD, 0xEE], [0x02, 0x10, 0x20, 0x30, 0x40, 0x50],
            (10 << 24) | 1, (10 << 24) | 2, 0, 64, 0, 0, 0)
    rng = np.random.default_rng(3)
    for n, df, ident in ((14, 1, 0), (64, 1, 0), (1500, 0, 0xFFFF), (65497, 1, 0x1234)):
        t["id"], t["flags"] = ident, tungen.TUN_DF if df else 0
        out = subprocess.run([exe, str(n), str(df), str(ident)], capture_output=True, text=True,
                             timeout=60, check=True).stdout.strip()
        f = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        st, slot, olen = tunnel_encap_host(f, t[0], 0)
        assert st == tungen.ST_DONE
        assert bytes.fromhex(out) == slot[:38].tobytes() == tungen.header(t[0], n, 0)


def test_sanitized_host_program(tmp_path):
    """tests/c/tunnel_asan.c with host/tunnel.c and host/ipcksum.c under
    ASan + UBSan, run as a program of its own."""
    exe = _cc(tmp_path, "tunnel_asan", ["tunnel.c", "ipcksum.c"],
              ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
               "-static-libasan", "-static-libubsan"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "tunnel ok" in out.stdout, out.stdout + out.stderr
