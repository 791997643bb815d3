"""IPv4 fragmentation to an egress MTU, CPU side: the NumPy restatement of
the contract (tests/fraggen.py) against the committed fixture
(tests/golden/fragment.npz), the restatement pinned to the reference and to
the oracle through their ip_set_hdr_cksum_calc and header getters, payload
reassembly, the per-packet host function pptk_ip_fragment_host byte for byte
against the fixture (NOROOM and -EINVAL included), and a stand-alone C
program that runs the host function and the new iphdr.h setters under
-fsanitize=address,undefined.

Fixture frames (fraggen.fixture_frames), DF clear unless said: tl = mtu and
mtu + 1 and datamax = k * per + {0, 1, 7, 8} for mtu 68 / 576 / 1280 / 1500;
ihl 20 / 24 / 40 / 60 (mtu 68 with ihl 60 leaves 8 bytes per fragment: a
1500-byte packet gives 180); a 9000-byte frame and one with tl = 65521; a
VLAN tag; odd lengths; Ethernet padding of 1..15 bytes; DF set, MF only,
offset only, a bad header checksum (too big: verdicts, nothing emitted; small
enough: FITS), the reserved bit (kept in every fragment); IPv6, ARP, a
truncated frame, runts and a 0-byte frame as non-subjects."""
import os
import subprocess

import numpy as np
import pytest

import fraggen
from conftest import ROOT, load_golden

KEYS = ("out_len", "out_src", "first", "count", "status", "totals")


@pytest.fixture(scope="module")
def fixture():
    z = load_golden("fragment")
    frames = [bytes(z["frames"][int(o):int(o) + int(l)]) for o, l in zip(z["off"], z["len"])]
    return z, frames


@pytest.fixture(scope="module")
def restated(fixture):
    _, frames = fixture
    return {mtu: fraggen.fragment_batch(frames, mtu) for mtu in fraggen.MTUS}


def test_fixture_frames_are_the_generators(fixture):
    z, frames = fixture
    assert frames == fraggen.fixture_frames()
    assert tuple(z["mtus"]) == fraggen.MTUS


@pytest.mark.parametrize("mtu", fraggen.MTUS)
def test_restatement_matches_fixture(fixture, restated, mtu):
    z, _ = fixture
    r = restated[mtu]
    assert np.array_equal(np.frombuffer(b"".join(r["frags"]), np.uint8), z[f"m{mtu}_out"])
    for k in KEYS:
        assert r[k].dtype == z[f"m{mtu}_{k}"].dtype and np.array_equal(r[k], z[f"m{mtu}_{k}"]), k


def test_fixture_covers_the_shapes(fixture, restated):
    """Every verdict occurs, at every mtu something is fragmented, and the
    180-fragment plan of mtu 68 / ihl 60 is there."""
    st = np.concatenate([restated[m]["status"] for m in fraggen.MTUS])
    for want in (0, 0x03, 0x05, 0x09, 0x11, 0x21, 0x39):
        assert (st == want).any(), hex(want)
    assert int(restated[68]["count"].max()) > 1000 and 180 in restated[68]["count"]
    assert all(restated[m]["totals"][0] > 40 for m in fraggen.MTUS)


@pytest.mark.parametrize("mtu", fraggen.MTUS)
def test_restatement_pinned_to_reference(fixture, restated, reference_lib, mtu):
    assert fraggen.check_with(reference_lib, fixture[1], restated[mtu]) == restated[mtu]["totals"][1]


@pytest.mark.parametrize("mtu", fraggen.MTUS)
def test_restatement_pinned_to_oracle(fixture, restated, oracle_lib, mtu):
    assert fraggen.check_with(oracle_lib, fixture[1], restated[mtu]) == restated[mtu]["totals"][1]


@pytest.mark.parametrize("mtu", fraggen.MTUS)
def test_payloads_reassemble(fixture, restated, mtu):
    _, frames = fixture
    r = restated[mtu]
    for i, f in enumerate(frames):
        if not r["count"][i]:
            continue
        l2, ihl, tl = fraggen.subject(f)
        mine = r["frags"][int(r["first"][i]):int(r["first"][i]) + int(r["count"][i])]
        assert all(len(x) <= l2 + mtu for x in mine)
        assert all((len(x) - l2 - ihl) % 8 == 0 for x in mine[:-1])
        assert b"".join(x[l2 + ihl:] for x in mine) == f[l2 + ihl:l2 + tl]
        assert np.all(r["out_src"][int(r["first"][i]):][:len(mine)] == i)


@pytest.mark.parametrize("mtu", fraggen.MTUS)
def test_host_function_matches_fixture(fixture, mtu):
    """pptk_ip_fragment_host, frame by frame: status, count, lengths and every
    byte of the slot buffer (0xEE outside the written range); with one slot
    too few NOROOM and nothing written."""
    from pptk_amd.rx import ip_fragment_host
    z, frames = fixture
    stride = fraggen.up16(18 + mtu)
    out, olen = z[f"m{mtu}_out"], z[f"m{mtu}_out_len"]
    pos = np.concatenate([[0], np.cumsum(olen.astype(np.int64))])
    for i, f in enumerate(frames):
        cnt, first = int(z[f"m{mtu}_count"][i]), int(z[f"m{mtu}_first"][i])
        want = [bytes(out[pos[s]:pos[s + 1]]) for s in range(first, first + cnt)]
        rc, st, got, glen = ip_fragment_host(f, mtu, cnt + 1)
        assert (rc, st) == (cnt, int(z[f"m{mtu}_status"][i])), i
        assert np.array_equal(glen[:cnt], olen[first:first + cnt])
        assert np.array_equal(got.reshape(-1), fraggen.slots(want, stride, cnt + 1)), i
        if cnt:
            rc, st, got, _ = ip_fragment_host(f, mtu, cnt - 1, out_stride=stride + 16)
            assert (rc, st) == (cnt, int(z[f"m{mtu}_status"][i]) | fraggen.ST_NOROOM)
            assert np.all(got == 0xEE)


def test_host_function_rejects_bad_arguments():
    import ctypes
    from pptk_amd.rx import ip_fragment_host, lib
    f = fraggen.frame4(np.random.default_rng(1), 1400)
    for mtu, stride in ((67, 96), (65536, 65568), (576, 592), (576, 600), (1500, 1504)):
        with pytest.raises(OSError):
            ip_fragment_host(f, mtu, 4, out_stride=stride)
    L = lib()
    st, buf, ol = ctypes.c_uint8(0xEE), ctypes.create_string_buffer(608), (ctypes.c_uint16 * 1)()
    assert L.pptk_ip_fragment_host(None, 64, 576, buf, 608, 1, ol, ctypes.byref(st)) == -22
    assert L.pptk_ip_fragment_host(f, len(f), 576, None, 608, 1, ol, ctypes.byref(st)) == -22
    assert L.pptk_ip_fragment_host(f, len(f), 576, buf, 608, 1, None, ctypes.byref(st)) == -22
    assert L.pptk_ip_fragment_host(f, len(f), 576, buf, 608, 1, ol, None) == -22
    assert st.value == 0xEE
    assert L.pptk_ip_fragment_host(None, 0, 576, buf, 608, 1, ol, ctypes.byref(st)) == 0
    assert st.value == 0


def test_random_batches_pinned_to_oracle(oracle_lib):
    """The random batches of the GPU tests hold every verdict and about half
    of their frames need fragmenting; their restated fragments pass the
    oracle's checks too."""
    frames = fraggen.random_frames(3000, 0x77)
    for mtu in (576, 1280):
        r = fraggen.fragment_batch(frames, mtu)
        done = (r["status"] & fraggen.ST_DONE) != 0
        assert 0.3 < done.mean() < 0.6
        for bit in (fraggen.ST_FITS, fraggen.ST_DF, fraggen.ST_ISFRAG, fraggen.ST_BADCKSUM):
            assert (r["status"] & bit).any()
        assert (r["status"] == 0).any()
        assert fraggen.check_with(oracle_lib, frames, r) == r["totals"][1]


def test_sanitized_host_program(tmp_path):
    """tests/c/ipfrag_asan.c with host/ipfrag.c and host/ipcksum.c under
    ASan + UBSan, run as a program of its own."""
    exe = str(tmp_path / "ipfrag_asan")
    src = [os.path.join(ROOT, "tests", "c", "ipfrag_asan.c"),
           os.path.join(ROOT, "pptk_amd", "csrc", "host", "ipfrag.c"),
           os.path.join(ROOT, "pptk_amd", "csrc", "host", "ipcksum.c")]
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include")] + src + ["-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ipfrag ok" in out.stdout, out.stdout + out.stderr
