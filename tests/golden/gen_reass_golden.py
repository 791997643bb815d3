"""Writes tests/golden/reass.npz: the fixture frames of tests/reassgen.py and
what the reassembly contract makes of them with max_candidates = n, out_cap =
the slots needed, out_stride = 65536 (out = the written slots back to back,
out_len, report, dgram, fstatus, hdr).  Frames and expected outputs only: the
records a test feeds in come from the receive transform it runs.  The
expected bytes come from reassgen's NumPy restatement over the reference's
own records (oracle/_ref/libpptkref.so); before anything is written every
reassembled header is pinned to the reference: its ip_set_hdr_cksum_calc
changes no byte of the slots and its getters return offset 0, MF clear and
the total length.

    python tests/golden/gen_reass_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import reassgen  # noqa: E402

OUT_STRIDE = 65536


def expected(lib):
    frames = reassgen.fixture_frames()
    buf, off, lens, recs, side = reassgen.records(lib, frames)
    r = reassgen.reassemble(frames, recs, side, len(frames), len(frames), OUT_STRIDE)
    return frames, buf, off, lens, r


def main():
    from oracle.oracle import Reference
    ref = Reference()
    frames, buf, off, lens, r = expected(ref)
    checked = reassgen.check_with(ref, r["slots"])
    z = dict(frames=buf, off=off, len=lens, out=np.frombuffer(b"".join(r["slots"]), np.uint8),
             out_len=r["out_len"], report=r["report"].view(np.uint8), dgram=r["dgram"],
             fstatus=r["fstatus"], hdr=np.array([r["hdr"]]).view(np.uint64),
             out_stride=np.array([OUT_STRIDE], np.uint64))
    path = os.path.join(HERE, "reass.npz")
    np.savez_compressed(path, **z)
    print(f"{len(frames)} frames, {int(r['hdr']['dgrams'])} datagrams, {checked} slots checked "
          f"against the reference, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
