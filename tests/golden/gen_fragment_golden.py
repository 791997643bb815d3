"""Writes tests/golden/fragment.npz: the fixture frames of tests/fraggen.py
and, per mtu, what the fragmentation contract makes of them (out = the
written fragments back to back, out_len, out_src, first, count, status,
totals).  The expected bytes come from fraggen's NumPy restatement; before
anything is written the restatement is pinned to the reference
(oracle/_ref/libpptkref.so): its ip_set_hdr_cksum_calc changes no byte of the
fragments and its header getters return the plan.

    python tests/golden/gen_fragment_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import fraggen   # noqa: E402
import framegen  # noqa: E402


def main():
    from oracle.oracle import Reference
    ref = Reference()
    frames = fraggen.fixture_frames()
    buf, off, lens = framegen.pack(frames)
    z = dict(frames=buf, off=off, len=lens, mtus=np.array(fraggen.MTUS, np.uint32))
    checked = 0
    for mtu in fraggen.MTUS:
        r = fraggen.fragment_batch(frames, mtu)
        checked += fraggen.check_with(ref, frames, r)
        z[f"m{mtu}_out"] = np.frombuffer(b"".join(r["frags"]), np.uint8)
        for k in ("out_len", "out_src", "first", "count", "status", "totals"):
            z[f"m{mtu}_{k}"] = r[k]
    path = os.path.join(HERE, "fragment.npz")
    np.savez_compressed(path, **z)
    print(f"{len(frames)} frames, {checked} fragments checked against the reference, "
          f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
