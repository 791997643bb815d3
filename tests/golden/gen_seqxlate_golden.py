"""Writes tests/golden/seqxlate.npz: the fixture frames of tests/seqgen.py
packed back to back, the 16-entry translation table with each frame's index,
and what the sequence-space translation contract (include/pptk_rx.h
pptk_tcp_seq_translate_device) makes of them, taken from the reference
(oracle/_ref/libpptkref.so):

- the TCP header of each frame is located from the reference's own records
  (ref_rx_batch: F_L4, proto, l4_off, l4_len);
- the subject and BADOPT rules and the ACK-flag guard are applied here;
- the ops are composed from the reference's functions through
  oracle/refgen.c ref_tcp_opt_op: op 6 with seq + add, op 7 with ack + add,
  then ops 2, 3, 4 and 1 -- on pinned frames only (seqgen.pinned: the inputs
  on which the reference returns);
- the status bits come from the reference's walks (ref_tcp_find_sack_ts,
  ref_tcp_find_sack).

Stored: buf / off / len, table, idx, the pinned mask, the expected status
(0xff on unpinned frames) and the expected bytes as changed positions and
values.  Nothing of the reference itself is stored.

    python tests/golden/gen_seqxlate_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import framegen  # noqa: E402
import seqgen    # noqa: E402

KEY = bytes(range(1, 17))


def main():
    from oracle.oracle import Reference, make_opts
    ref = Reference()
    frames, idx = seqgen.fixture()
    buf, off, lens = framegen.pack(frames, align=1)
    recs = ref.rx_batch(buf, off, lens, opts=make_opts(KEY))
    want, st, pin = seqgen.reference_translate(ref, buf, off, recs, seqgen.XL_TABLE, idx)
    pos = np.nonzero(want != buf)[0].astype(np.uint32)
    path = os.path.join(HERE, "seqxlate.npz")
    np.savez_compressed(path, buf=buf, off=off, len=lens,
                        table=seqgen.XL_TABLE.view(np.uint32).reshape(-1, 6),
                        idx=idx, pinned=pin, status=st, l4_off=recs["l4_off"],
                        l4_len=recs["l4_len"], subject=seqgen.is_subject(recs),
                        pos=pos, val=want[pos])
    print(f"{len(frames)} frames, {int((~pin).sum())} unpinned "
          f"({100.0 * (~pin).mean():.1f} %), {pos.size} changed bytes, "
          f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
