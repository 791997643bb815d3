"""BENCH TOOLING: the sequence-space translation kernel
(pptk_tcp_seq_translate_device) on resident frames, timed in one process and
on the same buffers against the header rewrite (pptk_tx_rewrite_device), the
MSS clamp (pptk_tcp_mss_clamp_device) and the harness stream kernel moving the
bytes the translation touches (harness/rwmix.py mix_ms); interleaved rounds,
medians.  Two workloads: 66-byte ACK segments with NOP NOP TS in 80-byte
slots (SEQ | ACK | TSVAL | TSECHO, a spliced flow's every packet), and
1500-byte segments with TS + SACK(2) in 1536-byte slots, all ops.

    python tools/ab_seq.py
    AB_LIBS=old=build/ab_old/libpptkrx.so python tools/ab_seq.py
    AB_FRAMES=... AB_ROUNDS=... AB_STEPS=...
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _timed(fn, steps, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(steps)]
    for a, z in ev:
        a.record()
        fn()
        z.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(z) for a, z in ev]))


def workloads():
    import struct
    import framegen
    rng = np.random.default_rng(0x5E9)
    ts = b"\x08\x0a" + struct.pack(">II", 1000, 2000)
    sack = b"\x05\x12" + struct.pack(">IIII", 5000, 6000, 8000, 9000)
    ack = framegen.frame_tcp_opts(rng, syn=False, opts=b"\x01\x01" + ts, payload=b"")
    big = framegen.frame_tcp_opts(rng, syn=False, opts=b"\x01\x01" + ts + b"\x01\x01" + sack,
                                  payload=bytes(rng.integers(0, 256, 1500 - 14 - 20 - 52,
                                                             dtype=np.uint8)))
    # (name, frame, stride, ops, chunks written per frame)
    return (("ack66_ts", ack, 80, 0x1b, 3), ("seg1500_ts_sack2", big, 1536, 0x3f, 4))


def main():
    import torch
    from harness.rwmix import mix_ms
    from pptk_amd.records import (REWRITE_DTYPE, RW_DPORT, RW_DST, RW_SPORT, RW_SRC,
                                  seqxlate_dtype)
    from pptk_amd.rx import RxContext
    dev = torch.device("cuda", 0)
    key = bytes(range(1, 17))
    libs = {"": None}
    for kv in filter(None, os.environ.get("AB_LIBS", "").split(",")):
        k, v = kv.split("=", 1)
        libs[k] = os.path.join(ROOT, v)
    n = int(os.environ.get("AB_FRAMES", 16 * 1024 * 1024))
    rounds = int(os.environ.get("AB_ROUNDS", 4))
    steps = int(os.environ.get("AB_STEPS", 10))
    out = {"frames": n}
    for name, f, stride, ops, wchunks in workloads():
        slot = np.zeros(stride, np.uint8)
        slot[:len(f)] = np.frombuffer(f, np.uint8)
        frames = torch.from_numpy(slot).to(dev).repeat(n)
        st = torch.empty(n, dtype=torch.uint8, device=dev)
        xl = np.zeros(1, seqxlate_dtype)
        xl[0] = (ops, 0x01020304, 0x0a0b0c0d, 0x00112233, 7, 9)
        d_xl = torch.from_numpy(xl.view(np.uint8)).to(dev)
        d_x0 = torch.zeros(24, dtype=torch.uint8, device=dev)   # ops == 0: load, park, parse only
        rw = np.zeros(1, REWRITE_DTYPE)
        rw[0] = (RW_SRC | RW_DST | RW_SPORT | RW_DPORT, 0x0a000001, 0xc0a80001, 1234, 4321)
        d_rw = torch.from_numpy(rw.view(np.uint8)).to(dev)
        kw = dict(stride=stride, fixed_len=len(f))
        # the stream stand-in: per 64-frame tile the bytes the translation
        # reads (the frame's first 128, or the whole short frame's slot) and
        # writes (the changed chunks and the status bytes), contiguous
        rb = 64 * min(stride, 128)
        wb = 64 * (16 * wchunks + 1)
        wb += -wb % 16
        sink = torch.empty(n // 64 * wb, dtype=torch.uint8, device=dev)
        res = {}
        for _ in range(rounds):
            for k, p in libs.items():
                ctx = RxContext(0, key, lib_path=p)
                tag = k or "current"
                res.setdefault(tag + ":seq", []).append(_timed(
                    lambda: ctx.seq_translate_device(frames, n, d_xl, status=st, **kw), steps))
                assert int((st & 1).sum().item()) == n, "every frame must be translated"
                res.setdefault(tag + ":seq_ops0", []).append(_timed(
                    lambda: ctx.seq_translate_device(frames, n, d_x0, status=st, **kw), steps))
                res.setdefault(tag + ":rewrite", []).append(_timed(
                    lambda: ctx.tx_rewrite_device(frames, n, d_rw, status=st, **kw), steps))
                res.setdefault(tag + ":mss", []).append(_timed(
                    lambda: ctx.mss_clamp_device(frames, n, 1200, status=st, **kw), steps))
                ctx.close()
            res.setdefault("stream", []).append(mix_ms(frames, rb, n // 64, sink, wb))
        med = {k: round(sorted(v)[len(v) // 2], 4) for k, v in res.items()}
        med["frame_bytes"], med["stride"], med["ops"] = len(f), stride, ops
        med["stream_tile"] = f"{rb} B read + {wb} B written per 64 frames"
        for k in list(med):
            if k.endswith(":seq"):
                t = k[:-4]
                med[t + ":seq/rewrite"] = round(med[k] / med[t + ":rewrite"], 3)
                med[t + ":seq/mss"] = round(med[k] / med[t + ":mss"], 3)
                med[t + ":seq/stream"] = round(med[k] / med["stream"], 3)
        out[name] = med
        del frames, st, sink
        torch.cuda.empty_cache()
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
