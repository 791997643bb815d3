"""MEASUREMENT (DESIGN.md "GRE tunnel gateway"): pptk_tunnel_encap_device and
pptk_tunnel_decap_device on 16 M frames generated in HBM (harness/synth.py:
64-byte and 1500-byte frames at a fixed stride), timed with device events,
beside harness/rwmix.py's speed-of-light kernels moving the same bytes on the
same GPU.

    python tools/tunnel_perf.py [--n 16777216] [--reps 9] [--lib PATH ...]

Bytes per frame.  Encap reads len and writes round_up(38 + len, 16): the
speed of light reads 64-frame tiles of 64 * len bytes and writes 64 *
round_up(38 + len, 16) per tile.  Decap reads the outer header (one 64-byte
line per frame where the slots are packed; at a 1552-byte stride every
frame's header is a line of its own) and writes 11 bytes of descriptor and
status: its speed of light reads 64 bytes and writes 16 per frame.

--lib: A/B builds of the library (make abvariant NAME=team4
DEFS=-DPPTK_TUN_TEAM=4); every library is timed in the same process, the
repetitions alternating between them.  One JSON line per size.

--sweep: encap only, fixed lengths from 64 to 1500 bytes and the mixed-length
batches of harness/synth.py through offset and length arrays, for every
--lib: where the team widths cross (pptk_amd/csrc/tx_tunnel.hip).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def sweep(args, ctxs, d_tun, dev, torch, synth):
    """Where the team widths cross.  Encap copies bytes without parsing them,
    so one buffer cut at a stride of L bytes serves every fixed length L; the
    mixed batches are offset-described (a length array: the kernel cannot know
    the lengths at launch)."""
    n = args.n

    def run(res, call):
        ts = {k: [] for k in ctxs}
        for r in range(args.reps + 2):
            for k, c in ctxs.items():
                t = timed(lambda: call(c), torch)
                if r >= 2:
                    ts[k].append(t)
        res["encap_ms"] = {k: round(median(v), 4) for k, v in ts.items()}
        print(json.dumps(res), flush=True)

    buf = synth.make_batch("c1500", n, dev)["frames"]
    for flen in (64, 128, 192, 218, 256, 384, 512, 768, 1024, 1500):
        ostr = (38 + flen + 15) & ~15
        out = torch.empty(n * ostr, dtype=torch.uint8, device=dev)
        run({"fixed_len": flen, "n": n},
            lambda c: c.tunnel_encap_device(buf, n, d_tun, stride=flen, fixed_len=flen, out=out,
                                            out_stride=ostr))
        del out
    del buf
    torch.cuda.empty_cache()
    out = torch.empty(n * 1552, dtype=torch.uint8, device=dev)
    for cfg in ("imix", "cmix"):
        b = synth.make_batch(cfg, n, dev)
        run({"cfg": cfg, "n": n, "bytes": b["bytes"]},
            lambda c: c.tunnel_encap_device(b["frames"], n, d_tun, off=b["off"], lens=b["lens"],
                                            out=out, out_stride=1552))
        del b
    for cfg, flen in (("c64", 64), ("c1500", 1500)):   # one length, but as a length array
        b = synth.make_batch(cfg, n, dev)
        lens = torch.full((n,), flen, dtype=torch.int16, device=dev)
        run({"cfg": cfg + " with lens", "n": n},
            lambda c: c.tunnel_encap_device(b["frames"], n, d_tun, lens=lens, stride=b["stride"],
                                            out=out, out_stride=1552))
        del b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--lib", action="append", default=[])
    ap.add_argument("--no-sol", action="store_true")
    ap.add_argument("--sweep", action="store_true",
                    help="instead: fixed lengths 64..1500 and the mixed-length batches "
                         "(length arrays) of harness/synth.py, encap only, every --lib")
    args = ap.parse_args()

    import numpy as np
    import torch
    from harness import rwmix, synth
    from pptk_amd.records import TUN_DF, TUNNEL_DTYPE
    from pptk_amd.rx import RxContext

    assert torch.cuda.is_available(), "tunnel_perf needs a GPU"
    dev = torch.device("cuda:0")
    n = args.n
    libs = args.lib or [None]
    ctxs = {os.path.basename(os.path.dirname(p)) if p else "product": RxContext(0, lib_path=p)
            for p in libs}
    tun = np.zeros(1, TUNNEL_DTYPE)
    tun[0] = ([2, 0, 0, 0, 0, 1], [2, 0, 0, 0, 0, 2], (10 << 24) | 1, (10 << 24) | 2, 0, 64, 0,
              TUN_DF, 0)
    d_tun = torch.from_numpy(tun.view(np.uint8).copy()).to(dev)

    if args.sweep:
        sweep(args, ctxs, d_tun, dev, torch, synth)
        return
    for cfg, flen in (("c64", 64), ("c1500", 1500)):
        b = synth.make_batch(cfg, n, dev)
        ostr = (38 + flen + 15) & ~15
        out = torch.empty(n * ostr, dtype=torch.uint8, device=dev)
        out_len = torch.empty(n, dtype=torch.int16, device=dev)
        status = torch.empty(n, dtype=torch.uint8, device=dev)
        in_off = torch.empty(n, dtype=torch.int64, device=dev)
        res = {"cfg": cfg, "n": n, "frame_bytes": flen, "out_stride": ostr,
               "read_bytes": n * flen, "written_bytes": n * ostr}

        def encap(c):
            c.tunnel_encap_device(b["frames"], n, d_tun, stride=b["stride"], fixed_len=flen,
                                  out=out, out_stride=ostr, out_len=out_len, status=status)

        def decap(c):
            c.tunnel_decap_device(out, n, stride=ostr, fixed_len=38 + flen, in_off=in_off,
                                  in_len=out_len, status=status)

        for name, fn in (("encap", encap), ("decap", decap)):
            ts = {k: [] for k in ctxs}
            for r in range(args.reps + 2):          # two warm-up rounds
                for k, c in ctxs.items():           # alternating between the libraries
                    t = timed(lambda: fn(c), torch)
                    if r >= 2:
                        ts[k].append(t)
            res[name + "_ms"] = {k: round(median(v), 4) for k, v in ts.items()}
            res[name + "_ms_min_max"] = {k: [round(min(v), 4), round(max(v), 4)]
                                         for k, v in ts.items()}
            if name == "encap":
                assert bool((status == 1).all()) and bool((out_len == 38 + flen).all())
            else:
                assert bool((status == 0x07).all()) and bool((out_len == flen).all())
        if not args.no_sol:
            ms, how = rwmix.sol_ms(b["frames"], n, out, 64 * ostr, rb=64 * flen)
            res["encap_sol_ms"], res["encap_sol_shape"] = round(ms, 4), how
            ms, how = rwmix.sol_ms(out, n, b["frames"], 64 * 16, rb=64 * 64)
            res["decap_sol_ms"], res["decap_sol_shape"] = round(ms, 4), how
            res["encap_over_sol"] = {k: round(v / res["encap_sol_ms"], 3)
                                     for k, v in res["encap_ms"].items()}
            res["decap_over_sol"] = {k: round(v / res["decap_sol_ms"], 3)
                                     for k, v in res["decap_ms"].items()}
            res["encap_TBps"] = {k: round((n * flen + n * ostr) / v / 1e9, 3)
                                 for k, v in res["encap_ms"].items()}
        print(json.dumps(res), flush=True)
        del b, out
        torch.cuda.empty_cache()
    for c in ctxs.values():
        c.close()


if __name__ == "__main__":
    main()
