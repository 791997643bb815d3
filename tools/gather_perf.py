"""MEASUREMENT (DESIGN.md "Egress gather"): pptk_tx_gather_device on 16 M
frames generated in HBM (harness/synth.py: C64, C1500, IMIX, CMIX), timed with
device events -- median of --reps after two warm-ups, min..max beside it --
for the identity list (entry g is frame g, one region) and for a 4-port
dispatch list with a tenth of the frames flooded (pptk_tx_dispatch_device's
own list, runs and header word, no download in between).  Two yardsticks run
in the same process on the same device:
  (a) harness/rwmix.py's fastest stream kernel over the same read and write
      bytes (64-frame tiles: the frame bytes in, the slot bytes out);
  (b) pptk_tunnel_encap_device on the same batch: the existing op of the same
      shape, a re-aligning team copy plus 38 bytes per frame.

    python tools/gather_perf.py [--frames 16777216] [--reps 9] [--out FILE]

One JSON line per batch and list.

--sweep: the identity list at fixed lengths from 64 to 1500 bytes, each once
as one fixed length (the team width the length selects: 4 / 8 / 16 / 32 lanes,
pptk_amd/csrc/tx_gather.hip) and once through a length array holding that
length (16 lanes): where another width beats 16 lanes.
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


def measure(fn, reps, torch):
    """(median, min, max) ms of `reps` calls after two warm-ups."""
    ts = []
    for r in range(reps + 2):
        t = timed(fn, torch)
        if r >= 2:
            ts.append(t)
    ts.sort()
    return round(ts[len(ts) // 2], 4), round(ts[0], 4), round(ts[-1], 4)


def emit(res, path):
    line = json.dumps(res)
    print(line, flush=True)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def gather_fn(ctx, b, n, entries, out_cap, keep, **kw):
    """A closure over one gather call with its outputs allocated once."""
    first = ctx.tx_gather_device(b["frames"], n, entries, out_cap, off=b.get("off"),
                                 lens=b.get("lens"), stride=b.get("stride", 0),
                                 fixed_len=b.get("fixed_len", 0) if "lens" not in b else 0, **kw)
    keep.update(first)

    def fn():
        ctx.tx_gather_device(b["frames"], n, entries, out_cap, off=b.get("off"), lens=b.get("lens"),
                             stride=b.get("stride", 0),
                             fixed_len=b.get("fixed_len", 0) if "lens" not in b else 0,
                             out=first["out"], pk_off=first["pk_off"], pk_len=first["pk_len"],
                             ports=first["ports"], hdr=first["hdr"], scratch=first["scratch"], **kw)
    return fn


def need_of(ctx, b, n, entries, torch, **kw):
    """hdr of a count-only call: what out_cap packs every entry."""
    from pptk_amd.records import GATHER_HDR_DTYPE
    r = ctx.tx_gather_device(b["frames"], n, entries, 0, off=b.get("off"), lens=b.get("lens"),
                             stride=b.get("stride", 0),
                             fixed_len=b.get("fixed_len", 0) if "lens" not in b else 0,
                             pk_off=False, pk_len=False, **kw)
    torch.cuda.synchronize()
    return r["hdr"].cpu().numpy().view(GATHER_HDR_DTYPE)[0]


def sweep(args, ctx, dev, torch, synth):
    n = args.frames
    buf = synth.make_batch("c1500", n, dev)["frames"]
    for flen in (64, 96, 128, 256, 320, 384, 768, 896, 1024, 1500):
        slot = (flen + 15) & ~15
        res = {"sweep": True, "fixed_len": flen, "n": n}
        for form in ("fixed", "lens"):
            b = dict(frames=buf, stride=flen)
            if form == "fixed":
                b["fixed_len"] = flen
            else:
                b["lens"] = torch.full((n,), flen, dtype=torch.int16, device=dev)
            keep = {}
            fn = gather_fn(ctx, b, n, n, n * slot, keep)
            res[form + "_ms"], lo, hi = measure(fn, args.reps, torch)
            res[form + "_ms_min_max"] = [lo, hi]
            del keep, fn
            torch.cuda.empty_cache()
        emit(res, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--cfg", action="append", default=[],
                    help="batches to run (default: c64 c1500 imix cmix)")
    ap.add_argument("--out", default="", help="append the JSON lines to this file too")
    ap.add_argument("--no-sol", action="store_true")
    ap.add_argument("--sweep", action="store_true",
                    help="instead: the identity list at fixed lengths 64..1500, one fixed length "
                         "(the selected team width) against a length array (16 lanes)")
    args = ap.parse_args()

    import numpy as np
    import torch
    from harness import rwmix, synth
    from pptk_amd.records import (DISPATCH_HDR_DTYPE, GATHER_HDR_DTYPE, PORT_FLOOD, TUN_DF,
                                  TUNNEL_DTYPE)
    from pptk_amd.rx import RxContext

    assert torch.cuda.is_available(), "gather_perf needs a GPU"
    dev = torch.device("cuda:0")
    n, nports = args.frames, 4
    ctx = RxContext(0)
    if args.sweep:
        sweep(args, ctx, dev, torch, synth)
        ctx.close()
        return
    tun = np.zeros(1, TUNNEL_DTYPE)
    tun[0] = ([2, 0, 0, 0, 0, 1], [2, 0, 0, 0, 0, 2], (10 << 24) | 1, (10 << 24) | 2, 0, 64, 0,
              TUN_DF, 0)
    d_tun = torch.from_numpy(tun.view(np.uint8).copy()).to(dev)
    rng = np.random.default_rng(1)
    port = rng.integers(0, nports, n).astype(np.uint8)
    port[rng.random(n) < 0.1] = PORT_FLOOD
    d_port = torch.from_numpy(port).to(dev)

    for cfg in args.cfg or ["c64", "c1500", "imix", "cmix"]:
        b = synth.make_batch(cfg, n, dev)
        mixed = "lens" in b
        desc = dict(off=b.get("off"), lens=b.get("lens"), stride=b.get("stride", 0),
                    fixed_len=0 if mixed else b["fixed_len"])
        res = {"cfg": cfg, "n": n, "frame_bytes": b["bytes"], "device": torch.cuda.get_device_name(dev)}

        # the identity list, one region
        h = need_of(ctx, b, n, n, torch)
        keep = {}
        fn = gather_fn(ctx, b, n, n, int(h["need"]), keep)
        res["identity_ms"], lo, hi = measure(fn, args.reps, torch)
        res["identity_ms_min_max"] = [lo, hi]
        got = keep["hdr"].cpu().numpy().view(GATHER_HDR_DTYPE)[0]
        assert got["packed"] == n and got["frame_bytes"] == b["bytes"], got
        res["identity_slot_bytes"] = int(got["bytes"])
        res["identity_TBps"] = round((b["bytes"] + int(got["bytes"])) / res["identity_ms"] / 1e9, 3)
        if not args.no_sol:                                  # (a) the stream kernels, same bytes
            wb = (int(got["bytes"]) // (n // 64)) & ~15   # per 64-frame tile, whole chunks
            if mixed:
                ms, how = rwmix.sol_ms(b["frames"], n, keep["out"], wb, off=b["off"], lens=b["lens"])
            else:
                ms, how = rwmix.sol_ms(b["frames"], n, keep["out"], wb, rb=64 * b["fixed_len"])
            res["sol_ms"], res["sol_shape"] = round(ms, 4), how
            res["identity_over_sol"] = round(res["identity_ms"] / ms, 3)
        del keep, fn
        torch.cuda.empty_cache()

        # (b) encap on the same batch
        ostr = (38 + b["max_len"] + 15) & ~15
        out = torch.empty(n * ostr, dtype=torch.uint8, device=dev)
        out_len = torch.empty(n, dtype=torch.int16, device=dev)
        status = torch.empty(n, dtype=torch.uint8, device=dev)
        res["encap_ms"], lo, hi = measure(
            lambda: ctx.tunnel_encap_device(b["frames"], n, d_tun, out=out, out_stride=ostr,
                                            out_len=out_len, status=status, **desc),
            args.reps, torch)
        res["encap_ms_min_max"] = [lo, hi]
        assert bool((status == 1).all())
        res["identity_over_encap"] = round(res["identity_ms"] / res["encap_ms"], 3)
        del out, out_len, status
        torch.cuda.empty_cache()

        # a 4-port dispatch list, a tenth of the frames flooded from port 0
        cap = 2 * n
        d = ctx.tx_dispatch_device(n, nports, port=d_port, in_port_all=0, cap=cap,
                                   out_off=False, out_len=False, **desc)
        written = d["hdr"].data_ptr() + DISPATCH_HDR_DTYPE.fields["written"][1]
        kw = dict(nports=nports, entries=d["list"], d_entries=written, runs=d["ports"])
        h = need_of(ctx, b, n, cap, torch, **kw)
        keep = {}
        fn = gather_fn(ctx, b, n, cap, int(h["need"]), keep, **kw)
        res["dispatch_ms"], lo, hi = measure(fn, args.reps, torch)
        res["dispatch_ms_min_max"] = [lo, hi]
        got = keep["hdr"].cpu().numpy().view(GATHER_HDR_DTYPE)[0]
        assert got["packed"] == got["entries"] == h["entries"] > n and got["bad"] == 0, got
        res["dispatch_entries"], res["dispatch_slot_bytes"] = int(got["entries"]), int(got["bytes"])
        res["dispatch_TBps"] = round((int(got["frame_bytes"]) + int(got["bytes"]))
                                     / res["dispatch_ms"] / 1e9, 3)
        emit(res, args.out)
        del keep, fn, d, b
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
