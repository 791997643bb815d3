"""MEASUREMENT TOOLING: time pptk_tx_dispatch_device.

16 M frames on the `port` form with descriptors on (out_off and out_len set),
fixed stride and length, one process on the card:

    nports  traffic
    4       unicast random
    16      unicast random
    64      unicast random
    16      1 % flood
    16      all frames to one port

Per configuration: milliseconds per call -- device events around one call of
the C function with a prebuilt struct pptk_dispatch (nothing of the Python
binding lies between the events; the C call's argument checks and its four
launches from the host do), the median of --calls calls after --warmup; beside
it --calls calls enqueued back to back between one pair of events, per call --
the bytes the contract obliges the call to move -- 1 B read per frame per pass
(two passes: count, scatter) and 14 B written per entry (list 4, out_off 8,
out_len 2) -- and that figure over the time.  The copy rate of harness/membench.py from the same process stands
beside it.  Writes one JSON document to --out and prints it.

    python tools/dispatch_perf.py --out profiles/dispatch/dispatch_perf.json
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = ((4, "unicast random"), (16, "unicast random"), (64, "unicast random"),
           (16, "1 % flood"), (16, "all to one port"))
PASSES = 2            # count and scatter each read the code bytes once
ENTRY_BYTES = 14      # list 4 + out_off 8 + out_len 2


def codes(torch, dev, n, nports, traffic, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    if traffic == "all to one port":
        return torch.full((n,), nports - 1, dtype=torch.uint8, device=dev)
    port = torch.randint(0, nports, (n,), generator=g, device=dev, dtype=torch.int32).to(torch.uint8)
    if traffic == "1 % flood":
        from pptk_amd.records import PORT_FLOOD
        port[torch.rand(n, generator=g, device=dev) < 0.01] = PORT_FLOOD
    return port


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=1 << 24)
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dispatch", "dispatch_perf.json"))
    a = ap.parse_args()
    import torch
    from harness import membench
    from pptk_amd.records import DISPATCH_HDR_DTYPE, PORT_DROP
    from pptk_amd.rx import Dispatch, RxContext, tx_dispatch_shape
    if not torch.cuda.is_available():
        sys.exit("dispatch_perf: needs a GPU")
    dev = torch.device("cuda:0")
    n = a.frames
    ctx = RxContext(0, bytes(16))
    rows = []
    for k, (nports, traffic) in enumerate(CONFIGS):
        port = codes(torch, dev, n, nports, traffic, 100 + k)
        cap = n + (n // 50) * nports            # room for every entry of 1 % floods
        # the binding once, for the outputs and the scratch; then the C call alone
        keep = ctx.tx_dispatch_device(n, nports, port=port, in_port_all=0, stride=2048,
                                      fixed_len=1514, cap=cap)
        d = Dispatch(n=n, port=port.data_ptr(), in_port_all=0, nports=nports, miss_code=PORT_DROP,
                     stride=2048, fixed_len=1514, list=keep["list"].data_ptr(),
                     out_off=keep["out_off"].data_ptr(), out_len=keep["out_len"].data_ptr(),
                     cap=cap, ports=keep["ports"].data_ptr(), hdr=keep["hdr"].data_ptr())
        call, ref = ctx._L.pptk_tx_dispatch_device, ctypes.byref(d)
        scratch = ctypes.c_void_p(keep["scratch"].data_ptr())
        size = keep["scratch"].numel()
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        times = []
        for it in range(a.warmup + a.calls):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            rc = call(ctx._ctx, ref, scratch, size, stream)
            t1.record()
            torch.cuda.synchronize(dev)
            assert rc == 0, rc
            if it >= a.warmup:
                times.append(t0.elapsed_time(t1))
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for it in range(a.calls):
            call(ctx._ctx, ref, scratch, size, stream)
        t1.record()
        torch.cuda.synchronize(dev)
        chained = t0.elapsed_time(t1) / a.calls
        times.sort()
        hdr = keep["hdr"].cpu().numpy().view(DISPATCH_HDR_DTYPE)[0]
        assert hdr["written"] == hdr["total"], "the cap is meant to hold every entry"
        ms = times[len(times) // 2]
        moved = PASSES * n + ENTRY_BYTES * int(hdr["total"])
        rows.append(dict(nports=nports, traffic=traffic, entries=int(hdr["total"]),
                         flood_frames=int(hdr["flood"]), ms_median=round(ms, 4),
                         ms_min=round(times[0], 4), ms_max=round(times[-1], 4),
                         ms_back_to_back=round(chained, 4),
                         contract_bytes=moved, contract_gbs=round(moved / (ms * 1e-3) / 1e9, 1)))
        del keep, port
    buf = torch.zeros(1 << 30, dtype=torch.uint8, device=dev)
    rates = membench.measure(buf)
    ctx.close()
    B, W = tx_dispatch_shape()
    doc = dict(tool="tools/dispatch_perf.py", device=torch.cuda.get_device_name(dev), frames=n,
               calls=a.calls, warmup=a.warmup, block_frames=B, scan_width=W,
               timing="device events around one C call with a prebuilt struct, median; "
                      "ms_back_to_back: `calls` calls between one pair of events, per call",
               membench=rates, configs=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
