"""BENCH TOOLING: pptk_ip_fragment_device on resident batches larger than
the 256 MiB cache, hipEvent-timed (median of AB_REPS >= 20 calls after
warm-up), beside -- in the same run, on the same input frames --
pptk_tx_cksum_device and the harness's trivial read/write stream
(harness/rwmix mix_ms) moving the contract's read and write bytes.

    python tools/ab_fragment.py            # cases a, b, c
    AB_CASES=a AB_REPS=40 python tools/ab_fragment.py

  a  1500-byte IPv4/UDP frames (harness c1500, DF cleared), mtu 576
  b  9000-byte frames, mtu 1500
  c  CMIX lengths (harness cmix, DF cleared), mtu 1280: most frames FITS

Per case one JSON line: ms of the call; plan_ms = the same call with
out_cap = 0 (plan + scan + apply run in full, the emit kernel only reads the
status bytes), so ms - plan_ms is the emit kernel's share; read_bytes (every
frame once) and write_bytes (every slot up to its length rounded up to 16,
plus the per-slot and per-frame words); sol_ms and sol_frac = sol_ms / ms;
tx_ms of the tx checksum op.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def clear_df(frames, off):
    """Clear DF in every untagged IPv4 frame (the harness recipes set it, as
    the reference's sender does) and fix the header checksum incrementally."""
    v4 = (frames[off + 12] == 8) & (frames[off + 13] == 0) & ((frames[off + 20] & 0x40) != 0)
    o = off[v4]
    frames[o + 20] = frames[o + 20] & 0xBF
    ck = (frames[o + 24].to(torch_i32()) << 8) | frames[o + 25].to(torch_i32())
    ck = ck + 0x4000
    ck = (ck & 0xFFFF) + (ck >> 16)
    frames[o + 24] = (ck >> 8).to(frames.dtype)
    frames[o + 25] = (ck & 0xFF).to(frames.dtype)


def torch_i32():
    import torch
    return torch.int32


def timed(fn, reps):
    import torch
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def make_case(case, dev):
    import torch
    from harness.synth import make_batch
    if case == "a":
        n = int(os.environ.get("AB_FRAMES_A", 1 << 20))
        b = make_batch("c1500", n, dev)
        clear_df(b["frames"], torch.arange(n, dtype=torch.int64, device=dev) * b["stride"])
        return b, n, 576, dict(stride=b["stride"], fixed_len=b["fixed_len"])
    if case == "b":
        import fraggen
        n = int(os.environ.get("AB_FRAMES_B", 1 << 17))
        tmpl = np.frombuffer(fraggen.frame4(np.random.default_rng(1), 9000 - 14), np.uint8)
        frames = torch.cat([torch.from_numpy(tmpl.copy()).to(dev).repeat(n),
                            torch.zeros(64, dtype=torch.uint8, device=dev)])
        return dict(frames=frames, max_len=9000), n, 1500, dict(stride=9000, fixed_len=9000)
    n = int(os.environ.get("AB_FRAMES_C", 1 << 22))
    b = make_batch("cmix", n, dev)
    clear_df(b["frames"], b["off"])
    return b, n, 1280, dict(off=b["off"], lens=b["lens"])


def main():
    import torch
    from harness.rwmix import mix_ms
    from pptk_amd.rx import RxContext
    dev = torch.device("cuda", 0)
    reps = max(20, int(os.environ.get("AB_REPS", 20)))
    ctx = RxContext(0, bytes(range(1, 17)))
    for case in os.environ.get("AB_CASES", "a,b,c").split(","):
        b, n, mtu, kw = make_case(case, dev)
        frames = b["frames"]
        # size the output from a planning call (out_cap = 0 writes no slot)
        r = ctx.ip_fragment_device(frames, n, mtu, 0, **kw)
        torch.cuda.synchronize()
        need = int(r["totals"][0].item())
        st = r["status"].cpu().numpy()
        r = ctx.ip_fragment_device(frames, n, mtu, need, **kw)
        torch.cuda.synchronize()
        assert int(r["totals"][1].item()) == need
        keep = {k: r[k] for k in ("out", "out_len", "out_src", "first", "count", "status", "totals",
                                  "scratch")}
        full = lambda: ctx.ip_fragment_device(frames, n, mtu, need, out_stride=r["out_stride"],
                                              **keep, **kw)
        plan = lambda: ctx.ip_fragment_device(frames, n, mtu, 0, out_stride=r["out_stride"],
                                              **keep, **kw)
        ms, plan_ms = timed(full, reps), timed(plan, reps)
        tx_ms = timed(lambda: ctx.tx_cksum_device(frames, n, max_len=b["max_len"], **kw), reps)
        ln = (r["out_len"].to(torch.int64) & 0xFFFF)
        rd = (int((kw["lens"].to(torch.int64) & 0xFFFF).sum().item()) if "lens" in kw
              else n * kw["fixed_len"])
        wr = int(((ln + 15) & ~15).sum().item()) + 6 * need + 9 * n
        nt = n // 64
        rb, wb = (64 * rd // n + 15) & ~15, max(16, (64 * wr // n + 15) & ~15)
        sol_out = torch.empty(nt * wb, dtype=torch.uint8, device=dev)
        sol = mix_ms(frames, rb, min(nt, (frames.numel() - 64) // rb), sol_out, wb, reps=reps)
        print(json.dumps({
            "case": case, "frames": n, "mtu": mtu, "slots": need,
            "done_frac": round(float((st & 4).astype(bool).mean()), 4),
            "ms": round(ms, 4), "plan_ms": round(plan_ms, 4), "emit_ms": round(ms - plan_ms, 4),
            "read_bytes": rd, "write_bytes": wr,
            "gbs": round((rd + wr) / ms / 1e6, 1),
            "sol_ms": round(sol, 4), "sol_rb": rb, "sol_wb": wb, "sol_frac": round(sol / ms, 3),
            "tx_ms": round(tx_ms, 4), "ratio_to_tx": round(ms / tx_ms, 3)}), flush=True)
        del b, r, keep, frames, sol_out, full, plan
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
