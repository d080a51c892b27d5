"""Microbench: resident attention kernels for head dims 72 and 80 against the
auto path of a baseline build of the extension.

    python benchmarks/attn_resident_d80_bench.py [--baseline /path/to/_hip*.so]

Sweep: D in {72, 80}, L in {96, 128, 197, 256}, B*H = 3072, forward and
backward separately, timed as benchmarks/attn_bench.py times them. With
--baseline (the extension built from the commit to compare against, loaded
next to this tree's) each round times baseline auto, then this tree's
path="resident", alternating; without it the baseline is this tree's
path="tiled". Per shape it prints the median over the rounds of both and the
spread (max - min) / median of the baseline rounds.
"""
import argparse, importlib.util, math, os, statistics, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import torch
import jimm_amd  # noqa
from jimm_amd.ops import _backend

ap = argparse.ArgumentParser()
ap.add_argument("--baseline", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=30)
args = ap.parse_args()

ext = _backend.ext()
if args.baseline:
    spec = importlib.util.spec_from_file_location("_hip", args.baseline)
    base = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(base)
    base_path = "auto"
else:
    base, base_path = ext, "tiled"

def bench(fn, iters=args.iters, warmup=8):
    for _ in range(warmup): fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters

def rounds(f_base, f_new):
    tb, tn = [], []
    for _ in range(args.rounds):
        tb.append(bench(f_base)); tn.append(bench(f_new))
    spread = (max(tb) - min(tb)) / statistics.median(tb)
    return statistics.median(tb), statistics.median(tn), spread, (max(tn) - min(tn)) / statistics.median(tn)

dev = torch.device("cuda:0")
B, H = 256, 12
print(f"baseline: {'--baseline build, auto' if args.baseline else 'this tree, tiled'}; "
      f"B*H = {B * H}, {args.rounds} rounds x {args.iters} calls")
for D in (72, 80):
    for L in (96, 128, 197, 256):
        # fused-QKV views, as the model passes them
        qkv = torch.randn(B, L, 3, H, D, device=dev).bfloat16()
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
        do = torch.randn(B, L, H, D, device=dev).bfloat16().transpose(1, 2)
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = (dqkv[:, :, i].transpose(1, 2) for i in range(3))
        scale = 1 / math.sqrt(D)
        o, lse = base.attn_fwd(q, k, v, False, scale, base_path)
        tf = 4 * B * H * L * L * D / 1e12
        for name, flops, fb, fn in (
            ("fwd", tf,
             lambda: base.attn_fwd(q, k, v, False, scale, base_path),
             lambda: ext.attn_fwd(q, k, v, False, scale, "resident")),
            ("bwd", 2.5 * tf,
             lambda: base.attn_bwd_fused(q, k, v, o, do, lse, dq, dk, dv, False, scale, base_path),
             lambda: ext.attn_bwd_fused(q, k, v, o, do, lse, dq, dk, dv, False, scale, "resident")),
        ):
            tb, tn, sb, sn = rounds(fb, fn)
            print(f"{name} D={D} L={L:3d}: baseline {tb*1e3:7.3f} ms ({flops/tb:6.1f} TF/s, spread "
                  f"{100*sb:4.1f}%)  resident {tn*1e3:7.3f} ms ({flops/tn:6.1f} TF/s, spread "
                  f"{100*sn:4.1f}%)  speedup {tb/tn:5.2f}x", flush=True)
