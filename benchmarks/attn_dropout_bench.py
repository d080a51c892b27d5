"""Cost of attention-probability dropout (profiles/attn_dropout_NOTES.md).

    python benchmarks/attn_dropout_bench.py --L 197 577

At B*H = --bh (default 3072 = ViT-B/16 batch 256), D = 64, forward and backward:
  hip p=0      the flash kernels as every call without dropout runs them;
  hip p        the DROP instantiations (mask computed in registers);
  composite p  the torch path (materialises (B, H, L, L) several times, mask
               from attn_keep_mask), which is what a user ran before; timed
               at --composite-bh heads and scaled to --bh (it is linear in BH).
Device events around --iters calls, variants alternating inside every round;
the table gives the median and the range of the rounds. One JSON line per
measurement on stdout.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from jimm_amd import ops  # noqa: E402
from jimm_amd.ops import _backend  # noqa: E402


def _time(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1000.0 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, nargs="+", default=[197, 577])
    ap.add_argument("--bh", type=int, default=3072)
    ap.add_argument("--composite-bh", type=int, default=96)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "attn_dropout_bench measures on the GPU only"
    ext = _backend.ext()
    dev = torch.device("cuda:0")
    H, D, p, site = args.heads, 64, args.p, 1 << 29
    scale = D ** -0.5
    rng = torch.tensor([1234, 0], dtype=torch.int64, device=dev)

    for L in args.L:
        g = torch.Generator(device="cuda").manual_seed(L)

        def views(bh):
            qkv = torch.randn(bh // H, L, 3, H, D, device=dev, generator=g).bfloat16()
            do = torch.randn(bh // H, L, H, D, device=dev, generator=g).bfloat16().transpose(1, 2)
            return qkv, tuple(qkv[:, :, i].transpose(1, 2) for i in range(3)), do

        qkv, (q, k, v), do = views(args.bh)
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = (dqkv[:, :, i].transpose(1, 2) for i in range(3))
        o0, lse0 = ext.attn_fwd(q, k, v, False, scale)
        o1, lse1 = ext.attn_fwd(q, k, v, False, scale, "auto", p, rng, site)

        qkv_c, _, do_c = views(args.composite_bh)
        qkv_c.requires_grad_()

        def composite():  # forward + backward: autograd holds the (B, H, L, L) tensors
            qc, kc, vc = (qkv_c[:, :, i].transpose(1, 2).float() for i in range(3))
            out = ops.attention(qc, kc, vc, dropout_p=p, rng=rng, site=site)
            out.backward(do_c.float())
            qkv_c.grad = None

        variants = {
            "fwd hip p=0": lambda: ext.attn_fwd(q, k, v, False, scale),
            "fwd hip p": lambda: ext.attn_fwd(q, k, v, False, scale, "auto", p, rng, site),
            "bwd hip p=0": lambda: ext.attn_bwd_fused(q, k, v, o0, do, lse0, dq, dk, dv, False, scale),
            "bwd hip p": lambda: ext.attn_bwd_fused(q, k, v, o1, do, lse1, dq, dk, dv, False, scale,
                                                    "auto", p, rng, site),
            "fwd+bwd composite p": composite,
        }
        for fn in variants.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():  # alternate the variants inside a round
                times[name].append(_time(fn, args.iters))
        for name, xs in times.items():
            f = args.bh / args.composite_bh if "composite" in name else 1.0
            print(json.dumps({"L": L, "bh": args.bh, "p": p, "variant": name, "unit": "us/call",
                              "median": statistics.median(xs) * f, "min": min(xs) * f,
                              "max": max(xs) * f, "rounds": len(xs)}), flush=True)


if __name__ == "__main__":
    main()
