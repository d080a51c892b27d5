"""Cost of global-norm gradient clipping in the fused Adam step (docs/kernels.md, K14).

    python benchmarks/gradclip_bench.py

ViT-B/16 parameter shapes in bf16 with fp32 masters, one process, device-event
timing. Two pairs, the variants alternating inside every round:

  norm  the fused norm + coefficient (grad_sqnorm + clip_finalize, a read of
        every gradient) against torch.nn.utils.clip_grad_norm_(foreach=True),
        which reads every gradient and then rewrites it. max_norm is small, so
        torch's rewrite really scales (its cost does not depend on that).
  step  opt.step() with max_grad_norm set against opt.step() without it (the
        parent commit's kernels, unchanged), on two optimizers over clones of
        the same parameters.

The bandwidth figures count the bytes the algorithm needs: a clipped-off step
reads g (2 B) + m, v, master (12 B) and writes m, v, master, p (14 B) per
element; the norm pass reads g alone. One JSON line per measurement on stdout.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=50, help="calls per round and variant")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--max-norm", type=float, default=1.0)
    return ap.parse_args()


def vit_b16_shapes():
    """Parameter shapes of the flagship model (152 tensors, 86.6 M elements)."""
    import jimm_amd

    model = jimm_amd.VisionTransformer(num_classes=1000, img_size=224, patch_size=16)
    return [tuple(p.shape) for p in model.parameters()]


def _summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "rounds": len(xs)}


def _emit(**kw):
    print(json.dumps(kw), flush=True)


def _time_alternating(torch, variants, args):
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.iters):
                fn()
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop) * 1000.0 / args.iters)
    return times


def main():
    args = _args()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import torch

    from jimm_amd.ops import _backend
    from jimm_amd.train import Adam

    assert torch.cuda.is_available(), "gradclip_bench measures on the GPU only"
    ext = _backend.ext()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cuda").manual_seed(0)
    shapes = vit_b16_shapes()

    def params():
        gen.manual_seed(0)
        ps = [(torch.randn(s, device=dev, generator=gen) * 0.02).bfloat16().requires_grad_(True)
              for s in shapes]
        for p in ps:
            p.grad = (torch.randn(p.shape, device=dev, generator=gen) * 0.01).bfloat16()
        return ps

    n_elem = sum(p.numel() for p in params())
    g_bytes = 2 * n_elem
    step_bytes = (2 + 12 + 14) * n_elem

    # -- 1. the norm pass alone ------------------------------------------------
    ps = params()
    gs = [p.grad for p in ps]
    desc, nchunks = ext.grad_desc_prepare(gs)
    nchunks = int(nchunks.item())
    partials = torch.zeros(nchunks, device=dev)
    stats = torch.zeros(4, device=dev)

    def fused_norm():
        ext.grad_sqnorm(desc, nchunks, partials, 0)
        ext.clip_finalize(partials, stats, args.max_norm)

    ps_t = params()

    def torch_clip():
        torch.nn.utils.clip_grad_norm_(ps_t, args.max_norm, foreach=True)

    times = _time_alternating(torch, {"fused norm+coef": fused_norm, "torch foreach clip": torch_clip}, args)
    for name, xs in times.items():
        passes = 1 if name.startswith("fused") else 3  # read; read + write
        _emit(pair="norm", variant=name, tensors=len(shapes), elements=n_elem, chunks=nchunks,
              unit="us/call", gbps_algorithmic=passes * g_bytes / statistics.median(xs) / 1e3,
              **_summary(xs))

    # -- 2. the optimizer step, clipping on vs off -----------------------------
    opt_off = Adam(params(), lr=1e-4, weight_decay=0.01)
    opt_on = Adam(params(), lr=1e-4, weight_decay=0.01, max_grad_norm=args.max_norm)
    times = _time_alternating(torch, {"step clip off": opt_off.step, "step clip on": opt_on.step}, args)
    off = statistics.median(times["step clip off"])
    on = statistics.median(times["step clip on"])
    adam_gbps = step_bytes / off / 1e3
    for name, xs in times.items():
        _emit(pair="step", variant=name, elements=n_elem, unit="us/call", **_summary(xs))
    _emit(pair="step", variant="summary", unit="us", added=on - off,
          adam_gbps_clip_off=adam_gbps,
          one_grad_read_at_adam_bandwidth=g_bytes / adam_gbps / 1e3,
          skipped_steps=opt_on.skipped_steps())


if __name__ == "__main__":
    main()
