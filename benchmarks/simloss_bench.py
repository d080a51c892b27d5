"""The fused similarity-loss head against the unfused one (docs/kernels.md, K12).

    python benchmarks/simloss_bench.py

One direction of the loss over an (M, N) logit block, forward + backward, on
L2-normalized bf16 operands, one process, device-event timing, the two variants
alternating inside every round:

  unfused  what ops/losses.py runs with fused=False: scale * a @ b^T through
           rocBLAS and autograd, then the row softmax-CE kernels (softmax), or
           the 8192-column chunk loop over sigmoid_loss_ew (sigmoid)
  fused    fused_similarity_loss: the logit block is computed on MFMA tiles
           and consumed in the epilogue, the backward recomputes it in chunks

For each shape: the median time of a forward + backward, the increase of
torch.cuda.max_memory_allocated over one forward + backward, and (at
--err-scale, default exp(logit_scale) = 100) the error of each variant's loss
and gradients against an fp64 oracle on the same operands, for the shapes up
to --err-max-elems logits. One JSON line per measurement on stdout.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

SHAPES = [
    ("softmax", 1024, 1024, 512),
    ("softmax", 1024, 8192, 512),
    ("softmax", 4096, 32768, 768),
    ("sigmoid", 512, 4096, 768),
]


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10, help="calls per round and variant")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=14.2857, help="exp(logit_scale) of the timed runs")
    ap.add_argument("--bias", type=float, default=-10.0)
    ap.add_argument("--chunk-size", type=int, default=8192)
    ap.add_argument("--err-scale", type=float, default=100.0)
    ap.add_argument("--err-max-elems", type=int, default=1 << 24)
    return ap.parse_args()


def _emit(**kw):
    print(json.dumps(kw), flush=True)


def main():
    args = _args()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import torch
    import torch.nn.functional as F

    from jimm_amd.ops import _backend
    from jimm_amd.ops import losses as L

    assert torch.cuda.is_available(), "simloss_bench measures on the GPU only"
    _backend.ext()
    dev = torch.device("cuda:0")

    def variants(mode, a, b, scale, bias):
        M, N = a.shape[0], b.shape[0]
        labels = torch.arange(M, device=dev)

        def unfused():
            if mode == "softmax":
                return L.softmax_cross_entropy(scale * a @ b.t(), labels)
            total = a.new_zeros((), dtype=torch.float32)
            for start in range(0, N, 8192):
                logits = scale * a @ b[start : start + 8192].t() + bias
                total = total + L._SigmoidLossFn.apply(logits.float(), -start)
            return total

        def fused():
            return L.fused_similarity_loss(a, b, scale, bias if mode == "sigmoid" else None, 0,
                                           mode, args.chunk_size)

        return {"unfused": unfused, "fused": fused}

    def leaves(mode, M, N, D, s):
        g = torch.Generator(device="cuda").manual_seed(M + N + D)
        a = F.normalize(torch.randn(M, D, device=dev, generator=g), dim=-1).bfloat16()
        b = F.normalize(torch.randn(N, D, device=dev, generator=g), dim=-1).bfloat16()
        scale = torch.tensor(s, device=dev, requires_grad=True)
        bias = torch.tensor(args.bias, device=dev, requires_grad=True)
        return a.requires_grad_(True), b.requires_grad_(True), scale, bias

    def step(fn, params):
        for p in params:
            p.grad = None
        fn().backward()

    for mode, M, N, D in SHAPES:
        a, b, scale, bias = leaves(mode, M, N, D, args.scale)
        fns = variants(mode, a, b, scale, bias)
        params = (a, b, scale, bias)
        for fn in fns.values():
            for _ in range(args.warmup):
                step(fn, params)
        torch.cuda.synchronize()

        # -- time ------------------------------------------------------------------
        times = {k: [] for k in fns}
        for _ in range(args.rounds):
            for name, fn in fns.items():
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(args.iters):
                    step(fn, params)
                stop.record()
                stop.synchronize()
                times[name].append(start.elapsed_time(stop) * 1000.0 / args.iters)

        # -- memory ----------------------------------------------------------------
        peaks = {}
        for name, fn in fns.items():
            for p in params:
                p.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            fn().backward()
            torch.cuda.synchronize()
            peaks[name] = torch.cuda.max_memory_allocated() - before
        for name, xs in times.items():
            _emit(mode=mode, M=M, N=N, D=D, scale=args.scale, variant=name, unit="us/fwd+bwd",
                  median=statistics.median(xs), min=min(xs), max=max(xs), rounds=len(xs),
                  peak_mem_increase_mib=peaks[name] / 2**20,
                  fp32_logits_mib=M * N * 4 / 2**20)
        del fns, a, b

        # -- error against fp64 ----------------------------------------------------
        if M * N > args.err_max_elems:
            _emit(mode=mode, M=M, N=N, D=D, errors="not measured (above --err-max-elems)")
            continue
        a, b, scale, bias = leaves(mode, M, N, D, args.err_scale)
        a64 = a.detach().double().requires_grad_(True)
        b64 = b.detach().double().requires_grad_(True)
        s64 = scale.detach().double().requires_grad_(True)
        x = s64 * (a64 @ b64.t())
        if mode == "softmax":
            ref = F.cross_entropy(x, torch.arange(M, device=dev))
        else:
            z = torch.full_like(x, -1.0)
            z.fill_diagonal_(1.0)
            ref = -F.logsigmoid(z * (x + args.bias)).sum()
        ref.backward()

        def rel(out, r):
            return ((out.double() - r).abs().max() / r.abs().max()).item()

        for name, fn in variants(mode, a, b, scale, bias).items():
            step(fn, (a, b, scale, bias))
            loss = fn().item()
            _emit(mode=mode, M=M, N=N, D=D, scale=args.err_scale, variant=name,
                  loss_abs_err=abs(loss - ref.item()), loss_ref=ref.item(),
                  dA_max_norm_err=rel(a.grad, a64.grad), dB_max_norm_err=rel(b.grad, b64.grad),
                  dscale_abs_err=abs(scale.grad.item() - s64.grad.item()),
                  dscale_ref=s64.grad.item())
        del a, b, a64, b64, x


if __name__ == "__main__":
    main()
