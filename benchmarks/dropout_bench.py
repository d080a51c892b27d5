"""Cost of dropout on the fused encoder path (profiles/dropout_NOTES.md).

    python benchmarks/dropout_bench.py --mode gemm
    python benchmarks/dropout_bench.py --mode e2e --dropout 0.1 --graph 1

--mode gemm  the two MLP GEMMs at ViT-B/16 b256 (M = 50432): the call with
             p = 0, the call with the mask fused into the epilogue, and the
             unfused alternative (p = 0 GEMM, then dropout_fwd over what the
             GEMM wrote). Variants alternate inside every round; the table
             gives the median and the range of the rounds.
--mode e2e   ViT-B/16@224 train step at the given dropout rate, eager or
             captured; per-round step times, median and range.

--root DIR puts another checkout (with its built extension) first on the
import path, so the same script times the parent commit; what that checkout
lacks (dropout_fwd, the p argument) is reported as absent, never emulated.
One JSON line per measurement on stdout.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["gemm", "e2e"], required=True)
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    ap.add_argument("--tag", default="this")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20, help="gemm: calls per round and variant")
    ap.add_argument("--p", type=float, default=0.1, help="gemm: dropout probability")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dropout", type=float, default=0.1, help="e2e: model dropout_rate")
    ap.add_argument("--graph", choices=["0", "1"], default="0")
    ap.add_argument("--steps", type=int, default=10, help="e2e: steps per round")
    ap.add_argument("--warmup", type=int, default=5)
    return ap.parse_args()


def _summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "rounds": len(xs)}


def _emit(**kw):
    print(json.dumps(kw), flush=True)


def bench_gemm(args, torch, ext):
    dev = torch.device("cuda:0")
    M, H, MLP = 197 * args.batch, 768, 3072
    g = torch.Generator(device="cuda").manual_seed(0)
    h2 = torch.randn(M, H, device=dev, generator=g).bfloat16()
    w1 = (torch.randn(MLP, H, device=dev, generator=g) / H ** 0.5).bfloat16()
    b1 = torch.randn(MLP, device=dev, generator=g).bfloat16()
    w2 = (torch.randn(H, MLP, device=dev, generator=g) / MLP ** 0.5).bfloat16()
    b2 = torch.randn(H, device=dev, generator=g).bfloat16()
    res = torch.randn(M, H, device=dev, generator=g).bfloat16()
    f_in = torch.randn(M, MLP, device=dev, generator=g).bfloat16()
    rng = torch.tensor([1234, 0], dtype=torch.int64, device=dev)
    has_drop = hasattr(ext, "dropout_fwd")
    p = args.p

    def fc1_plain():
        return ext.linear_fwd_actgrad(h2, w1, b1, "gelu", None)

    def fc2_plain():
        return ext.linear_fwd(f_in, w2, b2, "", res, False)

    variants = {"fc1 p=0": fc1_plain, "fc2 p=0": fc2_plain}
    if has_drop:
        f0, _ = fc1_plain()
        y0, _ = fc2_plain()

        def fc1_unfused():
            # g is fp16; dropout_fwd moves it as 2-byte elements (same traffic)
            f, gg = fc1_plain()
            return ext.dropout_fwd(f, p, rng, 0), ext.dropout_fwd(gg.view(torch.bfloat16), p, rng, 0)

        def fc2_unfused():
            y, _ = fc2_plain()
            return ext.dropout_fwd(y, p, rng, 1)

        variants.update({
            "fc1 fused": lambda: ext.linear_fwd_actgrad(h2, w1, b1, "gelu", None, p, rng, 0),
            "fc1 unfused": fc1_unfused,
            "fc2 fused": lambda: ext.linear_fwd(f_in, w2, b2, "", res, False, p, rng, 1),
            "fc2 unfused": fc2_unfused,
            "dropout_fwd (M,3072)": lambda: ext.dropout_fwd(f0, p, rng, 0),
            "dropout_fwd (M,768)": lambda: ext.dropout_fwd(y0, p, rng, 1),
        })

    for fn in variants.values():  # warm up every shape and code object
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():  # alternate the variants inside a round
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.iters):
                fn()
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop) * 1000.0 / args.iters)
    for name, xs in times.items():
        _emit(mode="gemm", tag=args.tag, variant=name, M=M, p=p, unit="us/call", **_summary(xs))


def bench_e2e(args, torch, jimm_amd):
    from jimm_amd.ops._backend import maybe_enable_tunableop
    from jimm_amd.train import SyntheticImages, TrainConfig, Trainer

    maybe_enable_tunableop()
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    model = jimm_amd.VisionTransformer(num_classes=1000, img_size=224, patch_size=16,
                                       dropout_rate=args.dropout).to(dev, torch.bfloat16)
    tr = Trainer(model, TrainConfig(task="vit"))
    it = iter(SyntheticImages(args.batch, 224, 1000, dev, dtype=torch.bfloat16, seed=0))
    if args.graph == "1":
        tr.enable_graph(next(it))
    for _ in range(args.warmup):
        tr.train_step(next(it))
    torch.cuda.synchronize()
    rounds = []
    last = None
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        for _ in range(args.steps):
            last = tr.train_step(next(it))
        torch.cuda.synchronize()
        rounds.append((time.perf_counter() - t0) * 1000.0 / args.steps)
    _emit(mode="e2e", tag=args.tag, dropout=args.dropout, graph=args.graph == "1", batch=args.batch,
          unit="ms/step", loss=float(last["loss"]), **_summary(rounds))


def main():
    args = _args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch

    import jimm_amd
    from jimm_amd.ops import _backend

    assert torch.cuda.is_available(), "dropout_bench measures on the GPU only"
    assert os.path.abspath(os.path.dirname(os.path.dirname(jimm_amd.__file__))) == os.path.abspath(args.root)
    if args.mode == "gemm":
        bench_gemm(args, torch, _backend.ext())
    else:
        bench_e2e(args, torch, jimm_amd)


if __name__ == "__main__":
    main()
