"""The in-house e4m3 GEMM (csrc/gemm8p_f8.hip) against hipBLASLt's e4m3 GEMM
and the bf16 8-phase kernel, on the fp8 sites of the bench models.

Per site (M, N, K) and its epilogue, on pre-quantised inputs:
  f8        ext.linear_fwd_f8, epilogue fused (one launch)
  f8_plain  ext.linear_fwd_f8 without an epilogue (GEMM only)
  mm        torch._scaled_mm on the same bytes, bias fused (GEMM only)
  mm_ep     mm + the elementwise pass the block runs after it
            (bias_act_fwd_fp8 for fc1, bias_act_fwd with the residual for fc2;
            qkv needs none)
  bf16      ext.linear_fwd (8-phase bf16 kernel), same epilogue fused

Variants alternate in one process; each sample is device-event time over
ITERS back-to-back calls. Reported: median TFLOP/s (2*M*N*K from the shape)
and the spread (max - min) / median over the rounds.

Run: python benchmarks/gemm_f8_bench.py [--rounds R] [--iters I]
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

import jimm_amd  # noqa: F401
from jimm_amd.ops import _backend

SITES = [
    # (model, site, M, N, K)
    ("ViT-B", "qkv", 201728, 2304, 768),
    ("ViT-B", "fc1", 201728, 3072, 768),
    ("ViT-B", "fc2", 201728, 768, 3072),
    ("ViT-L", "qkv", 73856, 3072, 1024),
    ("ViT-L", "fc1", 73856, 4096, 1024),
    ("ViT-L", "fc2", 73856, 1024, 4096),
]


def sample(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e-3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gemm_f8_bench needs a GPU")
    ext = _backend.ext()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    for model, site, M, N, K in SITES:
        x = torch.randn(M, K, device=dev).bfloat16()
        w = (torch.randn(N, K, device=dev) / K**0.5).bfloat16()
        b = torch.randn(N, device=dev).bfloat16()
        res = torch.randn(M, N, device=dev).bfloat16() if site == "fc2" else None
        act = "gelu" if site == "fc1" else ""
        sx = (x.abs().amax().float() / 448.0).reshape(1)
        sw = (w.abs().amax().float() / 448.0).reshape(1)
        x8 = (x.float() / sx).to(torch.float8_e4m3fn)
        w8 = (w.float() / sw).to(torch.float8_e4m3fn)
        so = torch.ones(1, device=dev)
        amax = torch.zeros(1, device=dev)

        def mm():
            return torch._scaled_mm(x8, w8.t(), scale_a=sx.view(1, 1), scale_b=sw.view(1, 1),
                                    bias=b, out_dtype=torch.bfloat16)

        def mm_ep():
            z = mm()
            if site == "fc1":
                return ext.bias_act_fwd_fp8(z, None, act, so, amax)[0]
            if site == "fc2":
                return ext.bias_act_fwd(z, None, "", res)
            return z

        fp8o = (so, amax) if site == "fc1" else (None, None)
        variants = {
            "f8": lambda: ext.linear_fwd_f8(x8, sx, w8, sw, b, act, res, bool(act), *fp8o)[0],
            "f8_plain": lambda: ext.linear_fwd_f8(x8, sx, w8, sw)[0],
            "mm": mm,
            "mm_ep": mm_ep,
            "bf16": lambda: ext.linear_fwd(x, w, b, act, res, bool(act))[0],
        }
        # same bytes, same result: the two e4m3 engines agree to output rounding
        ya, yb = variants["f8"]().float(), mm_ep().float()
        err = (ya - yb).abs().max().item() / yb.abs().max().item()
        times = {k: [] for k in variants}
        for fn in variants.values():  # warm-up: code objects, library algorithm picks
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for k, fn in variants.items():
                times[k].append(sample(fn, args.iters))
        tf = 2 * M * N * K / 1e12
        cells = []
        for k, ts in times.items():
            med = statistics.median(ts)
            cells.append(f"{k} {tf / med:6.0f} TF/s {med * 1e3:6.3f} ms +-{(max(ts) - min(ts)) / med:4.1%}")
        print(f"{model} {site} M={M} N={N} K={K} | " + " | ".join(cells)
              + f" | f8 vs mm_ep relerr {err:.1e}", flush=True)


if __name__ == "__main__":
    main()
