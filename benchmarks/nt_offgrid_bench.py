"""Forward, dX and fc2-dX GEMMs of the encoder block at widths off the 256
grid (ViT-S, ViT-Ti, SigLIP-so400m): the 128-tile NT kernel
(csrc/gemm_nt128.hip) against the route these sites took before it (addmm,
or matmul + the bias_act_fwd / act_bwd pass, TunableOp set up as the trainer
and bench.py set it up) and against ext.linear_fwd where it takes the shape
(K % 64 == 0: the 128-tile kernels of csrc/gemm.hip, or the 8-phase kernel
where N % 256 == 0 as well; neither has an off-grid fc2-dX form), and a
few bias-only forwards at the routing's row floor and at K % 64 != 0. One
process, alternating timing rounds, device events. Per site and contender:
median [min-max] ms per call over the rounds and the rate 2*M*N*K / time;
the [min-max] of one contender over the rounds is the run-to-run spread a
difference has to exceed. dX contenders include their weight transpose copy.

Before timing, the new kernel's result is compared with the old route's at
the timed size: the largest difference over the largest |value| is printed.

--block: also time one EncoderBlock, forward + backward, at each model's
shape: default routing, the same with the new kernel's row floor raised out of
reach (the routing before the kernel existed: rocBLAS forward and dX, dW on
the TN kernels), and JIMM_AMD_GEMM=blas.

Run: python benchmarks/nt_offgrid_bench.py [--rounds 5] [--iters 20]
         [--only so400m] [--block]
"""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from benchmarks.gemm8p_build_ab import t_ms  # noqa: E402
from jimm_amd.ops import _backend, hip_linear  # noqa: E402

# bias-only forwards beside the model sites: the row floor of the routing
# (M = 256, 1024) and a contraction length off the 64 grid inside the K cap
EXTRA = [(256, 1152, 384), (256, 384, 384), (1024, 1152, 384), (201728, 384, 328)]
MODELS = [  # (name, batch, tokens, hidden, heads, mlp)
    ("ViT-S", 1024, 197, 384, 6, 1536),
    ("ViT-Ti", 1024, 197, 192, 3, 768),
    ("so400m", 64, 729, 1152, 16, 4304),
]


def fmt(ts, tf):
    m = statistics.median(ts)
    return f"{m:7.3f} [{min(ts):.3f}-{max(ts):.3f}] ms {tf / m:5.0f} TF/s"


def alternate(variants, rounds, iters):
    """{name: [ms per call, one per round]}, the contenders taking turns."""
    times = {v: [] for v, _ in variants}
    for _, f in variants:  # warm up: code objects, LDS limits, library algorithm choice
        t_ms(f, 3)
    for _ in range(rounds):
        for v, f in variants:
            times[v].append(t_ms(f, iters))
    return times


def sites(ext, M, H, mlp):
    """(site name, N, K, [(contender, fn)]) for the block's 8 GEMM sites."""
    def rnd(*shape, scale=1.0):
        return ((torch.rand(*shape, device="cuda") * 2 - 1) * scale).bfloat16()

    for name, N, K, kind in [
        ("qkv fwd", 3 * H, H, "bias"), ("proj fwd", H, H, "res"), ("fc1 fwd", mlp, H, "act"),
        ("fc2 fwd", H, mlp, "res"), ("qkv dX", H, 3 * H, "dx"), ("proj dX", H, H, "dx"),
        ("fc1 dX", H, mlp, "dx"), ("fc2 dX", mlp, H, "dxact"),
    ]:
        x, w, b = rnd(M, K), rnd(N, K, scale=K ** -0.5), rnd(N)
        old_hip = K % 64 == 0  # linear_fwd's domain
        if kind in ("bias", "res", "act"):
            res = rnd(M, N) if kind == "res" else None
            act = "gelu" if kind == "act" else None
            save = "z" if act else None
            v = [("nt128", lambda: ext.gemm_nt_128(x, w, b, act or "", res,
                                                   "grad" if act else "none")),
                 ("blas", lambda: hip_linear.gemm_fwd(ext, x, w, b, act, res, hip=False, save=save))]
            if old_hip:
                v.append(("linear_fwd", lambda: hip_linear.gemm_fwd(ext, x, w, b, act, res, hip=True,
                                                                    save="g" if act else None)))
        elif kind == "dx":
            wd = w.t().contiguous()  # the (out, in) weight whose dX this is: dz @ wd
            v = [("nt128", lambda: ext.gemm_nt_128(x, wd.t().contiguous())),
                 ("blas", lambda: torch.matmul(x, wd))]
            if old_hip:
                v.append(("linear_fwd", lambda: ext.linear_fwd(x, wd.t().contiguous(), None, "", None,
                                                               False)))
        else:
            wd = w.t().contiguous()
            z = rnd(M, N, scale=2.0)
            g = (torch.rand(M, N, device="cuda") * 1.3 - 0.17).half()
            v = [("nt128 gradmul", lambda: ext.gemm_nt_128_gradmul(x, wd.t().contiguous(), g)),
                 ("nt128 gradact", lambda: ext.gemm_nt_128_gradact(x, wd.t().contiguous(), z, "gelu")),
                 ("blas", lambda: ext.act_bwd(torch.matmul(x, wd), z, "gelu"))]
        yield name, N, K, v


def first(out):
    return (out[0] if isinstance(out, (tuple, list)) else out).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default="", help="substring of the model names to run")
    ap.add_argument("--block", action="store_true", help="also time one encoder block")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    ext = _backend.ext()
    _backend.maybe_enable_tunableop()
    print(f"{a.rounds} alternating rounds of {a.iters} calls, median [min-max]")
    for M, N, K in EXTRA if not a.only else []:
        x, w, b = (((torch.rand(s, device="cuda") * 2 - 1) / 8).bfloat16()
                   for s in ((M, K), (N, K), (N,)))
        times = alternate([("nt128", lambda: ext.gemm_nt_128(x, w, b)),
                           ("blas", lambda: torch.addmm(b, x, w.t()))], a.rounds, a.iters)
        print(f"\nbias forward M={M} N={N} K={K}")
        for v in times:
            print(f"  {v:14s} {fmt(times[v], 2 * M * N * K / 1e9)}", flush=True)
    for model, B, L, H, heads, mlp in MODELS:
        if a.only not in model:
            continue
        M = B * L
        for name, N, K, variants in sites(ext, M, H, mlp):
            cmp_to = "nt128 gradact" if name == "fc2 dX" else "nt128"
            ours, theirs = first(dict(variants)[cmp_to]()), first(dict(variants)["blas"]())
            diff = ((ours - theirs).abs().max() / theirs.abs().max()).item()
            del ours, theirs
            print(f"\n{model} {name} M={M} N={N} K={K}: max |nt128 - blas| / max |blas| = {diff:.2e}")
            times = alternate(variants, a.rounds, a.iters)
            for v, _ in variants:
                print(f"  {v:14s} {fmt(times[v], 2 * M * N * K / 1e9)}", flush=True)
        if not a.block:
            continue
        from jimm_amd.models.common.transformer import EncoderBlock

        blk = EncoderBlock(H, heads, mlp, hidden_act="gelu", layernorm_epsilon=1e-6)
        blk = blk.to("cuda", torch.bfloat16)
        x = torch.randn(B, L, H, device="cuda").bfloat16().requires_grad_(True)
        dy = torch.randn(B, L, H, device="cuda").bfloat16()

        def step(mode, floor=hip_linear._NT128_MIN_M):
            os.environ["JIMM_AMD_GEMM"] = mode
            hip_linear._NT128_MIN_M = floor
            blk(x).backward(dy)

        times = alternate([("default", lambda: step("hip")),
                           ("no nt128", lambda: step("hip", 1 << 62)),
                           ("blas", lambda: step("blas"))], a.rounds, max(a.iters // 4, 3))
        step("hip")
        os.environ.pop("JIMM_AMD_GEMM")
        print(f"\n{model} encoder block fwd+bwd, x = ({B}, {L}, {H})")
        for v in times:
            m = statistics.median(times[v])
            print(f"  {v:14s} {m:7.3f} [{min(times[v]):.3f}-{max(times[v]):.3f}] ms", flush=True)
        del blk, x, dy


if __name__ == "__main__":
    main()
