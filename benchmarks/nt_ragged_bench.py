"""Forward, dX and fc2-dX GEMMs that neither the 8-phase grid kernel nor the
128-tile NT kernel serves (SigLIP-so400m's block, the long-K sites of ViT-S /
ViT-Ti): the ragged 8-phase kernel (gemm_nt_8p_ragged, csrc/gemm8p.hip)
against the route these sites took before it (addmm, or matmul + the
bias_act_fwd / act_bwd pass, TunableOp set up as the trainer sets it up) and
against ext.linear_fwd where it takes the shape (K % 64 == 0; no fc2-dX form).
One process, alternating timing rounds, device events; median [min-max] ms per
call and 2*M*N*K / time. dX contenders include their weight transpose copy.
Before timing, the new kernel's result is compared with the old route's at the
timed size.

Sections: the eight so400m block sites at M = 64*729, 64*256 and 1024*64; the
ViT-S / ViT-Ti sites rocBLAS holds; a row ladder on so400m fc1, proj and fc2-dX (the
routing's row floor); with --block one so400m EncoderBlock, forward + backward:
default routing, the ragged kernel switched off (row floor out of reach) and
JIMM_AMD_GEMM=blas.

Run: python benchmarks/nt_ragged_bench.py [--rounds 5] [--iters 20] [--block]
"""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from benchmarks.nt_offgrid_bench import alternate, first, fmt  # noqa: E402
from jimm_amd.ops import _backend, hip_linear  # noqa: E402

H, MLP = 1152, 4304  # so400m
BLOCK_SITES = [  # (site, N, K, kind)
    ("qkv fwd", 3 * H, H, "bias"), ("proj fwd", H, H, "res"), ("fc1 fwd", MLP, H, "act"),
    ("fc2 fwd", H, MLP, "res"), ("qkv dX", H, 3 * H, "dx"), ("proj dX", H, H, "dx"),
    ("fc1 dX", H, MLP, "dx"), ("fc2 dX", MLP, H, "dxact"),
]
OTHER_SITES = [  # (model, M, site, N, K, kind): what rocBLAS still holds of ViT-S / ViT-Ti
    ("ViT-S", 201728, "fc2 fwd", 384, 1536, "res"), ("ViT-S", 201728, "fc1 dX", 384, 1536, "dx"),
    ("ViT-S", 201728, "qkv dX", 384, 1152, "dx"),
    ("ViT-Ti", 201728, "fc2 fwd", 192, 768, "res"), ("ViT-Ti", 201728, "fc1 dX", 192, 768, "dx"),
]
LADDER = [512, 1024, 2048, 4096, 8192, 16384, 32768]


def rnd(*shape, scale=1.0):
    return ((torch.rand(*shape, device="cuda") * 2 - 1) * scale).bfloat16()


def contenders(ext, M, N, K, kind):
    """[(name, fn)]: the ragged kernel ("8pr", first), the parent route
    ("blas"), and linear_fwd where it takes the shape."""
    x, w, b = rnd(M, K), rnd(N, K, scale=K ** -0.5), rnd(N)
    old_hip = K % 64 == 0
    if kind in ("bias", "res", "act"):
        res = rnd(M, N) if kind == "res" else None
        act = "gelu_tanh" if kind == "act" else None
        v = [("8pr", lambda: ext.gemm_nt_8p_ragged(x, w, b, act or "", res,
                                                   "grad" if act else "none")),
             ("blas", lambda: hip_linear.gemm_fwd(ext, x, w, b, act, res, hip=False,
                                                  save="z" if act else None))]
        if old_hip:
            v.append(("linear_fwd", lambda: hip_linear.gemm_fwd(
                ext, x, w, b, act, res, hip=True, save="g" if act else None)))
    elif kind == "dx":
        wd = w.t().contiguous()  # the (out, in) weight whose dX this is: dz @ wd
        v = [("8pr", lambda: ext.gemm_nt_8p_ragged(x, wd.t().contiguous())),
             ("blas", lambda: torch.matmul(x, wd))]
        if old_hip:
            v.append(("linear_fwd", lambda: ext.linear_fwd(x, wd.t().contiguous(), None, "", None,
                                                           False)))
    else:
        wd = w.t().contiguous()
        z = rnd(M, N, scale=2.0)
        g = (torch.rand(M, N, device="cuda") * 1.3 - 0.17).half()
        v = [("8pr", lambda: ext.gemm_nt_8p_ragged_gradact(x, wd.t().contiguous(), z, "gelu_tanh")),
             ("8pr gradmul", lambda: ext.gemm_nt_8p_ragged_gradmul(x, wd.t().contiguous(), g)),
             ("blas", lambda: ext.act_bwd(torch.matmul(x, wd), z, "gelu_tanh"))]
    return v


def run_site(ext, label, M, N, K, kind, a):
    v = contenders(ext, M, N, K, kind)
    ours, theirs = first(v[0][1]()), first(dict(v)["blas"]())
    diff = ((ours - theirs).abs().max() / theirs.abs().max()).item()
    del ours, theirs
    print(f"\n{label} M={M} N={N} K={K}: max |8pr - blas| / max |blas| = {diff:.2e}")
    times = alternate(v, a.rounds, a.iters)
    for name, _ in v:
        print(f"  {name:12s} {fmt(times[name], 2 * M * N * K / 1e9)}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--block", action="store_true", help="also time one so400m encoder block")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    ext = _backend.ext()
    _backend.maybe_enable_tunableop()
    print(f"{a.rounds} alternating rounds of {a.iters} calls, median [min-max]")
    for M in (64 * 729, 64 * 256, 1024 * 64):
        for site, N, K, kind in BLOCK_SITES:
            run_site(ext, f"so400m {site}", M, N, K, kind, a)
    for model, M, site, N, K, kind in OTHER_SITES:
        run_site(ext, f"{model} {site}", M, N, K, kind, a)
    for M in LADDER:
        for site, N, K, kind in (BLOCK_SITES[2], BLOCK_SITES[1], BLOCK_SITES[7]):
            run_site(ext, f"ladder {site}", M, N, K, kind, a)
    if not a.block:
        return
    from jimm_amd.models.common.transformer import EncoderBlock

    B, L = 64, 729
    blk = EncoderBlock(H, 16, MLP, hidden_act="gelu_tanh", layernorm_epsilon=1e-6)
    blk = blk.to("cuda", torch.bfloat16)
    x = torch.randn(B, L, H, device="cuda").bfloat16().requires_grad_(True)
    dy = torch.randn(B, L, H, device="cuda").bfloat16()

    def step(mode, floor=hip_linear._NT8PR_MIN_M):
        os.environ["JIMM_AMD_GEMM"] = mode
        hip_linear._NT8PR_MIN_M = floor
        blk(x).backward(dy)

    times = alternate([("default", lambda: step("hip")),
                       ("no 8pr", lambda: step("hip", 1 << 62)),
                       ("blas", lambda: step("blas"))], a.rounds, max(a.iters // 4, 3))
    step("hip")
    os.environ.pop("JIMM_AMD_GEMM")
    print(f"\nso400m encoder block fwd+bwd, x = ({B}, {L}, {H})")
    for v in times:
        m = statistics.median(times[v])
        print(f"  {v:12s} {m:7.3f} [{min(times[v]):.3f}-{max(times[v]):.3f}] ms", flush=True)


if __name__ == "__main__":
    main()
