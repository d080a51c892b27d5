"""dW for weight shapes off the 256 grid: the 128-tile TN kernel
(csrc/gemm_tn128.hip) against the route these shapes took before it,
torch.matmul(dz.t(), x) (+ the colsum kernel where db is needed), in one
process with alternating timing rounds. Per shape and variant: median
[min-max] ms per call over the rounds and the rate 2*M*N*K / time; the
[min-max] of one variant over the rounds is the run-to-run spread a difference
has to exceed. TunableOp is set up as the trainer and bench.py set it up.

Before timing, dW of both routes (bf16 out) is compared at the timed size:
the largest difference over the largest |dW| is printed.

--splits a,b,...: also time the kernel at those split counts (tuning the
chooser); the default times the chooser's own count only.

Run: python benchmarks/dw_offgrid_bench.py [--rounds 7] [--iters 50]
         [--splits 4,8] [--only so400m] [--shape M,N,K]...
"""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from benchmarks.gemm8p_build_ab import t_ms  # noqa: E402
from jimm_amd.ops import _backend  # noqa: E402

VITS_M = 1024 * 197
SO400M_M = 64 * 729
SHAPES = [  # (name, M, N, Kw)
    ("ViT-S proj", VITS_M, 384, 384),
    ("ViT-S qkv", VITS_M, 1152, 384),
    ("ViT-S fc1", VITS_M, 1536, 384),
    ("ViT-S fc2", VITS_M, 384, 1536),
    ("so400m proj", SO400M_M, 1152, 1152),
    ("so400m qkv", SO400M_M, 3456, 1152),
    ("so400m fc1", SO400M_M, 4304, 1152),
    ("so400m fc2", SO400M_M, 1152, 4304),
    ("class head", 1024, 1000, 768),
]


def fmt(ts, tf):
    m = statistics.median(ts)
    return f"{m:7.3f} [{min(ts):.3f}-{max(ts):.3f}] ms {tf / m:5.0f} TF/s"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--splits", default="", help="extra split counts to time, comma-separated")
    ap.add_argument("--only", default="", help="substring of the shape names to run")
    ap.add_argument("--shape", action="append", default=[], metavar="M,N,K",
                    help="time this shape instead of the list (repeatable)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    ext = _backend.ext()
    _backend.maybe_enable_tunableop()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    extra = [int(s) for s in a.splits.split(",") if s]
    print(f"{a.rounds} alternating rounds of {a.iters} calls, median [min-max]; bf16 dW out; "
          f"{cus} CUs")
    shapes = [("--shape", *map(int, s.split(","))) for s in a.shape] or SHAPES
    for name, M, N, K in shapes:
        if a.only not in name:
            continue
        dz = (torch.rand(M, N, device="cuda") * 2 - 1).bfloat16()
        x = ((torch.rand(M, K, device="cuda") * 2 - 1) / 8).bfloat16()
        tiles = -(-N // 128) * -(-K // 128)
        split = ext.gemm_tn8p_choose_splitm(M, tiles, 2 * cus)
        tf = 2 * M * N * K / 1e9  # TF/s = tf / ms
        variants = [
            ("tn128 dW", lambda: ext.gemm_tn_128(dz, x, 0, True)),
            ("blas  dW", lambda: torch.matmul(dz.t(), x)),
            ("tn128 dW+db", lambda: ext.gemm_tn_128_db(dz, x, 0, True)),
            ("blas  dW+db", lambda: (torch.matmul(dz.t(), x), ext.colsum(dz).to(dz.dtype))),
        ]
        for s in extra:
            variants.append((f"tn128 dW+db s={s}", lambda s=s: ext.gemm_tn_128_db(dz, x, s, True)))
        ours, theirs = variants[0][1]().float(), variants[1][1]().float()
        diff = ((ours - theirs).abs().max() / theirs.abs().max()).item()
        print(f"\n{name} {N}x{K} M={M}: {tiles} tiles, split {split}; "
              f"max |dW - blas dW| / max |dW| = {diff:.2e}")
        del ours, theirs
        times = {v: [] for v, _ in variants}
        for v, f in variants:  # warm up: code objects, LDS limits, library algorithm choice
            t_ms(f, 3)
        for _ in range(a.rounds):
            for v, f in variants:
                times[v].append(t_ms(f, a.iters))
        for v, _ in variants:
            print(f"  {v:18s} {fmt(times[v], tf)}", flush=True)
        del dz, x


if __name__ == "__main__":
    main()
