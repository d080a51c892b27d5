"""dW at SigLIP-so400m's four weight sites: the ragged 256-tile TN kernel
(gemm_tn_8p_ragged, csrc/gemm_tn8p.hip) against the 128-tile TN kernel
(csrc/gemm_tn128.hip) and torch.matmul(dz.t(), x) (+ the colsum kernel where
db is needed), for dW alone and dW + db, in one process with alternating
timing rounds. Per site, M and variant: median [min-max] ms per call over the
rounds and the rate 2*M*N*K / time; the [min-max] of one variant over the
rounds is the run-to-run spread a difference has to exceed. TunableOp is set
up as the trainer and bench.py set it up.

The yardstick of a site is the engine gemm_dw_db runs there without the ragged
kernel (the 128-tile kernel up to its tile caps, else torch.matmul): the line
"vs parent" gives the ragged kernel's median over that engine's, and "ahead"
only where the two [min-max] ranges do not overlap.

Before timing, dW of the ragged kernel and of torch.matmul (bf16 out) are
compared at the timed size: the largest difference over the largest |dW|.

Run: python benchmarks/dw_ragged_bench.py [--rounds 7] [--iters 20]
         [--m 16384,46656,65536] [--only fc1]
"""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from benchmarks.gemm8p_build_ab import t_ms  # noqa: E402
from jimm_amd.ops import _backend, hip_linear  # noqa: E402

SITES = [  # (name, N, Kw)
    ("fc1", 4304, 1152),
    ("fc2", 1152, 4304),
    ("qkv", 3456, 1152),
    ("proj", 1152, 1152),
]


def fmt(ts, tf):
    m = statistics.median(ts)
    return f"{m:7.3f} [{min(ts):.3f}-{max(ts):.3f}] ms {tf / m:5.0f} TF/s"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--m", default="16384,46656,65536", help="row counts, comma-separated")
    ap.add_argument("--only", default="", help="substring of the site names to run")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    ext = _backend.ext()
    _backend.maybe_enable_tunableop()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"{a.rounds} alternating rounds of {a.iters} calls, median [min-max]; bf16 dW out; "
          f"{cus} CUs")
    for name, N, K in SITES:
        if a.only not in name:
            continue
        t128 = -(-N // 128) * -(-K // 128)
        t256 = -(-N // 256) * -(-K // 256)
        fill = N * K / (65536 * t256)
        for M in map(int, a.m.split(",")):
            dz = (torch.rand(M, N, device="cuda") * 2 - 1).bfloat16()
            x = ((torch.rand(M, K, device="cuda") * 2 - 1) / 8).bfloat16()
            tf = 2 * M * N * K / 1e9  # TF/s = tf / ms
            variants = {
                ("dW", "tn8pr"): lambda: ext.gemm_tn_8p_ragged(dz, x, 0, True),
                ("dW", "tn128"): lambda: ext.gemm_tn_128(dz, x, 0, True),
                ("dW", "blas"): lambda: torch.matmul(dz.t(), x),
                ("dW+db", "tn8pr"): lambda: ext.gemm_tn_8p_ragged_db(dz, x, 0, True),
                ("dW+db", "tn128"): lambda: ext.gemm_tn_128_db(dz, x, 0, True),
                ("dW+db", "blas"): lambda: (torch.matmul(dz.t(), x),
                                            ext.colsum(dz).to(dz.dtype)),
            }
            ours, theirs = variants["dW", "tn8pr"]().float(), variants["dW", "blas"]().float()
            diff = ((ours - theirs).abs().max() / theirs.abs().max()).item()
            del ours, theirs
            split = ext.gemm_tn8p_choose_splitm(M, t256, cus)
            print(f"\nso400m {name} {N}x{K} M={M}: {t256} tiles of 256 (fill {fill:.3f}), "
                  f"split {split}; {t128} tiles of 128; "
                  f"max |dW - blas dW| / max |dW| = {diff:.2e}")
            times = {v: [] for v in variants}
            for f in variants.values():  # warm up: code objects, LDS limits, algorithm choice
                t_ms(f, 3)
            for _ in range(a.rounds):
                for v, f in variants.items():
                    times[v].append(t_ms(f, a.iters))
            for what, cap in (("dW", hip_linear._TN128_MAX_TILES),
                              ("dW+db", hip_linear._TN128_MAX_TILES_DB)):
                for eng in ("tn8pr", "tn128", "blas"):
                    print(f"  {what:5s} {eng:5s} {fmt(times[what, eng], tf)}")
                parent = "tn128" if t128 <= cap else "blas"
                new, old = times[what, "tn8pr"], times[what, parent]
                verdict = ("ahead" if max(new) < min(old) else
                           "behind" if min(new) > max(old) else "within the spread")
                print(f"  {what:5s} vs parent ({parent}): "
                      f"{statistics.median(new) / statistics.median(old):.3f}x the time, {verdict}",
                      flush=True)
            del dz, x


if __name__ == "__main__":
    main()
