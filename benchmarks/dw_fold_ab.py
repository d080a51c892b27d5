"""A/B of builds of the extension on the dW kernel (csrc/gemm_tn8p.hip), in
one process: gemm_tn_8p (plain) and gemm_tn_8p_db (with the bias fold, the
variant the train step runs) on the twelve shapes of
profiles/dw_pipeline_NOTES.md section 3, at the chooser's split count.
Interleaved timing rounds, median [min-max] per build and variant, and the
cost of the fold (db minus plain) per build.

Every --other is another jimm_amd/_hip*.so, e.g. the parent commit's built
in a separate checkout; all are loaded side by side (extension modules are
keyed by path, the kernels live in anonymous namespaces). Without --other
this build is timed alone (plain against db).

With --check, dW of every other build must be torch.equal to this build's
(the split count is the same function of the shape in all of them) and db
must agree to 1e-5 of its largest element (an atomic sum).

Run: python benchmarks/dw_fold_ab.py [--other /path/to/_hip.so]... [--check]
         [--rounds 5] [--iters 10]
"""

import argparse
import importlib.machinery
import importlib.util
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from benchmarks.gemm8p_build_ab import t_ms  # noqa: E402
from jimm_amd.ops import _backend  # noqa: E402


def load_ext(path, name):
    """Another build of the extension. Every build needs a module name of its
    own (the interpreter hands back a loaded extension module by name); the
    part behind the last dot is the one the file's init symbol carries."""
    loader = importlib.machinery.ExtensionFileLoader(name, path)
    spec = importlib.util.spec_from_file_location(name, path, loader=loader)
    mod = importlib.util.module_from_spec(spec)
    loader.exec_module(mod)
    return mod

SHAPES = [  # (name, M, N, Kw, dW calls per bench.py step or 0)
    ("ViT-B qkv", 201728, 2304, 768, 12),
    ("ViT-B proj", 201728, 768, 768, 12),
    ("ViT-B fc1", 201728, 3072, 768, 12),
    ("ViT-B fc2", 201728, 768, 3072, 12),
    ("ViT-L qkv", 73856, 3072, 1024, 0),
    ("ViT-L proj", 73856, 1024, 1024, 0),
    ("ViT-L fc1", 73856, 4096, 1024, 0),
    ("ViT-L fc2", 73856, 1024, 4096, 0),
    ("CLIP text proj", 78848, 512, 512, 0),
    ("CLIP text qkv", 78848, 1536, 512, 0),
    ("CLIP text fc1", 78848, 2048, 512, 0),
    ("CLIP vision proj", 51200, 768, 768, 0),
]


def fmt(ts):
    return f"{statistics.median(ts):6.3f} [{min(ts):.3f}-{max(ts):.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", action="append", default=[], help="another build's _hip*.so")
    ap.add_argument("--check", action="store_true", help="compare dW bitwise and db to 1e-5")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    builds = [("this", _backend.ext())]
    for i, path in enumerate(a.other):
        tag = f"other{i}" if len(a.other) > 1 else "other"
        builds.append((tag, load_ext(path, f"{tag}._hip")))
    for tag, e in builds:
        print(f"{tag:7s} = {e.__file__}")
    assert len({e.__file__ for _, e in builds}) == len(builds)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    variants = [("plain", lambda e, dz, x: e.gemm_tn_8p(dz, x, 0, True)),
                ("db", lambda e, dz, x: e.gemm_tn_8p_db(dz, x, 0, True))]
    print(f"{a.rounds} interleaved rounds of {a.iters} calls, ms: median [min-max]; bf16 dW out")
    ok = True
    for name, M, N, K, calls in SHAPES:
        dz = (torch.rand(M, N, device="cuda") * 2 - 1).bfloat16()
        x = ((torch.rand(M, K, device="cuda") * 2 - 1) / 8).bfloat16()
        split = builds[0][1].gemm_tn8p_choose_splitm(M, (N // 256) * (K // 256), cus)
        tf = 2 * M * N * K / 1e9  # TF/s = tf / ms
        print(f"\n{name} {N}x{K} M={M} split {split}" + (f" ({calls} calls/step)" if calls else ""))
        if a.check:
            dw0, db0 = builds[0][1].gemm_tn_8p_db(dz, x, 0, False)
            pl0 = builds[0][1].gemm_tn_8p(dz, x, 0, False)
            for tag, e in builds[1:]:
                dw, db = e.gemm_tn_8p_db(dz, x, 0, False)
                eq = torch.equal(dw, dw0) and torch.equal(e.gemm_tn_8p(dz, x, 0, False), pl0)
                dberr = ((db - db0).abs().max() / db0.abs().max()).item()
                ok &= eq and dberr < 1e-5
                print(f"  check {tag}: dW equal = {eq}, db rel diff = {dberr:.2e}")
            eq = torch.equal(dw0, pl0)
            ok &= eq
            print(f"  check this: dW of db variant equal to plain = {eq}")
            del dw0, db0, pl0
        times = {(tag, v): [] for tag, _ in builds for v, _ in variants}
        for tag, e in builds:  # warm up, raise the LDS limits
            for v, f in variants:
                t_ms(lambda: f(e, dz, x), 3)
        for _ in range(a.rounds):
            for v, f in variants:
                for tag, e in builds:
                    times[tag, v].append(t_ms(lambda: f(e, dz, x), a.iters))
        for tag, _ in builds:
            p, d = times[tag, "plain"], times[tag, "db"]
            mp, md = statistics.median(p), statistics.median(d)
            print(f"  {tag:7s} plain {fmt(p)} {tf / mp:5.0f} TF/s   db {fmt(d)} {tf / md:5.0f} TF/s"
                  f"   fold {md - mp:+.3f}" + (f" = {calls * (md - mp):+.2f} ms/step" if calls else ""),
                  flush=True)
        del dz, x
    if not ok:
        sys.exit("results differ between the builds")


if __name__ == "__main__":
    main()
