"""A/B of two builds of the extension on the 8-phase NT GEMM forms, in one
process: bitwise comparison of the results, then interleaved timing rounds
(median [min-max] per build).

The second build is any other jimm_amd/_hip*.so, e.g. the parent commit's
built in a separate checkout. Both are loaded side by side (extension modules
are keyed by path, and the kernels live in anonymous namespaces).

Run: python benchmarks/gemm8p_build_ab.py --other /path/to/other/_hip.cpython-310-x86_64-linux-gnu.so
         [--m 201728] [--rounds 5] [--iters 20]
"""

import argparse
import importlib.machinery
import importlib.util
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from jimm_amd.ops import _backend  # noqa: E402


def load_ext(path):
    loader = importlib.machinery.ExtensionFileLoader("_hip", path)
    spec = importlib.util.spec_from_file_location("_hip", path, loader=loader)
    mod = importlib.util.module_from_spec(spec)
    loader.exec_module(mod)
    return mod


def t_ms(fn, iters):
    s = torch.cuda.Event(True)
    e = torch.cuda.Event(True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", required=True, help="the other build's _hip*.so")
    ap.add_argument("--m", type=int, default=201728)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    new, old = _backend.ext(), load_ext(a.other)
    assert new.__file__ != old.__file__
    print(f"this  = {new.__file__}\nother = {old.__file__}")

    M, H, F = a.m, 768, 3072
    gen = torch.Generator(device="cuda").manual_seed(0)

    def rn(*shape, scale=1.0):
        return (torch.randn(*shape, device="cuda", generator=gen) * scale).bfloat16()

    x = rn(M, H)            # block input / dy of width H
    xf = rn(M, F)           # fc2 input / dy of width F
    res = rn(M, H)
    w_qkv, b_qkv = rn(3 * H, H, scale=H ** -0.5), rn(3 * H)
    w_o, b_o = rn(H, H, scale=H ** -0.5), rn(H)
    w_fc1, b_fc1 = rn(F, H, scale=H ** -0.5), rn(F)
    w_fc2, b_fc2 = rn(H, F, scale=F ** -0.5), rn(H)
    g = (torch.rand(M, F, device="cuda", generator=gen) * 1.3 - 0.17).half()

    forms = [
        ("plain (3072,768)", lambda e: e.linear_fwd(x, w_fc1, None, "", None, False)),
        ("qkv bias (2304,768)", lambda e: e.linear_fwd(x, w_qkv, b_qkv, "", None, False)),
        ("bias+res (768,768)", lambda e: e.linear_fwd(x, w_o, b_o, "", res, False)),
        ("fc2 bias+res (768,3072)", lambda e: e.linear_fwd(xf, w_fc2, b_fc2, "", res, False)),
        ("fc1 gelu save g (3072,768)", lambda e: e.linear_fwd_actgrad(x, w_fc1, b_fc1, "gelu", None)),
        ("gradmul (3072,768)", lambda e: [e.gemm_nt_8p_gradmul(x, w_fc1, g)]),
        ("plain dX (768,3072)", lambda e: e.linear_fwd(xf, w_fc2, None, "", None, False)),
    ]

    # the remaining epilogue forms: compared, not timed
    z = rn(M, F)
    s8 = torch.ones(1, device="cuda")
    more = [(f"fc1 {act} save {'z' if sz else 'nothing'}",
             lambda e, act=act, sz=sz: e.linear_fwd(x, w_fc1, b_fc1, act, None, sz))
            for act in ("gelu", "gelu_tanh", "quickgelu") for sz in (True, False)]
    more += [(f"fc1 {act} save g",
              lambda e, act=act: e.linear_fwd_actgrad(x, w_fc1, b_fc1.float(), act, None))
             for act in ("gelu_tanh", "quickgelu")]
    more += [("gradact gelu", lambda e: [e.gemm_nt_8p_gradact(x, w_fc1, z, "gelu")]),
             ("gradact_fp8 gelu", lambda e: e.gemm_nt_8p_gradact_fp8(
                 x, w_fc1, z, "gelu", s8, torch.zeros(1, device="cuda")))]

    print(f"\nbitwise, M = {M}")
    all_equal = True
    for name, f in forms + more:
        o_new = [t for t in f(new) if t is not None]
        o_old = [t for t in f(old) if t is not None]
        eq = [torch.equal(p, q) for p, q in zip(o_new, o_old)]
        ndiff = [int((p != q).sum()) for p, q in zip(o_new, o_old)]
        all_equal &= len(o_new) == len(o_old) and all(eq)
        print(f"  {name:28s} equal per tensor = {eq}  differing elements = {ndiff}", flush=True)
        del o_new, o_old

    print(f"\ntiming, {a.rounds} interleaved rounds of {a.iters} calls, ms: median [min-max]")
    times = {(name, tag): [] for name, _ in forms for tag in ("other", "this")}
    for name, f in forms:  # warm up, raise the LDS limits
        for e in (old, new):
            t_ms(lambda: f(e), 3)
    for _ in range(a.rounds):
        for name, f in forms:
            times[name, "other"].append(t_ms(lambda: f(old), a.iters))
            times[name, "this"].append(t_ms(lambda: f(new), a.iters))
    for name, _ in forms:
        o, n = times[name, "other"], times[name, "this"]
        mo, mn = statistics.median(o), statistics.median(n)
        print(f"  {name:28s} other {mo:6.3f} [{min(o):.3f}-{max(o):.3f}]  "
              f"this {mn:6.3f} [{min(n):.3f}-{max(n):.3f}]  diff {mn - mo:+.3f}", flush=True)
    if not all_equal:
        sys.exit("results differ between the two builds")


if __name__ == "__main__":
    main()
