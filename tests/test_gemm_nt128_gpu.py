"""128-tile NT kernel (csrc/gemm_nt128.hip): Y = epilogue(X @ W^T) for shapes
off the 256 grid, against fp64 on the same bf16 inputs, its domain checks, and
the routes of the fused encoder block and ``ops.linear`` to it.

Bounds: bf16 products are exact in fp32, only the sums round, so with
mag = |X| @ |W|^T the fp32 pre-activation lies within
e = K * 2^-23 * mag + 2^-24 * |bias| of the reference (2^-23, not 2^-24: the
MFMA need not round to nearest). A bf16 result adds 2^-8 * |ref|, an fp16 one
2^-11 * |ref| + 2^-24; an activation scales e by at most |act'| <= 1.13 and
adds the fast erf / exp error, 2e-6; |act''| < 1 carries e into the saved
derivative. A dropped k-column or a misplaced output column is off by about
mag / K. Inputs carry a per-column offset so that swapped columns differ.
"""

import pytest
import torch

import jimm_amd  # noqa: F401
import jimm_amd.ops.functional as Fn
from jimm_amd.ops import _backend

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
BF16 = 2.0 ** -8
FORMS = ["plain", "gelu_z", "quick_g", "bias_res", "gradmul", "gradact"]


@pytest.fixture(scope="module")
def ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _backend.ext()  # fail loudly — never silently skip to eager on a GPU box


def operand(M, W, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.randn(M, W, device="cuda", generator=g)
    return (t + 0.01 * torch.arange(W, device="cuda")).bfloat16()


def assert_within(out, ref, bound, what):
    excess = ((out.double() - ref).abs() - bound).max().item()
    print(f"{what}: max |err| {(out.double() - ref).abs().max().item():.3e}, "
          f"max (|err| - bound) {excess:.3e}")
    assert out.shape == ref.shape and excess <= 0, (what, excess)


@pytest.mark.parametrize("M,N,K,form", [
    (1, 8, 8, "plain"),             # tail only: every row clamped, register-staged K alone
    (1, 8, 8, "bias_res"),
    (128, 128, 64, "plain"),        # one exact tile: ring only, no tail, no edge
    (128, 128, 64, "gelu_z"),
    (64, 64, 56, "plain"),          # one unit + a 24-column tail
    *[(200, 136, 232, f) for f in FORMS],  # ragged M, 8-column n-tile, 7 units + 8-column tail
    (256, 384, 384, "plain"),       # ViT-S proj: full tiles, 3 n-tiles
    (256, 384, 384, "quick_g"),
    (130, 1152, 4304, "plain"),     # so400m fc2: 134 units + 16-column tail
    (130, 1152, 4304, "gradmul"),
    (264, 4304, 1152, "plain"),     # so400m's mlp width as N: 34 n-tiles, the last of 80
    (264, 4304, 1152, "gradact"),
])
def test_against_fp64(ext, M, N, K, form):
    x, w = operand(M, K, 11 + M + K), (operand(N, K, 23 + N + K) * 0.03).bfloat16()
    acc, mag = x.double() @ w.double().t(), x.double().abs() @ w.double().abs().t()
    assert ext.gemm_nt_128_supported(M, N, K)
    b16, b32 = operand(1, N, 3)[0], operand(1, N, 4)[0].float() * 0.5
    res = operand(M, N, 5)
    if form == "plain":
        y, z = ext.gemm_nt_128(x, w)
        assert z is None and y.dtype == torch.bfloat16
        assert_within(y, acc, K * EPS * mag + BF16 * acc.abs(), "y")
        assert torch.equal(y, ext.gemm_nt_128(x, w)[0])
    elif form == "bias_res":
        ref = acc + b16.double() + res.double()
        e = K * EPS * mag + 2.0 ** -24 * b16.double().abs()
        y, _ = ext.gemm_nt_128(x, w, b16, "", res)
        assert_within(y, ref, e + BF16 * ref.abs(), "y")
        assert torch.equal(y, ext.gemm_nt_128(x, w, b16, "", res, "pre")[0])
    elif form in ("gelu_z", "quick_g"):
        act, bias = ("gelu", b16) if form == "gelu_z" else ("quickgelu", b32)
        pre = (acc + bias.double()).requires_grad_(True)
        yref = Fn._act(pre, act)
        (gref,) = torch.autograd.grad(yref.sum(), pre)
        pre, yref = pre.detach(), yref.detach()
        e = K * EPS * mag + 2.0 ** -24 * bias.double().abs()
        y_n, none = ext.gemm_nt_128(x, w, bias, act)
        y_z, z = ext.gemm_nt_128(x, w, bias, act, None, "pre")
        y_g, g = ext.gemm_nt_128(x, w, bias, act, None, "grad")
        assert none is None and z.dtype == torch.bfloat16 and g.dtype == torch.float16
        assert torch.equal(y_n, y_z) and torch.equal(y_n, y_g)  # mfma.h's promise
        assert_within(y_n, yref, 1.13 * e + 2e-6 + BF16 * yref.abs(), "y")
        assert_within(z, pre, 1.13 * e + 2e-6 + BF16 * pre.abs(), "z")
        assert_within(g, gref, e + 2e-6 + 2.0 ** -11 * gref.abs() + 2.0 ** -24, "g")
        assert torch.equal(g, ext.gemm_nt_128(x, w, bias, act, None, "grad")[1])
    elif form == "gradmul":
        gen = torch.Generator(device="cuda").manual_seed(9)
        g = (torch.rand(M, N, device="cuda", generator=gen) * 1.3 - 0.17).half()
        ref = acc * g.double()
        y = ext.gemm_nt_128_gradmul(x, w, g)
        assert_within(y, ref, K * EPS * mag * g.double().abs() + BF16 * ref.abs(), "dz")
        assert torch.equal(y, ext.gemm_nt_128_gradmul(x, w, g))
    else:
        gen = torch.Generator(device="cuda").manual_seed(10)
        z = torch.randn(M, N, device="cuda", generator=gen).bfloat16()
        zd = z.double().requires_grad_(True)
        (dact,) = torch.autograd.grad(Fn._act(zd, "gelu_tanh").sum(), zd)
        ref = acc * dact
        y = ext.gemm_nt_128_gradact(x, w, z, "gelu_tanh")
        assert_within(y, ref, K * EPS * mag * dact.abs() + 2e-6 * acc.abs() + BF16 * ref.abs(),
                      "dz")
        assert torch.equal(y, ext.gemm_nt_128_gradact(x, w, z, "gelu_tanh"))


def test_domain_edge(ext):
    assert not ext.gemm_nt_128_supported(64, 100, 128)
    assert not ext.gemm_nt_128_supported(64, 128, 36)
    with pytest.raises(RuntimeError):
        ext.gemm_nt_128(operand(64, 128, 1), operand(100, 128, 2))
    with pytest.raises(RuntimeError):
        ext.gemm_nt_128(operand(64, 36, 1), operand(128, 36, 2))
    with pytest.raises(RuntimeError):
        ext.gemm_nt_128_gradmul(operand(64, 36, 1), operand(128, 36, 2),
                                operand(64, 128, 3).half())


@pytest.fixture
def calls(ext, monkeypatch):
    """The names of the extension / torch GEMM calls, in call order."""
    for name in ("JIMM_AMD_ACT_SAVE", "JIMM_AMD_GEMM", "JIMM_AMD_DETERMINISTIC",
                 "JIMM_AMD_FUSED_BLOCK"):
        monkeypatch.delenv(name, raising=False)
    rec = []

    def spy(owner, name, label):
        def f(*a, _f=getattr(owner, name), **kw):
            rec.append(label)
            return _f(*a, **kw)
        monkeypatch.setattr(owner, name, f)

    for name in dir(ext):
        if not name.startswith("_") and not name.endswith("_supported") \
                and callable(getattr(ext, name)):
            spy(ext, name, name)
    for name in ("matmul", "addmm"):
        spy(torch, name, "torch." + name)
    return rec


@pytest.mark.parametrize("H,heads,mlp,nt128,blas", [
    # The measured routing (profiles/nt_offgrid_NOTES.md) leaves every site
    # with K > 576 on rocBLAS. ViT-S: qkv, proj and proj-dX on the new kernel;
    # fc2 (K = 1536), fc1-dX (1536) and qkv-dX (1152) stay matmul.
    (384, 6, 1536, 3, 3),
    # ViT-Ti: qkv-dX (K = 576) joins; fc2 and fc1-dX (768) stay.
    (192, 3, 768, 4, 2),
    # so400m: H = 1152 is beyond the cap, forward and fc2-dX stay on rocBLAS.
    (1152, 16, 4304, 0, None),
])
def test_block_routes(calls, monkeypatch, H, heads, mlp, nt128, blas):
    """EncoderBlock forward + backward, M = 256: the sites the measured
    routing gives to the in-house kernels run there (fc1 and fc2-dX of ViT-S /
    Ti are 8-phase shapes), no activation pass runs on its own, and the result
    agrees with the block on rocBLAS at the thresholds of
    test_block_mlp_not_multiple_of_256."""
    from jimm_amd.models.common.transformer import EncoderBlock

    torch.manual_seed(3)
    blk = EncoderBlock(H, heads, mlp, hidden_act="gelu", layernorm_epsilon=1e-6)
    blk = blk.to("cuda", torch.bfloat16)
    x = torch.randn(2, 128, H, device="cuda").bfloat16()
    dy = torch.randn_like(x)
    out = {}
    for mode in ("hip", "blas"):
        monkeypatch.setenv("JIMM_AMD_GEMM", mode)
        for p in blk.parameters():
            p.grad = None
        xi = x.detach().clone().requires_grad_(True)
        calls.clear()
        y = blk(xi)
        y.backward(dy)
        torch.cuda.synchronize()
        out[mode] = (list(calls), y.detach(), xi.grad.clone(),
                     {n: p.grad.clone() for n, p in blk.named_parameters()})
    trace, y, dx, grads = out["hip"]
    print(f"trace: {trace!r}")
    assert trace.count("gemm_nt_128") == nt128, trace
    if blas is None:
        # (the forward's 10 calls and fc2-dX; dW keeps its own per-shape rule)
        assert trace[:10] == out["blas"][0][:10] and "act_bwd" in trace, trace
    else:
        assert trace.count("torch.matmul") == blas and "torch.addmm" not in trace, trace
        assert "act_bwd" not in trace and trace.count("bias_act_fwd") == 1, trace  # fc2's
        assert "linear_fwd_actgrad" in trace and "gemm_nt_8p_gradmul" in trace, trace

    def rel_err(a, ref):
        return (a.float() - ref.float()).abs().max().item() / max(ref.float().abs().max().item(),
                                                                  1e-6)

    _, y_b, dx_b, grads_b = out["blas"]
    errs = {n: rel_err(grads[n], grads_b[n]) for n in grads}
    print(f"y {rel_err(y, y_b):.3e} dx {rel_err(dx, dx_b):.3e} "
          + " ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert len(grads) == 12
    assert rel_err(y, y_b) < 1e-2 and rel_err(dx, dx_b) < 2e-2
    assert all(e < 3e-2 for e in errs.values()), errs
    if H == 384:  # below the row floor the block stays where it was
        xs = x[:, :40].detach().clone().requires_grad_(True)
        monkeypatch.setenv("JIMM_AMD_GEMM", "hip")
        calls.clear()
        blk(xs).backward(dy[:, :40])
        assert "torch.matmul" in calls and "gemm_nt_128" not in calls, calls


@pytest.mark.parametrize("K,route", [(328, "gemm_nt_128"), (4304, "torch.addmm")])
def test_linear_route(calls, K, route):
    """ops.linear, M = 256, in_features no multiple of 64: the forward is the
    128-tile NT kernel's within its K cap; so400m's 4304 measured behind
    rocBLAS (profiles/nt_offgrid_NOTES.md) and stays there."""
    from jimm_amd.ops import linear

    x = operand(256, K, 5)
    w = (operand(1152, K, 6) * 0.03).bfloat16().requires_grad_(True)
    b = operand(1, 1152, 7)[0].requires_grad_(True)
    calls.clear()
    y = linear(x, w, b)
    torch.cuda.synchronize()
    assert calls == [route], calls
    ref = x.double() @ w.double().t() + b.double()
    mag = x.double().abs() @ w.double().abs().t()
    assert_within(y, ref, K * EPS * mag + 2.0 ** -24 * b.double().abs() + BF16 * ref.abs(), "y")
