"""Ragged 8-phase NT kernel (gemm_nt_8p_ragged, csrc/gemm8p.hip): any M,
N % 8 == 0, K % 8 == 0, K >= 128, against fp64 on the same bf16 inputs under
the bound scheme of tests/test_gemm_nt128_gpu.py (fp32 sums within
K * 2^-23 * |X| @ |W|^T, bf16 / fp16 output rounding on top, 1.13 and 2e-6 for
the activations; operands carry a per-column offset so that swapped columns
differ), its domain checks, and the routes of the fused encoder block and
``ops.linear`` to it (profiles/nt_ragged_NOTES.md).
"""

import pytest
import torch

import jimm_amd  # noqa: F401
import jimm_amd.ops.functional as Fn
from jimm_amd.ops import _backend, hip_linear

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
BF16 = 2.0 ** -8
FORMS = ["plain", "gelu_z", "quick_g", "bias_res", "gradmul", "gradact"]
FLOOR = hip_linear._NT8PR_MIN_M


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
    (1, 8, 128, "plain"),            # one row, one 8-column group: every staging row clamped
    (256, 256, 128, "plain"),        # an exact grid shape: the bits of linear_fwd
    (256, 256, 128, "bias_res"),
    (64, 72, 160, "plain"),          # a 32-column tail: the kh = 0 pair alone
    *[(200, 136, 136, f) for f in FORMS],  # ragged M, 8 valid rows in B half 1, 8-column tail
    (260, 264, 184, "plain"),        # 4-row m-tile, 8-column n-tile, 56-column tail
    (130, 1152, 4304, "plain"),      # so400m fc2 / fc1-dX: 67 tiles + 16, last n-tile half empty
    (130, 1152, 4304, "bias_res"),
    (264, 4304, 1152, "gelu_tanh_g"),  # so400m fc1 / fc2-dX: last n-tile of 208 columns
    (264, 4304, 1152, "gradmul"),
])
def test_against_fp64(ext, M, N, K, form):
    x, w = operand(M, K, 11 + M + K), (operand(N, K, 23 + N + K) * 0.03).bfloat16()
    acc, mag = x.double() @ w.double().t(), x.double().abs() @ w.double().abs().t()
    assert ext.gemm_nt_8p_ragged_supported(M, N, K)
    b16, b32 = operand(1, N, 3)[0], operand(1, N, 4)[0].float() * 0.5
    res = operand(M, N, 5)
    grid = ext.gemm8p_supported(M, N, K)
    if form == "plain":
        y, z = ext.gemm_nt_8p_ragged(x, w)
        assert z is None and y.dtype == torch.bfloat16
        assert_within(y, acc, K * EPS * mag + BF16 * acc.abs(), "y")
        assert torch.equal(y, ext.gemm_nt_8p_ragged(x, w)[0])
        if grid:  # the same K loop: the same sums, the same bits
            assert torch.equal(y, ext.linear_fwd(x, w, None, "", None, False)[0])
    elif form == "bias_res":
        ref = acc + b16.double() + res.double()
        e = K * EPS * mag + 2.0 ** -24 * b16.double().abs()
        y, _ = ext.gemm_nt_8p_ragged(x, w, b16, "", res)
        assert_within(y, ref, e + BF16 * ref.abs(), "y")
        assert torch.equal(y, ext.gemm_nt_8p_ragged(x, w, b16, "", res, "pre")[0])
        if grid:
            assert torch.equal(y, ext.linear_fwd(x, w, b16, "", res, False)[0])
    elif form in ("gelu_z", "quick_g", "gelu_tanh_g"):
        act, bias = {"gelu_z": ("gelu", b16), "quick_g": ("quickgelu", b32),
                     "gelu_tanh_g": ("gelu_tanh", b16)}[form]
        pre = (acc + bias.double()).requires_grad_(True)
        yref = Fn._act(pre, act)
        (gref,) = torch.autograd.grad(yref.sum(), pre)
        pre, yref = pre.detach(), yref.detach()
        e = K * EPS * mag + 2.0 ** -24 * bias.double().abs()
        y_n, none = ext.gemm_nt_8p_ragged(x, w, bias, act)
        y_z, z = ext.gemm_nt_8p_ragged(x, w, bias, act, None, "pre")
        y_g, g = ext.gemm_nt_8p_ragged(x, w, bias, act, None, "grad")
        assert none is None and z.dtype == torch.bfloat16 and g.dtype == torch.float16
        assert torch.equal(y_n, y_z) and torch.equal(y_n, y_g)  # mfma.h's promise
        assert_within(y_n, yref, 1.13 * e + 2e-6 + BF16 * yref.abs(), "y")
        assert_within(z, pre, 1.13 * e + 2e-6 + BF16 * pre.abs(), "z")
        assert_within(g, gref, e + 2e-6 + 2.0 ** -11 * gref.abs() + 2.0 ** -24, "g")
        assert torch.equal(g, ext.gemm_nt_8p_ragged(x, w, bias, act, None, "grad")[1])
    elif form == "gradmul":
        gen = torch.Generator(device="cuda").manual_seed(9)
        g = (torch.rand(M, N, device="cuda", generator=gen) * 1.3 - 0.17).half()
        ref = acc * g.double()
        y = ext.gemm_nt_8p_ragged_gradmul(x, w, g)
        assert_within(y, ref, K * EPS * mag * g.double().abs() + BF16 * ref.abs(), "dz")
        assert torch.equal(y, ext.gemm_nt_8p_ragged_gradmul(x, w, g))
    else:
        gen = torch.Generator(device="cuda").manual_seed(10)
        z = torch.randn(M, N, device="cuda", generator=gen).bfloat16()
        zd = z.double().requires_grad_(True)
        (dact,) = torch.autograd.grad(Fn._act(zd, "gelu_tanh").sum(), zd)
        ref = acc * dact
        y = ext.gemm_nt_8p_ragged_gradact(x, w, z, "gelu_tanh")
        assert_within(y, ref, K * EPS * mag * dact.abs() + 2e-6 * acc.abs() + BF16 * ref.abs(),
                      "dz")
        assert torch.equal(y, ext.gemm_nt_8p_ragged_gradact(x, w, z, "gelu_tanh"))


def test_domain_edge(ext):
    for N, K in ((100, 128), (128, 132), (128, 64)):  # N % 8, K % 8, K < 128
        assert not ext.gemm_nt_8p_ragged_supported(64, N, K)
        x, w, t = operand(64, K, 1), operand(N, K, 2), operand(64, N, 3)
        with pytest.raises(RuntimeError):
            ext.gemm_nt_8p_ragged(x, w)
        with pytest.raises(RuntimeError):
            ext.gemm_nt_8p_ragged_gradmul(x, w, t.half())
        with pytest.raises(RuntimeError):
            ext.gemm_nt_8p_ragged_gradact(x, w, t, "gelu")
    with pytest.raises(RuntimeError):  # no dropout form
        ext.gemm_nt_8p_ragged(operand(64, 128, 1), operand(72, 128, 2), p=0.1)


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


def test_block_routes(calls, monkeypatch):
    """so400m EncoderBlock forward + backward at the measured row floor: the
    sites the measured rule routes run the ragged kernel, with no separate
    bias_act_fwd / act_bwd pass, and the result agrees with the block on
    rocBLAS at the thresholds of test_block_mlp_not_multiple_of_256."""
    from jimm_amd.models.common.transformer import EncoderBlock

    torch.manual_seed(3)
    blk = EncoderBlock(1152, 16, 4304, hidden_act="gelu_tanh", layernorm_epsilon=1e-6)
    blk = blk.to("cuda", torch.bfloat16)
    x = torch.randn(FLOOR // 256, 256, 1152, device="cuda").bfloat16()
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
    # the measured rule admits N = 4304: fc1 (saving the derivative) and fc2-dX
    ragged = [c for c in trace if c.startswith("gemm_nt_8p_ragged")]
    assert ragged == ["gemm_nt_8p_ragged", "gemm_nt_8p_ragged_gradmul"], trace
    # no activation pass on its own; bias_act_fwd is proj's and fc2's (rocBLAS)
    assert "act_bwd" not in trace and trace.count("bias_act_fwd") == 2, trace

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


def test_linear_route(calls):
    """ops.linear at the row floor, (N, K) = (1152, 4304): the site measured
    behind rocBLAS at two of three sizes and fails the rule's n-tile fill
    condition, so the forward stays addmm."""
    from jimm_amd.ops import linear

    K = 4304
    x = operand(FLOOR, K, 5)
    w = (operand(1152, K, 6) * 0.03).bfloat16().requires_grad_(True)
    b = operand(1, 1152, 7)[0].requires_grad_(True)
    calls.clear()
    y = linear(x, w, b)
    torch.cuda.synchronize()
    assert calls == ["torch.addmm"], calls
    ref = x.double() @ w.double().t() + b.double()
    mag = x.double().abs() @ w.double().abs().t()
    assert_within(y, ref, K * EPS * mag + 2.0 ** -24 * b.double().abs() + BF16 * ref.abs(), "y")
