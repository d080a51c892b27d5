"""Activated-linear epilogues that save act'(pre) in the forward and multiply
in the backward: linear_fwd_actgrad (y, fp16 g) and gemm_nt_8p_gradmul, alone,
as a pair against the save-z / gradact pair, and inside the fused block.

Shapes: K = 128 is the smallest K the 8-phase kernel takes; N = 512 gives two
column tiles (a wrongly hoisted bias shows); M = 300 gives a second, ragged
row tile, M = 100 a single ragged one. N = 384 / M = 256 reaches the 128-tile
glds kernel and N = 200 / M = 100 the guarded 128-tile kernel.
All require an MI355X (gfx950)."""

import functools
import math

import pytest
import torch

import jimm_amd  # noqa: F401
import jimm_amd.ops.functional as Fn
from jimm_amd.ops import _backend

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    EXT = _backend.ext()  # fail loudly — never silently skip to eager on a GPU box
else:
    pytest.skip("no GPU", allow_module_level=True)

ACTS = ["gelu", "gelu_tanh", "quickgelu"]
K = 128
# max |g - act'(pre64)|: 2^-11 is half an fp16 ulp in [1, 2), where g peaks
# (1.13); 2e-5 covers the fp32 accumulation of pre and the fast-erf error.
G_TOL = 2.0 ** -11 + 2e-5


def dev():
    return torch.device("cuda:0")


def rel_err(out, ref):
    ref = ref.float()
    return (out.float() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)


@functools.lru_cache(maxsize=None)
def case(M, N, act, has_bias):
    """Inputs and fp64 references of one shape, built once and shared (read
    only): x, w, bias, dy, wt, pre64, act'(pre64), df64 = dy @ wt^T."""
    g = torch.Generator(device="cuda").manual_seed(1000 * M + N)
    x = torch.randn(M, K, device=dev(), generator=g).bfloat16()
    w = (torch.randn(N, K, device=dev(), generator=g) / math.sqrt(K)).bfloat16()
    bias = torch.randn(N, device=dev(), generator=g).bfloat16() if has_bias else None
    dy = torch.randn(M, K, device=dev(), generator=g).bfloat16()
    wt = (torch.randn(N, K, device=dev(), generator=g) / math.sqrt(K)).bfloat16()
    pre = x.double() @ w.double().t()
    if has_bias:
        pre = pre + bias.double()
    pre = pre.requires_grad_(True)
    (dact,) = torch.autograd.grad(Fn._act(pre, act).sum(), pre)
    df = dy.double() @ wt.double().t()
    return x, w, bias, dy, wt, pre.detach(), dact, df


def check_forward(M, N, act, has_bias):
    x, w, bias, _, _, _, dact, _ = case(M, N, act, has_bias)
    y_z, z = EXT.linear_fwd(x, w, bias, act, None, True)
    y_n, none = EXT.linear_fwd(x, w, bias, act, None, False)
    y_g, g = EXT.linear_fwd_actgrad(x, w, bias, act, None)
    assert none is None and z.dtype == torch.bfloat16
    assert g.dtype == torch.float16 and g.shape == (M, N)
    assert torch.equal(y_g, y_z) and torch.equal(y_n, y_z)
    err = (g.double() - dact).abs().max().item()
    print(f"fwd M={M} N={N} {act} bias={has_bias}: max|g-ref| = {err:.3e} (bound {G_TOL:.3e})")
    assert err <= G_TOL, err


def test_reference_fits_fp16():
    """The bound must be reachable: act'(pre64) rounded to fp16 meets it by
    itself (half an ulp, plus 2^-24 where the conversion rounds through
    fp32), which leaves the 2e-5 to the kernel's fp32 arithmetic."""
    for act in ACTS:
        dact = case(300, 512, act, True)[6]
        err = (dact.to(torch.float16).double() - dact).abs().max().item()
        assert err <= 2.0 ** -11 + 2.0 ** -24, (act, err)


@pytest.mark.parametrize("has_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("M", [256, 100, 300])
def test_forward_saves_derivative(M, act, has_bias):
    """8-phase kernel: y bitwise as in the other save modes, g within half an
    fp16 ulp (+2e-5) of the fp64 derivative."""
    assert EXT.gemm8p_supported(M, 512, K)
    check_forward(M, 512, act, has_bias)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("M,N", [(256, 384), (100, 200)], ids=["fast128", "guarded128"])
def test_forward_saves_derivative_128tile(M, N, act):
    """The same on the two 128-tile kernels (shapes the 8-phase kernel does
    not take)."""
    assert not EXT.gemm8p_supported(M, N, K)
    check_forward(M, N, act, True)


def test_forward_fp32_bias_and_residual():
    """An fp32 bias gives the bits a bf16 bias of the same values gives, and
    the derivative is saved before the residual is added."""
    x, w, bias, _, _, _, _, _ = case(300, 512, "gelu", True)
    res = torch.randn(300, 512, device=dev()).bfloat16()
    y_b, g_b = EXT.linear_fwd_actgrad(x, w, bias, "gelu", None)
    y_f, g_f = EXT.linear_fwd_actgrad(x, w, bias.float(), "gelu", None)
    assert torch.equal(y_b, y_f) and torch.equal(g_b, g_f)
    y_r, g_r = EXT.linear_fwd_actgrad(x, w, bias, "gelu", res)
    y_rz, _ = EXT.linear_fwd(x, w, bias, "gelu", res, True)
    assert torch.equal(y_r, y_rz) and torch.equal(g_r, g_b)
    with pytest.raises(RuntimeError):
        EXT.linear_fwd_actgrad(x, w, bias, "", None)


@pytest.mark.parametrize("gsrc", ["random", "forward"])
@pytest.mark.parametrize("M", [256, 100, 300])
def test_gradmul(M, gsrc):
    """dz = (dy @ wt^T) * g against fp64, at the line test_gemm_gradact uses."""
    x, w, bias, dy, wt, _, _, df = case(M, 512, "gelu", True)
    if gsrc == "random":
        gen = torch.Generator(device="cuda").manual_seed(M)
        g = (torch.rand(M, 512, device=dev(), generator=gen) * 1.4 - 0.2).half()
    else:
        _, g = EXT.linear_fwd_actgrad(x, w, bias, "gelu", None)
    dz = EXT.gemm_nt_8p_gradmul(dy, wt, g)
    assert dz.dtype == torch.bfloat16 and dz.shape == (M, 512)
    ref = df * g.double()
    err = rel_err(dz, ref)
    assert err < 2e-2, err
    with pytest.raises(RuntimeError):
        EXT.gemm_nt_8p_gradmul(dy, wt, g.bfloat16())


def l2_err(out, ref):
    return ((out.double() - ref).norm() / ref.norm()).item()


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("M", [256, 300])
def test_pair_against_pair(M, act):
    """save-g + gradmul is no less accurate than save-z + gradact: both
    against fp64 (dy @ wt^T) * act'(pre64). The error is the relative L2
    norm over the whole output: it averages the two schemes' rounding over
    1.3e5+ elements, where a max-norm compares one worst element of each.
    A CPU simulation of the two schemes gave new/present = 0.94-1.00; the
    5 % is for sampling."""
    x, w, bias, dy, wt, _, dact, df = case(M, 512, act, True)
    ref = df * dact
    _, g = EXT.linear_fwd_actgrad(x, w, bias, act, None)
    err_new = l2_err(EXT.gemm_nt_8p_gradmul(dy, wt, g), ref)
    _, z = EXT.linear_fwd(x, w, bias, act, None, True)
    err_old = l2_err(EXT.gemm_nt_8p_gradact(dy, wt, z, act), ref)
    print(f"pair M={M} {act}: new {err_new:.4e} present {err_old:.4e} ratio {err_new / err_old:.3f}")
    assert err_new <= 1.05 * err_old, (err_new, err_old)


@pytest.mark.parametrize("act", ["gelu", "quickgelu"])
def test_block_save_g_vs_save_z(act, monkeypatch):
    """The fused block at H = 256 (the HIP GEMM path; the H = 128 block test
    does not reach it): default (save g, gradmul) against JIMM_AMD_ACT_SAVE=z
    (save z, gradact), at the thresholds of test_fused_block_vs_composite."""
    from jimm_amd.models.common.transformer import EncoderBlock
    from jimm_amd.ops import block as block_mod

    torch.manual_seed(3)
    blk = EncoderBlock(256, 4, 512, hidden_act=act, layernorm_epsilon=1e-6).to(dev(), torch.bfloat16)
    x = torch.randn(2, 40, 256, device=dev()).bfloat16()
    dy = torch.randn_like(x)
    assert block_mod.fused_block_enabled(x, 0.0) and block_mod._hip_gemms(256, 512)

    calls = []
    for name in ("gemm_nt_8p_gradmul", "gemm_nt_8p_gradact"):
        def spy(*a, _f=getattr(EXT, name), _n=name):
            calls.append(_n)
            return _f(*a)
        monkeypatch.setattr(EXT, name, spy)

    def run():
        for p in blk.parameters():
            p.grad = None
        xi = x.detach().clone().requires_grad_(True)
        y = blk(xi)
        y.backward(dy)
        return y.detach(), xi.grad.clone(), {n: p.grad.clone() for n, p in blk.named_parameters()}

    monkeypatch.delenv("JIMM_AMD_ACT_SAVE", raising=False)
    y_g, dx_g, g_g = run()
    monkeypatch.setenv("JIMM_AMD_ACT_SAVE", "z")
    y_z, dx_z, g_z = run()
    assert calls == ["gemm_nt_8p_gradmul", "gemm_nt_8p_gradact"], calls
    assert torch.equal(y_g, y_z)
    assert rel_err(dx_g, dx_z) < 2e-2, rel_err(dx_g, dx_z)
    for n in g_g:
        assert rel_err(g_g[n], g_z[n]) < 3e-2, (n, rel_err(g_g[n], g_z[n]))
