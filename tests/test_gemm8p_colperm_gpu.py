"""Column-permuted 8-phase GEMM (gemm8p.hip): a lane of a non-dropout kernel
holds 4 consecutive columns and its epilogue makes one 8-byte access per
stream. Every epilogue form against torch in fp64, on inputs with a per-column
offset, so that a result landing in (or a bias / residual / multiplier taken
from) another column cannot pass.

Shapes (M, N, K): (256, 256, 128) is one tile at the smallest K; (300, 512,
192) has a ragged second row tile, two column tiles and an odd K-tile count
(the B slot rotation wraps); (70, 768, 256) has fewer rows than a row half.

The two test_columns_follow_* tests are exact (bitwise) for every stream; the
fp64 comparisons add the per-column offsets on top. Inputs: W row n =
(randn + n/64) / (4 sqrt(K)), bias = randn + n/64, residual = randn + n/64, multiplier g = rand * 1.4 - 0.2 + n/64. The 1/4 on W keeps
the pre-activation of the highest columns within a few units, where the
activations still bend. Bounds are those of tests/test_kernels_gpu.py
(2e-2 of the largest reference value for y, z and dz; 0.04 and 2^-8 for the
e4m3 copy and its amax) and tests/test_gemm_actgrad_gpu.py (G_TOL for the
saved derivative, 2e-2 for gradmul). All require an MI355X (gfx950)."""

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

SHAPES = [(256, 256, 128), (300, 512, 192), (70, 768, 256)]
ACTS = ["gelu", "gelu_tanh", "quickgelu"]
# tests/test_gemm_actgrad_gpu.py: half an fp16 ulp in [1, 2) + 2e-5 for the
# fp32 arithmetic in front of the rounding
G_TOL = 2.0 ** -11 + 2e-5


def dev():
    return torch.device("cuda:0")


def rel_err(out, ref):
    return (out.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)


@functools.lru_cache(maxsize=None)
def case(M, N, K):
    """Inputs of one shape, built once and shared (read only)."""
    gen = torch.Generator(device="cuda").manual_seed(7 * M + N + K)
    col = torch.arange(N, device=dev(), dtype=torch.float32) / 64.0

    def rn(*shape):
        return torch.randn(*shape, device=dev(), generator=gen)

    x = rn(M, K).bfloat16()
    w = ((rn(N, K) + col[:, None]) / (4.0 * math.sqrt(K))).bfloat16()
    bias = (rn(N) + col).bfloat16()
    res = (rn(M, N) + col).bfloat16()
    z = (rn(M, N) + col / 4.0).bfloat16()  # saved pre-activation of the gradact forms
    g = (torch.rand(M, N, device=dev(), generator=gen) * 1.4 - 0.2 + col).half()
    return dict(x=x, w=w, bias=bias, res=res, z=z, g=g, xw=x.double() @ w.double().t())


def act64(pre, act):
    """act(pre) and act'(pre) in fp64."""
    pre = pre.detach().requires_grad_(True)
    y = Fn._act(pre, act or None)
    (d,) = torch.autograd.grad(y.sum(), pre)
    return y.detach(), d


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_plain_and_bias(M, N, K):
    """No epilogue stream but Y; an fp32 bias (one 16-byte load) and a bf16
    bias (one 8-byte load) of the same values give the same bits."""
    c = case(M, N, K)
    y, none = EXT.linear_fwd(c["x"], c["w"], None, "", None, False)
    assert none is None and y.shape == (M, N)
    err = rel_err(y, c["xw"])
    print(f"plain {M}x{N}x{K}: {err:.3e}")
    assert err < 2e-2, err
    ref = c["xw"] + c["bias"].double()
    y_b, _ = EXT.linear_fwd(c["x"], c["w"], c["bias"], "", None, False)
    y_f, _ = EXT.linear_fwd(c["x"], c["w"], c["bias"].float(), "", None, False)
    err = rel_err(y_b, ref)
    print(f"bias  {M}x{N}x{K}: {err:.3e}")
    assert err < 2e-2, err
    assert torch.equal(y_b, y_f)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_columns_follow_weight_rows(M, N, K):
    """Output column n is x times W row n and nothing else: with the rows of W
    shuffled the columns of y are the same bits, shuffled the same way. A
    kernel that pairs any fragment with another column fails this exactly,
    whatever the data."""
    c = case(M, N, K)
    perm = torch.randperm(N, device=dev(), generator=torch.Generator(device="cuda").manual_seed(N))
    y, _ = EXT.linear_fwd(c["x"], c["w"], None, "", None, False)
    y_p, _ = EXT.linear_fwd(c["x"], c["w"][perm].contiguous(), None, "", None, False)
    assert torch.equal(y_p, y[:, perm])


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_columns_follow_every_stream(M, N, K):
    """The same, exactly, for the streams the epilogue reads and writes per
    column: with W rows, bias, residual, saved z and multiplier g all shuffled
    by one permutation, every output is the unshuffled output's bits with its
    columns shuffled. A bias, residual, z or g value taken from a neighbouring
    column (one apart or 16 apart alike) fails this whatever its size."""
    c = case(M, N, K)
    perm = torch.randperm(N, device=dev(), generator=torch.Generator(device="cuda").manual_seed(N + 1))
    x, w, wp = c["x"], c["w"], c["w"][perm].contiguous()
    b, bp = c["bias"], c["bias"][perm].contiguous()
    sh = lambda t: t[:, perm].contiguous()  # noqa: E731
    runs = {
        "bias+res": lambda w, b, r, z, g: EXT.linear_fwd(x, w, b, "", r, False),
        "fp32 bias": lambda w, b, r, z, g: EXT.linear_fwd(x, w, b.float(), "", None, False),
        "gelu save z": lambda w, b, r, z, g: EXT.linear_fwd(x, w, b, "gelu", r, True),
        "gelu save g": lambda w, b, r, z, g: EXT.linear_fwd_actgrad(x, w, b, "gelu", None),
        "gradmul": lambda w, b, r, z, g: [EXT.gemm_nt_8p_gradmul(x, w, g)],
        "gradact": lambda w, b, r, z, g: [EXT.gemm_nt_8p_gradact(x, w, z, "gelu")],
    }
    for name, f in runs.items():
        outs = f(w, b, c["res"], c["z"], c["g"])
        outs_p = f(wp, bp, sh(c["res"]), sh(c["z"]), sh(c["g"]))
        for o, o_p in zip(outs, outs_p):
            assert (o is None) == (o_p is None), name
            assert o is None or torch.equal(o_p, o[:, perm]), name


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_bias_residual(M, N, K):
    c = case(M, N, K)
    y, _ = EXT.linear_fwd(c["x"], c["w"], c["bias"], "", c["res"], False)
    ref = c["xw"] + c["bias"].double() + c["res"].double()
    err = rel_err(y, ref)
    print(f"bias+res {M}x{N}x{K}: {err:.3e}")
    assert err < 2e-2, err


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_activation_saves(M, N, K, act):
    """Activated forward with the pre-activation saved (bf16) and with the
    derivative saved (fp16); y is the same bits in both."""
    c = case(M, N, K)
    pre = c["xw"] + c["bias"].double()
    ref, dref = act64(pre, act)
    y_z, z = EXT.linear_fwd(c["x"], c["w"], c["bias"], act, None, True)
    y_g, g = EXT.linear_fwd_actgrad(c["x"], c["w"], c["bias"], act, None)
    assert z.dtype == torch.bfloat16 and g.dtype == torch.float16
    e_y, e_z = rel_err(y_z, ref), rel_err(z, pre)
    e_g = (g.double() - dref).abs().max().item()
    print(f"{act} {M}x{N}x{K}: y {e_y:.3e} z {e_z:.3e} g {e_g:.3e} (bound {G_TOL:.3e})")
    assert e_y < 2e-2, e_y
    assert e_z < 2e-2, e_z
    assert torch.equal(y_g, y_z)
    assert e_g <= G_TOL, e_g


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gradmul(M, N, K):
    c = case(M, N, K)
    dz = EXT.gemm_nt_8p_gradmul(c["x"], c["w"], c["g"])
    assert dz.dtype == torch.bfloat16 and dz.shape == (M, N)
    err = rel_err(dz, c["xw"] * c["g"].double())
    print(f"gradmul {M}x{N}x{K}: {err:.3e}")
    assert err < 2e-2, err


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gradact(M, N, K, act):
    """(dy @ wt^T) * act'(z), plain and with the fused e4m3 copy (the arguments
    of test_kernels_gpu.py::test_gemm_gradact)."""
    c = case(M, N, K)
    _, dact = act64(c["z"].double(), act)
    ref = c["xw"] * dact
    y = EXT.gemm_nt_8p_gradact(c["x"], c["w"], c["z"], act)
    err = rel_err(y, ref)
    print(f"gradact {act} {M}x{N}x{K}: {err:.3e}")
    assert err < 2e-2, err

    scale = (ref.abs().max() / 448.0).float().reshape(1)
    amax = torch.zeros(1, device=dev(), dtype=torch.float32)
    y2, y8 = EXT.gemm_nt_8p_gradact_fp8(c["x"], c["w"], c["z"], act, scale, amax)
    assert torch.equal(y2, y)
    deq = y8.view(torch.float8_e4m3fn).float() * scale
    # half an e4m3 ulp at the top binade is 16/448
    e8 = rel_err(deq, y.double())
    assert e8 < 0.04, e8
    # the kernel takes the max before the bf16 rounding (which moves a value by <= 2^-9)
    ymax = y.float().abs().max().item()
    assert abs(amax.item() - ymax) <= 2.0 ** -8 * ymax, (amax.item(), ymax)


def test_misaligned_residual_raises():
    """The 8-byte accesses need 8-byte aligned bases: a contiguous residual
    whose storage starts 2 bytes off is refused on the host."""
    M, N, K = SHAPES[0]
    c = case(M, N, K)
    store = torch.zeros(M * N + 4, device=dev(), dtype=torch.bfloat16)
    res = store[1:1 + M * N].view(M, N)
    assert res.is_contiguous() and res.data_ptr() % 8 == 2
    with pytest.raises(RuntimeError, match="aligned"):
        EXT.linear_fwd(c["x"], c["w"], c["bias"], "", res, False)
    # the same values from an aligned base pass
    y, _ = EXT.linear_fwd(c["x"], c["w"], c["bias"], "", res.clone(), False)
    assert torch.equal(y, EXT.linear_fwd(c["x"], c["w"], c["bias"], "", None, False)[0])
