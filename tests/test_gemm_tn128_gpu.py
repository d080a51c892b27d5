"""128-tile TN dW kernel (csrc/gemm_tn128.hip): dW = dz^T @ x and the folded
db = colsum(dz) for weight shapes off the 256 grid, against fp64 on the same
bf16 inputs, and the route of ``ops.linear`` to it.

Bounds: bf16 products are exact in fp32, only the sums round. With
mag = |dz|^T @ |x| and S splits, fp32 dW lies within (M + S) * 2^-23 * mag of
the reference (2^-23, not 2^-24: the MFMA need not round to nearest); a bf16
result adds its own rounding, 2^-8 * |ref|; db lies within
M * 2^-23 * colsum(|dz|). A dropped row or a misplaced column is off by about
mag / M. Inputs carry a per-column offset so that swapped columns differ.
"""

import pytest
import torch

import jimm_amd  # noqa: F401
from jimm_amd.ops import _backend

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
BF16 = 2.0 ** -8


@pytest.fixture(scope="module")
def ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _backend.ext()  # fail loudly — never silently skip to eager on a GPU box


def operand(M, W, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.randn(M, W, device="cuda", generator=g)
    return (t + 0.01 * torch.arange(W, device="cuda")).bfloat16()


_CASES = {}


def case(M, N, K):
    """(dz, x, ref, mag, db_ref, db_mag), made once per shape."""
    if (M, N, K) not in _CASES:
        dz, x = operand(M, N, 11 + M + N), operand(M, K, 23 + M + K)
        dzd, xd = dz.double(), x.double()
        _CASES[M, N, K] = (dz, x, dzd.t() @ xd, dzd.abs().t() @ xd.abs(), dzd.sum(0),
                           dzd.abs().sum(0))
    return _CASES[M, N, K]


def assert_dw(dw, ref, mag, M, S, what):
    bound = (M + S) * EPS * mag
    if dw.dtype == torch.bfloat16:
        bound = bound + BF16 * ref.abs()
    excess = ((dw.double() - ref).abs() - bound).max().item()
    print(f"{what}: max |err| {(dw.double() - ref).abs().max().item():.3e}, "
          f"max (|err| - bound) {excess:.3e}")
    assert dw.shape == ref.shape and excess <= 0, (what, excess)


def assert_db(db, db_ref, db_mag, M, what, rounded=False):
    bound = M * EPS * db_mag + (BF16 * db_ref.abs() if rounded else 0)
    excess = ((db.double() - db_ref).abs() - bound).max().item()
    print(f"{what}: max (|err| - bound) {excess:.3e}")
    assert db.shape == db_ref.shape and excess <= 0, (what, excess)


@pytest.mark.parametrize("out_bf16", [False, True])
@pytest.mark.parametrize("M,N,K,splitm", [
    (1, 8, 8, 1),            # tail only; one valid chunk per operand, the rest clamped
    (96, 128, 128, 1),       # one exact tile; ring plus a 32-row tail
    (453, 128, 128, 1),      # 14 units: the five-slot ring wraps; 5-row tail
    (330, 392, 264, 1),      # 4 x 3 tiles, the last n- and k-tile hold 8 columns
    (330, 392, 264, 3),      # the same through workspace + reduce, unequal chunks
    (256, 384, 1000, 2),     # ViT-S width against a class-head width
    (200, 4304, 136, 1),     # so400m's mlp width, 34 n-tiles
])
def test_dw_db(ext, M, N, K, splitm, out_bf16):
    dz, x, ref, mag, db_ref, db_mag = case(M, N, K)
    assert ext.gemm_tn_128_supported(M, N, K)
    dw = ext.gemm_tn_128(dz, x, splitm, out_bf16)
    assert dw.dtype == (torch.bfloat16 if out_bf16 else torch.float32)
    assert_dw(dw, ref, mag, M, splitm, "dW")
    assert torch.equal(dw, ext.gemm_tn_128(dz, x, splitm, out_bf16))
    dw2, db = ext.gemm_tn_128_db(dz, x, splitm, out_bf16)
    assert torch.equal(dw2, dw)
    assert db.dtype == torch.float32
    assert_db(db, db_ref, db_mag, M, "db")


def test_domain_edge(ext):
    assert not ext.gemm_tn_128_supported(64, 100, 128)
    assert not ext.gemm_tn_128_supported(64, 128, 4)
    with pytest.raises(RuntimeError):
        ext.gemm_tn_128(operand(64, 100, 1), operand(64, 128, 2), 1, False)


def test_linear_route(ext, monkeypatch):
    """ops.linear, (256, 384) x (1000, 384)^T + bias: dW and db come from the
    128-tile kernel; with 80 rows they do not. x needs no gradient, so the
    backward has no dX GEMM (its K = 1000 would be a torch.matmul of its own)
    and any torch.matmul would be the dW site's. The chooser's split count is
    at most the 4 m-steps; bf16 parameters round both gradients once more."""
    from jimm_amd.ops import linear

    for name in ("JIMM_AMD_GEMM", "JIMM_AMD_DETERMINISTIC"):
        monkeypatch.delenv(name, raising=False)
    calls = []

    def spy(owner, name, label):
        def f(*a, _f=getattr(owner, name), **kw):
            calls.append(label)
            return _f(*a, **kw)
        monkeypatch.setattr(owner, name, f)

    spy(ext, "gemm_tn_128_db", "gemm_tn_128_db")
    spy(torch, "matmul", "torch.matmul")
    for M in (256, 80):
        x = operand(M, 384, 5)
        w = (operand(1000, 384, 6) * 0.03).bfloat16().requires_grad_(True)
        b = operand(1, 1000, 7)[0].requires_grad_(True)
        dy = operand(M, 1000, 8)
        calls.clear()
        linear(x, w, b).backward(dy)
        torch.cuda.synchronize()
        print(f"M={M}: {calls!r}")
        if M == 80:
            assert "gemm_tn_128_db" not in calls, calls
            continue
        assert calls == ["gemm_tn_128_db"], calls
        dzd, xd = dy.double(), x.double()
        assert_dw(w.grad, dzd.t() @ xd, dzd.abs().t() @ xd.abs(), M, 4, "weight.grad")
        assert_db(b.grad, dzd.sum(0), dzd.abs().sum(0), M, "bias.grad", rounded=True)
