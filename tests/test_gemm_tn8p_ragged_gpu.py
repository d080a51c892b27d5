"""Ragged form of the 256-tile TN dW kernel (csrc/gemm_tn8p.hip, RAGGED):
dW = dz^T @ x and the folded db = colsum(dz) for any N % 8 == 0, K % 8 == 0,
against fp64 on the same bf16 inputs, and the JIMM_AMD_DW_RAGGED=1 route of
``ops.linear`` to it.

Bounds (tests/test_gemm_tn128_gpu.py, the same accumulation scheme): bf16
products are exact in fp32, only the sums round. With mag = |dz|^T @ |x| and S
splits, fp32 dW lies within (M + S) * 2^-23 * mag of the reference; a bf16
result adds 2^-8 * |ref|; db lies within M * 2^-23 * colsum(|dz|). Inputs carry
a per-column offset (column / 64, as tests/test_gemm8p_colperm_gpu.py), so a
misplaced column or a clamped staging chunk that reaches a stored element is
off by about mag / M.

The fp32 results are written into the middle of a larger buffer (``out=``):
the element range of dW starts as NaN, so an element that is not stored fails
the bound, and the bands on both sides, each as long as the stores of a whole
tile row beyond N would reach, must keep their fill."""

import pytest
import torch

import jimm_amd  # noqa: F401
from jimm_amd.ops import _backend

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
BF16 = 2.0 ** -8
FILL = -7.0


@pytest.fixture(scope="module")
def ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _backend.ext()  # fail loudly — never silently skip to eager on a GPU box


def operand(M, W, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.randn(M, W, device="cuda", generator=g)
    return (t + torch.arange(W, device="cuda") / 64.0).bfloat16()


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
    assert dw.shape == ref.shape, (what, dw.shape)
    excess = ((dw.double() - ref).abs() - bound).max().item()
    print(f"{what}: max |err| {(dw.double() - ref).abs().max().item():.3e}, "
          f"max (|err| - bound) {excess:.3e}")
    assert excess <= 0, (what, excess)


def assert_db(db, db_ref, db_mag, M, what, rounded=False):
    bound = M * EPS * db_mag + (BF16 * db_ref.abs() if rounded else 0)
    assert db.shape == db_ref.shape, (what, db.shape)
    excess = ((db.double() - db_ref).abs() - bound).max().item()
    print(f"{what}: max (|err| - bound) {excess:.3e}")
    assert excess <= 0, (what, excess)


def banded(N, K):
    """A NaN (N, K) fp32 view with FILL bands in front and behind."""
    G = 256 * (K + 256)
    buf = torch.full((2 * G + N * K,), FILL, device="cuda")
    out = buf[G:G + N * K].view(N, K)
    out.fill_(float("nan"))
    return buf, out, G


@pytest.mark.parametrize("splitm", [1, 3])
@pytest.mark.parametrize("M", [1, 63, 65, 352])
@pytest.mark.parametrize("K", [8, 136, 264])
@pytest.mark.parametrize("N", [8, 248, 264, 520])
def test_edges(ext, N, K, M, splitm):
    dz, x, ref, mag, db_ref, db_mag = case(M, N, K)
    assert ext.gemm_tn8p_ragged_supported(M, N, K)
    for with_db in (False, True):
        for out_bf16 in (False, True):
            what = f"db={with_db} bf16={out_bf16}"
            buf = None
            kw = {}
            if not out_bf16:
                buf, kw["out"], G = banded(N, K)
            if with_db:
                dw, db = ext.gemm_tn_8p_ragged_db(dz, x, splitm, out_bf16, **kw)
                assert db.dtype == torch.float32
                assert_db(db, db_ref, db_mag, M, "db " + what)
            else:
                dw = ext.gemm_tn_8p_ragged(dz, x, splitm, out_bf16, **kw)
            assert dw.dtype == (torch.bfloat16 if out_bf16 else torch.float32)
            assert_dw(dw, ref, mag, M, splitm, "dW " + what)
            if buf is not None:
                assert dw.data_ptr() == kw["out"].data_ptr()
                assert bool((buf[:G] == FILL).all()) and bool((buf[-G:] == FILL).all()), what


def test_deterministic(ext):
    dz, x, *_ = case(352, 520, 264)
    a = ext.gemm_tn_8p_ragged(dz, x, 3, False)
    b = ext.gemm_tn_8p_ragged(dz, x, 3, False)
    assert torch.equal(a, b)


def test_domain_edge(ext):
    assert not ext.gemm_tn8p_ragged_supported(64, 100, 128)
    assert not ext.gemm_tn8p_ragged_supported(64, 128, 4)
    with pytest.raises(RuntimeError):
        ext.gemm_tn_8p_ragged(operand(64, 100, 1), operand(64, 128, 2), 1, False)


def test_linear_route(ext, monkeypatch):
    """ops.linear at M = 512 with a 264 x 520 weight under JIMM_AMD_DW_RAGGED=1:
    dW and db come from the ragged kernel (by default the 128-tile kernel takes
    this shape). The chooser's split count is at most the 8 m-steps; bf16
    parameters round both gradients once more."""
    from jimm_amd.ops import linear

    for name in ("JIMM_AMD_GEMM", "JIMM_AMD_DETERMINISTIC"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("JIMM_AMD_DW_RAGGED", "1")
    calls = []

    def spy(*a, _f=ext.gemm_tn_8p_ragged_db, **kw):
        calls.append("gemm_tn_8p_ragged_db")
        return _f(*a, **kw)

    monkeypatch.setattr(ext, "gemm_tn_8p_ragged_db", spy)
    M, N, K = 512, 264, 520
    x = operand(M, K, 5)
    w = (operand(N, K, 6) * 0.03).bfloat16().requires_grad_(True)
    b = operand(1, N, 7)[0].requires_grad_(True)
    linear(x, w, b).sum().backward()
    torch.cuda.synchronize()
    assert calls == ["gemm_tn_8p_ragged_db"], calls
    dzd, xd = torch.ones(M, N, device="cuda", dtype=torch.float64), x.double()
    assert_dw(w.grad, dzd.t() @ xd, dzd.t() @ xd.abs(), M, 8, "weight.grad")
    assert_db(b.grad, dzd.sum(0), dzd.sum(0), M, "bias.grad", rounded=True)
