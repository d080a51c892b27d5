"""dW kernel (csrc/gemm_tn8p.hip): staging ring, ragged tail, split-M argument,
bias-gradient fold, bf16 reduce output and the split-count chooser.

Inputs: dz = randn (bf16), x = randn/8 (bf16); reference dz^T @ x in fp64.
Metric: max-abs error over max-abs reference.  Bound 1e-4: the operands are
exact in fp32 and the kernel accumulates in fp32, so only summation rounding
remains (measured 1.1e-7 .. 2.5e-7 on these cases before the ring was
introduced), while one stale, skipped or doubled 32-row unit at M <= 8192
moves the metric by 1e-2 or more.
"""

import pytest
import torch

import jimm_amd  # noqa: F401
from jimm_amd.ops import _backend

RING = 5  # ring slots of the kernel (csrc/gemm_tn8p.hip RING)
BOUND = 1e-4
DB_BOUND = 1e-3


@pytest.fixture(scope="module")
def ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _backend.ext()  # fail loudly — never silently skip to eager on a GPU box


def rel_err(out, ref):
    return (out.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)


_CACHE = {}


def operands(M, N, K):
    """(dz, x, fp64 dW reference, fp64 db reference), computed once per shape."""
    key = (M, N, K)
    if key not in _CACHE:
        g = torch.Generator(device="cuda").manual_seed(M * 7919 + N + K)
        dz = torch.randn(M, N, device="cuda", generator=g).bfloat16()
        x = (torch.randn(M, K, device="cuda", generator=g) / 8).bfloat16()
        _CACHE[key] = (dz, x, dz.double().t() @ x.double(), dz.double().sum(0))
    return _CACHE[key]


def check_dw(ext, M, N, K, splitm):
    dz, x, ref, _ = operands(M, N, K)
    dw = ext.gemm_tn_8p(dz, x, splitm)
    err = rel_err(dw, ref)
    print(f"dW M={M} N={N} K={K} splitm={splitm}: rel err {err:.3e}")
    assert dw.dtype == torch.float32
    assert err < BOUND, (M, N, K, splitm, err)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(1, 2 * RING + 2))
def test_ring_lengths(ext, k):
    """Chunks shorter than the ring, exactly the ring, and wrap-around."""
    check_dw(ext, 64 * k, 256, 256, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 31, 65, 96, 97, 127, 64 * RING + 33])
def test_ragged_tail(ext, M):
    check_dw(ext, M, 512, 256, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("M,splitm", [(4160, 1), (4160, 2), (4160, 5), (4160, 65), (7000, 3)])
def test_splits(ext, M, splitm):
    """Short last chunk (4160 = 65 tiles), one tile per split, ragged M."""
    check_dw(ext, M, 768, 512, splitm)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [320, 4160, 7000])
def test_bias_grad_fold(ext, M):
    dz, x, ref, db_ref = operands(M, 768, 512)
    dw, db = ext.gemm_tn_8p_db(dz, x)
    e_dw, e_db = rel_err(dw, ref), rel_err(db, db_ref)
    print(f"dW+db M={M}: dW rel err {e_dw:.3e}, db rel err {e_db:.3e}")
    assert e_dw < BOUND, (M, e_dw)
    assert e_db < DB_BOUND, (M, e_db)


@pytest.mark.gpu
@pytest.mark.parametrize("M,splitm", [(4160, 1), (4160, 5), (7000, 3), (7000, 0)])
def test_bf16_reduce_output(ext, M, splitm):
    """The reduce's bf16 output is the fp32 result rounded once."""
    dz, x, _, _ = operands(M, 768, 512)
    f32 = ext.gemm_tn_8p(dz, x, splitm)
    b16 = ext.gemm_tn_8p(dz, x, splitm, True)
    assert b16.dtype == torch.bfloat16
    assert torch.equal(b16, f32.to(torch.bfloat16))
    f32d, dbf = ext.gemm_tn_8p_db(dz, x, splitm)
    b16d, dbb = ext.gemm_tn_8p_db(dz, x, splitm, True)
    assert b16d.dtype == torch.bfloat16 and torch.equal(b16d, f32d.to(torch.bfloat16))
    assert dbb.dtype == torch.float32
    assert rel_err(dbb, dbf.double()) < 1e-5  # atomics: order may differ, value may not


def test_split_chooser():
    """Host-side split chooser (no GPU needed)."""
    choose = _backend.ext().gemm_tn8p_choose_splitm
    assert choose(201728, 27, 256) == 18
    for M in (1, 63, 64, 65, 640, 1000, 73856, 201728):
        for tiles in (1, 9, 16, 27, 36, 48, 64, 144):
            for cus in (64, 256, 304):
                s = choose(M, tiles, cus)
                assert 1 <= s <= max(24, cus // tiles)
                assert s <= (M + 63) // 64, (M, tiles, cus, s)
