"""dW kernel (csrc/gemm_tn8p.hip): the walk over ring units and the tail, and
the bias fold dealt out over waves and k-tiles (written with the read-ahead
experiment of profiles/dw_readahead_NOTES.md, whose edges the first test
names; it holds for any order of the reads).

Operands are integer-valued: dz and x are drawn from {-2, ..., 2} as bf16 and
M <= 8192, so every product is an integer of magnitude <= 4 and every fp32 sum
stays below 2^24: it is exact in any order.  dW must therefore EQUAL
dz^T @ x and db must EQUAL colsum(dz), both computed in fp64, with no
tolerance.  A skipped, doubled or stale 32-row unit cannot hide, in dW or in
the fold.
"""

import pytest
import torch

import jimm_amd  # noqa: F401
from jimm_amd.ops import _backend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _backend.ext()  # fail loudly — never silently skip to eager on a GPU box


_DZ, _X = {}, {}


def ints(M, W, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(-2, 3, (M, W), device="cuda", generator=g).bfloat16()


def dz_of(M, N):
    """(dz, fp64 db reference): one fixed dz per (M, N), whatever Kw."""
    if (M, N) not in _DZ:
        dz = ints(M, N, 1000003 * M + N)
        _DZ[M, N] = (dz, dz.double().sum(0))
    return _DZ[M, N]


def x_of(M, K):
    if (M, K) not in _X:
        _X[M, K] = ints(M, K, 7 + 999983 * M + K)
    return _X[M, K]


def dw_ref(M, N, K):
    return dz_of(M, N)[0].double().t() @ x_of(M, K).double()


def assert_exact(out, ref, what):
    assert out.dtype == torch.float32, (what, out.dtype)
    assert torch.equal(out.double(), ref), (what, (out.double() - ref).abs().max().item())


@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("M", [64 * k for k in range(1, 12)] + [1, 31, 33, 65, 97, 127, 353])
def test_ring_and_readahead_edges(ext, M, N):
    """Chunks shorter than the ring, the ring exactly, wrap-around; a tail
    alone, a tail after the ring and a tail after a wrapped ring."""
    dw = ext.gemm_tn_8p(dz_of(M, N)[0], x_of(M, 256), 1)
    assert_exact(dw, dw_ref(M, N, 256), (M, N))


@pytest.mark.parametrize("M,splitm", [(4160, 1), (4160, 2), (4160, 5), (4160, 65), (7000, 3), (7000, 0)])
def test_splits(ext, M, splitm):
    """Short last chunk (4160 = 65 tiles), one tile per split, ragged M, the
    chooser's own split: dW and db."""
    dz, db_ref = dz_of(M, 768)
    dw, db = ext.gemm_tn_8p_db(dz, x_of(M, 512), splitm)
    assert_exact(dw, dw_ref(M, 768, 512), ("dW", M, splitm))
    assert_exact(db, db_ref, ("db", M, splitm))
    assert_exact(ext.gemm_tn_8p(dz, x_of(M, 512), splitm), dw_ref(M, 768, 512), ("plain", M, splitm))


@pytest.mark.parametrize("splitm", [1, 3])
@pytest.mark.parametrize("M", [32, 64, 96, 320, 353, 4160])
@pytest.mark.parametrize("N", [256, 512])
def test_fold_coverage(ext, N, M, splitm):
    """nt_k = 1, 2, 3, 5 k-tiles share the fold: fewer units than k-tiles, a
    unit count that the number of folding k-tiles does not divide, a tail.
    db is exact for every Kw, hence the same for every Kw."""
    dz, db_ref = dz_of(M, N)
    dbs = []
    for K in (256, 512, 768, 1280):
        dw, db = ext.gemm_tn_8p_db(dz, x_of(M, K), splitm)
        assert_exact(db, db_ref, ("db", N, K, M, splitm))
        assert_exact(dw, dw_ref(M, N, K), ("dW", N, K, M, splitm))
        dbs.append(db)
    for db in dbs[1:]:
        assert torch.equal(db, dbs[0])


@pytest.mark.parametrize("splitm", [1, 3])
def test_bf16_output(ext, splitm):
    """bf16 dW is the fp32 result rounded once; db stays fp32 and exact."""
    M, N, K = 353, 512, 512
    dz, db_ref = dz_of(M, N)
    f32, _ = ext.gemm_tn_8p_db(dz, x_of(M, K), splitm)
    b16, db = ext.gemm_tn_8p_db(dz, x_of(M, K), splitm, True)
    assert_exact(f32, dw_ref(M, N, K), ("dW", splitm))
    assert b16.dtype == torch.bfloat16
    assert torch.equal(b16, f32.to(torch.bfloat16))
    assert_exact(db, db_ref, ("db", splitm))


def test_patch_embed_without_image_grad(ext):
    """An image that needs no gradient gets none, and the weight gradient is
    what the route with an image gradient computes."""
    from jimm_amd.ops import patch_embed

    torch.manual_seed(5)
    img = torch.randn(2, 3, 32, 32, device="cuda").bfloat16()
    w0 = (torch.randn(256, 3, 16, 16, device="cuda") * 0.03).bfloat16()
    b0 = torch.randn(256, device="cuda").bfloat16()
    dy = torch.randn(2, 4, 256, device="cuda").bfloat16()
    grads = {}
    for need in (False, True):
        im = img.clone().requires_grad_(need)
        w, b = w0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        patch_embed(im, w, b, 16).backward(dy)
        grads[need] = (im.grad, w.grad, b.grad)
    assert grads[False][0] is None
    assert grads[True][0] is not None and grads[True][0].shape == img.shape
    assert torch.equal(grads[False][1], grads[True][1])
    assert torch.equal(grads[False][2], grads[True][2])
