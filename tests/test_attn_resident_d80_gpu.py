"""Resident attention kernels for head dims 72 and 80 (attn_fwd and
attn_bwd_fused with path="resident") vs fp64 softmax attention and fp64
autograd on the same bf16 values.

Tolerances are those of the D = 64 resident tests (test_attn_fwd_resident_gpu,
test_attn_bwd_resident_gpu): the arithmetic is the same, with an 80-deep
contraction where D = 64 has a 64-deep one. q, k, v are the strided views of
one fused (B, L, 3, H, D) buffer, in which the columns that follow a head's D
are the next head's data; dq, dk, dv are the views of one dqkv buffer between
sentinel guard regions.
"""

import math

import pytest
import torch

import jimm_amd  # noqa: F401
from jimm_amd import ops
from jimm_amd.ops import _backend

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    EXT = _backend.ext()  # fail loudly — never silently skip to eager on a GPU box
else:
    pytest.skip("no GPU", allow_module_level=True)

B, H, G = 2, 3, 4096
TOL_O, TOL_LSE, TOL_BWD = 3e-2, 2e-2, 5e-2
SENTINEL = -7.0
# 81: smallest L, 3 waves, ragged last block; 97: one row past a 32 boundary;
# 197; 256: the LDS extreme
SHAPES = [(D, L) for D in (72, 80) for L in (81, 97, 197, 256)]


def dev():
    return torch.device("cuda:0")


def rel_err(out, ref):
    ref = ref.float()
    return (out.float() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)


_CASES = {}


def _case(D, L, qmul=1.0, offset=False, big_neighbours=False):
    """Fused qkv buffer, dO and the fp64 reference (o, lse, grads), once per
    case. offset: q = 1 + 0.1 randn, k = -1 + 0.1 randn. big_neighbours: every
    head but head 1 holds 64.0 in q, k and v, so head 1's columns D.. of the
    fused rows (head 2's data) and the columns in front of it are large."""
    key = (D, L, qmul, offset, big_neighbours)
    if key not in _CASES:
        g = torch.Generator(device=dev()).manual_seed(3000 + 10 * L + D)
        qkv = torch.randn(B, L, 3, H, D, device=dev(), generator=g)
        qkv[:, :, 0] *= qmul
        if offset:
            qkv[:, :, 0] = 1.0 + 0.1 * qkv[:, :, 0]
            qkv[:, :, 1] = -1.0 + 0.1 * qkv[:, :, 1]
        if big_neighbours:
            qkv[:, :, :, 0] = 64.0
            qkv[:, :, :, 2] = 64.0
        qkv = qkv.bfloat16()
        do = torch.randn(B, L, H, D, device=dev(), generator=g).bfloat16().transpose(1, 2)
        q64, k64, v64 = (qkv[:, :, i].transpose(1, 2).double().requires_grad_() for i in range(3))
        s = q64 @ k64.transpose(-1, -2) / math.sqrt(D)
        o64 = torch.softmax(s, dim=-1) @ v64
        grads = torch.autograd.grad(o64, (q64, k64, v64), do.double())
        _CASES[key] = (qkv, do, o64.detach(), torch.logsumexp(s.detach(), dim=-1), grads)
    return _CASES[key]


def _heads(qkv):
    return [qkv[:, :, i].transpose(1, 2) for i in range(3)]


def _check_fwd(case, D, path, heads=slice(None)):
    qkv, _, o64, lse64, _ = case
    o, lse = EXT.attn_fwd(*_heads(qkv), False, 1.0 / math.sqrt(D), path)
    eo = rel_err(o[:, heads], o64[:, heads])
    el = (lse.double() - lse64)[:, heads].abs().max().item()
    print(f"fwd {path}: o {eo:.4e} lse {el:.4e}")
    assert eo < TOL_O and el < TOL_LSE, (eo, el)
    return o, lse


@pytest.mark.parametrize("D,L", SHAPES)
def test_forward(D, L):
    o, _ = _check_fwd(_case(D, L), D, "resident")
    assert o.transpose(1, 2).is_contiguous()  # (B, L, H, D) storage


@pytest.mark.parametrize("D,L", SHAPES)
def test_backward(D, L):
    qkv, do, _, _, grads = _case(D, L)
    q, k, v = _heads(qkv)
    o, lse = EXT.attn_fwd(q, k, v, False, 1.0 / math.sqrt(D), "resident")
    buf = torch.full((qkv.numel() + 2 * G,), SENTINEL, device=dev(), dtype=torch.bfloat16)
    dqkv = buf[G:G + qkv.numel()].view_as(qkv)
    dqkv.fill_(float("nan"))  # unwritten elements fail
    EXT.attn_bwd_fused(q, k, v, o, do, lse, *_heads(dqkv), False, 1.0 / math.sqrt(D), "resident")
    for name, a, r in zip(("dq", "dk", "dv"), _heads(dqkv), grads):
        e = rel_err(a, r)
        print(f"bwd D={D} L={L} {name}: {e:.4e}")
        assert e < TOL_BWD, (name, e)
    assert bool((buf[:G] == SENTINEL).all()) and bool((buf[-G:] == SENTINEL).all())


def test_padding_is_inert():
    """D = 72 fills 80-column images. Head 1 is checked while its neighbours
    in the fused row hold 64.0: one leaked column adds 64 * q (or 64 * 64) to a
    score whose true value is about -8 +- 1 (offset inputs, q scaled by 4 in
    front of the offset), and a leaked V column moves O by 64."""
    _check_fwd(_case(72, 97, qmul=4.0, offset=True), 72, "resident")
    _check_fwd(_case(72, 97, qmul=4.0, offset=True, big_neighbours=True), 72, "resident",
               heads=slice(1, 2))


@pytest.mark.parametrize("D,L", SHAPES)
def test_auto_through_ops(D, L):
    """ops.attention_qkv forward and backward, whichever kernel auto picks."""
    qkv, do, o64, _, grads = _case(D, L)
    x = qkv.clone().requires_grad_()
    o = ops.attention_qkv(x)
    assert rel_err(o, o64) < TOL_O
    o.backward(do)
    for i, r in enumerate(grads):
        e = rel_err(x.grad[:, :, i].transpose(1, 2), r)
        assert e < TOL_BWD, (i, e)


def test_d96_still_rejected():
    q = torch.zeros(2, 2, 130, 96, device=dev(), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="resident"):
        EXT.attn_fwd(q, q, q, False, 0.125, "resident")
    dq = torch.empty_like(q)
    lse = torch.zeros(2, 2, 130, device=dev())
    with pytest.raises(RuntimeError, match="resident"):
        EXT.attn_bwd_fused(q, q, q, q, q, lse, dq, dq, dq, False, 0.125, "resident")


def test_dropout_stays_on_tiled_kernels():
    """D = 72 with p = 0.1 inside the resident L range: auto takes the tiled
    DROP kernels and matches the reference mask."""
    D, L, p, seed, step, site = 72, 130, 0.1, 99, 7, 5
    qkv, do, _, _, _ = _case(D, L)
    rng = torch.tensor([seed, step], dtype=torch.int64, device=dev())
    q64, k64, v64 = (t.double().requires_grad_() for t in _heads(qkv))
    keep = ops.attn_keep_mask(B * H, L, L, p, seed, step, site, dev()).view(B, H, L, L)
    sd = ops.attn_dropout_scale(ops.attn_dropout_threshold(p))
    o64 = (torch.softmax(q64 @ k64.transpose(-1, -2) / math.sqrt(D), dim=-1) * keep * sd) @ v64
    grads = torch.autograd.grad(o64, (q64, k64, v64), do.double())
    x = qkv.clone().requires_grad_()
    o = ops.attention_qkv(x, dropout_p=p, rng=rng, site=site)
    assert rel_err(o, o64) < TOL_O
    o.backward(do)
    for i, r in enumerate(grads):
        assert rel_err(x.grad[:, :, i].transpose(1, 2), r) < TOL_BWD, i
    with pytest.raises(RuntimeError, match="resident"):
        EXT.attn_fwd(*_heads(qkv), False, 1.0 / math.sqrt(D), "resident", p, rng, site)
