"""Attention-probability dropout: the mask definition and the composite path.

The integer reference `attn_keep_mask` is the oracle of the GPU tests; here
its statistics, its dependence on every argument, and the composite torch
path of `ops.attention(dropout_p=...)` against the formula written out:
O = ((P o m) * s) V with P normalised over all keys.
"""

import math

import pytest
import torch

from jimm_amd import ops

SEED, STEP, SITE = 1234, 5, (1 << 29) + 2


def _rng():
    return torch.tensor([SEED, STEP], dtype=torch.int64)


def test_keep_rate():
    """p = 0.1 runs at t8 / 256 = 26 / 256. Over n = 16384 bits the keep rate
    has sigma = sqrt(r (1 - r) / n) = 0.00236; the bound is 5 sigma."""
    assert ops.attn_dropout_threshold(0.1) == 26
    assert ops.attn_dropout_scale(26) == torch.tensor(256.0 / 230.0).item()
    keep = ops.attn_keep_mask(4, 64, 64, 0.1, SEED, STEP, SITE)
    assert keep.shape == (4, 64, 64) and keep.dtype == torch.bool
    assert abs(keep.float().mean().item() - (1 - 26 / 256)) < 0.012


@pytest.mark.parametrize("arg", ["bh", "site", "step", "seed"])
def test_mask_depends_on(arg):
    base = ops.attn_keep_mask(2, 64, 64, 0.5, SEED, STEP, SITE)
    if arg == "bh":
        other = base[1]
        base = base[0]
    else:
        kw = {"seed": SEED, "step": STEP, "site": SITE}
        kw[arg] += 1
        other = ops.attn_keep_mask(2, 64, 64, 0.5, **kw)
    # independent fair bits agree on half the positions: 5 sigma is 0.04 at 4096 bits
    assert abs((base == other).float().mean().item() - 0.5) < 0.05


def test_mask_is_a_function_of_the_element():
    """A window of a larger mask is the smaller mask: nothing depends on Lq, Lk or BH."""
    big = ops.attn_keep_mask(3, 37, 70, 0.3, SEED, STEP, SITE)
    small = ops.attn_keep_mask(2, 9, 13, 0.3, SEED, STEP, SITE)
    assert torch.equal(big[:2, :9, :13], small)


def test_composite_matches_formula_and_gradcheck():
    B, H, L, D, p = 1, 2, 6, 8, 0.4
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(B, H, L, D, generator=g, dtype=torch.float64, requires_grad=True)
               for _ in range(3))
    rng = _rng()
    out = ops.attention(q, k, v, dropout_p=p, rng=rng, site=SITE)
    keep = ops.attn_keep_mask(B * H, L, L, p, SEED, STEP, SITE).view(B, H, L, L)
    s = ops.attn_dropout_scale(ops.attn_dropout_threshold(p))
    assert not keep.all() and keep.any()
    P = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(D), dim=-1)
    ref = (P * keep * s) @ v
    assert torch.allclose(out, ref, rtol=1e-12, atol=1e-12)
    assert torch.autograd.gradcheck(
        lambda a, b, c: ops.attention(a, b, c, dropout_p=p, rng=rng, site=SITE), (q, k, v))


def test_default_is_unchanged():
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(2, 2, 9, 8, generator=g) for _ in range(3))
    qkv = torch.randn(2, 9, 3, 2, 8, generator=g)
    assert torch.equal(ops.attention(q, k, v), ops.attention(q, k, v, dropout_p=0.0))
    assert torch.equal(ops.attention_qkv(qkv), ops.attention_qkv(qkv, dropout_p=0.0, site=3))
    with pytest.raises(ValueError, match="rng"):
        ops.attention(q, k, v, dropout_p=0.1)
