"""Attention kernels on views that all have DIFFERENT layouts.

Each kernel takes one stride triple per tensor. The other strided tests pass
q, k, v (and dq, dk, dv) as views of one fused buffer, so all their triples
are equal and a swapped pair would go unnoticed. Here every tensor has its own
layout (and B != H), and the result must be bitwise equal to the same call on
contiguous clones of the same values.

Exact equality is derived, not measured: none of the kernels uses atomics, no
arithmetic depends on an address, and the dispatch depends only on shapes,
`causal`, `path` and the resident path's alignment predicate, which all these
layouts satisfy (strides multiples of 8, base offsets multiples of 16 bytes).

Output views and their backing storage start as NaN; whatever lies outside a
view must still be NaN afterwards.
"""

import math

import pytest
import torch

import jimm_amd  # noqa: F401
from jimm_amd.ops import _backend

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    EXT = _backend.ext()  # fail loudly — never silently skip to eager on a GPU box
else:
    pytest.skip("no GPU", allow_module_level=True)

B, H = 2, 3  # B != H on purpose
NAN = float("nan")


def dev():
    return torch.device("cuda:0")


def _randn(g, *shape):
    return torch.randn(*shape, device=dev(), generator=g).bfloat16()


_CASES = {}


def _case(L, D, causal):
    """Strided inputs, their contiguous clones and both forward results,
    built once per (L, D, causal)."""
    key = (L, D, causal)
    if key not in _CASES:
        g = torch.Generator(device=dev()).manual_seed(100 * L + D + int(causal))
        scale = 1.0 / math.sqrt(D)
        q = _randn(g, B, L, 3, H, D)[:, :, 0].transpose(1, 2)      # slot 0 of a fused qkv
        k = _randn(g, B, H, L, D)                                  # contiguous
        v = _randn(g, B, L + 3, H, D)[:, :L].permute(0, 2, 1, 3)   # padded-L storage
        do = _randn(g, B, L, H, D + 8)[..., :D].permute(0, 2, 1, 3)  # padded-D storage
        strided = (q, k, v, do)
        assert len({t.stride() for t in strided}) == 4
        contig = tuple(t.contiguous() for t in strided)
        fwd_s = EXT.attn_fwd(q, k, v, causal, scale)
        fwd_c = EXT.attn_fwd(*contig[:3], causal, scale)
        _CASES[key] = (strided, contig, fwd_s, fwd_c, scale)
    return _CASES[key]


FWD_CASES = [
    (70, 64, False),   # small forward
    (70, 64, True),
    (100, 64, False),  # tiled forward, DP = 64
    (100, 64, True),
    (100, 80, False),  # tiled forward, DP = 96 with ragged Dr
]


@pytest.mark.parametrize("L,D,causal", FWD_CASES)
def test_fwd_distinct_layouts(L, D, causal):
    _, _, (o_s, lse_s), (o_c, lse_c), _ = _case(L, D, causal)
    assert torch.equal(o_s, o_c)
    assert torch.equal(lse_s, lse_c)


@pytest.mark.parametrize(
    "L,D,causal,path",
    [
        (70, 64, False, "auto"),       # small backward
        (70, 64, True, "auto"),
        (70, 64, False, "tiled"),      # tiled backward below the small threshold
        (70, 64, True, "tiled"),
        (100, 64, False, "resident"),
        (100, 64, False, "tiled"),
        (100, 64, True, "tiled"),
        (100, 80, False, "tiled"),     # DP = 96 with ragged Dr
    ],
)
def test_bwd_distinct_layouts(L, D, causal, path):
    (q, k, v, do), (qc, kc, vc, doc), (o_s, lse), _, scale = _case(L, D, causal)
    # o input: padded-L storage, holding the forward's values
    o = torch.full((B, H, L + 1, D), NAN, device=dev(), dtype=torch.bfloat16)[:, :, :L]
    o.copy_(o_s)
    dq = torch.full((B, H, L, D), NAN, device=dev(), dtype=torch.bfloat16)
    # slot 1 of a second fused buffer; four slots, so that its strides differ from q's
    dk_buf = torch.full((B, L, 4, H, D), NAN, device=dev(), dtype=torch.bfloat16)
    dk = dk_buf[:, :, 1].transpose(1, 2)
    dv = torch.full((B, L, H, D), NAN, device=dev(), dtype=torch.bfloat16).permute(0, 2, 1, 3)
    assert len({t.stride() for t in (q, k, v, o, do, dk, dv)}) == 7  # dq shares k's (contiguous)
    EXT.attn_bwd_fused(q, k, v, o, do, lse, dq, dk, dv, causal, scale, path)

    ref = tuple(torch.full((B, H, L, D), NAN, device=dev(), dtype=torch.bfloat16) for _ in range(3))
    EXT.attn_bwd_fused(qc, kc, vc, o_s.contiguous(), doc, lse, *ref, causal, scale, path)
    for name, a, r in zip(("dq", "dk", "dv"), (dq, dk, dv), ref):
        assert torch.equal(a, r), name
    # the slots around dk are untouched
    assert bool(dk_buf[:, :, 0].isnan().all()) and bool(dk_buf[:, :, 2:].isnan().all())


def test_bwd_rejects_mismatched_dk():
    """Host-side shape check, raised before any launch (dk is the larger one,
    so even an unchecked launch would stay inside it)."""
    L, D = 70, 64
    (q, k, v, do), _, (o_s, lse), _, scale = _case(L, D, False)
    dq, dv = torch.empty_like(q), torch.empty_like(v)
    dk = torch.empty(B, H, L + 1, D, device=dev(), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="attn_bwd_fused: dk"):
        EXT.attn_bwd_fused(q, k, v, o_s, do, lse, dq, dk, dv, False, scale, "tiled")
