"""Resident attention backward (attn_bwd_fused path="resident") vs plain
softmax attention under fp64 autograd, and vs the tiled d2 + dkv + dq path.

Bound one is the project tolerance rel_err < 5e-2 (as in
test_attn_bwd_fused_kernel). Bound two ties the resident kernel to the tiled
pair on the same inputs: err_resident <= M_MARGIN * err_tiled for each of
dq, dk, dv. Both paths round P, dS and the outputs to bf16 and take delta
from the bf16 O, so their errors sit close together; a dropped or doubled
16-row strip moves the metric by several times. M_MARGIN is the largest
ratio measured over all cases of this file, rounded up to the next 0.25 and
at least 1.25 (profiles/attn_bwd_resident_NOTES.md has the ratios).
"""

import pytest
import torch

import jimm_amd  # noqa: F401
from jimm_amd.ops import _backend

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    EXT = _backend.ext()  # fail loudly — never silently skip to eager on a GPU box
else:
    pytest.skip("no GPU", allow_module_level=True)

LMAX = 256       # upper bound of the resident domain (RES_LMAX in attention_bwd_fused.hip)
M_MARGIN = 1.25
SCALE = 0.125
TOL = 5e-2


def dev():
    return torch.device("cuda:0")


def rel_err(out, ref):
    ref = ref.float()
    return (out.float() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)


def _ref_grads(q, k, v, do, causal=False):
    """fp64 autograd of plain softmax attention on the same bf16 values."""
    qr = q.detach().double().requires_grad_(True)
    kr = k.detach().double().requires_grad_(True)
    vr = v.detach().double().requires_grad_(True)
    s = torch.matmul(qr, kr.transpose(-1, -2)) * SCALE
    if causal:
        Lq, Lk = s.shape[-2], s.shape[-1]
        mask = torch.ones(Lq, Lk, dtype=torch.bool, device=s.device).tril()
        s = s.masked_fill(~mask, float("-inf"))
    torch.matmul(torch.softmax(s, dim=-1), vr).backward(do.double())
    return qr.grad, kr.grad, vr.grad


_CASES = {}


def _case(B, H, Lq, Lk, D=64, causal=False, qmul=1.0, seed=0):
    """Inputs, forward outputs and the fp64 reference, built once per case."""
    key = (B, H, Lq, Lk, D, causal, qmul, seed)
    if key not in _CASES:
        g = torch.Generator(device=dev()).manual_seed(1000 + seed)
        q = (torch.randn(B, H, Lq, D, device=dev(), generator=g) * qmul).bfloat16()
        k = torch.randn(B, H, Lk, D, device=dev(), generator=g).bfloat16()
        v = torch.randn(B, H, Lk, D, device=dev(), generator=g).bfloat16()
        do = torch.randn(B, H, Lq, D, device=dev(), generator=g).bfloat16()
        o, lse = EXT.attn_fwd(q, k, v, causal, SCALE)
        _CASES[key] = (q, k, v, do, o.contiguous(), lse, _ref_grads(q, k, v, do, causal))
    return _CASES[key]


def _run(case, causal, path):
    q, k, v, do, o, lse, _ = case
    nan = float("nan")
    dq, dk, dv = (torch.full_like(t, nan) for t in (q, k, v))  # unwritten rows fail
    EXT.attn_bwd_fused(q, k, v, o, do, lse, dq, dk, dv, causal, SCALE, path)
    return dq, dk, dv


def _errs(outs, refs):
    return [rel_err(a, r) for a, r in zip(outs, refs)]


def _check_both_bounds(case, tag):
    refs = case[6]
    e_res = _errs(_run(case, False, "resident"), refs)
    e_til = _errs(_run(case, False, "tiled"), refs)
    for name, er, et in zip(("dq", "dk", "dv"), e_res, e_til):
        print(f"{tag} {name}: resident {er:.4e} tiled {et:.4e} ratio {er / et:.3f}")
    for name, er, et in zip(("dq", "dk", "dv"), e_res, e_til):
        assert er < TOL, (tag, name, er)
        assert er <= M_MARGIN * et, (tag, name, er, et)


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("L", [81, 96, 112, 197, 208, LMAX - 1, LMAX])
def test_resident_strip_structure(L):
    """81: one valid row in the last strip; 96: whole 32-row blocks; 112: odd
    strip count (last 32-key step half padding); 197: flagship; 208: exact
    strips; LMAX-1 / LMAX: upper bounds (8 waves, 16 strips at 256)."""
    _check_both_bounds(_case(2, 3, L, L, seed=L), f"L={L}")


def test_resident_peaked_softmax():
    """q scaled by 4: P approaches 1 on some rows."""
    _check_both_bounds(_case(2, 3, 197, 197, qmul=4.0, seed=7), "peaked")


def test_resident_strided_io():
    """q/k/v are views of a fused (B,L,3,H,64) projection, dO/O have
    (B,L,H,64) storage, outputs are the three views of one dqkv buffer with
    sentinel guard zones in front and behind."""
    B, L, H, G = 2, 197, 3, 4096
    g = torch.Generator(device=dev()).manual_seed(11)
    qkv = torch.randn(B, L, 3, H, 64, device=dev(), generator=g).bfloat16()
    q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
    do = torch.randn(B, L, H, 64, device=dev(), generator=g).bfloat16().transpose(1, 2)
    o, lse = EXT.attn_fwd(q, k, v, False, SCALE)
    assert not q.is_contiguous() and not do.is_contiguous() and not o.is_contiguous()
    sentinel = -7.0
    buf = torch.full((qkv.numel() + 2 * G,), sentinel, device=dev(), dtype=torch.bfloat16)
    dqkv = buf[G:G + qkv.numel()].view_as(qkv)
    dqkv.fill_(float("nan"))
    dq, dk, dv = (dqkv[:, :, i].transpose(1, 2) for i in range(3))
    EXT.attn_bwd_fused(q, k, v, o, do, lse, dq, dk, dv, False, SCALE, "resident")
    refs = _ref_grads(q, k, v, do)
    for name, a, r in zip(("dq", "dk", "dv"), (dq, dk, dv), refs):
        assert rel_err(a, r) < TOL, (name, rel_err(a, r))
    assert bool((buf[:G] == sentinel).all()) and bool((buf[-G:] == sentinel).all())


@pytest.mark.parametrize(
    "B,H,Lq,Lk,D,causal",
    [
        (2, 2, 80, 80, 64, False),              # last L of the small kernel
        (2, 2, LMAX + 1, LMAX + 1, 64, False),  # first L past the resident domain
        (2, 2, 1, 256, 64, False),              # Lq != Lk (MAP head)
        (2, 2, 130, 130, 96, False),            # D != 64
        (2, 2, 130, 130, 64, True),             # causal stays on the tiled path
        (1, 2, 197, 197, 64, True),
    ],
)
def test_auto_dispatch_boundaries(B, H, Lq, Lk, D, causal):
    case = _case(B, H, Lq, Lk, D=D, causal=causal, seed=3)
    outs = _run(case, causal, "auto")
    for name, e in zip(("dq", "dk", "dv"), _errs(outs, case[6])):
        assert e < TOL, (name, e)


@pytest.mark.parametrize(
    "B,H,Lq,Lk,D,causal",
    [
        (2, 2, 130, 130, 96, False),
        (2, 2, 1, 256, 64, False),
        (2, 2, LMAX + 1, LMAX + 1, 64, False),
        (2, 2, 130, 130, 64, True),
    ],
)
def test_resident_rejects_out_of_domain(B, H, Lq, Lk, D, causal):
    """Host-side check, raised before any launch."""
    case = _case(B, H, Lq, Lk, D=D, causal=causal, seed=3)
    with pytest.raises(RuntimeError, match="resident"):
        _run(case, causal, "resident")


def test_resident_deterministic():
    case = _case(2, 3, 197, 197, seed=197)
    a = _run(case, False, "resident")
    b = _run(case, False, "resident")
    for x, y in zip(a, b):
        assert torch.equal(x, y)
