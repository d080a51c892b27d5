"""Resident attention forward (attn_fwd path="resident") vs fp64 softmax
attention on the same bf16 values, and vs the tiled kernel (path="tiled").

Bound one is the project tolerance: rel_err(o) < 3e-2 and
max |lse - lse64| < 2e-2. Bound two ties the resident kernel to the tiled one
on the same inputs: err_resident <= M * err_tiled, for o (rel_err) and for
lse (max abs difference). Both kernels round P and O to bf16 and keep the
statistics in fp32, so their errors sit close together; a dropped, doubled or
leaked 16-row strip or key tile moves either metric by orders of magnitude.
M is set per quantity by the project's rule: the largest ratio measured over
all cases of this file, rounded up to the next 0.25 and at least 1.25
(profiles/attn_fwd_resident_NOTES.md has the ratios).
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

LMAX = 256  # upper bound of the resident domain (RES_LMAX in mfma.h)
M_O = 1.25
M_LSE = 1.25
SCALE = 0.125
TOL_O = 3e-2
TOL_LSE = 2e-2
TOL_BWD = 5e-2


def dev():
    return torch.device("cuda:0")


def rel_err(out, ref):
    ref = ref.float()
    return (out.float() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)


def lse_err(lse, ref):
    return (lse.double() - ref).abs().max().item()


def _ref_fwd(q, k, v, causal=False):
    """fp64 softmax attention on the same bf16 values: (o64, lse64)."""
    s = torch.matmul(q.double(), k.double().transpose(-1, -2)) * SCALE
    if causal:
        Lq, Lk = s.shape[-2], s.shape[-1]
        mask = torch.ones(Lq, Lk, dtype=torch.bool, device=s.device).tril()
        s = s.masked_fill(~mask, float("-inf"))
    return torch.matmul(torch.softmax(s, dim=-1), v.double()), torch.logsumexp(s, dim=-1)


_CASES = {}


def _case(B, H, Lq, Lk, D=64, causal=False, qmul=1.0, seed=0, offset=False):
    """Inputs and the fp64 reference, built once per case. offset: q = 1 +
    0.1 randn, k = -1 + 0.1 randn, so every true score is about -8."""
    key = (B, H, Lq, Lk, D, causal, qmul, seed, offset)
    if key not in _CASES:
        g = torch.Generator(device=dev()).manual_seed(2000 + seed)
        qf = torch.randn(B, H, Lq, D, device=dev(), generator=g) * qmul
        kf = torch.randn(B, H, Lk, D, device=dev(), generator=g)
        if offset:
            qf, kf = 1.0 + 0.1 * qf, -1.0 + 0.1 * kf
        q, k = qf.bfloat16(), kf.bfloat16()
        v = torch.randn(B, H, Lk, D, device=dev(), generator=g).bfloat16()
        _CASES[key] = (q, k, v, _ref_fwd(q, k, v, causal))
    return _CASES[key]


def _errs(case, causal, path):
    q, k, v, (o64, lse64) = case
    o, lse = EXT.attn_fwd(q, k, v, causal, SCALE, path)
    return rel_err(o, o64), lse_err(lse, lse64)


def _check_tolerance(case, causal, path, tag):
    eo, el = _errs(case, causal, path)
    print(f"{tag} {path}: o {eo:.4e} lse {el:.4e}")
    assert eo < TOL_O, (tag, eo)
    assert el < TOL_LSE, (tag, el)


def _check_both_bounds(case, tag):
    ro, rl = _errs(case, False, "resident")
    to, tl = _errs(case, False, "tiled")
    print(f"{tag} o: resident {ro:.4e} tiled {to:.4e} ratio {ro / to:.3f}")
    print(f"{tag} lse: resident {rl:.4e} tiled {tl:.4e} ratio {rl / tl:.3f}")
    assert ro < TOL_O, (tag, ro)
    assert rl < TOL_LSE, (tag, rl)
    assert ro <= M_O * to, (tag, ro, to)
    assert rl <= M_LSE * tl, (tag, rl, tl)


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("L", [81, 96, 112, 197, 208, LMAX - 1, LMAX])
def test_resident_strip_structure(L):
    """81: one live row in the last strip; 96: whole 32-row blocks; 112: odd
    strip count (last 32-key block half padding); 197: flagship; 208: exact
    strips; LMAX-1 / LMAX: upper bounds (8 waves)."""
    _check_both_bounds(_case(2, 3, L, L, seed=L), f"L={L}")


def test_resident_peaked_softmax():
    """q scaled by 4: P approaches 1 on some rows."""
    _check_both_bounds(_case(2, 3, 197, 197, qmul=4.0, seed=7), "peaked")


@pytest.mark.parametrize("L", [81, 197, LMAX - 1])
def test_resident_padding_keys_do_not_count(L):
    """Every true score is about -8, so lse64 is about -8 + log L; one leaked
    zero-row key (score 0) would move lse by more than 2."""
    case = _case(2, 3, L, L, seed=50 + L, offset=True)
    lse64 = case[3][1]
    assert (lse64 - (-8.0 + math.log(L))).abs().max().item() < 0.5
    _check_both_bounds(case, f"offset L={L}")


def test_resident_strided_io():
    """q/k/v are views of a fused (B,L,3,H,64) projection; o comes back in
    (B,L,H,64) storage and the inputs stay untouched."""
    B, L, H = 2, 197, 3
    g = torch.Generator(device=dev()).manual_seed(11)
    qkv = torch.randn(B, L, 3, H, 64, device=dev(), generator=g).bfloat16()
    before = qkv.clone()
    q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
    assert not q.is_contiguous()
    o, lse = EXT.attn_fwd(q, k, v, False, SCALE, "resident")
    assert o.transpose(1, 2).is_contiguous()
    assert torch.equal(qkv.view(torch.int16), before.view(torch.int16))
    o64, lse64 = _ref_fwd(q, k, v)
    assert rel_err(o, o64) < TOL_O
    assert lse_err(lse, lse64) < TOL_LSE


_OUTSIDE = [
    (2, 2, 1, 256, 64, False),     # Lq != Lk (MAP head)
    (2, 2, 130, 130, 96, False),   # D != 64
    (2, 2, 130, 130, 64, True),    # causal stays on the tiled path
    (1, 2, 197, 197, 64, True),
]


@pytest.mark.parametrize(
    "B,H,Lq,Lk,D,causal",
    [
        (2, 2, 80, 80, 64, False),              # last L of the small kernel
        (2, 2, LMAX + 1, LMAX + 1, 64, False),  # first L past the resident domain
    ]
    + _OUTSIDE,
)
def test_auto_dispatch_boundaries(B, H, Lq, Lk, D, causal):
    case = _case(B, H, Lq, Lk, D=D, causal=causal, seed=3)
    _check_tolerance(case, causal, "auto", f"auto {Lq}x{Lk} D={D} causal={causal}")


@pytest.mark.parametrize("B,H,Lq,Lk,D,causal", _OUTSIDE)
def test_resident_rejects_out_of_domain(B, H, Lq, Lk, D, causal):
    """Host-side check, raised before any launch."""
    q, k, v, _ = _case(B, H, Lq, Lk, D=D, causal=causal, seed=3)
    with pytest.raises(RuntimeError, match="resident"):
        EXT.attn_fwd(q, k, v, causal, SCALE, "resident")


@pytest.mark.parametrize("L", [80, LMAX + 1])
def test_resident_rejects_lengths_outside(L):
    q, k, v, _ = _case(2, 2, L, L, seed=3)
    with pytest.raises(RuntimeError, match="resident"):
        EXT.attn_fwd(q, k, v, False, SCALE, "resident")


def test_resident_rejects_misaligned_view():
    """q starts 4 elements (8 bytes) into its buffer: not 16-byte aligned."""
    B, H, L = 2, 2, 130
    n = B * H * L * 64
    buf = torch.zeros(n + 8, device=dev(), dtype=torch.bfloat16)
    q = buf[4:4 + n].view(B, H, L, 64)
    k = torch.zeros(B, H, L, 64, device=dev(), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="resident"):
        EXT.attn_fwd(q, k, k, False, SCALE, "resident")
    # auto still serves the view, on the tiled kernel
    o, lse = EXT.attn_fwd(q, k, k, False, SCALE)
    assert bool((o == 0).all()) and lse_err(lse, torch.full_like(lse, math.log(L)).double()) < TOL_LSE


def test_resident_deterministic():
    q, k, v, _ = _case(2, 3, 197, 197, seed=197)
    a = EXT.attn_fwd(q, k, v, False, SCALE, "resident")
    b = EXT.attn_fwd(q, k, v, False, SCALE, "resident")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_auto_takes_resident_at_flagship_length():
    """auto and resident are the same kernel at L = 197: identical bits."""
    q, k, v, _ = _case(2, 3, 197, 197, seed=197)
    a = EXT.attn_fwd(q, k, v, False, SCALE)
    b = EXT.attn_fwd(q, k, v, False, SCALE, "resident")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_resident_forward_into_resident_backward():
    """Resident o and lse feed attn_bwd_fused(path="resident"); gradients meet
    the backward's 5e-2 bound against fp64 autograd."""
    q, k, v, _ = _case(2, 3, 197, 197, seed=197)
    g = torch.Generator(device=dev()).manual_seed(5)
    do = torch.randn(2, 3, 197, 64, device=dev(), generator=g).bfloat16()
    o, lse = EXT.attn_fwd(q, k, v, False, SCALE, "resident")
    dq, dk, dv = (torch.full_like(t, float("nan")) for t in (q, k, v))
    EXT.attn_bwd_fused(q, k, v, o, do, lse, dq, dk, dv, False, SCALE, "resident")
    qr, kr, vr = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    s = torch.matmul(qr, kr.transpose(-1, -2)) * SCALE
    torch.matmul(torch.softmax(s, dim=-1), vr).backward(do.double())
    for name, a, r in zip(("dq", "dk", "dv"), (dq, dk, dv), (qr.grad, kr.grad, vr.grad)):
        assert rel_err(a, r) < TOL_BWD, (name, rel_err(a, r))
