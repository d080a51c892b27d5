"""Attention-probability dropout inside the flash kernels (template flag DROP).

Oracle: the integer mask reference `ops.attn_keep_mask` and fp64 torch math on
the same bf16 inputs, O = ((P o m) * s) V with P normalised over all keys.
Bounds are the project's attention tolerances (test_attn_fwd_resident_gpu.py):
rel_err(o) < 3e-2, rel_err(dq, dk, dv) < 5e-2; lse is bitwise the p = 0 lse.
The exact-mask test decodes every keep bit from O. Inputs are strided views of
fused buffers, as in test_attn_strides_gpu.py.
"""

import math

import pytest
import torch

import jimm_amd  # noqa: F401
from jimm_amd import ops
from jimm_amd.models.common.transformer import Encoder
from jimm_amd.ops import _backend

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    EXT = _backend.ext()  # fail loudly — never silently skip to eager on a GPU box
else:
    pytest.skip("no GPU", allow_module_level=True)

B, H = 2, 3
TOL_O = 3e-2
TOL_LSE = 2e-2
TOL_BWD = 5e-2
SEED, STEP, SITE = 99, 7, (1 << 29) + 4

# (forward path, Lq, Lk, D)
CASES = [
    ("resident", 81, 81, 64),
    ("resident", 197, 197, 64),
    ("resident", 256, 256, 64),
    ("auto", 50, 50, 64),      # below the small-L threshold: auto -> tiled with p > 0
    ("tiled", 257, 257, 64),
    ("tiled", 100, 100, 72),   # DP = 96 with ragged Dr
    ("tiled", 1, 100, 64),     # MAP head
]
PS = [0.1, 0.5]


def dev():
    return torch.device("cuda:0")


def rel_err(out, ref):
    ref = ref.float()
    return (out.float() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)


def _rng():
    return torch.tensor([SEED, STEP], dtype=torch.int64, device=dev())


def _inputs(Lq, Lk, D):
    """q, k, v as (B, H, L, D) views of fused buffers, and dO."""
    g = torch.Generator(device=dev()).manual_seed(1000 * Lq + Lk + D)
    if Lq == Lk:
        qkv = torch.randn(B, Lk, 3, H, D, device=dev(), generator=g).bfloat16()
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
    else:
        qkv = None
        q = torch.randn(B, Lq, H, D, device=dev(), generator=g).bfloat16().transpose(1, 2)
        kv = torch.randn(B, Lk, 2, H, D, device=dev(), generator=g).bfloat16()
        k, v = kv[:, :, 0].transpose(1, 2), kv[:, :, 1].transpose(1, 2)
    do = torch.randn(B, Lq, H, D, device=dev(), generator=g).bfloat16().transpose(1, 2)
    return qkv, q, k, v, do


_REFS = {}


def _ref(Lq, Lk, D, p):
    """fp64 forward and gradients under the reference mask, once per case."""
    key = (Lq, Lk, D, p)
    if key not in _REFS:
        _, q, k, v, do = _inputs(Lq, Lk, D)
        q64, k64, v64 = (t.double().requires_grad_() for t in (q, k, v))
        keep = ops.attn_keep_mask(B * H, Lq, Lk, p, SEED, STEP, SITE, dev()).view(B, H, Lq, Lk)
        s = ops.attn_dropout_scale(ops.attn_dropout_threshold(p))
        sc = q64 @ k64.transpose(-1, -2) / math.sqrt(D)
        o64 = (torch.softmax(sc, dim=-1) * keep * s) @ v64
        grads = torch.autograd.grad(o64, (q64, k64, v64), do.double())
        _REFS[key] = (o64.detach(), grads, torch.logsumexp(sc.detach(), dim=-1))
    return _REFS[key]


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("path,Lq,Lk,D", CASES)
def test_forward(path, Lq, Lk, D, p):
    _, q, k, v, _ = _inputs(Lq, Lk, D)
    scale = 1.0 / math.sqrt(D)
    o, lse = EXT.attn_fwd(q, k, v, False, scale, path, p, _rng(), SITE)
    e = rel_err(o, _ref(Lq, Lk, D, p)[0])
    print(f"fwd {path} L=({Lq},{Lk}) D={D} p={p}: rel_err {e:.3e}")
    assert e < TOL_O


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("path,Lq,Lk,D", CASES)
def test_lse_is_undropped(path, Lq, Lk, D, p):
    """lse holds the undropped statistics: bit for bit the same kernel's lse at
    p = 0. At L <= 80 the p = 0 call runs the small-L kernel, another kernel,
    so there the project's lse bound against fp64 stands in."""
    _, q, k, v, _ = _inputs(Lq, Lk, D)
    scale = 1.0 / math.sqrt(D)
    _, lse = EXT.attn_fwd(q, k, v, False, scale, path, p, _rng(), SITE)
    if Lk <= 80:
        assert (lse.double() - _ref(Lq, Lk, D, p)[2]).abs().max().item() < TOL_LSE
        return
    lse0 = EXT.attn_fwd(q, k, v, False, scale, path)[1]
    print(f"lse {path} L=({Lq},{Lk}) D={D} p={p}: max |lse - lse0| "
          f"{(lse - lse0).abs().max().item():.3e}, {(lse != lse0).sum().item()} of {lse.numel()} differ")
    assert torch.equal(lse, lse0)


@pytest.mark.parametrize("path,L", [("resident", 197), ("tiled", 257)])
def test_exact_mask(path, L):
    """q = 0 makes every P equal; V[j, d] = 2^(j // 64) where j % 64 == d puts
    the keep bits of keys d, d + 64, ... of a query into O[i, d] as a binary
    number (at most 31, exact in bf16): all BH * L * L bits against the reference."""
    p, D = 0.5, 64
    q = torch.zeros(B, H, L, D, device=dev(), dtype=torch.bfloat16)
    k = torch.randn(B, H, L, D, device=dev()).bfloat16()
    j = torch.arange(L, device=dev())
    V = torch.zeros(L, D, device=dev())
    V[j, j % 64] = 2.0 ** (j // 64).float()
    v = V.bfloat16().expand(B, H, L, D).contiguous()
    o, _ = EXT.attn_fwd(q, k, v, False, 0.125, path, p, _rng(), SITE)
    s = ops.attn_dropout_scale(ops.attn_dropout_threshold(p))
    code = torch.round(o.float() * L / s).long()                     # (B, H, L, 64)
    got = ((code[..., j % 64] >> (j // 64)) & 1).bool().reshape(B * H, L, L)
    want = ops.attn_keep_mask(B * H, L, L, p, SEED, STEP, SITE, dev())
    assert torch.equal(got, want), f"{(got != want).sum().item()} of {want.numel()} bits differ"


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("path,Lq,Lk,D", CASES)
def test_backward(path, Lq, Lk, D, p):
    qkv, q, k, v, do = _inputs(Lq, Lk, D)
    if qkv is not None:
        qkv.requires_grad_()
        ops.attention_qkv(qkv, dropout_p=p, rng=_rng(), site=SITE).backward(do)
        got = tuple(qkv.grad[:, :, i].transpose(1, 2) for i in range(3))
    else:
        q, k, v = (t.detach().requires_grad_() for t in (q, k, v))
        ops.attention(q, k, v, dropout_p=p, rng=_rng(), site=SITE).backward(do)
        got = (q.grad, k.grad, v.grad)
    for name, a, r in zip(("dq", "dk", "dv"), got, _ref(Lq, Lk, D, p)[1]):
        e = rel_err(a, r)
        print(f"bwd L=({Lq},{Lk}) D={D} p={p} {name}: rel_err {e:.3e}")
        assert e < TOL_BWD, (name, e)


def _encoder(rate):
    torch.manual_seed(3)
    return Encoder(2, 128, 2, 256, attention_dropout_rate=rate).to(dev(), torch.bfloat16)


def _grads(enc, x, checkpointing):
    ops.set_dropout_seed(11)
    enc.gradient_checkpointing = checkpointing
    enc.zero_grad()
    x = x.clone().requires_grad_()
    y = enc(x)
    y.float().square().sum().backward()
    return [y.detach(), x.grad] + [p.grad.clone() for p in enc.parameters()]


def test_encoder_plumbing():
    x = torch.randn(2, 97, 128, device=dev()).bfloat16()
    enc = _encoder(0.25).train()
    plain, ckpt = _grads(enc, x, False), _grads(enc, x, True)
    assert all(torch.equal(a, b) for a, b in zip(plain, ckpt))   # the recompute replays the masks
    assert not torch.equal(enc(x), plain[0])                     # the next step draws new ones
    enc0 = _encoder(0.0).train()
    enc0.load_state_dict(enc.state_dict())
    assert not torch.equal(enc0(x), plain[0])                    # the dropout is active
    assert torch.equal(enc.eval()(x), enc0(x))                   # and off in eval mode


def test_domain():
    _, q, k, v, _ = _inputs(100, 100, 64)
    with pytest.raises(RuntimeError, match="causal"):
        EXT.attn_fwd(q, k, v, True, 0.125, "auto", 0.1, _rng(), SITE)
    with pytest.raises(RuntimeError, match="seed, step"):
        EXT.attn_fwd(q, k, v, False, 0.125, "auto", 0.1)
    # causal with dropout is served by the composite path
    o = ops.attention(q, k, v, causal=True, dropout_p=0.1, rng=_rng(), site=SITE)
    keep = ops.attn_keep_mask(B * H, 100, 100, 0.1, SEED, STEP, SITE, dev()).view(B, H, 100, 100)
    sc = (q.float() @ k.float().transpose(-1, -2)) * 0.125
    sc = sc.masked_fill(~torch.ones(100, 100, dtype=torch.bool, device=dev()).tril(), -math.inf)
    ref = (torch.softmax(sc, -1) * keep * ops.attn_dropout_scale(26)) @ v.float()
    assert rel_err(o, ref) < 2.0 ** -8  # the same fp32 math, rounded to bf16 once
