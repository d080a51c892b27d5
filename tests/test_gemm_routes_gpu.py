"""Which engine each GEMM path runs: the ordered list of extension and torch
GEMM calls that one forward + backward makes, per routing switch, against the
list the code made before the engine layer of ops/hip_linear.py existed. A
slip from an in-house kernel back to rocBLAS passes every numerical test; it
does not pass these.

The spies wrap every public callable of the extension and torch.matmul /
addmm / _scaled_mm. The shape predicates (``*_supported``) are wrapped but
not recorded: they launch nothing, and asking one is not a route.

Shapes: x = (2, 40, 256) is M = 80, one ragged row tile of the NT kernels and
one full 64-row step plus a 16-row tail of the TN kernel; L = 40 is the small
attention kernel; H = 256 / mlp = 512 are the smallest widths every in-house
GEMM of the block takes. All require an MI355X (gfx950)."""

import pytest
import torch

import jimm_amd  # noqa: F401
from jimm_amd.ops import _backend

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    EXT = _backend.ext()  # fail loudly — never silently skip to eager on a GPU box
else:
    pytest.skip("no GPU", allow_module_level=True)

SWITCHES = ("JIMM_AMD_ACT_SAVE", "JIMM_AMD_GEMM", "JIMM_AMD_DETERMINISTIC",
            "JIMM_AMD_FUSED_BLOCK", "JIMM_AMD_ATTN_BWD")


def dev():
    return torch.device("cuda:0")


def rel_err(out, ref):
    ref = ref.float()
    return (out.float() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)


@pytest.fixture
def trace(monkeypatch):
    """The names of the extension / torch GEMM calls, in call order."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    calls = []

    def wrap(owner, name, label):
        def spy(*a, _f=getattr(owner, name), **kw):
            if not label.endswith("_supported"):
                calls.append(label)
            return _f(*a, **kw)
        monkeypatch.setattr(owner, name, spy)

    for name in dir(EXT):
        if not name.startswith("_") and callable(getattr(EXT, name)):
            wrap(EXT, name, name)
    for name in ("matmul", "addmm", "_scaled_mm"):
        wrap(torch, name, "torch." + name)
    return calls


def make_block(H=256, heads=4, mlp=512, act="gelu", **kw):
    from jimm_amd.models.common.transformer import EncoderBlock

    torch.manual_seed(3)
    blk = EncoderBlock(H, heads, mlp, hidden_act=act, layernorm_epsilon=1e-6, **kw)
    blk = blk.to(dev(), torch.bfloat16)
    x = torch.randn(2, 40, H, device=dev()).bfloat16()
    return blk, x, torch.randn_like(x)


def run_block(blk, x, dy):
    for p in blk.parameters():
        p.grad = None
    xi = x.detach().clone().requires_grad_(True)
    y = blk(xi)
    y.backward(dy)
    torch.cuda.synchronize()
    return y.detach(), xi.grad.clone(), {n: p.grad.clone() for n, p in blk.named_parameters()}


# --- the fused block on the in-house GEMMs ---------------------------------

_LN_QKV_ATTN_PROJ_LN = ["layernorm_fwd", "linear_fwd", "attn_fwd", "linear_fwd", "layernorm_fwd"]
# after fc2-dX: fc2 dW+db, fc1 dX, fc1 dW+db, LN2, proj dX, proj dW+db,
# attention, qkv dX, qkv dW+db, LN1
_HIP_BWD_TAIL = [
    "gemm_tn_8p_db", "linear_fwd", "gemm_tn_8p_db", "layernorm_bwd",
    "linear_fwd", "gemm_tn_8p_db", "attn_bwd_fused",
    "linear_fwd", "gemm_tn_8p_db", "layernorm_bwd",
]

BLOCK_DEFAULT = (_LN_QKV_ATTN_PROJ_LN + ["linear_fwd_actgrad", "linear_fwd"]
                 + ["gemm_nt_8p_gradmul"] + _HIP_BWD_TAIL)
BLOCK_SAVE_Z = (_LN_QKV_ATTN_PROJ_LN + ["linear_fwd", "linear_fwd"]
                + ["gemm_nt_8p_gradact"] + _HIP_BWD_TAIL)
BLOCK_DROPOUT = (_LN_QKV_ATTN_PROJ_LN + ["linear_fwd_actgrad", "linear_fwd"]
                 + ["dropout_fwd", "gemm_nt_8p_gradmul"] + _HIP_BWD_TAIL)

# --- the fused block on rocBLAS (JIMM_AMD_GEMM=blas, or H below the gate) ---

_BLAS_FWD = [
    "layernorm_fwd", "torch.addmm", "attn_fwd", "torch.matmul", "bias_act_fwd",
    "layernorm_fwd", "torch.matmul", "bias_act_fwd", "torch.matmul", "bias_act_fwd",
]
BLOCK_BLAS = _BLAS_FWD + [
    "torch.matmul", "act_bwd", "torch.matmul", "colsum", "torch.matmul",
    "torch.matmul", "colsum", "layernorm_bwd",
    "torch.matmul", "torch.matmul", "colsum", "attn_bwd_fused",
    "torch.matmul", "torch.matmul", "colsum", "layernorm_bwd",
]
# hip mode, H = 128, mlp = 256: the block's own gate says blas, and none of
# its dX / dW shapes is one the per-shape gates of the helpers take. fc2-dX
# (80, 256, 128) is an 8-phase shape, but follows the block's gate.
BLOCK_H128 = BLOCK_BLAS

# deterministic: the fused dW+db kernel (db by fp32 atomics) gives way to
# matmul + colsum at all four sites
_DET_DW_DB = ["torch.matmul", "colsum"]
BLOCK_DETERMINISTIC = (
    _LN_QKV_ATTN_PROJ_LN + ["linear_fwd_actgrad", "linear_fwd", "gemm_nt_8p_gradmul"]
    + _DET_DW_DB + ["linear_fwd"] + _DET_DW_DB + ["layernorm_bwd", "linear_fwd"] + _DET_DW_DB
    + ["attn_bwd_fused", "linear_fwd"] + _DET_DW_DB + ["layernorm_bwd"]
)

# the composite block: four linear autograd Functions; fc2's backward comes
# first and has no activation, fc1's runs act_bwd ahead of its dX
BLOCK_COMPOSITE = [
    "layernorm_fwd", "linear_fwd", "attn_fwd", "linear_fwd", "layernorm_fwd",
    "linear_fwd", "linear_fwd",
    "linear_fwd", "gemm_tn_8p_db", "act_bwd", "linear_fwd", "gemm_tn_8p_db", "layernorm_bwd",
    "linear_fwd", "gemm_tn_8p_db", "attn_bwd_fused", "linear_fwd", "gemm_tn_8p_db",
    "layernorm_bwd",
]

BLOCK_FP8 = [
    "layernorm_fwd_fp8", "torch._scaled_mm", "attn_fwd", "linear_fwd",
    "layernorm_fwd_fp8", "torch._scaled_mm", "bias_act_fwd_fp8", "torch._scaled_mm",
    "bias_act_fwd",
    "gemm_nt_8p_gradact_fp8", "gemm_tn_8p_db", "torch._scaled_mm", "gemm_tn_8p_db",
    "layernorm_bwd", "linear_fwd", "gemm_tn_8p_db", "attn_bwd_fused",
    "linear_fwd", "gemm_tn_8p_db", "layernorm_bwd",
]

# hidden 256: forward and dX on the 8-phase kernel, dW on the TN kernel (its
# db is the separate colsum). hidden 384: N = 384 is no 8-phase shape, the
# forward and dW go to rocBLAS; dX (8, 768, 384) is one.
PATCH_EMBED_256 = ["im2col_patch", "linear_fwd", "linear_fwd", "col2im_patch", "gemm_tn_8p",
                   "colsum"]
PATCH_EMBED_384 = ["im2col_patch", "torch.matmul", "bias_act_fwd", "linear_fwd", "col2im_patch",
                   "torch.matmul", "colsum"]


def check(calls, expected):
    print(f"trace: {calls!r}")
    assert calls == expected, f"recorded trace: {calls!r}"


def test_block_default(trace):
    blk, x, dy = make_block()
    trace.clear()
    run_block(blk, x, dy)
    check(trace, BLOCK_DEFAULT)


def test_block_act_save_z(trace, monkeypatch):
    monkeypatch.setenv("JIMM_AMD_ACT_SAVE", "z")
    blk, x, dy = make_block()
    trace.clear()
    run_block(blk, x, dy)
    check(trace, BLOCK_SAVE_Z)


def test_block_gemm_blas(trace, monkeypatch):
    monkeypatch.setenv("JIMM_AMD_GEMM", "blas")
    blk, x, dy = make_block()
    trace.clear()
    run_block(blk, x, dy)
    check(trace, BLOCK_BLAS)


def test_block_deterministic(trace, monkeypatch):
    """Only the Python routing is observed here: the C++ LayerNorm backward
    reads JIMM_AMD_DETERMINISTIC once per process, so its own choice does not
    follow the variable set inside a running test."""
    monkeypatch.setenv("JIMM_AMD_DETERMINISTIC", "1")
    blk, x, dy = make_block()
    trace.clear()
    run_block(blk, x, dy)
    check(trace, BLOCK_DETERMINISTIC)


def test_block_composite(trace, monkeypatch):
    monkeypatch.setenv("JIMM_AMD_FUSED_BLOCK", "0")
    blk, x, dy = make_block()
    trace.clear()
    run_block(blk, x, dy)
    check(trace, BLOCK_COMPOSITE)


def test_block_dropout(trace):
    from jimm_amd.ops import set_dropout_seed

    set_dropout_seed(1234)
    blk, x, dy = make_block(dropout_rate=0.1)
    blk.train()
    trace.clear()
    run_block(blk, x, dy)
    check(trace, BLOCK_DROPOUT)


def test_block_fp8(trace):
    from jimm_amd.ops import block as blockmod
    from jimm_amd.ops import set_fp8

    blk, x, dy = make_block()
    set_fp8(True)
    blockmod._FP8_MIN_MH = 0
    try:
        trace.clear()
        run_block(blk, x, dy)
    finally:
        set_fp8(False)
        blockmod._FP8_MIN_MH = 1 << 26
    check(trace, BLOCK_FP8)


def test_block_below_h_gate(trace):
    blk, x, dy = make_block(H=128, heads=2, mlp=256)
    trace.clear()
    run_block(blk, x, dy)
    check(trace, BLOCK_H128)


@pytest.mark.parametrize("hidden,expected", [(256, "PATCH_EMBED_256"), (384, "PATCH_EMBED_384")])
def test_patch_embed(trace, hidden, expected):
    """(2, 3, 32, 32), patch 16: M = 8, K = 768; hidden 256 is an 8-phase
    shape, hidden 384 is not."""
    from jimm_amd.ops import patch_embed

    torch.manual_seed(5)
    img = torch.randn(2, 3, 32, 32, device=dev()).bfloat16().requires_grad_(True)
    w = (torch.randn(hidden, 3, 16, 16, device=dev()) * 0.03).bfloat16().requires_grad_(True)
    b = torch.randn(hidden, device=dev()).bfloat16().requires_grad_(True)
    trace.clear()
    y = patch_embed(img, w, b, 16)
    y.backward(torch.randn_like(y))
    torch.cuda.synchronize()
    assert y.shape == (2, 4, hidden)
    check(trace, globals()[expected])


# --- the MLP width the block's gate used not to look at ---------------------


@pytest.mark.parametrize("act", ["gelu", "quickgelu"])
@pytest.mark.parametrize("mlp", [384, 320])
def test_block_mlp_not_multiple_of_256(trace, monkeypatch, mlp, act):
    """H = 256 with an MLP width that is a multiple of 64 but not of 256: the
    8-phase kernel does not take fc1 (N = mlp), so the forward saves z, and
    fc2-dX cannot be the 8-phase gradact kernel either: it runs matmul +
    act_bwd. The fused block against the composite block, at the thresholds
    of test_fused_block_vs_composite. (fc1 goes through the guarded 128-tile
    kernel; fc2, with K = 384 or 320 and N = 256, is an 8-phase shape.)"""
    from jimm_amd.ops import block as block_mod

    blk, x, dy = make_block(mlp=mlp, act=act)
    assert block_mod.fused_block_enabled(x, 0.0)
    trace.clear()
    y_f, dx_f, g_f = run_block(blk, x, dy)
    fused = list(trace)
    assert "act_bwd" in fused and "gemm_nt_8p_gradact" not in fused, fused
    assert "linear_fwd" in fused and "torch.addmm" not in fused, fused
    monkeypatch.setenv("JIMM_AMD_FUSED_BLOCK", "0")
    y_c, dx_c, g_c = run_block(blk, x, dy)
    errs = {n: rel_err(g_f[n], g_c[n]) for n in g_f}
    print(f"mlp={mlp} {act}: y {rel_err(y_f, y_c):.3e} dx {rel_err(dx_f, dx_c):.3e} "
          + " ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert len(g_f) == 12
    assert rel_err(y_f, y_c) < 1e-2, rel_err(y_f, y_c)
    assert rel_err(dx_f, dx_c) < 2e-2, rel_err(dx_f, dx_c)
    for n, e in errs.items():
        assert e < 3e-2, (n, e)
