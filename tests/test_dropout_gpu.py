"""Counter-based dropout on the GPU against the CPU oracle
(jimm_amd.ops.philox_dropout): the standalone kernel, the fc1 and fc2
epilogues of the 8-phase GEMM, the fused block against the composite block,
checkpointing, a captured training step and eval mode.

GEMM shapes are those of test_gemm_actgrad_gpu.py, for its reasons: K = 128 is
the smallest K the 8-phase kernel takes, N = 512 gives two column tiles (so a
wrong column-group index shows), M = 300 a second, ragged row tile, M = 100 a
single ragged one. All require an MI355X (gfx950)."""

import functools
import math
import os
import subprocess
import sys

import pytest
import torch

import jimm_amd
import jimm_amd.ops.functional as Fn
from jimm_amd import ops
from jimm_amd.ops import _backend
from jimm_amd.ops import philox_dropout as D

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    EXT = _backend.ext()  # fail loudly — never silently skip to eager on a GPU box
else:
    pytest.skip("no GPU", allow_module_level=True)

ACTS = ["gelu", "gelu_tanh", "quickgelu"]
PS = [0.1, 0.5]
K, N = 128, 512
SEED, STEP = 1234, 3
BF16_REL = 2.0 ** -8  # one bf16 rounding, with room for the reference's own


def dev():
    return torch.device("cuda:0")


def rng_of(seed=SEED, step=STEP):
    return torch.tensor([seed, step], dtype=torch.int64, device=dev())


def oracle_mask(rows, cols, p, site, seed=SEED, step=STEP):
    return D.keep_mask(rows, cols, p, seed, step, site).to(dev())


def scale_of(p):
    return D.dropout_scale(D.dropout_threshold(p))


def rel_err(out, ref):
    ref = ref.float()
    return (out.float() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)


# ---------------------------------------------------------------------------
# standalone kernel
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("shape", [(5, 64), (37, 200), (300, 768), (6, 70)], ids=str)
def test_dropout_fwd_matches_oracle(shape, p):
    """(37, 200): odd row count and a ragged last 64-group; (6, 70): columns
    not a multiple of 4, the element-wise path. Inputs lie in [1, 2), so the
    zero pattern is the mask."""
    rows, cols = shape
    g = torch.Generator(device="cuda").manual_seed(rows * 1000 + cols)
    x = (1.0 + torch.rand(rows, cols, device=dev(), generator=g)).bfloat16()
    site = 7
    y = EXT.dropout_fwd(x, p, rng_of(), site)
    mask = oracle_mask(rows, cols, p, site)
    assert y.dtype == torch.bfloat16 and y.shape == x.shape
    assert torch.equal(y != 0, mask)
    ref = x.double() * scale_of(p)
    err = ((y.double() - ref).abs() / ref)[mask].max().item()
    print(f"dropout_fwd {shape} p={p}: kept {mask.float().mean().item():.4f}, max rel err {err:.3e}")
    assert err <= BF16_REL
    # the op: leading dimensions flatten into rows, backward = the same mask
    x3 = x.view(1, rows, cols).clone().requires_grad_(True)
    y3 = ops.dropout(x3, p, rng_of(), site)
    assert torch.equal(y3.detach().view(rows, cols), y)
    (dx,) = torch.autograd.grad(y3, x3, x3.detach())
    assert torch.equal(dx.view(rows, cols), y)


def test_dropout_fwd_arguments():
    x = torch.ones(4, 64, device=dev()).bfloat16()
    assert torch.equal(EXT.dropout_fwd(x, 0.0, None, 0), x)  # zero threshold: no rng needed
    with pytest.raises(RuntimeError):
        EXT.dropout_fwd(x, 0.1, None, 0)
    with pytest.raises(RuntimeError):
        EXT.dropout_fwd(x, 0.1, rng_of().cpu(), 0)
    with pytest.raises(RuntimeError):
        EXT.dropout_fwd(x, 1.0, rng_of(), 0)
    xf = 1.0 + torch.rand(9, 100, device=dev())
    yf = EXT.dropout_fwd(xf, 0.5, rng_of(), 2)
    assert torch.equal(yf, torch.where(oracle_mask(9, 100, 0.5, 2), xf * 2.0, torch.zeros_like(xf)))


# ---------------------------------------------------------------------------
# GEMM epilogues
# ---------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def case(M, act):
    """Inputs and fp64 references of one shape, built once and shared (read
    only): x, w, bias, res, pre64 = x @ w^T + bias, act'(pre64)."""
    g = torch.Generator(device="cuda").manual_seed(1000 * M + N)
    x = torch.randn(M, K, device=dev(), generator=g).bfloat16()
    w = (torch.randn(N, K, device=dev(), generator=g) / math.sqrt(K)).bfloat16()
    bias = torch.randn(N, device=dev(), generator=g).bfloat16()
    res = torch.randn(M, N, device=dev(), generator=g).bfloat16()
    pre = (x.double() @ w.double().t() + bias.double()).requires_grad_(True)
    dact = None
    if act:
        (dact,) = torch.autograd.grad(Fn._act(pre, act).sum(), pre)
    return x, w, bias, res, pre.detach(), dact


def g_tol(p, dact):
    """test_gemm_actgrad_gpu.py's G_TOL scaled by s: half an fp16 ulp at
    max |s * g| (2^-11 in [1, 2), 2^-10 in [2, 4)) plus s * 2e-5 for the fp32
    accumulation of pre and the fast-erf error."""
    s = scale_of(p)
    top = (s * dact).abs().max().item()
    half_ulp = 2.0 ** (math.floor(math.log2(top)) - 11)
    return half_ulp, half_ulp + s * 2e-5


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("act", ACTS)
def test_fc1_reference_fits_fp16(act, p):
    """The bound must be reachable: s * act'(pre64) rounded to fp16 meets it
    by itself (half an ulp, plus 2^-22 where the conversion rounds through
    fp32 below 4), which leaves the s * 2e-5 to the kernel's arithmetic."""
    dact = case(300, act)[5]
    half_ulp, _ = g_tol(p, dact)
    ref = scale_of(p) * dact
    err = (ref.to(torch.float16).double() - ref).abs().max().item()
    assert err <= half_ulp + 2.0 ** -22, (act, p, err)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("M", [256, 100, 300])
def test_fc1_epilogue(M, act, p):
    """f = act(z)*m*s and g = act'(z)*m*s against the oracle mask. Where the
    p = 0 outputs are themselves 0 (act or act' underflowing in bf16 / fp16 at
    a very negative z) a kept element is 0 too: the zero pattern is the
    mask's up to exactly those elements."""
    assert EXT.gemm8p_supported(M, N, K)
    x, w, bias, _, _, dact = case(M, act)
    site = 4
    f0, g0 = EXT.linear_fwd_actgrad(x, w, bias, act, None)
    f, g = EXT.linear_fwd_actgrad(x, w, bias, act, None, p, rng_of(), site)
    mask = oracle_mask(M, N, p, site)
    s = scale_of(p)
    assert f.dtype == torch.bfloat16 and g.dtype == torch.float16
    assert torch.equal(f != 0, mask & (f0 != 0))
    assert torch.equal(g != 0, mask & (g0 != 0))
    assert (f0 != 0).float().mean().item() > 0.999 and (g0 != 0).float().mean().item() > 0.999
    ref_f = s * f0.double()
    err_f = ((f.double() - ref_f).abs() / ref_f.abs().clamp_min(1e-300))[mask & (f0 != 0)].max().item()
    _, tol = g_tol(p, dact)
    err_g = (g.double() - s * dact).abs()[mask].max().item()
    print(f"fc1 M={M} {act} p={p}: f rel {err_f:.3e} (bound {BF16_REL:.3e}), "
          f"g abs {err_g:.3e} (bound {tol:.3e})")
    assert err_f <= BF16_REL
    assert err_g <= tol
    # the epilogue rounds act(z) to bf16 before it scales: exactly the
    # standalone kernel applied to the p = 0 output
    assert torch.equal(f, EXT.dropout_fwd(f0, p, rng_of(), site))


@pytest.mark.parametrize("act", ACTS)
def test_fc1_p_zero_is_the_plain_call(act):
    x, w, bias, _, _, _ = case(300, act)
    f0, g0 = EXT.linear_fwd_actgrad(x, w, bias, act, None)
    f1, g1 = EXT.linear_fwd_actgrad(x, w, bias, act, None, 0.0, rng_of(), 4)
    f2, g2 = EXT.linear_fwd_actgrad(x, w, bias, act, None, 0.0, None, 0)
    assert torch.equal(f0, f1) and torch.equal(g0, g1)
    assert torch.equal(f0, f2) and torch.equal(g0, g2)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("M", [256, 100, 300])
def test_fc2_epilogue(M, p):
    """y = res + m*s*(x @ w^T + bias). Dropped: y is res, bit for bit. Kept:
    one bf16 rounding of res + s * lin64 (relative 2^-8), plus s * 2e-5 for the
    fp32 accumulation (the allowance G_TOL makes for it), which matters only
    where res and s * lin cancel."""
    x, w, bias, res, lin, _ = case(M, "")
    site = 5
    y, none = EXT.linear_fwd(x, w, bias, "", res, False, p, rng_of(), site)
    y0, _ = EXT.linear_fwd(x, w, bias, "", res, False)
    y1, _ = EXT.linear_fwd(x, w, bias, "", res, False, 0.0, rng_of(), site)
    assert none is None and torch.equal(y0, y1)
    mask = oracle_mask(M, N, p, site)
    s = scale_of(p)
    assert torch.equal(y[~mask], res[~mask])
    ref = res.double() + s * lin
    over = ((y.double() - ref).abs() - BF16_REL * ref.abs())[mask].max().item()
    print(f"fc2 M={M} p={p}: max (|err| - 2^-8 |ref|) = {over:.3e} (bound {s * 2e-5:.3e})")
    assert over <= s * 2e-5
    assert not torch.equal(y[mask], res[mask])  # kept elements do carry the GEMM


def test_epilogue_refuses_what_it_cannot_do():
    """p > 0 outside the 8-phase kernel's shapes, or on another epilogue form,
    raises before any launch."""
    x, w, bias, res, _, _ = case(100, "")
    rng = rng_of()
    assert not EXT.gemm8p_supported(100, 384, K)
    with pytest.raises(RuntimeError):
        EXT.linear_fwd(x, w[:384].contiguous(), bias[:384].contiguous(), "", None, False, 0.1, rng, 0)
    with pytest.raises(RuntimeError):  # fc2 form without the residual
        EXT.linear_fwd(x, w, bias, "", None, False, 0.1, rng, 0)
    with pytest.raises(RuntimeError):  # saved pre-activation instead of the derivative
        EXT.linear_fwd(x, w, bias, "gelu", None, True, 0.1, rng, 0)
    with pytest.raises(RuntimeError):  # no rng
        EXT.linear_fwd(x, w, bias, "", res, False, 0.1, None, 0)


# ---------------------------------------------------------------------------
# blocks and models
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("B,L", [(2, 50), (2, 128)], ids=["M100", "M256"])
def test_fused_block_vs_composite_with_dropout(B, L, monkeypatch):
    """Same rng, p = 0.1: the fused Function (masks in the GEMM epilogues)
    against the composite block (ops.dropout), at the thresholds of
    test_fused_block_vs_composite / test_block_save_g_vs_save_z."""
    from jimm_amd.models.common.transformer import EncoderBlock
    from jimm_amd.ops import block as block_mod

    torch.manual_seed(3)
    blk = EncoderBlock(256, 4, 512, dropout_rate=0.1, hidden_act="gelu",
                       layernorm_epsilon=1e-6).to(dev(), torch.bfloat16).train()
    blk.site0 = 6
    x = torch.randn(B, L, 256, device=dev()).bfloat16()
    dy = torch.randn_like(x)
    rng = rng_of(55, 9)
    assert block_mod.fused_block_enabled(x, 0.1, 512)

    calls = []

    def spy(*a, _f=block_mod.encoder_block, **kw):
        calls.append((kw["p"], kw["site0"]))
        return _f(*a, **kw)

    monkeypatch.setattr(block_mod, "encoder_block", spy)

    def run():
        for prm in blk.parameters():
            prm.grad = None
        xi = x.detach().clone().requires_grad_(True)
        y = blk(xi, rng)
        y.backward(dy)
        return y.detach(), xi.grad.clone(), {n: prm.grad.clone() for n, prm in blk.named_parameters()}

    y_f, dx_f, g_f = run()
    assert calls == [(0.1, 6)], calls  # the fused Function really ran
    monkeypatch.setenv("JIMM_AMD_FUSED_BLOCK", "0")
    y_c, dx_c, g_c = run()
    assert calls == [(0.1, 6)], calls  # and the composite block did not use it
    assert len(g_f) == 12
    print(f"block M={B * L}: y {rel_err(y_f, y_c):.3e} dx {rel_err(dx_f, dx_c):.3e} "
          + " ".join(f"{n} {rel_err(g_f[n], g_c[n]):.2e}" for n in g_f))
    assert rel_err(y_f, y_c) < 1e-2, rel_err(y_f, y_c)
    assert rel_err(dx_f, dx_c) < 2e-2, rel_err(dx_f, dx_c)
    for n in g_f:
        assert rel_err(g_f[n], g_c[n]) < 3e-2, (n, rel_err(g_f[n], g_c[n]))
    # dropout is really on: another step gives another output
    assert not torch.equal(blk(x, rng_of(55, 10)), y_f)


def test_checkpointing_replays_masks_bitwise():
    """Same seed and step, checkpointing on and off: loss and every gradient
    bit for bit. The comparison runs in a child process because bitwise
    gradients need JIMM_AMD_DETERMINISTIC=1 (LayerNorm's dW / dB and the fused
    bias gradient otherwise add fp32 atomically, in any order), and the
    extension reads that once per process."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropout_ckpt_child.py")
    env = dict(os.environ, JIMM_AMD_DETERMINISTIC="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-s", child], env=env, capture_output=True, text=True,
                       timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "fused blocks: 4" in r.stdout and "checkpoint: bitwise equal" in r.stdout


def small_vit(dropout_rate):
    torch.manual_seed(5)
    return jimm_amd.VisionTransformer(
        num_classes=10, img_size=64, patch_size=16, num_layers=2, num_heads=4,
        mlp_dim=512, hidden_size=256, dropout_rate=dropout_rate,
    ).to(dev(), torch.bfloat16)


def test_captured_step_advances_masks():
    """hipGraph-captured step of a dropout model (lr = 0, one fixed batch):
    every replay reads the next step from device memory, and putting
    {seed, step} back reproduces a replay's loss bit for bit."""
    from jimm_amd.train import TrainConfig, Trainer

    model = small_vit(0.1).train()
    tr = Trainer(model, TrainConfig(task="vit", lr=0.0, seed=31))
    g = torch.Generator(device="cuda").manual_seed(1)
    batch = (torch.randn(8, 3, 64, 64, device=dev(), generator=g).bfloat16(),
             torch.randint(0, 10, (8,), device=dev(), generator=g))
    tr.enable_graph(batch)
    before = ops.get_dropout_state(dev())
    assert before[0] == 31 and before[1] > 0
    loss1 = tr.train_step(batch)["loss"].clone()
    mid = ops.get_dropout_state(dev())
    assert mid[0] == 31 and mid[1] > before[1]  # the replay advanced the device step
    loss2 = tr.train_step(batch)["loss"].clone()
    assert torch.isfinite(loss1) and torch.isfinite(loss2)
    assert not torch.equal(loss1, loss2)
    ops.set_dropout_state(dev(), *before)
    loss1_again = tr.train_step(batch)["loss"].clone()
    assert torch.equal(loss1_again, loss1)
    assert ops.get_dropout_state(dev()) == mid


def test_eval_of_dropout_model_is_the_dropout_free_model(monkeypatch):
    from jimm_amd.ops import block as block_mod

    drop, plain = small_vit(0.1).eval(), small_vit(0.0).eval()
    plain.load_state_dict(drop.state_dict())
    calls = []

    def spy(*a, _f=block_mod.encoder_block, **kw):
        calls.append(kw["p"])
        return _f(*a, **kw)

    monkeypatch.setattr(block_mod, "encoder_block", spy)
    x = torch.randn(4, 3, 64, 64, device=dev()).bfloat16()
    before = ops.get_dropout_state(dev())
    with torch.no_grad():
        y_drop = drop(x)
        assert calls == [0.0, 0.0], calls  # both layers on the fused block, dropout off
        y_plain = plain(x)
    assert torch.equal(y_drop, y_plain)
    assert ops.get_dropout_state(dev()) == before
