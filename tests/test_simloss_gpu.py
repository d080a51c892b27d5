"""The fused similarity-loss head on the GPU (csrc/simloss.hip, ops/losses.py
fused=True): the three kernels, the two public losses end to end, determinism,
the engines the backward GEMMs land on, peak memory, and graph capture.

Oracle: fp64 torch on the same bf16-rounded, L2-normalized operands,
x = s * (a @ b^T) (+ bias), then cross_entropy or the sigmoid sum.

Tolerances (eps(s, D) = s * D * 2^-24: fp32 accumulation of D products whose
absolute sum is at most about 1, times the scale):
  lse, pos, loss   2 * eps + 1e-4   (lse is 1-Lipschitz in the logits; 1e-4 is
                   what test_xent_rows_kernel allows the same __expf / __logf)
  sigmoid sum      M * N * (eps + 1e-6), on the sum itself
  G                1 bf16 ulp of the larger magnitude, against the bf16
                   rounding of the oracle's value
  dscale, dbias    softmax: 2 * g * (eps + 2^-20), as sum_j |r_ij acc_ij| <= 2
                   per row; sigmoid: (eps + 2^-20) * sum |r_ij| of the oracle
  dA, dB           max-normalized error < 1e-2 (test_contrastive_losses_gpu_vs_cpu)
All require an MI355X (gfx950)."""

import math

import pytest
import torch
import torch.nn.functional as F

import jimm_amd
from jimm_amd.ops import _backend
from jimm_amd.ops import losses as L

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    EXT = _backend.ext()  # fail loudly — never silently skip to eager on a GPU box
else:
    pytest.skip("no GPU", allow_module_level=True)

# (M, N, D, diag0): the smallest shapes that reach every branch
SHAPES = [
    (128, 128, 64, 0),    # one fast tile, nk = 1
    (256, 384, 128, 0),   # several fast tiles, both LDS buffers
    (130, 200, 192, 0),   # guarded form, ragged rows and columns across a tile edge, odd nk
    (70, 130, 64, 0),     # a fully masked 64-column group
    (8, 8, 64, 0),        # one partly filled tile
    (64, 256, 128, 128),  # positives away from the main diagonal
]
SCALES = [14.2857, 100.0]  # CLIP init; an unshifted exp overflows at 100
BIASES = [-10.0, 0.5]      # SigLIP init; a positive one
COEF = 0.37                # upstream coefficient of the kernel-level sim_grad cases


def dev():
    return torch.device("cuda:0")


def rel_err(out, ref):
    ref = ref.float()
    return (out.float() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)


def eps(s, D):
    return s * D * 2.0 ** -24


def scalar(v):
    return torch.tensor([v], device=dev(), dtype=torch.float32)


_OPERANDS = {}


def operands(M, N, D):
    """bf16 L2-normalized (a, b), made once per shape and never written to."""
    if (M, N, D) not in _OPERANDS:
        g = torch.Generator().manual_seed(1000 * M + N + D)
        a = F.normalize(torch.randn(M, D, generator=g), dim=-1).bfloat16().to(dev())
        b = F.normalize(torch.randn(N, D, generator=g), dim=-1).bfloat16().to(dev())
        _OPERANDS[(M, N, D)] = (a, b)
    return _OPERANDS[(M, N, D)]


def oracle_logits(a, b, s, bias=0.0):
    return s * (a.double() @ b.double().t()) + bias


def label_mask(M, N, diag0):
    z = torch.full((M, N), -1.0, device=dev(), dtype=torch.float64)
    rows = torch.arange(M, device=dev())
    col = rows + diag0
    own = (col >= 0) & (col < N)
    z[rows[own], col[own]] = 1.0
    return z


def bf16_ulp(v):
    """Spacing of bf16 at |v| (8 significant bits), and no less than 2^-126:
    the hardware exp flushes fp32 subnormals to zero, so a value of that size
    is only known to within the smallest normal number."""
    mag = v.abs().double().clamp_min(2.0 ** -119)
    return torch.exp2(torch.floor(torch.log2(mag)) - 7)


# --- kernel level ----------------------------------------------------------------


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("M,N,D,diag0", SHAPES)
def test_sim_lse_fwd(M, N, D, diag0, s):
    a, b = operands(M, N, D)
    lse, pos = EXT.sim_lse_fwd(a, b, scalar(s), diag0)
    x = oracle_logits(a, b, s)
    lse_ref = torch.logsumexp(x, dim=1)
    rows = torch.arange(M, device=dev())
    pos_ref = x[rows, rows + diag0]
    tol = 2 * eps(s, D) + 1e-4
    e_lse = (lse.double() - lse_ref).abs().max().item()
    e_pos = (pos.double() - pos_ref).abs().max().item()
    print(f"lse err {e_lse:.3e} pos err {e_pos:.3e} tol {tol:.3e}")
    assert torch.isfinite(lse).all() and torch.isfinite(pos).all()
    assert e_lse <= tol and e_pos <= tol, (e_lse, e_pos, tol)
    loss_ref = F.cross_entropy(x, torch.arange(M, device=dev()) + diag0).item()
    assert abs((lse - pos).double().mean().item() - loss_ref) <= tol


@pytest.mark.parametrize("bias", BIASES)
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("M,N,D,diag0", SHAPES)
def test_sim_sigmoid_fwd(M, N, D, diag0, s, bias):
    a, b = operands(M, N, D)
    out = EXT.sim_sigmoid_fwd(a, b, scalar(s), scalar(bias), diag0)
    x = oracle_logits(a, b, s, bias)
    ref = -F.logsigmoid(label_mask(M, N, diag0) * x).sum().item()
    tol = M * N * (eps(s, D) + 1e-6)
    err = abs(out.item() - ref)
    print(f"sigmoid sum {out.item():.6f} ref {ref:.6f} err {err:.3e} tol {tol:.3e}")
    assert out.shape == (1,) and err <= tol, (err, tol)


def _check_sim_grad(mode, M, N, D, diag0, s, bias):
    a, b = operands(M, N, D)
    x = oracle_logits(a, b, s, 0.0 if bias is None else bias)
    acc = a.double() @ b.double().t()
    if mode == 0:
        lse = torch.logsumexp(x, dim=1)
        r = torch.exp(x - lse[:, None]) - (label_mask(M, N, diag0) > 0).double()
        G, ds, db = EXT.sim_grad(a, b, scalar(s), None, lse.float(), scalar(COEF), diag0, 0)
        tol = 2 * COEF * M * (eps(s, D) + 2.0 ** -20)
    else:
        z = label_mask(M, N, diag0)
        r = -z * torch.sigmoid(-z * x)
        G, ds, db = EXT.sim_grad(a, b, scalar(s), scalar(bias), None, scalar(COEF), diag0, 1)
        tol = COEF * (eps(s, D) + 2.0 ** -20) * r.abs().sum().item()
    assert G.shape == (M, N) and G.dtype == torch.bfloat16 and G.is_contiguous()
    G_ref = (COEF * s * r).float().bfloat16()
    ulp = torch.maximum(bf16_ulp(G), bf16_ulp(G_ref))
    worst = ((G.double() - G_ref.double()).abs() / ulp).max().item()
    e_ds = abs(ds.item() - COEF * (r * acc).sum().item())
    e_db = abs(db.item() - COEF * r.sum().item())
    print(f"G worst {worst:.2f} ulp, dscale err {e_ds:.3e} dbias err {e_db:.3e} tol {tol:.3e}")
    assert worst <= 1.0, worst
    assert e_ds <= tol and e_db <= tol, (e_ds, e_db, tol)


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("M,N,D,diag0", SHAPES)
def test_sim_grad_softmax(M, N, D, diag0, s):
    _check_sim_grad(0, M, N, D, diag0, s, None)


@pytest.mark.parametrize("bias", BIASES)
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("M,N,D,diag0", SHAPES)
def test_sim_grad_sigmoid(M, N, D, diag0, s, bias):
    _check_sim_grad(1, M, N, D, diag0, s, bias)


def test_sim_grad_chunk_diagonal_outside():
    """diag0 relative to a chunk: negative (labels left of it) and past it."""
    M, N, D = 64, 256, 128
    for diag0 in (-128, 256):
        _check_sim_grad(1, M, N, D, diag0, 14.2857, -10.0)


def test_sim_supported():
    assert EXT.sim_supported(8, 8, 64, "torch.bfloat16")
    assert EXT.sim_supported(130, 200, 192, "torch.bfloat16")
    assert not EXT.sim_supported(8, 8, 32, "torch.bfloat16")
    assert not EXT.sim_supported(8, 8, 64, "torch.float32")


# --- end to end ------------------------------------------------------------------


def _raw_inputs(B, D, seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(B, D, generator=g).bfloat16().to(dev())
    txt = torch.randn(B, D, generator=g).bfloat16().to(dev())
    return img, txt


def _oracle_embed(raw):
    """fp64 leaf of the raw embedding and its normalized value as the loss head
    sees it: forward the bf16 output of the l2norm kernel, backward the fp64
    normalize (straight-through on the rounding)."""
    leaf = raw.double().requires_grad_(True)
    y = leaf / leaf.norm(dim=-1, keepdim=True)
    seen = L.l2norm(raw).double()
    return leaf, y + (seen - y).detach()


def _run_fused(task, raw_img, raw_txt, ls, lb, chunk):
    img = raw_img.clone().requires_grad_(True)
    txt = raw_txt.clone().requires_grad_(True)
    logit_scale = torch.tensor(ls, device=dev(), requires_grad=True)
    logit_bias = torch.tensor(lb, device=dev(), requires_grad=True)
    if task == "clip":
        loss = L.clip_contrastive_loss(img, txt, logit_scale, gather=False, fused=True,
                                       chunk_size=chunk)
    else:
        loss = L.siglip_sigmoid_loss(img, txt, logit_scale, logit_bias, gather=False, fused=True,
                                     chunk_size=chunk)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), img.grad, txt.grad, logit_scale.grad, logit_bias.grad


@pytest.mark.parametrize("chunk", [128, 1 << 20])
@pytest.mark.parametrize("B", [384, 200])  # aligned chunks; a last chunk of 72 columns
@pytest.mark.parametrize("s", SCALES)
def test_clip_loss_fused_vs_oracle(s, B, chunk):
    D = 128
    raw_img, raw_txt = _raw_inputs(B, D, 7)
    ls = math.log(s)
    loss, dimg, dtxt, dls, _ = _run_fused("clip", raw_img, raw_txt, ls, 0.0, chunk)

    img64, a = _oracle_embed(raw_img)
    txt64, b = _oracle_embed(raw_txt)
    ls64 = torch.tensor(ls, device=dev(), dtype=torch.float64, requires_grad=True)
    x = ls64.exp() * (a @ b.t())
    labels = torch.arange(B, device=dev())
    ref = 0.5 * (F.cross_entropy(x, labels) + F.cross_entropy(x.t(), labels))
    ref.backward()

    tol = 2 * eps(s, D) + 1e-4
    # two directions of weight g = 0.5 each; d/dlogit_scale = s * d/dscale
    tol_ls = s * 2 * (0.5 + 0.5) * (eps(s, D) + 2.0 ** -20)
    e_loss = abs(loss.item() - ref.item())
    e_ls = abs(dls.item() - ls64.grad.item())
    print(f"loss err {e_loss:.3e} (tol {tol:.3e}) dlogit_scale err {e_ls:.3e} (tol {tol_ls:.3e}) "
          f"dimg {rel_err(dimg, img64.grad):.3e} dtxt {rel_err(dtxt, txt64.grad):.3e}")
    assert e_loss <= tol, (e_loss, tol)
    assert e_ls <= tol_ls, (e_ls, tol_ls)
    assert rel_err(dimg, img64.grad) < 1e-2
    assert rel_err(dtxt, txt64.grad) < 1e-2


@pytest.mark.parametrize("chunk", [128, 1 << 20])
@pytest.mark.parametrize("B", [384, 200])
@pytest.mark.parametrize("s,bias", [(14.2857, -10.0), (100.0, 0.5)])
def test_siglip_loss_fused_vs_oracle(s, bias, B, chunk):
    D = 128
    raw_img, raw_txt = _raw_inputs(B, D, 11)
    ls = math.log(s)
    loss, dimg, dtxt, dls, dlb = _run_fused("siglip", raw_img, raw_txt, ls, bias, chunk)

    img64, a = _oracle_embed(raw_img)
    txt64, b = _oracle_embed(raw_txt)
    ls64 = torch.tensor(ls, device=dev(), dtype=torch.float64, requires_grad=True)
    lb64 = torch.tensor(bias, device=dev(), dtype=torch.float64, requires_grad=True)
    x = ls64.exp() * (a @ b.t()) + lb64
    z = label_mask(B, B, 0)
    ref = -F.logsigmoid(z * x).sum() / B
    ref.backward()
    r_abs = torch.sigmoid(-z * x.detach()).sum().item()  # sum |r_ij|

    tol = B * B * (eps(s, D) + 1e-6) / B
    tol_b = (eps(s, D) + 2.0 ** -20) * r_abs / B
    e_loss = abs(loss.item() - ref.item())
    e_ls = abs(dls.item() - ls64.grad.item())
    e_lb = abs(dlb.item() - lb64.grad.item())
    print(f"loss err {e_loss:.3e} (tol {tol:.3e}) dlogit_scale err {e_ls:.3e} (tol {s * tol_b:.3e}) "
          f"dlogit_bias err {e_lb:.3e} (tol {tol_b:.3e}) "
          f"dimg {rel_err(dimg, img64.grad):.3e} dtxt {rel_err(dtxt, txt64.grad):.3e}")
    assert e_loss <= tol, (e_loss, tol)
    assert e_ls <= s * tol_b, (e_ls, s * tol_b)
    assert e_lb <= tol_b, (e_lb, tol_b)
    assert rel_err(dimg, img64.grad) < 1e-2
    assert rel_err(dtxt, txt64.grad) < 1e-2


@pytest.mark.parametrize("task", ["clip", "siglip"])
def test_fused_loss_deterministic(task):
    raw_img, raw_txt = _raw_inputs(200, 128, 3)
    first = _run_fused(task, raw_img, raw_txt, math.log(100.0), -10.0, 128)
    second = _run_fused(task, raw_img, raw_txt, math.log(100.0), -10.0, 128)
    for u, v in zip(first, second):
        if u is not None:
            assert torch.equal(u, v)


# --- routes ----------------------------------------------------------------------


@pytest.fixture
def trace(monkeypatch):
    """The names of the extension / torch GEMM calls, in call order
    (tests/test_gemm_routes_gpu.py)."""
    for name in ("JIMM_AMD_GEMM", "JIMM_AMD_DETERMINISTIC"):
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


_CHUNK_BWD = ["sim_grad", "linear_fwd", "gemm_tn_8p"]
# what one rank of four sees: 128 local rows against 512 gathered columns
FUNCTION_128_512 = ["sim_lse_fwd"] + 2 * _CHUNK_BWD
# the public loss at world size 1 (N == M = 512), two directions, two chunks each
CLIP_FUSED_512 = (["l2norm_fwd", "l2norm_fwd", "sim_lse_fwd", "sim_lse_fwd"] + 4 * _CHUNK_BWD
                  + ["l2norm_bwd", "l2norm_bwd"])
# fused=False, recorded from the commit before the fused head: the logit GEMMs
# are Tensor.__matmul__ and its autograd, which the spies do not see
CLIP_UNFUSED_512 = ["l2norm_fwd", "l2norm_fwd", "xent_rows_fwd", "xent_rows_fwd",
                    "xent_rows_bwd", "xent_rows_bwd", "l2norm_bwd", "l2norm_bwd"]


def test_route_function_one_rank_of_four(trace):
    """(M, N, D) = (128, 512, 256), chunk_size 256: a world-1 CLIP loss has
    N == M, so the shape goes through the Function, as a rank of four calls it."""
    a, b = operands(128, 512, 256)
    a = a.clone().requires_grad_(True)
    b = b.clone().requires_grad_(True)
    scale = torch.tensor(100.0, device=dev(), requires_grad=True)
    trace.clear()
    L.fused_similarity_loss(a, b, scale, None, 128, "softmax", 256).backward()
    torch.cuda.synchronize()
    print(f"trace: {trace!r}")
    assert trace == FUNCTION_128_512, f"recorded trace: {trace!r}"


@pytest.mark.parametrize("fused,expected", [(True, CLIP_FUSED_512), (False, CLIP_UNFUSED_512)])
def test_route_clip_loss(trace, fused, expected):
    raw_img, raw_txt = _raw_inputs(512, 256, 5)
    img = raw_img.clone().requires_grad_(True)
    txt = raw_txt.clone().requires_grad_(True)
    logit_scale = torch.tensor(math.log(14.2857), device=dev(), requires_grad=True)
    trace.clear()
    kw = dict(fused=True, chunk_size=256) if fused else {}
    L.clip_contrastive_loss(img, txt, logit_scale, gather=False, **kw).backward()
    torch.cuda.synchronize()
    print(f"trace: {trace!r}")
    assert trace == expected, f"recorded trace: {trace!r}"
    assert not fused or not any(c in trace for c in ("torch.matmul", "torch.addmm"))


# --- memory ----------------------------------------------------------------------


def test_fused_head_peak_memory():
    """(M, N, D) = (512, 4096, 128), chunk_size 512: forward + backward of the
    fused head stays below one fp32 logit matrix (M * N * 4 = 8 MiB; it holds
    about 0.5 MB of G, 0.25 MB of partials and 3 MB of dB, the transposed chunk
    and dA32); the unfused expression of one direction does not."""
    M, N, D = 512, 4096, 128
    bound = M * N * 4
    a0, b0 = operands(M, N, D)
    scale = torch.tensor(14.2857, device=dev())

    def peak(fn):
        a = a0.clone().requires_grad_(True)
        b = b0.clone().requires_grad_(True)
        fn(a, b).backward()  # warm-up: kernels loaded, workspaces of the libraries made
        a.grad = b.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn(a, b).backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before

    fused = peak(lambda a, b: L.fused_similarity_loss(a, b, scale, None, 0, "softmax", 512))
    labels = torch.arange(M, device=dev())
    unfused = peak(lambda a, b: L.softmax_cross_entropy(scale * a @ b.t(), labels))
    print(f"peak increase: fused {fused} B, unfused {unfused} B, bound {bound} B")
    assert fused < bound, (fused, bound)
    assert unfused > bound, (unfused, bound)


# --- graph capture -----------------------------------------------------------------


def test_fused_head_graph_capture():
    """A captured CLIP step with the fused head against the eager one, at the
    tolerance of test_graph_captured_training (the warm-up and capture steps
    train on the example batch, so the two trajectories differ slightly)."""
    from jimm_amd.train import SyntheticImageText, TrainConfig, Trainer

    def run(graph):
        torch.manual_seed(7)
        m = jimm_amd.CLIP(embed_dim=64, image_resolution=64, vision_layers=2, vision_width=128,
                          vision_patch_size=32, context_length=12, vocab_size=99,
                          transformer_width=64, transformer_heads=1,
                          transformer_layers=2).to(dev(), torch.bfloat16)
        tr = Trainer(m, TrainConfig(task="clip", lr=1e-4, fused_loss_head=True))
        data = SyntheticImageText(8, 64, 12, 99, dev(), dtype=torch.bfloat16, seed=5)
        it = iter(data)
        batches = [next(it) for _ in range(5)]
        if graph:
            tr.enable_graph(batches[0])
        losses = [tr.train_step(b)["loss"].float().clone() for b in batches[1:]]
        torch.cuda.synchronize()
        return [l.item() for l in losses]

    eager = run(False)
    graphed = run(True)
    print(f"eager {eager} graphed {graphed}")
    for p, q in zip(eager, graphed):
        assert math.isfinite(q)
        assert abs(p - q) < 0.2, (p, q)
