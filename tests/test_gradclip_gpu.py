"""Global-norm gradient clipping on the GPU: the multi-tensor norm kernels, the
clipped / skipping Adam apply, graph replay, and the standalone
clip_grad_norm_. The eager CPU path (tests/test_gradclip_cpu.py) is the oracle.
All require an MI355X (gfx950)."""

import pytest
import torch

import jimm_amd
from jimm_amd.ops import _backend
from jimm_amd.train import Adam, TrainConfig, Trainer, clip_grad_norm_

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    EXT = _backend.ext()  # fail loudly — never silently skip to eager on a GPU box
else:
    pytest.skip("no GPU", allow_module_level=True)

CHUNK = 65536
# the smallest shapes that reach every branch of the chunked kernels:
SHAPES = [
    (),          # 1 element: tail only
    (3,),        # < 4 elements: tail only
    (1027,),     # vector body + tail of 3
    (65536,),    # exactly one chunk
    (65537,),    # crosses a chunk boundary; tail-only second chunk
    (256, 513),  # several chunks, ragged last one
]
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)

# Norm tolerance, from the kernel's summation order (csrc/adam.hip): a thread
# adds at most CHUNK / 256 threads = 256 squares in sequence, the wave butterfly
# is 6 levels deep, 3 more adds join the 4 waves; each square rounds once. That
# is under (256 + 10) * 2^-24 ~ 1.6e-5 relative on a chunk's sum of squares,
# the sqrt halves it, and the sum over chunks is fp64: 2e-5 on the norm.
NORM_TOL = 2e-5


def dev():
    return torch.device("cuda:0")


def rel_err(out, ref):
    # no absolute floor: a clipped v is of the order 1e-8 and must still be
    # measured against its own size
    ref = ref.float()
    return (out.float().cpu() - ref.cpu()).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def _mixed_grads(seed=0, scale=1.0):
    """Every shape once in fp32 and once in bf16, interleaved."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in SHAPES:
        for dt in (torch.float32, torch.bfloat16):
            out.append((torch.randn(s, generator=g) * scale).to(dt).to(dev()))
    return out


def _norm64(gs):
    """fp64 norm of the values as stored (i.e. after their bf16 rounding)."""
    return torch.sqrt(sum((g.double() ** 2).sum() for g in gs)).item()


def _device_norm(gs, max_norm):
    desc, nchunks = EXT.grad_desc_prepare(gs)
    n = int(nchunks.item())
    assert n == sum((g.numel() + CHUNK - 1) // CHUNK for g in gs)
    partials = torch.zeros(n, device=dev())
    stats = torch.zeros(4, device=dev())
    EXT.grad_sqnorm(desc, n, partials, 0)
    EXT.clip_finalize(partials, stats, max_norm)
    return stats, partials


def test_norm_kernel_shapes():
    gs = _mixed_grads()
    ref = _norm64(gs)
    stats, partials = _device_norm(gs, 1.0)
    norm, coef, finite, skipped = stats.tolist()
    print("norm", norm, "ref", ref, "rel", abs(norm - ref) / ref)
    assert abs(norm - ref) / ref < NORM_TOL
    assert abs(coef - min(1.0, 1.0 / (ref + 1e-6))) / coef < 2 * NORM_TOL
    assert finite == 1.0 and skipped == 0.0
    # one partial per chunk, indexed by chunk number: the first tensor is the
    # 0-d fp32 one, its single chunk holds its square
    assert abs(partials[0].item() - gs[0].item() ** 2) <= 1e-6 * gs[0].item() ** 2
    # no clip when the norm is under the bound
    stats, _ = _device_norm(gs, 2.0 * ref)
    assert stats[1].item() == 1.0


def test_norm_is_deterministic():
    gs = _mixed_grads(seed=3)
    a, pa = _device_norm(gs, 1.0)
    b, pb = _device_norm(gs, 1.0)
    assert torch.equal(a, b) and torch.equal(pa, pb)


# ---------------------------------------------------------------------------
def _make(pdtype, seed=1):
    g = torch.Generator().manual_seed(seed)
    vals = [torch.randn(s, generator=g).to(pdtype) for s in SHAPES]
    ps = [v.to(dev()).requires_grad_(True) for v in vals]
    ps_o = [v.float().clone().requires_grad_(True) for v in vals]  # CPU fp32 oracle copies
    return ps, ps_o


def _groups(ps):
    return [{"params": ps[:3]}, {"params": ps[3:]}]


def _give(ps, ps_o, seed, scale, pdtype, poison=None):
    g = torch.Generator().manual_seed(seed)
    for i, (p, po) in enumerate(zip(ps, ps_o)):
        val = (torch.randn(p.shape, generator=g) * scale).to(pdtype)
        if poison is not None and i == 3:
            val.view(-1)[17] = poison
        if p.grad is None:
            p.grad = val.to(dev())
        else:
            p.grad.copy_(val)  # static gradient buffers (descriptors, graphs)
        po.grad = val.float()


def _check_state(opt, ps, oracle, ps_o, pdtype):
    tol = 1e-6 if pdtype == torch.float32 else 1e-2
    for p, po in zip(ps, ps_o):
        st, so = opt.state[p], oracle.state[po]
        errs = rel_err(p, po), rel_err(st["m"], so["m"]), rel_err(st["v"], so["v"])
        print(tuple(p.shape), "p/m/v rel err", errs)
        assert errs[0] < tol and errs[1] < tol and errs[2] < tol, errs
        # a clip that was silently dropped would miss m by 1/coef
        assert errs[1] < 1e-5, errs
        if pdtype != torch.float32:
            assert rel_err(st["master"], po) < 1e-6


@pytest.mark.parametrize("pdtype", [torch.float32, torch.bfloat16])
def test_clipped_adam_matches_cpu_oracle(pdtype):
    c = 1.0
    ps, ps_o = _make(pdtype)
    opt = Adam(_groups(ps), max_grad_norm=c, **HP)
    oracle = Adam(_groups(ps_o), max_grad_norm=c, **HP)
    clipped = []
    # randn over 263432 elements has norm ~513 * scale
    for step, scale in enumerate([1.0, 1e-4, 0.01]):
        _give(ps, ps_o, 10 + step, scale, pdtype)
        opt.step()
        oracle.step()
        n, no = opt.last_grad_norm.item(), oracle.last_grad_norm.item()
        assert abs(n - no) / no < NORM_TOL, (n, no)
        clipped.append(no > c)
    assert clipped == [True, False, True]
    assert opt.skipped_steps() == 0
    opt.sync_step_from_device()
    assert all(opt.state[p]["step"] == 3 for p in ps)
    _check_state(opt, ps, oracle, ps_o, pdtype)
    if pdtype != torch.float32:
        assert all("master" in opt.state[p] for p in ps)


def test_nonfinite_norm_skips_on_device():
    pdtype = torch.bfloat16  # with masters
    ps, ps_o = _make(pdtype)
    opt = Adam(_groups(ps), max_grad_norm=1.0, **HP)
    oracle = Adam(_groups(ps_o), max_grad_norm=1.0, **HP)  # never sees the bad step
    _give(ps, ps_o, 20, 1.0, pdtype)
    opt.step()
    oracle.step()

    def snapshot():
        out = []
        for p in ps:
            st = opt.state[p]
            out += [p.detach().clone(), st["m"].clone(), st["v"].clone(), st["master"].clone()]
        return out + [prep[3].clone() for prep in opt._prepared.values()]

    before = snapshot()
    _give(ps, [q.detach().clone().requires_grad_(True) for q in ps_o], 21, 1.0, pdtype,
          poison=float("inf"))
    opt.step()
    assert opt.skipped_steps() == 1
    assert not torch.isfinite(opt.last_grad_norm).item()
    for a, b in zip(before, snapshot()):
        assert torch.equal(a, b)
    assert all(prep[3].item() == 1 for prep in opt._prepared.values())

    _give(ps, ps_o, 22, 1e-4, pdtype)
    opt.step()
    oracle.step()
    assert opt.skipped_steps() == 1
    assert all(prep[3].item() == 2 for prep in opt._prepared.values())
    _check_state(opt, ps, oracle, ps_o, pdtype)


def test_graph_replay_reads_clip_state_on_device():
    """opt.step() captured once; coef and the finite flag must come from device
    memory at replay time, not from the capture."""
    pdtype = torch.float32
    c = 1.0
    ps, ps_o = _make(pdtype)
    opt = Adam(_groups(ps), max_grad_norm=c, **HP)
    oracle = Adam(_groups(ps_o), max_grad_norm=c, **HP)
    # one eager step on a side stream: lazy state, descriptor tables
    _give(ps, ps_o, 30, 1.0, pdtype)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()
    torch.cuda.current_stream().wait_stream(side)
    oracle.step()
    snap = [p.detach().clone() for p in ps]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        opt.step()
    torch.cuda.synchronize()
    for p, s in zip(ps, snap):
        assert torch.equal(p, s)  # capture itself runs nothing

    norms = []
    seq = [(31, 1e-4, None), (32, 0.01, None), (33, 1.0, float("nan")), (34, 1e-4, None)]
    for seed, scale, poison in seq:
        _give(ps, ps_o, seed, scale, pdtype, poison=poison)
        g.replay()
        oracle.step()
        norms.append(opt.last_grad_norm.item())
    assert norms[0] < c < norms[1]  # a replay that clips and one that does not
    assert norms[2] != norms[2]  # NaN
    assert opt.skipped_steps() == 1 and oracle.skipped_steps() == 1
    opt.sync_step_from_device()
    assert all(opt.state[p]["step"] == 4 for p in ps)
    assert all(oracle.state[p]["step"] == 4 for p in ps_o)
    _check_state(opt, ps, oracle, ps_o, pdtype)


# ---------------------------------------------------------------------------
def _bf16_ulp(ref):
    """Spacing of bf16 (8 significand bits) at the magnitude of ``ref``."""
    _, e = torch.frexp(ref.float().abs())  # |ref| = m * 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(ref, dtype=torch.float32), e - 8)


def test_clip_grad_norm_matches_torch():
    """torch.nn.utils.clip_grad_norm_ is the reference. It rounds each bf16
    tensor's norm to bf16 (about 1e-3 off) before combining them, so the norm is
    compared with torch's result on an fp32 clone of the same values; the
    scaled bf16 gradients are compared with both of torch's results."""
    max_norm = 1.0
    gs = _mixed_grads(seed=5, scale=0.01)
    ours = [torch.zeros_like(g).requires_grad_(True) for g in gs]
    t32 = [torch.zeros_like(g, dtype=torch.float32).requires_grad_(True) for g in gs]
    tnat = [torch.zeros_like(g).requires_grad_(True) for g in gs]
    for p, a, b, g in zip(ours, t32, tnat, gs):
        p.grad, a.grad, b.grad = g.clone(), g.float().clone(), g.clone()
    norm = clip_grad_norm_(ours, max_norm)
    norm_t = torch.nn.utils.clip_grad_norm_(t32, max_norm)
    torch.nn.utils.clip_grad_norm_(tnat, max_norm)
    assert norm.shape == () and norm.is_cuda and norm.dtype == torch.float32
    print("norm", norm.item(), "torch", norm_t.item())
    assert norm_t.item() > max_norm  # it did clip
    assert abs(norm.item() - norm_t.item()) / norm_t.item() < NORM_TOL
    for p, a, b in zip(ours, t32, tnat):
        if p.dtype == torch.float32:
            assert rel_err(p.grad, a.grad) < 1e-6
        else:
            for ref in (a.grad, b.grad.float()):
                # the ulp of the larger of the two, so that a pair straddling a
                # power of two is still measured in one unit
                ulp = _bf16_ulp(torch.maximum(ref.abs(), p.grad.float().abs()))
                assert ((p.grad.float() - ref).abs() <= ulp).all()
    # under the bound nothing is rewritten
    keep = [p.grad.clone() for p in ours]
    clip_grad_norm_(ours, 10.0)
    for p, k in zip(ours, keep):
        assert torch.equal(p.grad, k)


def test_trainer_grad_norm_live_under_graph():
    from jimm_amd.train import SyntheticImages

    torch.manual_seed(7)
    m = jimm_amd.VisionTransformer(num_classes=10, img_size=64, patch_size=16,
                                   num_layers=2, num_heads=2, mlp_dim=256,
                                   hidden_size=128).to(dev(), torch.bfloat16)
    tr = Trainer(m, TrainConfig(task="vit", lr=1e-3, max_grad_norm=0.05))
    it = iter(SyntheticImages(8, 64, 10, dev(), dtype=torch.bfloat16, seed=5))
    batches = [next(it) for _ in range(5)]
    tr.enable_graph(batches[0])
    norms = []
    for b in batches[1:]:
        out = tr.train_step(b)
        assert out["grad_norm"].is_cuda and out["grad_norm"].shape == ()
        norms.append(out["grad_norm"].item())
    print("grad norms", norms)
    assert all(n == n and 0.0 < n < float("inf") for n in norms)
    assert len(set(norms)) > 1  # live, not a stale captured value
    assert tr.opt.skipped_steps() == 0
    assert all(torch.isfinite(p).all() for p in m.parameters())
