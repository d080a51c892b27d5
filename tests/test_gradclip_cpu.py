"""Global-norm gradient clipping in the Adam step — CPU oracle tests.

The eager path of ``Adam(max_grad_norm=c)`` is the numerics oracle for the HIP
kernels, so it is checked here against torch's own
``clip_grad_norm_`` + ``AdamW``."""

import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import jimm_amd
from jimm_amd.train import Adam, TrainConfig, Trainer, clip_grad_norm_

HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
SHAPES = [(7,), (33, 5), (64,), (16, 16)]  # first two -> group 0, rest -> group 1


def rel_err(out, ref):
    ref = ref.float()
    return (out.float() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).requires_grad_(True) for s in SHAPES]


def _groups(ps):
    return [{"params": ps[:2]}, {"params": ps[2:], "lr": 3e-3}]


def _grads(step, scale):
    g = torch.Generator().manual_seed(100 + step)
    return [torch.randn(s, generator=g) * scale for s in SHAPES]


def test_matches_torch_clip_then_adamw():
    """Five steps, two param groups, decoupled decay: Adam(max_grad_norm=c) ==
    clip_grad_norm_(params, c) followed by AdamW, to fp32 rounding."""
    c = 1.0
    ps, ps_t = _params(), _params()
    opt = Adam(_groups(ps), max_grad_norm=c, **HP)
    opt_t = torch.optim.AdamW(_groups(ps_t), **HP)
    # randn grads over 332 elements have norm ~18 * scale
    scales = [1.0, 0.01, 0.5, 0.02, 2.0]
    clipped = []
    for step, scale in enumerate(scales):
        for p, pt, g in zip(ps, ps_t, _grads(step, scale)):
            p.grad, pt.grad = g.clone(), g.clone()
        norm_t = torch.nn.utils.clip_grad_norm_(ps_t, c)
        opt_t.step()
        opt.step()
        clipped.append(norm_t.item() > c)
        assert opt.last_grad_norm.shape == () and opt.last_grad_norm.dtype == torch.float32
        assert abs(opt.last_grad_norm.item() - norm_t.item()) <= 1e-6 * norm_t.item()
        # the Adam path never rewrites the gradients
        for p, g in zip(ps, _grads(step, scale)):
            assert torch.equal(p.grad, g)
    assert any(clipped) and not all(clipped), clipped
    for p, pt in zip(ps, ps_t):
        assert rel_err(p, pt) < 1e-6, rel_err(p, pt)
    assert opt.skipped_steps() == 0


def test_norm_is_global_across_groups():
    """A large gradient in group 0 scales the small one in group 1 by the same coef."""
    big = torch.zeros(8, requires_grad=True)
    small = torch.zeros(8, requires_grad=True)
    big.grad = torch.full((8,), 100.0)
    small.grad = torch.full((8,), 1e-3)
    hp = dict(HP, weight_decay=0.0)
    opt = Adam([{"params": [big]}, {"params": [small]}], max_grad_norm=1.0, **hp)
    opt.step()
    norm = (8 * 100.0**2 + 8 * 1e-3**2) ** 0.5
    coef = 1.0 / (norm + 1e-6)
    assert abs(opt.last_grad_norm.item() - norm) < 1e-6 * norm
    # m after step 1 is (1 - b1) * coef * g: shows which coef reached group 1
    m_small = opt.state[small]["m"]
    expect = 0.1 * coef * 1e-3
    assert rel_err(m_small, torch.full((8,), expect)) < 1e-5
    # alone, the small gradient (norm 2.8e-3) would not have been clipped at all
    assert expect < 0.1 * 1e-3 / 100


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_nonfinite_norm_skips_the_step(bad):
    ps, ps_o = _params(), _params()
    opt = Adam(_groups(ps), max_grad_norm=1.0, **HP)
    oracle = Adam(_groups(ps_o), max_grad_norm=1.0, **HP)  # never sees the bad step

    def give(params, step, scale=1.0):
        for p, g in zip(params, _grads(step, scale)):
            p.grad = g.clone()

    give(ps, 0), give(ps_o, 0)
    opt.step(), oracle.step()
    before = [(p.detach().clone(), opt.state[p]["m"].clone(), opt.state[p]["v"].clone(),
               opt.state[p]["step"]) for p in ps]
    give(ps, 1)
    ps[2].grad[5] = bad  # one element, in the second group
    opt.step()
    assert opt.skipped_steps() == 1
    assert not torch.isfinite(opt.last_grad_norm)
    for p, (p0, m0, v0, s0) in zip(ps, before):
        st = opt.state[p]
        assert torch.equal(p, p0) and torch.equal(st["m"], m0) and torch.equal(st["v"], v0)
        assert st["step"] == s0 == 1
    # next finite step: bias correction uses the unskipped count (2, not 3)
    give(ps, 2, 0.01), give(ps_o, 2, 0.01)
    opt.step(), oracle.step()
    for p, po in zip(ps, ps_o):
        assert torch.equal(p, po)
        assert opt.state[p]["step"] == oracle.state[po]["step"] == 2
    assert opt.skipped_steps() == 1 and oracle.skipped_steps() == 0


def test_clip_grad_norm_cpu_matches_torch():
    ps, ps_t = _params(), _params()
    for p, pt, g in zip(ps, ps_t, _grads(0, 1.0)):
        p.grad, pt.grad = g.clone(), g.clone()
    norm = clip_grad_norm_(ps, 0.5)
    norm_t = torch.nn.utils.clip_grad_norm_(ps_t, 0.5)
    assert abs(norm.item() - norm_t.item()) <= 1e-6 * norm_t.item()
    for p, pt in zip(ps, ps_t):
        assert rel_err(p.grad, pt.grad) < 1e-6


def test_max_grad_norm_must_be_positive():
    with pytest.raises(ValueError):
        Adam(_params(), max_grad_norm=0.0)


# ---------------------------------------------------------------------------
def _tiny_vit():
    torch.manual_seed(42)
    return jimm_amd.VisionTransformer(num_classes=5, img_size=32, patch_size=16,
                                      num_layers=1, num_heads=2, mlp_dim=64, hidden_size=32)


def _batch(n=4):
    g = torch.Generator().manual_seed(7)
    return torch.randn(n, 3, 32, 32, generator=g), torch.randint(0, 5, (n,), generator=g)


def test_trainer_reports_grad_norm():
    tr = Trainer(_tiny_vit(), TrainConfig(task="vit", lr=1e-3, max_grad_norm=0.05))
    out = tr.train_step(_batch())
    assert "grad_norm" in out and out["grad_norm"].shape == ()
    assert torch.isfinite(out["grad_norm"]) and out["grad_norm"].item() > 0
    off = Trainer(_tiny_vit(), TrainConfig(task="vit", lr=1e-3))
    assert sorted(off.train_step(_batch())) == ["accuracy", "loss"]


# ---------------------------------------------------------------------------
def _run(rank, world, fn, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(0)
    try:
        fn(rank, world)
    finally:
        dist.destroy_process_group()


def spawn(fn, world=2, port=29541):
    mp.spawn(_run, args=(world, fn, port), nprocs=world, join=True)


def _check_clipped_dp_invariance(rank, world):
    """Clipped Trainer at DP=2 == single process on the same global batch: the
    norm is taken on the DP-averaged gradients, identically on every rank."""
    from jimm_amd.parallel.ddp import DataParallelGrads

    c = 0.05
    imgs, labels = _batch(4)

    ref = _tiny_vit()
    ref_tr = Trainer.__new__(Trainer)  # build without DDP broadcast
    ref_tr.model = ref
    ref_tr.cfg = TrainConfig(task="vit", lr=1e-3, max_grad_norm=c)
    ref_tr.ddp = DataParallelGrads.__new__(DataParallelGrads)
    ref_tr.ddp.enabled = False
    ref_tr.ddp.buckets = []
    ref_tr.ddp.zero_grad = lambda: ref.zero_grad(set_to_none=False)
    ref_tr.ddp.finalize = lambda: None
    ref_tr.opt = Adam(ref.parameters(), lr=1e-3, max_grad_norm=c)
    ref_tr.group = None
    ref_tr.step_idx = 0
    ref_tr._roctx = False
    ref_tr._graph = None
    for _ in range(3):
        ref_tr.train_step((imgs, labels))

    model = _tiny_vit()
    tr = Trainer(model, TrainConfig(task="vit", lr=1e-3, max_grad_norm=c))
    lo, hi = rank * 2, rank * 2 + 2
    for _ in range(3):
        out = tr.train_step((imgs[lo:hi], labels[lo:hi]))
        assert out["grad_norm"].item() > c  # small enough to clip, every step
        norms = [torch.zeros(()) for _ in range(world)]
        dist.all_gather(norms, out["grad_norm"].clone())
        assert all(torch.equal(n, norms[0]) for n in norms), norms

    # same bound as the unclipped test_trainer_dp_invariance
    for p, q in zip(ref.parameters(), model.parameters()):
        assert torch.allclose(p, q, atol=5e-3), (p - q).abs().max()


@pytest.mark.dist
def test_clipped_trainer_dp_invariance():
    spawn(_check_clipped_dp_invariance, port=29541)
