"""The fused similarity-loss head (ops/losses.py, fused=True) on the CPU: its
torch arm runs the same chunk / diag0 / gather logic as the HIP arm, in fp32
torch ops, and has to agree with the unfused losses and with plain autograd.

Tolerances: 1e-5 on fp32 losses and gradients is what
test_siglip_loss_chunking_invariant gives a reordered fp32 sum; the world-2
cases use _dp_invariance's 1e-5 (loss) and 1e-4 (parameter gradients)."""

import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

import jimm_amd
from jimm_amd.ops import losses as L

CHUNKS = [4, 5, 1 << 20]  # 5: ragged last chunk, the diagonal straddles chunks


def _leaves(B, D, seed=0):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(B, D, generator=g).requires_grad_(True)
    txt = torch.randn(B, D, generator=g).requires_grad_(True)
    s = torch.tensor(0.5, requires_grad=True)
    b = torch.tensor(-1.0, requires_grad=True)
    return img, txt, s, b


def _close(got, ref, what, atol=1e-5):
    assert torch.allclose(got, ref, atol=atol), f"{what}: {(got - ref).abs().max().item():.3e}"


@pytest.mark.parametrize("chunk", CHUNKS)
def test_clip_fused_equals_unfused(chunk):
    ref = _leaves(16, 32)
    L.clip_contrastive_loss(ref[0], ref[1], ref[2], gather=False).backward()
    got = _leaves(16, 32)
    loss = L.clip_contrastive_loss(got[0], got[1], got[2], gather=False, fused=True,
                                   chunk_size=chunk)
    loss.backward()
    _close(loss.detach(), L.clip_contrastive_loss(ref[0], ref[1], ref[2], gather=False).detach(),
           "loss")
    for name, g, r in zip(("img", "txt", "logit_scale"), got, ref):
        _close(g.grad, r.grad, name)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_siglip_fused_equals_unfused(chunk):
    ref = _leaves(16, 32)
    loss_r = L.siglip_sigmoid_loss(*ref, gather=False)
    loss_r.backward()
    got = _leaves(16, 32)
    loss = L.siglip_sigmoid_loss(*got, gather=False, fused=True, chunk_size=chunk)
    loss.backward()
    _close(loss.detach(), loss_r.detach(), "loss")
    for name, g, r in zip(("img", "txt", "logit_scale", "logit_bias"), got, ref):
        _close(g.grad, r.grad, name)


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("mode", ["softmax", "sigmoid"])
def test_function_offset_diagonal(mode, chunk):
    """M = 6 rows against N = 18 columns, labels at columns 6 .. 11 (what rank 1
    of 3 sees), through the Function itself, against plain autograd."""
    M, N, D, diag0 = 6, 18, 32, 6

    def leaves():
        g = torch.Generator().manual_seed(1)
        a = torch.randn(M, D, generator=g).requires_grad_(True)
        b = torch.randn(N, D, generator=g).requires_grad_(True)
        s = torch.tensor(1.7, requires_grad=True)
        bias = torch.tensor(-0.8, requires_grad=True) if mode == "sigmoid" else None
        return a, b, s, bias

    a, b, s, bias = leaves()
    x = s * a @ b.t()
    if mode == "softmax":
        ref = F.cross_entropy(x, torch.arange(M) + diag0)
    else:
        z = torch.full((M, N), -1.0)
        z[torch.arange(M), torch.arange(M) + diag0] = 1.0
        ref = -F.logsigmoid(z * (x + bias)).sum()
    ref.backward()

    a2, b2, s2, bias2 = leaves()
    out = L.fused_similarity_loss(a2, b2, s2, bias2, diag0, mode, chunk)
    out.backward()
    _close(out.detach(), ref.detach(), "loss")
    _close(a2.grad, a.grad, "a")
    _close(b2.grad, b.grad, "b")
    _close(s2.grad, s.grad, "scale")
    if mode == "sigmoid":
        _close(bias2.grad, bias.grad, "bias")


def test_function_rejects_mismatched_bias():
    a, b, s, bias = torch.randn(4, 8), torch.randn(4, 8), torch.tensor(1.0), torch.tensor(0.0)
    with pytest.raises(ValueError):
        L.fused_similarity_loss(a, b, s, bias, 0, "softmax")
    with pytest.raises(ValueError):
        L.fused_similarity_loss(a, b, s, None, 0, "sigmoid")


# --- world-2 gloo: DP invariance with the fused head -------------------------


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


def _tiny_clip():
    return jimm_amd.CLIP(embed_dim=16, image_resolution=32, vision_layers=1, vision_width=64,
                         vision_patch_size=16, context_length=8, vocab_size=100,
                         transformer_width=64, transformer_heads=1, transformer_layers=1)


def _dp_invariance_fused(rank, world):
    """Fused CLIP loss + grads at DP=2 equal the single-process global batch."""
    from jimm_amd.parallel.ddp import DataParallelGrads

    torch.manual_seed(0)
    model = _tiny_clip()
    ddp = DataParallelGrads(model)  # also broadcasts params
    torch.manual_seed(42)
    imgs = torch.randn(4, 3, 32, 32)
    ids = torch.randint(0, 99, (4, 8))
    ids[:, -1] = 99
    b = 4 // world
    my_imgs, my_ids = imgs[rank * b : (rank + 1) * b], ids[rank * b : (rank + 1) * b]
    ddp.zero_grad()
    # chunk_size 3 of 4 global columns: a ragged chunk that splits rank 1's labels
    loss = L.clip_contrastive_loss(model.encode_image(my_imgs), model.encode_text(my_ids),
                                   model.logit_scale, fused=True, chunk_size=3)
    loss.backward()
    ddp.finalize()

    model_ref = _tiny_clip()
    model_ref.load_state_dict(model.state_dict())
    loss_r = L.clip_contrastive_loss(model_ref.encode_image(imgs), model_ref.encode_text(ids),
                                     model_ref.logit_scale, gather=False)
    loss_r.backward()

    lt = loss.detach().clone()
    dist.all_reduce(lt)
    assert torch.allclose(lt / world, loss_r.detach(), atol=1e-5), (lt / world, loss_r)
    for (n, p), (nr, pr) in zip(model.named_parameters(), model_ref.named_parameters()):
        assert n == nr
        if pr.grad is None:
            continue
        assert torch.allclose(p.grad, pr.grad, atol=1e-4), f"{n}: {(p.grad - pr.grad).abs().max()}"


@pytest.mark.dist
def test_dp_invariance_clip_fused():
    spawn(_dp_invariance_fused, port=29541)


def _siglip_invariance_fused(rank, world):
    torch.manual_seed(0)
    img = torch.randn(6, 16)
    txt = torch.randn(6, 16)
    scale = torch.tensor(0.7, requires_grad=True)
    bias = torch.tensor(-1.0, requires_grad=True)
    b = 6 // world
    my_img = img[rank * b : (rank + 1) * b].clone().requires_grad_(True)
    my_txt = txt[rank * b : (rank + 1) * b].clone().requires_grad_(True)
    loss = L.siglip_sigmoid_loss(my_img, my_txt, scale, bias, chunk_size=4, fused=True)
    loss.backward()
    img_r = img.clone().requires_grad_(True)
    txt_r = txt.clone().requires_grad_(True)
    scale_r = torch.tensor(0.7, requires_grad=True)
    bias_r = torch.tensor(-1.0, requires_grad=True)
    loss_r = L.siglip_sigmoid_loss(img_r, txt_r, scale_r, bias_r, gather=False)
    loss_r.backward()
    lt = loss.detach().clone()
    dist.all_reduce(lt)
    assert torch.allclose(lt / world, loss_r.detach(), atol=1e-5)
    # the loss is normalized by B_local here and by B_global in the reference
    assert torch.allclose(my_img.grad / world, img_r.grad[rank * b : (rank + 1) * b], atol=1e-5)
    assert torch.allclose(my_txt.grad / world, txt_r.grad[rank * b : (rank + 1) * b], atol=1e-5)
    for p, pr in ((scale, scale_r), (bias, bias_r)):
        t = p.grad.clone()
        dist.all_reduce(t)
        assert torch.allclose(t / world, pr.grad, atol=1e-5), (t / world, pr.grad)


@pytest.mark.dist
def test_dp_invariance_siglip_fused():
    spawn(_siglip_invariance_fused, port=29542)


# --- Trainer -------------------------------------------------------------------


def test_trainer_clip_step_fused_equals_unfused():
    from jimm_amd.train import SyntheticImageText, TrainConfig, Trainer

    def step(fused):
        torch.manual_seed(3)
        tr = Trainer(_tiny_clip(), TrainConfig(task="clip", lr=1e-3, fused_loss_head=fused))
        data = SyntheticImageText(4, 32, 8, 100, torch.device("cpu"), seed=5)
        out = tr.train_step(next(iter(data)))
        return out["loss"], {n: p.grad.clone() for n, p in tr.model.named_parameters()
                             if p.grad is not None}

    loss_r, grads_r = step(False)
    loss, grads = step(True)
    assert torch.allclose(loss, loss_r, atol=1e-5), (loss, loss_r)
    assert grads.keys() == grads_r.keys() and "logit_scale" in grads
    for n in grads:
        assert torch.allclose(grads[n], grads_r[n], atol=1e-4), \
            f"{n}: {(grads[n] - grads_r[n]).abs().max()}"
