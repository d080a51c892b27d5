"""Counter-based dropout on the CPU: the Philox generator against published
known answers, the element addressing against fixed fixture values, the
statistics of the mask, and the properties the models rely on (identity at
p = 0 and in eval mode, gradient = mask * s, checkpoint recompute and trainer
checkpoints replay the same masks).

Statistical bounds: over n = 2^20 elements the keep rate of an ideal
generator has sigma = sqrt(q (1 - q) / n); 5 sigma leaves a false-alarm rate
of 6e-7 per case. A sample correlation of two independent bit streams has
sigma ~ 1 / sqrt(n) = 9.8e-4, so 5e-3 is 5 sigma as well, and so is the
agreement rate of two independent masks (sigma <= 0.5 / sqrt(n) = 4.9e-4)."""

import functools
import math

import pytest
import torch

import jimm_amd
from jimm_amd import ops
from jimm_amd.models.common.transformer import EncoderBlock
from jimm_amd.ops import philox_dropout as D

TUPLES = [(1234, 0, 0), (1234, 1, 0), (1234, 0, 1), (99, 7, 23)]
PS = [0.1, 0.5]
N = 1024


@functools.lru_cache(maxsize=None)
def u_of(seed, step, site):
    """u over 1024 x 1024, computed once per tuple and shared (read only)."""
    return D.dropout_u(N, N, seed, step, site)


def keep_of(p, tup):
    return u_of(*tup) >= D.dropout_threshold(p)


def rng_of(seed, step):
    return torch.tensor([seed, step], dtype=torch.int64)


def hexwords(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_philox_known_answers():
    assert hexwords(D.philox4x32((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert hexwords(D.philox4x32((ones,) * 4, (ones,) * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    pi = (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344)
    assert hexwords(D.philox4x32(pi, (0xA4093822, 0x299F31D0))) == "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_fixture_values():
    u = D.dropout_u(37, 200, 1234, 0, 0)
    assert u[0, 0].item() == 45896
    assert u[0, 1].item() == 7001
    assert u[1, 0].item() == 8336
    assert u[36, 199].item() == 44664
    assert 0 <= u.min().item() and u.max().item() <= 0xFFFF


def test_threshold_and_scale():
    assert D.dropout_threshold(0.0) == 0
    assert D.dropout_threshold(0.1) == 6554
    assert D.dropout_threshold(0.5) == 32768
    assert D.dropout_scale(32768) == 2.0
    assert D.dropout_scale(6554) == torch.tensor(65536.0 / 58982.0, dtype=torch.float32).item()
    with pytest.raises(ValueError):
        D.dropout_threshold(1.0)


@pytest.mark.parametrize("tup", TUPLES, ids=str)
@pytest.mark.parametrize("p", PS)
def test_keep_rate(p, tup):
    q = 1.0 - D.dropout_threshold(p) / 65536.0
    sigma = math.sqrt(q * (1.0 - q) / (N * N))
    rate = keep_of(p, tup).double().mean().item()
    print(f"p={p} {tup}: keep rate {rate:.6f}, expected {q:.6f}, {(rate - q) / sigma:+.2f} sigma")
    assert abs(rate - q) <= 5.0 * sigma


def corr(a, b):
    a = a.double().flatten() - a.double().mean()
    b = b.double().flatten() - b.double().mean()
    return ((a * b).mean() / (a.pow(2).mean().sqrt() * b.pow(2).mean().sqrt())).item()


@pytest.mark.parametrize("tup", TUPLES, ids=str)
@pytest.mark.parametrize("p", PS)
def test_neighbour_correlation(p, tup):
    keep = keep_of(p, tup)
    c_col = corr(keep[:, :-1], keep[:, 1:])
    c_row = corr(keep[:-1, :], keep[1:, :])
    print(f"p={p} {tup}: corr columns {c_col:+.2e}, rows {c_row:+.2e}")
    assert abs(c_col) < 5e-3 and abs(c_row) < 5e-3


@pytest.mark.parametrize("other", [(1234, 1, 0), (1234, 0, 1)], ids=["step", "site"])
@pytest.mark.parametrize("p", PS)
def test_masks_independent(p, other):
    q = 1.0 - D.dropout_threshold(p) / 65536.0
    agree = (keep_of(p, (1234, 0, 0)) == keep_of(p, other)).double().mean().item()
    print(f"p={p} {other}: agreement {agree:.4f}, expected {q * q + (1 - q) ** 2:.4f}")
    assert abs(agree - (q * q + (1.0 - q) ** 2)) <= 5e-3


def test_p_zero_is_identity():
    x = torch.randn(5, 7)
    assert ops.dropout(x, 0.0, None, 3) is x
    assert ops.dropout(x, 0.0, rng_of(1, 2), 3) is x
    with pytest.raises(ValueError):
        ops.dropout(x, 0.1, None, 0)


def test_forward_and_gradient_are_mask_times_s():
    """Leading dimensions flatten into rows; y = x * mask * s and so is dy."""
    p, seed, step, site = 0.5, 1234, 3, 5
    x = (1.0 + torch.rand(3, 5, 70)).requires_grad_(True)
    y = ops.dropout(x, p, rng_of(seed, step), site)
    mask = D.keep_mask(15, 70, p, seed, step, site).view(3, 5, 70)
    s = D.dropout_scale(D.dropout_threshold(p))
    assert 0 < mask.sum().item() < mask.numel()
    assert torch.equal(y.detach(), x.detach() * mask * s)
    dy = torch.randn_like(x)
    (dx,) = torch.autograd.grad(y, x, dy)
    assert torch.equal(dx, dy * mask * s)


def make_block(dropout_rate):
    torch.manual_seed(11)
    return EncoderBlock(64, 2, 128, dropout_rate=dropout_rate, layernorm_epsilon=1e-6)


def test_eval_mode_is_dropout_free():
    x = torch.randn(2, 9, 64)
    drop, plain = make_block(0.1).eval(), make_block(0.0).eval()
    before = ops.get_dropout_state("cpu")
    assert torch.equal(drop(x), plain(x))
    assert ops.get_dropout_state("cpu") == before  # nothing drawn in eval
    drop.train()
    assert not torch.equal(drop(x), plain(x))


def test_block_uses_both_sites_and_given_rng():
    """Training output is a function of rng and the block's sites alone."""
    blk = make_block(0.5).train()
    x = torch.randn(2, 9, 64)
    y0 = blk(x, rng_of(5, 0))
    assert torch.equal(y0, blk(x, rng_of(5, 0)))
    assert not torch.equal(y0, blk(x, rng_of(5, 1)))
    blk.site0 = 2
    assert not torch.equal(y0, blk(x, rng_of(5, 0)))


def test_encoder_draws_one_step_per_forward():
    from jimm_amd.models.common.transformer import Encoder

    torch.manual_seed(0)
    enc = Encoder(2, 64, 2, 128, dropout_rate=0.5).train()
    assert [layer.site0 for layer in enc.layers] == [0, 2]
    x = torch.randn(2, 9, 64)
    ops.set_dropout_seed(17)
    assert ops.get_dropout_state("cpu") == (17, 0)
    y0 = enc(x)
    assert ops.get_dropout_state("cpu") == (17, 1)
    y1 = enc(x)
    assert not torch.equal(y0, y1)  # a second forward gets the next step
    ops.set_dropout_state("cpu", 17, 0)
    assert torch.equal(enc(x), y0)


def test_checkpoint_replays_masks():
    from torch.utils.checkpoint import checkpoint

    blk = make_block(0.5).train()
    x = torch.randn(2, 9, 64)
    dy = torch.randn(2, 9, 64)
    rng = rng_of(77, 4)

    def grads(fn):
        for prm in blk.parameters():
            prm.grad = None
        xi = x.clone().requires_grad_(True)
        y = fn(xi)
        y.backward(dy)
        return [y.detach(), xi.grad] + [prm.grad.clone() for prm in blk.parameters()]

    plain = grads(lambda xi: blk(xi, rng))
    ckpt = grads(lambda xi: checkpoint(blk, xi, rng, use_reentrant=False))
    assert len(plain) == 2 + 12
    for a, b in zip(plain, ckpt):
        assert torch.equal(a, b)


def test_trainer_checkpoint_round_trip(tmp_path):
    """Save, step, load, step: the second step repeats the first bit for bit,
    which needs the dropout {seed, step} restored with the weights."""
    from jimm_amd.train import TrainConfig, Trainer

    torch.manual_seed(3)
    model = jimm_amd.VisionTransformer(
        num_classes=5, img_size=32, patch_size=16, num_layers=2, num_heads=2,
        mlp_dim=64, hidden_size=32, dropout_rate=0.1,
    ).float().train()
    tr = Trainer(model, TrainConfig(task="vit", lr=1e-3, seed=21))
    batch = (torch.randn(4, 3, 32, 32), torch.randint(0, 5, (4,)))
    tr.train_step(batch)  # move off step 0
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    state = ops.get_dropout_state("cpu")
    assert state[0] == 21 and state[1] > 0
    loss1 = tr.train_step(batch)["loss"].clone()
    assert ops.get_dropout_state("cpu") != state
    tr.load_checkpoint(path)
    assert ops.get_dropout_state("cpu") == state
    loss2 = tr.train_step(batch)["loss"]
    assert torch.equal(loss1, loss2)
    # and the masks matter: the same weights at the next step give another loss
    tr.load_checkpoint(path)
    ops.set_dropout_state("cpu", state[0], state[1] + 1)
    assert not torch.equal(tr.train_step(batch)["loss"], loss1)
