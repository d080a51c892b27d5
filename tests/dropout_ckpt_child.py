"""Child process of test_dropout_gpu.py::test_checkpointing_replays_masks_bitwise
(started with JIMM_AMD_DETERMINISTIC=1): one training forward + backward of a
2-layer dropout ViT with and without gradient checkpointing, from the same
dropout {seed, step}; loss and all gradients must agree bit for bit."""

import sys

import torch

import jimm_amd
from jimm_amd import ops
from jimm_amd.ops import block as block_mod


def main() -> int:
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    model = jimm_amd.VisionTransformer(
        num_classes=10, img_size=64, patch_size=16, num_layers=2, num_heads=4,
        mlp_dim=512, hidden_size=256, dropout_rate=0.1,
    ).to(dev, torch.bfloat16).train()
    images = torch.randn(8, 3, 64, 64, device=dev).bfloat16()
    labels = torch.randint(0, 10, (8,), device=dev)

    fused_calls = []
    inner = block_mod.encoder_block

    def spy(*a, **kw):
        fused_calls.append(kw["p"])
        return inner(*a, **kw)

    block_mod.encoder_block = spy

    def run(ckpt: bool):
        model.vision.encoder.gradient_checkpointing = ckpt
        for prm in model.parameters():
            prm.grad = None
        ops.set_dropout_state(dev, 77, 4)
        del fused_calls[:]
        loss = torch.nn.functional.cross_entropy(model(images).float(), labels)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), [prm.grad.clone() for prm in model.parameters()], len(fused_calls)

    loss_a, grads_a, n_a = run(False)
    loss_b, grads_b, n_b = run(True)
    print(f"fused blocks: {n_b} (plain run: {n_a})")
    if n_a != 2 or n_b != 4:
        print("the fused block did not run as expected")
        return 1
    bad = [n for (n, _), a, b in zip(model.named_parameters(), grads_a, grads_b) if not torch.equal(a, b)]
    if not torch.equal(loss_a, loss_b) or bad:
        print(f"loss {loss_a.item()} vs {loss_b.item()}; differing gradients: {bad}")
        return 1
    # the masks are live: another step changes the loss
    ops.set_dropout_state(dev, 77, 5)
    with torch.no_grad():
        other = torch.nn.functional.cross_entropy(model(images).float(), labels)
    if torch.equal(other, loss_a):
        print("the loss does not depend on the dropout step")
        return 1
    print("checkpoint: bitwise equal")
    return 0


if __name__ == "__main__":
    sys.exit(main())
