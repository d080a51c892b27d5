"""Transformer building blocks (MI355X-first re-design of the reference's
``src/jimm/common/transformer.py``).

Semantics preserved from the reference:
  * pre-LN residual block: ``x = x + attn(LN1(x))`` then ``x = x + mlp(LN2(x))``
    (/root/reference/src/jimm/common/transformer.py:130-131)
  * MLP = Linear -> (quick)gelu -> Dropout -> Linear -> Dropout
    (transformer.py:92-114); quickgelu = x*sigmoid(1.702x) (transformer.py:12-19)
  * optional causal masking for the CLIP text tower (models/clip.py:62)

MI355X-first deltas (deliberate, not a port):
  * fused QKV projection: one (3H, H) GEMM instead of the reference's three
    separate (H, heads, d) kernels (transformer.py:67-79) — one MFMA GEMM
    feeding the flash-attention kernel's (B, heads, L, d) layout;
  * gelu is the exact erf GELU (matches the HuggingFace PyTorch oracle the
    parity tests compare against; the reference uses flax's tanh approx);
  * attention runs in a single flash-style HIP kernel (K5) on GPU.
"""

from __future__ import annotations

import torch
from torch import nn

from jimm_amd import ops


class EncoderBlock(nn.Module):
    """Pre-LN transformer encoder block with fused-QKV attention."""

    def __init__(
        self,
        hidden_size: int,
        num_heads: int,
        mlp_dim: int,
        *,
        dropout_rate: float = 0.0,
        hidden_act: str = "gelu",
        layernorm_epsilon: float = 1e-5,
        causal: bool = False,
    ) -> None:
        super().__init__()
        if hidden_size % num_heads != 0:
            raise ValueError(f"hidden_size {hidden_size} not divisible by num_heads {num_heads}")
        self.hidden_size = hidden_size
        self.num_heads = num_heads
        self.head_dim = hidden_size // num_heads
        self.causal = causal
        self.eps = layernorm_epsilon
        self.act = hidden_act

        self.norm1 = nn.LayerNorm(hidden_size, eps=layernorm_epsilon)
        self.norm2 = nn.LayerNorm(hidden_size, eps=layernorm_epsilon)
        self.qkv = nn.Linear(hidden_size, 3 * hidden_size, bias=True)
        self.proj = nn.Linear(hidden_size, hidden_size, bias=True)
        self.fc1 = nn.Linear(hidden_size, mlp_dim, bias=True)
        self.fc2 = nn.Linear(mlp_dim, hidden_size, bias=True)
        self.dropout = nn.Dropout(dropout_rate)  # holds p; ops.dropout does the work
        # dropout sites of this block: site0 after the activation, site0 + 1
        # after fc2 (an Encoder numbers its layers 2 * layer_index)
        self.site0 = 0

    def _forward_tp(self, x: torch.Tensor) -> torch.Tensor:
        """Tensor-parallel path (parallel/tp.py): local heads + local MLP
        shard, partial out-projections all-reduced over the TP group."""
        from jimm_amd.parallel.tp import copy_to_tp, reduce_from_tp

        B, L, H = x.shape
        g = self._tp_group
        h = ops.layer_norm(x, self.norm1.weight, self.norm1.bias, self.eps)
        h = copy_to_tp(h, g)
        qkv = ops.linear(h, self.qkv.weight, self.qkv.bias)  # (B, L, 3*H_local)
        qkv = qkv.view(B, L, 3, self.num_heads, self.head_dim)
        o = ops.attention_qkv(qkv, causal=self.causal)       # local heads
        o = o.transpose(1, 2).reshape(B, L, self.num_heads * self.head_dim)
        part = ops.linear(o, self.proj.weight)               # partial, no bias
        x = reduce_from_tp(part, g) + self.proj.bias + x

        h = ops.layer_norm(x, self.norm2.weight, self.norm2.bias, self.eps)
        h = copy_to_tp(h, g)
        h = ops.linear(h, self.fc1.weight, self.fc1.bias, act=self.act)
        part = ops.linear(h, self.fc2.weight)
        return reduce_from_tp(part, g) + self.fc2.bias + x

    def forward(self, x: torch.Tensor, rng: torch.Tensor | None = None) -> torch.Tensor:
        """rng: the ``{seed, step}`` snapshot of this forward pass
        (``ops.next_dropout_rng``), handed down by the Encoder so that a
        checkpoint recompute sees the same masks; a block called on its own
        draws one. Only read in training mode with dropout_rate > 0."""
        if getattr(self, "_tp_group", None) is not None:
            return self._forward_tp(x)
        from jimm_amd.ops import block as fused

        # the ACTIVE dropout probability: eval of a dropout-built model is
        # the dropout-free model, fused block included
        p = self.dropout.p if self.training else 0.0
        if p > 0 and rng is None:
            rng = ops.next_dropout_rng(x.device)
        if (
            fused.fused_block_enabled(x, p, self.fc1.out_features)
            and self.head_dim in (64, 72, 80, 96, 128)
        ):
            import math

            return fused.encoder_block(
                x, self.norm1, self.qkv, self.proj, self.norm2, self.fc1, self.fc2,
                num_heads=self.num_heads, act=self.act, eps=self.eps,
                causal=self.causal, scale=1.0 / math.sqrt(self.head_dim),
                p=p, rng=rng, site0=self.site0,
            )
        B, L, H = x.shape
        h = ops.layer_norm(x, self.norm1.weight, self.norm1.bias, self.eps)
        qkv = ops.linear(h, self.qkv.weight, self.qkv.bias)  # (B, L, 3H)
        qkv = qkv.view(B, L, 3, self.num_heads, self.head_dim)
        o = ops.attention_qkv(qkv, causal=self.causal)  # (B, heads, L, d)
        o = o.transpose(1, 2).reshape(B, L, H)
        x = ops.linear(o, self.proj.weight, self.proj.bias, residual=x)

        h = ops.layer_norm(x, self.norm2.weight, self.norm2.bias, self.eps)
        h = ops.linear(h, self.fc1.weight, self.fc1.bias, act=self.act)
        if p > 0:
            h = ops.dropout(h, p, rng, self.site0)
            h = ops.linear(h, self.fc2.weight, self.fc2.bias)
            return x + ops.dropout(h, p, rng, self.site0 + 1)
        # dropout inactive: residual add fused into the fc2 epilogue (K8)
        return ops.linear(h, self.fc2.weight, self.fc2.bias, residual=x)


class Encoder(nn.Module):
    """Stack of N identical pre-LN encoder blocks.

    Reference: ``Transformer`` (/root/reference/src/jimm/common/transformer.py:135-196).
    """

    def __init__(
        self,
        num_layers: int,
        hidden_size: int,
        num_heads: int,
        mlp_dim: int,
        *,
        dropout_rate: float = 0.0,
        hidden_act: str = "gelu",
        layernorm_epsilon: float = 1e-6,
        causal: bool = False,
    ) -> None:
        super().__init__()
        self.layers = nn.ModuleList(
            EncoderBlock(
                hidden_size,
                num_heads,
                mlp_dim,
                dropout_rate=dropout_rate,
                hidden_act=hidden_act,
                layernorm_epsilon=layernorm_epsilon,
                causal=causal,
            )
            for _ in range(num_layers)
        )
        self.dropout_rate = dropout_rate
        for i, layer in enumerate(self.layers):
            layer.site0 = 2 * i

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        # One {seed, step} snapshot per forward pass, shared by every block:
        # a checkpointed block's recompute replays identical masks, and a
        # second tower or a second forward draws the next step.
        rng = None
        if self.training and self.dropout_rate > 0:
            rng = ops.next_dropout_rng(x.device)
        if getattr(self, "gradient_checkpointing", False) and torch.is_grad_enabled():
            from torch.utils.checkpoint import checkpoint

            # recompute checkpointed blocks' forwards during backward:
            # activation memory per block drops from ~16 to ~1 tensors of
            # (B,L,H) (needed for e.g. SigLIP at 4096 pairs/GPU = the
            # 32k-global BASELINE config on 8 GPUs; without it b4096 OOMs
            # 288 GB). checkpoint_every = n > 1 is the selective variant:
            # only every n-th block recomputes — 1/n of the recompute cost
            # for ~(1 - 1/n) of the memory win's complement; pick n by how
            # much headroom the batch leaves.
            every = int(getattr(self, "checkpoint_every", 1) or 1)
            for i, layer in enumerate(self.layers):
                if i % every == 0:
                    x = checkpoint(layer, x, rng, use_reentrant=False)
                else:
                    x = layer(x, rng)
            return x
        for layer in self.layers:
            x = layer(x, rng)
        return x
