"""Adam optimizer with a fused HIP multi-tensor kernel on GPU (K14).

Matches optax.adam semantics used by the reference trainer
(/root/reference/examples/vit_training.py:202-203): bias-corrected first and
second moments, no weight decay by default (AdamW-style decoupled decay
available via ``weight_decay``).

Mixed precision: parameters may be bf16; moments (and optional fp32 master
weights) are kept in fp32. On GPU the whole update runs in one fused HIP
kernel launch per bucket of tensors (csrc/adam.hip); the CPU path is the
numerics oracle.

Global-norm gradient clipping (``max_grad_norm``) runs in the same place: one
multi-tensor read pass for the norm (train/clip.py), then the clip coefficient
is a device scalar that the Adam kernel multiplies into ``g`` as it loads it.
A non-finite norm skips the step and leaves every piece of state untouched.
"""

from __future__ import annotations

import torch

from jimm_amd.ops import _backend
from jimm_amd.train.clip import STATS_LEN, ref_clip_coef


class Adam(torch.optim.Optimizer):
    def __init__(
        self,
        params,
        lr: float = 1e-4,
        betas: tuple[float, float] = (0.9, 0.999),
        eps: float = 1e-8,
        weight_decay: float = 0.0,
        *,
        master_weights: bool = True,
        max_grad_norm: float | None = None,
    ) -> None:
        if max_grad_norm is not None and not max_grad_norm > 0.0:
            raise ValueError(f"max_grad_norm must be positive, got {max_grad_norm}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.master_weights = master_weights
        # graph-capturable fast path: chunk descriptors uploaded once, lr and
        # step live on-device (csrc/adam.hip adam_prepare/adam_apply).
        # Keyed per param group: each group gets its own descriptor table,
        # lr and device-side step counter.
        self._prepared: dict[int, tuple] = {}
        self._last_lr: dict[int, float] = {}
        # global-norm clipping: None = off (every path below stays as it is)
        self.max_grad_norm = max_grad_norm
        self._stats: torch.Tensor | None = None  # [norm, coef, finite, skipped]
        self._partials: tuple | None = None  # (one fp32 per chunk, {group: offset})

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.max_grad_norm is not None:
            self._step_clipped()
            return loss
        for gi, group in enumerate(self.param_groups):
            lr, (b1, b2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
            ps, gs, ms, vs, masters = [], [], [], [], []
            step_t = None
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["m"] = torch.zeros_like(p, dtype=torch.float32)
                    st["v"] = torch.zeros_like(p, dtype=torch.float32)
                    if self.master_weights and p.dtype != torch.float32:
                        st["master"] = p.detach().clone().float()
                st["step"] += 1
                step_t = st["step"]
                ps.append(p)
                gs.append(p.grad)
                ms.append(st["m"])
                vs.append(st["v"])
                masters.append(st.get("master"))
            if not ps:
                continue
            if ps[0].is_cuda and not _backend.force_eager():
                ext = _backend.ext()
                if gi not in self._prepared:
                    if step_t == 1:
                        # first step initializes state lazily; take it eagerly
                        # then freeze the descriptor table (pointers stable)
                        ext.adam_step(ps, gs, ms, vs, masters, lr, b1, b2, eps, wd, step_t)
                    desc, nchunks = ext.adam_prepare(ps, gs, ms, vs, masters)
                    lr_dev = torch.full((1,), lr, dtype=torch.float32, device=ps[0].device)
                    # adam_apply pre-increments on device: seed so the next
                    # apply computes bias correction for the right step
                    seed = step_t if step_t == 1 else step_t - 1
                    step_dev = torch.full((1,), seed, dtype=torch.int32, device=ps[0].device)
                    self._prepared[gi] = (desc, int(nchunks.item()), lr_dev, step_dev)
                    if step_t == 1:
                        continue
                desc, nchunks, lr_dev, step_dev = self._prepared[gi]
                if lr != self._last_lr.get(gi):
                    lr_dev.fill_(lr)
                    self._last_lr[gi] = lr
                ext.adam_apply(desc, nchunks, lr_dev, step_dev, b1, b2, eps, wd)
            else:
                self._ref_step(ps, gs, ms, vs, masters, lr, b1, b2, eps, wd, step_t)
        return loss

    # -- global-norm clipping --------------------------------------------------
    def _gather(self, group):
        ps, gs, ms, vs, masters = [], [], [], [], []
        for p in group["params"]:
            if p.grad is None:
                continue
            st = self.state[p]
            if not st:
                st["step"] = 0
                st["m"] = torch.zeros_like(p, dtype=torch.float32)
                st["v"] = torch.zeros_like(p, dtype=torch.float32)
                if self.master_weights and p.dtype != torch.float32:
                    st["master"] = p.detach().clone().float()
            ps.append(p)
            gs.append(p.grad)
            ms.append(st["m"])
            vs.append(st["v"])
            masters.append(st.get("master"))
        return ps, gs, ms, vs, masters

    def _stats_buf(self) -> torch.Tensor:
        dev = self.param_groups[0]["params"][0].device
        if self._stats is None or self._stats.device != dev:
            self._stats = torch.zeros(STATS_LEN, dtype=torch.float32, device=dev)
        return self._stats

    @property
    def last_grad_norm(self) -> torch.Tensor:
        """Pre-clip global L2 norm of the latest step: a 0-d fp32 view of the
        device stats buffer (no sync to read it; stays live under graph replay)."""
        return self._stats_buf()[0]

    def skipped_steps(self) -> int:
        """Steps skipped so far because the global norm was inf or NaN (syncs)."""
        return int(self._stats_buf()[3].item())

    def _prepare_clipped(self, groups) -> None:
        """Freeze the per-group descriptor tables right after lazy state init,
        so the device path (and with it the clip) runs from step 1 on."""
        ext = _backend.ext()
        self.sync_step_from_device()  # tables being replaced: keep their counters
        self._prepared, self._last_lr, offs, total = {}, {}, {}, 0
        for gi, group, (ps, gs, ms, vs, masters) in groups:
            desc, nchunks = ext.adam_prepare(ps, gs, ms, vs, masters)
            n = int(nchunks.item())
            dev = ps[0].device
            lr_dev = torch.full((1,), group["lr"], dtype=torch.float32, device=dev)
            # the apply pre-increments on device: seed with the steps taken so far
            step_dev = torch.full((1,), int(self.state[ps[-1]]["step"]), dtype=torch.int32, device=dev)
            self._prepared[gi] = (desc, n, lr_dev, step_dev)
            self._last_lr[gi] = group["lr"]
            offs[gi] = total
            total += n
        self._partials = (torch.zeros(total, dtype=torch.float32, device=dev), offs)

    def _step_clipped(self) -> None:
        groups = [(gi, group, self._gather(group)) for gi, group in enumerate(self.param_groups)]
        groups = [g for g in groups if g[2][0]]
        if not groups:
            return
        stats = self._stats_buf()
        if groups[0][2][0][0].is_cuda and not _backend.force_eager():
            ext = _backend.ext()
            if self._partials is None or any(gi not in self._prepared for gi, _, _ in groups):
                self._prepare_clipped(groups)
            partials, offs = self._partials
            # the norm is global: every group's partials, then ONE finalize,
            # before any group is updated. Host per-param step counters do not
            # advance here (a skip is decided on the device); state_dict() and
            # sync_step_from_device() read them back.
            for gi, _, _ in groups:
                ext.grad_sqnorm(self._prepared[gi][0], self._prepared[gi][1], partials, offs[gi])
            ext.clip_finalize(partials, stats, float(self.max_grad_norm))
            for gi, group, _ in groups:
                desc, nchunks, lr_dev, step_dev = self._prepared[gi]
                if group["lr"] != self._last_lr.get(gi):
                    lr_dev.fill_(group["lr"])
                    self._last_lr[gi] = group["lr"]
                (b1, b2) = group["betas"]
                ext.adam_apply_clipped(desc, nchunks, lr_dev, step_dev, stats, b1, b2,
                                       group["eps"], group["weight_decay"])
            return
        norm, coef = ref_clip_coef([g for _, _, t in groups for g in t[1]], float(self.max_grad_norm))
        finite = bool(torch.isfinite(norm))
        stats[0], stats[1], stats[2] = norm, coef, float(finite)
        if not finite:
            stats[3] += 1
            return
        for _, group, (ps, gs, ms, vs, masters) in groups:
            for p in ps:
                self.state[p]["step"] += 1
            (b1, b2) = group["betas"]
            self._ref_step(ps, [g.float() * coef for g in gs], ms, vs, masters, group["lr"],
                           b1, b2, group["eps"], group["weight_decay"], self.state[ps[-1]]["step"])

    def state_dict(self):
        if self.max_grad_norm is not None:
            self.sync_step_from_device()  # host counters do not see device-side skips
        return super().state_dict()

    def set_device_lr(self, lr: float) -> None:
        """Refresh the device-side lr used by graph-replayed adam_apply."""
        for gi, prep in self._prepared.items():
            prep[2].fill_(lr)
            self._last_lr[gi] = lr

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        # The base class casts loaded state to the param dtype; for bf16
        # params that would silently demote the fp32 moments/master weights
        # (and break the fused kernel's data_ptr<float>()). Restore fp32.
        for group in self.param_groups:
            for p in group["params"]:
                st = self.state.get(p)
                if not st:
                    continue
                for key in ("m", "v", "master"):
                    if key in st and st[key] is not None and st[key].dtype != torch.float32:
                        st[key] = st[key].float()
        self._prepared = {}  # moment tensors were replaced: descriptors stale
        self._last_lr = {}
        # chunk partials are laid out by the descriptor tables: rebuilt with them
        # (the stats buffer stays, so last_grad_norm and the skip count live on)
        self._partials = None

    @torch.no_grad()
    def sync_step_from_device(self) -> None:
        """Copy the on-device step counter back into per-param state (needed
        after graph-replayed training, where host counters do not advance)."""
        if not self._prepared:
            return
        for gi, group in enumerate(self.param_groups):
            if gi not in self._prepared:
                continue
            step = int(self._prepared[gi][3].item())
            for p in group["params"]:
                if self.state[p]:
                    self.state[p]["step"] = step

    @staticmethod
    def _ref_step(ps, gs, ms, vs, masters, lr, b1, b2, eps, wd, t):
        bc1 = 1.0 - b1**t
        bc2 = 1.0 - b2**t
        for p, g, m, v, master in zip(ps, gs, ms, vs, masters):
            gf = g.float()
            m.mul_(b1).add_(gf, alpha=1 - b1)
            v.mul_(b2).addcmul_(gf, gf, value=1 - b2)
            mhat = m / bc1
            vhat = v / bc2
            upd = mhat / (vhat.sqrt() + eps)
            target = master if master is not None else p
            if wd != 0.0:
                upd = upd + wd * target.float()
            target.add_(upd.to(target.dtype), alpha=-lr)
            if master is not None:
                p.copy_(master.to(p.dtype))
