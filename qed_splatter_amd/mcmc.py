"""Splatfacto's ``strategy="mcmc"`` (nerfstudio 1.1.5, backed by gsplat's ``MCMCStrategy``): a fixed budget of Gaussians
that grows by 5 % per refinement up to ``cap_max``, relocation of dead Gaussians onto live ones, and position noise every
step.  The regularisers that go with it (``mcmc_opacity_reg`` / ``mcmc_scale_reg``) are part of the model's loss
(model.py, ``config.strategy == "mcmc"``).

``McmcStrategy.step_post_backward`` takes the place of splatfacto's ``strategy.step_post_backward`` callback.  The
per-Gaussian work runs in csrc/mcmc.hip on the flat parameter / Adam-moment buffers; this file sequences the launches and,
when the count grows, swaps the buffers in as ``densify.Densifier`` does.  A relocation rewrites the buffers in place and
never reads anything back: once N sits at the cap, a captured step (graph.GraphedTrainStep) stays valid.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import torch
from torch import Tensor

from . import _lib as L

_stream = L.current_stream


@dataclass
class McmcConfig:
    """gsplat MCMCStrategy as splatfacto configures it: refine_start = warmup_length, refine_stop = stop_split_at,
    min_opacity = cull_alpha_thresh (the reference's 0.005, config.py:40)."""
    cap_max: int = 1_000_000
    noise_lr: float = 5e5
    refine_start: int = 500
    refine_stop: int = 15000
    refine_every: int = 100
    min_opacity: float = 0.005

    def refines_at(self, step: int) -> bool:
        """Does ``step_post_backward(step)`` relocate and add?"""
        return self.refine_start < step < self.refine_stop and step % self.refine_every == 0

    @classmethod
    def from_model(cls, model_config) -> "McmcConfig":
        return cls(cap_max=int(model_config.max_gs_num), noise_lr=float(model_config.noise_lr))


class McmcStrategy:
    """Relocation, growth and noise on ``model`` and its optimiser (``FlatAdam`` or ``QedAdamSet``).

    ``seed`` keys every draw and every noise sample: (seed, refinement counter, row) for the draws, (seed, step, row) for
    the noise.  Data-parallel replicas built with the same seed take the same decisions and add the same noise without
    exchanging anything."""

    def __init__(self, model, optimizer, config: Optional[McmcConfig] = None, seed: int = 0):
        from .optim import FlatAdam, QedAdamSet
        if getattr(model, "_flat", None) is None:
            raise RuntimeError("McmcStrategy needs the flat parameter layout: the model was built with separate_params=True")
        if getattr(model.config, "strategy", "default") != "mcmc":
            raise ValueError(f"McmcStrategy: the model's config.strategy is {model.config.strategy!r}; set "
                             "strategy='mcmc' (the loss then carries the MCMC regularisers)")
        if not isinstance(optimizer, (FlatAdam, QedAdamSet)):
            raise TypeError(f"McmcStrategy rewrites the Adam moments in place: it needs a FlatAdam or a QedAdamSet, not "
                            f"{type(optimizer).__name__}")
        self.model, self.optimizer = model, optimizer
        self.config = config or McmcConfig.from_model(model.config)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.n_refinements = 0          # counter of the draws (relocate and add each take one value)
        self.n_noise = 0                # host step of inject_noise calls given no step
        self._ws: Optional[Tensor] = None
        self._n_dead = torch.zeros(1, dtype=torch.int32, device=model.device)
        self.last_info: Dict = {}

    # ---- splatfacto's strategy.step_post_backward ----
    @torch.no_grad()
    def step_post_backward(self, step: int, device_state: bool = False) -> Dict:
        """After the optimiser step of ``step``: relocation + growth on refinement steps, then the noise.
        ``device_state``: the optimiser stepped with ``device_state=True`` (the noise then reads its step and means
        rate from the device, and the launch can be captured)."""
        m = self.model
        info = {"n_dead": 0, "n_added": 0, "n_before": m.num_points, "n_after": m.num_points}
        if self.config.refines_at(step):
            info["n_dead"] = self.relocate()
            info["n_added"] = self.add()
        self.inject_noise(step=None if device_state else step, device_state=device_state)
        info["n_after"] = m.num_points
        self.last_info = info
        return info

    # ---- the three public pieces ----
    @torch.no_grad()
    def relocate(self, sources: Optional[Tensor] = None) -> Tensor:
        """Dead Gaussians (sigmoid(opacity) <= min_opacity) take the parameters of live ones drawn in proportion to their
        opacity, which split their opacity and shrink their scales for it (gsplat ``relocate``); the sources' Adam moments
        are zeroed.  In place: nothing is allocated, nothing is read back.  ``sources`` (tests): int32 [N], read at the
        dead rows only, replaces the draw.  Returns the number of dead rows as a DEVICE int32 tensor (0-dim)."""
        m, opt = self.model, self.optimizer
        n = m.num_points
        if n == 0:
            return self._n_dead[0]
        src = self._rows(sources, n, "relocate") if sources is not None else None
        ws = self._workspace(n, n)
        L.check(L.load().qed_mcmc_relocate(n, L.ptr(m.flat_params), L.ptr(opt.exp_avg), L.ptr(opt.exp_avg_sq),
                                           m.layout.c_begin_ptr, float(self.config.min_opacity), L.ptr(src),
                                           self.seed, self.n_refinements, L.ptr(self._n_dead), L.ptr(ws), ws.numel(),
                                           _stream()), "qed_mcmc_relocate")
        self.n_refinements += 1
        return self._n_dead[0]

    @torch.no_grad()
    def add(self, sources: Optional[Tensor] = None) -> int:
        """Grow to min(cap_max, int(1.05 N)) by copying Gaussians drawn in proportion to their opacity (gsplat
        ``sample_add``): the sources are updated as in ``relocate`` and keep their moments, the copies start with zero
        moments.  Swaps in new flat buffers (``rebind_flat`` / ``rebind``) only when something is added.  ``sources``
        (tests): int32 [n_add] in [0, N).  Returns the number of Gaussians added."""
        m, opt = self.model, self.optimizer
        n = m.num_points
        n_add = max(0, min(int(self.config.cap_max), int(1.05 * n)) - n)
        if n_add == 0 or n == 0:
            return 0
        src = self._rows(sources, n_add, "add") if sources is not None else None
        if src is not None and (int(src.min()) < 0 or int(src.max()) >= n):
            raise ValueError(f"McmcStrategy.add: sources must lie in [0, {n})")
        new = m.layout.resized(n + n_add)
        new_p, new_m, new_v = new.empty_like_state(m.device)
        ws = self._workspace(n, n_add)
        L.check(L.load().qed_mcmc_add(n, n_add, L.ptr(m.flat_params), L.ptr(opt.exp_avg), L.ptr(opt.exp_avg_sq),
                                      m.layout.c_begin_ptr, float(self.config.min_opacity), L.ptr(src), self.seed,
                                      self.n_refinements, L.ptr(new_p), L.ptr(new_m), L.ptr(new_v),
                                      new.c_begin_ptr, L.ptr(ws), ws.numel(), _stream()), "qed_mcmc_add")
        self.n_refinements += 1
        m.rebind_flat(new_p, n + n_add)
        opt.rebind(new_m, new_v)
        return n_add

    @torch.no_grad()
    def inject_noise(self, noise: Optional[Tensor] = None, step: Optional[int] = None, device_state: bool = False) -> None:
        """means += Sigma (eps gate lr_means noise_lr) (gsplat ``inject_noise_to_position``), Sigma = R diag(s^2) R^T,
        gate = sigmoid(100 ((1 - sigma) - 0.995)).

        ``lr_means`` is the means rate the optimiser applied in the step just taken: FlatAdam's schedule value, its
        ``dev_lr`` slot under ``device_state=True``, or the means QedAdam's rate.  (Nerfstudio reads its scheduler after
        stepping it, i.e. one step later: 1.5e-4 relative under the reference's schedule.)  eps: standard normals keyed by
        (seed, step, row), with the step from ``FlatAdam.dev_state`` under ``device_state=True`` (capturable), else
        ``step`` or this object's own count of calls; ``noise`` [N,3] (tests) replaces them.  A step whose frame
        overflowed its intersection buffer (the Adam skip word) adds no noise."""
        from .optim import FlatAdam, _skip_flag
        m, opt = self.model, self.optimizer
        n = m.num_points
        if n == 0:
            return
        if noise is not None:
            noise = noise.to(device=m.device, dtype=torch.float32).contiguous()
            if noise.shape != (n, 3):
                raise ValueError(f"inject_noise: noise must be [{n}, 3]")
        i_means = m.group_names.index("means")
        dev_lr = dev_state = None
        if isinstance(opt, FlatAdam):
            lr, skip = float(opt.lr[i_means]), opt._skip()
            if device_state:
                dev_lr, dev_state = opt.dev_lr[i_means:i_means + 1], opt.dev_state
        else:
            if device_state:
                raise RuntimeError("inject_noise(device_state=True) needs a FlatAdam stepped with device_state=True")
            lr, skip = float(opt.optimizers["means"].param_groups[0]["lr"]), _skip_flag(m.device)
        if step is None and not device_state:
            self.n_noise += 1
            step = self.n_noise
        L.check(L.load().qed_mcmc_noise(n, L.ptr(m.means), L.ptr(m.scales), L.ptr(m.quats), L.ptr(m.opacities),
                                        L.ptr(noise), lr, L.ptr(dev_lr), float(self.config.noise_lr), int(step or 0),
                                        L.ptr(dev_state), self.seed, skip, _stream()), "qed_mcmc_noise")

    # ---- checkpointing ----
    def state_dict(self) -> Dict:
        return {"seed": self.seed, "n_refinements": self.n_refinements, "n_noise": self.n_noise,
                "config": dict(self.config.__dict__)}

    def load_state_dict(self, sd: Dict) -> None:
        self.seed = int(sd["seed"])
        self.n_refinements = int(sd["n_refinements"])
        self.n_noise = int(sd.get("n_noise", 0))
        if "config" in sd:
            self.config = McmcConfig(**sd["config"])

    # ---- helpers ----
    def _rows(self, t: Tensor, n: int, who: str) -> Tensor:
        t = t.to(device=self.model.device, dtype=torch.int32).contiguous()
        if t.numel() != n:
            raise ValueError(f"McmcStrategy.{who}: sources must hold {n} rows")
        return t

    def _workspace(self, n: int, n_draws: int) -> Tensor:
        need = int(L.load().qed_mcmc_workspace_bytes(n, n_draws))
        if need < 0:
            raise L.QedSplatError("qed_mcmc_workspace_bytes: bad arguments")
        if self._ws is None or self._ws.numel() < need or self._ws.device != self.model.device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.model.device)
        return self._ws


def sample(opacities: Tensor, n_draws: int, min_opacity: float = 0.0, seed: int = 0, counter: int = 0) -> Tensor:
    """The strategy's sampler on its own: int32 [n_draws] rows of ``opacities`` (logits, [N] or [N,1]) drawn with
    replacement in proportion to sigmoid(logit) among the rows above ``min_opacity``."""
    op = opacities.detach().reshape(-1).to(torch.float32).contiguous()
    n = op.numel()
    out = torch.empty(n_draws, dtype=torch.int32, device=op.device)
    lib = L.load()
    need = int(lib.qed_mcmc_workspace_bytes(n, n_draws))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=op.device)
    L.check(lib.qed_mcmc_sample(n, L.ptr(op), float(min_opacity), int(n_draws), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                int(counter), L.ptr(out), L.ptr(ws), ws.numel(), _stream()), "qed_mcmc_sample")
    return out
