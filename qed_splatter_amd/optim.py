"""The Adam optimisers of the Gaussians: ``FlatAdam`` (the fused training step's, over the model's flat parameter buffer)
and ``QedAdam`` (a ``torch.optim.Optimizer`` for one parameter group: what Nerfstudio's
``AdamOptimizerConfig(_target=QedAdam)`` builds), ``QedAdamSet`` (the QedAdam instances of one model seen as one optimiser
over the flat buffer) and the "means" rate schedule ``exponential_decay_lr``.  The update itself runs in adam.hip."""
from __future__ import annotations

import ctypes as C
import math
import weakref
from typing import Dict, Optional

import torch
from torch import Tensor

from . import _lib as L
from .binning import _workspace
from .parallel import exchange_state
from .rasterization import _stream
from .sh_grad import explicit_record


_RAW_GRAD = torch.Tensor.grad                 # the C-level descriptor: reads / writes the field without the subclass's hooks


def _raw_grad(p: Tensor) -> Optional[Tensor]:
    return _RAW_GRAD.__get__(p)


def _counted_step(opt, device) -> None:
    """Tell the device's workspace that ``opt`` has counted a step behind the current frame (see binning._Workspace.counted_step)."""
    if device.type == "cuda":
        _workspace(device).counted_step(opt)


def exponential_decay_lr(step: int, lr_init: float, lr_final: float, max_steps: int, warmup_steps: int = 0,
                         lr_pre_warmup: float = 0.0, ramp: str = "cosine") -> float:
    """Nerfstudio's ExponentialDecayScheduler (the schedule config.py:46-51 / :63-67 attach to "means" and
    "camera_opt"): log-linear from lr_init to lr_final over max_steps after an optional warm-up ramp."""
    if step < warmup_steps:
        if ramp == "cosine":
            return lr_pre_warmup + (lr_init - lr_pre_warmup) * math.sin(0.5 * math.pi * min(max(step / warmup_steps, 0), 1))
        return lr_pre_warmup + (lr_init - lr_pre_warmup) * step / warmup_steps
    t = min(max((step - warmup_steps) / (max_steps - warmup_steps), 0.0), 1.0)
    return math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t)


class FlatAdam:
    """Fused multi-tensor Adam over the model's flat parameter buffer, one learning rate per group
    (the six Gaussian groups of config.py:44-68, eps=1e-15) and the reference's exponential decay of
    the "means" rate (config.py:46-51).  SURVEY 8(f) rank 2."""

    MEANS_SCHEDULE = (1.6e-6, 30000)           # lr_final, max_steps (config.py:48-50)

    DEFAULT_LRS = {"means": 1.6e-4, "scales": 0.005, "quats": 0.001, "opacities": 0.05,
                   "features_dc": 0.0025, "features_rest": 0.0025 / 20}

    def __init__(self, model: "QEDSplatterModel", lrs: Optional[Dict[str, float]] = None, betas=(0.9, 0.999),
                 eps: float = 1e-15, means_schedule: Optional[tuple] = None):
        """``means_schedule=(lr_final, max_steps)`` turns on the exponential decay of the "means" rate
        (``FlatAdam.MEANS_SCHEDULE`` is the reference's); None keeps every rate constant."""
        self.model = model
        self.means_schedule = means_schedule
        lrs = {**self.DEFAULT_LRS, **(lrs or {})}
        self._means_lr_init = float(lrs["means"])
        self.lr = [float(lrs[n]) for n in model.group_names]
        self._lr = (C.c_float * len(self.lr))(*self.lr)
        self.betas, self.eps = betas, eps
        self.exp_avg = torch.zeros_like(model.flat_params)
        self.exp_avg_sq = torch.zeros_like(model.flat_params)
        self._flat_ref = model.flat_params         # (held: a freed buffer's address can be handed out again)
        self.t = 0
        # device-resident step state + learning rates: what a captured hipGraph replays against
        self.dev_state = torch.zeros(4, dtype=torch.float32, device=model.device)
        self.dev_lr = torch.zeros(8, dtype=torch.float32, device=model.device)
        self.dev_lr[:len(self.lr)] = torch.tensor(self.lr)
        _workspace(model.device).steppers.add(self)

    def on_skipped_step(self) -> None:
        """The device skipped the step this optimiser's host counter has already counted (the frame behind it overflowed its
        intersection buffer: binning._Workspace.poll_pending): take it back, so that the bias corrections of the host-counter path
        stay in step with the moments.  (The device-state path counts on the device, where the tick honours the skip.)
        Not in a data-parallel job: there the skip is collective (parallel.py) but only the rank whose frame overflowed
        hears of it on the host -- taking the step back here alone would make the replicas' bias corrections differ.  All
        ranks' host counters then run one ahead of the moments together; step with device_state=True for exact counts."""
        if exchange_state(self.model).skip is not None:
            return
        self.t = max(self.t - 1, 0)

    def take_tick(self):
        """The qed_adam_tick_t that lets ANOTHER launch of the step advance this optimiser's device step state
        (model.fused_loss(optimizer=...): the loss pass's fold launch does it); the next
        ``step(device_state=True, fused_sh=True)`` then launches no tick of its own.  None while a tick is pending."""
        if getattr(self, "_ticked", False):
            return None
        i = self.model.group_names.index("means")
        t = L.AdamTick()
        t.dev_state, t.beta1, t.beta2 = self.dev_state.data_ptr(), self.betas[0], self.betas[1]
        t.skip_flag = self._skip()
        if self.means_schedule is not None:
            lr_final, max_steps = self.means_schedule
            t.dev_lr_slot = self.dev_lr[i:i + 1].data_ptr()
            t.lr_init, t.lr_final, t.max_steps = self._means_lr_init, float(lr_final), int(max_steps)
        else:
            t.dev_lr_slot, t.lr_init, t.lr_final, t.max_steps = None, 0.0, 0.0, 0
        self._tick_struct, self._ticked = t, True               # (kept alive: the C call reads it through a pointer)
        return t

    def drop_tick(self) -> None:
        """Forget a tick handed out by take_tick() whose launch never happened (a failed graph capture, an exception
        between take_tick() and the loss launch)."""
        self._ticked = False

    def _skip(self) -> int:
        """``skip_flag`` of the Adam entry points: the binning overflow word of this device (a frame whose intersection
        list overflowed renders empty; a step enqueued behind it without a host round trip must be a no-op)."""
        # data parallel: the MAXIMUM of the ranks' words, so that every replica skips the same steps (parallel.py)
        dp = exchange_state(self.model).skip
        if dp is not None:
            return dp.data_ptr()
        return _workspace(self.model.device).skip_flag_ptr()

    # ---- checkpointing (config.py:29 steps_per_save: the trainer saves every optimiser's state_dict) ----
    def state_dict(self) -> Dict:
        return {"t": self.t, "lr": list(self.lr), "betas": tuple(self.betas), "eps": self.eps,
                "means_schedule": self.means_schedule, "means_lr_init": self._means_lr_init,
                "exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(),
                "dev_state": self.dev_state.clone(), "dev_lr": self.dev_lr.clone(), "numel": self.exp_avg.numel()}

    def load_state_dict(self, sd: Dict) -> None:
        if int(sd["numel"]) != self.model.flat_params.numel():
            raise ValueError(f"FlatAdam.load_state_dict: the checkpoint holds moments for {sd['numel']} parameters, the "
                             f"model has {self.model.flat_params.numel()} (load the model's Gaussians first)")
        self._check("load_state_dict", compact_ok=True)
        self.t = int(sd["t"])
        self.betas, self.eps = tuple(sd["betas"]), float(sd["eps"])
        self.means_schedule, self._means_lr_init = sd["means_schedule"], float(sd["means_lr_init"])
        for i, lr in enumerate(sd["lr"]):
            self._set_host_lr(i, lr)
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.dev_state.copy_(sd["dev_state"])
        self.dev_lr.copy_(sd["dev_lr"])
        self._ticked = False

    def set_lr(self, name: str, lr: float) -> None:
        i = self.model.group_names.index(name)
        self._set_host_lr(i, lr)
        self.dev_lr[i] = float(lr)

    def _set_host_lr(self, i: int, lr: float) -> None:
        """Group ``i``'s host rate: ``lr`` and the ctypes copy ``_lr`` that the host-state launches read."""
        self.lr[i] = self._lr[i] = float(lr)

    def _schedule_means_lr(self) -> None:
        """The host rate of "means" for the step about to be taken (the schedule at the current step count)."""
        lr_final, max_steps = self.means_schedule
        self._set_host_lr(self.model.group_names.index("means"),
                          exponential_decay_lr(self.t, self._means_lr_init, lr_final, max_steps))

    def rebind(self, exp_avg: Tensor, exp_avg_sq: Tensor) -> None:
        """Adopt new moment buffers after the model adopted a new flat parameter buffer (densification);
        the step count carries on, as torch.optim.Adam's per-parameter ``step`` does in the reference."""
        assert exp_avg.numel() == self.model.flat_params.numel() == exp_avg_sq.numel()
        self.exp_avg, self.exp_avg_sq = exp_avg, exp_avg_sq
        self._flat_ref = self.model.flat_params

    def _check(self, who: str, compact_ok: bool = False) -> None:
        """Refuse to train on garbage: moments of a flat buffer the model has left (model.to() / densification without
        rebind(); the group begins are ``model.layout``'s at every launch), or compact SH gradients consumed by a plain step."""
        m = self.model
        if m.flat_params is not self._flat_ref or m.flat_params.device != self.exp_avg.device:
            raise RuntimeError(f"FlatAdam.{who}: the model adopted a new flat parameter buffer (model.to() or "
                               "densification); call rebind(exp_avg, exp_avg_sq) or build a new optimiser")
        if not compact_ok and explicit_record(m) is not None:
            raise RuntimeError(f"FlatAdam.{who}: the last backward wrote compact SH gradients "
                               "(fused_loss(compact_sh_grad=True)); step with fused_sh=True")

    # ---- one step in pieces: lets a data-parallel job update a range of the flat buffer as soon as that
    # range of the gradient has been all-reduced, while later ranges are still on the wire ----
    @torch.no_grad()
    def begin_step(self) -> None:
        """Advance the (host-side) step counter and the scheduled rates; follow with step_range() calls that
        together cover [0, numel)."""
        if self.means_schedule is not None:
            self._schedule_means_lr()
        self.t += 1
        _counted_step(self, self.model.device)

    @torch.no_grad()
    def step_range(self, lo: int, hi: int) -> None:
        """Adam update of flat elements [lo, hi) (lo a multiple of 4) with the current step count."""
        assert 0 <= lo <= hi <= self.model.flat_params.numel() and lo % 4 == 0
        if hi == lo:
            return
        self._check("step_range")
        g = self.model.flat_grad()
        p = self.model.flat_params
        L.check(L.load().qed_adam_step(L.ptr(p[lo:hi]), L.ptr(g[lo:hi]), L.ptr(self.exp_avg[lo:hi]),
                                       L.ptr(self.exp_avg_sq[lo:hi]), len(self.lr),
                                       C.cast(self.model.layout.clipped_begin(lo, hi), C.c_void_p),
                                       C.cast(self._lr, C.c_void_p), self.betas[0], self.betas[1], self.eps, self.t,
                                       self._skip(), _stream()), "qed_adam_step")

    @torch.no_grad()
    def step(self, device_state: bool = False, fused_sh: bool = False, part: int = 3) -> None:
        """One Adam step.  ``device_state=True`` keeps the step counter / bias corrections in device
        memory (qed_adam_step_dev), which is what makes the step replayable from a hipGraph.

        ``fused_sh=True`` (after ``fused_loss(..., compact_sh_grad=True)`` + backward): the 48 N SH-coefficient
        gradients are never written or read -- qed_adam_step_sh evaluates b_k(dir) x colour gradient while it
        updates features_dc / features_rest (one view: this rank's; data parallel: the views gathered by
        ``parallel.exchange_grads_compact(..., rebuild=False)``).  Same update as the plain step.

        ``part`` (fused_sh only): 1 = the step counter / schedule + the two SH groups (needs the gathered views, not the
        reduced geometry gradients), 2 = the leading groups, 3 = both.  A data-parallel step calls 1 then 2 around the
        wait for the geometry all-reduce (``parallel.exchange_grads_compact_begin``)."""
        assert part in (1, 2, 3) and (fused_sh or part == 3)
        m = self.model
        p = m.flat_params
        g = m.flat_grad()
        if g is None:
            return
        self._check("step", compact_ok=fused_sh)
        lib = L.load()
        sched = (-1, 0.0, 0.0, 0)
        if self.means_schedule is not None and (part & 1):      # the rate of the step about to be taken
            lr_final, max_steps = self.means_schedule
            i = self.model.group_names.index("means")
            if device_state and fused_sh:                        # evaluated by qed_adam_step_sh's own tick launch
                sched = (i, self._means_lr_init, float(lr_final), int(max_steps))
            elif device_state:
                L.check(lib.qed_lr_exp_decay_dev(L.ptr(self.dev_lr[i:i + 1]), L.ptr(self.dev_state), self._means_lr_init,
                                                 float(lr_final), int(max_steps), _stream()), "qed_lr_exp_decay_dev")
            else:
                self._schedule_means_lr()
        if part & 1:
            self.t += 1
            _counted_step(self, self.model.device)
        if fused_sh:
            rec = explicit_record(m)
            if rec is None:
                raise RuntimeError("fused_sh needs gradients from fused_loss(..., compact_sh_grad=True)")
            assert m.group_names[-2:] == ["features_dc", "features_rest"]
            if getattr(self, "_ticked", False) and (part & 1):       # take_tick(): the state is advanced already
                if not device_state:
                    raise RuntimeError("the device step state was advanced by fused_loss(optimizer=...): step with "
                                       "device_state=True")
                part, self._ticked = part | 4, False
            L.check(lib.qed_adam_step_sh(
                L.ptr(p), L.ptr(g), L.ptr(self.exp_avg), L.ptr(self.exp_avg_sq), len(self.lr),
                m.layout.c_begin_ptr, None if device_state else C.cast(self._lr, C.c_void_p),
                L.ptr(self.dev_lr) if device_state else None, self.betas[0], self.betas[1], self.eps, self.t,
                L.ptr(self.dev_state) if device_state else None, *sched, m.num_points, rec.deg, L.ptr(m.means),
                *rec.optimiser_views(g, m.group_begin).c_args(), int(part), self._skip(), _stream()), "qed_adam_step_sh")
            return
        if device_state:
            L.check(lib.qed_adam_step_dev(L.ptr(p), L.ptr(g), L.ptr(self.exp_avg), L.ptr(self.exp_avg_sq),
                                          len(self.lr), m.layout.c_begin_ptr, L.ptr(self.dev_lr),
                                          self.betas[0], self.betas[1], self.eps, L.ptr(self.dev_state), self._skip(),
                                          _stream()), "qed_adam_step_dev")
            return
        L.check(lib.qed_adam_step(L.ptr(p), L.ptr(g), L.ptr(self.exp_avg), L.ptr(self.exp_avg_sq),
                                  len(self.lr), m.layout.c_begin_ptr, C.cast(self._lr, C.c_void_p),
                                  self.betas[0], self.betas[1], self.eps, self.t, self._skip(), _stream()),
                "qed_adam_step")


class _SharedFlatState:
    """What the QedAdam instances of one model share: the moments over the whole flat buffer and this step's
    bookkeeping (which groups have called step(), with which rate)."""

    def __init__(self, flat: Tensor):
        self.flat_ptr = flat.data_ptr()
        self.numel = flat.numel()
        self.exp_avg = torch.zeros_like(flat)
        self.exp_avg_sq = torch.zeros_like(flat)
        self.members = weakref.WeakValueDictionary()   # flat offset -> optimiser instance
        self.pending: Dict[int, float] = {}            # flat offset -> lr of the step() call waiting to be launched
        self.t: Dict[int, int] = {}                    # flat offset -> steps taken


class QedAdamSet:
    """The per-group QedAdam instances of one model, seen as ONE optimiser over the flat buffer -- what
    ``densify.Densifier`` needs (it rewrites parameters and both Adam moments in one pass when the number of Gaussians
    changes, as the parent's dup_in_all_optim / remove_from_all_optim do group by group).

        optimizers = {name: QedAdam([model.gauss_params[name]], lr=..., eps=1e-15) for name in model.group_names}
        densifier = Densifier(model, QedAdamSet(model, optimizers), ...)
    """

    def __init__(self, model: "QEDSplatterModel", optimizers: Dict[str, "QedAdam"]):
        assert set(optimizers) >= set(model.group_names), "one QedAdam per parameter group"
        self.model, self.optimizers = model, optimizers

    def _state(self) -> _SharedFlatState:
        return self.optimizers[self.model.group_names[0]]._attach()

    @property
    def exp_avg(self) -> Tensor:
        return self._state().exp_avg

    @property
    def exp_avg_sq(self) -> Tensor:
        return self._state().exp_avg_sq

    def rebind(self, exp_avg: Tensor, exp_avg_sq: Tensor) -> None:
        """After ``model.rebind_flat``: point every instance at its new Parameter and adopt the new moments (the step
        counts carry on, as torch.optim.Adam's per-parameter ``step`` does in the reference)."""
        m = self.model
        old = self._state_or_none()
        steps = {}
        for name, beg in zip(m.group_names, m.group_begin):
            opt = self.optimizers[name]
            old_off = opt._param().storage_offset()
            steps[beg] = old.t.get(old_off, 0) if old is not None else 0
            opt.param_groups[0]["params"] = [m.gauss_params[name]]
            opt._shared = None
            opt.state.clear()                                    # (views of the old moments, keyed by the old Parameter)
        st = self._state()                                       # a fresh shared state over the new flat buffer
        assert exp_avg.numel() == st.numel == exp_avg_sq.numel()
        st.exp_avg, st.exp_avg_sq = exp_avg, exp_avg_sq
        st.t.update(steps)
        for opt in self.optimizers.values():                     # optimizer.state[param]: views of the adopted moments
            opt.state.clear()
            if opt._shared is st:
                opt._expose_views(st)

    def _state_or_none(self) -> Optional[_SharedFlatState]:
        return self.optimizers[self.model.group_names[0]]._shared


_FLAT_STATES: "weakref.WeakValueDictionary[int, _SharedFlatState]" = weakref.WeakValueDictionary()
_ALL_QED_ADAMS: "weakref.WeakSet[QedAdam]" = weakref.WeakSet()


def _all_groups_stepped_by_qed_adam(flat: Tensor, n_groups: int) -> bool:
    """Whether QedAdam instances step all ``n_groups`` groups of the flat buffer ``flat`` (one instance per group)."""
    st = _FLAT_STATES.get(flat.untyped_storage().data_ptr())
    return st is not None and len(st.members) == n_groups


def _skip_flag(device) -> int:
    return _workspace(device).skip_flag_ptr()


class QedAdam(torch.optim.Optimizer):
    """``torch.optim.Adam`` semantics (no weight decay, no amsgrad) for ONE parameter group of the Gaussians, as a
    ``torch.optim.Optimizer`` subclass: Nerfstudio's ``AdamOptimizerConfig(_target=QedAdam, lr=..., eps=1e-15)`` builds
    it unchanged for every group of config.py:44-68 and its schedulers / GradScaler / checkpointing keep working
    (``param_groups[0]["lr"]`` is read at every step).  Two layouts, told apart by the Parameter's storage:

    * **separately held Parameters** (what Nerfstudio's parent class keeps: six tensors in a ``ParameterDict``,
      model.py:12,50-58): the moments live in ``self.state[param]`` exactly as ``torch.optim.Adam`` keeps them
      (``step`` / ``exp_avg`` / ``exp_avg_sq``), so code that rewrites them when the number of Gaussians changes (the
      parent's dup / remove-from-optimiser routines, gsplat's strategies) works unchanged; every ``step()`` is one
      ``qed_adam_step`` launch over that tensor.
    * **views of ONE flat buffer** (this package's ``QEDSplatterModel``): the instances of one buffer find each other
      through a registry and the LAST one to be stepped launches a single ``qed_adam_step`` over the whole buffer with
      one rate per group (one pass at HBM speed instead of six times ~10 eager launches).  The shared moments are
      visible as VIEWS under ``self.state[param]``; replacing them there is refused with an error that names
      ``densify.Densifier`` / ``QedAdamSet`` (which rewrite parameters and moments in one pass).  A group that is
      stepped twice before the others, ``zero_grad()``, ``state_dict()`` or ``flush()`` update just the waiting groups'
      ranges -- so a group whose ``.grad`` is None in some iteration never delays the others past that iteration."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0):
        if weight_decay != 0.0:
            raise NotImplementedError("QedAdam: weight_decay is not used by the reference (config.py:44-68)")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        ps = [p for g in self.param_groups for p in g["params"]]
        if len(ps) != 1:
            raise ValueError("QedAdam steps one parameter group per instance "
                             "(Nerfstudio builds one optimiser per group name)")
        self._shared: Optional[_SharedFlatState] = None
        _ALL_QED_ADAMS.add(self)
        p0 = ps[0]
        if p0.is_cuda:
            _workspace(p0.device).steppers.add(self)

    # -- layout -----------------------------------------------------------------------------------------
    def _param(self) -> Tensor:
        return self.param_groups[0]["params"][0]

    @staticmethod
    def _is_flat_view(p: Tensor) -> bool:
        """A view into a larger allocation (the flat buffer) rather than a tensor that owns its storage."""
        return p.storage_offset() != 0 or p.untyped_storage().nbytes() > 4 * p.numel()

    @staticmethod
    def _require_gpu(p: Tensor) -> None:
        if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
            raise L.QedSplatError("QedAdam needs contiguous float32 GPU parameters (there is no CPU path)")

    def _attach(self) -> _SharedFlatState:
        p = self._param()
        base = p.untyped_storage().data_ptr()
        st = self._shared
        if st is not None and st.flat_ptr == base and self._views_intact(p):      # the steady state: nothing to do
            return st
        self._require_gpu(p)
        st = _FLAT_STATES.get(base)
        if st is None or self._shared is not st:
            if st is None:
                flat = torch.empty(0, dtype=torch.float32, device=p.device).set_(
                    p.untyped_storage(), 0, (p.untyped_storage().nbytes() // 4,))
                st = _SharedFlatState(flat)
                _FLAT_STATES[base] = st
                st._keepalive_flat = flat
            # every live instance whose Parameter is a view of this buffer is a member from the start: the fused
            # launch waits for all of them, whichever is stepped first
            for inst in list(_ALL_QED_ADAMS):
                q = inst._param()
                if q.is_cuda and q.untyped_storage().data_ptr() == base:
                    inst._shared = st
                    st.members[q.storage_offset()] = inst
                    st.t.setdefault(q.storage_offset(), 0)
        off = p.storage_offset()
        st.members[off] = self
        st.t.setdefault(off, 0)
        self._expose_views(st)
        return st

    def _views_intact(self, p: Tensor) -> bool:
        """``self.state[param]`` still holds the very view objects _expose_views put there (identity, no tensor calls)."""
        held = self.__dict__.get("_views")
        if held is None or held[0] is not p:
            return False
        cur = self.state.get(p)
        return cur is held[1] and cur.get("exp_avg") is held[2] and cur.get("exp_avg_sq") is held[3]

    def _expose_views(self, st: _SharedFlatState) -> None:
        """``self.state[param]`` in torch.optim.Adam's layout, as views of the shared moments."""
        p = self._param()
        if self._views_intact(p) and self._views[2].untyped_storage().data_ptr() == st.exp_avg.untyped_storage().data_ptr():
            return
        off, n = p.storage_offset(), p.numel()
        cur = self.state.get(p)
        m, v = st.exp_avg[off:off + n].view(p.shape), st.exp_avg_sq[off:off + n].view(p.shape)
        if cur is not None and len(cur) and "exp_avg" in cur:
            if cur["exp_avg"].data_ptr() == m.data_ptr() and cur["exp_avg_sq"].data_ptr() == v.data_ptr() \
                    and cur["exp_avg"].shape == p.shape:
                self._views = (p, cur, cur["exp_avg"], cur["exp_avg_sq"])
                return
            raise RuntimeError(
                "QedAdam: optimizer.state[param] of a flat-buffer group was replaced from outside (the parent class's "
                "dup / remove-from-optimiser routines do that).  With Parameters that are views of one flat buffer the "
                "number of Gaussians is changed by qed_splatter_amd.densify.Densifier(model, QedAdamSet(model, "
                "optimizers)), which rewrites parameters and both moments in one pass; or hold the six Parameters as "
                "separate tensors, in which case QedAdam keeps torch.optim.Adam's own per-parameter state.")
        entry = {"step": torch.tensor(float(st.t.get(off, 0))), "exp_avg": m, "exp_avg_sq": v}
        self.state[p] = entry
        self._views = (p, entry, m, v)

    # -- stepping ---------------------------------------------------------------------------------------
    # torch.optim.Optimizer wraps every subclass's step() in a profiler range + hook dispatch (~25 us of Python per call,
    # six calls per iteration on a route whose host cost is what bounds it).  `step.hooked = True` (below the class) tells
    # it not to; registered step hooks are honoured here, so the Optimizer contract stands.
    def step(self, closure=None):
        from torch.optim import optimizer as _O
        pre, post = self._optimizer_step_pre_hooks, self._optimizer_step_post_hooks
        if pre or post or _O._global_optimizer_pre_hooks or _O._global_optimizer_post_hooks:
            args, kwargs = (closure,), {}
            for hook in (*_O._global_optimizer_pre_hooks.values(), *pre.values()):
                result = hook(self, args, kwargs)
                if result is not None:
                    args, kwargs = result
            out = self._step(*args, **kwargs)
            for hook in (*post.values(), *_O._global_optimizer_post_hooks.values()):
                hook(self, args, kwargs)
            return out
        return self._step(closure)

    def _step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        p = self.param_groups[0]["params"][0]
        if _raw_grad(p) is None:               # (the field itself: a compact SH gradient is not materialised by asking)
            return loss
        with torch.no_grad():
            if p.storage_offset() == 0 and not self._is_flat_view(p):
                self._step_own(p)
                return loss
            st = self._attach()
            off = p.storage_offset()
            pending = st.pending
            if off in pending:                     # stepped twice before the others: launch what is waiting first
                self._launch(st, sorted(pending))
            pending[off] = float(self.param_groups[0]["lr"])
            if len(pending) == len(st.members):
                self._launch(st, sorted(pending))
        return loss

    def _step_own(self, p: Tensor) -> None:
        """A Parameter that owns its storage: torch.optim.Adam's state layout, one fused launch."""
        self._require_gpu(p)
        g = p.grad
        grp = self.param_groups[0]
        state = self.state[p]
        if len(state) == 0:
            state["step"] = torch.tensor(0.0)
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        m, v = state["exp_avg"], state["exp_avg_sq"]
        if m.shape != p.shape or v.shape != p.shape:
            raise RuntimeError(f"QedAdam: the moments in optimizer.state ({tuple(m.shape)}) do not match the parameter "
                               f"({tuple(p.shape)}): resize both when the number of Gaussians changes")
        if not (m.is_contiguous() and v.is_contiguous()):
            m = state["exp_avg"] = m.contiguous()
            v = state["exp_avg_sq"] = v.contiguous()
        state["step"] += 1
        _counted_step(self, p.device)
        t = int(state["step"])
        if g.dtype != torch.float32 or not g.is_contiguous():
            g = g.to(torch.float32).contiguous()
        beta1, beta2 = grp["betas"]
        if (p.data_ptr() | m.data_ptr() | v.data_ptr()) % 16 or g.data_ptr() % 4:
            raise L.QedSplatError("QedAdam: parameter / moment tensors must be 16-byte aligned")
        n = p.numel()
        h_begin = (C.c_int64 * 2)(0, n)
        h_lr = (C.c_float * 1)(float(grp["lr"]))
        L.check(L.load().qed_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 1,
                                       C.cast(h_begin, C.c_void_p), C.cast(h_lr, C.c_void_p), float(beta1), float(beta2),
                                       float(grp["eps"]), t, _skip_flag(p.device), _stream()), "qed_adam_step")

    def on_skipped_step(self) -> None:
        """See FlatAdam.on_skipped_step: the launch that this instance's last step() counted did nothing on the device."""
        p = self._param()
        if self._shared is not None and self._is_flat_view(p):
            st, off = self._shared, p.storage_offset()
            if st.t.get(off, 0) > 0:
                st.t[off] -= 1
                held = self.__dict__.get("_views")
                if held is not None:
                    held[1]["step"].fill_(float(st.t[off]))
            return
        state = self.state.get(p)
        if state and float(state["step"]) > 0:
            state["step"] -= 1

    def flush(self) -> None:
        """Launch the update of the groups that have called step() but are still waiting for the others."""
        st = self._shared
        if st is not None and st.pending:
            self._launch(st, sorted(st.pending))

    def zero_grad(self, set_to_none: bool = True) -> None:
        # a waiting update reads .grad at launch time: launch it before the gradients go away (a group that skipped
        # this iteration -- .grad None, or a GradScaler that found an inf for that optimiser only -- must not hold the
        # others' update back into the next iteration's gradients).  One parameter: done here, without the base class's
        # generic (and, per call, several times costlier) walk over groups.
        st = self._shared
        if st is not None and st.pending:
            self._launch(st, sorted(st.pending))
        p = self.param_groups[0]["params"][0]
        g = _raw_grad(p)
        if g is not None:
            if set_to_none:
                p.grad = None                          # (through the subclass's setter: drops a compact form nobody read)
            else:
                if g.grad_fn is not None:
                    g.detach_()
                else:
                    g.requires_grad_(False)
                g.zero_()

    @staticmethod
    def _launch(st: _SharedFlatState, offs) -> None:
        lib = L.load()
        members = [st.members[o] for o in offs]
        ps = [m.param_groups[0]["params"][0] for m in members]
        for mem in members:
            _counted_step(mem, ps[0].device)
        # compact SH gradients (QEDSplatterModel, lazy_sh_grad): consumed as they are when this launch covers all six
        # groups in one run (below); any other launch first has the coefficient gradients written out
        owner = ps[-1].__dict__.get("_qed_owner")
        model = owner() if owner is not None else None
        lazy = model.__dict__.get("compact_sh") if model is not None else None
        if lazy is not None and not lazy.implicit:     # (the caller asked for that form: FlatAdam.step(fused_sh=True)'s)
            lazy = None
        if lazy is not None and len(offs) != len(st.members):
            model._materialise_sh_grads()
            lazy = None
        gs = [_raw_grad(p) for p in ps]
        for mem, p in zip(members, ps):
            if not mem._views_intact(p):
                mem._expose_views(st)          # (re-creates the views, or refuses moments that were replaced from outside)
        # maximal runs of groups that are adjacent in the flat buffer, share betas / eps / step count and whose
        # gradients are adjacent pieces of one allocation (what _ProjectSH.backward produces): one launch per run
        n_el = [p.numel() for p in ps]
        gptr = [g.data_ptr() for g in gs]
        keys = [m.defaults_key() for m in members]
        runs, cur = [], [0]
        for i in range(1, len(ps)):
            same = (offs[i] == offs[i - 1] + n_el[i - 1] and gptr[i] == gptr[i - 1] + 4 * n_el[i - 1]
                    and keys[i] == keys[i - 1] and st.t[offs[i]] == st.t[offs[i - 1]]
                    and gs[i].dtype == torch.float32 and gs[i].is_contiguous() and gs[i - 1].is_contiguous())
            if same:
                cur.append(i)
            else:
                runs.append(cur)
                cur = [i]
        runs.append(cur)
        stream = L.current_stream()
        skip = _skip_flag(ps[0].device)
        flat_ptr = st.flat_ptr
        m_ptr, v_ptr = st.exp_avg.data_ptr(), st.exp_avg_sq.data_ptr()
        if lazy is not None and not (len(runs) == 1 and offs[0] == 0 and gptr[0] % 16 == 0
                                     and gs[0].is_contiguous() and gs[0].dtype == torch.float32):
            model._materialise_sh_grads()              # (the six groups do not form one run: plain gradients, then)
            lazy = None
        for run in runs:
            first, last = run[0], run[-1]
            lo, hi = offs[first], offs[last] + n_el[last]
            g = gs[first]
            grp = members[first].param_groups[0]
            beta1, beta2 = grp["betas"]
            eps = grp["eps"]
            t = st.t[offs[first]] + 1
            if lo % 4 != 0 or gptr[first] % 4 != 0 or not g.is_contiguous() or g.dtype != torch.float32:
                # a lone group whose range is not 16-byte aligned (only when the groups are stepped out of step with
                # each other and N is not a multiple of 4): the same update with eager torch ops
                for i in run:
                    o, n = offs[i], n_el[i]
                    gi = gs[i].reshape(-1).to(torch.float32)
                    m, v = st.exp_avg[o:o + n], st.exp_avg_sq[o:o + n]
                    m.mul_(beta1).add_(gi, alpha=1 - beta1)
                    v.mul_(beta2).addcmul_(gi, gi, value=1 - beta2)
                    denom = (v.sqrt() / math.sqrt(1 - beta2 ** t)).add_(eps)
                    ps[i].data.reshape(-1).addcdiv_(m, denom, value=-st.pending[offs[i]] / (1 - beta1 ** t))
                    st.t[offs[i]] = t
                    members[i].state[ps[i]]["step"].fill_(float(t))
                continue
            k = len(run)
            h_begin = (C.c_int64 * (k + 1))(*[offs[i] - lo for i in run], hi - lo)
            h_lr = (C.c_float * k)(*[st.pending[offs[i]] for i in run])
            if lazy is not None:
                # the fused step's optimiser launches: the SH groups from the colour gradient + the view (before the means
                # move), then the leading groups.  The two fields are emptied: the compact form is used up
                L.check(lib.qed_adam_step_sh(
                    flat_ptr, gptr[first], m_ptr, v_ptr, k, C.cast(h_begin, C.c_void_p), C.cast(h_lr, C.c_void_p), None,
                    float(beta1), float(beta2), float(eps), t, None, -1, 0.0, 0.0, 0, lazy.n, lazy.deg,
                    flat_ptr + 4 * offs[0], *lazy.optimiser_views().c_args(), 3, skip, stream), "qed_adam_step_sh")
                model.__dict__["compact_sh"] = None
                _RAW_GRAD.__set__(ps[-1], None)
                _RAW_GRAD.__set__(ps[-2], None)
                lazy = None
            else:
                L.check(lib.qed_adam_step(flat_ptr + 4 * lo, gptr[first], m_ptr + 4 * lo, v_ptr + 4 * lo, k,
                                          C.cast(h_begin, C.c_void_p), C.cast(h_lr, C.c_void_p), float(beta1), float(beta2),
                                          float(eps), t, skip, stream), "qed_adam_step")
            ft = float(t)
            for i in run:
                st.t[offs[i]] = t
                members[i]._views[1]["step"].fill_(ft)
        st.pending.clear()

    def defaults_key(self):
        g = self.param_groups[0]
        return (tuple(g["betas"]), float(g["eps"]))

    step.hooked = True          # (see step(): torch.optim.Optimizer must not wrap it again)

    # -- checkpointing: torch.optim.Adam's layout in both cases ------------------------------------------
    def state_dict(self):
        self.flush()
        p = self._param()
        if not self._is_flat_view(p):
            return super().state_dict()
        sd = super().state_dict()
        st = self._shared
        if st is not None:
            # copies of this group's slice (a view would drag the whole flat buffer into the checkpoint)
            off, n = p.storage_offset(), p.numel()
            sd["state"] = {0: {"step": torch.tensor(float(st.t.get(off, 0))),
                               "exp_avg": st.exp_avg[off:off + n].view(p.shape).clone(),
                               "exp_avg_sq": st.exp_avg_sq[off:off + n].view(p.shape).clone()}}
        return sd

    def load_state_dict(self, state_dict):
        p = self._param()
        if not self._is_flat_view(p):
            super().load_state_dict(state_dict)
            stt = self.state.get(p)
            if stt is not None and "step" in stt and torch.is_tensor(stt["step"]):
                stt["step"] = stt["step"].detach().to("cpu", torch.float32).reshape(())    # host counter, as created
            return
        state = state_dict.get("state", {})
        super().load_state_dict({"state": {}, "param_groups": state_dict["param_groups"]})
        st = self._attach()
        if state:
            off, n = p.storage_offset(), p.numel()
            s0 = state[0] if 0 in state else next(iter(state.values()))
            st.exp_avg[off:off + n] = s0["exp_avg"].reshape(-1).to(st.exp_avg)
            st.exp_avg_sq[off:off + n] = s0["exp_avg_sq"].reshape(-1).to(st.exp_avg_sq)
            st.t[off] = int(s0["step"])
            self.state[p]["step"].fill_(float(st.t[off]))
