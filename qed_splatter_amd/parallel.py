"""Camera-sharded data parallelism: one process per GPU, every rank holds the
full Gaussian set and renders its own camera; after backward ONE collective averages the flat
59 N-float gradient buffer (RCCL over xGMI; `nccl` backend == RCCL on ROCm), then every rank takes the
identical fused Adam step.  The reference itself is single-GPU, one camera per step
(/root/reference/qed_splatter/model.py:210-212); there is no collective to translate.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from .sh_grad import SHViews, explicit_record

# Rehearsal hook (bench.py QED_BENCH_RCCL_SELF=1, tests): issue the collectives even in a process group of ONE rank, so
# that a one-GPU box drives the real RCCL calls (AVG all-reduce, all_gather_into_tensor, async works waited on the
# compute stream) of the N > 1 path.  Off in production: a single rank has nothing to exchange.
FORCE_COLLECTIVES = False


def _single(world_size: int) -> bool:
    return world_size <= 1 and not FORCE_COLLECTIVES


class ExchangeState:
    """What the exchanges keep per model from call to call (``exchange_state(model)``)."""

    __slots__ = ("dense", "sparse", "skip", "early", "early_work")

    def __init__(self):
        # (send [row], receive [ranks, row]) of the dense and of the sparse message: persistent, so that captured graphs
        # keep reading the right memory
        self.dense = self.sparse = None
        # int32[1], the MAXIMUM of the ranks' overflow words, which the optimiser launches of a data-parallel step take as
        # ``skip_flag`` (FlatAdam._skip); None: the optimiser takes the device's own overflow word
        self.skip = None
        self.early, self.early_work = False, None    # early_gather: the message is packed; its gather in flight, if any

    @staticmethod
    def fitting(pair, row: int, n_rows: int, device):
        """``pair`` if it still is (send [row], receive [n_rows, row]) on ``device``, else a new pair (zeroed)."""
        if pair is None or pair[0].numel() != row or pair[1].shape != (n_rows, row) or pair[0].device != device:
            pair = (torch.zeros(row, dtype=torch.float32, device=device),               # (the row's padding stays 0)
                    torch.zeros(n_rows, row, dtype=torch.float32, device=device))
        return pair

    def skip_word(self, device) -> torch.Tensor:
        """The persistent skip word.  A rank whose frame overflowed renders it empty and skips its update on the device;
        unless its peers skip the same step, the replicas' parameters, moments and step counters part for good (per-rank
        cameras make the list length rank dependent, so an overflow need not hit every rank in the same step)."""
        if self.skip is None or self.skip.device != device:
            self.skip = torch.zeros(1, dtype=torch.int32, device=device)
        return self.skip


def exchange_state(model) -> ExchangeState:
    st = model.__dict__.get("_exchange")
    if st is None:
        st = model.__dict__["_exchange"] = ExchangeState()
    return st


def _gather_rows(recv: torch.Tensor, send: torch.Tensor, group, async_op: bool = False):
    """Every rank's ``send`` row into ``recv`` [ranks, row]; the work handle when ``async_op``."""
    if dist.get_backend(group) == "nccl":
        return dist.all_gather_into_tensor(recv.view(-1), send, group=group, async_op=async_op)
    return dist.all_gather(list(recv.unbind(0)), send, group=group, async_op=async_op)       # gloo (rehearsal / CPU tests)


def _average(t: torch.Tensor, world_size: int, group, async_op: bool = False):
    """All-reduce ``t`` towards its average over the ranks: (work handle when ``async_op``, factor still to apply)."""
    if dist.get_backend(group) == "nccl":
        return dist.all_reduce(t, op=dist.ReduceOp.AVG, group=group, async_op=async_op), 1.0    # ncclAvg: no scaling pass
    return dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group, async_op=async_op), 1.0 / max(world_size, 1)  # gloo: no AVG


def allreduce_flat_grad(model, world_size: int, group=None) -> torch.Tensor:
    """Average the model's six parameter gradients across ranks with a single all-reduce.

    The gradients already alias one contiguous allocation (``model.flat_grad()``), so nothing is
    packed or copied.  Loss is normalised by the global camera count, i.e. gradients are averaged.
    """
    g, _ = _checked_grad(model, "allreduce_flat_grad", compact=False)
    if _single(world_size):
        exchange_state(model).skip = None
        return g
    collective_skip_flag(model, world_size, group)
    _, factor = _average(g, world_size, group)
    if factor != 1.0:
        g.mul_(factor)
    return g


def _refuse_camera_optimizer(model, who: str) -> None:
    """A data-parallel step behind fused_loss(camera_optimizer=...): every rank renders another camera and would step
    another row of pose_adjustment from its own gradient; the rows and their Adam state are not exchanged."""
    ctx = model.__dict__.get("_step")                # (model.StepContext: what the last forward call ran with)
    if ctx is not None and ctx.pose_optimizer is not None:
        raise NotImplementedError(f"{who}: the last fused_loss ran with a camera optimiser; pose optimisation under data "
                                  "parallelism is not supported")
    if ctx is not None and ctx.grid_optimizer is not None:
        raise NotImplementedError(f"{who}: the last fused_loss ran with a bilateral-grid optimiser; every rank would step "
                                  "the grids from its own frame, and neither they nor their Adam state are exchanged")
    if ctx is not None and getattr(ctx, "normal_loss", False):
        raise NotImplementedError(f"{who}: the last step carried the normal loss (config.use_normal_loss); the exchanges "
                                  "know the colour pass's gradient records only, not the normal pass's")
    if ctx is not None and getattr(ctx, "normal_reg", False):
        raise NotImplementedError(f"{who}: the last step carried the normal consistency or smoothness term "
                                  "(config.use_normal_consistency / use_normal_tv); the exchanges know the colour pass's "
                                  "gradient records only, not the normal pass's")
    if ctx is not None and getattr(ctx, "depth_distortion", False):
        raise NotImplementedError(f"{who}: the last step carried the depth distortion term "
                                  "(config.depth_distortion_lambda); the exchanges know the colour pass's gradient records "
                                  "only, not the rows that term merges into them")


def _checked_grad(model, who: str, compact: bool):
    """(flat gradient, compact record | None) for the exchange ``who``.  After fused_loss(compact_sh_grad=True) features_dc.grad
    holds colour gradients and features_rest.grad is unwritten memory: only exchange_grads_compact* / FlatAdam.step(fused_sh=
    True) may consume them (``compact``), and they consume nothing else."""
    _refuse_camera_optimizer(model, who)
    g = model.flat_grad()
    if g is None:
        raise RuntimeError(f"no gradients to {'exchange' if compact else 'reduce'}: call backward() first")
    rec = explicit_record(model)
    if compact and rec is None:
        raise RuntimeError(f"{who} needs gradients from fused_loss(..., compact_sh_grad=True)")
    if rec is not None and not compact:
        raise RuntimeError(f"{who}: the last backward wrote compact SH gradients (fused_loss(compact_sh_grad=True)); "
                           "use exchange_grads_compact() / FlatAdam.step(fused_sh=True), or render without the flag")
    return g, rec


def exchange_grads_compact(model, world_size: int, group=None, views=None, rebuild: bool = True) -> torch.Tensor:
    """Data-parallel gradient exchange that moves ~2.6x fewer bytes than all-reducing the flat gradient.

    The 48 SH-coefficient gradients of a Gaussian are b_k(direction to the camera) x (3 colour gradients): a
    rank-1 product per view.  After ``model.fused_loss(..., compact_sh_grad=True)`` + backward, this
      1. all-reduces (AVG) the 11 N geometry floats (means, scales, quats, opacities),
      2. all-gathers ONE message per rank: its 3 N clamp-masked colour gradients + its 4x4 view matrix,
      3. rebuilds the averaged features_dc / features_rest gradients locally (qed_sh_grad_from_views),
    leaving ``model.flat_grad()`` exactly as ``allreduce_flat_grad`` would (up to fp32 summation order).
    At 8 ranks / 500 k Gaussians a rank receives 42 + 19 MB instead of moving 206 MB.

    ``views`` (tests): a list of (colour-gradient [N,3], viewmat [1,4,4]) pairs standing in for the gather.

    ``rebuild=False`` skips step 3 and leaves the gathered views in ``model.compact_sh.views`` for
    ``FlatAdam.step(fused_sh=True)``, which evaluates the coefficient gradients inside the optimiser pass
    (the message buffers are persistent, so a captured Adam graph keeps reading the right memory)."""
    g, rec = _checked_grad(model, "exchange_grads_compact", compact=True)
    state = exchange_state(model)
    n_rows = len(views) if views is not None else max(world_size, 1)
    geo, send, recv, nv, row = _compact_buffers(model, g, n_rows)
    if views is not None:
        for c, (v, m) in enumerate(views):
            recv[c, :nv] = v.reshape(-1)
            recv[c, nv:nv + 16] = m.reshape(-1)
        state.skip = None
    elif not _single(world_size):
        _, factor = _average(geo, world_size, group)
        if factor != 1.0:
            geo.mul_(factor)
        _gather_rows(recv, send, group)
        _fold_skip_words(model, recv, nv)
    else:
        recv = send.view(1, row)
        state.skip = None
    rec.views = SHViews.rows(recv, nv)
    if rebuild:
        rec.write_out(model, g)                    # the flat gradient is complete again
    return g


class CompactExchange:
    """The two collectives of ``exchange_grads_compact_begin`` in flight.  ``wait_views()`` makes the current stream
    wait for the gathered colour gradients (what the SH part of the optimiser reads), ``wait_geometry()`` for the
    averaged geometry gradients (what the leading groups read)."""

    def __init__(self, gather, reduce, geo, scale_after: float, fold=None):
        self._gather, self._reduce, self._geo, self._scale_after, self._fold = gather, reduce, geo, scale_after, fold

    def wait_views(self) -> None:
        if self._gather is not None:
            self._gather.wait()
            self._gather = None
            if self._fold is not None:          # the ranks' overflow words -> the step's collective skip flag
                self._fold()

    def wait_geometry(self) -> None:
        if self._reduce is not None:
            self._reduce.wait()
            self._reduce = None
            if self._scale_after != 1.0:                          # gloo has no AVG
                self._geo.mul_(self._scale_after)


class early_gather:
    """Context manager: while it is active, the backward pass of ``model.fused_loss(..., compact_sh_grad=True)`` issues the
    all-gather of the colour-gradient message ITSELF, between the compositing backward and the projection backward
    (a hook registered for THIS model in rasterization.PRE_PROJECT_BWD): the message is K7's colour gradient under the forward pass's clamp mask
    (qed_pack_color_grad) -- exactly what the projection backward would write -- so the 6 MB per rank are on the links
    while the projection backward (~30 us at 500 k Gaussians) runs.  ``exchange_grads_compact_begin`` then finds the
    gather in flight and only adds the geometry all-reduce.

        with early_gather(model, world):
            model.backward_fused(losses)
        ex = exchange_grads_compact_begin(model, world)
        ...
    """

    def __init__(self, model, world_size: int, group=None):
        self.model, self.world_size, self.group = model, world_size, group

    def _hook(self, vsplat, sh_jac, total):
        from . import _lib as L
        m = self.model
        N = m.num_points
        assert total == N, "one camera per rank in the data-parallel exchange"
        dev = vsplat.device
        nv, row = 3 * N, 3 * N + 16 + 4
        state = exchange_state(m)
        send, recv = state.dense = state.fitting(state.dense, row, max(self.world_size, 1), dev)
        L.check(L.load().qed_pack_color_grad(total, L.ptr(vsplat), L.ptr(sh_jac), L.ptr(send),
                                             torch.cuda.current_stream().cuda_stream), "qed_pack_color_grad")
        send[nv:nv + 16] = m.compact_sh.viewmat.reshape(-1).to(torch.float32)
        send[nv + 16:nv + 17].view(torch.int32).copy_(_local_overflow_word(dev))
        state.early = True
        state.early_work = None if _single(self.world_size) else _gather_rows(recv, send, self.group, async_op=True)

    def __enter__(self):
        from . import rasterization as R
        self._key = self.model.means.untyped_storage().data_ptr()       # this model's hook only (rasterization.PRE_PROJECT_BWD)
        self._prev = R.PRE_PROJECT_BWD.get(self._key)
        R.PRE_PROJECT_BWD[self._key] = self._hook
        exchange_state(self.model).early = False
        return self

    def __exit__(self, *exc):
        from . import rasterization as R
        if self._prev is None:
            R.PRE_PROJECT_BWD.pop(self._key, None)
        else:
            R.PRE_PROJECT_BWD[self._key] = self._prev
        return False


def backward_with_early_gather(model, losses, world_size: int, group=None) -> None:
    """``model.backward_fused(losses)`` in two phases run from THIS thread, with the colour-gradient all-gather issued
    between them: (1) the loss's and the compositing backward (autograd.grad up to the projected splats), (2) pack the
    message from K7's rows + launch the all-gather, (3) the projection backward.  Same gradients as backward_fused; the
    6 MB per rank are on the links while the projection backward runs.

    Why not simply from a hook inside ONE backward pass (``early_gather``): the autograd engine runs the nodes on its own
    worker thread, and ProcessGroupNCCL decides by the CALLING thread's stream state whether a collective is being
    captured into a graph -- issued from the worker thread during a capture, its work object reaches the watchdog, which
    queries an event recorded on a capturing stream (hipErrorCapturedEvent) and aborts the process.  From the capturing
    thread itself the collectives are captured (bench.py --dp-one-graph)."""
    from .losses import _unit_grad
    from .rasterization import _VSPLAT_REGISTRY
    info = model.info
    names = ("means2d", "conics", "colors", "opacities", "depths")
    inter = [info[k] for k in names]
    node = inter[0].grad_fn                                        # _ProjectSH's backward node: its saved tensors hold sh_jac
    loss = losses["loss"]
    g = torch.autograd.grad(loss, inter, grad_outputs=_unit_grad(loss.device), allow_unused=True)
    vsplat = _VSPLAT_REGISTRY.get(g[0].untyped_storage().data_ptr())
    from .rasterization import _ProjectSH
    sh_jac = _ProjectSH.saved(node, "sh_jac")
    eg = early_gather(model, world_size, group)
    exchange_state(model).early = False
    if vsplat is not None and sh_jac is not None and explicit_record(model) is not None:
        eg._hook(vsplat, sh_jac, vsplat.shape[0])
    keep = [(t, gi) for t, gi in zip(inter, g) if gi is not None]
    torch.autograd.backward([t for t, _ in keep], [gi for _, gi in keep])


# ---- sparse colour-gradient message -------------------------------------------------------------------------------------
# The colour gradient of a Gaussian that a rank's camera does not see (radii == 0) is zero, so a rank need only send the
# rows it has: (index, 3 floats) per VISIBLE Gaussian = 16 B against 12 B per Gaussian of the dense message.  In SURVEY
# 8d's synthetic scene 95 % are visible (the dense form is smaller); a camera of a real capture sees a fraction of the
# scene, and xGMI links, not HBM, bound the exchange.  The message is capacity-bounded like the intersection list: ``cap``
# rows (agreed by all ranks at set-up: sparse_message_capacity), a rank with more visible rows than that marks the step as
# overflowed -- the word every rank's optimiser takes as skip_flag -- and the caller re-calibrates.  Row layout (floats):
#   [0:16] view matrix | [16] overflow word (int32 bits) | [17] visible rows (int32 bits) | [18:20] pad |
#   [20 : 20 + cap] indices (int32 bits) | [20 + cap : 20 + 4 cap] colour gradients
# The receiver scatters the R lists into the dense [R, 3 N + 20] rows the optimiser pass reads (SHViews.rows), header behind the
# colours as in the dense message, so nothing downstream changes.  Plain torch ops without a host read: the same code runs
# on CPU tensors in the gloo tests and on the GPU inside a captured graph.
SPARSE_HEADER = 20


def sparse_row_floats(cap: int) -> int:
    return SPARSE_HEADER + 4 * int(cap)


def sparse_message_capacity(model, world_size: int, group=None, headroom: float = 1.5, visible=None):
    """Set-up time (one host read, one MAX all-reduce): the row capacity every rank will use, or None when the dense
    message is no larger (capacity >= 3/4 N: 16 B per visible row against 12 B per Gaussian)."""
    vis = _visible_rows(model, visible)
    n = vis.numel()
    count = vis.sum().to(torch.int64).reshape(1)
    if not _single(world_size):
        dist.all_reduce(count, op=dist.ReduceOp.MAX, group=group)
    cap = min(n, max(4, (int(int(count) * headroom) + 3) // 4 * 4))          # (a multiple of 4: the row's parts stay 16-byte aligned)
    return None if 4 * cap >= 3 * n else cap


def _visible_rows(model, visible=None) -> torch.Tensor:
    if visible is not None:
        return visible.reshape(-1)
    return (model.info["radii"][0] > 0).reshape(-1)


def pack_sparse_message(v_color: torch.Tensor, visible: torch.Tensor, viewmat: torch.Tensor, overflow_word: torch.Tensor,
                        cap: int, out: torch.Tensor) -> None:
    """This rank's sparse row (layout above) into ``out`` [20 + 4 cap].  ``v_color`` [N,3] or [3 N]; ``visible`` [N] bool.
    A rank with more than ``cap`` visible rows sends the first ``cap`` and raises its overflow word to the count it needed."""
    n = visible.numel()
    vis = visible.reshape(-1)
    pos = torch.cumsum(vis.to(torch.int32), 0, dtype=torch.int32) - 1          # position of a visible row in the list
    count = pos[-1:] + 1 if n > 0 else torch.zeros(1, dtype=torch.int32, device=out.device)
    keep = vis & (pos < cap)
    dst = torch.where(keep, pos, torch.full_like(pos, cap)).to(torch.int64)     # (slot `cap` takes what is not sent)
    idx_buf = torch.zeros(cap + 1, dtype=torch.int32, device=out.device)
    rgb_buf = torch.zeros(cap + 1, 3, dtype=torch.float32, device=out.device)
    idx_buf.scatter_(0, dst, torch.arange(n, dtype=torch.int32, device=out.device))
    rgb_buf.index_copy_(0, dst, v_color.reshape(n, 3).to(torch.float32)) if n > 0 else None
    out[:16] = viewmat.reshape(-1).to(torch.float32)
    over = torch.where(count > cap, count, torch.zeros_like(count))
    out[16:17].view(torch.int32).copy_(torch.maximum(overflow_word.reshape(1).to(torch.int32), over))
    out[17:18].view(torch.int32).copy_(count)
    out[18:20] = 0.0
    out[SPARSE_HEADER:SPARSE_HEADER + cap].view(torch.int32).copy_(idx_buf[:cap])
    out[SPARSE_HEADER + cap:].copy_(rgb_buf[:cap].reshape(-1))


def unpack_sparse_messages(rows: torch.Tensor, n: int, cap: int, dense: torch.Tensor) -> None:
    """The gathered sparse rows [R, 20 + 4 cap] -> dense [R, 3 n + 20]: colour gradients scattered to their Gaussians (zero
    elsewhere), then the 20 header floats (view matrix, overflow word, count) as in the dense message."""
    R = rows.shape[0]
    nv = 3 * n
    dense[:, :nv] = 0.0
    counts = rows[:, 17:18].view(torch.int32).clamp(max=cap)                                     # [R,1]
    idx = rows[:, SPARSE_HEADER:SPARSE_HEADER + cap].view(torch.int32).to(torch.int64)           # [R,cap]
    rgb = rows[:, SPARSE_HEADER + cap:].reshape(R, cap, 3)
    live = torch.arange(cap, device=rows.device).reshape(1, cap) < counts                       # rows beyond the count: unset
    body = torch.zeros(R, n + 1, 3, dtype=torch.float32, device=rows.device)                     # (slot n takes the dead rows)
    dst = torch.where(live, idx, torch.full_like(idx, n))
    body.scatter_(1, dst.unsqueeze(-1).expand(R, cap, 3), rgb)
    dense[:, :nv] = body[:, :n].reshape(R, nv)
    dense[:, nv:nv + SPARSE_HEADER] = rows[:, :SPARSE_HEADER]


def prepare_compact_message(model, world_size: int) -> None:
    """Assemble this rank's message (colour gradients, view matrix, overflow word) in the persistent send buffer.  What
    ``exchange_grads_compact_begin`` does first; as a call of its own it can be CAPTURED at the end of the forward+backward
    graph (three small launches that then cost graph nodes, not eager dispatches) -- pass ``prepared=True`` to the exchange."""
    g, _ = _checked_grad(model, "prepare_compact_message", compact=True)
    _compact_buffers(model, g, max(world_size, 1), fill=True)


def fold_skip_words(model) -> None:
    """The gathered overflow words -> the collective skip word (``exchange_grads_compact_begin(..., fold=False)`` leaves
    this to the caller, who can capture it in front of the optimiser launches that read the flag)."""
    send, recv = exchange_state(model).dense
    _fold_skip_words(model, recv, send.numel() - 20)


def exchange_grads_compact_begin(model, world_size: int, group=None, prepared: bool = False,
                                 fold: bool = True, sparse_cap=None, visible=None) -> CompactExchange:
    """``exchange_grads_compact(..., rebuild=False)`` with both collectives left in flight, the all-gather of the
    colour gradients FIRST: the SH part of the optimiser (88 us at 500 k Gaussians, two thirds of the Adam pass) needs
    only that message and runs while the geometry all-reduce is still on the links:

        ex = exchange_grads_compact_begin(model, world)
        ex.wait_views();    optimizer.step(fused_sh=True, part=1)      # tick + features_dc / features_rest
        ex.wait_geometry(); optimizer.step(fused_sh=True, part=2)      # means, scales, quats, opacities

    xGMI is point to point, so the two messages share the same links and are issued back to back, not concurrently.
    Same result as exchange_grads_compact + step(fused_sh=True).

    ``prepared``: the message is in the send buffer already (prepare_compact_message, e.g. captured behind the backward
    pass).  ``fold=False``: the caller folds the gathered overflow words itself (fold_skip_words) after wait_views() and
    before the optimiser launches -- in a captured optimiser graph that is a graph node instead of an eager launch.

    ``sparse_cap`` (from sparse_message_capacity, the same on every rank): the all-gather carries only the rows of the
    Gaussians this rank's camera saw (index + colour gradient, at most ``sparse_cap`` of them); ``wait_views()`` scatters
    the gathered lists into the dense rows the optimiser reads.  Same ``compact_sh.views``, same update as the dense message
    (a Gaussian a rank did not see has a zero colour gradient there either way)."""
    g, rec = _checked_grad(model, "exchange_grads_compact_begin", compact=True)
    state, N, n_rows = exchange_state(model), model.num_points, max(world_size, 1)
    early, w_early = state.early, state.early_work
    state.early, state.early_work = False, None       # (the early gather belongs to ONE backward pass)
    sparse = sparse_cap is not None
    geo, send, recv, nv, row = _compact_buffers(model, g, n_rows, fill=not (early or prepared or sparse))
    dense, after_gather = recv, (lambda: _fold_skip_words(model, recv, nv)) if fold else None
    if sparse:
        # the all-gather carries the sparse rows; what the optimiser / fold_skip_words read stays the dense receive buffer
        cap = int(sparse_cap)
        send, recv = state.sparse = state.fitting(state.sparse, sparse_row_floats(cap), n_rows, g.device)
        pack_sparse_message(g[geo.numel():geo.numel() + nv], _visible_rows(model, visible), rec.viewmat,
                            _local_overflow_word(g.device), cap, send)

        def after_gather():
            unpack_sparse_messages(recv, N, cap, dense)
            if fold:
                _fold_skip_words(model, dense, nv)
    if _single(world_size):
        if sparse:
            recv[0].copy_(send)
            after_gather()
            state.skip_word(g.device)
        else:
            dense, state.skip = send.view(1, row), None
        rec.views = SHViews.rows(dense, nv)
        return CompactExchange(None, None, geo, 1.0)
    # (the backward pass may have issued the gather itself: early_gather)
    w_gather = w_early if early and not sparse else _gather_rows(recv, send, group, async_op=True)
    w_reduce, factor = _average(geo, world_size, group, async_op=True)
    rec.views = SHViews.rows(dense, nv)
    state.skip_word(g.device)                   # (exists before anything captures an optimiser launch that reads it)
    return CompactExchange(w_gather, w_reduce, geo, factor, fold=after_gather)


def _fold_skip_words(model, recv: torch.Tensor, nv: int) -> None:
    """The collective skip word = max over the gathered rows' overflow words (one small launch; the words are counts >= 0)."""
    words = recv[:, nv + 16:nv + 17].view(torch.int32)            # [ranks, 1]
    torch.amax(words, dim=0, out=exchange_state(model).skip_word(recv.device))


def _compact_buffers(model, g, n_rows: int, fill: bool = True):
    """(geometry slice of the flat gradient, this rank's message, the receive buffer, 3 N, message length): the
    message buffers are persistent, so captured graphs keep reading the right memory.  ``fill=False``: the message has been
    written already (early_gather)."""
    lo, hi = model.layout.span("features_dc")     # (the geometry groups lie ahead of it, features_rest behind it)
    geo, v_local = g[:lo], g[lo:hi]
    nv = v_local.numel()                                          # 3 N
    # one message per rank: colour gradients + view matrix + (bits of) this rank's intersection-overflow word (4 floats, so
    # that rows stay 16-byte aligned): the optimiser step is skipped on EVERY rank when ANY rank's frame overflowed
    row = nv + 16 + 4
    state = exchange_state(model)
    send, recv = state.dense = state.fitting(state.dense, row, n_rows, g.device)
    if fill:
        send[:nv] = v_local
        send[nv:nv + 16] = model.compact_sh.viewmat.reshape(-1).to(torch.float32)
        send[nv + 16:nv + 17].view(torch.int32).copy_(_local_overflow_word(g.device))
    return geo, send, recv, nv, row


def _local_overflow_word(device) -> torch.Tensor:
    """int32[1] view of this device's binning overflow word (non-zero: the frame just rendered overflowed its intersection
    buffer and is empty; what single-GPU optimiser launches take as ``skip_flag``)."""
    if device.type != "cuda":          # gloo rehearsals on CPU tensors (tests): no binning workspace; tests fill the word
        return _CPU_OVERFLOW_WORD
    from .binning import _workspace
    return _workspace(device).overflow_word


_CPU_OVERFLOW_WORD = torch.zeros(1, dtype=torch.int32)


def collective_skip_flag(model, world_size: int, group=None) -> torch.Tensor:
    """For the exchanges that gather no message (allreduce_flat_grad, allreduce_and_step): one MAX all-reduce of the
    overflow word into the collective skip word."""
    g = model.flat_grad()
    w = exchange_state(model).skip_word(g.device)
    w.copy_(_local_overflow_word(g.device))
    if not _single(world_size):
        dist.all_reduce(w, op=dist.ReduceOp.MAX, group=group)
    return w


def allreduce_and_step(model, optimizer, world_size: int, n_chunks: int = 4, group=None) -> None:
    """Gradient all-reduce and Adam step, pipelined: the flat gradient is reduced in ``n_chunks`` contiguous
    pieces issued back to back on the process group's stream, and each piece's range of the flat parameter
    buffer is updated (``FlatAdam.step_range``) as soon as its reduction has finished -- the HBM-bound
    optimiser pass hides behind the link-bound collectives of the later pieces.  Same result as
    ``allreduce_flat_grad`` + ``optimizer.step()``.

    Whether it pays depends on how RCCL's bus bandwidth falls off with message size on the node at hand:
    hiding the ~0.13 ms Adam pass of config B is worth it only if four 30 MB all-reduces cost less than
    0.13 ms more than one 118 MB all-reduce.  bench.py keeps the single collective (not measurable on the
    one-GPU development box); ``scripts/dp_rehearsal.py`` checks the equivalence on two ranks."""
    g, _ = _checked_grad(model, "allreduce_and_step", compact=False)
    total = g.numel()
    if _single(world_size):
        exchange_state(model).skip = None
        optimizer.begin_step()
        optimizer.step_range(0, total)
        return
    collective_skip_flag(model, world_size, group)
    n_chunks = max(1, min(int(n_chunks), total // 4 or 1))
    bounds = [min(total, (total * k // n_chunks) // 4 * 4) for k in range(n_chunks)] + [total]
    works = [_average(g[a:b], world_size, group, async_op=True) for a, b in zip(bounds[:-1], bounds[1:])]
    optimizer.begin_step()
    for (w, factor), a, b in zip(works, bounds[:-1], bounds[1:]):
        w.wait()                                   # the current stream waits for this piece only
        if factor != 1.0:
            g[a:b].mul_(factor)
        optimizer.step_range(a, b)


def allreduce_densification_stats(xys_absgrad_norm: torch.Tensor, vis_counts: torch.Tensor,
                                  max_radii: torch.Tensor, group=None) -> None:
    """Reduce what Nerfstudio's densifier accumulates from model.py:289-292 side effects:
    sum of |means2d.absgrad| norms and visibility counts (SUM), largest screen radius (MAX)."""
    dist.all_reduce(xys_absgrad_norm, op=dist.ReduceOp.SUM, group=group)
    dist.all_reduce(vis_counts, op=dist.ReduceOp.SUM, group=group)
    dist.all_reduce(max_radii, op=dist.ReduceOp.MAX, group=group)
