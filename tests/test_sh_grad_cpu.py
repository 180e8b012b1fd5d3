"""sh_grad.py on the CPU: the rules of the compact SH gradient's record (``model.compact_sh``), with the one binding of
qed_sh_grad_from_views stubbed to count its calls.  The device side is tests/test_api_path.py (test_lazy_sh_gradients_*,
test_flat_adam_refuses_stale_buffers_and_compact_gradients, test_compact_record_survives_an_eval_render_*)."""
from __future__ import annotations

import pytest
import torch

from tests.util import PARAM_NAMES, scene


@pytest.fixture()
def setup(monkeypatch):
    from qed_splatter_amd import sh_grad
    from qed_splatter_amd.model import QEDSplatterModel
    sc = scene(40, 32, 32, seed=3)
    m = QEDSplatterModel(None, **{k: sc[k] for k in PARAM_NAMES})
    m.train()
    calls = []
    monkeypatch.setattr(sh_grad, "write_sh_grads", lambda *a: calls.append(a))
    return m, calls


def _fill_grads(m):
    """Gradients laid out as the projection backward lays them out: six views of one allocation, in group order."""
    from qed_splatter_amd.model import _RAW_GRAD
    flat = torch.arange(m.flat_params.numel(), dtype=torch.float32)
    views = {}
    for name, a, b in zip(m.group_names, m.group_begin[:-1], m.group_begin[1:]):
        views[name] = flat[a:b].view(m.gauss_params[name].shape)
        _RAW_GRAD.__set__(m.gauss_params[name], views[name])
    return flat, views


def test_view_constructors_give_the_six_values_both_entry_points_read():
    from qed_splatter_amd.sh_grad import SHViews
    viewmat, v_color = torch.eye(4).reshape(1, 4, 4), torch.zeros(5, 3)
    own = SHViews.own(viewmat, v_color)
    assert own[0] == 1 and own[1] is viewmat and own[2] == 16 and own[3] is v_color and own[4] == 0 and own[5] == 1.0
    assert own.c_args() == (1, viewmat.data_ptr(), 16, v_color.data_ptr(), 0, 1.0)
    nv = 15
    for R in (1, 2):
        buf = torch.zeros(R, nv + 20)
        got = SHViews.rows(buf, nv)
        assert got[0] == R and got[2] == nv + 20 and got[3] is buf and got[4] == nv + 20 and got[5] == 1.0 / R
        assert got[1].data_ptr() == buf[:, nv:].data_ptr() and got[1].shape[0] == R
        assert got.c_args() == (R, buf.data_ptr() + 4 * nv, nv + 20, buf.data_ptr(), nv + 20, 1.0 / R)
    # the single-rank shape of the exchange: the send buffer seen as one row
    send = torch.zeros(nv + 20)
    one = SHViews.rows(send.view(1, nv + 20), nv)
    assert one[0] == 1 and one[5] == 1.0 and one[3].data_ptr() == send.data_ptr() and one[1].data_ptr() == send[nv:].data_ptr()


def test_explicit_record_is_the_callers_to_consume(setup):
    """fused_loss(compact_sh_grad=True)'s record: reads of ``.grad`` and flat_grad() never write out, everything that would
    train on the fields refuses, a forward without grad or in eval mode leaves it alone, a training forward with grad
    replaces it, the rebuilding exchange ends it with ONE write-out of the gathered views."""
    from qed_splatter_amd import parallel as P
    from qed_splatter_amd.sh_grad import CompactSHGrad, explicit_record
    m, calls = setup
    flat, views = _fill_grads(m)
    viewmat = torch.eye(4).reshape(1, 4, 4)
    rec = m.compact_sh = CompactSHGrad(viewmat, 3)
    assert not rec.implicit and rec.views is None and explicit_record(m) is rec
    assert m.features_dc.grad is views["features_dc"] and m.features_rest.grad is views["features_rest"]
    g = m.flat_grad()
    assert g.data_ptr() == flat.data_ptr() and m.compact_sh is rec and not calls
    # this rank's view only: the colour gradient is the features_dc range of the flat gradient
    own = rec.optimiser_views(g, m.group_begin)
    assert own[0] == 1 and own[1] is viewmat and own[3].data_ptr() == views["features_dc"].data_ptr() and own[4] == 0
    # writes of the fields leave it alone too (bench.py empties all six before every fused_loss)
    for p in m.parameters():
        p.grad = None
    assert m.compact_sh is rec
    flat, views = _fill_grads(m)
    with pytest.raises(RuntimeError, match="compact"):
        P.allreduce_flat_grad(m, 1)
    with pytest.raises(RuntimeError, match="compact"):
        P.allreduce_and_step(m, None, 1)
    # forwards that no backward pass follows
    with torch.no_grad():
        assert m._resolve_sh_grad() is False and m.compact_sh is rec
    m.eval()
    assert m._resolve_sh_grad() is False and m.compact_sh is rec
    m.train()
    # the exchange that leaves the views for the optimiser keeps it; the rebuilding one ends it
    P.exchange_grads_compact(m, 1, rebuild=False)
    assert m.compact_sh is rec and rec.views[0] == 1 and rec.optimiser_views() is rec.views and not calls
    assert rec.views[3].data_ptr() == P.exchange_state(m).dense[0].data_ptr() and P.exchange_state(m).skip is None
    P.exchange_grads_compact(m, 1)
    assert m.compact_sh is None and len(calls) == 1
    means, used, deg, out_dc, out_rest = calls[0]
    assert means is m.gauss_params["means"] and used[0] == 1 and deg == 3
    assert out_dc.data_ptr() == views["features_dc"].data_ptr() and out_rest.data_ptr() == views["features_rest"].data_ptr()
    P.allreduce_flat_grad(m, 1)                                        # full gradients again: accepted
    with pytest.raises(RuntimeError, match="compact_sh_grad=True"):
        P.exchange_grads_compact(m, 1)
    # a training forward with grad enabled: the new step's own state replaces it, nothing is written
    m.compact_sh = CompactSHGrad(viewmat, 3)
    assert m._resolve_sh_grad() is False and m.compact_sh is None and len(calls) == 1


def test_implicit_record_is_completed_for_every_reader(setup):
    """config.lazy_sh_grad's record: made by the projection backward's question, written out in place ONCE by the first
    Python read, dropped by ``.grad = None`` on both fields and by rebind_flat, completed by the next training forward
    with grad enabled -- and by no other forward; means modified in between raise."""
    from qed_splatter_amd.model import _RAW_GRAD, _raw_grad
    m, calls = setup
    dc, rest, means = m.gauss_params["features_dc"], m.gauss_params["features_rest"], m.gauss_params["means"]
    viewmat = torch.eye(4).reshape(1, 4, 4)

    def backward():
        """What a backward pass with QED_F_SH_GRAD_COMPACT does on the host: ask, then leave the views in the fields."""
        for p in (dc, rest):
            _RAW_GRAD.__set__(p, None)
        v_dc, v_rest = torch.zeros_like(dc), torch.zeros_like(rest)
        assert m._lazy_sh_begin(v_dc, v_rest, viewmat, 2) is True
        _RAW_GRAD.__set__(dc, v_dc)
        _RAW_GRAD.__set__(rest, v_rest)
        return v_dc, v_rest

    v_dc, v_rest = backward()
    rec = m.compact_sh
    assert rec.implicit and rec.deg == 2 and rec.n == 40 and rec.viewmat is viewmat
    assert rec.v_color is not v_dc and rec.v_color.data_ptr() == v_dc.data_ptr()      # aliases, never the objects
    assert rec.v_rest is not v_rest and rec.v_rest.data_ptr() == v_rest.data_ptr()
    own = rec.optimiser_views()
    assert own[0] == 1 and own[1] is viewmat and own[3] is rec.v_color and own[4] == 0
    # the raw accessor (QedAdam's) does not write out; forwards that no backward pass follows leave it alone
    assert _raw_grad(dc) is v_dc and m.compact_sh is rec and not calls
    with torch.no_grad():
        assert m._resolve_sh_grad() is False
    m.eval()
    assert m._resolve_sh_grad() is False and m.compact_sh is rec and not calls
    m.train()
    # the first Python read writes out once, in place
    assert rest.grad is v_rest and m.compact_sh is None and len(calls) == 1
    assert dc.grad is v_dc and len(calls) == 1
    got_means, used, deg, out_dc, out_rest = calls[0]
    assert got_means is means and deg == 2 and used[3] is out_dc and out_dc.data_ptr() == v_dc.data_ptr()
    assert out_rest.data_ptr() == v_rest.data_ptr()
    # the question of a second backward pass completes what waits and answers no
    backward()
    assert m._lazy_sh_begin(torch.zeros_like(dc), torch.zeros_like(rest), viewmat, 2) is False
    assert m.compact_sh is None and len(calls) == 2
    # the next training forward with grad enabled completes it
    backward()
    assert m._resolve_sh_grad() is True and m.compact_sh is None and len(calls) == 3
    # .grad = None on one field keeps it, on both drops it, without a write-out
    backward()
    dc.grad = None
    assert m.compact_sh is not None
    rest.grad = None
    assert m.compact_sh is None and len(calls) == 3
    # means modified between the backward pass and the read
    backward()
    with torch.no_grad():
        means.add_(0.0)
    with pytest.raises(RuntimeError, match="the means were modified after the backward pass"):
        dc.grad
    assert m.compact_sh is None and len(calls) == 3
    # densification
    backward()
    m.rebind_flat(m.flat_params.detach().clone(), m.num_points)
    assert m.compact_sh is None and len(calls) == 3
