"""The intersection-buffer protocol of qed_splatter_amd.binning without a GPU and without the library: the bookkeeping of
``_Workspace`` runs on a CPU device as it stands (calibration, the count that arrives a call late, overflow recovery, the
watchdog), with a plain numpy array standing in for the pinned words a binning launch stores into."""
from __future__ import annotations

import ast
import os
import warnings

import numpy as np
import pytest
import torch

from qed_splatter_amd import _lib as L
from qed_splatter_amd import binning
from qed_splatter_amd.binning import _Workspace

KEY, OTHER = ((160, 112), 3000, 1), ((320, 224), 3000, 1)


def _grown(M: int) -> int:
    return int(M * _Workspace.HEADROOM) + 4096


def _ws() -> _Workspace:
    return _Workspace(torch.device("cpu"))


def _words(*w) -> np.ndarray:
    return np.array(w, dtype=np.int32)


class _Stepper:
    def __init__(self):
        self.skipped = 0

    def on_skipped_step(self):
        self.skipped += 1


def test_calibration_is_per_shape_and_bounded():
    ws = _ws()
    assert not ws.may_skip_readback(KEY) and not ws.may_capture(KEY) and ws.capacity == 0
    ws.saw(KEY, 10_000)
    assert ws.capacity == _grown(10_000) and ws.m_seen[KEY] == 10_000
    assert ws.may_skip_readback(KEY) and ws.may_capture(KEY)
    assert not ws.may_skip_readback(OTHER) and not ws.may_capture(OTHER)
    ws.saw(KEY, 5_000)                                          # the longest list seen stays
    assert ws.capacity == _grown(10_000) and ws.m_seen[KEY] == 10_000
    # the two predicates differ exactly where they should: a pending re-calibration refuses the asynchronous call, not a
    # capture; words that do not arrive through pinned memory refuse the asynchronous call for good
    ws.force_sync = True
    assert not ws.may_skip_readback(KEY) and ws.may_capture(KEY)
    ws.force_sync, ws.host_words_ok = False, False
    assert not ws.may_skip_readback(KEY) and ws.may_capture(KEY)
    ws.host_words_ok = True
    for i in range(200):
        ws.saw(((i, i), 1, 1), 1)
        assert len(ws.m_seen) <= 64
    ws.force_sync = True
    ws.reset()
    assert ws.capacity == 0 and ws.m_seen == {} and not ws.force_sync and not ws.may_skip_readback(KEY)


@pytest.mark.parametrize("M2", [4_000, 25_000])
def test_a_count_that_arrives_late_keeps_the_capacity_up(M2):
    M = 10_000
    ws = _ws()
    ws.saw(KEY, M)
    ws.arm_pending(_words(M2, 0, 0, 0), KEY)
    assert ws.pending is not None
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ws.poll_pending()
        ws.poll_pending()                                       # (nothing pending: a no-op)
    assert ws.pending is None and ws.m_seen[KEY] == max(M, M2) and ws.capacity == _grown(max(M, M2))
    assert ws.overflows == 0 and ws.may_skip_readback(KEY) and ws.take_overflow_flag() is False


def test_overflow_recovery_tells_the_optimisers_that_stepped_behind_that_frame():
    M, need = 10_000, 50_001
    ws = _ws()
    ws.saw(KEY, M)
    earlier, behind, never = _Stepper(), _Stepper(), _Stepper()
    for s in (earlier, behind, never):
        ws.steppers.add(s)
    ws.arm_pending(_words(M, 0, 0, 0), KEY)
    ws.counted_step(earlier)
    ws.poll_pending()
    ws.status[0], ws.status[1] = need, 0                        # (what the overflowing launch left on the device)
    ws.arm_pending(_words(need, need, 0, 0), KEY)
    ws.counted_step(behind)
    with pytest.warns(RuntimeWarning) as caught:
        ws.poll_pending()
    assert len(caught) == 1 and str(need) in str(caught[0].message) and str(_grown(M)) in str(caught[0].message)
    assert caught[0].category is RuntimeWarning and caught[0].filename != binning.__file__   # (stacklevel: a caller's line)
    assert ws.pending is None and ws.overflows == 1 and ws.force_sync
    assert not ws.may_skip_readback(KEY) and ws.may_capture(KEY)
    assert ws.capacity >= _grown(need) and ws.m_seen[KEY] == need
    assert ws.status.tolist() == [0] * L.STATUS_WORDS and int(ws.overflow_word) == 0
    assert ws.take_overflow_flag() is True and ws.take_overflow_flag() is False
    assert (earlier.skipped, behind.skipped, never.skipped) == (0, 1, 0)
    ws.poll_pending()                                           # told once
    assert behind.skipped == 1 and ws.overflows == 1


def test_watchdog_word_raises_and_clears_the_status_words():
    ws = _ws()
    ws.saw(KEY, 10_000)
    ws.status[1] = 1
    ws.arm_pending(_words(10_000, 0, 1, 0), KEY)
    with pytest.raises(L.QedSplatError, match="watchdog fired in the previous asynchronous rasterization"):
        ws.poll_pending()
    assert ws.status.tolist() == [0] * L.STATUS_WORDS and ws.pending is None and ws.overflows == 0
    ws.status[1] = 1
    with pytest.raises(L.QedSplatError, match="^some other text$"):
        ws.watchdog_fired("some other text")
    assert ws.status.tolist() == [0] * L.STATUS_WORDS


def test_overflow_of_a_graphed_frame_grows_by_the_same_formula_and_records_no_shape():
    ws = _ws()
    ws.saw(KEY, 10_000)
    seen = dict(ws.m_seen)
    ws.status[0] = 70_000
    assert ws.read_words()[1:] == [70_000, 0]
    old = ws.overflowed(70_000)
    assert old == _grown(10_000) and ws.capacity == _grown(70_000)
    assert ws.m_seen == seen and ws.overflows == 1 and ws.force_sync
    assert ws.status.tolist() == [0] * L.STATUS_WORDS


def test_overflow_word_is_the_first_status_word():
    ws = _ws()
    word = ws.overflow_word
    assert word.dtype == torch.int32 and tuple(word.shape) == (1,)
    assert word.data_ptr() == ws.status.data_ptr() == ws.skip_flag_ptr() == ws.words.data_ptr() + 4
    ws.status[0] = 3
    assert int(word) == 3


def _package_source(name: str) -> str:
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "qed_splatter_amd", name)) as f:
        return f.read()


def test_binning_sits_below_the_operator_and_rasterization_hands_out_the_same_objects():
    from qed_splatter_amd import rasterization
    for name in ("_Workspace", "_WORKSPACES", "_workspace", "_bin_and_sort"):
        assert getattr(rasterization, name) is getattr(binning, name), name
    for node in ast.walk(ast.parse(_package_source("binning.py"))):
        if isinstance(node, ast.ImportFrom) and (node.level > 0 or (node.module or "").startswith("qed_splatter_amd")):
            assert node.level == 1 and node.module is None and [a.name for a in node.names] == ["_lib"], ast.dump(node)
        if isinstance(node, ast.Import):
            assert not any(a.name.startswith("qed_splatter_amd") for a in node.names), ast.dump(node)


def test_graph_py_leaves_the_workspace_bookkeeping_to_the_workspace():
    src = _package_source("graph.py")

    def is_workspace(v) -> bool:
        return (isinstance(v, ast.Name) and v.id == "ws") or (isinstance(v, ast.Attribute) and v.attr == "ws")

    for node in ast.walk(ast.parse(src)):
        targets = node.targets if isinstance(node, ast.Assign) else \
            [node.target] if isinstance(node, (ast.AugAssign, ast.AnnAssign)) else []
        for t in targets:
            for leaf in ast.walk(t):
                assert not (isinstance(leaf, ast.Attribute) and is_workspace(leaf.value)), ast.dump(node)
    assert "HEADROOM) +" not in src and "4096" not in src and ".status" not in src
