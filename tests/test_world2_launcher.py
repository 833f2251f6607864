"""The world-2 launcher (tests/world2_launch.py + tests/world2_rank.py) on a machine without a GPU: two gloo ranks over a file
rendezvous on CPU tensors.  The plumbing tests/test_gpu_world2.py relies on — results come back per rank, a failing rank fails
the pair at once with its traceback and leaves nobody behind — is proven here before any rank touches a device."""
import time

import pytest
import torch

from tests import world2_launch as L

CHILD_LIMIT, COLLECTIVE_TIMEOUT = 120, 60


def test_clean_pair_returns_the_reduced_tensor(tmp_path):
    res, seconds = L.run_pair(["cpu_allreduce"], tmp_path, CHILD_LIMIT, COLLECTIVE_TIMEOUT)
    assert len(res) == 2
    for r in res:
        assert sorted(r) == ["cpu_allreduce"]
        assert torch.equal(r["cpu_allreduce"]["sum"], torch.arange(8, dtype=torch.float32) * 3)        # x (1 + 2)
    assert seconds < COLLECTIVE_TIMEOUT


def test_failing_rank_fails_the_pair_with_its_traceback_and_leaves_no_child(tmp_path):
    """rank 1 raises before any collective while rank 0 waits in one: the launcher must not wait for rank 0's collective to time
    out — it sees rank 1's exit status, kills rank 0 and reports rank 1's traceback"""
    t0 = time.perf_counter()
    with pytest.raises(L.World2Failure) as ei:
        L.run_pair(["cpu_raise_rank1", "cpu_allreduce"], tmp_path, CHILD_LIMIT, COLLECTIVE_TIMEOUT)
    wall = time.perf_counter() - t0
    e = ei.value
    assert "rank 1 fails here, before any collective" in str(e) and "Traceback (most recent call last)" in e.stderr[1]
    assert "sc_cpu_raise_rank1" in e.stderr[1]
    assert e.returncodes[1] == 1
    assert wall < COLLECTIVE_TIMEOUT, wall
    assert all(pid is not None for pid in e.pids)
    assert not any(L.pid_alive(pid) for pid in e.pids)
    # what rank 1 had when it failed: the traceback and the scenario's name, and nothing after it was started
    assert e.partial[1]["failed_in"] == "cpu_raise_rank1" and "cpu_allreduce" not in e.partial[1]
    assert "RuntimeError" in e.partial[1]["traceback"]


def test_unknown_scenario_is_refused_by_both_ranks(tmp_path):
    with pytest.raises(L.World2Failure) as ei:
        L.run_pair(["no_such_scenario"], tmp_path, CHILD_LIMIT, COLLECTIVE_TIMEOUT)
    assert "unknown scenarios" in str(ei.value)
