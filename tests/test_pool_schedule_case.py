"""CPU: the recovery pool's schedule model tied down, and what its schedules cover.

A dry run (no GPU, no library) of every (code, seed) that tests/test_gpu_pool_schedules.py
runs: the generator draws from the model alone, so these are the GPU runs step for step.

Tie-down.  Replies and given residuals are the true bytes of a consistent stripe set when they
are sent.  A request with no SET on its units between its first reply or given residual and a
solve must therefore rebuild the live data: every such solve of the dry run is compared, and
every loss count 1..min(k, m) must occur among them.

Coverage.  Hard asserts on the dry run's event counters (pool_schedule_case.coverage_gaps), so a
schedule cannot pass by doing little; CODES records the seeds and the length that meet them.
"""
from __future__ import annotations

import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pool_schedule_case as ps  # noqa: E402

CASES = [pytest.param(k, m, seed, id=f"rs{k}_{m}-seed{seed}") for (k, m), cfg in ps.CODES.items() for seed in cfg["seeds"]]
_RUNS: dict = {}


def dry_run(oracle, k, m, seed):
    if (k, m, seed) not in _RUNS:
        _RUNS[(k, m, seed)] = ps.schedule(k, m, oracle.big_vandermonde(k + m, k), seed)
    return _RUNS[(k, m, seed)]


def test_codes_and_leaders():
    assert {km: c["leader"] for km, c in ps.CODES.items()} == {(3, 2): 4, (6, 4): 6, (3, 4): 3, (10, 8): 17}
    assert all(c["steps"] % 100 == 0 and c["seeds"] for c in ps.CODES.values())
    assert ps.CAP == 24 and ps.ARENA_UNITS == 32


@pytest.mark.parametrize("k,m,seed", CASES)
def test_clean_requests_rebuild_the_live_data(oracle, k, m, seed):
    model, steps = dry_run(oracle, k, m, seed)
    assert len(steps) == ps.CODES[(k, m)]["steps"]
    wrong = [t for t in model.tie if not t[3]]
    assert not wrong, f"RS({k},{m}) seed {seed}: (step, handle, losses) {[t[:3] for t in wrong[:5]]}"
    assert {t[2] for t in model.tie} == set(range(1, min(k, m) + 1))


@pytest.mark.parametrize("k,m,seed", CASES)
def test_schedule_covers_every_condition(oracle, k, m, seed):
    model, _ = dry_run(oracle, k, m, seed)
    assert ps.coverage_gaps(model) == [], (k, m, seed, dict(model.ev))


@pytest.mark.parametrize("k,m", list(ps.CODES))
def test_length_is_the_smallest_multiple_of_100(oracle, k, m):
    """100 steps fewer leave a condition unmet for at least one seed of the code."""
    cfg = ps.CODES[(k, m)]
    mat = oracle.big_vandermonde(k + m, k)
    assert cfg["steps"] > 100
    assert any(ps.coverage_gaps(ps.schedule(k, m, mat, s, cfg["steps"] - 100)[0]) for s in cfg["seeds"])


def test_dry_run_is_deterministic(oracle):
    k, m = 3, 2
    seed = ps.CODES[(k, m)]["seeds"][0]
    mat = oracle.big_vandermonde(k + m, k)
    assert ps.schedule(k, m, mat, seed, 100)[1] == ps.schedule(k, m, mat, seed, 100)[1] == dry_run(oracle, k, m, seed)[1][:100]


def test_begin_is_drawn_only_where_every_placement_agrees(oracle):
    """Every begin the generator expects to succeed has F >= (L + 1)(n - 1) + 1 and lies in the
    arena; every probe has F < n or n > capacity (Model.apply asserts both as it goes)."""
    for k, m, seed in [(3, 2, ps.CODES[(3, 2)]["seeds"][0])]:
        _, steps = dry_run(oracle, k, m, seed)
        begins = [s for s in steps if s["op"] == "begin"]
        assert {s["expect"] for s in begins} == {"ok", "full"}
        assert all(0 <= s["ub"] <= s["ue"] < ps.ARENA_UNITS for s in begins)
