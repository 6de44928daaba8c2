"""GPU: every compiled combine_kernel instantiation, and which one each op ran.

Every operation of the library goes through one kernel template, compiled by
launch_narrow / launch_exact / launch_generic (cec_runtime.hip; which one a launch takes
is plan_combine's choice, cec_launchplan.hpp) into 112 kernels: per
engine 4 narrow 1 x 1 kernels, 40 exact shapes and 12 capacity kernels, each with its own
register allocation and unrolled code.  The parity tests compare bytes; these tests also
read the launch record (cec_last_launch) after every launch, so a change of the dispatch
that silently moves a shape onto another kernel fails here, and they reach every kernel
a public call can land on:

* (a) all 256 coefficients on both engines, through the narrow kernels and the exact
  8 x 4 kernel, aligned and a byte off;
* (b) every exact shape over full aligned tiles and over ragged / misaligned ones;
* (c) every reachable capacity kernel; reached + listed-unreachable = the 12 x 2 compiled;
* (d) the input-count limit of cec_residual;
* (e) the store-policy bit and the workgroup split nobody picks, in child processes;
* the census: everything reached above plus kernel_matrix_case.UNREACHABLE is exactly the
  set of compiled instantiations.

The reference is a bit-serial GF(2^8) product table built in tests/kernel_matrix_case.py
(one CPU test ties it to oracle/); every comparison is bit-exact.
"""
from __future__ import annotations

import functools
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_matrix_case as kc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINES = [pytest.param(kc.PERM, id="perm"), pytest.param(kc.LDS, id="lds")]


def test_product_table_matches_oracle(oracle):
    """The bit-serial table of this file's reference against the oracle's product, all
    65,536 pairs: the two references the GPU suite compares with agree."""
    for a in range(256):
        for b in range(256):
            assert kc.MUL[a][b] == oracle.gf_mul(a, b), (a, b)
    assert all(kc.MUL[a][kc.gf_inv(a)] == 1 for a in range(1, 256))


def test_instantiation_lists():
    """The census' own arithmetic: 2 x (4 + 40 + 12) compiled, the unreachable among them."""
    assert len(kc.all_instantiations()) == 112
    assert kc.unreachable_instantiations() < kc.all_instantiations()


# Each part runs once per session and engine; the census reuses what the part's own test
# reached (a part that failed is run again there, and fails again).
@functools.lru_cache(maxsize=None)
def _reached(part: str, engine: int, case) -> frozenset:
    return frozenset(getattr(kc, part)(case, engine))


PARTS = ("check_every_coefficient", "check_exact_shapes", "check_capacity_kernels", "check_five_outputs",
         "check_residual_limits")


@pytest.fixture(scope="module")
def session_case(gpu):
    torch, ec = gpu
    engine = ec.get_engine()
    yield kc.Case(torch, ec)
    ec.set_engine(engine)


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ENGINES)
def test_every_coefficient(session_case, engine):
    """(a) 256 coefficients x {write, XOR} through the four narrow kernels (device memory,
    and pinned host memory for the system-release pair), 8 launches of 32 coefficients
    through the exact 8 x 4 kernel, again with one input and one output a byte off."""
    reached = _reached("check_every_coefficient", engine, session_case)
    assert {i[1:] for i in reached} == {(kc.NARROW, 1, 1, acc, rel) for acc in (kc.ACC_NONE, kc.ACC_ALL)
                                        for rel in (False, True)} | {(kc.EXACT, 8, 4, kc.ACC_NONE, False)}


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ENGINES)
def test_every_exact_shape(session_case, engine):
    """(b) the 32 write shapes and the 7 reachable read-modify-write shapes of launch_exact,
    plus the narrow pair that the 1 x 1 ops take, each over plan A and plan B with the
    kernel asserted from the launch record.  Default store policy: the write-through bit
    of every one of these small launches is set (e)."""
    reached = _reached("check_exact_shapes", engine, session_case)
    exact = {i for i in kc.all_instantiations() if i[0] == engine and i[1] == kc.EXACT}
    assert reached == (exact - kc.unreachable_instantiations()) | {
        (engine, kc.NARROW, 1, 1, kc.ACC_NONE, False), (engine, kc.NARROW, 1, 1, kc.ACC_ALL, False)}


@pytest.mark.gpu
def test_every_capacity_kernel(session_case):
    """(c) a public call for each capacity kernel NT in {2,4,8,16} x LT in {1,2,4} on each
    engine: the reached set and the unreachable list together are exactly the 12 x 2
    compiled, so a change of the dispatch shows up."""
    reached = set()
    for engine in (kc.PERM, kc.LDS):
        reached |= _reached("check_capacity_kernels", engine, session_case)
    compiled = {i for i in kc.all_instantiations() if i[1] == kc.GENERIC}
    unreachable = {i for i in kc.unreachable_instantiations() if i[1] == kc.GENERIC}
    assert len(compiled) == 24
    assert not reached & unreachable
    assert reached | unreachable == compiled, (sorted(compiled - reached - unreachable),
                                               sorted(reached - compiled))


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ENGINES)
def test_five_outputs_split_in_two_launches(session_case, engine):
    """(c) m = 4 with install: two launches (4 + 1 outputs), the install after both read
    the old bytes."""
    assert _reached("check_five_outputs", engine, session_case) == {
        (engine, kc.EXACT, 2, 1, kc.ACC_NONE, False)}


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ENGINES)
def test_residual_input_limit(session_case, engine):
    """(d) cec_residual: 17 inputs refused with CEC_EINVAL before anything is built or
    launched; 16 inputs (a recovery mask at k = 16) computed on the 16 x 1 capacity kernel."""
    assert _reached("check_residual_limits", engine, session_case) == {
        (engine, kc.GENERIC, 16, 1, kc.ACC_RUNTIME, False)}


@pytest.mark.gpu
def test_census_of_instantiations(session_case):
    """Reached by the parts above + UNREACHABLE = everything compiled, nothing in both."""
    reached = set()
    for part in PARTS:
        for engine in (kc.PERM, kc.LDS):
            reached |= _reached(part, engine, session_case)
    unreachable = kc.unreachable_instantiations()
    compiled = kc.all_instantiations()
    assert not reached & unreachable, sorted(reached & unreachable)
    assert reached | unreachable == compiled, (sorted(compiled - reached - unreachable),
                                               sorted(reached - compiled))
    assert (len(reached), len(unreachable)) == (108, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("env,args", [
    pytest.param({"CEC_STORE_POLICY": "nt"}, ["--expect-wt", "0"], id="store_policy_nt"),
    pytest.param({"CEC_SPLIT_SHIFT": "1"}, ["--expect-split", "1"], id="split_shift_1"),
])
def test_exact_shapes_under_pinned_environment(gpu, env, args):
    """(e) every exact shape again in a child process (the library reads both variables
    once): with non-temporal stores forced, the write-through bit clear on every launch;
    with two 128-lane workgroups per tile, the split the automatic rule never picks."""
    e = {x: v for x, v in os.environ.items()
         if x not in ("CEC_STORE_POLICY", "CEC_WT_MAX_BYTES", "CEC_SPLIT_SHIFT")}
    e.update(env)
    r = subprocess.run(["python", os.path.join(ROOT, "tests", "kernel_matrix_case.py"), *args], env=e,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]
