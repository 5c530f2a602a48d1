"""The input transform on the MI355X: bodahip_data_transform (kernels/data_f32.hip) byte for byte against its numpy twin (tests/data_ref.py) over the sampled shape
product, from NaN-filled outputs and with guard vars; every refusal with its sentence; and the two drivers on be=hip: the step fed bytes against the step fed the twin's
floats -- eager, as serial and as parallel graph replays, and on (be=hip,devices=0:0) -- and EvalPipe under the centre plan.

Every value is two IEEE operations on exact inputs: all comparisons are equalities on the bytes (a NaN where the twin has one)."""
import pytest

import data_ref as D
from boda_amd.rtc import make_rtc

pytestmark = pytest.mark.gpu
CASES = D.function_cases(seed=22)     # the corners, and another draw from the product than the be=cpu file's


@pytest.fixture(scope="module")
def hip():
    r = make_rtc("(be=hip)", 0)
    r.init()
    yield r
    r.close()


# ---- 1. the function
@pytest.mark.parametrize("c", CASES, ids=D.case_id)
def test_function_is_the_twin(hip, c):
    keep = []
    n = D.check_case(hip, c, keep=keep)
    for k in keep:     # one launch: a thread per four flat elements, workgroups of 256
        assert k["kernel"] == "bodahip_data_transform" and k["kernels"] == 1 and k["grid"] == -(-(-(-n // 4)) // 256) and k["block"] == 256, k


def test_corner_grids(hip):
    """135 elements: 34 threads, the last owns three; 3900 elements: 975 threads in four workgroups."""
    for c, grid in ((CASES[4], 1), (CASES[8], 4)):
        keep = []
        assert D.check_case(hip, c, keep=keep) in (135, 3900) and keep[0]["grid"] == grid


def test_realistic_case(hip):
    keep = []
    D.check_realistic(hip, keep=keep)
    assert keep[0]["kernel"] == "bodahip_data_transform" and keep[0]["grid"] == -(-(2 * 3 * 227 * 227 // 4 + 1) // 256)


def test_bad_ops_are_refused_with_their_sentences(hip):
    D.check_bad_ops(hip)


def test_bad_calls_are_refused_and_larger_vars_run(hip):
    D.check_bad_calls(hip)


# ---- 2. the step
@pytest.mark.parametrize("name,iter_size", [("chain", 1), ("chain", 2), ("residual", 1)])
def test_step_is_the_step_on_the_twins_floats(hip, name, iter_size):
    D.check_step(hip, name, iter_size)


@pytest.mark.parametrize("name", ["chain", "residual"])
@pytest.mark.parametrize("graph", ["serial", "parallel"])
def test_graph_replays_follow_the_pass_counter(hip, name, graph):
    """One captured graph, three replays: the plan lives in a var, so every replay crops and mirrors under its own pass's plan and leaves the eager run's bytes."""
    D.check_step(hip, name, 2 if name == "chain" else 1, graph=graph)


@pytest.mark.parametrize("name", ["chain", "residual"])
def test_call_deps_put_the_transform_in_front_of_datas_readers(hip, name):
    D.check_call_deps(hip, name)


def test_step_on_two_shards():
    """(be=hip,devices=0:0): src, plan and out are img shards, the mean is whole on every device; every node holds the bytes of the multi-device step fed the twin's
    floats."""
    multi = make_rtc("(be=hip,devices=0:0)"); multi.init()
    try:
        D.check_step(multi, "chain", 1)
    finally:
        multi.close()


# ---- 3. EvalPipe
@pytest.mark.parametrize("name", ["chain", "residual"])
@pytest.mark.parametrize("graph", [False, True])
def test_eval_pipe_uses_the_centre_plan(hip, name, graph):
    D.check_eval(hip, name, graph=graph)


@pytest.mark.parametrize("graph", [False, True])
def test_training_is_undisturbed_by_evaluations(hip, graph):
    D.check_training_is_undisturbed(hip, "chain", graph=graph)


def test_refusals_and_defaults(hip):
    D.check_refusals_and_defaults(hip)
