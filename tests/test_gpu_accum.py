"""Gradient accumulation on the MI355X: bodahip_grad_accum and the -DACCUM=1 form of bodahip_solver_update_{sgd,nesterov,adam} (kernels/solver_update_f32.hip) bit for bit
against the numpy twins (tests/accum_ref.py), and ConvPipeBck(solver=Solver(...), iter_size=n) on be=hip -- eager, as replays of ONE captured hipGraph, on two shards of
device 0, with a BatchNorm pipe -- every pass held to the twins on the backend's own recorded gradients.

Every comparison is on the uint32 views, except where the twin yields NaN (the backend must yield NaN).  Neither function has a pure output, so the check that nothing else
is written is a guard var behind every var of a call."""
import numpy as np
import pytest

import accum_ref as A
import solver_ref as V
from boda_amd.bck_pipe import LrPolicy
from boda_amd.rtc import make_rtc

from test_accum_cpu import test_cpu_batchnorm_pipe_with_adam_and_iter_size_two as batchnorm_pipe, test_cpu_calls_vars_skip_and_reset as calls_vars_skip_and_reset

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def hip():
    r = make_rtc("(be=hip)", 0)
    r.init()
    yield r
    r.close()


@pytest.fixture(scope="module")
def hip2():
    """The eager driver's backend: a second instance, with a stream, vars and kernels of its own."""
    r = make_rtc("(be=hip)", 0)
    r.init()
    yield r
    r.close()


# ---- 1. the two functions
def test_accum_first_add_add(hip):
    for sizes in A.ACCUM_CASES:
        keep = A.check_accum_three_calls(hip, sizes)
        for k in keep:
            assert k["kernel"] == "bodahip_grad_accum" and k["kernels"] == 1 and k["grid"] == sum(-(-n // 4096) for n in sizes) and k["block"] == 256
            assert k["algo_bytes"] == 12.0 * sum(sizes)


def test_accum_special_values(hip):
    A.check_accum_special_values(hip)


@pytest.mark.parametrize("form", V.FORMS, ids=V.form_id)
def test_update_acc(hip, form):
    for sizes in A.UPDATE_CASES:
        for k in A.check_update_acc(hip, sizes, form):
            assert k["kernel"] == "bodahip_solver_update_" + form[0] and k["kernels"] == 1 and k["grid"] == sum(-(-n // 4096) for n in sizes)
            assert k["algo_bytes"] == (28.0 if form[0] == "adam" else 20.0) * sum(sizes)


# ---- 2. the driver
@pytest.mark.parametrize("form", V.FORMS, ids=V.form_id)
@pytest.mark.parametrize("name", ["chain", "fan"])
def test_six_passes_are_the_twins(hip, name, form):
    packed = A.six_passes(hip, name, A.mk_solver(form, 32))
    three = A.six_passes(hip, name, A.mk_solver(form, 3))
    for vn in packed:
        assert V.same_bits(packed[vn], three[vn]), vn


def test_step_policy_boundary_between_the_two_updates(hip):
    A.six_passes(hip, "chain", A.mk_solver(("adam", True, False), policy=LrPolicy(policy="step", gamma=0.5, stepsize=1)))


def test_calls_vars_skip_and_reset(hip):
    calls_vars_skip_and_reset(hip)


def test_batchnorm_pipe_with_adam_and_iter_size_two(hip):
    batchnorm_pipe(hip)


# ---- 3. graph and devices
@pytest.mark.parametrize("name", ["chain", "fan"])
def test_one_capture_serves_every_micro_step(hip, hip2, name):
    """One capture, six replays -- serial, then (a new driver) parallel=True: every var holds the bytes of an eager driver fed the same inputs, after every pass."""
    mk = lambda: A.mk_solver(("adam", True, False), policy=LrPolicy(policy="step", gamma=0.5, stepsize=1))
    eager = []
    A.six_passes(hip2, name, mk(), record=eager, seed_in_var=True)
    for parallel in (False, True):
        got = []
        A.six_passes(hip, name, mk(), graph=parallel, record=got, seed_in_var=True)
        assert len(got) == len(eager) == 6
        for k, (g, e) in enumerate(zip(got, eager)):
            assert set(g) == set(e)
            for vn in g:
                assert g[vn] == e[vn], (parallel, k, vn)


def test_two_shards_of_one_device(hip):
    """(be=hip,devices=0:0): the accumulate and update calls run on every device's replicas; device 0's are held to the twins on that backend's own recorded gradients."""
    multi = make_rtc("(be=hip,devices=0:0)"); multi.init()
    try:
        A.six_passes(multi, "chain", A.mk_solver(("adam", True, False), 3))
        A.six_passes(multi, "fan", A.mk_solver(("nesterov", False, False)))
    finally:
        multi.close()


# ---- 4. meaning
def test_meaning_two_halves_are_one_batch(hip):
    dev = A.meaning_dev(hip)
    print("one sgd step at batch %d against iter_size=2 at batch %d: largest relative difference of the params %.3e (bound %.3e)" % (2 * A.MEANING_B, A.MEANING_B, dev, A.MEANING_BOUND))
    assert dev <= A.MEANING_BOUND, dev
