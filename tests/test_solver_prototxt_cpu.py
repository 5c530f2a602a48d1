"""prototxt.solver_spec: Caffe's SolverParameter text form -> (Solver, iter_size, ignored).

The fixture tests/golden/solver/firenet8-solver.prototxt is the one solver file the reference holds (nets/firenet8-CE-0.125/solver.prototxt), copied by hand: its
settings, without its two commented-out lines.  tests/golden/make_fixtures.py does not make it."""
import os

import pytest

import solver_ref as V
from boda_amd.bck_pipe import LrPolicy, Solver
from boda_amd.op import RtErr, UnsupErr
from boda_amd.prototxt import solver_spec
from boda_amd.rtc import make_rtc

HERE = os.path.dirname(os.path.abspath(__file__))


def test_the_reference_s_solver_file():
    sv, iter_size, ignored = solver_spec(open(os.path.join(HERE, "golden", "solver", "firenet8-solver.prototxt")).read())
    assert sv == Solver(type="sgd", lr=0.08, momentum=0.9, weight_decay=0.0002, lr_policy=LrPolicy("poly", power=0.5, max_iter=85000))
    assert iter_size == 1
    assert ignored == {"test_iter": ["49"], "test_interval": ["500"], "display": ["40"], "snapshot": ["1000"], "snapshot_prefix": ["train"], "solver_mode": ["GPU"],
                       "random_seed": ["42"], "net": ["trainval.prototxt"], "test_initialization": ["false"], "average_loss": ["40"]}
    assert sv.lr_policy.lr_at(sv.lr, 0) == 0.08 and sv.lr_policy.lr_at(sv.lr, 85000) == 0.0


def test_caffe_s_defaults_not_the_dataclass_s():
    sv, iter_size, ignored = solver_spec("base_lr: 0.01")
    assert sv == Solver(type="sgd", lr=0.01, momentum=0.0, momentum2=0.999, delta=1e-8, weight_decay=0.0, clip_gradients=0.0, lr_policy=None)
    assert (iter_size, ignored) == (1, {})
    assert solver_spec("base_lr: 0.01 clip_gradients: -1")[0].clip_gradients == 0.0
    with pytest.raises(RtErr, match="no base_lr"):
        solver_spec("")


@pytest.mark.parametrize("text,want", [('type: "SGD"', "sgd"), ('type: "Nesterov"', "nesterov"), ('type: "Adam"', "adam"), ("solver_type: SGD", "sgd"),
                                       ("solver_type: NESTEROV", "nesterov"), ("solver_type: ADAM", "adam")])
def test_both_spellings_of_the_type(text, want):
    assert solver_spec("base_lr: 0.5\n" + text)[0].type == want


def test_policies_iter_size_and_clipping():
    sv, iter_size, ignored = solver_spec('''
        # a comment
        net: "train_val.prototxt"
        type: "Adam"  base_lr: 0.001  momentum: 0.9  momentum2: 0.99  delta: 1e-6
        lr_policy: "multistep"  gamma: 0.5  stepvalue: 100  stepvalue: 200  stepvalue: 350
        weight_decay: 0.0005  clip_gradients: 35  iter_size: 8  regularization_type: "L2"
        snapshot_after_train: true''')
    assert sv == Solver(type="adam", lr=0.001, momentum=0.9, momentum2=0.99, delta=1e-6, weight_decay=0.0005, clip_gradients=35.0,
                        lr_policy=LrPolicy("multistep", gamma=0.5, stepvalues=(100, 200, 350)))
    assert iter_size == 8 and ignored == {"net": ["train_val.prototxt"], "snapshot_after_train": ["true"]}
    assert [sv.lr_policy.lr_at(1.0, it) for it in (99, 100, 200, 350)] == [1.0, 0.5, 0.25, 0.125]
    sv, _, _ = solver_spec('base_lr: 0.1 lr_policy: "step" gamma: 0.1 stepsize: 1000')
    assert sv.lr_policy == LrPolicy("step", gamma=0.1, stepsize=1000)
    assert solver_spec('base_lr: 0.1 lr_policy: "fixed"')[0].lr_policy == LrPolicy("fixed")
    assert solver_spec('base_lr: 0.1 lr_policy: "inv" gamma: 0.0001 power: 0.75')[0].lr_policy == LrPolicy("inv", gamma=0.0001, power=0.75)


@pytest.mark.parametrize("text,msg", [('type: "AdaGrad"', "'AdaGrad'"), ('type: "RMSProp"', "'RMSProp'"), ('type: "AdaDelta"', "'AdaDelta'"), ("solver_type: ADAGRAD", "'ADAGRAD'"),
                                      ("solver_type: RMSPROP", "'RMSPROP'"), ("solver_type: ADADELTA", "'ADADELTA'"), ('regularization_type: "L1"', "'L1'")])
def test_refused_naming_the_value(text, msg):
    with pytest.raises(UnsupErr, match=msg):
        solver_spec("base_lr: 0.1\n" + text)


def test_malformed():
    for text, msg in (('base_lr: 0.1 type: "Momentum"', "'Momentum'"), ('base_lr: 0.1 lr_policy: "cosine"', "policy must be one of"), ("base_lr: 0.1 iter_size: 0", "iter_size=0"),
                      ("base_lr: 0.1 base_lr: 0.2", "2 times"), ("base_lr: fast", "not a number"), ('base_lr: 0.1 type: "SGD" solver_type: SGD', "both")):
        with pytest.raises(RtErr, match=msg):
            solver_spec(text)


def test_the_result_drives_a_step_on_cpu():
    sv, iter_size, _ = solver_spec('base_lr: 0.05 momentum: 0.9 weight_decay: 0.0005 type: "Nesterov" lr_policy: "step" gamma: 0.5 stepsize: 1 iter_size: 2 clip_gradients: 0.05')
    cpu = make_rtc("(be=cpu)"); cpu.init()
    try:
        import accum_ref as A
        drv, bp = V.make_driver(cpu, "chain", sv, iter_size=iter_size)
        try:
            A.passes(cpu, drv, bp, 2)
            assert (drv.iter, drv.micro) == (1, 0)
        finally:
            drv.release()
        sv1, one, _ = solver_spec('base_lr: 0.05 momentum: 0.9 type: "Adam"')
        assert one == 1
        V.three_steps(cpu, "chain", sv1)
    finally:
        cpu.close()
