"""The prototxt readers of the evaluation pass: prototxt.test_spec (the test keys of a solver file, Caffe's defaults for absent ones) and prototxt.accuracy_layers (a net
file's Accuracy layers); solver_spec's output on the fixture stays what it was."""
import os

import pytest

from boda_amd.op import RtErr, UnsupErr
from boda_amd.prototxt import accuracy_layers, conv_ops, pipe_spec, solver_spec, test_spec as read_test_spec

HERE = os.path.dirname(os.path.abspath(__file__))
FIRENET = open(os.path.join(HERE, "golden", "solver", "firenet8-solver.prototxt")).read()

NET = """
name: "tiny"
layer { name: "data" type: "Data" top: "data" top: "label" include { phase: TEST } transform_param { crop_size: 8 } }
layer { name: "conv1" type: "Convolution" bottom: "data" top: "conv1" convolution_param { num_output: 4 kernel_size: 3 } }
layer { name: "relu1" type: "ReLU" bottom: "conv1" top: "conv1" }
layer { name: "fc" type: "InnerProduct" bottom: "conv1" top: "fc" inner_product_param { num_output: 10 } }
layer { name: "loss" type: "SoftmaxWithLoss" bottom: "fc" bottom: "label" top: "loss" }
layer { name: "accuracy" type: "Accuracy" bottom: "fc" bottom: "label" top: "accuracy" include { phase: TEST } }
layer { name: "accuracy_top5" type: "Accuracy" bottom: "fc" bottom: "label" top: "accuracy_top5" accuracy_param { top_k: 5 } }
layer { name: "train_only" type: "Accuracy" bottom: "fc" bottom: "label" top: "t" include { phase: TRAIN } }
"""


def test_test_spec_on_the_fixture_and_defaults():
    assert read_test_spec(FIRENET) == {"test_iter": 49, "test_interval": 500, "test_initialization": False}
    assert read_test_spec("base_lr: 0.1") == {"test_iter": 0, "test_interval": 0, "test_initialization": True}
    assert read_test_spec("test_iter: 7 test_iter: 9 test_initialization: true") == {"test_iter": 7, "test_interval": 0, "test_initialization": True}
    for bad, msg in (("test_iter: x", "test_iter: 'x' is not an integer"), ("test_interval: -5", "test_interval=-5"), ("test_initialization: maybe", "neither true nor false"),
                     ("test_interval: 1 test_interval: 2", "'test_interval' is given 2 times"), ("test_iter { a: 1 }", "must be a value")):
        with pytest.raises(RtErr, match=msg):
            read_test_spec(bad)


def test_solver_spec_is_unchanged_on_the_fixture():
    sv, iter_size, ignored = solver_spec(FIRENET)
    assert (sv.type, sv.lr, sv.momentum, sv.weight_decay, sv.clip_gradients, iter_size) == ("sgd", 0.08, 0.9, 0.0002, 0.0, 1)
    assert (sv.lr_policy.policy, sv.lr_policy.power, sv.lr_policy.max_iter) == ("poly", 0.5, 85000)
    assert ignored == {"test_iter": ["49"], "test_interval": ["500"], "display": ["40"], "snapshot": ["1000"], "snapshot_prefix": ["train"], "solver_mode": ["GPU"],
                       "random_seed": ["42"], "net": ["trainval.prototxt"], "test_initialization": ["false"], "average_loss": ["40"]}


def test_accuracy_layers():
    assert accuracy_layers(NET) == [("accuracy", "fc", "label", 1), ("accuracy_top5", "fc", "label", 5)]
    assert accuracy_layers('layer { name: "c" type: "ReLU" bottom: "a" top: "a" }') == []
    assert [n for n, _ in conv_ops(NET, 2, (3, 8, 8))] == ["conv1", "fc"]     # the shape-inference readers keep ignoring these layers
    assert not any("accuracy" in l for l in pipe_spec(NET, (3, 8, 8)))
    one = lambda body: 'layer { name: "acc" type: "Accuracy" bottom: "fc" bottom: "label" top: "acc" accuracy_param { %s } }' % body
    with pytest.raises(UnsupErr, match="'acc': ignore_label"):
        accuracy_layers(one("ignore_label: 255"))
    with pytest.raises(UnsupErr, match="'acc': axis=2"):
        accuracy_layers(one("axis: 2"))
    assert accuracy_layers(one("axis: 1 top_k: 3")) == [("acc", "fc", "label", 3)]
    with pytest.raises(RtErr, match="top_k=0"):
        accuracy_layers(one("top_k: 0"))
    with pytest.raises(RtErr, match="1 bottoms"):
        accuracy_layers('layer { name: "acc" type: "Accuracy" bottom: "fc" top: "acc" }')
