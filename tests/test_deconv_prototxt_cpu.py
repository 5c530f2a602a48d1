"""The prototxt readers on Deconvolution and Crop layers (no GPU): pipe_spec's records, conv_ops' op lines and shapes, one offset or one per axis, and the refusals."""
import pytest

from boda_amd import prototxt
from boda_amd.conv_pipe import pipe_from_spec
from boda_amd.op import UnsupErr

FCN = """
name: "fcn_mini"
input: "data"
input_dim: 2 input_dim: 3 input_dim: 16 input_dim: 16
layer { name: "conv1" type: "Convolution" bottom: "data" top: "conv1" convolution_param { num_output: 8 kernel_size: 3 pad: 1 stride: 2 } }
layer { name: "relu1" type: "ReLU" bottom: "conv1" top: "conv1" }
layer { name: "score" type: "Convolution" bottom: "conv1" top: "score" convolution_param { num_output: 5 kernel_size: 1 } }
layer { name: "up" type: "Deconvolution" bottom: "score" top: "up" convolution_param { num_output: 5 kernel_size: 4 stride: 2 } }
layer { name: "crop" type: "Crop" bottom: "up" bottom: "data" top: "out" crop_param { axis: 2 offset: 1 } }
"""


def test_records_and_ops():
    spec = prototxt.pipe_spec(FCN)
    assert spec == ["input data 3 16 16", "conv conv1 data conv1 8 3 3 2 2 1 1", "relu relu1 conv1 conv1", "conv score conv1 score 5 1 1 1 1 0 0",
                    "deconv up score up 5 4 4 2 2 0 0", "crop crop up data out 1 1"]
    cp = pipe_from_spec("fcn_mini", spec, 2)
    assert cp.nodes["up"].sizes == (2, 5, 18, 18) and cp.nodes["out"].sizes == (2, 5, 16, 16)
    assert cp.ops[-1].type == "Crop" and cp.ops[-1].bots == ("up", "data") and cp.ops[-1].offset == (1, 1)
    ops = dict(prototxt.conv_ops(FCN, 2))
    assert list(ops) == ["conv1", "score", "up"] and ops["up"].get_type() == "Deconvolution"
    assert ops["up"].to_str() == cp.conv_op(cp.ops[3]).to_str()   # the readers agree on the op line
    assert ops["up"].deconv_geom()["OH"] == 18 and ops["up"].get_dims("filts").names == ("in_chan", "out_chan", "y", "x")


def test_one_offset_per_axis_and_the_default():
    two = FCN.replace("crop_param { axis: 2 offset: 1 }", "crop_param { axis: 2 offset: 2 offset: 0 }")
    assert prototxt.pipe_spec(two)[-1] == "crop crop up data out 2 0"
    none = FCN.replace("crop_param { axis: 2 offset: 1 }", "crop_param { }")
    assert prototxt.pipe_spec(none)[-1] == "crop crop up data out 0 0"


def test_conv_ops_checks_the_crop_window():
    from boda_amd.op import RtErr
    with pytest.raises(RtErr, match=r"crop 'crop': offset \(3, 3\) \+ 'data''s plane \(16, 16\) exceeds 'up''s plane \(18, 18\)"):
        prototxt.conv_ops(FCN.replace("offset: 1", "offset: 3"), 2)


def test_refusals_by_name():
    with pytest.raises(UnsupErr, match="crop 'crop': axis=1: only axis 2"):
        prototxt.pipe_spec(FCN.replace("axis: 2", "axis: 1"))
    with pytest.raises(UnsupErr, match="deconvolution 'up': group=5: a Deconvolution with group > 1 is out of scope"):
        prototxt.pipe_spec(FCN.replace("kernel_size: 4 stride: 2", "kernel_size: 4 stride: 2 group: 5"))
    with pytest.raises(UnsupErr, match="deconvolution 'up': group=5"):
        prototxt.conv_ops(FCN.replace("kernel_size: 4 stride: 2", "kernel_size: 4 stride: 2 group: 5"), 2)
