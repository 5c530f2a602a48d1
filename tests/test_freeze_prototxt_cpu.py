"""prototxt.freeze_spec: what a net definition says about fine-tuning (lr_mult: 0 on every blob of a layer, use_global_stats on a BatchNorm) as a bck_pipe.Freeze,
on a small hand-written net (tests/golden/freeze_net.prototxt), its refusals, and the Freeze it gives on a driver."""
import os

import pytest

import bn_ref as R
from boda_amd import prototxt
from boda_amd.bck_pipe import ConvPipeBck, Freeze, add_bck_ops, host_params
from boda_amd.conv_pipe import ConvPipe, PipeOp
from boda_amd.op import Dims, RtErr
from boda_amd.rtc import make_rtc

TEXT = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "freeze_net.prototxt")).read()


def the_pipe(B=2):
    """The fixture's net as a ConvPipe, its layers' names the op tags."""
    p = ConvPipe("freeze_net", "data", Dims.make("float", img=B, chan=3, y=9, x=9))
    for i, (bot, k, pad) in enumerate((("data", 3, 1), ("conv1", 1, 0), ("conv2", 1, 0)), 1):
        t = f"conv{i}"
        p.add(PipeOp(t, "Convolution", bot, t, out_chans=8, kern_sz=(k, k), in_pad=(pad, pad)))
        p.add(PipeOp(f"bn{i}", "BatchNorm", t, t)); p.add(PipeOp(f"scale{i}", "Scale", t, t))
        if i == 1:
            p.add(PipeOp("relu1", "ReLU", t, t))
    p.add(PipeOp("pool", "Pooling", "conv3", "pool", kern_sz=None, avg_pool=1))
    p.add(PipeOp("fc_fixed", "Convolution", "pool", "fc_fixed", out_chans=6, kern_sz=(1, 1)))
    p.add(PipeOp("fc", "Convolution", "fc_fixed", "fc", out_chans=5, kern_sz=(1, 1)))
    return p


def test_the_fixture_maps_to_its_freeze():
    want = Freeze(params=("conv1", "scale1", "fc_fixed"), bn_global_stats=["bn1"], keep_grads=())
    assert prototxt.freeze_spec(TEXT) == want
    assert prototxt.freeze_spec(TEXT, the_pipe()) == want
    # nothing fixed: an empty Freeze, bn_global_stats False
    plain = TEXT.replace("lr_mult: 0.0", "lr_mult: 1").replace("lr_mult: 0", "lr_mult: 1").replace("use_global_stats: true", "use_global_stats: false")
    assert prototxt.freeze_spec(plain) == Freeze()


def test_refusals():
    with pytest.raises(RtErr, match="freeze_spec: layer 'conv1' is no op of the pipe 'residual'"):
        prototxt.freeze_spec(TEXT, R.residual())
    bad = TEXT.replace('scale_param { bias_term: true } }\nlayer { name: "relu1"', 'batch_norm_param { use_global_stats: true } }\nlayer { name: "relu1"')
    assert bad != TEXT
    with pytest.raises(RtErr, match="freeze_spec: layer 'scale1' is a Scale, not a BatchNorm: use_global_stats is a BatchNorm layer's"):
        prototxt.freeze_spec(bad)
    with pytest.raises(RtErr, match="freeze_spec: layer 'conv2': lr_mult must be a number"):
        prototxt.freeze_spec(TEXT.replace("lr_mult: 2", "lr_mult: two"))


def test_the_freeze_on_a_driver():
    cp = the_pipe()
    bp = add_bck_ops(cp)
    cpu = make_rtc("(be=cpu)"); cpu.init()
    drv = ConvPipeBck(cpu, freeze=prototxt.freeze_spec(TEXT, cp))
    try:
        drv.init(bp, host_params(bp, 3))
        assert drv.frozen["params"] == ["conv1_filts", "conv1_biases", "scale1_scale", "scale1_bias", "fc_fixed_filts", "fc_fixed_biases"] and drv.frozen["bn_global"] == ["bn1"]
        fns = {t: f.get_func_name() for t, f, _ in drv.calls()}
        assert fns["bn1"] == "hip_bnf_prep" and fns["bn2"] == "hip_bn_stats" and "conv1_bck" not in fns and "bn1_bck" not in fns and "scale1_bck" not in fns and "relu1_bck" not in fns
        assert fns["fc_fixed_bck"] == "hip_bconv_in" and [t for t, _, _ in drv.calls()].count("fc_fixed_bck") == 1    # a frozen layer above trainable ones: its data gradient alone
        assert "scale2_scale" in drv.sgd_params and "scale2_bias" in drv.sgd_params
    finally:
        drv.release(); cpu.close()
