"""prototxt.loss_spec: a net definition's SoftmaxWithLoss layers -> (name, bottom, label, LossSpec), with Caffe's defaults, the legacy
`normalize:` key, the phase filter and the refusal of every other loss layer.  The definitions are tests/golden/loss_net.prototxt."""
import os

import pytest

from boda_amd.bck_graph import LossSpec
from boda_amd.op import RtErr, UnsupErr
from boda_amd.prototxt import loss_spec

HERE = os.path.dirname(os.path.abspath(__file__))


def nets():
    text = open(os.path.join(HERE, "golden", "loss_net.prototxt")).read()
    out = {}
    for blk in text.split("#== ")[1:]:
        head, body = blk.split("\n", 1)
        out[head.split(":")[0]] = body
    return out


def test_googlenet_heads():
    got = loss_spec(nets()["googlenet"])
    assert [(n, b, l) for n, b, l, _ in got] == [("loss1/loss", "loss1/classifier", "label"), ("loss2/loss", "loss2/classifier", "label"), ("loss3/loss3", "loss3/classifier", "label")]
    assert [s.weight for *_, s in got] == [0.3, 0.3, 1.0]
    assert all(s.ignore_label is None and s.normalization == "valid" for *_, s in got)   # Caffe's defaults


def test_loss_param_legacy_key_and_phases():
    got = {n: (b, s) for n, b, _, s in loss_spec(nets()["dense"])}
    assert list(got) == ["seg_loss", "old_loss", "old_loss_true", "both_keys"]   # definition order; the TEST-only layer is left out
    assert got["seg_loss"] == ("score", LossSpec(1.0, 255, "full"))
    assert got["old_loss"] == ("score2", LossSpec(0.5, None, "batch_size"))
    assert got["old_loss_true"] == ("score3", LossSpec(1.0, -1, "valid"))
    assert got["both_keys"][1].normalization == "none"   # normalization wins over the legacy key, as in Caffe
    test = [n for n, *_ in loss_spec(nets()["dense"], phase="TEST")]
    assert test == ["seg_loss", "old_loss", "old_loss_true", "test_only"]


def test_refusals():
    with pytest.raises(UnsupErr, match="EuclideanLoss"):
        loss_spec(nets()["euclid"])
    with pytest.raises(RtErr, match="phase must be"):
        loss_spec(nets()["dense"], phase="both")
    bad = 'layer { name: "l" type: "SoftmaxWithLoss" bottom: "a" bottom: "label" loss_param { normalization: MEAN } }'
    with pytest.raises(RtErr, match="'MEAN' is none of"):
        loss_spec(bad)
    with pytest.raises(RtErr, match="is not an integer"):
        loss_spec(bad.replace("normalization: MEAN", "ignore_label: 2.5"))
    with pytest.raises(RtErr, match="has 1 bottoms"):
        loss_spec('layer { name: "l" type: "SoftmaxWithLoss" bottom: "a" }')
