"""Host-side tests (no GPU) of the depthwise channels-last bf16 convolution, hip_conv_nhwc_dw: the annotation, the planner's choice on MobileNet's shapes, the refusals
(each by the field it names) and the call list of MobileNet-v1 on a recording backend."""
import re

import pytest

from boda_amd import nhwc
from boda_amd.cnn_op import OpTune, add_codegen_annotations, pipe_func_args
from boda_amd.conv_pipe import ConvPipeFwd, DryRtc, mobilenet_v1
from boda_amd.op import UnsupErr, parse_op
from boda_amd.rtc import explain_plan

NHWC = dict(hip_dtype="bf16", hip_layout="nhwc")
LDS_BUDGET = 32 * 1024   # kDwLdsBudget of csrc/native_plan.cc


def dw_op(B, C, H, W, K, S, P, OC=None, group=None):
    OC = C if OC is None else OC; group = C if group is None else group
    OH, OW = (H + 2 * P - K) // S + 1, (W + 2 * P - K) // S + 1
    return parse_op(f"(str_vals=(type=Convolution),nda_vals=(biases=(dims=(out_chan={OC})),filts=(dims=(out_chan={OC},in_chan={C // group},y={K},x={K})),group=(tn=uint32_t,v={group}),"
                    f"in=(dims=(img={B},chan={C},y={H},x={W})),in_pad=(tn=none,dims=(y={P},x={P})),kern_sz=(tn=none,dims=(y={K},x={K})),"
                    f"out=(dims=(img={B},chan={OC},y={OH},x={OW})),out_chans=(tn=uint32_t,v={OC}),stride=(tn=none,dims=(y={S},x={S}))))")


@pytest.mark.parametrize("case,out", [((2, 8, 5, 7, 3, 1, 1), ""), ((1, 24, 9, 10, 3, 2, 1), "f32")])
def test_annotation(case, out):
    B, C, H, W, K, S, P = case
    a = add_codegen_annotations(dw_op(*case), OpTune(hip_out=out, **NHWC))
    OH, OW = (H + 2 * P - K) // S + 1, (W + 2 * P - K) // S + 1
    assert a.get_func_name() == "hip_conv_nhwc_dw"
    assert (a.get_dims("in").names, a.get_dims("in").sizes, a.get_dims("in").tn) == (("img", "y", "x", "chan"), (B, H, W, C), "bfloat16")
    assert (a.get_dims("filts").names, a.get_dims("filts").sizes, a.get_dims("filts").tn) == (("y", "x", "chan"), (K, K, C), "bfloat16")
    assert (a.get_dims("out").names, a.get_dims("out").sizes, a.get_dims("out").tn) == (("img", "y", "x", "chan"), (B, OH, OW, C), "float" if out else "bfloat16")
    assert a.get_dims("filts_ref").sizes == (C, 1, K, K) and a.get_dims("in_ref").sizes == (B, C, H, W) and a.get_dims("out_ref").sizes == (B, C, OH, OW)
    assert [n for n, _ in pipe_func_args(a)] == ["filts", "biases", "in", "stride", "in_pad", "out"]
    assert not nhwc.set_eligible(a) and not nhwc.multi_eligible(a)
    assert "hip_tile" not in add_codegen_annotations(dw_op(*case), OpTune(hip_tile="64x128x64x2x2", **NHWC)).str_vals      # another kernel's tile passes by
    assert add_codegen_annotations(dw_op(*case), OpTune(hip_tile="dw:2x4x1", **NHWC)).str_vals["hip_tile"] == "dw:2x4x1"


@pytest.mark.parametrize("case", [(64, 32, 112, 112, 3, 1, 1), (64, 1024, 7, 7, 3, 1, 1)], ids=["112x112x32", "7x7x1024"])
def test_plan_on_mobilenet_shapes(case):
    plan = explain_plan(add_codegen_annotations(dw_op(*case), OpTune(**NHWC)), 256)
    assert plan.split()[0] == "bodahip_conv_nhwc_dw_bf16", plan
    grid, block, lds = (int(re.search(rf" {k}=(\d+)", plan).group(1)) for k in ("grid", "block", "lds"))
    assert 0 < lds <= LDS_BUDGET and grid >= 2 * 256 and block <= 256, plan
    assert explain_plan(add_codegen_annotations(dw_op(*case), OpTune(hip_tile="dw:7x7x4", **NHWC)), 256).split()[1].startswith("7x7x4_")      # a forced split


def test_refusals_name_the_field():
    ok = (2, 16, 9, 9, 3, 1, 1)
    for kw, m in ((dict(OC=32), "group=16: a grouped convolution has no form"), (dict(group=2), "group=2: a grouped"), (dict(group=4, OC=32), "group=4: a grouped")):
        with pytest.raises(UnsupErr, match=m):      # channel multiplier 2, in.chan/group > 1: the grouped family's refusal, as before
            add_codegen_annotations(dw_op(*ok, **kw), OpTune(**NHWC))
    with pytest.raises(UnsupErr, match="hip_conv_nhwc_dw: out_chan=32"):      # the annotator itself names the channel multiplier
        nhwc.annotate_dw(dw_op(*ok, OC=32))
    for case, m in (((2, 12, 9, 9, 3, 1, 1), "in.chan=12"), ((1, 8, 9, 9, 3, 3, 1), "stride 3 x 3"), ((1, 8, 9, 9, 3, 1, 3), "in_pad 3 x 3")):
        with pytest.raises(UnsupErr, match=m):
            add_codegen_annotations(dw_op(*case), OpTune(**NHWC))
    with pytest.raises(UnsupErr, match="kern_sz 9 x 9"):
        add_codegen_annotations(dw_op(1, 8, 12, 12, 9, 1, 4), OpTune(**NHWC))
    for tune in (OpTune(hip_dtype="bf16"), OpTune(hip_algo="winograd", **NHWC), OpTune(k1conv=1, **NHWC), OpTune(tconv=1, **NHWC), OpTune(ipconv=1, **NHWC), OpTune(use_culibs=1, **NHWC)):
        with pytest.raises(UnsupErr, match="group=16"):      # a depthwise op under any other tune: the grouped family's refusal, as before
            add_codegen_annotations(dw_op(*ok), tune)
    a = add_codegen_annotations(dw_op(*ok), OpTune(**NHWC))
    for what, call in (("fuse_residual", lambda: nhwc.fuse_residual(a.copy())), ("fuse_pool", lambda: nhwc.fuse_pool(a.copy(), a.get_dims("in_ref"), (3, 3), (1, 1))),
                       ("fuse_post", lambda: nhwc.fuse_post(a.copy(), a.get_dims("out_ref"), (3, 3), (2, 2), (0, 0))), ("hip_conv_nhwc_grp", lambda: nhwc.annotate_group([a, a])),
                       ("hip_conv_nhwc_set", lambda: nhwc.annotate_set([a, a])), ("hip_conv_nhwc_multi", lambda: nhwc.annotate_multi([a, a]))):
        with pytest.raises(UnsupErr, match=what + ": hip_conv_nhwc_dw"):
            call()
    for tile, m in (("dw:0x4x1", "unsupported tile configuration dw:0x4x1"), ("dw:4x600x2", "unsupported tile configuration"), ("dw:4x4", "bad tile")):
        with pytest.raises(UnsupErr, match=m):
            explain_plan(a, 256, tile)


def test_mobilenet_call_list_on_a_recording_backend():
    cp = mobilenet_v1(2, 32, 0.25)
    assert [t for t in cp.nodes if "/" in t] == [] and cp.nodes[cp.out_node()].sizes == (2, 1000, 1, 1)
    dry = DryRtc(); fwd = ConvPipeFwd(dry, OpTune(**NHWC)); fwd.init(cp)
    funcs = {c.tag: c.func for c in fwd.fwd_calls}
    dw = [f"conv{i}_dw" for i in range(2, 15)]
    assert [funcs[t] for t in dw] == ["hip_conv_nhwc_dw"] * 13
    others = {t: f for t, f in funcs.items() if t not in dw and f.startswith("hip_conv")}
    assert len(others) >= 1 and all(f.startswith("hip_conv_nhwc") and f != "hip_conv_nhwc_dw" for f in others.values()), others
    assert not any(f in ("nhwc_relu", "hip_chan_affine") for f in funcs.values())      # every BatchNorm / Scale / ReLU run is folded into its convolution
    dry = DryRtc(); fwd = ConvPipeFwd(dry); fwd.init(cp)                                # the fp32 path takes the same net as it stands
    assert [c.func for c in fwd.fwd_calls if c.tag in dw] == ["hip_conv_grp"] * 13
