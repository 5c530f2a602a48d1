"""Host-side tests (no GPU) of the fused depthwise + pointwise pair, hip_conv_nhwc_dw_pw: the annotation and its arg list, the refusals (each by the field it names),
the planner's choice on MobileNet's first and last pair, and the call lists of the forward pipe on a recording backend."""
import re

import pytest

from boda_amd import nhwc
from boda_amd.cnn_op import NATIVE_ARGS, OpTune, add_codegen_annotations, pipe_func_args
from boda_amd.conv_pipe import ConvPipe, ConvPipeFwd, DryRtc, PipeOp, mobilenet_v1
from boda_amd.op import Dims, Nda, RtErr, UnsupErr, parse_op
from boda_amd.rtc import explain_plan

NHWC = dict(hip_dtype="bf16", hip_layout="nhwc")
LDS_BUDGET = 80 * 1024   # kDwpwLdsBudget of csrc/native_plan.cc: two workgroups per CU


def conv(B, C, H, W, K, S, P, OC, group=1, out="", tile=""):
    OH, OW = (H + 2 * P - K) // S + 1, (W + 2 * P - K) // S + 1
    op = parse_op(f"(str_vals=(type=Convolution),nda_vals=(biases=(dims=(out_chan={OC})),filts=(dims=(out_chan={OC},in_chan={C // group},y={K},x={K})),"
                  + (f"group=(tn=uint32_t,v={group})," if group > 1 else "") +
                  f"in=(dims=(img={B},chan={C},y={H},x={W})),in_pad=(tn=none,dims=(y={P},x={P})),kern_sz=(tn=none,dims=(y={K},x={K})),"
                  f"out=(dims=(img={B},chan={OC},y={OH},x={OW})),out_chans=(tn=uint32_t,v={OC}),stride=(tn=none,dims=(y={S},x={S}))))")
    return add_codegen_annotations(op, OpTune(hip_out=out, hip_tile=tile, **NHWC))


def pair(B, C, H, OC, K=3, S=1, P=1, K2=1, S2=1, P2=0, out=""):
    dw = conv(B, C, H, H, K, S, P, C, group=C); OH = dw.get_dims("out").dsz("y")
    return dw, conv(B, C, OH, OH, K2, S2, P2, OC, out=out)


@pytest.mark.parametrize("out", ["", "f32"])
def test_annotation(out):
    dw, pw = pair(2, 24, 9, 40, S=2, out=out)
    assert nhwc.dw_pw_applies(dw, pw)
    pw.nda_vals["conv_has_relu"].v = (0,)
    f = nhwc.annotate_dw_pw(dw, pw)
    assert f.get_func_name() == "hip_conv_nhwc_dw_pw" and pipe_func_args(f) == NATIVE_ARGS["hip_conv_nhwc_dw_pw"]
    assert [n for n, _ in pipe_func_args(f)] == ["filts", "biases", "filts2", "biases2", "in", "stride", "in_pad", "out"]
    assert f.get_dims("in") == dw.get_dims("in") and f.get_dims("filts") == dw.get_dims("filts") and f.get_dims("stride") == dw.get_dims("stride")
    assert (f.get_dims("filts2").names, f.get_dims("filts2").sizes) == (("out_chan", "y", "x", "in_chan"), (40, 1, 1, 24))
    assert (f.get_dims("out").sizes, f.get_dims("out").tn) == ((2, 5, 5, 40), "float" if out else "bfloat16")
    assert (f.get_u32("conv_has_relu"), f.get_u32("conv2_has_relu"), f.get_u32("group")) == (1, 0, 24)
    assert "hip_tile" not in f.str_vals and nhwc.annotate_dw_pw(dw, pw, "dwpw:2x3x1").str_vals["hip_tile"] == "dwpw:2x3x1"
    for other in (conv(2, 24, 9, 9, 3, 1, 1, 24, group=24, tile="dwpw:2x3x1"), conv(2, 24, 9, 9, 1, 1, 0, 40, tile="dwpw:2x3x1")):     # a dwpw: tile passes every other function by
        assert "hip_tile" not in other.str_vals


@pytest.mark.parametrize("kw,field", [(dict(K2=3, P2=1), "kern_sz is 3 x 3"), (dict(S2=2), "stride is 2 x 2"), (dict(OC=20), "out_chan=20"), (dict(C=1032), "in.chan=1032"),
                                      (dict(K=7, P=3), "kern_sz 7 x 7")])
def test_refusals_name_the_field(kw, field):
    a = dict(B=1, C=16, H=14, OC=16); a.update(kw)
    dw, pw = pair(**a)
    assert not nhwc.dw_pw_applies(dw, pw)
    with pytest.raises(UnsupErr, match="hip_conv_nhwc_dw_pw: .*" + field):
        nhwc.annotate_dw_pw(dw, pw)


def test_flagged_consumers_and_planner_refusals():
    dw, pw = pair(2, 16, 14, 16)
    for flag in ("nhwc_residual", "nhwc_pool"):
        q = pw.copy(); q.nda_vals[flag] = Nda(None, "uint32_t", (1,))
        assert not nhwc.dw_pw_applies(dw, q)
        with pytest.raises(UnsupErr, match=flag + "=1"):
            nhwc.annotate_dw_pw(dw, q)
    assert not nhwc.dw_pw_applies(pw, pw) and not nhwc.dw_pw_applies(dw, dw)
    f = nhwc.annotate_dw_pw(dw, pw)
    for tile, m in (("dwpw:0x4x1", "unsupported tile configuration dwpw:0x4x1"), ("dwpw:20x14x2", "unsupported tile configuration"), ("dwpw:4x4", "bad tile")):
        with pytest.raises(UnsupErr, match=m):
            explain_plan(f, 256, tile)
    g = f.copy(); g.nda_vals["filts2"] = Nda(dims=Dims(("out_chan", "y", "x", "in_chan"), (12, 1, 1, 16), "bfloat16"), tn="bfloat16")
    with pytest.raises(UnsupErr, match="filts2.out_chan=12"):     # the backend reads the same scope from the op
        explain_plan(g, 256)


@pytest.mark.parametrize("case", [(64, 32, 112, 64), (64, 1024, 7, 1024)], ids=["conv2", "conv14"])
def test_plan_on_mobilenet_pairs(case):
    f = nhwc.annotate_dw_pw(*pair(*case))
    plan = explain_plan(f, 256)
    assert plan.split()[0] == "bodahip_conv_nhwc_dwpw_bf16" and f"-DNOC={case[3]}" in plan, plan
    grid, block, lds = (int(re.search(rf" {k}=(\d+)", plan).group(1)) for k in ("grid", "block", "lds"))
    assert 0 < lds <= LDS_BUDGET and grid >= 256 and block % 64 == 0 and block <= 1024, plan
    assert explain_plan(f, 256, "dwpw:2x7x4").split()[1].startswith("2x7x4_")      # a forced split
    assert explain_plan(f, 256, "dw:2x7x4") == plan                                 # another function's tile passes by


def test_call_lists_on_a_recording_backend():
    cp = mobilenet_v1(2, 32, 0.25)
    fwd = ConvPipeFwd(DryRtc(), OpTune(**NHWC), fuse_dw_pw="all"); fwd.init(cp)
    funcs = [c.func for c in fwd.fwd_calls]
    assert funcs.count("hip_conv_nhwc_dw_pw") == 13 and "hip_conv_nhwc_dw" not in funcs and len(fwd.fused_dw_pw) == 13
    assert [c.tag for c in fwd.fwd_calls if c.func == "hip_conv_nhwc_dw_pw"] == [f"conv{i}_dw+conv{i}_sep" for i in range(2, 15)] and not fwd.level_sets and not fwd.groups
    call = next(c for c in fwd.fwd_calls if c.tag == "conv3_dw+conv3_sep")
    assert {a: v.n for a, v in call.rfc.arg_map.items() if v.is_var()} == {"filts": "conv3_dw_filts", "biases": "conv3_dw_biases", "filts2": "conv3_sep_filts", "biases2": "conv3_sep_biases",
                                                                         "in": "conv2_sep", "out": "conv3_sep"}
    with pytest.raises(RtErr, match="'conv3_dw' is never written"):     # the depthwise top has no var
        fwd.run_fwd([], {}, ["conv3_dw"])
    for kw in ({}, {"fuse_dw_pw": False}):     # the default call list is untouched
        fwd = ConvPipeFwd(DryRtc(), OpTune(**NHWC), **kw); fwd.init(cp)
        assert [c.func for c in fwd.fwd_calls].count("hip_conv_nhwc_dw") == 13 and not fwd.fused_dw_pw
    # a depthwise top with a second reader keeps its two calls
    p = ConvPipe("two_readers", "data", Dims.make("float", img=2, chan=16, y=8, x=8))
    p.add(PipeOp("dw", "Convolution", "data", "dw", out_chans=16, kern_sz=(3, 3), stride=(1, 1), in_pad=(1, 1), group=16))
    p.add(PipeOp("pw", "Convolution", "dw", "pw", out_chans=24, kern_sz=(1, 1)))
    p.add(PipeOp("pw_b", "Convolution", "dw", "pw_b", out_chans=8, kern_sz=(1, 1)))
    fwd = ConvPipeFwd(DryRtc(), OpTune(**NHWC), fuse_dw_pw="all", fuse_siblings=False, fuse_levels=False); fwd.init(p)
    assert [(c.tag, c.func) for c in fwd.fwd_calls if c.func.startswith("hip_conv")] == [("dw", "hip_conv_nhwc_dw"), ("pw", "hip_conv_nhwc"), ("pw_b", "hip_conv_nhwc")] and not fwd.fused_dw_pw
