"""Host-side tests (no GPU) of hip_bconv_fb_nhwc, the filter and bias gradient from channels-last bf16 tensors: the annotation and its arg list, one refusal per scope
rule from the annotator and from the backend (each by the field it names), the planner's choice on two ResNet-50 layers at 32 images, forced and foreign tiles, and
the cross-compile for gfx950."""
import re

import pytest

from boda_amd import nhwc
from boda_amd.cnn_op import NATIVE_ARGS
from boda_amd.op import Nda, UnsupErr, parse_op
from boda_amd.rtc import explain_plan, func_args, native_funcs, prebuild
from test_gpu_bconv_fb_nhwc import bck_op

LDS_BUDGET, NUM_CUS = 80 * 1024, 256   # kFbnLdsBudget of csrc/native_plan.cc: two workgroups per CU


def raw_fop(B, C, OC, H, W, K, S, P, group=0):
    """The function op written out, past the annotator: what the backend alone has to refuse."""
    OH, OW = (H + 2 * P - K) // S + 1, (W + 2 * P - K) // S + 1
    return parse_op(f"(str_vals=(func_name=hip_bconv_fb_nhwc,type=BckConv),nda_vals=(biases_grad_loss=(dims=(out_chan={OC})),filts_grad_loss=(dims=(out_chan={OC},y={K},x={K},in_chan={C})),"
                    + (f"group=(tn=uint32_t,v={group})," if group else "") +
                    f"in=(tn=bfloat16,dims=(img={B},y={H},x={W},chan={C})),in_pad=(tn=none,dims=(y={P},x={P})),out_grad_loss=(tn=bfloat16,dims=(img={B},y={OH},x={OW},chan={OC})),"
                    f"stride=(tn=none,dims=(y={S},x={S}))))")


def test_annotation():
    f = nhwc.annotate_bconv_fb(bck_op(2, 40, 72, 6, 9, 3, (2, 1), 1))
    assert f.get_func_name() == nhwc.BCONV_FB_FUNC == "hip_bconv_fb_nhwc" and f.get_type() == "BckConv"
    assert func_args(f) == NATIVE_ARGS["hip_bconv_fb_nhwc"] == NATIVE_ARGS["hip_bconv_filts_biases"]
    want = {"in": (("img", "y", "x", "chan"), (2, 6, 9, 40), "bfloat16"), "out_grad_loss": (("img", "y", "x", "chan"), (2, 3, 9, 72), "bfloat16"),
            "filts_grad_loss": (("out_chan", "y", "x", "in_chan"), (72, 3, 3, 40), "float"), "biases_grad_loss": (("out_chan",), (72,), "float")}
    assert {an: (f.get_dims(an).names, f.get_dims(an).sizes, f.get_dims(an).tn) for an in want} == want
    assert "hip_tile" not in f.str_vals and nhwc.annotate_bconv_fb(bck_op(1, 8, 8, 3, 3, 1, 1, 0), "fbn:32x32x16x1").str_vals["hip_tile"] == "fbn:32x32x16x1"
    row = native_funcs()["hip_bconv_fb_nhwc"]
    assert (row["family"], row["be"], row["multi_dev"], row["flags"], row["opt"]) == ("bconv_nhwc", ("hip",), "one_device", (), ())


@pytest.mark.parametrize("case,field", [((1, 12, 8, 5, 5, 1, 1, 0), "in.chan=12"), ((1, 8, 20, 5, 5, 1, 1, 0), "out_grad_loss.chan=20"), ((1, 8, 8, 9, 9, 8, 1, 0), "kern_sz 8 x 8"),
                                        ((1, 8, 8, 9, 9, 3, 3, 0), "stride 3 x 3"), ((1, 8, 8, 5, 5, 1, 1, 1), "in_pad 1 x 1"), ((1, 8, 8, 5, 5, 1, 1, 0, 2), "group=2")])
def test_refusals_name_the_field(case, field):
    bare = bck_op(*case[:8])
    if len(case) > 8:
        bare.nda_vals["group"] = Nda(None, "uint32_t", (case[8],))
    for refuse in (lambda: nhwc.annotate_bconv_fb(bare), lambda: explain_plan(raw_fop(*case)), lambda: prebuild(raw_fop(*case))):
        with pytest.raises(UnsupErr, match="^(error: )?hip_bconv_fb_nhwc: " + re.escape(field)):     # (the backend's message carries its "error: " in front)
            refuse()


@pytest.mark.parametrize("case", [(32, 64, 64, 56, 56, 1, 1, 0), (32, 256, 256, 14, 14, 3, 1, 1)], ids=["56x56_64_1x1", "14x14_256_3x3"])
def test_planner_fills_the_chip_inside_the_lds_budget(case):
    plan = explain_plan(nhwc.annotate_bconv_fb(bck_op(*case)), NUM_CUS)
    f = {k: int(v) for k, v in re.findall(r"(grid|block|lds|ksl)=(\d+)", plan)}
    assert plan.split()[0] == "bodahip_bconv_fb_nhwc_bf16" and plan.endswith("| bodahip_bconv_slab_sum"), plan
    assert f["lds"] <= LDS_BUDGET and 1 < f["ksl"] <= 1024 and f["grid"] >= NUM_CUS, plan


def test_forced_and_foreign_tiles():
    f = nhwc.annotate_bconv_fb(bck_op(2, 40, 72, 6, 9, 3, 1, 1))
    planned = explain_plan(f)
    forced = explain_plan(f, tile="fbn:32x64x16x3x8")
    assert forced.split()[1] == "32x64x16_w1x2_s3" and "ksl=3" in forced and "xb=8" in forced and forced != planned, forced
    assert explain_plan(f, tile="64x64x16x2x2") == planned and explain_plan(f, tile="dwpw:2x3x1") == planned          # another function's tile passes by
    assert "ksl=2 " in explain_plan(nhwc.annotate_bconv_fb(bck_op(2, 8, 8, 5, 5, 1, 1, 0), "fbn:32x32x16x3"))          # 4 stages: KSL 3 -> 2 slices of 2, none empty
    with pytest.raises(UnsupErr, match="hip_bconv_fb_nhwc: unsupported tile configuration fbn:48x64x16x1"):
        explain_plan(f, tile="fbn:48x64x16x1")
    other = parse_op("(str_vals=(type=BckConv,func_name=hip_bconv_filts_biases),nda_vals=(biases=(dims=(out_chan=16)),biases_grad_loss=(dims=(out_chan=16)),filts=(dims=(out_chan=16,in_chan=8,y=1,x=1)),"
                     "filts_grad_loss=(dims=(out_chan=16,in_chan=8,y=1,x=1)),in=(dims=(img=2,chan=8,y=5,x=5)),in_grad_loss=(dims=(img=2,chan=8,y=5,x=5)),in_pad=(tn=none,dims=(y=0,x=0)),"
                     "kern_sz=(tn=none,dims=(y=1,x=1)),out_chans=(tn=uint32_t,v=16),out_grad_loss=(dims=(img=2,chan=16,y=5,x=5)),stride=(tn=none,dims=(y=1,x=1))))")
    assert explain_plan(other, tile="fbn:32x64x16x3") == explain_plan(other)                                            # and a fbn: tile passes the others by


@pytest.mark.parametrize("case,tile", [((2, 40, 72, 6, 9, 3, 1, 1), ""), ((3, 8, 16, 9, 9, 3, 2, 1), "fbn:32x64x16x3x8")])
def test_prebuild_cross_compiles(case, tile):
    assert prebuild(nhwc.annotate_bconv_fb(bck_op(*case), tile)) > 1000
