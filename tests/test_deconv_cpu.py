"""The Deconvolution family and Crop on be=cpu, the op types and the annotators (no GPU).
  * the four be=cpu functions equal the existing functions on exchanged roles, bit for bit (tests/deconv_ref.py: exchanged)
  * they stay within (n + 1) * 2^-24 * sum |terms| of float64 (torch conv_transpose2d and autograd), n the chain length
  * the dims rule OH = (H-1)*S + K - 2*P, the inverse of the convolution's; refusals by name; the planner's strings
  * hip_crop / hip_crop_bck against numpy, the +0 outside the window by bits"""
import numpy as np
import pytest

from boda_amd import rtc as rtc_mod
from boda_amd.cnn_op import BCK_DECONV_FUNCS, DECONV_FUNC, NATIVE_ARGS, OpTune, add_bck_deconv_annotations, add_bck_op_annotations, add_deconv_annotations
from boda_amd.op import RtErr, UnsupErr, parse_op
from boda_amd.rtc import make_rtc

from boda_amd.cnn_op import bck_deconv_calls, deconv_calls, deconv_form

from deconv_ref import (CASE_IDS, CASES, CROP_CASES, MATRIX_CASES, PLANNER_MATRIX, bck_deconv_op, bits_equal, can_matrix, crop_ops, deconv_funcs, deconv_op, exchanged, out_plane, path_calls,
                        rand_ins, run_calls, run_func, torch_twin, within_f64_bound)


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_functions_are_the_exchanged_roles(cpu, case):
    ins = rand_ins(case, 7)
    funcs = deconv_funcs(case)
    twin = torch_twin(case, ins)
    for which in ("fwd", "in", "biases", "filts"):
        got, _ = run_func(cpu, funcs[which], ins)
        assert bits_equal(got, exchanged(cpu, case, ins, which)), (case, which)
        assert within_f64_bound(got, twin, case, which), (case, which)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_both_paths_are_one_function_on_cpu(cpu, case):
    """The planner's choice and both forced paths, bound by role as a driver binds them (views of the blob under the exchanged dims, the ones / zeros constants):
    on be=cpu every path is the same loops, so all of them give the direct function's bits."""
    ins = rand_ins(case, 7)
    for which in ("fwd", "in", "biases", "filts"):
        want, _ = run_func(cpu, deconv_funcs(case)[which], ins)
        for form in ("", "direct") + (("matrix",) if can_matrix(case) else ()):
            op, calls = path_calls(case, which, form)
            got, _ = run_calls(cpu, op, calls, ins, which, guards=True)
            assert bits_equal(got, want), (case, which, form)


def test_planner_rule_and_forcing_tiles():
    """The rule reads the op alone: direct where min(C, OC) < 32 and a gradient's chain max(C, OC) x KH x KW is below 1024 terms, or the exchanged geometry is outside
    an existing function's limits (strides above 16); else matrix."""
    names = lambda calls: [f.get_func_name() for f, _ in calls]
    for case in CASES:
        want = "matrix" if case in PLANNER_MATRIX else "direct"
        assert deconv_form(deconv_op(case), OpTune()) == want and deconv_form(bck_deconv_op(case), OpTune()) == want, case
    wide_far = (1, 64, 2, 2, 64, (64, 64), (32, 32), (0, 0))   # wide, but stride 32 is outside hip_bconv_in's limits
    assert deconv_form(deconv_op(wide_far), OpTune()) == "direct" and deconv_form(deconv_op((1, 32, 4, 4, 32, (4, 4), (2, 2), (1, 1))), OpTune()) == "matrix"
    assert deconv_form(deconv_op((1, 31, 4, 4, 63, (4, 4), (2, 2), (1, 1))), OpTune()) == "direct" and deconv_form(deconv_op((1, 31, 4, 4, 64, (4, 4), (2, 2), (1, 1))), OpTune()) == "matrix"
    for k, s, hw, want in ((4, 2, 16, "direct"), (16, 8, 34, "matrix"), (64, 32, 16, "direct")):   # FCN's three heads at 21 channels
        assert deconv_form(deconv_op((8, 21, hw, hw, 21, (k, k), (s, s), (0, 0))), OpTune()) == want
    m, d = MATRIX_CASES[0], CASES[0]
    assert names(deconv_calls(deconv_op(m), OpTune())) == ["hip_bconv_in", "hip_chan_affine"]
    assert names(bck_deconv_calls(bck_deconv_op(m), OpTune())) == ["hip_conv", "hip_deconv_bck_biases", "hip_bconv_filts"]
    assert names(deconv_calls(deconv_op(d), OpTune())) == ["hip_deconv"]
    assert names(bck_deconv_calls(bck_deconv_op(d), OpTune())) == ["hip_deconv_bck_in", "hip_deconv_bck_biases", "hip_deconv_bck_filts"]
    # a tile string forces either path and travels with that path's functions
    forced = bck_deconv_calls(bck_deconv_op(m), OpTune(hip_tile="1x1x10x2x2x1x3"))
    assert names(forced) == ["hip_deconv_bck_in", "hip_deconv_bck_biases", "hip_deconv_bck_filts"] and forced[2][0].str_vals["hip_tile"] == "1x1x10x2x2x1x3"
    forced = bck_deconv_calls(bck_deconv_op(d), OpTune(hip_tile="32x32x16x1x4"))
    assert names(forced) == ["hip_conv", "hip_deconv_bck_biases", "hip_bconv_filts"] and forced[0][0].str_vals["hip_tile"] == "32x32x16x1x4"
    assert names(deconv_calls(deconv_op(d), OpTune(hip_tile="32x32x16x1x4"))) == ["hip_bconv_in", "hip_chan_affine"]
    with pytest.raises(UnsupErr, match="asks for the matrix path, but stride 32 x 32 is outside"):
        deconv_calls(deconv_op(CASES[1]), OpTune(hip_tile="32x32x16x1x4"))
    a, b = deconv_calls(deconv_op(m), OpTune())   # the matrix forward: no ReLU on the affine, the bias through a view named as hip_chan_affine names it
    assert b[0].get_u32("relu") == 0 and b[1] == {"in": "out", "a": "ones", "b": "biases_x", "out": "out"} and a[1]["filts"] == "filts_x"
    assert bck_deconv_calls(bck_deconv_op(m), OpTune())[0][0].get_u32("conv_has_relu") == 0


def test_unreached_outputs_are_the_bias(cpu):
    case = CASES[6]   # 1x1 at stride 2: the odd rows and columns meet no term
    ins = rand_ins(case, 7)
    got, _ = run_func(cpu, deconv_funcs(case)["fwd"], ins)
    want = np.broadcast_to((np.float32(0.0) + ins["biases"]).reshape(1, -1, 1, 1), got.shape)
    assert bits_equal(got[:, :, 1::2, :], want[:, :, 1::2, :]) and bits_equal(got[:, :, :, 1::2], want[:, :, :, 1::2])


def test_dims_are_the_inverse_of_the_convolution():
    """OH = (H-1)*S + K - 2*P: the input size a convolution of (K, S, P) needs for H outputs when the division leaves no rest (the reference's conv_out_sz_to_in_sz,
    src/conv_util.cc:224, without its padding term subtracted twice)."""
    for H, K, S, P, want in ((16, 4, 2, 0, 34), (34, 16, 8, 0, 280), (16, 64, 32, 0, 544), (4, 4, 2, 1, 8), (5, 3, 2, 0, 11), (3, 1, 2, 0, 5), (28, 4, 2, 1, 56)):
        case = (1, 2, H, H, 3, (K, K), (S, S), (P, P))
        assert out_plane(case) == (want, want)
        g = deconv_op(case).deconv_geom()
        assert (g["OH"], g["OW"]) == (want, want) and (want + 2 * P - K) // S + 1 == H   # a convolution of the same (K, S, P) maps it back
        assert deconv_op(case).flops() == 2 * 1 * 2 * H * H * 3 * K * K and bck_deconv_op(case).flops() == 2 * deconv_op(case).flops()
    with pytest.raises(RtErr, match=r"out OH=9 != \(H-1\)\*SY\+KH-2\*PY = 8"):
        parse_op("(str_vals=(type=Deconvolution),nda_vals=(biases=(dims=(out_chan=2)),filts=(dims=(in_chan=2,out_chan=2,y=4,x=4)),in=(dims=(img=1,chan=2,y=4,x=4)),"
                 "out=(dims=(img=1,chan=2,y=9,x=8)),in_pad=(tn=none,dims=(y=1,x=1)),kern_sz=(tn=none,dims=(y=4,x=4)),out_chans=(tn=uint32_t,v=2),stride=(tn=none,dims=(y=2,x=2))))")


def test_refusals_by_name(cpu):
    case = CASES[0]
    with pytest.raises(UnsupErr, match="group=2: a Deconvolution with group > 1 is out of scope"):
        deconv_op(case, extra="group=(tn=uint32_t,v=2),")
    with pytest.raises(UnsupErr, match="conv_has_relu=1: a Deconvolution has no fused ReLU"):
        deconv_op(case, extra="conv_has_relu=(tn=uint32_t,v=1),")
    with pytest.raises(RtErr, match="filts must be in_chan:out_chan:y:x"):
        parse_op("(str_vals=(type=Deconvolution),nda_vals=(biases=(dims=(out_chan=2)),filts=(dims=(out_chan=2,in_chan=2,y=4,x=4)),in=(dims=(img=1,chan=2,y=4,x=4)),"
                 "out=(dims=(img=1,chan=2,y=8,x=8)),in_pad=(tn=none,dims=(y=1,x=1)),kern_sz=(tn=none,dims=(y=4,x=4)),out_chans=(tn=uint32_t,v=2),stride=(tn=none,dims=(y=2,x=2))))")
    for tune in (OpTune(hip_dtype="bf16"), OpTune(hip_layout="nhwc"), OpTune(use_culibs=1)):
        with pytest.raises(UnsupErr, match="a Deconvolution has no form under op_tune"):
            add_deconv_annotations(deconv_op(case), tune)
        with pytest.raises(UnsupErr, match="a Deconvolution has no form under op_tune"):
            add_bck_deconv_annotations(bck_deconv_op(case), tune)
    # the backend refuses a function op whose op grew a group or a ReLU behind the annotator's back, and a call on the wrong var
    f = deconv_funcs(case)["fwd"].copy(); f.set_u32("group", 3)
    with pytest.raises(Exception, match="hip_deconv: the op carries group=3"):
        run_func(cpu, f, rand_ins(case, 1))
    f = deconv_funcs(case)["fwd"].copy(); f.set_u32("conv_has_relu", 1)
    with pytest.raises(Exception, match="hip_deconv: the op carries conv_has_relu=1"):
        run_func(cpu, f, rand_ins(case, 1))
    big = (2, 3, 5, 4, 5, (65, 4), (2, 2), (1, 1))
    with pytest.raises(Exception, match="hip_deconv: unsupported geometry"):
        run_func(cpu, deconv_funcs(big)["fwd"], rand_ins(big, 1))


def test_table_and_plans():
    table = rtc_mod.native_funcs()
    for fn in (DECONV_FUNC,) + BCK_DECONV_FUNCS:
        r = table[fn]
        assert r["family"] == "deconv" and r["multi_dev"] == "one_device" and set(r["be"]) == {"hip", "cpu"} and not r["flags"], r
        assert rtc_mod.func_args(parse_op(f"(str_vals=(type={r['types'][0]},func_name={fn}),nda_vals=())")) == NATIVE_ARGS[fn]
    assert [table[fn]["member"] for fn in (DECONV_FUNC,) + BCK_DECONV_FUNCS] == [1, 2, 3, 4]
    for fn, t in (("hip_crop", "Crop"), ("hip_crop_bck", "BckCrop")):
        assert table[fn]["family"] == "bck_op" and table[fn]["types"] == (t,) and table[fn]["multi_dev"] == "on_shards"
    # the planner reads the op alone: FCN's 4/2 head at 8 images has few outputs and a long K, so its filter gradient is sliced; the 64/32 head's is not
    head = lambda k, s, hw: deconv_funcs((8, 21, hw, hw, 21, (k, k), (s, s), (0, 0)))
    p = rtc_mod.explain_plan(head(4, 2, 16)["filts"])
    assert p.startswith("bodahip_deconv_bck_filts_direct 1x1x32_w2x2_s") and p.endswith("| bodahip_deconv_bck_filts_slab_sum"), p
    p = rtc_mod.explain_plan(head(64, 32, 16)["filts"])
    assert p.startswith("bodahip_deconv_bck_filts_direct 1x1x32_w2x2 grid="), p
    assert rtc_mod.explain_plan(head(64, 32, 16)["fwd"]).startswith("bodahip_deconv_direct 1x4x1_w2x2 grid=")
    assert rtc_mod.explain_plan(head(64, 32, 16)["in"]).startswith("bodahip_deconv_bck_in_direct 1x1x1_w2x2 grid=")
    f = head(4, 2, 16)["filts"].copy(); f.str_vals["hip_tile"] = "1x1x10x2x2x1x3"
    assert rtc_mod.explain_plan(f).startswith("bodahip_deconv_bck_filts_direct 1x1x10_w2x2_s3 ")
    f.str_vals["hip_tile"] = "1x1x10x2x2x1x2000"
    with pytest.raises(Exception, match="hip_deconv_bck_filts: unsupported tile configuration"):
        rtc_mod.explain_plan(f)


@pytest.mark.parametrize("c", CROP_CASES, ids=["x".join(str(v) for v in c) for c in CROP_CASES])
def test_crop(cpu, c):
    B, C, H, W, OH, OW, oy, ox = c
    fwd, bck = crop_ops(*c)
    (ff,), (fb,) = add_bck_op_annotations(fwd, OpTune()), add_bck_op_annotations(bck, OpTune())
    rng = np.random.default_rng(3)
    a = rng.uniform(-5, 5, (B, C, H, W)).astype(np.float32)
    g = -np.abs(rng.uniform(0.5, 5, (B, C, OH, OW))).astype(np.float32)   # (all negative: a -0 outside the window would show)
    got, _ = run_func(cpu, ff, {"in": a}, guards=True)
    assert bits_equal(got, a[:, :, oy:oy + OH, ox:ox + OW])
    want = np.zeros((B, C, H, W), np.float32); want[:, :, oy:oy + OH, ox:ox + OW] = g
    got, _ = run_func(cpu, fb, {"out_grad_loss": g}, guards=True)
    assert bits_equal(got, want)


def test_crop_refusals():
    with pytest.raises(RtErr, match=r"Crop: offset \(3, 0\) \+ window \(8, 8\) exceeds the plane \(10, 10\)"):
        crop_ops(2, 3, 10, 10, 8, 8, 3, 0)
    with pytest.raises(RtErr, match="differs from the plane's tensor"):
        parse_op("(str_vals=(type=Crop),nda_vals=(in=(dims=(img=2,chan=3,y=10,x=10)),out=(dims=(img=2,chan=4,y=8,x=8)),offset=(tn=none,dims=(y=1,x=1))))")
