"""BckConv (the backward convolution) without a GPU: the op and its validation, the three annotated gradient functions, the native planner's plans for
every recorded shape (tests/golden/ops/bck-conv-ops.txt), and be=cpu's gradients -- the reference templates' fmaf chains in their own loop orders
(test/rtc/BckConv_*_grad_loss.cucl) -- against torch float64.

mrd here is max|x - r| / max|r| over a tensor (r the float64 result)."""
import os

import numpy as np
import pytest
import torch

from boda_amd import rtc as rtc_mod
from boda_amd.cnn_op import NATIVE_ARGS, OpTune, add_bck_conv_annotations, add_codegen_annotations
from boda_amd.op import RtErr, UnsupErr, parse_op, read_ops
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops", "bck-conv-ops.txt")
FILTS_MRD = 1e-5   # the filter / bias gradients: a different association than the reference's single chain (K slices, trees); bound against float64


def bck_op(B, C, H, W, OC, KH, KW, SY, SX, PY, PX, ogl=None):
    OH, OW = (H + 2 * PY - KH) // SY + 1, (W + 2 * PX - KW) // SX + 1
    oh, ow = ogl or (OH, OW)
    f = f"dims=(out_chan={OC},in_chan={C},y={KH},x={KW})"
    i = f"dims=(img={B},chan={C},y={H},x={W})"
    return parse_op(f"(str_vals=(type=BckConv),nda_vals=(biases=(dims=(out_chan={OC})),biases_grad_loss=(dims=(out_chan={OC})),filts=({f}),filts_grad_loss=({f}),"
                    f"in=({i}),in_grad_loss=({i}),in_pad=(tn=none,dims=(y={PY},x={PX})),kern_sz=(tn=none,dims=(y={KH},x={KW})),"
                    f"out_chans=(tn=uint32_t,v={OC}),out_grad_loss=(dims=(img={B},chan={OC},y={oh},x={ow})),stride=(tn=none,dims=(y={SY},x={SX}))))")


def run_func(rtc, fop, ins):
    """Run one annotated gradient function on `rtc` with host inputs -> its output array."""
    fn = fop.get_func_name()
    rtc.compile([RtcFuncInfo("f", "", [a for a, _ in NATIVE_ARGS[fn]], fop)])
    am, made = {}, []
    try:
        for an, io in NATIVE_ARGS[fn]:
            if io == "REF":
                am[an] = RtcArg.ref(fop.get_dims(an)); continue
            rtc.create_var_with_dims(an, fop.get_dims(an)); made.append(an); am[an] = RtcArg.var(an)
            if io == "IN":
                rtc.copy_nda_to_var(an, np.ascontiguousarray(ins[an], dtype=np.float32))
        rtc.run(RtcFuncCall("f", am))
        rtc.finish_and_sync()
        return rtc.copy_var_to_nda([a for a, io in NATIVE_ARGS[fn] if io == "OUT"][0])
    finally:
        for vn in made:
            rtc.release_var(vn)
        rtc.release_func("f"); rtc.release_per_call_id_data()


def torch_grads(op, x, w, g):
    """float64 gradients: (in_grad_loss, filts_grad_loss, biases_grad_loss)."""
    geo = op.bck_conv_geom()
    st, pad = (geo["SY"], geo["SX"]), (geo["PY"], geo["PX"])
    xd, wd, gd = (torch.from_numpy(np.asarray(a, dtype=np.float64)) for a in (x, w, g))
    gi = torch.nn.grad.conv2d_input(xd.shape, wd, gd, stride=st, padding=pad)
    gw = torch.nn.grad.conv2d_weight(xd, wd.shape, gd, stride=st, padding=pad)
    return gi.numpy(), gw.numpy(), gd.sum(dim=(0, 2, 3)).numpy()


def mrd(x, r):
    return float(np.max(np.abs(np.asarray(x, np.float64) - r)) / max(np.max(np.abs(r)), 1e-30))


def rand_ins(op, seed):
    rng = np.random.default_rng(seed)
    return {an: rng.uniform(-5, 5, op.get_dims(an).sizes).astype(np.float32) for an in ("in", "filts", "out_grad_loss")}


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


# ---- op layer
def test_fixture_lines_parse():
    ops = read_ops(GOLD)
    assert len(ops) >= 90
    for op in ops:
        g = op.bck_conv_geom()
        assert op.get_dims("in_grad_loss") == op.get_dims("in") and op.get_dims("filts_grad_loss") == op.get_dims("filts")
        assert op.get_dims("out_grad_loss").sizes == (g["B"], g["OC"], g["OH"], g["OW"])
    geoms = {(o.bck_conv_geom()["KH"], o.bck_conv_geom()["SY"]) for o in ops}
    assert {(1, 1), (3, 1), (5, 1), (11, 4)} <= geoms


def test_validation_rejects_inconsistent_out_grad_loss():
    bck_op(2, 8, 9, 9, 16, 3, 3, 2, 2, 1, 1)   # consistent: parses
    with pytest.raises(RtErr):
        bck_op(2, 8, 9, 9, 16, 3, 3, 2, 2, 1, 1, ogl=(5, 4))
    with pytest.raises(RtErr):   # gradient dims must equal the matching input's
        parse_op(bck_op(2, 8, 9, 9, 16, 3, 3, 1, 1, 1, 1).to_str().replace("in_grad_loss=(dims=(img=2,chan=8,", "in_grad_loss=(dims=(img=2,chan=9,"))


def test_annotations_three_functions():
    op = bck_op(2, 8, 9, 9, 16, 3, 3, 2, 2, 1, 1)
    fi, fb, ff = add_bck_conv_annotations(op, OpTune())
    assert [f.get_func_name() for f in (fi, fb, ff)] == ["hip_bconv_in", "hip_bconv_biases", "hip_bconv_filts"]
    assert NATIVE_ARGS["hip_bconv_in"] == (("filts", "IN"), ("out_grad_loss", "IN"), ("stride", "REF"), ("in_pad", "REF"), ("in_grad_loss", "OUT"))
    assert NATIVE_ARGS["hip_bconv_filts"] == (("in", "IN"), ("out_grad_loss", "IN"), ("stride", "REF"), ("in_pad", "REF"), ("filts_grad_loss", "OUT"))
    assert NATIVE_ARGS["hip_bconv_biases"] == (("out_grad_loss", "IN"), ("biases_grad_loss", "OUT"))
    ti, _, tf = add_bck_conv_annotations(op, OpTune(hip_tile="64x128x16x2x2"))
    assert ti.str_vals["hip_tile"] == tf.str_vals["hip_tile"] == "64x128x16x2x2"
    with pytest.raises(UnsupErr):
        add_bck_conv_annotations(op, OpTune(hip_dtype="bf16"))
    with pytest.raises(UnsupErr):   # unchanged: BckConv is not a forward hot-path op
        add_codegen_annotations(op, OpTune())


def test_plans_for_every_fixture_shape():
    for op in read_ops(GOLD):
        plan = rtc_mod.explain_plan(op)
        assert "bodahip_bconv_in" in plan and "bodahip_bconv_filts" in plan and "bodahip_bconv_biases" in plan, plan
        for f in add_bck_conv_annotations(op, OpTune()):
            assert rtc_mod.explain_plan(f).startswith("bodahip_bconv_")


def test_plan_forced_tile_and_slices():
    op = bck_op(64, 96, 27, 27, 256, 5, 5, 1, 1, 2, 2)
    _, _, ff = add_bck_conv_annotations(op, OpTune())
    assert int(rtc_mod.explain_plan(ff).split("ksl=")[1].split()[0]) > 1   # long K, few tiles: sliced
    assert "ksl=3" in rtc_mod.explain_plan(ff, tile="64x128x32x2x2x1x3")
    assert "64x128x32" in rtc_mod.explain_plan(ff, tile="64x128x32x2x2x1x3")
    with pytest.raises(UnsupErr):
        rtc_mod.explain_plan(ff, tile="100x128x32x2x2")


# ---- be=cpu against float64
SMALL = [(2, 5, 9, 9, 7, 3, 3, 1, 1, 1, 1), (2, 6, 11, 10, 5, 3, 3, 2, 2, 1, 1), (1, 3, 23, 23, 8, 11, 11, 4, 4, 0, 0), (2, 8, 9, 9, 6, 1, 1, 2, 2, 0, 0),
         (2, 4, 12, 12, 6, 5, 5, 2, 2, 3, 3), (3, 7, 8, 8, 33, 1, 1, 1, 1, 0, 0), (1, 2, 13, 7, 3, 7, 3, 3, 2, 2, 1)]


@pytest.mark.parametrize("shape", SMALL)
def test_cpu_against_float64(cpu, shape):
    op = bck_op(*shape)
    ins = rand_ins(op, sum(shape))
    fi, fb, ff = add_bck_conv_annotations(op, OpTune())
    gi, gw, gb = torch_grads(op, ins["in"], ins["filts"], ins["out_grad_loss"])
    assert mrd(run_func(cpu, fi, ins), gi) < 2e-4
    assert mrd(run_func(cpu, ff, ins), gw) < FILTS_MRD
    assert mrd(run_func(cpu, fb, ins), gb) < FILTS_MRD


def test_cpu_fixture_subset_against_float64(cpu):
    small = [op for op in read_ops(GOLD) if op.flops() < 1.5e8][:8]
    assert len(small) >= 5
    for k, op in enumerate(small):
        ins = rand_ins(op, k)
        fi, fb, ff = add_bck_conv_annotations(op, OpTune())
        gi, gw, gb = torch_grads(op, ins["in"], ins["filts"], ins["out_grad_loss"])
        assert mrd(run_func(cpu, fi, ins), gi) < 2e-4
        assert mrd(run_func(cpu, ff, ins), gw) < FILTS_MRD
        assert mrd(run_func(cpu, fb, ins), gb) < FILTS_MRD


def test_cpu_data_gradient_follows_the_x_outer_order(cpu):
    """2x2 kernel, stride 1, one channel each way, 1x1 input: in_grad = sum over (ox, oy) of ogl * the flipped taps.  The reference chains out_x OUTER, out_y
    inner; with these values the y-outer order rounds differently, so only the reference order gives the bits."""
    op = bck_op(1, 1, 1, 1, 1, 2, 2, 1, 1, 1, 1)            # out is 2x2; in pel (0,0) meets all four taps
    w = np.array([[[[1.0, 1.0], [1.0, 1.0]]]], np.float32)   # filts[fy][fx]
    ogl = np.array([[[[2.0 ** 24, 1.0], [-(2.0 ** 24), 0.0]]]], np.float32)   # ogl[oy][ox]
    f32 = np.float32
    x_outer = f32(f32(f32(f32(0) + ogl[0, 0, 0, 0]) + ogl[0, 0, 1, 0]) + ogl[0, 0, 0, 1]) + ogl[0, 0, 1, 1]   # (ox=0: oy 0,1) (ox=1: oy 0,1)
    y_outer = f32(f32(f32(f32(0) + ogl[0, 0, 0, 0]) + ogl[0, 0, 0, 1]) + ogl[0, 0, 1, 0]) + ogl[0, 0, 1, 1]
    assert x_outer != y_outer
    fi, _, _ = add_bck_conv_annotations(op, OpTune())
    got = run_func(cpu, fi, {"filts": w, "out_grad_loss": ogl})
    assert got.reshape(-1)[0] == x_outer


def test_cpu_rejects_dims_that_disagree(cpu):
    op = bck_op(2, 4, 8, 8, 6, 3, 3, 1, 1, 1, 1)
    fi, _, _ = add_bck_conv_annotations(op, OpTune())
    bad = bck_op(2, 4, 8, 8, 6, 3, 3, 1, 1, 0, 0)   # 6x6 out_grad_loss planes: run with the first op's in_pad
    cpu.compile([RtcFuncInfo("g", "", [a for a, _ in NATIVE_ARGS["hip_bconv_in"]], fi)])
    try:
        for an in ("filts", "out_grad_loss", "in_grad_loss"):
            cpu.create_var_with_dims(an, bad.get_dims(an))
        am = {an: RtcArg.var(an) for an in ("filts", "out_grad_loss", "in_grad_loss")}
        am["stride"] = RtcArg.ref(op.get_dims("stride")); am["in_pad"] = RtcArg.ref(op.get_dims("in_pad"))
        with pytest.raises(RtErr):
            cpu.run(RtcFuncCall("g", am))
    finally:
        for an in ("filts", "out_grad_loss", "in_grad_loss"):
            cpu.release_var(an)
        cpu.release_func("g"); cpu.release_per_call_id_data()
