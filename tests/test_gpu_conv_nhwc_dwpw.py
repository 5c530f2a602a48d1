"""Tests (-m gpu) of the fused depthwise + pointwise pair on channels-last bf16 tensors (func hip_conv_nhwc_dw_pw, kernels/conv_nhwc_dwpw_bf16.hip): vars filled
directly with seeded bf16 bit patterns, a NaN-filled out, one call, fetch.  The reference is numpy: t = the float32 chain twin of tests/test_gpu_conv_nhwc_dw.py rounded
to bf16 -- the definition of the intermediate, so exact -- and want = t @ F2^T + b2 in float64.  The bound is the derived one of tests/test_gpu_nhwc.py with K = C,
element by element: |got - want| <= 2 (C + 1) 2^-24 (|t| @ |F2|^T + |b2|), plus 2^-8 |want| for a bf16 out.  No element may be NaN: every element is written."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import resnet_ref as rr
from test_gpu_conv_nhwc_dw import dw_op, twin
from boda_amd import nhwc
from boda_amd.cnn_op import NATIVE_ARGS, OpTune, add_codegen_annotations
from boda_amd.conv_pipe import ConvPipeFwd, mobilenet_v1
from boda_amd.op import parse_op
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc
from oracle import boda_oracle as bo

NHWC = dict(hip_dtype="bf16", hip_layout="nhwc")
bits = lambda a: (bo.to_bf16(a).view(np.uint32) >> 16).astype(np.uint16)          # float32 -> bf16 bit patterns
widen = lambda u: (np.asarray(u, np.uint16).astype(np.uint32) << 16).view(np.float32)


@pytest.fixture(scope="module")
def hip():
    rtc = make_rtc("(be=hip)", 0)
    rtc.init()
    yield rtc
    rtc.finish_and_sync()
    rtc.close()


def check(got, x, f, b, f2, b2, stride, pad, relus, out_f32, what):
    """got, x img:chan:y:x; f [C][1][KH][KW], f2 [OC][C] (bf16 values); the bound of the module docstring."""
    t = bo.to_bf16(twin(x, f, b, stride, pad, relus[0])).astype(np.float64)
    want = np.einsum("bchw,oc->bohw", t, f2.astype(np.float64)) + b2[None, :, None, None]
    S = np.einsum("bchw,oc->bohw", np.abs(t), np.abs(f2).astype(np.float64)) + np.abs(b2)[None, :, None, None]
    if relus[1]:
        want = np.maximum(want, 0.0)
    lim = 2.0 * (x.shape[1] + 1) * 2.0 ** -24 * S + (0.0 if out_f32 else 2.0 ** -8 * np.abs(want))
    assert got.shape == want.shape and not np.isnan(got).any(), what
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= lim).all(), (what, float((err / np.maximum(lim, 1e-300)).max()))


CASES = [(2, 8, 5, 7, 3, 1, 1, 8),                    # one chunk, C < 16, OC < 32, ragged second pel tile
         (1, 24, 9, 10, 3, 2, 1, 40),                 # stride 2, K tail C % 16 == 8, ragged out_chan block
         (1, 16, 3, 3, 3, 1, 1, 16),                  # plane no larger than the kernel
         (3, 72, 17, 6, 3, 1, 1, 136),                # several images and strips, more out_chan blocks than waves
         (1, 40, 12, 33, 5, 1, 2, 24),                # 5 x 5, more than one column segment
         (1, 16, 8, 9, (5, 3), (1, 2), (2, 1), 8),    # rectangular kernel, mixed strides
         (1, 264, 6, 6, 3, 1, 1, 32)]                 # several chunk blocks with a ragged last one, 17 K steps
# forced tiles dwpw:TYxTXxCB (the planner halves TY to 1 on planes this small), one per field: a ragged strip of two pel tiles, a ragged segment, a ragged chunk block
TILED = [((1, 8, 11, 5, 3, 1, 1, 16), "dwpw:8x5x1"), ((1, 8, 5, 11, 3, 2, 1, 16), "dwpw:3x4x1"), ((1, 40, 5, 5, 3, 1, 1, 16), "dwpw:3x5x2")]


@pytest.mark.parametrize("out_f32", [True, False], ids=["f32", "bf16"])
@pytest.mark.parametrize("relu", [1, 0], ids=["relu", "lin"])
@pytest.mark.parametrize("case,tile", [(c, "") for c in CASES] + TILED, ids=lambda v: v if isinstance(v, str) else "x".join(str(e) for e in v).replace(" ", ""))
def test_dw_pw_pair_within_the_derived_bound(hip, case, tile, relu, out_f32):
    OC = case[7]
    dop = dw_op(*case[:7]); g = dop.conv_geom(); B, C, OH, OW = g["B"], g["C"], g["OH"], g["OW"]
    pop = parse_op(f"(str_vals=(type=Convolution),nda_vals=(biases=(dims=(out_chan={OC})),filts=(dims=(out_chan={OC},in_chan={C},y=1,x=1)),in=(dims=(img={B},chan={C},y={OH},x={OW})),"
                   f"in_pad=(tn=none,dims=(y=0,x=0)),kern_sz=(tn=none,dims=(y=1,x=1)),out=(dims=(img={B},chan={OC},y={OH},x={OW})),out_chans=(tn=uint32_t,v={OC}),stride=(tn=none,dims=(y=1,x=1))))")
    da = add_codegen_annotations(dop, OpTune(**NHWC)); pa = add_codegen_annotations(pop, OpTune(hip_out="f32" if out_f32 else "", **NHWC))
    da.nda_vals["conv_has_relu"].v = (relu,); pa.nda_vals["conv_has_relu"].v = (relu,)
    assert nhwc.dw_pw_applies(da, pa)
    fop = nhwc.annotate_dw_pw(da, pa, tile)
    rng = np.random.default_rng(7)
    data = {"in": bits(rng.uniform(-1, 1, fop.get_dims("in").sizes)), "filts": bits(rng.uniform(-1, 1, fop.get_dims("filts").sizes)), "biases": rng.uniform(-1, 1, C).astype(np.float32),
            "filts2": bits(rng.uniform(-1, 1, fop.get_dims("filts2").sizes) * C ** -0.5), "biases2": rng.uniform(-1, 1, OC).astype(np.float32),
            "out": np.full(fop.get_dims("out").sizes, np.nan, np.float32) if out_f32 else np.full(fop.get_dims("out").sizes, 0x7fc0, np.uint16)}
    hip.compile([RtcFuncInfo("dwpw", "", [a for a, _ in NATIVE_ARGS[nhwc.DW_PW_FUNC]], fop)])
    try:
        for an, arr in data.items():
            hip.create_var_with_dims("dwpw_" + an, fop.get_dims(an)); hip.copy_nda_to_var("dwpw_" + an, arr)
        am = dict({an: RtcArg.var("dwpw_" + an) for an in data}, stride=RtcArg.ref(fop.get_dims("stride")), in_pad=RtcArg.ref(fop.get_dims("in_pad")))
        hip.run(RtcFuncCall("dwpw", am)); hip.finish_and_sync()
        launch = hip.last_launch()
        got = np.asarray(hip.copy_var_to_nda("dwpw_out"))
    finally:
        for an in data:
            hip.release_var("dwpw_" + an)
        hip.release_func("dwpw"); hip.release_per_call_id_data()
    assert launch["kernel"] == "bodahip_conv_nhwc_dwpw_bf16", launch
    if tile:
        assert launch["cfg"].startswith(tile[5:] + "_"), launch
    got = (got if out_f32 else widen(got)).transpose(0, 3, 1, 2)
    x = widen(data["in"]).transpose(0, 3, 1, 2); f = np.ascontiguousarray(widen(data["filts"]).transpose(2, 0, 1))[:, None]
    check(got, x, f, data["biases"], widen(data["filts2"]).reshape(OC, C), data["biases2"], (g["SY"], g["SX"]), (g["PY"], g["PX"]), (relu, relu), out_f32, (case, launch))


def test_mobilenet_fused_pairs_and_graph_replay(hip):
    cp = mobilenet_v1(2, in_hw=32, width=0.25)
    P = rr.he_params(cp, 5)
    xs = [np.random.default_rng(20 + i).uniform(-1, 1, cp.nodes["data"].sizes).astype(np.float32) for i in range(2)]
    f = ConvPipeFwd(hip, OpTune(**NHWC), fuse_dw_pw="all")
    f.init(cp, P)
    try:
        funcs = [c.func for c in f.fwd_calls]
        assert funcs.count("hip_conv_nhwc_dw_pw") == 13 and "hip_conv_nhwc_dw" not in funcs and len(f.fused_dw_pw) == 13
        ops = {o.tag: o for o in cp.ops}
        fwd = {"data": xs[0]}
        f.run_fwd(["data"], fwd, [ops[d].bot for d, _ in f.fused_dw_pw] + [ops[p].top for _, p in f.fused_dw_pw] + ["fc"])
        for d, p in f.fused_dw_pw:     # the call on the GPU's own input node, with the folded params as the device holds them
            F = np.ascontiguousarray(widen(hip.copy_var_to_nda(d + "_filts")).transpose(2, 0, 1))[:, None]
            F2 = widen(hip.copy_var_to_nda(p + "_filts")); F2 = F2.reshape(F2.shape[0], -1)
            b, b2 = (np.asarray(hip.copy_var_to_nda(t + "_biases"), np.float32).reshape(-1) for t in (d, p))
            check(fwd[ops[p].top], fwd[ops[d].bot], F, b, F2, b2, tuple(ops[d].stride), tuple(ops[d].in_pad), (1, 1), False, p)
        assert np.isfinite(fwd["fc"]).all() and np.abs(fwd["fc"]).max() > 0
        assert f.capture_graph() == len(f.fwd_calls)
        hip.copy_nda_to_var(f.in_var, xs[1]); hip.finish_and_sync()
        f.run_graph()
        replay, eager = f._fetch("fc"), {"data": xs[1]}
        f.run_fwd(["data"], eager, ["fc"])
        assert rr.bits_eq(replay, eager["fc"]) and not rr.bits_eq(eager["fc"], fwd["fc"])
    finally:
        f.release()
