"""Tests (-m gpu) of the depthwise channels-last bf16 convolution (func hip_conv_nhwc_dw, kernels/conv_nhwc_dw_bf16.hip), through OpsBackend / profile_rcg_call and the
`<arg>_ref` + xpose protocol, and of MobileNet-v1 on the channels-last forward pipe.  The kernel is held to BITS: per output, in fp32, acc = +0; for ky, then kx
ascending acc = fmaf(in, filt, acc) (a padded tap a product with +0); + bias; ReLU; one rounding to bf16 or none.  A product of two bf16 values is exact in fp32, so
`twin` below is that chain in numpy float32 multiplies and adds.  Independently both outputs are held to the derived bound of tests/test_gpu_nhwc.py against float64:
2 (K + 1) 2^-24 S, plus 2^-8 |want| for bf16, K = KH * KW, S = sum |in| |filt| + |bias|."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import resnet_ref as rr
from boda_amd.cnn_op import OpTune, add_codegen_annotations
from boda_amd.conv_pipe import ConvPipeFwd, mobilenet_v1
from boda_amd.op import parse_op
from boda_amd.ops_prof import OpsBackend, profile_rcg_call
from boda_amd.rtc import make_rtc
from oracle import boda_oracle as bo


@pytest.fixture(scope="module")
def hip():
    rtc = make_rtc("(be=hip)", 0)
    rtc.init()
    yield rtc
    rtc.finish_and_sync()
    rtc.close()


def dw_op(B, C, H, W, K, S, P):
    (KH, KW), (SY, SX), (PY, PX) = (v if isinstance(v, tuple) else (v, v) for v in (K, S, P))
    OH, OW = (H + 2 * PY - KH) // SY + 1, (W + 2 * PX - KW) // SX + 1
    return parse_op(f"(str_vals=(type=Convolution),nda_vals=(biases=(dims=(out_chan={C})),filts=(dims=(out_chan={C},in_chan=1,y={KH},x={KW})),group=(tn=uint32_t,v={C}),"
                    f"in=(dims=(img={B},chan={C},y={H},x={W})),in_pad=(tn=none,dims=(y={PY},x={PX})),kern_sz=(tn=none,dims=(y={KH},x={KW})),"
                    f"out=(dims=(img={B},chan={C},y={OH},x={OW})),out_chans=(tn=uint32_t,v={C}),stride=(tn=none,dims=(y={SY},x={SX}))))")


def twin(x, f, b, stride, pad, relu, dt=np.float32):
    """The chain on x[B][C][H][W], f[C][1][KH][KW], b[C] (values that are bf16 already), evaluated in `dt`."""
    (SY, SX), (PY, PX) = stride, pad
    B, C, H, W = x.shape; KH, KW = f.shape[2:]
    OH, OW = (H + 2 * PY - KH) // SY + 1, (W + 2 * PX - KW) // SX + 1
    xp = np.zeros((B, C, H + 2 * PY + SY, W + 2 * PX + SX), dt); xp[:, :, PY:PY + H, PX:PX + W] = x
    acc = np.zeros((B, C, OH, OW), dt)
    for ky in range(KH):
        for kx in range(KW):
            acc = (xp[:, :, ky:ky + OH * SY:SY, kx:kx + OW * SX:SX] * f[None, :, 0, ky, kx, None, None].astype(dt) + acc).astype(dt)
    acc = (acc + b[None, :, None, None].astype(dt)).astype(dt)
    return np.where(acc > 0, acc, dt(0)) if relu else acc


def check(got, x, f, b, stride, pad, relu, out_f32, what):
    want = twin(x, f, b, stride, pad, relu)
    assert not np.isnan(got).any(), what                                   # the output was NaN-filled: every element is written
    assert rr.bits_eq(got, want if out_f32 else bo.to_bf16(want)), what
    w64 = twin(x, f, b, stride, pad, relu, np.float64); S = twin(np.abs(x), np.abs(f), np.abs(b), stride, pad, False, np.float64)
    lim = 2.0 * (f.shape[2] * f.shape[3] + 1) * 2.0 ** -24 * S + (0.0 if out_f32 else 2.0 ** -8 * np.abs(w64))
    assert (np.abs(got.astype(np.float64) - w64) <= lim).all(), what


CASES = [(2, 8, 5, 7, 3, 1, 1),                  # one chunk, plane below any tile
         (2, 16, 3, 3, 3, 1, 1),                 # plane no larger than the kernel
         (1, 24, 9, 10, 3, 2, 1),                # stride 2, even width (the last right-pad column is never read); chunk count no power of two
         (1, 8, 7, 7, 3, 2, 0),                  # stride 2 unpadded
         (1, 40, 12, 33, 5, 1, 2),               # 5 x 5, more than one column segment
         (3, 72, 17, 6, 3, 1, 1),                # more than one row strip, several images, more chunks than one wave row
         (1, 16, 8, 9, (5, 3), (1, 2), (2, 1))]  # rectangular kernel, mixed strides
# forced tiles dw:TYxTXxCB (these shapes are below two workgroups per CU: the planner's TY is 1), one per field: ragged last strip with steady periods, ragged segment, ragged chunk block
TILED = [((1, 8, 23, 5, 3, 1, 1), "dw:9x5x1"), ((1, 8, 5, 11, 3, 2, 1), "dw:3x4x1"), ((1, 40, 5, 5, 3, 1, 1), "dw:3x5x2")]


@pytest.mark.parametrize("out_f32", [True, False], ids=["f32", "bf16"])
@pytest.mark.parametrize("relu", [1, 0], ids=["relu", "lin"])
@pytest.mark.parametrize("case,tile", [(c, "") for c in CASES] + TILED, ids=lambda v: v if isinstance(v, str) else "x".join(str(e) for e in v).replace(" ", ""))
def test_dw_conv_is_the_chain_by_bits(hip, case, tile, relu, out_f32):
    op = dw_op(*case)
    anno = add_codegen_annotations(op, OpTune(hip_dtype="bf16", hip_layout="nhwc", hip_out="f32" if out_f32 else "", hip_tile=tile))
    assert anno.get_func_name() == "hip_conv_nhwc_dw"
    anno.nda_vals["conv_has_relu"].v = (relu,)
    nan = np.full(anno.get_dims("out").sizes, np.nan, np.float32) if out_f32 else np.full(anno.get_dims("out").sizes, 0x7fc0, np.uint16)
    outs, prc = profile_rcg_call(OpsBackend(hip), anno, 5, 0.0, 1, include_ins=True, tile=tile, ins={"out": nan})
    assert prc.launch["kernel"] == "bodahip_conv_nhwc_dw_bf16", prc.launch
    if tile:
        assert prc.launch["cfg"].startswith(tile[3:] + "_"), prc.launch
    g = op.conv_geom()
    check(outs["out"], bo.to_bf16(outs["in"]), bo.to_bf16(outs["filts"]), outs["biases"], (g["SY"], g["SX"]), (g["PY"], g["PX"]), relu, out_f32, (case, prc.launch))


def test_mobilenet_dw_calls_by_bits_and_graph_replay(hip):
    cp = mobilenet_v1(2, in_hw=32, width=0.25)
    P = rr.he_params(cp, 5)
    xs = [np.random.default_rng(20 + i).uniform(-1, 1, cp.nodes["data"].sizes).astype(np.float32) for i in range(2)]
    f = ConvPipeFwd(hip, OpTune(hip_dtype="bf16", hip_layout="nhwc"))
    f.init(cp, P)
    try:
        dws = [o for o in cp.ops if o.type == "Convolution" and o.group > 1]
        assert len(dws) == 13 and {c.tag: c.func for c in f.fwd_calls}.items() >= {o.tag: "hip_conv_nhwc_dw" for o in dws}.items()
        fwd = {"data": xs[0]}
        f.run_fwd(["data"], fwd, [n for n in cp.nodes if n != "data"])
        for o in dws:     # the call on the GPU's own input node, with the folded params as the device holds them
            F16 = np.asarray(hip.copy_var_to_nda(o.tag + "_filts"), np.uint16)                                  # y:x:chan bf16 bit patterns
            F = np.ascontiguousarray((F16.astype(np.uint32) << 16).view(np.float32).transpose(2, 0, 1))[:, None]
            Bv = np.asarray(hip.copy_var_to_nda(o.tag + "_biases"), np.float32).reshape(-1)
            check(fwd[o.top], fwd[o.bot], F, Bv, tuple(o.stride), tuple(o.in_pad), True, False, o.tag)
        assert np.isfinite(fwd["fc"]).all() and np.abs(fwd["fc"]).max() > 0
        assert f.capture_graph() == len(f.fwd_calls)
        hip.copy_nda_to_var(f.in_var, xs[1]); hip.finish_and_sync()
        f.run_graph()
        replay, eager = f._fetch("fc"), {"data": xs[1]}
        f.run_fwd(["data"], eager, ["fc"])
        assert rr.bits_eq(replay, eager["fc"]) and not rr.bits_eq(eager["fc"], fwd["fc"])
    finally:
        f.release()
