"""Test (-m gpu) of the filter and bias gradient from channels-last bf16 tensors (func hip_bconv_fb_nhwc, kernels/bconv_fb_nhwc_bf16.hip): vars filled with seeded bf16
bit patterns, NaN-filled outputs, one call under the planner's choice and one under a forced tile with KSL = 3.  The reference is the definition in float64, plain
numpy loops over taps.  Bound per element of both outputs (DESIGN.md section 3.16, fp32 additions in any order): |got - S| <= 2 (K + KSL + 3) 2^-24 A, A the same sum
over absolute values, K = B * OH * OW, KSL as the launch reports it.  Largest observed fraction of the bound on the MI355X: 0.070."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from boda_amd import nhwc
from boda_amd.cnn_op import NATIVE_ARGS
from boda_amd.op import parse_op
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc
from oracle import boda_oracle as bo

bits = lambda a: (bo.to_bf16(a).view(np.uint32) >> 16).astype(np.uint16)          # float32 -> bf16 bit patterns
widen = lambda u: (np.asarray(u, np.uint16).astype(np.uint32) << 16).view(np.float32)
TILE = "fbn:32x64x16x3x8"    # the forced tile: KSL = 3, unequal sides, stages of one MFMA step: 16 pels, or blocks of 2 x 8 (the planner's stages are 64 pels)


def bck_op(B, C, OC, H, W, kern, stride, pad):
    """A bare BckConv op in the reference layouts; kern, stride, pad: an int or (y, x)."""
    (KH, KW), (SY, SX), (PY, PX) = (v if isinstance(v, tuple) else (v, v) for v in (kern, stride, pad))
    OH, OW = (H + 2 * PY - KH) // SY + 1, (W + 2 * PX - KW) // SX + 1
    return parse_op(f"(str_vals=(type=BckConv),nda_vals=(biases=(dims=(out_chan={OC})),biases_grad_loss=(dims=(out_chan={OC})),filts=(dims=(out_chan={OC},in_chan={C},y={KH},x={KW})),"
                    f"filts_grad_loss=(dims=(out_chan={OC},in_chan={C},y={KH},x={KW})),in=(dims=(img={B},chan={C},y={H},x={W})),in_grad_loss=(dims=(img={B},chan={C},y={H},x={W})),"
                    f"in_pad=(tn=none,dims=(y={PY},x={PX})),kern_sz=(tn=none,dims=(y={KH},x={KW})),out_chans=(tn=uint32_t,v={OC}),out_grad_loss=(dims=(img={B},chan={OC},y={OH},x={OW})),"
                    f"stride=(tn=none,dims=(y={SY},x={SX}))))")


@pytest.fixture(scope="module")
def hip():
    rtc = make_rtc("(be=hip)", 0)
    rtc.init()
    yield rtc
    rtc.finish_and_sync()
    rtc.close()


def reference(x, g, fop):
    """-> (filter sums, their absolute twins, bias sums, their absolute twins) in float64.  x img:y:x:chan, g img:oy:ox:oc."""
    st, pad, f = fop.get_dims("stride"), fop.get_dims("in_pad"), fop.get_dims("filts_grad_loss")
    (SY, SX), (PY, PX), (KH, KW) = (st.dsz("y"), st.dsz("x")), (pad.dsz("y"), pad.dsz("x")), (f.dsz("y"), f.dsz("x"))
    B, H, W, C = x.shape; _, OH, OW, OC = g.shape
    xp = np.zeros((B, H + 2 * PY + SY, W + 2 * PX + SX, C)); xp[:, PY:PY + H, PX:PX + W] = x
    S = np.zeros((OC, KH, KW, C)); A = np.zeros_like(S)
    for ky in range(KH):
        for kx in range(KW):
            win = xp[:, ky:ky + OH * SY:SY, kx:kx + OW * SX:SX]
            S[:, ky, kx] = np.einsum("byxo,byxc->oc", g, win); A[:, ky, kx] = np.einsum("byxo,byxc->oc", np.abs(g), np.abs(win))
    return S, A, g.sum((0, 1, 2)), np.abs(g).sum((0, 1, 2))


CASES = [(2, 8, 8, 5, 5, 1, 1, 0),               # K = 50: a tail shorter than one MFMA step, a single tile
         (1, 16, 24, 7, 7, 1, 2, 0),             # skipped input pels
         (1, 136, 264, 4, 4, 1, 1, 0),           # several tiles each way, ragged last tile, K = 16
         (4, 16, 1000, 1, 1, 1, 1, 0),           # fc shape, K = img
         (2, 40, 72, 6, 9, 3, 1, 1),             # padding on every side, non-square map, ragged channels
         (3, 8, 16, 9, 9, 3, 2, 1),              # stride in the patch
         (1, 8, 8, 3, 3, 5, 1, 2),               # every tap but the centre meets padding
         (2, 8, 64, 17, 17, 7, 2, 3),            # the stem: taps split over groups
         (2, 8, 16, 6, 10, (1, 3), (2, 1), (0, 1))]   # per-axis kernel, stride and pad


@pytest.mark.parametrize("tile", ["", TILE], ids=["planned", "forced"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(e) for e in c).replace(" ", ""))
def test_filter_and_bias_gradient_within_the_bound(hip, case, tile):
    fop = nhwc.annotate_bconv_fb(bck_op(*case), tile)
    rng = np.random.default_rng(11)
    data = {an: bits(rng.uniform(-1, 1, fop.get_dims(an).sizes)) for an in ("in", "out_grad_loss")}
    outs = ("filts_grad_loss", "biases_grad_loss")
    K = int(np.prod(fop.get_dims("out_grad_loss").sizes[:3]))
    hip.compile([RtcFuncInfo("fbn", "", [a for a, _ in NATIVE_ARGS[nhwc.BCONV_FB_FUNC]], fop)])
    try:
        for an in data:
            hip.create_var_with_dims("fbn_" + an, fop.get_dims(an)); hip.copy_nda_to_var("fbn_" + an, data[an])
        for an in outs:
            hip.create_var_with_dims("fbn_" + an, fop.get_dims(an)); hip.copy_nda_to_var("fbn_" + an, np.full(fop.get_dims(an).sizes, np.nan, np.float32))
        am = dict({an: RtcArg.var("fbn_" + an) for an in tuple(data) + outs}, stride=RtcArg.ref(fop.get_dims("stride")), in_pad=RtcArg.ref(fop.get_dims("in_pad")))
        runs = []
        for _ in range(2):
            hip.run(RtcFuncCall("fbn", am)); hip.finish_and_sync()
            runs.append([np.asarray(hip.copy_var_to_nda("fbn_" + an)).copy() for an in outs])
        launch = hip.last_launch()
    finally:
        for an in tuple(data) + outs:
            hip.release_var("fbn_" + an)
        hip.release_func("fbn"); hip.release_per_call_id_data()
    assert launch["kernel"] == "bodahip_bconv_fb_nhwc_bf16", launch
    m = re.search(r"_s(\d+)", launch["cfg"]); ksl = int(m.group(1)) if m else 1
    if tile:   # a forced KSL above the number of stages (of BK = 16 pels) is clamped to the slices that are not empty
        B, OH, OW = fop.get_dims("out_grad_loss").sizes[:3]
        stages = -(-K // 16) if case[5] == 1 else B * -(-OH // 2) * -(-OW // 8)
        assert launch["cfg"].startswith("32x64x16_") and ksl == -(-stages // -(-stages // min(3, stages))), (launch, stages)
    S, A, Sb, Ab = reference(widen(data["in"]).astype(np.float64), widen(data["out_grad_loss"]).astype(np.float64), fop)
    worst = 0.0
    for got, again, want, mag in zip(runs[0], runs[1], (S, Sb), (A, Ab)):
        assert got.shape == want.shape and not np.isnan(got).any(), (case, launch)
        assert got.tobytes() == again.tobytes(), (case, launch)            # a second call leaves the same bits
        lim = 2.0 * (K + ksl + 3) * 2.0 ** -24 * mag
        err = np.abs(got.astype(np.float64) - want)
        worst = max(worst, float((err / np.maximum(lim, 1e-300)).max()))
        assert (err <= lim).all(), (case, launch, worst)
    print(f"hip_bconv_fb_nhwc {case} {launch['cfg']} grid={launch['grid']}: largest fraction of the bound {worst:.4f}")
