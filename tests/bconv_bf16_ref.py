"""What tests/test_bconv_bf16_cpu.py and tests/test_gpu_bconv_bf16.py share: the shapes, the runner (NaN-poisoned outputs, a guard var behind every var), the
float64 references and THE BOUND of hip_operands=bf16.

With r = oracle.boda_oracle.to_bf16 (fp32 -> bf16 round-to-nearest-even -> fp32), for each element of filts_grad_loss and in_grad_loss

    |got - S| <= 2 * (K + KSL + 3) * u * A,      u = 2^-24,

S the float64 sum over the r-rounded operands, A the same sum over their absolute values (test_bck_conv_cpu.torch_grads on r(.) and on |r(.)|), K the number of terms
(img * OH * OW for the filter gradient, OC * KH * KW for the data gradient) and KSL the K slices of the launch (1 for the data gradient and on be=cpu).  Products of
bf16 values are exact in fp32, so this is the any-order bound for the fp32 additions, (K - 1) + (KSL - 1) of them at the most, with a factor 2 of margin.  It is not
tuned.  Also: NRMS against the UNROUNDED float64 gradients < 1e-2, the forward bf16 kernels' stated bound."""
import numpy as np

from boda_amd.cnn_op import OpTune, add_bck_conv_annotations, bconv_filts_biases_func_op, bf16_operands, fuse_zero_if_in_non_pos, pipe_func_args
from boda_amd.op import Dims
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo

from oracle.boda_oracle import to_bf16

from test_bck_conv_cpu import bck_op, torch_grads

F = np.float32
U = 2.0 ** -24
NRMS_BOUND = 1e-2
GUARD = np.full(4, 0x7FC0BEEF, np.uint32)   # a NaN with a payload: what the guard vars hold

# the data-gradient shapes of the GPU file: (img, in_chan, H, W, out_chan, k, stride, pad)
IN_SHAPES = {
    "k1_tail24": (2, 40, 9, 9, 24, 1, 1, 0),        # K = 24: a tail inside one 16-deep step, ragged channels
    "k1_stride2": (3, 16, 9, 9, 70, 1, 2, 0),       # unreached positions are +0, odd planes
    "k3_borders": (2, 19, 7, 7, 33, 3, 1, 1),       # K = 297
    "k3_stride2": (2, 8, 10, 10, 20, 3, 2, 1),      # phases with different tap counts
    "k7_stem": (2, 3, 23, 23, 16, 7, 2, 3),
    "k11_s4": (1, 3, 35, 35, 8, 11, 4, 0),
    "k5_pad2": (1, 12, 6, 6, 9, 5, 1, 2),
    "k3_tiles": (5, 70, 13, 13, 40, 3, 1, 1),       # several tiles both ways (also under forced tiles)
}
IN_FORCED = {"k3_tiles": ["32x32x32x1x1", "64x64x64x2x2"]}
FC_SHAPE = (4, 6, 3, 3, 50, 3, 1, 0)                 # fc-shaped: K = img = 4, N = C * KH * KW
FB_FORCED = {"64x64x32x2x2x1x1": None,                      # forced tile -> the bconv_fb_ref.SHAPES it runs on (None: all).  One slice: the outputs are written directly
             "64x64x32x2x2x1x7": ("k1_ohw49_tail",),        # K = 147: five K steps over seven slices, empty slices
             "32x128x64x1x4x1x3": None,                     # K < BK on the short shapes
             "64x64x16x2x2x2x98": ("k1_long_k",)}
FC_TILE, REUSE_TILE = "32x128x16x1x4x1x2", "64x64x32x2x2x1x5"


def in_op(name):
    B, C, H, W, OC, k, s, p = IN_SHAPES[name]
    return bck_op(B, C, H, W, OC, k, k, s, s, p, p)


def shape8_op(t):
    B, C, H, W, OC, k, s, p = t
    return bck_op(B, C, H, W, OC, k, k, s, s, p, p)


def in_func(op, tile="", zinp=False, bf16=True):
    f = add_bck_conv_annotations(op, OpTune(hip_tile=tile))[0]
    if zinp:
        f = fuse_zero_if_in_non_pos(f)
    return bf16_operands(f) if bf16 else f


def fb_func(op, tile="", bf16=True):
    f = bconv_filts_biases_func_op(op, OpTune(hip_tile=tile))
    return bf16_operands(f) if bf16 else f


def recorded_ops():
    """Eight lines of the recorded BckConv shapes (tests/golden/ops/bck-conv-ops.txt), the smallest of each class by flops: four 1x1, two 3x3, one 5x5, one strided."""
    from boda_amd.op import read_ops
    from test_bck_conv_cpu import GOLD
    ops = sorted(read_ops(GOLD), key=lambda o: (o.flops(), o.to_str()))
    cls = lambda o: (o.bck_conv_geom()["KH"], o.bck_conv_geom()["SY"])
    pick = lambda want, n: [o for o in ops if want(*cls(o))][:n]
    out = pick(lambda k, s: k == 1 and s == 1, 4) + pick(lambda k, s: k == 3 and s == 1, 2) + pick(lambda k, s: k == 5 and s == 1, 1) + pick(lambda k, s: s > 1, 1)
    assert len(out) == 8
    return out


def single_call_fops():
    """Every flagged function op tests/test_gpu_bconv_bf16.py runs as a single call (the pre-specialisation fixture tests/golden/ops/bconv-bf16-ops.txt lists them)."""
    import bconv_fb_ref as fb
    out = []
    for name in sorted(IN_SHAPES):
        for tile in [""] + IN_FORCED.get(name, []):
            out += [in_func(in_op(name), tile), in_func(in_op(name), tile, zinp=True)]
    for name in sorted(fb.SHAPES):
        out += [fb_func(fb.shape_op(name))] + [fb_func(fb.shape_op(name), t) for t, only in FB_FORCED.items() if only is None or name in only]
    out += [fb_func(shape8_op(FC_SHAPE)), fb_func(shape8_op(FC_SHAPE), FC_TILE), fb_func(fb.shape_op("k1_many_tiles"), REUSE_TILE)]
    for op in recorded_ops():
        out += [in_func(op), fb_func(op)]
    return out


def unchanged_grad_nodes(loss_tops):
    """The gradient nodes grad_operands="bf16" leaves with the default driver's bits: a loss top's own gradient (the softmax gradient) and the bias gradient of the
    convolution that writes the top, which is summed from that unrounded gradient.  Every other gradient node lies behind a rounded product."""
    return {t + sfx for t in loss_tops for sfx in ("_grad_loss", "_biases_grad_loss")}


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def rand_ins(op, seed):
    """Values with full fp32 mantissas (so that rounding to bf16 changes every one), both signs, a few exact zeros in `in` for the zero_if_in_non_pos select."""
    rng = np.random.default_rng([seed, 16])
    ins = {an: rng.uniform(-2, 2, op.get_dims(an).sizes).astype(F) for an in ("in", "filts", "out_grad_loss")}
    ins["in"].reshape(-1)[::7] = 0.0
    return ins


def run_fop(rtc, fop, ins, compile_opts=None, launch=False):
    """One annotated gradient function on `rtc` with host inputs.  Every OUT var starts as NaN; a 4-float guard var is created right behind every var and must come
    back unchanged; the IN vars must come back unchanged.  -> {out arg: array} (+ "launch": rtc.last_launch() if asked).  `ins` may be a list of input sets: they
    run one after the other through the SAME vars (so the same per-call workspace), the outputs poisoned again before each -> a list."""
    seq = ins if isinstance(ins, (list, tuple)) else [ins]
    args = pipe_func_args(fop)
    rtc.compile([RtcFuncInfo("f16", "", [a for a, _ in args], fop)], compile_opts)
    am, made, outs = {}, [], []
    try:
        for an, io in args:
            if io == "REF":
                am[an] = RtcArg.ref(fop.get_dims(an)); continue
            rtc.create_var_with_dims(an, fop.get_dims(an)); made.append(an); am[an] = RtcArg.var(an)
            rtc.create_var_with_dims(an + "_guard", Dims.make("float", v=4)); made.append(an + "_guard")
            rtc.copy_nda_to_var(an + "_guard", GUARD.view(F))
        for cur in seq:
            for an, io in args:
                if io != "REF":
                    rtc.copy_nda_to_var(an, np.ascontiguousarray(cur[an], F) if io == "IN" else np.full(fop.get_dims(an).sizes, np.nan, F))
            rtc.run(RtcFuncCall("f16", am))
            out = {"launch": rtc.last_launch()} if launch else {}
            rtc.finish_and_sync()
            for an, io in args:
                if io == "REF":
                    continue
                assert np.array_equal(bits(rtc.copy_var_to_nda(an + "_guard")), GUARD), (an, "a guard var was written")
                if io == "IN":
                    assert same_bits(rtc.copy_var_to_nda(an).reshape(np.shape(cur[an])), np.asarray(cur[an], F)), (an, "an input was written")
                else:
                    out[an] = rtc.copy_var_to_nda(an)
            outs.append(out)
        return outs if isinstance(ins, (list, tuple)) else outs[0]
    finally:
        for vn in made:
            rtc.release_var(vn)
        rtc.release_func("f16"); rtc.release_per_call_id_data()


_REFS = {}


def refs(op, ins, key=None):
    """-> {"S": (in, filts), "A": (in, filts), "W": (in, filts, biases)}: float64 gradients on the rounded operands, on their absolute values, and on the unrounded
    operands.  Computed once per key and left unchanged."""
    if key is not None and key in _REFS:
        return _REFS[key]
    rx, rw, rg = (to_bf16(ins[an]) for an in ("in", "filts", "out_grad_loss"))
    r = {"S": torch_grads(op, rx, rw, rg)[:2], "A": torch_grads(op, np.abs(rx), np.abs(rw), np.abs(rg))[:2], "W": torch_grads(op, ins["in"], ins["filts"], ins["out_grad_loss"])}
    if key is not None:
        _REFS[key] = r
    return r


def n_terms(op, which):
    g = op.bck_conv_geom()
    return g["B"] * g["OH"] * g["OW"] if which == "filts" else g["OC"] * g["KH"] * g["KW"]


def nrms(got, want):
    return float(np.sqrt(np.sum((np.asarray(got, np.float64) - want) ** 2) / max(np.sum(np.asarray(want, np.float64) ** 2), 1e-300)))


def check_bound(op, which, got, r, ksl=1, what=""):
    """The bound and the NRMS condition on one output -> the largest observed fraction of the bound (printed)."""
    i = 0 if which == "in" else 1
    S, A, W = r["S"][i], r["A"][i], r["W"][i]
    got = np.asarray(got, np.float64).reshape(S.shape)
    assert np.all(np.isfinite(got)), (what, which, "NaN / inf left in the output")
    K = n_terms(op, which)
    bound = 2.0 * (K + ksl + 3) * U * A
    err = np.abs(got - S)
    frac = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    e = nrms(got, W)
    print(f"{what} {which}: K={K} ksl={ksl} largest fraction of the bound {frac:.3f}, NRMS vs unrounded float64 {e:.2e}")
    assert frac <= 1.0, (what, which, f"K={K} ksl={ksl}: |got - S| reaches {frac:.3f} of the bound")
    assert e < NRMS_BOUND, (what, which, e)
    return frac


def plan_of(launch, kernel="bodahip_bconv_filts_biases_bf16"):
    """(BK, KSL) of a launch, from its configuration string BIxBJxBK_wWIxWJ[_sKSL]."""
    assert launch["kernel"] == kernel, launch
    cfg = launch["cfg"]
    return int(cfg.split("_")[0].split("x")[2]), (int(cfg.split("_s")[1].split("_")[0]) if "_s" in cfg else 1)
