"""The ReLU gradient folded into the call before it (the function-op flag zero_if_in_non_pos; ConvPipeBck(fuse_relu_grad=True)) without a GPU.

The rule is hip_zero_if_non_pos's with cond = the producer's forward input: in_grad_loss[e] = in[e] > 0 ? g[e] : +0, g[e] what the unflagged function writes -- a select, so a
+0, -0 or NaN condition gives +0 whatever g is.  Every comparison here is np.array_equal on the uint32 views: the flagged function on be=cpu against the unflagged function
followed by hip_zero_if_non_pos, the fused step against the default step node by node.  The shapes are the ones tests/test_gpu_bck_fuse.py runs on be=hip."""
import os

import numpy as np
import pytest

from boda_amd.bck_pipe import ConvPipeBck, add_bck_ops, plan_relu_grad_folds
from boda_amd.cnn_op import NATIVE_ARGS, OpTune, add_bck_conv_annotations, add_bck_op_annotations, fuse_zero_if_in_non_pos, pipe_func_args
from boda_amd.conv_pipe import ConvPipe, PipeOp, _conv, alexnet_ng_conv, googlenet_conv, nin_imagenet
from boda_amd.op import Dims, RtErr
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc

from test_bck_conv_cpu import bck_op
from test_bck_ops_cpu import bck_lrn_op, pool_op, spreading_op, zinp_op
from test_bck_pipe_cpu import GOOGLENET_TOPS, N_CLASS, grad_nodes, run_func, small_inputs, small_params

B = 3
# (B, C, H, W, OC, KH, KW, SY, SX, PY, PX)
CONV = {
    "k3s1p1_5to7_6x5": (B, 5, 6, 5, 7, 3, 3, 1, 1, 1, 1),
    "k3s2p1_7x7": (B, 4, 7, 7, 6, 3, 3, 2, 2, 1, 1),
    "k1s2p0_5x5": (B, 6, 5, 5, 8, 1, 1, 2, 2, 0, 0),       # the odd rows / columns are reached by no term: +0 with or without the flag
    "k5s1p2_c33": (B, 33, 6, 6, 4, 5, 5, 1, 1, 2, 2),      # one channel more than a 32-row MFMA block
}
# (B, C, H, W, kern, stride, pad, avg)
SPREAD = {
    "max_k3s2_partial": (B, 5, 8, 8, (3, 3), (2, 2), (0, 0), 0),   # 8 = 2 * 3 + 2: the last window is clipped
    "avg_global_6x6": (B, 8, 6, 6, (6, 6), (1, 1), (0, 0), 1),
}
LRN_SHAPE = (B, 8, 3, 3, 5, 2.0)   # (B, C, H, W, local_size, k)
ALPHA, BETA = 0.05, 0.75
# forced tiles of hip_bconv_in (BI x BJ x BK x WI x WJ; a wave owns BI/(32 WI) x BJ/(32 WJ) blocks of 32 x 32) and the shapes they run on: the epilogue's index map
TILES = ["64x128x16x1x2",    # 1 x 2 waves, 2 x 2 blocks per wave
         "128x64x16x2x1",    # 2 x 1 waves, 2 x 2 blocks per wave
         "64x64x16x2x2",     # 2 x 2 waves, one block per wave
         "32x128x16x1x4"]    # 1 x 4 waves, one block per wave
TILE_SHAPES = {
    "k5s1p2_c33": CONV["k5s1p2_c33"],                       # 33 channels, 108 pels: ragged against every tile
    "k3s2p1_7x7": CONV["k3s2p1_7x7"],                       # four phases of 48 / 36 / 36 / 27 pels
    "k3s1p1_c70_9x9": (B, 70, 9, 9, 8, 3, 3, 1, 1, 1, 1),   # 70 channels (two or three channel tiles), 243 pels (two to four pel tiles), both ragged
}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops", "bck-fuse-ops.txt")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits_eq(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(bits(a), bits(b))


def special_in(shape, seed):
    """A forward input with every kind of condition value: negative, +0, -0, NaN and positive ones (asserted)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2, 2, shape).astype(np.float32)
    kind = rng.integers(0, 10, shape)
    x[kind == 0] = 0.0; x[kind == 1] = -0.0; x[kind == 2] = np.nan
    flat = x.reshape(-1)
    flat[:5] = np.array([0.0, -0.0, np.nan, -1.5, 1e-45], np.float32)   # (1e-45: the smallest positive value still passes)
    b = bits(x)
    assert np.any(x < 0) and np.any(b == 0) and np.any(b == 0x80000000) and np.any(np.isnan(x)) and np.any(x > 0)
    return x


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


# ---- the three functions and their inputs
def conv_funcs(shape, tile=""):
    fi = add_bck_conv_annotations(bck_op(*shape), OpTune(hip_tile=tile))[0]
    return fi, fuse_zero_if_in_non_pos(fi)


def conv_ins(shape, seed):
    B_, C, H, W, OC, KH, KW = shape[:7]
    op = bck_op(*shape)
    rng = np.random.default_rng(seed)
    return {"filts": rng.uniform(-1, 1, op.get_dims("filts").sizes).astype(np.float32), "out_grad_loss": rng.uniform(-2, 2, op.get_dims("out_grad_loss").sizes).astype(np.float32),
            "in": special_in((B_, C, H, W), seed + 1)}


def spread_funcs(geom):
    f = add_bck_op_annotations(spreading_op(*geom[:7], avg=geom[7]), OpTune())[0]
    return f, fuse_zero_if_in_non_pos(f)


def spread_ins(rtc_cpu, geom, seed):
    """`in` with the special values, the forward pooling of it on be=cpu (out, and for a max pooling its argmax), a random out_grad_loss."""
    x = special_in(geom[:4], seed)
    fp = add_bck_op_annotations(pool_op(*geom[:7], avg=geom[7], emit=0 if geom[7] else 1), OpTune())[0]
    fwd = run_func(rtc_cpu, fp, {"in": x})
    ogl = np.random.default_rng(seed + 1).uniform(-2, 2, fwd["out"].shape).astype(np.float32)
    return {"out": fwd["out"], "out_grad_loss": ogl, "out_in_yx": fwd["out_in_yx"], "in": x}


def lrn_funcs(shape=LRN_SHAPE):
    B_, C, H, W, ls, k = shape
    f = add_bck_op_annotations(bck_lrn_op(B_, C, H, W, ls, ALPHA, BETA, k), OpTune())[0]
    return f, fuse_zero_if_in_non_pos(f)


def lrn_ins(shape, seed):
    """bck_lrn's gradient at an element reads `in` at that element only, so out / out_scale_base need not follow from `in`: finite values of the right magnitude."""
    rng = np.random.default_rng(seed)
    s = shape[:4]
    return {"in": special_in(s, seed + 1), "out": rng.uniform(-2, 2, s).astype(np.float32), "out_grad_loss": rng.uniform(-2, 2, s).astype(np.float32),
            "out_scale_base": rng.uniform(1, 3, s).astype(np.float32)}


def then_zinp(rtc, g, cond):
    """hip_zero_if_non_pos(in = g, cond) on `rtc`."""
    dims = tuple(zip(("img", "chan", "y", "x"), g.shape))
    return run_func(rtc, add_bck_op_annotations(zinp_op(dims), OpTune())[0], {"in": g, "cond": cond})["out"]


def check_func(rtc, plain, flagged, ins):
    """flagged == plain followed by hip_zero_if_non_pos(cond = in), bit for bit; in_grad_loss starts as NaN and must come back wholly written."""
    g = run_func(rtc, plain, {k: v for k, v in ins.items() if k in dict(pipe_func_args(plain))})["in_grad_loss"]
    want = then_zinp(rtc, g, ins["in"])
    got = run_func(rtc, flagged, dict(ins, in_grad_loss=np.full(g.shape, np.nan, np.float32)))["in_grad_loss"]
    assert bits_eq(got, want)
    assert not np.any(np.isnan(got[ins["in"] > 0])) and np.all(bits(got)[~(ins["in"] > 0)] == 0)
    return g, got


def fixture_ops():
    """The function ops tests/test_gpu_bck_fuse.py launches that no other fixture lists (flagged ones, and forced tiles with and without the flag), in a fixed order:
    what tests/golden/ops/bck-fuse-ops.txt holds, so that build() specialises them ahead of the GPU run."""
    from boda_amd.conv_pipe import DryRtc
    ops = []
    for name in sorted(CONV):
        ops += list(conv_funcs(CONV[name]))
    for name in sorted(SPREAD):
        ops += list(spread_funcs(SPREAD[name]))
    ops += list(lrn_funcs())
    for t in TILES:
        for name in sorted(TILE_SHAPES):
            ops += list(conv_funcs(TILE_SHAPES[name], t))
    drv = ConvPipeBck(DryRtc(), fuse_relu_grad=True); drv.init(add_bck_ops(nin_imagenet(2)), {n: np.zeros(d.sizes, np.float32) for n, d in nin_imagenet(2).params.items()})
    ops += [f for _, f, _ in drv.calls() if f.has("zero_if_in_non_pos")]
    seen, out = set(), []
    for f in ops:
        if f.to_str() not in seen:
            seen.add(f.to_str()); out.append(f)
    return out


def test_fixture_file_lists_these_ops():
    from boda_amd.op import read_ops
    assert [o.to_str() for o in read_ops(GOLD)] == [o.to_str() for o in fixture_ops()]


# ---- 1. the functions on be=cpu
def test_arg_lists_and_flag():
    fi, ffi = conv_funcs(CONV["k3s2p1_7x7"])
    assert not fi.has("zero_if_in_non_pos") and ffi.get_u32("zero_if_in_non_pos") == 1 and ffi.get_func_name() == "hip_bconv_in"
    assert pipe_func_args(fi) == NATIVE_ARGS["hip_bconv_in"]
    assert pipe_func_args(ffi) == (("filts", "IN"), ("out_grad_loss", "IN"), ("stride", "REF"), ("in_pad", "REF"), ("in", "IN"), ("in_grad_loss", "OUT"))
    fs, ffs = spread_funcs(SPREAD["max_k3s2_partial"])
    assert pipe_func_args(fs) == NATIVE_ARGS["hip_spreading"]
    assert pipe_func_args(ffs) == NATIVE_ARGS["hip_spreading"][:-1] + (("in", "IN"), ("in_grad_loss", "OUT"))
    fl, ffl = lrn_funcs()
    assert pipe_func_args(ffl) == pipe_func_args(fl) == NATIVE_ARGS["hip_bck_lrn"] and ffl.get_u32("zero_if_in_non_pos") == 1
    assert NATIVE_ARGS["hip_bconv_in"][-2:] == (("in_pad", "REF"), ("in_grad_loss", "OUT"))   # the table itself is unchanged
    for other in (add_bck_conv_annotations(bck_op(*CONV["k3s2p1_7x7"]), OpTune())[1:] + add_bck_op_annotations(zinp_op((("v", 8),)), OpTune())):
        with pytest.raises(RtErr, match="fuse_zero_if_in_non_pos"):
            fuse_zero_if_in_non_pos(other)


def test_explain_plan_shows_the_flag():
    from boda_amd import rtc as rtc_mod
    for plain, flagged in (conv_funcs(CONV["k3s2p1_7x7"]), spread_funcs(SPREAD["max_k3s2_partial"]), lrn_funcs()):
        p, f = rtc_mod.explain_plan(plain), rtc_mod.explain_plan(flagged)
        assert "ZINP" not in p and f == p + " -DZINP=1", (p, f)
    with pytest.raises(RtErr, match="zero_if_in_non_pos"):
        ff = add_bck_conv_annotations(bck_op(*CONV["k3s2p1_7x7"]), OpTune())[2]; ff.set_u32("zero_if_in_non_pos", 1)
        rtc_mod.explain_plan(ff)


@pytest.mark.parametrize("name", sorted(CONV))
def test_cpu_bconv_in(cpu, name):
    g, got = check_func(cpu, *conv_funcs(CONV[name]), conv_ins(CONV[name], 11))
    if name == "k1s2p0_5x5":   # pels no term reaches: +0 from the unflagged function already, +0 under any condition
        assert np.all(bits(g[:, :, 1::2, :]) == 0) and np.all(bits(g[:, :, :, 1::2]) == 0) and np.all(bits(got[:, :, 1::2, :]) == 0)


@pytest.mark.parametrize("name", sorted(SPREAD))
def test_cpu_spreading(cpu, name):
    check_func(cpu, *spread_funcs(SPREAD[name]), spread_ins(cpu, SPREAD[name], 21))


def test_cpu_bck_lrn(cpu):
    check_func(cpu, *lrn_funcs(), lrn_ins(LRN_SHAPE, 31))


def test_flag_zero_is_the_unflagged_function(cpu):
    fi, ffi = conv_funcs(CONV["k3s1p1_5to7_6x5"])
    f0 = fi.copy(); f0.set_u32("zero_if_in_non_pos", 0)
    ins = conv_ins(CONV["k3s1p1_5to7_6x5"], 41)
    assert pipe_func_args(f0) == NATIVE_ARGS["hip_bconv_in"]
    assert bits_eq(run_func(cpu, f0, ins)["in_grad_loss"], run_func(cpu, fi, ins)["in_grad_loss"])


# ---- 2. a non-finite gradient under a non-positive condition: +0, so a select and not a product
def nonfinite_cases(rtc_cpu):
    """(name, plain, flagged, ins, where): out_grad_loss holds +inf / NaN so that the unflagged gradient is non-finite exactly on `where`, and in <= 0 (or NaN) exactly there."""
    rng = np.random.default_rng(51)
    cases = []
    # 1x1 / stride 1 convolution: a pel's gradient reads out_grad_loss at that pel only.  Pels (y + x) % 3 == 0 are the poisoned ones
    shape = (B, 5, 4, 5, 6, 1, 1, 1, 1, 0, 0)
    bad = (np.add.outer(np.arange(4), np.arange(5)) % 3 == 0)[None, None]
    ins = conv_ins(shape, 52)
    ins["filts"] = np.abs(ins["filts"]) + np.float32(0.5)   # (every product with the +inf is +inf: no inf - inf left to chance, the NaN pels are NaN anyway)
    ins["in"] = np.where(bad, rng.choice(np.array([-1.0, 0.0, -0.0, np.nan], np.float32), ins["in"].shape), np.abs(rng.uniform(0.5, 2, ins["in"].shape))).astype(np.float32)
    ogl = np.abs(ins["out_grad_loss"]) + np.float32(0.5)
    ogl[:, 0:1] = np.where(bad, np.float32(np.inf), ogl[:, 0:1]); ogl[:, 3:4] = np.where(bad & (np.arange(5) % 2 == 0), np.float32(np.nan), ogl[:, 3:4])
    ins["out_grad_loss"] = ogl
    cases.append(("bconv_in", *conv_funcs(shape), ins, np.broadcast_to(bad, ins["in"].shape)))
    # global average pooling: a plane's gradient is its one out_grad_loss value / area.  Odd channels are the poisoned planes
    geom = SPREAD["avg_global_6x6"]
    ins = spread_ins(rtc_cpu, geom, 53)
    badp = np.broadcast_to((np.arange(geom[1]) % 2 == 1)[None, :, None, None], ins["in"].shape)
    ins["in"] = np.where(badp, rng.choice(np.array([-1.0, 0.0, -0.0, np.nan], np.float32), ins["in"].shape), np.abs(rng.uniform(0.5, 2, ins["in"].shape))).astype(np.float32)
    ogl = ins["out_grad_loss"].copy(); ogl[:, 1::4] = np.inf; ogl[:, 3::4] = np.nan
    ins["out_grad_loss"] = ogl
    cases.append(("spreading", *spread_funcs(geom), ins, badp))
    # LRN gradient: an element reads out_grad_loss at its pel, in a window of channels.  Poisoned pels: the centre column of the 3 x 3 plane
    ins = lrn_ins(LRN_SHAPE, 54)
    badl = np.broadcast_to((np.arange(3) == 1)[None, None, None, :], ins["in"].shape)
    ins["in"] = np.where(badl, rng.choice(np.array([-1.0, 0.0, -0.0, np.nan], np.float32), ins["in"].shape), np.abs(rng.uniform(0.5, 2, ins["in"].shape))).astype(np.float32)
    ogl = ins["out_grad_loss"].copy(); ogl[:, :, :, 1] = np.inf; ogl[:, 2, :, 1] = np.nan
    ins["out_grad_loss"] = ogl
    cases.append(("bck_lrn", *lrn_funcs(), ins, badl))
    return cases


def check_nonfinite(rtc, case):
    name, plain, flagged, ins, where = case
    g = run_func(rtc, plain, {k: v for k, v in ins.items() if k in dict(pipe_func_args(plain))})["in_grad_loss"]
    assert not np.any(np.isfinite(g[where])) and np.all(np.isfinite(g[~where])), name   # the test's own premise
    assert not np.any(ins["in"][where] > 0) and np.all(ins["in"][~where] > 0), name
    got = run_func(rtc, flagged, dict(ins, in_grad_loss=np.full(g.shape, np.nan, np.float32)))["in_grad_loss"]
    assert np.all(bits(got)[where] == 0), name                    # +0, not NaN (0 * inf) and not -0
    assert np.array_equal(bits(got)[~where], bits(g)[~where]), name


def test_cpu_non_finite_gradient_is_selected_away(cpu):
    cases = nonfinite_cases(cpu)
    assert [c[0] for c in cases] == ["bconv_in", "spreading", "bck_lrn"]
    for case in cases:
        check_nonfinite(cpu, case)


# ---- 3. refusals
def run_with_vars(rtc, fop, var_dims, arg_map, arg_names):
    rtc.compile([RtcFuncInfo("g", "", list(arg_names), fop)])
    try:
        for vn, d in var_dims.items():
            rtc.create_var_with_dims(vn, d)
        rtc.run(RtcFuncCall("g", arg_map))
        rtc.finish_and_sync()
    finally:
        for vn in var_dims:
            rtc.release_var(vn)
        rtc.release_func("g"); rtc.release_per_call_id_data()


def check_refusals(rtc):
    shape = CONV["k3s2p1_7x7"]
    op = bck_op(*shape)
    fi, fb, ff = add_bck_conv_annotations(op, OpTune())
    ffi = fuse_zero_if_in_non_pos(fi)
    refs = {"stride": RtcArg.ref(op.get_dims("stride")), "in_pad": RtcArg.ref(op.get_dims("in_pad"))}
    # the flag on the filter gradient (it reads out_grad_loss against in, it writes no in_grad_loss)
    bad = ff.copy(); bad.set_u32("zero_if_in_non_pos", 1)
    vd = {an: op.get_dims(an) for an in ("in", "out_grad_loss", "filts_grad_loss")}
    with pytest.raises(RtErr, match="zero_if_in_non_pos"):
        run_with_vars(rtc, bad, vd, dict({an: RtcArg.var(an) for an in vd}, **refs), [a for a, _ in NATIVE_ARGS["hip_bconv_filts"]])
    badb = fb.copy(); badb.set_u32("zero_if_in_non_pos", 1)
    with pytest.raises(RtErr, match="zero_if_in_non_pos"):
        run_with_vars(rtc, badb, {an: op.get_dims(an) for an in ("out_grad_loss", "biases_grad_loss")}, {an: RtcArg.var(an) for an in ("out_grad_loss", "biases_grad_loss")},
                      [a for a, _ in NATIVE_ARGS["hip_bconv_biases"]])
    names = [a for a, _ in pipe_func_args(ffi)]
    vd = {an: op.get_dims(an) for an in ("filts", "out_grad_loss", "in", "in_grad_loss")}
    # a flagged call that binds no `in`
    am = dict({an: RtcArg.var(an) for an in ("filts", "out_grad_loss", "in_grad_loss")}, **refs)
    with pytest.raises(RtErr, match="'in'"):
        run_with_vars(rtc, ffi, vd, am, names)
    # `in` with other dims than the op's in
    wrong = dict(vd, **{"in": Dims.make("float", img=shape[0], chan=shape[1], y=shape[2], x=shape[3] + 1)})
    with pytest.raises(RtErr, match="arg 'in' has dims"):
        run_with_vars(rtc, ffi, wrong, dict(am, **{"in": RtcArg.var("in")}), names)
    # `in` and in_grad_loss one var
    with pytest.raises(RtErr, match="same var"):
        run_with_vars(rtc, ffi, vd, dict(am, **{"in": RtcArg.var("in_grad_loss")}), names)
    # the two other functions refuse the alias as well
    fs, ffs = spread_funcs(SPREAD["max_k3s2_partial"])
    vs = {an: ffs.get_dims(an) for an in ("out", "out_grad_loss", "out_in_yx", "in_grad_loss")}
    ams = dict({an: RtcArg.var(an) for an in vs}, **{an: RtcArg.ref(ffs.get_dims(an)) for an in ("kern_sz", "stride", "in_pad")})
    with pytest.raises(RtErr, match="same var"):
        run_with_vars(rtc, ffs, vs, dict(ams, **{"in": RtcArg.var("in_grad_loss")}), [a for a, _ in pipe_func_args(ffs)])
    with pytest.raises(RtErr, match="'in'"):
        run_with_vars(rtc, ffs, vs, ams, [a for a, _ in pipe_func_args(ffs)])
    fl, ffl = lrn_funcs()
    vl = {an: ffl.get_dims(an) for an in ("out", "out_grad_loss", "out_scale_base", "in_grad_loss")}
    with pytest.raises(RtErr, match="same var"):
        run_with_vars(rtc, ffl, vl, dict({an: RtcArg.var(an) for an in vl}, **{"in": RtcArg.var("in_grad_loss")}), [a for a, _ in NATIVE_ARGS["hip_bck_lrn"]])


def test_cpu_refusals(cpu):
    check_refusals(cpu)


# ---- 4. which ReLU gradients fold
def _head(p, bot):
    """global average -> 1x1 conv -> loss: ends a hand-built pipe in the 1 x 1 plane the softmax loss takes"""
    p.add(PipeOp("gap", "Pooling", bot, "gap", kern_sz=None, avg_pool=1))
    p.add(PipeOp("fc", "Convolution", "gap", "fc", out_chans=N_CLASS, kern_sz=(1, 1)))
    return p


def relu_conv():
    p = ConvPipe("relu_conv", "data", Dims.make("float", img=B, chan=3, y=7, x=7))
    _conv(p, "c1", "data", 6, 3, 1, 1); _conv(p, "c2", "c1", 5, 3, 2, 1)
    return _head(p, "c2")


def relu_pool():
    p = ConvPipe("relu_pool", "data", Dims.make("float", img=B, chan=3, y=8, x=8))
    _conv(p, "c1", "data", 6, 3, 1, 1)
    p.add(PipeOp("p1", "Pooling", "c1", "p1", kern_sz=(3, 3), stride=(2, 2)))
    return _head(p, "p1")


def relu_lrn():
    p = ConvPipe("relu_lrn", "data", Dims.make("float", img=B, chan=3, y=6, x=6))
    _conv(p, "c1", "data", 8, 3, 1, 1)
    p.add(PipeOp("n1", "LRN", "c1", "n1", lrn=(5, 0.05, 0.75, 1.0)))
    return _head(p, "n1")


def relu_drop_conv():
    p = ConvPipe("relu_drop_conv", "data", Dims.make("float", img=B, chan=3, y=7, x=7))
    _conv(p, "c1", "data", 6, 3, 1, 1)
    p.add(PipeOp("d1", "Dropout", "c1", "c1"))
    p.add(PipeOp("c2", "Convolution", "c1", "c2", out_chans=5, kern_sz=(3, 3), in_pad=(1, 1)))
    return _head(p, "c2")


def relu_two_convs():
    p = ConvPipe("relu_two_convs", "data", Dims.make("float", img=B, chan=3, y=7, x=7))
    _conv(p, "c1", "data", 6, 3, 1, 1)
    p.add(PipeOp("a", "Convolution", "c1", "a", out_chans=4, kern_sz=(1, 1)))
    p.add(PipeOp("b", "Convolution", "c1", "b", out_chans=3, kern_sz=(3, 3), in_pad=(1, 1)))
    p.add(PipeOp("cat", "Concat", "a", "cat", bots=("a", "b")))
    return _head(p, "cat")


# name -> (builder, {folded ZeroIfNonPos tag: the op that takes it}, unfolded tags)
HAND = {
    "relu_conv": (relu_conv, {"relu_c1_bck": "c2_bck", "relu_c2_bck": "gap_bck"}, []),
    "relu_pool": (relu_pool, {"relu_c1_bck": "p1_bck"}, []),
    "relu_lrn": (relu_lrn, {"relu_c1_bck": "n1_bck"}, []),
    "relu_drop_conv": (relu_drop_conv, {}, ["relu_c1_bck"]),
    "relu_two_convs": (relu_two_convs, {}, ["relu_c1_bck"]),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_which_fold_hand_built(name):
    mk, want, unfolded = HAND[name]
    folds, why = plan_relu_grad_folds(add_bck_ops(mk()))
    assert folds == want and sorted(why) == unfolded
    if name == "relu_drop_conv":
        assert "BckDropout" in why["relu_c1_bck"]
    if name == "relu_two_convs":
        assert "Reduce" in why["relu_c1_bck"]


def test_which_fold_real_nets():
    """The unfolded ReLU gradients, read off the net definitions: a ReLU whose node a Dropout rewrites (AlexNet fc6 / fc7, GoogLeNet's cls1_fc1 / cls2_fc1), and a ReLU whose
    node goes into a Concat (GoogLeNet's icpN_out0 .. 3: a Split writes their gradient).  Everything else has one reader that is a convolution, a pooling or an LRN."""
    folds, why = plan_relu_grad_folds(add_bck_ops(nin_imagenet(2)))
    assert why == {} and len(folds) == 12
    assert folds["relu_cccp8_bck"] == "pool4_bck" and folds["relu_cccp6_bck"] == "pool3_bck" and folds["relu_conv4_bck"] == "cccp7_bck"
    folds, why = plan_relu_grad_folds(add_bck_ops(alexnet_ng_conv(2)))
    assert sorted(why) == ["relu_fc6_bck", "relu_fc7_bck"]
    assert folds == {"relu_conv5_bck": "pool5_bck", "relu_conv4_bck": "conv5_bck", "relu_conv3_bck": "conv4_bck", "relu_conv2_bck": "norm2_bck", "relu_conv1_bck": "norm1_bck"}
    folds, why = plan_relu_grad_folds(add_bck_ops(googlenet_conv(2), loss_tops=GOOGLENET_TOPS))
    assert sorted(why) == sorted([f"relu_icp{n}_out{k}_bck" for n in range(1, 10) for k in range(4)] + ["relu_cls1_fc1_bck", "relu_cls2_fc1_bck"])
    want = {"relu1_bck": "pool1_bck", "relu_reduction2_bck": "conv2_bck", "relu2_bck": "norm2_bck", "relu_cls1_reduction_bck": "cls1_fc1-conv_bck", "relu_cls2_reduction_bck": "cls2_fc1-conv_bck"}
    for n in range(1, 10):
        want[f"relu_icp{n}_reduction1_bck"] = f"icp{n}_out1_bck"; want[f"relu_icp{n}_reduction2_bck"] = f"icp{n}_out2_bck"
    assert folds == want


# ---- 5. the whole step on be=cpu
def step(rtc, bp, fuse, params, data, label, gets):
    drv = ConvPipeBck(rtc, fuse_relu_grad=fuse); drv.init(bp, params)
    try:
        drv.set_det_drop_seed(1234)
        fwd = {"data": data, "label": label}
        drv.run_bck(["data", "label"], fwd, gets)
        return fwd, [(t, f.get_func_name()) for t, f, _ in drv.calls()], drv.calls(), dict(drv.fused_relu_grads)
    finally:
        drv.release()


@pytest.mark.parametrize("name", sorted(HAND))
def test_cpu_fused_step_equals_default(cpu, name):
    mk, want, unfolded = HAND[name]
    cp = mk(); bp = add_bck_ops(cp)
    params = small_params(cp, 3); data, label = small_inputs(cp, 3)
    gets = [n for n in bp.nodes if n != bp.label_node]   # every node: activations, params, every *_grad_loss, the loss
    a, names_a, _, info_a = step(cpu, bp, False, params, data, label, gets)
    b, names_b, calls_b, info_b = step(cpu, bp, True, params, data, label, gets)
    for n in gets:
        assert bits_eq(a[n], b[n]), n
    assert set(grad_nodes(bp)) <= set(gets) and "loss" in gets
    assert info_a["folded"] == [] and sorted(info_a["unfolded"]) == sorted(list(want) + unfolded)
    assert sorted(info_b["folded"]) == sorted(want) and sorted(info_b["unfolded"]) == unfolded
    # the fused list: the default list without the folded calls; the ops that take a ReLU gradient carry the flag and bind `in` to the ReLU's node
    assert names_b == [(t, f) for t, f in names_a if t not in want]
    assert [t for t, f in names_a if f == "hip_zero_if_non_pos"] == [o.tag for o in bp.bck_ops() if o.type == "ZeroIfNonPos"]
    takers = set(want.values())
    for t, f, am in calls_b:
        flagged = f.has("zero_if_in_non_pos") and f.get_u32("zero_if_in_non_pos") == 1
        assert flagged == (t in takers and f.get_func_name() in ("hip_bconv_in", "hip_spreading", "hip_bck_lrn")), (t, f.get_func_name())
        if flagged:
            relu = [z for z, p in want.items() if p == t][0]
            assert am["in"].n == relu[len("relu_"):-len("_bck")] and am["in_grad_loss"].n == am["in"].n + "_grad_loss"


def test_cpu_default_calls_are_todays(cpu):
    """The default call list of the `chain` pipe of tests/test_bck_pipe_cpu.py, as that file pins it; fuse_relu_grad=True drops exactly relu_conv1_bck from it."""
    from test_bck_pipe_cpu import chain
    cp = chain(); bp = add_bck_ops(cp)
    params = small_params(cp, 0); data, label = small_inputs(cp, 0)
    gets = grad_nodes(bp) + ["loss"]
    a, names_a, calls_a, _ = step(cpu, bp, False, params, data, label, gets)
    assert names_a == [("conv1", "hip_conv"), ("norm1", "hip_lrn_sb"), ("pool1", "hip_pool_yx"), ("drop1", "hip_dropout"), ("fc", "hip_conv"),
                       ("loss", "hip_softmax"), ("loss", "hip_sm_grad_and_loss"), ("loss", "hip_sum_loss_over_imgs"),
                       ("fc_bck", "hip_bconv_in"), ("fc_bck", "hip_bconv_biases"), ("fc_bck", "hip_bconv_filts"), ("drop1_bck", "hip_dropout"), ("pool1_bck", "hip_spreading"),
                       ("norm1_bck", "hip_bck_lrn"), ("relu_conv1_bck", "hip_zero_if_non_pos"),
                       ("conv1_bck", "hip_bconv_in"), ("conv1_bck", "hip_bconv_biases"), ("conv1_bck", "hip_bconv_filts")]
    assert not any(f.has("zero_if_in_non_pos") for _, f, _ in calls_a)
    b, names_b, _, info = step(cpu, bp, True, params, data, label, gets)
    assert names_b == [x for x in names_a if x[0] != "relu_conv1_bck"] and info["folded"] == ["relu_conv1_bck"]
    for n in gets:
        assert bits_eq(a[n], b[n]), n
