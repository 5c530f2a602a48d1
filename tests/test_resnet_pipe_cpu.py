"""ResNet-50 as a whole net, without a GPU: the three op types of the pipe (BatchNorm, Scale, Eltwise), resnet50() against the shipped convolution lists, fold_affine,
hip_chan_affine on be=cpu bit for bit against numpy, what ConvPipeFwd compiles for the net on a recording backend (fp32: hip_chan_affine / hip_reduce /
hip_zero_if_non_pos; channels-last bf16: affine runs folded into their convolutions, 16 of 16 residual adds in a convolution's epilogue, or 16 nhwc_eltwise calls with
fuse_residual=False), and every refusal of the residual epilogue that needs no device.  The GPU side is tests/test_gpu_resnet.py."""
import os
from collections import Counter

import numpy as np
import pytest

import resnet_ref as rr
from boda_amd import conv_pipe as cpm, nhwc, rtc as rtc_mod
from boda_amd.cnn_op import NATIVE_ARGS, OpTune, add_codegen_annotations, chan_affine_func_op, pipe_func_args
from boda_amd.conv_pipe import ConvPipe, ConvPipeFwd, DryRtc, PipeOp, fold_affine, resnet50
from boda_amd.op import Dims, RtErr, UnsupErr, data_path, parse_op
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc

NHWC = OpTune(hip_dtype="bf16", hip_layout="nhwc")


# ---- the pipe's three op types
def _pipe(C=8, H=6):
    p = ConvPipe("t", "data", Dims.make("float", img=2, chan=C, y=H, x=H))
    p.add(PipeOp("c1", "Convolution", "data", "c1", out_chans=16, kern_sz=(3, 3), in_pad=(1, 1)))
    p.add(PipeOp("c2", "Convolution", "data", "c2", out_chans=16, kern_sz=(1, 1)))
    return p


def test_batchnorm_scale_eltwise_shape_inference_and_params():
    p = _pipe()
    p.add(PipeOp("bn1", "BatchNorm", "c1", "c1")).add(PipeOp("sc1", "Scale", "c1", "c1"))
    assert p.nodes["c1"] == Dims.make("float", img=2, chan=16, y=6, x=6)
    ch = Dims.make("float", chan=16)
    assert {k: v for k, v in p.params.items() if k.startswith(("bn1", "sc1"))} == {"bn1_mean": ch, "bn1_var": ch, "sc1_scale": ch, "sc1_bias": ch}
    assert p.ops[-2].eps == 1e-5 and PipeOp("b", "BatchNorm", "c1", "c1", eps=1e-3).eps == 1e-3
    p.add(PipeOp("sum", "Eltwise", "c1", "sum", bots=("c1", "c2")))
    assert p.nodes["sum"] == p.nodes["c1"] and "sum_filts" not in p.params
    p.add(PipeOp("sum3", "Eltwise", "c1", "sum3", bots=("c1", "c2", "sum")))
    assert p.nodes["sum3"] == p.nodes["c1"]


def test_op_type_errors():
    p = _pipe()
    with pytest.raises(UnsupErr, match="in place"):
        p.add(PipeOp("bn", "BatchNorm", "c1", "other"))
    with pytest.raises(RtErr, match="unknown node"):
        p.add(PipeOp("bn", "Scale", "nope", "nope"))
    with pytest.raises(RtErr, match="unknown node"):
        p.add(PipeOp("s", "Eltwise", "c1", "s", bots=("c1", "nope")))
    p.add(PipeOp("c3", "Convolution", "data", "c3", out_chans=8, kern_sz=(1, 1)))
    with pytest.raises(RtErr, match="mismatched sizes"):
        p.add(PipeOp("s", "Eltwise", "c1", "s", bots=("c1", "c3")))
    with pytest.raises(UnsupErr, match="2 to 8"):
        p.add(PipeOp("s", "Eltwise", "c1", "s", bots=("c1",)))
    with pytest.raises(UnsupErr, match="2 to 8"):
        p.add(PipeOp("s", "Eltwise", "c1", "s", bots=("c1",) * 9))
    with pytest.raises(RtErr, match="new node"):
        p.add(PipeOp("s", "Eltwise", "c1", "c1", bots=("c1", "c2")))
    with pytest.raises(RtErr, match="written twice"):
        p.add(PipeOp("s", "Eltwise", "c1", "c2", bots=("c1", "c1")))
    with pytest.raises(UnsupErr, match="no forward kernel"):
        p.add(PipeOp("x", "Sigmoid", "c1", "c1"))


def test_resnet50_equals_the_shipped_convolution_lists():
    p = resnet50(1)
    convs = [o for o in p.ops if o.type == "Convolution"]
    with open(data_path("ops", "resnet-50-conv-ops-b1.txt")) as f:
        want_ops = [l.strip() for l in f if l.strip()]
    with open(data_path("nets", "resnet-50-conv-bottoms.txt")) as f:
        want_bots = [l.split() for l in f if l.strip()]
    assert len(convs) == 54 == len(want_ops)
    for o, w, wb in zip(convs, want_ops, want_bots):
        assert p.conv_op(o).to_str() == w, o.tag
        assert [o.tag, o.bot] == wb
    t = Counter(o.type for o in p.ops)
    assert t == {"Convolution": 54, "BatchNorm": 53, "Scale": 53, "ReLU": 49, "Eltwise": 16, "Pooling": 2}
    assert [o.tag for o in p.ops[:6]] == ["conv1", "bn_conv1", "scale_conv1", "conv1_relu", "pool1", "res2a_branch1"]
    assert [o.tag for o in p.ops if o.type == "Eltwise"] == [f"res{s}{b}" for s, n in ((2, 3), (3, 4), (4, 6), (5, 3)) for b in "abcdef"[:n]]
    e = {o.tag: o for o in p.ops}
    assert e["res2a"].bots == ("res2a_branch1", "res2a_branch2c") and e["res2b"].bots == ("res2a", "res2b_branch2c") and e["res5c"].bots == ("res5b", "res5c_branch2c")
    assert {"bn2a_branch1_mean", "bn2a_branch1_var", "scale2a_branch1_scale", "scale2a_branch1_bias", "res2a_branch1_biases", "fc1000_biases"} <= set(p.params)
    assert p.out_node() == "fc1000" and p.nodes["fc1000"] == Dims.make("float", img=1, chan=1000, y=1, x=1) and p.nodes["pool5"].sizes == (1, 2048, 1, 1)
    small = resnet50(2, 64)     # the global pool5 follows the input size
    assert small.nodes["res5c"].sizes == (2, 2048, 2, 2) and small.nodes["pool5"].sizes == (2, 2048, 1, 1) and small.nodes["res3a"].sizes == (2, 512, 8, 8)


# ---- fold_affine
def _steps(C, seed, kinds):
    rng = np.random.default_rng(seed)
    st = []
    for k in kinds:
        if k == "BatchNorm":
            st.append(("BatchNorm", rng.uniform(-2, 2, C).astype(np.float32), rng.uniform(0.01, 4, C).astype(np.float32), 1e-5))
        else:
            st.append(("Scale", rng.uniform(-2, 2, C).astype(np.float32), rng.uniform(-1, 1, C).astype(np.float32)))
    return st


@pytest.mark.parametrize("kinds", [("BatchNorm",), ("Scale",), ("BatchNorm", "Scale"), ("Scale", "BatchNorm", "Scale")])
def test_fold_affine_written_order_and_float64(kinds):
    f32 = np.float32
    st = _steps(37, len(kinds), kinds)
    a, b = fold_affine(st)
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == (37,)
    # its own written order, every operation rounded to fp32: from (1, 0); a' = a2 * a; b' = a2 * b + b2
    wa, wb = np.ones(37, f32), np.zeros(37, f32)
    for s in st:
        if s[0] == "BatchNorm":
            a2 = f32(1.0) / np.sqrt(s[2] + f32(s[3])); b2 = -(s[1] * a2)
        else:
            a2, b2 = s[1], s[2]
        wa, wb = a2 * wa, a2 * wb + b2
    assert rr.bits_eq(a, wa) and rr.bits_eq(b, wb)
    # ... and the same composition in float64.  a is a product of at most 3 factors, each within 1.5 ulp (a rounded sum, a correctly rounded sqrt and quotient): 3 ulp
    # hold for a; b is a sum that may cancel, so its error is measured against the magnitude of its terms, in ulps of that
    da, db, mag = np.ones(37), np.zeros(37), np.zeros(37)
    for s in st:
        if s[0] == "BatchNorm":
            a2 = 1.0 / np.sqrt(s[2].astype(np.float64) + np.float64(f32(s[3]))); b2 = -(s[1].astype(np.float64) * a2)
        else:
            a2, b2 = s[1].astype(np.float64), s[2].astype(np.float64)
        da, db, mag = a2 * da, a2 * db + b2, np.abs(a2) * mag + np.abs(b2)
    ulp = lambda x: np.spacing(np.abs(x).astype(f32)).astype(np.float64)
    assert (np.abs(a - da) <= 3 * ulp(da)).all() if len(kinds) <= 2 else (np.abs(a - da) <= 3 * len(kinds) * ulp(da)).all()
    assert (np.abs(b - db) <= 3 * len(kinds) * ulp(mag)).all()


def test_fold_affine_errors():
    with pytest.raises(RtErr, match="no steps"):
        fold_affine([])
    with pytest.raises(RtErr, match="neither"):
        fold_affine([("LRN", np.ones(3), np.ones(3))])
    with pytest.raises(RtErr, match="per channel"):
        fold_affine([("Scale", np.ones(3), np.ones(3)), ("Scale", np.ones(4), np.ones(4))])


# ---- hip_chan_affine: the op, the plan, be=cpu
def test_chan_affine_function_op_and_plan():
    f = rr.affine_op((3, 5, 7, 7), 1)
    assert f.get_func_name() == "hip_chan_affine" and f.get_type() == "ChanAffine" and f.get_u32("relu") == 1
    assert NATIVE_ARGS["hip_chan_affine"] == (("in", "IN"), ("a", "IN"), ("b", "IN"), ("out", "OUT")) == pipe_func_args(f)
    assert f.get_dims("a") == Dims(("chan",), (5,), "float") == f.get_dims("b") and f.flops() == 0
    assert parse_op(f.to_str()) == f and rtc_mod.parse_op_native(f.to_str()) == f.to_str()
    assert rtc_mod.explain_plan(f) == "bodahip_chan_affine grid=3 block=256 -DRELU=1"           # (one thread per element at most: 735 elements)
    assert rtc_mod.explain_plan(rr.affine_op((1, 8, 8, 8), 0)) == "bodahip_chan_affine grid=2 block=256 -DRELU=0"
    with pytest.raises(RtErr, match="one float per channel"):
        parse_op("(str_vals=(type=ChanAffine),nda_vals=(a=(dims=(chan=4)),b=(dims=(chan=5)),in=(dims=(img=1,chan=5,y=2,x=2)),out=(dims=(img=1,chan=5,y=2,x=2)),relu=(tn=uint32_t,v=0)))")
    with pytest.raises(RtErr, match="equal dims"):
        parse_op("(str_vals=(type=ChanAffine),nda_vals=(a=(dims=(chan=5)),b=(dims=(chan=5)),in=(dims=(img=1,chan=5,y=2,x=2)),out=(dims=(img=1,chan=5,y=2,x=3)),relu=(tn=uint32_t,v=0)))")
    with pytest.raises(RtErr, match="relu"):
        parse_op("(str_vals=(type=ChanAffine),nda_vals=(a=(dims=(chan=5)),b=(dims=(chan=5)),in=(dims=(img=1,chan=5,y=2,x=2)),out=(dims=(img=1,chan=5,y=2,x=2)),relu=(tn=uint32_t,v=2)))")


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


@pytest.mark.parametrize("shape", rr.AFFINE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_chan_affine_on_cpu_equals_numpy(cpu, shape):
    x, a, b = rr.affine_data(shape)
    for relu in (0, 1):
        want = rr.chan_affine_ref(x, a, b, relu)
        if relu:
            assert not np.signbit(want[want == 0]).any()
        for in_place in (False, True):
            assert rr.bits_eq(rr.run_affine(cpu, shape, relu, in_place, x, a, b), want), (shape, relu, in_place)


def test_chan_affine_refuses_wrong_vars(cpu):
    f = rr.affine_op((2, 5, 3, 3), 0)
    cpu.compile([RtcFuncInfo("g", "", ["in", "a", "b", "out"], f)])
    try:
        cpu.create_var_with_dims("x", f.get_dims("in")); cpu.create_var_with_dims("a", f.get_dims("a")); cpu.create_var_with_dims("b4", Dims(("chan",), (4,), "float"))
        with pytest.raises(RtErr, match="arg 'b' has dims"):
            cpu.run(RtcFuncCall("g", {"in": RtcArg.var("x"), "a": RtcArg.var("a"), "b": RtcArg.var("b4"), "out": RtcArg.var("x")}))
    finally:
        for v in ("x", "a", "b4"):
            cpu.release_var(v)
        cpu.release_func("g")


def test_golden_function_ops_are_current(golden_dir):
    with open(os.path.join(golden_dir, "ops", "resnet-ops.txt")) as f:
        assert [l.strip() for l in f if l.strip()] == rr.golden_lines()


# ---- what ConvPipeFwd compiles
def _dry(tune=None, cp=None, **kw):
    dry = DryRtc(); f = ConvPipeFwd(dry, tune, **kw); f.init(cp if cp is not None else resnet50(1))
    return dry, f


def test_fp32_net_runs_affine_runs_eltwise_and_its_relu_natively():
    dry, f = _dry()
    assert Counter(c.func for c in f.fwd_calls) == {"hip_conv": 54, "hip_chan_affine": 53, "hip_reduce": 16, "hip_zero_if_non_pos": 16, "fwd_pool": 2}
    by = {c.tag: c for c in f.fwd_calls}
    ops = {fi.func_name: fi.op for fi in dry.infos if fi.op is not None}
    # no fused ReLU in a convolution in front of an affine run; the run carries the ReLU behind it
    assert all(o.get_u32("conv_has_relu") == 0 for n, o in ops.items() if n.startswith("hip_conv__"))
    c = by["bn2a_branch2a+scale2a_branch2a+res2a_branch2a_relu"]
    assert ops[c.rfc.rtc_func_name].get_u32("relu") == 1 and c.rfc.arg_map["in"].n == c.rfc.arg_map["out"].n == "res2a_branch2a"
    assert ops[by["bn2a_branch2c+scale2a_branch2c"].rfc.rtc_func_name].get_u32("relu") == 0
    e = by["res2b"].rfc.arg_map
    assert (e["ins_0"].n, e["ins_1"].n, e["out"].n) == ("res2a", "res2b_branch2c", "res2b")
    z = by["res2b_relu"].rfc.arg_map
    assert z["in"].n == z["cond"].n == z["out"].n == "res2b"
    assert f.fused_residuals == {"folded": [], "unfolded": {}}
    # the dependencies of the step know the new args: the sum waits for both branches, the ReLU for the sum
    ix = {c.tag: i for i, c in enumerate(f.fwd_calls)}
    deps = f._call_deps()
    assert {ix["bn2a_branch1+scale2a_branch1"], ix["bn2a_branch2c+scale2a_branch2c"]} <= set(deps[ix["res2a"]]) and ix["res2a"] in deps[ix["res2a_relu"]]


def test_bf16_nhwc_net_folds_every_affine_run_and_every_residual():
    dry, f = _dry(NHWC)
    funcs = Counter(c.func for c in f.fwd_calls)
    assert not ({"nhwc_eltwise", "nhwc_relu", "hip_chan_affine", "hip_reduce", "hip_zero_if_non_pos"} & set(funcs)), funcs
    flagged = [fi.op for fi in dry.infos if fi.op is not None and fi.op.has("nhwc_residual") and fi.op.get_u32("nhwc_residual")]
    assert len(flagged) == 16 and all(o.get_func_name() == "hip_conv_nhwc" and o.get_u32("conv_has_relu") == 1 and o.get_dims("res") == o.get_dims("out") for o in flagged)
    elt = [o.tag for o in resnet50(1).ops if o.type == "Eltwise"]
    assert f.fused_residuals == {"folded": elt, "unfolded": {}}
    by = {c.tag: c for c in f.fwd_calls}
    a = by["res2a_branch2c+res2a+res2a_relu"].rfc.arg_map
    assert (a["res"].n, a["out"].n, a["in"].n) == ("res2a_branch1", "res2a", "res2a_branch2b")
    b = by["res2b_branch2c+res2b+res2b_relu"].rfc.arg_map
    assert (b["res"].n, b["out"].n) == ("res2a", "res2b")
    # a flagged convolution is a call of its own: in no level set, in no sibling group
    members = {t for s in f.level_sets for m in s for t in m.split("+")} | {t for g in f.groups for t in g}
    assert not any(t.endswith("branch2c") for t in members) and ("res2a_branch1", "res2a_branch2a") in f.level_sets
    # res counts as a read: the flagged call waits for the call that wrote the shortcut
    ix = {c.tag: i for i, c in enumerate(f.fwd_calls)}
    deps = f._call_deps()
    assert ix["res2a_branch2c+res2a+res2a_relu"] in deps[ix["res2b_branch2c+res2b+res2b_relu"]]
    assert ix["res2a_branch1+res2a_branch2a"] in deps[ix["res2a_branch2c+res2a+res2a_relu"]]
    # every convolution in front of a ReLU-terminated run fuses that ReLU; the folded params live in <param>_raw
    ops = {fi.func_name: fi.op for fi in dry.infos if fi.op is not None}
    assert ops["hip_conv_nhwc__resnet50_res2a_branch2b"].get_u32("conv_has_relu") == 1
    assert "res2a_branch2b_filts_raw" in dry._dims and "res2a_branch2b_biases_raw" in dry._dims and "fc1000_filts_raw" not in dry._dims
    with pytest.raises(RtErr, match="never written"):
        f.run_fwd([], {}, ["res2a_branch2c"])


def test_bf16_nhwc_net_without_residual_fusion_runs_sixteen_eltwise_kernels():
    dry, f = _dry(NHWC, fuse_residual=False)
    funcs = Counter(c.func for c in f.fwd_calls)
    assert funcs["nhwc_eltwise"] == 16 and "nhwc_relu" not in funcs
    assert not any(fi.op is not None and fi.op.has("nhwc_residual") for fi in dry.infos)
    assert f.fused_residuals["folded"] == [] and set(f.fused_residuals["unfolded"].values()) == {"fuse_residual is off"} and len(f.fused_residuals["unfolded"]) == 16
    c = {c.tag: c for c in f.fwd_calls}["res2a+res2a_relu"].rfc.arg_map
    assert (c["in_0"].n, c["in_1"].n, c["out"].n, int(c["relu"].v[0])) == ("res2a_branch1", "res2a_branch2c", "res2a", 1)


def test_plans_of_the_existing_nets_are_unchanged_by_the_option():
    for make in (lambda: cpm.googlenet_conv(3), lambda: cpm.nin_imagenet(2)):
        a = _dry(NHWC, make())[0]; b = _dry(NHWC, make(), fuse_residual=False)[0]
        sa = [(fi.func_name, fi.op.to_str()) for fi in a.infos if fi.op is not None]
        assert sa == [(fi.func_name, fi.op.to_str()) for fi in b.infos if fi.op is not None]
        assert not any("nhwc_residual" in s or "RES" in s for _, s in sa)


def test_residual_folds_say_why_not():
    def net(mid):
        p = ConvPipe("t", "data", Dims.make("float", img=2, chan=16, y=6, x=6))
        p.add(PipeOp("a", "Convolution", "data", "a", out_chans=32, kern_sz=(1, 1)))
        mid(p)
        return p
    def plain(p):
        p.add(PipeOp("b", "Convolution", "data", "b", out_chans=32, kern_sz=(1, 1)))
        p.add(PipeOp("s", "Eltwise", "a", "s", bots=("a", "b")))
    _, f = _dry(NHWC, net(plain))
    assert f.fused_residuals == {"folded": ["s"], "unfolded": {}}
    def relu_first(p):
        p.add(PipeOp("b", "Convolution", "data", "b", out_chans=32, kern_sz=(1, 1))); p.add(PipeOp("rb", "ReLU", "b", "b"))
        p.add(PipeOp("s", "Eltwise", "a", "s", bots=("a", "b")))
    assert "ReLU of its own" in _dry(NHWC, net(relu_first))[1].fused_residuals["unfolded"]["s"]
    def two_readers(p):
        p.add(PipeOp("b", "Convolution", "data", "b", out_chans=32, kern_sz=(1, 1)))
        p.add(PipeOp("s", "Eltwise", "a", "s", bots=("a", "b"))); p.add(PipeOp("c", "Convolution", "b", "c", out_chans=8, kern_sz=(1, 1)))
    assert "also read by c" in _dry(NHWC, net(two_readers))[1].fused_residuals["unfolded"]["s"]
    def three_by_three(p):     # the later-defined bottom comes from the input-patch kernel
        p.add(PipeOp("b", "Convolution", "data", "b", out_chans=32, kern_sz=(3, 3), in_pad=(1, 1)))
        p.add(PipeOp("s", "Eltwise", "a", "s", bots=("a", "b")))
    _, f = _dry(NHWC, net(three_by_three))
    assert "input-patch" in f.fused_residuals["unfolded"]["s"] and Counter(c.func for c in f.fwd_calls)["nhwc_eltwise"] == 1
    def pooled(p):
        p.add(PipeOp("b", "Pooling", "a", "b", kern_sz=(3, 3), stride=(1, 1), in_pad=(1, 1)))
        p.add(PipeOp("s", "Eltwise", "a", "s", bots=("a", "b")))
    assert "a Pooling" in _dry(NHWC, net(pooled))[1].fused_residuals["unfolded"]["s"]
    def lone_affine(p):
        p.add(PipeOp("pl", "Pooling", "a", "pl", kern_sz=(3, 3), stride=(1, 1), in_pad=(1, 1))); p.add(PipeOp("bn", "BatchNorm", "pl", "pl"))
    with pytest.raises(UnsupErr, match="does not directly follow a convolution"):
        _dry(NHWC, net(lone_affine))
    def three(p):
        p.add(PipeOp("b", "Convolution", "data", "b", out_chans=32, kern_sz=(1, 1))); p.add(PipeOp("c", "Convolution", "data", "c", out_chans=32, kern_sz=(1, 1)))
        p.add(PipeOp("s", "Eltwise", "a", "s", bots=("a", "b", "c")))
    with pytest.raises(UnsupErr, match="sums 3 nodes"):
        _dry(NHWC, net(three))
    _dry(None, net(three))     # (fp32: hip_reduce takes up to eight)


# ---- the flagged function: args, plans, refusals
def _anno(B=2, C=64, HW=14, OC=64, k=1, pad=0, **kw):
    return add_codegen_annotations(rr.conv_op(B, C, HW, OC, k, pad), OpTune(hip_dtype="bf16", hip_layout="nhwc", **kw))


def test_fuse_residual_adds_res_in_front_of_out_and_only_res_to_the_plan():
    a = _anno()
    plain_args, plain_plan = pipe_func_args(a), rtc_mod.explain_plan(a)
    assert plain_args == NATIVE_ARGS["hip_conv_nhwc"] and "RES" not in plain_plan
    f = a.copy(); nhwc.fuse_residual(f)
    assert pipe_func_args(f) == NATIVE_ARGS["hip_conv_nhwc"][:-1] + (("res", "IN"), ("out", "OUT"))
    assert f.get_u32("nhwc_residual") == 1 and f.get_dims("res") == f.get_dims("out") and not a.has("nhwc_residual")
    assert rtc_mod.explain_plan(f) == plain_plan + " -DRES=1" and rtc_mod.explain_plan(a) == plain_plan
    fo = _anno(hip_out="f32"); nhwc.fuse_residual(fo)
    assert fo.get_dims("res").tn == "float" and rtc_mod.explain_plan(fo).endswith("-DOUT_F32=1 -DNBUF=4 -DRES=1")
    ks = rr.res_func_op("ksl4_2x512x7x64", False, 1)
    assert rtc_mod.explain_plan(ks).endswith("-DKSL=4 -DRES=1")


def test_fuse_residual_refusals(monkeypatch):
    with pytest.raises(UnsupErr, match="input-patch"):                       # the patch kernel (3x3) ...
        nhwc.fuse_residual(_anno(k=3, pad=1))
    stem = add_codegen_annotations(parse_op("(str_vals=(type=Convolution),nda_vals=(biases=(dims=(out_chan=64)),filts=(dims=(out_chan=64,in_chan=3,y=7,x=7)),in=(dims=(img=2,chan=3,y=64,x=64)),"
                                            "in_pad=(tn=none,dims=(y=3,x=3)),kern_sz=(tn=none,dims=(y=7,x=7)),out=(dims=(img=2,chan=64,y=32,x=32)),out_chans=(tn=uint32_t,v=64),stride=(tn=none,dims=(y=2,x=2))))"), NHWC)
    with pytest.raises(UnsupErr, match="rolling-rows"):                      # ... which is also the form that binds the rolling-rows kernel
        nhwc.fuse_residual(stem)
    p = _anno(); nhwc.fuse_pool(p, p.get_dims("in_ref"), (3, 3), (1, 1))
    with pytest.raises(UnsupErr, match="POOL"):
        nhwc.fuse_residual(p)
    f = _anno(); nhwc.fuse_residual(f)
    with pytest.raises(UnsupErr, match="already"):
        nhwc.fuse_residual(f)
    with pytest.raises(UnsupErr, match="not a plain"):
        nhwc.fuse_residual(add_codegen_annotations(rr.conv_op(2, 64, 14, 64), OpTune()))
    # sibling groups, sets and multi-problem launches refuse a flagged member (they would drop the flag), and say so
    g = _anno(OC=32)
    with pytest.raises(UnsupErr, match="nhwc_residual"):
        nhwc.annotate_group([f, g])
    with pytest.raises(UnsupErr, match="nhwc_residual"):
        nhwc.annotate_set([g, f])
    with pytest.raises(UnsupErr, match="nhwc_residual"):
        nhwc.annotate_multi([g, f])
    assert not nhwc.set_eligible(f) and not nhwc.multi_eligible(f) and nhwc.set_eligible(g) and nhwc.multi_eligible(g)
    # the native side: a patch-form function with the flag set by hand, the flag on another function, a missing or wrong res, the two-kernel form of the K slices
    h = _anno(k=3, pad=1); h.set_u32("nhwc_residual", 1); h.nda_vals["res"] = h.nda_vals["out"]
    with pytest.raises(UnsupErr, match="input-patch and rolling-rows"):
        rtc_mod.explain_plan(h)
    gg = nhwc.annotate_group([g, _anno(OC=16)]); gg.set_u32("nhwc_residual", 1)
    with pytest.raises(UnsupErr, match="only a plain hip_conv_nhwc"):
        rtc_mod.explain_plan(gg)
    m = f.copy(); del m.nda_vals["res"]
    with pytest.raises(RtErr, match="without the arg 'res'"):
        rtc_mod.explain_plan(m)
    w = f.copy(); w.nda_vals["res"] = _anno(OC=32).nda_vals["out"]
    with pytest.raises(RtErr, match="differ from out's"):
        rtc_mod.explain_plan(w)
    t = f.copy(); t.nda_vals["res"] = _anno(hip_out="f32").nda_vals["out"]
    with pytest.raises(RtErr, match="differ from out's"):
        rtc_mod.explain_plan(t)
    ks = rr.res_func_op("ksl4_2x512x7x64", False, 1)
    monkeypatch.setenv("BODAHIP_NHWC_SPLITK2", "1")
    with pytest.raises(UnsupErr, match="two-kernel form"):
        rtc_mod.explain_plan(ks)
