"""The training BatchNorm of the gradient pipe without a GPU: the five native functions on be=cpu bit for bit against the numpy twin of their
written formulas and of the chain of their sums (tests/bn_ref.py), their refusals, add_bck_ops on a hand-built residual pipe and on ResNet-50, and ConvPipeBck on be=cpu
against a float64 walk, with a solver, and with its call list run in other topological orders.

The float64 comparison uses the existing cap 5e-4 on max|got - want| / max|want| per node (tests/test_bck_pipe_cpu.py).  The largest value measured on be=cpu over the
three seeds is printed (run with -s) and recorded as DRIVER_DEV_CPU; both backends are then held to ten times that as well.
Seeds: the float64 walk's guard (no ReLU input within 1e-4 max|v| of zero) is a condition, not a tolerance.  With some 17 000 ReLU inputs in the residual pipe it holds
for about one seed in 3 000; 2477, 8679 and 9116 are the first three of 0 .. 9116 for which the float64 walk ALONE passes it (bn_ref.RES_SEEDS).
The biases of a convolution in front of a BatchNorm have the exact gradient 0 (the BatchNorm subtracts the mean again): what the pipe leaves there is rounding noise, so
those nodes are held to |got| <= 5e-4 * max over channels of SUM |X_grad_loss| instead of to a quotient whose divisor is 1e-17."""
import numpy as np
import pytest

import bck_pipe_ref as ref
import bn_ref as R
from boda_amd import rtc as rtc_mod
from boda_amd.bck_pipe import BN_IN_SFX, SGD_HIST_SFX, ConvPipeBck, SgdSolver, add_bck_ops, bn_stat_params, host_params
from boda_amd.cnn_op import (BN_OP_FUNCS, NATIVE_ARGS, PIPE_OP_FUNCS, bn_bck_in_func_op, bn_bck_sums_func_op, bn_fwd_func_op, bn_stats_func_op, fan_out_func_op,
                             pipe_func_args)
from boda_amd.conv_pipe import ConvPipe, PipeOp, resnet50
from boda_amd.op import Dims, Nda, RtErr, UnsupErr, parse_op
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc

from sgd_ref import sgd_np
from test_bck_graph_cpu import run_in_order, topo_order

CAP = 5e-4
DRIVER_DEV_CPU = R.DRIVER_DEV_CPU


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


# ---- the functions against the numpy twin
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_cpu_functions_against_numpy(cpu, case):
    shape, slab = case
    relu = (shape[0] + shape[1]) % 2
    r = R.run_all_five(cpu, shape, slab, relu=relu)
    R.check_against_numpy(r, shape, slab, relu=relu)
    if shape == (1, 1, 1, 1):   # N = 1: var = 0, the N == 1 branch (no multiply by N / (N - 1))
        i = R.make_inputs(shape)
        assert r["mean"][0] == i["x"].reshape(-1)[0] and r["inv_std"][0] == R.F(1) / np.sqrt(R.F(R.EPS))
        assert R.same_bits(r["run_var2"], R.F(R.MAF) * i["run_var"] + (R.F(1) - R.F(R.MAF)) * R.F(0))
    C = shape[1]
    if C > 1:     # the channel of constants: a variance of exactly 0 or rounding noise, never negative, and a finite inv_std
        assert np.all(np.isfinite(r["inv_std"])) and r["inv_std"][C - 1] > 100


def test_forced_slabs_cut_where_they_say():
    d = R.dims_of((2, 3, 57, 57))
    plan = rtc_mod.explain_plan(bn_stats_func_op(d, R.EPS, R.MAF, 2000))
    assert plan.endswith("slab=2000 slabs=4"), plan
    n_slabs = int(plan.rsplit("slabs=", 1)[1])
    assert n_slabs >= 3 and 2000 * (n_slabs - 1) < 2 * 57 * 57 < 2000 * n_slabs and 2000 < 57 * 57 < 4000   # ragged last slab, an edge inside a plane, a slab across images
    assert R.slab_plan(3, 2 * 57 * 57, 2000) == (2000, 4) and R.slab_plan(3, 2 * 57 * 57) == (4096, 2)
    # the planner: two workgroups per CU on 256 CUs where C * N allows it, one slab where a channel is short -- and nothing of it depends on a device
    assert rtc_mod.explain_plan(bn_stats_func_op(R.dims_of((64, 64, 112, 112)), R.EPS, R.MAF)).endswith("slab=100352 slabs=8")
    assert rtc_mod.explain_plan(bn_bck_sums_func_op(R.dims_of((64, 2048, 7, 7)))).endswith("slab=4096 slabs=1")
    assert R.slab_plan(64, 64 * 112 * 112) == (100352, 8) and R.slab_plan(2048, 64 * 49) == (4096, 1)
    for C, N in ((64, 802816), (256, 200704), (512, 50176), (1024, 12544), (1, 5000), (3, 6498)):
        slab, n = R.slab_plan(C, N)
        assert rtc_mod.explain_plan(bn_bck_sums_func_op(Dims.make("float", img=1, chan=C, y=1, x=N))).endswith(f"slab={slab} slabs={n}")


@pytest.mark.parametrize("n", [2, 3, 8])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cpu_fan_out(cpu, shape, n):
    x = R.make_inputs(shape)["x"]
    x.reshape(-1)[0] = -0.0
    out = R.run_func(cpu, fan_out_func_op(R.dims_of(shape), n), {"in": x})[0]
    assert sorted(out) == sorted(f"outs_{i}" for i in range(n))
    for a in out.values():
        assert R.same_bits(a, x)


def test_cpu_running_pair_after_two_calls(cpu):
    shape = (3, 5, 3, 3)
    i = R.make_inputs(shape)
    got = R.run_func(cpu, bn_stats_func_op(R.dims_of(shape), R.EPS, R.MAF), {"in": i["x"], "run_mean": i["run_mean"], "run_var": i["run_var"]}, repeat=2)
    m1, s1, rm1, rv1 = R.stats_np(i["x"], i["run_mean"], i["run_var"])
    m2, s2, rm2, rv2 = R.stats_np(i["x"], rm1, rv1)
    assert R.same_bits(got[0]["run_mean"], rm1) and R.same_bits(got[0]["run_var"], rv1)
    assert R.same_bits(got[1]["run_mean"], rm2) and R.same_bits(got[1]["run_var"], rv2) and not R.same_bits(rm1, rm2)
    assert R.same_bits(got[1]["mean"], m1) and R.same_bits(got[1]["inv_std"], s1)


def test_cpu_in_place_forms(cpu):
    """hip_bn_fwd with out on in's var and hip_bn_bck_in with in_grad_loss on out_grad_loss's var leave the bits of the two-var forms."""
    shape = (3, 2, 7, 7)
    d = R.dims_of(shape)
    r = R.run_all_five(cpu, shape)
    common = {"in": r["x"], "mean": r["mean"], "inv_std": r["inv_std"]}
    out = R.run_func(cpu, bn_fwd_func_op(d, 1), dict(common, scale=r["scale"], bias=r["bias"]), bind={"out": "in"})[0]["out"]
    assert R.same_bits(out, r["out"])
    dx = R.run_func(cpu, bn_bck_in_func_op(d), dict(common, scale=r["scale"], scale_grad_loss=r["sg"], bias_grad_loss=r["bg"], out_grad_loss=r["dy"]),
                    bind={"in_grad_loss": "out_grad_loss"})[0]["in_grad_loss"]
    assert R.same_bits(dx, r["dx"])


@pytest.mark.parametrize("case", [c for c in R.CASES if c[0][0] * c[0][2] * c[0][3] >= 8], ids=R.case_id)
def test_cpu_float64_bounds(cpu, case):
    """The per-element bounds of bn_ref.f64_bounds_fractions (derived there, one u per written operation, not tuned).  Shapes with fewer than 8 elements per channel are
    held bit for bit only: at N = 2 dx is a cancellation.  Largest fractions observed on these cases: out 0.88, dx 0.96, scale_grad 0.011, bias_grad 0.017, S1 0.040."""
    shape, slab = case
    r = R.run_all_five(cpu, shape, slab, relu=0)
    fr = R.f64_bounds_fractions(r, shape, relu=0)
    print(R.case_id(case), {k: round(v, 4) for k, v in fr.items()})
    for k, v in fr.items():
        assert v <= 1.0, (k, v)


# ---- tables, arg lists, plans
def test_tables_arg_lists_and_plans():
    assert BN_OP_FUNCS == {"BnStats": ("hip_bn_stats",), "BnFwd": ("hip_bn_fwd",), "BnBckSums": ("hip_bn_bck_sums",), "BnBckIn": ("hip_bn_bck_in",), "FanOut": ("hip_fan_out",)}
    assert not set(BN_OP_FUNCS) & set(PIPE_OP_FUNCS)
    d = R.dims_of((2, 3, 4, 4))
    fs = bn_stats_func_op(d, 1e-5, 0.999)
    assert fs.get_func_name() == "hip_bn_stats" and fs.get_type() == "BnStats" and fs.get_u32("slab") == 0 and fs.get_f32("maf") == float(np.float32(0.999))
    assert pipe_func_args(fs) == NATIVE_ARGS["hip_bn_stats"] == (("in", "IN"), ("mean", "OUT"), ("inv_std", "OUT"), ("run_mean", "INOUT"), ("run_var", "INOUT"))
    assert pipe_func_args(bn_fwd_func_op(d, 1)) == (("in", "IN"), ("mean", "IN"), ("inv_std", "IN"), ("scale", "IN"), ("bias", "IN"), ("out", "OUT"))
    assert pipe_func_args(bn_bck_sums_func_op(d)) == (("in", "IN"), ("mean", "IN"), ("inv_std", "IN"), ("out_grad_loss", "IN"), ("scale_grad_loss", "OUT"), ("bias_grad_loss", "OUT"))
    assert pipe_func_args(bn_bck_in_func_op(d)) == (("in", "IN"), ("mean", "IN"), ("inv_std", "IN"), ("scale", "IN"), ("scale_grad_loss", "IN"), ("bias_grad_loss", "IN"),
                                                    ("out_grad_loss", "IN"), ("in_grad_loss", "OUT"))
    assert pipe_func_args(fan_out_func_op(d, 3)) == (("in", "IN"), ("outs_0", "OUT"), ("outs_1", "OUT"), ("outs_2", "OUT"))
    assert fs.get_dims("mean") == Dims(("chan",), (3,), "float")
    for f in (fs, bn_fwd_func_op(d, 0), bn_bck_sums_func_op(d, 8), bn_bck_in_func_op(d), fan_out_func_op(d, 8)):
        assert parse_op(f.to_str()).to_str() == f.to_str() and rtc_mod.parse_op_native(f.to_str()) == f.to_str()
        assert f.flops() == 0 and rtc_mod.prebuild(f) > 0      # cross-compiles for gfx950
    assert fs.algo_bytes() == 4 * (96 + 4 * 3) and fan_out_func_op(d, 3).algo_bytes() == 4 * 96 * 4
    assert rtc_mod.explain_plan(fs) == "bodahip_bn_sum grid=3 block=256 -DMODE=0 | bodahip_bn_sum grid=3 block=256 -DMODE=1 | bodahip_bn_fin grid=1 block=256 -DFIN=1 | slab=4096 slabs=1"
    assert rtc_mod.explain_plan(bn_bck_sums_func_op(d, 8)) == "bodahip_bn_sum grid=12 block=256 -DMODE=2 | bodahip_bn_fin grid=1 block=256 -DFIN=2 | slab=8 slabs=4"
    assert rtc_mod.explain_plan(bn_fwd_func_op(d, 1)) == "bodahip_bn_fwd -DRELU=1" and rtc_mod.explain_plan(bn_bck_in_func_op(d)) == "bodahip_bn_bck_in"
    assert rtc_mod.explain_plan(fan_out_func_op(d, 5)) == "bodahip_fan_out -DNOUT=5"


def fixture_ops(rtc):
    """The function ops the GPU tests run (tests/golden/ops/bn-ops.txt: what build() pre-specialises): the function matrix, and every function op of the residual
    pipe's step with a solver (its convolutions and their gradients included)."""
    ops = []
    for shape, slab in R.CASES:
        d = R.dims_of(shape)
        ops += [bn_stats_func_op(d, R.EPS, R.MAF, slab), bn_fwd_func_op(d, 0), bn_fwd_func_op(d, 1), bn_bck_sums_func_op(d, slab), bn_bck_in_func_op(d)]
    ops += [fan_out_func_op(R.dims_of((3, 5, 3, 3)), n) for n in range(2, 9)]
    cp = R.residual()
    drv = ConvPipeBck(rtc, solver=SgdSolver(lr=0.05, momentum=0.9, weight_decay=5e-4, lr_mult={"biases": 2.0, "scale": 0.5}, decay_mult={"biases": 0.0, "bias": 0.0}), bn_maf=0.9)
    drv.init(add_bck_ops(cp), R.res_params(cp, 1))
    ops += [f for _, f, _ in drv.calls()]
    drv.release()
    seen, out = set(), []
    for o in ops:
        if o.to_str() not in seen:
            seen.add(o.to_str()); out.append(o)
    return out


def test_fixture_file_lists_these_ops(cpu):
    import os
    from boda_amd.op import read_ops
    ops = read_ops(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops", "bn-ops.txt"))
    assert [o.to_str() for o in ops] == [o.to_str() for o in fixture_ops(cpu)]
    for o in ops:
        assert rtc_mod.explain_plan(o)


# ---- refusals
def bad_op(f, **nda):
    b = f.copy()
    for k, v in nda.items():
        if v is None:
            b.nda_vals.pop(k)
        else:
            b.nda_vals[k] = v
    return b


def compile_only(rtc, f):
    rtc.compile([RtcFuncInfo("bn_bad", "", [a for a, _ in NATIVE_ARGS[f.get_func_name()]], f)])
    rtc.release_func("bn_bad")


def test_refusals_of_the_op(cpu):
    d = R.dims_of((2, 3, 4, 4))
    u32 = lambda v: Nda(None, "uint32_t", (v,))
    other = Nda(dims=R.dims_of((2, 3, 4, 5)), tn="float")
    with pytest.raises(UnsupErr, match="2 to 8 outputs"):
        fan_out_func_op(d, 1)
    with pytest.raises(UnsupErr, match="2 to 8 outputs"):
        fan_out_func_op(d, 9)
    with pytest.raises(RtErr, match="multiple of 4"):
        bn_stats_func_op(d, 1e-5, 0.9, 6)
    with pytest.raises(RtErr, match="img:chan:y:x"):
        bn_fwd_func_op(Dims.make("float", img=2, chan=3, x=4), 0)
    with pytest.raises(RtErr, match="relu must be 0 . 1"):
        bn_fwd_func_op(d, 2)
    cases = [
        (bad_op(bn_fwd_func_op(d, 0), out=other), RtErr, "out dims .* differ from in's"),                                   # wrong dims of a tensor arg
        (bad_op(bn_bck_in_func_op(d), in_grad_loss=Nda(dims=Dims(d.names, d.sizes, "half"), tn="half")), RtErr, "differ from in's"),   # wrong type of one
        (bad_op(bn_stats_func_op(d, 1e-5, 0.9), **{"in": Nda(dims=Dims(d.names, d.sizes, "half"), tn="half")}), RtErr, "fp32 only"),
        (bad_op(bn_stats_func_op(d, 1e-5, 0.9), mean=Nda(dims=Dims(("chan",), (4,), "float"), tn="float")), RtErr, "mean dims .*one float per channel"),   # a per-channel arg of another length
        (bad_op(bn_bck_sums_func_op(d), bias_grad_loss=Nda(dims=Dims(("v",), (3,), "float"), tn="float")), RtErr, "bias_grad_loss dims .*one float per channel"),
        (bad_op(fan_out_func_op(d, 2), outs_num=u32(9)), UnsupErr, "outs_num=9: 2 to 8 outputs"),
        (bad_op(fan_out_func_op(d, 2), outs_num=u32(1)), UnsupErr, "outs_num=1: 2 to 8 outputs"),
        (bad_op(fan_out_func_op(d, 2), outs_1=other), RtErr, "outs_1 dims .* differ from in's"),
        (bad_op(bn_stats_func_op(d, 1e-5, 0.9), slab=u32(6)), RtErr, "slab=6: a forced slab length is a multiple of 4"),
        (bad_op(bn_stats_func_op(d, 1e-5, 0.9), maf=None), RtErr, "no 'maf'"),
        (bad_op(bn_fwd_func_op(d, 0), relu=u32(2)), RtErr, "relu must be 0 . 1"),
        (bad_op(bn_fwd_func_op(d, 0), scale=None), RtErr, "no 'scale'"),
    ]
    for fl in ("img_shards", "seed_from_var", "zero_if_in_non_pos"):
        for f in (bn_stats_func_op(d, 1e-5, 0.9), bn_fwd_func_op(d, 0), bn_bck_sums_func_op(d), bn_bck_in_func_op(d), fan_out_func_op(d, 2)):
            cases.append((bad_op(f, **{fl: u32(1)}), RtErr, f"{fl}=1 on '{f.get_func_name()}'"))
    for f, err, msg in cases:
        with pytest.raises(err, match=msg):
            compile_only(cpu, f)
        if "=1 on " not in msg or "zero_if_in_non_pos" not in msg:    # (the planner reads zero_if_in_non_pos through a check of its own, which words it differently)
            with pytest.raises(err, match=msg):
                rtc_mod.explain_plan(f)
    wrong_type = bn_fwd_func_op(d, 0); wrong_type.str_vals["type"] = "BnStats"
    with pytest.raises(RtErr, match="a function of op type BnFwd, not BnStats"):
        compile_only(cpu, wrong_type)
    big = Dims.make("float", img=8, chan=1024, y=256, x=256)     # 2 GiB exactly
    for f in (lambda: bn_stats_func_op(big, 1e-5, 0.9), lambda: bn_fwd_func_op(big, 0), lambda: bn_bck_sums_func_op(big), lambda: bn_bck_in_func_op(big), lambda: fan_out_func_op(big, 2)):
        with pytest.raises(UnsupErr, match="2 GiB"):
            rtc_mod.explain_plan(f())
        with pytest.raises(UnsupErr, match="2 GiB"):
            compile_only(cpu, f())


def run_bound(rtc, f, bind, dims=None):
    """Run f with arg -> var name from `bind` (vars made here: one per distinct name, of the arg's op dims or dims[name])."""
    spec = pipe_func_args(f)
    rtc.compile([RtcFuncInfo("bn_r", "", [a for a, _ in spec], f)])
    made = []
    try:
        for an, _ in spec:
            vn = bind.get(an, "rv_" + an)
            if vn not in made:
                rtc.create_var_with_dims(vn, (dims or {}).get(vn, f.get_dims(an))); made.append(vn)
        rtc.run(RtcFuncCall("bn_r", {an: RtcArg.var(bind.get(an, "rv_" + an)) for an, _ in spec}))
        rtc.finish_and_sync()
    finally:
        for vn in made:
            rtc.release_var(vn)
        rtc.release_func("bn_r"); rtc.release_per_call_id_data()


def var_refusals(rtc):
    d = R.dims_of((2, 3, 4, 4))
    ch4 = Dims(("chan",), (4,), "float")
    with pytest.raises(RtErr, match="args 'mean' and 'inv_std' are the same var"):            # hip_bn_stats outputs aliased
        run_bound(rtc, bn_stats_func_op(d, 1e-5, 0.9), {"inv_std": "rv_mean"})
    with pytest.raises(RtErr, match="args 'mean' and 'run_mean' are the same var"):
        run_bound(rtc, bn_stats_func_op(d, 1e-5, 0.9), {"run_mean": "rv_mean"})
    with pytest.raises(RtErr, match="args 'run_mean' and 'run_var' are the same var"):
        run_bound(rtc, bn_stats_func_op(d, 1e-5, 0.9), {"run_var": "rv_run_mean"})
    with pytest.raises(RtErr, match="args 'in' and 'outs_1' are the same var"):                # outs_i aliased to in ...
        run_bound(rtc, fan_out_func_op(d, 3), {"outs_1": "rv_in"})
    with pytest.raises(RtErr, match="args 'outs_0' and 'outs_2' are the same var"):            # ... or to each other
        run_bound(rtc, fan_out_func_op(d, 3), {"outs_2": "rv_outs_0"})
    with pytest.raises(RtErr, match="args 'scale_grad_loss' and 'bias_grad_loss' are the same var"):
        run_bound(rtc, bn_bck_sums_func_op(d), {"bias_grad_loss": "rv_scale_grad_loss"})
    with pytest.raises(RtErr, match="args 'in' and 'in_grad_loss' are the same var"):
        run_bound(rtc, bn_bck_in_func_op(d), {"in_grad_loss": "rv_in"})
    with pytest.raises(RtErr, match="arg 'scale' has dims .*chan=4.*the op says"):             # a per-channel var whose length is not chan
        run_bound(rtc, bn_fwd_func_op(d, 0), {"scale": "short"}, {"short": ch4})
    with pytest.raises(RtErr, match="arg 'out' has dims .*the op says"):                       # wrong dims of a var
        run_bound(rtc, bn_fwd_func_op(d, 0), {"out": "other"}, {"other": R.dims_of((2, 3, 4, 5))})
    with pytest.raises(RtErr, match="arg 'in' has dims .*img=1.*the op says"):                 # no img shards: the sums run over the whole batch
        run_bound(rtc, bn_stats_func_op(d, 1e-5, 0.9), {"in": "shard"}, {"shard": R.dims_of((1, 3, 4, 4))})
    with pytest.raises(RtErr, match="has type uint32_t: fp32 only"):
        run_bound(rtc, bn_stats_func_op(d, 1e-5, 0.9), {"mean": "words"}, {"words": Dims(("chan",), (3,), "uint32_t")})
    run_bound(rtc, bn_fwd_func_op(d, 1), {"out": "rv_in"})                                      # the two allowed in-place forms
    run_bound(rtc, bn_bck_in_func_op(d), {"in_grad_loss": "rv_out_grad_loss"})


def test_cpu_refusals_of_the_call(cpu):
    var_refusals(cpu)


# ---- add_bck_ops
def run_group(tag, bot, in_gl, relu=True, x_gl=None):
    """The gradient ops of conv `tag` + BatchNorm + Scale (+ ReLU), in run order: ZeroIfNonPos, BckScale, BckBatchNorm, BckConv."""
    gl = tag + "_grad_loss"
    out = [(tag + "_relu_bck", "ZeroIfNonPos", [gl, tag], [gl])] if relu else []
    return out + [
        ("scale_" + tag + "_bck", "BckScale", [gl, tag, f"scale_{tag}_scale"], [gl, f"scale_{tag}_scale_grad_loss", f"scale_{tag}_bias_grad_loss"]),
        ("bn_" + tag + "_bck", "BckBatchNorm", [gl, tag], [gl]),
        (tag + "_bck", "BckConv", [bot, tag + "_filts", tag + "_biases", gl], [in_gl, tag + "_filts_grad_loss", tag + "_biases_grad_loss"]),
    ]


def test_add_bck_ops_residual_pipe():
    bp = add_bck_ops(R.residual())
    ra = [f"res_a_res_a_relu_0_split_{i}_grad_loss" for i in range(2)]     # the identity shortcut: res_a is read by b_2a and by the Eltwise res_b
    st = [f"stem_stem_relu_0_split_{i}_grad_loss" for i in range(2)]       # stem is read by the projection a_b1 and by a_2a
    want = [
        ("fc_bck", "BckConv", ["gap", "fc_filts", "fc_biases", "fc_grad_loss"], ["gap_grad_loss", "fc_filts_grad_loss", "fc_biases_grad_loss"]),
        ("gap_bck", "Spreading", ["gap", "gap_grad_loss", "res_b"], ["res_b_grad_loss"]),
        ("res_b_relu_bck", "ZeroIfNonPos", ["res_b_grad_loss", "res_b"], ["res_b_grad_loss"]),
        ("res_b_bck", "BckEltwise", ["res_b_grad_loss"], [ra[1], "b_2c_grad_loss"]),
    ]
    want += run_group("b_2c", "b_2b", "b_2b_grad_loss", relu=False) + run_group("b_2b", "b_2a", "b_2a_grad_loss") + run_group("b_2a", "res_a", ra[0])
    want += [("reduce_res_a_grad_loss", "Reduce", ra, ["res_a_grad_loss"]),
             ("res_a_relu_bck", "ZeroIfNonPos", ["res_a_grad_loss", "res_a"], ["res_a_grad_loss"]),
             ("res_a_bck", "BckEltwise", ["res_a_grad_loss"], ["a_b1_grad_loss", "a_2c_grad_loss"])]
    want += run_group("a_2c", "a_2b", "a_2b_grad_loss", relu=False) + run_group("a_2b", "a_2a", "a_2a_grad_loss") + run_group("a_2a", "stem", st[1])
    want += run_group("a_b1", "stem", st[0], relu=False)
    want += [("reduce_stem_grad_loss", "Reduce", st, ["stem_grad_loss"])] + run_group("stem", "data", "data_grad_loss")
    assert [(o.tag, o.type, o.bots, o.tops) for o in bp.bck_ops()] == want
    fwd = {o.tag: o for o in bp.fwd_ops()}
    assert (fwd["bn_stem"].type, fwd["bn_stem"].bots, fwd["bn_stem"].tops, fwd["bn_stem"].in_place) == ("BatchNorm", ["stem", "bn_stem_mean", "bn_stem_var"], ["stem"], True)
    assert (fwd["scale_stem"].bots, fwd["scale_stem"].in_place) == (["stem", "scale_stem_scale", "scale_stem_bias"], True)
    assert (fwd["res_a"].type, fwd["res_a"].bots, fwd["res_a"].tops, fwd["res_a"].in_place) == ("Eltwise", ["a_b1", "a_2c"], ["res_a"], False)
    assert bp.nodes["scale_stem_scale_grad_loss"] == bp.cp.params["scale_stem_scale"] and bp.nodes[ra[1]] == bp.nodes["res_a"]
    assert not any(n.startswith("bn_") and n.endswith("_grad_loss") for n in bp.nodes)     # _mean / _var get no gradient node


def test_in_place_order_of_every_other_node_is_unchanged():
    """[ReLU, Dropout] on one node keep today's order (the gradient ops run in FORWARD order there, harmless because they commute); only a node with a BatchNorm / Scale
    among its in-place ops runs them in true reverse."""
    p = ConvPipe("rd", "data", Dims.make("float", img=2, chan=3, y=5, x=5))
    p.add(PipeOp("c", "Convolution", "data", "c", out_chans=4, kern_sz=(3, 3))); p.add(PipeOp("r", "ReLU", "c", "c")); p.add(PipeOp("d", "Dropout", "c", "c"))
    p.add(PipeOp("fc", "Convolution", "c", "fc", out_chans=5, kern_sz=(0, 0)))
    assert [o.tag for o in add_bck_ops(p).bck_ops()] == ["fc_bck", "r_bck", "d_bck", "c_bck"]


def test_add_bck_ops_resnet50_structure():
    cp = resnet50(2, 32)
    bp = add_bck_ops(cp)
    from collections import Counter
    n = Counter(o.type for o in bp.bck_ops())
    assert (n["BckBatchNorm"], n["BckScale"], n["BckEltwise"], n["BckConv"]) == (53, 53, 16, 54)
    readers = Counter(b for o in cp.ops if not o.in_place for b in (o.bots or (o.bot,)))
    multi = [x for x, k in readers.items() if k > 1]
    assert len(multi) == 16 and sorted(o.tops[0] for o in bp.bck_ops() if o.type == "Reduce") == sorted(x + "_grad_loss" for x in multi)
    written = set(cp.nodes) | set(cp.params) | {"label"}
    for o in bp.ops:
        for b in o.bots:
            assert b in written, (o.tag, b)
        written.update(o.tops)
    stats = set(bn_stat_params(cp))
    assert len(stats) == 106
    for pn in cp.params:
        assert (pn + "_grad_loss" in bp.nodes) == (pn not in stats), pn
    tags = [o.tag for o in bp.bck_ops()]
    for o in cp.ops:     # ZeroIfNonPos, BckScale, BckBatchNorm, then the convolution's gradient
        if o.type == "BatchNorm":
            i = tags.index(o.tag + "_bck")
            assert bp.bck_ops()[i - 1].type == "BckScale" and bp.bck_ops()[i + 1].type == "BckConv" and bp.bck_ops()[i + 1].bots[3] == o.bot + "_grad_loss"
            if o.bot + "_relu_bck" in tags:
                assert tags.index(o.bot + "_relu_bck") == i - 2


# ---- the driver on be=cpu
def res_step(rtc, seed, **kw):
    cp = R.residual(); bp = add_bck_ops(cp)
    params = R.res_params(cp, seed); data, label = R.res_inputs(cp, seed)
    drv = ConvPipeBck(rtc, bn_maf=0.9, **kw); drv.init(bp, params)
    fwd = {"data": data, "label": label}
    gets = [n for n in bp.nodes if n.endswith("_grad_loss")] + ["loss"] + [o.tag + s for o in cp.ops if o.type == "BatchNorm" for s in ("_batch_mean", "_batch_inv_std", "_mean", "_var")]
    drv.run_bck(["data", "label"], fwd, gets)
    return drv, bp, params, data, label, fwd


def check_against_f64(bp, params, data, label, fwd, where, bound):
    """-> the largest quotient seen."""
    cp = bp.cp
    want = R.net_bn_f64(cp, params, data, label)
    zero_biases = {o.bot + "_biases_grad_loss": o.bot for o in cp.ops if o.type == "BatchNorm"}     # exact gradient 0: see the module docstring
    worst, checked = 0.0, 0
    for n in [n for n in bp.nodes if n.endswith("_grad_loss")] + ["loss"]:
        if "_split_" in n:
            continue
        got = fwd[n]
        assert got.shape == tuple(bp.nodes[n].sizes) and np.all(np.isfinite(got)), n
        if n in zero_biases:
            assert np.max(np.abs(want[n])) < 1e-12
            err = float(np.max(np.abs(got)) / np.max(np.abs(want[zero_biases[n] + "_grad_loss"]).sum(axis=(0, 2, 3))))
        elif n == "loss":
            err = abs(got.item() - want[n]) / abs(want[n])
        else:
            err = ref.rel_err(got, want[n])
        assert err <= bound, (where, n, err)
        worst = max(worst, err); checked += 1
    assert checked >= len(cp.params) - 20 + 10
    for o in cp.ops:     # the batch statistics themselves, and the running pair moved by them (maf = 0.9)
        if o.type == "BatchNorm":
            m, v = want[o.tag + "_batch_mean"], want[o.tag + "_batch_var"]
            N = data.shape[0] * cp.nodes[o.bot].dsz("y") * cp.nodes[o.bot].dsz("x")
            assert ref.rel_err(fwd[o.tag + "_batch_mean"], m) <= bound + 1e-6 / max(np.max(np.abs(m)), 1e-30) and ref.rel_err(fwd[o.tag + "_batch_inv_std"], 1 / np.sqrt(v + 1e-5)) <= bound
            assert ref.rel_err(fwd[o.tag + "_mean"], 0.9 * params[o.tag + "_mean"].astype(np.float64) + 0.1 * m) <= 1e-5
            assert ref.rel_err(fwd[o.tag + "_var"], 0.9 * params[o.tag + "_var"].astype(np.float64) + 0.1 * v * N / (N - 1)) <= 1e-5
    return worst


@pytest.mark.parametrize("seed", R.RES_SEEDS)
def test_cpu_driver_against_float64(cpu, seed):
    drv, bp, params, data, label, fwd = res_step(cpu, seed)
    try:
        fns = [f.get_func_name() for _, f, _ in drv.calls()]
        assert (fns.count("hip_bn_stats"), fns.count("hip_bn_fwd"), fns.count("hip_bn_bck_sums"), fns.count("hip_bn_bck_in"), fns.count("hip_fan_out")) == (8, 8, 8, 8, 2)
        assert fns.count("hip_reduce") == 2 + 2 and "hip_chan_affine" not in fns       # two Eltwise sums, two fan-outs' Reduce
        by_tag = {t: (f, am) for t, f, am in drv.calls()}
        f, am = by_tag["stem"]
        assert f.get_u32("conv_has_relu") == 0 and am["out"].n == "stem" + BN_IN_SFX       # the convolution writes the side var
        assert by_tag["scale_stem"][0].get_u32("relu") == 1 and by_tag["scale_a_2c"][0].get_u32("relu") == 0 and "stem_relu" not in by_tag
        assert by_tag["bn_stem_bck"][1]["in_grad_loss"].n == by_tag["bn_stem_bck"][1]["out_grad_loss"].n == "stem_grad_loss"
        worst = check_against_f64(bp, params, data, label, fwd, "be=cpu", CAP)
        print(f"be=cpu residual seed {seed}: largest max|got - want| / max|want| = {worst:.3e}")
        assert worst <= 10 * DRIVER_DEV_CPU
    finally:
        drv.release()


def test_float64_batchnorm_gradient_against_central_differences():
    """So that a wrong formula cannot be consistently wrong on both sides: the float64 walk's data gradient (through eight training BatchNorms) against central
    differences of the float64 loss on a dozen input elements."""
    seed = R.RES_SEEDS[0]
    cp = R.residual()
    params = R.res_params(cp, seed); data, label = R.res_inputs(cp, seed)
    g = R.net_bn_f64(cp, params, data, label)["data_grad_loss"]
    rng = np.random.default_rng(5)
    h = 1e-6
    for ix in rng.choice(data.size, 12, replace=False):
        d = data.astype(np.float64).reshape(-1).copy()
        d[ix] += h; up = R.net_bn_f64(cp, params, d.reshape(data.shape), label, guard_rel=0.0, only_loss=True)["loss"]
        d[ix] -= 2 * h; dn = R.net_bn_f64(cp, params, d.reshape(data.shape), label, guard_rel=0.0, only_loss=True)["loss"]
        num = (up - dn) / (2 * h)
        assert abs(num - g.reshape(-1)[ix]) <= 1e-6 * np.max(np.abs(g)) + 1e-9, (ix, num, g.reshape(-1)[ix])
    # and a Scale's gradients: d loss / d scale[c], d loss / d bias[c]
    want = R.net_bn_f64(cp, params, data, label)
    for pn, c in (("scale_a_2b_scale", 3), ("scale_stem_bias", 0), ("scale_b_2c_scale", 7)):
        p2 = {k: v.astype(np.float64) for k, v in params.items()}
        p2[pn] = p2[pn].copy(); p2[pn][c] += h; up = R.net_bn_f64(cp, p2, data, label, guard_rel=0.0, only_loss=True)["loss"]
        p2[pn][c] -= 2 * h; dn = R.net_bn_f64(cp, p2, data, label, guard_rel=0.0, only_loss=True)["loss"]
        assert abs((up - dn) / (2 * h) - want[pn + "_grad_loss"][c]) <= 1e-6 * np.max(np.abs(want[pn + "_grad_loss"])) + 1e-9, pn


def test_cpu_fuse_relu_grad_and_seed_in_var_leave_the_same_bits(cpu):
    seed = R.RES_SEEDS[0]
    drv, bp, *_, plain = res_step(cpu, seed)
    drv.release()
    drv, bp, *_, fused = res_step(cpu, seed, fuse_relu_grad=True, seed_in_var=True)
    try:
        assert drv.fused_relu_grads["folded"]        # e.g. a_2b_relu_bck, taken into a_2c_bck's data gradient
        for n in plain:
            assert R.same_bits(plain[n], fused[n]), n
    finally:
        drv.release()


def three_solver_steps(rtc, graph=None, check=True):
    """Three steps of the residual pipe with a solver (new inputs each, the rate changed once) -> the state after each step.  check: scale / bias / filts / biases move
    by the numpy update of the backend's own gradients, the BatchNorm statistics are untouched by the solver, and the running pair moves."""
    solver = SgdSolver(lr=0.05, momentum=0.9, weight_decay=5e-4, lr_mult={"biases": 2.0, "scale": 0.5}, decay_mult={"biases": 0.0, "bias": 0.0, "scale": 0.0})
    cp = R.residual(); bp = add_bck_ops(cp)
    drv = ConvPipeBck(rtc, solver=solver, bn_maf=0.9, seed_in_var=True); drv.init(bp, R.res_params(cp, 1))
    try:
        stats = bn_stat_params(cp)
        assert len(stats) == 16 and drv.sgd_params == [p for p in cp.params if p not in stats] and drv.n_sgd_calls == -(-len(drv.sgd_params) // 32)
        assert not any(s + SGD_HIST_SFX in drv.vars for s in stats)
        for _, f, am in drv.calls()[-drv.n_sgd_calls:]:
            assert not {a.n for a in am.values()} & set(stats)
        sv = list(cp.params) + [p + SGD_HIST_SFX for p in drv.sgd_params]
        if graph is not None:
            drv.capture_graph(parallel=graph)
        state = {n: rtc.copy_var_to_nda(n) for n in sv}
        hyper = [0.05, 0.9, 5e-4]
        states = []
        for k in range(3):
            if k == 1:
                drv.set_sgd_hyper(lr=0.02); hyper[0] = 0.02
            data, label = R.res_inputs(cp, 100 + k)
            drv.set_det_drop_seed(1000 + k)
            fwd = {"data": data, "label": label}
            gets = [p + "_grad_loss" for p in drv.sgd_params] + ["loss"] + [s.rsplit("_", 1)[0] + "_batch_mean" for s in stats if s.endswith("_mean")]
            drv.run_bck(["data", "label"], fwd, gets, graph=graph is not None)
            after = {n: rtc.copy_var_to_nda(n) for n in sv}
            if check:
                for p in drv.sgd_params:
                    w2, h2 = sgd_np(state[p], fwd[p + "_grad_loss"], state[p + SGD_HIST_SFX], hyper[0], hyper[1], hyper[2], solver.mult_of(solver.lr_mult, p), solver.mult_of(solver.decay_mult, p))
                    assert R.same_bits(after[p + SGD_HIST_SFX].reshape(-1), h2.reshape(-1)) and R.same_bits(after[p].reshape(-1), w2.reshape(-1)), p
                    if not p.endswith("_biases") or p == "fc_biases":
                        assert not R.same_bits(after[p], state[p]), (p, "the step changed nothing")
                for s in stats:
                    if s.endswith("_mean"):     # moved by the forward pass alone: maf * old + (1 - maf) * batch mean, two products and an add
                        bm = fwd[s.rsplit("_", 1)[0] + "_batch_mean"]
                        assert R.same_bits(after[s], R.F(0.9) * state[s] + (R.F(1) - R.F(0.9)) * bm) and not R.same_bits(after[s], state[s]), s
                    else:
                        assert not R.same_bits(after[s], state[s]), s
                assert solver.mult_of(solver.lr_mult, "scale_stem_scale") == 0.5 and solver.mult_of(solver.decay_mult, "scale_stem_bias") == 0.0
            state = after
            states.append(dict(after, loss=fwd["loss"]))
        return states
    finally:
        drv.release()


def test_cpu_solver_three_steps(cpu):
    states = three_solver_steps(cpu)
    assert all(np.isfinite(s["loss"]).all() for s in states)


def test_cpu_call_list_in_other_topological_orders(cpu):
    """_call_deps covers the new args and side vars: the call list run in two other topological orders on poisoned vars leaves the bits of the list order.  The running
    pair is read and written (INOUT), so the params are uploaded anew before every run."""
    cp = R.residual(); bp = add_bck_ops(cp)
    params = R.res_params(cp, 1); data, label = R.res_inputs(cp, 1)
    drv = ConvPipeBck(cpu, solver=SgdSolver(lr=0.05), bn_maf=0.9); drv.init(bp, params)
    try:
        keep = set(cp.params) | {p + SGD_HIST_SFX for p in drv.sgd_params} | {"data", "label", "sgd_hyper"}

        def run(order):
            for n, a in params.items():
                cpu.copy_nda_to_var(n, a)
            drv.zero_sgd_history()
            cpu.copy_nda_to_var("data", data); cpu.copy_nda_to_var("label", label)
            return run_in_order(cpu, drv, order, keep)
        deps = drv._call_deps()
        n = len(deps)
        calls = drv.bck_calls
        ix = {(c.tag, c.fop.get_func_name()): i for i, c in enumerate(calls)}
        assert ix[("stem", "hip_conv")] in deps[ix[("bn_stem", "hip_bn_stats")]] and ix[("bn_stem", "hip_bn_stats")] in deps[ix[("scale_stem", "hip_bn_fwd")]]
        assert ix[("scale_stem_bck", "hip_bn_bck_sums")] in deps[ix[("bn_stem_bck", "hip_bn_bck_in")]]
        want = run(range(n))
        rng = np.random.default_rng(17)
        for what, order in {"latest ready first": topo_order(deps, max), "random topological": topo_order(deps, lambda r: r[int(rng.integers(len(r)))])}.items():
            assert sorted(order) == list(range(n)) and order != list(range(n)), what
            got = run(order)
            for vn in drv.vars:
                assert got[vn].tobytes() == want[vn].tobytes(), (what, vn)
        victim = ix[("bn_stem_bck", "hip_bn_bck_in")]      # and the check can fail: the data gradient ahead of its two sums
        loose = [([] if i == victim else d) for i, d in enumerate(deps)]
        got = run(topo_order(loose, max))
        assert any(got[vn].tobytes() != want[vn].tobytes() for vn in drv.vars)
    finally:
        drv.release()


def test_driver_refusals(cpu):
    def pipe(kinds, on_conv=True):
        p = ConvPipe("bad", "data", Dims.make("float", img=2, chan=3, y=5, x=5))
        p.add(PipeOp("c", "Convolution", "data", "c", out_chans=4, kern_sz=(3, 3)))
        x = "c"
        if not on_conv:
            p.add(PipeOp("pl", "Pooling", "c", "pl", kern_sz=(2, 2), stride=(1, 1), avg_pool=1)); x = "pl"
        for i, k in enumerate(kinds):
            p.add(PipeOp(f"{k.lower()}{i}", k, x, x))
        p.add(PipeOp("fc", "Convolution", x, "fc", out_chans=5, kern_sz=(0, 0)))
        return add_bck_ops(p)
    for kinds, on_conv, msg in ((["Scale"], True, "the in-place ops on c are Scale; only the run .BatchNorm, Scale."),
                                (["BatchNorm"], True, "the in-place ops on c are BatchNorm; only the run"),
                                (["ReLU", "BatchNorm", "Scale"], True, "the in-place ops on c are ReLU BatchNorm Scale; only the run"),
                                (["BatchNorm", "Scale", "Dropout"], True, "behind .BatchNorm, Scale. only one in-place ReLU"),
                                (["BatchNorm", "Scale", "ReLU", "ReLU"], True, "behind .BatchNorm, Scale. only one in-place ReLU"),
                                (["BatchNorm", "Scale"], False, "a BatchNorm / Scale on pl, which a Pooling produces")):
        drv = ConvPipeBck(cpu)
        with pytest.raises(UnsupErr, match=msg):
            drv.init(pipe(kinds, on_conv))
        assert drv.vars == [] and drv.funcs == []
    drv = ConvPipeBck(cpu); drv.init(pipe(["BatchNorm", "Scale", "ReLU"])); drv.release()     # the supported shape


def test_host_params_of_a_batchnorm_pipe():
    bp = add_bck_ops(R.residual())
    hp = host_params(bp)
    assert not np.any(hp["bn_stem_mean"]) and np.all(hp["bn_stem_var"] == 1) and np.all(np.abs(hp["scale_stem_scale"] - 1) <= 0.1) and np.all(np.abs(hp["scale_stem_bias"]) <= 0.05)
    assert set(hp) == set(bp.cp.params)
