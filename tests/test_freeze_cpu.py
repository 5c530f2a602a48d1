"""Fine-tuning without a GPU: the three hip_bnf_* functions on be=cpu bit for bit against their numpy twins, their tables, plans and refusals;
Freeze's pruning rule as call lists written out here; param freezing held bit for bit to today's driver under lr_mult = decay_mult = 0; the frozen-BatchNorm step
against a float64 walk on the running pair.  tests/test_gpu_freeze.py runs the same checks on the MI355X."""
import os

import numpy as np
import pytest

import bn_ref as R
import eval_ref
import freeze_ref as Z
import solver_ref
import test_bck_pipe_cpu as P
from boda_amd import rtc as rtc_mod
from boda_amd.bck_pipe import ConvPipeBck, Freeze, SgdSolver, Solver, add_bck_ops, bn_stat_params
from boda_amd.cnn_op import BN_FUNCS, BNF_FUNCS, BNF_OP_FUNCS, NATIVE_ARGS, bnf_bck_func_op, bnf_bck_in_func_op, bnf_prep_func_op, pipe_func_args
from boda_amd.eval_pipe import EvalPipe
from boda_amd.op import Dims, Nda, RtErr, UnsupErr, read_ops
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc

HERE = os.path.dirname(os.path.abspath(__file__))
SPECIAL_CASE = ((2, 3, 57, 57), 2000)     # slabs inside a plane and across the two images, the element path


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


# ---- the functions
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_cpu_functions_against_numpy(cpu, case):
    shape, slab = case
    Z.check_against_numpy(Z.run_all_three(cpu, shape, slab), shape, slab)


def test_cpu_special_values_in_out_grad_loss(cpu):
    shape, slab = SPECIAL_CASE
    dy = Z.special_dy(shape)
    r = Z.run_all_three(cpu, shape, slab, dy=dy)
    Z.check_against_numpy(r, shape, slab)
    assert np.isnan(r["sg"][0]) and np.isnan(r["bg"][0]) and np.isinf(r["bg"][2]) and np.isfinite(r["sg"][1]) and np.isfinite(r["bg"][1])     # contained in their channels
    assert np.isnan(r["dx"]).sum() == 1 and np.isinf(r["dx"]).sum() == 1 and np.signbit(r["dx"][0, 0, 0, 1]) != np.signbit(r["scale"][0] * r["inv_std"][0])


def test_tables_arg_lists_and_plans():
    assert BNF_OP_FUNCS == {"BnfPrep": ("hip_bnf_prep",), "BnfBck": ("hip_bnf_bck",), "BnfBckIn": ("hip_bnf_bck_in",)} and set(BNF_FUNCS) <= set(BN_FUNCS)
    table = rtc_mod.native_funcs()
    for member, (t, (fn,)) in enumerate(BNF_OP_FUNCS.items(), 6):
        r = table[fn]
        assert (r["family"], r["member"], r["types"], r["multi_dev"], r["be"], r["flags"], r["opt"], r["why"]) == ("bnf", member, (t,), "one_device", ("hip", "cpu"), (), (), ""), fn
    d = R.dims_of((2, 3, 57, 57))
    for f in (bnf_prep_func_op(d, R.EPS), bnf_bck_func_op(d, 2000), bnf_bck_in_func_op(d)):
        assert rtc_mod.func_args(f) == pipe_func_args(f) == NATIVE_ARGS[f.get_func_name()]
    assert rtc_mod.explain_plan(bnf_bck_func_op(d, 2000)) == "bodahip_bn_sum grid=12 block=256 -DMODE=2 -DDX=1 | bodahip_bn_fin grid=1 block=256 -DFIN=2 | slab=2000 slabs=4"
    assert rtc_mod.explain_plan(bnf_prep_func_op(d, R.EPS)) == "bodahip_bnf_prep grid=1 block=256" and rtc_mod.explain_plan(bnf_bck_in_func_op(d)) == "bodahip_bnf_bck_in"


def test_fixture_file_lists_these_ops(cpu):
    ops = read_ops(os.path.join(HERE, "golden", "ops", "freeze-ops.txt"))
    assert [o.to_str() for o in ops] == [o.to_str() for o in Z.fixture_ops(cpu)]
    for o in ops:
        assert rtc_mod.explain_plan(o)


def compile_only(rtc, f):
    rtc.compile([RtcFuncInfo("bnf_bad", "", [a for a, _ in NATIVE_ARGS[f.get_func_name()]], f)])
    rtc.release_func("bnf_bad")


def bad_op(f, **nda):
    b = f.copy()
    b.nda_vals.update(nda)
    return b


def op_refusals(rtc):
    d = R.dims_of((2, 3, 4, 4))
    ch = lambda c: Nda(dims=Dims(("chan",), (c,), "float"), tn="float")
    with pytest.raises(RtErr, match="in_grad_loss dims .* differ from in's"):
        compile_only(rtc, bad_op(bnf_bck_func_op(d), in_grad_loss=Nda(dims=R.dims_of((2, 3, 4, 5)), tn="float")))
    with pytest.raises(RtErr, match="out_grad_loss dims .* differ from in's"):
        compile_only(rtc, bad_op(bnf_bck_in_func_op(d), out_grad_loss=Nda(dims=R.dims_of((1, 3, 4, 4)), tn="float")))
    with pytest.raises(RtErr, match="run_var dims .*: one float per channel of in"):
        compile_only(rtc, bad_op(bnf_prep_func_op(d, R.EPS), run_var=ch(4)))
    with pytest.raises(RtErr, match="eps must not be negative"):
        compile_only(rtc, bad_op(bnf_prep_func_op(d, R.EPS), eps=Nda(None, "float", (-1.0,))))
    with pytest.raises(RtErr, match="slab=6: a forced slab length is a multiple of 4"):
        compile_only(rtc, bad_op(bnf_bck_func_op(d), slab=Nda(None, "uint32_t", (6,))))


def call_refusals(rtc):
    """A var of other dims than the op's, and every alias but in_grad_loss = out_grad_loss."""
    shape = (2, 3, 4, 4)
    d = R.dims_of(shape)
    i = R.make_inputs(shape)
    ins = {"in": i["x"], "mean": i["run_mean"], "inv_std": i["run_var"], "scale": i["scale"], "out_grad_loss": i["dy"]}
    with pytest.raises(RtErr, match="args 'in' and 'in_grad_loss' are the same var"):
        R.run_func(rtc, bnf_bck_func_op(d), ins, bind={"in_grad_loss": "in"})
    with pytest.raises(RtErr, match="args 'scale_grad_loss' and 'bias_grad_loss' are the same var"):
        R.run_func(rtc, bnf_bck_func_op(d), ins, bind={"bias_grad_loss": "scale_grad_loss"})
    with pytest.raises(RtErr, match="args 'run_mean' and 'mean' are the same var"):
        R.run_func(rtc, bnf_prep_func_op(d, R.EPS), {"run_mean": i["run_mean"], "run_var": i["run_var"]}, bind={"mean": "run_mean"})
    with pytest.raises(RtErr, match="args 'inv_std' and 'scale' are the same var"):
        R.run_func(rtc, bnf_bck_in_func_op(d), {"inv_std": i["run_var"], "out_grad_loss": i["dy"]}, bind={"scale": "inv_std"})
    f = bnf_bck_in_func_op(d)     # a var of another image count: the hip_bnf_* functions take exactly the op's dims
    rtc.compile([RtcFuncInfo("bnf_w", "", [a for a, _ in pipe_func_args(f)], f)])
    names = {"inv_std": Dims.make("float", chan=3), "scale": Dims.make("float", chan=3), "out_grad_loss": R.dims_of((1, 3, 4, 4)), "in_grad_loss": R.dims_of((1, 3, 4, 4))}
    try:
        for an, dd in names.items():
            rtc.create_var_with_dims("bnfw_" + an, dd)
        with pytest.raises(RtErr, match="out_grad_loss"):
            rtc.run(RtcFuncCall("bnf_w", {an: RtcArg.var("bnfw_" + an) for an in names}))
    finally:
        for an in names:
            rtc.release_var("bnfw_" + an)
        rtc.release_func("bnf_w")


def test_refusals_of_the_op(cpu):
    op_refusals(cpu)


def test_cpu_refusals_of_the_call(cpu):
    call_refusals(cpu)


# ---- the plan: the call lists of the pruned backward walk, written out.  A convolution's gradient op emits hip_bconv_in, hip_bconv_biases, hip_bconv_filts under one tag
def run_of(tag, relu, conv=3):
    """The gradient calls of conv -> BatchNorm -> Scale (-> ReLU), in run order; conv: how many of the convolution's three calls are left."""
    return ([tag + "_relu_bck"] if relu else []) + ["scale_" + tag + "_bck", "bn_" + tag + "_bck"] + [tag + "_bck"] * conv


RES_FWD = ["stem", "bn_stem", "scale_stem", "a_b1", "bn_a_b1", "scale_a_b1", "a_2a", "bn_a_2a", "scale_a_2a", "a_2b", "bn_a_2b", "scale_a_2b", "a_2c", "bn_a_2c", "scale_a_2c", "res_a", "res_a_relu",
           "b_2a", "bn_b_2a", "scale_b_2a", "b_2b", "bn_b_2b", "scale_b_2b", "b_2c", "bn_b_2c", "scale_b_2c", "res_b", "res_b_relu", "gap", "fc", "loss", "loss", "loss"]
RES_TOP = ["fc_bck"] * 3 + ["gap_bck", "res_b_relu_bck", "res_b_bck"]
RES_BLOCK_B = run_of("b_2c", False) + run_of("b_2b", True) + run_of("b_2a", True) + ["reduce_res_a_grad_loss", "res_a_relu_bck", "res_a_bck"]
RES_BRANCH2 = run_of("a_2c", False) + run_of("a_2b", True)
RES_TODAY = RES_TOP + RES_BLOCK_B + RES_BRANCH2 + run_of("a_2a", True) + run_of("a_b1", False) + ["reduce_stem_grad_loss"] + run_of("stem", True)
STEM, BRANCH2 = ("stem", "scale_stem"), ("a_2a", "scale_a_2a", "a_2b", "scale_a_2b", "a_2c", "scale_a_2c")


def keep_data_tags():
    """RES_TODAY with every convolution below fc left with its hip_bconv_in alone."""
    out = list(RES_TOP)
    for t in RES_TODAY[len(RES_TOP):]:
        if out[-1] != t:
            out.append(t)
    return out


RES_PLANS = {
    "nothing": (lambda cp: Freeze(), RES_TODAY[:-1], ["data_grad_loss"]),     # the stem's hip_bconv_in alone
    # the stem fixed: nothing below stem's two readers needs a gradient -- their data gradients, the Reduce of the fan-out and the stem's whole run go
    "stem": (lambda cp: Freeze(params=STEM), RES_TOP + RES_BLOCK_B + RES_BRANCH2 + run_of("a_2a", True, 2) + run_of("a_b1", False, 2), ["stem_grad_loss", "stem_filts_grad_loss", "scale_stem_scale_grad_loss"]),
    "all_but_last": (lambda cp: Freeze(params=Z.all_but(cp, "fc")), ["fc_bck"] * 2, ["gap_grad_loss", "res_b_grad_loss", "b_2c_filts_grad_loss"]),
    # the stem and branch 2 of block a: the Eltwise gradient of res_a keeps ONE output (a hip_split copy), the shortcut's, whose convolution needs no data gradient
    "one_branch": (lambda cp: Freeze(params=STEM + BRANCH2), RES_TOP + RES_BLOCK_B + run_of("a_b1", False, 2), ["a_2c_grad_loss", "a_2a_filts_grad_loss", "stem_grad_loss"]),
    # a saliency map of the linear probe: every data gradient, the BatchNorm runs' sums, no filter or bias gradient below fc
    "keep_data": (lambda cp: Freeze(params=Z.all_but(cp, "fc"), keep_grads=("data",)), keep_data_tags(), ["stem_filts_grad_loss", "scale_b_2c_scale_grad_loss"][:1]),
}
FAN_FWD = ["stem", "a", "b", "cp", "c", "cat", "cat", "cat", "gap", "fc", "loss", "loss", "loss"]
FAN_TODAY = ["fc_bck"] * 3 + ["gap_bck"] + ["cat_bck"] * 3 + ["c_bck"] * 3 + ["cp_bck", "relu_b_bck"] + ["b_bck"] * 3 + ["relu_a_bck"] + ["a_bck"] * 3 + ["reduce_stem_grad_loss", "relu_stem_bck"] + ["stem_bck"] * 3
# everything under the Concat's third arm (the pooling cp and the convolution c) and the stem: hip_split writes two of the three arms
FAN_ARM = ["fc_bck"] * 3 + ["gap_bck"] + ["cat_bck"] * 2 + ["relu_b_bck"] + ["b_bck"] * 2 + ["relu_a_bck"] + ["a_bck"] * 2


def tags_of(drv):
    return [c.tag for c in drv.bck_calls]


def made(rtc, cp, params, freeze="absent", **kw):
    drv = ConvPipeBck(rtc, **kw) if freeze == "absent" else ConvPipeBck(rtc, freeze=freeze, **kw)
    drv.init(add_bck_ops(cp), params)
    return drv


def describe(drv):
    return (tags_of(drv), [(t, f.to_str(), {k: v.n for k, v in am.items() if v.is_var()}) for t, f, am in drv.calls()], list(drv.vars), drv._call_deps(), list(drv.sgd_params))


def test_no_freeze_is_todays_driver(cpu):
    for cp, fwd_tags, today in ((R.residual(), RES_FWD, RES_TODAY), (P.fan(), FAN_FWD, FAN_TODAY)):
        params = R.res_params(cp) if "res_a" in cp.nodes else P.small_params(cp, 0)
        got = []
        for kw in ({}, {"freeze": None}):     # a driver built without the argument, and one built with freeze=None
            drv = made(cpu, cp, params, **kw)
            try:
                got.append(describe(drv))
                assert drv.frozen == {"params": [], "dropped_calls": [], "bn_global": []}
            finally:
                drv.release()
        assert got[0] == got[1] and got[0][0] == fwd_tags + today


@pytest.mark.parametrize("name", sorted(RES_PLANS))
def test_plan_of_the_residual_pipe(cpu, name):
    cp = R.residual()
    mk, want, dropped = RES_PLANS[name]
    drv = made(cpu, cp, R.res_params(cp), freeze=mk(cp))
    try:
        assert tags_of(drv) == RES_FWD + want
        assert "data_grad_loss" not in drv.vars if name != "keep_data" else "data_grad_loss" in drv.vars
        fwd = dict(zip(("data", "label"), R.res_inputs(cp)))
        for vn in dropped:     # no dropped var exists, and asking for one names the rule
            assert vn not in drv.vars
            with pytest.raises(RtErr, match=vn + ".*is not computed by this driver.*needs a gradient.*keep_grads"):
                drv.run_bck(["data", "label"], fwd, [vn])
        fns = [f.get_func_name() for _, f, _ in drv.calls()]
        assert ("hip_split" in fns) == (name == "one_branch") and fns.count("hip_fan_out") == {"all_but_last": 0, "one_branch": 1}.get(name, 2)
        drv.run_bck(["data", "label"], fwd, ["loss"] + ([] if name != "keep_data" else ["data_grad_loss"]))
        assert np.isfinite(fwd["loss"]).all()
    finally:
        drv.release()


def test_plan_under_a_concat_arm(cpu):
    cp = P.fan()
    drv = made(cpu, cp, P.small_params(cp, 0), freeze=Freeze(params=("stem", "c")))
    try:
        assert tags_of(drv) == FAN_FWD + FAN_ARM
        assert drv.frozen == {"params": ["stem_filts", "stem_biases", "c_filts", "c_biases"], "dropped_calls": ["c_bck", "cp_bck", "reduce_stem_grad_loss", "relu_stem_bck", "stem_bck"], "bn_global": []}
        assert not {"c_grad_loss", "cp_grad_loss", "stem_grad_loss", "c_filts_grad_loss", "data_grad_loss"} & set(drv.vars)
        assert [am["out"].n for t, f, am in drv.calls() if t == "cat_bck"] == ["a_grad_loss", "b_grad_loss"]
    finally:
        drv.release()


def test_plan_with_relu_folds(cpu):
    """fuse_relu_grad: a fold whose producer's data gradient was dropped is dropped with it; one whose producer stays still takes its mask."""
    cp = P.fan()
    drv = made(cpu, cp, P.small_params(cp, 0), freeze=Freeze(params=("stem",)), fuse_relu_grad=True)
    try:
        assert "relu_stem_bck" not in tags_of(drv) and "reduce_stem_grad_loss" not in tags_of(drv) and tags_of(drv).count("a_bck") == 2
    finally:
        drv.release()


def test_plan_with_the_fused_filter_and_bias_gradient(cpu):
    """fuse_filts_biases needs no new form: a convolution whose params are not both frozen keeps the one fused call, a frozen one loses it; the step holds the bits of the
    unfused frozen step in every node both compute but the fused gradients' own."""
    cp = P.fan()
    fz = Freeze(params=("stem", "c", "a_filts"))     # a_filts alone: per-param freezing inside a convolution is not provided, both gradients stay, only a_biases trains
    fwd_of = {}
    for fused in (False, True):
        drv = made(cpu, cp, P.small_params(cp, 0), freeze=fz, fuse_filts_biases=fused)
        try:
            fns = [(t, f.get_func_name()) for t, f, _ in drv.calls()]
            assert [f for t, f in fns if t == "a_bck"] == (["hip_bconv_filts_biases"] if fused else ["hip_bconv_biases", "hip_bconv_filts"]) and not [f for t, f in fns if t in ("c_bck", "stem_bck")]
            assert "a_filts" not in drv.sgd_params and "a_biases" in drv.sgd_params and "a_filts_grad_loss" in drv.vars
            fwd = dict(zip(("data", "label"), P.small_inputs(cp, 3)))
            drv.run_bck(["data", "label"], fwd, ["loss", "a_grad_loss", "b_grad_loss", "gap_grad_loss", "a_biases_grad_loss"])
            fwd_of[fused] = fwd
        finally:
            drv.release()
    for n in ("loss", "a_grad_loss", "b_grad_loss", "gap_grad_loss", "a_biases_grad_loss"):
        assert R.same_bits(fwd_of[False][n], fwd_of[True][n]), n


def test_frozen_batchnorm_call_list(cpu):
    cp = R.residual()
    fn_of = lambda drv: [(t, f.get_func_name()) for t, f, _ in drv.calls()]
    drv = made(cpu, cp, R.res_params(cp), freeze=Z.frozen_bn())
    try:
        fns = fn_of(drv)
        assert [f for t, f in fns if t.startswith("bn_") and not t.endswith("_bck")] == ["hip_bnf_prep"] * 8 and [f for t, f in fns if t.startswith("scale_") and not t.endswith("_bck")] == ["hip_bn_fwd"] * 8
        # BckScale is hip_bnf_bck in place on X_grad_loss, BckBatchNorm emits nothing (the stem's run too: its convolution's gradients read stem_grad_loss)
        assert [f for t, f in fns if t.startswith("scale_") and t.endswith("_bck")] == ["hip_bnf_bck"] * 8 and not [t for t, f in fns if t.startswith("bn_") and t.endswith("_bck")]
        am = dict((t, a) for t, _, a in drv.calls())["scale_a_2b_bck"]
        assert am["in_grad_loss"].n == am["out_grad_loss"].n == "a_2b_grad_loss" and am["in"].n == "a_2b_bn_in" and am["mean"].n == "bn_a_2b_batch_mean"
        assert drv.frozen["bn_global"] == [o.tag for o in cp.ops if o.type == "BatchNorm"] and drv.frozen["params"] == []
    finally:
        drv.release()
    drv = made(cpu, cp, R.res_params(cp), freeze=Freeze(params=("stem",), bn_global_stats=["bn_stem"]))
    try:     # the run's input needs no gradient (a frozen convolution on the input node), its Scale trains: the sums alone, hip_bn_bck_sums as it is
        fns = dict(fn_of(drv))
        assert fns["scale_stem_bck"] == "hip_bn_bck_sums" and "bn_stem_bck" not in fns and "stem_bck" not in fns and "stem_relu_bck" in fns and "stem_grad_loss" in drv.vars
    finally:
        drv.release()
    drv = made(cpu, cp, R.res_params(cp), freeze=Freeze(params=("scale", "bias"), bn_global_stats=["bn_a_2b", "bn_stem"]))
    try:
        fns = dict(fn_of(drv))
        assert fns["bn_a_2b_bck"] == "hip_bnf_bck_in" and "scale_a_2b_bck" not in fns and fns["bn_stem_bck"] == "hip_bnf_bck_in" and "scale_stem_bck" not in fns     # both Scale params frozen
        assert fns["bn_a_2b"] == "hip_bnf_prep" and fns["bn_a_2a"] == "hip_bn_stats" and fns["scale_a_2a_bck"] == "hip_bn_bck_sums" and fns["bn_a_2a_bck"] == "hip_bn_bck_in"
        assert "scale_a_2b_scale_grad_loss" not in drv.vars and "scale_a_2a_scale_grad_loss" in drv.vars and "scale_a_2a_scale" not in drv.sgd_params
    finally:
        drv.release()


def test_driver_refusals(cpu):
    cp = R.residual()
    params = R.res_params(cp)
    for fz, err, msg in ((Freeze(params=("stem", "no_such_layer")), RtErr, "params names 'no_such_layer', which is no param of the pipe"),
                         (Freeze(params=("bn_stem_mean",)), RtErr, "params names 'bn_stem_mean'.*running statistics are never solver params"),
                         (Freeze(bn_global_stats=["scale_stem"]), RtErr, "bn_global_stats names 'scale_stem', which is no BatchNorm op"),
                         (Freeze(keep_grads=("label",)), RtErr, "keep_grads names 'label', which is no node of the pipe"),
                         (Freeze(params=("filts", "biases", "scale", "bias")), RtErr, "Freeze leaves nothing trainable")):
        drv = ConvPipeBck(cpu, freeze=fz)
        with pytest.raises(err, match=msg):
            drv.init(add_bck_ops(cp), params)
        assert drv.vars == [] and drv.funcs == []
    drv = ConvPipeBck(cpu, freeze=Z.frozen_bn(), img_chunks=2)
    with pytest.raises(UnsupErr, match="bn_global_stats=.* together with img_chunks=2: the hip_bnf_\\* functions have no chunked chain"):
        drv.init(add_bck_ops(cp), params)
    assert drv.vars == [] and drv.funcs == []
    with pytest.raises(RtErr, match="freeze must be a bck_pipe.Freeze or None"):
        ConvPipeBck(cpu, freeze=("stem",))


# ---- param freezing by bits
FROZEN_PIPES = {"residual": (R.residual, lambda cp: R.res_params(cp, 1), lambda cp, k: R.res_inputs(cp, 100 + k), STEM),
                "fan": (P.fan, lambda cp: P.small_params(cp, 0), lambda cp, k: P.small_inputs(cp, 20 + k), ("stem", "c")),
                "chain": (P.chain, lambda cp: P.small_params(cp, 0), lambda cp, k: P.small_inputs(cp, 20 + k), ("conv1",))}
SOLVERS = {"sgd": dict(type="sgd", lr=0.05, momentum=0.9, weight_decay=5e-4), "adam": dict(type="adam", lr=0.01, momentum=0.9, weight_decay=5e-4)}


def steps(rtc, cp, params, inputs, solver, freeze="absent", n=3, graph=None, **kw):
    """n steps -> (the state after each: loss, every gradient node the driver computes, every param, every history; the driver's frozen report, its sgd_params)."""
    drv = made(rtc, cp, params, freeze=freeze, solver=solver, seed_in_var=True, **kw)
    try:
        if graph is not None:
            drv.capture_graph(parallel=graph)
        gets = [n_ for n_ in drv.bp.nodes if n_.endswith("_grad_loss") and n_ in drv.vars] + ["loss"] + solver_ref.state_vars(drv)
        out = []
        for k in range(n):
            data, label = inputs(cp, k)
            drv.set_det_drop_seed(1000 + k)
            fwd = {"data": data, "label": label}
            drv.run_bck(["data", "label"], fwd, gets, graph=graph is not None)
            out.append({v: fwd[v] for v in gets})
        return out, dict(drv.frozen), list(drv.sgd_params)
    finally:
        drv.release()


def check_param_freezing(rtc, name, which, rtc_today=None):
    mk, mk_params, inputs, tags = FROZEN_PIPES[name]
    cp = mk()
    params = mk_params(cp)
    froz, rep, trainable = steps(rtc, cp, params, inputs, Solver(**SOLVERS[which]), freeze=Freeze(params=tags))
    zero = {p: 0.0 for p in rep["params"]}
    today, _, all_params = steps(rtc_today or rtc, cp, params, inputs, Solver(lr_mult=zero, decay_mult=zero, **SOLVERS[which]))
    assert rep["params"] and set(trainable) == set(all_params) - set(rep["params"]) and rep["dropped_calls"]
    for k, (a, b) in enumerate(zip(froz, today)):
        assert not [v for v in a if v.endswith(("_sgd_hist", "_sgd_hist2", "_grad_acc")) and v.rsplit("_sgd_", 1)[0] in rep["params"]]     # no solver var of a frozen param
        for v in a:     # the loss, every kept gradient node, every param, the trainable params' histories
            assert R.same_bits(a[v], b[v]), (name, which, k, v)
        for p in rep["params"]:
            assert R.same_bits(a[p], np.asarray(params[p], np.float32).reshape(a[p].shape)) and R.same_bits(b[p], a[p]), (p, "a frozen param moved")
        assert all(not R.same_bits(a[p], np.asarray(params[p], np.float32).reshape(a[p].shape)) for p in trainable if p.endswith("_filts"))
    assert len(froz[0]) < len(today[0])     # fewer gradient nodes and no history of a frozen param


@pytest.mark.parametrize("which", sorted(SOLVERS))
@pytest.mark.parametrize("name", sorted(FROZEN_PIPES))
def test_cpu_param_freezing_by_bits(cpu, name, which):
    check_param_freezing(cpu, name, which)


def test_cpu_clipped_steps_against_the_twin(cpu):
    """With clipping the norm is the trainable params' alone: partials, norm, coef and every update held to tests/solver_ref.py's twins over sgd_params."""
    for which in ("sgd", "adam"):
        solver_ref.three_steps(cpu, "fan", Solver(clip_gradients=0.05, **SOLVERS[which]), freeze=Freeze(params=("stem", "c")))
        solver_ref.three_steps(cpu, "chain", Solver(clip_gradients=0.05, **SOLVERS[which]), freeze=Freeze(params=("conv1",)), seed_in_var=True)


def test_cpu_iter_size_and_sgd_solver(cpu):
    """iter_size accumulates the trainable params' gradients alone; an SgdSolver updates them alone."""
    cp = P.fan()
    drv = made(cpu, cp, P.small_params(cp, 0), freeze=Freeze(params=("stem", "c")), solver=Solver(type="sgd", lr=0.05), iter_size=2)
    try:
        assert sorted(v[:-len("_grad_acc")] for v in drv.vars if v.endswith("_grad_acc")) == sorted(drv.sgd_params) == sorted(["a_filts", "a_biases", "b_filts", "b_biases", "fc_filts", "fc_biases"])
    finally:
        drv.release()
    drv = made(cpu, cp, P.small_params(cp, 0), freeze=Freeze(params=("stem", "c")), solver=SgdSolver(lr=0.05))
    try:
        before = {p: cpu.copy_var_to_nda(p) for p in cp.params}
        fwd = dict(zip(("data", "label"), P.small_inputs(cp, 3)))
        drv.run_bck(["data", "label"], fwd, ["loss"])
        for p in cp.params:
            assert R.same_bits(cpu.copy_var_to_nda(p), before[p]) == (p in drv.frozen["params"]), p
    finally:
        drv.release()


# ---- the frozen BatchNorm step
def frozen_res_step(rtc, seed, **kw):
    cp = R.residual(); bp = add_bck_ops(cp)
    params = R.res_params(cp, seed); data, label = R.res_inputs(cp, seed)
    drv = ConvPipeBck(rtc, freeze=Freeze(bn_global_stats=True, keep_grads=("data",)), **kw); drv.init(bp, params)
    fwd = {"data": data, "label": label}
    drv.run_bck(["data", "label"], fwd, Z.res_grad_nodes(drv, bp) + bn_stat_params(cp) + Z.relu_nodes(cp))
    return drv, bp, params, data, label, fwd


def check_frozen_step_against_f64(rtc, seed, where):
    drv, bp, params, data, label, fwd = frozen_res_step(rtc, seed)
    try:
        nodes = Z.res_grad_nodes(drv, bp)
        assert len(nodes) == 1 + len(Z.trainable_params(bp.cp)) + len(bp.cp.nodes)     # the loss, every param's and every node's gradient (data's: keep_grads)
        worst = Z.frozen_dev(fwd, Z.net_bnf_f64(bp.cp, params, data, label, {n: fwd[n] > 0 for n in Z.relu_nodes(bp.cp)}), nodes)
        print(f"{where} frozen residual seed {seed}: largest max|got - want| / max|want| = {worst:.3e}")
        for s in bn_stat_params(bp.cp):     # the running pair is only read
            assert R.same_bits(fwd[s], params[s]), s
        return worst
    finally:
        drv.release()


@pytest.mark.parametrize("seed", R.RES_SEEDS)
def test_cpu_frozen_step_against_float64(cpu, seed):
    worst = check_frozen_step_against_f64(cpu, seed, "be=cpu")
    assert worst <= 10 * Z.FROZEN_DEV_CPU and worst <= Z.CAP


def test_frozen_dev_constant_is_the_measured_one(cpu):
    got = [check_frozen_step_against_f64(cpu, s, "be=cpu") for s in R.RES_SEEDS]
    assert abs(max(got) - Z.FROZEN_DEV_CPU) <= 1e-3 * Z.FROZEN_DEV_CPU, got


def check_running_pair_after_three_steps(rtc):
    cp = R.residual()
    params = R.res_params(cp, 1)
    out, rep, _ = steps(rtc, cp, params, lambda cp_, k: R.res_inputs(cp_, 100 + k), Solver(**SOLVERS["sgd"]), freeze=Z.frozen_bn())
    for s in bn_stat_params(cp):
        assert R.same_bits(out[-1][s], params[s]), s
    assert not R.same_bits(out[-1]["scale_stem_scale"], params["scale_stem_scale"]) and len(rep["bn_global"]) == 8


def test_cpu_running_pair_keeps_its_bits(cpu):
    check_running_pair_after_three_steps(cpu)


def check_eval_over_a_frozen_driver(rtc):
    """EvalPipe keeps its own arithmetic (hip_bn_fold + hip_chan_affine): over the frozen driver it returns what it returns over an unfrozen one holding the same params."""
    cp = R.residual()
    params = R.res_params(cp, 1)
    res = []
    for fz in (Freeze(params=STEM, bn_global_stats=True), None):
        drv = made(rtc, cp, params, freeze=fz)
        ev = EvalPipe(drv, top_k=2)
        try:
            for k in range(2):
                data, label = R.res_inputs(cp, 300 + k)
                ev.run_batch({"data": data, "label": label})
            res.append(ev.result())
        finally:
            ev.release(); drv.release()
    assert res[0] == res[1] and res[0]["images"] == 6, res


def test_cpu_eval_over_a_frozen_driver(cpu):
    check_eval_over_a_frozen_driver(cpu)
