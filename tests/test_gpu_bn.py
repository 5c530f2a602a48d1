"""The training BatchNorm on the MI355X (kernels/bn_f32.hip): the five functions on be=hip bit for bit against be=cpu and the numpy twin of the
written chain (tests/bn_ref.py), the residual pipe's step against the float64 walk and call by call against be=cpu on the GPU's own inputs, the step as a serial and
as a parallel hipGraph replay against the eager step, and the refusal on several devices.

Every function comparison is np.array_equal on the uint32 views.  Outputs start from NaN and a guard var -- four floats holding a NaN with a payload -- stands behind
every var (bn_ref.run_func); the var bound to an arg must have exactly the op's dims, so the guard cannot live inside a wider var.  Not covered: tensors whose pointers
are not 16-byte aligned (the element path on a plane of whole quads), which no var of this backend produces; the element path itself runs on the odd planes."""
import numpy as np
import pytest

import bn_ref as R
import test_bn_cpu as T
import test_gpu_bck_pipe as P
from boda_amd import rtc as rtc_mod
from boda_amd.bck_pipe import ConvPipeBck, SgdSolver, add_bck_ops
from boda_amd.cnn_op import BN_FUNCS, bn_bck_in_func_op, bn_bck_sums_func_op, bn_fwd_func_op, bn_stats_func_op, fan_out_func_op, pipe_func_args
from boda_amd.conv_pipe import ConvPipe, PipeOp
from boda_amd.op import Dims, RtErr, UnsupErr
from boda_amd.rtc import make_rtc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    r = make_rtc("(be=hip)", 0)
    r.init()
    yield r
    r.close()


@pytest.fixture(scope="module")
def hip2():
    """The eager driver's backend: a second instance, with a stream, vars and kernels of its own."""
    r = make_rtc("(be=hip)", 0)
    r.init()
    yield r
    r.close()


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


# ---- the functions
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_functions_against_cpu_and_numpy(hip, cpu, case):
    shape, slab = case
    for relu in (0, 1):
        g = R.run_all_five(hip, shape, slab, relu=relu, repeat=2)      # (every reducing function launched twice on the same workspace)
        c = R.run_all_five(cpu, shape, slab, relu=relu)
        for k in ("mean", "inv_std", "run_mean2", "run_var2", "out", "sg", "bg", "dx"):
            assert R.same_bits(g[k], c[k]), (k, relu)
        R.check_against_numpy(g, shape, slab, relu=relu)
        ln = g["launch_stats"]
        C, N = shape[1], shape[0] * shape[2] * shape[3]
        assert ln["kernel"] == "bodahip_bn_sum" and ln["kernels"] == 3 and ln["grid"] == C * R.slab_plan(C, N, slab)[1], ln
    if N >= 8:
        fr = R.f64_bounds_fractions(g, shape, relu=1)
        print(R.case_id(case), {k: round(v, 4) for k, v in fr.items()})
        assert all(v <= 1.0 for v in fr.values()), fr


@pytest.mark.parametrize("n", [2, 3, 8])
def test_fan_out(hip, n):
    for shape in R.SHAPES:     # (2,3,1,1: one quad and a 2-element tail; 5,65,4,4: whole quads over several workgroups; the odd sizes: quads and a tail)
        x = R.make_inputs(shape)["x"]
        x.reshape(-1)[0] = -0.0
        keep = []
        out = R.run_func(hip, fan_out_func_op(R.dims_of(shape), n), {"in": x}, keep=keep)[0]
        assert len(out) == n and keep[0]["kernel"] == "bodahip_fan_out" and keep[0]["kernels"] == 1
        for a in out.values():
            assert R.same_bits(a, x)


def test_in_place_forms(hip):
    for shape in ((3, 2, 7, 7), (5, 65, 4, 4)):      # the element path and the quad path
        d = R.dims_of(shape)
        r = R.run_all_five(hip, shape)
        common = {"in": r["x"], "mean": r["mean"], "inv_std": r["inv_std"]}
        out = R.run_func(hip, bn_fwd_func_op(d, 1), dict(common, scale=r["scale"], bias=r["bias"]), bind={"out": "in"})[0]["out"]
        assert R.same_bits(out, r["out"])
        dx = R.run_func(hip, bn_bck_in_func_op(d), dict(common, scale=r["scale"], scale_grad_loss=r["sg"], bias_grad_loss=r["bg"], out_grad_loss=r["dy"]),
                        bind={"in_grad_loss": "out_grad_loss"})[0]["in_grad_loss"]
        assert R.same_bits(dx, r["dx"])


def test_refusals_of_the_call_on_hip(hip):
    T.var_refusals(hip)


def test_running_pair_after_two_calls(hip):
    shape = (3, 5, 3, 3)
    i = R.make_inputs(shape)
    got = R.run_func(hip, bn_stats_func_op(R.dims_of(shape), R.EPS, R.MAF), {"in": i["x"], "run_mean": i["run_mean"], "run_var": i["run_var"]}, repeat=2)
    m1, s1, rm1, rv1 = R.stats_np(i["x"], i["run_mean"], i["run_var"])
    m2, s2, rm2, rv2 = R.stats_np(i["x"], rm1, rv1)
    assert R.same_bits(got[1]["run_mean"], rm2) and R.same_bits(got[1]["run_var"], rv2) and R.same_bits(got[1]["mean"], m1)


# ---- the residual pipe
def test_residual_step_against_float64(hip):
    """The wiring: a wrong var would pass call by call, not this."""
    seed = R.RES_SEEDS[0]
    drv, bp, params, data, label, fwd = T.res_step(hip, seed)
    try:
        worst = T.check_against_f64(bp, params, data, label, fwd, "be=hip", T.CAP)
        print(f"be=hip residual seed {seed}: largest max|got - want| / max|want| = {worst:.3e}")
        assert worst <= 10 * R.DRIVER_DEV_CPU
    finally:
        drv.release()


def test_residual_step_call_by_call(hip, cpu):
    """The kernels, independent of the plumbing: every call against be=cpu on the GPU's own inputs -- the five new functions bit for bit."""
    drv, bp, params, data, label, fwd = T.res_step(hip, R.RES_SEEDS[1])
    try:
        hip.copy_nda_to_var("data", data); hip.copy_nda_to_var("label", label)
        seen = []
        for c in drv.bck_calls:
            fn = c.fop.get_func_name()
            if fn not in BN_FUNCS:
                seen.append(P.check_call(hip, cpu, c.tag, c.fop, c.rfc)); continue
            spec = pipe_func_args(c.fop)
            ins = {an: hip.copy_var_to_nda(c.rfc.arg_map[an].n) for an, io in spec if io in ("IN", "INOUT")}
            hip.run(c.rfc); hip.finish_and_sync()
            assert hip.last_launch()["kernel"] in ("bodahip_bn_sum", "bodahip_bn_fwd", "bodahip_bn_bck_in", "bodahip_fan_out")
            got = {an: hip.copy_var_to_nda(c.rfc.arg_map[an].n) for an, io in spec if io != "IN"}
            bind = {"in_grad_loss": "out_grad_loss"} if fn == "hip_bn_bck_in" else None
            want = R.run_func(cpu, c.fop, ins, bind=bind)[0]
            for an in got:
                assert R.same_bits(got[an], want[an]), (c.tag, fn, an)
            seen.append(fn)
        hip.release_per_call_id_data()
        assert len(seen) == len(drv.calls()) and all(seen.count(f) == k for f, k in (("hip_bn_stats", 8), ("hip_bn_fwd", 8), ("hip_bn_bck_sums", 8), ("hip_bn_bck_in", 8), ("hip_fan_out", 2)))
        for n in fwd:     # stepping through the calls one by one is the same step (the running pair aside: it has moved twice)
            if n.endswith("_grad_loss") or n == "loss":
                assert R.same_bits(hip.copy_var_to_nda(n), fwd[n]), n
    finally:
        drv.release()


def test_graph_replays_with_solver(hip, hip2):
    """The step as a serial and as a parallel graph replay against the eager step, over three rounds of new inputs and seeds each, with a solver: every gradient, the
    loss, every param, the history and the running statistics bit for bit."""
    mk_solver = lambda: SgdSolver(lr=0.05, momentum=0.9, weight_decay=5e-4, lr_mult={"biases": 2.0, "scale": 0.5}, decay_mult={"biases": 0.0, "bias": 0.0})
    cp = R.residual(); bp = add_bck_ops(cp)
    G = ConvPipeBck(hip, solver=mk_solver(), bn_maf=0.9, seed_in_var=True); G.init(bp, R.res_params(cp, 1))
    E = ConvPipeBck(hip2, solver=mk_solver(), bn_maf=0.9); E.init(add_bck_ops(R.residual()), R.res_params(cp, 1))
    try:
        state = list(cp.params) + [p + "_sgd_hist" for p in G.sgd_params]
        gets = [n for n in bp.nodes if n.endswith("_grad_loss")] + ["loss"] + state
        fetch = lambda r: {n: r.copy_var_to_nda(n) for n in state}
        rounds = [(11, None), (12, 0.02), (13, None), (14, 0.1), (15, None), (16, 0.01)]
        for parallel, some in ((False, rounds[:3]), (True, rounds[3:])):
            before = fetch(hip)
            n = G.capture_graph(parallel=parallel)     # (the first: no step has run on G, capture_graph runs one -- without the update calls)
            assert n == len(G.calls())
            after = fetch(hip)
            for vn in state:     # a capture leaves params, history and the running statistics as they were
                assert R.same_bits(before[vn], after[vn]), ("capture_graph changed", vn, parallel)
            for inp, lr in some:
                if lr is not None:
                    G.set_sgd_hyper(lr=lr); E.set_sgd_hyper(lr=lr)
                data, label = R.res_inputs(cp, inp)
                outs = []
                for d, graph in ((G, True), (E, False)):
                    d.set_det_drop_seed(inp)
                    fwd = {"data": data, "label": label}
                    d.run_bck(["data", "label"], fwd, gets, graph=graph)
                    outs.append(fwd)
                g, e = outs
                for vn in gets:
                    assert R.same_bits(g[vn], e[vn]), (parallel, inp, vn)
                assert not R.same_bits(g["bn_stem_mean"], before["bn_stem_mean"]) and not R.same_bits(g["scale_stem_scale"], before["scale_stem_scale"])
    finally:
        G.release(); E.release()


def test_solver_three_steps(hip):
    states = T.three_solver_steps(hip)
    assert all(np.isfinite(s["loss"]).all() for s in states)


# ---- several devices
def test_two_shards_refuse_it(hip):
    multi = make_rtc("(be=hip,devices=0:0)"); multi.init()
    try:
        cp = R.residual(4); bp = add_bck_ops(cp)
        drv = ConvPipeBck(multi)
        with pytest.raises(UnsupErr, match="the pipe has a BatchNorm.*not provided on a multi-device backend"):
            drv.init(bp, R.res_params(cp, 1))
        assert drv.vars == [] and drv.funcs == []      # refused before anything was created
        p = ConvPipe("elt", "data", Dims.make("float", img=4, chan=3, y=5, x=5))      # an Eltwise and no BatchNorm: its gradient is hip_fan_out
        for t in ("a", "b"):
            p.add(PipeOp(t, "Convolution", "data", t, out_chans=4, kern_sz=(3, 3)))
        p.add(PipeOp("s", "Eltwise", "a", "s", bots=("a", "b"))); p.add(PipeOp("fc", "Convolution", "s", "fc", out_chans=5, kern_sz=(0, 0)))
        drv = ConvPipeBck(multi)
        with pytest.raises(UnsupErr, match="the pipe has an Eltwise.*not provided on a multi-device backend"):
            drv.init(add_bck_ops(p))
        assert drv.vars == [] and drv.funcs == []
        shape = (4, 3, 2, 2)
        d = R.dims_of(shape)
        i = R.make_inputs(shape)
        x, ch = i["x"], i["scale"]
        common = {"in": x, "mean": ch, "inv_std": ch}
        for fop, ins, msg in ((bn_stats_func_op(d, R.EPS, R.MAF), {"in": x, "run_mean": ch, "run_var": ch}, "per-channel sums.*WHOLE batch"),
                              (bn_bck_sums_func_op(d), dict(common, out_grad_loss=x), "per-channel sums.*WHOLE batch"),
                              (bn_bck_in_func_op(d), dict(common, scale=ch, scale_grad_loss=ch, bias_grad_loss=ch, out_grad_loss=x), "data gradient.*WHOLE batch"),
                              (bn_fwd_func_op(d, 1), dict(common, scale=ch, bias=ch), "hip_bn_fwd.*not img shards"),
                              (fan_out_func_op(d, 2), {"in": x}, "hip_fan_out.*not img shards")):
            with pytest.raises(UnsupErr, match=msg):
                R.run_func(multi, fop, ins)
    finally:
        multi.close()
