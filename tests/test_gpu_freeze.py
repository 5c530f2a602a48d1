"""Fine-tuning on the MI355X: the three hip_bnf_* functions bit for bit against be=cpu and their numpy twins, their launch record and refusals;
param freezing held bit for bit to today's driver under lr_mult = decay_mult = 0, on one device and on two shards; the frozen-BatchNorm step against the float64 walk,
call by call against be=cpu, over three steps and under the evaluation pass; the frozen step as a serial and as a parallel graph replay."""
import numpy as np
import pytest

import bn_ref as R
import freeze_ref as Z
import bck_shards_ref as sref
import solver_ref
import test_freeze_cpu as T
import test_gpu_bck_pipe as P
from boda_amd.bck_pipe import ConvPipeBck, Freeze, LrPolicy, Solver, add_bck_ops, bn_stat_params
from boda_amd.cnn_op import BN_FUNCS, IMG_SHARDS_FUNCS, bnf_bck_func_op, bnf_bck_in_func_op, bnf_prep_func_op, has_img_shards_flag, pipe_func_args
from boda_amd.op import RtErr, UnsupErr
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
    g = Z.run_all_three(hip, shape, slab)
    c = Z.run_all_three(cpu, shape, slab)
    for k in Z.RESULT_KEYS:
        assert R.same_bits(g[k], c[k]), k
    Z.check_against_numpy(g, shape, slab)
    ln = g["launch"]     # two kernels: the slab sums that also store dx, one workgroup per (channel, slab), and the step that adds the slab partials
    C, N = shape[1], shape[0] * shape[2] * shape[3]
    assert ln["kernel"] == "bodahip_bn_sum" and ln["kernels"] == 2 and ln["grid"] == C * R.slab_plan(C, N, slab)[1] and ln["block"] == 256, ln


def test_special_values_in_out_grad_loss(hip, cpu):
    shape, slab = T.SPECIAL_CASE
    dy = Z.special_dy(shape)
    g = Z.run_all_three(hip, shape, slab, dy=dy)
    c = Z.run_all_three(cpu, shape, slab, dy=dy)
    for k in Z.RESULT_KEYS:
        print(k, "hip / cpu bits at the specials:", [hex(int(v)) for v in g[k].reshape(-1).view(np.uint32)[~np.isfinite(g[k].reshape(-1))][:4]],
              [hex(int(v)) for v in c[k].reshape(-1).view(np.uint32)[~np.isfinite(c[k].reshape(-1))][:4]])
    for k in Z.RESULT_KEYS:
        assert R.same_bits(g[k], c[k]), k
    Z.check_against_numpy(g, shape, slab)


def test_refusals_of_the_op_and_the_call_on_hip(hip):
    T.op_refusals(hip)
    T.call_refusals(hip)


def test_two_shards_refuse_the_functions_and_the_option():
    multi = make_rtc("(be=hip,devices=0:0)"); multi.init()
    try:
        shape = (4, 3, 2, 2)
        d = R.dims_of(shape)
        i = R.make_inputs(shape)
        x, ch = i["x"], i["scale"]
        why = "BatchNorm on its running pair.*exactly its op's dims, not img shards.*frozen statistics on several devices are out of scope"
        for fop, ins in ((bnf_prep_func_op(d, R.EPS), {"run_mean": ch, "run_var": ch}), (bnf_bck_func_op(d), {"in": x, "mean": ch, "inv_std": ch, "scale": ch, "out_grad_loss": x}),
                         (bnf_bck_in_func_op(d), {"inv_std": ch, "scale": ch, "out_grad_loss": x})):
            with pytest.raises(UnsupErr, match=why):
                R.run_func(multi, fop, ins)
        cp = R.residual(4)
        drv = ConvPipeBck(multi, freeze=Z.frozen_bn(), img_chunks=2)
        with pytest.raises(UnsupErr, match="Freeze\\(bn_global_stats=...\\): a BatchNorm on its running pair.*not provided on a multi-device backend"):
            drv.init(add_bck_ops(cp), R.res_params(cp, 1))
        assert drv.vars == [] and drv.funcs == []      # refused before anything was created
    finally:
        multi.close()


# ---- param freezing by bits
@pytest.mark.parametrize("which", sorted(T.SOLVERS))
@pytest.mark.parametrize("name", sorted(T.FROZEN_PIPES))
def test_param_freezing_by_bits(hip, hip2, name, which):
    T.check_param_freezing(hip, name, which, rtc_today=hip2)


def test_clipped_steps_against_the_twin(hip):
    solver_ref.three_steps(hip, "fan", Solver(clip_gradients=0.05, **T.SOLVERS["adam"]), freeze=Freeze(params=("stem", "c")))
    solver_ref.three_steps(hip, "chain", Solver(clip_gradients=0.05, **T.SOLVERS["sgd"]), freeze=Freeze(params=("conv1",)), seed_in_var=True)


def test_param_freezing_on_two_shards(hip):
    """tests/test_gpu_bck_shards.py's bars on the pruned step: every img-leading node and the loss the bits of the one-device step, every filter / bias gradient the
    per-shard gradients added in device order; fewer calls and fewer shard sums than the unfrozen step."""
    cp = T.P.fan(3)
    params = T.P.small_params(cp, 0)
    multi = make_rtc("(be=hip,devices=0:0)"); multi.init()
    fz = Freeze(params=("stem", "c"))
    d1 = ConvPipeBck(hip, freeze=fz); dm = ConvPipeBck(multi, freeze=fz)
    try:
        d1.init(add_bck_ops(cp), params); dm.init(add_bck_ops(cp), params)
        assert [t for t, _, _ in d1.calls()] == [t for t, _, _ in dm.calls()] == T.FAN_FWD + T.FAN_ARM
        assert all(has_img_shards_flag(f) == (f.get_func_name() in IMG_SHARDS_FUNCS) for _, f, _ in dm.calls())
        sums = [t for t, f, _ in dm.calls() if f.get_func_name() in ("hip_bconv_filts", "hip_bconv_biases")]
        assert sorted(set(sums)) == ["a_bck", "b_bck", "fc_bck"] and len(sums) == 6      # of ten on the unfrozen step
        bp = d1.bp
        gets = [n for n, d in bp.nodes.items() if n in d1.vars and (n == "loss" or (d.names and d.names[0] == "img") or n.endswith(("_filts_grad_loss", "_biases_grad_loss")))]
        assert "stem_grad_loss" not in gets and "a_filts_grad_loss" in gets and "a_grad_loss" in gets
        for seed, (data, label) in ((5, T.P.small_inputs(cp, 20)), (6, T.P.small_inputs(cp, 21))):
            outs = []
            for d in (d1, dm):
                for v in gets:
                    d.rtc.copy_nda_to_var(v, np.full(bp.nodes[v].sizes, np.nan, np.float32))
                d.set_det_drop_seed(seed)
                fwd = {"data": data, "label": label}
                d.run_bck(["data", "label"], fwd, gets)
                outs.append(fwd)
            one, many = outs
            grads = {}
            for c in d1.bck_calls:
                if c.fop.get_func_name() in ("hip_bconv_filts", "hip_bconv_biases"):
                    an = sref.grad_arg(c.fop)
                    grads[c.args[an]] = sref.sharded_grad(hip, c.fop, {a: hip.copy_var_to_nda(c.args[a]) for a in c.args if a != an}, 2)
            assert len(grads) == 6
            for v in gets:
                assert np.all(np.isfinite(many[v])), v
                assert sref.bits_eq(many[v], grads[v] if v in grads else one[v]), (seed, v)
    finally:
        d1.release(); dm.release(); multi.close()


# ---- the frozen BatchNorm step
@pytest.mark.parametrize("seed", R.RES_SEEDS)
def test_frozen_step_against_float64(hip, seed):
    worst = T.check_frozen_step_against_f64(hip, seed, "be=hip")
    assert worst <= 10 * Z.FROZEN_DEV_CPU and worst <= Z.CAP


def test_frozen_step_call_by_call(hip, cpu):
    """Every call of the frozen step against be=cpu on the GPU's own inputs, bit for bit; the hip_bnf_* functions with their in-place binding."""
    drv, bp, params, data, label, fwd = T.frozen_res_step(hip, R.RES_SEEDS[1])
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
            assert hip.last_launch()["kernel"] in ("bodahip_bnf_prep", "bodahip_bn_sum", "bodahip_bn_fwd", "bodahip_fan_out")
            got = {an: hip.copy_var_to_nda(c.rfc.arg_map[an].n) for an, io in spec if io != "IN"}
            bind = {"in_grad_loss": "out_grad_loss"} if fn == "hip_bnf_bck" else None
            assert bind is None or c.rfc.arg_map["in_grad_loss"].n == c.rfc.arg_map["out_grad_loss"].n
            want = R.run_func(cpu, c.fop, ins, bind=bind)[0]
            for an in got:
                assert R.same_bits(got[an], want[an]), (c.tag, fn, an)
            seen.append(fn)
        hip.release_per_call_id_data()
        assert len(seen) == len(drv.calls()) and all(seen.count(f) == k for f, k in (("hip_bnf_prep", 8), ("hip_bn_fwd", 8), ("hip_bnf_bck", 8), ("hip_fan_out", 2), ("hip_bn_stats", 0), ("hip_bn_bck_in", 0)))
        for n in fwd:     # stepping through the calls one by one is the same step, the running pair included: it is only read
            if n.endswith("_grad_loss") or n == "loss" or n in params:
                assert R.same_bits(hip.copy_var_to_nda(n), fwd[n]), n
    finally:
        drv.release()


def test_frozen_scale_call_by_call(hip, cpu):
    """hip_bnf_bck_in in the driver (both Scale params frozen), in place, against be=cpu on the GPU's own inputs."""
    cp = R.residual(); bp = add_bck_ops(cp)
    drv = ConvPipeBck(hip, freeze=Freeze(params=("scale", "bias"), bn_global_stats=True)); drv.init(bp, R.res_params(cp, 1))
    try:
        fwd = dict(zip(("data", "label"), R.res_inputs(cp, 7)))
        drv.run_bck(["data", "label"], fwd, ["loss"])
        hip.copy_nda_to_var("data", fwd["data"]); hip.copy_nda_to_var("label", fwd["label"])
        n = 0
        for c in drv.bck_calls:
            spec = pipe_func_args(c.fop)
            ins = {an: hip.copy_var_to_nda(c.rfc.arg_map[an].n) for an, io in spec if io in ("IN", "INOUT")}
            hip.run(c.rfc); hip.finish_and_sync()
            if c.fop.get_func_name() == "hip_bnf_bck_in":
                assert c.rfc.arg_map["in_grad_loss"].n == c.rfc.arg_map["out_grad_loss"].n and hip.last_launch()["kernel"] == "bodahip_bnf_bck_in"
                want = R.run_func(cpu, c.fop, ins, bind={"in_grad_loss": "out_grad_loss"})[0]
                assert R.same_bits(hip.copy_var_to_nda(c.rfc.arg_map["in_grad_loss"].n), want["in_grad_loss"]), c.tag
                n += 1
        hip.release_per_call_id_data()
        assert n == 8
    finally:
        drv.release()


def test_running_pair_keeps_its_bits(hip):
    T.check_running_pair_after_three_steps(hip)


def test_eval_over_a_frozen_driver(hip):
    T.check_eval_over_a_frozen_driver(hip)


# ---- graph
def test_graph_replays_of_the_frozen_step(hip, hip2):
    """The frozen residual step (a fixed stem, every BatchNorm on its running pair, a learning-rate schedule) as a serial and as a parallel graph replay against the eager
    step, two steps each: every var the driver holds bit for bit."""
    cp = R.residual()
    mk = lambda: Solver(type="sgd", lr=0.05, momentum=0.9, weight_decay=5e-4, lr_policy=LrPolicy(policy="step", gamma=0.5, stepsize=1))
    fz = Freeze(params=T.STEM, bn_global_stats=True)
    G = ConvPipeBck(hip, solver=mk(), freeze=fz, seed_in_var=True); G.init(add_bck_ops(cp), R.res_params(cp, 1))
    E = ConvPipeBck(hip2, solver=mk(), freeze=fz); E.init(add_bck_ops(cp), R.res_params(cp, 1))
    try:
        gets = [v for v in E.vars if v not in ("data", "label")]
        assert set(gets) <= set(G.vars) and "stem_grad_loss" not in gets and "scale_a_2b_scale_sgd_hist" in gets and "stem_filts_sgd_hist" not in gets
        inp = 11
        for parallel in (False, True):
            before = {s: hip.copy_var_to_nda(s) for s in list(cp.params)}
            assert G.capture_graph(parallel=parallel) == len(G.calls())
            for s in before:     # a capture leaves the params and the running pair as they were
                assert R.same_bits(hip.copy_var_to_nda(s), before[s]), ("capture_graph changed", s)
            for _ in range(2):
                data, label = R.res_inputs(cp, inp); inp += 1
                outs = []
                for d, graph in ((G, True), (E, False)):
                    fwd = {"data": data, "label": label}
                    d.run_bck(["data", "label"], fwd, gets, graph=graph)
                    outs.append(fwd)
                for vn in gets:
                    assert R.same_bits(np.asarray(outs[0][vn], np.float32), np.asarray(outs[1][vn], np.float32)) if outs[0][vn].dtype == np.float32 else np.array_equal(outs[0][vn], outs[1][vn]), (parallel, vn)
        assert G.iter == E.iter == 4
        for s in bn_stat_params(cp):
            assert R.same_bits(hip.copy_var_to_nda(s), R.res_params(cp, 1)[s]), s
    finally:
        G.release(); E.release()
