"""Gradient accumulation without a GPU: hip_grad_accum and hip_solver_update_acc on be=cpu bit for bit against their numpy twins (tests/accum_ref.py), their refusals,
table rows, arg lists and plans, and ConvPipeBck(solver=Solver(...), iter_size=n) on be=cpu -- every pass held to the twins on the backend's own recorded gradients."""
import os

import numpy as np
import pytest

import accum_ref as A
import bn_ref as R
import solver_ref as V
from boda_amd import rtc as rtc_mod
from boda_amd.bck_pipe import GRAD_ACC_SFX, SOLVER_ACCUM_VAR, SOLVER_HYPER_VAR, SOLVER_STATE_VAR, ConvPipeBck, LrPolicy, SgdSolver, Solver, add_bck_ops, bn_stat_params
from boda_amd.cnn_op import ACCUM_OP_FUNCS, NATIVE_ARGS, SOLVER_OP_FUNCS, grad_accum_func_op, pipe_func_args, solver_update_acc_func_op, solver_update_func_op
from boda_amd.op import Dims, Nda, Op, RtErr, UnsupErr, parse_op, read_ops
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


# ---- 1. the two functions
@pytest.mark.parametrize("sizes", A.ACCUM_CASES, ids=lambda s: f"n{len(s)}_{s[0]}")
def test_cpu_accum_first_add_add(cpu, sizes):
    A.check_accum_three_calls(cpu, sizes)


def test_cpu_accum_special_values(cpu):
    A.check_accum_special_values(cpu)


@pytest.mark.parametrize("form", V.FORMS, ids=V.form_id)
@pytest.mark.parametrize("sizes", A.UPDATE_CASES, ids=lambda s: f"n{len(s)}_{s[0]}")
def test_cpu_update_acc(cpu, sizes, form):
    A.check_update_acc(cpu, sizes, form)


# ---- 2. refusals, tables, arg lists, plans
def bad_op(f, strs=None, **nda):
    b = f.copy()
    for k, v in nda.items():
        if v is None:
            b.nda_vals.pop(k)
        else:
            b.nda_vals[k] = v
    b.str_vals.update(strs or {})
    return b


def test_refusals_of_the_op(cpu):
    d = Dims.make("float", v=7)
    u32 = lambda v: Nda(None, "uint32_t", (v,))
    fv = lambda n, tn="float": Nda(dims=Dims.make(tn, v=n), tn=tn)
    for mk in (grad_accum_func_op, lambda ds: solver_update_acc_func_op(ds, "adam")):
        with pytest.raises(RtErr, match="1 to 32 tensors"):
            mk([])
        with pytest.raises(RtErr, match="1 to 32 tensors"):
            mk([d] * 33)
    with pytest.raises(RtErr, match="solver_type must be sgd | nesterov | adam".replace("|", r"\|")):
        solver_update_acc_func_op([d], "rmsprop")
    with pytest.raises(RtErr, match="decoupled_wd"):
        solver_update_acc_func_op([d], "nesterov", decoupled_wd=True)
    ga, ua = grad_accum_func_op([d, d]), solver_update_acc_func_op([d, d], "adam", clip=True)
    cases = [
        (bad_op(ga, tens_num=u32(0)), "tens_num=0: 1 to 32 tensors"),
        (bad_op(ga, tens_num=u32(33)), "tens_num=33: 1 to 32 tensors"),
        (bad_op(ua, tens_num=u32(0)), "tens_num=0: 1 to 32 tensors"),
        (bad_op(ua, tens_num=u32(33)), "tens_num=33: 1 to 32 tensors"),
        (bad_op(ga, a_1=fv(8)), "a_1 dims .* differ from g_1's"),
        (bad_op(ga, a_1=None), "the op has no 'a_1'"),
        (bad_op(ga, g_0=fv(7, "uint32_t")), "g_0 has type uint32_t"),
        (bad_op(ga, a_0=fv(7, "uint32_t")), "a_0 has type uint32_t"),
        (bad_op(ga, accum=fv(3)), "accum must be float v=4"),
        (bad_op(ga, accum=fv(4, "uint32_t")), "accum must be float v=4"),
        (bad_op(ga, accum=None), "the op has no 'accum'"),
        (bad_op(ua, accum=fv(8)), "accum must be float v=4"),
        (bad_op(ua, accum=None), "the op has no 'accum'"),
        (bad_op(ua, {"solver_type": "adagrad"}), "solver_type must be sgd"),
        (bad_op(ua, h2_1=None), "the op has no 'h2_1'"),
        (bad_op(ua, g_1=fv(8)), "g_1 dims .* differ from w_1's"),
        (bad_op(ua, hyper=fv(4)), "hyper must be float v=8"),
        (bad_op(ua, state=fv(3)), "state must be float v=4"),
        (bad_op(ua, clip=u32(2)), "clip must be 0 | 1".replace("|", r"\|")),
    ]
    for f in (ga, ua):
        fn = f.get_func_name()
        cases += [(bad_op(f, img_shards=u32(1)), f"img_shards=1 on '{fn}'"), (bad_op(f, seed_from_var=u32(1)), f"seed_from_var=1 on '{fn}'"),
                  (bad_op(f, zero_if_in_non_pos=u32(1)), f"zero_if_in_non_pos=1 on '{fn}'")]
        wrong = f.copy(); wrong.str_vals["type"] = "Reduce"
        cases.append((wrong, f"a function of op type {f.get_type()}"))
    for bad, msg in cases:
        with pytest.raises(RtErr, match=msg):
            cpu.compile([RtcFuncInfo("bad", "", [a for a, _ in pipe_func_args(ua)], bad)])
        if bad.get_type() != "Reduce":
            with pytest.raises(RtErr, match=msg):
                rtc_mod.explain_plan(bad)
    for f in (ga, ua):     # compiling an op without tens_num stays an error; asking for its arg list answers the fixed args
        with pytest.raises(RtErr, match="the op has no 'tens_num'"):
            cpu.compile([RtcFuncInfo("bad", "", [a for a, _ in pipe_func_args(ua)], bad_op(f, tens_num=None))])
    for mk in (grad_accum_func_op, lambda ds: solver_update_acc_func_op(ds, "sgd")):
        with pytest.raises(UnsupErr, match="2 GiB"):
            rtc_mod.explain_plan(mk([Dims.make("float", v=536870912)]))


def test_refusals_of_the_call(cpu):
    d = Dims.make("float", v=8)
    for f, pairs in ((grad_accum_func_op([d, d]), (("g_0", "a_0"), ("a_0", "a_1"), ("g_0", "g_1"), ("g_1", "a_0"))),
                     (solver_update_acc_func_op([d, d], "adam", clip=True), (("w_0", "g_0"), ("h_0", "h2_0"), ("h2_0", "h2_1"), ("w_1", "g_0")))):
        spec = pipe_func_args(f)
        order = [a for a, _ in spec]
        cpu.compile([RtcFuncInfo("acc_r", "", order, f)])
        made = []
        try:
            for an, _ in spec:
                cpu.create_var_with_dims("rv_" + an, f.get_dims(an)); made.append("rv_" + an)
                cpu.copy_nda_to_var("rv_" + an, np.ones(f.get_dims(an).sizes, F))
            for vn, dims in (("rv_u32", Dims.make("uint32_t", v=8)), ("rv_nine", Dims.make("float", v=9)), ("rv_four", Dims.make("float", v=4))):
                cpu.create_var_with_dims(vn, dims); made.append(vn)
            good = {an: RtcArg.var("rv_" + an) for an, _ in spec}
            run = lambda **kw: cpu.run(RtcFuncCall("acc_r", dict(good, **{k: RtcArg.var(v) for k, v in kw.items()})))
            with pytest.raises(RtErr, match="arg 'accum' not found"):
                cpu.run(RtcFuncCall("acc_r", {k: v for k, v in good.items() if k != "accum"}))
            with pytest.raises(RtErr, match="arg 'g_1' not found"):
                cpu.run(RtcFuncCall("acc_r", {k: v for k, v in good.items() if k != "g_1"}))
            with pytest.raises(RtErr, match="arg 'g_0' .* has type uint32_t"):
                run(g_0="rv_u32")
            with pytest.raises(RtErr, match="arg 'g_1' has dims .*, the op says"):
                run(g_1="rv_nine")
            with pytest.raises(RtErr, match="arg 'accum' has dims .*, the op says"):
                run(accum="rv_nine")
            for a, b in pairs:     # any two of the call's vars being one var
                first, second = (a, b) if order.index(a) < order.index(b) else (b, a)
                with pytest.raises(RtErr, match=f"args '{first}' and '{second}' are the same var 'rv_{first}'"):
                    run(**{second: "rv_" + first})
            cpu.run(RtcFuncCall("acc_r", good))
            assert np.all(cpu.copy_var_to_nda("rv_g_0") == 1.0)
        finally:
            for vn in made:
                cpu.release_var(vn)
            cpu.release_func("acc_r"); cpu.release_per_call_id_data()


def new_func_ops():
    d = [Dims.make("float", v=9000), Dims.make("float", a=3, b=5)]
    ops = [solver_update_acc_func_op(d, t, [1, 2], [1, 0], clip=c, decoupled_wd=w) for t, c, w in V.FORMS]
    return ops + [solver_update_acc_func_op([d[1]] * 32, "adam"), grad_accum_func_op(d), grad_accum_func_op([d[1]] * 32)]


def fixture_ops():
    d = [Dims.make("float", out_chan=8, in_chan=3, y=3, x=3), Dims.make("float", out_chan=8)]
    return [grad_accum_func_op(d)] + [solver_update_acc_func_op(d, t, [1, 2], [1, 0], clip=c, decoupled_wd=w) for t, c, w in V.FORMS]     # (every kernel of the two functions)


def test_tables_arg_lists_and_plans():
    assert ACCUM_OP_FUNCS == {"GradAccum": ("hip_grad_accum",), "SolverUpdateAcc": ("hip_solver_update_acc",)}
    assert SOLVER_OP_FUNCS == {"SolverUpdate": ("hip_solver_update",), "GradSumsq": ("hip_grad_sumsq",), "GradNorm": ("hip_grad_norm",)}     # (pinned: the new two have a table of their own)
    table = rtc_mod.native_funcs()
    for member, (t, (fn,)) in enumerate(ACCUM_OP_FUNCS.items(), 4):
        r = table[fn]
        assert (r["family"], r["member"], r["types"], r["multi_dev"], r["be"], r["flags"], r["opt"], r["why"]) == ("solver", member, (t,), "replicated_vars", ("hip", "cpu"), (), (), ""), fn
    assert NATIVE_ARGS["hip_grad_accum"] == (("accum", "IN"),) and NATIVE_ARGS["hip_solver_update_acc"] == (("hyper", "IN"), ("state", "IN"), ("accum", "IN"))
    gold = read_ops(os.path.join(HERE, "golden", "ops", "accum-ops.txt"))
    assert [o.to_str() for o in gold] == [o.to_str() for o in fixture_ops()]
    for f in new_func_ops() + gold:
        assert rtc_mod.func_args(f) == pipe_func_args(f), f.to_str()
        assert parse_op(f.to_str()).to_str() == f.to_str() and rtc_mod.parse_op_native(f.to_str()) == f.to_str()
        assert f.flops() == 0
    for fn in ACCUM_OP_FUNCS["GradAccum"] + ACCUM_OP_FUNCS["SolverUpdateAcc"]:     # the arg-list query of a bare op: the fixed args alone
        assert rtc_mod.func_args(Op({"type": table[fn]["types"][0], "func_name": fn}, {})) == NATIVE_ARGS[fn]
    d = [Dims.make("float", v=9000), Dims.make("float", a=3, b=5)]
    ga, ad, ne = grad_accum_func_op(d), solver_update_acc_func_op(d, "adam", clip=True), solver_update_acc_func_op(d, "nesterov")
    assert pipe_func_args(ga) == (("g_0", "IN"), ("a_0", "INOUT"), ("g_1", "IN"), ("a_1", "INOUT"), ("accum", "IN"))
    assert pipe_func_args(ad)[:8] == pipe_func_args(solver_update_func_op(d, "adam", clip=True))[:8] and pipe_func_args(ad)[8:] == (("hyper", "IN"), ("state", "IN"), ("accum", "IN"))
    assert [a for a, _ in pipe_func_args(ne)] == ["w_0", "g_0", "h_0", "w_1", "g_1", "h_1", "hyper", "state", "accum"]
    assert (ga.algo_bytes(), ad.algo_bytes(), ne.algo_bytes()) == (12 * 9015, 28 * 9015, 20 * 9015)
    assert rtc_mod.explain_plan(ga) == "bodahip_grad_accum grid=4 block=256 tens=2 chunk=4096"
    assert rtc_mod.explain_plan(ad) == "bodahip_solver_update_adam grid=4 block=256 tens=2 chunk=4096 clip=1 decoupled_wd=0 accum=1"
    assert rtc_mod.explain_plan(ne) == "bodahip_solver_update_nesterov grid=4 block=256 tens=2 chunk=4096 clip=0 accum=1"
    assert rtc_mod.explain_plan(solver_update_func_op(d, "nesterov")) == "bodahip_solver_update_nesterov grid=4 block=256 tens=2 chunk=4096 clip=0"     # (the update's own line stays)
    for f in (ga, ad, ne):
        assert rtc_mod.prebuild(f) > 0      # cross-compiles for gfx950


# ---- 3. the driver
@pytest.mark.parametrize("form", V.FORMS, ids=V.form_id)
@pytest.mark.parametrize("name", ["chain", "fan"])
def test_cpu_six_passes_are_the_twins(cpu, name, form):
    packed = A.six_passes(cpu, name, A.mk_solver(form, 32))
    three = A.six_passes(cpu, name, A.mk_solver(form, 3))     # a last call with fewer tensors than the others
    assert set(packed) == set(three)
    for vn in packed:
        assert V.same_bits(packed[vn], three[vn]), vn


def test_cpu_step_policy_boundary_between_the_two_updates(cpu):
    pol = LrPolicy(policy="step", gamma=0.5, stepsize=1)     # update 0 (passes 0 .. 2) at 0.05, update 1 (passes 3 .. 5) at 0.025: passes() checks the words at every pass
    assert [pol.lr_at(0.05, k) for k in range(2)] == [0.05, 0.025]
    A.six_passes(cpu, "chain", A.mk_solver(("adam", True, False), policy=pol))
    A.six_passes(cpu, "chain", A.mk_solver(("nesterov", False, False), policy=pol))


def test_cpu_calls_vars_skip_and_reset(cpu):
    sv = A.mk_solver(("adam", True, False), 3)
    drv, bp = V.make_driver(cpu, "chain", sv, iter_size=3)
    try:
        pn = drv.sgd_params
        tail = drv.calls()[-drv.n_sgd_calls:]
        assert [t for t, _, _ in tail] == ["grad_accum_0", "grad_accum_1", "grad_sumsq_0", "grad_sumsq_1", "grad_norm", "solver_update_0", "solver_update_1"] and drv.n_sgd_calls == 7
        assert [f.get_func_name() for _, f, _ in tail] == ["hip_grad_accum"] * 2 + ["hip_grad_sumsq"] * 2 + ["hip_grad_norm"] + ["hip_solver_update_acc"] * 2
        assert {k: v.n for k, v in tail[1][2].items()} == {"g_0": "fc_biases_grad_loss", "a_0": "fc_biases_grad_acc", "accum": SOLVER_ACCUM_VAR}
        assert {k: v.n for k, v in tail[3][2].items()} == {"g_0": "fc_biases_grad_acc", "partials": "solver_gnorm_partials"}
        assert {k: v.n for k, v in tail[6][2].items()} == {"w_0": "fc_biases", "g_0": "fc_biases_grad_acc", "h_0": "fc_biases_sgd_hist", "h2_0": "fc_biases_sgd_hist2",
                                                         "hyper": SOLVER_HYPER_VAR, "state": SOLVER_STATE_VAR, "accum": SOLVER_ACCUM_VAR}
        assert cpu.get_var_dims(SOLVER_ACCUM_VAR) == Dims(("v",), (4,), "float") and all(cpu.get_var_dims(p + GRAD_ACC_SFX) == bp.cp.params[p] for p in pn)
        # the declared directions order them: every accumulate behind its gradients' writers, every sumsq behind its accumulate, the updates behind the norm
        deps, n = drv._call_deps(), len(drv.bck_calls)
        reach = []
        for d in deps:
            r = set(d)
            for j in d:
                r |= reach[j]
            reach.append(r)
        assert (n - 7) in reach[n - 5] and (n - 6) in reach[n - 4] and {n - 5, n - 4} <= reach[n - 3] and {n - 3, n - 7} <= reach[n - 2] and {n - 3, n - 6} <= reach[n - 1]
        assert all(deps[i] and max(deps[i]) < n - 7 for i in (n - 7, n - 6))     # an accumulate waits for gradient ops only
        A.passes(cpu, drv, bp, 2)
        assert (drv.micro, drv.iter) == (2, 0)
        accs = V.fetch(cpu, [p + GRAD_ACC_SFX for p in pn])
        drv.run_device_only(skip_sgd=True)     # a pass without the solver's calls moves neither micro nor an accumulator
        assert (drv.micro, drv.iter) == (2, 0)
        for vn, a in accs.items():
            assert A.bits_equal(cpu.copy_var_to_nda(vn), a), vn
        drv.zero_sgd_history()
        assert (drv.micro, drv.iter) == (0, 0)
        A.passes(cpu, drv, bp, 3)     # (the stale accumulators do not matter: the first micro-step overwrites them)
        assert (drv.micro, drv.iter) == (0, 1)
    finally:
        drv.release()
    for bad, msg in ((dict(solver=SgdSolver(lr=0.1), iter_size=2), r'Solver\(type="sgd"'), (dict(iter_size=2), r'Solver\(type="sgd"'), (dict(solver=sv, iter_size=0), "iter_size"),
                     (dict(solver=sv, iter_size=-3), "iter_size")):
        with pytest.raises(RtErr, match=msg):
            ConvPipeBck(cpu, **bad)


@pytest.mark.parametrize("form", [("sgd", False, False), ("adam", True, False)], ids=V.form_id)
def test_cpu_iter_size_one_is_the_driver_without_the_keyword(cpu, form):
    one, bp = V.make_driver(cpu, "chain", A.mk_solver(form, 3), iter_size=1)
    try:
        calls_one, vars_one = [(t, f.to_str(), {k: v.n for k, v in am.items() if hasattr(v, "n")}) for t, f, am in one.calls()], list(one.vars)
    finally:
        one.release()
    old, _ = V.make_driver(cpu, "chain", A.mk_solver(form, 3))
    try:
        assert [(t, f.to_str(), {k: v.n for k, v in am.items() if hasattr(v, "n")}) for t, f, am in old.calls()] == calls_one and list(old.vars) == vars_one
        assert SOLVER_ACCUM_VAR not in vars_one and not any(v.endswith(GRAD_ACC_SFX) for v in vars_one)
    finally:
        old.release()
    a = V.three_steps(cpu, "chain", A.mk_solver(form, 3), iter_size=1)
    b = V.three_steps(cpu, "chain", A.mk_solver(form, 3))
    assert set(a) == set(b) and all(A.bits_equal(a[vn], b[vn]) for vn in a)


def test_cpu_batchnorm_pipe_with_adam_and_iter_size_two(cpu):
    """The small residual pipe of tests/test_bn_cpu.py: four passes, two updates; the running statistics move on every pass, by the forward pass alone."""
    sv = Solver(type="adam", lr=0.01, clip_gradients=0.5, lr_mult={"biases": 2.0, "scale": 0.5}, decay_mult={"biases": 0.0, "bias": 0.0, "scale": 0.0})
    cp = R.residual(); bp = add_bck_ops(cp)
    drv = ConvPipeBck(cpu, solver=sv, bn_maf=0.9, iter_size=2); drv.init(bp, R.res_params(cp, 1))
    try:
        stats = bn_stat_params(cp)
        assert drv.sgd_params == [p for p in cp.params if p not in stats] and not any(s + GRAD_ACC_SFX in drv.vars for s in stats)
        seen = []
        before = V.fetch(cpu, stats)

        def inputs(cp_, k):
            seen.append(V.fetch(cpu, stats))
            return R.res_inputs(cp_, 100 + k)
        A.passes(cpu, drv, bp, 4, inputs=inputs)
        assert drv.iter == 2
        seen.append(V.fetch(cpu, stats))
        for k in range(4):
            assert all(not A.bits_equal(seen[k][s], seen[k + 1][s]) for s in stats if s.endswith("_mean")), k
        assert all(A.bits_equal(before[s], seen[0][s]) for s in stats)
    finally:
        drv.release()


# ---- 4. meaning
def test_cpu_meaning_two_halves_are_one_batch(cpu):
    dev = A.meaning_dev(cpu)
    print("one sgd step at batch %d against iter_size=2 at batch %d: largest relative difference of the params %.3e (recorded %.3e)" % (2 * A.MEANING_B, A.MEANING_B, dev, A.MEANING_DEV_CPU))
    assert dev <= A.MEANING_DEV_CPU
    assert dev < 1e-5     # and that is rounding, not another update: one step moves a param by lr * gradient, around 1e-2 of its size
