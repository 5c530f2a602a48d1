"""The solver family without a GPU: hip_solver_update, hip_grad_sumsq and hip_grad_norm on be=cpu bit for bit against the numpy twins of their written chains
(tests/solver_ref.py), their refusals, tables, arg lists and plans, LrPolicy against its written formulas, and ConvPipeBck(solver=Solver(...)) on be=cpu -- every step
held to the twins on the backend's own values, a BatchNorm pipe with adam, and two descent runs on `chain` against float64 trajectories.

Descent (solver_ref.DESCENT): fixed data / label / dropout seed; the float64 loss at least halves; be=cpu's largest deviation from the float64 loss is recorded in
solver_ref.DESCENT_DEV_CPU, and the bound both backends are held to is that times 10, the margin being for the GPU's different K-slice summation order in the filter
gradients."""
import math
import os

import numpy as np
import pytest

import bn_ref as R
import sgd_ref as S
import solver_ref as V
from boda_amd import rtc as rtc_mod
from boda_amd.bck_pipe import (SGD_HIST2_SFX, SGD_HIST_SFX, SOLVER_HYPER_VAR, SOLVER_PARTS_VAR, SOLVER_STATE_VAR, ConvPipeBck, LrPolicy, SgdSolver, Solver, add_bck_ops,
                               bn_stat_params)
from boda_amd.cnn_op import (NATIVE_ARGS, SGD_OP_FUNCS, SOLVER_OP_FUNCS, grad_norm_func_op, grad_sumsq_func_op, pipe_func_args, sgd_update_func_op,
                             solver_update_func_op)
from boda_amd.op import Dims, Nda, Op, RtErr, UnsupErr, parse_op, read_ops
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [[n] for n in S.SIZES] + [S.MIXED_32]
STATE = np.array([0.37, 9.0, 81.0, 0.0], F)     # what the update reads with clip=1: coef = 0.37
HYPERS = [V.hyper8(0.01, 0.9, 5e-4, 0.999, 1e-8, V.corr_f64(0.9, 0.999, 1)), V.hyper8(0.5, 0.25, 0.125, 0.5, 1e-3, V.corr_f64(0.25, 0.5, 2)),
          V.hyper8(0.02, 0.0, 0.0, 0.9, 1e-8, V.corr_f64(0.0, 0.9, 3))]     # three calls, hyper rewritten in between


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


def mults(n):
    return [float(1 + i % 2) for i in range(n)], [float((i + 1) % 2) for i in range(n)]


# ---- 1. the update function
@pytest.mark.parametrize("form", V.FORMS, ids=V.form_id)
@pytest.mark.parametrize("sizes", CASES, ids=lambda s: f"n{len(s)}_{s[0]}")
def test_cpu_update_against_numpy(cpu, sizes, form):
    lm, dm = mults(len(sizes))
    ins = V.make_inputs(sizes)
    got, guards = V.run_update(cpu, sizes, form, lm, dm, HYPERS, ins, STATE, guards=True)
    want = V.want_update(form, lm, dm, HYPERS, ins, STATE)
    for i, (g_, w_) in enumerate(zip(got, want)):
        assert S.same_bits(g_[1], ins[i][1].reshape(-1)) or (np.isnan(ins[i][1]).any() and V.same_bits(g_[1], ins[i][1])), (i, "g was written")
        for k, nm in ((2, "history"), (3, "second history"), (0, "param")):
            assert V.same_bits(g_[k], w_[k]), (i, sizes[i], nm)
    if sizes[0] >= 10:     # the special values did what they are there for
        w, g, h, h2 = want[0]
        assert np.isnan(w[7]) and np.isfinite(w[5]) and np.isfinite(w[6])
    for vn, a in guards.items():
        assert np.array_equal(a.view(np.uint32), np.full(4, V.GUARD_BITS, np.uint32)), (vn, "an element outside the tensors changed")


def test_special_values_reach_the_branches_they_are_for():
    """On the twin: q = g1 * g1 is a denormal at [5], zero at [8] and inf at [6], where r = m' / inf = 0 leaves w' = w (no decoupled decay)."""
    (w, g, h, h2), = V.make_inputs([4097])
    hy = HYPERS[0]
    with np.errstate(all="ignore"):
        q = (g + F(hy[2]) * w) * (g + F(hy[2]) * w)
    assert 0 < q[5] < np.finfo(F).tiny and q[8] == 0 and np.isinf(q[6]) and np.isnan(q[7])
    w2, m, v = V.solver_np("adam", w, g, h, h2, hy)
    assert np.isinf(v[6]) and w2[6] == w[6] and np.isnan(w2[7]) and np.isnan(m[7]) and np.isnan(v[7])
    assert 0 < v[5] < np.finfo(F).tiny     # momentum2 * 1e-44 + (1 - momentum2) * q stays a denormal


@pytest.mark.parametrize("sizes", CASES, ids=lambda s: f"n{len(s)}_{s[0]}")
def test_cpu_sgd_form_leaves_hip_sgd_update_s_bits(cpu, sizes):
    lm, dm = mults(len(sizes))
    ins = V.make_inputs(sizes)
    hy = [h for h in HYPERS]
    got, _ = V.run_update(cpu, sizes, ("sgd", False, False), lm, dm, hy, ins, STATE)
    old, _ = S.run_sgd(cpu, sizes, lm, dm, [tuple(h[:3]) for h in hy], [t[:3] for t in ins])
    for i in range(len(sizes)):
        for k in (0, 2):
            assert V.same_bits(got[i][k], old[i][k]) and (np.isnan(old[i][k]).any() or S.same_bits(got[i][k], old[i][k])), (i, k)


# ---- 2. the norm
NORM_SIZES = [1, 255, 256, 257, 4095, 4096, 4097, 9000]
BIG = 4096 * 257 + 5     # 258 partials: the finish's lanes 0 and 1 chain two terms


def norm_grads(kind, seed=0):
    rng = np.random.default_rng([seed, 91])
    gs = [rng.uniform(-1, 1, n).astype(F) for n in NORM_SIZES]
    if kind == "zero":
        gs = [np.zeros(n, F) for n in NORM_SIZES]
    elif kind == "nan":
        gs[6][4096] = np.nan
    elif kind == "inf":
        gs[7][8999] = -np.inf
    return gs


def norm_case(rtc, kind, clip, keep=None):
    """Two hip_grad_sumsq calls with different part0 into one partials var that has two slots in front and one behind them which no call owns."""
    gs = norm_grads(kind)
    a, b = gs[:5], gs[5:]
    ca, cb = sum(-(-g.size // 4096) for g in a), sum(-(-g.size // 4096) for g in b)
    total = 2 + ca + cb + 1
    prefill = np.full(total, 0.5, F)
    calls = [(2 + ca, b), (2, a)]     # the later slots first: the order of the calls does not matter
    got = V.run_norm(rtc, calls, total, prefill, clip, keep)
    want = V.want_norm(calls, prefill, clip)
    return got, want, (ca, cb, total)


@pytest.mark.parametrize("kind,clip", [("plain", 1e6), ("plain", 1.0), ("zero", 1.0), ("nan", 1.0), ("inf", 1.0)], ids=lambda x: str(x))
def test_cpu_norm_against_numpy(cpu, kind, clip):
    (seen, state), (wseen, wstate), (ca, cb, total) = norm_case(cpu, kind, clip)
    for s, w in zip(seen, wseen):
        assert V.same_bits(s, w)
    assert np.all(seen[0][:2 + ca] == 0.5) and seen[0][-1] == 0.5 and np.all(seen[1][[0, 1, -1]] == 0.5)     # slots outside a call's range are untouched
    assert V.same_bits(state, wstate), (state, wstate)
    coef, norm = state[0], state[1]
    if kind == "plain" and clip == 1e6:
        assert norm < clip and coef.view(np.uint32) == F(1.0).view(np.uint32)
    elif kind == "plain":
        assert norm > clip and 0 < coef < 1
    elif kind == "nan":
        assert np.isnan(norm) and coef == 1.0
    elif kind == "inf":
        assert np.isinf(norm) and coef == 0.0 and not np.signbit(coef)


def test_cpu_norm_three_four_five_and_big(cpu):
    g = np.array([3.0, 4.0], F)
    (seen,), state = V.run_norm(cpu, [(0, [g])], 1, np.zeros(1, F), 5.0)
    assert seen[0] == 25.0 and list(state) == [1.0, 5.0, 25.0, 0.0]     # norm == clip: coef is 1
    (seen,), state = V.run_norm(cpu, [(0, [g])], 1, np.zeros(1, F), 2.5)
    assert list(state) == [0.5, 5.0, 25.0, 0.0]
    big = np.random.default_rng(3).uniform(-1, 1, BIG).astype(F)
    (seen,), state = V.run_norm(cpu, [(0, [big])], 258, np.zeros(258, F), 10.0)
    (wseen,), wstate = V.want_norm([(0, [big])], np.zeros(258, F), 10.0)
    assert seen.size == 258 and V.same_bits(seen, wseen) and V.same_bits(state, wstate)
    assert abs(float(state[2]) - float(np.sum(big.astype(np.float64) ** 2))) <= 1e-5 * float(state[2])     # and the chain is a sum of squares


# ---- 3. refusals and tables
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
    with pytest.raises(RtErr, match="solver_type must be sgd | nesterov | adam".replace("|", r"\|")):
        solver_update_func_op([d], "rmsprop")
    for mk in (lambda ds: solver_update_func_op(ds, "adam"), lambda ds: grad_sumsq_func_op(ds, 0, 64)):
        with pytest.raises(RtErr, match="1 to 32 tensors"):
            mk([])
        with pytest.raises(RtErr, match="1 to 32 tensors"):
            mk([d] * 33)
    with pytest.raises(RtErr, match="decoupled_wd"):
        solver_update_func_op([d], "sgd", decoupled_wd=True)
    with pytest.raises(RtErr, match="exceed the 2 partials"):
        grad_sumsq_func_op([d, d], 1, 2)
    up, ss, gn = solver_update_func_op([d, d], "adam", clip=True), grad_sumsq_func_op([d, d], 1, 4), grad_norm_func_op(4)
    cases = [
        (bad_op(up, {"solver_type": "adagrad"}), "solver_type must be sgd"),
        (bad_op(up, tens_num=u32(0)), "tens_num=0: 1 to 32 tensors"),
        (bad_op(up, tens_num=u32(33)), "tens_num=33: 1 to 32 tensors"),
        (bad_op(ss, tens_num=u32(0)), "tens_num=0: 1 to 32 tensors"),
        (bad_op(ss, tens_num=u32(33)), "tens_num=33: 1 to 32 tensors"),
        (bad_op(up, h2_1=None), "the op has no 'h2_1'"),
        (bad_op(solver_update_func_op([d], "nesterov"), {"solver_type": "adam"}), "the op has no 'h2_0'"),     # a missing h2 for adam
        (bad_op(up, g_1=fv(8)), "g_1 dims .* differ from w_1's"),
        (bad_op(up, h2_0=fv(7, "uint32_t")), "h2_0 has type uint32_t"),
        (bad_op(ss, g_0=fv(7, "uint32_t")), "g_0 has type uint32_t"),
        (bad_op(up, hyper=fv(4)), "hyper must be float v=8"),
        (bad_op(up, state=fv(3)), "state must be float v=4"),
        (bad_op(gn, state=fv(4, "uint32_t")), "state must be float v=4"),
        (bad_op(up, clip=u32(2)), "clip must be 0 | 1".replace("|", r"\|")),
        (bad_op(up, decay_mult_0=None), "the op has no 'decay_mult_0'"),
        (bad_op(ss, part0=u32(3)), "part0=3 .* exceed the 4 partials"),
        (bad_op(ss, part0=None), "the op has no 'part0'"),
    ]
    for f in (up, ss, gn):
        fn = f.get_func_name()
        cases += [(bad_op(f, img_shards=u32(1)), f"img_shards=1 on '{fn}'"), (bad_op(f, seed_from_var=u32(1)), f"seed_from_var=1 on '{fn}'"),
                  (bad_op(f, zero_if_in_non_pos=u32(1)), f"zero_if_in_non_pos=1 on '{fn}'")]
        wrong = f.copy(); wrong.str_vals["type"] = "Reduce"
        cases.append((wrong, f"a function of op type {f.get_type()}"))
    for bad, msg in cases:
        with pytest.raises(RtErr, match=msg):
            cpu.compile([RtcFuncInfo("bad", "", [a for a, _ in pipe_func_args(up)], bad)])
        if bad.get_type() != "Reduce":
            with pytest.raises(RtErr, match=msg):
                rtc_mod.explain_plan(bad)
    for f in (up, ss):     # compiling an op without tens_num stays an error; asking for its arg list answers the fixed args
        with pytest.raises(RtErr, match="the op has no 'tens_num'"):
            cpu.compile([RtcFuncInfo("bad", "", [a for a, _ in pipe_func_args(up)], bad_op(f, tens_num=None))])


def test_refusals_of_the_call(cpu):
    d = Dims.make("float", v=8)
    f = solver_update_func_op([d, d], "adam", clip=True)
    spec = pipe_func_args(f)
    cpu.compile([RtcFuncInfo("slv_r", "", [a for a, _ in spec], f)])
    made = []
    try:
        for an, _ in spec:
            cpu.create_var_with_dims("rv_" + an, f.get_dims(an)); made.append("rv_" + an)
            cpu.copy_nda_to_var("rv_" + an, np.ones(f.get_dims(an).sizes, F))
        for vn, dims in (("rv_u32", Dims.make("uint32_t", v=8)), ("rv_nine", Dims.make("float", v=9))):
            cpu.create_var_with_dims(vn, dims); made.append(vn)
        good = {an: RtcArg.var("rv_" + an) for an, _ in spec}
        run = lambda **kw: cpu.run(RtcFuncCall("slv_r", dict(good, **{k: RtcArg.var(v) for k, v in kw.items()})))
        with pytest.raises(RtErr, match="arg 'h2_1' not found"):
            cpu.run(RtcFuncCall("slv_r", {k: v for k, v in good.items() if k != "h2_1"}))
        with pytest.raises(RtErr, match="arg 'state' not found"):
            cpu.run(RtcFuncCall("slv_r", {k: v for k, v in good.items() if k != "state"}))
        with pytest.raises(RtErr, match="arg 'h2_0' .* has type uint32_t"):
            run(h2_0="rv_u32")
        with pytest.raises(RtErr, match="arg 'g_0' has dims .*, the op says"):
            run(g_0="rv_nine")
        for a, b in (("w_0", "g_0"), ("w_0", "h2_0"), ("h_0", "h2_0"), ("h2_0", "h2_1"), ("g_0", "g_1"), ("hyper", "w_1")):     # any two of the call's vars being one var
            first, second = (a, b) if [x for x, _ in spec].index(a) < [x for x, _ in spec].index(b) else (b, a)
            with pytest.raises(RtErr, match=f"args '{first}' and '{second}' are the same var 'rv_{first}'"):
                run(**{second: "rv_" + first})
        cpu.run(RtcFuncCall("slv_r", good))
        assert np.all(cpu.copy_var_to_nda("rv_g_0") == 1.0)
    finally:
        for vn in made:
            cpu.release_var(vn)
        cpu.release_func("slv_r"); cpu.release_per_call_id_data()
    # hip_grad_sumsq: g_i and partials; hip_grad_norm: partials / hyper / state
    g4 = Dims.make("float", v=4)
    fs, fn = grad_sumsq_func_op([g4, g4], 0, 4), grad_norm_func_op(4)
    cpu.compile([RtcFuncInfo("ss_r", "", [a for a, _ in pipe_func_args(fs)], fs), RtcFuncInfo("gn_r", "", [a for a, _ in pipe_func_args(fn)], fn)])
    made = []
    try:
        for vn in ("a", "b", "c"):
            cpu.create_var_with_dims("nr_" + vn, g4); made.append("nr_" + vn)
        cpu.create_var_with_dims("nr_hy", Dims.make("float", v=8)); made.append("nr_hy")
        v = RtcArg.var
        with pytest.raises(RtErr, match="args 'g_0' and 'g_1' are the same var 'nr_a'"):
            cpu.run(RtcFuncCall("ss_r", {"g_0": v("nr_a"), "g_1": v("nr_a"), "partials": v("nr_c")}))
        with pytest.raises(RtErr, match="args 'g_1' and 'partials' are the same var 'nr_b'"):
            cpu.run(RtcFuncCall("ss_r", {"g_0": v("nr_a"), "g_1": v("nr_b"), "partials": v("nr_b")}))
        with pytest.raises(RtErr, match="args 'partials' and 'state' are the same var 'nr_a'"):
            cpu.run(RtcFuncCall("gn_r", {"partials": v("nr_a"), "hyper": v("nr_hy"), "state": v("nr_a")}))
    finally:
        for vn in made:
            cpu.release_var(vn)
        cpu.release_func("ss_r"); cpu.release_func("gn_r")


def new_func_ops():
    d = [Dims.make("float", v=9000), Dims.make("float", a=3, b=5)]
    ops = [solver_update_func_op(d, t, [1, 2], [1, 0], clip=c, decoupled_wd=w) for t, c, w in V.FORMS]
    ops += [solver_update_func_op([d[1]] * 32, "adam"), grad_sumsq_func_op(d, 3, 8), grad_sumsq_func_op([d[1]] * 32, 0, 32), grad_norm_func_op(8), grad_norm_func_op(258)]
    return ops


def test_tables_arg_lists_and_plans():
    assert SOLVER_OP_FUNCS == {"SolverUpdate": ("hip_solver_update",), "GradSumsq": ("hip_grad_sumsq",), "GradNorm": ("hip_grad_norm",)}
    assert SGD_OP_FUNCS == {"SgdUpdate": ("hip_sgd_update",)}
    table = rtc_mod.native_funcs()
    for member, (t, (fn,)) in enumerate(SOLVER_OP_FUNCS.items(), 1):
        r = table[fn]
        assert (r["family"], r["member"], r["types"], r["multi_dev"], r["be"], r["flags"], r["opt"], r["why"]) == ("solver", member, (t,), "replicated_vars", ("hip", "cpu"), (), (), ""), fn
    assert NATIVE_ARGS["hip_solver_update"] == (("hyper", "IN"), ("state", "IN")) and NATIVE_ARGS["hip_grad_sumsq"] == (("partials", "INOUT"),)
    assert NATIVE_ARGS["hip_grad_norm"] == (("partials", "IN"), ("hyper", "IN"), ("state", "OUT"))
    gold = read_ops(os.path.join(HERE, "golden", "ops", "solver-ops.txt"))
    assert {o.get_func_name() for o in gold} == set(NATIVE_ARGS) & {"hip_solver_update", "hip_grad_sumsq", "hip_grad_norm"}
    for f in new_func_ops() + gold:
        assert rtc_mod.func_args(f) == pipe_func_args(f), f.to_str()
        assert parse_op(f.to_str()).to_str() == f.to_str() and rtc_mod.parse_op_native(f.to_str()) == f.to_str()
        assert f.flops() == 0
    for fn in ("hip_solver_update", "hip_grad_sumsq"):     # the arg-list query of a bare op: the fixed args alone
        assert rtc_mod.func_args(Op({"type": table[fn]["types"][0], "func_name": fn}, {})) == NATIVE_ARGS[fn]
    d = [Dims.make("float", v=9000), Dims.make("float", a=3, b=5)]
    ad = solver_update_func_op(d, "adam", clip=True)
    assert pipe_func_args(ad)[:8] == (("w_0", "INOUT"), ("g_0", "IN"), ("h_0", "INOUT"), ("h2_0", "INOUT"), ("w_1", "INOUT"), ("g_1", "IN"), ("h_1", "INOUT"), ("h2_1", "INOUT"))
    assert pipe_func_args(ad)[8:] == (("hyper", "IN"), ("state", "IN"))
    ne = solver_update_func_op(d, "nesterov")
    assert [a for a, _ in pipe_func_args(ne)] == ["w_0", "g_0", "h_0", "w_1", "g_1", "h_1", "hyper", "state"]
    assert pipe_func_args(grad_sumsq_func_op(d, 3, 8)) == (("g_0", "IN"), ("g_1", "IN"), ("partials", "INOUT"))
    assert (ad.algo_bytes(), ne.algo_bytes(), grad_sumsq_func_op(d, 3, 8).algo_bytes(), grad_norm_func_op(8).algo_bytes()) == (28 * 9015, 20 * 9015, 4 * 9015 + 16, 48)
    assert rtc_mod.explain_plan(ad) == "bodahip_solver_update_adam grid=4 block=256 tens=2 chunk=4096 clip=1 decoupled_wd=0"
    assert rtc_mod.explain_plan(ne) == "bodahip_solver_update_nesterov grid=4 block=256 tens=2 chunk=4096 clip=0"
    assert rtc_mod.explain_plan(solver_update_func_op(d, "sgd", clip=True)) == "bodahip_solver_update_sgd grid=4 block=256 tens=2 chunk=4096 clip=1"
    assert rtc_mod.explain_plan(grad_sumsq_func_op(d, 3, 8)) == "bodahip_grad_sumsq grid=4 block=256 tens=2 chunk=4096 part0=3"
    assert rtc_mod.explain_plan(grad_norm_func_op(258)) == "bodahip_grad_norm grid=1 block=256 parts=258"
    for f in (ad, grad_sumsq_func_op(d, 3, 8), grad_norm_func_op(8)):
        assert rtc_mod.prebuild(f) > 0      # cross-compiles for gfx950
    with pytest.raises(UnsupErr, match="2 GiB"):
        rtc_mod.explain_plan(solver_update_func_op([Dims.make("float", v=536870912)], "sgd"))


def test_fixture_file_lists_these_ops():
    d = [Dims.make("float", out_chan=8, in_chan=3, y=3, x=3), Dims.make("float", out_chan=8)]
    want = [solver_update_func_op(d, "sgd", [1, 2], [1, 0]), solver_update_func_op(d, "nesterov", [1, 2], [1, 0], clip=True), solver_update_func_op(d, "adam", [1, 2], [1, 0], clip=True),
            solver_update_func_op(d, "adam", [1, 2], [1, 0], decoupled_wd=True), grad_sumsq_func_op(d, 0, 2), grad_norm_func_op(2)]
    assert [o.to_str() for o in read_ops(os.path.join(HERE, "golden", "ops", "solver-ops.txt"))] == [o.to_str() for o in want]


def test_lr_policies_match_their_written_formulas():
    base = 0.1
    its = [0, 1, 4, 5, 6, 9, 10, 11]     # spans the step boundaries at 5 and 10
    pol = lambda **kw: LrPolicy(**kw)
    for it in its:
        assert pol(policy="fixed").lr_at(base, it) == base
        assert pol(policy="step", gamma=0.5, stepsize=5).lr_at(base, it) == base * 0.5 ** (it // 5)
        assert pol(policy="exp", gamma=0.9).lr_at(base, it) == base * 0.9 ** it
        assert pol(policy="inv", gamma=0.01, power=0.75).lr_at(base, it) == base * (1 + 0.01 * it) ** -0.75
        assert pol(policy="multistep", gamma=0.1, stepvalues=(5, 10)).lr_at(base, it) == base * 0.1 ** ((it >= 5) + (it >= 10))
        assert pol(policy="poly", power=2.0, max_iter=20).lr_at(base, it) == base * (1 - it / 20) ** 2.0
        assert pol(policy="sigmoid", gamma=-0.5, stepsize=5).lr_at(base, it) == base * (1 / (1 + math.exp(0.5 * (it - 5))))
    st = pol(policy="step", gamma=0.5, stepsize=5)
    assert [st.lr_at(base, it) for it in (4, 5, 9, 10)] == [0.1, 0.05, 0.05, 0.025]
    assert type(st.lr_at(base, 3)) is float
    with pytest.raises(RtErr, match="policy must be one of"):
        LrPolicy(policy="cosine")
    with pytest.raises(RtErr, match="stepsize >= 1"):
        LrPolicy(policy="step", stepsize=0)


# ---- 4. the driver
MULTS = dict(lr_mult={"biases": 2.0}, decay_mult={"biases": 0.0})


def mk_solver(form, per_call=32, policy=None, lr=0.05):
    t, clip, dwd = form
    return Solver(type=t, lr=lr, momentum=0.9, weight_decay=5e-4, decoupled_wd=dwd, clip_gradients=0.05 if clip else 0.0, lr_policy=policy, tensors_per_call=per_call, **MULTS)


@pytest.mark.parametrize("form", V.FORMS, ids=V.form_id)
@pytest.mark.parametrize("name", ["chain", "fan"])
def test_cpu_three_steps_are_the_twins(cpu, name, form):
    packed = V.three_steps(cpu, name, mk_solver(form, 32))
    three = V.three_steps(cpu, name, mk_solver(form, 3))     # a last call with fewer tensors than the others
    assert set(packed) == set(three)
    for vn in packed:
        assert V.same_bits(packed[vn], three[vn]), vn


def test_cpu_step_policy_boundary_inside_the_three_steps(cpu):
    pol = LrPolicy(policy="step", gamma=0.5, stepsize=2)     # steps 0, 1 at 0.05; step 2 at 0.025 (three_steps checks the uploaded words at every step)
    assert [pol.lr_at(0.05, k) for k in range(3)] == [0.05, 0.05, 0.025]
    V.three_steps(cpu, "chain", mk_solver(("adam", True, False), policy=pol))
    V.three_steps(cpu, "chain", mk_solver(("nesterov", False, False), policy=pol))


def test_solver_calls_vars_and_hyper(cpu):
    sv = Solver(type="adam", lr=0.1, clip_gradients=2.0, lr_policy=LrPolicy(policy="exp", gamma=0.5), tensors_per_call=3, **MULTS)
    drv, bp = V.make_driver(cpu, "chain", sv)
    try:
        pn = list(bp.cp.params)
        assert pn == ["conv1_filts", "conv1_biases", "fc_filts", "fc_biases"] == drv.sgd_params
        tail = drv.calls()[-drv.n_sgd_calls:]
        assert [t for t, _, _ in tail] == ["grad_sumsq_0", "grad_sumsq_1", "grad_norm", "solver_update_0", "solver_update_1"] and drv.n_sgd_calls == 5
        chunks = [-(-bp.cp.params[p].dims_prod() // 4096) for p in pn]
        assert [f.get_u32("part0") for _, f, _ in tail[:2]] == [0, sum(chunks[:3])] and cpu.get_var_dims(SOLVER_PARTS_VAR) == Dims(("v",), (sum(chunks),), "float")
        assert {k: v.n for k, v in tail[4][2].items()} == {"w_0": "fc_biases", "g_0": "fc_biases_grad_loss", "h_0": "fc_biases_sgd_hist", "h2_0": "fc_biases_sgd_hist2",
                                                         "hyper": SOLVER_HYPER_VAR, "state": SOLVER_STATE_VAR}
        assert {k: v.n for k, v in tail[2][2].items()} == {"partials": SOLVER_PARTS_VAR, "hyper": SOLVER_HYPER_VAR, "state": SOLVER_STATE_VAR}
        assert tail[3][1].get_u32("clip") == 1 and tail[3][1].str_vals["solver_type"] == "adam" and tail[3][1].get_f32("lr_mult_1") == 2.0
        assert cpu.get_var_dims(SOLVER_HYPER_VAR) == Dims(("v",), (8,), "float") and cpu.get_var_dims(SOLVER_STATE_VAR) == Dims(("v",), (4,), "float")
        for p in pn:
            for sfx in (SGD_HIST_SFX, SGD_HIST2_SFX):
                assert cpu.get_var_dims(p + sfx) == bp.cp.params[p] and not np.any(cpu.copy_var_to_nda(p + sfx))
        # the dependencies order them: every sumsq behind its gradients' writers, the norm behind every sumsq, every update behind the norm
        deps, n = drv._call_deps(), len(drv.bck_calls)
        reach = []
        for d in deps:
            r = set(d)
            for j in d:
                r |= reach[j]
            reach.append(r)
        assert {n - 5, n - 4} <= reach[n - 3] and (n - 3) in reach[n - 2] and (n - 3) in reach[n - 1] and (n - 2) not in reach[n - 1]
        data, label = V.small_inputs(bp.cp, 0)
        for k in range(2):
            drv.run_bck(["data", "label"], {"data": data, "label": label}, [])
            assert drv.iter == k + 1 and V.same_bits(cpu.copy_var_to_nda(SOLVER_HYPER_VAR), V.want_hyper(sv, k))
        with pytest.raises(RtErr, match="lr is set by the solver's lr_policy"):
            drv.set_sgd_hyper(lr=0.5)
        with pytest.raises(RtErr, match="cannot be switched on or off"):
            drv.set_sgd_hyper(clip_gradients=0.0)
        drv.set_sgd_hyper(momentum2=0.99, delta=1e-6, clip_gradients=3.0, momentum=0.8)
        sv.momentum, sv.momentum2, sv.delta, sv.clip_gradients = 0.8, 0.99, 1e-6, 3.0
        assert V.same_bits(cpu.copy_var_to_nda(SOLVER_HYPER_VAR), V.want_hyper(sv, 2))
        drv.run_device_only(skip_sgd=True)
        assert drv.iter == 2     # a step without the update calls is no solver step
        assert any(np.any(cpu.copy_var_to_nda(p + SGD_HIST2_SFX)) for p in pn)
        drv.zero_sgd_history()
        assert drv.iter == 0 and not any(np.any(cpu.copy_var_to_nda(p + sfx)) for p in pn for sfx in (SGD_HIST_SFX, SGD_HIST2_SFX))
    finally:
        drv.release()
    with pytest.raises(RtErr, match="Solver.type must be"):
        V.make_driver(cpu, "chain", Solver(type="adagrad", lr=0.1))
    with pytest.raises(RtErr, match="tensors_per_call=33"):
        V.make_driver(cpu, "chain", Solver(type="adam", lr=0.1, tensors_per_call=33))
    drv, bp = V.make_driver(cpu, "chain", SgdSolver(lr=0.1))     # an SgdSolver goes down the path it always went
    try:
        assert [t for t, _, _ in drv.calls()][-1] == "sgd_update_0" and SOLVER_HYPER_VAR not in drv.vars
        with pytest.raises(RtErr, match="are a Solver's"):
            drv.set_sgd_hyper(momentum2=0.5)
    finally:
        drv.release()


def test_cpu_batchnorm_pipe_with_adam(cpu):
    """The small residual pipe of tests/test_bn_cpu.py: scale / bias (and filts / biases) move by adam's twin, the running statistics are the forward pass's alone."""
    sv = Solver(type="adam", lr=0.01, clip_gradients=0.5, lr_mult={"biases": 2.0, "scale": 0.5}, decay_mult={"biases": 0.0, "bias": 0.0, "scale": 0.0})
    cp = R.residual(); bp = add_bck_ops(cp)
    drv = ConvPipeBck(cpu, solver=sv, bn_maf=0.9); drv.init(bp, R.res_params(cp, 1))
    try:
        stats = bn_stat_params(cp)
        assert len(stats) == 16 and drv.sgd_params == [p for p in cp.params if p not in stats]
        assert not any(s + sfx in drv.vars for s in stats for sfx in (SGD_HIST_SFX, SGD_HIST2_SFX))
        for _, f, am in drv.calls()[-drv.n_sgd_calls:]:
            assert not {a.n for a in am.values()} & set(stats)
        names = V.state_vars(drv)
        state = V.fetch(cpu, names)
        for k in range(2):
            data, label = R.res_inputs(cp, 100 + k)
            fwd = {"data": data, "label": label}
            drv.run_bck(["data", "label"], fwd, [p + "_grad_loss" for p in drv.sgd_params] + [s.rsplit("_", 1)[0] + "_batch_mean" for s in stats if s.endswith("_mean")])
            after = V.fetch(cpu, names)
            sv_check = [p for p in drv.sgd_params]
            hyper = V.want_hyper(sv, k)
            want_state = V.norm_np(V.partials_np([fwd[p + "_grad_loss"] for p in sv_check]), hyper[6])
            assert V.same_bits(cpu.copy_var_to_nda(SOLVER_STATE_VAR), want_state)
            for p in sv_check:
                w2, m, v = V.solver_np("adam", state[p], fwd[p + "_grad_loss"], state[p + SGD_HIST_SFX], state[p + SGD_HIST2_SFX], hyper, sv.mult_of(sv.lr_mult, p),
                                       sv.mult_of(sv.decay_mult, p), True, want_state[0], False)
                assert V.same_bits(after[p], w2) and V.same_bits(after[p + SGD_HIST_SFX], m) and V.same_bits(after[p + SGD_HIST2_SFX], v), p
            assert any(not V.same_bits(after[p], state[p]) for p in sv_check if p.endswith("_scale")) and any(not V.same_bits(after[p], state[p]) for p in sv_check if p.endswith("_bias"))
            for s in stats:
                if s.endswith("_mean"):     # moved by the forward pass alone: maf * old + (1 - maf) * batch mean
                    bm = fwd[s.rsplit("_", 1)[0] + "_batch_mean"]
                    assert R.same_bits(after[s], R.F(0.9) * state[s] + (R.F(1) - R.F(0.9)) * bm), s
            state = after
    finally:
        drv.release()


# ---- 6. descent
@pytest.mark.parametrize("which", sorted(V.DESCENT))
def test_cpu_descent_follows_the_float64_trajectory(cpu, which):
    l64 = V.descent_f64(which)
    assert l64[-1] <= 0.5 * l64[0], l64                      # lr and the step count make the float64 loss at least halve
    got = V.descent_run(cpu, which)
    dev = max(abs(a - b) for a, b in zip(got, l64))
    print(which, "descent: float64", ["%.6f" % x for x in l64], "be=cpu", ["%.6f" % x for x in got], "max deviation %.3e (bound %.3e)" % (dev, V.DESCENT_BOUND[which]))
    assert got[-1] < got[0]
    assert dev <= V.DESCENT_BOUND[which], dev
