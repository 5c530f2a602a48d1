"""The SGD update without a GPU: hip_sgd_update on be=cpu bit for bit against the numpy twin of its written formula (tests/sgd_ref.py), its refusals, its arg list
and plan, and ConvPipeBck(solver=...) on be=cpu -- the step held to the numpy update of the backend's own values, the dependency lists shown sufficient by running the
call list in other topological orders with poisoned vars, and a descent run on `chain` against a float64 trajectory.

Descent: lr = 0.002, 12 steps, momentum 0.9, weight decay 5e-4, fixed data / label / dropout seed.  The float64 loss falls 0.6126 -> 0.0005.  be=cpu's largest
deviation from the float64 loss over the 12 steps is measured at 1.681e-07; the bound both backends are held to is that times 10,
1.681e-06 (sgd_ref.DESCENT_BOUND), the margin being for the GPU's different K-slice summation order in the filter gradients."""
import numpy as np
import pytest

import sgd_ref as S
from boda_amd import rtc as rtc_mod
from boda_amd.bck_pipe import SGD_HIST_SFX, SGD_HYPER_VAR, ConvPipeBck, SgdSolver, add_bck_ops
from boda_amd.cnn_op import NATIVE_ARGS, PIPE_OP_FUNCS, SGD_OP_FUNCS, pipe_func_args, sgd_update_func_op
from boda_amd.conv_pipe import ConvPipe, PipeOp, _conv
from boda_amd.op import Dims, Nda, RtErr, UnsupErr, parse_op
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc

from test_bck_graph_cpu import run_in_order, topo_order
from test_bck_pipe_cpu import PIPES, SEED_A, small_inputs, small_params

HYPER = (0.01, 0.9, 5e-4)


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


# ---- the function against numpy
def mults(n, lr_mult, decay_mult):
    """Every tensor the given multipliers, except that (where there is more than one tensor) they alternate with the other value of the matrix."""
    return [float(lr_mult if i % 2 == 0 else 3 - lr_mult) for i in range(n)], [float(decay_mult if i % 2 == 0 else 1 - decay_mult) for i in range(n)]


CASES = [[n] for n in S.SIZES] + [[4097, 5], S.SIZES[:7], S.MIXED_32]


@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("lr_mult,decay_mult", [(1, 1), (2, 0), (1, 0), (2, 1)])
@pytest.mark.parametrize("sizes", CASES, ids=lambda s: f"n{len(s)}_{s[0]}")
def test_cpu_function_against_numpy(cpu, sizes, lr_mult, decay_mult, momentum):
    assert len(sizes) in (1, 2, 7, 32)
    lm, dm = mults(len(sizes), lr_mult, decay_mult)
    ins = S.make_inputs(sizes)
    hy = [(HYPER[0], momentum, HYPER[2])]
    got, _ = S.run_sgd(cpu, sizes, lm, dm, hy, ins)
    want = S.want_sgd(sizes, lm, dm, hy, ins)
    for i, ((w, g, h), (ww, _, wh)) in enumerate(zip(got, want)):
        assert S.same_bits(g, ins[i][1]), (i, "g was written")
        assert S.same_bits(h, wh), (i, "history")
        assert S.same_bits(w, ww), (i, "param")
        assert not S.same_bits(w, ins[i][0])


def test_cpu_zeros_keep_their_written_signs(cpu):
    """w = g = h = +0 gives h' = +0 and w' = +0 - +0 = +0; all three -0 (wd_i, momentum, lr_i > 0) gives h' = -0 and w' = -0 - -0 = +0: the twin says so, and be=cpu with it."""
    ins = S.make_inputs([9000])
    (w, g, h), = S.run_sgd(cpu, [9000], [1.0], [1.0], [HYPER], ins)[0]
    bits = lambda a, i: int(a.view(np.uint32)[i])
    assert (bits(w, 4), bits(h, 4)) == (0, 0) and (bits(w, 8999), bits(h, 8999)) == (0, 0x80000000)


def test_cpu_two_calls_are_two_numpy_steps_and_hyper_needs_no_compile(cpu):
    sizes = [4097, 5, 1023]
    lm, dm = [1.0, 2.0, 1.0], [1.0, 0.0, 1.0]
    ins = S.make_inputs(sizes, 3)
    same = [HYPER, HYPER]
    got, _ = S.run_sgd(cpu, sizes, lm, dm, same, ins)
    for (w, g, h), (ww, _, wh) in zip(got, S.want_sgd(sizes, lm, dm, same, ins)):
        assert S.same_bits(w, ww) and S.same_bits(h, wh)
    # hyper rewritten between the calls: the second call runs with the new values, and nothing is compiled for it
    fop = sgd_update_func_op([S.tensor_dims(n, i) for i, n in enumerate(sizes)], lm, dm)
    spec = pipe_func_args(fop)
    cpu.compile([RtcFuncInfo("sgd_h", "", [a for a, _ in spec], fop)])
    made = []
    try:
        for an, _ in spec:
            cpu.create_var_with_dims("hv_" + an, fop.get_dims(an)); made.append("hv_" + an)
        for i, t in enumerate(ins):
            for b, a in zip("wgh", t):
                cpu.copy_nda_to_var(f"hv_{b}_{i}", a)
        call = RtcFuncCall("sgd_h", {an: RtcArg.var("hv_" + an) for an, _ in spec})
        before = rtc_mod.compile_stats()
        steps = [HYPER, (0.5, 0.25, 0.125)]
        for hy in steps:
            cpu.copy_nda_to_var("hv_hyper", np.array(list(hy) + [0.0], np.float32))
            cpu.run(call)
        after = rtc_mod.compile_stats()
        assert (after["compiled"], after["cache_hits"]) == (before["compiled"], before["cache_hits"])
        want = S.want_sgd(sizes, lm, dm, steps, ins)
        wrong = S.want_sgd(sizes, lm, dm, same, ins)
        for i in range(len(sizes)):
            w = cpu.copy_var_to_nda(f"hv_w_{i}").reshape(-1)
            assert S.same_bits(w, want[i][0]) and not S.same_bits(w, wrong[i][0])
    finally:
        for vn in made:
            cpu.release_var(vn)
        cpu.release_func("sgd_h"); cpu.release_per_call_id_data()


# ---- tables, arg list, plan
def test_tables_arg_list_and_plan():
    assert SGD_OP_FUNCS == {"SgdUpdate": ("hip_sgd_update",)} and "SgdUpdate" not in PIPE_OP_FUNCS
    f = sgd_update_func_op([Dims.make("float", v=9000), Dims.make("float", a=3, b=5)], [1, 2], [1, 0])
    assert f.get_func_name() == "hip_sgd_update" and f.get_type() == "SgdUpdate" and f.get_u32("tens_num") == 2
    assert pipe_func_args(f) == (("w_0", "INOUT"), ("g_0", "IN"), ("h_0", "INOUT"), ("w_1", "INOUT"), ("g_1", "IN"), ("h_1", "INOUT"), ("hyper", "IN"))
    assert NATIVE_ARGS["hip_sgd_update"] == (("hyper", "IN"),)
    assert f.get_dims("hyper") == Dims(("v",), (4,), "float") and f.get_f32("lr_mult_1") == 2.0 and f.get_f32("decay_mult_1") == 0.0
    assert parse_op(f.to_str()).to_str() == f.to_str() and rtc_mod.parse_op_native(f.to_str()) == f.to_str()
    assert f.algo_bytes() == 20 * 9015 and f.flops() == 0
    plan = rtc_mod.explain_plan(f)
    assert plan.startswith("bodahip_sgd_update grid=4 block=256"), plan      # 9000 floats: three chunks of 4096; 15 floats: one
    assert rtc_mod.explain_plan(sgd_update_func_op([Dims.make("float", v=n) for n in S.MIXED_32])).startswith("bodahip_sgd_update grid=%d " % sum(-(-n // 4096) for n in S.MIXED_32))
    assert rtc_mod.prebuild(f) > 0      # cross-compiles for gfx950
    with pytest.raises(UnsupErr, match="2 GiB"):
        rtc_mod.explain_plan(sgd_update_func_op([Dims.make("float", v=536870912)]))


def test_fixture_file_lists_the_function_op():
    """tests/golden/ops/sgd-ops.txt: what build() pre-specialises (one kernel for every call: the table rides in the arguments)."""
    import os
    from boda_amd.op import read_ops
    ops = read_ops(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops", "sgd-ops.txt"))
    want = sgd_update_func_op([Dims.make("float", out_chan=8, in_chan=3, y=3, x=3), Dims.make("float", out_chan=8)], [1, 2], [1, 0])
    assert [o.to_str() for o in ops] == [want.to_str()]


# ---- refusals
def bad_op(f, **nda):
    b = f.copy()
    for k, v in nda.items():
        if v is None:
            b.nda_vals.pop(k)
        else:
            b.nda_vals[k] = v
    return b


def test_refusals_of_the_op(cpu):
    d = Dims.make("float", v=7)
    f = sgd_update_func_op([d, d])
    with pytest.raises(RtErr, match="1 to 32 tensors"):
        sgd_update_func_op([])
    with pytest.raises(RtErr, match="1 to 32 tensors"):
        sgd_update_func_op([d] * 33)
    u32 = lambda v: Nda(None, "uint32_t", (v,))
    cases = [
        (bad_op(f, tens_num=u32(0)), "tens_num=0: 1 to 32 tensors"),
        (bad_op(f, tens_num=u32(33)), "tens_num=33: 1 to 32 tensors"),
        (bad_op(f, g_1=None), "the op has no 'g_1'"),
        (bad_op(f, hyper=None), "the op has no 'hyper'"),
        (bad_op(f, decay_mult_0=None), "the op has no 'decay_mult_0'"),
        (bad_op(f, h_0=Nda(dims=Dims.make("uint32_t", v=7), tn="uint32_t")), "h_0 has type uint32_t"),
        (bad_op(f, g_1=Nda(dims=Dims.make("float", v=8), tn="float")), "g_1 dims .* differ from w_1's"),
        (bad_op(f, hyper=Nda(dims=Dims.make("float", v=3), tn="float")), "hyper must be float v=4"),
        (bad_op(f, hyper=Nda(dims=Dims.make("uint32_t", v=4), tn="uint32_t")), "hyper must be float v=4"),
        (bad_op(f, img_shards=u32(1)), "img_shards=1 on 'hip_sgd_update'"),
        (bad_op(f, seed_from_var=u32(1)), "seed_from_var=1 on 'hip_sgd_update'"),
        (bad_op(f, zero_if_in_non_pos=u32(1)), "zero_if_in_non_pos=1 on 'hip_sgd_update'"),
    ]
    for bad, msg in cases:
        with pytest.raises(RtErr, match=msg):
            cpu.compile([RtcFuncInfo("bad", "", [a for a, _ in pipe_func_args(f)], bad)])
        with pytest.raises(RtErr, match=msg):
            rtc_mod.explain_plan(bad)
        with pytest.raises(RtErr, match=msg):
            rtc_mod.prebuild(bad)
    wrong_type = f.copy(); wrong_type.str_vals["type"] = "Reduce"
    with pytest.raises(RtErr, match="a function of op type SgdUpdate"):
        cpu.compile([RtcFuncInfo("bad", "", [a for a, _ in pipe_func_args(f)], wrong_type)])


def test_refusals_of_the_call(cpu):
    d = Dims.make("float", v=7)
    f = sgd_update_func_op([d, d])
    spec = pipe_func_args(f)
    cpu.compile([RtcFuncInfo("sgd_r", "", [a for a, _ in spec], f)])
    made = []
    try:
        for an, _ in spec:
            cpu.create_var_with_dims("rv_" + an, f.get_dims(an)); made.append("rv_" + an)
            cpu.copy_nda_to_var("rv_" + an, np.ones(f.get_dims(an).sizes, np.float32))
        for vn, dims in (("rv_u32", Dims.make("uint32_t", v=7)), ("rv_eight", Dims.make("float", v=8)), ("rv_h3", Dims.make("float", v=3))):
            cpu.create_var_with_dims(vn, dims); made.append(vn)
        good = {an: RtcArg.var("rv_" + an) for an, _ in spec}
        run = lambda **kw: cpu.run(RtcFuncCall("sgd_r", dict(good, **{k: (RtcArg.var(v) if v else None) for k, v in kw.items()})))
        with pytest.raises(RtErr, match="arg 'g_1' not found"):
            cpu.run(RtcFuncCall("sgd_r", {k: v for k, v in good.items() if k != "g_1"}))
        with pytest.raises(RtErr, match="arg 'hyper' not found"):
            cpu.run(RtcFuncCall("sgd_r", {k: v for k, v in good.items() if k != "hyper"}))
        with pytest.raises(RtErr, match="arg 'h_0' .* has type uint32_t"):
            run(h_0="rv_u32")
        with pytest.raises(RtErr, match="arg 'g_0' has dims .*, the op says"):
            run(g_0="rv_eight")
        with pytest.raises(RtErr, match="arg 'hyper' has dims .*, the op says"):
            run(hyper="rv_h3")
        for a, b in (("w_0", "g_0"), ("w_0", "h_0"), ("g_0", "h_0"), ("w_0", "w_1"), ("g_0", "g_1"), ("h_0", "w_1")):   # any two of the 3n + 1 vars being one var
            with pytest.raises(RtErr, match=f"args '{a}' and '{b}' are the same var 'rv_{a}'"):
                run(**{b: "rv_" + a})
        for vn in ("rv_g4", "rv_h4"):
            cpu.create_var_with_dims(vn, Dims.make("float", v=4)); made.append(vn)
        f4 = sgd_update_func_op([Dims.make("float", v=4)])
        cpu.compile([RtcFuncInfo("sgd_r4", "", [a for a, _ in pipe_func_args(f4)], f4)])
        try:
            with pytest.raises(RtErr, match="args 'w_0' and 'hyper' are the same var 'rv_hyper'"):     # hyper is one of the 3n + 1
                cpu.run(RtcFuncCall("sgd_r4", {"w_0": RtcArg.var("rv_hyper"), "g_0": RtcArg.var("rv_g4"), "h_0": RtcArg.var("rv_h4"), "hyper": RtcArg.var("rv_hyper")}))
        finally:
            cpu.release_func("sgd_r4")
        cpu.run(RtcFuncCall("sgd_r", good))   # the refusals left everything usable
        assert np.all(cpu.copy_var_to_nda("rv_g_0") == 1.0)
    finally:
        for vn in made:
            cpu.release_var(vn)
        cpu.release_func("sgd_r"); cpu.release_per_call_id_data()


# ---- the driver
@pytest.mark.parametrize("name", sorted(PIPES))
def test_no_solver_is_the_driver_as_it_was(cpu, name):
    mk, tops, seed = PIPES[name]
    cp = mk(); bp = add_bck_ops(cp, loss_tops=tops)
    a = ConvPipeBck(cpu); a.init(bp, small_params(cp, seed))
    try:
        ca, da, va = [(t, f.to_str(), {k: (v.n, None if v.v is None else v.v.tolist()) for k, v in am.items()}) for t, f, am in a.calls()], a._call_deps(), list(a.vars)
    finally:
        a.release()
    b = ConvPipeBck(cpu, solver=None); b.init(bp, small_params(cp, seed))
    try:
        cb, db, vb = [(t, f.to_str(), {k: (v.n, None if v.v is None else v.v.tolist()) for k, v in am.items()}) for t, f, am in b.calls()], b._call_deps(), list(b.vars)
        assert b.n_sgd_calls == 0 and not any(v.endswith(SGD_HIST_SFX) or v == SGD_HYPER_VAR for v in vb)
        with pytest.raises(RtErr, match="without a solver"):
            b.set_sgd_hyper(lr=1.0)
        with pytest.raises(RtErr, match="without a solver"):
            b.zero_sgd_history()
    finally:
        b.release()
    assert ca == cb and da == db and va == vb
    s, _ = S.make_sgd_driver(cpu, name, SgdSolver(lr=0.1))
    try:   # with a solver: the same calls in front, the update calls behind them
        cs = [(t, f.to_str(), {k: (v.n, None if v.v is None else v.v.tolist()) for k, v in am.items()}) for t, f, am in s.calls()]
        assert cs[:len(ca)] == ca and [t for t, _, _ in cs[len(ca):]] == ["sgd_update_0"] and s._call_deps()[:len(da)] == da
    finally:
        s.release()


@pytest.mark.parametrize("name", sorted(PIPES))
def test_cpu_three_steps_are_numpy_updates(cpu, name):
    packed = S.three_steps(cpu, name, 32)
    single = S.three_steps(cpu, name, 1)
    assert set(packed) == set(single)
    for vn in packed:
        assert S.same_bits(packed[vn], single[vn]), vn
    two = S.three_steps(cpu, name, 3)     # a last call with fewer tensors than the others
    for vn in packed:
        assert S.same_bits(packed[vn], two[vn]), vn


def test_solver_calls_vars_and_mults(cpu):
    solver = SgdSolver(lr=0.1, lr_mult={"biases": 2.0, "fc_biases": 4.0}, decay_mult={"biases": 0.0}, tensors_per_call=3)
    drv, bp = S.make_sgd_driver(cpu, "chain", solver)
    try:
        pn = list(bp.cp.params)
        assert pn == ["conv1_filts", "conv1_biases", "fc_filts", "fc_biases"]
        upd = [(t, f, am) for t, f, am in drv.calls() if f.get_func_name() == "hip_sgd_update"]
        assert [t for t, _, _ in upd] == ["sgd_update_0", "sgd_update_1"] == [c.tag for c in drv.bck_calls[-2:]] and drv.n_sgd_calls == 2
        (_, f0, a0), (_, f1, a1) = upd
        assert f0.get_u32("tens_num") == 3 and f1.get_u32("tens_num") == 1
        assert {k: v.n for k, v in a0.items()} == {"w_0": "conv1_filts", "g_0": "conv1_filts_grad_loss", "h_0": "conv1_filts_sgd_hist", "w_1": "conv1_biases",
                                                  "g_1": "conv1_biases_grad_loss", "h_1": "conv1_biases_sgd_hist", "w_2": "fc_filts", "g_2": "fc_filts_grad_loss",
                                                  "h_2": "fc_filts_sgd_hist", "hyper": "sgd_hyper"}
        assert {k: v.n for k, v in a1.items()} == {"w_0": "fc_biases", "g_0": "fc_biases_grad_loss", "h_0": "fc_biases_sgd_hist", "hyper": "sgd_hyper"}
        assert [f0.get_f32(f"lr_mult_{i}") for i in range(3)] == [1.0, 2.0, 1.0] and [f0.get_f32(f"decay_mult_{i}") for i in range(3)] == [1.0, 0.0, 1.0]
        assert f1.get_f32("lr_mult_0") == 4.0 and f1.get_f32("decay_mult_0") == 0.0     # a param's name wins over its suffix
        for p in pn:
            assert cpu.get_var_dims(p + SGD_HIST_SFX) == bp.cp.params[p] and not np.any(cpu.copy_var_to_nda(p + SGD_HIST_SFX))
        assert cpu.get_var_dims(SGD_HYPER_VAR) == Dims(("v",), (4,), "float")
        assert S.same_bits(cpu.copy_var_to_nda(SGD_HYPER_VAR), np.array([0.1, 0.9, 5e-4, 0.0], np.float32))
        forms_before = None
        data, label = small_inputs(bp.cp, 0)
        drv.run_bck(["data", "label"], {"data": data, "label": label}, [])
        forms_before = [c.rfc.__dict__.get("_c_form") for c in drv.bck_calls]
        stats = rtc_mod.compile_stats()
        drv.set_sgd_hyper(momentum=0.5)
        assert S.same_bits(cpu.copy_var_to_nda(SGD_HYPER_VAR), np.array([0.1, 0.5, 5e-4, 0.0], np.float32))
        drv.set_sgd_hyper(lr=0.25, weight_decay=0.0)
        assert S.same_bits(cpu.copy_var_to_nda(SGD_HYPER_VAR), np.array([0.25, 0.5, 0.0, 0.0], np.float32))
        assert all(a is b and a is not None for a, b in zip(forms_before, [c.rfc.__dict__.get("_c_form") for c in drv.bck_calls]))   # no call was touched
        assert (rtc_mod.compile_stats()["compiled"], rtc_mod.compile_stats()["cache_hits"]) == (stats["compiled"], stats["cache_hits"])
        assert any(np.any(cpu.copy_var_to_nda(p + SGD_HIST_SFX)) for p in pn)
        drv.zero_sgd_history()
        assert not any(np.any(cpu.copy_var_to_nda(p + SGD_HIST_SFX)) for p in pn)
        # the update calls sit behind every reader of their params and every writer of their gradients
        deps, calls = drv._call_deps(), drv.bck_calls
        reach = []
        for d in deps:
            r = set(d)
            for j in d:
                r |= reach[j]
            reach.append(r)
        for i in (len(calls) - 2, len(calls) - 1):
            mine = {v.n for v in calls[i].rfc.arg_map.values() if v.n and v.n != SGD_HYPER_VAR}
            for j, c in enumerate(calls[:len(calls) - 2]):
                if mine & {v.n for v in c.rfc.arg_map.values() if v.n}:
                    assert j in reach[i], (calls[i].tag, c.tag)
        assert (len(calls) - 2) not in reach[len(calls) - 1]      # the two update calls share only sgd_hyper, which both read: independent
    finally:
        drv.release()
    with pytest.raises(RtErr, match="tensors_per_call=0"):
        S.make_sgd_driver(cpu, "chain", SgdSolver(lr=0.1, tensors_per_call=0))
    with pytest.raises(RtErr, match="tensors_per_call=33"):
        S.make_sgd_driver(cpu, "chain", SgdSolver(lr=0.1, tensors_per_call=33))


def test_history_var_name_clash(cpu):
    p = ConvPipe("clash", "data", Dims.make("float", img=2, chan=3, y=5, x=5))
    _conv(p, "c1", "data", 4, 3)
    _conv(p, "c1_filts_sgd_hist", "c1", 4, 1)
    p.add(PipeOp("fc", "Convolution", "c1_filts_sgd_hist", "fc", out_chans=5, kern_sz=(0, 0)))
    bp = add_bck_ops(p)
    drv = ConvPipeBck(cpu, solver=SgdSolver(lr=0.1))
    with pytest.raises(RtErr, match="'c1_filts_sgd_hist', which is a node of the pipe"):
        drv.init(bp, small_params(p, 0))
    assert drv.vars == [] and drv.funcs == []   # refused before anything was created


# ---- dependencies: other topological orders, written vars poisoned
@pytest.mark.parametrize("per_call", [32, 1])
@pytest.mark.parametrize("name", sorted(PIPES))
def test_call_deps_with_solver_are_sufficient(cpu, name, per_call):
    solver = SgdSolver(lr=0.05, lr_mult={"biases": 2.0}, decay_mult={"biases": 0.0}, tensors_per_call=per_call)
    drv, bp = S.make_sgd_driver(cpu, name, solver, seed_in_var=True)
    try:
        mk, tops, seed = PIPES[name]
        data, label = small_inputs(bp.cp, seed)
        params = small_params(bp.cp, seed)
        hist = {p + SGD_HIST_SFX: np.random.default_rng([5, i]).uniform(-0.1, 0.1, a.shape).astype(np.float32) for i, (p, a) in enumerate(params.items())}
        keep = set(params) | set(hist) | {"data", "label", "det_drop_seed", SGD_HYPER_VAR}
        deps = drv._call_deps()
        n = len(deps)

        def run(order):
            drv.set_det_drop_seed(SEED_A)
            for vn, a in list(params.items()) + list(hist.items()) + [("data", data), ("label", label)]:
                cpu.copy_nda_to_var(vn, a)
            return run_in_order(cpu, drv, order, keep)
        want = run(range(n))
        for p in params:   # the list order is the step followed by the numpy update
            w2, h2 = S.sgd_np(params[p], want[p + "_grad_loss"], hist[p + SGD_HIST_SFX], 0.05, 0.9, 5e-4, solver.mult_of(solver.lr_mult, p), solver.mult_of(solver.decay_mult, p))
            assert S.same_bits(want[p], w2) and S.same_bits(want[p + SGD_HIST_SFX], h2), p
        rng = np.random.default_rng(17)
        orders = {"latest ready first": topo_order(deps, max), "random topological": topo_order(deps, lambda r: r[int(rng.integers(len(r)))])}
        for what, order in orders.items():
            assert sorted(order) == list(range(n)) and order != list(range(n)), what
            got = run(order)
            for vn in drv.vars:
                assert got[vn].tobytes() == want[vn].tobytes(), (what, vn)
        # and the check can fail: an update call without its dependencies runs first, ahead of the gradient it reads and the forward pass that reads its param
        victim = n - 1
        loose = [([] if i == victim else d) for i, d in enumerate(deps)]
        got = run(topo_order(loose, max))
        assert any(got[vn].tobytes() != want[vn].tobytes() for vn in drv.vars)
    finally:
        drv.release()


# ---- descent
def test_cpu_descent_follows_the_float64_trajectory(cpu):
    l64 = S.descent_f64()
    assert l64[-1] <= 0.5 * l64[0], l64                      # lr and the step count make the float64 loss at least halve
    got = S.descent_run(cpu)
    dev = max(abs(a - b) for a, b in zip(got, l64))
    print("descent: float64", ["%.6f" % x for x in l64], "be=cpu", ["%.6f" % x for x in got], "max deviation %.3e (bound %.3e)" % (dev, S.DESCENT_BOUND))
    assert got[-1] < got[0]
    assert dev <= S.DESCENT_BOUND, dev
