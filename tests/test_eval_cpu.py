"""The evaluation pass without a GPU: hip_accuracy, hip_eval_accum and hip_bn_fold on be=cpu word for word against their twins (tests/eval_ref.py; hip_bn_fold against
conv_pipe.fold_affine), their refusals, table rows, arg lists and plan lines, and EvalPipe on be=cpu: the test-phase pass, its result against the twins on the backend's
own logits and losses, the side-effect contract, and a training run that evaluations leave undisturbed."""
import os

import numpy as np
import pytest

import eval_ref as E
from boda_amd import rtc as rtc_mod
from boda_amd.bck_pipe import ConvPipeBck, add_bck_ops
from boda_amd.cnn_op import ACCUM_OP_FUNCS, EVAL_OP_FUNCS, NATIVE_ARGS, accuracy_func_op, bn_fold_func_op, eval_accum_func_op, pipe_func_args
from boda_amd.conv_pipe import ConvPipe, _conv
from boda_amd.eval_pipe import EVAL_CTL_VAR, EvalPipe
from boda_amd.op import Dims, Nda, Op, RtErr, UnsupErr, parse_op, read_ops
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc

from test_bck_pipe_cpu import N_CLASS, small_params

F, U32 = np.float32, np.uint32
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


# ---- 1. the three functions
@pytest.mark.parametrize("C", E.ACC_CHANS)
def test_cpu_accuracy(cpu, C):
    E.check_accuracy(cpu, C)


def test_accuracy_rule_on_named_images():
    """The twin itself, on images whose rank is known without it."""
    x = np.array([[1, 5, 3, 5, 2]], F)
    assert list(E.accuracy_np(np.repeat(x, 5, 0), np.arange(5, dtype=F))) == [4, 1, 2, 1, 3]     # the two 5s tie: each has the other against it
    assert list(E.accuracy_np(x, [4.999])) == [3] and list(E.accuracy_np(x, [5.0])) == [E.INVALID] and list(E.accuracy_np(x, [-0.0])) == [4]     # (-0 >= 0: class 0)
    assert list(E.accuracy_np(np.zeros((1, 1000), F), [7.0])) == [999]     # a net that answers a constant scores 0 under every k < 1000


@pytest.mark.parametrize("top_k", E.ACCUM_TOP_KS)
@pytest.mark.parametrize("B", E.ACCUM_IMGS)
def test_cpu_eval_accum(cpu, B, top_k):
    E.check_eval_accum(cpu, B, top_k)


@pytest.mark.parametrize("C", E.FOLD_CHANS)
def test_cpu_bn_fold(cpu, C):
    a, b = E.check_bn_fold(cpu, C)
    if C > 8:
        assert np.isnan(a[3]) and np.isnan(b[3])                              # var + eps < 0: what numpy gives
        assert a[5] == 0 and np.isfinite(b[5])                                # var = Inf
        assert b[1] != 0 or not np.signbit(b[1])
    E.check_bn_fold(cpu, C, eps=0.0)


def test_bn_fold_minus_zero_becomes_plus_zero(cpu):
    """mean = +0 gives b2 = -(+0 * a2) = -0; the chain's a2 * 0 + b2 turns it into +0, so b = scale * +0 + bias keeps bias's bits even for bias = -0 ... + (+0) = +0."""
    fop = bn_fold_func_op(2, 1e-5)
    vals = {"run_mean": np.zeros(2, F), "run_var": np.ones(2, F), "scale": np.array([1.0, -1.0], F), "bias": np.array([-0.0, -0.0], F), "a": np.zeros(2, F), "b": np.ones(2, F)}
    (seen,), _ = E.run_steps(cpu, "foldz", fop, vals, [{}])
    from boda_amd.conv_pipe import fold_affine
    wa, wb = fold_affine([("BatchNorm", vals["run_mean"], vals["run_var"], 1e-5), ("Scale", vals["scale"], vals["bias"])])
    assert seen["b"].tobytes() == wb.tobytes() and seen["a"].tobytes() == wa.tobytes()
    assert not np.signbit(seen["b"][0]) and np.signbit(seen["b"][1])     # scale * (+0) + (-0): +0 for scale > 0, (-0) + (-0) = -0 for scale < 0


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


D4 = Dims.make("float", img=5, chan=7, y=1, x=1)


def test_refusals_of_the_op(cpu):
    u32 = lambda v: Nda(None, "uint32_t", (v,))
    vec = lambda tn, **kw: Nda(dims=Dims.make(tn, **kw), tn=tn)
    with pytest.raises(RtErr, match="top_k=0"):
        eval_accum_func_op(5, 0)
    with pytest.raises(UnsupErr, match="only 1 x 1 planes"):
        accuracy_func_op(Dims.make("float", img=5, chan=7, y=2, x=1))
    with pytest.raises(RtErr, match="eps must not be negative"):
        bn_fold_func_op(7, -1e-5)
    ac, ea, bf = accuracy_func_op(D4), eval_accum_func_op(5, 5), bn_fold_func_op(7, 1e-5)
    cases = [
        (bad_op(ac, rank=vec("uint32_t", img=6)), RtErr, "rank must be uint32_t img=5"),
        (bad_op(ac, rank=vec("float", img=5)), RtErr, "rank must be uint32_t img=5"),
        (bad_op(ac, rank=None), RtErr, "the op has no 'rank'"),
        (bad_op(ac, label=vec("float", img=4, y=1, x=1)), UnsupErr, "only 1 x 1 planes"),
        (bad_op(ac, label=vec("uint32_t", img=5, y=1, x=1)), RtErr, "label has type uint32_t"),
        (bad_op(ac, **{"in": vec("float", img=5, chan=7, y=3, x=3)}), UnsupErr, "only 1 x 1 planes"),
        (bad_op(ac, **{"in": vec("float", img=5, chan=7)}), RtErr, "in must be float img:chan:y:x"),
        (bad_op(ea, top_k=u32(0)), RtErr, "top_k=0: top_k must be at least 1"),
        (bad_op(ea, top_k=None), RtErr, "the op has no 'top_k'"),
        (bad_op(ea, rank=vec("float", img=5)), RtErr, "rank must be uint32_t img="),
        (bad_op(ea, loss=vec("float", v=1)), RtErr, "loss must be float y=1:x=1"),
        (bad_op(ea, ctl=vec("float", v=4)), RtErr, "ctl must be uint32_t v=4"),
        (bad_op(ea, ctl=vec("uint32_t", v=1)), RtErr, "ctl must be uint32_t v=4"),
        (bad_op(ea, counts=vec("uint32_t", v=3)), RtErr, "counts must be uint32_t v=4"),
        (bad_op(ea, loss_sum=vec("float", v=4)), RtErr, "loss_sum must be float v=1"),
        (bad_op(ea, loss_sum=None), RtErr, "the op has no 'loss_sum'"),
        (bad_op(bf, a=vec("float", chan=8)), RtErr, "a must be float chan=7"),
        (bad_op(bf, scale=vec("uint32_t", chan=7)), RtErr, "scale must be float chan=7"),
        (bad_op(bf, eps=None), RtErr, "the op has no 'eps'"),
        (bad_op(bf, eps=Nda(None, "float", (-1.0,))), RtErr, "eps must not be negative"),
    ]
    for f in (ac, ea, bf):
        fn = f.get_func_name()
        cases += [(bad_op(f, img_shards=u32(1)), RtErr, f"img_shards=1 on '{fn}'"), (bad_op(f, seed_from_var=u32(1)), RtErr, f"seed_from_var=1 on '{fn}'"),
                  (bad_op(f, zero_if_in_non_pos=u32(1)), RtErr, f"zero_if_in_non_pos=1 on '{fn}'")]
        wrong = f.copy(); wrong.str_vals["type"] = "Reduce"
        cases.append((wrong, RtErr, f"a function of op type {f.get_type()}"))
    for bad, err, msg in cases:
        with pytest.raises(err, match=msg):
            cpu.compile([RtcFuncInfo("bad", "", [a for a, _ in pipe_func_args(bad)], bad)])
        if bad.get_type() != "Reduce":
            with pytest.raises(err, match=msg):
                rtc_mod.explain_plan(bad)
    with pytest.raises(RtErr, match="a bare EvalAccum op"):
        rtc_mod.explain_plan(Op({"type": "EvalAccum"}, dict(ea.nda_vals)))


def test_refusals_of_the_call(cpu):
    """Wrong types and dims of the vars, and any two args one var, worded like hip_grad_accum's."""
    f = eval_accum_func_op(4, 5)     # (rank and ctl, and ctl and counts, have the same dims: one var can be bound to both)
    spec = pipe_func_args(f)
    order = [a for a, _ in spec]
    cpu.compile([RtcFuncInfo("ea_r", "", order, f)])
    made = []
    try:
        for an, _ in spec:
            cpu.create_var_with_dims("rv_" + an, f.get_dims(an)); made.append("rv_" + an)
        for vn, dims in (("rv_f4", Dims.make("float", v=4)), ("rv_u5", Dims.make("uint32_t", v=5)), ("rv_u1", Dims.make("uint32_t", v=1)), ("rv_rank9", Dims.make("uint32_t", img=9))):
            cpu.create_var_with_dims(vn, dims); made.append(vn)
        good = {an: RtcArg.var("rv_" + an) for an, _ in spec}
        run = lambda **kw: cpu.run(RtcFuncCall("ea_r", dict(good, **{k: RtcArg.var(v) for k, v in kw.items()})))
        with pytest.raises(RtErr, match="arg 'ctl' not found"):
            cpu.run(RtcFuncCall("ea_r", {k: v for k, v in good.items() if k != "ctl"}))
        with pytest.raises(RtErr, match="arg 'counts' .* has type float"):
            run(counts="rv_f4")
        with pytest.raises(RtErr, match="arg 'loss_sum' .* has type uint32_t"):
            run(loss_sum="rv_u1")
        with pytest.raises(RtErr, match="arg 'ctl' has dims .*, the op says"):
            run(ctl="rv_u5")
        with pytest.raises(RtErr, match="arg 'rank' has dims .*, the op says"):
            run(rank="rv_rank9")     # (the image count is the op's: the function sums over the images)
        for a, b in (("ctl", "counts"),):
            with pytest.raises(RtErr, match=f"args '{a}' and '{b}' are the same var 'rv_{a}'"):
                run(**{b: "rv_" + a})
        cpu.copy_nda_to_var("rv_ctl", np.array([1, 0, 0, 0], U32))
        cpu.run(RtcFuncCall("ea_r", good))
        assert list(cpu.copy_var_to_nda("rv_counts")) == [4, 4, 4, 1]     # (zero-filled ranks: every image a hit)
    finally:
        for vn in made:
            cpu.release_var(vn)
        cpu.release_func("ea_r"); cpu.release_per_call_id_data()
    fb = bn_fold_func_op(3, 1e-5)     # six vars of equal dims: any two of them
    cpu.compile([RtcFuncInfo("bf_r", "", [a for a, _ in pipe_func_args(fb)], fb)])
    try:
        for an, _ in pipe_func_args(fb):
            cpu.create_var_with_dims("fv_" + an, fb.get_dims(an))
        good = {an: RtcArg.var("fv_" + an) for an, _ in pipe_func_args(fb)}
        for a, b in (("run_mean", "run_var"), ("scale", "a"), ("a", "b"), ("run_var", "b")):
            with pytest.raises(RtErr, match=f"args '{a}' and '{b}' are the same var 'fv_{a}'"):
                cpu.run(RtcFuncCall("bf_r", dict(good, **{b: RtcArg.var("fv_" + a)})))
    finally:
        for an, _ in pipe_func_args(fb):
            cpu.release_var("fv_" + an)
        cpu.release_func("bf_r"); cpu.release_per_call_id_data()


def fixture_ops():
    return [accuracy_func_op(D4), accuracy_func_op(Dims.make("float", img=9, chan=1000, y=1, x=1)), eval_accum_func_op(5, 5), eval_accum_func_op(1000, 1), bn_fold_func_op(7, 1e-5),
            bn_fold_func_op(257, 0.0)]


def test_tables_arg_lists_and_plans():
    assert EVAL_OP_FUNCS == {"Accuracy": ("hip_accuracy",), "EvalAccum": ("hip_eval_accum",), "BnFold": ("hip_bn_fold",)}
    assert ACCUM_OP_FUNCS == {"GradAccum": ("hip_grad_accum",), "SolverUpdateAcc": ("hip_solver_update_acc",)}     # (the table beside it stays)
    table = rtc_mod.native_funcs()
    modes = {"hip_accuracy": "on_shards", "hip_eval_accum": "replicated_vars", "hip_bn_fold": "replicated_vars"}
    for member, (t, (fn,)) in enumerate(EVAL_OP_FUNCS.items(), 1):
        r = table[fn]
        assert (r["family"], r["member"], r["types"], r["multi_dev"], r["be"], r["flags"], r["opt"], r["why"]) == ("eval", member, (t,), modes[fn], ("hip", "cpu"), (), (), ""), fn
    assert [r["family"] for r in table.values()][-3:] == ["eval"] * 3 and list(table)[-3:] == ["hip_accuracy", "hip_eval_accum", "hip_bn_fold"]     # appended at the end
    assert NATIVE_ARGS["hip_accuracy"] == (("in", "IN"), ("label", "IN"), ("rank", "OUT"))
    assert NATIVE_ARGS["hip_eval_accum"] == (("rank", "IN"), ("loss", "IN"), ("ctl", "IN"), ("counts", "INOUT"), ("loss_sum", "INOUT"))
    assert NATIVE_ARGS["hip_bn_fold"] == (("run_mean", "IN"), ("run_var", "IN"), ("scale", "IN"), ("bias", "IN"), ("a", "OUT"), ("b", "OUT"))
    gold = read_ops(os.path.join(HERE, "golden", "ops", "eval-ops.txt"))
    assert [o.to_str() for o in gold] == [o.to_str() for o in fixture_ops()]
    for f in gold:
        assert rtc_mod.func_args(f) == pipe_func_args(f) == NATIVE_ARGS[f.get_func_name()], f.to_str()
        assert parse_op(f.to_str()).to_str() == f.to_str() and rtc_mod.parse_op_native(f.to_str()) == f.to_str()
        assert f.flops() == 0
        assert rtc_mod.prebuild(f) > 0      # cross-compiles for gfx950
    for fn in NATIVE_ARGS:
        if fn.startswith(("hip_accuracy", "hip_eval_accum", "hip_bn_fold")):     # the arg-list query of a bare op
            assert rtc_mod.func_args(Op({"type": table[fn]["types"][0], "func_name": fn}, {})) == NATIVE_ARGS[fn]
    ac, big, ea, ea1k, bf, bf257 = gold
    assert rtc_mod.explain_plan(ac) == "bodahip_accuracy grid=2 block=256 imgs=5 chans=7"
    assert rtc_mod.explain_plan(big) == "bodahip_accuracy grid=3 block=256 imgs=9 chans=1000"
    assert rtc_mod.explain_plan(ea) == "bodahip_eval_accum grid=1 block=256 imgs=5 top_k=5"
    assert rtc_mod.explain_plan(ea1k) == "bodahip_eval_accum grid=1 block=256 imgs=1000 top_k=1"
    assert rtc_mod.explain_plan(bf) == "bodahip_bn_fold grid=1 block=256 chans=7"
    assert rtc_mod.explain_plan(bf257) == "bodahip_bn_fold grid=2 block=256 chans=257"
    with pytest.raises(UnsupErr, match="2 GiB"):
        rtc_mod.explain_plan(accuracy_func_op(Dims.make("float", img=65536, chan=8192, y=1, x=1)))


# ---- 3. the pass
def test_cpu_chain_is_the_pipe_without_dropout(cpu):
    E.check_chain_is_the_pipe_without_dropout(cpu)


@pytest.mark.parametrize("name,loss", [("fan", None), ("heads", "loss1"), ("heads", "loss2"), ("heads", None)])
def test_cpu_result_is_the_twin(cpu, name, loss):
    got, _, _ = E.check_result_is_the_twin(cpu, name, loss)
    print(name, loss, got)


def test_cpu_calls_reuse_the_drivers(cpu):
    """No convolution, pooling or LRN is compiled twice: every call but the two behind the loss is the driver's own function with the driver's own bindings."""
    drv, bp = E.make_driver(cpu, "chain")
    try:
        ev = EvalPipe(drv)
        assert ev.top_k == 5 and ev.loss == "loss"
        mine = [(t, f.get_func_name(), am) for t, f, am in ev.calls()]
        theirs = [(t, f.get_func_name(), am) for t, f, am in drv.calls()]
        assert [m[:2] for m in mine] == [("conv1", "hip_conv"), ("norm1", "hip_lrn_sb"), ("pool1", "hip_pool_yx"), ("fc", "hip_conv"), ("loss", "hip_softmax"),
                                         ("loss", "hip_sm_grad_and_loss"), ("loss", "hip_sum_loss_over_imgs"), ("loss", "hip_accuracy"), ("loss", "hip_eval_accum")]
        assert len(ev.funcs) == 2 and all(c.rfc is d.rfc for c, d in zip([c for c in ev.eval_calls if c.fop.get_func_name() not in ("hip_accuracy", "hip_eval_accum")],
                                                                         [d for d in drv.bck_calls[:8] if d.tag != "drop1"]))
        assert theirs[3][:2] == ("drop1", "hip_dropout")
        assert {k: v.n for k, v in mine[-2][2].items()} == {"in": "fc", "label": "label", "rank": "eval_rank"}     # the LOGITS, not prob
        assert {k: v.n for k, v in mine[-1][2].items()} == {"rank": "eval_rank", "loss": "loss", "ctl": "eval_ctl", "counts": "eval_counts", "loss_sum": "eval_loss_sum"}
        assert ev.result()["batches"] == 0 and np.isnan(ev.result()["top1"])
        with pytest.raises(RtErr, match="no captured graph"):
            ev.run_batch({}, graph=True)
        ev.release()
    finally:
        drv.release()


def test_cpu_constructor_refusals(cpu):
    drv, bp = E.make_driver(cpu, "heads")
    try:
        for bad in (0, -1, 2.0, True):
            with pytest.raises(RtErr, match="top_k must be an int >= 1"):
                EvalPipe(drv, top_k=bad)
        with pytest.raises(RtErr, match="loss='fc_main' is no SoftmaxWithLoss top"):
            EvalPipe(drv, loss="fc_main")
        with pytest.raises(RtErr, match="an initialised ConvPipeBck"):
            EvalPipe(ConvPipeBck(cpu))
        with pytest.raises(RtErr):
            cpu.get_var_dims(EVAL_CTL_VAR)     # nothing was created
    finally:
        drv.release()
    p = ConvPipe("clash", "data", Dims.make("float", img=2, chan=3, y=5, x=5))     # a node of the pipe has a name the pass needs
    _conv(p, "eval_rank", "data", 4, 3, 1)
    from boda_amd.conv_pipe import PipeOp
    p.add(PipeOp("fc", "Convolution", "eval_rank", "fc", out_chans=N_CLASS, kern_sz=(0, 0)))
    drv = ConvPipeBck(cpu); drv.init(add_bck_ops(p), small_params(p, 0))
    try:
        with pytest.raises(RtErr, match="needs the var name 'eval_rank', which is a node of the pipe"):
            EvalPipe(drv)
        with pytest.raises(RtErr):
            cpu.get_var_dims(EVAL_CTL_VAR)
    finally:
        drv.release()


@pytest.mark.parametrize("img_chunks", [0, 3])
def test_cpu_residual_uses_the_running_pair(cpu, img_chunks):
    E.check_residual_uses_the_running_pair(cpu, img_chunks)


@pytest.mark.parametrize("name", ["chain", "residual"])
def test_cpu_training_is_undisturbed(cpu, name):
    E.check_training_is_undisturbed(cpu, name)
