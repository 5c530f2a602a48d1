"""The full SoftmaxWithLoss without a GPU: LossSpec and add_bck_ops' loss_specs, the rows of the native table, the three function ops against
tests/golden/ops/loss-ops.txt, every refusal, the functions on be=cpu -- hip_softmax_loss_fwd against the float64 formulas under the written bounds, hip_loss_norm and
hip_softmax_loss_bck bit for bit against the numpy twins (tests/loss_ref.py) --, and the driver on be=cpu: weighted heads, a dense head with an ignore_label, the
multi-device refusal, EvalPipe.  Every bounded check prints its worst |err| / bound (run with -s)."""
import os

import numpy as np
import pytest

import loss_ref as R
from boda_amd import rtc as rtc_mod
from boda_amd.bck_graph import GradOp, LossSpec, add_bck_ops
from boda_amd.bck_pipe import ConvPipeBck
from boda_amd.cnn_op import LOSS_FUNCS, LOSS_OP_FUNCS, NATIVE_ARGS, loss_norm_func_op, pipe_func_args, softmax_loss_bck_func_op, softmax_loss_fwd_func_op
from boda_amd.conv_pipe import ConvPipe, PipeOp, _conv
from boda_amd.eval_pipe import EvalPipe
from boda_amd.op import Dims, RtErr, UnsupErr, read_ops
from boda_amd.rtc import RtcFuncInfo, make_rtc

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
WORST = {}
SHAPES = [s for s, _ in R.SHAPES]


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


def within(name, got, want, bound, worst=WORST):
    err = np.abs(np.asarray(got, np.float64) - want)
    frac = float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))
    worst[name] = max(worst.get(name, 0.0), frac)
    print(f"{name}: worst |got - want| / bound = {frac:.3f}")
    assert frac <= 1.0, (name, frac)


# ---- the interface
def test_table_rows():
    table = rtc_mod.native_funcs()
    names = list(table)
    for member, (t, (fn,)) in enumerate(LOSS_OP_FUNCS.items(), 1):
        r = table[fn]
        assert (r["family"], r["member"], r["types"], r["multi_dev"], r["be"], r["flags"], r["opt"], r["why"]) == ("loss", member, (t,), "one_device", ("hip", "cpu"), (), (), ""), fn
    i = names.index("hip_data_transform")
    assert tuple(names[i - 3:i]) == LOSS_FUNCS and names[i:] == ["hip_data_transform", "hip_accuracy", "hip_eval_accum", "hip_bn_fold"]   # in front of the last four


def test_function_ops_match_the_golden_list():
    want = read_ops(os.path.join(HERE, "golden", "ops", "loss-ops.txt"))
    got = R.golden_specs()
    assert [o.to_str() for o in got] == [o.to_str() for o in want]
    for f in got:
        assert rtc_mod.func_args(f) == pipe_func_args(f) == NATIVE_ARGS[f.get_func_name()]
        g = f.loss_geom()
        assert g["form"] == R.form_of((g["B"], g["C"] or 1, 1, g["HW"]))
    forms = {(f.get_dims("in").sizes): f.loss_geom()["form"] for f in got if f.get_func_name() == "hip_softmax_loss_fwd"}
    assert forms == {s: w for s, w in R.SHAPES}
    plans = {f.get_dims("in").sizes: rtc_mod.explain_plan(f) for f in got if f.get_func_name() == "hip_softmax_loss_fwd"}
    assert "form=pel -DCREG=5" in plans[(2, 5, 9, 9)] and "form=wave" in plans[(2, 5, 9, 7)] and "form=pel -DCREG=0" in plans[(1, 70, 8, 8)] and "form=wave" in plans[(1, 3, 1, 63)] and "form=pel" in plans[(2, 1, 8, 8)]


def tiny(B=2, y=9, x=7, C=5):
    p = ConvPipe("dense", "data", Dims.make("float", img=B, chan=3, y=y, x=x))
    p.add(PipeOp("score", "Convolution", "data", "score", out_chans=C, kern_sz=(3, 3), in_pad=(1, 1)))
    return p


def test_loss_spec_and_refusals():
    assert LossSpec() == LossSpec(1.0, None, "valid")
    for bad, m in ((LossSpec(normalization="mean"), "normalization must be"), (LossSpec(weight=float("inf")), "weight must be a finite"), (LossSpec(weight=float("nan")), "weight must be"),
                   (LossSpec(ignore_label=2.5), "ignore_label must be an integer"), (LossSpec(ignore_label="255"), "ignore_label must be an integer")):
        with pytest.raises(RtErr, match=m):
            add_bck_ops(tiny(), loss_specs=bad)
        with pytest.raises(RtErr, match=m):
            loss_norm_func_op(R.dims_of((2, 5, 9, 7)), bad)
    with pytest.raises(RtErr, match="2\\^24 or more"):
        add_bck_ops(tiny(B=64, y=512, x=512), loss_specs=LossSpec())
    with pytest.raises(RtErr, match="2\\^24 or more"):
        softmax_loss_fwd_func_op(R.dims_of((64, 2, 512, 512)), LossSpec())
    with pytest.raises(RtErr, match="no loss top"):
        add_bck_ops(tiny(), loss_specs={"nope": LossSpec()})
    with pytest.raises(RtErr, match="1 loss_specs for 2"):
        add_bck_ops(heads3(), loss_tops=["aux1", "aux2"], loss_specs=[LossSpec()])
    p = tiny(); p.add(PipeOp("gap", "Pooling", "score", "gap", kern_sz=None, avg_pool=1))
    with pytest.raises(RtErr, match="must share its plane"):
        add_bck_ops(p, loss_tops=["score", "gap"])
    # a larger plane without a spec behaves as if given LossSpec(); a 1 x 1 head without one keeps spec None
    bp = add_bck_ops(tiny())
    assert bp.fwd_ops()[-1].spec == LossSpec() and bp.nodes["label"] == Dims.make("float", img=2, y=9, x=7)
    assert add_bck_ops(heads3(), loss_tops=HEADS).fwd_ops()[-1].spec is None and GradOp("t", "ReLU", ["a"], ["a"]).spec is None
    got = [o.spec for o in add_bck_ops(heads3(), loss_tops=HEADS, loss_specs={"main": LossSpec(0.5)}).fwd_ops()[-3:]]
    assert got == [None, None, LossSpec(0.5)]


def test_cpu_refuses_wrong_vars_and_ops(cpu):
    fop = loss_norm_func_op(R.dims_of((2, 5, 9, 7)), LossSpec())
    bad = fop.copy(); bad.str_vals["normalization"] = "mean"
    with pytest.raises(RtErr, match="normalization must be valid \\| full \\| batch_size \\| none"):
        cpu.compile([RtcFuncInfo("lt_bad", "", [a for a, _ in NATIVE_ARGS["hip_loss_norm"]], bad)])
    with pytest.raises(RtErr, match="the op says"):
        R.bare_run(cpu, fop, {"label": Dims.make("float", img=2, y=9, x=8)})
    with pytest.raises(RtErr, match="has type"):
        R.bare_run(cpu, fop, {"loss_state": Dims(("v",), (4,), "uint32_t")})


# ---- the functions on be=cpu
def check_fwd(rtc, shape, kind, name, lab, ig, worst, kernel=None):
    """One forward call against the float64 formulas; -> (prob, loss_per_pel) as the backend left them."""
    C = shape[1]
    spec = LossSpec(1.0, ig, "valid")
    x = R.logits(shape, kind)
    got = R.run_func(rtc, softmax_loss_fwd_func_op(R.dims_of(shape), spec), {"in": x, "label": lab}, kernel=kernel)
    want = R.softmax_f64(x)
    assert np.all(np.isfinite(got["prob"])) and np.all(np.isfinite(got["loss_per_pel"]))
    within(f"prob/{R.form_of(shape)}", got["prob"], want, R.prob_bound(want, C), worst)
    own = R.lpp_f64(got["prob"], lab, spec)
    within("loss_per_pel", got["loss_per_pel"], own, R.lpp_bound(own), worst)
    ignored, valid, _ = R.classes(lab, C, spec)
    assert np.all(R.bits(got["loss_per_pel"])[ignored] == 0)
    assert np.all(R.bits(got["loss_per_pel"])[~ignored & ~valid] == R.bits(R.INVALID_LOSS))
    return got["prob"], got["loss_per_pel"]


@pytest.mark.parametrize("shape", SHAPES, ids=R.SID)
def test_cpu_fwd_against_float64(cpu, shape):
    for name, lab, ig, meant in R.label_sets(shape):
        spec = LossSpec(1.0, ig, "valid")
        assert int(R.classes(lab, shape[1], spec)[0].sum()) == meant, (name, meant)
        for kind in (R.DATA if name in ("valid", "ign255") else ("pm4",)):
            prob, lpp = check_fwd(cpu, shape, kind, name, lab, ig, WORST)
            if shape[1] == 1:
                assert np.all(prob == 1.0) and np.all(lpp[R.classes(lab, 1, spec)[1]] == 0.0)


def check_norm_and_bck(rtc, shape, other=None, kernels=False):
    """hip_loss_norm and hip_softmax_loss_bck on host-made inputs, over every label set x normalisation x weight: bit for bit against the twins (and `other`, a second backend)."""
    C = shape[1]
    prob = R.softmax_f64(R.logits(shape, "pm4", seed=3)).astype(F)
    d = R.dims_of(shape)
    for name, lab, ig, meant in R.label_sets(shape):
        lpp = R.lpp_of_prob_f32(prob, lab, LossSpec(1.0, ig))
        for nz in R.NORMS:
            for w in R.WEIGHTS:
                spec = LossSpec(w, ig, nz)
                ins = {"label": lab, "loss_per_pel": lpp}
                got = R.run_func(rtc, loss_norm_func_op(d, spec), ins, kernel=R.KERNELS["hip_loss_norm"] if kernels else None)
                loss, state = R.norm_f32(lab, lpp, spec)
                n = lab.size
                assert state[2] == n - meant and state[0] == {"valid": max(1, n - meant), "full": n, "batch_size": shape[0], "none": 1}[nz]   # count and Z: exact
                assert R.bits_eq(got["loss"], loss) and R.bits_eq(got["loss_state"], state), (name, nz, w)
                ins_b = {"prob": prob, "label": lab, "loss_state": state}
                gb = R.run_func(rtc, softmax_loss_bck_func_op(d, spec), ins_b, kernel=R.KERNELS["hip_softmax_loss_bck"] if kernels else None)["in_grad_loss"]
                assert R.bits_eq(gb, R.bck_f32(prob, lab, state, spec)), (name, nz, w)
                ignored = R.classes(lab, C, spec)[0]
                assert np.all(R.bits(gb)[np.broadcast_to(ignored[:, None], gb.shape)] == 0)   # +0 bits in every channel of an ignored pel
                if meant == n:
                    assert R.bits(got["loss"]).item() == 0 and not np.any(R.bits(gb)) and not np.any(np.isnan(got["loss_state"]))
                if other is not None:
                    o = R.run_func(other, loss_norm_func_op(d, spec), ins)
                    assert R.bits_eq(got["loss"], o["loss"]) and R.bits_eq(got["loss_state"], o["loss_state"])
                    assert R.bits_eq(gb, R.run_func(other, softmax_loss_bck_func_op(d, spec), ins_b)["in_grad_loss"])


@pytest.mark.parametrize("shape", SHAPES, ids=R.SID)
def test_cpu_norm_and_bck_bits(cpu, shape):
    check_norm_and_bck(cpu, shape)


def order_inputs():
    """816 pels whose sum depends on the order: thread 0's chain is 2^24, 1, 1, 1 -- sequentially from +0 it stays 2^24; a tree or a pairwise order gives 2^24 + 2 or + 4."""
    lpp = np.zeros(R.BIG[0] * R.BIG[2] * R.BIG[3], F)
    lpp[0] = 2.0 ** 24; lpp[256] = 1.0; lpp[512] = 1.0; lpp[768] = 1.0
    lpp[1] = 1.0; lpp[129] = 1.0   # the tree: s[1] + s[129] = 2 at h = 128, then 2^24 + 2 at h = 1 -- not 2^24 + 1 + 1
    return lpp.reshape(R.BIG[0], R.BIG[2], R.BIG[3])


def check_order(rtc, kernel=None):
    lpp = order_inputs(); lab = np.zeros(lpp.shape, F)
    spec = LossSpec(1.0, None, "none")
    got = R.run_func(rtc, loss_norm_func_op(R.dims_of(R.BIG), spec), {"label": lab, "loss_per_pel": lpp}, kernel=kernel)
    assert got["loss"].item() == 2.0 ** 24 + 2.0 and R.bits_eq(got["loss"], R.norm_f32(lab, lpp, spec)[0])
    assert float(np.sum(lpp, dtype=np.float64)) == 2.0 ** 24 + 5.0   # what an exact sum gives


def test_cpu_loss_sum_is_the_written_chain(cpu):
    check_order(cpu)


# ---- the driver
HEADS = ["aux1", "aux2", "main"]


def heads3(B=4, C=7):
    """conv + ReLU -> two side convs and a main conv over the whole map: three 1 x 1 heads"""
    p = ConvPipe("heads3", "data", Dims.make("float", img=B, chan=3, y=6, x=6))
    _conv(p, "conv1", "data", 8, 3, 1)
    for t in HEADS:
        p.add(PipeOp(t, "Convolution", "conv1", t, out_chans=C, kern_sz=(0, 0)))
    return p


def pipe_inputs(cp, C, label_shape, seed=5):
    rng = np.random.default_rng(seed)
    params = {}
    for n, d in cp.params.items():
        params[n] = (rng.standard_normal(d.sizes) * 0.3).astype(F) if n.endswith("_filts") else rng.uniform(0.1, 0.5, d.sizes).astype(F)
    data = rng.uniform(-1, 1, cp.nodes["data"].sizes).astype(F)
    return params, data, rng.integers(0, C, label_shape).astype(F)


def step(rtc, cp, tops, specs, params, data, label, want):
    """One step on a driver of its own -> ([(tag, function name)] of its calls, its vars, {node: array}); the driver is released."""
    drv = ConvPipeBck(rtc); drv.init(add_bck_ops(cp, loss_tops=tops, loss_specs=specs), params)
    try:
        fwd = {"data": data, "label": label}
        drv.run_bck(["data", "label"], fwd, want)
        return [(t, f.get_func_name()) for t, f, _ in drv.calls()], list(drv.vars), fwd
    finally:
        drv.release()


def weighted_heads(rtc):
    """(a): the three-head net under weights w against the weighted sum of three one-head pipes -> {weights: (got, want)} for conv1_filts_grad_loss."""
    cp = heads3(); params, data, label = pipe_inputs(cp, 7, (4, 1, 1))
    single = {}
    for t in HEADS:
        one = {k: v for k, v in params.items() if k.startswith("conv1_") or k.startswith(t + "_")}
        p1 = ConvPipe("one", "data", cp.nodes["data"]); _conv(p1, "conv1", "data", 8, 3, 1); p1.add(PipeOp(t, "Convolution", "conv1", t, out_chans=7, kern_sz=(0, 0)))
        single[t] = step(rtc, p1, [t], LossSpec(), one, data, label, ["conv1_filts_grad_loss"])[2]["conv1_filts_grad_loss"].astype(np.float64)
    out = {}
    for ws in ((0.3, 0.3, 1.0), (0.0, 0.0, 1.0)):
        calls, _, fwd = step(rtc, cp, HEADS, [LossSpec(w) for w in ws], params, data, label, ["conv1_filts_grad_loss", "loss1", "loss2", "loss3"])
        assert [fn for _, fn in calls].count("hip_loss_norm") == 3
        out[ws] = (fwd["conv1_filts_grad_loss"], sum(float(F(w)) * single[t] for w, t in zip(ws, HEADS)))
    return out


def mrd(x, r):
    return float(np.max(np.abs(np.asarray(x, np.float64) - r)) / max(np.max(np.abs(r)), 1e-30))


def test_cpu_weighted_heads(cpu):
    for ws, (got, want) in weighted_heads(cpu).items():
        print(f"weights {ws}: mrd {mrd(got, want):.3e}")
        assert mrd(got, want) <= 1e-5 and np.any(want != 0)   # (the filter gradient's own bar, tests/test_bck_conv_cpu.py FILTS_MRD)


def dense_step(rtc, label):
    cp = tiny(); params, data, _ = pipe_inputs(cp, 5, (2, 9, 7))
    return step(rtc, cp, None, LossSpec(ignore_label=255), params, data, label, ["score", "loss", "loss_state", "score_grad_loss", "loss_per_pel", "loss_prob"])


def dense_labels(n_ignored, seed=8):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, 5, 126).astype(F)
    lab[rng.permutation(126)[:n_ignored]] = 255
    return lab.reshape(2, 9, 7)


def check_dense(rtc, worst):
    """(b): the dense head runs, the loss matches the float64 formulas on the backend's own logits, and a pel's gradient changes when, and only when, its label does."""
    lab = dense_labels(40)
    calls, vars, fwd = dense_step(rtc, lab)
    spec = LossSpec(ignore_label=255)
    w = R.loss_f64(fwd["score"], lab, spec)
    assert fwd["loss_state"][2] == 86 and fwd["loss_state"][0] == 86
    within("loss", fwd["loss"], w["loss"], R.loss_bound(w, 5), worst)
    within("gradient", fwd["score_grad_loss"], w["grad"], R.grad_bound(w, 5), worst)
    ig = np.argwhere(lab == 255)[0]; lab2 = lab.copy(); lab2[tuple(ig)] = 3.0   # one pel: ignored -> class 3.  Z moves from 86 to 87, so every gradient is rescaled ...
    fwd2 = dense_step(rtc, lab2)[2]
    g1, g2 = fwd["score_grad_loss"] / fwd["loss_state"][1], fwd2["score_grad_loss"] / fwd2["loss_state"][1]   # ... which dividing by s takes out again
    changed = np.any(np.abs(g1 - g2) > 1e-5, axis=1)
    assert changed[tuple(ig)] and changed.sum() == 1
    assert not np.any(fwd["score_grad_loss"][ig[0], :, ig[1], ig[2]]) and np.any(fwd2["score_grad_loss"][ig[0], :, ig[1], ig[2]])
    assert [fn for t, fn in calls if t == "loss"] == ["hip_softmax_loss_fwd", "hip_loss_norm", "hip_softmax_loss_bck"]
    assert {"loss_prob", "loss_per_pel", "loss_state"} <= set(vars)


def test_cpu_dense_head(cpu):
    check_dense(cpu, WORST)


class _TwoDevices:
    """What plan() asks of a backend: nothing but its device list.  A backend call would be an AttributeError."""
    devices = [0, 0]


def test_devices_refuse_a_spec_before_anything_exists():
    bp = add_bck_ops(tiny(), loss_specs=LossSpec(ignore_label=255))
    drv = ConvPipeBck(_TwoDevices())
    with pytest.raises(UnsupErr, match="the loss 'loss' has a LossSpec.*multi-device"):
        drv.init(bp)
    assert drv.vars == [] and not drv.bck_calls


def eval_heads(rtc, worst):
    """(e): EvalPipe on the three-head net with specs against the pipe without: the main head's loss within the loss bound, the same counts."""
    cp = heads3(); params, data, label = pipe_inputs(cp, 7, (4, 1, 1))
    res = []
    for specs in ([LossSpec(0.3), LossSpec(0.3), LossSpec(1.0)], None):
        drv = ConvPipeBck(rtc); drv.init(add_bck_ops(cp, loss_tops=HEADS, loss_specs=specs), params)
        ev = EvalPipe(drv, top_k=3)
        if specs:
            assert [c.fop.get_func_name() for c in ev.eval_calls][-4:] == ["hip_softmax_loss_fwd", "hip_loss_norm", "hip_accuracy", "hip_eval_accum"]
        ev.reset()
        ev.run_batch({"data": data, "label": label})
        res.append((ev.result(), rtc.copy_var_to_nda("main")))
        ev.release(); drv.release()
    (a, logits), (b, _) = res
    w = R.loss_f64(logits, label, LossSpec())
    assert (a["top1"], a["topk"], a["images"]) == (b["top1"], b["topk"], b["images"])
    within("eval loss", a["loss"], w["loss"], R.loss_bound(w, 7), worst)
    within("eval loss (unspec'd pipe)", b["loss"], w["loss"], R.loss_bound(w, 7) + 16 * R.U * abs(w["loss"]), {})
    for cp, tops, m in ((tiny(), None, "accuracy over a plane or with an ignore_label is not built"), (heads3(), HEADS, "ignore_label=-1")):
        drv = ConvPipeBck(rtc); drv.init(add_bck_ops(cp, loss_tops=tops, loss_specs=LossSpec(ignore_label=255 if tops is None else -1)))
        try:
            with pytest.raises(UnsupErr, match=m):
                EvalPipe(drv)
        finally:
            drv.release()


def test_cpu_eval_pipe(cpu):
    eval_heads(cpu, WORST)


NIN_TINY_CALLS = ["hip_conv", "hip_conv", "hip_pool_yx", "hip_dropout", "hip_conv", "hip_pool_yx", "hip_softmax", "hip_sm_grad_and_loss", "hip_sum_loss_over_imgs", "hip_spreading",
                  "hip_zero_if_non_pos", "hip_bconv_in", "hip_bconv_biases", "hip_bconv_filts", "hip_dropout", "hip_spreading", "hip_zero_if_non_pos", "hip_bconv_in",
                  "hip_bconv_biases", "hip_bconv_filts", "hip_zero_if_non_pos", "hip_bconv_in", "hip_bconv_biases", "hip_bconv_filts"]


def nin_tiny(B=2):
    """NiN's shape in small: conv + ReLU -> 1x1 conv + ReLU -> max pool -> Dropout -> 1x1 conv + ReLU to the classes -> global average pool -> loss"""
    p = ConvPipe("nin_tiny", "data", Dims.make("float", img=B, chan=3, y=9, x=9))
    _conv(p, "conv1", "data", 8, 3, 1); _conv(p, "cccp1", "conv1", 6, 1)
    p.add(PipeOp("pool1", "Pooling", "cccp1", "pool1", kern_sz=(3, 3), stride=(2, 2)))
    p.add(PipeOp("drop", "Dropout", "pool1", "pool1"))
    _conv(p, "cccp2", "pool1", 5, 1)
    p.add(PipeOp("gap", "Pooling", "cccp2", "gap", kern_sz=None, avg_pool=1))
    return p


def test_without_a_spec_the_call_list_is_the_parents(cpu):
    drv = ConvPipeBck(cpu); drv.init(add_bck_ops(nin_tiny()))
    assert [f.get_func_name() for _, f, _ in drv.calls()] == NIN_TINY_CALLS
    assert "loss_state" not in drv.vars and not any(f.get_func_name() in LOSS_FUNCS for _, f, _ in drv.calls())
    drv.release()
    spec = ConvPipeBck(cpu); spec.init(add_bck_ops(nin_tiny(), loss_specs=LossSpec()))
    got = [f.get_func_name() for _, f, _ in spec.calls()]
    spec.release()
    assert got[6:9] == list(LOSS_FUNCS) and got[:6] + got[9:] == NIN_TINY_CALLS[:6] + NIN_TINY_CALLS[9:]


def test_print_worst():
    print("loss, be=cpu: worst |err| / bound per check:", {k: round(v, 3) for k, v in sorted(WORST.items())})
