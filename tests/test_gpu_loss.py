"""The full SoftmaxWithLoss on the MI355X (kernels/loss_f32.hip) through the C ABI.  Inputs come from the host (fixed seeds); every run asserts
the launched kernel's name, fills its outputs with a payload NaN first and checks a guard var in front of and behind every var (tests/loss_ref.py run_func).

BOUNDED against the float64 formulas on the same fp32 inputs (u = 2^-24; the bounds of tests/loss_ref.py, derived there): hip_softmax_loss_fwd's prob in both forms and its
loss_per_pel against -log of its OWN stored prob[L]; chained on the device, the gradient and the loss end to end.
BIT-IDENTICAL to the numpy twins and to be=cpu: hip_loss_norm (count and Z exact, the loss sum in its written chain of ceil(N / 256) + 8 adds) and hip_softmax_loss_bck on
host-made inputs; every function run to run; a replayed graph against the eager step.
The driver on be=hip: weighted heads, a dense head with an ignore_label, one captured graph under label planes with different numbers of ignored pels, the
multi-device refusal and EvalPipe.  Every bounded check prints its worst |err| / bound (run with -s); the last test prints the maxima section 3.23 records."""
import numpy as np
import pytest

import loss_ref as R
import test_loss_cpu as T
from boda_amd.bck_graph import LossSpec, add_bck_ops
from boda_amd.bck_pipe import ConvPipeBck
from boda_amd.cnn_op import NATIVE_ARGS, loss_norm_func_op, softmax_loss_bck_func_op, softmax_loss_fwd_func_op
from boda_amd.op import UnsupErr
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc

pytestmark = pytest.mark.gpu
F = np.float32
WORST = {}
K = R.KERNELS


@pytest.fixture(scope="module")
def hip():
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


@pytest.mark.parametrize("shape", T.SHAPES, ids=R.SID)
def test_fwd_against_float64(hip, shape):
    for name, lab, ig, meant in R.label_sets(shape):
        assert int(R.classes(lab, shape[1], LossSpec(1.0, ig))[0].sum()) == meant, (name, meant)
        for kind in (R.DATA if name in ("valid", "ign255") else ("pm4",)):
            prob, lpp = T.check_fwd(hip, shape, kind, name, lab, ig, WORST, kernel=K["hip_softmax_loss_fwd"])
            if shape[1] == 1:
                assert np.all(prob == 1.0) and np.all(lpp[R.classes(lab, 1, LossSpec(1.0, ig))[1]] == 0.0)


@pytest.mark.parametrize("shape", T.SHAPES, ids=R.SID)
def test_norm_and_bck_bits(hip, cpu, shape):
    T.check_norm_and_bck(hip, shape, other=cpu, kernels=True)


def test_loss_sum_is_the_written_chain(hip):
    T.check_order(hip, kernel=K["hip_loss_norm"])


def test_same_bits_run_to_run(hip):
    shape = R.BIG; d = R.dims_of(shape)
    name, lab, ig, _ = R.label_sets(shape)[1]
    spec = LossSpec(0.3, ig, "valid")
    x = R.logits(shape, "wide")
    a, b = (R.run_func(hip, softmax_loss_fwd_func_op(d, spec), {"in": x, "label": lab}, kernel=K["hip_softmax_loss_fwd"]) for _ in range(2))
    assert R.bits_eq(a["prob"], b["prob"]) and R.bits_eq(a["loss_per_pel"], b["loss_per_pel"])
    ins = {"label": lab, "loss_per_pel": a["loss_per_pel"]}
    n1, n2 = (R.run_func(hip, loss_norm_func_op(d, spec), ins, kernel=K["hip_loss_norm"]) for _ in range(2))
    assert R.bits_eq(n1["loss"], n2["loss"]) and R.bits_eq(n1["loss_state"], n2["loss_state"])
    ins = {"prob": a["prob"], "label": lab, "loss_state": n1["loss_state"]}
    g1, g2 = (R.run_func(hip, softmax_loss_bck_func_op(d, spec), ins, kernel=K["hip_softmax_loss_bck"])["in_grad_loss"] for _ in range(2))
    assert R.bits_eq(g1, g2)


@pytest.mark.parametrize("shape", [(3, 21, 16, 17), (1, 70, 8, 8), (4, 1000, 1, 1), (2, 70, 2, 3)], ids=R.SID)
def test_chained_on_the_device_end_to_end(hip, shape):
    """fwd -> norm -> bck with the vars kept on the device, against float64 on the logits: the gradient within s ((C + 8) u p + 4 u |p - d|), the loss within
    (depth + 2) u SUM|loss_per_pel| + SUM(per-pel bound), depth = ceil(N / 256) + 8."""
    C = shape[1]; d = R.dims_of(shape)
    for (name, lab, ig, _), nz, wgt, kind in zip(R.label_sets(shape)[:4], R.NORMS, (1.0, 0.3, 0.3, 1.0), ("pm4", "wide", "low", "pm4")):
        spec = LossSpec(wgt, ig, nz)
        x = R.logits(shape, kind, seed=2)
        fops = {"f": softmax_loss_fwd_func_op(d, spec), "n": loss_norm_func_op(d, spec), "b": softmax_loss_bck_func_op(d, spec)}
        hip.compile([RtcFuncInfo("lc_" + k, "", [a for a, _ in NATIVE_ARGS[f.get_func_name()]], f) for k, f in fops.items()])
        vars = {"in": d, "prob": d, "in_grad_loss": d, "label": fops["n"].get_dims("label"), "loss_per_pel": fops["n"].get_dims("label"), "loss": fops["n"].get_dims("loss"),
                "loss_state": fops["n"].get_dims("loss_state")}
        try:
            for vn, dd in vars.items():
                hip.create_var_with_dims("lc_" + vn, dd)
            hip.copy_nda_to_var("lc_in", x); hip.copy_nda_to_var("lc_label", lab)
            for k, f in fops.items():
                hip.run(RtcFuncCall("lc_" + k, {a: RtcArg.var("lc_" + a) for a, _ in NATIVE_ARGS[f.get_func_name()]}))
                assert hip.last_launch()["kernel"] == K[f.get_func_name()]
            hip.finish_and_sync()
            got = {vn: hip.copy_var_to_nda("lc_" + vn) for vn in ("in_grad_loss", "loss", "loss_state")}
        finally:
            for vn in vars:
                hip.release_var("lc_" + vn)
            for k in fops:
                hip.release_func("lc_" + k)
            hip.release_per_call_id_data()
        w = R.loss_f64(x, lab, spec)
        assert got["loss_state"][2] == w["count"] and got["loss_state"][0] == w["Z"]
        T.within("chained gradient", got["in_grad_loss"], w["grad"], R.grad_bound(w, C), WORST)
        T.within("chained loss", got["loss"], w["loss"], R.loss_bound(w, C), WORST)


# ---- the driver
def test_weighted_heads(hip, cpu):
    """(a) on be=hip: against the weighted sum of three one-head pipes, and against be=cpu's three-head step, under the filter gradient's own bar."""
    on_cpu = T.weighted_heads(cpu)
    for ws, (got, want) in T.weighted_heads(hip).items():
        print(f"weights {ws}: mrd to the weighted sum {T.mrd(got, want):.3e}, to be=cpu {T.mrd(got, on_cpu[ws][0].astype(np.float64)):.3e}")
        assert T.mrd(got, want) <= 1e-5 and T.mrd(got, on_cpu[ws][0].astype(np.float64)) <= 1e-5


def test_dense_head(hip):
    T.check_dense(hip, WORST)


def test_one_graph_serves_label_planes_with_other_counts(hip):
    """(c): capture the dense step, serially and in parallel, then replay under a label plane with ANOTHER number of ignored pels: every node holds the eager step's
    bits for those labels.  A graph that had frozen s = weight / Z could not."""
    cp = T.tiny(); params, data, _ = T.pipe_inputs(cp, 5, (2, 9, 7))
    nodes = ["score", "loss_prob", "loss_per_pel", "loss", "loss_state", "score_grad_loss", "score_filts_grad_loss", "score_biases_grad_loss", "data_grad_loss"]
    lab_a, lab_b = T.dense_labels(40), T.dense_labels(11, seed=9)
    drv = ConvPipeBck(hip); drv.init(add_bck_ops(cp, loss_specs=LossSpec(0.3, 255)), params)
    try:
        eager = {"data": data, "label": lab_b}
        drv.run_bck(["data", "label"], eager, nodes)
        assert eager["loss_state"][2] == 126 - 11
        for parallel in (False, True):
            first = {"data": data, "label": lab_a}
            drv.run_bck(["data", "label"], first, nodes)
            assert first["loss_state"][2] == 126 - 40
            assert drv.capture_graph(parallel=parallel) == len(drv.calls())
            rep = {"data": data, "label": lab_b}
            drv.run_bck(["data", "label"], rep, nodes, graph=True)
            for n in nodes:
                assert R.bits_eq(rep[n], eager[n]), (parallel, n)
            assert not R.bits_eq(rep["score_grad_loss"], first["score_grad_loss"])
    finally:
        drv.release()


def test_two_devices_refuse_a_spec_before_any_var_exists():
    multi = make_rtc("(be=hip,devices=0:0)"); multi.init()
    try:
        drv = ConvPipeBck(multi)
        with pytest.raises(UnsupErr, match="the loss 'loss' has a LossSpec.*multi-device"):
            drv.init(add_bck_ops(T.tiny(), loss_specs=LossSpec(ignore_label=255)))
        assert drv.vars == [] and not drv.bck_calls
        for ctor in (softmax_loss_fwd_func_op, loss_norm_func_op, softmax_loss_bck_func_op):
            with pytest.raises(UnsupErr, match="the full softmax loss.*several devices is out of scope"):
                R.bare_run(multi, ctor(R.dims_of((4, 3, 2, 2)), LossSpec()))
    finally:
        multi.close()


def test_eval_pipe(hip):
    T.eval_heads(hip, WORST)


def test_print_worst():
    print("loss, be=hip: worst |err| / bound per check:", {k: round(v, 3) for k, v in sorted(WORST.items())})
