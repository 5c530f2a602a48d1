"""The evaluation pass on the MI355X: bodahip_accuracy, bodahip_eval_accum and bodahip_bn_fold (kernels/eval_f32.hip) word for word against their twins
(tests/eval_ref.py; hip_bn_fold against conv_pipe.fold_affine) from pre-filled outputs and with guard vars, and EvalPipe on be=hip: the test-phase pass, its result
against the twins on the backend's own logits and losses, every call against be=cpu by the function's own rule, the side-effect contract, and a training run -- eager,
and with BOTH graphs captured and their replays interleaved -- that evaluations leave undisturbed.

Everything is integers or a written fp32 chain, so the bars are equalities.  The one bound: hip_softmax sums in another order than be=cpu, so an eval loss compared
ACROSS backends takes the bound tests/test_gpu_bck_ops.py holds that function and the loss to (test_chained_softmax_loss_end_to_end): per image (chan + 8) u (1 + 2 (chan
+ 8) u) + 4 u max(1, |want|), averaged, plus (B + 1) u sum|want| / B for the chain and the divide -- against float64 on the logits, which on `fan` are the same bits on
both backends."""
import numpy as np
import pytest

import bck_ops_ref as oref
import eval_ref as E
from boda_amd.cnn_op import pipe_func_args
from boda_amd.eval_pipe import EvalPipe
from boda_amd.op import UnsupErr
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc

from test_gpu_bck_pipe import BIT_EXACT, check_call

pytestmark = pytest.mark.gpu
F, U32 = np.float32, np.uint32
EVAL_BIT_EXACT = BIT_EXACT | {"hip_accuracy", "hip_eval_accum", "hip_bn_fold", "hip_chan_affine"}     # (hip_chan_affine: bit for bit, tests/test_gpu_resnet.py)


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


# ---- 1. the three functions
@pytest.mark.parametrize("C", E.ACC_CHANS)
def test_accuracy(hip, C):
    keep = []
    E.check_accuracy(hip, C, keep=keep)
    for k, B in zip(keep, E.ACC_IMGS):
        assert k["kernel"] == "bodahip_accuracy" and k["kernels"] == 1 and k["grid"] == -(-B // 4) and k["block"] == 256, k


@pytest.mark.parametrize("B", E.ACCUM_IMGS)
def test_eval_accum(hip, B):
    for top_k in E.ACCUM_TOP_KS:
        keep = []
        E.check_eval_accum(hip, B, top_k, keep=keep)
        for k in keep:
            assert k["kernel"] == "bodahip_eval_accum" and k["kernels"] == 1 and k["grid"] == 1 and k["block"] == 256, k


@pytest.mark.parametrize("C", E.FOLD_CHANS)
def test_bn_fold(hip, C):
    for eps in (E.FOLD_EPS, 0.0):
        keep = []
        E.check_bn_fold(hip, C, eps, keep=keep)
        assert keep[0]["kernel"] == "bodahip_bn_fold" and keep[0]["kernels"] == 1 and keep[0]["grid"] == -(-C // 256), keep


# ---- 2. the pass
def test_chain_is_the_pipe_without_dropout(hip):
    E.check_chain_is_the_pipe_without_dropout(hip)


@pytest.mark.parametrize("name,loss", [("fan", None), ("heads", "loss1"), ("heads", "loss2")])
def test_result_is_the_twin(hip, name, loss):
    E.check_result_is_the_twin(hip, name, loss)


def test_result_from_graph_replays(hip):
    E.check_result_is_the_twin(hip, "heads", "loss2", graph=True)


def loss_bound(z, label):
    """(float64 loss on the logits z, the bound of tests/test_gpu_bck_ops.py's end-to-end chain for it)."""
    B, C = z.shape[:2]
    lab = np.asarray(label, F).reshape(B)
    valid = (lab >= 0) & (lab < C)     # an invalid label: hip_sm_grad_and_loss takes prob = 0, so the image's loss is -log(FLT_MIN) (kernels/bck_ops_f32.hip OP 7)
    wl = oref.loss_per_pel_f64(oref.softmax_f64(z), np.where(valid, lab, 0).reshape(B, 1, 1)).reshape(B)
    wl = np.where(valid, wl, -np.log(np.float64(np.finfo(F).tiny)))
    pb = (C + 8) * oref.U
    lb = pb * (1 + 2 * pb) + 4 * oref.U * np.maximum(1.0, np.abs(wl))
    return float(wl.mean()), float(lb.mean() + (B + 1) * oref.U * np.abs(wl).sum() / B)


def test_eval_loss_across_backends(hip, cpu):
    """`fan` has no function with a bound in front of the loss: the logits are the same bits on both backends, the counts therefore equal, and the two losses each lie
    within the loss chain's bound of the float64 loss on those logits."""
    g, zg, wg = E.check_result_is_the_twin(hip, "fan")
    c, zc, wc = E.check_result_is_the_twin(cpu, "fan")
    assert {k: v for k, v in g.items() if k != "loss"} == {k: v for k, v in c.items() if k != "loss"}
    want, bound = 0.0, 0.0
    for k in range(3):
        assert zg[k].tobytes() == zc[k].tobytes(), (k, "the logits differ across the backends")
        w, b = loss_bound(zg[k], E.eval_feed("fan", E.PIPES["fan"][0](), k)["label"])
        for got in (wg[k], wc[k]):
            assert abs(got.item() - w) <= b, (k, got.item(), w, b)
        want += w / 3; bound += b / 3
    bound += 4 * oref.U * abs(want)     # (the two adds of loss_sum and the host's divide)
    print("eval loss hip %.9g cpu %.9g float64 %.9g bound %.3g" % (g["loss"], c["loss"], want, bound))
    assert abs(g["loss"] - want) <= bound and abs(c["loss"] - want) <= bound


@pytest.mark.parametrize("img_chunks", [0, 3])
def test_residual_uses_the_running_pair(hip, img_chunks):
    E.check_residual_uses_the_running_pair(hip, img_chunks)


def run_typed(rtc, fop, ins):
    """One call of an eval-family function on `rtc` from host inputs -> {arg: array} of its OUT and INOUT args."""
    (seen,), _ = E.run_steps(rtc, "cbc", fop, ins, [{}])
    return {an: seen[an] for an, io in pipe_func_args(fop) if io in ("OUT", "INOUT")}


@pytest.mark.parametrize("name", ["chain", "heads", "residual"])
def test_eval_pass_call_by_call(hip, cpu, name):
    """Every call of an eval batch on the GPU and the same function on be=cpu on the GPU's own inputs, by each function's existing rule (tests/test_gpu_bck_pipe.py's
    check_call), the three new functions and hip_chan_affine bit for bit."""
    drv, bp = E.make_driver(hip, name)
    try:
        if name == "residual":
            data, label = E.inputs_of(name, bp.cp, 0)
            drv.run_bck(["data", "label"], {"data": data, "label": label}, [])     # (a running pair that has moved)
        ev = EvalPipe(drv, top_k=2)
        ev.run_batch(E.eval_feed(name, bp.cp, 0)); ev.run_batch(E.eval_feed(name, bp.cp, 2))     # (every kernel built, every var holding sane data, every label valid -- check_call's float64 loss knows no other; ctl says `add`)
        seen = []
        for c in ev.eval_calls:
            fn = c.fop.get_func_name()
            if fn in ("hip_accuracy", "hip_eval_accum", "hip_bn_fold", "hip_chan_affine"):
                spec = [(an, io) for an, io in pipe_func_args(c.fop)]
                am = c.rfc.arg_map
                ins = {an: hip.copy_var_to_nda(am[an].n) for an, io in spec}
                hip.run(c.rfc); hip.finish_and_sync()
                assert hip.last_launch()["kernel"] == "bodahip_" + fn[4:], (c.tag, hip.last_launch())
                want = run_typed(cpu, c.fop, ins)
                for an in want:
                    assert E.same_bits(hip.copy_var_to_nda(am[an].n), want[an]), (c.tag, fn, an)
            else:
                check_call(hip, cpu, c.tag, c.fop, c.rfc)
            assert fn in EVAL_BIT_EXACT or fn in ("hip_lrn_sb", "hip_softmax", "hip_sm_grad_and_loss"), fn
            seen.append(fn)
        hip.release_per_call_id_data()
        assert seen[-2:] == ["hip_accuracy", "hip_eval_accum"] and ("hip_bn_fold" in seen) == (name == "residual")
        ev.release()
    finally:
        drv.release()


# ---- 3. training is undisturbed
@pytest.mark.parametrize("name", ["chain", "residual"])
def test_training_is_undisturbed(hip, name):
    E.check_training_is_undisturbed(hip, name)


@pytest.mark.parametrize("name", ["chain", "residual"])
def test_training_is_undisturbed_with_both_graphs_interleaved(hip, name):
    """The driver's graph and the EvalPipe's graph both captured, every pass and every eval batch a replay, against the eager run without evaluations."""
    E.check_training_is_undisturbed(hip, name, graph=True)


def test_capturing_either_graph_keeps_the_other(hip):
    drv, bp = E.make_driver(hip, "chain", seed_in_var=True)
    try:
        ev = EvalPipe(drv, top_k=2)
        n_ev = ev.capture_graph()
        assert drv.capture_graph() == len(drv.calls()) and n_ev == len(ev.calls())     # (the driver's capture behind the EvalPipe's)
        feed = lambda i: E.eval_feed("chain", bp.cp, i)
        a = ev.evaluate(2, feed, graph=True)
        assert ev.capture_graph() == n_ev     # (a second capture of the EvalPipe's: the driver's graph stays)
        data, label = E.inputs_of("chain", bp.cp, 0)
        fwd = {"data": data, "label": label}
        drv.run_bck(["data", "label"], fwd, ["loss"], graph=True)
        assert np.isfinite(fwd["loss"]).all()
        assert ev.evaluate(2, feed, graph=True) == a == ev.evaluate(2, feed)     # a replay and an eager batch leave the same words
        ev.release()
        drv.run_bck(["data", "label"], fwd, ["loss"], graph=True)     # release() leaves the driver and its graph usable
    finally:
        drv.release()


def test_multi_device_is_refused_before_anything_exists():
    multi = make_rtc("(be=hip,devices=0:0)"); multi.init()
    try:
        drv, bp = E.make_driver(multi, "fan")
        try:
            with pytest.raises(UnsupErr, match="EvalPipe: not provided on a multi-device backend"):
                EvalPipe(drv)
            for vn in ("eval_ctl", "eval_counts", "eval_loss_sum", "eval_rank"):
                with pytest.raises(Exception):
                    multi.get_var_dims(vn)
        finally:
            drv.release()
    finally:
        multi.close()
