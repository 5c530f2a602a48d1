"""Deconvolution and Crop layers in the pipes on the MI355X: fcn_tiny's gradient step call by call -- every Deconvolution / Crop call against be=cpu on the GPU's own
inputs (the forward, the data gradient, the crops bit for bit; the filter gradient against oracle/bck_chain.py's chain on the exchanged roles with the launched
BK / KSL; the bias gradient against its tree), every other call run as it is (other files hold those functions) --, the captured step replayed against the eager
step, one solver step against be=cpu, and the forward pipe against the step's forward nodes."""
import numpy as np
import pytest

from boda_amd import conv_pipe
from boda_amd.bck_graph import LossSpec
from boda_amd.bck_pipe import ConvPipeBck, Solver, add_bck_ops
from boda_amd.cnn_op import pipe_func_args
from boda_amd.conv_pipe import ConvPipeFwd
from boda_amd.rtc import make_rtc
from oracle import bck_chain as bc

from deconv_ref import bits_equal, exchanged_geom, run_func
from test_deconv_pipe_cpu import CAP, fcn_params, inputs

pytestmark = pytest.mark.gpu


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


def make(rtc, **kw):
    cp = conv_pipe.fcn_tiny(2); bp = add_bck_ops(cp, loss_specs=LossSpec(ignore_label=255))
    params = fcn_params(bp)
    drv = ConvPipeBck(rtc, **kw); drv.init(bp, params)
    return drv, bp, params


def grad_nodes(drv, bp):
    return [n for n in bp.nodes if n.endswith("_grad_loss") and n in drv.vars]


def check_own_call(hip, cpu, tag, fop, rfc):
    """One Deconvolution / Crop call of the step on the GPU, and be=cpu's same function on the GPU's own inputs."""
    fn, am = fop.get_func_name(), rfc.arg_map
    ins = {an: hip.copy_var_to_nda(am[an].n) for an, io in pipe_func_args(fop) if io == "IN"}
    out_an = [an for an, io in pipe_func_args(fop) if io == "OUT"][0]
    hip.copy_nda_to_var(am[out_an].n, np.full(fop.get_dims(out_an).sizes, np.nan, np.float32))   # every element must be written
    hip.run(rfc); hip.finish_and_sync()
    launch = hip.last_launch()
    got = hip.copy_var_to_nda(am[out_an].n)
    if fn == "hip_deconv_bck_filts":
        cfg = launch["cfg"]
        bk, ksl = int(cfg.split("_")[0].split("x")[2]), (int(cfg.split("_s")[1].split("_")[0]) if "_s" in cfg else 1)
        g = fop.deconv_geom()
        case = (g["B"], g["C"], g["H"], g["W"], g["OC"], (g["KH"], g["KW"]), (g["SY"], g["SX"]), (g["PY"], g["PX"]))
        assert bits_equal(got, bc.filts_chain(ins["out_grad_loss"], ins["in"], exchanged_geom(case), bk, ksl)), (tag, fn, cfg)
    elif fn == "hip_deconv_bck_biases":
        assert bits_equal(got, bc.biases_chain(ins["out_grad_loss"])), (tag, fn)
    else:
        assert bits_equal(got, run_func(cpu, fop, ins)[0]), (tag, fn)
    return fn


def test_step_call_by_call(hip, cpu):
    drv, bp, params = make(hip)
    try:
        data, label = inputs(bp.cp, 2)
        fwd = {"data": data, "label": label}
        drv.run_bck(["data", "label"], fwd, grad_nodes(drv, bp) + bp.loss_nodes)   # one whole step first: every kernel specialised, every var holding sane data
        hip.copy_nda_to_var("data", data); hip.copy_nda_to_var("label", label)
        seen = []
        for c in drv.bck_calls:
            fn = c.fop.get_func_name()
            if fn.startswith(("hip_deconv", "hip_crop")):
                seen.append(check_own_call(hip, cpu, c.tag, c.fop, c.rfc))
            else:
                hip.run(c.rfc)
        hip.finish_and_sync(); hip.release_per_call_id_data()
        assert sorted(seen) == sorted(["hip_deconv", "hip_deconv_bck_in", "hip_deconv_bck_biases", "hip_deconv_bck_filts"] * 2 + ["hip_crop", "hip_crop_bck"] * 2)
        for n in grad_nodes(drv, bp):   # stepping through the calls one by one is the same step
            assert bits_equal(hip.copy_var_to_nda(n), fwd[n]), n
    finally:
        drv.release()


def test_captured_step_replays_the_eager_bits(hip):
    E, bp, params = make(hip)
    data, label = inputs(bp.cp, 2)
    try:
        gets = grad_nodes(E, bp) + bp.loss_nodes
        want = {"data": data, "label": label}
        E.run_bck(["data", "label"], want, gets)
    finally:
        E.release()
    G, bp, _ = make(hip, seed_in_var=True)
    try:
        assert G.capture_graph() == len(G.calls())
        got = {"data": data, "label": label}
        G.run_bck(["data", "label"], got, gets, graph=True)
        for n in gets:
            assert bits_equal(got[n], want[n]), n
        G.run_graph()
        for n in gets:
            assert bits_equal(hip.copy_var_to_nda(n), want[n]), ("replayed twice", n)
    finally:
        G.release()


def test_solver_step_and_forward_pipe_against_cpu(hip, cpu):
    """One SGD step on both backends from the same params and batch.  The two sides associate the filter / bias gradients and the loss's sums differently, so the loss
    and every gradient are held to the gradient pipes' cap of 5e-4 (of the node's largest element), and a param after the step to lr times that."""
    res = {}
    sv = dict(type="sgd", lr=0.05, momentum=0.9)
    for name, rtc in (("hip", hip), ("cpu", cpu)):
        drv, bp, params = make(rtc, solver=Solver(**sv))
        try:
            data, label = inputs(bp.cp, 2)
            fwd = {"data": data, "label": label}
            drv.run_bck(["data", "label"], fwd, grad_nodes(drv, bp) + bp.loss_nodes + ["up2", "score"])
            res[name] = (fwd, {p: rtc.copy_var_to_nda(p) for p in drv.sgd_params})
        finally:
            drv.release()
    (fh, ph), (fc, pc) = res["hip"], res["cpu"]
    assert bits_equal(fh["up2"], fc["up2"]) and bits_equal(fh["score"], fc["score"])   # the forward pass is be=cpu's bits
    assert abs(fh["loss"].item() - fc["loss"].item()) <= CAP * abs(fc["loss"].item())
    for p in ph:
        g = fc[p + "_grad_loss"]
        assert np.max(np.abs(fh[p + "_grad_loss"] - g)) <= CAP * np.max(np.abs(g)), p
        assert np.max(np.abs(ph[p] - pc[p])) <= sv["lr"] * CAP * np.max(np.abs(g)) + 2.0 ** -23 * np.max(np.abs(pc[p])), p
        assert not np.array_equal(pc[p], params[p])
    cp = conv_pipe.fcn_tiny(2)
    f = ConvPipeFwd(hip); f.init(cp, op_params=params)
    try:
        io = {"data": inputs(cp, 2)[0]}
        f.run_fwd(["data"], io, ["up2", "score"])
    finally:
        f.release()
    assert bits_equal(io["up2"], fc["up2"]) and bits_equal(io["score"], fc["score"])


def test_wide_layer_on_the_matrix_path(hip, cpu):
    """dec_tiny's Deconvolution 32 -> 32 takes the matrix path (hip_bconv_in + hip_chan_affine, hip_conv, hip_bconv_filts on views of the blob): the step on the GPU
    against be=cpu -- the forward nodes bit for bit, the loss and the gradients under the gradient pipes' cap --, the captured step, serial and with the calls'
    dependencies as edges (a call on a view is ordered as a call on its var), against the eager bits, and the forward pipe against the step's forward node."""
    from test_deconv_pipe_cpu import dec_step, dec_tiny
    res = {}
    for name, rtc in (("hip", hip), ("cpu", cpu)):
        drv, bp, params, fwd, ins = dec_step(rtc, gets=None)
        try:
            assert [f.get_func_name() for t, f, _ in drv.calls() if t in ("up", "up_bck")] == ["hip_bconv_in", "hip_chan_affine", "hip_conv", "hip_deconv_bck_biases", "hip_bconv_filts"]
            fwd["up"] = rtc.copy_var_to_nda("up")
            res[name] = fwd
        finally:
            drv.release()
    fh, fc = res["hip"], res["cpu"]
    assert bits_equal(fh["up"], fc["up"])   # the forward pass is be=cpu's bits
    assert abs(fh["loss"].item() - fc["loss"].item()) <= CAP * abs(fc["loss"].item())
    for n in fc:
        if n.endswith("_grad_loss"):
            assert np.max(np.abs(fh[n] - fc[n])) <= CAP * np.max(np.abs(fc[n])), n
    for parallel in (False, True):
        G, bp, params, fwd, ins = dec_step(hip, gets=None, seed_in_var=True)
        try:
            gets = [n for n in fh if n.endswith("_grad_loss")] + ["loss"]
            assert G.capture_graph(parallel=parallel) == len(G.calls())
            got = dict(ins)
            G.run_bck(["data", "label"], got, gets, graph=True)
            for n in gets:
                assert bits_equal(got[n], fh[n]), (parallel, n)
        finally:
            G.release()
    f = ConvPipeFwd(hip); f.init(dec_tiny(2), op_params=params)
    try:
        assert [c.func for c in f.fwd_calls if c.tag.startswith("up")] == ["hip_bconv_in", "hip_chan_affine"]
        io = {"data": ins["data"]}
        f.run_fwd(["data"], io, ["up"])
    finally:
        f.release()
    assert bits_equal(io["up"], fc["up"])
