"""Grouped convolutions in the pipes on the MI355X: dw_sep_tiny's gradient step call by call against be=cpu on the GPU's own inputs, by the rule each function has
(tests/test_gpu_bck_pipe.py: check_call; the grouped forward and data gradient bit for bit, the grouped filter gradient against oracle/bck_chain.py's chain with the
launched BK / KSL on the slices), the captured step replayed against the eager step, a solver step against be=cpu, and the published AlexNet's forward pass."""
import numpy as np
import pytest

from boda_amd import conv_pipe
from boda_amd.bck_pipe import ConvPipeBck, Solver, add_bck_ops, host_params
from boda_amd.cnn_op import OpTune, add_codegen_annotations, pipe_func_args
from boda_amd.conv_pipe import ConvPipeFwd
from boda_amd.rtc import make_rtc
from oracle import bck_chain as bc

from conv_grp_ref import bits_equal, run_func, slice_ins
from test_conv_grp_pipe_cpu import inputs
from test_gpu_bck_pipe import check_call

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
    cp = conv_pipe.dw_sep_tiny(3); bp = add_bck_ops(cp)
    params = host_params(bp, 1)
    drv = ConvPipeBck(rtc, **kw); drv.init(bp, params)
    return drv, bp, params


def grad_nodes(drv, bp):
    return [n for n in bp.nodes if n.endswith("_grad_loss") and n in drv.vars]


def check_grouped_call(hip, cpu, tag, fop, rfc):
    """One grouped call of the step on the GPU, and be=cpu's same function on the GPU's own inputs."""
    fn, am = fop.get_func_name(), rfc.arg_map
    ins = {an: hip.copy_var_to_nda(am[an].n) for an, io in pipe_func_args(fop) if io == "IN"}
    out_an = [an for an, io in pipe_func_args(fop) if io == "OUT"][0]
    hip.copy_nda_to_var(am[out_an].n, np.full(fop.get_dims(out_an).sizes, np.nan, np.float32))   # every element must be written
    hip.run(rfc); hip.finish_and_sync()
    launch = hip.last_launch()
    got = hip.copy_var_to_nda(am[out_an].n)
    if fn != "hip_bconv_filts_grp":
        assert bits_equal(got, run_func(cpu, fop, ins)[0]), (tag, fn)
    else:
        cfg = launch["cfg"]
        bk, ksl = int(cfg.split("_")[0].split("x")[2]), (int(cfg.split("_s")[1].split("_")[0]) if "_s" in cfg else 1)
        g = fop.bck_conv_geom()
        case = (g["B"], g["G"], g["C"], g["OC"], g["H"], g["W"], g["KH"], g["SY"], g["PY"])
        geom = dict(g, C=g["CG"], OC=g["OCG"])
        parts = []
        for j in range(g["G"]):
            s = slice_ins(case, {"in": ins["in"], "out_grad_loss": ins["out_grad_loss"]}, j)
            parts.append(bc.filts_chain(s["in"], s["out_grad_loss"], geom, bk, ksl))
        assert bits_equal(got, np.concatenate(parts, axis=0)), (tag, fn, cfg)
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
            grouped = c.fop.get_func_name().endswith("_grp")
            seen.append(check_grouped_call(hip, cpu, c.tag, c.fop, c.rfc) if grouped else check_call(hip, cpu, c.tag, c.fop, c.rfc))
        hip.release_per_call_id_data()
        assert seen.count("hip_conv_grp") == 2 and seen.count("hip_bconv_in_grp") == 2 and seen.count("hip_bconv_filts_grp") == 2 and len(seen) == len(drv.calls())
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
        E.set_det_drop_seed(7); E.run_bck(["data", "label"], want, gets)
    finally:
        E.release()
    G, bp, _ = make(hip, seed_in_var=True)
    try:
        assert G.capture_graph() == len(G.calls())
        got = {"data": data, "label": label}
        G.set_det_drop_seed(7); G.run_bck(["data", "label"], got, gets, graph=True)
        for n in gets:
            assert bits_equal(got[n], want[n]), n
        G.run_graph()
        for n in gets:
            assert bits_equal(hip.copy_var_to_nda(n), want[n]), ("replayed twice", n)
    finally:
        G.release()


def test_solver_step_matches_cpu(hip, cpu):
    """Forward passes and data gradients are be=cpu's bits, so both backends feed every filter / bias gradient the same operands and the loss of the step is held to
    bits.  A filter gradient's K slices and a bias gradient's tree are not be=cpu's single chains: each side lies within FILTS_MRD (of the gradient's largest element)
    of float64, the two sides therefore within twice that, and the first SGD step moves a param by lr times its gradient (the history starts at zero; weight decay
    adds the same term on both sides) -- so the params after the step differ by at most 2 * lr * FILTS_MRD * max|g|, plus the update's own rounding, one ulp of the
    param (2^-23 of its largest element)."""
    from test_bck_conv_cpu import FILTS_MRD
    res = {}
    sv = dict(type="sgd", lr=0.05, momentum=0.9, weight_decay=5e-4)
    for name, rtc in (("hip", hip), ("cpu", cpu)):
        drv, bp, params = make(rtc, solver=Solver(**sv))
        try:
            data, label = inputs(bp.cp, 2)
            fwd = {"data": data, "label": label}
            gets = grad_nodes(drv, bp) + bp.loss_nodes
            drv.run_bck(["data", "label"], fwd, gets)
            res[name] = (fwd, {p: rtc.copy_var_to_nda(p) for p in drv.sgd_params})
        finally:
            drv.release()
    (fh, ph), (fc, pc) = res["hip"], res["cpu"]
    assert bits_equal(fh["loss"], fc["loss"])
    for p in ph:
        g = fc[p + "_grad_loss"]
        assert np.max(np.abs(ph[p] - pc[p])) <= 2 * sv["lr"] * FILTS_MRD * np.max(np.abs(g)) + 2.0 ** -23 * np.max(np.abs(pc[p])), p
        assert not np.array_equal(pc[p], params[p])


def test_alexnet_forward_convolutions(hip, cpu):
    cp = conv_pipe.alexnet(2)
    rng = np.random.default_rng(4)
    params = {n: ((rng.standard_normal(d.sizes) * np.sqrt(2.0 / (d.dsz("in_chan") * d.dsz("y") * d.dsz("x")))) if n.endswith("_filts") else rng.uniform(-0.1, 0.1, d.sizes)).astype(np.float32)
              for n, d in cp.params.items()}
    data = rng.uniform(-1, 1, cp.nodes["data"].sizes).astype(np.float32)
    convs = [o for o in cp.ops if o.tag in ("conv1", "conv2", "conv3", "conv4", "conv5")]
    fwd = ConvPipeFwd(hip); fwd.init(cp, op_params=params)
    try:
        assert [c.func for c in fwd.fwd_calls if c.tag in ("conv2", "conv4", "conv5")] == ["hip_conv_grp"] * 3
        io = {"data": data}
        fwd.run_fwd(["data"], io, sorted({o.bot for o in convs} | {o.top for o in convs}))
    finally:
        fwd.release()
    for o in convs:   # be=cpu's function on the GPU's own input of the layer (every one of the five has its ReLU fused)
        fop = add_codegen_annotations(cp.conv_op(o), OpTune())
        want, _ = run_func(cpu, fop, {"in": io[o.bot], "filts": params[o.tag + "_filts"], "biases": params[o.tag + "_biases"]})
        assert bits_equal(io[o.top], want), o.tag
