"""Deconvolution and Crop layers in the pipes, without a GPU: ConvPipe.add's dims, the spec records, conv_pipe.fcn_tiny and bilinear_filts, ConvPipeFwd's calls on a
recording backend, and a ConvPipeBck step of fcn_tiny on be=cpu -- every Deconvolution / Crop call of the step held, bit for bit, to the existing function on
exchanged roles (resp. to numpy) on the tensors the step itself produced, and every gradient node to a float64 backprop of the whole net (torch autograd,
conv_transpose2d) under the gradient pipes' cap of 5e-4."""
import numpy as np
import pytest
import torch

from boda_amd import conv_pipe
from boda_amd.bck_graph import LossSpec
from boda_amd.bck_pipe import ConvPipeBck, Freeze, Solver, add_bck_ops, host_params
from boda_amd.cnn_op import OpTune
from boda_amd.conv_pipe import ConvPipe, ConvPipeFwd, DryRtc, PipeOp, bilinear_filts, pipe_from_spec
from boda_amd.op import Dims, RtErr, UnsupErr
from boda_amd.rtc import make_rtc

from deconv_ref import bits_equal, exchanged

CAP = 5e-4   # the reference's bar for its gradient pipes (mrd_toler, src/test_compute.cc:45), as tests/test_bck_pipe_cpu.py
N_CLASS = 5


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


def inputs(cp, seed):
    rng = np.random.default_rng([seed, 13])
    data = rng.uniform(-1, 1, cp.nodes["data"].sizes).astype(np.float32)
    label = rng.integers(0, N_CLASS, (data.shape[0],) + data.shape[2:]).astype(np.float32)
    label[0, 0, :3] = 255   # a few ignored pels
    return data, label


def fcn_params(bp, seed=4):
    params = host_params(bp, seed)
    for tag in ("up2", "up1"):   # the upsampling layers start as Caffe starts them: bilinear on the diagonal
        params[tag + "_filts"] = bilinear_filts(N_CLASS, N_CLASS, 4)
    return params


def step(rtc, gets=None, batch=2, **kw):
    cp = conv_pipe.fcn_tiny(batch)
    bp = add_bck_ops(cp, loss_specs=LossSpec(ignore_label=255))
    params = fcn_params(bp)
    drv = ConvPipeBck(rtc, **kw); drv.init(bp, params)
    data, label = inputs(cp, 2)
    fwd = {"data": data, "label": label}
    gets = gets if gets is not None else [n for n in bp.nodes if n.endswith("_grad_loss") and n in drv.vars] + bp.loss_nodes
    drv.run_bck(["data", "label"], fwd, gets)
    return drv, bp, params, fwd


def test_dims_spec_records_and_the_net():
    cp = conv_pipe.fcn_tiny(2)
    assert cp.nodes["score2"].sizes == (2, 5, 4, 4) and cp.nodes["up2"].sizes == (2, 5, 10, 10) and cp.nodes["up2c"].sizes == (2, 5, 8, 8)
    assert cp.nodes["up1"].sizes == (2, 5, 18, 18) and cp.nodes["score"].sizes == (2, 5, 16, 16) and cp.out_node() == "score"
    assert cp.params["up2_filts"].names == ("in_chan", "out_chan", "y", "x") and cp.params["up2_filts"].sizes == (5, 5, 4, 4)
    up2 = next(o for o in cp.ops if o.tag == "up2")
    op = cp.conv_op(up2)
    assert op.get_type() == "Deconvolution" and op.flops() == 2 * 2 * 5 * 4 * 4 * 5 * 4 * 4 and op.deconv_geom()["OH"] == 10
    # FCN's heads: the sizes that invert a convolution's (the reference's conv_out_sz_to_in_sz on shapes that divide)
    for hw, k, s, pad, want in ((16, 4, 2, 0, 34), (34, 16, 8, 0, 280), (16, 64, 32, 0, 544), (28, 4, 2, 1, 56)):
        p = ConvPipe("t", "data", Dims.make("float", img=1, chan=21, y=hw, x=hw))
        p.add(PipeOp("up", "Deconvolution", "data", "up", out_chans=21, kern_sz=(k, k), stride=(s, s), in_pad=(pad, pad)))
        assert p.nodes["up"].sizes == (1, 21, want, want) and (want + 2 * pad - k) // s + 1 == hw
    spec = ["input data 3 16 16", "conv c data c 5 3 3 2 2 1 1", "deconv up c up 5 4 4 2 2 1 1", "crop cr up data sc 0 0", "relu r sc sc"]
    sp = pipe_from_spec("t", spec, 2)
    assert [(o.tag, o.type) for o in sp.ops] == [("c", "Convolution"), ("up", "Deconvolution"), ("cr", "Crop"), ("r", "ReLU")]
    assert sp.nodes["up"].sizes == (2, 5, 16, 16) and sp.ops[2].bots == ("up", "data") and sp.ops[2].offset == (0, 0) and sp.nodes["sc"].sizes == (2, 5, 16, 16)


def test_add_refusals():
    p = ConvPipe("t", "data", Dims.make("float", img=1, chan=4, y=6, x=6))
    with pytest.raises(UnsupErr, match="deconvolution up: group=2: a Deconvolution with group > 1 is out of scope"):
        p.add(PipeOp("up", "Deconvolution", "data", "up", out_chans=4, kern_sz=(4, 4), stride=(2, 2), group=2))
    p.add(PipeOp("up", "Deconvolution", "data", "up", out_chans=4, kern_sz=(4, 4), stride=(2, 2)))   # 14 x 14
    with pytest.raises(RtErr, match=r"crop c: offset \(9, 0\) \+ data's plane \(6, 6\) exceeds up's plane \(14, 14\)"):
        p.add(PipeOp("c", "Crop", "up", "c", bots=("up", "data"), offset=(9, 0)))
    with pytest.raises(RtErr, match="bots must be"):
        p.add(PipeOp("c", "Crop", "up", "c", bots=("up",)))


def test_bilinear_filts():
    for k in (4, 3, 16, 64):
        w = bilinear_filts(3, 5, k)
        f = -(-k // 2); c0 = (2 * f - 1 - f % 2) / (2.0 * f)
        want = np.array([[(1 - abs(y / f - c0)) * (1 - abs(x / f - c0)) for x in range(k)] for y in range(k)])
        assert w.shape == (3, 5, k, k) and w.dtype == np.float32
        for c in range(3):
            for oc in range(5):
                assert np.allclose(w[c, oc], want if c == oc else 0.0, rtol=0, atol=2e-7)
    assert np.array_equal(bilinear_filts(1, 1, 4)[0, 0, 0], np.array([0.0625, 0.1875, 0.1875, 0.0625], np.float32))   # Caffe's 4/2 kernel: (.25 .75 .75 .25) x .25


def test_forward_pipe_calls_on_a_recording_backend():
    cp = conv_pipe.fcn_tiny(2)
    f = ConvPipeFwd(DryRtc()); f.init(cp)
    fns = {c.tag: c.func for c in f.fwd_calls}
    assert fns["up2"] == fns["up1"] == "hip_deconv" and fns["up2c"] == fns["score"] == "hip_crop" and fns["fuse1"] == "hip_reduce"
    for tune in (OpTune(hip_dtype="bf16"), OpTune(hip_dtype="bf16", hip_layout="nhwc")):
        with pytest.raises(UnsupErr, match="pipe fcn_tiny: Deconvolution up2: a Deconvolution layer has no bf16 or channels-last form"):
            ConvPipeFwd(DryRtc(), op_tune=tune).init(cp)


def test_gradient_graph_names():
    bp = add_bck_ops(conv_pipe.fcn_tiny(2), loss_specs=LossSpec(ignore_label=255))
    bck = {o.tag: o for o in bp.bck_ops()}
    assert bck["up2_bck"].type == "BckDeconv" and bck["up2_bck"].tops == ["score2_grad_loss", "up2_filts_grad_loss", "up2_biases_grad_loss"]
    assert bck["up2_bck"].bots == ["score2", "up2_filts", "up2_biases", "up2_grad_loss"]
    assert bck["score_bck"].type == "BckCrop" and bck["score_bck"].bots == ["score_grad_loss"] and bck["score_bck"].tops == ["up1_grad_loss"]
    assert bp.nodes["up1_grad_loss"].sizes == (2, 5, 18, 18) and bp.nodes["up2_filts_grad_loss"] == bp.cp.params["up2_filts"]
    assert "data_grad_loss" in bp.nodes and not any("data" in t and "split" in t for o in bp.bck_ops() for t in o.tops)   # the Crop's `ref` gets no gradient from it
    assert bp.nodes["label"].sizes == (2, 16, 16)


def test_step_calls_are_the_exchanged_functions(cpu):
    drv, bp, params, fwd = step(cpu)
    try:
        var = lambda n: cpu.copy_var_to_nda(n)
        calls = [(t, f.get_func_name()) for t, f, _ in drv.calls()]
        assert [fn for t, fn in calls if t == "up1_bck"] == ["hip_deconv_bck_in", "hip_deconv_bck_biases", "hip_deconv_bck_filts"]
        assert ("up2", "hip_deconv") in calls and ("score", "hip_crop") in calls and ("score_bck", "hip_crop_bck") in calls
        checked = 0
        for tag, fop, am in drv.calls():
            fn = fop.get_func_name()
            v = {an: var(a.n) for an, a in am.items() if a.is_var()}
            if fn.startswith("hip_deconv"):
                g = fop.deconv_geom()
                case = (g["B"], g["C"], g["H"], g["W"], g["OC"], (g["KH"], g["KW"]), (g["SY"], g["SX"]), (g["PY"], g["PX"]))
                layer = tag[:-4] if tag.endswith("_bck") else tag
                ins = {"in": var(next(o for o in bp.cp.ops if o.tag == layer).bot), "filts": var(layer + "_filts"), "biases": var(layer + "_biases"), "out_grad_loss": v.get("out_grad_loss")}
                which, out = {"hip_deconv": ("fwd", "out"), "hip_deconv_bck_in": ("in", "in_grad_loss"), "hip_deconv_bck_biases": ("biases", "biases_grad_loss"),
                              "hip_deconv_bck_filts": ("filts", "filts_grad_loss")}[fn]
                assert bits_equal(v[out], exchanged(cpu, case, ins, which)), (tag, fn)
                checked += 1
            elif fn == "hip_crop":
                assert bits_equal(v["out"], v["in"][:, :, 1:1 + v["out"].shape[2], 1:1 + v["out"].shape[3]]); checked += 1
            elif fn == "hip_crop_bck":
                want = np.zeros(v["in_grad_loss"].shape, np.float32); g = v["out_grad_loss"]
                want[:, :, 1:1 + g.shape[2], 1:1 + g.shape[3]] = g
                assert bits_equal(v["in_grad_loss"], want); checked += 1
        assert checked == 2 * 4 + 4
    finally:
        drv.release()


def torch_step(cp, params, data, label):
    """float64 backprop of fcn_tiny by torch autograd; the loss is averaged over the pels that are not ignored (LossSpec's default normaliser, VALID)."""
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    P = {n: t(a).requires_grad_(True) for n, a in params.items()}
    x = t(data).requires_grad_(True); nodes = {"data": x}
    F = torch.nn.functional
    for o in cp.ops:
        if o.type == "Convolution":
            y = F.conv2d(nodes[o.bot], P[o.tag + "_filts"], P[o.tag + "_biases"], stride=o.stride, padding=o.in_pad)
        elif o.type == "Deconvolution":
            y = F.conv_transpose2d(nodes[o.bot], P[o.tag + "_filts"], P[o.tag + "_biases"], stride=o.stride, padding=o.in_pad)
        elif o.type == "ReLU":
            y = torch.relu(nodes[o.bot])
        elif o.type == "Pooling":
            y = F.max_pool2d(nodes[o.bot], o.kern_sz, o.stride)
        elif o.type == "Crop":
            r = nodes[o.bots[1]]
            y = nodes[o.bot][:, :, o.offset[0]:o.offset[0] + r.shape[2], o.offset[1]:o.offset[1] + r.shape[3]]
        else:
            y = nodes[o.bots[0]] + nodes[o.bots[1]]
        nodes[o.top] = y
    loss = F.cross_entropy(nodes[cp.out_node()], torch.from_numpy(label.astype(np.int64)), ignore_index=255)
    loss.backward()
    want = {n + "_grad_loss": p.grad.numpy() for n, p in P.items()}
    want["data_grad_loss"] = x.grad.numpy(); want["loss"] = float(loss.detach())
    return want


def test_step_against_float64(cpu):
    drv, bp, params, fwd = step(cpu)
    try:
        want = torch_step(bp.cp, params, *inputs(bp.cp, 2))
        assert abs(fwd["loss"].item() - want["loss"]) / want["loss"] <= CAP
        for n in [p + "_grad_loss" for p in bp.cp.params] + ["data_grad_loss"]:
            err = float(np.max(np.abs(fwd[n].astype(np.float64) - want[n])) / np.max(np.abs(want[n])))
            print(n, err)
            assert fwd[n].shape == want[n].shape and err <= CAP, (n, err)
    finally:
        drv.release()


def test_freeze_of_both_deconvolutions_and_a_solver(cpu):
    drv, bp, params, fwd = step(cpu, gets=["loss"], solver=Solver(type="sgd", lr=0.05, momentum=0.9), freeze=Freeze(params=("up2", "up1")))
    try:
        assert not any(n.startswith(("up1_", "up2_")) for n in drv.sgd_params) and "score2_filts" in drv.sgd_params
        for n in ("up1_filts_grad_loss", "up2_filts_grad_loss", "up1_biases_grad_loss", "up2_biases_grad_loss"):
            assert n not in drv.vars   # no filter gradient var exists
        calls = [(t, f.get_func_name()) for t, f, _ in drv.calls()]
        assert [fn for t, fn in calls if t == "up1_bck"] == ["hip_deconv_bck_in"] and [fn for t, fn in calls if t == "up2_bck"] == ["hip_deconv_bck_in"]
        assert np.array_equal(cpu.copy_var_to_nda("up1_filts"), params["up1_filts"]) and not np.array_equal(cpu.copy_var_to_nda("score2_filts"), params["score2_filts"])
        first = fwd["loss"].item()
        for _ in range(3):
            drv.run_bck(["data", "label"], fwd, ["loss"])
        assert fwd["loss"].item() < first   # the same batch four times: the loss falls
    finally:
        drv.release()


def test_options_pass_the_layers_by_or_refuse_them(cpu):
    bp = add_bck_ops(conv_pipe.fcn_tiny(2), loss_specs=LossSpec(ignore_label=255))
    for kw in ({"fuse_relu_grad": True}, {"fuse_filts_biases": True}, {"grad_operands": "bf16"}):
        plan = ConvPipeBck(cpu, **kw).plan(bp)
        fns = [(t, f.get_func_name()) for t, f, _ in plan.calls]
        assert [fn for t, fn in fns if t == "up2_bck"] == ["hip_deconv_bck_in", "hip_deconv_bck_biases", "hip_deconv_bck_filts"], kw
        assert not any(f.str_vals.get("hip_operands") for t, f, _ in plan.calls if t in ("up1_bck", "up2_bck"))
    two = DryRtc(); two.devices = [0, 1]   # (what a multi-device backend carries; plan() makes no backend call)
    with pytest.raises(UnsupErr, match=r"'up2' is a Deconvolution.*devices="):
        ConvPipeBck(two).plan(bp)


def test_iter_size_accumulates_the_deconvolution_gradients(cpu):
    """Two micro-steps on the same batch: the accumulators hold g + g, the params move only behind the second."""
    drv, bp, params, fwd = step(cpu, gets=["up2_filts_grad_loss", "up1_biases_grad_loss"], solver=Solver(type="sgd", lr=0.05, momentum=0.9), iter_size=2)
    try:
        assert np.array_equal(cpu.copy_var_to_nda("up1_biases"), params["up1_biases"]) and np.array_equal(cpu.copy_var_to_nda("score2_filts"), params["score2_filts"])
        g = {n: fwd[n].copy() for n in ("up2_filts_grad_loss", "up1_biases_grad_loss")}
        assert bits_equal(cpu.copy_var_to_nda("up2_filts_grad_acc"), g["up2_filts_grad_loss"])   # the first micro-step overwrites
        drv.run_bck(["data", "label"], fwd, list(g))
        for n in g:
            assert bits_equal(fwd[n], g[n]) and bits_equal(cpu.copy_var_to_nda(n[:-len("_grad_loss")] + "_grad_acc"), g[n] + g[n]), n
        assert not np.array_equal(cpu.copy_var_to_nda("up1_biases"), params["up1_biases"]) and not np.array_equal(cpu.copy_var_to_nda("up2_filts"), params["up2_filts"])
    finally:
        drv.release()


# ---- a wide layer: the matrix path in the pipes
def dec_tiny(batch):
    """A decoder layer in miniature: conv 3x3 to 32 channels, a Deconvolution 32 -> 32 at 4/2 (the planner's matrix path) with a ReLU behind it, a 1x1 score."""
    p = ConvPipe("dec_tiny", "data", Dims.make("float", img=batch, chan=3, y=6, x=6))
    p.add(PipeOp("c1", "Convolution", "data", "c1", out_chans=32, kern_sz=(3, 3), in_pad=(1, 1))); p.add(PipeOp("r1", "ReLU", "c1", "c1"))
    p.add(PipeOp("up", "Deconvolution", "c1", "up", out_chans=32, kern_sz=(4, 4), stride=(2, 2), in_pad=(1, 1))); p.add(PipeOp("r2", "ReLU", "up", "up"))
    p.add(PipeOp("score", "Convolution", "up", "score", out_chans=N_CLASS, kern_sz=(1, 1)))
    return p


def dec_step(rtc, gets=None, **kw):
    cp = dec_tiny(2)
    bp = add_bck_ops(cp, loss_specs=LossSpec(ignore_label=255))
    params = host_params(bp, 4)
    drv = ConvPipeBck(rtc, **kw); drv.init(bp, params)
    rng = np.random.default_rng(5)
    fwd = {"data": rng.uniform(-1, 1, cp.nodes["data"].sizes).astype(np.float32), "label": rng.integers(0, N_CLASS, (2, 12, 12)).astype(np.float32)}
    ins = dict(fwd)
    gets = gets if gets is not None else [n for n in bp.nodes if n.endswith("_grad_loss") and n in drv.vars] + bp.loss_nodes
    drv.run_bck(["data", "label"], fwd, gets)
    return drv, bp, params, fwd, ins


def test_wide_layer_takes_the_matrix_path(cpu):
    drv, bp, params, fwd, ins = dec_step(cpu)
    try:
        calls = [(t, f.get_func_name()) for t, f, _ in drv.calls()]
        assert [fn for t, fn in calls if t == "up"] == ["hip_bconv_in", "hip_chan_affine"]
        assert [fn for t, fn in calls if t == "up_bck"] == ["hip_conv", "hip_deconv_bck_biases", "hip_bconv_filts"]
        assert ("r2", "hip_zero_if_non_pos") in calls   # the ReLU behind it: as behind any op that is no Convolution
        for v in ("up_filts_x", "up_biases_x", "up_filts_grad_loss_x", "up_ones", "up_zeros"):
            assert v in drv.vars
        assert np.all(cpu.copy_var_to_nda("up_ones") == 1) and np.all(cpu.copy_var_to_nda("up_zeros").view(np.uint32) == 0)
        assert bits_equal(cpu.copy_var_to_nda("up_filts_x").reshape(-1), params["up_filts"].reshape(-1))   # the view is the blob
        i = [t for t, _ in calls].index("up_bck")
        deps = drv._call_deps()   # a call on a view is ordered as a call on the var: whoever reads up_filts_grad_loss follows hip_bconv_filts
        want = torch_step(bp.cp, params, ins["data"], ins["label"])
        for n in [p + "_grad_loss" for p in bp.cp.params] + ["data_grad_loss"]:
            err = float(np.max(np.abs(fwd[n].astype(np.float64) - want[n])) / np.max(np.abs(want[n])))
            assert fwd[n].shape == want[n].shape and err <= CAP, (n, err)
    finally:
        drv.release()
    # the same step with the direct forms forced (a seven-field tile travels through the pipe's tune): be=cpu runs the same loops, so every node has the same bits
    drv2, bp2, _, fwd2, _ = dec_step(cpu, op_tune=OpTune(hip_tile="1x1x32x2x2x1x1"))
    try:
        assert [f.get_func_name() for t, f, _ in drv2.calls() if t == "up_bck"] == ["hip_deconv_bck_in", "hip_deconv_bck_biases", "hip_deconv_bck_filts"]
        for n in fwd:
            assert bits_equal(fwd[n], fwd2[n]), n
    finally:
        drv2.release()


def test_solver_reads_the_gradient_behind_the_view(cpu):
    drv, bp, params, fwd, ins = dec_step(cpu, gets=["loss"], solver=Solver(type="sgd", lr=0.05, momentum=0.9))
    try:
        calls = drv.calls(); deps = drv._call_deps()
        ff = next(i for i, (t, f, _) in enumerate(calls) if t == "up_bck" and f.get_func_name() == "hip_bconv_filts")
        upd = [i for i, (t, f, am) in enumerate(calls) if any(a.is_var() and a.n == "up_filts_grad_loss" for a in am.values()) and i != ff]
        assert upd and all(ff in deps[i] for i in upd)
        assert not np.array_equal(cpu.copy_var_to_nda("up_filts"), params["up_filts"])
    finally:
        drv.release()
