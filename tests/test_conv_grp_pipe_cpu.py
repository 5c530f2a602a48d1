"""Grouped convolutions in the pipes, without a GPU: PipeOp.group through the spec records and the prototxt readers, the two nets in code, ConvPipeFwd's calls on a
recording backend, and a ConvPipeBck step of dw_sep_tiny on be=cpu -- every grouped call of the step held, bit for bit, to the ungrouped function on the slices of
the tensors the step itself produced, and every gradient node to a float64 backprop (torch autograd, groups=g) under the gradient pipes' cap of 5e-4.

The pipe has no forward channel-slice op, so the slice / per-group convolution / Concat twin is formed per call from the step's own vars, not as a second pipe.
NOT covered by bits therefore: the equality of whole gradient nodes of the step with those of a twin PIPE.  What is asserted by bits is every grouped call on the
step's own operands; the ungrouped calls downstream of a grouped one read those very tensors through functions other tests hold to bits, and the step as a whole is
held to float64 only."""
import numpy as np
import pytest
import torch

from boda_amd import conv_pipe, prototxt
from boda_amd.bck_pipe import ConvPipeBck, Freeze, Solver, add_bck_ops, host_params
from boda_amd.cnn_op import OpTune
from boda_amd.conv_pipe import ConvPipeFwd, DryRtc, pipe_from_spec
from boda_amd.eval_pipe import EvalPipe
from boda_amd.op import RtErr, UnsupErr
from boda_amd.rtc import make_rtc

from conv_grp_ref import bits_equal, sliced

CAP = 5e-4   # the reference's bar for its gradient pipes (mrd_toler, src/test_compute.cc:45), as tests/test_bck_pipe_cpu.py
N_CLASS = 10

PROTOTXT = """
name: "grp_tiny"
input: "data"
input_dim: 2 input_dim: 8 input_dim: 9 input_dim: 9
layer { name: "c1" type: "Convolution" bottom: "data" top: "c1" convolution_param { num_output: 16 kernel_size: 3 pad: 1 group: 2 } }
layer { name: "r1" type: "ReLU" bottom: "c1" top: "c1" }
layer { name: "dw" type: "Convolution" bottom: "c1" top: "dw" convolution_param { num_output: 16 kernel_size: 3 pad: 1 stride: 2 group: 16 } }
layer { name: "pw" type: "Convolution" bottom: "dw" top: "pw" convolution_param { num_output: 5 kernel_size: 1 } }
"""


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


def inputs(cp, seed):
    rng = np.random.default_rng([seed, 11])
    data = rng.uniform(-1, 1, cp.nodes["data"].sizes).astype(np.float32)
    return data, rng.integers(0, N_CLASS, (data.shape[0], 1, 1)).astype(np.float32)


# ---- readers and nets
def test_spec_record_and_prototxt():
    spec = prototxt.pipe_spec(PROTOTXT)
    assert spec == ["input data 8 9 9", "conv c1 data c1 16 3 3 1 1 1 1 2", "relu r1 c1 c1", "conv dw c1 dw 16 3 3 2 2 1 1 16", "conv pw dw pw 5 1 1 1 1 0 0"]
    cp = pipe_from_spec("grp_tiny", spec, 2)
    assert [(o.tag, o.group) for o in cp.ops if o.type == "Convolution"] == [("c1", 2), ("dw", 16), ("pw", 1)]
    assert cp.params["c1_filts"].sizes == (16, 4, 3, 3) and cp.params["dw_filts"].sizes == (16, 1, 3, 3) and cp.params["pw_filts"].sizes == (5, 16, 1, 1)
    assert cp.nodes["dw"].sizes == (2, 16, 5, 5)
    assert cp.conv_op(cp.ops[0]).get_u32("group") == 2 and not cp.conv_op(cp.ops[-1]).has("group")
    old = pipe_from_spec("t", ["input data 8 9 9", "conv c1 data c1 16 3 3 1 1 1 1"], 2)   # a record without the twelfth field reads as before
    assert old.ops[0].group == 1 and old.params["c1_filts"].sizes == (16, 8, 3, 3)
    ops = dict(prototxt.conv_ops(PROTOTXT, 2))
    assert ops["c1"].conv_geom()["CG"] == 4 and ops["dw"].conv_geom()["G"] == 16 and not ops["pw"].has("group")
    assert ops["dw"].get_dims("in").sizes == (2, 16, 9, 9) and ops["pw"].get_dims("in").sizes == (2, 16, 5, 5)
    with pytest.raises(RtErr, match="group=3"):
        prototxt.conv_ops(PROTOTXT.replace("group: 2", "group: 3"), 2)
    with pytest.raises(RtErr, match="group=3"):
        pipe_from_spec("t", ["input data 8 9 9", "conv c1 data c1 16 3 3 1 1 1 1 3"], 2)


def test_nets_in_code():
    cp = conv_pipe.alexnet(2)
    assert cp.params["conv2_filts"].sizes == (256, 48, 5, 5) and cp.params["conv4_filts"].sizes == (384, 192, 3, 3) and cp.params["conv5_filts"].sizes == (256, 192, 3, 3)
    assert [o.group for o in cp.ops if o.type == "Convolution"] == [1, 2, 1, 2, 2, 1, 1, 1]
    ng = conv_pipe.alexnet_ng_conv(2)
    assert {n: d.sizes for n, d in cp.nodes.items()} == {n: d.sizes for n, d in ng.nodes.items()}   # the same maps as the rewrite without groups
    dw = conv_pipe.dw_sep_tiny(3)
    assert [(o.tag, o.group, o.stride[0]) for o in dw.ops if o.type == "Convolution"] == [("stem", 1, 1), ("dw1", 8, 1), ("pw1", 1, 1), ("dw2", 12, 2), ("pw2", 1, 1), ("fc", 1, 1)]
    assert dw.params["dw2_filts"].sizes == (12, 1, 3, 3) and dw.nodes[dw.out_node()].sizes == (3, N_CLASS, 1, 1)


def test_forward_pipe_calls_on_a_recording_backend():
    dry = DryRtc(); fwd = ConvPipeFwd(dry, fuse_k1_chains="all"); fwd.init(conv_pipe.alexnet(2))
    funcs = {c.tag: c.func for c in fwd.fwd_calls}
    assert [funcs[t] for t in ("conv1", "conv2", "conv3", "conv4", "conv5")] == ["hip_conv", "hip_conv_grp", "hip_conv", "hip_conv_grp", "hip_conv_grp"]
    dry = DryRtc(); fwd = ConvPipeFwd(dry, fuse_k1_chains="all"); fwd.init(conv_pipe.dw_sep_tiny(3))
    assert [(c.tag, c.func) for c in fwd.fwd_calls if c.func.startswith("hip_conv")] == [("stem", "hip_conv"), ("dw1", "hip_conv_grp"), ("pw1", "hip_conv"),
                                                                                          ("dw2", "hip_conv_grp"), ("pw2", "hip_conv"), ("fc", "hip_conv")]
    for tune in (OpTune(hip_dtype="bf16", hip_layout="nhwc"), OpTune(hip_dtype="bf16")):
        dry = DryRtc()
        with pytest.raises(UnsupErr, match="convolution conv2: group=2"):   # the first grouped layer, by name
            ConvPipeFwd(dry, tune).init(conv_pipe.alexnet(2))
        assert not dry.infos   # before anything is created


# ---- the gradient step
def step(rtc, gets=None, **kw):
    cp = conv_pipe.dw_sep_tiny(3); bp = add_bck_ops(cp)
    params = host_params(bp, 1)
    drv = ConvPipeBck(rtc, **kw); drv.init(bp, params)
    data, label = inputs(cp, 2)
    fwd = {"data": data, "label": label}
    gets = gets if gets is not None else [n for n in bp.nodes if n.endswith("_grad_loss") and n in drv.vars] + bp.loss_nodes
    drv.run_bck(["data", "label"], fwd, gets)
    return drv, bp, params, fwd


def test_step_calls(cpu):
    for kw, bck_of_dw2 in (({}, ["hip_bconv_in_grp", "hip_bconv_biases", "hip_bconv_filts_grp"]), ({"fuse_filts_biases": True}, ["hip_bconv_in_grp", "hip_bconv_biases", "hip_bconv_filts_grp"]),
                           ({"fuse_relu_grad": True}, ["hip_bconv_in_grp", "hip_bconv_biases", "hip_bconv_filts_grp"])):
        drv, bp, _, _ = step(cpu, **kw)
        try:
            calls = [(t, f.get_func_name()) for t, f, _ in drv.calls()]
            assert [fn for t, fn in calls if t == "dw2_bck"] == bck_of_dw2 and [fn for t, fn in calls if t in ("dw1", "dw2")] == ["hip_conv_grp"] * 2
            assert ("pw2_bck", "hip_bconv_filts_biases") in calls if kw.get("fuse_filts_biases") else ("pw2_bck", "hip_bconv_filts") in calls
            # the ReLU gradient in front of a grouped data gradient stays its own call: relu_pw1_bck masks what dw2_bck wrote, relu_stem_bck what dw1_bck wrote
            assert ("relu_pw1_bck", "hip_zero_if_non_pos") in calls and ("relu_stem_bck", "hip_zero_if_non_pos") in calls
            if kw.get("fuse_relu_grad"):
                assert ("relu_dw2_bck", "hip_zero_if_non_pos") not in calls   # (pw2_bck, an ungrouped data gradient, took the mask of dw2's ReLU)
        finally:
            drv.release()


def test_step_grouped_calls_are_the_ungrouped_functions_on_slices(cpu):
    drv, bp, params, fwd = step(cpu)
    try:
        var = lambda n: cpu.copy_var_to_nda(n)
        checked = 0
        for tag, fop, am in drv.calls():
            fn = fop.get_func_name()
            if not fn.endswith("_grp"):
                continue
            g = fop.conv_geom() if fn == "hip_conv_grp" else fop.bck_conv_geom()
            case = (g["B"], g["G"], g["C"], g["OC"], g["H"], g["W"], g["KH"], g["SY"], g["PY"])
            v = {an: var(a.n) for an, a in am.items() if a.is_var()}
            ins = {"in": v.get("in"), "filts": v.get("filts"), "biases": v.get("biases"), "out_grad_loss": v.get("out_grad_loss")}
            layer = tag[:-4] if tag.endswith("_bck") else tag
            bot = next(o for o in bp.cp.ops if o.tag == layer).bot
            if fn == "hip_conv_grp":      # (its ReLU is the call's own: every layer of this net has one)
                assert fop.get_u32("conv_has_relu") == 1 and bits_equal(v["out"], sliced(cpu, case, ins, "fwd"))
            elif fn == "hip_bconv_filts_grp":
                ins["in"] = var(bot); assert bits_equal(v["filts_grad_loss"], sliced(cpu, case, ins, "filts"))
            else:   # the data gradient, as the ReLU gradient behind it left it: X_grad_loss = X > 0 ? value : +0
                ins["filts"] = var(layer + "_filts")
                want = sliced(cpu, case, ins, "in")
                assert bits_equal(v["in_grad_loss"], np.where(var(bot) > 0, want, np.float32(0.0)))
            checked += 1
        assert checked == 6
    finally:
        drv.release()


def torch_step(cp, params, data, label):
    """float64 backprop of dw_sep_tiny by torch autograd: conv2d(groups=g) + ReLU per layer, global average, fc, softmax loss averaged over the images."""
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    P = {n: t(a).requires_grad_(True) for n, a in params.items()}
    x = t(data).requires_grad_(True); nodes = {"data": x}
    for o in cp.ops:
        if o.type == "Convolution":
            y = torch.nn.functional.conv2d(nodes[o.bot], P[o.tag + "_filts"], P[o.tag + "_biases"], stride=o.stride, padding=o.in_pad, groups=o.group)
        elif o.type == "ReLU":
            y = torch.relu(nodes[o.bot])
        else:
            y = nodes[o.bot].mean(dim=(2, 3), keepdim=True)
        y.retain_grad(); nodes[o.top] = y
    loss = torch.nn.functional.cross_entropy(nodes[cp.out_node()].reshape(data.shape[0], -1), torch.from_numpy(label.reshape(-1).astype(np.int64)))
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


def test_solver_freeze_and_eval_run(cpu):
    drv, bp, params, fwd = step(cpu, gets=["loss"], solver=Solver(type="sgd", lr=0.05, momentum=0.9), freeze=Freeze(params=("dw1",)))
    try:
        assert "dw1_filts" not in drv.sgd_params and "dw2_filts" in drv.sgd_params
        calls = [(t, f.get_func_name()) for t, f, _ in drv.calls()]
        assert [fn for t, fn in calls if t == "dw1_bck"] == ["hip_bconv_in_grp"]   # frozen: the data gradient alone
        assert np.array_equal(cpu.copy_var_to_nda("dw1_filts"), params["dw1_filts"]) and not np.array_equal(cpu.copy_var_to_nda("dw2_filts"), params["dw2_filts"])
        first = fwd["loss"].item()
        for _ in range(3):
            drv.run_bck(["data", "label"], fwd, ["loss"])
        assert fwd["loss"].item() < first   # the same batch four times: the loss falls
        data, label = inputs(bp.cp, 2)
        res = EvalPipe(drv, top_k=2).evaluate(2, lambda i: {"data": data, "label": label})
        assert res["images"] == 6 and res["batches"] == 2 and np.isfinite(res["loss"]) and 0.0 <= res["top1"] <= res["topk"] <= 1.0
    finally:
        drv.release()


def test_init_refusals(cpu):
    bp = add_bck_ops(conv_pipe.dw_sep_tiny(3))
    with pytest.raises(UnsupErr, match="'dw1' has group=8"):
        ConvPipeBck(cpu, grad_operands="bf16").plan(bp)
    had = getattr(cpu, "devices", None)
    cpu.devices = [0, 1]   # (what a multi-device backend carries; plan() makes no backend call)
    try:
        with pytest.raises(UnsupErr, match=r"'dw1' has group=8.*devices="):
            ConvPipeBck(cpu).plan(bp)
    finally:
        cpu.devices = had
