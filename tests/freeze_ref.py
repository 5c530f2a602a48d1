"""What the fine-tuning tests share (tests/test_freeze_cpu.py, tests/test_gpu_freeze.py): the numpy twins of the three hip_bnf_* functions (boda_amd/csrc/kernels/bn_f32.hip,
DESIGN.md section 3.22), a runner that feeds each function the backend's own upstream results, the function ops of the fixture file, the float64 walk of the residual pipe
on its RUNNING pair, and the Freeze values the tests use.  The twins are the written formulas on np.float32 arrays, one numpy operation per rounding; the two sums are
bn_ref.bck_sums_np, unchanged.  Every equality is bn_ref.same_bits."""
import numpy as np

import bck_pipe_ref as ref
import bn_ref as R
from boda_amd.bck_pipe import ConvPipeBck, Freeze, Solver, add_bck_ops
from boda_amd.cnn_op import bnf_bck_func_op, bnf_bck_in_func_op, bnf_prep_func_op

F = R.F

# the largest max|got - want| / max|want| over the nodes of the frozen residual step (every BatchNorm on its running pair) and the three seeds of bn_ref.RES_SEEDS, measured
# on be=cpu against net_bnf_f64 (1.527e-06, 3.267e-06, 1.634e-06; tests/test_freeze_cpu.py prints them).  Both backends are held to ten times this besides the cap 5e-4
FROZEN_DEV_CPU = 3.267e-06
CAP = 5e-4


def prep_np(run_mean, run_var, eps=R.EPS):
    ve = np.asarray(run_var, F) + F(eps)
    sd = np.sqrt(ve)
    istd = F(1) / sd
    assert istd.dtype == F
    return np.array(run_mean, F), istd


def dx_np(scale, istd, dy):
    k = np.asarray(scale, F) * np.asarray(istd, F)
    dx = R.bc(k) * dy
    assert dx.dtype == F
    return dx


def special_dy(shape, seed=0):
    """make_inputs' dy (at least three channels) with a -0 and a NaN in channel 0 and a +Inf in the last channel.  Placed so that every special value of the results is
    PROPAGATED from the inputs, never made: no Inf meets the exact zero of scale[1] (0 * Inf) and no channel's sum holds Infs of both signs (Inf - Inf).  A made NaN has
    whatever sign and payload the hardware picks, and only a propagated one can be held to bits."""
    B, C, H, W = shape
    assert C >= 3
    dy = R.make_inputs(shape, seed)["dy"].copy()
    dy[0, 0, 0, min(1, W - 1)] = F(-0.0)
    dy[B - 1, 0, H - 1, max(W - 2, 0)] = F(np.nan)
    dy[0, C - 1, H // 2, W // 2] = F(np.inf)
    return dy


def run_all_three(rtc, shape, forced=0, seed=0, repeat=2, dy=None):
    """The three functions on one backend, each fed the BACKEND's own upstream results; hip_bnf_bck and hip_bnf_bck_in also in place -> dict of everything."""
    d = R.dims_of(shape)
    i = R.make_inputs(shape, seed)
    if dy is not None:
        i["dy"] = dy
    r = dict(i)
    pr = R.run_func(rtc, bnf_prep_func_op(d, R.EPS), {"run_mean": i["run_mean"], "run_var": i["run_var"]})[0]   # (run_func asserts that the IN args came back unchanged)
    r.update(mean=pr["mean"], inv_std=pr["inv_std"])
    ins = {"in": i["x"], "mean": r["mean"], "inv_std": r["inv_std"], "scale": i["scale"], "out_grad_loss": i["dy"]}
    keep = []
    outs = R.run_func(rtc, bnf_bck_func_op(d, forced), ins, repeat=repeat, keep=keep)     # launched `repeat` times on the same workspace
    for o in outs[1:]:
        for an in o:
            assert R.same_bits(o[an], outs[0][an]), (an, "a repeated launch on the same workspace changed bits")
    r["launch"] = keep[0]
    r.update(sg=outs[0]["scale_grad_loss"], bg=outs[0]["bias_grad_loss"], dx=outs[0]["in_grad_loss"])
    o = R.run_func(rtc, bnf_bck_func_op(d, forced), ins, bind={"in_grad_loss": "out_grad_loss"})[0]
    r.update(sg_ip=o["scale_grad_loss"], bg_ip=o["bias_grad_loss"], dx_ip=o["in_grad_loss"])
    ins2 = {"inv_std": r["inv_std"], "scale": i["scale"], "out_grad_loss": i["dy"]}
    r["dx_in"] = R.run_func(rtc, bnf_bck_in_func_op(d), ins2)[0]["in_grad_loss"]
    r["dx_in_ip"] = R.run_func(rtc, bnf_bck_in_func_op(d), ins2, bind={"in_grad_loss": "out_grad_loss"})[0]["in_grad_loss"]
    return r


RESULT_KEYS = ("mean", "inv_std", "sg", "bg", "dx", "sg_ip", "bg_ip", "dx_ip", "dx_in", "dx_in_ip")


def check_against_numpy(r, shape, forced=0):
    mean, istd = prep_np(r["run_mean"], r["run_var"])
    assert R.same_bits(r["mean"], mean) and R.same_bits(r["inv_std"], istd), "prep"
    sg, bg = R.bck_sums_np(r["x"], mean, istd, r["dy"], forced)     # the twin of hip_bn_bck_sums, on hip_bnf_prep's outputs
    dx = dx_np(r["scale"], istd, r["dy"])
    for k in ("sg", "sg_ip"):
        assert R.same_bits(r[k], sg), k
    for k in ("bg", "bg_ip"):
        assert R.same_bits(r[k], bg), k
    for k in ("dx", "dx_ip", "dx_in", "dx_in_ip"):
        assert R.same_bits(r[k], dx), k


def fixture_ops(rtc):
    """Every function op of tests/golden/ops/freeze-ops.txt: the three functions on every case of bn_ref.CASES, and every function op of the frozen residual steps the GPU
    tests run that bn-ops.txt does not hold already."""
    ops = []
    for shape, slab in R.CASES:
        d = R.dims_of(shape)
        ops += [bnf_prep_func_op(d, R.EPS), bnf_bck_func_op(d, slab), bnf_bck_in_func_op(d)]
    cp = R.residual()
    for fz, kw in ((frozen_bn(), dict(solver=Solver(type="sgd", lr=0.05), seed_in_var=True)), (Freeze(params=("scale", "bias"), bn_global_stats=True), {}),
                   (Freeze(params=all_but(cp, "fc"), bn_global_stats=True), dict(solver=Solver(type="adam", lr=0.01)))):
        drv = ConvPipeBck(rtc, freeze=fz, **kw)
        drv.init(add_bck_ops(cp), R.res_params(cp, 1))
        ops += [f for _, f, _ in drv.calls() if f.get_func_name().startswith(("hip_bnf_", "hip_solver_", "hip_split"))]
        drv.release()
    seen, out = set(), []
    for o in ops:
        if o.to_str() not in seen:
            seen.add(o.to_str()); out.append(o)
    return out


# ---- the Freeze values
def trainable_params(cp):
    return [p for p in cp.params if not p.endswith(("_mean", "_var"))]


def all_but(cp, *tags):
    """Every param of the pipe but those of the ops `tags`."""
    return tuple(p for p in trainable_params(cp) if not any(p in (t + "_filts", t + "_biases", t + "_scale", t + "_bias") for t in tags))


def frozen_bn():
    return Freeze(bn_global_stats=True)


# ---- the float64 walk of the residual pipe on its running pair
def relu_nodes(cp):
    return [o.top for o in cp.ops if o.type == "ReLU"]


def net_bnf_f64(cp, params, data, label, masks, guard_rel=1e-4):
    """bn_ref.net_bn_f64 with every BatchNorm on its RUNNING pair: y = (x - run_mean) / sqrt(run_var + eps), the statistics constants of the step, so that the BatchNorm's
    data gradient is og / sqrt(run_var + eps).  -> {<node>_grad_loss, <param>_grad_loss, loss}.
    The ReLU masks: bn_ref.RES_SEEDS were picked so that the TRAINING walk has no ReLU input within guard_rel max|v| of zero; on the running pair the same seeds do have
    such inputs (down to 1e-6 max|v|), where fp32 and float64 may disagree about the sign and a cap on max|got - want| / max|want| means nothing.  So the walk takes the
    BACKEND's masks (masks[node] = the fp32 node, which holds the rectified values, > 0) and differentiates the same linear piece the backend was on -- and refuses a mask
    that differs from its own where its own input is NOT within guard_rel max|v| of zero: a wrong mask is still an error, a rounding of a value at zero is not."""
    f64 = lambda a: np.asarray(a, np.float64)
    ax = (0, 2, 3)
    pc = lambda a: f64(a).reshape(1, -1, 1, 1)
    val = {cp.in_node: f64(data)}
    keep, res = {}, {}
    for o in cp.ops:
        x = val[o.bot]
        if o.type == "Convolution":
            keep[o.tag] = x
            val[o.top] = ref.conv_f64(x, f64(params[o.tag + "_filts"]), f64(params[o.tag + "_biases"]), o.stride, o.in_pad)
        elif o.type == "ReLU":
            m = np.asarray(masks[o.top], bool)
            if np.any((m != (x > 0)) & (np.abs(x) >= guard_rel * np.max(np.abs(x)))):
                raise AssertionError(f"net_bnf_f64: the backend's mask of ReLU {o.tag} differs from the float64 one at an input that is not within {guard_rel} max|v| of zero")
            keep[o.tag] = m
            val[o.top] = np.where(m, x, 0.0)
        elif o.type == "Pooling":
            assert o.avg_pool
            d = cp.nodes[o.top]
            out, arg = ref.pool_f64(x, (d.dsz("y"), d.dsz("x")), o.kern_sz, o.stride, o.in_pad, 1, 0.0)
            keep[o.tag] = (x.shape, arg); val[o.top] = out
        elif o.type == "BatchNorm":
            istd = 1.0 / np.sqrt(pc(params[o.tag + "_var"]) + float(F(o.eps)))
            xh = (x - pc(params[o.tag + "_mean"])) * istd
            keep[o.tag] = istd; val[o.top] = xh
        elif o.type == "Scale":
            keep[o.tag] = x
            val[o.top] = x * pc(params[o.tag + "_scale"]) + pc(params[o.tag + "_bias"])
        elif o.type == "Eltwise":
            val[o.top] = sum(val[b] for b in o.bots)
        else:
            raise AssertionError(o.type)
    B = data.shape[0]
    lab = np.asarray(label).reshape(B).astype(int)
    t = cp.out_node()
    z = val[t].reshape(B, -1)
    e = np.exp(z - z.max(axis=1, keepdims=True)); p = e / e.sum(axis=1, keepdims=True)
    res["loss"] = float(-np.log(p[np.arange(B), lab]).mean())
    p[np.arange(B), lab] -= 1.0
    grad = {t: (p / B).reshape(val[t].shape)}
    for o in reversed(cp.ops):
        og = grad[o.top]
        if o.type == "Convolution":
            gx, gf, gb = ref.conv_bck_f64(keep[o.tag], f64(params[o.tag + "_filts"]), og, o.stride, o.in_pad)
            res[o.tag + "_filts_grad_loss"] = gf; res[o.tag + "_biases_grad_loss"] = gb
            grad[o.bot] = grad.get(o.bot, 0.0) + gx
        elif o.type == "ReLU":
            grad[o.top] = np.where(keep[o.tag], og, 0.0)
        elif o.type == "Pooling":
            shp, arg = keep[o.tag]
            grad[o.bot] = grad.get(o.bot, 0.0) + ref.pool_bck_f64(shp, og, arg, o.kern_sz, o.stride, o.in_pad, 1)
        elif o.type == "Scale":
            res[o.tag + "_scale_grad_loss"] = (og * keep[o.tag]).sum(axis=ax); res[o.tag + "_bias_grad_loss"] = og.sum(axis=ax)
            grad[o.top] = og * pc(params[o.tag + "_scale"])
        elif o.type == "BatchNorm":
            grad[o.top] = keep[o.tag] * og
        elif o.type == "Eltwise":
            for b in o.bots:
                grad[b] = grad.get(b, 0.0) + og
    for n, g in grad.items():
        res[n + "_grad_loss"] = g
    return res


def frozen_dev(fwd, want, nodes):
    """The largest max|got - want| / max|want| over `nodes` (a loss: relative).  The biases of a convolution in front of a BatchNorm on its running pair DO get a
    gradient (the statistics are constants), so no node is special here."""
    worst = 0.0
    for n in nodes:
        got = fwd[n]
        assert np.all(np.isfinite(got)), n
        err = abs(got.item() - want[n]) / abs(want[n]) if n == "loss" else ref.rel_err(got, want[n])
        worst = max(worst, err)
    return worst


def res_grad_nodes(drv, bp):
    """The gradient nodes the driver computes that the float64 walk knows (no partial of a fan-out), and the loss."""
    return [n for n in bp.nodes if n.endswith("_grad_loss") and "_split_" not in n and n in drv.vars] + ["loss"]
