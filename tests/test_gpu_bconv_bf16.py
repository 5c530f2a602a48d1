"""hip_operands=bf16 on the MI355X: kernels/bconv_in_bf16.hip and kernels/bconv_fb_bf16.hip held to the bound of tests/bconv_bf16_ref.py (and the bias gradient to
its written chain, bit for bit), every output NaN-poisoned with a guard var behind every var; then ConvPipeBck(grad_operands="bf16") call by call, against float64,
as a graph replay, and on two shards."""
import numpy as np
import pytest

import bck_pipe_ref as ref
import bconv_bf16_ref as R
import bconv_fb_ref as fb
import bn_ref as BN
import sgd_ref as S
from boda_amd.bck_pipe import ConvPipeBck, SgdSolver, add_bck_ops
from boda_amd.cnn_op import BN_FUNCS, OpTune, add_bck_op_annotations, has_bf16_operands, pipe_func_args
from boda_amd.op import Nda, Op, UnsupErr
from boda_amd.rtc import make_rtc

from test_bck_pipe_cpu import CAP, PIPES, SEED_A, SEED_B, grad_nodes, small_inputs, small_params, want_f64
from test_bck_pipe_cpu import run_func as cpu_run_func

pytestmark = pytest.mark.gpu

F = np.float32
IN_KERNEL, FB_KERNEL = "bodahip_bconv_in_bf16", "bodahip_bconv_filts_biases_bf16"
FB_FORCED = R.FB_FORCED


@pytest.fixture(scope="module")
def hip():
    r = make_rtc("(be=hip)", 0)
    r.init()
    yield r
    r.close()


@pytest.fixture(scope="module")
def hip2():
    """The eager driver's backend: a second instance, with a stream, vars and kernels of its own."""
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


def tile_ran(tile, launch):
    v = [int(x) for x in tile.split("x")]
    return launch["cfg"].startswith(f"{v[0]}x{v[1]}x{v[2]}_w{v[3]}x{v[4]}")


def zero_if_non_pos(rtc, g, cond):
    op = Op({"type": "ZeroIfNonPos"}, {an: Nda(dims=R.Dims.make("float", **dict(zip(("img", "chan", "y", "x"), g.shape))), tn="float") for an in ("in", "cond", "out")})
    return R.run_fop(rtc, add_bck_op_annotations(op, OpTune())[0], {"in": g, "cond": cond})["out"]


# ---- the data gradient
def check_in(hip, op, ins, r, tile, what):
    a = R.run_fop(hip, R.in_func(op, tile), ins, launch=True)
    assert a["launch"]["kernel"] == IN_KERNEL and (not tile or tile_ran(tile, a["launch"])), a["launch"]
    frac = R.check_bound(op, "in", a["in_grad_loss"], r, what=f"be=hip {what} {a['launch']['cfg']}")
    unreached = r["A"][0] == 0
    assert np.all(R.bits(a["in_grad_loss"])[unreached] == 0), (what, "a position no term reaches is not +0")
    b = R.run_fop(hip, R.in_func(op, tile), ins)
    assert R.same_bits(a["in_grad_loss"], b["in_grad_loss"]), (what, "two runs differ")
    z = R.run_fop(hip, R.in_func(op, tile, zinp=True), ins, launch=True)
    assert z["launch"]["kernel"] == IN_KERNEL, z["launch"]
    want = zero_if_non_pos(hip, a["in_grad_loss"], ins["in"])
    assert R.same_bits(z["in_grad_loss"], want), (what, "zero_if_in_non_pos=1 differs from the unflagged call followed by hip_zero_if_non_pos")
    return frac


@pytest.mark.parametrize("name", sorted(R.IN_SHAPES))
def test_data_gradient(hip, name):
    op = R.in_op(name)
    ins = R.rand_ins(op, len(name))
    r = R.refs(op, ins)
    if name == "k1_stride2":
        assert np.any(r["A"][0] == 0)
    for tile in [""] + R.IN_FORCED.get(name, []):
        check_in(hip, op, ins, r, tile, f"{name} {tile or 'planner'}")


# ---- the fused filter and bias gradient
def check_fb(hip, op, ins, r, tile, what, seq=None):
    outs = R.run_fop(hip, R.fb_func(op, tile), [ins] + list(seq or []), launch=True)
    a = outs[0]
    bk, ksl = R.plan_of(a["launch"], FB_KERNEL)
    assert not tile or (tile_ran(tile, a["launch"]) and ksl == int(tile.split("x")[6])), (tile, a["launch"])
    R.check_bound(op, "filts", a["filts_grad_loss"], r, ksl=ksl, what=f"be=hip {what} {a['launch']['cfg']}")
    for o, cur in zip(outs, [ins] + list(seq or [])):
        assert R.same_bits(o["biases_grad_loss"].reshape(-1), fb.biases_chain(cur["out_grad_loss"], bk, ksl)), (what, "biases differ from biases_chain", bk, ksl)
    return outs, ksl


@pytest.mark.parametrize("name", sorted(fb.SHAPES))
def test_filter_and_bias_gradient(hip, name):
    op = fb.shape_op(name)
    ins = R.rand_ins(op, len(name))
    r = R.refs(op, ins)
    (a,), ksl = check_fb(hip, op, ins, r, "", f"{name} planner")
    if name == "k1_long_k":
        assert ksl > 1      # K = 3136 on one tile: the planner slices it
    (b,), _ = check_fb(hip, op, ins, r, "", f"{name} planner again")
    assert R.same_bits(a["filts_grad_loss"], b["filts_grad_loss"]) and R.same_bits(a["biases_grad_loss"], b["biases_grad_loss"]), "two runs differ"
    for tile, only in FB_FORCED.items():
        if only is None or name in only:
            check_fb(hip, op, ins, r, tile, f"{name} {tile}")


def test_fc_shape_and_the_slab_workspace_on_other_data(hip):
    op = R.shape8_op(R.FC_SHAPE)                    # K = img = 4, N = 54
    ins = R.rand_ins(op, 3)
    check_fb(hip, op, ins, R.refs(op, ins), "", "fc planner")
    check_fb(hip, op, ins, R.refs(op, ins), R.FC_TILE, "fc two slices, the second empty")
    op = fb.shape_op("k1_many_tiles")               # ragged tiles both ways; three data sets through the same vars, so the same slabs
    sets = [R.rand_ins(op, s) for s in (21, 22, 23)]
    outs, ksl = check_fb(hip, op, sets[0], R.refs(op, sets[0]), R.REUSE_TILE, "many tiles, five slices", seq=sets[1:])
    for o, cur in zip(outs[1:], sets[1:]):
        R.check_bound(op, "filts", o["filts_grad_loss"], R.refs(op, cur), ksl=ksl, what="be=hip the workspace on other data")


# ---- recorded shapes
@pytest.mark.parametrize("i", range(8))
def test_recorded_shapes(hip, i):
    op = R.recorded_ops()[i]
    ins = R.rand_ins(op, 50 + i)
    r = R.refs(op, ins)
    g = op.bck_conv_geom()
    what = f"recorded k{g['KH']} s{g['SY']} {g['B']}x{g['C']}x{g['H']}->{g['OC']}"
    a = R.run_fop(hip, R.in_func(op), ins, launch=True)
    assert a["launch"]["kernel"] == IN_KERNEL
    R.check_bound(op, "in", a["in_grad_loss"], r, what=f"be=hip {what} {a['launch']['cfg']}")
    check_fb(hip, op, ins, r, "", what)


# ---- the pipe
def conv_calls(drv):
    return [c for c in drv.bck_calls if c.fop.get_func_name() in ("hip_bconv_in", "hip_bconv_filts_biases")]


def check_conv_call(hip, cpu, c):
    """One flagged conv gradient call of the step, run alone on what the step left in its inputs, against be=cpu in the same mode on the same inputs (the bound,
    centred on be=cpu's float64 twin S; the biases bit for bit against their chain)."""
    fop, am = c.fop, c.rfc.arg_map
    assert has_bf16_operands(fop), c.tag
    spec = pipe_func_args(fop)
    ins = {an: hip.copy_var_to_nda(am[an].n) for an, io in spec if io == "IN"}
    hip.run(c.rfc); launch = hip.last_launch(); hip.finish_and_sync()
    got = {an: hip.copy_var_to_nda(am[an].n) for an, io in spec if io == "OUT"}
    op = fop
    full = {"in": ins.get("in", np.zeros(op.get_dims("in").sizes, F)), "filts": ins.get("filts", np.zeros(op.get_dims("filts").sizes, F)), "out_grad_loss": ins["out_grad_loss"]}
    r = R.refs(op, full)
    want = cpu_run_func(cpu, fop, ins)
    if fop.get_func_name() == "hip_bconv_in":
        assert launch["kernel"] == IN_KERNEL, launch
        if "in" in ins:      # zero_if_in_non_pos=1: the select on both sides of the comparison
            sel = ins["in"] > 0
            r = {k: tuple(np.where(sel, v[0], 0.0) if j == 0 else v[j] for j in range(len(v))) for k, v in r.items()}
        R.check_bound(op, "in", got["in_grad_loss"], r, what=f"be=hip pipe {c.tag}")
        R.check_bound(op, "in", want["in_grad_loss"], r, what=f"be=cpu pipe {c.tag}")
    else:
        bk, ksl = R.plan_of(launch, FB_KERNEL)
        R.check_bound(op, "filts", got["filts_grad_loss"], r, ksl=ksl, what=f"be=hip pipe {c.tag}")
        R.check_bound(op, "filts", want["filts_grad_loss"], r, what=f"be=cpu pipe {c.tag}")
        assert R.same_bits(got["biases_grad_loss"].reshape(-1), fb.biases_chain(ins["out_grad_loss"], bk, ksl)), c.tag


def check_nodes_against_float64(what, nodes, loss_tops, hip_fwd, cpu_fwd, f32_fwd, want):
    """Per gradient node the option changes: its distance to the float64 walk is at most twice be=cpu's own in the same mode (both carry the same bf16 rounding of the
    same operands and differ in the order of their fp32 additions).  The nodes the option does NOT change are exactly R.unchanged_grad_nodes(loss_tops) -- a loss top's
    gradient and the bias gradient summed from it, which pass no rounded product: they must hold the bits of the fp32 driver with the same call list
    (fuse_filts_biases=True: the same bias chains) on the same device, f32_fwd, so their distance to float64 is that driver's own (asserted equal), at the 1e-7 level where the GPU's and be=cpu's softmax differ by more than a factor 2 with the option
    off as well (chain fc_grad_loss: be=hip 1.02e-07, be=cpu 2.82e-08)."""
    unchanged = R.unchanged_grad_nodes(loss_tops)
    assert unchanged <= set(nodes)
    for n in nodes:
        eg, ec = ref.rel_err(hip_fwd[n], want[n]), ref.rel_err(cpu_fwd[n], want[n])
        print(f"E {what} {n}: be=hip {eg:.3e} be=cpu {ec:.3e}" + (" (the fp32 driver's bits)" if n in unchanged else ""))
        if n in unchanged:
            assert R.same_bits(hip_fwd[n], f32_fwd[n]), n
            assert eg == ref.rel_err(f32_fwd[n], want[n]) <= CAP, (n, eg)
        else:
            assert not R.same_bits(hip_fwd[n], f32_fwd[n]), n
            assert eg <= 2 * ec, (n, eg, ec)


def pipe_step(rtc, name, **kw):
    mk, tops, seed = PIPES[name]
    cp = mk(); bp = add_bck_ops(cp, loss_tops=tops)
    data, label = small_inputs(cp, seed)
    drv = ConvPipeBck(rtc, **kw); drv.init(bp, small_params(cp, seed))
    drv.set_det_drop_seed(SEED_A)
    fwd = {"data": data, "label": label}
    drv.run_bck(["data", "label"], fwd, grad_nodes(bp) + bp.loss_nodes)
    return drv, bp, fwd


@pytest.mark.parametrize("name", sorted(PIPES))
def test_pipe_call_by_call_and_against_float64(hip, cpu, name):
    from test_gpu_bck_pipe import check_call
    c_drv, bp, c_fwd = pipe_step(cpu, name, grad_operands="bf16")
    c_drv.release()
    d_drv, bp, d_fwd = pipe_step(hip, name, fuse_filts_biases=True)      # the fp32 step with the same call list
    d_drv.release()
    drv, bp, fwd = pipe_step(hip, name, grad_operands="bf16")
    try:
        want = want_f64(name, drv)
        for n in bp.loss_nodes:      # the forward pass and the loss are untouched: the fp32 rules of tests/test_gpu_bck_pipe.py hold for them
            assert abs(fwd[n].item() - want[n]) / abs(want[n]) <= 5e-4
        mk, tops, seed = PIPES[name]
        check_nodes_against_float64(name, [n for n in grad_nodes(bp) if "_split_" not in n], tops or [bp.cp.out_node()], fwd, c_fwd, d_fwd, want)
        data, label = small_inputs(bp.cp, seed)
        hip.copy_nda_to_var("data", data); hip.copy_nda_to_var("label", label)
        for c in drv.bck_calls:      # every call alone, in order, on what the calls before it left
            if c in conv_calls(drv):
                check_conv_call(hip, cpu, c)
            else:
                check_call(hip, cpu, c.tag, c.fop, c.rfc)
        hip.release_per_call_id_data()
        assert len(conv_calls(drv)) == 2 * sum(1 for o in bp.bck_ops() if o.type == "BckConv") >= 4
        assert not any(c.fop.get_func_name() in ("hip_bconv_filts", "hip_bconv_biases") for c in drv.bck_calls)
        for n in grad_nodes(bp):     # stepping through the calls one by one is the same step: the same bits
            assert R.same_bits(hip.copy_var_to_nda(n), fwd[n]), n
    finally:
        drv.release()


def test_residual_pipe(hip, cpu):
    """The residual pipe with the option on: against float64, then every call of the step alone, in order, against be=cpu on the GPU's own inputs -- the two flagged
    conv gradients within the bound, the BatchNorm functions and every other call by the rules of tests/test_gpu_bn.py (bit for bit where the function is)."""
    from test_gpu_bck_pipe import check_call
    seed = BN.RES_SEEDS[0]
    out = {}
    cp = BN.residual(); bp = add_bck_ops(cp)
    params = BN.res_params(cp, seed); data, label = BN.res_inputs(cp, seed)
    want = BN.net_bn_f64(cp, params, data, label)
    for be, rtc, kw in (("cpu", cpu, {"grad_operands": "bf16"}), ("f32", hip, {"fuse_filts_biases": True}), ("hip", hip, {"grad_operands": "bf16"})):
        cp = BN.residual(); bp = add_bck_ops(cp)
        drv = ConvPipeBck(rtc, bn_maf=0.9, **kw); drv.init(bp, params)
        try:
            fwd = {"data": data, "label": label}
            drv.run_bck(["data", "label"], fwd, grad_nodes(bp) + ["loss"])
            out[be] = fwd
            if be != "hip":
                continue
            hip.copy_nda_to_var("data", data); hip.copy_nda_to_var("label", label)
            seen = []
            for c in drv.bck_calls:
                fn = c.fop.get_func_name()
                if c in conv_calls(drv):
                    check_conv_call(hip, cpu, c); seen.append(fn)
                elif fn not in BN_FUNCS:
                    seen.append(check_call(hip, cpu, c.tag, c.fop, c.rfc))
                else:
                    spec = pipe_func_args(c.fop)
                    ins = {an: hip.copy_var_to_nda(c.rfc.arg_map[an].n) for an, io in spec if io in ("IN", "INOUT")}
                    hip.run(c.rfc); hip.finish_and_sync()
                    assert hip.last_launch()["kernel"] in ("bodahip_bn_sum", "bodahip_bn_fwd", "bodahip_bn_bck_in", "bodahip_fan_out")
                    got = {an: hip.copy_var_to_nda(c.rfc.arg_map[an].n) for an, io in spec if io != "IN"}
                    w = BN.run_func(cpu, c.fop, ins, bind={"in_grad_loss": "out_grad_loss"} if fn == "hip_bn_bck_in" else None)[0]
                    for an in got:
                        assert R.same_bits(got[an], w[an]), (c.tag, fn, an)
                    seen.append(fn)
            hip.release_per_call_id_data()
            n_conv = sum(1 for o in bp.bck_ops() if o.type == "BckConv")
            assert len(seen) == len(drv.calls()) and seen.count("hip_bconv_in") == seen.count("hip_bconv_filts_biases") == n_conv
            assert all(seen.count(f) == k for f, k in (("hip_bn_stats", 8), ("hip_bn_fwd", 8), ("hip_bn_bck_sums", 8), ("hip_bn_bck_in", 8), ("hip_fan_out", 2)))
            assert "hip_bconv_filts" not in seen and "hip_bconv_biases" not in seen
            for n in fwd:     # stepping through the calls one by one is the same step (the running pair aside: it has moved twice)
                if n.endswith("_grad_loss") or n == "loss":
                    assert R.same_bits(hip.copy_var_to_nda(n), fwd[n]), n
        finally:
            drv.release()
    assert abs(out["hip"]["loss"].item() - want["loss"]) / abs(want["loss"]) <= 5e-4
    nodes = [n for n in grad_nodes(bp) if "_split_" not in n and float(np.max(np.abs(want[n]))) >= 1e-12]    # (not: a partial gradient; a bias in front of a BatchNorm, exact gradient 0)
    check_nodes_against_float64("residual", nodes, [cp.out_node()], out["hip"], out["cpu"], out["f32"], want)


@pytest.mark.parametrize("name", ["fan"])
def test_graph_replay_with_solver_equals_the_eager_driver(hip, hip2, name):
    mk_solver = lambda: SgdSolver(lr=0.05, momentum=0.9, weight_decay=5e-4, lr_mult={"biases": 2.0}, decay_mult={"biases": 0.0})
    G, bp = S.make_sgd_driver(hip, name, mk_solver(), seed_in_var=True, fuse_relu_grad=True, grad_operands="bf16")
    E, _ = S.make_sgd_driver(hip2, name, mk_solver(), fuse_relu_grad=True, grad_operands="bf16")
    try:
        state = S.state_vars(bp)
        gets = [pn + "_grad_loss" for pn in bp.cp.params] + bp.loss_nodes + state
        rounds = [(SEED_A, 0), (SEED_B, 1), (SEED_A, 2), (SEED_B, 0)]
        for parallel, some in ((False, rounds[:2]), (True, rounds[2:])):
            n = G.capture_graph(parallel=parallel)
            assert n == len(G.calls()) and any(has_bf16_operands(f) for _, f, _ in G.calls())
            for seed, inp in some:
                data, label = small_inputs(bp.cp, inp)
                outs = []
                for d, graph in ((G, True), (E, False)):
                    d.set_det_drop_seed(seed)
                    fwd = {"data": data, "label": label}
                    d.run_bck(["data", "label"], fwd, gets, graph=graph)
                    outs.append(fwd)
                for vn in gets:
                    assert S.same_bits(outs[0][vn], outs[1][vn]), (parallel, seed, inp, vn)
    finally:
        G.release(); E.release()


def test_two_shards(hip):
    multi = make_rtc("(be=hip,devices=0:0)"); multi.init()
    try:
        mk, tops, seed = PIPES["chain"]
        cp = mk(); bp = add_bck_ops(cp, loss_tops=tops)
        drv = ConvPipeBck(multi, grad_operands="bf16")
        with pytest.raises(UnsupErr, match="grad_operands='bf16'"):
            drv.init(bp, small_params(cp, seed))
        assert drv.vars == [] and drv.funcs == []      # refused before anything was created
        op = R.in_op("k1_stride2")                      # three images on two shards; the flagged data gradient runs on img shards as the unflagged one does
        ins = R.rand_ins(op, 9)
        a = R.run_fop(multi, R.in_func(op), ins)
        R.check_bound(op, "in", a["in_grad_loss"], R.refs(op, ins), what="be=hip devices=0:0")
        assert R.same_bits(a["in_grad_loss"], R.run_fop(hip, R.in_func(op), ins)["in_grad_loss"])      # independent per image: the one-device bits
        with pytest.raises(UnsupErr, match="hip_bconv_filts_biases"):
            R.run_fop(multi, R.fb_func(op), ins)
    finally:
        multi.close()
