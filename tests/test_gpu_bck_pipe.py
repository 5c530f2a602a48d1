"""The full-net gradient pipe on the MI355X: the four plumbing kernels of kernels/bck_ops_f32.hip (bodahip_reduce, bodahip_dropout, bodahip_concat, bodahip_split) bit for
bit against be=cpu, the three small pipes of tests/test_bck_pipe_cpu.py on be=hip -- per node against the float64 backprop (the wiring) and call by call against be=cpu on
the GPU's own inputs (the kernels) --, one step of NiN at two images, and the functions on img shards of a multi-device backend.

Call by call, each function is held to the rule it already has (DESIGN.md sections 3.11 / 3.12): bit-identical to be=cpu, except the written float64 bounds of lrn_sb's
out, bck_lrn, softmax's prob and loss_per_pel, and the filter / bias gradients, which equal oracle/bck_chain.py's emulation of the launch's own K slices."""
import numpy as np
import pytest

import bck_ops_ref as oref
import bck_pipe_ref as ref
from boda_amd import rtc as rtc_mod
from boda_amd.bck_pipe import ConvPipeBck, add_bck_ops
from boda_amd.cnn_op import OpTune, add_bck_op_annotations, pipe_func_args
from boda_amd.conv_pipe import nin_imagenet
from boda_amd.op import RtErr, UnsupErr, parse_op
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc
from oracle import bck_chain as bc

from test_bck_conv_cpu import FILTS_MRD, mrd
from test_bck_pipe_cpu import (CAP, PIPES, SEED_A, ann, bits_eq, check_against_f64, concat_inputs, concat_op, concat_round_trip, dropout_op, grad_nodes, reduce_inputs, reduce_op,
                               run_func, run_pipe)

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


def gpu(hip, fop, ins, **kw):
    """run_func on the GPU; the launch must be the function's own kernel."""
    keep = []
    outs = run_func(hip, fop, ins, keep=keep, **kw)
    assert keep == ["bodahip_" + fop.get_func_name()[4:]], keep
    return outs


# ---- the four kernels
@pytest.mark.parametrize("n", [2, 3, 8])
def test_reduce(hip, cpu, n):
    xs = reduce_inputs(n)   # 1023 elements: 255 quads and a tail of three
    ins = {f"ins_{i}": x for i, x in enumerate(xs)}
    f = ann(reduce_op(n))[0]
    got = gpu(hip, f, ins)["out"]
    assert bits_eq(got, run_func(cpu, f, ins)["out"]) and bits_eq(got, ref.reduce_f32(xs))
    assert bits_eq(got[:1], np.zeros(1, np.float32)) and got[1] == (2.0 ** 24 if n == 2 else 0.0)


def test_reduce_several_workgroups_4d(hip, cpu):
    f = ann(reduce_op(4, "(dims=(img=3,chan=7,y=13,x=11))"))[0]   # 3003 elements: three workgroups of quads, a tail of three
    xs = reduce_inputs(4, 3003, seed=5)
    ins = {f"ins_{i}": x.reshape(3, 7, 13, 11) for i, x in enumerate(xs)}
    assert bits_eq(gpu(hip, f, ins)["out"], run_func(cpu, f, ins)["out"])


@pytest.mark.parametrize("ratio", [0.5, 0.1])
def test_dropout_and_seed_is_no_compile(hip, cpu, ratio):
    x = np.random.default_rng(3).uniform(-2, 2, (2, 3, 7, 11)).astype(np.float32)   # 462 elements: 115 quads and a tail of two
    f = ann(dropout_op(ratio))[0]
    hit = ref.dropout_seed_hitting(ratio, 5)   # element 5 hashes to exactly the threshold: dropped by `>`
    assert gpu(hip, f, {"inout": x}, seed=hit)["inout"].ravel()[5] == 0 and x.ravel()[5] != 0
    for seed in (7, 8, 2 ** 32 - 100, hit):
        got = gpu(hip, f, {"inout": x}, seed=seed)["inout"]
        assert bits_eq(got, run_func(cpu, f, {"inout": x}, seed=seed)["inout"]) and bits_eq(got, ref.dropout_f32(x, ratio, seed))
    before = rtc_mod.compile_stats()
    got = gpu(hip, f, {"inout": x}, seed=12345)["inout"]   # a seed never seen: no compile, not even a cache look-up
    after = rtc_mod.compile_stats()
    assert (after["compiled"], after["cache_hits"]) == (before["compiled"], before["cache_hits"])
    assert bits_eq(got, ref.dropout_f32(x, ratio, 12345))


def test_concat_split_aligned_and_misaligned(hip, cpu):
    keep = []
    g = concat_round_trip(hip, 2, (1, 2, 5), 3, 5, keep=keep)        # runs of 15 / 30 / 75 floats: scalars
    assert bits_eq(g, concat_round_trip(cpu, 2, (1, 2, 5), 3, 5))
    g = concat_round_trip(hip, 3, (4, 8, 4), 2, 2, keep=keep)        # every run a multiple of four floats at a multiple of four: quads
    assert bits_eq(g, concat_round_trip(cpu, 3, (4, 8, 4), 2, 2))
    assert keep == (["bodahip_concat"] * 3 + ["bodahip_split"] * 3) * 2
    xs = concat_inputs(2, (3, 4), 2, 2, seed=9)                        # 12 + 16 floats per image: the second range starts on a quad, the first is whole quads too
    wide = np.zeros((2, 7, 2, 2), np.float32)
    for f, x in zip(ann(concat_op(2, (3, 4), 2, 2)), xs):
        wide = gpu(hip, f, {"in": x, "out": wide})["out"]
    assert bits_eq(wide, ref.concat_f32(xs))
    for f, x in zip(ann(concat_op(2, (3, 4), 2, 2, typ="Split")), xs):
        assert bits_eq(gpu(hip, f, {"in": wide})["out"], x)
    big = concat_inputs(2, (40, 24), 9, 7, seed=10)                    # several workgroups; 63-float planes: scalars
    wide = np.zeros((2, 64, 9, 7), np.float32)
    for f, x in zip(ann(concat_op(2, (40, 24), 9, 7)), big):
        wide = gpu(hip, f, {"in": x, "out": wide})["out"]
    assert bits_eq(wide, ref.concat_f32(big))


def test_in_place_zero_if_non_pos_and_dropout(hip, cpu):
    """`in` and `out` bound to ONE var, as the pipe does."""
    from test_bck_ops_cpu import zinp_data, zinp_op
    x, cond = zinp_data(1023, seed=4)
    fz = add_bck_op_annotations(zinp_op((("v", 1023),)), OpTune())[0]
    got = gpu(hip, fz, {"in": x, "cond": cond}, alias={"out": "in"})["out"]
    assert bits_eq(got, oref.zero_if_non_pos_f32(x, cond)) and bits_eq(got, run_func(cpu, fz, {"in": x, "cond": cond}, alias={"out": "in"})["out"])
    self_cond = gpu(hip, fz, {"in": x}, alias={"out": "in", "cond": "in"})["out"]   # the node as its own condition: a ReLU
    assert bits_eq(self_cond, oref.zero_if_non_pos_f32(x, x))
    fd = ann(dropout_op(0.5, "(dims=(v=1023))"))[0]
    assert bits_eq(gpu(hip, fd, {"inout": x}, seed=3)["inout"], ref.dropout_f32(x, 0.5, 3))


def test_refusals(hip):
    f = ann(reduce_op(2))[0]
    hip.compile([RtcFuncInfo("g", "", ["ins_0", "ins_1", "out"], f)])
    try:
        from boda_amd.op import Dims
        for an, n in (("ins_0", 1023), ("ins_1", 1022), ("out", 1023)):
            hip.create_var_with_dims(an, Dims(("v",), (n,), "float"))
        with pytest.raises(RtErr, match="the op says"):
            hip.run(RtcFuncCall("g", {an: RtcArg.var(an) for an in ("ins_0", "ins_1", "out")}))
    finally:
        for an in ("ins_0", "ins_1", "out"):
            hip.release_var(an)
        hip.release_func("g")
    fd = ann(dropout_op(0.5))[0]; fd.nda_vals["dropout_ratio"] = parse_op("(str_vals=(type=x),nda_vals=(r=(tn=float,v=1.0)))").get("r")
    with pytest.raises(RtErr, match="inside"):
        run_func(hip, fd, {"inout": np.zeros((2, 3, 7, 11), np.float32)}, seed=1)
    fc = ann(concat_op(2, (1, 2, 5), 3, 5))[2]; fc.nda_vals["ocix"] = parse_op("(str_vals=(type=x),nda_vals=(n=(tn=uint32_t,v=4)))").get("n")
    with pytest.raises(RtErr, match="do not fit"):
        run_func(hip, fc, {"in": np.zeros((2, 5, 3, 5), np.float32)})


# ---- the three small pipes
@pytest.mark.parametrize("name", sorted(PIPES))
def test_pipe_against_float64(hip, name):
    """The wiring: a wrong var would pass call by call, not this."""
    drv, bp, params, data, label, fwd = run_pipe(hip, name)
    try:
        check_against_f64(name, drv, bp, fwd, "be=hip")
    finally:
        drv.release()


BIT_EXACT = {"hip_conv", "hip_pool_yx", "hip_spreading", "hip_zero_if_non_pos", "hip_sum_loss_over_imgs", "hip_bconv_in", "hip_reduce", "hip_dropout",
             "hip_concat", "hip_split"}


def check_call(hip, cpu, tag, fop, rfc):
    """Run one call of the step on the GPU and the same function on be=cpu on the GPU's own inputs; compare by the function's rule."""
    fn = fop.get_func_name()
    spec = pipe_func_args(fop)
    am = rfc.arg_map
    ins = {an: hip.copy_var_to_nda(am[an].n) for an, io in spec if io in ("IN", "OUT")}   # (OUT too: in-place functions, the other ranges of a concat output)
    hip.run(rfc); hip.finish_and_sync()
    launch = hip.last_launch()
    assert launch["kernel"].startswith("bodahip_"), launch
    if fn not in ("hip_conv", "hip_bconv_in", "hip_bconv_filts", "hip_bconv_biases"):
        assert launch["kernel"] == "bodahip_" + fn[4:], (tag, launch)
    got = {an: hip.copy_var_to_nda(am[an].n) for an, io in spec if io == "OUT"}
    seed = int(am["det_drop_seed"].v[0]) if "det_drop_seed" in am else None
    want = run_func(cpu, fop, ins, seed=seed)
    U = oref.U
    if fn in BIT_EXACT:
        for an in got:
            assert bits_eq(got[an], want[an]), (tag, fn, an)
    elif fn == "hip_lrn_sb":
        assert bits_eq(got["out_scale_base"], want["out_scale_base"])
        w = oref.lrn_out_f64(ins["in"], want["out_scale_base"], fop.get_f32("beta"))
        assert np.all(np.abs(got["out"] - w) <= 8 * U * np.abs(w)), (tag, fn)
    elif fn == "hip_bck_lrn":
        ls = fop.get_u32("local_size")
        w, S = oref.bck_lrn_f64(ins["in"], ins["out"], ins["out_grad_loss"], ins["out_scale_base"], ls, fop.get_f32("alpha"), fop.get_f32("beta"), fop.get_f32("k"))
        assert np.all(np.abs(got["in_grad_loss"] - w) <= 2 * (ls + 8) * U * S), (tag, fn)
    elif fn == "hip_softmax":
        w = oref.softmax_f64(ins["in"]); C = w.shape[1]
        assert np.all(np.abs(got["prob"] - w) <= (C + 8) * U * w), (tag, fn)
    elif fn == "hip_sm_grad_and_loss":
        assert bits_eq(got["in_grad_loss"], want["in_grad_loss"]), (tag, fn)
        wl = oref.loss_per_pel_f64(ins["prob"], ins["label"])
        assert np.all(np.abs(got["loss_per_pel"] - wl) <= 4 * U * np.maximum(1.0, np.abs(wl))), (tag, fn)
    elif fn == "hip_bconv_biases":
        assert bits_eq(got["biases_grad_loss"], bc.biases_chain(ins["out_grad_loss"])), (tag, fn)
    elif fn == "hip_bconv_filts":
        cfg = launch["cfg"]
        bk, ksl = int(cfg.split("_")[0].split("x")[2]), (int(cfg.split("_s")[1].split("_")[0]) if "_s" in cfg else 1)
        I, J = bc.filts_operands(ins["in"], ins["out_grad_loss"], fop.bck_conv_geom())
        assert bits_eq(got["filts_grad_loss"], bc.filts_sliced_chain(I, J, bk, ksl, got["filts_grad_loss"].shape)), (tag, fn, cfg)
    else:
        raise AssertionError(f"no rule for {fn}")
    return fn


@pytest.mark.parametrize("name", sorted(PIPES))
def test_pipe_call_by_call(hip, cpu, name):
    """The kernels, independent of the plumbing."""
    drv, bp, params, data, label, fwd = run_pipe(hip, name)   # (one whole step first: every kernel specialised, every var holding sane data)
    try:
        hip.copy_nda_to_var("data", data); hip.copy_nda_to_var("label", label)
        seen = [check_call(hip, cpu, c.tag, c.fop, c.rfc) for c in drv.bck_calls]
        hip.release_per_call_id_data()
        assert len(seen) == len(drv.calls()) and "hip_bconv_filts" in seen and "hip_softmax" in seen
        again = {n: hip.copy_var_to_nda(n) for n in grad_nodes(bp)}   # stepping through the calls one by one is the same step
        for n in again:
            assert bits_eq(again[n], fwd[n]), n
    finally:
        drv.release()


def test_loss_per_pel_bound(hip, cpu):
    drv, bp, params, data, label, fwd = run_pipe(hip, "chain")
    try:
        prob, lpp = hip.copy_var_to_nda("loss_prob"), hip.copy_var_to_nda("loss_per_pel")
        wl = oref.loss_per_pel_f64(prob, label)
        assert np.all(np.abs(lpp - wl) <= 4 * oref.U * np.maximum(1.0, np.abs(wl)))
    finally:
        drv.release()


def test_seed_protocol(hip):
    a1 = run_pipe(hip, "chain", SEED_A); a1[0].release()
    b = run_pipe(hip, "chain", 99); b[0].release()
    a2 = run_pipe(hip, "chain", SEED_A); a2[0].release()
    for n in grad_nodes(a1[1]) + ["loss"]:
        assert bits_eq(a1[5][n], a2[5][n]), n
    assert not bits_eq(a1[5]["conv1_filts_grad_loss"], b[5]["conv1_filts_grad_loss"])


# ---- one real net
def test_nin_two_images(hip):
    cp = nin_imagenet(2); bp = add_bck_ops(cp)
    drv = ConvPipeBck(hip); drv.init(bp)
    try:
        drv.set_det_drop_seed(5)
        rng = np.random.default_rng(0)
        data = rng.uniform(-1, 1, cp.nodes["data"].sizes).astype(np.float32)
        label = np.array([3, 998], np.float32).reshape(2, 1, 1)
        gets = grad_nodes(bp) + ["loss", "pool4"]
        fwd = {"data": data, "label": label}
        drv.run_bck(["data", "label"], fwd, gets)
        z = fwd["pool4"].astype(np.float64).reshape(2, -1)
        lse = z.max(axis=1) + np.log(np.exp(z - z.max(axis=1, keepdims=True)).sum(axis=1))
        want = float(np.mean(lse - z[np.arange(2), [3, 998]]))
        print(f"NiN loss {fwd['loss'].item():.6f} want {want:.6f}")
        assert abs(fwd["loss"].item() - want) <= 4 * oref.U * max(1.0, abs(want))
        for n in grad_nodes(bp):
            assert fwd[n].shape == tuple(bp.nodes[n].sizes) and np.all(np.isfinite(fwd[n])), n
        assert np.any(fwd["conv1_filts_grad_loss"] != 0) and np.any(fwd["data_grad_loss"] != 0)
        g = fwd["conv1_grad_loss"].astype(np.float64)
        assert mrd(fwd["conv1_biases_grad_loss"], g.sum(axis=(0, 2, 3))) < FILTS_MRD
    finally:
        drv.release()


# ---- several devices
def test_multi_device(hip):
    """devices=0:0: three images split between two backends on one GPU.  The three per-image functions equal one device bit for bit; dropout is refused."""
    r = make_rtc("(be=hip,devices=0:0)")
    r.init()
    try:
        d4 = "(dims=(img=3,chan=5,y=3,x=5))"
        xs = [x.reshape(3, 5, 3, 5) for x in reduce_inputs(3, 225, seed=31)]
        f = ann(reduce_op(3, d4))[0]; ins = {f"ins_{i}": x for i, x in enumerate(xs)}
        assert bits_eq(gpu(hip, f, ins)["out"], run_func(r, f, ins)["out"])
        assert bits_eq(concat_round_trip(hip, 3, (1, 2, 5), 3, 5, keep=[]), concat_round_trip(r, 3, (1, 2, 5), 3, 5))
        with pytest.raises(UnsupErr, match="GLOBAL flat index"):
            run_func(r, ann(dropout_op(0.5, d4))[0], {"inout": xs[0]}, seed=1)
    finally:
        r.close()
