"""The training BatchNorm over img chunks on the MI355X (kernels/bn_f32.hip).  One device: the four hip_bnc_* functions bit for bit against be=cpu
and the numpy twin of the chunked chain (tests/bnc_ref.py), the hip_split copy an Eltwise gradient runs as, and ConvPipeBck(img_chunks=2) as a serial and a parallel
hipGraph replay against the eager step.  Several devices (shards of device 0, like tests/test_gpu_bck_shards.py): every function against be=cpu with chunks = the device
count, every device's replicas of the per-channel results, the residual pipe's step against the ONE-device step with the same img_chunks, a solver, and the refusals.

Every function comparison is np.array_equal on the uint32 views; outputs start from NaN with a guard var behind each (bn_ref.run_func) and every summing call is
launched twice on the same workspace.  The cross-device path runs on shards of ONE physical GPU here: that exercises the chain, the exchange and its event order, and
says nothing about scaling."""
import numpy as np
import pytest

import bck_pipe_ref as pref
import bck_shards_ref as sref
import bn_ref as R
import bnc_ref as RC
import test_bn_cpu as T
import test_bnc_cpu as TC
from boda_amd.bck_pipe import ConvPipeBck, SgdSolver, add_bck_ops
from boda_amd.cnn_op import OpTune, add_pipe_op_annotations, bnc_bck_in_func_op, bnc_bck_sums_func_op, bnc_fwd_func_op, bnc_stats_func_op, pipe_func_args
from boda_amd.op import Nda, Op, RtErr, UnsupErr
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc

pytestmark = pytest.mark.gpu

RES4_SEED = 26209     # data / param seed of the four-image residual pipe for which the float64 walk passes its guards (found as bn_ref.RES_SEEDS were)
KEYS = ("mean", "inv_std", "run_mean2", "run_var2", "out", "sg", "bg", "dx")


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


@pytest.fixture(scope="module")
def multis():
    made = {}
    for n in (2, 3):
        made[n] = make_rtc("(be=hip,devices=" + ":".join(["0"] * n) + ")"); made[n].init()
    yield made
    for r in made.values():
        r.close()


# ---- one device
@pytest.mark.parametrize("case", RC.CASES, ids=RC.case_id)
def test_functions_against_cpu_and_numpy(hip, cpu, case):
    shape, n, slab = case
    relu = (shape[0] + shape[1]) % 2
    g = RC.run_all_four(hip, shape, n, slab, relu=relu, repeat=2)      # (every summing function launched twice on the same workspace)
    c = RC.run_all_four(cpu, shape, n, slab, relu=relu)
    for k in KEYS:
        assert R.same_bits(g[k], c[k]), k
    RC.check_against_numpy(g, shape, n, slab, relu=relu)


@pytest.mark.parametrize("case", [c for c in R.CASES if c[1] == 0], ids=R.case_id)
def test_one_chunk_is_the_twin_function(hip, case):
    shape, slab = case
    a = RC.run_all_four(hip, shape, 1, slab)
    b = R.run_all_five(hip, shape, slab)
    for k in KEYS:
        assert R.same_bits(a[k], b[k]), k


def test_big_term_case(hip):
    assert TC.big_term_sums(hip) == {1: 16777218.0, 2: 16777220.0}


def test_in_place_forms_and_refusals(hip):
    shape, n = (5, 65, 4, 4), 3
    d = R.dims_of(shape)
    r = RC.run_all_four(hip, shape, n)
    common = {"in": r["x"], "mean": r["mean"], "inv_std": r["inv_std"]}
    out = R.run_func(hip, bnc_fwd_func_op(d, 1), dict(common, scale=r["scale"], bias=r["bias"]), bind={"out": "in"})[0]["out"]
    assert R.same_bits(out, r["out"])
    dx = R.run_func(hip, bnc_bck_in_func_op(d), dict(common, scale=r["scale"], scale_grad_loss=r["sg"], bias_grad_loss=r["bg"], out_grad_loss=r["dy"]),
                    bind={"in_grad_loss": "out_grad_loss"})[0]["in_grad_loss"]
    assert R.same_bits(dx, r["dx"])
    TC.var_refusals(hip)


def split_copy_op(d):
    """The function op ConvPipeBck(img_chunks=n) emits per output of a BckEltwise: hip_split of ALL of in's channels."""
    return add_pipe_op_annotations(Op({"type": "Split"}, {"in": Nda(d), "outs_0": Nda(d), "outs_num": Nda(None, "uint32_t", (1,))}), OpTune())[0]


@pytest.mark.parametrize("shape", [(2, 3, 1, 1), (3, 5, 3, 3), (5, 65, 4, 4), (2, 3, 57, 57)], ids=lambda s: "x".join(map(str, s)))
def test_split_copies_bit_for_bit(hip, shape):
    """A full-range hip_split (icix=0, out of in's dims) is a copy of the bits: -0.0, infinities, denormals, quiet and signalling NaNs with payloads."""
    x = R.make_inputs(shape)["x"]
    w = x.reshape(-1).view(np.uint32)
    special = np.array([0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x7FC00000, 0xFFC0BEEF, 0x7F800001, 0xFFBFFFFF, 0x7FFFFFFF], np.uint32)
    k = min(special.size, w.size)
    w[:k] = special[:k]; w[-1] = 0xFFC00123
    f = split_copy_op(R.dims_of(shape))
    assert f.get_func_name() == "hip_split" and f.get_u32("icix") == 0 and f.get_dims("in") == f.get_dims("out")
    out = R.run_func(hip, f, {"in": x})[0]["out"]
    assert np.array_equal(out.reshape(-1).view(np.uint32), w)


def graph_rounds(hip, hip2, parallel):
    cp = R.residual(); bp = add_bck_ops(cp)
    G = ConvPipeBck(hip, bn_maf=0.9, seed_in_var=True, img_chunks=2); G.init(bp, R.res_params(cp, 1))
    E = ConvPipeBck(hip2, bn_maf=0.9, img_chunks=2); E.init(add_bck_ops(R.residual()), R.res_params(cp, 1))
    try:
        gets = [n for n in bp.nodes if n.endswith("_grad_loss")] + ["loss"] + list(cp.params)
        before = {n: hip.copy_var_to_nda(n) for n in cp.params}
        assert G.capture_graph(parallel=parallel) == len(G.calls())
        for vn in cp.params:     # a capture leaves the params, the running statistics among them, as they were
            assert R.same_bits(before[vn], hip.copy_var_to_nda(vn)), vn
        for inp in (21, 22):
            data, label = R.res_inputs(cp, inp)
            outs = []
            for d, graph in ((G, True), (E, False)):
                fwd = {"data": data, "label": label}
                d.run_bck(["data", "label"], fwd, gets, graph=graph)
                outs.append(fwd)
            for vn in gets:
                assert R.same_bits(outs[0][vn], outs[1][vn]), (parallel, inp, vn)
            assert not R.same_bits(outs[0]["bn_stem_mean"], before["bn_stem_mean"])
    finally:
        G.release(); E.release()


def test_serial_graph_replay(hip, hip2):
    graph_rounds(hip, hip2, False)


def test_parallel_graph_replay(hip, hip2):
    graph_rounds(hip, hip2, True)


def test_one_device_step_with_three_chunks(hip):
    """The wiring of the one-device step with img_chunks=3: the first layer's batch statistics against the twin on the GPU's own stem_bn_in, bit for bit, and every node
    against the float64 walk under the cap."""
    drv, bp, params, data, label, fwd = T.res_step(hip, R.RES_SEEDS[0], img_chunks=3)
    try:
        x = hip.copy_var_to_nda("stem_bn_in")
        eps = next(o for o in bp.cp.ops if o.tag == "bn_stem").eps
        mean, istd, _, _ = RC.stats_np(x, params["bn_stem_mean"], params["bn_stem_var"], 3, eps, 0.9)
        assert R.same_bits(fwd["bn_stem_batch_mean"], mean) and R.same_bits(fwd["bn_stem_batch_inv_std"], istd)
        worst = T.check_against_f64(bp, params, data, label, fwd, "be=hip", T.CAP)
        print(f"be=hip residual img_chunks=3: largest max|got - want| / max|want| = {worst:.3e}")
    finally:
        drv.release()


# ---- several devices: shards of device 0
def run_on_devices(multi, n_dev, fop, ins, probe=(), repeat=1):
    """bn_ref.run_func on a multi-device backend, with every device's copy of the replicated vars `probe` read (bck_shards_ref.probe_copies) before the vars go
    -> ([{arg: array}] per run, {arg: (n_dev, C) copies})."""
    spec = pipe_func_args(fop)
    multi.compile([RtcFuncInfo("bnc_f", "", [a for a, _ in spec], fop)])
    made, am = [], {}
    try:
        for an, io in spec:
            vn = "bncv_" + an
            d = fop.get_dims(an)
            multi.create_var_with_dims(vn, d); made.append(vn); am[an] = RtcArg.var(vn)
            multi.copy_nda_to_var(vn, np.ascontiguousarray(ins[an], R.F).reshape(d.sizes) if an in ins else np.full(d.sizes, np.nan, R.F))
        res = []
        for _ in range(repeat):
            multi.run(RtcFuncCall("bnc_f", am)); multi.finish_and_sync()
            res.append({an: multi.copy_var_to_nda(am[an].n) for an, io in spec if io != "IN"})
        copies = {an: sref.probe_copies(multi, am[an].n, n_dev) for an in probe}
        for an, io in spec:
            if io == "IN" and an in ins:
                assert R.same_bits(multi.copy_var_to_nda(am[an].n).reshape(-1), np.asarray(ins[an], R.F).reshape(-1)), (an, "an IN arg was written")
        return res, copies
    finally:
        for vn in made:
            multi.release_var(vn)
        multi.release_func("bnc_f"); multi.release_per_call_id_data()


def same_on_every_device(copies, want):
    for an, rows in copies.items():
        for i, row in enumerate(rows):     # (probe_copies reads a -0 back as +0: compared as values where the bits differ only in that)
            w = np.asarray(want[an], R.F).reshape(-1)
            assert np.array_equal(row.view(np.uint32), (w + R.F(0)).view(np.uint32)), (an, "device", i)


DEV_CASES = [((2, 4, 2, 2), 3, 0), ((2, 3, 57, 57), 2, 2000), ((3, 5, 3, 3), 2, 0), ((3, 5, 3, 3), 3, 0), ((5, 65, 4, 4), 3, 16), ((1, 1, 1, 1), 2, 0)]


@pytest.mark.parametrize("case", DEV_CASES, ids=RC.case_id)
def test_functions_on_devices_against_cpu(multis, cpu, case):
    """chunks = the device count; (2,4,2,2) x 3 leaves device 0 without images, (1,1,1,1) x 2 likewise."""
    shape, n, slab = case
    multi = multis[n]
    d = R.dims_of(shape)
    c = RC.run_all_four(cpu, shape, n, slab, relu=1, repeat=2)
    i = R.make_inputs(shape)
    sts, cp1 = run_on_devices(multi, n, bnc_stats_func_op(d, R.EPS, R.MAF, n, slab), {"in": i["x"], "run_mean": i["run_mean"], "run_var": i["run_var"]},
                              probe=("mean", "inv_std", "run_mean", "run_var"), repeat=2)
    assert R.same_bits(sts[0]["mean"], c["mean"]) and R.same_bits(sts[0]["inv_std"], c["inv_std"])
    assert R.same_bits(sts[0]["run_mean"], c["run_mean2"]) and R.same_bits(sts[0]["run_var"], c["run_var2"])
    assert R.same_bits(sts[1]["mean"], c["mean"]) and R.same_bits(sts[1]["run_mean"], c["run_mean3"]) and R.same_bits(sts[1]["run_var"], c["run_var3"])
    same_on_every_device(cp1, sts[1])
    common = {"in": i["x"], "mean": c["mean"], "inv_std": c["inv_std"]}
    out, _ = run_on_devices(multi, n, bnc_fwd_func_op(d, 1), dict(common, scale=i["scale"], bias=i["bias"]))
    assert R.same_bits(out[0]["out"], c["out"])
    sums, cp2 = run_on_devices(multi, n, bnc_bck_sums_func_op(d, n, slab), dict(common, out_grad_loss=i["dy"]), probe=("scale_grad_loss", "bias_grad_loss"), repeat=2)
    for s in sums:
        assert R.same_bits(s["scale_grad_loss"], c["sg"]) and R.same_bits(s["bias_grad_loss"], c["bg"])
    same_on_every_device(cp2, sums[0])
    dx, _ = run_on_devices(multi, n, bnc_bck_in_func_op(d), dict(common, scale=i["scale"], scale_grad_loss=c["sg"], bias_grad_loss=c["bg"], out_grad_loss=i["dy"]))
    assert R.same_bits(dx[0]["in_grad_loss"], c["dx"])


def test_chunks_must_be_the_device_count(multis):
    d = R.dims_of((4, 3, 2, 2))
    for f in (bnc_stats_func_op(d, R.EPS, R.MAF, 3), bnc_bck_sums_func_op(d, 3)):
        with pytest.raises(RtErr, match="chunks=3 on 2 devices"):
            multis[2].compile([RtcFuncInfo("bnc_bad", "", [a for a, _ in pipe_func_args(f)], f)])
    f = bnc_stats_func_op(d, R.EPS, R.MAF, 2)      # (nothing was left behind: the name is free)
    multis[2].compile([RtcFuncInfo("bnc_bad", "", [a for a, _ in pipe_func_args(f)], f)])
    multis[2].release_func("bnc_bad")


# ---- the driver on several devices
def step(rtc, B, seed, **kw):
    cp = R.residual(B); bp = add_bck_ops(cp)
    params = R.res_params(cp, seed); data, label = R.res_inputs(cp, seed)
    drv = ConvPipeBck(rtc, bn_maf=0.9, **kw); drv.init(bp, params)
    fwd = {"data": data, "label": label}
    gets = [n for n in bp.nodes if n.endswith("_grad_loss")] + ["loss"] + list(cp.params) + [o.tag + s for o in cp.ops if o.type == "BatchNorm" for s in ("_batch_mean", "_batch_inv_std")]
    drv.run_bck(["data", "label"], fwd, gets)
    return drv, bp, params, data, label, fwd


def test_driver_on_two_devices_against_one(hip, multis):
    """Every node but the convolutions' filter / bias gradients holds the bits of the one-device step with the same img_chunks; those follow the shard-sum chain of
    DESIGN.md section 3.13 and are held to the float64 walk under the cap."""
    one, bp, params, data, label, want = step(hip, 4, RES4_SEED, img_chunks=2)
    one.release()
    drv, bp, params, data, label, got = step(multis[2], 4, RES4_SEED, img_chunks=2)
    try:
        assert sum(f.has("img_shards") for _, f, _ in drv.calls()) > 0      # the five functions are flagged as on every other net
        conv_sums = [n for n in got if n.endswith("_filts_grad_loss") or n.endswith("_biases_grad_loss")]
        assert len(conv_sums) == 2 * 9      # (the pipe has nine convolutions)
        for n in got:
            if n not in conv_sums:
                assert R.same_bits(got[n], want[n]), n
        f64 = R.net_bn_f64(bp.cp, params, data, label)
        zero_biases = {o.bot + "_biases_grad_loss": o.bot for o in bp.cp.ops if o.type == "BatchNorm"}     # exact gradient 0: held as test_bn_cpu.check_against_f64 holds them
        for n in conv_sums:
            if n in zero_biases:
                err = float(np.max(np.abs(got[n])) / np.max(np.abs(f64[zero_biases[n] + "_grad_loss"]).sum(axis=(0, 2, 3))))
            else:
                err = pref.rel_err(got[n], f64[n])
            assert err <= T.CAP, (n, err)
        for vn in ("scale_stem_scale_grad_loss", "scale_b_2c_bias_grad_loss", "bn_stem_mean", "bn_a_2b_var", "bn_stem_batch_mean", "bn_b_2c_batch_inv_std"):
            rows = sref.probe_copies(multis[2], vn, 2)
            assert np.array_equal(rows[0].view(np.uint32), rows[1].view(np.uint32)), vn
    finally:
        drv.release()


def test_driver_refusals_on_devices(multis):
    cp = R.residual(4); bp = add_bck_ops(cp)
    drv = ConvPipeBck(multis[2], img_chunks=3)
    with pytest.raises(RtErr, match="img_chunks=3 on 2 devices"):
        drv.init(bp, R.res_params(cp, 1))
    assert drv.vars == [] and drv.funcs == []      # refused before anything was created
    drv = ConvPipeBck(multis[2], img_chunks=2); drv.init(bp, R.res_params(cp, 1))
    try:
        with pytest.raises(UnsupErr, match="capture_graph: not provided on a multi-device backend"):
            drv.capture_graph()
    finally:
        drv.release()
    for kw in ({"fuse_filts_biases": True}, {"grad_operands": "bf16"}):
        drv = ConvPipeBck(multis[2], img_chunks=2, **kw)
        with pytest.raises(UnsupErr, match="not provided on a multi-device"):
            drv.init(bp, R.res_params(cp, 1))
        assert drv.vars == []


def test_capturing_a_call_on_devices_is_refused(multis):
    multi = multis[2]
    d = R.dims_of((4, 3, 2, 2))
    f = bnc_bck_sums_func_op(d, 2)
    spec = pipe_func_args(f)
    multi.compile([RtcFuncInfo("bnc_cap", "", [a for a, _ in spec], f)])
    made = []
    try:
        for an, _ in spec:
            multi.create_var_with_dims("cap_" + an, f.get_dims(an)); made.append("cap_" + an)
        call = RtcFuncCall("bnc_cap", {an: RtcArg.var("cap_" + an) for an, _ in spec})
        multi.run(call); multi.finish_and_sync()
        multi.graph_begin()
        with pytest.raises(UnsupErr, match="hip_bnc_bck_sums.*cannot be captured into a graph"):
            multi.run(call)
        multi.run(call); multi.finish_and_sync()      # the capture was dropped: the backend runs on
    finally:
        for vn in made:
            multi.release_var(vn)
        multi.release_func("bnc_cap"); multi.release_per_call_id_data()


def test_solver_three_steps_on_two_devices(multis):
    multi = multis[2]
    solver = SgdSolver(lr=0.05, momentum=0.9, weight_decay=5e-4, lr_mult={"biases": 2.0, "scale": 0.5}, decay_mult={"biases": 0.0, "bias": 0.0, "scale": 0.0})
    cp = R.residual(4); bp = add_bck_ops(cp)
    drv = ConvPipeBck(multi, solver=solver, bn_maf=0.9, img_chunks=2); drv.init(bp, R.res_params(cp, 1))
    try:
        start = multi.copy_var_to_nda("scale_stem_scale")
        for k in range(3):
            data, label = R.res_inputs(cp, 100 + k)
            fwd = {"data": data, "label": label}
            drv.run_bck(["data", "label"], fwd, ["loss"])
            assert np.isfinite(fwd["loss"]).all()
        rows = sref.probe_copies(multi, "scale_stem_scale", 2)
        assert np.array_equal(rows[0].view(np.uint32), rows[1].view(np.uint32)) and not R.same_bits(multi.copy_var_to_nda("scale_stem_scale"), start)
    finally:
        drv.release()
