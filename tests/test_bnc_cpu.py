"""The training BatchNorm over img chunks without a GPU: the four hip_bnc_* functions on be=cpu bit for bit against the numpy twin of the chunked
chain (tests/bnc_ref.py), chunks=1 against the hip_bn_* functions, the tables, the refusals, and ConvPipeBck(img_chunks=n) on be=cpu: n=1 bit for bit against the default
driver, n=2 and 3 against the float64 walk under the existing cap, with a solver, and with its call list run in other topological orders.

The float64 comparison uses test_bn_cpu's cap 5e-4 on max|got - want| / max|want| per node and its three seeds: the float64 walk's guard is a property of the data, not
of the chunking.  The largest value seen is printed (run with -s) and recorded in DESIGN.md; nothing is gated on a multiple of it.  Conv-bias nodes in front of a
BatchNorm are held as test_bn_cpu.check_against_f64 holds them."""
import numpy as np
import pytest

import bn_ref as R
import bnc_ref as RC
import test_bn_cpu as T
from boda_amd import rtc as rtc_mod
from boda_amd.bck_pipe import SGD_HIST_SFX, ConvPipeBck, SgdSolver, add_bck_ops
from boda_amd.cnn_op import (BN_OP_FUNCS, BNC_OP_FUNCS, IMG_SHARDS_FUNCS, NATIVE_ARGS, PIPE_OP_FUNCS, bn_bck_in_func_op, bn_bck_sums_func_op, bn_fwd_func_op, bn_stats_func_op,
                             bnc_bck_in_func_op, bnc_bck_sums_func_op, bnc_fwd_func_op, bnc_stats_func_op, pipe_func_args)
from boda_amd.op import Dims, Nda, RtErr, UnsupErr, parse_op
from boda_amd.rtc import make_rtc

from test_bck_graph_cpu import run_in_order, topo_order


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


# ---- the functions against the numpy twin
@pytest.mark.parametrize("case", RC.CASES, ids=RC.case_id)
def test_cpu_functions_against_numpy(cpu, case):
    """Also the running pair after two calls (repeat=2: the second call starts from the first call's pair)."""
    shape, n, slab = case
    relu = (shape[0] + shape[1]) % 2
    r = RC.run_all_four(cpu, shape, n, slab, relu=relu, repeat=2)
    RC.check_against_numpy(r, shape, n, slab, relu=relu)
    if shape == (1, 1, 1, 1):   # N = 1: var = 0, the N == 1 branch, and one of the two chunks is empty
        i = R.make_inputs(shape)
        assert RC.chunks(1, 2) == [(0, 0), (0, 1)]
        assert r["mean"][0] == i["x"].reshape(-1)[0] and r["inv_std"][0] == R.F(1) / np.sqrt(R.F(R.EPS))
        assert R.same_bits(r["run_var2"], R.F(R.MAF) * i["run_var"] + (R.F(1) - R.F(R.MAF)) * R.F(0))
    if shape == (2, 4, 2, 2):
        assert RC.chunks(2, 3)[0] == (0, 0)     # chunk 0 is the empty one
    if shape[1] > 1:
        assert np.all(np.isfinite(r["inv_std"]))


def test_the_chunked_order_is_another_order(cpu):
    """On uniform(-2, 2) data of shape (3, 5, 3, 3) the sums of chunks=1 and chunks=2 differ in bits for many channels: the chunked chain is not the plain one by accident."""
    shape = (3, 5, 3, 3)
    differ = 0
    for seed in range(5):
        rng = np.random.default_rng(seed)
        i = R.make_inputs(shape)
        i["x"] = rng.uniform(-2, 2, shape).astype(R.F); i["dy"] = rng.uniform(-2, 2, shape).astype(R.F)
        a = RC.run_all_four(cpu, shape, 1, inputs=i); b = RC.run_all_four(cpu, shape, 2, inputs=i)
        differ += sum(int(x != y) for k in ("sg", "bg") for x, y in zip(a[k].view(np.uint32), b[k].view(np.uint32)))
    assert differ > 0


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_one_chunk_is_the_twin_function(cpu, case):
    shape, slab = case
    relu = (shape[0] + shape[1]) % 2
    a = RC.run_all_four(cpu, shape, 1, slab, relu=relu)
    b = R.run_all_five(cpu, shape, slab, relu=relu)
    for k in ("mean", "inv_std", "run_mean2", "run_var2", "out", "sg", "bg", "dx"):
        assert R.same_bits(a[k], b[k]), k


def big_term_sums(rtc):
    """-> {chunks: bias_grad_loss[0]} on the 2^24 case."""
    x, dy = RC.big_term_inputs()
    d = R.dims_of(x.shape)
    out = {}
    for n in (1, 2):
        st = R.run_func(rtc, bnc_stats_func_op(d, R.EPS, R.MAF, n), {"in": x, "run_mean": np.zeros(1, R.F), "run_var": np.ones(1, R.F)})[0]
        s = R.run_func(rtc, bnc_bck_sums_func_op(d, n), {"in": x, "mean": st["mean"], "inv_std": st["inv_std"], "out_grad_loss": dy})[0]
        out[n] = float(s["bias_grad_loss"][0])
    return out


def test_cpu_big_term_case(cpu):
    """[2^24, 1, 1 | 1, 1, 1]: one chunk gives 2^24 + 2 = 16777218, two chunks 2^24 + 3, which rounds to 16777220 (bnc_ref.big_term_inputs)."""
    assert big_term_sums(cpu) == {1: 16777218.0, 2: 16777220.0}


def test_cpu_in_place_forms(cpu):
    for shape, n in (((3, 2, 7, 7), 2), ((5, 65, 4, 4), 3)):
        d = R.dims_of(shape)
        r = RC.run_all_four(cpu, shape, n)
        common = {"in": r["x"], "mean": r["mean"], "inv_std": r["inv_std"]}
        out = R.run_func(cpu, bnc_fwd_func_op(d, 1), dict(common, scale=r["scale"], bias=r["bias"]), bind={"out": "in"})[0]["out"]
        assert R.same_bits(out, r["out"])
        dx = R.run_func(cpu, bnc_bck_in_func_op(d), dict(common, scale=r["scale"], scale_grad_loss=r["sg"], bias_grad_loss=r["bg"], out_grad_loss=r["dy"]),
                        bind={"in_grad_loss": "out_grad_loss"})[0]["in_grad_loss"]
        assert R.same_bits(dx, r["dx"])


@pytest.mark.parametrize("case", [c for c in RC.CASES if c[0][0] * c[0][2] * c[0][3] >= 8], ids=RC.case_id)
def test_cpu_float64_bounds(cpu, case):
    """bn_ref.f64_bounds_fractions: the per-element bounds of out and dx with the backend's own fp32 statistics and sums, and the sums' bound, which holds for any order."""
    shape, n, slab = case
    r = RC.run_all_four(cpu, shape, n, slab, relu=0)
    fr = R.f64_bounds_fractions(r, shape, relu=0)
    print(RC.case_id(case), {k: round(v, 4) for k, v in fr.items()})
    for k, v in fr.items():
        assert v <= 1.0, (k, v)


# ---- tables, arg lists, plans
def ctor_ops(d):
    return [bnc_stats_func_op(d, 1e-5, 0.999, 2), bnc_stats_func_op(d, 1e-5, 0.9, 64, 8), bnc_fwd_func_op(d, 0), bnc_fwd_func_op(d, 1), bnc_bck_sums_func_op(d, 3), bnc_bck_sums_func_op(d, 1, 8),
            bnc_bck_in_func_op(d)]


def test_tables_arg_lists_and_plans():
    assert BNC_OP_FUNCS == {"BncStats": ("hip_bnc_stats",), "BncFwd": ("hip_bnc_fwd",), "BncBckSums": ("hip_bnc_bck_sums",), "BncBckIn": ("hip_bnc_bck_in",)}
    assert not set(BNC_OP_FUNCS) & (set(BN_OP_FUNCS) | set(PIPE_OP_FUNCS))
    table = rtc_mod.native_funcs()
    twin = {"hip_bnc_stats": "hip_bn_stats", "hip_bnc_fwd": "hip_bn_fwd", "hip_bnc_bck_sums": "hip_bn_bck_sums", "hip_bnc_bck_in": "hip_bn_bck_in"}
    for t, (fn,) in BNC_OP_FUNCS.items():
        row = table[fn]
        assert row["family"] == "bnc" and row["types"] == (t,) and row["flags"] == () and row["opt"] == () and row["be"] == ("hip", "cpu")
        assert row["multi_dev"] not in ("needs_flag", "refused", "replicated_only") and row["why"] == ""
        assert NATIVE_ARGS[fn] == NATIVE_ARGS[twin[fn]] and row["member"] == table[twin[fn]]["member"]
        assert fn not in IMG_SHARDS_FUNCS
    d = R.dims_of((2, 3, 4, 4))
    for f in ctor_ops(d):
        assert rtc_mod.func_args(f) == pipe_func_args(f) == NATIVE_ARGS[f.get_func_name()]
        assert parse_op(f.to_str()).to_str() == f.to_str() and rtc_mod.parse_op_native(f.to_str()) == f.to_str()
        assert rtc_mod.prebuild(f) > 0      # cross-compiles for gfx950
    fs = bnc_stats_func_op(d, 1e-5, 0.999, 2)
    assert fs.get_func_name() == "hip_bnc_stats" and fs.get_type() == "BncStats" and fs.get_u32("chunks") == 2 and fs.get_u32("slab") == 0 and fs.get_f32("maf") == float(np.float32(0.999))
    assert fs.get_dims("in") == d and fs.get_dims("mean") == Dims(("chan",), (3,), "float")
    assert rtc_mod.explain_plan(fs) == ("bodahip_bn_sum -DMODE=0 | bodahip_bn_fin grid=1 block=256 -DFIN=4 | bodahip_bn_fin grid=1 block=256 -DFIN=3 -DXCH=1 | bodahip_bn_sum -DMODE=3 | "
                                        "bodahip_bn_fin grid=1 block=256 -DFIN=1 -DXCH=1 | chunks=2 | chunk 0: imgs=1 slab=4096 slabs=1 | chunk 1: imgs=1 slab=4096 slabs=1")
    assert rtc_mod.explain_plan(bnc_bck_sums_func_op(d, 3, 8)) == ("bodahip_bn_sum -DMODE=2 | bodahip_bn_fin grid=1 block=256 -DFIN=2 | bodahip_bn_fin grid=1 block=256 -DFIN=2 -DXCH=1 | chunks=3 | "
                                                                  "chunk 0: empty | chunk 1: imgs=1 slab=8 slabs=2 | chunk 2: imgs=1 slab=8 slabs=2")
    # one chunk: the twin's launches, then the chunk's plan
    assert rtc_mod.explain_plan(bnc_bck_sums_func_op(d, 1, 8)) == "bodahip_bn_sum grid=12 block=256 -DMODE=2 | bodahip_bn_fin grid=1 block=256 -DFIN=2 | chunks=1 | chunk 0: imgs=2 slab=8 slabs=4"
    assert rtc_mod.explain_plan(bnc_fwd_func_op(d, 1)) == "bodahip_bn_fwd -DRELU=1" and rtc_mod.explain_plan(bnc_bck_in_func_op(d)) == "bodahip_bn_bck_in"


# ---- refusals
def test_refusals_of_the_op(cpu):
    d = R.dims_of((2, 3, 4, 4))
    u32 = lambda v: Nda(None, "uint32_t", (v,))
    other = Nda(dims=R.dims_of((2, 3, 4, 5)), tn="float")
    for n in (0, 65):
        with pytest.raises(UnsupErr, match=f"chunks={n}: 1 to 64 img chunks"):
            bnc_stats_func_op(d, 1e-5, 0.9, n)
        with pytest.raises(UnsupErr, match=f"chunks={n}: 1 to 64 img chunks"):
            bnc_bck_sums_func_op(d, n)
    with pytest.raises(RtErr, match="multiple of 4"):
        bnc_stats_func_op(d, 1e-5, 0.9, 2, 6)
    with pytest.raises(RtErr, match="img:chan:y:x"):
        bnc_fwd_func_op(Dims.make("float", img=2, chan=3, x=4), 0)
    half = Nda(dims=Dims(d.names, d.sizes, "half"), tn="half")
    cases = [
        (T.bad_op(bnc_stats_func_op(d, 1e-5, 0.9, 2), chunks=u32(0)), UnsupErr, "hip_bnc_stats: chunks=0: 1 to 64 img chunks"),
        (T.bad_op(bnc_bck_sums_func_op(d, 2), chunks=u32(65)), UnsupErr, "hip_bnc_bck_sums: chunks=65: 1 to 64 img chunks"),
        (T.bad_op(bnc_stats_func_op(d, 1e-5, 0.9, 2), chunks=None), RtErr, "no 'chunks'"),
        (T.bad_op(bnc_fwd_func_op(d, 0), out=other), RtErr, "out dims .* differ from in's"),
        (T.bad_op(bnc_bck_in_func_op(d), in_grad_loss=half), RtErr, "differ from in's"),
        (T.bad_op(bnc_stats_func_op(d, 1e-5, 0.9, 2), **{"in": half}), RtErr, "fp32 only"),
        (T.bad_op(bnc_stats_func_op(d, 1e-5, 0.9, 2), mean=Nda(dims=Dims(("chan",), (4,), "float"), tn="float")), RtErr, "mean dims .*one float per channel"),
        (T.bad_op(bnc_bck_sums_func_op(d, 2), bias_grad_loss=Nda(dims=Dims(("v",), (3,), "float"), tn="float")), RtErr, "bias_grad_loss dims .*one float per channel"),
        (T.bad_op(bnc_stats_func_op(d, 1e-5, 0.9, 2), slab=u32(6)), RtErr, "slab=6: a forced slab length is a multiple of 4"),
        (T.bad_op(bnc_stats_func_op(d, 1e-5, 0.9, 2), maf=None), RtErr, "no 'maf'"),
        (T.bad_op(bnc_fwd_func_op(d, 0), relu=u32(2)), RtErr, "relu must be 0 . 1"),
    ]
    for fl in ("img_shards", "seed_from_var", "zero_if_in_non_pos"):
        for f in (bnc_stats_func_op(d, 1e-5, 0.9, 2), bnc_fwd_func_op(d, 0), bnc_bck_sums_func_op(d, 2), bnc_bck_in_func_op(d)):
            cases.append((T.bad_op(f, **{fl: u32(1)}), RtErr, f"{fl}=1 on '{f.get_func_name()}'"))
    for f, err, msg in cases:
        with pytest.raises(err, match=msg):
            T.compile_only(cpu, f)
        if "=1 on " not in msg or "zero_if_in_non_pos" not in msg:
            with pytest.raises(err, match=msg):
                rtc_mod.explain_plan(f)
    wrong_type = bnc_fwd_func_op(d, 0); wrong_type.str_vals["type"] = "BnFwd"
    with pytest.raises(RtErr, match="a function of op type BncFwd, not BnFwd"):
        T.compile_only(cpu, wrong_type)
    # a forced slab is applied to every chunk's plan: 4 cuts a chunk of 6 images x 57 x 57 into more than 4096 slabs
    with pytest.raises(UnsupErr, match="slab=4 cuts a channel of 19494 elements"):
        T.compile_only(cpu, bnc_stats_func_op(R.dims_of((12, 3, 57, 57)), 1e-5, 0.9, 2, 4))
    big = Dims.make("float", img=8, chan=1024, y=256, x=256)     # 2 GiB exactly
    for f in (lambda: bnc_stats_func_op(big, 1e-5, 0.9, 2), lambda: bnc_fwd_func_op(big, 0), lambda: bnc_bck_sums_func_op(big, 2), lambda: bnc_bck_in_func_op(big)):
        with pytest.raises(UnsupErr, match="2 GiB"):
            T.compile_only(cpu, f())


def var_refusals(rtc):
    d = R.dims_of((2, 3, 4, 4))
    with pytest.raises(RtErr, match="args 'mean' and 'inv_std' are the same var"):
        T.run_bound(rtc, bnc_stats_func_op(d, 1e-5, 0.9, 2), {"inv_std": "rv_mean"})
    with pytest.raises(RtErr, match="args 'run_mean' and 'run_var' are the same var"):
        T.run_bound(rtc, bnc_stats_func_op(d, 1e-5, 0.9, 2), {"run_var": "rv_run_mean"})
    with pytest.raises(RtErr, match="args 'scale_grad_loss' and 'bias_grad_loss' are the same var"):
        T.run_bound(rtc, bnc_bck_sums_func_op(d, 2), {"bias_grad_loss": "rv_scale_grad_loss"})
    with pytest.raises(RtErr, match="args 'in' and 'in_grad_loss' are the same var"):
        T.run_bound(rtc, bnc_bck_in_func_op(d), {"in_grad_loss": "rv_in"})
    with pytest.raises(RtErr, match="arg 'scale' has dims .*chan=4.*the op says"):
        T.run_bound(rtc, bnc_fwd_func_op(d, 0), {"scale": "short"}, {"short": Dims(("chan",), (4,), "float")})
    with pytest.raises(RtErr, match="arg 'out' has dims .*the op says"):
        T.run_bound(rtc, bnc_fwd_func_op(d, 0), {"out": "other"}, {"other": R.dims_of((2, 3, 4, 5))})
    with pytest.raises(RtErr, match="arg 'out' has 2 images, another arg 1"):                  # the image count is free, but must agree between the vars
        T.run_bound(rtc, bnc_fwd_func_op(d, 0), {"in": "shard"}, {"shard": R.dims_of((1, 3, 4, 4))})
    with pytest.raises(RtErr, match="hold 1 images, the op says 2"):                           # a whole summing call needs the whole batch
        T.run_bound(rtc, bnc_stats_func_op(d, 1e-5, 0.9, 2), {"in": "shard"}, {"shard": R.dims_of((1, 3, 4, 4))})
    with pytest.raises(RtErr, match="has type uint32_t: fp32 only"):
        T.run_bound(rtc, bnc_stats_func_op(d, 1e-5, 0.9, 2), {"mean": "words"}, {"words": Dims(("chan",), (3,), "uint32_t")})
    T.run_bound(rtc, bnc_fwd_func_op(d, 1), {"out": "rv_in"})                                   # the two allowed in-place forms
    T.run_bound(rtc, bnc_bck_in_func_op(d), {"in_grad_loss": "rv_out_grad_loss"})
    sh = R.dims_of((1, 3, 4, 4))                                                                 # fewer images than the op in every tensor var: an img shard
    T.run_bound(rtc, bnc_fwd_func_op(d, 1), {"in": "s_in", "out": "s_out"}, {"s_in": sh, "s_out": sh})


def test_cpu_refusals_of_the_call(cpu):
    var_refusals(cpu)


def test_fwd_and_bck_in_on_fewer_images_divide_by_the_whole_batch(cpu):
    """hip_bnc_bck_in on the first image alone, with the op's dims those of the whole batch, writes that image's rows of the whole call."""
    shape = (3, 5, 3, 3)
    d = R.dims_of(shape)
    r = RC.run_all_four(cpu, shape, 2)
    f = bnc_bck_in_func_op(d)
    part = d.__class__(d.names, (1,) + tuple(d.sizes[1:]), "float")
    ins = {"in": r["x"][:1], "out_grad_loss": r["dy"][:1], "mean": r["mean"], "inv_std": r["inv_std"], "scale": r["scale"], "scale_grad_loss": r["sg"], "bias_grad_loss": r["bg"]}
    spec = pipe_func_args(f)
    from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo
    cpu.compile([RtcFuncInfo("bnc_part", "", [a for a, _ in spec], f)])
    made = []
    try:
        for an, io in spec:
            dd = part if f.get_dims(an) == d else f.get_dims(an)
            cpu.create_var_with_dims("pv_" + an, dd); made.append("pv_" + an)
            cpu.copy_nda_to_var("pv_" + an, np.ascontiguousarray(ins[an], R.F).reshape(dd.sizes) if an in ins else np.full(dd.sizes, np.nan, R.F))
        cpu.run(RtcFuncCall("bnc_part", {an: RtcArg.var("pv_" + an) for an, _ in spec}))
        assert R.same_bits(cpu.copy_var_to_nda("pv_in_grad_loss"), r["dx"][:1])
    finally:
        for vn in made:
            cpu.release_var(vn)
        cpu.release_func("bnc_part"); cpu.release_per_call_id_data()


# ---- the driver on be=cpu
def test_cpu_driver_one_chunk_leaves_the_default_bits(cpu):
    seed = R.RES_SEEDS[0]
    drv, bp, *_, plain = T.res_step(cpu, seed)
    names = [(c.tag, c.fop.get_func_name()) for c in drv.bck_calls]
    drv.release()
    drv, bp, *_, one = T.res_step(cpu, seed, img_chunks=1)
    try:
        fns = [f.get_func_name() for _, f, _ in drv.calls()]
        assert (fns.count("hip_bnc_stats"), fns.count("hip_bnc_fwd"), fns.count("hip_bnc_bck_sums"), fns.count("hip_bnc_bck_in"), fns.count("hip_split")) == (8, 8, 8, 8, 4)
        assert not any(f.startswith("hip_bn_") or f == "hip_fan_out" for f in fns)
        # the same tags in the same order; a BckEltwise is one hip_split per output where it was one hip_fan_out
        twin = {"hip_bnc_stats": "hip_bn_stats", "hip_bnc_fwd": "hip_bn_fwd", "hip_bnc_bck_sums": "hip_bn_bck_sums", "hip_bnc_bck_in": "hip_bn_bck_in"}
        got = [(c.tag, twin.get(c.fop.get_func_name(), c.fop.get_func_name())) for c in drv.bck_calls]
        want = [x for t, f in names for x in ([(t, "hip_split")] * 2 if f == "hip_fan_out" else [(t, f)])]
        assert got == want
        for _, f, am in drv.calls():
            if f.get_func_name() == "hip_split":
                assert f.get_u32("icix") == 0 and f.get_dims("in") == f.get_dims("out")
            if f.get_func_name() in ("hip_bnc_stats", "hip_bnc_bck_sums"):
                assert f.get_u32("chunks") == 1
        assert set(one) == set(plain)
        for n in plain:
            assert R.same_bits(plain[n], one[n]), n
    finally:
        drv.release()


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("seed", R.RES_SEEDS)
def test_cpu_driver_against_float64(cpu, seed, n):
    drv, bp, params, data, label, fwd = T.res_step(cpu, seed, img_chunks=n)
    try:
        assert all(f.get_u32("chunks") == n for _, f, _ in drv.calls() if f.get_func_name() in ("hip_bnc_stats", "hip_bnc_bck_sums"))
        worst = T.check_against_f64(bp, params, data, label, fwd, "be=cpu", T.CAP)
        print(f"be=cpu residual seed {seed} img_chunks={n}: largest max|got - want| / max|want| = {worst:.3e}")
    finally:
        drv.release()


def test_cpu_driver_composes_with_the_other_options(cpu):
    seed = R.RES_SEEDS[0]
    drv, bp, *_, plain = T.res_step(cpu, seed, img_chunks=2)
    drv.release()
    drv, bp, *_, fused = T.res_step(cpu, seed, img_chunks=2, fuse_relu_grad=True, seed_in_var=True)
    try:
        assert drv.fused_relu_grads["folded"]
        for n in plain:
            assert R.same_bits(plain[n], fused[n]), n
    finally:
        drv.release()
    drv, bp, *_, fb = T.res_step(cpu, seed, img_chunks=2, fuse_filts_biases=True)      # (on be=cpu the fused gradient holds the pair's bits)
    try:
        for n in plain:
            assert R.same_bits(plain[n], fb[n]), n
    finally:
        drv.release()


def test_driver_refuses_a_bad_img_chunks(cpu):
    for bad in (-1, 65, 2.0, True):
        with pytest.raises(RtErr, match="img_chunks must be an int"):
            ConvPipeBck(cpu, img_chunks=bad)


def solver_steps(rtc, n, steps=3, **kw):
    """Three steps of the residual pipe with a solver and img_chunks=n -> [{param or history or loss: array}] after each step."""
    solver = SgdSolver(lr=0.05, momentum=0.9, weight_decay=5e-4, lr_mult={"biases": 2.0, "scale": 0.5}, decay_mult={"biases": 0.0, "bias": 0.0, "scale": 0.0})
    cp = R.residual(kw.pop("B", 3)); bp = add_bck_ops(cp)
    drv = ConvPipeBck(rtc, solver=solver, bn_maf=0.9, img_chunks=n, **kw); drv.init(bp, R.res_params(cp, 1))
    try:
        sv = list(cp.params) + [p + SGD_HIST_SFX for p in drv.sgd_params]
        states = []
        for k in range(steps):
            if k == 1:
                drv.set_sgd_hyper(lr=0.02)
            data, label = R.res_inputs(cp, 100 + k)
            fwd = {"data": data, "label": label}
            drv.run_bck(["data", "label"], fwd, ["loss"])
            states.append(dict({v: rtc.copy_var_to_nda(v) for v in sv}, loss=fwd["loss"]))
        return states, drv
    finally:
        drv.release()


def test_cpu_solver_three_steps(cpu):
    states, _ = solver_steps(cpu, 2)
    assert all(np.isfinite(s["loss"]).all() for s in states)
    for a, b in zip(states, states[1:]):
        assert not R.same_bits(a["scale_stem_scale"], b["scale_stem_scale"]) and not R.same_bits(a["bn_stem_mean"], b["bn_stem_mean"])
    one, _ = solver_steps(cpu, 1)
    assert any(not R.same_bits(one[-1][k], states[-1][k]) for k in one[-1])      # (another order of the sums: other bits after three steps)


def test_cpu_call_list_in_other_topological_orders(cpu):
    """_call_deps covers the hip_bnc_* args and the hip_split copies: the call list run in two other topological orders on poisoned vars leaves the bits of the list order."""
    cp = R.residual(); bp = add_bck_ops(cp)
    params = R.res_params(cp, 1); data, label = R.res_inputs(cp, 1)
    drv = ConvPipeBck(cpu, solver=SgdSolver(lr=0.05), bn_maf=0.9, img_chunks=2); drv.init(bp, params)
    try:
        keep = set(cp.params) | {p + SGD_HIST_SFX for p in drv.sgd_params} | {"data", "label", "sgd_hyper"}

        def run(order):
            for n, a in params.items():
                cpu.copy_nda_to_var(n, a)
            drv.zero_sgd_history()
            cpu.copy_nda_to_var("data", data); cpu.copy_nda_to_var("label", label)
            return run_in_order(cpu, drv, order, keep)
        deps = drv._call_deps()
        n = len(deps)
        ix = {}
        for i, c in enumerate(drv.bck_calls):
            ix.setdefault((c.tag, c.fop.get_func_name()), i)
        assert ix[("stem", "hip_conv")] in deps[ix[("bn_stem", "hip_bnc_stats")]] and ix[("bn_stem", "hip_bnc_stats")] in deps[ix[("scale_stem", "hip_bnc_fwd")]]
        assert ix[("scale_stem_bck", "hip_bnc_bck_sums")] in deps[ix[("bn_stem_bck", "hip_bnc_bck_in")]]
        assert ix[("res_b_relu_bck", "hip_zero_if_non_pos")] in deps[ix[("res_b_bck", "hip_split")]]
        want = run(range(n))
        rng = np.random.default_rng(17)
        for what, order in {"latest ready first": topo_order(deps, max), "random topological": topo_order(deps, lambda r: r[int(rng.integers(len(r)))])}.items():
            assert sorted(order) == list(range(n)) and order != list(range(n)), what
            got = run(order)
            for vn in drv.vars:
                assert got[vn].tobytes() == want[vn].tobytes(), (what, vn)
        victim = ix[("bn_stem_bck", "hip_bnc_bck_in")]      # and the check can fail: the data gradient ahead of its two sums
        loose = [([] if i == victim else d) for i, d in enumerate(deps)]
        got = run(topo_order(loose, max))
        assert any(got[vn].tobytes() != want[vn].tobytes() for vn in drv.vars)
    finally:
        drv.release()
