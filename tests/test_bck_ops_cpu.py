"""The non-conv ops of the gradient pipe without a GPU: the op types and their validation, add_bck_op_annotations, the native planner's plans, and be=cpu's loops --
the reference templates' own order (test/rtc/pool.cucl, spreading.cucl, lrn.cucl, bck_lrn.cucl, ZeroIfNonPos.cucl, softmax.cucl, sm_grad_and_loss.cucl,
sum_loss_over_imgs.cucl) -- held BIT FOR BIT to the numpy restatement of the semantics in tests/bck_ops_ref.py.  be=cpu is the checker of the HIP kernels
(tests/test_gpu_bck_ops.py); this file checks the checker.  The shapes are the ones the GPU file uses."""
import numpy as np
import pytest
import torch

import bck_ops_ref as ref
from boda_amd import rtc as rtc_mod
from boda_amd.cnn_op import NATIVE_ARGS, OpTune, add_bck_op_annotations, add_codegen_annotations
from boda_amd.op import OP_INFO, RtErr, UnsupErr, parse_op
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc
from oracle import boda_oracle as oracle


# ---- op builders
def _t(B, C, H, W):
    return f"(dims=(img={B},chan={C},y={H},x={W}))"


def _yx(y, x):
    return f"(tn=none,dims=(y={y},x={x}))"


def pool_out(H, W, kern, stride, pad):
    if H + 2 * pad[0] < kern[0] or W + 2 * pad[1] < kern[1]:   # either padded dim below the window: 1 x 1
        return 1, 1
    return ref.pool_out_sz(H, kern[0], stride[0], pad[0]), ref.pool_out_sz(W, kern[1], stride[1], pad[1])


def pool_op(B, C, H, W, kern, stride, pad, avg=0, emit=1, out_hw=None, typ="Pooling"):
    OH, OW = out_hw or pool_out(H, W, kern, stride, pad)
    extra = f"in_grad_loss={_t(B, C, H, W)},out_grad_loss={_t(B, C, OH, OW)}," if typ == "Spreading" else ""
    return parse_op(f"(str_vals=(type={typ}),nda_vals=(avg_pool=(tn=uint32_t,v={avg}),emit_out_in_yx=(tn=uint32_t,v={emit}),in={_t(B, C, H, W)},{extra}"
                    f"in_pad={_yx(*pad)},kern_sz={_yx(*kern)},out={_t(B, C, OH, OW)},stride={_yx(*stride)}))")


def spreading_op(B, C, H, W, kern, stride, pad, avg=0, **kw):
    return pool_op(B, C, H, W, kern, stride, pad, avg=avg, emit=0 if avg else 1, typ="Spreading", **kw)


def lrn_op(B, C, H, W, ls, alpha=1e-4, beta=0.75, k=1.0, emit=1, typ="LRN"):
    d = _t(B, C, H, W)
    extra = f"in_grad_loss={d},out_grad_loss={d}," if typ == "BckLRN" else ""
    return parse_op(f"(str_vals=(type={typ}),nda_vals=(alpha=(tn=float,v={alpha!r}),beta=(tn=float,v={beta!r}),emit_out_scale_base=(tn=uint32_t,v={emit}),in={d},{extra}"
                    f"k=(tn=float,v={k!r}),local_size=(tn=uint32_t,v={ls}),out={d}))")


def bck_lrn_op(*a, **kw):
    return lrn_op(*a, typ="BckLRN", **kw)


def zinp_op(dims):
    d = "(dims=(" + ",".join(f"{n}={s}" for n, s in dims) + "))"
    return parse_op(f"(str_vals=(type=ZeroIfNonPos),nda_vals=(cond={d},in={d},out={d}))")


def softmax_op(B, C, y=1, x=1):
    return parse_op(f"(str_vals=(type=SoftmaxWithLoss),nda_vals=(in={_t(B, C, y, x)},in_grad_loss={_t(B, C, y, x)},label=(dims=(img={B},y={y},x={x})),loss=(dims=(y={y},x={x}))))")


def run_all(rtc, fop, ins):
    """Run one annotated function on `rtc` with host inputs (every IN arg from `ins`) -> {OUT arg: array}."""
    fn = fop.get_func_name()
    rtc.compile([RtcFuncInfo("f", "", [a for a, _ in NATIVE_ARGS[fn]], fop)])
    am, made = {}, []
    try:
        for an, io in NATIVE_ARGS[fn]:
            if io == "REF":
                am[an] = RtcArg.ref(fop.get_dims(an)); continue
            rtc.create_var_with_dims(an, fop.get_dims(an)); made.append(an); am[an] = RtcArg.var(an)
            if io == "IN":
                rtc.copy_nda_to_var(an, np.ascontiguousarray(ins[an], dtype=np.float32))
        rtc.run(RtcFuncCall("f", am))
        rtc.finish_and_sync()
        return {a: rtc.copy_var_to_nda(a) for a, io in NATIVE_ARGS[fn] if io == "OUT"}
    finally:
        for vn in made:
            rtc.release_var(vn)
        rtc.release_func("f"); rtc.release_per_call_id_data()


def bits_eq(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- shapes (the smallest at which each kernel can go wrong).  Pooling / Spreading: (B, C, H, W, kern, stride, pad)
POOL = {
    "overlap_7x7_k3s2": (2, 5, 7, 7, (3, 3), (2, 2), (0, 0)),
    "disjoint_6x6_k2s2": (2, 5, 6, 6, (2, 2), (2, 2), (0, 0)),
    "gaps_9x9_k2s3": (2, 5, 9, 9, (2, 2), (3, 3), (0, 0)),          # stride > kernel: some inputs receive nothing and must be exactly +0
    "pad_8x8_k3s2p1": (3, 4, 8, 8, (3, 3), (2, 2), (1, 1)),
    "nonsquare_13x11": (2, 3, 13, 11, (3, 2), (2, 1), (1, 0)),
    "global_6x6": (3, 8, 6, 6, (6, 6), (1, 1), (0, 0)),
    "alexnet_55x55_c96": (2, 96, 55, 55, (3, 3), (2, 2), (0, 0)),   # more pels than one workgroup
}
LRN = {   # (B, C, H, W, local_size, k)
    "c3_ls5": (2, 3, 3, 3, 5, 1.0),          # fewer channels than the window
    "c7_ls5": (2, 7, 3, 3, 5, 2.0),
    "c96_ls5_5x5": (2, 96, 5, 5, 5, 1.0),    # several channel blocks
    "c100_ls5_5x5": (2, 100, 5, 5, 5, 1.0),  # ... plus a ragged one (blocks of 8 channels)
    "c8_ls3": (3, 8, 4, 4, 3, 2.0),
    "c5_ls1": (2, 5, 3, 3, 1, 1.0),          # the window is the channel itself
    "c8_ls5_1x1": (3, 8, 1, 1, 5, 1.0),
    "c16_ls5_13x13": (3, 16, 13, 13, 5, 2.0),
}
SOFTMAX = [(B, C) for C in (1, 5, 64, 65, 1000) for B in (1, 3)]
ZINP = [1, 3, 257, 4096]
ALPHA, BETA = 1e-4, 0.75


def pool_in(name, seed=0):
    B, C, H, W = POOL[name][:4]
    return np.random.default_rng(seed).uniform(-4, 4, (B, C, H, W)).astype(np.float32)


def labels(B, C, seed=0):
    """0, chan-1 and a middle value, then random ones."""
    l = [0, C - 1, C // 2] + list(np.random.default_rng(seed).integers(0, C, B))
    return np.array(l[:B], np.float32).reshape(B, 1, 1)


def zinp_data(n, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-3, 3, n).astype(np.float32)
    cond = rng.uniform(-1, 1, n).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754944e-38, np.nan], np.float32)   # exact +0 / -0, the smallest positive values, a NaN
    cond[:min(n, special.size)] = special[:min(n, special.size)]
    if n > 8:
        cond[rng.integers(0, n, n // 5)] = 0.0
        cond[rng.integers(0, n, n // 5)] = -0.0
    return x, cond


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


# ---- the op layer
def test_tables():
    pool_p = ("kern_sz", "stride", "in_pad", "avg_pool", "emit_out_in_yx")
    lrn_p = ("alpha", "beta", "k", "local_size", "emit_out_scale_base")
    assert OP_INFO["Pooling"] == (("in",), ("out",), pool_p)
    assert OP_INFO["LRN"] == (("in",), ("out",), lrn_p)
    assert OP_INFO["Spreading"] == (("out", "out_grad_loss", "in"), ("in_grad_loss",), pool_p)
    assert OP_INFO["BckLRN"] == (("in", "out", "out_grad_loss"), ("in_grad_loss",), lrn_p)
    assert OP_INFO["ZeroIfNonPos"] == (("in", "cond"), ("out",), ())
    assert OP_INFO["SoftmaxWithLoss"] == (("in", "label"), ("in_grad_loss", "loss"), ())
    I, O, R = "IN", "OUT", "REF"
    assert NATIVE_ARGS["hip_pool_yx"] == (("in", I), ("kern_sz", R), ("stride", R), ("in_pad", R), ("out", O), ("out_in_yx", O))
    assert NATIVE_ARGS["hip_lrn_sb"] == (("in", I), ("out", O), ("out_scale_base", O))
    assert NATIVE_ARGS["hip_spreading"] == (("out", I), ("out_grad_loss", I), ("out_in_yx", I), ("kern_sz", R), ("stride", R), ("in_pad", R), ("in_grad_loss", O))
    assert NATIVE_ARGS["hip_bck_lrn"] == (("in", I), ("out", I), ("out_grad_loss", I), ("out_scale_base", I), ("in_grad_loss", O))
    assert NATIVE_ARGS["hip_zero_if_non_pos"] == (("in", I), ("cond", I), ("out", O))
    assert NATIVE_ARGS["hip_softmax"] == (("in", I), ("prob", O))
    assert NATIVE_ARGS["hip_sm_grad_and_loss"] == (("prob", I), ("label", I), ("in_grad_loss", O), ("loss_per_pel", O))
    assert NATIVE_ARGS["hip_sum_loss_over_imgs"] == (("loss_per_pel", I), ("loss", O))


def all_ops():
    g = POOL["pad_8x8_k3s2p1"]
    return [pool_op(*g), spreading_op(*g), spreading_op(*g, avg=1), lrn_op(2, 7, 3, 3, 5), bck_lrn_op(2, 7, 3, 3, 5, k=2.0), zinp_op((("img", 2), ("chan", 3), ("y", 4), ("x", 5))),
            zinp_op((("v", 257),)), softmax_op(3, 65)]


def test_parse_round_trip_flops_and_bytes():
    for op in all_ops():
        again = parse_op(op.to_str())
        assert again == op and again.to_str() == op.to_str()
        assert rtc_mod.parse_op_native(op.to_str())   # the backend's own parser takes the line too
        assert op.flops() == 0
        ins, outs, _ = OP_INFO[op.get_type()]
        assert op.algo_bytes() == sum(4 * op.get_dims(a).dims_prod() for a in ins + outs)
    assert lrn_op(2, 7, 3, 3, 5).get_f32("alpha") == 1e-4 and lrn_op(2, 7, 3, 3, 5).get_u32("local_size") == 5


def test_parse_refusals():
    g = POOL["pad_8x8_k3s2p1"]
    with pytest.raises(RtErr):   # 8x8, k3 s2 p1: the pooling rule gives 5x5 (a partial last window counts), the convolution rule's 4x4 is refused
        pool_op(*g, out_hw=(4, 4))
    with pytest.raises(RtErr):
        spreading_op(*g, out_hw=(5, 6))
    with pytest.raises(RtErr):   # in_grad_loss must have in's dims
        parse_op(spreading_op(*g).to_str().replace("in_grad_loss=(dims=(img=3,chan=4,", "in_grad_loss=(dims=(img=3,chan=5,"))
    with pytest.raises(UnsupErr):
        pool_op(*g, avg=1, emit=1)
    pool_op(*g, avg=1, emit=0)   # an average without the argmax parses
    with pytest.raises(UnsupErr):
        lrn_op(2, 8, 3, 3, 4)
    with pytest.raises(UnsupErr):
        bck_lrn_op(2, 8, 3, 3, 2)
    with pytest.raises(RtErr):   # equal dims everywhere
        parse_op(bck_lrn_op(2, 8, 3, 3, 5).to_str().replace("out_grad_loss=(dims=(img=2,chan=8,", "out_grad_loss=(dims=(img=2,chan=7,"))
    with pytest.raises(RtErr):
        parse_op(zinp_op((("v", 8),)).to_str().replace("cond=(dims=(v=8))", "cond=(dims=(v=9))"))
    with pytest.raises(UnsupErr):
        softmax_op(2, 10, y=2, x=2)
    with pytest.raises(UnsupErr):
        softmax_op(2, 10, y=1, x=3)
    with pytest.raises(RtErr):
        parse_op("(str_vals=(type=ZeroIfNonPos),nda_vals=(in=(dims=(v=8)),out=(dims=(v=8))))")   # cond is missing


def test_annotations_in_call_order():
    g = POOL["pad_8x8_k3s2p1"]
    names = lambda op: [f.get_func_name() for f in add_bck_op_annotations(op, OpTune())]
    assert names(spreading_op(*g)) == ["hip_spreading"]
    assert names(bck_lrn_op(2, 7, 3, 3, 5)) == ["hip_bck_lrn"]
    assert names(zinp_op((("v", 9),))) == ["hip_zero_if_non_pos"]
    assert names(softmax_op(3, 10)) == ["hip_softmax", "hip_sm_grad_and_loss", "hip_sum_loss_over_imgs"]
    assert names(pool_op(*g)) == ["hip_pool_yx"]
    assert names(lrn_op(2, 7, 3, 3, 5)) == ["hip_lrn_sb"]
    sm = add_bck_op_annotations(softmax_op(3, 10), OpTune())
    for f in sm:   # the intermediate vars keep the reference's names and dims
        assert f.get_dims("prob") == f.get_dims("in") and f.get_dims("loss_per_pel") == f.get_dims("label")
    assert add_bck_op_annotations(spreading_op(*g), OpTune())[0].get_dims("out_in_yx") == spreading_op(*g).get_dims("out")
    assert add_bck_op_annotations(lrn_op(2, 7, 3, 3, 5), OpTune())[0].get_dims("out_scale_base") == lrn_op(2, 7, 3, 3, 5).get_dims("out")
    for f in sm:   # every arg of every function has dims in the annotated op
        for an, _ in NATIVE_ARGS[f.get_func_name()]:
            f.get_dims(an)


def test_annotation_refusals():
    g = POOL["pad_8x8_k3s2p1"]
    with pytest.raises(UnsupErr, match="forward pipe"):
        add_bck_op_annotations(pool_op(*g, emit=0), OpTune())
    with pytest.raises(UnsupErr, match="forward pipe"):
        add_bck_op_annotations(lrn_op(2, 7, 3, 3, 5, emit=0), OpTune())
    for tune in (OpTune(hip_dtype="bf16"), OpTune(hip_layout="nhwc"), OpTune(hip_algo="winograd")):
        for op in all_ops():
            with pytest.raises(UnsupErr):
                add_bck_op_annotations(op, tune)
    with pytest.raises(RtErr):
        add_bck_op_annotations(parse_op("(str_vals=(type=sgemm),nda_vals=(a=(dims=(K=4,M=4)),b=(dims=(K=4,N=4)),c=(dims=(M=4,N=4))))"), OpTune())
    with pytest.raises(UnsupErr):   # unchanged: none of these is a forward hot-path op
        add_codegen_annotations(spreading_op(*g), OpTune())


def test_explain_plan_names_the_kernels():
    g = POOL["pad_8x8_k3s2p1"]
    want = {"Pooling": ["bodahip_pool_yx"], "Spreading": ["bodahip_spreading"], "LRN": ["bodahip_lrn_sb"], "BckLRN": ["bodahip_bck_lrn"],
            "ZeroIfNonPos": ["bodahip_zero_if_non_pos"], "SoftmaxWithLoss": ["bodahip_softmax", "bodahip_sm_grad_and_loss", "bodahip_sum_loss_over_imgs"]}
    for op in all_ops():
        plan = rtc_mod.explain_plan(op)
        assert [p.split()[0] for p in plan.split(" | ")] == want[op.get_type()], plan
        assert all("grid=" in p for p in plan.split(" | "))
        for f, k in zip(add_bck_op_annotations(op, OpTune()), want[op.get_type()]):
            assert rtc_mod.explain_plan(f).startswith(k + " grid=")
    assert "grid=2 " in rtc_mod.explain_plan(pool_op(*g))          # 3 x 4 x 5 x 5 = 300 outputs: two workgroups of 256
    assert "-DAVG=1" in rtc_mod.explain_plan(spreading_op(*g, avg=1)) and "-DKH=3" in rtc_mod.explain_plan(spreading_op(*g))
    assert "-DCB=8" in rtc_mod.explain_plan(bck_lrn_op(2, 100, 5, 5, 5))   # small planes: blocks of 8 channels, the last one ragged
    with pytest.raises(UnsupErr, match="2 GiB"):
        rtc_mod.explain_plan(zinp_op((("v", 1 << 29),)))
    with pytest.raises(UnsupErr, match="forward pipe"):
        rtc_mod.explain_plan(pool_op(*g, emit=0))


# ---- be=cpu bit for bit against the numpy restatement
@pytest.mark.parametrize("name", sorted(POOL))
def test_cpu_pool_yx_and_spreading(cpu, name):
    B, C, H, W, kern, stride, pad = POOL[name]
    x = pool_in(name)
    got = run_all(cpu, add_bck_op_annotations(pool_op(*POOL[name]), OpTune())[0], {"in": x})
    out, yx = ref.pool_yx_f32(x, kern, stride, pad)
    assert bits_eq(got["out"], out) and bits_eq(got["out_in_yx"], yx)
    assert bits_eq(got["out"], oracle.pool_fwd(x, kern, stride, pad))
    ogl = np.random.default_rng(1).uniform(-2, 2, out.shape).astype(np.float32)
    for avg in (0, 1):
        f = add_bck_op_annotations(spreading_op(*POOL[name], avg=avg), OpTune())[0]
        igl = run_all(cpu, f, {"out": out, "out_grad_loss": ogl, "out_in_yx": yx})["in_grad_loss"]
        assert bits_eq(igl, ref.spreading_f32(ogl, yx, (H, W), kern, stride, pad, avg)), (name, avg)
    if name == "gaps_9x9_k2s3":   # pels that no window holds are exactly +0
        assert bits_eq(igl[:, :, 2::3, :], np.zeros_like(igl[:, :, 2::3, :])) and bits_eq(igl[:, :, :, 2::3], np.zeros_like(igl[:, :, :, 2::3]))


def tie_input(seed=3):
    return np.random.default_rng(seed).integers(0, 3, (2, 4, 9, 9)).astype(np.float32)   # quantised to {0, 1, 2}: most windows have several maxima


def test_cpu_ties_take_the_first_tap_in_kx_ky_order(cpu):
    geom = (2, 4, 9, 9, (3, 3), (2, 2), (1, 1))
    x = tie_input()
    got = run_all(cpu, add_bck_op_annotations(pool_op(*geom), OpTune())[0], {"in": x})
    out, yx = ref.pool_yx_f32(x, *geom[4:])
    assert bits_eq(got["out"], out) and bits_eq(got["out_in_yx"], yx)
    # by hand: plane [[1, 2], [2, 0]] under one 2x2 window -- kx outer, ky inner visits (0,0) (1,0) (0,1) (1,1): the first 2 is at y=1, x=0 -> 1*2 + 0
    one = run_all(cpu, add_bck_op_annotations(pool_op(1, 1, 2, 2, (2, 2), (2, 2), (0, 0)), OpTune())[0], {"in": np.array([[[[1, 2], [2, 0]]]], np.float32)})
    assert one["out"].item() == 2.0 and one["out_in_yx"].item() == 2.0
    ogl = np.random.default_rng(4).uniform(-2, 2, out.shape).astype(np.float32)
    igl = run_all(cpu, add_bck_op_annotations(spreading_op(*geom), OpTune())[0], {"out": out, "out_grad_loss": ogl, "out_in_yx": yx})["in_grad_loss"]
    assert bits_eq(igl, ref.spreading_f32(ogl, yx, (9, 9), *geom[4:], 0))


def test_cpu_all_equal_negatives(cpu):
    geom = (2, 3, 7, 7, (3, 3), (2, 2), (1, 1))
    x = np.full((2, 3, 7, 7), -2.5, np.float32)
    got = run_all(cpu, add_bck_op_annotations(pool_op(*geom), OpTune())[0], {"in": x})
    out, yx = ref.pool_yx_f32(x, *geom[4:])
    assert bits_eq(got["out"], out) and bits_eq(got["out_in_yx"], yx)
    assert np.all(got["out"] == -2.5) and got["out_in_yx"][0, 0, 0, 0] == 0.0 and got["out_in_yx"][0, 0, 1, 1] == 1 * 7 + 1   # the first tap INSIDE the plane


def test_cpu_spreading_order_and_full_area_divisor(cpu):
    # 1x1 input under a 2x2 window, pad 1, stride 1: out is 2x2 and all four outputs hold the pel.  out_x outer, out_y inner rounds differently than y outer here
    f = np.float32
    ogl = np.array([[[[2.0 ** 24, 1.0], [-(2.0 ** 24), 0.0]]]], f)   # ogl[oy][ox]
    x_outer = f(f(f(f(0) + ogl[0, 0, 0, 0]) + ogl[0, 0, 1, 0]) + ogl[0, 0, 0, 1]) + ogl[0, 0, 1, 1]
    y_outer = f(f(f(f(0) + ogl[0, 0, 0, 0]) + ogl[0, 0, 0, 1]) + ogl[0, 0, 1, 0]) + ogl[0, 0, 1, 1]
    assert x_outer != y_outer
    geom = (1, 1, 1, 1, (2, 2), (1, 1), (1, 1))
    yx = np.zeros((1, 1, 2, 2), f)   # every window's maximum is the one pel
    sp = add_bck_op_annotations(spreading_op(*geom), OpTune())[0]
    assert run_all(cpu, sp, {"out": ogl, "out_grad_loss": ogl, "out_in_yx": yx})["in_grad_loss"].item() == x_outer
    # average on 8x8 k3 s2 p1: the corner pel lies in ONE window, clipped to 2x2 by the border -- the divisor is still 9
    g = POOL["pad_8x8_k3s2p1"]
    ogl = np.random.default_rng(5).uniform(1, 2, (3, 4, 5, 5)).astype(f)
    igl = run_all(cpu, add_bck_op_annotations(spreading_op(*g, avg=1), OpTune())[0], {"out": ogl, "out_grad_loss": ogl, "out_in_yx": ogl})["in_grad_loss"]
    assert bits_eq(igl[:, :, 0, 0], ogl[:, :, 0, 0] / f(9)) and not bits_eq(igl[:, :, 0, 0], ogl[:, :, 0, 0] / f(4))
    assert bits_eq(igl, ref.spreading_f32(ogl, None, (8, 8), *g[4:], 1))


@pytest.mark.parametrize("name", ["overlap_7x7_k3s2", "disjoint_6x6_k2s2", "pad_8x8_k3s2p1", "global_6x6"])
def test_cpu_spreading_against_torch_max_pool_backward(cpu, name):
    """An independent check where there are no ties (random floats): torch's max_pool2d backward, ceil_mode chosen to match the plane."""
    B, C, H, W, kern, stride, pad = POOL[name]
    x = pool_in(name, seed=7)
    out, yx = ref.pool_yx_f32(x, kern, stride, pad)
    ogl = np.random.default_rng(8).uniform(-2, 2, out.shape).astype(np.float32)
    igl = run_all(cpu, add_bck_op_annotations(spreading_op(*POOL[name]), OpTune())[0], {"out": out, "out_grad_loss": ogl, "out_in_yx": yx})["in_grad_loss"]
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    for ceil in (False, True):
        y = torch.nn.functional.max_pool2d(xt, kern, stride, pad, ceil_mode=ceil)
        if tuple(y.shape) == out.shape:
            break
    assert tuple(y.shape) == out.shape
    y.backward(torch.from_numpy(ogl.astype(np.float64)))
    want = xt.grad.numpy()
    assert np.max(np.abs(igl - want)) <= 1e-6 * np.max(np.abs(want))


def lrn_inputs(name, seed=0):
    B, C, H, W, ls, k = LRN[name]
    rng = np.random.default_rng(seed)
    return rng.uniform(-30, 30, (B, C, H, W)).astype(np.float32), rng.uniform(-2, 2, (B, C, H, W)).astype(np.float32)


@pytest.mark.parametrize("name", sorted(LRN))
def test_cpu_lrn_sb_and_bck_lrn(cpu, name):
    B, C, H, W, ls, k = LRN[name]
    x, ogl = lrn_inputs(name)
    got = run_all(cpu, add_bck_op_annotations(lrn_op(B, C, H, W, ls, ALPHA, BETA, k), OpTune())[0], {"in": x})
    out, sb = ref.lrn_sb_f32(x, ls, ALPHA, BETA, k)
    assert bits_eq(got["out_scale_base"], sb) and bits_eq(got["out"], out)
    assert bits_eq(got["out"], oracle.lrn_fwd(x, ls, ALPHA, BETA, k))
    igl = run_all(cpu, add_bck_op_annotations(bck_lrn_op(B, C, H, W, ls, ALPHA, BETA, k), OpTune())[0],
                  {"in": x, "out": out, "out_grad_loss": ogl, "out_scale_base": sb})["in_grad_loss"]
    assert bits_eq(igl, ref.bck_lrn_f32(x, out, ogl, sb, ls, ALPHA, BETA, k))
    want, S = ref.bck_lrn_f64(x, out, ogl, sb, ls, ALPHA, BETA, k)
    assert np.all(np.abs(igl - want) <= 2 * (ls + 8) * ref.U * S)


def test_cpu_bck_lrn_against_torch_autograd(cpu):
    """The formula itself: d/d in of sum(ogl * lrn(in)) by torch autograd in float64 (caffe's across-channel LRN)."""
    B, C, H, W, ls, k = 2, 7, 3, 3, 5, 2.0
    alpha = 0.05   # large enough that the delta-scale term matters
    rng = np.random.default_rng(11)
    x = rng.uniform(-3, 3, (B, C, H, W)).astype(np.float32); ogl = rng.uniform(-2, 2, x.shape).astype(np.float32)
    fwd = run_all(cpu, add_bck_op_annotations(lrn_op(B, C, H, W, ls, alpha, BETA, k), OpTune())[0], {"in": x})
    igl = run_all(cpu, add_bck_op_annotations(bck_lrn_op(B, C, H, W, ls, alpha, BETA, k), OpTune())[0],
                  {"in": x, "out": fwd["out"], "out_grad_loss": ogl, "out_scale_base": fwd["out_scale_base"]})["in_grad_loss"]
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    y = torch.nn.functional.local_response_norm(xt, ls, alpha=float(np.float32(alpha)), beta=BETA, k=k)
    y.backward(torch.from_numpy(ogl.astype(np.float64)))
    assert np.max(np.abs(igl - xt.grad.numpy())) < 1e-5 * np.max(np.abs(xt.grad.numpy()))


@pytest.mark.parametrize("n", ZINP)
def test_cpu_zero_if_non_pos(cpu, n):
    x, cond = zinp_data(n)
    got = run_all(cpu, add_bck_op_annotations(zinp_op((("v", n),)), OpTune())[0], {"in": x, "cond": cond})["out"]
    assert bits_eq(got, ref.zero_if_non_pos_f32(x, cond))
    assert bits_eq(got[:1], np.zeros(1, np.float32))    # cond = +0: out is +0 whatever in is (the code's `>`, not the comment's `>=`)
    if n >= 3:
        assert bits_eq(got[1:2], np.zeros(1, np.float32)) and got[2] == x[2]   # -0 -> +0; the smallest denormal is positive


def softmax_in(B, C, lo=-4.0, hi=4.0, seed=0):
    return np.random.default_rng(seed + 17 * C + B).uniform(lo, hi, (B, C, 1, 1)).astype(np.float32)


@pytest.mark.parametrize("B,C", SOFTMAX)
def test_cpu_softmax_with_loss(cpu, B, C):
    fs, fg, fl = add_bck_op_annotations(softmax_op(B, C), OpTune())
    for x in (softmax_in(B, C), softmax_in(B, C, -6.0, -1.0)):   # the second: all negative -- pel_max stays 0, which only be=cpu pins bit for bit
        prob = run_all(cpu, fs, {"in": x})["prob"]
        assert bits_eq(prob, ref.softmax_f32(x))
        assert np.all(np.abs(prob - ref.softmax_f64(x)) <= (C + 8) * ref.U * ref.softmax_f64(x))
        lab = labels(B, C)
        got = run_all(cpu, fg, {"prob": prob, "label": lab})
        igl, lpp = ref.sm_grad_and_loss_f32(prob, lab)
        assert bits_eq(got["in_grad_loss"], igl) and bits_eq(got["loss_per_pel"], lpp)
        loss = run_all(cpu, fl, {"loss_per_pel": lpp})["loss"]
        assert bits_eq(loss, ref.sum_loss_over_imgs_f32(lpp))
    shifted = np.exp(x.astype(np.float64) - x.max(axis=1, keepdims=True))   # what a max-shifted softmax would give: the same value, other bits
    assert np.allclose(prob, shifted / shifted.sum(axis=1, keepdims=True), rtol=1e-5)


def test_cpu_softmax_loss_quirks(cpu):
    fs, fg, fl = add_bck_op_annotations(softmax_op(2, 4), OpTune())
    prob = np.array([[0.0, 1.0, 0.0, 0.0], [0.25, 0.25, 0.25, 0.25]], np.float32).reshape(2, 4, 1, 1)
    got = run_all(cpu, fg, {"prob": prob, "label": np.array([0, 3], np.float32).reshape(2, 1, 1)})
    assert got["loss_per_pel"][0, 0, 0] == -ref.logf(np.float32(ref.FLT_MIN))   # prob[label] = 0 is clamped to FLT_MIN
    assert bits_eq(got["in_grad_loss"].reshape(2, 4)[1], np.array([0.125, 0.125, 0.125, (np.float32(0.25) - np.float32(1)) / np.float32(2)], np.float32))
    # the sum over the images is a sequential chain from +0: 2^24 + 1 + 1 stays 2^24, the other order would not
    lpp = np.array([2.0 ** 24, 1.0, 1.0], np.float32).reshape(3, 1, 1)
    loss = run_all(cpu, add_bck_op_annotations(softmax_op(3, 4), OpTune())[2], {"loss_per_pel": lpp})["loss"]
    assert loss.item() == np.float32(2.0 ** 24) / np.float32(3)


def test_cpu_refuses_vars_that_disagree_with_the_op(cpu):
    f = add_bck_op_annotations(spreading_op(*POOL["pad_8x8_k3s2p1"]), OpTune())[0]
    bad = spreading_op(*POOL["overlap_7x7_k3s2"])
    cpu.compile([RtcFuncInfo("g", "", [a for a, _ in NATIVE_ARGS["hip_spreading"]], f)])
    names = ("out", "out_grad_loss", "out_in_yx", "in_grad_loss")
    try:
        for an in names:
            cpu.create_var_with_dims(an, bad.get_dims("out" if an == "out_in_yx" else an))
        am = {an: RtcArg.var(an) for an in names}
        for an in ("kern_sz", "stride", "in_pad"):
            am[an] = RtcArg.ref(f.get_dims(an))
        with pytest.raises(RtErr, match="the op says"):
            cpu.run(RtcFuncCall("g", am))
    finally:
        for an in names:
            cpu.release_var(an)
        cpu.release_func("g"); cpu.release_per_call_id_data()
