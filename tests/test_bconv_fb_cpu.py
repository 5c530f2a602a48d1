"""hip_bconv_filts_biases (the fused filter + bias gradient, opt-in) without a GPU: the function op and its arg table, be=cpu's call against the two calls it
replaces (bit for bit), the numpy twin of the GPU kernel's bias chain (tests/bconv_fb_ref.py) against a plain sum and float64, the planner (more than 32 slices,
never a slice depth under 8 K steps), the refusals by name, and ConvPipeBck(fuse_filts_biases=True) on the three small pipes of tests/test_bck_pipe_cpu.py.

The float64 bound is FILTS_MRD = 1e-5 of tests/test_bck_conv_cpu.py: max|x - r| / max|r| per tensor."""
import numpy as np
import pytest

import bconv_fb_ref as fb
from boda_amd import rtc as rtc_mod
from boda_amd.bck_pipe import ConvPipeBck, add_bck_ops
from boda_amd.cnn_op import NATIVE_ARGS, OpTune, add_bck_conv_annotations, bconv_filts_biases_func_op, fuse_zero_if_in_non_pos, on_img_shards, pipe_func_args
from boda_amd.op import Nda, RtErr, UnsupErr
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc

from oracle import bck_chain as bc

from test_bck_conv_cpu import FILTS_MRD, bck_op, mrd, rand_ins, run_func, torch_grads
from test_bck_pipe_cpu import PIPES, SEED_A, grad_nodes, small_inputs, small_params

FN = "hip_bconv_filts_biases"


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_fused(rtc, fop, ins):
    """One hip_bconv_filts_biases call on `rtc` with host inputs -> (filts_grad_loss, biases_grad_loss)."""
    rtc.compile([RtcFuncInfo("fb", "", [a for a, _ in NATIVE_ARGS[FN]], fop)])
    am, made = {}, []
    try:
        for an, io in NATIVE_ARGS[FN]:
            if io == "REF":
                am[an] = RtcArg.ref(fop.get_dims(an)); continue
            vn = an
            rtc.create_var_with_dims(vn, fop.get_dims(vn)); made.append(vn)
            am[an] = RtcArg.var(vn)
            if io == "IN":
                rtc.copy_nda_to_var(vn, np.ascontiguousarray(ins[an], dtype=np.float32))
        rtc.run(RtcFuncCall("fb", am))
        rtc.finish_and_sync()
        return rtc.copy_var_to_nda(am["filts_grad_loss"].n), rtc.copy_var_to_nda(am["biases_grad_loss"].n)
    finally:
        for vn in made:
            rtc.release_var(vn)
        rtc.release_func("fb"); rtc.release_per_call_id_data()


# ---- the function op
def test_function_op_and_arg_table():
    op = fb.shape_op("k3_borders")
    f = bconv_filts_biases_func_op(op, OpTune())
    assert f.get_func_name() == FN and f.get_type() == "BckConv" and "hip_tile" not in f.str_vals
    assert NATIVE_ARGS[FN] == (("in", "IN"), ("out_grad_loss", "IN"), ("stride", "REF"), ("in_pad", "REF"), ("filts_grad_loss", "OUT"), ("biases_grad_loss", "OUT"))
    assert pipe_func_args(f) == NATIVE_ARGS[FN]
    assert bconv_filts_biases_func_op(op, OpTune(hip_tile="64x128x32x2x2x2x5")).str_vals["hip_tile"] == "64x128x32x2x2x2x5"
    assert [x.get_func_name() for x in add_bck_conv_annotations(op, OpTune())] == ["hip_bconv_in", "hip_bconv_biases", "hip_bconv_filts"]   # stays as it is
    with pytest.raises(UnsupErr):
        bconv_filts_biases_func_op(op, OpTune(hip_dtype="bf16"))
    other = op.copy(); other.str_vals["type"] = "Convolution"
    with pytest.raises(RtErr, match="not BckConv"):
        bconv_filts_biases_func_op(other, OpTune())


# ---- be=cpu: one call equals the two it replaces
@pytest.mark.parametrize("name", sorted(fb.SHAPES))
def test_cpu_call_equals_the_pair_bit_for_bit(cpu, name):
    op = fb.shape_op(name)
    ins = rand_ins(op, 3)
    _, fbias, ffilts = add_bck_conv_annotations(op, OpTune())
    want_f, want_b = run_func(cpu, ffilts, ins), run_func(cpu, fbias, ins)
    got_f, got_b = run_fused(cpu, bconv_filts_biases_func_op(op, OpTune()), ins)
    assert got_f.shape == want_f.shape and np.array_equal(bits(got_f), bits(want_f))
    assert got_b.shape == want_b.shape and np.array_equal(bits(got_b), bits(want_b))
    _, w64, b64 = torch_grads(op, ins["in"], ins["filts"], ins["out_grad_loss"])
    assert mrd(got_f, w64) <= FILTS_MRD and mrd(got_b, b64) <= FILTS_MRD


# ---- the numpy twin of the GPU's bias chain
def test_bias_twin_with_one_chain_is_the_sequential_sum():
    g = rand_ins(fb.shape_op("k1_ohw49_tail"), 5)["out_grad_loss"]
    B, OC = g.shape[:2]
    want = np.zeros(OC, np.float32)
    for img in range(B):
        for e in g[img].reshape(OC, -1).T:
            want = want + e
    assert np.array_equal(bits(fb.biases_chain(g, 1, 1)), bits(want))


def test_bias_twin_depends_on_the_plan_and_on_nothing_else():
    g = rand_ins(fb.shape_op("k1_long_k"), 6)["out_grad_loss"]
    a, b, c = fb.biases_chain(g, 32, 1), fb.biases_chain(g, 32, 12), fb.biases_chain(g, 16, 12)
    assert not np.array_equal(bits(a), bits(b)) and not np.array_equal(bits(b), bits(c))
    assert np.array_equal(bits(b), bits(fb.biases_chain(g.copy(), 32, 12)))
    assert bc.filts_slices(3136, 32, 98) == [(32 * s, 32 * s + 32) for s in range(98)]   # (the slice ranges the twin takes: whole K steps)


@pytest.mark.parametrize("name", sorted(fb.SHAPES))
def test_twins_within_bound_of_float64(name):
    op = fb.shape_op(name)
    ins = rand_ins(op, 4)
    _, w64, b64 = torch_grads(op, ins["in"], ins["filts"], ins["out_grad_loss"])
    I, J = bc.filts_operands(ins["in"], ins["out_grad_loss"], op.bck_conv_geom())
    for bk, ksl in fb.PLANS:
        eb = mrd(fb.biases_chain(ins["out_grad_loss"], bk, ksl), b64)
        ef = mrd(bc.filts_sliced_chain(I, J, bk, ksl, w64.shape), w64)
        print(f"{name} (BK, KSL) = ({bk}, {ksl}): bias {eb:.2e} filts {ef:.2e}")
        assert eb <= FILTS_MRD and ef <= FILTS_MRD, (name, bk, ksl, eb, ef)


# ---- the planner
def ksl_of(plan):
    return int(plan.split("ksl=")[1].split()[0])


def test_explain_plan_names_the_kernel_and_ksl():
    op = fb.shape_op("k1_long_k")
    f = bconv_filts_biases_func_op(op, OpTune())
    plan = rtc_mod.explain_plan(f)
    assert plan.startswith("bodahip_bconv_filts_biases ") and "ksl=" in plan, plan
    assert ksl_of(plan) > 1 and "bodahip_bconv_slab_sum" in plan                      # sliced: the second launch is named too
    one = rtc_mod.explain_plan(f, tile="64x64x32x2x2x1x1")
    assert "ksl=1" in one and "slab_sum" not in one and "64x64x32_w2x2" in one        # one slice: no second launch
    assert "ksl=40" in rtc_mod.explain_plan(bconv_filts_biases_func_op(op, OpTune(hip_tile="32x128x32x1x4x1x40")))   # the tile travels with the function
    assert "bconv_filts_biases" not in rtc_mod.explain_plan(op)                        # the bare op: still the three calls of the default pipe


def test_planner_exceeds_32_slices_on_one_tile_and_long_k():
    """64 -> 64 channels, 1x1, 56 x 56 maps, 32 images on 256 CUs: one 64 x 128 tile, K = 100 352 = 3136 K steps of 32.  hip_bconv_filts stops at its cap of 32
    slices; the fused function takes min(2 * 256 / 1, 3136 / 8) = 392."""
    op = bck_op(32, 64, 56, 56, 64, 1, 1, 1, 1, 0, 0)
    assert ksl_of(rtc_mod.explain_plan(bconv_filts_biases_func_op(op, OpTune()), num_cus=256)) == 392
    assert ksl_of(rtc_mod.explain_plan(add_bck_conv_annotations(op, OpTune())[2], num_cus=256)) == 32


def test_planner_never_plans_a_slice_depth_under_8_k_steps():
    """Over a sweep of K and tile counts: KSL > 1 only with kt_per = ceil(nkt / KSL) >= 8 (the last slice holds the remainder), 1 <= KSL <= 1024, and about two
    workgroups per CU where K allows it."""
    seen_big = 0
    for B, C, H, OC in [(1, 8, 5, 8), (1, 8, 15, 8), (2, 8, 16, 8), (3, 20, 7, 24), (4, 8, 28, 8), (32, 64, 56, 64), (32, 256, 56, 64), (256, 96, 55, 96), (64, 16, 112, 16),
                        (256, 16, 112, 16), (32, 512, 7, 2048), (5, 600, 9, 300)]:
        for cus in (8, 104, 256):
            op = bck_op(B, C, H, H, OC, 1, 1, 1, 1, 0, 0)
            plan = rtc_mod.explain_plan(bconv_filts_biases_func_op(op, OpTune()), num_cus=cus)
            bi, bj, bk = (int(v) for v in plan.split()[1].split("_")[0].split("x"))
            ksl = ksl_of(plan)
            nkt = -(-(B * H * H) // bk)
            tiles = -(-OC // bi) * -(-C // bj)
            assert 1 <= ksl <= 1024
            if ksl > 1:
                assert -(-nkt // ksl) >= 8, (plan, nkt)
            assert ksl == max(1, min(1024, -(-2 * cus // tiles), max(1, nkt // 8))), (plan, cus)
            seen_big += ksl > 32
    assert seen_big >= 4


# ---- refusals, by name
def test_refusals_by_name(cpu):
    op = fb.shape_op("k3_borders")
    f = bconv_filts_biases_func_op(op, OpTune())
    for tile in ("100x128x32x2x2", "64x64x32x2x2x1x0", "64x64x32x2x2x1x1025", "64x64x31x2x2x1x1", "64x64x48x2x2x1x1"):
        with pytest.raises(UnsupErr, match="hip_bconv_filts_biases: unsupported tile configuration"):
            rtc_mod.explain_plan(f, tile=tile)
    with pytest.raises(UnsupErr, match="hip_bconv_filts_biases: bad tile"):
        rtc_mod.explain_plan(f, tile="64x64")
    assert "ksl=1024" in rtc_mod.explain_plan(f, tile="64x64x32x2x2x1x1024")
    with pytest.raises(UnsupErr, match="hip_bconv_filts_biases: unsupported geometry"):
        rtc_mod.explain_plan(bconv_filts_biases_func_op(bck_op(1, 2, 40, 40, 3, 3, 3, 17, 17, 0, 0), OpTune()))
    with pytest.raises(RtErr, match="on_img_shards.*hip_bconv_filts_biases"):
        on_img_shards(f)
    with pytest.raises(RtErr, match="fuse_zero_if_in_non_pos.*hip_bconv_filts_biases"):
        fuse_zero_if_in_non_pos(f)
    for flag, msg in (("img_shards", "img_shards=1 on 'hip_bconv_filts_biases'"), ("zero_if_in_non_pos", "zero_if_in_non_pos=1 on 'hip_bconv_filts_biases'")):
        g = f.copy()
        g.nda_vals[flag] = Nda(None, "uint32_t", (1,))
        with pytest.raises(RtErr, match=msg):    # the backend's own refusal, at compile
            cpu.compile([RtcFuncInfo("bad", "", [a for a, _ in NATIVE_ARGS[FN]], g)])
        with pytest.raises(RtErr, match=msg):
            rtc_mod.explain_plan(g)


def test_cpu_refuses_aliased_outputs_and_missing_args(cpu):
    op = bck_op(2, 4, 5, 5, 4, 1, 1, 1, 1, 0, 0)   # in and out_grad_loss have the same dims: a var can be bound to both
    f = bconv_filts_biases_func_op(op, OpTune())
    ins = rand_ins(op, 1)
    run_fused(cpu, f, ins)
    cpu.compile([RtcFuncInfo("fb", "", [a for a, _ in NATIVE_ARGS[FN]], f)])
    made = []
    try:
        am = {}
        for an, io in NATIVE_ARGS[FN]:
            if io == "REF":
                am[an] = RtcArg.ref(f.get_dims(an))
            else:
                cpu.create_var_with_dims(an, f.get_dims(an)); made.append(an); am[an] = RtcArg.var(an)
        for missing in ("biases_grad_loss", "filts_grad_loss", "in", "stride"):
            with pytest.raises(RtErr, match=missing if missing != "stride" else "stride"):
                cpu.run(RtcFuncCall("fb", {k: v for k, v in am.items() if k != missing}))
        alias = dict(am, filts_grad_loss=RtcArg.var("in"))       # 2 x 4 x 5 x 5 is not filts' dims: refused on dims or as an alias, never run
        with pytest.raises(RtErr):
            cpu.run(RtcFuncCall("fb", alias))
    finally:
        for vn in made:
            cpu.release_var(vn)
        cpu.release_func("fb"); cpu.release_per_call_id_data()


# ---- the pipe
def run_small_pipe(rtc, name, **kw):
    mk, tops, seed = PIPES[name]
    cp = mk(); bp = add_bck_ops(cp, loss_tops=tops)
    data, label = small_inputs(cp, seed)
    drv = ConvPipeBck(rtc, **kw); drv.init(bp, small_params(cp, seed))
    drv.set_det_drop_seed(SEED_A)
    fwd = {"data": data, "label": label}
    drv.run_bck(["data", "label"], fwd, grad_nodes(bp) + bp.loss_nodes)
    return drv, bp, fwd


def call_list(drv):
    return [(t, f.get_func_name(), tuple(sorted((an, a.n) for an, a in am.items() if a.n))) for t, f, am in drv.calls()]


@pytest.mark.parametrize("name", sorted(PIPES))
def test_cpu_pipe_with_the_option_replaces_the_pairs_and_keeps_every_bit(cpu, name):
    off, bp, fwd_off = run_small_pipe(cpu, name)
    try:
        calls_off = call_list(off)
    finally:
        off.release()
    on, _, fwd_on = run_small_pipe(cpu, name, fuse_filts_biases=True)
    try:
        calls_on = call_list(on)
        deps = on._call_deps()
        fused_ix = [i for i, c in enumerate(on.bck_calls) if c.fop.get_func_name() == FN]
        for i in fused_ix:   # two written vars: both order the call
            am = on.bck_calls[i].rfc.arg_map
            assert [an for an, io in pipe_func_args(on.bck_calls[i].fop) if io == "OUT"] == ["filts_grad_loss", "biases_grad_loss"]
            assert am["filts_grad_loss"].n.endswith("_filts_grad_loss") and am["biases_grad_loss"].n.endswith("_biases_grad_loss")
            writer = max(j for j in range(i) if am["out_grad_loss"].n in [a.n for an, a in on.bck_calls[j].rfc.arg_map.items()
                                                                         if dict(pipe_func_args(on.bck_calls[j].fop)).get(an) in ("OUT", "INOUT") or an == "inout"])
            assert writer in deps[i], (i, deps[i], writer)   # it follows the last writer of the gradient it reads
    finally:
        on.release()
    # the call list: every (hip_bconv_biases, hip_bconv_filts) pair of one op becomes one hip_bconv_filts_biases with the union of their args; nothing else moves
    want, i = [], 0
    while i < len(calls_off):
        t, fn, args = calls_off[i]
        if fn == "hip_bconv_biases":
            t2, fn2, args2 = calls_off[i + 1]
            assert fn2 == "hip_bconv_filts" and t2 == t
            want.append((t, FN, tuple(sorted(set(args) | set(args2))))); i += 2
        else:
            want.append(calls_off[i]); i += 1
    assert calls_on == want
    n_conv = sum(1 for _, fn, _ in calls_off if fn == "hip_bconv_in")
    assert sum(1 for _, fn, _ in calls_on if fn == FN) == n_conv >= 2 and len(calls_on) == len(calls_off) - n_conv
    for n in grad_nodes(bp) + bp.loss_nodes:   # be=cpu: both forms are the single chains
        assert np.array_equal(bits(fwd_on[n]), bits(fwd_off[n])), n


def test_option_off_is_the_default_call_list(cpu):
    a, _, _ = run_small_pipe(cpu, "chain")
    try:
        la, fa = call_list(a), list(a.funcs)
    finally:
        a.release()
    b, _, _ = run_small_pipe(cpu, "chain", fuse_filts_biases=False)
    try:
        lb, fb_ = call_list(b), list(b.funcs)
    finally:
        b.release()
    assert la == lb and fa == fb_
    assert [(t, fn) for t, fn, _ in la] == [
        ("conv1", "hip_conv"), ("norm1", "hip_lrn_sb"), ("pool1", "hip_pool_yx"), ("drop1", "hip_dropout"), ("fc", "hip_conv"),
        ("loss", "hip_softmax"), ("loss", "hip_sm_grad_and_loss"), ("loss", "hip_sum_loss_over_imgs"),
        ("fc_bck", "hip_bconv_in"), ("fc_bck", "hip_bconv_biases"), ("fc_bck", "hip_bconv_filts"), ("drop1_bck", "hip_dropout"), ("pool1_bck", "hip_spreading"),
        ("norm1_bck", "hip_bck_lrn"), ("relu_conv1_bck", "hip_zero_if_non_pos"),
        ("conv1_bck", "hip_bconv_in"), ("conv1_bck", "hip_bconv_biases"), ("conv1_bck", "hip_bconv_filts")]
    assert fa[8:11] == ["bck_8_hip_bconv_in", "bck_9_hip_bconv_biases", "bck_10_hip_bconv_filts"]
