"""img_shards=1 without a GPU: the flag (cnn_op.on_img_shards) on the five functions that are not independent per image and its refusal everywhere else -- at annotation,
at compile and in the planner --, flagged equal to unflagged on be=cpu (one shard: a chain of one term), the planner's view of a flagged op, the driver's flagging on a
multi-device backend, and tests/bck_shards_ref.py -- the helper that builds the expected filter / bias gradient of a sharded call -- against float64.

The helper adds per-chunk gradients in numpy fp32; each chunk's gradient is be=cpu's single chain over the chunk's images, within FILTS_MRD of float64 as the whole
batch's chain is (tests/test_bck_conv_cpu.py), and the few adds between chunks re-associate a sum whose bound does not depend on the association: the same bound holds."""
import os

import numpy as np
import pytest

import bck_shards_ref as sref
from boda_amd import rtc as rtc_mod
from boda_amd.bck_pipe import ConvPipeBck, add_bck_ops
from boda_amd.cnn_op import (IMG_SHARDS_FLAG, IMG_SHARDS_FUNCS, NATIVE_ARGS, OpTune, add_bck_conv_annotations, add_bck_op_annotations, add_codegen_annotations,
                             add_pipe_op_annotations, fuse_zero_if_in_non_pos, has_img_shards_flag, on_img_shards, pipe_func_args, seed_from_var)
from boda_amd.conv_pipe import DryRtc, nin_imagenet
from boda_amd.op import Nda, Op, RtErr, parse_op, read_ops
from boda_amd.rtc import RtcFuncInfo, make_rtc

from test_bck_conv_cpu import FILTS_MRD, bck_op, mrd, rand_ins, torch_grads
from test_bck_ops_cpu import labels, pool_op, softmax_in, softmax_op, zinp_op
from test_bck_pipe_cpu import PIPES, dropout_op, reduce_op

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops", "bck-shards-ops.txt")
MULTI_OP = (4, 24, 11, 11, 40, 3, 3, 2, 2, 1, 1)      # the shape of the existing multi-device test (tests/test_gpu_bck_conv.py)
KSL_OP = (3, 8, 27, 27, 16, 3, 3, 1, 1, 1, 1)         # over two shards (1 + 2 images) both per-shard plans cut K into slices
K1S2_OP = (3, 8, 9, 9, 6, 1, 1, 2, 2, 0, 0)           # 1 x 1, stride 2
RAGGED_OP = (5, 7, 8, 8, 33, 3, 3, 1, 1, 1, 1)        # 7 in / 33 out channels: no multiple of any tile
TWO_IMG_OP = (2, 5, 9, 9, 7, 3, 3, 1, 1, 1, 1)        # two images over three shards: the first device holds none
NINE_IMG_OP = (9, 6, 7, 7, 10, 3, 3, 2, 2, 1, 1)      # nine images over eight shards: 1, 1, 1, 1, 1, 1, 1, 2
# (shape, device counts) of the filter / bias gradient cases the GPU test runs
GRAD_CASES = [(MULTI_OP, (2, 3)), (KSL_OP, (2,)), (K1S2_OP, (2,)), (RAGGED_OP, (3,)), (TWO_IMG_OP, (3,)), (NINE_IMG_OP, (8,))]
DROP_DIMS = "(dims=(img=3,chan=5,y=3,x=5))"            # 75 elements per image: no multiple of 4
LOSS_CASES = [(3, 2), (3, 3), (7, 2), (7, 3), (2, 3)]  # (images, shards); 2 over 3: one empty shard
N_CLASS = 65


def ann(op):
    return add_pipe_op_annotations(op, OpTune())


def five(B=3):
    """One annotated function op of each of the five functions."""
    _, fb, ff = add_bck_conv_annotations(bck_op(B, 5, 9, 9, 7, 3, 3, 1, 1, 1, 1), OpTune())
    _, fg, fl = add_bck_op_annotations(softmax_op(B, N_CLASS), OpTune())
    return {"hip_bconv_filts": ff, "hip_bconv_biases": fb, "hip_sm_grad_and_loss": fg, "hip_sum_loss_over_imgs": fl, "hip_dropout": ann(dropout_op(0.5, DROP_DIMS))[0]}


def others():
    """Annotated function ops of native functions that are independent per image (or take no images at all)."""
    op = bck_op(2, 5, 9, 9, 7, 3, 3, 1, 1, 1, 1)
    conv = parse_op("(str_vals=(type=Convolution),nda_vals=(biases=(dims=(out_chan=7)),filts=(dims=(out_chan=7,in_chan=5,y=3,x=3)),in=(dims=(img=2,chan=5,y=9,x=9)),"
                    "in_pad=(tn=none,dims=(y=1,x=1)),kern_sz=(tn=none,dims=(y=3,x=3)),out=(dims=(img=2,chan=7,y=9,x=9)),out_chans=(tn=uint32_t,v=7),stride=(tn=none,dims=(y=1,x=1))))")
    sgemm = parse_op("(str_vals=(type=sgemm),nda_vals=(a=(dims=(K=8,M=16)),b=(dims=(K=8,N=16)),c=(dims=(M=16,N=16))))")
    return [add_bck_conv_annotations(op, OpTune())[0], add_bck_op_annotations(softmax_op(2, 5), OpTune())[0], add_bck_op_annotations(zinp_op((("v", 7),)), OpTune())[0],
            add_bck_op_annotations(pool_op(2, 3, 7, 7, (3, 3), (2, 2), (0, 0)), OpTune())[0], ann(reduce_op(2))[0], add_codegen_annotations(conv, OpTune()),
            add_codegen_annotations(sgemm, OpTune())]


def force_flag(fop):
    a = fop.copy()
    a.nda_vals[IMG_SHARDS_FLAG] = Nda(None, "uint32_t", (1,))
    return a


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


# ---- the flag
def test_on_img_shards_takes_the_five_functions():
    assert IMG_SHARDS_FUNCS == ("hip_bconv_filts", "hip_bconv_biases", "hip_sm_grad_and_loss", "hip_sum_loss_over_imgs", "hip_dropout")
    for fn, f in five().items():
        a = on_img_shards(f)
        assert has_img_shards_flag(a) and not has_img_shards_flag(f) and a.get_func_name() == fn
        assert "img_shards=(tn=uint32_t,v=1)" in a.to_str() and "img_shards" not in f.to_str()
        assert pipe_func_args(a) == pipe_func_args(f)                                  # no new var args
        assert parse_op(a.to_str()).to_str() == a.to_str()
        b = a.copy(); b.nda_vals[IMG_SHARDS_FLAG] = Nda(None, "uint32_t", (0,))
        assert not has_img_shards_flag(b)
    sd = on_img_shards(seed_from_var(five()["hip_dropout"]))                           # the two dropout flags combine
    assert has_img_shards_flag(sd) and [a for a, _ in pipe_func_args(sd)] == ["inout", "det_drop_seed_var", "det_drop_seed"]


def test_every_other_native_function_is_refused_at_annotation():
    rest = [fn for fn in NATIVE_ARGS if fn not in IMG_SHARDS_FUNCS]
    assert len(rest) >= 20
    for fn in rest:
        with pytest.raises(RtErr, match="on_img_shards"):
            on_img_shards(Op({"type": "x", "func_name": fn}, {}))
    with pytest.raises(RtErr, match="on_img_shards"):
        on_img_shards(bck_op(2, 5, 9, 9, 7, 3, 3, 1, 1, 1, 1))   # a bare op: no function yet
    for f in others():
        with pytest.raises(RtErr, match="on_img_shards"):
            on_img_shards(f)


def test_every_other_native_function_is_refused_at_compile_and_in_the_planner(cpu):
    for f in others():
        bad = force_flag(f)
        with pytest.raises(RtErr, match="img_shards=1 on '" + f.get_func_name()):
            cpu.compile([RtcFuncInfo("g", "", [a for a, _ in pipe_func_args(f)], bad)])
        with pytest.raises(RtErr, match="img_shards=1 on '" + f.get_func_name()):
            rtc_mod.explain_plan(bad)
        with pytest.raises(RtErr, match="img_shards=1 on '" + f.get_func_name()):
            rtc_mod.prebuild(bad)
    with pytest.raises(RtErr, match="img_shards=1 on"):                   # a fused ReLU gradient changes nothing about that
        rtc_mod.explain_plan(force_flag(fuse_zero_if_in_non_pos(others()[0])))


def test_planner_shows_the_flag_only_where_it_adds_a_kernel():
    """A flagged function plans as the unflagged one -- the flag is host work --, except that a filter / bias gradient names the kernel that sums the per-device
    partials.  prebuild cross-compiles that kernel for gfx950."""
    fs = five()
    for fn in ("hip_sm_grad_and_loss", "hip_sum_loss_over_imgs", "hip_dropout"):
        assert rtc_mod.explain_plan(on_img_shards(fs[fn])) == rtc_mod.explain_plan(fs[fn])
    for fn in ("hip_bconv_filts", "hip_bconv_biases"):
        plain, flagged = rtc_mod.explain_plan(fs[fn]), rtc_mod.explain_plan(on_img_shards(fs[fn]))
        assert "shard_sum" not in plain and flagged == plain + " | bodahip_shard_sum -DOP=14"
        assert rtc_mod.prebuild(on_img_shards(fs[fn])) > rtc_mod.prebuild(fs[fn]) > 0
    ff = add_bck_conv_annotations(bck_op(*KSL_OP), OpTune())[2]
    ksl = [int(rtc_mod.explain_plan(sref.chunk_op(ff, e - b)).split("ksl=")[1].split()[0]) for b, e in sref.chunks(3, 2)]
    assert min(ksl) > 1, ksl                                                # the case tests/test_gpu_bck_shards.py runs for its K slices


# ---- be=cpu: one shard, a chain of one term
def test_cpu_flagged_equals_unflagged(cpu):
    fs = five()
    op = bck_op(3, 5, 9, 9, 7, 3, 3, 1, 1, 1, 1)
    ins = rand_ins(op, 41)
    for fn in ("hip_bconv_filts", "hip_bconv_biases"):
        an = sref.grad_arg(fs[fn])
        assert sref.bits_eq(sref.run_func(cpu, on_img_shards(fs[fn]), ins)[an], sref.run_func(cpu, fs[fn], ins)[an])
    x = np.random.default_rng(42).uniform(-2, 2, (3, 5, 3, 5)).astype(np.float32)
    for seed in (1, 0xffffffc0):
        assert sref.bits_eq(sref.run_func(cpu, on_img_shards(fs["hip_dropout"]), {"inout": x}, seed=seed)["inout"], sref.run_func(cpu, fs["hip_dropout"], {"inout": x}, seed=seed)["inout"])
        fv = seed_from_var(fs["hip_dropout"]); word = np.array([seed], np.uint32)
        assert sref.bits_eq(sref.run_func(cpu, on_img_shards(fv), {"inout": x, "det_drop_seed_var": word}, seed=7)["inout"],
                            sref.run_func(cpu, fs["hip_dropout"], {"inout": x}, seed=seed + 7)["inout"])
    prob = softmax_in(3, N_CLASS, 0.0, 1.0, seed=43); prob /= prob.sum(axis=1, keepdims=True)
    lab = labels(3, N_CLASS); lab[1] = N_CLASS                            # a label outside [0, chan)
    one, two = sref.run_func(cpu, fs["hip_sm_grad_and_loss"], {"prob": prob, "label": lab}), sref.run_func(cpu, on_img_shards(fs["hip_sm_grad_and_loss"]), {"prob": prob, "label": lab})
    assert sref.bits_eq(one["in_grad_loss"], two["in_grad_loss"]) and sref.bits_eq(one["loss_per_pel"], two["loss_per_pel"])
    lpp = one["loss_per_pel"]
    assert sref.bits_eq(sref.run_func(cpu, on_img_shards(fs["hip_sum_loss_over_imgs"]), {"loss_per_pel": lpp})["loss"], sref.run_func(cpu, fs["hip_sum_loss_over_imgs"], {"loss_per_pel": lpp})["loss"])


# ---- the helper
def test_chunks_are_the_backends_floor_split():
    assert sref.chunks(3, 2) == [(0, 1), (1, 3)] and sref.chunks(5, 3) == [(0, 1), (1, 3), (3, 5)] and sref.chunks(2, 3) == [(0, 0), (0, 1), (1, 2)]
    assert [e - b for b, e in sref.chunks(9, 8)] == [1, 1, 1, 1, 1, 1, 1, 2]
    f = sref.chunk_op(add_bck_conv_annotations(bck_op(*MULTI_OP), OpTune())[2], 1)
    assert f.get_dims("in").sizes == (1, 24, 11, 11) and f.get_dims("out_grad_loss").sizes == (1, 40, 6, 6) and f.get_dims("filts_grad_loss").sizes == (40, 24, 3, 3)
    assert not has_img_shards_flag(sref.unflagged(on_img_shards(f)))


@pytest.mark.parametrize("shape,devs", GRAD_CASES)
def test_helper_chain_against_float64(cpu, shape, devs):
    op = bck_op(*shape)
    ins = rand_ins(op, sum(shape))
    _, fb, ff = add_bck_conv_annotations(op, OpTune())
    _, gw, gb = torch_grads(op, ins["in"], ins["filts"], ins["out_grad_loss"])
    for n in devs:
        w = sref.sharded_grad(cpu, on_img_shards(ff), {"in": ins["in"], "out_grad_loss": ins["out_grad_loss"]}, n)
        b = sref.sharded_grad(cpu, on_img_shards(fb), {"out_grad_loss": ins["out_grad_loss"]}, n)
        print(f"{shape} over {n}: filts mrd {mrd(w, gw):.3e} biases mrd {mrd(b, gb):.3e}")
        assert w.shape == gw.shape and mrd(w, gw) < FILTS_MRD and mrd(b, gb) < FILTS_MRD
    one = sref.sharded_grad(cpu, ff, {"in": ins["in"], "out_grad_loss": ins["out_grad_loss"]}, 1)   # one shard: the function itself, no add
    assert sref.bits_eq(one, sref.run_func(cpu, ff, ins)["filts_grad_loss"])


def test_helper_adds_in_device_order(cpu):
    """(2^24 + 1) - 2^24 = 0 in fp32, any other order gives 1: the chain is ((p_0 + p_1) + p_2), from p_0."""
    og = np.zeros((3, 1, 1, 1), np.float32); og[:, 0, 0, 0] = [2.0 ** 24, 1.0, -(2.0 ** 24)]
    fb = add_bck_conv_annotations(bck_op(3, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0), OpTune())[1]
    assert sref.sharded_grad(cpu, fb, {"out_grad_loss": og}, 3).item() == 0.0
    assert sref.sharded_grad(cpu, fb, {"out_grad_loss": og[[1, 2, 0]]}, 3).item() == 1.0
    assert sref.sharded_grad(cpu, fb, {"out_grad_loss": og[[1, 0, 2]]}, 3).item() == 0.0   # (1 + 2^24) - 2^24
    assert sref.sharded_grad(cpu, fb, {"out_grad_loss": og[[1, 0, 2]]}, 2).item() == 1.0   # 1 + (2^24 - 2^24): each chunk is summed first


# ---- the driver
class MultiDry(DryRtc):
    devices = [0, 0, 0]


@pytest.mark.parametrize("name", sorted(PIPES))
def test_driver_flags_the_five_functions_on_several_devices_only(name):
    mk, tops, _ = PIPES[name]
    cp = mk(3); zeros = {n: np.zeros(d.sizes, np.float32) for n, d in cp.params.items()}
    for kw in ({}, {"seed_in_var": True, "fuse_relu_grad": True}):
        one = ConvPipeBck(DryRtc(), **kw); one.init(add_bck_ops(cp, loss_tops=tops), zeros)
        multi = ConvPipeBck(MultiDry(), **kw); multi.init(add_bck_ops(cp, loss_tops=tops), zeros)
        assert not any(has_img_shards_flag(f) for _, f, _ in one.calls())
        assert [(t, f.get_func_name()) for t, f, _ in one.calls()] == [(t, f.get_func_name()) for t, f, _ in multi.calls()]
        for (_, f1, a1), (_, f2, a2) in zip(one.calls(), multi.calls()):
            assert has_img_shards_flag(f2) == (f2.get_func_name() in IMG_SHARDS_FUNCS) and sorted(a1) == sorted(a2)
            assert sref.unflagged(f2).to_str() == f1.to_str()
        assert {f.get_func_name() for _, f, _ in multi.calls() if has_img_shards_flag(f)} >= {"hip_bconv_filts", "hip_bconv_biases", "hip_sm_grad_and_loss", "hip_sum_loss_over_imgs"}


# ---- the ops build() specialises ahead of the GPU run
def fixture_ops():
    """The function ops tests/test_gpu_bck_shards.py launches, in a fixed order: the per-chunk (and whole-batch) forms of its gradient, dropout and loss cases, the
    calls of its small pipes and of NiN at the image counts a device or the one-device reference sees there -- and one flagged filter / bias gradient, which makes
    build() specialise bodahip_shard_sum ahead of the GPU run."""
    ops = [on_img_shards(f) for f in add_bck_conv_annotations(bck_op(*MULTI_OP), OpTune())[1:]]
    for shape, devs in GRAD_CASES:
        cnts = sorted({shape[0]} | {e - b for n in devs for b, e in sref.chunks(shape[0], n) if e > b})
        for c in cnts:
            _, fb, ff = add_bck_conv_annotations(bck_op(c, *shape[1:]), OpTune())
            ops += [ff, fb]
    for T, n in LOSS_CASES:
        for c in sorted({T} | {e - b for b, e in sref.chunks(T, n) if e > b}):
            ops += list(add_bck_op_annotations(softmax_op(c, N_CLASS), OpTune()))
    d = ann(dropout_op(0.5, DROP_DIMS))[0]
    for c in (1, 2, 3):
        ops += [sref.chunk_op(d, c), sref.chunk_op(seed_from_var(d), c)]
    for name in sorted(PIPES):
        mk, tops, _ = PIPES[name]
        for B in (1, 2, 3, 5):
            cp = mk(B)
            for kw in ({}, {"fuse_relu_grad": True}):
                drv = ConvPipeBck(DryRtc(), **kw); drv.init(add_bck_ops(cp, loss_tops=tops), {n: np.zeros(dd.sizes, np.float32) for n, dd in cp.params.items()})
                ops += [f for _, f, _ in drv.calls()]
    cp = nin_imagenet(1)
    drv = ConvPipeBck(DryRtc()); drv.init(add_bck_ops(cp), {n: np.zeros(dd.sizes, np.float32) for n, dd in cp.params.items()})
    ops += [f for _, f, _ in drv.calls()]
    seen, out = set(), []
    for f in ops:
        if f.to_str() not in seen:
            seen.add(f.to_str()); out.append(f)
    return out


def test_fixture_file_lists_these_ops():
    have = [o.to_str() for o in read_ops(GOLD)]
    assert have == [f.to_str() for f in fixture_ops()] and len(have) >= 50
