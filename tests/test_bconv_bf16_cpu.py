"""hip_operands=bf16 without a GPU: the op value and its refusals, cnn_op.bf16_operands, the planners of the two bf16-operand kernels, be=cpu's semantics (operands
rounded by its own round-to-nearest-even helper, the template loops, unrounded biases) held bit for bit to be=cpu WITHOUT the value fed oracle-rounded operands, the
bound of tests/bconv_bf16_ref.py, and ConvPipeBck(grad_operands="bf16") on the three small pipes and the residual pipe."""
import os

import numpy as np
import pytest

import bck_pipe_ref as ref
import bconv_bf16_ref as R
import bconv_fb_ref as fb
import bn_ref as BN
from boda_amd import rtc as rtc_mod
from boda_amd.bck_pipe import ConvPipeBck, add_bck_ops
from boda_amd.cnn_op import OpTune, add_bck_conv_annotations, bconv_filts_biases_func_op, bf16_operands, has_bf16_operands
from boda_amd.op import RtErr, UnsupErr, read_ops
from boda_amd.rtc import RtcFuncInfo, make_rtc

from oracle.boda_oracle import to_bf16

from test_bck_conv_cpu import SMALL, bck_op
from test_bck_pipe_cpu import PIPES, SEED_A, grad_nodes, small_inputs, small_params, want_f64

F = np.float32
CPU_SHAPES = [("small%d" % i, bck_op(*s)) for i, s in enumerate(SMALL)] + [(n, fb.shape_op(n)) for n in sorted(fb.SHAPES)]


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


# ---- the value on the op, host side
def test_bf16_operands_on_each_of_the_four_functions():
    op = bck_op(2, 8, 9, 9, 16, 3, 3, 2, 2, 1, 1)
    fi, fbi, ff = add_bck_conv_annotations(op, OpTune())
    ffb = bconv_filts_biases_func_op(op, OpTune())
    for f in (fi, ffb):
        a = bf16_operands(f)
        assert a is not f and a.str_vals["hip_operands"] == "bf16" and has_bf16_operands(a) and "hip_operands" not in f.str_vals and not has_bf16_operands(f)
        assert a.get_func_name() == f.get_func_name()
        assert rtc_mod.func_args(a) == rtc_mod.func_args(f)          # the arg list is unchanged
    for f in (ff, fbi):
        with pytest.raises(UnsupErr, match="hip_bconv_filts_biases"):
            bf16_operands(f)
    with pytest.raises(RtErr, match="bf16_operands"):
        bf16_operands(op)                                              # a bare op
    for tune in (OpTune(hip_dtype="bf16"),):                           # the tune keeps refusing bf16: the value is not a tune
        with pytest.raises(UnsupErr):
            add_bck_conv_annotations(op, tune)
        with pytest.raises(UnsupErr):
            bconv_filts_biases_func_op(op, tune)


def test_backend_refusals_at_plan_prebuild_compile_and_run(cpu):
    op = bck_op(2, 8, 9, 9, 16, 3, 3, 2, 2, 1, 1)
    fi, fbi, ff = add_bck_conv_annotations(op, OpTune())
    ffb = bconv_filts_biases_func_op(op, OpTune())
    for f in (ff, fbi):                                                # bf16 on the unfused pair: UnsupErr naming the fused call
        b = f.copy(); b.str_vals["hip_operands"] = "bf16"
        with pytest.raises(UnsupErr, match="hip_bconv_filts_biases"):
            rtc_mod.explain_plan(b)
        with pytest.raises(UnsupErr, match="hip_bconv_filts_biases"):
            rtc_mod.prebuild(b)
        with pytest.raises(UnsupErr, match="hip_bconv_filts_biases"):
            cpu.compile([RtcFuncInfo("bad", "", [], b)])
    for f in (fi, ffb):                                                # any other value: RtErr naming the two legal ones
        b = f.copy(); b.str_vals["hip_operands"] = "fp16"
        with pytest.raises(RtErr, match="f32 \\| bf16"):
            rtc_mod.explain_plan(b)
        with pytest.raises(RtErr, match="f32 \\| bf16"):
            cpu.compile([RtcFuncInfo("bad", "", [], b)])
        with pytest.raises(RtErr, match="f32 \\| bf16"):
            R.run_fop(cpu, b, R.rand_ins(op, 0))
        for v in ("f32", ""):                                          # f32, or present and empty: the function as it is
            c = f.copy(); c.str_vals["hip_operands"] = v
            assert rtc_mod.explain_plan(c) == rtc_mod.explain_plan(f)
    from test_bck_pipe_cpu import ann, dropout_op                      # another family does not look at the value
    d = ann(dropout_op(0.5))[0]
    e = d.copy(); e.str_vals["hip_operands"] = "fp16"
    assert rtc_mod.explain_plan(e) == rtc_mod.explain_plan(d)


# ---- plans
def test_plans_forced_tiles_and_limits():
    op = bck_op(4, 96, 27, 27, 256, 5, 5, 1, 1, 2, 2)
    fi, ffb = R.in_func(op), R.fb_func(op)
    p = rtc_mod.explain_plan(fi)
    assert p.startswith("bodahip_bconv_in_bf16 ") and " grid=" in p and "ZINP" not in p, p
    assert rtc_mod.explain_plan(R.in_func(op, zinp=True)).endswith(" -DZINP=1")
    p = rtc_mod.explain_plan(ffb)
    assert p.startswith("bodahip_bconv_filts_biases_bf16 ") and " ksl=" in p, p
    ksl = int(p.split("ksl=")[1].split()[0])
    assert (ksl > 1) == p.endswith(" | bodahip_bconv_slab_sum"), p
    assert rtc_mod.explain_plan(R.fb_func(bck_op(4, 8, 28, 28, 8, 1, 1, 1, 1, 0, 0))).endswith("| bodahip_bconv_slab_sum")     # a long K on one tile: sliced
    # the slice rule starts as the fp32 fused call's: the same KSL at the same (default) tile
    assert ksl == int(rtc_mod.explain_plan(R.fb_func(op, bf16=False)).split("ksl=")[1].split()[0])
    assert rtc_mod.explain_plan(fi, tile="64x64x64x2x2").startswith("bodahip_bconv_in_bf16 64x64x64_w2x2 ")
    assert rtc_mod.explain_plan(R.in_func(op, tile="32x32x32x1x1")).startswith("bodahip_bconv_in_bf16 32x32x32_w1x1 ")           # a tile that travels with the function
    p = rtc_mod.explain_plan(ffb, tile="64x64x16x2x2x2x98")
    assert p.startswith("bodahip_bconv_filts_biases_bf16 64x64x16_w2x2") and "ksl=98 | bodahip_bconv_slab_sum" in p, p
    assert "ksl=1" in rtc_mod.explain_plan(ffb, tile="64x64x32x2x2x1x1") and "slab_sum" not in rtc_mod.explain_plan(ffb, tile="64x64x32x2x2x1x1")
    assert "ksl=1024" in rtc_mod.explain_plan(ffb, tile="64x64x32x2x2x1x1024")
    for f, what in ((fi, "hip_bconv_in"), (ffb, "hip_bconv_filts_biases")):
        for bad in ("64x64x24x2x2", "64x64x8x2x2",              # BK not a multiple of 16 (both are legal fp32 tiles)
                    "64x64x32x2x2x1x0", "64x64x32x2x2x1x1025",   # KSL 0 / 1025
                    "128x128x256x4x4",                           # 2 * 256 * 264 * 2 bytes of LDS: above 160 KiB
                    "100x128x32x2x2"):
            with pytest.raises(UnsupErr, match=what + " \\(hip_operands=bf16\\): unsupported tile"):
                rtc_mod.explain_plan(f, tile=bad)
        assert "128x128x128_w4x4" in rtc_mod.explain_plan(f, tile="128x128x128x4x4")     # 139264 bytes: fits
    with pytest.raises(UnsupErr, match="hip_bconv_in \\(hip_operands=bf16\\)"):
        rtc_mod.explain_plan(fi, tile="64x64x32x2x2x1x2")                                 # the data gradient has no K slices
    assert rtc_mod.explain_plan(R.in_func(op, bf16=False), tile="64x64x8x2x2").startswith("bodahip_bconv_in 64x64x8")   # the fp32 functions are as they were


def test_both_kernels_cross_compile():
    op = bck_op(2, 19, 7, 7, 33, 3, 3, 1, 1, 1, 1)
    assert rtc_mod.prebuild(R.in_func(op, zinp=True)) > 0
    assert rtc_mod.prebuild(R.fb_func(op, tile="64x64x32x2x2x1x3")) > 0


# ---- be=cpu: the checker
def test_cpu_rounding_helper_against_the_oracle(cpu):
    """A 1x1 convolution with one out_chan and out_grad_loss = 1: in_grad_loss[c] = 0 + r(1) * r(filts[c]) = r(filts[c]) (a -0 becomes +0 in the sum from +0:
    compared by value).  Ties both ways, values just below / above a tie, zeros, infinities, NaN, the largest finite bf16 and the values that round up to inf."""
    u = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFFFFFFF,
                  0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0xFF7F8000, 0x00010000, 0x00008000, 0x00008001, 0x3F800000, 0xBF808000, 0xBF818000], np.uint32)
    vals = u.view(F)
    want = to_bf16(vals)
    assert want.view(np.uint32)[0] == 0x3F800000 and want.view(np.uint32)[1] == 0x3F820000       # the two ties: to even, down and up
    assert want.view(np.uint32)[14] == 0x7F7F0000 and np.isinf(want[15]) and np.isinf(want[16])
    op = bck_op(1, len(vals), 1, 1, 1, 1, 1, 1, 1, 0, 0)
    got = R.run_fop(cpu, R.in_func(op), {"filts": vals.reshape(1, -1, 1, 1), "out_grad_loss": np.ones((1, 1, 1, 1), F)})["in_grad_loss"].reshape(-1)   # (every channel a sum of its own: one term)
    for k in range(len(vals)):
        if np.isnan(want[k]):
            assert np.isnan(got[k]), (hex(u[k]), got[k])
        else:
            assert got[k] == want[k] and (want[k] == 0 or R.bits(got[k:k + 1])[0] == R.bits(want[k:k + 1])[0]), (hex(u[k]), got[k], want[k])


@pytest.mark.parametrize("name,op", CPU_SHAPES, ids=[n for n, _ in CPU_SHAPES])
def test_cpu_value_equals_rounded_operands_and_holds_the_bound(cpu, name, op):
    ins = R.rand_ins(op, len(name) + op.get_dims("in").sizes[1])
    rnd = {an: to_bf16(ins[an]) for an in ("filts", "out_grad_loss", "in")}
    r = R.refs(op, ins)
    # data gradient, without and with zero_if_in_non_pos: the condition `in` is read unrounded
    for zinp in (False, True):
        got = R.run_fop(cpu, R.in_func(op, zinp=zinp), ins)["in_grad_loss"]
        want = R.run_fop(cpu, R.in_func(op, zinp=zinp, bf16=False), {"filts": rnd["filts"], "out_grad_loss": rnd["out_grad_loss"], "in": ins["in"]})["in_grad_loss"]
        assert R.same_bits(got, want), (name, zinp)
        if not zinp:
            plain = got
            R.check_bound(op, "in", got, r, what=f"be=cpu {name}")
        else:
            assert R.same_bits(got, np.where(ins["in"] > 0, plain, F(0))), name
            assert np.any(ins["in"] <= 0)
    # fused filter and bias gradient: filters from the rounded operands, biases from the UNROUNDED out_grad_loss
    got = R.run_fop(cpu, R.fb_func(op), ins)
    want = R.run_fop(cpu, R.fb_func(op, bf16=False), {"in": rnd["in"], "out_grad_loss": rnd["out_grad_loss"]})
    unr = R.run_fop(cpu, R.fb_func(op, bf16=False), ins)
    assert R.same_bits(got["filts_grad_loss"], want["filts_grad_loss"]), name
    assert R.same_bits(got["biases_grad_loss"], unr["biases_grad_loss"]), name
    assert not R.same_bits(got["filts_grad_loss"], unr["filts_grad_loss"])     # the value does something
    R.check_bound(op, "filts", got["filts_grad_loss"], r, what=f"be=cpu {name}")


def test_cpu_condition_is_read_unrounded(cpu):
    """in = 2^-140 > 0 rounds to +0 in bf16 (a subnormal below half the smallest bf16 subnormal): the select must keep the gradient."""
    op = bck_op(1, 2, 1, 1, 1, 1, 1, 1, 1, 0, 0)
    tiny = F(2.0 ** -140)
    assert tiny > 0 and to_bf16(np.array([tiny]))[0] == 0
    ins = {"filts": np.array([3.0, 5.0], F).reshape(1, 2, 1, 1), "out_grad_loss": np.ones((1, 1, 1, 1), F), "in": np.array([tiny, -tiny], F).reshape(1, 2, 1, 1)}
    got = R.run_fop(cpu, R.in_func(op, zinp=True), ins)["in_grad_loss"].reshape(-1)
    assert got[0] == 3.0 and R.bits(got[1:])[0] == 0


# ---- the pipe
class _TwoDevices:
    devices = [0, 0]


def test_driver_refusals():
    mk, tops, seed = PIPES["chain"]
    cp = mk(); bp = add_bck_ops(cp, loss_tops=tops)
    for bad in ("fp16", "BF16", "bf16 ", "f32"):
        with pytest.raises(RtErr, match="grad_operands"):
            ConvPipeBck(None, grad_operands=bad)
    assert ConvPipeBck(None).grad_operands == "" and not ConvPipeBck(None).fuse_filts_biases
    assert ConvPipeBck(None, grad_operands="bf16").fuse_filts_biases
    drv = ConvPipeBck(_TwoDevices(), grad_operands="bf16")
    with pytest.raises(UnsupErr, match="grad_operands='bf16'.*multi-device"):
        drv.init(bp, small_params(cp, seed))
    assert drv.vars == [] and drv.funcs == []      # refused before anything was created


def _fwd_nodes(bp):
    return [n for n in bp.nodes if not n.endswith("_grad_loss") and n not in bp.loss_nodes and n not in ("data", "label") and n not in bp.cp.params]


def _check_calls(drv, bp):
    fns = [(f.get_func_name(), f) for _, f, _ in drv.calls()]
    n_conv = sum(1 for o in bp.bck_ops() if o.type == "BckConv")
    assert sum(1 for n, f in fns if n == "hip_bconv_in" and has_bf16_operands(f)) == n_conv >= 2
    assert sum(1 for n, f in fns if n == "hip_bconv_filts_biases" and has_bf16_operands(f)) == n_conv
    assert not any(n in ("hip_bconv_filts", "hip_bconv_biases") for n, _ in fns)
    assert not any(has_bf16_operands(f) for n, f in fns if not n.startswith("hip_bconv"))


@pytest.mark.parametrize("name", sorted(PIPES))
def test_cpu_pipe_with_bf16_gradient_operands(cpu, name):
    mk, tops, seed = PIPES[name]
    out = {}
    for mode, kw in (("", {}), ("bf16", {"grad_operands": "bf16"}), ("bf16+fuse_relu_grad", {"grad_operands": "bf16", "fuse_relu_grad": True})):
        cp = mk(); bp = add_bck_ops(cp, loss_tops=tops)
        data, label = small_inputs(cp, seed)
        drv = ConvPipeBck(cpu, **kw); drv.init(bp, small_params(cp, seed))
        try:
            drv.set_det_drop_seed(SEED_A)
            fwd = {"data": data, "label": label}
            drv.run_bck(["data", "label"], fwd, grad_nodes(bp) + bp.loss_nodes + _fwd_nodes(bp))
            if mode:
                _check_calls(drv, bp)
                want = want_f64(name, drv)
            out[mode] = fwd
        finally:
            drv.release()
    for n in _fwd_nodes(bp) + bp.loss_nodes:   # the forward pass and the loss are untouched
        assert R.same_bits(out["bf16"][n], out[""][n]), n
    for n in grad_nodes(bp):
        if "_split_" in n:
            continue
        assert np.all(np.isfinite(out["bf16"][n])), n
        print(f"E_cpu {name} {n}: bf16 {ref.rel_err(out['bf16'][n], want[n]):.3e} (fp32 {ref.rel_err(out[''][n], want[n]):.3e})")
    # the loss tops' gradients and the biases' gradients of the convolutions that write them pass no rounded product: the default driver's bits; every other node changes
    assert {n for n in grad_nodes(bp) if R.same_bits(out["bf16"][n], out[""][n])} == R.unchanged_grad_nodes(tops or [bp.cp.out_node()])
    folded = out["bf16+fuse_relu_grad"]       # zero_if_in_non_pos composes: the folded ReLU gradients leave the same bits
    for n in [pn + "_grad_loss" for pn in bp.cp.params]:
        assert R.same_bits(folded[n], out["bf16"][n]), n


def test_cpu_residual_pipe_with_bf16_gradient_operands(cpu):
    seed = BN.RES_SEEDS[0]
    out = {}
    for mode in ("", "bf16"):
        cp = BN.residual(); bp = add_bck_ops(cp)
        params = BN.res_params(cp, seed); data, label = BN.res_inputs(cp, seed)
        drv = ConvPipeBck(cpu, bn_maf=0.9, grad_operands=mode); drv.init(bp, params)
        try:
            fwd = {"data": data, "label": label}
            drv.run_bck(["data", "label"], fwd, grad_nodes(bp) + ["loss"] + _fwd_nodes(bp))
            if mode:
                _check_calls(drv, bp)
            out[mode] = fwd
        finally:
            drv.release()
    want = BN.net_bn_f64(cp, params, data, label)
    for n in _fwd_nodes(bp) + ["loss"]:
        assert R.same_bits(out["bf16"][n], out[""][n]), n
    for n in grad_nodes(bp):
        if "_split_" in n or float(np.max(np.abs(want[n]))) < 1e-12:    # (a partial gradient; a bias in front of a BatchNorm: exact gradient 0)
            continue
        assert np.all(np.isfinite(out["bf16"][n])), n
        print(f"E_cpu residual {n}: bf16 {ref.rel_err(out['bf16'][n], want[n]):.3e} (fp32 {ref.rel_err(out[''][n], want[n]):.3e})")


# ---- the pre-specialisation fixture
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops", "bconv-bf16-ops.txt")


def fixture_lines(cpu):
    """The flagged function ops tests/test_gpu_bconv_bf16.py runs: its single calls, and the flagged calls of its pipes' steps (found by a dry init on be=cpu)."""
    fops = R.single_call_fops()
    runs = [(PIPES[n][0], PIPES[n][1], {}) for n in sorted(PIPES)] + [(PIPES["fan"][0], PIPES["fan"][1], {"fuse_relu_grad": True}), (BN.residual, None, {"bn_maf": 0.9})]
    for mk, tops, kw in runs:
        cp = mk(); bp = add_bck_ops(cp, loss_tops=tops) if tops else add_bck_ops(cp)
        drv = ConvPipeBck(cpu, grad_operands="bf16", **kw); drv.init(bp)
        try:
            fops += [f for _, f, _ in drv.calls() if has_bf16_operands(f)]
        finally:
            drv.release()
    lines = []
    for f in fops:
        if f.to_str() not in lines:
            lines.append(f.to_str())
    return lines


def test_fixture_file_lists_these_ops(cpu):
    """tests/golden/ops/bconv-bf16-ops.txt is what the build pre-specialises; it must list exactly the ops above (write fixture_lines(cpu) to it when they change)."""
    lines = fixture_lines(cpu)
    assert [l for l in open(FIXTURE).read().splitlines() if l and not l.startswith("#")] == lines
    assert all(has_bf16_operands(o) for o in read_ops(FIXTURE)) and len(lines) >= 60
