"""Seeded random-geometry sweeps of the backward kernels on the MI355X: kernels/bconv_in_f32.hip, bconv_filts_f32.hip, the twelve functions of bck_ops_f32.hip and the
-DZINP=1 forms, on the cases of tools/fuzz_bck.py under the seed table of tests/test_bck_fuzz_cpu.py (which holds the checkers to their bounds on these very cases).

Every case compares a HIP kernel with its bit-exact twin (be=cpu, oracle/bck_chain.py's emulation of the launch's own K slices, the numpy restatements) AND with float64
under the bound the function already has (tests/test_gpu_bck_conv.py, tests/test_gpu_bck_ops.py); every output var is filled with NaN before the launch, and every launch
must be the function's own kernel.  The check_*_case functions are also what tools/fuzz_bck.py runs, in volume.

Every random geometry is a fresh hiprtc specialisation, so the counts are small on purpose (12 per parameter / family).  Measured on one MI355X (pytest --durations):
no run recorded yet."""
import numpy as np
import pytest

import bck_ops_ref as oref
import bck_pipe_ref as pref
from boda_amd.cnn_op import OpTune, add_bck_conv_annotations, add_bck_op_annotations, fuse_zero_if_in_non_pos
from boda_amd.rtc import make_rtc
from oracle import bck_chain as bc

from test_bck_conv_cpu import FILTS_MRD, bck_op, rand_ins, torch_grads
from test_bck_fuse_cpu import bits, then_zinp
from test_bck_fuzz_cpu import (FTILES, IN_TILES, MULTI, OPS_SEEDS, ZINP_TILES, concat_inputs, concat_round_trip, conv_data_seed, conv_list, conv_zinp_ins, flat_case_cpu, flat_reduce_inputs, frac_of,
                               lrn_funcs, lrn_input, lrn_zinp_in, multi_list, ops_list, pool_funcs, pool_input, softmax_input, zinp_in)
from test_bck_ops_cpu import softmax_op
from test_bck_pipe_cpu import ann, reduce_op, run_func
from test_gpu_bck_fuse import flagged_run
from test_gpu_bck_pipe import gpu

pytestmark = pytest.mark.gpu
WORST = {}   # bound name -> largest observed fraction of it
USED = {}    # "kernel cfg" -> launches


class Mismatch(AssertionError):
    """A failed compare: what was compared, the launch's kernel cfg, how many of how many elements differ."""
    def __init__(self, what, case, cfg, count, size):
        super().__init__(f"{what}: {count} of {size} elements differ, case {case}, launch {cfg}")
        self.what, self.case, self.cfg, self.count, self.size = what, case, cfg, count, size


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


def launch_cfg(hip):
    l = hip.last_launch()
    key = l["kernel"].replace("bodahip_", "") + " " + l.get("cfg", "")
    USED[key] = USED.get(key, 0) + 1
    return key


def same_bits(what, case, cfg, got, want):
    g, w = bits(got), bits(want)
    if g.shape != w.shape:
        raise Mismatch(what + f" (shape {g.shape} against {w.shape})", case, cfg, g.size, w.size)
    if not np.array_equal(g, w):
        raise Mismatch(what, case, cfg, int((g != w).sum()), w.size)


def under(name, case, cfg, frac):
    WORST[name] = max(WORST.get(name, 0.0), frac)
    if not frac <= 1.0:
        raise Mismatch(f"{name}: {frac:.3g} of the bound", case, cfg, 1, 1)


def within(name, case, cfg, got, want, bound):
    """Per element |got - want| <= bound (float64 want); NaN fails."""
    err = np.abs(np.asarray(got, np.float64) - want) / np.maximum(bound, 1e-300)
    frac = float(np.max(np.where(np.isnan(err), np.inf, err)))
    WORST[name] = max(WORST.get(name, 0.0), frac)
    if not frac <= 1.0:
        raise Mismatch(f"{name}: {frac:.3g} of the bound", case, cfg, int((~(err <= 1.0)).sum()), err.size)


def tile_cfg(tile):
    """The start of the launch's configuration string (BIxBJxBK_wWIxWJ...) under a forced tile BIxBJxBKxWIxWJ[x...]."""
    f = tile.split("x")
    return "x".join(f[:3]) + "_w" + "x".join(f[3:5])


def nan_like(fop, an):
    return np.full(tuple(fop.get_dims(an).sizes), np.nan, np.float32)


# ---- BckConv
def check_bconv_in(hip, cpu, case, seed, tile=""):
    op = bck_op(*case)
    ins = rand_ins(op, seed)
    fi = add_bck_conv_annotations(op, OpTune(hip_tile=tile))[0]
    got = gpu(hip, fi, dict(ins, in_grad_loss=nan_like(fi, "in_grad_loss")))["in_grad_loss"]
    cfg = launch_cfg(hip)
    if tile:
        assert cfg.split()[1].startswith(tile_cfg(tile)), (tile, cfg)
    same_bits("in_grad_loss against be=cpu", case, cfg, got, run_func(cpu, fi, ins)["in_grad_loss"])
    ti, _, _ = torch_grads(op, ins["in"], ins["filts"], ins["out_grad_loss"])
    under("in_grad_loss mrd 2e-4", case, cfg, frac_of(got, ti, 2e-4))


def check_bconv_filts(hip, cpu, case, seed, ftile=""):
    op = bck_op(*case)
    ins = rand_ins(op, seed)
    _, fb, ff = add_bck_conv_annotations(op, OpTune())
    if ftile:
        ff.str_vals["hip_tile"] = ftile
    got = gpu(hip, ff, dict(ins, filts_grad_loss=nan_like(ff, "filts_grad_loss")))["filts_grad_loss"]
    cfg = launch_cfg(hip)
    c = hip.last_launch()["cfg"]
    bk, ksl = int(c.split("_")[0].split("x")[2]), (int(c.split("_s")[1].split("_")[0]) if "_s" in c else 1)   # the launch's own K step and slices
    if ftile:
        assert c.startswith(tile_cfg(ftile)) and ksl == int(ftile.split("x")[6]), (ftile, c)
    I, J = bc.filts_operands(ins["in"], ins["out_grad_loss"], op.bck_conv_geom())
    same_bits(f"filts_grad_loss against the chain of BK={bk}, {ksl} slices", case, cfg, got, bc.filts_sliced_chain(I, J, bk, ksl, got.shape))
    _, tf, tb = torch_grads(op, ins["in"], ins["filts"], ins["out_grad_loss"])
    under("filts_grad_loss FILTS_MRD", case, cfg, frac_of(got, tf, FILTS_MRD))
    gb = gpu(hip, fb, dict(ins, biases_grad_loss=nan_like(fb, "biases_grad_loss")))["biases_grad_loss"]
    same_bits("biases_grad_loss against biases_chain", case, launch_cfg(hip), gb, bc.biases_chain(ins["out_grad_loss"]))
    under("biases_grad_loss FILTS_MRD", case, cfg, frac_of(gb, tb, FILTS_MRD))


def check_flagged(hip, cpu, case, plain, flagged, ins, cpu_twin, tile=""):
    """flagged launch == unflagged launch followed by hip_zero_if_non_pos on the GPU (== the flagged function on be=cpu, where it has a bit-exact twin)."""
    g = gpu(hip, plain, dict(ins, in_grad_loss=nan_like(plain, "in_grad_loss")))["in_grad_loss"]
    want = then_zinp(hip, g, ins["in"])
    got = flagged_run(hip, flagged, ins)
    cfg = launch_cfg(hip)
    if tile:
        assert cfg.split()[1].startswith(tile_cfg(tile)), (tile, cfg)
    same_bits("flagged against unflagged + zero_if_non_pos", case, cfg, got, want)
    same_bits("flagged: +0 under every non-positive condition", case, cfg, got[~(ins["in"] > 0)], np.zeros(int((~(ins["in"] > 0)).sum()), np.float32))
    if cpu_twin:
        same_bits("flagged against flagged be=cpu", case, cfg, got, flagged_run(cpu, flagged, ins, kernel=False))


def check_bconv_zinp(hip, cpu, case, seed, tile=""):
    fi = add_bck_conv_annotations(bck_op(*case), OpTune(hip_tile=tile))[0]
    check_flagged(hip, cpu, case, fi, fuse_zero_if_in_non_pos(fi), conv_zinp_ins(case, seed), True, tile)


def check_conv_case(hip, cpu, case, seed, tile="", ftile=""):
    check_bconv_in(hip, cpu, case, seed, tile)
    check_bconv_filts(hip, cpu, case, seed, ftile)
    check_bconv_zinp(hip, cpu, case, seed, tile)


@pytest.mark.parametrize("tile", list(IN_TILES))
def test_bconv_random_geometries(hip, cpu, tile):
    k = IN_TILES[tile]
    for i, case in enumerate(conv_list(k)):
        check_bconv_in(hip, cpu, case, conv_data_seed(k, i), tile)


@pytest.mark.parametrize("ftile", list(FTILES))
def test_bconv_filts_random_geometries(hip, cpu, ftile):
    k = FTILES[ftile]
    for i, case in enumerate(conv_list(k)):
        check_bconv_filts(hip, cpu, case, conv_data_seed(k, i), ftile)


@pytest.mark.parametrize("tile", list(ZINP_TILES))
def test_bconv_in_zinp_random_geometries(hip, cpu, tile):
    k = ZINP_TILES[tile]
    for i, case in enumerate(conv_list(k)):
        check_bconv_zinp(hip, cpu, case, conv_data_seed(k, i), tile)


# ---- pooling argmax, Spreading
def check_pool_case(hip, cpu, case, i, seed):
    B, C, H, W, kern, stride, pad, avg = case
    fp, fs, ffs = pool_funcs(case)
    x = pool_input(case, i, seed)
    g = gpu(hip, fp, {"in": x, "out": nan_like(fp, "out"), "out_in_yx": nan_like(fp, "out_in_yx")})
    cfg = launch_cfg(hip)
    c = run_func(cpu, fp, {"in": x})
    same_bits("pool_yx out", case, cfg, g["out"], c["out"]); same_bits("pool_yx out_in_yx", case, cfg, g["out_in_yx"], c["out_in_yx"])
    ogl = np.random.default_rng([seed, 7]).uniform(-2, 2, c["out"].shape).astype(np.float32)
    ins = {"out": c["out"], "out_grad_loss": ogl, "out_in_yx": c["out_in_yx"], "in": zinp_in(x.shape, seed)}
    got = gpu(hip, fs, dict(ins, in_grad_loss=nan_like(fs, "in_grad_loss")))["in_grad_loss"]
    cfg = launch_cfg(hip)
    same_bits("spreading against be=cpu", case, cfg, got, run_func(cpu, fs, ins)["in_grad_loss"])
    same_bits("spreading against numpy", case, cfg, got, oref.spreading_f32(ogl, c["out_in_yx"], (H, W), kern, stride, pad, avg))
    check_flagged(hip, cpu, case, fs, ffs, ins, True)


def test_pool_spreading_random(hip, cpu):
    for i, case in enumerate(ops_list("pool")):
        check_pool_case(hip, cpu, case, i, OPS_SEEDS["pool"] + i)


# ---- LRN with scale_base, BckLRN
def check_lrn_case(hip, cpu, case, seed):
    B, C, H, W, ls, alpha, beta, k = case
    fl, fb, ffb = lrn_funcs(case)
    x, ogl = lrn_input(case, seed)
    g = gpu(hip, fl, {"in": x, "out": nan_like(fl, "out"), "out_scale_base": nan_like(fl, "out_scale_base")})
    cfg = launch_cfg(hip)
    c = run_func(cpu, fl, {"in": x})
    same_bits("lrn_sb out_scale_base", case, cfg, g["out_scale_base"], c["out_scale_base"])
    want = oref.lrn_out_f64(x, c["out_scale_base"], beta)
    within("lrn_sb out", case, cfg, g["out"], want, 8 * oref.U * np.abs(want))
    ins = {"in": x, "out": c["out"], "out_grad_loss": ogl, "out_scale_base": c["out_scale_base"]}   # the CPU forward: the backward does not inherit forward error
    igl = gpu(hip, fb, dict(ins, in_grad_loss=nan_like(fb, "in_grad_loss")))["in_grad_loss"]
    cfg = launch_cfg(hip)
    want, S = oref.bck_lrn_f64(x, c["out"], ogl, c["out_scale_base"], ls, alpha, beta, k)
    within("bck_lrn in_grad_loss", case, cfg, igl, want, 2 * (ls + 8) * oref.U * S)
    check_flagged(hip, cpu, case, fb, ffb, dict(ins, **{"in": lrn_zinp_in(case, seed)}), False)   # (powf: no bit-exact CPU twin)


def test_lrn_random(hip, cpu):
    for i, case in enumerate(ops_list("lrn")):
        check_lrn_case(hip, cpu, case, OPS_SEEDS["lrn"] + i)


# ---- softmax with loss
def check_softmax_case(hip, cpu, case, seed):
    B, C = case[:2]
    x, lab = softmax_input(case, seed)
    fs, fg, fl = add_bck_op_annotations(softmax_op(B, C), OpTune())
    prob = gpu(hip, fs, {"in": x, "prob": nan_like(fs, "prob")})["prob"]
    cfg = launch_cfg(hip)
    want = oref.softmax_f64(x)
    within("softmax prob", case, cfg, prob, want, (C + 8) * oref.U * want)
    cprob = run_func(cpu, fs, {"in": x})["prob"]
    g = gpu(hip, fg, {"prob": cprob, "label": lab, "in_grad_loss": nan_like(fg, "in_grad_loss"), "loss_per_pel": nan_like(fg, "loss_per_pel")})
    cfg = launch_cfg(hip)
    c = run_func(cpu, fg, {"prob": cprob, "label": lab})
    same_bits("sm_grad_and_loss in_grad_loss", case, cfg, g["in_grad_loss"], c["in_grad_loss"])
    wl = oref.loss_per_pel_f64(cprob, lab)
    within("loss_per_pel", case, cfg, g["loss_per_pel"], wl, 4 * oref.U * np.maximum(1.0, np.abs(wl)))
    loss = gpu(hip, fl, {"loss_per_pel": c["loss_per_pel"], "loss": nan_like(fl, "loss")})["loss"]
    same_bits("sum_loss_over_imgs", case, launch_cfg(hip), loss, run_func(cpu, fl, {"loss_per_pel": c["loss_per_pel"]})["loss"])


def test_softmax_random(hip, cpu):
    for i, case in enumerate(ops_list("softmax")):
        check_softmax_case(hip, cpu, case, OPS_SEEDS["softmax"] + i)


# ---- zero_if_non_pos, reduce, dropout; concat / split
def check_flat_case(hip, cpu, case, seed):
    flat_case_cpu(hip, case, seed, run=gpu)   # against the numpy restatements, every launch the function's own kernel ...
    launch_cfg(hip)
    size, nin, ratio = case                   # ... and reduce against be=cpu as well
    xs = flat_reduce_inputs(nin, size, seed); f = ann(reduce_op(nin, f"(dims=(v={size}))"))[0]
    ins = {f"ins_{j}": v for j, v in enumerate(xs)}
    same_bits("reduce against be=cpu", case, "reduce", gpu(hip, f, ins)["out"], run_func(cpu, f, ins)["out"])


def check_concat_case(hip, cpu, case, seed):
    wide = concat_round_trip(hip, case, seed, run=gpu)
    same_bits("concat against be=cpu", case, launch_cfg(hip), wide, concat_round_trip(cpu, case, seed))
    same_bits("concat against numpy", case, "concat", wide, pref.concat_f32(concat_inputs(case, seed)))


def test_flat_random(hip, cpu):
    for i, case in enumerate(ops_list("flat")):
        check_flat_case(hip, cpu, case, OPS_SEEDS["flat"] + i)


def test_concat_split_random(hip, cpu):
    for i, case in enumerate(ops_list("concat")):
        check_concat_case(hip, cpu, case, OPS_SEEDS["concat"] + i)


# ---- several devices
def test_multi_device_random(hip):
    """devices=0:0: the images of each case shared out between two backends on one GPU; the sharded result equals one device bit for bit."""
    r = make_rtc("(be=hip,devices=0:0)")
    r.init()
    try:
        for i, case in enumerate(multi_list("conv")):
            ins = rand_ins(bck_op(*case), 9000 + i)
            fi = add_bck_conv_annotations(bck_op(*case), OpTune())[0]
            pre = dict(ins, in_grad_loss=nan_like(fi, "in_grad_loss"))
            same_bits("devices=0:0 bconv_in", case, "", run_func(r, fi, pre)["in_grad_loss"], gpu(hip, fi, pre)["in_grad_loss"])
        for i, case in enumerate(multi_list("pool")):
            seed = MULTI["pool"][1] + i
            fp, fs, _ = pool_funcs(case)
            one = gpu(hip, fp, {"in": pool_input(case, i, seed)})
            ogl = np.random.default_rng([seed, 7]).uniform(-2, 2, one["out"].shape).astype(np.float32)
            pre = {"out": one["out"], "out_grad_loss": ogl, "out_in_yx": one["out_in_yx"], "in_grad_loss": nan_like(fs, "in_grad_loss")}
            same_bits("devices=0:0 spreading", case, "", run_func(r, fs, pre)["in_grad_loss"], gpu(hip, fs, pre)["in_grad_loss"])
        for i, case in enumerate(multi_list("lrn")):
            fl, fb, _ = lrn_funcs(case)
            x, ogl = lrn_input(case, MULTI["lrn"][1] + i)
            one = gpu(hip, fl, {"in": x})
            pre = {"in": x, "out": one["out"], "out_grad_loss": ogl, "out_scale_base": one["out_scale_base"], "in_grad_loss": nan_like(fb, "in_grad_loss")}
            same_bits("devices=0:0 bck_lrn", case, "", run_func(r, fb, pre)["in_grad_loss"], gpu(hip, fb, pre)["in_grad_loss"])
        for i, (size, nin, _) in enumerate(multi_list("flat")):   # reduce on img:chan:y:x tensors of B = 2 .. 5 images
            B = 2 + i % 4 + 2 * (i // 4 % 2)
            d = f"(dims=(img={B},chan=3,y={1 + size % 7},x={1 + size % 5}))"
            n = B * 3 * (1 + size % 7) * (1 + size % 5)
            xs = [x.reshape(B, 3, 1 + size % 7, 1 + size % 5) for x in flat_reduce_inputs(nin, n, MULTI["flat"][1] + i)]
            f = ann(reduce_op(nin, d))[0]; pre = dict({f"ins_{j}": x for j, x in enumerate(xs)}, out=np.full(xs[0].shape, np.nan, np.float32))
            same_bits("devices=0:0 reduce", (B, size, nin), "", run_func(r, f, pre)["out"], gpu(hip, f, pre)["out"])
        for i, case in enumerate(multi_list("concat")):
            seed = MULTI["concat"][1] + i
            same_bits("devices=0:0 concat / split", case, "", concat_round_trip(r, case, seed), concat_round_trip(hip, case, seed, run=gpu))
    finally:
        r.close()


def test_zz_report_worst_fractions_of_the_bounds():
    """Not a check of its own: prints what the sweeps above measured (run with -s) and the kernels / tile configs they launched."""
    for name in sorted(WORST):
        print(f"largest observed fraction of the bound, {name}: {WORST[name]:.3f}")
    print("kernels / tile configs used:", dict(sorted(USED.items(), key=lambda kv: -kv[1])))
    assert all(v <= 1.0 for v in WORST.values())
