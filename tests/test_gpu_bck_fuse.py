"""The ReLU gradient folded into the call before it, on the MI355X: bodahip_bconv_in -DZINP=1 (kernels/bconv_in_f32.hip) and bodahip_spreading / bodahip_bck_lrn -DZINP=1
(kernels/bck_ops_f32.hip), and one NiN step of ConvPipeBck(fuse_relu_grad=True).

Everything is compared bit for bit (np.array_equal on the uint32 views): the flagged launch against the unflagged launch followed by hip_zero_if_non_pos on the GPU, the
flagged hip_bconv_in / hip_spreading against the flagged function on be=cpu as well (hip_bck_lrn's powf differs from libm's within its written bound, so it has no bit-exact
CPU twin), devices=0:0 against one device, the fused step against the default step.  in_grad_loss is filled with NaN before every flagged launch.  Shapes, inputs and forced
tiles are those of tests/test_bck_fuse_cpu.py."""
import numpy as np
import pytest

from boda_amd.bck_pipe import ConvPipeBck, add_bck_ops
from boda_amd.cnn_op import pipe_func_args
from boda_amd.conv_pipe import nin_imagenet
from boda_amd.rtc import make_rtc

from test_bck_fuse_cpu import (CONV, LRN_SHAPE, SPREAD, TILES, TILE_SHAPES, bits, bits_eq, check_nonfinite, check_refusals, conv_funcs, conv_ins, lrn_funcs, lrn_ins,
                               nonfinite_cases, spread_funcs, spread_ins, then_zinp)
from test_bck_pipe_cpu import run_func

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


def flagged_run(rtc, flagged, ins, kernel=True):
    """The flagged function with in_grad_loss pre-filled with NaN; on be=hip the launch must be the function's own kernel."""
    keep = [] if kernel else None
    shape = tuple(flagged.get_dims("in_grad_loss").sizes)
    got = run_func(rtc, flagged, dict(ins, in_grad_loss=np.full(shape, np.nan, np.float32)), keep=keep)["in_grad_loss"]
    if kernel:
        assert keep == ["bodahip_" + flagged.get_func_name()[4:]], keep
    return got


def check_on_gpu(hip, cpu, plain, flagged, ins, cpu_twin):
    g = run_func(hip, plain, {k: v for k, v in ins.items() if k in dict(pipe_func_args(plain))})["in_grad_loss"]
    want = then_zinp(hip, g, ins["in"])
    got = flagged_run(hip, flagged, ins)
    assert bits_eq(got, want)
    assert not np.any(np.isnan(got[ins["in"] > 0])) and np.all(bits(got)[~(ins["in"] > 0)] == 0)   # every element written; +0 under every non-positive condition
    if cpu_twin:
        assert bits_eq(got, flagged_run(cpu, flagged, ins, kernel=False))
    return got


# ---- 1. the functions on be=hip
@pytest.mark.parametrize("name", sorted(CONV))
def test_bconv_in(hip, cpu, name):
    got = check_on_gpu(hip, cpu, *conv_funcs(CONV[name]), conv_ins(CONV[name], 11), True)
    if name == "k1s2p0_5x5":
        assert np.all(bits(got[:, :, 1::2, :]) == 0) and np.all(bits(got[:, :, :, 1::2]) == 0)   # the pels no term reaches


@pytest.mark.parametrize("name", sorted(SPREAD))
def test_spreading(hip, cpu, name):
    check_on_gpu(hip, cpu, *spread_funcs(SPREAD[name]), spread_ins(cpu, SPREAD[name], 21), True)


def test_bck_lrn(hip, cpu):
    check_on_gpu(hip, cpu, *lrn_funcs(), lrn_ins(LRN_SHAPE, 31), False)


def test_non_finite_gradient_is_selected_away(hip, cpu):
    for case in nonfinite_cases(cpu):
        check_nonfinite(hip, case)


def test_refusals(hip):
    check_refusals(hip)


# ---- 2. forced tiles: the epilogue's index map
@pytest.mark.parametrize("tile", TILES)
def test_bconv_in_forced_tiles(hip, cpu, tile):
    for name in sorted(TILE_SHAPES):
        plain, flagged = conv_funcs(TILE_SHAPES[name], tile)
        ins = conv_ins(TILE_SHAPES[name], 61)
        check_on_gpu(hip, cpu, plain, flagged, ins, True)
        cfg = hip.last_launch()["cfg"]
        assert cfg.startswith("x".join(tile.split("x")[:3])), (tile, cfg)   # the launch ran the tile asked for


# ---- 3. several devices
def test_multi_device(hip, cpu):
    """devices=0:0: the three images split 1 + 2 between two backends on one GPU; `in` shards like in_grad_loss."""
    r = make_rtc("(be=hip,devices=0:0)")
    r.init()
    try:
        for (plain, flagged), ins in ((conv_funcs(CONV["k3s2p1_7x7"]), conv_ins(CONV["k3s2p1_7x7"], 71)),
                                      (spread_funcs(SPREAD["max_k3s2_partial"]), spread_ins(cpu, SPREAD["max_k3s2_partial"], 72)),
                                      (lrn_funcs(), lrn_ins(LRN_SHAPE, 73))):
            assert bits_eq(flagged_run(r, flagged, ins, kernel=False), flagged_run(hip, flagged, ins)), flagged.get_func_name()
    finally:
        r.close()


# ---- 4. one real net
def test_nin_two_images_fused_equals_default(hip):
    cp = nin_imagenet(2); bp = add_bck_ops(cp)
    rng = np.random.default_rng(0)
    data = rng.uniform(-1, 1, cp.nodes["data"].sizes).astype(np.float32)
    label = np.array([3, 998], np.float32).reshape(2, 1, 1)
    # cccp7_grad_loss is written by a data gradient, cccp6_grad_loss by a max Spreading, cccp8_grad_loss by the average Spreading: the producer kinds NiN has (no LRN)
    gets = ["loss", "data_grad_loss", "conv1_filts_grad_loss", "cccp8_biases_grad_loss", "cccp7_grad_loss", "cccp6_grad_loss", "cccp8_grad_loss", "conv1_grad_loss"]
    res = {}
    for fuse in (False, True):
        drv = ConvPipeBck(hip, fuse_relu_grad=fuse); drv.init(bp)
        try:
            drv.set_det_drop_seed(5)
            fwd = {"data": data, "label": label}
            drv.run_bck(["data", "label"], fwd, gets)
            res[fuse] = (fwd, [(t, f.get_func_name()) for t, f, _ in drv.calls()], dict(drv.fused_relu_grads))
        finally:
            drv.release()
    relus = sorted(o.tag for o in bp.bck_ops() if o.type == "ZeroIfNonPos")
    assert len(relus) == 12 and sorted(res[True][2]["folded"]) == relus and res[True][2]["unfolded"] == {}
    assert res[False][2]["folded"] == [] and sorted(res[False][2]["unfolded"]) == relus
    assert res[True][1] == [c for c in res[False][1] if c[1] != "hip_zero_if_non_pos"] and len(res[False][1]) - len(res[True][1]) == 12
    for n in gets:
        assert bits_eq(res[True][0][n], res[False][0][n]), n
    assert np.isfinite(res[True][0]["loss"]).all() and np.any(res[True][0]["data_grad_loss"] != 0) and np.any(res[True][0]["cccp7_grad_loss"] == 0)
