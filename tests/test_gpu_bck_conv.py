"""BckConv on the MI355X: the native gradient kernels (kernels/bconv_in_f32.hip, kernels/bconv_filts_f32.hip) on the reference's test pattern (gen_data mode 5).
  * in_grad_loss: BIT-IDENTICAL to be=cpu (the reference template's fma chain, out_chan / out_x / out_y order)
  * filts_grad_loss / biases_grad_loss: within FILTS_MRD of float64, and the same bits run to run and across tiles with the same K-slice count
mrd = max|x - r| / max|r| over the tensor (r = float64)."""

import numpy as np
import pytest

from boda_amd.cnn_op import OpTune, add_bck_conv_annotations
from boda_amd.op import UnsupErr, read_ops
from boda_amd.ops_prof import OpsBackend, profile_rcg_call
from boda_amd.rtc import make_rtc

from test_bck_conv_cpu import GOLD, FILTS_MRD, bck_op, mrd, run_func, torch_grads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    r = make_rtc("(be=hip)", 0)
    r.init()
    yield OpsBackend(r)
    r.close()


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


def gpu_grads(be, op, tile="", runs=1, ftile=""):
    """-> ({in, filts, out_grad_loss}, in_grad_loss, filts_grad_loss, biases_grad_loss) from the GPU (mode-5 inputs generated on the device); `tile` forces the
    data gradient's tile, `ftile` the filter gradient's."""
    fi, fb, ff = add_bck_conv_annotations(op, OpTune())
    for f, t in ((fi, tile), (ff, ftile)):
        if t:
            f.str_vals["hip_tile"] = t
    o_in, prc = profile_rcg_call(be, fi, 5, include_ins=True)
    assert prc.launch["kernel"] == "bodahip_bconv_in"
    o_f, prc = profile_rcg_call(be, ff, 5, include_ins=True, run_iter=runs)
    assert prc.launch["kernel"] == "bodahip_bconv_filts"
    o_b, prc = profile_rcg_call(be, fb, 5, include_ins=True)
    assert np.array_equal(o_in["out_grad_loss"], o_f["out_grad_loss"]) and np.array_equal(o_b["out_grad_loss"], o_f["out_grad_loss"])
    ins = {"in": o_f["in"], "filts": o_in["filts"], "out_grad_loss": o_f["out_grad_loss"]}
    return ins, o_in["in_grad_loss"], o_f["filts_grad_loss"], o_b["biases_grad_loss"]


def check_op(hip, cpu, op):
    ins, gi, gf, gb = gpu_grads(hip, op)
    fi, _, _ = add_bck_conv_annotations(op, OpTune())
    want = run_func(cpu, fi, ins)
    assert np.array_equal(gi.view(np.uint32), want.view(np.uint32)), f"in_grad_loss not bit-identical to be=cpu: {op.to_str()}"
    ti, tf, tb = torch_grads(op, ins["in"], ins["filts"], ins["out_grad_loss"])
    assert mrd(gi, ti) < 2e-4
    assert mrd(gf, tf) < FILTS_MRD, (mrd(gf, tf), op.to_str())
    assert mrd(gb, tb) < FILTS_MRD, (mrd(gb, tb), op.to_str())


def test_every_fixture_shape(hip, cpu):
    for op in read_ops(GOLD):
        check_op(hip, cpu, op)


EDGE = {   # (B, C, H, W, OC, KH, KW, SY, SX, PY, PX)
    "1x1_s2_stride_gt_kernel": (2, 40, 14, 14, 36, 1, 1, 2, 2, 0, 0),
    "11x11_s4": (2, 3, 67, 67, 40, 11, 11, 4, 4, 0, 0),
    "3x3_s2_k_not_multiple_of_s": (3, 17, 15, 16, 45, 3, 3, 2, 2, 1, 1),
    "5x5_s2_pad3_pad_ge_stride": (2, 9, 13, 13, 20, 5, 5, 2, 2, 3, 3),
    "7x3_s3x2_odd_channels": (1, 5, 19, 11, 33, 7, 3, 3, 2, 2, 1),
    "3x3_s1_img1_chan_not_32": (1, 70, 9, 9, 100, 3, 3, 1, 1, 1, 1),
}


@pytest.mark.parametrize("name", sorted(EDGE))
def test_edge_geometries(hip, cpu, name):
    check_op(hip, cpu, bck_op(*EDGE[name]))


def test_filts_deterministic_runs_and_tiles(hip):
    op = bck_op(8, 96, 27, 27, 128, 5, 5, 1, 1, 2, 2)
    _, _, f1, b1 = gpu_grads(hip, op, runs=2)
    _, _, f2, b2 = gpu_grads(hip, op)
    assert np.array_equal(f1.view(np.uint32), f2.view(np.uint32)) and np.array_equal(b1.view(np.uint32), b2.view(np.uint32))
    _, _, fa, _ = gpu_grads(hip, op, ftile="128x128x32x2x2x1x4")
    _, _, fb, _ = gpu_grads(hip, op, ftile="64x128x32x2x2x1x4")
    _, _, fc, _ = gpu_grads(hip, op, ftile="32x64x32x1x2x1x4")
    assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)) and np.array_equal(fa.view(np.uint32), fc.view(np.uint32))
    _, _, f1s, _ = gpu_grads(hip, op, ftile="128x128x32x2x2x1x1")   # one slice: a single exact chain, the same bits for any tile
    _, _, f1t, _ = gpu_grads(hip, op, ftile="64x64x16x2x2x1x1")
    assert np.array_equal(f1s.view(np.uint32), f1t.view(np.uint32))


def test_data_gradient_forced_tiles_bit_identical(hip, cpu):
    op = bck_op(3, 70, 13, 13, 50, 3, 3, 2, 2, 1, 1)
    outs = [gpu_grads(hip, op, tile=t)[1] for t in ("", "32x128x16x1x4", "64x64x16x2x2", "128x256x16x2x4")]
    for o in outs[1:]:
        assert np.array_equal(outs[0].view(np.uint32), o.view(np.uint32))


def test_alexnet_conv2_b32_sampled_float64(hip):
    op = bck_op(32, 96, 27, 27, 256, 5, 5, 1, 1, 2, 2)
    ins, gi, gf, gb = gpu_grads(hip, op)
    x, w, g = (ins[a].astype(np.float64) for a in ("in", "filts", "out_grad_loss"))
    xp = np.pad(x, ((0, 0), (0, 0), (2, 2), (2, 2)))
    rng = np.random.default_rng(7)
    scale_f = np.abs(gf).max()
    for _ in range(48):   # filter gradient: sum over img, oy, ox of ogl * the shifted input plane
        oc, c, fy, fx = (int(rng.integers(n)) for n in (256, 96, 5, 5))
        r = float(np.sum(g[:, oc] * xp[:, c, fy:fy + 27, fx:fx + 27]))
        assert abs(gf[oc, c, fy, fx] - r) / scale_f < FILTS_MRD
    gpad = np.pad(g, ((0, 0), (0, 0), (2, 2), (2, 2)))
    scale_i = np.abs(gi).max()
    for _ in range(48):   # data gradient: correlation of ogl with the flipped filter
        b, c, y, xx = (int(rng.integers(n)) for n in (32, 96, 27, 27))
        r = float(np.sum(gpad[b, :, y:y + 5, xx:xx + 5] * w[:, c, ::-1, ::-1]))
        assert abs(gi[b, c, y, xx] - r) / scale_i < 2e-4
    assert mrd(gb, g.sum(axis=(0, 2, 3))) < FILTS_MRD


def test_multi_device(hip):
    op = bck_op(4, 24, 11, 11, 40, 3, 3, 2, 2, 1, 1)
    _, want, _, _ = gpu_grads(hip, op)
    r = make_rtc("(be=hip,devices=0:0)")
    r.init()
    try:
        be = OpsBackend(r)
        fi, fb, ff = add_bck_conv_annotations(op, OpTune())
        o, _ = profile_rcg_call(be, fi, 5)
        assert np.array_equal(o["in_grad_loss"].view(np.uint32), want.view(np.uint32))
        for f in (fb, ff):
            with pytest.raises(UnsupErr):
                profile_rcg_call(be, f, 5)
    finally:
        r.close()
