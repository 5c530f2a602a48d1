"""The exact-chain emulator of the BckConv gradient kernels (oracle/bck_chain.py) against be=cpu and float64, without a GPU.

The GPU tests (tests/test_gpu_bck_chain.py) hold the kernels to this emulator bit for bit, so it is checked here first, by an independent construction:
  * one slice, any K step: filts_sliced_chain equals be=cpu's hip_bconv_filts (the reference template's loop) BIT FOR BIT
  * in_grad_chain equals be=cpu's hip_bconv_in BIT FOR BIT -- which also pins the oracle the GPU data gradient is held to
  * biases_chain and the sliced chains (a different association) are within FILTS_MRD of float64
on the SMALL shapes, the EDGE geometries and every recorded fixture op, with host-supplied random data."""
import numpy as np
import pytest

from boda_amd.cnn_op import OpTune, add_bck_conv_annotations
from boda_amd.op import read_ops

from oracle import bck_chain as bc

from test_bck_conv_cpu import GOLD, FILTS_MRD, SMALL, bck_op, cpu, mrd, rand_ins, run_func, torch_grads   # noqa: F401 (cpu: the module's be=cpu fixture)
from test_gpu_bck_conv import EDGE


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_against_cpu(cpu, op, seed, bks=(32,)):
    """Emulator == be=cpu, bit for bit: the filter gradient as one slice (for every K step in `bks`) and the data gradient."""
    geom = op.bck_conv_geom()
    ins = rand_ins(op, seed)
    fi, _, ff = add_bck_conv_annotations(op, OpTune())
    I, J = bc.filts_operands(ins["in"], ins["out_grad_loss"], geom)
    want_f = run_func(cpu, ff, ins)
    for bk in bks:
        got = bc.filts_sliced_chain(I, J, bk, 1, want_f.shape)
        assert np.array_equal(bits(got), bits(want_f)), f"filts chain (BK={bk}, one slice) is not be=cpu's bits: {op.to_str()}"
    want_i = run_func(cpu, fi, ins)
    got = bc.in_grad_chain(ins["filts"], ins["out_grad_loss"], geom)
    assert np.array_equal(bits(got), bits(want_i)), f"in_grad chain is not be=cpu's bits: {op.to_str()}"
    return ins, I, J


def check_against_float64(op, ins, I, J, plans):
    """biases_chain and the sliced filter chains (BK, KSL > 1) against torch float64: the existing bound, unchanged."""
    _, tf, tb = torch_grads(op, ins["in"], ins["filts"], ins["out_grad_loss"])
    assert mrd(bc.biases_chain(ins["out_grad_loss"]), tb) < FILTS_MRD, op.to_str()
    for bk, ksl in plans:
        got = bc.filts_sliced_chain(I, J, bk, ksl, tf.shape)
        assert mrd(got, tf) < FILTS_MRD, (bk, ksl, op.to_str())


@pytest.mark.parametrize("shape", SMALL)
def test_small_shapes_equal_cpu_bits(cpu, shape):
    op = bck_op(*shape)
    ins, I, J = check_against_cpu(cpu, op, sum(shape) + 1, bks=(2, 8, 16, 32, 64, 1 << 20))
    check_against_float64(op, ins, I, J, ((32, 2), (16, 3), (32, 4), (8, 32)))


@pytest.mark.parametrize("name", sorted(EDGE))
def test_edge_geometries_equal_cpu_bits(cpu, name):
    op = bck_op(*EDGE[name])
    ins, I, J = check_against_cpu(cpu, op, len(name), bks=(8, 16, 32, 64))
    check_against_float64(op, ins, I, J, ((32, 2), (16, 3), (32, 4), (64, 7), (16, 32)))


@pytest.mark.slow
def test_every_fixture_op_equals_cpu_bits(cpu):
    ops = read_ops(GOLD)
    assert len(ops) >= 90
    for k, op in enumerate(ops):
        ins, I, J = check_against_cpu(cpu, op, 1000 + k)
        check_against_float64(op, ins, I, J, ((32, 4),))


def test_slices_cover_k_once_in_order():
    """filts_slices: the slices tile [0, K) in ascending order without gap or overlap; K < BK and KSL * kt_per > nkt leave empty slices at the end."""
    for K in (1, 9, 31, 32, 33, 300, 338, 1050, 16245):
        for bk in (8, 16, 32, 64):
            for ksl in (1, 2, 3, 4, 7, 17, 32):
                sl = bc.filts_slices(K, bk, ksl)
                assert len(sl) == ksl and sl[0][0] == 0 and max(k1 for _, k1 in sl) == K
                assert all(a[1] == b[0] or b[0] == b[1] == K for a, b in zip(sl, sl[1:]))
                assert all(k0 <= k1 and (k0 % bk == 0 or k0 == K) for k0, k1 in sl)
    assert bc.filts_slices(9, 32, 4) == [(0, 9), (9, 9), (9, 9), (9, 9)]
    assert bc.filts_slices(338, 32, 3) == [(0, 128), (128, 256), (256, 338)]
    sl = bc.filts_slices(1050, 32, 32)   # nkt = 33, kt_per = 2: slice 16 holds the last K step, 17..31 are empty
    assert sl[16] == (1024, 1050) and all(s == (1050, 1050) for s in sl[17:])


def test_slicing_changes_the_bits():
    """A constructed case that tells the slice plans apart: K = 4, two K steps of 2.  One chain: ((2^24 + 1) + 1) - 2^24 = 0 (each +1 is rounded away); two slices:
    (2^24 + 1) + (1 - 2^24) = 2^24 + (1 - 2^24) = 1.  So a test that compares a sliced launch with the one-slice chain (or the other way round) fails."""
    I = np.array([[2.0 ** 24], [1.0], [1.0], [-(2.0 ** 24)]], np.float32)   # [K = 4, OC = 1]
    J = np.ones((4, 1), np.float32)
    one = bc.filts_sliced_chain(I, J, 2, 1)
    two = bc.filts_sliced_chain(I, J, 2, 2)
    assert one.shape == two.shape == (1, 1)
    assert one[0, 0] == 0.0 and two[0, 0] == 1.0
    assert not np.array_equal(bits(one), bits(two))
    # and on plain random data: the K steps per slice, not the slice count alone, fix the association (kt_per * BK = 128 against 112)
    op = bck_op(3, 5, 10, 10, 7, 3, 3, 1, 1, 1, 1)   # K = 300
    ins = rand_ins(op, 5)
    I, J = bc.filts_operands(ins["in"], ins["out_grad_loss"], op.bck_conv_geom())
    assert bc.filts_slices(300, 32, 3) != bc.filts_slices(300, 16, 3)
    assert not np.array_equal(bits(bc.filts_sliced_chain(I, J, 32, 3)), bits(bc.filts_sliced_chain(I, J, 16, 3)))
    assert not np.array_equal(bits(bc.filts_sliced_chain(I, J, 32, 1)), bits(bc.filts_sliced_chain(I, J, 32, 3)))


def test_operands_are_plain_gathers():
    """filts_operands against the definition, element by element, on a strided, padded, non-square case."""
    op = bck_op(2, 3, 9, 7, 4, 3, 2, 2, 3, 2, 1)
    g = op.bck_conv_geom()
    ins = rand_ins(op, 3)
    I, J = bc.filts_operands(ins["in"], ins["out_grad_loss"], g)
    assert I.shape == (g["B"] * g["OH"] * g["OW"], g["OC"]) and J.shape == (I.shape[0], g["C"] * g["KH"] * g["KW"])
    n_zero = 0
    for k in range(I.shape[0]):
        img, pel = divmod(k, g["OH"] * g["OW"]); oy, ox = divmod(pel, g["OW"])
        assert np.array_equal(I[k], ins["out_grad_loss"][img, :, oy, ox])
        for j in range(J.shape[1]):
            c, f = divmod(j, g["KH"] * g["KW"]); fy, fx = divmod(f, g["KW"])
            iy, ix = oy * g["SY"] - g["PY"] + fy, ox * g["SX"] - g["PX"] + fx
            inside = 0 <= iy < g["H"] and 0 <= ix < g["W"]
            n_zero += not inside
            assert bits(J[k, j]) == (bits(ins["in"][img, c, iy, ix]) if inside else 0)
    assert n_zero > 0


def test_biases_chain_order():
    """The bias chain follows the kernel's order, not a plain running sum: 2^24 at flat index 0 and ones at 256 and 512 land in thread 0's chain and are rounded away
    there; the same ones at 1 and 2 meet in the tree first and survive."""
    g = np.zeros((1, 1, 1, 600), np.float32)
    g[0, 0, 0, 0] = 2.0 ** 24; g[0, 0, 0, 256] = 1.0; g[0, 0, 0, 512] = 1.0
    assert bc.biases_chain(g)[0] == 2.0 ** 24
    g[0, 0, 0, 256] = g[0, 0, 0, 512] = 0.0; g[0, 0, 0, 1] = 1.0; g[0, 0, 0, 3] = 1.0   # red[1] + red[3] = 2 (h = 2), then red[0] + red[1] (h = 1)
    assert bc.biases_chain(g)[0] == 2.0 ** 24 + 2.0
    g2 = np.arange(2 * 3 * 5, dtype=np.float32).reshape(2, 3, 1, 5)   # (img, pel) order across images, per out_chan
    assert np.array_equal(bc.biases_chain(g2), g2.sum(axis=(0, 2, 3)))
