"""The Deconvolution family (kernels/deconv_f32.hip) and hip_crop / hip_crop_bck on the MI355X, held to BITS.
  * hip_deconv, hip_deconv_bck_in and, with one K slice, hip_deconv_bck_filts equal be=cpu, which IS the existing functions on exchanged roles (tests/test_deconv_cpu.py)
  * hip_deconv_bck_filts equals oracle/bck_chain.filts_chain on the exchanged roles with the (BK, KSL) of the launch: the planner's and forced ones -- KSL 1 / 2 / 3 /
    more than the K steps, a BK that does not divide K
  * hip_deconv_bck_biases equals oracle/bck_chain.biases_chain (it is hip_bconv_biases' launch)
  * every output is NaN-filled before the call, a guard var stands in front of and behind every var, inputs keep their bits, two runs give the same bits
  * a NaN in one in_chan's filters and an Inf in `in` at one pel change only what the definition says they change
  * the matrix path (the existing functions on the exchanged roles, bound by role as a driver binds them), on every case whose geometry it takes and as the planner's
    choice on the two wide cases and the 16/8 head: the forward held to oracle/bck_chain.in_grad_chain with the launched BK plus the one bias add, the data gradient to be=cpu (hip_conv
    is exact), the filter gradient to filts_chain with the launched BK / KSL
Every case runs both forced paths where both can run; the direct tests force the direct forms (deconv_ref.deconv_funcs)."""
import numpy as np
import pytest

from boda_amd.cnn_op import OpTune, add_bck_op_annotations
from boda_amd.rtc import make_rtc
from oracle import bck_chain

from deconv_ref import (CASE_IDS, CASES, CROP_CASES, PLANNER_MATRIX, bits_equal, can_matrix, cfg_bk_ksl, crop_ops, deconv_funcs, exchanged_geom, filts_tiles, out_plane,
                        path_calls, rand_ins, run_calls, run_func, torch_twin, within_f64_bound)

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


_REF = {}


def ref(cpu, case, which, ins=None, key=None):
    """be=cpu's function, computed once per (case, function) and shared."""
    k = (case, which, key)
    if k not in _REF:
        _REF[k] = run_func(cpu, deconv_funcs(case)[which], ins if ins is not None else rand_ins(case, 11))[0]
        _REF[k].setflags(write=False)
    return _REF[k]


def plan_of(launch):
    """(BK, KSL) of a launch, from its configuration string BIxBJxBK_wWIxWJ[_sKSL] (tests/test_gpu_bck_chain.py: plan_of)."""
    cfg = launch["cfg"]
    return int(cfg.split("_")[0].split("x")[2]), (int(cfg.split("_s")[1].split("_")[0]) if "_s" in cfg else 1)


def same_with_nans(a, b):
    """Equal NaN positions, equal bits everywhere else."""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_forward_and_data_gradient_bits(hip, cpu, case):
    ins = rand_ins(case, 11)
    funcs = deconv_funcs(case)
    for which, kernel in (("fwd", "bodahip_deconv_direct"), ("in", "bodahip_deconv_bck_in_direct")):
        got, launch = run_func(hip, funcs[which], ins, runs=2, guards=True)
        assert launch["kernel"] == kernel, launch
        assert bits_equal(got, ref(cpu, case, which)), (case, which, launch)
        assert bits_equal(run_func(hip, funcs[which], ins)[0], got)   # the same bits on two runs
    got, launch = run_func(hip, funcs["biases"], ins, guards=True)
    assert launch["kernel"] == "bodahip_bconv_biases" and bits_equal(got, bck_chain.biases_chain(ins["out_grad_loss"])), (case, launch)


def test_unreached_outputs_are_written(hip):
    case = CASES[6]   # 1x1 at stride 2: the odd rows and columns meet no term: +0 + bias, and written (the output was NaN-filled)
    ins = rand_ins(case, 11)
    got, _ = run_func(hip, deconv_funcs(case)["fwd"], ins)
    want = np.broadcast_to((np.float32(0.0) + ins["biases"]).reshape(1, -1, 1, 1), got.shape)
    assert bits_equal(got[:, :, 1::2, :], want[:, :, 1::2, :]) and bits_equal(got[:, :, :, 1::2], want[:, :, :, 1::2])


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_filter_gradient_chain(hip, cpu, case):
    ins = rand_ins(case, 11)
    ff = deconv_funcs(case)["filts"]
    geom = exchanged_geom(case)
    chain = lambda bk, ksl: bck_chain.filts_chain(ins["out_grad_loss"], ins["in"], geom, bk, ksl)   # (in := out_grad_loss, out_grad_loss := in)
    got, launch = run_func(hip, ff, ins, runs=2, guards=True)   # the planner's default, held to the chain with its launched (BK, KSL)
    assert launch["kernel"] == "bodahip_deconv_bck_filts_direct", launch
    BK, KSL = plan_of(launch)
    assert bits_equal(got, chain(BK, KSL)), (case, launch)
    assert bits_equal(run_func(hip, ff, ins)[0], got)
    for tile, bk, ksl in filts_tiles(case):
        got, launch = run_func(hip, ff, ins, tile, guards=True)
        assert plan_of(launch) == (bk, ksl), launch
        assert bits_equal(got, chain(bk, ksl)), (case, bk, ksl)
        if ksl == 1:   # one slice: be=cpu's single chain, for any BK
            assert bits_equal(got, ref(cpu, case, "filts")), (case, bk)


M_CASES = [c for c in CASES if can_matrix(c)]


@pytest.mark.parametrize("case", M_CASES, ids=[CASE_IDS[CASES.index(c)] for c in M_CASES])
def test_matrix_path(hip, cpu, case):
    ins = rand_ins(case, 11)
    geom = exchanged_geom(case)
    OC = case[4]
    for form in ("matrix",) + (("",) if case in PLANNER_MATRIX else ()):   # forced, and -- the wide cases and the 16/8 head -- the planner's own choice
        op, calls = path_calls(case, "fwd", form)
        got, launches = run_calls(hip, op, calls, ins, "fwd", guards=True)
        assert [l["kernel"] for l in launches][1] == "bodahip_chan_affine" and launches[0]["kernel"].startswith("bodahip_bconv_in"), launches
        acc = bck_chain.in_grad_chain(ins["filts"], ins["in"], geom, cfg_bk_ksl(launches[0])[0])   # (filts := the blob as out_chan=C : in_chan=OC, out_grad_loss := in)
        assert bits_equal(got, (acc * np.float32(1.0) + ins["biases"].reshape(1, OC, 1, 1)).astype(np.float32)), (case, form, launches[0])
        assert bits_equal(got, ref(cpu, case, "fwd")), (case, form)   # (finite data without underflow: the chain with +0 operands is be=cpu's chain)
        op, calls = path_calls(case, "in", form)
        got, launches = run_calls(hip, op, calls, ins, "in", guards=True)
        assert not launches[0]["kernel"].startswith("bodahip_deconv"), launches
        assert bits_equal(got, ref(cpu, case, "in")), (case, form, launches[0])
        op, calls = path_calls(case, "filts", form)
        got, launches = run_calls(hip, op, calls, ins, "filts", guards=True)
        assert launches[0]["kernel"].startswith("bodahip_bconv_filts"), launches
        bk, ksl = cfg_bk_ksl(launches[0])
        assert bits_equal(got, bck_chain.filts_chain(ins["out_grad_loss"], ins["in"], geom, bk, ksl)), (case, form, launches[0])
        again, _ = run_calls(hip, op, calls, ins, "filts")
        assert bits_equal(again, got)   # the same bits on two runs


def test_float64(hip):
    """The float64 bound on the longest chains of the list: FCN's 64/32 head in miniature (data gradient: 86016 terms) and the 16/8 head."""
    for case in (CASES[1], CASES[2]):
        ins = rand_ins(case, 11)
        funcs = deconv_funcs(case)
        twin = torch_twin(case, ins)
        for which in ("fwd", "in", "filts"):
            got, launch = run_func(hip, funcs[which], ins)
            assert within_f64_bound(got, twin, case, which, plan_of(launch)[1]), (case, which)


@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[6]], ids=[CASE_IDS[0], CASE_IDS[2], CASE_IDS[6]])
def test_poisoned_operands(hip, cpu, case):
    B, C, H, W, OC, (KH, KW), (SY, SX), (PY, PX) = case
    clean = rand_ins(case, 11)
    f = deconv_funcs(case)["fwd"]
    base, _ = run_func(hip, f, clean)
    # a NaN in one in_chan's filters: every output that meets a term at all meets one of that channel, the others keep +0 + bias -- be=cpu's result, NaN for NaN
    ins = {k: v.copy() for k, v in clean.items()}
    ins["filts"][C - 1] = np.nan
    got, _ = run_func(hip, f, ins)
    assert same_with_nans(got, ref(cpu, case, "fwd", ins, "nan")), case
    reached = np.zeros(got.shape[2:], bool)
    for iy in range(H):
        for ix in range(W):
            y0, x0 = iy * SY - PY, ix * SX - PX
            reached[max(y0, 0):max(y0 + KH, 0), max(x0, 0):max(x0 + KW, 0)] = True
    assert np.all(np.isnan(got[:, :, reached])) and bits_equal(got[:, :, ~reached], base[:, :, ~reached])
    # an Inf in `in` at one pel changes only that pel's kernel window, in its image
    ins = {k: v.copy() for k, v in clean.items()}
    img, iy, ix = B - 1, H // 2, W - 1
    ins["in"][img, 0, iy, ix] = np.inf
    got, _ = run_func(hip, f, ins)
    assert same_with_nans(got, ref(cpu, case, "fwd", ins, "inf")), case
    win = np.zeros(got.shape, bool)
    y0, x0 = iy * SY - PY, ix * SX - PX
    win[img, :, max(y0, 0):max(y0 + KH, 0), max(x0, 0):max(x0 + KW, 0)] = True
    assert bits_equal(got[~win], base[~win]) and np.all(~np.isfinite(got[win]))


@pytest.mark.parametrize("c", CROP_CASES, ids=["x".join(str(v) for v in c) for c in CROP_CASES])
def test_crop(hip, c):
    B, C, H, W, OH, OW, oy, ox = c
    fwd, bck = crop_ops(*c)
    (ff,), (fb,) = add_bck_op_annotations(fwd, OpTune()), add_bck_op_annotations(bck, OpTune())
    rng = np.random.default_rng(3)
    a = rng.uniform(-5, 5, (B, C, H, W)).astype(np.float32)
    g = -np.abs(rng.uniform(0.5, 5, (B, C, OH, OW))).astype(np.float32)   # (all negative: a -0 outside the window would show)
    got, launch = run_func(hip, ff, {"in": a}, runs=2, guards=True)
    assert launch["kernel"] == "bodahip_crop" and bits_equal(got, a[:, :, oy:oy + OH, ox:ox + OW])
    want = np.zeros((B, C, H, W), np.float32); want[:, :, oy:oy + OH, ox:ox + OW] = g
    got, launch = run_func(hip, fb, {"out_grad_loss": g}, runs=2, guards=True)
    assert launch["kernel"] == "bodahip_crop_bck" and bits_equal(got, want)   # the +0 outside the window by bits
