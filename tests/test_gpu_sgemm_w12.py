"""The staging-wave sgemm kernel's forms of twelve multiplying waves (kernels/sgemm_big_f32.hip: 4 x 3 | 3 x 4 waves of 64 x 64 on a 256 x 192 | 192 x 256 tile, 1024 threads),
forced by tile string with two and four K tiles in flight and three and four LDS stages (the eleventh field).  Every output is one ascending-k fma chain in one lane:
bit-identical to the oracle and to the general kernel."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fwd_special_ref as R
from boda_amd.cnn_op import OpTune, add_codegen_annotations
from boda_amd.op import UnsupErr, parse_op
from boda_amd.ops_prof import OpsBackend, profile_rcg_call
from boda_amd.rtc import make_rtc
from oracle import boda_oracle as bo

GENERAL = "128x128x16x2x2x2"
STG64 = "64x64x16x2x2x4x1x32x2x3"
# (M, N, K): one tile, one K step, all padded steps | ragged row and column edges, K tail inside a step | 2 x 2 tiles, K no multiple of 16 | K shorter than a step |
# partial last tiles both ways and more than eight tiles (the XCD-banded map's rr != 0 branch)
SHAPES = [(256, 192, 16), (260, 196, 40), (512, 384, 72), (768, 580, 8), (1028, 772, 136)]
TILES = [f"{form % pf}{nstg}" for form in ("256x192x16x4x3x4x1x32x%dx3", "192x256x16x3x4x4x1x32x%dx3") for pf in (2, 4) for nstg in ("", "x3")]   # ("": four stages)


@pytest.fixture(scope="module")
def be():
    rtc = make_rtc("(be=hip)", 0)
    rtc.init()
    b = OpsBackend(rtc)
    yield b
    rtc.finish_and_sync()


def _op(M, N, K):
    return parse_op(f"(str_vals=(type=sgemm),nda_vals=(a=(dims=(K={K},M={M})),b=(dims=(K={K},N={N})),c=(dims=(M={M},N={N}))))")


def _run(be, shape, tile):
    return profile_rcg_call(be, add_codegen_annotations(_op(*shape), OpTune(hip_tile=tile)), 5, 0.0, 1, include_ins=True, tile=tile)


_REF = {}


def _ref(be, shape):
    """Per shape, once: the oracle's c on the mode-5 operands and the general kernel's."""
    if shape not in _REF:
        outs, prc = _run(be, shape, GENERAL)
        assert prc.launch["kernel"] == "bodahip_sgemm_f32", prc.launch
        want = bo.sgemm(outs["a"], outs["b"])
        for v in (want, outs["c"]): v.setflags(write=False)
        _REF[shape] = (want, outs["c"])
    return _REF[shape]


@pytest.mark.parametrize("tile", TILES)
def test_w12_forms_bit_exact(be, tile):
    bi, bj = (int(x) for x in tile.split("x")[:2])
    for shape in SHAPES:
        want, general = _ref(be, shape)
        outs, prc = _run(be, shape, tile)
        what = (shape, tile, prc.launch)
        assert prc.launch["kernel"] == "bodahip_sgemm_big_f32" and prc.launch["block"] == 1024 and prc.launch["cfg"].startswith(f"{bi}x{bj}x16_") and prc.launch["cfg"].endswith("_stg"), what
        assert prc.launch["grid"] == -(-shape[0] // bi) * -(-shape[1] // bj), what
        assert np.array_equal(want, outs["c"]), what
        assert np.array_equal(general, outs["c"]), what


@pytest.mark.parametrize("tile", [TILES[0], TILES[5]])
def test_w12_nan_filled_output(be, tile):
    """c prefilled with a payload NaN, a guard var behind every var: every element of c is stored, nothing past the ragged edges is (dropped edge stores leave nothing
    written), the operands read back unchanged; wide-range data against the oracle."""
    geom = (260, 196, 40)
    res = R.run_sgemm(be.rtc, geom, {"wide": R.sgemm_data("wide", geom)}, tile=tile)["wide"]
    what = (geom, tile, res["launch"])
    assert res["launch"]["kernel"] == "bodahip_sgemm_big_f32" and res["launch"]["block"] == 1024, what
    R.assert_no_poison(res["c"], what)
    R.assert_same(R.sgemm_want("wide", geom), res["c"], what)


def test_w12_parts_against_single_launch(be):
    """1536^3 cut into rectangles of the new forms (and a corner on 64 x 64 tiles) through BODAHIP_SGEMM_PARTS == the planner's own launch == the oracle."""
    shape = (1536, 1536, 1536)
    op = add_codegen_annotations(_op(*shape), OpTune())
    single, prc1 = profile_rcg_call(be, op, 5, 0.0, 1, include_ins=True)
    parts = f"1536:0,768,0,1536,{TILES[0]}/768,768,0,768,{TILES[4]}/768,768,768,768,{STG64}"
    os.environ["BODAHIP_SGEMM_PARTS"] = parts
    try: cut, prc = profile_rcg_call(be, op, 5, 0.0, 1)
    finally: del os.environ["BODAHIP_SGEMM_PARTS"]
    assert prc.launch["kernel"] == "bodahip_sgemm_big_f32" and prc.launch["block"] == 1024 and prc.launch["grid"] == 3 * 8 + 4 * 3 + 12 * 12, prc.launch
    assert prc1.launch["grid"] != prc.launch["grid"], prc1.launch
    assert np.array_equal(single["c"], cut["c"])
    assert np.array_equal(bo.sgemm(single["a"], single["b"]), cut["c"])


def test_w12_malformed_tiles_unsupported(be):
    for tile in ("256x192x8x4x3x4x1x32x2x3", "320x192x16x5x3x4x1x32x2x3", "256x192x32x4x3x4x1x32x2x3", "256x192x16x4x3x4x1x32x2x3x5"):
        with pytest.raises(UnsupErr):
            _run(be, (260, 196, 40), tile)
