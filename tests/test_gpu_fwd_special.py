"""The forward convolution and sgemm kernels on data and outputs that the other GPU files never give them (-m gpu; DESIGN.md section 3.0, helpers and data classes in
tests/fwd_special_ref.py, the reference side proven on the CPU by tests/test_fwd_special_cpu.py).  One test per launch form: the kernel is compiled once, then run
over every data class and both ReLU settings into an output refilled with a payload NaN before every run -- a conv into channels [2, 2 + OC) of a tensor of OC + 5.
  C1  no output element keeps the poison, the guard channels / guard vars keep it bit for bit, the inputs read back unchanged
  C2  wide / subnormal / overflow: equal to the oracle by value (NaN mask, +-Inf positions and signs, == elsewhere)
  C3  nan_inf: the same; inf_last_chan (the documented exception): non-finite exactly where the oracle is, equal elsewhere; what became of the +Inf is recorded per form
Every test asserts the kernel and the tile it ran, so no case falls back to another form.  The blindness caps are asserted on the oracle's result before a kernel's
result is looked at.  Nothing here reads /root/reference or starts a process."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fwd_special_ref as R
from boda_amd.cnn_op import OpTune, add_codegen_annotations
from boda_amd.digest import SsdsDiff
from boda_amd.rtc import explain_plan, make_rtc
from oracle import boda_oracle as bo

F = np.float32
MRD_REASSOC = 2e-3     # the reference's bound for kernels that re-associate the sum (tests/test_gpu_parity.py: _assert_matches_oracle)
REPORT = {}            # form -> (outputs where the oracle has the +Inf's Inf and the kernel the same Inf, ... and the kernel a NaN), inf_last_chan without ReLU


@pytest.fixture(scope="module")
def rtc():
    r = make_rtc("(be=hip)", 0)
    r.init()
    assert r.get_plat_tag().startswith("hip:")
    yield r
    r.finish_and_sync()
    r.close()


def _caps_first(shape, classes):
    for cls in classes:
        R.assert_caps(cls, R.conv_want(cls, shape, 0), R.whole_input(shape))


def _plan(shape, tile=""):
    return explain_plan(add_codegen_annotations(R.conv_op(*shape), OpTune()), 256, tile)


def _check_conv(form, shape, res, kernel, cfg_re, reassoc=False):
    """What every fp32 conv form is held to (the runner has checked the guards and the inputs)."""
    mask = {c: R.window_mask(shape, R.conv_data(c, shape)["inj"]) for c in ("nan_inf", "inf_last_chan")}
    for (cls, relu), r in res.items():
        what = (form, shape, cls, relu, r["launch"]["kernel"], r["launch"]["cfg"])
        assert r["launch"]["kernel"] == kernel and re.search(cfg_re, r["launch"]["cfg"]), what
        got = r["out"]
        R.assert_no_poison(got, what)
        if cls == "clean":
            continue
        want = R.conv_want(cls, shape, relu)
        if cls == "inf_last_chan":
            # (split-K: the oracle's masks; the finite values are the kernel's own clean run's, below)
            same, nan = R.assert_contained(np.where(np.isfinite(want), got, want) if reassoc else want, got, what, relu=bool(relu))
            if not relu:
                REPORT[form] = (same, nan)
            R.assert_c3_against_clean(res[("clean", relu)]["out"] if reassoc else R.conv_clean(shape, relu), got, mask[cls], what)
        elif not reassoc:
            R.assert_same(want, got, what)
        elif cls == "wide":      # split-K re-associates: the reference's bound for such kernels on the finite class
            sd = SsdsDiff.of(want, got)
            assert not sd.has_nan() and sd.mrd < MRD_REASSOC, (what, sd.basic_str())
        else:                    # nan_inf under split-K: C3 in full -- the oracle's NaN and Inf masks, and the kernel's own clean run everywhere else
            assert cls == "nan_inf"
            assert np.array_equal(np.isnan(want), np.isnan(got)) and np.array_equal(np.isposinf(want), np.isposinf(got)) and np.array_equal(np.isneginf(want), np.isneginf(got)), what
            R.assert_c3_against_clean(res[("clean", relu)]["out"], got, mask[cls], what)


def _data(shape, classes):
    d = {c: R.conv_data(c, shape) for c in classes}
    if "nan_inf" in classes:
        n = R.conv_data("nan_inf", shape)
        d = dict(clean={"in": n["base_in"], "filts": n["filts"], "biases": n["biases"]}, **d)
    return d


T17 = (2, 17, 9, 9, 40, 3, 3, 1, 1)     # K = 153 (a K tail at every K step used), 40 out_chans, 2 x 81 pels: a 64-pel tile straddles the images and the last is ragged; padding
NOP = {"BODAHIP_NO_PATCH": "1", "BODAHIP_NO_ROW_GATHER": "1"}
# (form, shape, conv_tile, environment, kernel, cfg pattern, what the plan's options must hold)
CONV_FORMS = [
    ("default_lds_patch", (4, 20, 8, 8, 100, 3, 3, 1, 1), "", {}, "bodahip_conv_f32", r"^\d+x\d+x\d+_w", "-DJ_MODE=7"),
    ("default_1x1", (3, 4, 9, 9, 33, 1, 1, 1, 0), "", {}, "bodahip_conv_f32", r"^\d+x\d+x\d+_w", "-DJ_MODE=5"),
    ("default_1x1_padded", (2, 8, 7, 7, 16, 1, 1, 1, 1), "", {}, "bodahip_conv_f32", r"^\d+x\d+x\d+_w", "-DJ_MODE=2"),
    ("default_5x5_stride2", (2, 5, 17, 13, 7, 5, 5, 2, 2), "", {}, "bodahip_conv_f32", r"^\d+x\d+x\d+_w", "-DJ_MODE=2"),
    ("default_11x11_stride4", (2, 3, 35, 35, 96, 11, 11, 4, 0), "", {}, "bodahip_conv_f32", r"^\d+x\d+x\d+_w", "-DRDEC=1"),
    ("table_gather", (4, 20, 8, 8, 100, 3, 3, 1, 1), "", NOP, "bodahip_conv_f32", r"^\d+x\d+x\d+_w", "-DJ_MODE=2"),
    ("row_gather", (2, 5, 17, 13, 7, 5, 5, 2, 2), "", {"BODAHIP_ROW_GATHER_MIN_KW": "2"}, "bodahip_conv_f32", r"^\d+x\d+x\d+_w", "-DJ_MODE=6"),
    ("mfma_16x16", T17, "32x64x32x2x2x1x1x16", {}, "bodahip_conv_f32", r"^32x64x32_w2x2_m16$", "-DMT=16"),
    ("two_k_tiles_in_flight", T17, "64x64x16x2x2x2x1x32x2", {}, "bodahip_conv_f32", r"^64x64x\d+_w2x2_p2$", "-DJ_MODE=7"),
    ("staging_waves", T17, "64x64x16x2x2x2x1x32x1x1", {}, "bodahip_conv_f32", r"^64x64x\d+_w2x2_sw$", "-DJ_MODE=7"),
    ("k_hand_off", T17, "64x64x16x2x2x2x1x32x1x0x3", {}, "bodahip_conv_f32", r"^64x64x\d+_w2x2_h3$", "-DKHO=1"),
    ("split_k", T17, "64x64x16x2x2x2x3", {}, "bodahip_conv_f32", r"^64x64x16_w2x2_s3$", "-DSPLITK=1"),
    ("row_decimated_patch", (3, 3, 51, 51, 96, 11, 11, 4, 0), "", {"BODAHIP_RDEC": None}, "bodahip_conv_f32", r"^\d+x\d+x\d+_w", "-DRDEC=1"),
]
# kernels/conv_big_f32.hip: the tile 128x256x32 takes 3 x 3 patch geometries only (its LDS stages at a K step of 32 exceed the CU's for the others: UnsupErr) -- it runs on a
# 3 x 3 shape with the five properties (19 channels against K steps of four, 70 out_chans, 3 x 121 pels against 256-pel tiles that straddle the images, padding); the
# table-gather and 1 x 1 pel forms of the same kernel run on CBIG_SHAPES' 5 x 5 and 1 x 1 members (tests/test_gpu_parity.py), at that tile's K step of 16
CBIG = [("128x256x32x2x4x2x1x32x2x2", (3, 19, 11, 11, 70, 3, 3, 1, 1), "-DJ_MODE=7"), ("128x256x16x2x4x2x1x32x2x2", (4, 17, 9, 9, 70, 5, 5, 1, 2), "-DJ_MODE=2"),
        ("128x256x16x2x4x2x1x32x2x2", (5, 96, 7, 7, 130, 1, 1, 1, 0), "-DJ_MODE=5")]
CONV_FORMS += [(f"staging_wave_kernel_{filt}_{R.sid(s)}", s, t, ({"BODAHIP_CBIG_IVW": "direct"} if filt == "direct" else {"BODAHIP_CBIG_IVW": None}), "bodahip_conv_big_f32",
                r"^128x256x\d+_w2x4_p2_big$", jm) for t, s, jm in CBIG for filt in ("scratch", "direct")]
CONV_FORMS += [("fc_kernel", (3, 31, 4, 4, 65, 4, 4, 1, 0), "", {"BODAHIP_FC": "32x32x32x4"}, "bodahip_fc_f32", r"^32x32x32_", "")]


def _setenv(monkeypatch, env):
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


@pytest.mark.parametrize("form", CONV_FORMS, ids=lambda f: f[0])
def test_conv_form(rtc, form, monkeypatch):
    name, shape, tile, env, kernel, cfg_re, opt = form
    reassoc = name == "split_k"
    classes = ("wide", "nan_inf", "inf_last_chan") if reassoc else R.CLASSES     # (split-K: an overflow or an underflow moves with the association)
    _caps_first(shape, classes)
    _setenv(monkeypatch, env)
    if opt:
        plan = _plan(shape, tile)
        assert opt in plan and kernel in plan, plan
        if "direct" in name:
            assert "-DI_VW=0" not in plan, plan
        elif "scratch" in name:
            assert "-DI_VW=0" in plan, plan
    res = R.run_conv(rtc, shape, _data(shape, classes), tile=tile, wide=not reassoc)     # (a split-K tile refuses a channel slice of a wider output: exact dims, NaN prefill, guard vars)
    _check_conv(name, shape, res, kernel, cfg_re, reassoc)


@pytest.mark.parametrize("spec,kernel", [("2x2x2x2", "bodahip_k1_stream_f32"), ("q4x3x1", "bodahip_k1_quad_f32")])
def test_k1_kernels(rtc, spec, kernel):
    """kernels/k1_stream_f32.hip and k1_quad_f32.hip on the odd-in_chan case of K1S_CASES (tests/test_gpu_parity.py): the new data classes."""
    shape = (5, 33, 13, 13, 70, 1, 1, 1, 0)
    _caps_first(shape, R.CLASSES)
    try:
        res = R.run_conv(rtc, shape, _data(shape, R.CLASSES), before_run=lambda: rtc.set_tune("k1_stream", spec))
    finally:
        rtc.set_tune("k1_stream", "")
    _check_conv(kernel[8:], shape, res, kernel, r".")


# ---- sgemm
SGEMM_FORMS = [("default", (100, 36, 50), "", "bodahip_sgemm_f32", r"."), ("default", (33, 257, 19), "", "bodahip_sgemm_f32", r"."), ("default", (1, 1, 1), "", "bodahip_sgemm_f32", r"."),
               ("256x256", (260, 132, 70), "256x256x16x2x4x1x1x32x2", "bodahip_sgemm_big_f32", r"^256x256x"), ("twelve_waves", (260, 132, 70), "128x128x16x3x4x1", "bodahip_sgemm_big_f32", r"^128x128x16_w3x4"),
               ("four_multiplying_waves", (260, 132, 70), "64x64x16x2x2x4x1x32x2x3", "bodahip_sgemm_big_f32", r"^64x64x16_.*_stg$")]


@pytest.mark.parametrize("form", SGEMM_FORMS, ids=lambda f: f[0] + "_" + R.sid(f[1]))
def test_sgemm_form(rtc, form):
    name, geom, tile, kernel, cfg_re = form
    classes = R.CLASSES[:4]
    for cls in classes:
        R.assert_caps(cls, R.sgemm_want(cls, geom))
    res = R.run_sgemm(rtc, geom, {c: R.sgemm_data(c, geom) for c in classes}, tile=tile)
    for cls, r in res.items():
        what = (name, geom, cls, r["launch"]["kernel"], r["launch"]["cfg"])
        assert r["launch"]["kernel"] == kernel and re.search(cfg_re, r["launch"]["cfg"]), what
        R.assert_no_poison(r["c"], what)
        R.assert_same(R.sgemm_want(cls, geom), r["c"], what)


def test_sgemm_half_storage(rtc):
    """bodahip_sgemm_f16s: fp32 math on half operands, c rounded to half once (tests/test_gpu_parity.py: test_sgemm_half_storage_fp32_math) -- results beyond the
    largest half store as +-Inf, subnormal halves come and go unflushed, a NaN stays in its row / column."""
    geom = (100, 36, 50)
    data = R.gen_sgemm_half(geom)
    want = {c: R.to_half(bo.sgemm(d["a"].astype(F), d["b"].astype(F))) for c, d in data.items()}
    assert 0.1 < np.isinf(want["big"]).mean() < 0.9 and ((np.abs(want["subnormal"]) < 2.0 ** -14) & (want["subnormal"] != 0)).mean() > 0.2 and np.isnan(want["nan"]).any()
    res = R.run_sgemm(rtc, geom, data, tn="half")
    for cls, r in res.items():
        what = (geom, cls, r["launch"]["kernel"], r["launch"]["cfg"])
        assert r["launch"]["kernel"] == "bodahip_sgemm_f16s" and r["c"].dtype == np.float16, what
        R.assert_no_poison(r["c"], what)
        R.assert_same(want[cls], r["c"], what)


# ---- bf16 operands: nan_inf and inf_last_chan.  The reference is the oracle on to_bf16 operands; equal NaN / +-Inf masks, and on the finite elements the bounds of
# tests/test_gpu_nhwc.py as they stand
from test_gpu_nhwc import NHWC, NHWC_F32, _bound, _derived_limit

BF16_CLASSES = ("nan_inf", "inf_last_chan")


def _check_bf16_ops(form, shape, res, kernel, bf16_out, s2d=False):
    """s2d: the strided form of hip_conv_bf16 runs as a stride-1 convolution on a space-to-depth copy of `in`, its window rounded up to a multiple of the stride with
    zero filter taps -- operands of the MFMA loop itself.  A NaN or Inf under such a tap reaches outputs whose window does not hold it (x * 0): the documented exception
    of DESIGN.md section 3.0.  Held to containment: the outputs within stride - 1 rows / columns of a window that holds an injected element are not compared (how many
    of them came back non-finite is recorded); every other output is held to everything below."""
    op = R.conv_op(*shape)
    K = shape[1] * shape[5] * shape[6]; S, P = shape[7], shape[8]
    for (cls, relu), r in res.items():
        loose = None
        if s2d:
            inj = R.conv_data(cls, shape)["inj"]
            loose = np.zeros_like(R.window_mask(shape, inj))     # (element by element: beside one element's window may be inside another's)
            for one in inj:
                loose |= R.window_mask(shape, [one], ext=S - 1) & ~R.window_mask(shape, [one])
        what = (form, shape, cls, relu, r["launch"]["kernel"], r["launch"]["cfg"])
        assert re.search(kernel, r["launch"]["kernel"]), what
        d = R.conv_data(cls, shape)
        x16, f16 = bo.to_bf16(d["in"]), bo.to_bf16(d["filts"])
        assert np.array_equal(np.isnan(x16), np.isnan(d["in"])) and np.array_equal(np.isinf(x16), np.isinf(d["in"]))       # (the helper keeps what the kernels' conversion keeps)
        want = bo.conv_fwd(x16, f16, d["biases"], (S, S), (P, P), bool(relu))
        got = r["out"]
        assert got.dtype == F and got.shape == want.shape, what
        pz = (R.BF16_POISON << 16) if bf16_out else R.POISON_BITS
        assert not (R.bits(got) == pz).any(), (what, "an output element was never stored")
        if loose is not None:
            lm = np.broadcast_to(loose[:, None], got.shape)
            if not relu:
                REPORT[f"{form} {cls}: non-finite among the {int(lm.sum())} outputs beside a window"] = (int((lm & np.isfinite(got)).sum()), int((lm & ~np.isfinite(got)).sum()))
            got = np.where(lm, want, got)
        if cls == "inf_last_chan":
            same, nan = R.assert_contained(np.where(np.isfinite(want), got, want), got, what, relu=bool(relu))     # (the masks only: the finite values have their bounds below)
            if not relu:
                REPORT[form] = (same, nan)
        else:     # a payload-carrying NaN of `in` arrives as NaN: through the layout pass's conversion and the kernel's
            assert np.array_equal(np.isnan(want), np.isnan(got)), (what, "NaN masks differ", int(np.isnan(want).sum()), int(np.isnan(got).sum()))
            assert np.array_equal(np.isposinf(want), np.isposinf(got)) and np.array_equal(np.isneginf(want), np.isneginf(got)), (what, "Inf masks differ")
        fin = np.isfinite(want) & np.isfinite(got)
        w = np.where(fin, want, 0).astype(np.float64); g = np.where(fin, got, 0).astype(np.float64)
        lim = np.where(fin, _derived_limit(op, {"in": np.where(np.isfinite(d["in"]), d["in"], 0), "filts": d["filts"], "biases": d["biases"]}), 0.0)
        err = np.abs(g - w)
        if bf16_out:
            gf = got[fin]
            assert np.array_equal(bo.to_bf16(gf), gf), (what, "an output is not a bf16 value")
            assert (err <= 2.0 ** -8 * np.abs(w) + _bound(K) * np.maximum(1.0, np.abs(w))).all(), what
            assert (err <= 2.0 ** -8 * (np.abs(w) + lim) + lim).all(), (what, "derived bound")
        else:
            sd = SsdsDiff.of(w.astype(F), g.astype(F))
            assert sd.mrd < _bound(K), (what, sd.basic_str())
            assert (err <= lim).all(), (what, "derived bound", float((err / np.maximum(lim, 1e-300)).max()))


@pytest.mark.parametrize("shape", [T17, (2, 5, 17, 13, 7, 5, 5, 2, 2)], ids=R.sid)
def test_conv_bf16_operands_on_float_tensors(rtc, shape):
    _caps_first(shape, BF16_CLASSES)
    res = R.run_conv(rtc, shape, {c: R.conv_data(c, shape) for c in BF16_CLASSES}, tune=OpTune(hip_dtype="bf16"), func="hip_conv_bf16")
    s2d = shape[7] > 1
    assert ("(s2d)" in res[("nan_inf", 1)]["launch"]["kernel"]) == s2d, res[("nan_inf", 1)]["launch"]
    _check_bf16_ops("conv_bf16_" + R.sid(shape), shape, res, r"bf16", False, s2d=s2d)


NHWC_FORMS = [("nhwc_implicit_gemm", T17, dict(hip_patch=0), "", {}, r"^bodahip_conv_nhwc_bf16$", r"."),
              ("nhwc_input_patch", T17, {}, "", {}, r"^bodahip_conv_nhwc_patch_bf16$", r"."),
              ("nhwc_rolling_rows", (5, 16, 19, 23, 40, 3, 3, 1, 1), {}, "", {"BODAHIP_NHWC_ROWS": "1"}, r"^bodahip_conv_nhwc_(rows|patch)_bf16$", r"."),
              ("nhwc_k_sliced", T17, dict(hip_patch=0), "64x64x64x2x2x2x3", {}, r"^bodahip_conv_nhwc_bf16$", r"_s\d")]


@pytest.mark.parametrize("out", ["f32", "bf16"])
@pytest.mark.parametrize("form", NHWC_FORMS, ids=lambda f: f[0])
def test_conv_nhwc_form(rtc, form, out, monkeypatch):
    name, shape, tune, tile, env, kernel, cfg_re = form
    _caps_first(shape, BF16_CLASSES)
    _setenv(monkeypatch, env)
    t = OpTune(hip_tile=tile, **tune, **(NHWC_F32 if out == "f32" else NHWC))
    res = R.run_nhwc(rtc, shape, {c: R.conv_data(c, shape) for c in BF16_CLASSES}, t, tile=tile)
    for r in res.values():
        assert re.search(cfg_re, r["launch"]["cfg"]), r["launch"]
        if name == "nhwc_rolling_rows":      # (the rolling-rows kernel writes bf16 only: float outputs stay on the input-patch kernel)
            assert r["launch"]["kernel"] == ("bodahip_conv_nhwc_rows_bf16" if out == "bf16" else "bodahip_conv_nhwc_patch_bf16"), r["launch"]
    _check_bf16_ops(f"{name}_{out}", shape, res, kernel, out == "bf16")


def test_zz_report_what_became_of_an_inf_in_the_last_channel():
    """Per form: the outputs whose window holds inf_last_chan's +Inf (all of them +-Inf in the oracle) -- how many the kernel returned as the same Inf, how many as NaN
    (a K tail that re-reads the image's last channel against a zero filter value forms Inf * 0).  DESIGN.md section 3.0 holds the table."""
    print("\ninf_last_chan per form: same Inf / NaN")
    for form, (same, nan) in REPORT.items():
        print(f"  {form:60s} {same:6d} {nan:6d}  {'Inf' if not nan else ('NaN' if not same else 'mixed')}")
    assert REPORT
