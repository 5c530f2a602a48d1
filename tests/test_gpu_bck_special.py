"""The backward kernels on data and outputs that the other GPU files never give them (-m gpu; DESIGN.md section 3.11a, helpers and data classes in
tests/bck_special_ref.py, the reference side proven on the CPU by tests/test_bck_special_cpu.py).  One test per launch form: the kernel is compiled once, then run
over every data class into outputs refilled with a payload NaN before every run, a 4-float guard var behind every var.
  B1  no output element keeps the poison, every guard var keeps its bits, every IN arg reads back bit for bit (the runner asserts the last two on every run)
  B2  wide / subnormal / overflow: each fp32 conv-gradient launch equals its written chain emulator BY BITS (oracle/bck_chain.py, tests/bconv_fb_ref.py, with
      (BK, KSL) read from the launch); a NaN the arithmetic produced is compared as a NaN
  B3  nan_inf (NaNs and Infs in out_grad_loss), nan_inf_in (in `in`), nan_inf_filts (in `filts`: the stated exception): the rules of section 3.11a against be=cpu
      and the same kernel's clean run; how many elements of L \\ R / padding taps came back non-finite is recorded per form
The bf16-operand forms are held to float64 on to_bf16 operands under the bound of tests/bconv_bf16_ref.py, their masks to be=cpu's in the same mode.  Every test
asserts the kernel and the tile it ran.  The other backward functions (kernels/bck_ops_f32.hip) run the cases of bck_special_ref.CASES against be=cpu.
Nothing here starts a process or waits.

Measured on an MI355X (pytest --durations, the kernels pre-specialised by the build from tests/golden/ops/bck-special-ops.txt): the file's 69 tests take 2.9 s in
all; the slowest is test_bconv_in_form[planner-3x3_s1_img1_chan_not_32] at 0.10 s (the module fixture's setup, charged to the first test, 0.20 s)."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bck_special_ref as R
import bconv_bf16_ref as B16
import bconv_fb_ref as fb
from boda_amd.rtc import make_rtc
from fwd_special_ref import assert_no_poison, bits
from oracle import bck_chain as bc
from test_gpu_bck_chain import forced, plan_of

F = np.float32
REPORT = {}      # form -> what came back of the padded terms (printed by the last test: the tables of DESIGN.md section 3.11a)
PLANNER = r"^\d+x\d+x\d+_w\d+x\d+"


@pytest.fixture(scope="module")
def hip():
    r = make_rtc("(be=hip)", 0)
    r.init()
    assert r.get_plat_tag().startswith("hip:")
    yield r
    r.finish_and_sync()
    r.close()


def _ran(launch, kernel, tile):
    """The launch was this kernel, on the forced tile (BIxBJxBKxWIxWJ...) or on a plan of the planner's."""
    assert launch["kernel"] == kernel, (kernel, launch)
    if tile:
        v = tile.split("x")
        assert launch["cfg"].startswith(f"{v[0]}x{v[1]}x{v[2]}_w{v[3]}x{v[4]}"), (tile, launch)
    else:
        assert re.search(PLANNER, launch["cfg"]), launch


def _caps_first(grad, shape, classes):
    for cls in classes:
        if cls in R.FINITE + ("nan_inf", "nan_inf_in"):
            R.assert_caps(cls, R.cpu_want(cls, grad, shape), R.reached(grad, shape))


def _what_an_inf_became(d, got, want):
    """Among the elements where be=cpu has an Inf: how many the kernel returned as the same Inf / as a NaN."""
    wi = np.isinf(want)
    got = np.asarray(got).reshape(want.shape)
    return int((wi & (got == want)).sum()), int((wi & np.isnan(got)).sum())


# ---- the data gradient, fp32
IN_CLASSES = R.FINITE + ("clean", "nan_inf", "nan_inf_filts")


@pytest.mark.parametrize("form", R.IN_FORMS, ids=lambda f: f"{f[0]}-{f[1]}")
def test_bconv_in_form(hip, form):
    _, name, tile = form
    shape = R.SHAPES[name]
    _caps_first("in", shape, IN_CLASSES)
    sets = {c: R.data(c, "in", shape) for c in IN_CLASSES}
    res = R.run_fop(hip, R.func_of("in", shape, tile), sets)
    for c, r in res.items():
        what = (form, c, r["launch"]["cfg"])
        _ran(r["launch"], "bodahip_bconv_in", tile)
        got = r["in_grad_loss"]
        assert_no_poison(got, what)
        R.assert_bits(R.emu(c, "in", shape, R.bk_of(r["launch"])), got, what)      # B2 on the finite classes; on the injected ones the emulator's padded operands give the kernel's NaNs as well
    clean = res["clean"]["in_grad_loss"]
    want = R.cpu_want("nan_inf", "in", shape)
    leaked, of = R.check_in_b3(shape, sets["nan_inf"], res["nan_inf"]["in_grad_loss"], clean, want, form)
    same, nan = _what_an_inf_became(sets["nan_inf"], res["nan_inf"]["in_grad_loss"], want)
    REPORT[f"bconv_in {form[0]} {name}"] = f"L\\R non-finite {leaked} of {of}; be=cpu's Infs: {same} the same Inf, {nan} NaN"
    assert nan == 0 and (leaked == of if of else True)
    nf, ref_nf = R.check_in_b3_filts(shape, sets["nan_inf_filts"], res["nan_inf_filts"]["in_grad_loss"], clean, R.cpu_want("nan_inf_filts", "in", shape), form)
    REPORT[f"bconv_in {form[0]} {name} (non-finite filts)"] = f"{nf} non-finite elements inside the injected in_chans, be=cpu {ref_nf}"


@pytest.mark.parametrize("name", ["3x3_s2_k_not_multiple_of_s", "3x3_s1_two_imgs_17_chans"])
def test_bconv_in_zero_if_in_non_pos_form(hip, name):
    """-DZINP=1: +0 wherever `in` <= 0 or `in` is a NaN, whatever the gradient -- a NaN, an Inf, a leaked NaN of L \\ R --, the unflagged chain's bits elsewhere."""
    shape = R.SHAPES[name]
    zin = R.zinp_in(shape)
    sets = {c: dict(R.data(c, "in", shape), **{"in": zin}) for c in IN_CLASSES}
    res = R.run_fop(hip, R.func_of("in", shape, zinp=True), sets)
    pos = zin > 0
    for c, r in res.items():
        what = ("zinp", name, c, r["launch"]["cfg"])
        _ran(r["launch"], "bodahip_bconv_in", "")
        got = r["in_grad_loss"]
        assert_no_poison(got, what)
        assert (bits(got)[~pos] == 0).all(), (what, "not +0 where in <= 0 or in is a NaN")
        R.assert_bits(np.where(pos, R.emu(c, "in", shape, R.bk_of(r["launch"])), F(0)), got, what)
    g = res["nan_inf"]["in_grad_loss"]
    assert np.isnan(g).any() and np.isinf(g).any() and (~np.isfinite(R.emu("nan_inf", "in", shape)[~pos])).any()     # (both branches of the select met a non-finite gradient)


@pytest.mark.parametrize("OC,tile", [(16, R.M0_TILE), (1, "")])
def test_bconv_in_minus_zero_under_a_padded_term(hip, OC, tile):
    """The directed case of tests/test_bck_special_cpu.py on the kernel: the emulator's bits.  144 terms in whole K steps of 16: +0 in the bottom row and the right
    column, whose chains end in a padded term, where be=cpu returns -0, and -0 on the other nine pels; 9 terms and a K tail: +0 everywhere."""
    shape, d = R.minus_zero_case(OC)
    r = R.run_fop(hip, R.func_of("in", shape, tile), {"m0": d})["m0"]
    _ran(r["launch"], "bodahip_bconv_in", tile)
    g = r["in_grad_loss"]
    assert_no_poison(g)
    assert (g == 0).all()      # by value: be=cpu's result
    bk = R.bk_of(r["launch"])
    assert (9 * OC) % bk == (0 if OC == 16 else 9)
    R.assert_bits(bc.in_grad_chain(d["filts"], d["out_grad_loss"], R.geom_of(shape), bk), g, (OC, r["launch"]["cfg"]))
    assert bits(g)[0, 0, 3, 3] == 0 and (bits(g)[0, 0, 0, 0] == 0x80000000) == (OC == 16)


# ---- the filter gradient, fp32
F_CLASSES = R.FINITE + ("clean", "nan_inf", "nan_inf_in")


def _check_filts(form, shape, sets, res, out, bk, ksl):
    for c, r in res.items():
        what = (form, c, r["launch"]["cfg"])
        assert_no_poison(r[out], what)
        R.assert_bits(R.emu(c, "filts", shape, bk, ksl), r[out], what)      # (`overflow` on a sliced form: the sliced emulator's Inf - Inf NaNs)
    clean = res["clean"][out]
    want = R.cpu_want("nan_inf", "filts", shape)
    leaked, of = R.check_filts_b3_ogl(shape, sets["nan_inf"], res["nan_inf"][out], clean, want, form)
    same, nan = _what_an_inf_became(sets["nan_inf"], res["nan_inf"][out], want)
    R.check_filts_b3_in(sets["nan_inf_in"], res["nan_inf_in"][out], clean, R.cpu_want("nan_inf_in", "filts", shape), form)
    return f"padding taps non-finite {leaked} (of {of} row elements); be=cpu's Infs: {same} the same Inf, {nan} NaN"


@pytest.mark.parametrize("form", R.FILTS_FORMS, ids=lambda f: f"{f[0]}-{f[1]}")
def test_bconv_filts_form(hip, form):
    tile, name = form
    shape = R.SHAPES[name]
    _caps_first("filts", shape, F_CLASSES)
    g = R.geom_of(shape); K = g["B"] * g["OH"] * g["OW"]
    bk, ksl = forced(tile)
    if tile == R.KSL7:
        assert K < 7 * 16 and (K, K) in bc.filts_slices(K, bk, ksl)      # empty slices
    if ksl == 3 and name != "3x3_s2_k_not_multiple_of_s" and name != "5x5_s2_pad3_pad_ge_stride":
        assert K % bk      # a K tail
    sets = {c: R.data(c, "filts", shape) for c in F_CLASSES}
    res = R.run_fop(hip, R.func_of("filts", shape, tile), sets)
    for r in res.values():
        _ran(r["launch"], "bodahip_bconv_filts", tile)
        assert plan_of(r["launch"]) == (bk, ksl), r["launch"]
    REPORT[f"bconv_filts {tile} {name}"] = _check_filts(form, shape, sets, res, "filts_grad_loss", bk, ksl)


@pytest.mark.parametrize("name", list(R.SHAPES))
def test_bconv_biases(hip, name):
    shape = R.SHAPES[name]
    _caps_first("biases", shape, R.FINITE + ("nan_inf",))
    sets = {c: R.data(c, "biases", shape) for c in R.FINITE + ("clean", "nan_inf")}
    res = R.run_fop(hip, R.func_of("biases", shape), sets)
    for c, r in res.items():
        assert r["launch"]["kernel"] == "bodahip_bconv_biases", r["launch"]
        assert_no_poison(r["biases_grad_loss"], (name, c))
        R.assert_bits(R.emu(c, "biases", shape), r["biases_grad_loss"].reshape(-1), (name, c))
    assert set(R.kind(res["nan_inf"]["biases_grad_loss"]).reshape(-1)) == {0, 1, 2, 3}


@pytest.mark.parametrize("form", R.FB_FORMS, ids=lambda f: f"{f[0]}-{f[1]}")
def test_bconv_filts_biases_form(hip, form):
    tile, name = form
    shape = R.FB_SHAPES[name]
    _caps_first("filts", shape, F_CLASSES)
    sets = {c: R.data(c, "filts", shape) for c in F_CLASSES}
    res = R.run_fop(hip, R.func_of("fb", shape, tile), sets)
    bk, ksl = forced(tile)
    for c, r in res.items():
        _ran(r["launch"], "bodahip_bconv_filts_biases", tile)
        assert fb.plan_of(r["launch"]) == (bk, ksl), r["launch"]
        assert_no_poison(r["biases_grad_loss"], (form, c))
        R.assert_bits(R.emu(c, "biases", shape, bk, ksl, fused=True), r["biases_grad_loss"].reshape(-1), (form, c, "biases"))
    REPORT[f"bconv_filts_biases {tile} {name}"] = _check_filts(form, shape, sets, res, "filts_grad_loss", bk, ksl)


# ---- bf16 operands
def _flush_stat(shape, which, got, r, ksl):
    """On `subnormal`: the elements beyond the bound WITHOUT its flush allowance, and the largest error in units of 2^-149."""
    i = 0 if which == "in" else 1
    S, A = r["S"][i], r["A"][i]
    K = B16.n_terms(R.op_of(tuple(shape)), which)
    err = np.abs(np.asarray(got, np.float64).reshape(S.shape) - S)
    lost = (S != 0) & (np.asarray(got).reshape(S.shape) == 0)
    return f"{int((err > 2.0 * (K + ksl + 3) * R.U * A).sum())} of {S.size} beyond the bound without the allowance, largest error {float(err.max() / 2.0 ** -149):.2f} x 2^-149, " \
           f"{int(lost.sum())} nonzero sums returned as 0 (smallest |S| among them {float(np.abs(S[lost]).min()) if lost.any() else 0:.3g})"


BF_IN_CLASSES = ("wide", "subnormal", "clean", "nan_inf", "bf16_saturate")


@pytest.mark.parametrize("form", R.BF_IN_FORMS, ids=lambda f: f"{f[0]}-{f[1]}")
def test_bconv_in_bf16_form(hip, form):
    _, name, tile = form
    shape = R.SHAPES[name]
    _caps_first("in", shape, BF_IN_CLASSES)
    sets = {c: R.data(c, "in", shape) for c in BF_IN_CLASSES}
    res = R.run_fop(hip, R.func_of("in", shape, tile, bf16=True), sets)
    for c, r in res.items():
        _ran(r["launch"], "bodahip_bconv_in_bf16", tile)
        assert_no_poison(r["in_grad_loss"], (form, c))
    out = lambda c: res[c]["in_grad_loss"]
    R.check_bf16_bound(shape, "in", out("wide"), R.bf16_refs(shape, sets["wide"]), 1, with_nrms=True, what=(form, "wide"))
    rs = R.bf16_refs(shape, sets["subnormal"])
    R.check_bf16_bound(shape, "in", out("subnormal"), rs, 1, flush=True, what=(form, "subnormal"))      # (asserts: no NaN / Inf)
    REPORT[f"bconv_in_bf16 {form[0]} {name} subnormal"] = _flush_stat(shape, "in", out("subnormal"), rs, 1)
    for c in ("nan_inf", "bf16_saturate"):
        want = R.cpu_want(c, "in", shape, bf16=True)
        leaked, of = R.check_in_b3(shape, sets[c], out(c), out("clean"), want, (form, c))
        REPORT[f"bconv_in_bf16 {form[0]} {name} {c}"] = f"L\\R non-finite {leaked} of {of}; be=cpu's Infs: %d the same Inf, %d NaN" % _what_an_inf_became(sets[c], out(c), want)
        L = np.any([R.in_windows(shape, one)[1] for one in sets[c]["inj"]], axis=0)
        R.check_bf16_bound(shape, "in", out(c), R.bf16_refs(shape, sets[c]), 1, fin=np.broadcast_to(~L[:, None], out(c).shape), what=(form, c))


BF_FB_CLASSES = ("wide", "subnormal", "clean", "nan_inf", "nan_inf_in", "bf16_saturate", "bf16_saturate_in")


@pytest.mark.parametrize("form", R.BF_FB_FORMS, ids=lambda f: f"{f[0]}-{f[1]}")
def test_bconv_filts_biases_bf16_form(hip, form):
    _, name, tile = form
    shape = R.FB_SHAPES[name]
    _caps_first("filts", shape, BF_FB_CLASSES)
    sets = {c: R.data(c, "filts", shape) for c in BF_FB_CLASSES}
    res = R.run_fop(hip, R.func_of("fb", shape, tile, bf16=True), sets)
    bk, ksl = B16.plan_of(res["wide"]["launch"])
    assert not tile or (bk, ksl) == forced(tile)
    for c, r in res.items():
        _ran(r["launch"], "bodahip_bconv_filts_biases_bf16", tile)
        assert B16.plan_of(r["launch"]) == (bk, ksl)
        assert_no_poison(r["filts_grad_loss"], (form, c)); assert_no_poison(r["biases_grad_loss"], (form, c))
        R.assert_bits(R.emu(c, "biases", shape, bk, ksl, fused=True), r["biases_grad_loss"].reshape(-1), (form, c, "the bias keeps the fp32 chain's bits"))
    out = lambda c: res[c]["filts_grad_loss"]
    R.check_bf16_bound(shape, "filts", out("wide"), R.bf16_refs(shape, sets["wide"]), ksl, with_nrms=True, what=(form, "wide"))
    rs = R.bf16_refs(shape, sets["subnormal"])
    R.check_bf16_bound(shape, "filts", out("subnormal"), rs, ksl, flush=True, what=(form, "subnormal"))
    REPORT[f"bconv_filts_biases_bf16 {form[0]} {name} subnormal"] = _flush_stat(shape, "filts", out("subnormal"), rs, ksl)
    for c in ("nan_inf", "bf16_saturate"):
        want = R.cpu_want(c, "fb", shape, bf16=True)
        leaked, of = R.check_filts_b3_ogl(shape, sets[c], out(c), out("clean"), want, (form, c))
        REPORT[f"bconv_filts_biases_bf16 {form[0]} {name} {c}"] = f"padding taps non-finite {leaked} (of {of} row elements); be=cpu's Infs: %d the same Inf, %d NaN" % _what_an_inf_became(sets[c], out(c), want)
        rows = np.zeros(shape[4], bool); rows[[one[1] for one in sets[c]["inj"]]] = True
        R.check_bf16_bound(shape, "filts", out(c), R.bf16_refs(shape, sets[c]), ksl, fin=np.broadcast_to(~rows[:, None, None, None], want.shape), what=(form, c))
    for c in ("nan_inf_in", "bf16_saturate_in"):
        want = R.cpu_want(c, "fb", shape, bf16=True)
        got = out(c).reshape(want.shape)
        assert np.array_equal(R.kind(got), R.kind(want)), (form, c, "NaN / Inf masks differ from be=cpu")
        R.check_bf16_bound(shape, "filts", got, R.bf16_refs(shape, sets[c]), ksl, fin=np.isfinite(want), what=(form, c))
        fin = np.isfinite(want)
        assert np.array_equal(bits(got)[fin], bits(out("clean").reshape(want.shape))[fin]), (form, c, "a finite element differs from the clean run")


# ---- the other backward functions
@pytest.mark.parametrize("case", sorted(R.CASES))
def test_other_backward_function(hip, case):
    seen = R.CASES[case](hip, R.cpu_rtc())
    assert seen
    for fn, launch in seen:
        assert launch["kernel"] == "bodahip_" + fn[4:], (fn, launch)


def test_zz_report_what_became_of_the_padded_terms():
    """Per form: how many elements of L \\ R (data gradient) / padding taps (filter gradient) came back non-finite and what be=cpu's Infs became; the bf16 forms'
    `subnormal` finding.  DESIGN.md section 3.11a holds the tables."""
    print()
    for form, line in REPORT.items():
        print(f"  {form:75s} {line}")
    assert REPORT
