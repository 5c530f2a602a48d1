"""The seeded random-geometry sweeps of the grouped convolution, the Deconvolution family and Crop without a GPU: the case generators of tools/fuzz_grp.py, the one
table of seeds, lists and forced tiles that tests/test_gpu_grp_fuzz.py runs on be=hip, and the DEFINITIONS and float64 bounds on those very cases -- so that a mismatch
on the GPU can only be the kernel.

  * generators: pure functions of (n, seed); every case stays inside its ranges and builds an op the annotators accept; every forced tile is one the planner takes for
    every case of the list it runs on (planned here, on the host); every branch category of fuzz_grp.grp_categories / deconv_categories is reached by at least two
    cases of the list meant for it, the aligned input span at each of PX % 4 = 0 .. 3; deconv_categories' restatement of deconv_grid gives the planner's own grid
  * grouped cases: be=cpu's three grouped functions equal be=cpu's ungrouped functions on the slices bit for bit (conv_grp_ref.sliced), the filter gradient equals
    oracle/bck_chain.filts_chain per group with one slice, and all three stay under the existing bounds against float64 (FWD_MRD, 2e-4, FILTS_MRD; conv_grp_ref.torch_twin)
  * Deconvolution cases: be=cpu's four functions equal the existing functions on the exchanged roles bit for bit (deconv_ref.exchanged), the filter gradient equals
    filts_chain on the exchanged roles with one slice, and all stay within deconv_ref.within_f64_bound of torch's conv_transpose2d
  * Crop: be=cpu equals the numpy window; hip_crop_bck is +0 by bits outside it

Counts: 7 lists of 12 grouped cases, 12 + 4 Deconvolution cases (the four hand-made ones reach `passes` and `lds_chunks`, which under 3 % of the draws do), 12 Crop windows."""
import os
import sys

import numpy as np
import pytest

_TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if _TOOLS not in sys.path:
    sys.path.insert(0, _TOOLS)
import fuzz_grp as F

import conv_grp_ref as G
import deconv_ref as D
from boda_amd import rtc as rtc_mod
from boda_amd.cnn_op import OpTune, add_bck_op_annotations
from boda_amd.rtc import make_rtc
from oracle import bck_chain

from test_bck_conv_cpu import FILTS_MRD
from test_bck_fuzz_cpu import frac_of

FWD_MRD = 2e-4   # the forward tests' bound against float64 (tests/test_conv_grp_cpu.py)

# ---- the one table of seeds, lists and parameters (tests/test_gpu_grp_fuzz.py imports it)
N = 12   # cases per list: every random geometry is a fresh hiprtc specialisation
GRP_LISTS = {   # list -> (function, form the list is bent for, seed)
    "fwd_d": ("fwd", "direct", 1101), "fwd_m": ("fwd", "matrix", 1102),
    "in_d": ("in", "direct", 1201), "in_d4": ("in", "direct_vx4", 1202), "in_m": ("in", "matrix", 1203),
    "filts_d": ("filts", "direct", 1301), "filts_m": ("filts", "matrix", 1302),
}
# the GPU test's parameters: id -> (list, name of the forced tile in fuzz_grp.forced_tiles, "" = the planner's choice)
FWD_PARAMS = {"planner_d": ("fwd_d", ""), "planner_m": ("fwd_m", ""), "vx1": ("fwd_d", "vx1"), "vx2": ("fwd_d", "vx2"), "vx4": ("fwd_d", "vx4"),
              "m32": ("fwd_m", "m32"), "m32x2x2": ("fwd_m", "m32x2x2"), "m16": ("fwd_m", "m16")}
IN_PARAMS = {"planner_d": ("in_d", ""), "planner_m": ("in_m", ""), "vx1": ("in_d", "vx1"), "vx4": ("in_d4", "vx4"), "m32": ("in_m", "m32"), "m32x2x2": ("in_m", "m32x2x2"), "m16": ("in_m", "m16")}
FILTS_PARAMS = dict({"planner_d": ("filts_d", ""), "planner_m": ("filts_m", "")}, **{n: ("filts_d", n) for n in F.FILTS_DIRECT_PLANS}, **{n: ("filts_m", n) for n in F.FILTS_MATRIX_PLANS})
PARAMS = {"fwd": FWD_PARAMS, "in": IN_PARAMS, "filts": FILTS_PARAMS}
CONTAIN = {"direct": [("fwd_d", 0), ("in_d", 1)], "matrix": [("fwd_m", 0), ("filts_m", 1)]}   # the containment test's two cases per form: (list, index)

DECONV_SEED = 1409   # (seeds are chosen so that each list reaches every category at least twice: test_lists_have_their_lengths_and_reach_every_category_twice)
# `passes` needs OC * SY >= 1024 on a 256-CU chip (deconv_grid wants eight workgroups a CU before it lets one make a second pass) and then more than 256 resp. 512
# (img, row, quad) items; with B <= 4 and planes <= 8 that is a 2 x 8 map at stride 32: about 1.9 M outputs of one term each, the smallest the restatement finds
# (outputs = OC * SY * items * the quad's share of OW >= 2048 * 256 either way).  `lds_chunks` needs C * ceil(KH/SY) * KW > 8192 floats: 33 channels x 4 rows x 64 taps
# = 8448, two chunks, the second of one channel.  The two are kept apart: a 33-channel 64 x 64 kernel over 1.9 M outputs is minutes on be=cpu.
DECONV_HAND = [
    D._c(4, 1, 8, 2, 64, 1, 32, 0),                              # passes: want = 1, one chunk of 288 items (two passes, the second ragged)
    D._c(4, 1, 8, 3, 33, (2, 2), (32, 32), (0, 0)),              # passes under two chunks: 544 items, per = 272
    D._c(1, 33, 2, 2, 2, 64, 16, 0),                             # lds_chunks: 8448 floats
    D._c(2, 33, 1, 2, 1, (61, 64), (16, 8), (3, 5)),             # lds_chunks, rectangular, the last filter row past the kernel
]
CROP_SEED = 1501


def grp_list(key):
    func, form, seed = GRP_LISTS[key]
    return F.grp_cases(N, seed, func, form)


def grp_data_seed(key, i):
    return 100 * (1 + list(GRP_LISTS).index(key)) + i


def grp_tile(key, name, case):
    func, form, _ = GRP_LISTS[key]
    return F.forced_tiles(case, func, form)[name] if name else ""


def deconv_list():
    return F.deconv_cases(N, DECONV_SEED) + DECONV_HAND


def deconv_data_seed(i):
    return 2000 + i


def crop_list():
    return F.crop_cases(N, CROP_SEED)


def case_id(case):
    return "-".join("x".join(str(i) for i in v) if isinstance(v, tuple) else str(v) for v in case)


def grp_filts_chain(case, ins, BK, KSL):
    """oracle/bck_chain.filts_chain per group on the slices, side by side along the filter-row axis."""
    geom = G.bck_op(*G.slice_case(case), group_field=False).bck_conv_geom()
    parts = []
    for j in range(case[1]):
        s = G.slice_ins(case, ins, j)
        parts.append(bck_chain.filts_chain(s["in"], s["out_grad_loss"], geom, BK, KSL))
    return np.concatenate(parts, axis=0)


def grp_func(case, func):
    fc, fi, _, ff = G.grouped_funcs(case)
    return {"fwd": fc, "in": fi, "filts": ff}[func]


GRP_BOUND = {"fwd": ("forward FWD_MRD", FWD_MRD), "in": ("in_grad_loss mrd 2e-4", 2e-4), "filts": ("filts_grad_loss FILTS_MRD", FILTS_MRD)}


def grp_twin(case, ins):
    o, gi, gw = G.torch_twin(case, ins)
    return {"fwd": o, "in": gi, "filts": gw}


def deconv_frac(got, twin, case, which, ksl=1):
    """The largest |got - float64| as a fraction of deconv_ref.within_f64_bound's bound (n + 1) * 2^-24 * sum |terms|; an element whose bound is 0 must be exact."""
    n = D.chain_len(case, which, ksl)
    err = np.abs(got.astype(np.float64) - twin[which])
    bound = (n + 1) * 2.0 ** -24 * twin["abs"][which]
    with np.errstate(divide="ignore", invalid="ignore"):
        fr = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(np.max(fr)) if fr.size else 0.0


def crop_data(case, seed):
    B, C, H, W, OH, OW, oy, ox = case
    rng = np.random.default_rng(seed)
    a = rng.uniform(-5, 5, (B, C, H, W)).astype(np.float32)
    g = -np.abs(rng.uniform(0.5, 5, (B, C, OH, OW))).astype(np.float32)   # (all negative: a -0 outside the window would show)
    return a, g


def crop_funcs(case):
    fwd, bck = D.crop_ops(*case)
    (ff,), (fb,) = add_bck_op_annotations(fwd, OpTune()), add_bck_op_annotations(bck, OpTune())
    return ff, fb


def check_crop(rtc, case, seed, kernel_names=False):
    B, C, H, W, OH, OW, oy, ox = case
    ff, fb = crop_funcs(case)
    a, g = crop_data(case, seed)
    got, launch = D.run_func(rtc, ff, {"in": a}, runs=2, guards=True)
    assert D.bits_equal(got, a[:, :, oy:oy + OH, ox:ox + OW]), case
    assert not kernel_names or launch["kernel"] == "bodahip_crop", launch
    want = np.zeros((B, C, H, W), np.float32); want[:, :, oy:oy + OH, ox:ox + OW] = g
    got, launch = D.run_func(rtc, fb, {"out_grad_loss": g}, runs=2, guards=True)
    assert D.bits_equal(got, want), case   # the +0 outside the window by bits
    assert not kernel_names or launch["kernel"] == "bodahip_crop_bck", launch


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


# ---- the generators
def test_generators_are_pure_functions_of_n_and_seed():
    gens = [lambda n, s, fu=fu, fo=fo: F.grp_cases(n, s, fu, fo) for fu, fo in F.GRP_WANTS] + [F.deconv_cases, F.crop_cases]
    for gen in gens:
        assert gen(24, 5) == gen(24, 5) and gen(24, 5) != gen(24, 6) and len(gen(24, 5)) == 24
        assert gen(24, 5)[:8] == gen(8, 5)   # a longer list extends a shorter one


def test_grouped_cases_stay_inside_their_ranges():
    for func, form in F.GRP_WANTS:
        cases = F.grp_cases(160, 3, func, form)
        for B, g, C, OC, H, W, (KH, KW), (SY, SX), (PY, PX) in cases:
            assert 1 <= B <= 4 and C % g == 0 and OC % g == 0 and 1 <= H <= 24 and 1 <= W <= 24
            assert (g in F.GROUPS and C // g in F.EXTS and OC // g in F.EXTS) or (g in F.DW_CHANS and C == g and OC // g in (1, 2, 3))
            assert 1 <= KH <= 7 and 1 <= KW <= 7 and 1 <= SY <= 4 and 1 <= SX <= 4 and 0 <= PY < KH and 0 <= PX < KW and H + 2 * PY >= KH and W + 2 * PX >= KW
            OH, OW = (H + 2 * PY - KH) // SY + 1, (W + 2 * PX - KW) // SX + 1
            assert 2.0 * B * OH * OW * OC * (C // g) * KH * KW <= F.FLOP_CAP and (form != "direct_vx4" or SX == 1)
        share = lambda pred: sum(1 for c in cases if pred(c)) / len(cases)
        assert 0.15 < share(lambda c: c[6][0] != c[6][1]) < 0.7 and share(lambda c: c[1] == c[2]) > 0.1, (func, form)   # non-square kernels; depthwise draws
        assert form == "direct_vx4" or 0.15 < share(lambda c: c[7][0] != c[7][1]) < 0.7, (func, form)
        for cat in F.GRP_WANTS[(func, form)]:
            assert share(lambda c: cat in F.grp_categories(c, func, form)) > 0.08, (func, form, cat)


def test_deconv_and_crop_cases_stay_inside_their_ranges():
    cases = F.deconv_cases(300, 3)
    for case in cases:
        B, C, H, W, OC, (KH, KW), (SY, SX), (PY, PX) = case
        assert 1 <= B <= 4 and C in F.DECONV_CHANS and OC in F.DECONV_CHANS and 1 <= H <= 8 and 1 <= W <= 8
        assert all(1 <= k <= 16 or k == 64 for k in (KH, KW)) and all(1 <= s <= 8 or s in (16, 32) for s in (SY, SX)) and 0 <= PY < KH and 0 <= PX < KW
        assert min(F.deconv_out_plane(case)) >= 1 and F.deconv_out_plane(case) == D.out_plane(case) and 2.0 * B * C * H * W * OC * KH * KW <= F.FLOP_CAP
    assert any(64 in c[5] for c in cases) and any(max(c[6]) >= 16 for c in cases)
    for cat in F.DECONV_WANTS:
        assert sum(1 for c in cases if cat in F.deconv_categories(c)) > 0.06 * len(cases), cat
    for B, C, H, W, OH, OW, oy, ox in F.crop_cases(120, 3):
        assert 1 <= OH and oy + OH <= H <= 24 and 1 <= OW and ox + OW <= W <= 24 and oy >= 0 and ox >= 0


def test_lists_have_their_lengths_and_reach_every_category_twice():
    """Every branch named in grp_categories at least twice in the list bent for it, the aligned input span at each PX % 4; the Deconvolution forward's zs > 1, a ragged
    chunk, per > 256, kNC > 1, SX in 4..7 and an empty phase; the Crop kinds."""
    for key, (func, form, _) in GRP_LISTS.items():
        cases = grp_list(key)
        assert len(cases) == N
        count = {cat: sum(1 for c in cases if cat in F.grp_categories(c, func, form)) for cat in F.GRP_WANTS[(func, form)] + (["aligned_span", "wide_span"] if key == "fwd_d" else [])}
        print(key, count)
        for cat, v in count.items():
            assert v >= (1 if cat.startswith("aligned_span_p") else 2), (key, cat, count)
        if key == "filts_d":   # the split quad under the odd-BK plan itself, the empty slices under the 300-slice plan
            assert sum(1 for c in cases if "split_quad" in F.grp_categories(c, func, form, F.filts_tile("dodd_s3", c))) >= 2
            assert sum(1 for c in cases if "empty_slices" in F.grp_categories(c, func, form, F.filts_tile("d4s300", c))) >= 2
    for func, params in PARAMS.items():   # every parameter's list is one of the function's, and every forced tile of a list is run
        for pid, (key, name) in params.items():
            assert GRP_LISTS[key][0] == func and (not name or name in F.forced_tiles(grp_list(key)[0], func, GRP_LISTS[key][1])), (func, pid)
        for key, (fu, form, _) in GRP_LISTS.items():
            if fu == func:
                assert {n for k, n in params.values() if k == key} - {""} == set(F.forced_tiles(grp_list(key)[0], func, form)), (func, key)
    dl = deconv_list()
    assert len(dl) == N + len(DECONV_HAND) and len(set(dl)) == len(dl)
    count = {cat: sum(1 for c in dl if cat in F.deconv_categories(c)) for cat in F.DECONV_WANTS + ["share", "passes", "lds_chunks"]}
    print("deconv", count)
    assert all(v >= 2 for v in count.values()), count
    assert all("passes" in F.deconv_categories(c) for c in DECONV_HAND[:2]) and all("lds_chunks" in F.deconv_categories(c) for c in DECONV_HAND[2:])
    assert {"chunks", "ragged_chunk", "passes"} <= F.deconv_categories(DECONV_HAND[1])   # chunk boundaries inside a workgroup's second pass
    assert sum(1 for c in F.deconv_cases(400, 9) if {"passes", "lds_chunks"} & F.deconv_categories(c)) < 12   # (why they are hand-made: under 3 % of the draws)
    cl = crop_list()
    assert len(cl) == N and all(sum(1 for c in cl if k in F.crop_kinds(c)) >= 2 for k in F.CROP_KINDS)


def test_every_case_builds_and_every_forced_tile_plans():
    """No (case, tile) pair is left to be skipped at run time: the planner takes every forced tile on every case of the list it runs on, and reports it."""
    for func, params in PARAMS.items():
        for pid, (key, name) in params.items():
            for case in grp_list(key):
                f = grp_func(case, func)
                tile = grp_tile(key, name, case)
                if tile:
                    f = f.copy(); f.str_vals["hip_tile"] = tile
                plan = rtc_mod.explain_plan(f).split()
                base = {"fwd": "bodahip_conv_grp_", "in": "bodahip_bconv_in_grp_", "filts": "bodahip_bconv_filts_grp_"}[func]
                assert plan[0] in (base + "direct", base + "mfma"), (case, tile, plan[0])
                if tile:
                    t = tile.split("x")
                    assert plan[0] == base + ("mfma" if int(t[0]) > 1 else "direct") and plan[1].startswith("x".join(t[:3]) + "_w" + "x".join(t[3:5])), (case, tile, plan[:2])
                    assert ("_s" + t[6] in plan[1]) == (int(t[6]) > 1), (case, tile, plan[1])
    bad = next(c for c in grp_list("in_d") if c[7][1] != 1)   # why the VX = 4 list draws SX == 1 only
    f = grp_func(bad, "in").copy(); f.str_vals["hip_tile"] = F.IN_VX4_TILES["vx4"]
    with pytest.raises(Exception, match="unsupported tile"):
        rtc_mod.explain_plan(f)
    for case in deconv_list():
        funcs = D.deconv_funcs(case)
        grid, zs, per, items = F.deconv_fwd_grid(case)
        plan = rtc_mod.explain_plan(funcs["fwd"]).split()
        assert plan[0] == "bodahip_deconv_direct" and plan[2] == f"grid={grid}", (case, plan[:3], grid)   # deconv_grid, restated
        assert rtc_mod.explain_plan(funcs["in"]).startswith("bodahip_deconv_bck_in_direct ")
        for tile, bk, ksl in [("", 0, 0)] + D.filts_tiles(case):
            f = funcs["filts"].copy()
            if tile:
                f.str_vals["hip_tile"] = tile
            plan = rtc_mod.explain_plan(f).split()
            assert plan[0] == "bodahip_deconv_bck_filts_direct" and (not tile or plan[1] == f"1x1x{bk}_w2x2" + (f"_s{ksl}" if ksl > 1 else "")), (case, tile, plan[:2])
    for case in crop_list():
        assert [rtc_mod.explain_plan(f).split()[0] for f in crop_funcs(case)] == ["bodahip_crop", "bodahip_crop_bck"]


# ---- the definitions and the float64 bounds on be=cpu, on the GPU's cases
@pytest.mark.parametrize("key", list(GRP_LISTS))
def test_cpu_grouped_definitions_and_bounds(cpu, key):
    worst = {}
    for i, case in enumerate(grp_list(key)):
        ins = G.rand_ins(case, grp_data_seed(key, i))
        twin = grp_twin(case, ins)
        for which in ("fwd", "in", "filts"):
            got = D.run_func(cpu, grp_func(case, which), ins, guards=True)[0]
            assert G.bits_equal(got, G.sliced(cpu, case, ins, which)), (case, which)
            if which == "filts":
                assert G.bits_equal(got, grp_filts_chain(case, ins, 32, 1)), case
                if GRP_LISTS[key][0] == "filts":   # the sliced chains of the plans the GPU test forces on this list: under the bound as well
                    for tile in F.forced_tiles(case, "filts", GRP_LISTS[key][1]).values():
                        bk, ksl = int(tile.split("x")[2]), int(tile.split("x")[6])
                        fr = frac_of(grp_filts_chain(case, ins, bk, ksl), twin[which], FILTS_MRD)
                        worst["filts (sliced chain) FILTS_MRD"] = max(worst.get("filts (sliced chain) FILTS_MRD", 0.0), fr)
                        assert fr < 1.0, (case, tile, fr)
            name, bound = GRP_BOUND[which]
            fr = frac_of(got, twin[which], bound)
            worst[name] = max(worst.get(name, 0.0), fr)
            assert fr < 1.0, (case, name, fr)
    print(f"grouped list {key}: worst fraction of each bound on be=cpu:", {n: round(v, 4) for n, v in worst.items()})


@pytest.mark.parametrize("i", range(N + len(DECONV_HAND)))
def test_cpu_deconv_definitions_and_bounds(cpu, i):
    case = deconv_list()[i]
    ins = D.rand_ins(case, deconv_data_seed(i))
    funcs = D.deconv_funcs(case)
    twin = D.torch_twin(case, ins)
    for which in ("fwd", "in", "biases", "filts"):
        got, _ = D.run_func(cpu, funcs[which], ins, guards=True)
        assert D.bits_equal(got, D.exchanged(cpu, case, ins, which)), (case, which)
        assert D.within_f64_bound(got, twin, case, which) and deconv_frac(got, twin, case, which) <= 1.0, (case, which, deconv_frac(got, twin, case, which))
        if which == "filts":
            assert D.bits_equal(got, bck_chain.filts_chain(ins["out_grad_loss"], ins["in"], D.exchanged_geom(case), 32, 1)), case
        if which == "biases":
            assert D.within_f64_bound(bck_chain.biases_chain(ins["out_grad_loss"]), twin, case, which), case   # (the GPU launch's tree sum: another order than be=cpu's)


def test_cpu_crop_cases(cpu):
    for i, case in enumerate(crop_list()):
        check_crop(cpu, case, CROP_SEED + i)
