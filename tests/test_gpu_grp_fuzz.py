"""Seeded random-geometry sweeps of the grouped convolution (kernels/conv_grp_f32.hip), the Deconvolution family (kernels/deconv_f32.hip) and hip_crop / hip_crop_bck on
the MI355X, on the cases of tools/fuzz_grp.py under the table of tests/test_grp_fuzz_cpu.py (which holds the definitions and the bounds on these very cases on be=cpu).

  * grouped: every function under the planner's choice and under every forced tile of tests/test_gpu_conv_grp.py, one parameter each, twelve geometries a parameter.
    Forward and data gradient equal be=cpu's ungrouped function on the slices by bits; the filter gradient equals oracle/bck_chain.filts_chain per group with the
    launched (BK, KSL) and, with one slice, be=cpu; each is also held to its float64 bound (FWD_MRD, 2e-4, FILTS_MRD against torch conv2d(groups) and autograd)
  * containment: group 0's share of each operand filled with NaN / Inf changes no bit outside group 0, on two random cases per form
  * Deconvolution: hip_deconv and hip_deconv_bck_in equal be=cpu by bits, hip_deconv_bck_filts equals filts_chain on the exchanged roles with the launched (BK, KSL) under
    the planner's tile and deconv_ref.filts_tiles, hip_deconv_bck_biases equals biases_chain, all within deconv_ref.within_f64_bound; the forced matrix path where the
    geometry allows it; the forward's grid equals fuzz_grp.deconv_fwd_grid, so that the chunk / pass categories counted on the host are what ran
  * Crop: both functions against numpy by bits
Every launch: NaN-filled outputs, a guard var in front of and behind every var, inputs that keep their bits (deconv_ref.run_func, guards=True), the function's own kernel,
under a forced tile the forced configuration; the planner's launch twice with the same bits.  The check_*_case functions are also what tools/fuzz_grp.py runs, in volume.

Measured on one MI355X (pytest --durations=0, a cold code-object cache: every geometry compiled by hiprtc), 42 tests in 77 s: the grouped forward's eight parameters
0.7-2.0 s each, the data gradient's seven 0.3-1.8 s, the filter gradient's ten 0.6-3.3 s (the sliced direct plans: 300 slabs emulated on the host), containment 0.03-1.0 s,
test_deconv_forward 3.7 s, test_deconv_data_and_bias_gradient 2.0 s, test_deconv_filter_gradient's seven 0.4-3.4 s, test_deconv_matrix_path 7.0 s, the Crop windows 2.4 s.
Largest observed fractions of the bounds: forward FWD_MRD 0.007, in_grad_loss 2e-4 0.002, filts_grad_loss FILTS_MRD 0.049; deconv fwd 0.625, in 0.286, filts 0.452,
biases 0.033 of (n + 1) * 2^-24 * sum |terms|.  No mismatch on these lists; with the direct filter gradient's quad test taken against K instead of the slice end, the
matrix data gradient's (tx, ty) order swapped, or the Deconvolution forward's SHARE form taken for every quad at SX >= 4, the sweeps fail (dodd_s3; the matrix
parameters; test_deconv_forward) where tests/test_gpu_conv_grp.py's nine cases see only the second and tests/test_gpu_deconv.py's eleven none of them."""
import numpy as np
import pytest

import conv_grp_ref as G
import deconv_ref as D
from boda_amd.cnn_op import OpTune, deconv_form
from boda_amd.rtc import make_rtc
from oracle import bck_chain

from test_grp_fuzz_cpu import (CONTAIN, DECONV_HAND, GRP_BOUND, GRP_LISTS, PARAMS, check_crop, crop_list, deconv_data_seed, deconv_frac, deconv_list, grp_data_seed,
                               grp_filts_chain, grp_func, grp_list, grp_tile, grp_twin, CROP_SEED, F)
from test_bck_fuzz_cpu import frac_of

pytestmark = pytest.mark.gpu
WORST = {}   # bound name -> largest observed fraction of it
USED = {}    # "kernel cfg" -> launches
KERNEL = {"fwd": "bodahip_conv_grp_", "in": "bodahip_bconv_in_grp_", "filts": "bodahip_bconv_filts_grp_"}


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


def note(launch):
    key = launch["kernel"].replace("bodahip_", "") + " " + launch.get("cfg", "")
    USED[key] = USED.get(key, 0) + 1
    return key


def same_bits(what, case, cfg, got, want):
    if got.shape != want.shape:
        raise Mismatch(what + f" (shape {got.shape} against {want.shape})", case, cfg, got.size, want.size)
    g, w = np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32)
    if not np.array_equal(g, w):
        raise Mismatch(what, case, cfg, int((g != w).sum()), w.size)


def under(name, case, cfg, frac):
    WORST[name] = max(WORST.get(name, 0.0), frac)
    if not frac <= 1.0:
        raise Mismatch(f"{name}: {frac:.3g} of the bound", case, cfg, 1, 1)


def plan_of(launch):
    """(form, BK, KSL) of a grouped launch: the form from the kernel's name, BK and KSL from its configuration string BIxBJxBK_wWIxWJ[_m16][_sKSL]."""
    cfg = launch["cfg"]
    return launch["kernel"].rsplit("_", 1)[1], int(cfg.split("_")[0].split("x")[2]), (int(cfg.split("_s")[1].split("_")[0]) if "_s" in cfg else 1)


_REF = {}


def cached(kind, case, seed, which, make):
    """A reference computed once per (case, data seed, function) and shared by the parameters that run the case; read-only."""
    key = (kind, case, seed, which)
    if key not in _REF:
        if len(_REF) > 400:   # (a volume run of tools/fuzz_grp.py)
            _REF.clear()
        _REF[key] = make()
        for a in (_REF[key].values() if isinstance(_REF[key], dict) else [_REF[key]]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _REF[key]


# ---- the grouped functions
def check_grp_case(hip, cpu, case, seed, func, tile=""):
    ins = G.rand_ins(case, seed)
    f = grp_func(case, func)
    got, launch = D.run_func(hip, f, ins, tile, guards=True)
    cfg = note(launch)
    form, BK, KSL = plan_of(launch)
    assert launch["kernel"] == KERNEL[func] + form and form in ("direct", "mfma"), launch
    if tile:   # the launched configuration is the forced one
        t = tile.split("x")
        assert form == ("mfma" if int(t[0]) > 1 else "direct") and launch["cfg"].startswith("x".join(t[:3]) + "_w" + "x".join(t[3:5])) and KSL == int(t[6]), (tile, launch)
        assert ("_m16" in launch["cfg"]) == (form == "mfma" and int(t[0]) // int(t[3]) == 16), (tile, launch)
    if func == "filts" and form == "mfma":
        assert launch["block"] == 64 * KSL, launch
    ref = lambda: cached("sliced", case, seed, func, lambda: G.sliced(cpu, case, ins, func))
    if func == "filts":
        same_bits(f"filts_grad_loss against the per-group chain of BK={BK}, {KSL} slices", case, cfg, got, grp_filts_chain(case, ins, BK, KSL))
        if KSL == 1:
            same_bits("filts_grad_loss against be=cpu on the slices", case, cfg, got, ref())
    else:
        same_bits(f"{func} against be=cpu on the slices", case, cfg, got, ref())
    name, bound = GRP_BOUND[func]
    under(name, case, cfg, frac_of(got, cached("twin", case, seed, "", lambda: grp_twin(case, ins))[func], bound))
    if not tile:   # the planner's launch twice: the same bits
        again, _ = D.run_func(hip, f, ins, tile, runs=2, guards=True)
        same_bits(f"{func}: a second and third run", case, cfg, again, got)


@pytest.mark.parametrize("pid", list(PARAMS["fwd"]))
def test_grouped_forward(hip, cpu, pid):
    key, name = PARAMS["fwd"][pid]
    for i, case in enumerate(grp_list(key)):
        check_grp_case(hip, cpu, case, grp_data_seed(key, i), "fwd", grp_tile(key, name, case))


@pytest.mark.parametrize("pid", list(PARAMS["in"]))
def test_grouped_data_gradient(hip, cpu, pid):
    key, name = PARAMS["in"][pid]
    for i, case in enumerate(grp_list(key)):
        check_grp_case(hip, cpu, case, grp_data_seed(key, i), "in", grp_tile(key, name, case))


@pytest.mark.parametrize("pid", list(PARAMS["filts"]))
def test_grouped_filter_gradient(hip, cpu, pid):
    key, name = PARAMS["filts"][pid]
    for i, case in enumerate(grp_list(key)):
        check_grp_case(hip, cpu, case, grp_data_seed(key, i), "filts", grp_tile(key, name, case))


CONTAIN_TILES = {
    "direct": {"fwd": ("", "1x4x1x2x2x1x1"), "in": ("", "1x1x1x2x2x1x1"), "filts": ("", "1x1x32x2x2x1x2")},
    "matrix": {"fwd": ("32x128x2x1x4x1x1", "16x64x4x1x4x1x1"), "in": ("32x128x2x1x4x1x1", "16x64x4x1x4x1x1"), "filts": ("32x32x32x1x1x1x2", "16x32x12x1x1x1x3")},
}


@pytest.mark.parametrize("form", list(CONTAIN))
@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_containment(hip, form, bad):
    """Group 0's share of each operand in turn filled with NaN / Inf: every output outside group 0 keeps the bits of the clean run (tests/test_gpu_conv_grp.py's scheme)."""
    for key, i in CONTAIN[form]:
        case = grp_list(key)[i]
        g, C, OC = case[1:4]
        cg, ocg = C // g, OC // g
        clean = G.rand_ins(case, grp_data_seed(key, i))
        fc, fi, _, ff = G.grouped_funcs(case)
        share = {"in": (slice(None), slice(0, cg)), "filts": (slice(0, ocg),), "biases": (slice(0, ocg),), "out_grad_loss": (slice(None), slice(0, ocg))}
        outside = {"fwd": lambda a: a[:, ocg:], "in": lambda a: a[:, cg:], "filts": lambda a: a[ocg:]}
        for which, f, operands in (("fwd", fc, ("in", "filts", "biases")), ("in", fi, ("filts", "out_grad_loss")), ("filts", ff, ("in", "out_grad_loss"))):
            for tile in CONTAIN_TILES[form][which]:
                want, launch = D.run_func(hip, f, clean, tile, guards=True)
                for an in operands:
                    ins = {k: v.copy() for k, v in clean.items()}
                    ins[an][share[an]] = bad
                    got, _ = D.run_func(hip, f, ins, tile, guards=True)
                    same_bits(f"containment: {which} outside group 0 with {bad} in group 0's {an}", case, note(launch), outside[which](got), outside[which](want))


# ---- the Deconvolution family
def deconv_refs(cpu, case, seed):
    ins = D.rand_ins(case, seed)
    funcs = D.deconv_funcs(case)
    return cached("deconv", case, seed, "", lambda: dict({w: D.run_func(cpu, funcs[w], ins)[0] for w in ("fwd", "in", "filts")}, twin=D.torch_twin(case, ins)))


def check_deconv_fwd(hip, cpu, case, seed):
    ins, f, refs = D.rand_ins(case, seed), D.deconv_funcs(case)["fwd"], deconv_refs(cpu, case, seed)
    got, launch = D.run_func(hip, f, ins, runs=2, guards=True)
    cfg = note(launch)
    assert launch["kernel"] == "bodahip_deconv_direct", launch
    grid, zs, per, _ = F.deconv_fwd_grid(case, hip.get_device_info()["num_cus"])
    assert launch["grid"] == grid, (case, launch, grid, zs, per)   # deconv_grid, restated: the chunks and passes counted on the host are what ran
    same_bits("deconv forward against be=cpu", case, cfg, got, refs["fwd"])
    same_bits("deconv forward: a third run", case, cfg, D.run_func(hip, f, ins)[0], got)
    under("deconv fwd bound", case, cfg, deconv_frac(got, refs["twin"], case, "fwd"))


def check_deconv_in(hip, cpu, case, seed):
    ins, funcs, refs = D.rand_ins(case, seed), D.deconv_funcs(case), deconv_refs(cpu, case, seed)
    got, launch = D.run_func(hip, funcs["in"], ins, runs=2, guards=True)
    cfg = note(launch)
    assert launch["kernel"] == "bodahip_deconv_bck_in_direct", launch
    same_bits("deconv data gradient against be=cpu", case, cfg, got, refs["in"])
    same_bits("deconv data gradient: a third run", case, cfg, D.run_func(hip, funcs["in"], ins)[0], got)
    under("deconv in bound", case, cfg, deconv_frac(got, refs["twin"], case, "in"))
    got, launch = D.run_func(hip, funcs["biases"], ins, guards=True)
    assert launch["kernel"] == "bodahip_bconv_biases", launch
    same_bits("deconv bias gradient against biases_chain", case, note(launch), got, bck_chain.biases_chain(ins["out_grad_loss"]))
    under("deconv biases bound", case, cfg, deconv_frac(got, refs["twin"], case, "biases"))


def check_deconv_filts(hip, cpu, case, seed, plan):
    """plan: -1 = the planner's tile, else an index into deconv_ref.filts_tiles(case)."""
    ins, f, refs = D.rand_ins(case, seed), D.deconv_funcs(case)["filts"], deconv_refs(cpu, case, seed)
    tile, bk, ksl = ("", 0, 0) if plan < 0 else D.filts_tiles(case)[plan]
    got, launch = D.run_func(hip, f, ins, tile, runs=1 if tile else 2, guards=True)
    cfg = note(launch)
    assert launch["kernel"] == "bodahip_deconv_bck_filts_direct", launch
    BK, KSL = D.cfg_bk_ksl(launch)
    assert not tile or (BK, KSL) == (bk, ksl), (tile, launch)
    same_bits(f"deconv filter gradient against the chain of BK={BK}, {KSL} slices", case, cfg, got,
              bck_chain.filts_chain(ins["out_grad_loss"], ins["in"], D.exchanged_geom(case), BK, KSL))   # (in := out_grad_loss, out_grad_loss := in)
    if KSL == 1:
        same_bits("deconv filter gradient against be=cpu", case, cfg, got, refs["filts"])
    if not tile:
        same_bits("deconv filter gradient: a third run", case, cfg, D.run_func(hip, f, ins)[0], got)
    under("deconv filts bound", case, cfg, deconv_frac(got, refs["twin"], case, "filts", KSL))
    assert D.within_f64_bound(got, refs["twin"], case, "filts", KSL), (case, launch)


def check_deconv_matrix(hip, cpu, case, seed):
    """The forced matrix path (and the planner's, where it chooses it) bound by role as a driver binds it: tests/test_gpu_deconv.py's test_matrix_path."""
    ins, refs, geom, OC = D.rand_ins(case, seed), deconv_refs(cpu, case, seed), D.exchanged_geom(case), case[4]
    for form in ("matrix",) + (("",) if deconv_form(D.deconv_op(case), OpTune()) == "matrix" else ()):
        op, calls = D.path_calls(case, "fwd", form)
        got, launches = D.run_calls(hip, op, calls, ins, "fwd", guards=True)
        assert launches[1]["kernel"] == "bodahip_chan_affine" and launches[0]["kernel"].startswith("bodahip_bconv_in"), launches
        cfg = note(launches[0])
        acc = bck_chain.in_grad_chain(ins["filts"], ins["in"], geom, D.cfg_bk_ksl(launches[0])[0])
        same_bits("deconv matrix forward against in_grad_chain + bias", case, cfg, got, (acc * np.float32(1.0) + ins["biases"].reshape(1, OC, 1, 1)).astype(np.float32))
        same_bits("deconv matrix forward against be=cpu", case, cfg, got, refs["fwd"])
        op, calls = D.path_calls(case, "in", form)
        got, launches = D.run_calls(hip, op, calls, ins, "in", guards=True)
        assert not launches[0]["kernel"].startswith("bodahip_deconv"), launches
        same_bits("deconv matrix data gradient against be=cpu", case, note(launches[0]), got, refs["in"])
        op, calls = D.path_calls(case, "filts", form)
        got, launches = D.run_calls(hip, op, calls, ins, "filts", guards=True)
        assert launches[0]["kernel"].startswith("bodahip_bconv_filts"), launches
        bk, ksl = D.cfg_bk_ksl(launches[0])
        same_bits(f"deconv matrix filter gradient against the chain of BK={bk}, {ksl} slices", case, note(launches[0]), got,
                  bck_chain.filts_chain(ins["out_grad_loss"], ins["in"], geom, bk, ksl))
        under("deconv filts bound", case, cfg, deconv_frac(got, refs["twin"], case, "filts", ksl))


def check_deconv_case(hip, cpu, case, seed):
    check_deconv_fwd(hip, cpu, case, seed)
    check_deconv_in(hip, cpu, case, seed)
    for plan in range(-1, len(D.filts_tiles(case))):
        check_deconv_filts(hip, cpu, case, seed, plan)
    if D.can_matrix(case):
        check_deconv_matrix(hip, cpu, case, seed)


def test_deconv_forward(hip, cpu):
    for i, case in enumerate(deconv_list()):
        check_deconv_fwd(hip, cpu, case, deconv_data_seed(i))


def test_deconv_hand_made_cases_reach_their_branches_on_this_device(hip):
    cus = hip.get_device_info()["num_cus"]
    assert all("passes" in F.deconv_categories(c, cus) for c in DECONV_HAND[:2]) and {"chunks", "ragged_chunk"} <= F.deconv_categories(DECONV_HAND[1], cus), cus
    assert sum(1 for c in deconv_list() if "chunks" in F.deconv_categories(c, cus)) >= 2 and all("lds_chunks" in F.deconv_categories(c, cus) for c in DECONV_HAND[2:])


def test_deconv_data_and_bias_gradient(hip, cpu):
    for i, case in enumerate(deconv_list()):
        check_deconv_in(hip, cpu, case, deconv_data_seed(i))


@pytest.mark.parametrize("plan", range(-1, 6), ids=["planner", "bk32_s1", "bk32_s2", "odd_s3", "odd_s1", "one_empty_slice", "bk1_many"])
def test_deconv_filter_gradient(hip, cpu, plan):
    for i, case in enumerate(deconv_list()):
        assert len(D.filts_tiles(case)) == 6
        check_deconv_filts(hip, cpu, case, deconv_data_seed(i), plan)


M_CASES = [(i, c) for i, c in enumerate(deconv_list()) if D.can_matrix(c)]   # (a property of the geometry: strides above 16 have no matrix path)


def test_deconv_matrix_path(hip, cpu):
    assert len(M_CASES) >= 8
    for i, case in M_CASES:
        check_deconv_matrix(hip, cpu, case, deconv_data_seed(i))


# ---- Crop
def check_crop_case(hip, case, seed):
    check_crop(hip, case, seed, kernel_names=True)


def test_crop_random_windows(hip):
    for i, case in enumerate(crop_list()):
        check_crop_case(hip, case, CROP_SEED + i)


def test_zz_report_worst_fractions_of_the_bounds():
    """Not a check of its own: prints what the sweeps above measured (run with -s) and the kernels / tile configs they launched."""
    for name in sorted(WORST):
        print(f"largest observed fraction of the bound, {name}: {WORST[name]:.3f}")
    print("kernels / tile configs used:", dict(sorted(USED.items(), key=lambda kv: -kv[1])))
    assert all(v <= 1.0 for v in WORST.values())
