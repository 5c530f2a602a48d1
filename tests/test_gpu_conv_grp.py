"""The grouped convolution on the MI355X (kernels/conv_grp_f32.hip): hip_conv_grp, hip_bconv_in_grp and hip_bconv_filts_grp held to BITS.
  * hip_conv_grp / hip_bconv_in_grp equal be=cpu's hip_conv / hip_bconv_in on the op sliced per group (tests/conv_grp_ref.py: sliced)
  * hip_bconv_filts_grp equals oracle/bck_chain.filts_chain on the slices with the (BK, KSL) of the launch; with KSL = 1 also be=cpu's hip_bconv_filts on the slices
  * containment: an Inf or NaN in group 0's operands changes no bit outside group 0's outputs
Every output is NaN-filled before the call, a guard var stands in front of and behind every var and must keep its bits, and inputs keep their bits
(conv_grp_ref.run_func, guards=True).  Every case runs in BOTH forms, forced by tile -- the matrix form on 32 x 32 x 2 and on 16 x 16 x 4
blocks, with one and with several blocks per wave; the direct form -- and under the planner's own choice; so does the containment test: in the matrix form the first
case has both groups inside one tile's reach (rows 5..31 of a group's block are masked, never the neighbour's), the second one whole 32-row block per group."""
import numpy as np
import pytest

from boda_amd.rtc import make_rtc
from oracle import bck_chain

from conv_grp_ref import CASE_IDS, CASES, bck_op, bits_equal, grouped_funcs, mrd, rand_ins, run_func, slice_case, slice_ins, sliced, torch_twin
from test_bck_conv_cpu import FILTS_MRD

pytestmark = pytest.mark.gpu
FWD_MRD = 2e-4   # the forward tests' bound against float64 (the reference's max-rel-diff tolerance, src/rtc_prof.cc:161)


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


def ref(cpu, case, which):
    """be=cpu's ungrouped function on the slices, computed once per (case, function) and shared."""
    key = (case, which)
    if key not in _REF:
        _REF[key] = sliced(cpu, case, rand_ins(case, 11), which)
        _REF[key].setflags(write=False)
    return _REF[key]


def plan_of(launch):
    """(form, BK, KSL) of a grouped launch: the form from the kernel's name, BK and KSL from its configuration string BIxBJxBK_wWIxWJ[_sKSL]."""
    cfg = launch["cfg"]
    assert ("_m16" in cfg) == (launch["kernel"].endswith("_mfma") and int(cfg.split("_w")[0].split("x")[0]) // int(cfg.split("_w")[1].split("x")[0]) == 16)
    return launch["kernel"].rsplit("_", 1)[1], int(cfg.split("_")[0].split("x")[2]), (int(cfg.split("_s")[1].split("_")[0]) if "_s" in cfg else 1)


def chain(case, ins, BK, KSL):
    """oracle/bck_chain.filts_chain per group on the slices, side by side along the filter-row axis."""
    geom = bck_op(*slice_case(case), group_field=False).bck_conv_geom()
    parts = []
    for j in range(case[1]):
        s = slice_ins(case, ins, j)
        parts.append(bck_chain.filts_chain(s["in"], s["out_grad_loss"], geom, BK, KSL))
    return np.concatenate(parts, axis=0)


MATRIX_TILES = ("32x128x2x1x4x1x1", "64x128x2x1x2x1x1", "16x64x4x1x4x1x1", "32x64x8x2x2x1x1")   # 32-blocks, 2 x 2 of them per wave, 16-blocks (twice)
DIRECT_FWD_TILES = ("1x1x1x2x2x1x1", "1x2x1x2x2x1x1", "1x4x1x2x2x1x1")                            # one, two and four adjacent outputs per thread


def want_form(tile, launch):
    return tile == "" or plan_of(launch)[0] == ("mfma" if int(tile.split("x")[0]) > 1 else "direct")


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_forward_bits(hip, cpu, case):
    ins = rand_ins(case, 11)
    fc = grouped_funcs(case)[0]
    want = ref(cpu, case, "fwd")
    for tile in ("",) + MATRIX_TILES + DIRECT_FWD_TILES:
        got, launch = run_func(hip, fc, ins, tile, guards=True)
        assert launch["kernel"].startswith("bodahip_conv_grp_") and want_form(tile, launch), launch
        assert bits_equal(got, want), (case, tile, launch)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_data_gradient_bits(hip, cpu, case):
    ins = rand_ins(case, 11)
    fi = grouped_funcs(case)[1]
    want = ref(cpu, case, "in")
    for tile in ("",) + MATRIX_TILES + ("1x1x1x2x2x1x1",) + (("1x4x1x2x2x1x1",) if case[7] == 1 else ()):   # direct: one output a thread; four adjacent x (stride 1)
        got, launch = run_func(hip, fi, ins, tile, guards=True)
        assert launch["kernel"].startswith("bodahip_bconv_in_grp_") and want_form(tile, launch), launch
        assert bits_equal(got, want), (case, tile, launch)
        if case == CASES[4]:   # 1x1 at stride 2: the odd rows and columns meet no term and are +0 (and written: the output was NaN-filled)
            assert np.all(got[:, :, 1::2, :].view(np.uint32) == 0) and np.all(got[:, :, :, 1::2].view(np.uint32) == 0)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_filter_gradient_chain(hip, cpu, case):
    ins = rand_ins(case, 11)
    ff = grouped_funcs(case)[3]
    B, g, C, OC, H, W, k, s, p = case
    K = B * ((H + 2 * p - k) // s + 1) * ((W + 2 * p - k) // s + 1)
    got, launch = run_func(hip, ff, ins, runs=2, guards=True)   # the planner's default, held to the chain with its launched (BK, KSL); two runs into the same var
    form, BK, KSL = plan_of(launch)
    assert launch["kernel"] == "bodahip_bconv_filts_grp_" + form
    assert bits_equal(got, chain(case, ins, BK, KSL)), (case, launch)
    again, _ = run_func(hip, ff, ins, guards=True)
    assert bits_equal(got, again)   # the same bits on two runs
    bk_odd = next(b for b in (10, 14, 6, 22, 7) if K % b)   # a BK that does not divide B * OH * OW
    nkt = -(-K // 32)
    for bk, ksl in ((32, 1), (32, 2), (bk_odd, 3), (32, min(256, nkt + 1))):   # KSL 1, 2, 3 and one larger than the number of K steps (empty slices)
        got, launch = run_func(hip, ff, ins, f"1x1x{bk}x2x2x1x{ksl}", guards=True)
        assert plan_of(launch) == ("direct", bk, ksl), launch
        assert bits_equal(got, chain(case, ins, bk, ksl)), (case, bk, ksl)
        if ksl == 1:   # one slice: be=cpu's single chain on the slices, for any BK
            assert bits_equal(got, ref(cpu, case, "filts")), (case, bk)
    got, _ = run_func(hip, ff, ins, f"1x1x{bk_odd}x2x2x1x1", guards=True)
    assert bits_equal(got, ref(cpu, case, "filts")), (case, bk_odd)
    got, launch = run_func(hip, ff, ins, "1x1x4x2x2x1x300", guards=True)   # 300 slices: slabs in the call's workspace, added by the second launch (the launch record is the main kernel's)
    assert plan_of(launch) == ("direct", 4, 300), launch
    assert bits_equal(got, chain(case, ins, 4, 300)), case
    # the matrix form: the tile is one wave's, the workgroup's KSL (1..16) waves are its slices.  32- and 16-row blocks, two blocks per wave
    bk4 = next(b for b in (12, 20, 28, 44) if K % b)          # a multiple of both k steps that does not divide K
    bk_few = 4 * (-(-K // 40))                                # at most ten K steps: one slice more than that fits the 16 waves
    few = -(-K // bk_few) + 1
    for bi, bj, plans in ((32, 32, ((32, 1), (32, 2), (bk4, 3), (bk4, 1), (bk_few, few))), (16, 32, ((bk4, 3), (32, 1))), (32, 64, ((32, 2),))):
        for bk, ksl in plans:
            got, launch = run_func(hip, ff, ins, f"{bi}x{bj}x{bk}x1x1x1x{ksl}", guards=True)
            assert plan_of(launch) == ("mfma", bk, ksl) and launch["block"] == 64 * ksl, launch
            assert bits_equal(got, chain(case, ins, bk, ksl)), (case, bi, bj, bk, ksl)
            if ksl == 1:
                assert bits_equal(got, ref(cpu, case, "filts")), (case, bi, bj, bk)


def test_float64(hip):
    """One float64 check per function, on the AlexNet conv2 shrunk (the longest K of the list)."""
    case = CASES[2]
    ins = rand_ins(case, 11)
    fc, fi, _, ff = grouped_funcs(case)
    o, gi, gw = torch_twin(case, ins)
    assert mrd(run_func(hip, fc, ins)[0], o) < FWD_MRD
    assert mrd(run_func(hip, fi, ins)[0], gi) < 2e-4
    assert mrd(run_func(hip, ff, ins)[0], gw) < FILTS_MRD


@pytest.mark.parametrize("case", [CASES[0], CASES[5]], ids=[CASE_IDS[0], CASE_IDS[5]])
@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_containment(hip, case, bad):
    """Group 0's share of each operand in turn filled with NaN / Inf: every output outside group 0 keeps the bits of the clean run."""
    B, g, C, OC = case[:4]
    cg, ocg = C // g, OC // g
    clean = rand_ins(case, 11)
    fc, fi, _, ff = grouped_funcs(case)
    share = {"in": (slice(None), slice(0, cg)), "filts": (slice(0, ocg),), "biases": (slice(0, ocg),), "out_grad_loss": (slice(None), slice(0, ocg))}
    outside = {"fwd": lambda a: a[:, ocg:], "in": lambda a: a[:, cg:], "filts": lambda a: a[ocg:]}
    tiles = {"fwd": ("", "32x128x2x1x4x1x1", "16x64x4x1x4x1x1", "1x4x1x2x2x1x1"), "in": ("", "32x128x2x1x4x1x1", "16x64x4x1x4x1x1", "1x1x1x2x2x1x1"),
             "filts": ("", "32x32x32x1x1x1x2", "16x32x12x1x1x1x3", "1x1x32x2x2x1x2")}
    for which, f, operands in (("fwd", fc, ("in", "filts", "biases")), ("in", fi, ("filts", "out_grad_loss")), ("filts", ff, ("in", "out_grad_loss"))):
        for tile in tiles[which]:
            want = outside[which](run_func(hip, f, clean, tile)[0])
            for an in operands:
                ins = {k: v.copy() for k, v in clean.items()}
                ins[an][share[an]] = bad
                got = outside[which](run_func(hip, f, ins, tile)[0])
                assert bits_equal(got, want), (case, which, tile, an, bad)


def test_planner_chooses_the_form_from_the_op(hip):
    """AlexNet conv2 shrunk and the OCG = 32 case take the matrix form; the depthwise cases, the ragged CG = 3 case and the grouped 1x1 (8 terms) the direct form; the launch says which."""
    for case, form in ((CASES[2], "mfma"), (CASES[1], "mfma"), (CASES[3], "direct"), (CASES[5], "direct"), (CASES[7], "direct"), (CASES[0], "direct")):
        ins = rand_ins(case, 11)
        fc, fi, _, ff = grouped_funcs(case)
        forms = [plan_of(run_func(hip, f, ins)[1])[0] for f in (fc, ff)]
        assert forms == [form, form], (case, forms)
