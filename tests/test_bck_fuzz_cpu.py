"""The seeded random-geometry sweeps of the backward kernels without a GPU: the case generators of tools/fuzz_bck.py, the one table of seeds and counts that
tests/test_gpu_bck_fuzz.py runs on be=hip, and the CHECKERS on those very cases -- so that a mismatch on the GPU can only be the kernel.

  * generators: pure functions of (n, seed); every case builds an op the annotators and the planner accept; the categories a .. g of fuzz_bck.conv_categories (and the
    bent pooling / LRN / flat / concat shapes) occur among the cases the GPU test uses -- counted here
  * conv cases: be=cpu's hip_bconv_in against torch float64 (mrd < 2e-4), oracle/bck_chain.py's one-slice chain bit-equal to be=cpu's filter gradient, in_grad_chain
    bit-equal to be=cpu's data gradient, biases_chain and the sliced chain of the plan the GPU test forces against float64 under FILTS_MRD -- the bounds of
    tests/test_bck_conv_cpu.py; where a float64 gradient is zero throughout, the bits are compared with +0 instead
  * pool / LRN / softmax / flat / concat cases: be=cpu bit for bit against tests/bck_ops_ref.py / tests/bck_pipe_ref.py, the float64 helpers under the bounds written
    in tests/test_gpu_bck_ops.py.  Max-pooling inputs are random normal (ties have measure zero); 2 of every 12 cases are quantised to five levels (ties everywhere)
  * ZINP forms (conv, pool, LRN): flagged be=cpu == unflagged be=cpu followed by hip_zero_if_non_pos, bit for bit; `in` is about half non-positive, +0 and -0 included

Counts: 5 lists of 12 conv cases + 4 multi-device ones, 12 cases each of pool / LRN / softmax / flat / concat + 9 multi-device ones = 133 cases; 6 s here (be=cpu and the chain emulators on every one of them)."""
import os
import sys

import numpy as np
import pytest

_TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if _TOOLS not in sys.path:
    sys.path.insert(0, _TOOLS)
import fuzz_bck as F

import bck_ops_ref as oref
import bck_pipe_ref as pref
from boda_amd import rtc as rtc_mod
from boda_amd.cnn_op import OpTune, add_bck_conv_annotations, add_bck_op_annotations, fuse_zero_if_in_non_pos, pipe_func_args
from boda_amd.op import UnsupErr
from boda_amd.rtc import make_rtc
from oracle import bck_chain as bc

from test_bck_conv_cpu import FILTS_MRD, bck_op, rand_ins, torch_grads
from test_bck_fuse_cpu import bits, bits_eq, then_zinp
from test_bck_ops_cpu import bck_lrn_op, labels, lrn_op, pool_op, softmax_op, spreading_op, zinp_data, zinp_op
from test_bck_pipe_cpu import ann, concat_op, dropout_op, reduce_op, run_func

# ---- the one table of seeds and counts (tests/test_gpu_bck_fuzz.py imports it)
N_CONV = 12                               # conv cases per parameter of a GPU test
N_OPS = 12                                # cases per non-conv family
CONV_SEEDS = (101, 102, 103, 104, 105)    # five lists of N_CONV geometries
IN_TILES = {"": 0, "32x128x16x1x4": 1, "64x64x16x2x2": 2, "128x256x16x2x4": 3}                                                  # data-gradient tile -> list
FTILES = {"": 0, "64x64x16x2x2x1x1": 1, "32x64x32x1x2x1x2": 2, "64x64x16x2x2x1x3": 3, "64x128x32x2x2x1x4": 4}               # filter-gradient tile -> list
ZINP_TILES = {"": 4, "64x128x16x1x2": 0}                                                                                       # flagged data gradient: tile -> list
OPS_SEEDS = {"pool": 201, "lrn": 301, "softmax": 401, "flat": 501, "concat": 601}
MULTI = {"conv": (4, 701), "pool": (3, 702), "lrn": (3, 703), "flat": (2, 704), "concat": (1, 705)}                            # devices=0:0: (count, seed)


def conv_list(k):
    return F.conv_cases(N_CONV, CONV_SEEDS[k])


def conv_data_seed(k, i):
    return 1000 * (k + 1) + i


def ops_list(fam):
    return getattr(F, fam + "_cases")(N_OPS, OPS_SEEDS[fam])


def with_imgs(case, i):
    """A multi-device case: the generator's geometry with B = 2 .. 5 (the images are what the devices share out)."""
    return (2 + i % 4,) + tuple(case[1:])


def multi_list(fam):
    n, seed = MULTI[fam]
    cases = getattr(F, fam + "_cases")(n, seed)
    return cases if fam == "flat" else [with_imgs(c, i) for i, c in enumerate(cases)]


def all_conv_cases():
    """Every conv case the GPU test runs, with its data seed: [(case, seed)]."""
    out = [(c, conv_data_seed(k, i)) for k in range(len(CONV_SEEDS)) for i, c in enumerate(conv_list(k))]
    return out + [(c, 9000 + i) for i, c in enumerate(multi_list("conv"))]


# ---- inputs (shared with the GPU file)
def zinp_in(shape, seed, nan=True):
    """A forward input as the folded ReLU gradient's condition: about half non-positive, a tenth each +0 and -0, and (where `nan`) NaN."""
    rng = np.random.default_rng([seed, 5])
    x = rng.uniform(-2, 2, shape).astype(np.float32)
    kind = rng.integers(0, 12, shape)
    x[kind == 0] = 0.0; x[kind == 1] = -0.0
    if nan:
        x[kind == 2] = np.nan
    return x


def pool_input(case, i, seed):
    """Random normal values; cases 5 and 11 of every 12 are quantised to five levels, so that most windows hold several maxima."""
    rng = np.random.default_rng([seed, 1])
    if i % 6 == 5:
        return rng.integers(-2, 3, case[:4]).astype(np.float32)
    return rng.standard_normal(case[:4]).astype(np.float32)


def pool_funcs(case):
    """-> (hip_pool_yx of the max pooling, hip_spreading of the case's avg, its flagged form)."""
    geom, avg = case[:7], case[7]
    fs = add_bck_op_annotations(spreading_op(*geom, avg=avg), OpTune())[0]
    return add_bck_op_annotations(pool_op(*geom), OpTune())[0], fs, fuse_zero_if_in_non_pos(fs)


def lrn_funcs(case):
    B, C, H, W, ls, alpha, beta, k = case
    fb = add_bck_op_annotations(bck_lrn_op(B, C, H, W, ls, alpha, beta, k), OpTune())[0]
    return add_bck_op_annotations(lrn_op(B, C, H, W, ls, alpha, beta, k), OpTune())[0], fb, fuse_zero_if_in_non_pos(fb)


def lrn_input(case, seed):
    rng = np.random.default_rng([seed, 2])
    return rng.uniform(-30, 30, case[:4]).astype(np.float32), rng.uniform(-2, 2, case[:4]).astype(np.float32)


def lrn_zinp_in(case, seed):
    """bck_lrn reads `in` at the element itself only, so for the flagged form it need not be the input `out` came from: the same range, half non-positive, +0 and -0."""
    return zinp_in(case[:4], seed, nan=False) * np.float32(15)


def softmax_input(case, seed):
    B, C = case[:2]
    rng = np.random.default_rng([seed, 3])
    lo, hi = ((-4.0, 4.0), (-6.0, -1.0))[seed % 2]   # every other case all negative: pel_max stays 0
    return rng.uniform(lo, hi, (B, C, 1, 1)).astype(np.float32), labels(B, C, seed)


def flat_reduce_inputs(n, size, seed):
    """n inputs of `size` floats; element 0 is -0 everywhere (the sum from +0 is +0) and element 1 tells the order of the chain: ((0 + 2^24) + 1) - 2^24 = 0."""
    rng = np.random.default_rng([seed, 4])
    xs = [rng.uniform(-3, 3, size).astype(np.float32) for _ in range(n)]
    for i, x in enumerate(xs):
        x[0] = -0.0
        if size > 1:
            x[1] = ([2.0 ** 24, 1.0, -(2.0 ** 24)] + [0.0] * 8)[i]
    return xs


def dropout_seeds(size, ratio, seed):
    """Three seeds: a plain one, one under which index + seed wraps past 2^32 inside the tensor, one under which the middle element hashes to exactly the threshold."""
    return [seed + 7, 2 ** 32 - 1 - size // 2, pref.dropout_seed_hitting(ratio, size // 2)]


def concat_inputs(case, seed):
    B, chans, H, W = case
    rng = np.random.default_rng([seed, 6])
    return [rng.uniform(-3, 3, (B, c, H, W)).astype(np.float32) for c in chans]


FILL = 7.0


def concat_round_trip(rtc, case, seed, run=run_func):
    """Every member into a wide tensor pre-filled with FILL -- after each call the ranges written so far hold their data and the others still the fill --, then every
    member split out again into a NaN-filled var.  -> the wide tensor."""
    B, chans, H, W = case
    xs = concat_inputs(case, seed)
    wide = np.full((B, sum(chans), H, W), FILL, np.float32)
    c0 = 0
    for f, x in zip(ann(concat_op(B, chans, H, W)), xs):
        wide = run(rtc, f, {"in": x, "out": wide})["out"]
        c0 += x.shape[1]
        want = np.concatenate([pref.concat_f32(xs)[:, :c0], np.full((B, sum(chans) - c0, H, W), FILL, np.float32)], axis=1)
        assert bits_eq(wide, want), (case, c0)
    for f, x in zip(ann(concat_op(B, chans, H, W, typ="Split")), xs):
        assert bits_eq(run(rtc, f, {"in": wide, "out": np.full(x.shape, np.nan, np.float32)})["out"], x), case
    return wide


def frac_of(got, want, bound):
    """mrd(got, want) / bound with mrd = max|got - want| / max|want|; where want is zero throughout, got must be +0 bit for bit (-> 0.0, or inf)."""
    want = np.asarray(want, np.float64)
    m = float(np.max(np.abs(want)))
    if m == 0.0:
        return 0.0 if np.all(bits(got) == 0) else float("inf")
    return float(np.max(np.abs(np.asarray(got, np.float64).reshape(want.shape) - want))) / m / bound


def filts_plan(ff, ftile):
    """(BK, KSL) of the filter gradient's launch: the forced tile's fields, or the planner's choice as explain_plan names it."""
    if ftile:
        f = ftile.split("x")
        return int(f[2]), int(f[6])
    plan = rtc_mod.explain_plan(ff)
    return int(plan.split()[1].split("_")[0].split("x")[2]), int(plan.split("ksl=")[1].split()[0])


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


# ---- the generators
def test_generators_are_pure_functions_of_n_and_seed():
    for gen in (F.conv_cases, F.pool_cases, F.lrn_cases, F.softmax_cases, F.flat_cases, F.concat_cases):
        assert gen(24, 5) == gen(24, 5) and gen(24, 5) != gen(24, 6) and len(gen(24, 5)) == 24
        assert gen(24, 5)[:8] == gen(8, 5)   # a longer list extends a shorter one


def test_conv_cases_stay_inside_their_ranges():
    for case in F.conv_cases(300, 3):
        B, C, H, W, OC, KH, KW, SY, SX, PY, PX = case
        assert 1 <= B <= 4 and C in F.CHANS and OC in F.CHANS and 1 <= H <= 24 and 1 <= W <= 24
        assert (1 <= KH <= 7 or KH == 11) and (1 <= KW <= 7 or KW == 11) and 1 <= SY <= 4 and 1 <= SX <= 4 and 0 <= PY < KH and 0 <= PX < KW
        assert H + 2 * PY >= KH and W + 2 * PX >= KW
        OH, OW = (H + 2 * PY - KH) // SY + 1, (W + 2 * PX - KW) // SX + 1
        assert 2.0 * B * OH * OW * OC * C * KH * KW <= F.FLOP_CAP
    cases = F.conv_cases(400, 4)
    share = lambda pred: sum(1 for c in cases if pred(c)) / len(cases)
    assert 0.2 < share(lambda c: c[5] != c[6]) < 0.5 and 0.2 < share(lambda c: c[7] != c[8]) < 0.5   # about a third non-square / unequal strides
    assert share(lambda c: 11 in c[5:7]) > 0.01
    for cat in "abcdefg":   # roughly one case in six each (d and g are also common by themselves)
        assert share(lambda c: cat in F.conv_categories(c)) > 0.12, cat


def test_conv_categories_among_the_gpu_cases():
    """Each of a .. g at least twice among the cases the GPU test uses -- and in every list of twelve at least once, so that each forced tile meets each branch."""
    cases = [c for c, _ in all_conv_cases()]
    assert len(cases) == len(CONV_SEEDS) * N_CONV + MULTI["conv"][0]
    count = {cat: sum(1 for c in cases if cat in F.conv_categories(c)) for cat in ("a", "b", "c", "d", "e", "e_odd", "e_small", "f", "g")}
    print("conv categories among the GPU cases:", count)
    assert all(v >= 2 for v in count.values()), count
    if N_CONV >= 8:
        for k in range(len(CONV_SEEDS)):
            for cat in "abcdefg":
                assert any(cat in F.conv_categories(c) for c in conv_list(k)), (k, cat)
    C = {c[1] for c in cases}
    assert min(C) < 32 and {33, 65} & C and {129, 130} & C   # a channel count on each side of the tile breaks
    assert set(IN_TILES.values()) | set(FTILES.values()) | set(ZINP_TILES.values()) == set(range(len(CONV_SEEDS)))


def test_every_conv_case_builds_and_plans():
    for case, _ in all_conv_cases():
        op = bck_op(*case)
        plan = rtc_mod.explain_plan(op)
        assert "bodahip_bconv_in" in plan and "bodahip_bconv_filts" in plan and "bodahip_bconv_biases" in plan
        for f in add_bck_conv_annotations(op, OpTune()):
            assert rtc_mod.explain_plan(f).startswith("bodahip_bconv_")
    for tiles, which in ((IN_TILES, 0), (ZINP_TILES, 0), (FTILES, 2)):   # the forced tiles are taken on the lists they run on
        for tile, k in tiles.items():
            for case in conv_list(k) if tile else []:
                f = add_bck_conv_annotations(bck_op(*case), OpTune())[which]
                assert rtc_mod.explain_plan(f, tile=tile).split()[1].startswith("x".join(tile.split("x")[:3]))


def test_non_conv_cases_build_plan_and_cover_their_shapes():
    pools = ops_list("pool") + multi_list("pool")
    for case in pools:
        for f in pool_funcs(case):
            assert rtc_mod.explain_plan(f).startswith("bodahip_")
        assert case[7] in (0, 1) and all(1 <= k <= 7 and 1 <= s <= 4 and 0 <= p < k for k, s, p in zip(case[4], case[5], case[6]))
    small = lambda c: c[2] + 2 * c[6][0] < c[4][0] or c[3] + 2 * c[6][1] < c[4][1]
    assert any(small(c) for c in pools) and any(c[5][0] > c[4][0] and c[5][1] <= c[4][1] for c in pools)            # a window above the plane; stride > kernel on y only
    assert any(c[4] == (c[2], c[3]) for c in pools) and any(c[6] == (c[4][0] - 1, c[4][1] - 1) and c[6] != (0, 0) for c in pools)   # a global window; pad = kernel - 1
    assert any(c[2] * c[3] > 256 for c in pools) and {0, 1} == {c[7] for c in pools}
    lrns = ops_list("lrn") + multi_list("lrn")
    for case in lrns:
        for f in lrn_funcs(case):
            assert rtc_mod.explain_plan(f).startswith("bodahip_")
        assert case[4] % 2 == 1 and 1 <= case[4] <= 15 and 1 <= case[1] <= 140 and 1e-4 <= case[5] <= 0.1 + 1e-9
    assert any(c[1] < c[4] for c in lrns) and any(c[1] % 8 == 0 for c in lrns) and any(c[1] % 8 for c in lrns) and any(7 <= c[4] <= 15 and c[1] < c[4] for c in lrns)
    assert {c[1] % 8 for c in F.lrn_cases(64, 1)} == set(range(8))
    for B, C, y, x in ops_list("softmax"):
        assert (y, x) == (1, 1) and [p.split()[0] for p in rtc_mod.explain_plan(softmax_op(B, C)).split(" | ")] == ["bodahip_softmax", "bodahip_sm_grad_and_loss", "bodahip_sum_loss_over_imgs"]
    with pytest.raises(UnsupErr):   # why softmax_cases keeps y = x = 1: a spatial softmax is refused by the op
        softmax_op(2, 10, y=2, x=3)
    flats = ops_list("flat") + multi_list("flat")
    for size, nin, ratio in flats:
        assert 1 <= size <= 5000 and 2 <= nin <= 8 and 0.0 < ratio < 1.0
        for f in (ann(reduce_op(nin, f"(dims=(v={size}))"))[0], ann(dropout_op(ratio, f"(dims=(v={size}))"))[0], add_bck_op_annotations(zinp_op((("v", size),)), OpTune())[0]):
            assert rtc_mod.explain_plan(f).startswith("bodahip_")
    sizes = {c[0] for c in F.flat_cases(16, 9)}
    assert {1, 2, 3, 4, 1023, 1024, 1025, 4096} <= sizes and {0.01, 0.99} <= {c[2] for c in ops_list("flat")}
    cats = ops_list("concat") + multi_list("concat")
    for B, chans, H, W in cats:
        assert 2 <= len(chans) <= 5 and all(1 <= c <= 9 for c in chans)
        for f in ann(concat_op(B, chans, H, W)) + ann(concat_op(B, chans, H, W, typ="Split")):
            assert rtc_mod.explain_plan(f).startswith("bodahip_")
    assert {(H * W) % 4 for _, _, H, W in ops_list("concat")} == {0, 1, 2, 3}
    starts = {(sum(ch[:j]) * H * W) % 4 for _, ch, H, W in ops_list("concat") for j in range(len(ch))}
    assert starts == {0, 1, 2, 3}   # runs start on a quad and at every offset off it


# ---- conv: the checkers on the GPU's cases
def check_conv_checkers(cpu, case, seed, ftile):
    op = bck_op(*case); geom = op.bck_conv_geom()
    ins = rand_ins(op, seed)
    fi, fb, ff = add_bck_conv_annotations(op, OpTune())
    ti, tf, tb = torch_grads(op, ins["in"], ins["filts"], ins["out_grad_loss"])
    gi = run_func(cpu, fi, ins)["in_grad_loss"]
    fr = {"in_grad_loss 2e-4": frac_of(gi, ti, 2e-4)}
    assert bits_eq(bc.in_grad_chain(ins["filts"], ins["out_grad_loss"], geom), gi), case
    gf = run_func(cpu, ff, ins)["filts_grad_loss"]
    I, J = bc.filts_operands(ins["in"], ins["out_grad_loss"], geom)
    assert bits_eq(bc.filts_sliced_chain(I, J, 32, 1, gf.shape), gf), case
    fr["filts (one slice) FILTS_MRD"] = frac_of(gf, tf, FILTS_MRD)
    bk, ksl = filts_plan(ff, ftile)
    fr[f"filts (sliced) FILTS_MRD"] = frac_of(bc.filts_sliced_chain(I, J, bk, ksl, gf.shape), tf, FILTS_MRD)
    fr["biases FILTS_MRD"] = frac_of(bc.biases_chain(ins["out_grad_loss"]), tb, FILTS_MRD)
    for name, v in fr.items():
        assert v < 1.0, (name, v, case)
    # pels behind the last window and pels no tap reaches: exactly +0
    B, C, H, W, OC, KH, KW, SY, SX, PY, PX = case
    OH, OW = geom["OH"], geom["OW"]
    yr = np.array([any(0 <= y + PY - fy and (y + PY - fy) % SY == 0 and (y + PY - fy) // SY < OH for fy in range(KH)) for y in range(H)])
    xr = np.array([any(0 <= x + PX - fx and (x + PX - fx) % SX == 0 and (x + PX - fx) // SX < OW for fx in range(KW)) for x in range(W)])
    assert np.all(bits(gi[:, :, ~yr, :]) == 0) and np.all(bits(gi[:, :, :, ~xr]) == 0), case
    return fr


@pytest.mark.parametrize("k", range(len(CONV_SEEDS)))
def test_cpu_conv_checkers_on_the_gpu_cases(cpu, k):
    ftile = [t for t, kk in FTILES.items() if kk == k][0]
    worst = {}
    for i, case in enumerate(conv_list(k)):
        for name, v in check_conv_checkers(cpu, case, conv_data_seed(k, i), ftile).items():
            worst[name] = max(worst.get(name, 0.0), v)
    print(f"conv list {k}: worst fraction of each bound on be=cpu / the chains:", {n: round(v, 4) for n, v in worst.items()})


def test_cpu_conv_checkers_on_the_multi_device_cases(cpu):
    for i, case in enumerate(multi_list("conv")):
        check_conv_checkers(cpu, case, 9000 + i, "")


def conv_zinp_ins(case, seed):
    op = bck_op(*case)
    return dict(rand_ins(op, seed), **{"in": zinp_in(op.get_dims("in").sizes, seed)})


def check_flagged_cpu(cpu, plain, flagged, ins):
    """flagged be=cpu == plain be=cpu followed by hip_zero_if_non_pos, bit for bit, from a NaN-filled in_grad_loss.  -> the flagged result."""
    g = run_func(cpu, plain, {k: v for k, v in ins.items() if k in dict(pipe_func_args(plain))})["in_grad_loss"]
    got = run_func(cpu, flagged, dict(ins, in_grad_loss=np.full(g.shape, np.nan, np.float32)))["in_grad_loss"]
    assert bits_eq(got, then_zinp(cpu, g, ins["in"])) and np.all(bits(got)[~(ins["in"] > 0)] == 0)
    return got


def test_cpu_conv_zinp_forms(cpu):
    for tile, k in ZINP_TILES.items():
        for i, case in enumerate(conv_list(k)):
            fi = add_bck_conv_annotations(bck_op(*case), OpTune())[0]
            ins = conv_zinp_ins(case, conv_data_seed(k, i))
            assert 0.3 < np.mean(~(ins["in"] > 0)) <= 1.0 or ins["in"].size < 16
            check_flagged_cpu(cpu, fi, fuse_zero_if_in_non_pos(fi), ins)


# ---- the non-conv families: be=cpu against the numpy restatements
def pool_case_cpu(cpu, case, i, seed):
    B, C, H, W, kern, stride, pad, avg = case
    fp, fs, ffs = pool_funcs(case)
    x = pool_input(case, i, seed)
    got = run_func(cpu, fp, {"in": x})
    out, yx = oref.pool_yx_f32(x, kern, stride, pad)
    assert bits_eq(got["out"], out) and bits_eq(got["out_in_yx"], yx), case
    ogl = np.random.default_rng([seed, 7]).uniform(-2, 2, out.shape).astype(np.float32)
    ins = {"out": out, "out_grad_loss": ogl, "out_in_yx": yx, "in": zinp_in(x.shape, seed)}
    igl = run_func(cpu, fs, ins)["in_grad_loss"]
    assert bits_eq(igl, oref.spreading_f32(ogl, yx, (H, W), kern, stride, pad, avg)), case
    check_flagged_cpu(cpu, fs, ffs, ins)
    return x, out


def test_cpu_pool_cases(cpu):
    ties = 0
    for i, case in enumerate(ops_list("pool")):
        x, out = pool_case_cpu(cpu, case, i, OPS_SEEDS["pool"] + i)
        ties += i % 6 == 5 and x.size > 8
    assert ties >= N_OPS // 12   # (a quantised case of more than a handful of elements)
    for i, case in enumerate(multi_list("pool")):
        pool_case_cpu(cpu, case, i, MULTI["pool"][1] + i)


def lrn_case_cpu(cpu, case, seed):
    B, C, H, W, ls, alpha, beta, k = case
    fl, fb, ffb = lrn_funcs(case)
    x, ogl = lrn_input(case, seed)
    got = run_func(cpu, fl, {"in": x})
    out, sb = oref.lrn_sb_f32(x, ls, alpha, beta, k)
    assert bits_eq(got["out_scale_base"], sb) and bits_eq(got["out"], out), case
    want = oref.lrn_out_f64(x, sb, beta)
    fr = {"lrn_sb out": float(np.max(np.abs(out - want) / np.maximum(8 * oref.U * np.abs(want), 1e-300)))}
    ins = {"in": x, "out": out, "out_grad_loss": ogl, "out_scale_base": sb}
    igl = run_func(cpu, fb, ins)["in_grad_loss"]
    assert bits_eq(igl, oref.bck_lrn_f32(x, out, ogl, sb, ls, alpha, beta, k)), case
    want, S = oref.bck_lrn_f64(x, out, ogl, sb, ls, alpha, beta, k)
    fr["bck_lrn in_grad_loss"] = float(np.max(np.abs(igl - want) / np.maximum(2 * (ls + 8) * oref.U * S, 1e-300)))
    assert all(v <= 1.0 for v in fr.values()), (fr, case)
    check_flagged_cpu(cpu, fb, ffb, dict(ins, **{"in": lrn_zinp_in(case, seed)}))
    return fr


def test_cpu_lrn_cases(cpu):
    worst = {}
    for i, case in enumerate(ops_list("lrn")):
        for n, v in lrn_case_cpu(cpu, case, OPS_SEEDS["lrn"] + i).items():
            worst[n] = max(worst.get(n, 0.0), v)
    for i, case in enumerate(multi_list("lrn")):
        lrn_case_cpu(cpu, case, MULTI["lrn"][1] + i)
    print("lrn cases: worst fraction of each bound on be=cpu:", {n: round(v, 3) for n, v in worst.items()})


def test_cpu_softmax_cases(cpu):
    for i, case in enumerate(ops_list("softmax")):
        B, C = case[:2]
        x, lab = softmax_input(case, OPS_SEEDS["softmax"] + i)
        fs, fg, fl = add_bck_op_annotations(softmax_op(B, C), OpTune())
        prob = run_func(cpu, fs, {"in": x})["prob"]
        assert bits_eq(prob, oref.softmax_f32(x)), case
        want = oref.softmax_f64(x)
        assert np.all(np.abs(prob - want) <= (C + 8) * oref.U * want), case
        got = run_func(cpu, fg, {"prob": prob, "label": lab})
        igl, lpp = oref.sm_grad_and_loss_f32(prob, lab)
        assert bits_eq(got["in_grad_loss"], igl) and bits_eq(got["loss_per_pel"], lpp), case
        wl = oref.loss_per_pel_f64(prob, lab)
        assert np.all(np.abs(lpp - wl) <= 4 * oref.U * np.maximum(1.0, np.abs(wl))), case
        assert bits_eq(run_func(cpu, fl, {"loss_per_pel": lpp})["loss"], oref.sum_loss_over_imgs_f32(lpp)), case


def flat_case_cpu(rtc, case, seed, run=run_func):
    """zero_if_non_pos (out of place, in place, as its own condition), reduce and dropout (three seeds) on one flat size, each against its numpy restatement."""
    size, nin, ratio = case
    x, cond = zinp_data(size, seed)
    fz = add_bck_op_annotations(zinp_op((("v", size),)), OpTune())[0]
    want = oref.zero_if_non_pos_f32(x, cond)
    nan = np.full(size, np.nan, np.float32)
    assert bits_eq(run(rtc, fz, {"in": x, "cond": cond, "out": nan})["out"], want), case
    assert bits_eq(run(rtc, fz, {"in": x, "cond": cond}, alias={"out": "in"})["out"], want), case
    assert bits_eq(run(rtc, fz, {"in": x}, alias={"out": "in", "cond": "in"})["out"], oref.zero_if_non_pos_f32(x, x)), case
    xs = flat_reduce_inputs(nin, size, seed)
    got = run(rtc, ann(reduce_op(nin, f"(dims=(v={size}))"))[0], dict({f"ins_{j}": v for j, v in enumerate(xs)}, out=nan))["out"]
    assert bits_eq(got, pref.reduce_f32(xs)) and bits(got)[0] == 0, case
    fd = ann(dropout_op(ratio, f"(dims=(v={size}))"))[0]
    for s in dropout_seeds(size, ratio, seed):
        assert bits_eq(run(rtc, fd, {"inout": x}, seed=s)["inout"], pref.dropout_f32(x, ratio, s)), (case, s)
    hit = dropout_seeds(size, ratio, seed)[2]
    assert pref.dropout_hash(size, hit)[size // 2] == pref.dropout_thresh(ratio)


def test_cpu_flat_cases(cpu):
    for i, case in enumerate(ops_list("flat")):
        flat_case_cpu(cpu, case, OPS_SEEDS["flat"] + i)


def test_cpu_concat_cases(cpu):
    for i, case in enumerate(ops_list("concat")):
        concat_round_trip(cpu, case, OPS_SEEDS["concat"] + i)
    for i, case in enumerate(multi_list("concat")):
        concat_round_trip(cpu, case, MULTI["concat"][1] + i)
