"""The seeded random-geometry sweeps of the FORWARD kernels without a GPU: the case generators of tools/fuzz_fwd.py, the one table of seeds and counts that
tests/test_gpu_fwd_fuzz.py runs on be=hip, the input data both files share, and the REFERENCE SIDE on those very cases -- so that a mismatch on the GPU can only be
the kernel.

  * generators: pure functions of (n, seed); every case builds an op the annotators and the planner accept, or a pipe that ConvPipeFwd lays out on a recording backend
    (with the function forms the GPU file expects: fwd_pool__ / fwd_lrn__ and their BODAHIP_POOL_UNCOND / BODAHIP_LRN_FASTPOW switches, nhwc_pool / nhwc_pool_c...,
    nhwc_lrn / nhwc_lrn_c..., the fused pairs), or is refused by UnsupErr where the project documents a refusal (a forced channels-last tile the layer's kernel does
    not take); the categories of fuzz_fwd.pool_categories / lrn_categories / conv_categories occur on the lists as used -- counted here
  * conv / sgemm: the oracle against torch float64 on every case (on the bf16-rounded operands for the bf16 families) under mrd < 2e-4, the bound of that pair in
    tests/test_bck_conv_cpu.py / tests/test_gpu_parity.py; be=cpu's hip_conv and hip_sgemm (the functions be=cpu carries) bit-equal to the oracle, from a poisoned output
  * pool / LRN: bo.pool_fwd and bo.lrn_fwd against a numpy float64 restatement of the formulas in the oracle's comments (oracle/boda_oracle.c).  A maximum is equal,
    -FLT_MAX on a window wholly in the padding; an average is NaN exactly on those windows and elsewhere within one fp32 rounding of the result plus the rounding of
    the n - 1 additions in front of it ((n - 1) 2^-24 mean|v|: an fp32 chain of n terms is not within ONE rounding of the exact sum; against the same chain in
    fp32 -- x outer, y inner -- it is bit-equal, asserted too).  LRN, relative to float64, largest distance measured on these cases per alpha:
        alpha 1e-4: 1.42e-7     alpha 2e-2: 2.43e-7     alpha 0.5: 2.75e-6       (the carried sum loses digits as alpha grows); twice that is asserted (LRN_F64_BOUND)
  * data: max-pool inputs are random normal; cases 6 and 8 of every twelve are quantised to five levels (ties everywhere); cases 4 and 10 hold -0, +-Inf and NaN
    (max pooling, ReLU, Concat and the layout passes; `v > acc` drops a NaN, in the oracle as in the kernels)

Counts: 12 cases per list; 2 lists each of conv and conv_bf16, one each of winograd, k1s, nhwc_conv, sgemm, pool, lrn, pool_lrn_pair, elementwise = 144 cases; 5 s here."""
import os
import sys

import numpy as np
import pytest

_TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if _TOOLS not in sys.path:
    sys.path.insert(0, _TOOLS)
import fuzz_fwd as F

import fwd_special_ref as R
from boda_amd import rtc as rtc_mod
from boda_amd.cnn_op import OpTune, add_codegen_annotations
from boda_amd.conv_pipe import ConvPipe, ConvPipeFwd, DryRtc, PipeOp
from boda_amd.op import Dims, UnsupErr
from boda_amd.rtc import make_rtc
from oracle import boda_oracle as bo

from test_bck_conv_cpu import mrd

# ---- the one table of seeds and counts (tests/test_gpu_fwd_fuzz.py imports it)
N = 12                                                                   # cases per list
TILES = {"conv": {"": 0, "64x64x32x2x2x1x1x32x4": 1},                    # family -> {forced tile ("": the planner's): list}
         "conv_bf16": {"": 0, "32x64x32x1x2": 1}}
SEEDS = {"conv": (1101, 1102), "conv_bf16": (1201, 1202), "winograd": (1301,), "k1s": (1401,), "nhwc_conv": (1501,), "sgemm": (1601,),
         "pool": (1701,), "lrn": (1801,), "pool_lrn_pair": (1901,), "elementwise": (2001,)}
MRD = 2e-4                                                               # oracle <-> float64 (tests/test_bck_conv_cpu.py, tests/test_gpu_parity.py)
LRN_F64_BOUND = {1e-4: 2 * 1.42e-7, 2e-2: 2 * 2.43e-7, 0.5: 2 * 2.75e-6}      # twice the largest relative distance measured on the lists below (see the docstring)
NHWC_TUNE = dict(hip_dtype="bf16", hip_layout="nhwc")
U32, FLT_MAX = 2.0 ** -24, np.float32(3.402823466e+38)


def cases(fam, k=0):
    return getattr(F, fam + "_cases")(N, SEEDS[fam][k])


def data_seed(fam, k, i):
    return SEEDS[fam][k] * 100 + i


# ---- inputs (shared with the GPU file)
def conv_data(shape, seed):
    B, C, H, W, OC, KH, KW, S, P = shape
    rng = np.random.default_rng([seed, 1])
    return {"in": rng.uniform(-5, 5, (B, C, H, W)).astype(np.float32), "filts": rng.uniform(-5, 5, (OC, C, KH, KW)).astype(np.float32), "biases": rng.uniform(-5, 5, OC).astype(np.float32)}


def sgemm_data(geom, seed):
    M, N_, K = geom
    rng = np.random.default_rng([seed, 2])
    return {"a": rng.uniform(-5, 5, (K, M)).astype(np.float32), "b": rng.uniform(-5, 5, (K, N_)).astype(np.float32)}


def special(x, seed):
    """A twelfth each of -0, +Inf, -Inf and NaN (two bit patterns) over x, in place."""
    rng = np.random.default_rng([seed, 3])
    kind = rng.integers(0, 12, x.shape)
    x[kind == 0] = -0.0; x[kind == 1] = np.inf; x[kind == 2] = -np.inf
    R.bits(x)[kind == 3] = np.where(rng.integers(0, 2, int((kind == 3).sum())) == 0, 0x7FC00000, 0xFFC00001).astype(np.uint32)
    return x


def pool_input(case, i, seed):
    """Random normal; slots 6 and 8 of every twelve quantised to five levels; slots 4 and 10 with special values where the case is a maximum."""
    rng = np.random.default_rng([seed, 4])
    shape = case[:4]
    if i % 12 in (6, 8):
        return rng.integers(-2, 3, shape).astype(np.float32)
    x = (rng.standard_normal(shape) * 3).astype(np.float32)
    return special(x, seed) if (i % 12 in (4, 10) and not case[7]) else x


def lrn_input(case, seed):
    return (np.random.default_rng([seed, 5]).standard_normal(case[:4]) * 3).astype(np.float32)


def elementwise_inputs(case, i, seed):
    """Three tensors of the case's channel counts; slots 4 and 10 of every twelve with special values, slots 6 and 8 with many exact zeros of both signs."""
    B, chans, H, W = case
    rng = np.random.default_rng([seed, 6])
    xs = [(rng.standard_normal((B, c, H, W)) * 3).astype(np.float32) for c in chans]
    if i % 12 in (4, 10):
        xs = [special(x, seed + j) for j, x in enumerate(xs)]
    if i % 12 in (6, 8):
        for x in xs:
            z = rng.integers(0, 4, x.shape); x[z == 0] = 0.0; x[z == 1] = -0.0
    return xs


# ---- pipes (shared with the GPU file)
def _dims(B, C, H, W):
    return Dims.make("float", img=B, chan=C, y=H, x=W)


def pool_pipe(case):
    B, C, H, W, kern, stride, pad, avg = case
    return ConvPipe("fzp", "data", _dims(B, C, H, W)).add(PipeOp("p", "Pooling", "data", "p", kern_sz=kern, stride=stride, in_pad=pad, avg_pool=avg))


def lrn_pipe(case):
    B, C, H, W, ls, alpha, beta, k = case
    return ConvPipe("fzl", "data", _dims(B, C, H, W)).add(PipeOp("l", "LRN", "data", "l", lrn=(ls, alpha, beta, k)))


def pair_pipe(case):
    """data -> x0 (a 1 x 1 max pooling: the identity, so that the pair does not read the net's input, which ConvPipeFwd keeps apart) -> a -> b."""
    B, C, H, W, lrn_first, (kern, stride, pad), lrn = case
    p = ConvPipe("fzq", "data", _dims(B, C, H, W)).add(PipeOp("x0", "Pooling", "data", "x0", kern_sz=(1, 1), stride=(1, 1)))
    pool = lambda bot: PipeOp("p", "Pooling", bot, "p", kern_sz=kern, stride=stride, in_pad=pad)
    norm = lambda bot: PipeOp("l", "LRN", bot, "l", lrn=lrn)
    return p.add(norm("x0")).add(pool("l")) if lrn_first else p.add(pool("x0")).add(norm("p"))


def elt_pipe(case):
    """data -> sm (3 x 3 / 1 pad 1 average: a second tensor of the same dims); e0 = data + sm; e1 = ReLU(sm + data); last, a stand-alone ReLU in place on data itself
    (the only node of a pipe without convolutions that holds the NaNs as given: a maximum drops them)."""
    B, chans, H, W = case
    p = ConvPipe("fze", "data", _dims(B, chans[0], H, W))
    p.add(PipeOp("sm", "Pooling", "data", "sm", kern_sz=(3, 3), stride=(1, 1), in_pad=(1, 1), avg_pool=1))
    p.add(PipeOp("e0", "Eltwise", "data", "e0", bots=("data", "sm")))
    p.add(PipeOp("e1", "Eltwise", "sm", "e1", bots=("sm", "data"))).add(PipeOp("e1r", "ReLU", "e1", "e1"))
    return p.add(PipeOp("rr", "ReLU", "data", "data"))


def pipe_fwd(rtc, cp, nhwc, spec=True, **kw):
    fwd = ConvPipeFwd(rtc, OpTune(**NHWC_TUNE) if nhwc else None, spec_fwd=spec, **kw)
    fwd.init(cp, op_params={})
    return fwd


def call_names(fwd):
    return {c.tag: c.rfc.rtc_func_name for c in fwd.fwd_calls}


def pool_nonempty_small(case):
    """What sends a pooling to the specialised forms: every window meets the plane, at most 64 taps."""
    kern = F.pool_geom(case)[0]
    return sum(F.empty_windows(case)) == 0 and kern[0] * kern[1] <= 64


def expect_pool_name(case, nhwc, spec):
    if not nhwc:
        return "fwd_pool__"
    return "nhwc_pool_c" if (spec and pool_nonempty_small(case)) else "nhwc_pool"


def expect_lrn_name(case, nhwc, spec):
    if not nhwc:
        return "fwd_lrn__"
    return "nhwc_lrn_c" if (spec and case[4] % 2 == 1) else "nhwc_lrn"


def name_is(name, want):
    """`want` ending in _c or __: a prefix (a specialised / generated function); otherwise the generic function's whole name."""
    return name.startswith(want) if want.endswith(("_c", "__")) else name == want


# ---- numpy float64 restatements (oracle/boda_oracle.c: the comments above bo_pool_fwd and bo_lrn_fwd)
def pool_f64(x, case):
    """Padding never takes part; a maximum starts from -FLT_MAX and keeps what `v > acc` keeps (a NaN is dropped); an average divides the sum of the in-plane taps by
    their number (0 / 0 on a window wholly in the padding).  -> (out float64, taps per window, mean |v| per window)."""
    B, C, H, W = x.shape
    kern, stride, pad, OH, OW = F.pool_geom(case)
    avg = case[7]
    xd = x.astype(np.float64)
    out = np.empty((B, C, OH, OW)); taps = np.zeros((OH, OW), int); mag = np.zeros((B, C, OH, OW))
    for oy in range(OH):
        ya, yb = max(0, oy * stride[0] - pad[0]), min(H, oy * stride[0] - pad[0] + kern[0])
        for ox in range(OW):
            xa, xb = max(0, ox * stride[1] - pad[1]), min(W, ox * stride[1] - pad[1] + kern[1])
            win = xd[:, :, ya:max(ya, yb), xa:max(xa, xb)].reshape(B, C, -1)
            n = taps[oy, ox] = win.shape[2]
            if avg:
                with np.errstate(invalid="ignore", divide="ignore"):
                    out[:, :, oy, ox] = win.sum(axis=2) / n
                    mag[:, :, oy, ox] = np.abs(win).sum(axis=2) / max(n, 1)
            else:
                out[:, :, oy, ox] = np.fmax.reduce(win, axis=2, initial=-float(FLT_MAX))      # (fmax drops a NaN; -Inf stays below the start value)
    return out, taps, mag


def pool_f32_chain(x, case):
    """An average as the fp32 chain the oracle's comment fixes: columns outer, rows inner, from +0, one fp32 division by the tap count."""
    B, C, H, W = x.shape
    kern, stride, pad, OH, OW = F.pool_geom(case)
    out = np.empty((B, C, OH, OW), np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for oy in range(OH):
            ya, yb = max(0, oy * stride[0] - pad[0]), min(H, oy * stride[0] - pad[0] + kern[0])
            for ox in range(OW):
                xa, xb = max(0, ox * stride[1] - pad[1]), min(W, ox * stride[1] - pad[1] + kern[1])
                acc = np.zeros((B, C), np.float32)
                for xx in range(xa, xb):
                    for yy in range(ya, yb):
                        acc = acc + x[:, :, yy, xx]
                out[:, :, oy, ox] = acc / np.float32(max(0, yb - ya) * max(0, xb - xa))
    return out


def lrn_f64(x, ls, alpha, beta, k):
    """out[c] = in[c] * (k + alpha / local_size * sum of in[c']^2 over the window) ^ -beta; the window is the last local_size channels entered once channel
    c + local_size / 2 has: c - (local_size - 1 - local_size / 2) .. c + local_size / 2 (symmetric for an odd size); channels outside the tensor count as zero."""
    B, C, H, W = x.shape
    half = ls // 2; lo = ls - 1 - half
    sq = np.zeros((B, C + lo + half, H, W)); sq[:, lo:lo + C] = x.astype(np.float64) ** 2
    s = sum(sq[:, d:d + C] for d in range(ls))
    return x.astype(np.float64) * (float(np.float32(k)) + s * (float(np.float32(alpha)) / ls)) ** -float(np.float32(beta))


def same_values(a, b):
    """Equal by value with equal NaN masks (-0 == +0)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and bool(np.all((a == b) | np.isnan(a)))


def avg_close_to_f64(got, case, x):
    """NaN exactly on the empty windows; elsewhere |got - want| <= 2^-24 |want| + (n - 1) 2^-24 mean|v| -> the largest fraction of that bound."""
    want, taps, mag = pool_f64(x, case)
    empty = np.broadcast_to(taps == 0, want.shape)
    assert np.array_equal(np.isnan(got), empty), (case, "NaN exactly on the windows wholly in the padding")
    lim = U32 * np.abs(want) + np.maximum(taps - 1, 0) * U32 * mag
    fr = np.abs(got.astype(np.float64) - want)[~empty] / np.maximum(lim[~empty], 1e-300)
    return float(fr.max()) if fr.size else 0.0


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


# ---- the generators
def test_generators_are_pure_functions_of_n_and_seed():
    for fam in F.FAMILIES:
        gen = getattr(F, fam + "_cases")
        assert gen(24, 5) == gen(24, 5) and gen(24, 5) != gen(24, 6) and len(gen(24, 5)) == 24, fam
        if fam not in ("conv_bf16", "winograd", "k1s"):     # (these filter a longer conv list: a longer list is another list)
            assert gen(24, 5)[:8] == gen(8, 5), fam
    assert {v.__name__ for v in vars(F).values() if isinstance(v, type(os))} == {"numpy"}      # the generators import neither torch nor a backend
    assert set(SEEDS) == set(F.FAMILIES) and all(len(SEEDS[f]) == len(TILES.get(f, {"": 0})) for f in SEEDS)


def test_the_hand_run_tools_draw_what_they_drew_before():
    """The generators moved out of tools/fuzz_conv.py unchanged: its names still give the same lists (tests/test_gpu_parity.py imports `cases` from there)."""
    import fuzz_conv
    assert fuzz_conv.cases(4, 5) == F.conv_cases(4, 5) == [(2, 64, 22, 26, 1, 5, 5, 3, 1), (1, 2, 4, 3, 160, 3, 3, 1, 0), (17, 2, 18, 12, 128, 2, 2, 2, 0), (8, 19, 20, 26, 1, 5, 5, 3, 2)]
    assert fuzz_conv.cases_mode(3, 1, False, "bf16") == [(2, 24, 33, 38, 128, 3, 3, 1, 0), (1, 1, 26, 22, 128, 3, 3, 1, 1), (1, 4, 19, 32, 3, 5, 5, 3, 1)]
    assert fuzz_conv.cases_mode(4, 1, False, "k1s") == [c for c, _ in F.k1s_cases(4, 1)]


def test_cases_stay_inside_their_bounds():
    for fam in ("conv", "conv_bf16", "winograd", "k1s", "nhwc_conv"):
        for c in getattr(F, fam + "_cases")(60, 3):
            B, C, H, W, OC, KH, KW, S, P = c[0] if fam in ("k1s", "nhwc_conv") else c
            OH, OW = (H + 2 * P - KH) // S + 1, (W + 2 * P - KW) // S + 1
            assert OH >= 1 and OW >= 1 and 2.0 * B * OH * OW * OC * C * KH * KW <= F.CONV_FLOP_CAP, (fam, c)
    assert all((c[5], c[6], c[7]) == (3, 3, 1) for c in F.winograd_cases(40, 2)) and all(c[0][5:] == (1, 1, 1, 0) for c in F.k1s_cases(40, 2))
    assert all(1 <= v <= 300 for c in F.sgemm_cases(200, 2) for v in c)
    for c in F.pool_cases(120, 2):
        kern, stride, pad, OH, OW = F.pool_geom(c)
        assert c[0] * c[1] * c[2] * c[3] <= F.ELEMS_CAP and pad[0] < kern[0] and pad[1] < kern[1] and min(stride) >= 1 and OH >= 1 and OW >= 1, c
    for c in F.lrn_cases(120, 2):
        assert c[0] * c[1] * c[2] * c[3] <= F.ELEMS_CAP and 1 <= c[4] <= 17 and c[5] in F.ALPHAS, c
    for c in F.pool_lrn_pair_cases(60, 2):
        assert c[0] * c[1] * c[2] * c[3] <= F.ELEMS_CAP and c[6][0] % 2 == 1, c
    assert {c[4] for c in F.pool_lrn_pair_cases(12, 2)} == {0, 1}
    assert all(sum(F.empty_windows(c[:4] + c[5] + (0,))) == 0 for c in cases("pool_lrn_pair"))     # (an empty window's -inf would make the carried sum of the oracle's LRN Inf - Inf)
    for B, chans, H, W in F.elementwise_cases(60, 2):
        assert len(set(chans)) == 3 and all(c % 8 == 0 for c in chans) and B * sum(chans) * H * W <= F.ELEMS_CAP


def test_the_empty_window_of_the_ceil_rule():
    """A plane of height 3 with k 2, s 2, p 1 has three output rows and the last row's window lies wholly in the padding: -FLT_MAX for a maximum, NaN for an average."""
    case = (1, 1, 3, 4, (2, 2), (2, 2), (1, 1), 0)
    assert F.pool_geom(case)[3:] == (3, 3) and F.empty_windows(case) == (1, 0) and "empty" in F.pool_categories(case)
    x = np.arange(12, dtype=np.float32).reshape(1, 1, 3, 4)
    assert np.all(bo.pool_fwd(x, (2, 2), (2, 2), (1, 1), False)[0, 0, 2] == -FLT_MAX) and np.all(np.isnan(bo.pool_fwd(x, (2, 2), (2, 2), (1, 1), True)[0, 0, 2]))
    assert pool_pipe(case).nodes["p"].sizes == (1, 1, 3, 3)


def test_pool_categories_on_the_list_as_used():
    pools = cases("pool")
    count = {cat: sum(1 for c in pools if cat in F.pool_categories(c)) for cat in F.POOL_CATS}
    print("pool categories among the GPU cases:", count)
    assert all(v >= 1 for v in count.values()), count
    empties = [c for c in pools if "empty" in F.pool_categories(c)]
    assert {c[7] for c in empties} == {0, 1}                                 # a maximum and an average over a window wholly in the padding
    assert any(c[7] == 0 and i % 12 in (4, 10) for i, c in enumerate(pools)) and any(c[7] == 0 and i % 12 in (6, 8) for i, c in enumerate(pools))   # special / tied data reach a maximum
    assert any(not pool_nonempty_small(c) for c in pools) and sum(pool_nonempty_small(c) for c in pools) >= 6      # both the generic and the specialised forms
    spec = [c for c in pools if pool_nonempty_small(c)]
    assert any(c[5][0] != c[5][1] for c in spec) and any(F.pool_geom(c)[0][0] != F.pool_geom(c)[0][1] for c in spec) and any(c[6][0] != c[6][1] for c in spec) and any(c[2] != c[3] for c in spec)   # y / x mix-ups show in the specialised forms
    xt = lambda c: F.pool_geom(c)[4]
    assert any(xt(c) >= 8 and xt(c) % 4 for c in pools if pool_nonempty_small(c))                                  # the XT = 4 tail of the specialised kernel


def test_lrn_categories_on_the_list_as_used():
    lrns = cases("lrn")
    count = {cat: sum(1 for c in lrns if cat in F.lrn_categories(c)) for cat in F.LRN_CATS}
    print("lrn categories among the GPU cases:", count)
    assert all(v >= 1 for v in count.values()), count
    assert {c[4] for c in lrns if c[4] % 2 == 0} >= {2, 4}


def test_conv_categories_on_the_lists_as_used():
    for fam in TILES:
        for k in TILES[fam].values():
            cats = set().union(*(F.conv_categories(c) for c in cases(fam, k)))
            assert cats >= {"non_square", "k1", "strided", "padded", "c_ragged", "oc_ragged", "tail"}, (fam, k, cats)
    assert "pad_ge_k" in set().union(*(F.conv_categories(c) for k in (0, 1) for c in cases("conv", k)))
    assert {"padded", "one_out", "c_ragged", "oc_ragged"} <= set().union(*(F.conv_categories(c) for c in cases("winograd")))
    k1s = cases("k1s")
    assert any(s.startswith("q") for _, s in k1s) and any(not s.startswith("q") for _, s in k1s)
    nh = cases("nhwc_conv")
    assert any(t for _, t, _ in nh) and any(not t for _, t, _ in nh) and {f for _, _, f in nh} == {True, False}
    sg = cases("sgemm")
    assert any(m % 4 or n % 4 for m, n, _ in sg) and any(m % 4 == 0 and n % 4 == 0 for m, n, _ in sg) and any(k % 2 for _, _, k in sg)


# ---- every case builds
def nhwc_tile_refused(shape, tile, f32):
    """Does the planner refuse the forced tile for the layer's kernel (the refusal tools/fuzz_nhwc.py skips)?"""
    anno = add_codegen_annotations(R.conv_op(*shape), OpTune(hip_tile=tile, **dict(NHWC_TUNE, **({"hip_out": "f32"} if f32 else {}))))
    assert anno.get_func_name() == "hip_conv_nhwc"
    try:
        rtc_mod.explain_plan(anno, tile=tile)
    except UnsupErr:
        assert tile, (shape, "the planner's own choice is never refused")
        return True
    return False


def plan_cfg(plan):
    """The tile configuration of explain_plan's answer: the word behind the kernel's name (a space-to-depth plan names its regrouping first)."""
    w = plan.split()
    return w[[i for i, t in enumerate(w) if "bodahip_" in t][0] + 1]


def forced_tile_taken(cfg, tile):
    f = tile.split("x")
    return cfg.startswith(f"{f[0]}x{f[1]}x") and f"_w{f[3]}x{f[4]}" in cfg


def test_every_conv_and_sgemm_case_builds_and_plans():
    for fam, func, tune in (("conv", "hip_conv", {}), ("conv_bf16", "hip_conv_bf16", {"hip_dtype": "bf16"})):
        for tile, k in TILES[fam].items():
            for c in cases(fam, k):
                anno = add_codegen_annotations(R.conv_op(*c), OpTune(hip_tile=tile, **tune))
                assert anno.get_func_name() == func
                plan = rtc_mod.explain_plan(anno, tile=tile)
                assert "bodahip_conv" in plan.split()[0] and (not tile or forced_tile_taken(plan_cfg(plan), tile)), (c, tile, plan)
    for c in cases("winograd") + [s for s, _ in cases("k1s")]:
        assert rtc_mod.explain_plan(add_codegen_annotations(R.conv_op(*c), OpTune())).startswith("bodahip_")
    refused = sum(nhwc_tile_refused(*c) for c in cases("nhwc_conv"))
    assert refused <= N // 2, refused
    for g in cases("sgemm"):
        assert rtc_mod.explain_plan(add_codegen_annotations(R.sgemm_op(*g), OpTune())).startswith("bodahip_sgemm")


def test_every_pool_and_lrn_case_lays_out_as_the_expected_form():
    for case in cases("pool"):
        for nhwc in (False, True):
            for spec in (True, False):
                dry = DryRtc(); fwd = pipe_fwd(dry, pool_pipe(case), nhwc, spec)
                name = call_names(fwd)["p"]
                assert name_is(name, expect_pool_name(case, nhwc, spec)), (case, nhwc, spec, name)
                if not nhwc:
                    src = [i.func_src for i in dry.infos if i.func_name == name][0]
                    assert f"#define BODAHIP_POOL_UNCOND {int(spec and pool_nonempty_small(case))}\n" in src, (case, spec)
    for case in cases("lrn"):
        for nhwc in (False, True):
            for spec in (True, False):
                dry = DryRtc(); fwd = pipe_fwd(dry, lrn_pipe(case), nhwc, spec)
                name = call_names(fwd)["l"]
                assert name_is(name, expect_lrn_name(case, nhwc, spec)), (case, nhwc, spec, name)
                if not nhwc:
                    src = [i.func_src for i in dry.infos if i.func_name == name][0]
                    assert f"#define BODAHIP_LRN_FASTPOW {int(spec)}\n" in src, (case, spec)
    with pytest.raises(UnsupErr):       # the documented refusal of the channels-last LRN: a window of more than 17 channels
        pipe_fwd(DryRtc(), lrn_pipe((1, 8, 2, 2, 19, 1e-4, 0.75, 1.0)), True)


def pair_forms(case):
    """How ConvPipeFwd(fuse_pool_lrn=True / "pool_first") runs a pair: "lds" | "reg" | "apart"."""
    out = {}
    for mode in (True, "pool_first"):
        fwd = pipe_fwd(DryRtc(), pair_pipe(case), True, True, fuse_pool_lrn=mode)
        names = list(call_names(fwd).values())
        out[mode] = "lds" if any(n.startswith("nhwc_lrn_pool_lds_c") for n in names) else ("reg" if any(n.startswith(("nhwc_pool_lrn_c", "nhwc_lrn_pool_c")) for n in names) else "apart")
    return out


def test_pair_and_elementwise_cases_lay_out():
    forms = [pair_forms(c) for c in cases("pool_lrn_pair")]
    print("pair forms among the GPU cases:", forms)
    assert sum(f["pool_first"] == "lds" for f in forms) >= 2 and sum(f[True] == "reg" for f in forms) >= 2 and sum(f["pool_first"] == "reg" for f in forms) >= 2
    for case in cases("pool_lrn_pair"):
        assert set(call_names(pipe_fwd(DryRtc(), pair_pipe(case), True, True, fuse_pool_lrn=False))) == {"xpose_data", "x0", "p", "l"}
        assert set(call_names(pipe_fwd(DryRtc(), pair_pipe(case), False))) == {"x0", "p", "l"}
    for case in cases("elementwise"):
        nh = call_names(pipe_fwd(DryRtc(), elt_pipe(case), True))
        assert (nh["e0"], nh["e1+e1r"], nh["rr"]) == ("nhwc_eltwise", "nhwc_eltwise", "nhwc_relu") and nh["sm"].startswith("nhwc_pool_c"), nh
        f32 = call_names(pipe_fwd(DryRtc(), elt_pipe(case), False))
        assert f32["e0"].startswith("hip_reduce__") and f32["e1"].startswith("hip_reduce__") and f32["e1r"].startswith("hip_zero_if_non_pos__") and f32["rr"] == "fwd_relu", f32


# ---- the reference side: conv and sgemm
def torch_conv_f64(d, shape, relu=True):
    import torch
    S, P = shape[7], shape[8]
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    y = torch.nn.functional.conv2d(t(d["in"]), t(d["filts"]), t(d["biases"]), stride=S, padding=P)
    return (torch.relu(y) if relu else y).numpy()


@pytest.mark.parametrize("fam,k", [(f, k) for f in ("conv", "conv_bf16", "winograd", "k1s", "nhwc_conv") for k in range(len(SEEDS[f]))])
def test_conv_oracle_against_float64_on_the_gpu_cases(cpu, fam, k):
    worst = 0.0
    for i, c in enumerate(cases(fam, k)):
        shape = c[0] if fam in ("k1s", "nhwc_conv") else c
        d = conv_data(shape, data_seed(fam, k, i))
        if fam in ("conv_bf16", "nhwc_conv"):
            d = dict(d, **{"in": bo.to_bf16(d["in"]), "filts": bo.to_bf16(d["filts"])})
        S, P = shape[7], shape[8]
        want = bo.conv_fwd(d["in"], d["filts"], d["biases"], (S, S), (P, P), True)
        t64 = torch_conv_f64(d, shape)
        v = mrd(want, t64) if np.abs(t64).max() > 0 else float(np.abs(want).max())
        worst = max(worst, v)
        assert v < MRD, (fam, c, v)
        if fam in ("conv", "winograd", "k1s"):      # be=cpu carries hip_conv: bit-equal to the oracle, from a poisoned output
            r = R.run_conv(cpu, shape, {"d": d}, relus=(1,), wide=False)[("d", 1)]
            R.assert_no_poison(r["out"], c)
            assert np.array_equal(R.bits(r["out"]), R.bits(want)), (fam, c)
    print(f"{fam} list {k}: worst mrd of the oracle against float64 {worst:.2e} (bound {MRD})")


def test_sgemm_oracle_against_float64_on_the_gpu_cases(cpu):
    for i, g in enumerate(cases("sgemm")):
        d = sgemm_data(g, data_seed("sgemm", 0, i))
        want = bo.sgemm(d["a"], d["b"])
        assert mrd(want, d["a"].astype(np.float64).T @ d["b"].astype(np.float64)) < MRD, g
        r = R.run_sgemm(cpu, g, {"d": d})["d"]
        R.assert_no_poison(r["c"], g)
        assert np.array_equal(R.bits(r["c"]), R.bits(want)), g


# ---- the reference side: pooling and LRN
def check_pool_oracle(case, x):
    kern, stride, pad, OH, OW = F.pool_geom(case)
    got = bo.pool_fwd(x, kern, stride, pad, bool(case[7]))
    assert got.shape == x.shape[:2] + (OH, OW), case
    if case[7]:
        fr = avg_close_to_f64(got, case, x)
        assert fr <= 1.0, (case, fr)
        assert same_values(got, pool_f32_chain(x, case)), case
        return fr
    want, taps, _ = pool_f64(x, case)
    assert same_values(got, want.astype(np.float32)) and not np.isnan(got).any(), case
    assert np.all(got[np.broadcast_to(taps == 0, got.shape)] == -FLT_MAX), case
    return 0.0


def test_pool_oracle_against_float64_on_the_gpu_cases():
    worst = 0.0
    for i, case in enumerate(cases("pool")):
        x = pool_input(case, i, data_seed("pool", 0, i))
        worst = max(worst, check_pool_oracle(case, x))
        check_pool_oracle(case, bo.to_bf16(x))       # the values the channels-last kernels consume
    print(f"pool cases: worst fraction of the average's bound {worst:.3f}")
    for i, case in enumerate(cases("pool_lrn_pair")):
        B, C, H, W, _, (kern, stride, pad), _ = case
        check_pool_oracle((B, C, H, W, kern, stride, pad, 0), bo.to_bf16(lrn_input(case, data_seed("pool_lrn_pair", 0, i))))


def lrn_rel(got, want):
    nz = want != 0
    assert np.all(got[~nz] == 0)
    return float(np.max(np.abs(got[nz].astype(np.float64) - want[nz]) / np.abs(want[nz]))) if nz.any() else 0.0


def test_lrn_oracle_against_float64_on_the_gpu_cases():
    worst = {a: 0.0 for a in F.ALPHAS}
    todo = [(c, lrn_input(c, data_seed("lrn", 0, i))) for i, c in enumerate(cases("lrn"))]
    todo += [(c[:4] + c[6], lrn_input(c, data_seed("pool_lrn_pair", 0, i))) for i, c in enumerate(cases("pool_lrn_pair"))]
    for case, x in todo:
        B, C, H, W, ls, alpha, beta, k = case
        for xx in (x, bo.to_bf16(x)):
            v = lrn_rel(bo.lrn_fwd(xx, ls, alpha, beta, k), lrn_f64(xx, ls, alpha, beta, k))
            worst[alpha] = max(worst[alpha], v)
            assert v <= LRN_F64_BOUND[alpha], (case, v)
    print("lrn cases: largest relative distance of the oracle from float64 per alpha:", {a: f"{v:.2e}" for a, v in worst.items()})
    assert all(v > 0.25 * LRN_F64_BOUND[a] for a, v in worst.items()), worst      # the bound is twice what these cases measure, not looser
    x = todo[5][1]                                                                   # an even window is {c - 1 .. c + 2} for local_size 4: not the symmetric one
    sym = lrn_f64(np.concatenate([x[:, :1] * 0, x], axis=1), 5, 0.5 * 5 / 4, 0.75, 1.0)[:, 1:]
    assert lrn_rel(bo.lrn_fwd(x, 4, 0.5, 0.75, 1.0), lrn_f64(x, 4, 0.5, 0.75, 1.0)) <= LRN_F64_BOUND[0.5] and (x.shape[1] < 3 or not np.allclose(sym, lrn_f64(x, 4, 0.5, 0.75, 1.0), rtol=1e-3))


# ---- the numpy statements of the element-wise kernels (boda_amd/conv_pipe.py FWD_SRC, boda_amd/nhwc.py FWD_SRC)
def relu_ref(x):
    """fwd_relu / nhwc_relu: every value <= 0 (so -0 too) becomes +0; a NaN is kept."""
    y = np.array(x, np.float32)
    y[y <= 0] = 0.0
    return y


def eltwise_ref(a, b, relu, bf16):
    """fp32 sum (hip_reduce: a chain from +0, so -0 + -0 = +0); ReLU as x > 0 ? x : +0, which turns a NaN into +0 (hip_zero_if_non_pos, nhwc_eltwise with relu);
    channels-last: one rounding to bf16 at the end."""
    with np.errstate(invalid="ignore"):
        s = (np.float32(0) + a) + b if not bf16 else a + b
        if relu:
            s = np.where(s > 0, s, np.float32(0))
    return bo.to_bf16(s) if bf16 else s.astype(np.float32)


def test_elementwise_references_state_what_a_nan_becomes():
    x = special((np.random.default_rng(1).standard_normal((2, 8, 3, 3)) * 3).astype(np.float32), 7)
    assert np.isnan(x).any() and np.isinf(x).any() and np.signbit(x[x == 0]).any()
    assert same_values(relu_ref(x), bo.relu(x)) and np.array_equal(np.isnan(relu_ref(x)), np.isnan(x)) and not np.signbit(relu_ref(x)[relu_ref(x) == 0]).any()
    e = eltwise_ref(x, x[::-1], True, False)
    assert not np.isnan(e).any() and np.isnan(eltwise_ref(x, x[::-1], False, False)).any() and np.all(e >= 0)
