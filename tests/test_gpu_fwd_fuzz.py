"""Seeded random-geometry sweeps of the FORWARD kernels on the MI355X: hip_conv (planner's tile and a forced one), hip_conv_bf16, the Winograd path, random k1_stream
specs, hip_conv_nhwc (drawn forced tiles, float and bf16 outputs), hip_sgemm, and the non-conv kernels of ConvPipeFwd in fp32 and in channels-last bf16, specialised and
generic: pooling, LRN, their fused pairs, ReLU, Eltwise, Concat -- on the cases of tools/fuzz_fwd.py under the seed table of tests/test_fwd_fuzz_cpu.py, which proves the
reference side (oracle against float64, be=cpu against the oracle, the categories) on these very cases.

One test per case.  Every output var -- and every node of a pipe -- is filled with the payload NaN of tests/fwd_special_ref.py before the launch and may not keep it;
every launch must be the form the case expects (kernel and tile for the convolutions, the function-name prefix for pool / LRN).  A failed compare raises Mismatch
(the case, the launch, how many elements differ); the last test prints the forms launched (USED) and the largest observed fraction of every bound (WORST).

What a NaN becomes under each ReLU, asserted below: kept by the stand-alone ReLU kernels (fwd_relu, nhwc_relu: `v <= 0 ? 0 : v`, as the oracle's bo_relu), turned into +0
by the ReLU behind an Eltwise (hip_zero_if_non_pos / nhwc_eltwise with relu: `x > 0 ? x : +0`, as tests/resnet_ref.py states it).

Every random geometry is a fresh hiprtc specialisation, so the counts are small on purpose (12 per list).  Measured on one MI355X (pytest --durations):
181 tests in 39 s from a cold code-object cache; the slowest case 0.9 s (a fused pair: three pipes), most 0.2 - 0.4 s.  The measured USED and WORST tables: DESIGN.md 3.0a."""
import re
import types

import numpy as np
import pytest

import fwd_special_ref as R
from boda_amd import nhwc
from boda_amd.cnn_op import OpTune
from boda_amd.digest import SsdsDiff
from boda_amd.op import Dims, UnsupErr
from boda_amd.rtc import RtcArg, RtcFuncCall, make_rtc
from oracle import boda_oracle as bo

import test_fwd_fuzz_cpu as T
from test_fwd_fuzz_cpu import F, N, NHWC_TUNE, TILES, cases, data_seed
from test_gpu_nhwc import _check_bf16, _check_f32

pytestmark = pytest.mark.gpu
WORST = {}   # bound name -> largest observed fraction of it
USED = {}    # "kernel cfg" / function form -> launches
PAIRS = {"lds": 0, "reg": 0, "apart": 0, "ran": 0}
K1S = {"ran": 0, "refused": 0}


class Mismatch(AssertionError):
    """A failed compare: what was compared, the case, the launch's kernel and cfg (or function names), how many of how many elements differ."""
    def __init__(self, what, case, cfg, count, size):
        super().__init__(f"{what}: {count} of {size} elements differ, case {case}, launch {cfg}")
        self.what, self.case, self.cfg, self.count, self.size = what, case, cfg, count, size


@pytest.fixture(scope="module")
def hip():
    r = make_rtc("(be=hip)", 0)
    r.init()
    yield r
    r.finish_and_sync()
    r.close()


def used(key):
    USED[key] = USED.get(key, 0) + 1
    return key


def launch_cfg(launch):
    return used(launch["kernel"].replace("bodahip_", "") + " " + launch.get("cfg", ""))


def form(name):
    """A generated / specialised function's name without its geometry: fwd_pool__*, nhwc_pool_c*, nhwc_lrn_pool_lds_c* ..."""
    return re.sub(r"(__|_c)\d.*$", r"\1*", name)


def same(what, case, cfg, got, want, by_bits=False):
    """Equal NaN masks and equal values elsewhere (by_bits: equal bit patterns elsewhere, so the sign of a zero counts)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        raise Mismatch(what + f" (shape {got.shape} against {want.shape})", case, cfg, got.size, want.size)
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (gn != wn) | (~wn & ((R.bits(got) != R.bits(want)) if by_bits else (got != want)))
    if bad.any():
        raise Mismatch(what, case, cfg, int(bad.sum()), want.size)


def within(name, case, cfg, got, want, lim):
    """|got - want| <= lim element by element where want is a number; equal NaN masks."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        raise Mismatch(f"{name}: shapes or NaN masks differ", case, cfg, int((np.isnan(got) != np.isnan(want)).sum()) if got.shape == want.shape else got.size, want.size)
    ok = ~np.isnan(want) & np.isfinite(want)
    same(name + " (non-finite values)", case, cfg, got[~ok], want[~ok])
    err = np.abs(got[ok] - want[ok]) / np.maximum(np.broadcast_to(lim, want.shape)[ok], 1e-300)
    frac = float(err.max()) if err.size else 0.0
    WORST[name] = max(WORST.get(name, 0.0), frac)
    if not frac <= 1.0:
        raise Mismatch(f"{name}: {frac:.3g} of the bound", case, cfg, int((err > 1.0).sum()), want.size)


def under(name, case, cfg, frac):
    WORST[name] = max(WORST.get(name, 0.0), frac)
    if not frac <= 1.0:
        raise Mismatch(f"{name}: {frac:.3g} of the bound", case, cfg, 1, 1)


def unpoisoned(what, case, cfg, raw):
    b = R.bits(raw)
    p = R.BF16_POISON if b.dtype == np.uint16 else R.POISON_BITS
    if (b == p).any():
        raise Mismatch(what + ": elements never stored", case, cfg, int((b == p).sum()), b.size)


# ---- convolutions and sgemm
def conv_case(fam, k, i):
    c = cases(fam, k)[i]
    return c, (c[0] if fam in ("k1s", "nhwc_conv") else c), T.conv_data((c[0] if fam in ("k1s", "nhwc_conv") else c), data_seed(fam, k, i))


def oracle_conv(shape, d, bf16=False):
    S, P = shape[7], shape[8]
    r = (lambda a: bo.to_bf16(a)) if bf16 else (lambda a: a)
    return bo.conv_fwd(r(d["in"]), r(d["filts"]), d["biases"], (S, S), (P, P), True)


@pytest.mark.parametrize("i", range(N))
@pytest.mark.parametrize("tile", list(TILES["conv"]), ids=lambda t: t or "planner")
def test_conv_exact(hip, tile, i):
    c, shape, d = conv_case("conv", TILES["conv"][tile], i)
    r = R.run_conv(hip, shape, {"d": d}, relus=(1,), tile=tile)[("d", 1)]
    cfg = launch_cfg(r["launch"])
    unpoisoned("hip_conv out", c, cfg, r["out"])
    assert not tile or T.forced_tile_taken(r["launch"]["cfg"], tile), (tile, cfg)
    same("hip_conv against the oracle", c, cfg, r["out"], oracle_conv(shape, d))


@pytest.mark.parametrize("i", range(N))
@pytest.mark.parametrize("tile", list(TILES["conv_bf16"]), ids=lambda t: t or "planner")
def test_conv_bf16(hip, tile, i):
    c, shape, d = conv_case("conv_bf16", TILES["conv_bf16"][tile], i)
    r = R.run_conv(hip, shape, {"d": d}, relus=(1,), tile=tile, tune=OpTune(hip_dtype="bf16"), func="hip_conv_bf16")[("d", 1)]
    cfg = launch_cfg(r["launch"])
    unpoisoned("hip_conv_bf16 out", c, cfg, r["out"])
    assert not tile or T.forced_tile_taken(r["launch"]["cfg"], tile), (tile, cfg)
    under("hip_conv_bf16 mrd", c, cfg, _check_f32(R.conv_op(*shape), dict(d, out=r["out"]), types.SimpleNamespace(launch=r["launch"])))


@pytest.mark.parametrize("i", range(N))
def test_conv_winograd(hip, i):
    c, shape, d = conv_case("winograd", 0, i)
    try:
        r = R.run_conv(hip, shape, {"d": d}, relus=(1,), before_run=lambda: hip.set_tune("conv_algo", "winograd_all"))[("d", 1)]
    finally:
        hip.set_tune("conv_algo", "")
    cfg = launch_cfg(r["launch"])
    unpoisoned("winograd out", c, cfg, r["out"])
    assert r["launch"]["kernel"] == "bodahip_conv_winograd_f32", cfg
    sd = SsdsDiff.of(oracle_conv(shape, d), r["out"])
    assert not sd.has_nan(), (c, cfg)
    under("winograd mrd 2e-3", c, cfg, sd.mrd / 2e-3)


@pytest.mark.parametrize("i", range(N))
def test_conv_k1_stream_specs(hip, i):
    (shape, spec), _, d = conv_case("k1s", 0, i)
    K1S["ran"] += 1
    try:
        r = R.run_conv(hip, shape, {"d": d}, relus=(1,), before_run=lambda: hip.set_tune("k1_stream", spec))[("d", 1)]
    except Exception as e:      # a spec the kernel does not take for this shape: the documented refusal (tools/fuzz_conv.py counts them)
        if "unsupported configuration" not in str(e):
            raise
        used("(k1_stream spec refused)"); K1S["refused"] += 1
        return
    finally:
        hip.set_tune("k1_stream", "")
    cfg = launch_cfg(r["launch"])
    unpoisoned("k1_stream out", (shape, spec), cfg, r["out"])
    assert r["launch"]["kernel"] == ("bodahip_k1_quad_f32" if spec.startswith("q") else "bodahip_k1_stream_f32"), (spec, cfg)
    same("k1_stream against the oracle", (shape, spec), cfg, r["out"], oracle_conv(shape, d))


@pytest.mark.parametrize("i", range(N))
def test_conv_nhwc(hip, i):
    (shape, tile, f32), _, d = conv_case("nhwc_conv", 0, i)
    tune = OpTune(hip_tile=tile, **dict(NHWC_TUNE, **({"hip_out": "f32"} if f32 else {})))
    if T.nhwc_tile_refused(shape, tile, f32):      # (a forced tile the layer's kernel does not take)
        with pytest.raises(UnsupErr):
            R.run_nhwc(hip, shape, {"d": d}, tune, relus=(1,), tile=tile)
        used("(nhwc tile refused)")
        return
    r = R.run_nhwc(hip, shape, {"d": d}, tune, relus=(1,), tile=tile)[("d", 1)]
    cfg = launch_cfg(r["launch"])
    unpoisoned("hip_conv_nhwc out", (shape, tile, f32), cfg, r["out"])
    assert r["out_tn"] == ("float" if f32 else "bfloat16") and (not tile or T.forced_tile_taken(r["launch"]["cfg"], tile)), (tile, cfg)
    (_check_f32 if f32 else _check_bf16)(R.conv_op(*shape), dict(d, out=r["out"]), types.SimpleNamespace(launch=r["launch"]))


@pytest.mark.parametrize("i", range(N))
def test_sgemm(hip, i):
    g = cases("sgemm")[i]
    d = T.sgemm_data(g, data_seed("sgemm", 0, i))
    r = R.run_sgemm(hip, g, {"d": d})["d"]
    cfg = launch_cfg(r["launch"])
    unpoisoned("hip_sgemm c", g, cfg, r["c"])
    same("hip_sgemm against the oracle", g, cfg, r["c"], bo.sgemm(d["a"], d["b"]))


# ---- pipes: pooling, LRN, pairs, ReLU / Eltwise
def poison_like(d):
    return np.full(d.sizes, R.BF16_POISON, np.uint16) if d.tn == "bfloat16" else R.poison(d.sizes)


def read_node(hip, fwd, cp, node, what, case, cfg):
    """A node in the reference layout; a channels-last bf16 var is widened and transposed here (its pad channels, which the pipe's own fetch refuses, are cut off)."""
    raw = hip.copy_var_to_nda(fwd.var_of(node))
    unpoisoned(f"{what} node {node}", case, cfg, raw)
    if raw.dtype != np.uint16:
        return raw
    f = (raw.astype(np.uint32) << 16).view(np.float32)
    return np.ascontiguousarray(f.transpose(0, 3, 1, 2)[:, :cp.nodes[node].dsz("chan")])


def run_pipe(hip, cp, nhwc_mode, x, case, spec=True, **kw):
    """ConvPipeFwd over the pipe: every node's var poisoned, the input set, the calls run.  -> ({node: value}, {tag: function name}, the driver's fused-pair tables)."""
    fwd = T.pipe_fwd(hip, cp, nhwc_mode, spec, **kw)
    try:
        names = T.call_names(fwd)
        for n in names.values():
            used(form(n))
        for node in cp.nodes:
            vn = fwd.var_of(node)
            hip.copy_nda_to_var(vn, poison_like(hip.get_var_dims(vn)))
        hip.copy_nda_to_var(fwd.in_var, x)
        for c in fwd.fwd_calls:
            hip.run(c.rfc)
        hip.finish_and_sync()
        lazy = set(fwd._lazy)
        out = {node: read_node(hip, fwd, cp, node, cp.name, case, names) for node in cp.nodes if node not in lazy}
        return out, names, (set(fwd.lds_pool_lrn), dict(fwd.fused_pool_lrn))
    finally:
        fwd.release()
        hip.release_per_call_id_data()


def f32_switch(hip, name, macro):
    """The value of a fp32 template's switch in the generated function that ran."""
    inst = [v for v in hip.__dict__["_pool_funcs"].values() if v.func_name == name][0]
    return int(re.search(rf"#define {macro} (\d)", inst.src)[1])


@pytest.mark.parametrize("layout", ["f32", "nhwc"])
@pytest.mark.parametrize("i", range(N))
def test_pool(hip, i, layout):
    case = cases("pool")[i]
    nh = layout == "nhwc"
    x = T.pool_input(case, i, data_seed("pool", 0, i))
    xd = bo.to_bf16(x) if nh else x
    kern, stride, pad, OH, OW = F.pool_geom(case)
    want = bo.pool_fwd(xd, kern, stride, pad, bool(case[7]))
    ulp = 2.0 ** -8 if nh else 2.0 ** -22
    res = {}
    for spec in (True, False):
        out, names, _ = run_pipe(hip, T.pool_pipe(case), nh, x, case, spec)
        assert T.name_is(names["p"], T.expect_pool_name(case, nh, spec)), (case, spec, names)
        if not nh:
            assert f32_switch(hip, names["p"], "BODAHIP_POOL_UNCOND") == int(spec and T.pool_nonempty_small(case)), (case, spec)
        else:
            same("the layout pass", case, names, out["data"], xd, by_bits=True)
        res[spec] = out["p"]
        if case[7]:     # an average: within the tool's bound of the oracle, NaN exactly where the oracle has it
            w = want.astype(np.float64)
            within(f"avg pool {layout}", case, names, out["p"], w, 2 * ulp * np.abs(w) + 1e-6)
        else:           # a maximum: the oracle's, on the values the device consumed (a bf16 tensor stores the -FLT_MAX of an empty window as -inf)
            same(f"max pool {layout} against the oracle", case, names, out["p"], bo.to_bf16(want) if nh else want)
            if nh and sum(F.empty_windows(case)):
                assert np.isneginf(out["p"]).any(), case
    same(f"pool {layout}: specialised against generic", case, layout, res[True], res[False], by_bits=True)


def lrn_lim(w, ulp, extra):
    return 2 * max(ulp, 2.5e-5) * np.abs(w) + extra      # (tools/fuzz_pool_lrn.py: the carried sum of squares loses digits at alpha 0.5, in the oracle's order as in the kernels')


@pytest.mark.parametrize("layout", ["f32", "nhwc"])
@pytest.mark.parametrize("i", range(N))
def test_lrn(hip, i, layout):
    """Even windows included: both layouts compute the oracle's window (c - 1 .. c + 2 for local_size 4); the channels-last kernel for them is the generic one."""
    case = cases("lrn")[i]
    nh = layout == "nhwc"
    x = T.lrn_input(case, data_seed("lrn", 0, i))
    xd = bo.to_bf16(x) if nh else x
    w = bo.lrn_fwd(xd, *case[4:]).astype(np.float64)
    ulp = 2.0 ** -8 if nh else 2.0 ** -22
    res = {}
    for spec in (True, False):
        out, names, _ = run_pipe(hip, T.lrn_pipe(case), nh, x, case, spec)
        assert T.name_is(names["l"], T.expect_lrn_name(case, nh, spec)), (case, spec, names)
        if not nh:
            assert f32_switch(hip, names["l"], "BODAHIP_LRN_FASTPOW") == int(spec), (case, spec)
        res[spec] = out["l"]
        within(f"lrn {layout} against the oracle", case, names, out["l"], w, lrn_lim(w, ulp, 1e-5))
    gen = res[False].astype(np.float64)
    within(f"lrn {layout}: specialised against generic", case, layout, res[True], gen, lrn_lim(gen, ulp, 1e-6))


@pytest.mark.parametrize("i", range(N))
def test_pool_lrn_pair(hip, i):
    """A max pooling and an LRN chained, channels-last: fused in one launch (register form, LDS form) and apart, bit for bit; apart, each op against the oracle on the
    values the device handed it."""
    case = cases("pool_lrn_pair")[i]
    B, C, H, W, lrn_first, (kern, stride, pad), lrn = case
    x = T.lrn_input(case, data_seed("pool_lrn_pair", 0, i))
    last = "p" if lrn_first else "l"
    res = {}
    for mode in (False, True, "pool_first"):
        out, names, (lds, fused) = run_pipe(hip, T.pair_pipe(case), True, x, case, True, fuse_pool_lrn=mode)
        res[mode] = out
        if mode:
            how = "lds" if lds else ("reg" if fused else "apart")
            assert how == T.pair_forms(case)[mode], (case, mode, how)
            PAIRS[how] += 1
            same(f"pair fused ({mode}, {how}) against apart", case, names, out[last], res[False][last], by_bits=True)
    PAIRS["ran"] += 1
    apart = res[False]
    same("pair: x0 is the input", case, "apart", apart["x0"], bo.to_bf16(x), by_bits=True)
    first_in = apart["x0"]
    if lrn_first:
        w = bo.lrn_fwd(first_in, *lrn).astype(np.float64)
        within("pair lrn against the oracle", case, "apart", apart["l"], w, lrn_lim(w, 2.0 ** -8, 1e-5))
        same("pair pooling against the oracle", case, "apart", apart["p"], bo.to_bf16(bo.pool_fwd(apart["l"], kern, stride, pad, False)))
    else:
        same("pair pooling against the oracle", case, "apart", apart["p"], bo.to_bf16(bo.pool_fwd(first_in, kern, stride, pad, False)))
        w = bo.lrn_fwd(apart["p"], *lrn).astype(np.float64)      # (no window of a pair case is empty: every value is finite -- tests/test_fwd_fuzz_cpu.py)
        within("pair lrn against the oracle", case, "apart", apart["l"], w, lrn_lim(w, 2.0 ** -8, 1e-5))


def _u16(x):
    """float -> the bf16 bit patterns, img:y:x:chan."""
    return np.ascontiguousarray((R.bits(bo.to_bf16(x)) >> 16).astype(np.uint16).transpose(0, 2, 3, 1))


def concat_case(hip, case, xs, nh):
    """Each input copied into a poisoned output by its own launch (fwd_copy / nhwc_copy): after every copy the ranges written so far hold their data bit for bit and
    the others still the poison."""
    B, chans, H, W = case
    hw, ctot = H * W, sum(chans)
    mk = (lambda c: Dims(("img", "y", "x", "chan"), (B, H, W, c), "bfloat16")) if nh else (lambda c: Dims.make("float", img=B, chan=c, y=H, x=W))
    vs = R._Vars(hip, "fzc_")
    try:
        ins = [vs.make(f"in{j}", mk(c)) for j, c in enumerate(chans)]
        out = vs.make("out", mk(ctot))
        for v, x in zip(ins, xs):
            hip.copy_nda_to_var(v, _u16(x) if nh else x)
        hip.copy_nda_to_var(out, poison_like(mk(ctot)))
        want = R.bits(poison_like(mk(ctot))).copy()
        c0 = 0
        for j, (v, x, c) in enumerate(zip(ins, xs, chans)):
            if nh:
                call = nhwc.copy_call(v, out, mk(c), mk(ctot), c0)
                want[..., c0:c0 + c] = _u16(x)
            else:
                n = B * c * hw
                am = {"in": RtcArg.var(v), "out": RtcArg.var(out), "n_in": RtcArg.scalar(n, "uint32_t"), "chw_in": RtcArg.scalar(c * hw, "uint32_t"),
                      "chw_out": RtcArg.scalar(ctot * hw, "uint32_t"), "off_out": RtcArg.scalar(c0 * hw, "uint32_t")}
                call = RtcFuncCall("fwd_copy", am, tpb=256, blks=(n + 255) // 256)
                want[:, c0:c0 + c] = R.bits(x)
            hip.run(call); hip.finish_and_sync()
            used(call.rtc_func_name)
            got = R.bits(hip.copy_var_to_nda(out))
            if not np.array_equal(got, want):
                raise Mismatch(f"concat copy {j}: its range holds the input, every other range what it held", case, call.rtc_func_name, int((got != want).sum()), want.size)
            vs.check_guards()
            c0 += c
    finally:
        hip.finish_and_sync()
        vs.release()


@pytest.mark.parametrize("layout", ["f32", "nhwc"])
@pytest.mark.parametrize("i", range(N))
def test_relu_eltwise_concat(hip, i, layout):
    case = cases("elementwise")[i]
    nh = layout == "nhwc"
    xs = T.elementwise_inputs(case, i, data_seed("elementwise", 0, i))
    out, names, _ = run_pipe(hip, T.elt_pipe(case), nh, xs[0], case)
    xd = bo.to_bf16(xs[0]) if nh else xs[0]
    if nh:
        assert (names["e0"], names["e1+e1r"], names["rr"]) == ("nhwc_eltwise", "nhwc_eltwise", "nhwc_relu"), names
    else:
        assert names["e0"].startswith("hip_reduce__") and names["e1r"].startswith("hip_zero_if_non_pos__") and names["rr"] == "fwd_relu", names
    sm = out["sm"]      # the second operand as the device holds it (the pooling that made it is test_pool's business)
    same(f"relu {layout}: <= 0 becomes +0, a NaN is kept", case, names, out["data"], T.relu_ref(xd), by_bits=True)      # (in place on data, after every reader of data)
    assert np.array_equal(np.isnan(out["data"]), np.isnan(xd))
    same(f"eltwise {layout}", case, names, out["e0"], T.eltwise_ref(xd, sm, False, nh), by_bits=True)
    same(f"eltwise + relu {layout}: not (x > 0) becomes +0, a NaN too", case, names, out["e1"], T.eltwise_ref(sm, xd, True, nh), by_bits=True)
    assert not np.isnan(out["e1"]).any()
    concat_case(hip, case, xs, nh)


def test_zz_report_forms_and_worst_fractions_of_the_bounds():
    """Not a check of its own beyond the two pair forms: prints what the sweeps above launched and measured (run with -s)."""
    for name in sorted(WORST):
        print(f"largest observed fraction of the bound, {name}: {WORST[name]:.3f}")
    print("kernels / tile configs / function forms used:", dict(sorted(USED.items(), key=lambda kv: -kv[1])))
    print("pooling <-> LRN pairs by form (fuse_pool_lrn True and pool_first):", PAIRS)
    assert all(v <= 1.0 for v in WORST.values())
    assert K1S["ran"] < N or K1S["refused"] <= N // 2, K1S
    if PAIRS["ran"] == N:
        assert PAIRS["lds"] >= 2 and PAIRS["reg"] >= 2, PAIRS
