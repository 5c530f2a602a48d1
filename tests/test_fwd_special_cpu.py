"""The reference side of the special-data tests of the forward convolution and sgemm kernels (tests/fwd_special_ref.py; the GPU side is tests/test_gpu_fwd_special.py),
on a machine without a GPU: the generators give what they say, the oracle's results on them stay inside the blindness caps for every geometry the GPU file uses, the
comparison functions refuse what they must, be=cpu's hip_conv / hip_sgemm meet the contract on every class, and oracle.to_bf16 keeps NaNs."""
import numpy as np
import pytest

import fwd_special_ref as R
from boda_amd.rtc import make_rtc
from oracle import boda_oracle as bo

F = np.float32


@pytest.fixture(scope="module")
def rtc():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


def _mag_range(v):
    a = np.abs(v[np.isfinite(v) & (v != 0)].astype(np.float64))
    return float(np.log2(a.min())), float(np.log2(a.max()))


def test_generators_give_what_they_say():
    shape = (2, 5, 17, 13, 7, 5, 5, 2, 2)
    d = R.gen_conv("wide", shape)
    for an in ("in", "filts", "biases"):
        lo, hi = _mag_range(d[an]); assert -40 <= lo and hi <= 30 and np.isfinite(d[an]).all()
    x = d["in"]
    pz = float(((x == 0) & ~np.signbit(x)).mean()); nz = float(((x == 0) & np.signbit(x)).mean())
    assert 0.03 < pz < 0.07 and 0.03 < nz < 0.07 and 0.4 < float((x < 0).mean()) < 0.6
    d = R.gen_conv("subnormal", shape)
    tiny = np.finfo(F).tiny
    sub = (np.abs(d["in"]) < tiny) & (d["in"] != 0)
    assert 0 < sub.sum() <= d["in"].size // 20 and (R.bits(np.abs(d["in"][sub])) <= 0x007FFFFF).all()
    lo, hi = _mag_range(d["in"][~sub]); assert -76 <= lo and hi <= -62
    lo, hi = _mag_range(d["filts"]); assert -76 <= lo and hi <= -62
    b = d["biases"]
    assert (b[0::2] == 0).all() and ((np.abs(b[1::2]) < tiny) & (b[1::2] != 0)).all()
    d = R.gen_conv("overflow", shape)
    for an in ("in", "filts"):
        lo, hi = _mag_range(d[an]); assert 55 <= lo and hi <= 64
    assert np.isfinite(d["biases"]).all() and np.abs(d["biases"]).max() <= 5
    # a moved window keeps its width
    s4 = (3, 4, 9, 9, 33, 1, 1, 1, 0); sh = R.SHIFT[("overflow", s4)]
    lo, hi = _mag_range(R.gen_conv("overflow", s4)["in"]); assert 55 + sh <= lo and hi <= 64 + sh
    # the same seed gives the same data, another seed other data
    assert np.array_equal(R.bits(R.gen_conv("wide", shape)["in"]), R.bits(R.gen_conv("wide", shape)["in"]))
    assert not np.array_equal(R.bits(R.gen_conv("wide", shape, seed=1)["in"]), R.bits(R.gen_conv("wide", shape)["in"]))


@pytest.mark.parametrize("shape", R.CONV_SHAPES, ids=R.sid)
def test_nan_inf_placement(shape):
    B, C, H, W = shape[:4]
    d = R.gen_conv("nan_inf", shape)
    x = d["in"]
    nan, inf = np.isnan(x), np.isinf(x)
    assert 3 <= nan.sum() <= 6 and 2 <= inf.sum() <= 4 and np.isfinite(d["filts"]).all() and np.isfinite(d["biases"]).all()
    assert not inf[:, C - 1].any()                                     # no Inf in an image's last channel
    assert set(np.unique(R.bits(x)[nan])) <= set(R.NAN_BITS) and len(set(np.unique(R.bits(x)[nan]))) >= 3     # the payloads survive the generator
    assert nan[0, 0, 0, 0] and nan[0, C - 1, H - 1, W - 1]            # first image / first channel / corner; the pel before an image boundary
    assert (nan | inf)[0].any() and (nan | inf)[B - 1].any()          # first and last image
    assert R.whole_input(shape) or nan[B - 1, 0].any()                # the first channel of the last image: what a K tail that ran on into the next image would read
    assert len(d["inj"]) == nan.sum() + inf.sum()
    assert np.isfinite(d["base_in"]).all() and np.array_equal(d["base_in"][~(nan | inf)], x[~(nan | inf)])
    e = R.gen_conv("inf_last_chan", shape)
    assert np.isinf(e["in"]).sum() == 1 and not np.isnan(e["in"]).any() and np.isposinf(e["in"][:, C - 1]).sum() == 1
    assert np.array_equal(e["base_in"], d["base_in"]) and np.array_equal(e["filts"], d["filts"])


@pytest.mark.parametrize("shape", R.CONV_SHAPES, ids=R.sid)
def test_conv_oracle_stays_inside_the_caps(shape):
    """Every class on every geometry of the GPU file, on the oracle alone; prints the fractions (DESIGN.md section 3.0 records them)."""
    for cls in R.CLASSES:
        fr = R.assert_caps(cls, R.conv_want(cls, shape, 0), R.whole_input(shape))
        print(f"caps conv {R.sid(shape)} {cls}: " + " ".join(f"{k}={v:.3f}" for k, v in fr.items()))
    # C3 on the oracle itself: non-finite exactly inside the windows of the injected elements, the clean run's values outside
    for cls in ("nan_inf", "inf_last_chan"):
        d = R.conv_data(cls, shape); m = R.window_mask(shape, d["inj"])
        for relu in (0, 1):
            R.assert_c3_against_clean(R.conv_clean(shape, relu), R.conv_want(cls, shape, relu), m)
        w = R.conv_want(cls, shape, 0)
        assert (~np.isfinite(w)).any(axis=1)[m].all() or shape[4] > 1     # (a window's outputs are non-finite unless a filter value is exactly 0: U(-5, 5) has none)
        assert not np.isfinite(w[np.broadcast_to(m[:, None], w.shape)]).any()


@pytest.mark.parametrize("geom", R.SGEMM_GEOMS, ids=R.sid)
def test_sgemm_oracle_stays_inside_the_caps(geom):
    for cls in R.CLASSES[:4]:
        fr = R.assert_caps(cls, R.sgemm_want(cls, geom))
        print(f"caps sgemm {R.sid(geom)} {cls}: " + " ".join(f"{k}={v:.3f}" for k, v in fr.items()))
    d = R.sgemm_data("nan_inf", geom)
    if geom != (1, 1, 1):
        assert 3 <= np.isnan(d["a"]).sum() <= 6 and 3 <= np.isnan(d["b"]).sum() <= 6 and 2 <= np.isinf(d["a"]).sum() + np.isinf(d["b"]).sum() <= 4
    # outputs are non-finite exactly in the rows of a's and the columns of b's injected elements
    w = R.sgemm_want("nan_inf", geom)
    rows = ~np.isfinite(d["a"]).all(axis=0); cols = ~np.isfinite(d["b"]).all(axis=0)
    assert np.array_equal(~np.isfinite(w), rows[:, None] | cols[None, :])


def test_half_classes_hold_what_they_say():
    g = (100, 36, 50)
    h = R.gen_sgemm_half(g)
    want = {c: bo.sgemm(d["a"].astype(F), d["b"].astype(F)) for c, d in h.items()}
    big = want["big"]
    assert np.isfinite(big).all() and 0.1 < float((np.abs(big) > 65504).mean()) < 0.9            # finite in fp32, beyond the largest half: stores as Inf
    assert np.isinf(R.to_half(big)).mean() > 0.1
    sub = R.to_half(want["subnormal"])
    assert ((np.abs(sub) < 2.0 ** -14) & (sub != 0)).mean() > 0.2                                 # subnormal half results
    assert ((np.abs(h["subnormal"]["a"]) < 2.0 ** -14) & (h["subnormal"]["a"] != 0)).any()        # and subnormal half operands
    n = want["nan"]
    assert np.isnan(n).any() and np.isinf(n).any() and np.isfinite(n).mean() > 0.9


def test_assert_same_refuses_what_it_must():
    w = np.array([1.0, np.nan, np.inf, -np.inf, 0.0, 1e-40], F)
    R.assert_same(w, w.copy())
    R.assert_same(w, np.array([1.0, np.nan, np.inf, -np.inf, -0.0, 1e-40], F))                    # the sign of a zero is outside the contract
    g = w.copy(); R.bits(g)[1] = 0xFFC00001; R.assert_same(w, g)                                   # ... and so is a NaN's payload
    for bad in ([1.0, 1.0, np.inf, -np.inf, 0.0, 1e-40], [np.nan, np.nan, np.inf, -np.inf, 0.0, 1e-40], [1.0, np.nan, -np.inf, -np.inf, 0.0, 1e-40],
                [1.0, np.nan, np.inf, np.nan, 0.0, 1e-40], [1.0, np.nan, np.inf, -np.inf, 0.0, 0.0], [1.0, np.nan, 3e38, -np.inf, 0.0, 1e-40],
                [np.float32(1.0000001), np.nan, np.inf, -np.inf, 0.0, 1e-40]):
        with pytest.raises(AssertionError):
            R.assert_same(w, np.array(bad, F))
    assert R.assert_contained(w, np.array([1.0, np.inf, np.nan, -np.inf, 0.0, 1e-40], F)) == (1, 1)
    with pytest.raises(AssertionError):
        R.assert_contained(w, np.array([np.nan, np.nan, np.inf, -np.inf, 0.0, 1e-40], F))
    with pytest.raises(AssertionError):
        R.assert_contained(w, np.array([1.0, np.nan, np.inf, np.inf, 0.0, 1e-40], F))
    wr = np.array([1.0, 0.0, np.inf, 0.0, 0.0, 2.0], F)      # under the ReLU the exception's NaN is a 0 where the oracle has +Inf -- and nowhere else
    assert R.assert_contained(wr, np.array([1.0, 0.0, 0.0, 0.0, 0.0, 2.0], F), relu=True) == (0, 1) and R.assert_contained(wr, wr.copy(), relu=True) == (1, 0)
    for bad in ([1.0, 0.0, 0.0, 0.0, 0.0, 2.0], ):
        with pytest.raises(AssertionError):
            R.assert_contained(wr, np.array(bad, F))
    with pytest.raises(AssertionError):
        R.assert_contained(wr, np.array([0.0, 0.0, np.inf, 0.0, 0.0, 2.0], F), relu=True)
    with pytest.raises(AssertionError):
        R.assert_contained(wr, np.array([1.0, 0.0, np.inf, np.inf, 0.0, 2.0], F), relu=True)
    with pytest.raises(AssertionError):
        R.assert_no_poison(R.poison((3,)))
    R.assert_no_poison(w)


def test_window_mask_is_the_oracles():
    """One NaN through the oracle marks exactly the mask's pels, in every channel."""
    shape = (2, 5, 17, 13, 7, 5, 5, 2, 2)
    d = R.conv_data("wide", shape)
    x = d["in"].copy(); x[1, 3, 8, 6] = np.nan
    w = bo.conv_fwd(x, d["filts"] + F(1e-30), d["biases"], (2, 2), (2, 2), False)
    m = R.window_mask(shape, [(1, 3, 8, 6, "nan")])
    assert m.sum() == 9 and np.array_equal(np.isnan(w), np.broadcast_to(m[:, None], w.shape))


@pytest.mark.parametrize("shape", R.CONV_SHAPES, ids=R.sid)
def test_cpu_backend_conv_meets_the_contract(rtc, shape):
    """be=cpu's hip_conv (exact dims: NaN prefill and guard vars) on every class and both ReLU settings against the oracle."""
    res = R.run_conv(rtc, shape, {c: R.conv_data(c, shape) for c in R.CLASSES}, wide=False)
    for (cls, relu), r in res.items():
        what = (shape, cls, relu)
        R.assert_no_poison(r["out"], what)
        R.assert_same(R.conv_want(cls, shape, relu), r["out"], what)     # (be=cpu re-reads nothing: inf_last_chan too is equal outright)


@pytest.mark.parametrize("geom", R.SGEMM_GEOMS, ids=R.sid)
def test_cpu_backend_sgemm_meets_the_contract(rtc, geom):
    res = R.run_sgemm(rtc, geom, {c: R.sgemm_data(c, geom) for c in R.CLASSES[:4]})
    for cls, r in res.items():
        R.assert_no_poison(r["c"], (geom, cls))
        R.assert_same(R.sgemm_want(cls, geom), r["c"], (geom, cls))


def test_to_bf16_keeps_nans_and_rounds_the_rest_as_before():
    def one(u):
        return int(bo.to_bf16(np.array([u], np.uint32).view(F)).view(np.uint32)[0])
    # the four NaN patterns: the quiet NaN of the same sign and the same top 7 mantissa bits
    assert one(0x7FC00000) == 0x7FC00000 and one(0x7FFFFFFF) == 0x7FFF0000 and one(0xFFC00001) == 0xFFC00000 and one(0x7F800001) == 0x7FC00000
    assert one(0xFFFFFFFF) == 0xFFFF0000 and one(0x7F80FFFF) == 0x7FC00000
    assert one(0x7F800000) == 0x7F800000 and one(0xFF800000) == 0xFF800000                       # +-Inf
    assert one(0x7F7FFFFF) == 0x7F800000 and one(0x7F7F7FFF) == 0x7F7F0000 and one(0x7F7F8000) == 0x7F800000     # FLT_MAX rounds to Inf under RNE; below the half-way point it does not
    assert one(0x00000001) == 0 and one(0x00008000) == 0 and one(0x00008001) == 0x00010000 and one(0x807FFFFF) == 0x80800000     # subnormals (the smallest tie goes to even: 0)
    assert one(0x00000000) == 0 and one(0x80000000) == 0x80000000                                 # +-0
    assert one(0x3F808000) == 0x3F800000 and one(0x3F818000) == 0x3F820000 and one(0x3F808001) == 0x3F810000      # ties to even, both ways; just above a tie
    # finite data: bit for bit what the integer rounding gave before
    rng = np.random.default_rng(3)
    u = rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)
    u = u[(u & 0x7F800000) != 0x7F800000]
    old = ((u.astype(np.uint64) + (((u.astype(np.uint64) >> 16) & 1) + 0x7FFF)) & 0xFFFF0000).astype(np.uint32)
    assert np.array_equal(bo.to_bf16(u.view(F)).view(np.uint32), old)
    x = bo.gen_conv_in(2, 3, 9, 7)
    assert bo.to_bf16(x).shape == x.shape and np.array_equal(bo.to_bf16(bo.to_bf16(x)), bo.to_bf16(x))
