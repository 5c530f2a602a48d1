"""The reference side of the special-data tests of the backward kernels (tests/bck_special_ref.py; the GPU side is tests/test_gpu_bck_special.py), on a machine
without a GPU: the generators give what they say, be=cpu's gradients on them stay inside the blindness caps for every (gradient, shape, class) the GPU file uses, the
written chain emulators (oracle/bck_chain.py, tests/bconv_fb_ref.py) equal be=cpu by value on every finite class, the B3 rules hold on the emulators -- which form
the kernels' padded zero operands, so what the GPU file will see of a leak is seen here first --, the comparison functions refuse what they must, and the runner's
guards, poison and read-back run on be=cpu (every be=cpu result of this file went through them).  DESIGN.md section 3.11a holds the contract and the figures
printed here (run with -s)."""
import numpy as np
import pytest

import bck_special_ref as R
import bconv_fb_ref as fb
from fwd_special_ref import NAN_BITS, POISON_BITS, assert_no_poison, assert_same, bits, poison
from oracle import bck_chain as bc
from oracle.boda_oracle import to_bf16

F = np.float32
CONV = [(g, n) for n in R.SHAPES for g in R.GRADS] + [("filts", n) for n in R.FB_SHAPES]
shape_of = lambda n: R.SHAPES.get(n) or R.FB_SHAPES[n]


def _mag_range(v):
    a = np.abs(v[np.isfinite(v) & (v != 0)].astype(np.float64))
    return float(np.log2(a.min())), float(np.log2(a.max()))


def test_generators_give_what_they_say():
    shape = R.SHAPES["5x5_s2_pad3_pad_ge_stride"]
    d = R.gen("wide", "in", shape)
    for an in ("in", "filts", "out_grad_loss"):
        lo, hi = _mag_range(d[an]); assert -40 <= lo and hi <= 30 and np.isfinite(d[an]).all()
        assert 0.02 < float(((d[an] == 0) & np.signbit(d[an])).mean()) < 0.08
    tiny = np.finfo(F).tiny
    for grad in ("in", "filts"):
        d = R.gen("subnormal", grad, shape); s = R.shift_of("subnormal", grad, shape)
        g = d["out_grad_loss"]; sub = (np.abs(g) < tiny) & (g != 0)
        lo, hi = _mag_range(g[~sub]); assert -76 + s <= lo and hi <= -62 + s and 0 < sub.sum() <= g.size // 20 + 1
        lo, hi = _mag_range(d["filts"]); assert -76 <= lo and hi <= -62
        d = R.gen("overflow", grad, shape); s = R.shift_of("overflow", grad, shape)
        lo, hi = _mag_range(d["out_grad_loss"]); assert 55 + s <= lo and hi <= 64 + s
        lo, hi = _mag_range(d["in"]); assert 55 <= lo and hi <= 64
    # a moved window keeps its width; the bias gradient's lies at the edge of the format and stays finite
    e = R.SHAPES["3x3_s1_img1_chan_not_32"]
    lo, hi = _mag_range(R.gen("overflow", "in", e)["out_grad_loss"]); assert 54 <= lo and hi <= 63 and R.shift_of("overflow", "in", e) == -1
    g = R.gen("overflow", "biases", shape)["out_grad_loss"]; assert np.isfinite(g).all() and _mag_range(g)[0] >= 55 + 63
    g = R.gen("subnormal", "biases", shape)["out_grad_loss"]; assert ((np.abs(g) < tiny) & (g != 0)).mean() > 0.3
    assert np.array_equal(bits(R.gen("wide", "in", shape)["in"]), bits(R.gen("wide", "in", shape)["in"]))
    assert not np.array_equal(bits(R.gen("wide", "in", shape, seed=1)["in"]), bits(R.gen("wide", "in", shape)["in"]))
    assert not np.array_equal(bits(R.gen("wide", "filts", shape)["in"]), bits(R.gen("wide", "in", shape)["in"]))
    z = R.zinp_in(shape)
    assert all((bits(z) == p).sum() > 0 for p in (0, 0x80000000, 0x7FC00000, 0xFFC00001, 0xFF800000, 1, 0x80000001)) and 0.3 < (z > 0).mean() < 0.6


@pytest.mark.parametrize("name", list(R.SHAPES) + list(R.FB_SHAPES))
def test_nan_inf_placement(name):
    shape = shape_of(name)
    B, C, H, W, OC = shape[:5]
    OH, OW = R.out_hw(shape)
    clean = R.gen("clean", "in", shape)
    for cls, an in (("nan_inf", "out_grad_loss"), ("nan_inf_in", "in"), ("nan_inf_filts", "filts"), ("bf16_saturate", "out_grad_loss"), ("bf16_saturate_in", "in")):
        d = R.gen(cls, "in", shape)
        x = d[an]; nf = ~np.isfinite(x)
        assert d["where"] == an and nf.sum() == (0 if cls.startswith("bf16") else len(d["inj"]))
        for other in ("in", "filts", "out_grad_loss"):     # one tensor is injected, everything else is the clean base
            m = nf if other == an else np.zeros(d[other].shape, bool)
            if cls.startswith("bf16") and other == an:
                m = np.zeros(x.shape, bool)
                for *at, _ in d["inj"]:
                    m[tuple(at)] = True
            assert np.isfinite(d[other][~m]).all() and np.array_equal(d[other][~m], clean[other][~m])
        if cls == "nan_inf_filts":
            assert np.isnan(x).sum() == 1 and np.isinf(x).sum() == 1
            continue
        if cls.startswith("bf16"):
            v = np.array([x[tuple(at)] for *at, _ in d["inj"]])
            with np.errstate(over="ignore"):
                r = to_bf16(v)
            assert np.isfinite(v).all() and np.isinf(r).all() and (bits(np.abs(v)) >= 0x7F7F8000).all()
            assert [k for *_, k in d["inj"]] == ["+inf" if s > 0 else "-inf" for s in np.sign(r)]
            continue
        nan, inf = np.isnan(x), np.isinf(x)
        assert 4 <= nan.sum() <= 6 and 2 <= inf.sum() <= 4 + (an == "in"), (nan.sum(), inf.sum())
        assert set(np.unique(bits(x)[nan])) == set(NAN_BITS) and np.isposinf(x).any() and np.isneginf(x).any()
        assert nan.reshape(-1)[0] and nf.reshape(-1)[-1]                                   # the first and the last element
        at = [one[:4] for one in d["inj"]]
        if an == "out_grad_loss":
            assert any(a[0] == 0 and a[2:] == (OH - 1, OW - 1) for a in at) and any(a[0] == B - 1 and a[2:] == (0, 0) for a in at)     # the last pel of an image, the first of the next
            assert any(0 < a[2] < OH - 1 and 0 < a[3] < OW - 1 for a in at) or min(OH, OW) < 3                                          # an interior pel
            assert any((a[2] in (0, OH - 1)) != (a[3] in (0, OW - 1)) for a in at) or min(OH, OW) < 3                                   # a border pel that is no corner
            for i, a in enumerate(at):                     # no two within one window of each other: no in pel's chain holds two injected values
                for b in at[:i]:
                    assert not (R.in_windows(shape, d["inj"][i])[1] & R.in_windows(shape, (b[0], 0, b[2], b[3], ""))[1]).any(), (a, b)
            rows = {}
            for _, oc, _, _, k in d["inj"]:
                rows.setdefault(oc, set()).add(k)
            assert {"+inf"} in rows.values() and {"-inf"} in rows.values() and len(rows) <= 4     # a row of +Inf alone, one of -Inf alone


def _bias_bound(g):
    a = np.abs(np.asarray(g, np.float64)).sum(axis=(0, 2, 3))
    n = g.size // g.shape[1]
    return (n + 8) * R.U * a + n * 2.0 ** -149


@pytest.mark.parametrize("grad,name", CONV, ids=lambda v: v if isinstance(v, str) else None)
def test_caps_and_emulators_against_the_cpu_backend(grad, name):
    """Per (gradient, shape): every class's be=cpu result inside the caps (on the outputs a real term reaches); on every finite class the single-chain emulator
    equals be=cpu by value -- be=cpu skips the padded terms, so the sign of a zero is outside this comparison.  The bias emulators are other associations than
    be=cpu's sequential chain (a strided chain per thread and a tree; BK residue chains): both are held to float64 instead, and `overflow`, which moves with the
    association, is compared on the GPU against the emulator alone."""
    shape = shape_of(name)
    reach = R.reached(grad, shape)
    assert bool(reach.all()) == (name not in ("1x1_s2_stride_gt_kernel",) or grad != "in")
    for cls in R.FINITE + ("nan_inf",) + (("nan_inf_in",) if grad == "filts" else ()):
        want = R.cpu_want(cls, grad, shape)
        fr = R.assert_caps(cls, want, reach)
        print(f"caps {grad} {name} {cls} shift={R.shift_of(cls, grad, shape) if cls in ('subnormal', 'overflow') else 0}: " + " ".join(f"{k}={v:.3f}" for k, v in fr.items()))
        if cls not in R.FINITE:
            continue
        if grad != "biases":
            assert_same(want, R.emu(cls, grad, shape).reshape(want.shape), (grad, name, cls))
            assert (bits(want)[~reach] == 0).all()          # what no term reaches is exactly +0
        elif cls != "overflow":
            g = R.data(cls, grad, shape)["out_grad_loss"]
            s = np.asarray(g, np.float64).sum(axis=(0, 2, 3))
            for got in (want.reshape(-1), R.emu(cls, grad, shape), fb.biases_chain(g, 16, 3), fb.biases_chain(g, 32, 7)):
                assert (np.abs(got.astype(np.float64) - s) <= _bias_bound(g)).all(), (name, cls)


def test_caps_refuse_blind_data():
    shape = R.T17
    u5 = R.cpu_want("clean", "in", shape)
    for cls in ("subnormal", "overflow", "nan_inf"):
        with pytest.raises(AssertionError):
            R.assert_caps(cls, u5)
    with pytest.raises(AssertionError):     # 75 % exact zeros: a 1x1 at stride 2 without the reach mask
        R.assert_caps("wide", R.cpu_want("wide", "in", R.SHAPES["1x1_s2_stride_gt_kernel"]))
    with pytest.raises(AssertionError):     # the windows without their shift: K = 900 terms overflow nearly always
        e = R.SHAPES["3x3_s1_img1_chan_not_32"]
        d = R.gen("overflow", "in", e, shift=2)
        R.assert_caps("overflow", bc.in_grad_chain(d["filts"], d["out_grad_loss"], R.geom_of(e)))


@pytest.mark.parametrize("name", list(R.SHAPES))
def test_b3_rules_hold_on_the_emulators(name):
    """The emulators form the kernels' padded +0 operands: run as `the kernel` through the GPU file's B3 checks they pass, and show the leaks a kernel may show."""
    shape = R.SHAPES[name]
    B, C, H, W, OC, KH, KW, SY, SX, PY, PX = shape
    d = R.data("nan_inf", "in", shape)
    leaked, of = R.check_in_b3(shape, d, R.emu("nan_inf", "in", shape), R.emu("clean", "in", shape), R.cpu_want("nan_inf", "in", shape), name)
    print(f"emulator in_grad {name}: {leaked} of {of} elements of L \\ R non-finite")
    if KH % SY == 0 and KW % SX == 0:
        assert of == 0      # the stride divides the kernel size: L is R
    else:
        assert leaked == of > 0      # a zero tap times a NaN or an Inf: every one of them leaks, as a NaN
    # be=cpu itself: nothing outside R
    w = R.cpu_want("nan_inf", "in", shape)
    assert R.check_in_b3(shape, d, w, R.cpu_want("clean", "in", shape), w, name)[0] == 0
    for bk, ksl in ((32, 1), (16, 3), (16, 7)):
        leaked, of = R.check_filts_b3_ogl(shape, d, R.emu("nan_inf", "filts", shape, bk, ksl), R.emu("clean", "filts", shape, bk, ksl), R.cpu_want("nan_inf", "filts", shape), name)
        print(f"emulator filts_grad {name} bk={bk} ksl={ksl}: {leaked} padding taps of {of} row elements non-finite where be=cpu is finite")
        assert (leaked > 0) == (PY > 0 or PX > 0) or ksl > 1
        di = R.data("nan_inf_in", "in", shape)
        R.check_filts_b3_in(di, R.emu("nan_inf_in", "filts", shape, bk, ksl), R.emu("clean", "filts", shape, bk, ksl), R.cpu_want("nan_inf_in", "filts", shape), name)
    df = R.data("nan_inf_filts", "in", shape)
    got, ref_ = R.check_in_b3_filts(shape, df, R.emu("nan_inf_filts", "in", shape), R.emu("clean", "in", shape), R.cpu_want("nan_inf_filts", "in", shape), name)
    print(f"emulator in_grad {name}, non-finite filts: {got} non-finite elements, be=cpu {ref_}")
    assert got >= ref_ > 0
    g = d["out_grad_loss"]
    with np.errstate(all="ignore"):      # one non-finite term decides a sum in any association: the three bias chains agree on the masks
        k = R.kind(R.cpu_want("nan_inf", "biases", shape).reshape(-1))
        assert np.array_equal(k, R.kind(bc.biases_chain(g))) and np.array_equal(k, R.kind(fb.biases_chain(g, 16, 3))) and set(k) == {0, 1, 2, 3}


def test_b3_checks_refuse_what_they_must():
    shape = R.S2
    d = R.data("nan_inf", "in", shape)
    got, clean, want = R.emu("nan_inf", "in", shape), R.emu("clean", "in", shape), R.cpu_want("nan_inf", "in", shape)
    Rm, Lm = (np.any([R.in_windows(shape, one)[i] for one in d["inj"]], axis=0) for i in (0, 1))
    out = tuple(int(v[0]) for v in np.nonzero(~Lm)); inr = tuple(int(v[0]) for v in np.nonzero(Rm))
    for at, val in (((out[0], 3) + out[1:], np.nan), ((out[0], 3) + out[1:], 1.0), ((inr[0], 2) + inr[1:], 1.0)):
        bad = got.copy(); bad[at] = val
        with pytest.raises(AssertionError):
            R.check_in_b3(shape, d, bad, clean, want)
    inf_at = [one for one in d["inj"] if one[4] == "+inf"][0]
    m = np.broadcast_to(R.in_windows(shape, inf_at)[0][:, None], got.shape)
    bad = got.copy(); bad[m] = np.nan      # an Inf's pels came back as NaN: not the reference's kind
    with pytest.raises(AssertionError):
        R.check_in_b3(shape, d, bad, clean, want)
    gf, cf, wf = R.emu("nan_inf", "filts", shape), R.emu("clean", "filts", shape), R.cpu_want("nan_inf", "filts", shape)
    rows = sorted({one[1] for one in d["inj"]}); free = [r for r in range(shape[4]) if r not in rows][0]
    for at, val in (((free, 0, 0, 0), np.inf), ((free, 1, 1, 1), 0.5), ((rows[0], 2, 1, 1), 0.5)):
        bad = gf.copy(); bad[at] = val
        with pytest.raises(AssertionError):
            R.check_filts_b3_ogl(shape, d, bad, cf, wf)
    di = R.data("nan_inf_in", "in", shape)
    gi, wi = R.emu("nan_inf_in", "filts", shape), R.cpu_want("nan_inf_in", "filts", shape)
    fin = tuple(int(v[0]) for v in np.nonzero(np.isfinite(wi))); nf = tuple(int(v[0]) for v in np.nonzero(np.isposinf(wi)))
    for at, val in ((fin, np.nan), (fin, 0.25), (nf, -np.inf), (nf, np.nan)):
        bad = gi.copy(); bad[at] = val
        with pytest.raises(AssertionError):
            R.check_filts_b3_in(di, bad, cf, wi)
    w = np.array([1.0, -0.0, np.nan, np.inf, 1e-40], F)
    R.assert_bits(w, w.copy())
    g = w.copy(); bits(g)[2] = 0xFFC00001; R.assert_bits(w, g)     # a NaN's payload is outside the contract
    for bad in ([1.0, 0.0, np.nan, np.inf, 1e-40], [1.0, -0.0, 1.0, np.inf, 1e-40], [1.0, -0.0, np.nan, -np.inf, 1e-40], [1.0, -0.0, np.nan, np.inf, 0.0], [np.nan, -0.0, np.nan, np.inf, 1e-40]):
        with pytest.raises(AssertionError):     # ... the sign of a zero is inside it
            R.assert_bits(w, np.array(bad, F))
    with pytest.raises(AssertionError):
        assert_no_poison(poison((3,)))


def test_minus_zero_where_the_reference_skips_a_padded_term():
    """A bordered pel whose real products all underflow negative: fma(g, w, +0) rounds to -0 and stays -0 through every real term.  be=cpu, which skips the terms
    outside the plane, returns -0; the emulator (and the kernel, tests/test_gpu_bck_special.py) forms fma(+0, w, -0) = +0 for a padded term that comes last in the
    chain, as it does in the bottom row and the right column (out_x outer, out_y inner, ascending).  At the top left corner the padded terms come first: -0 both ways.
    With a K tail (9 terms under a K step of 16) the chain always ends in fma(+0, +0, acc): +0 everywhere."""
    shape, d = R.minus_zero_case(16)
    cpu = R.run_fop(R.cpu_rtc(), R.func_of("in", shape), {"m0": d}, pfx="bsm_")["m0"]["in_grad_loss"]
    assert (bits(cpu) == 0x80000000).all()
    for bk in (0, 16):      # 144 terms: whole K steps
        em = bc.in_grad_chain(d["filts"], d["out_grad_loss"], R.geom_of(shape), bk)
        assert (bits(em)[0, 0, :3, :3] == 0x80000000).all() and (bits(em)[0, 0, 3, :] == 0).all() and (bits(em)[0, 0, :, 3] == 0).all()
        assert_same(cpu, em)      # by value they agree: the contract's comparison on the CPU
    assert (bits(bc.in_grad_chain(d["filts"], d["out_grad_loss"], R.geom_of(shape), 32)) == 0).all()      # 144 = 4 * 32 + 16: a tail
    shape, d = R.minus_zero_case(1)
    cpu = R.run_fop(R.cpu_rtc(), R.func_of("in", shape), {"m0": d}, pfx="bsm_")["m0"]["in_grad_loss"]
    assert (bits(cpu) == 0x80000000).all() and (bits(bc.in_grad_chain(d["filts"], d["out_grad_loss"], R.geom_of(shape), 16)) == 0).all()
    # the filter gradient's emulator: a slice that ends in the K tail turns its -0 into +0, whole K steps keep it
    I = np.full((16, 1), -(2.0 ** -100), F); J = np.full((16, 2), 2.0 ** -100, F)
    assert (bits(bc.filts_sliced_chain(I, J, 16, 1)) == 0x80000000).all() and (bits(bc.filts_sliced_chain(I, J, 8, 1)) == 0x80000000).all()
    assert (bits(bc.filts_sliced_chain(I, J, 32, 1)) == 0).all() and (bits(bc.filts_sliced_chain(I[:15], J[:15], 8, 1)) == 0).all()
    assert (bits(bc.filts_sliced_chain(I, J, 8, 3)) == 0).all()      # ... and an empty third slice adds its +0 slab


def test_runner_poisons_guards_and_reads_back_on_the_cpu_backend():
    shape = R.T17
    cpu = R.cpu_rtc()
    made = []
    orig = cpu.copy_nda_to_var
    try:      # every OUT var is refilled with the payload NaN before every run, every guard var filled once
        cpu.copy_nda_to_var = lambda vn, a: (made.append((vn, np.array(a))), orig(vn, a))[1]
        res = R.run_fop(cpu, R.func_of("fb", shape), {c: R.data(c, "filts", shape) for c in ("wide", "clean")}, pfx="bsq_")
    finally:
        del cpu.copy_nda_to_var
    for an in ("filts_grad_loss", "biases_grad_loss"):
        fills = [a for vn, a in made if vn == "bsq_" + an]
        assert len(fills) == 2 and all((bits(a) == POISON_BITS).all() for a in fills)
        assert_no_poison(res["wide"][an]); assert_no_poison(res["clean"][an])
    assert sorted(vn for vn, a in made if vn.endswith("_guard")) == sorted("bsq_" + an + "_guard" for an in ("in", "out_grad_loss", "filts_grad_loss", "biases_grad_loss"))
    assert_same(res["wide"]["filts_grad_loss"], R.cpu_want("wide", "filts", shape))


# ---- bf16 operands on be=cpu
@pytest.mark.parametrize("name", ["3x3_s2_k_not_multiple_of_s", "3x3_s1_two_imgs_17_chans"])
def test_cpu_backend_bf16_operands(name):
    """be=cpu's hip_operands=bf16 forms (the template loops on rounded copies): the reference of the GPU file's masks.  Held here to the bound on `wide`, and on
    bf16_saturate to the masks of the fp32 function on operands rounded by oracle.to_bf16."""
    shape = R.SHAPES[name]
    cpu = R.cpu_rtc()
    for grad, out in (("in", "in_grad_loss"), ("fb", "filts_grad_loss")):
        which = "in" if grad == "in" else "filts"
        sat = ("bf16_saturate",) + (("bf16_saturate_in",) if grad == "fb" else ())      # (the data gradient does not read `in`)
        sets = {c: R.data(c, which, shape) for c in ("wide",) + sat}
        res = R.run_fop(cpu, R.func_of(grad, shape, bf16=True), sets, pfx="bsb_")
        R.check_bf16_bound(shape, which, res["wide"][out], R.bf16_refs(shape, sets["wide"]), 1, with_nrms=True, what=(name, grad))
        for c in sat:
            with np.errstate(over="ignore"):
                rounded = {an: (to_bf16(v) if isinstance(v, np.ndarray) else v) for an, v in sets[c].items()}
            w = R.run_fop(cpu, R.func_of(grad, shape), {c: rounded}, pfx="bsc_")[c][out]
            assert np.array_equal(R.kind(res[c][out]), R.kind(w)) and (R.kind(w) >= 2).any(), (name, grad, c)
        if grad == "fb":      # the bias gradient is summed from the unrounded out_grad_loss
            R.assert_bits(R.run_fop(cpu, R.func_of("fb", shape), {"s": sets["bf16_saturate"]}, pfx="bsc_")["s"]["biases_grad_loss"], res["bf16_saturate"]["biases_grad_loss"])


def test_fixture_file_lists_the_gpu_files_function_ops():
    """tests/golden/ops/bck-special-ops.txt is what the build pre-specialises for tests/test_gpu_bck_special.py: exactly the function ops of its forms (write
    the lines of R.gpu_fops() to it when a form changes)."""
    import os
    from boda_amd.op import read_ops
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops", "bck-special-ops.txt")
    lines = list(dict.fromkeys(f.to_str() for f in R.gpu_fops()))
    assert [l for l in open(path).read().splitlines() if l and not l.startswith("#")] == lines
    assert len(read_ops(path)) == len(lines) >= 70


# ---- the other backward functions on be=cpu (the cases of tests/bck_special_ref.py): the checks of the GPU file, with be=cpu as the function under test
@pytest.mark.parametrize("case", sorted(R.CASES))
def test_cpu_backend_other_backward_functions(case):
    R.CASES[case](R.cpu_rtc(), R.cpu_rtc())
