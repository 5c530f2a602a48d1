"""ResNet-50's new pieces on the MI355X (-m gpu):
  1. hip_chan_affine (kernels/bck_ops_f32.hip OP 13) on be=hip, bit for bit against be=cpu;
  2. the residual epilogue of the channels-last bf16 convolution (kernels/conv_nhwc_bf16.hip -DRES=1), one op at a time through profile_rcg_call, against
     want = relu(conv_fwd(bf16 in, bf16 filts, biases, no relu) + float(res)) from the oracle, held to the DERIVED bound of tests/test_gpu_nhwc.py with one more addition
     and S' = S + |res|:  |got - want| <= 2 (K + 2) 2^-24 S', a bf16 output + 2^-8 (|want| + that).  No fitted constant;
  3. the fp32 net (resnet50(2, 64) up to res3a) on be=hip, every node bit for bit against numpy (bo.conv_fwd, bo.pool_fwd, fold_affine and the written formulas);
  4. the channels-last bf16 net, whole, with the shortcut in the convolution's epilogue and without: every convolution call checked on the GPU's OWN inputs with the
     folded filters as the oracle's operands, the unfused sums exactly, and two graph replays on new inputs bit for bit against the eager step;
  5. the largest observed fraction of each bound, printed (DESIGN section 3.14 quotes them).
Nothing here reads the reference project."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import resnet_ref as rr
from boda_amd import conv_pipe as cpm
from boda_amd.cnn_op import OpTune
from boda_amd.conv_pipe import ConvPipeFwd, fold_affine, resnet50
from boda_amd.ops_prof import OpsBackend, profile_rcg_call
from boda_amd.rtc import make_rtc
from oracle import boda_oracle as bo

WORST = {}     # name of a bound -> the largest observed |got - want| / bound


def _note(name, err, lim):
    frac = float((err / np.maximum(lim, 1e-300)).max())
    WORST[name] = max(WORST.get(name, 0.0), frac)
    return frac


@pytest.fixture(scope="module")
def hip():
    r = make_rtc("(be=hip)", 0)
    r.init()
    yield r
    r.finish_and_sync()
    r.close()


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


# ---- 1. hip_chan_affine
@pytest.mark.parametrize("shape", rr.AFFINE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_chan_affine_on_hip_equals_cpu(hip, cpu, shape):
    x, a, b = rr.affine_data(shape)
    for relu in (0, 1):
        for in_place in (False, True):
            got = rr.run_affine(hip, shape, relu, in_place, x, a, b)
            launch = hip.last_launch()
            assert launch["kernel"] == "bodahip_chan_affine" and launch["block"] == 256, launch
            assert rr.bits_eq(got, rr.run_affine(cpu, shape, relu, in_place, x, a, b)), (shape, relu, in_place)


# ---- 2. the residual convolution, one op at a time
def _run_res(be, case, out_f32, relu, run_iter=1):
    a = rr.res_func_op(case, out_f32, relu)
    up, res = rr.res_data(case, out_f32)
    outs, prc = profile_rcg_call(be, a, 5, 0.0, run_iter, include_ins=True, tile=rr.RES_CASES[case][4], ins={"res": up})
    return outs, prc, res


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("case", sorted(rr.RES_CASES))
def test_residual_conv_vs_oracle(hip, case, relu):
    be = OpsBackend(hip)
    o32, p32, res = _run_res(be, case, True, relu)
    o16, p16, res16 = _run_res(be, case, False, relu)
    assert np.array_equal(res, res16)
    for prc in (p32, p16):
        assert prc.launch["kernel"] == "bodahip_conv_nhwc_bf16", prc.launch
    if rr.RES_CASES[case][4]:
        assert "_s4" in p32.launch["cfg"] and "_s4" in p16.launch["cfg"], (p32.launch, p16.launch)      # four K slices, reduced inside the launch
    want, lim = rr.res_want_and_limit(o32["in"], o32["filts"], o32["biases"], res, relu)
    assert (res > 0).any() and (res < 0).any()
    if relu:
        cut = (want == 0); assert cut.any() and (~cut).any()       # the ReLU cuts some sums and leaves others
    g32, g16 = o32["out"], o16["out"]
    assert np.isfinite(g32).all() and np.isfinite(g16).all()
    e32 = np.abs(g32.astype(np.float64) - want.astype(np.float64))
    f32 = _note("residual conv, float out: 2 (K + 2) 2^-24 S'", e32, lim)
    print(f"{case} relu={relu} float out: worst err / bound = {f32:.4f} [{p32.launch['cfg']}]")
    assert (e32 <= lim).all(), (case, relu, p32.launch["cfg"], f32)
    assert np.array_equal(bo.to_bf16(g16), g16)                    # every value is a bf16
    e16 = np.abs(g16.astype(np.float64) - want.astype(np.float64)); lim16 = rr.bf16_limit(want, lim)
    f16 = _note("residual conv, bf16 out: + 2^-8 (|want| + that)", e16, lim16)
    print(f"{case} relu={relu} bf16 out:  worst err / bound = {f16:.4f} [{p16.launch['cfg']}]")
    assert (e16 <= lim16).all(), (case, relu, p16.launch["cfg"], f16)
    # ONE rounding: the bf16 launch is the float launch's fp32 sum rounded once (same tile, same slices: the same fp32 value per output)
    assert p16.launch["cfg"] == p32.launch["cfg"], (p16.launch, p32.launch)
    assert np.array_equal(g16, bo.to_bf16(g32)), (case, relu, float(np.abs(g16 - bo.to_bf16(g32)).max()))
    # the flagged launch again and again on the same workspace (the K slices' tickets are reset by the last arriver): the same bits
    for out_f32, first in ((True, g32), (False, g16)):
        again, _, _ = _run_res(be, case, out_f32, relu, run_iter=3)
        assert rr.bits_eq(again["out"], first), (case, relu, out_f32)


def test_residual_conv_refusals_at_run_time(hip):
    """What only the call can see: no `res` var, a var of other dims or another element type, `res` aliased to `out`, an output channel slice.  Each is refused with its
    own message before anything is launched."""
    from boda_amd.cnn_op import pipe_func_args
    from boda_amd.op import Dims, RtErr, UnsupErr
    from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo
    a = rr.res_func_op("ragged_2x24x7x40", False, 1)
    hip.compile([RtcFuncInfo("rf", "", [n for n, _ in pipe_func_args(a)], a)])
    made = []
    def var(vn, d):
        hip.create_var_with_dims(vn, d); made.append(vn)
    try:
        for an in ("filts", "biases", "in", "out", "res"):
            var(an, a.get_dims(an))
        o = a.get_dims("out")
        var("res_small", Dims(o.names, (o.sizes[0], o.sizes[1], o.sizes[2], 32), "bfloat16"))
        var("res_f32", Dims(o.names, o.sizes, "float"))
        var("out_wide", Dims(o.names, (o.sizes[0], o.sizes[1], o.sizes[2], 48), "bfloat16")); var("res_wide", Dims(o.names, (o.sizes[0], o.sizes[1], o.sizes[2], 48), "bfloat16"))
        am = {"filts": RtcArg.var("filts"), "biases": RtcArg.var("biases"), "in": RtcArg.var("in"), "stride": RtcArg.ref(a.get_dims("stride")), "in_pad": RtcArg.ref(a.get_dims("in_pad")),
              "res": RtcArg.var("res"), "out": RtcArg.var("out")}
        bad = lambda **kw: RtcFuncCall("rf", dict({k: v for k, v in am.items() if kw.get(k, 1) is not None}, **{k: v for k, v in kw.items() if v is not None}))
        with pytest.raises(RtErr, match="the var arg 'res' is required"):
            hip.run(bad(res=None))
        with pytest.raises(RtErr, match="res dims"):
            hip.run(bad(res=RtcArg.var("res_small")))
        with pytest.raises(RtErr, match="res has type float, out bfloat16"):
            hip.run(bad(res=RtcArg.var("res_f32")))
        with pytest.raises(RtErr, match="are the same var"):
            hip.run(bad(res=RtcArg.var("out")))
        with pytest.raises(UnsupErr, match="output channel slice"):
            hip.run(bad(out=RtcArg.var("out_wide"), res=RtcArg.var("res_wide"), out_chan_off=RtcArg.scalar(8, "uint32_t")))
        hip.run(RtcFuncCall("rf", am)); hip.finish_and_sync()      # (and the well-formed call runs)
        assert hip.last_launch()["kernel"] == "bodahip_conv_nhwc_bf16"
    finally:
        hip.finish_and_sync()
        for vn in made:
            hip.release_var(vn)
        hip.release_func("rf"); hip.release_per_call_id_data()


# ---- 3. the fp32 net
def test_fp32_net_every_node_bit_equal_to_numpy(hip):
    cp = rr.truncated(resnet50(2, 64), "res3a")
    P = rr.he_params(cp, 1)
    x = np.random.default_rng(2).uniform(-1, 1, cp.nodes["data"].sizes).astype(np.float32)
    val, snaps = rr.ref_forward_f32(cp, P, x)
    f = ConvPipeFwd(hip)
    f.init(cp, P)
    try:
        funcs = {c.func for c in f.fwd_calls}
        assert {"hip_conv", "hip_chan_affine", "hip_reduce", "hip_zero_if_non_pos", "fwd_pool"} == funcs, funcs
        nodes = [n for n in cp.nodes if n != "data"]
        fwd = {"data": x}
        f.run_fwd(["data"], fwd, nodes)
        kinds = {}
        for kind, top, _ in snaps:
            kinds[top] = kind      # (what wrote the node last)
        assert set(kinds.values()) == {"affine", "pool", "relu"} and {k for k, _, _ in snaps} >= {"conv", "eltwise"}
        for n in nodes:
            assert np.isfinite(val[n]).all() and rr.bits_eq(fwd[n], val[n]), (n, kinds[n], float(np.abs(fwd[n] - val[n]).max()))
        assert (val["res3a"] > 0).any() and (val["res2a_branch2c"] < 0).any()
        # ... and call by call on the device's own inputs, so that a convolution and a sum are each seen alone: run the step again one call at a time
        hip.copy_nda_to_var("data", x)
        it = iter(snaps)
        for c in f.fwd_calls:
            hip.run(c.rfc); hip.finish_and_sync()
            kind, top, want = next(it)
            if c.func == "hip_conv":      # (a convolution's ReLU, where it has one, is part of its call and of its snapshot)
                assert kind == "conv"
            got = hip.copy_var_to_nda(f.var_of(top))
            assert rr.bits_eq(got, want), (c.tag, c.func, kind, top)
    finally:
        f.release()


# ---- 4. the channels-last bf16 net
def _conv_operands(cp, P):
    """Per convolution: the fp32 filters and biases its call reads, i.e. the affine run behind it folded in (fold_affine; filts * a, biases * a + b), and whether a ReLU ends the run."""
    runs = {r["conv"].tag: r for r in cpm.affine_runs(cp) if r["conv"] is not None}
    out = {}
    for i, o in enumerate(cp.ops):
        if o.type != "Convolution":
            continue
        F, Bv = P[o.tag + "_filts"], P[o.tag + "_biases"]
        if o.tag in runs:
            a, b = fold_affine(rr.affine_steps(P, runs[o.tag]["ops"]))
            F = (F * a[:, None, None, None]).astype(np.float32); Bv = (Bv * a + b).astype(np.float32)
            relu = runs[o.tag]["relu"] is not None
        else:
            relu = i + 1 < len(cp.ops) and cp.ops[i + 1].type == "ReLU" and cp.ops[i + 1].bot == o.top
        out[o.tag] = (F, Bv, relu)
    return out


@pytest.fixture(scope="module")
def net():
    cp = resnet50(2, 64)
    P = rr.he_params(cp, 3)
    xs = [np.random.default_rng(10 + i).uniform(-1, 1, cp.nodes["data"].sizes).astype(np.float32) for i in range(3)]
    return cp, P, xs, _conv_operands(cp, P)


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])
def test_bf16_net_every_conv_on_the_gpus_own_inputs_and_graph_replays(hip, net, fuse):
    cp, P, xs, operands = net
    f = ConvPipeFwd(hip, OpTune(hip_dtype="bf16", hip_layout="nhwc"), fuse_residual=fuse)
    f.init(cp, P)
    try:
        elt = {o.tag: o for o in cp.ops if o.type == "Eltwise"}
        funcs = [c.func for c in f.fwd_calls]
        if fuse:
            assert f.fused_residuals == {"folded": list(elt), "unfolded": {}} and "nhwc_eltwise" not in funcs and "nhwc_relu" not in funcs
        else:
            assert funcs.count("nhwc_eltwise") == 16 and f.fused_residuals["folded"] == []
        nodes = [n for n in cp.nodes if n != "data" and n not in f._res_nodes]
        fwd = {"data": xs[0]}
        f.run_fwd(["data"], fwd, nodes)
        for n in nodes:
            assert np.isfinite(fwd[n]).all(), n
            assert np.array_equal(bo.to_bf16(fwd[n]), fwd[n]), n      # every node holds bf16 values
        assert np.abs(fwd["fc1000"]).max() > 0 and (fwd["res5c"] > 0).any()
        folded = {q: e for q, e in f._res_nodes.items()}                 # node of a flagged convolution -> the Eltwise top it writes
        tag = "fused" if fuse else "unfused"
        data16 = bo.to_bf16(xs[0])                                        # (the layout pass rounds the net's input)
        for o in cp.ops:
            if o.type != "Convolution":
                continue
            F, Bv, relu = operands[o.tag]
            inp = data16 if o.bot == "data" else fwd[o.bot]
            res, out_node = None, o.top
            if o.top in folded:           # the call adds the shortcut and applies the block's ReLU
                e = elt[folded[o.top]]
                other = e.bots[0] if e.bots[1] == o.top else e.bots[1]
                res, out_node, relu = fwd[other], e.top, True
            want, lim = rr.res_want_and_limit(inp, F, Bv, res, relu, tuple(o.stride), tuple(o.in_pad))
            lim16 = rr.bf16_limit(want, lim)
            err = np.abs(fwd[out_node].astype(np.float64) - want.astype(np.float64))
            frac = _note(f"bf16 net ({tag}), " + ("flagged convolutions" if res is not None else "plain convolutions"), err, lim16)
            assert (err <= lim16).all(), (o.tag, out_node, frac)
        if not fuse:      # the generic kernel: fp32 sum of the two bf16 values, ReLU, ONE rounding -- exactly, on the device's own inputs
            for e in elt.values():
                s = fwd[e.bots[0]] + fwd[e.bots[1]]
                assert np.array_equal(fwd[e.top], bo.to_bf16(np.where(s > 0, s, np.float32(0.0)).astype(np.float32))), e.tag
        # poolings: a maximum is exact; the global average is an fp32 sum of 4 values divided by 4, rounded once
        assert np.array_equal(fwd["pool1"], bo.pool_fwd(fwd["conv1"], (3, 3), (2, 2), (0, 0), False))
        p5 = bo.pool_fwd(fwd["res5c"], (2, 2), (1, 1), (0, 0), True)
        assert (np.abs(fwd["pool5"] - p5) <= 2.0 ** -8 * np.abs(p5) + 4 * 2.0 ** -24 * bo.pool_fwd(np.abs(fwd["res5c"]), (2, 2), (1, 1), (0, 0), True) * 4).all()
        # one graph replay per new input against the eager step on the same input: every node the step writes, bit for bit
        stay = [n for n in nodes if n not in f._lazy]
        n_calls = f.capture_graph()
        assert n_calls == len(f.fwd_calls)
        for x in xs[1:]:
            hip.copy_nda_to_var(f.in_var, x); hip.finish_and_sync()
            f.run_graph()
            replay = {n: f._fetch(n) for n in stay}
            eager = {"data": x}
            f.run_fwd(["data"], eager, stay)
            for n in stay:
                assert rr.bits_eq(replay[n], eager[n]), (n, tag)
            assert not rr.bits_eq(eager["fc1000"], fwd["fc1000"])       # (a new input gives new values: the replay did not just leave the old ones)
    finally:
        f.release()


# ---- 5. the figures
def test_zz_print_worst_fractions_of_the_bounds():
    assert WORST, "run with the tests above: they record the figures"
    for name in sorted(WORST):
        print(f"worst |got - want| / bound -- {name}: {WORST[name]:.4f}")
    assert all(v <= 1.0 for v in WORST.values())
