"""hip_bconv_filts_biases on the MI355X, held to its written chains: every comparison of a launch is np.array_equal on the fp32 bit patterns, against
oracle/bck_chain.filts_chain(in, out_grad_loss, geom, BK, KSL) and tests/bconv_fb_ref.biases_chain(out_grad_loss, BK, KSL), with (BK, KSL) read from the launch.

Seven shapes (tests/bconv_fb_ref.SHAPES), each under the planner's plan and under forced plans: one slice at four K step depths (filters also bit-equal to
be=cpu), 40 and 98 slices on a K of 50 .. 150 (mostly empty slices), K < BK, 1 x 4 and 2 x 2 wave layouts, one and 2 x 2 blocks per wave.  Also: the same (BK, KSL)
under two tile shapes, NaN-poisoned outputs, the slab workspace reused on other data, a captured graph replayed on new data, the devices=... refusal, and the three
small pipes of tests/test_bck_pipe_cpu.py with the option on.  Every result is also within FILTS_MRD of float64."""
import numpy as np
import pytest

import bconv_fb_ref as fb
from boda_amd import rtc as rtc_mod
from boda_amd.bck_pipe import ConvPipeBck, add_bck_ops
from boda_amd.cnn_op import NATIVE_ARGS, OpTune, add_bck_conv_annotations, bconv_filts_biases_func_op
from boda_amd.op import RtErr, UnsupErr
from boda_amd.ops_prof import OpsBackend, profile_rcg_call
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc

from oracle import bck_chain as bc

from test_bck_conv_cpu import FILTS_MRD, mrd, rand_ins, run_func, torch_grads
from test_bck_pipe_cpu import PIPES, SEED_A, check_against_f64, grad_nodes, small_inputs, small_params

pytestmark = pytest.mark.gpu

FN = "hip_bconv_filts_biases"
ONE_SLICE = ["64x64x8x2x2x1x1", "64x64x16x2x2x1x1", "128x128x32x2x2x1x1", "128x128x64x2x2x1x1"]
MANY = ["32x128x32x1x4x1x40", "64x64x32x2x2x1x98"]          # K of 50 .. 150: 2 .. 5 K steps, so most slices are empty; 1 x 4 and 2 x 2 waves
SLICED = ["64x64x128x2x2x1x2", "128x128x32x2x2x2x3", "64x64x16x2x2x2x7"]   # K < BK on the short shapes; 2 x 2 blocks per wave; a K step of 16


@pytest.fixture(scope="module")
def hip():
    r = make_rtc("(be=hip)", 0)
    r.init()
    yield OpsBackend(r)
    r.close()


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def where_differs(got, want):
    d = np.argwhere(bits(got) != bits(want))
    if not len(d):
        return "equal"
    i = tuple(int(v) for v in d[0])
    return f"{len(d)} of {got.size} elements differ; first at {i}: got {got[i]!r} want {want[i]!r}; max|diff| {float(np.max(np.abs(got.astype(np.float64) - want))):.3g}"


def forced(tile):
    v = [int(x) for x in tile.split("x")]
    assert len(v) == 7
    return v[2], v[6]


def func(op, tile=""):
    return bconv_filts_biases_func_op(op, OpTune(hip_tile=tile))


def launch(be, op, tile="", vi=0.0, runs=1):
    """One call on device-generated mode-5 inputs -> (arrays, (BK, KSL) as launched, the launch).  A forced tile must be the tile that ran."""
    o, prc = profile_rcg_call(be, func(op, tile), 5, vi, runs, include_ins=True)
    plan = fb.plan_of(prc.launch)
    if tile:
        v = [int(x) for x in tile.split("x")]
        assert plan == forced(tile) and prc.launch["cfg"].startswith(f"{v[0]}x{v[1]}x{v[2]}_w{v[3]}x{v[4]}"), (tile, prc.launch)
    return o, plan, prc.launch


_F64 = {}


def check(be, name, tile="", vi=0.0, runs=1, operands=None):
    """One launch against its own emulation and float64 -> (arrays, (BK, KSL), (I, J))."""
    op = fb.shape_op(name)
    o, (bk, ksl), lch = launch(be, op, tile, vi, runs)
    I, J = operands or bc.filts_operands(o["in"], o["out_grad_loss"], op.bck_conv_geom())
    want_f = bc.filts_sliced_chain(I, J, bk, ksl, o["filts_grad_loss"].shape)
    want_b = fb.biases_chain(o["out_grad_loss"], bk, ksl)
    assert same_bits(o["filts_grad_loss"], want_f), (name, tile or "planner", lch, where_differs(o["filts_grad_loss"], want_f))
    assert same_bits(o["biases_grad_loss"].reshape(-1), want_b), (name, tile or "planner", lch, where_differs(o["biases_grad_loss"].reshape(-1), want_b))
    if (name, vi) not in _F64:
        _F64[(name, vi)] = torch_grads(op, o["in"], np.zeros(op.get_dims("filts").sizes, np.float32), o["out_grad_loss"])[1:]
    w64, b64 = _F64[(name, vi)]
    ef, eb = mrd(o["filts_grad_loss"], w64), mrd(o["biases_grad_loss"].reshape(-1), b64)
    print(f"{name} {tile or 'planner'} {lch['cfg']} grid {lch['grid']}: vs float64 filts {ef:.2e} bias {eb:.2e}")
    assert ef <= FILTS_MRD and eb <= FILTS_MRD, (name, tile, ef, eb)
    return o, (bk, ksl), (I, J)


# ---- every shape: the planner's plan and the forced plans
@pytest.mark.parametrize("name", sorted(fb.SHAPES))
def test_planner_and_forced_plans_equal_their_chains(hip, cpu, name):
    op = fb.shape_op(name)
    K = op.bck_conv_geom()["B"] * op.bck_conv_geom()["OH"] * op.bck_conv_geom()["OW"]
    o, (bk, ksl), operands = check(hip, name)
    plan = rtc_mod.explain_plan(func(op), num_cus=hip.rtc.get_device_info()["num_cus"])
    assert f"ksl={ksl} " in plan + " " and ("bodahip_bconv_slab_sum" in plan) == (ksl > 1), plan
    if name == "k1_long_k":
        assert ksl > 1      # K = 3136 on one tile: the planner slices it
    want_cpu = run_func(cpu, add_bck_conv_annotations(op, OpTune())[2], o)   # (mode-5 inputs: the same for every tile)
    for tile in ONE_SLICE:
        o1, plan1, _ = check(hip, name, tile, operands=operands)
        assert plan1[1] == 1 and "slab_sum" not in rtc_mod.explain_plan(func(op, tile))     # one slice: the outputs are written directly, no second launch
        assert same_bits(o1["filts_grad_loss"], want_cpu), (tile, where_differs(o1["filts_grad_loss"], want_cpu))   # the single chain: be=cpu's bits
    for tile in SLICED + (MANY if 50 <= K <= 150 else []):
        check(hip, name, tile, operands=operands)
    if K < 128:
        assert bc.filts_slices(K, 128, 2) == [(0, K), (K, K)]                         # "64x64x128...x2": K < BK, the second slice empty
    if K <= 150:
        assert sum(1 for k0, k1 in bc.filts_slices(K, 32, 98) if k0 == k1) >= 93      # 98 slices over at most five K steps


def test_same_bk_and_ksl_under_two_tile_shapes_gives_the_same_bits(hip):
    for name in ("k1_ohw49_tail", "k3_borders"):
        a, pa, ops_ = check(hip, name, "32x128x32x1x4x1x40")
        b, pb, _ = check(hip, name, "64x64x32x2x2x1x40", operands=ops_)
        assert pa == pb == (32, 40)
        assert same_bits(a["filts_grad_loss"], b["filts_grad_loss"]) and same_bits(a["biases_grad_loss"], b["biases_grad_loss"])
    a, _, ops_ = check(hip, "k1_long_k", "32x128x32x1x4x1x12")
    b, _, _ = check(hip, "k1_long_k", "64x64x32x2x2x2x12", operands=ops_)
    c, _, _ = check(hip, "k1_long_k", "64x64x16x2x2x2x12", operands=ops_)            # another K step depth: other slices of the bias residues
    assert same_bits(a["filts_grad_loss"], b["filts_grad_loss"]) and same_bits(a["biases_grad_loss"], b["biases_grad_loss"])
    assert not same_bits(a["biases_grad_loss"], c["biases_grad_loss"])


# ---- call sequences profile_rcg_call does not express
class FbCall:
    """The function compiled on be=hip over vars of its own ('<arg>_<tag>')."""
    ARGS = ("in", "out_grad_loss", "filts_grad_loss", "biases_grad_loss")

    def __init__(self, be, op, tile, tag):
        self.rtc, self.op, self.tag = be.rtc, op, tag
        f = func(op, tile)
        self.vars = []
        for an in self.ARGS:
            self.rtc.create_var_with_dims(f"{an}_{tag}", op.get_dims(an)); self.vars.append(f"{an}_{tag}")
        self.name = f"{FN}__{tag}"
        self.rtc.compile([RtcFuncInfo(self.name, f"CUCL_GLOBAL_KERNEL void {self.name}( void ) {{ }}\n", [a for a, _ in NATIVE_ARGS[FN]], f)], be.compile_opts)
        self.call = RtcFuncCall(self.name, {an: (RtcArg.ref(f.get_dims(an)) if io == "REF" else RtcArg.var(f"{an}_{tag}")) for an, io in NATIVE_ARGS[FN]})

    def set_ins(self, ins):
        for an in ("in", "out_grad_loss"):
            self.rtc.copy_nda_to_var(f"{an}_{self.tag}", ins[an])

    def poison_outs(self):
        for an in ("filts_grad_loss", "biases_grad_loss"):
            self.rtc.copy_nda_to_var(f"{an}_{self.tag}", np.full(self.op.get_dims(an).sizes, np.nan, np.float32))

    def check_outs(self, ins, bk, ksl, what):
        self.rtc.finish_and_sync()
        want = {"filts_grad_loss": bc.filts_chain(ins["in"], ins["out_grad_loss"], self.op.bck_conv_geom(), bk, ksl),
                "biases_grad_loss": fb.biases_chain(ins["out_grad_loss"], bk, ksl)}
        for an, w in want.items():
            got = self.rtc.copy_var_to_nda(f"{an}_{self.tag}").reshape(w.shape)
            assert same_bits(got, w), (what, an, where_differs(got, w))

    def release(self):
        self.rtc.finish_and_sync()
        for v in self.vars:
            self.rtc.release_var(v)
        self.rtc.release_func(self.name)
        self.rtc.release_per_call_id_data()


@pytest.mark.parametrize("tile", ["64x64x32x2x2x1x1", "64x64x32x2x2x1x5", "32x128x32x1x4x1x40"])
def test_nan_poisoned_outputs_are_fully_overwritten_and_the_workspace_serves_other_data(hip, tile):
    """Ragged tiles both ways (OC = 70, C = 130 at 64 x 64 and 32 x 128 tiles).  Outputs filled with NaN before every call: every element is written, by the main
    kernel (one slice) or by the slab sum.  Three calls on three data sets through the same vars, so the same slab workspace: no slab of an earlier call is read."""
    op = fb.shape_op("k1_many_tiles")
    bk, ksl = forced(tile)
    c = FbCall(hip, op, tile, "p")
    try:
        for seed in (21, 22, 23):
            ins = rand_ins(op, seed)
            c.set_ins(ins); c.poison_outs()
            hip.rtc.run(c.call)
            assert fb.plan_of(hip.rtc.last_launch()) == (bk, ksl)
            c.check_outs(ins, bk, ksl, f"seed {seed}")
    finally:
        c.release()


def test_graph_capture_needs_one_plain_run_then_replays_on_new_data(hip):
    rtc = hip.rtc
    op = fb.shape_op("k3_borders")
    tile = "64x64x16x2x2x2x3"
    bk, ksl = forced(tile)
    warm, cold = FbCall(hip, op, tile, "warm"), FbCall(hip, op, tile, "cold")
    try:
        ins = rand_ins(op, 31)
        warm.set_ins(ins); cold.set_ins(ins)
        rtc.run(warm.call)                       # both kernels are compiled and loaded; warm's workspace exists, cold's does not
        warm.check_outs(ins, bk, ksl, "plain run")
        rtc.graph_begin()
        with pytest.raises(RtErr, match="workspace"):
            rtc.run(cold.call)
        with pytest.raises(RtErr):               # the refused call ended the capture
            rtc.graph_end()
        rtc.finish_and_sync()
        rtc.run(cold.call)
        cold.check_outs(ins, bk, ksl, "first plain run")
        rtc.graph_begin()
        rtc.run(cold.call)
        gid, n = rtc.graph_end()
        assert n == 1
        try:
            for r in range(3):
                ins = rand_ins(op, 40 + r)
                cold.set_ins(ins); cold.poison_outs()
                rtc.graph_launch(gid)
                cold.check_outs(ins, bk, ksl, f"replay {r}")
        finally:
            rtc.graph_destroy(gid)
    finally:
        warm.release(); cold.release()


# ---- several devices
def test_two_shards_refuse_it_by_name():
    multi = make_rtc("(be=hip,devices=0:0)"); multi.init()
    try:
        op = fb.shape_op("k3_borders")
        with pytest.raises(UnsupErr, match="hip_bconv_filts_biases"):
            profile_rcg_call(OpsBackend(multi), func(op), 5)
        mk, tops, seed = PIPES["chain"]
        cp = mk(); bp = add_bck_ops(cp, loss_tops=tops)
        drv = ConvPipeBck(multi, fuse_filts_biases=True)
        with pytest.raises(UnsupErr, match="fuse_filts_biases"):
            drv.init(bp, small_params(cp, seed))
        assert drv.vars == [] and drv.funcs == []      # refused before anything was created
    finally:
        multi.close()


# ---- the pipe
def step(rtc, name, extra=(), **kw):
    mk, tops, seed = PIPES[name]
    cp = mk(); bp = add_bck_ops(cp, loss_tops=tops)
    data, label = small_inputs(cp, seed)
    drv = ConvPipeBck(rtc, **kw); drv.init(bp, small_params(cp, seed))
    drv.set_det_drop_seed(SEED_A)
    fwd = {"data": data, "label": label}
    drv.run_bck(["data", "label"], fwd, grad_nodes(bp) + bp.loss_nodes + list(extra))
    return drv, bp, fwd


@pytest.mark.parametrize("name", sorted(PIPES))
def test_pipe_with_the_option_on(hip, name):
    rtc = hip.rtc
    off, bp, fwd_off = step(rtc, name)
    off.release()
    fwd_nodes = [n for n in bp.nodes if not n.endswith("_grad_loss") and n not in bp.loss_nodes and n not in ("data", "label") and n not in bp.cp.params]
    on, bp, fwd = step(rtc, name, extra=fwd_nodes, fuse_filts_biases=True)
    try:
        fused = [c for c in on.bck_calls if c.fop.get_func_name() == FN]
        assert len(fused) == sum(1 for o in bp.bck_ops() if o.type == "BckConv") >= 2
        assert not any(c.fop.get_func_name() in ("hip_bconv_filts", "hip_bconv_biases") for c in on.bck_calls)
        written = {c.args[a] for c in fused for a in ("filts_grad_loss", "biases_grad_loss")}
        for n in grad_nodes(bp) + bp.loss_nodes:
            if n not in written:
                assert same_bits(fwd[n], fwd_off[n]), (n, where_differs(fwd[n], fwd_off[n]))
        vals = fwd   # (data and label as set, every fetched node)
        for c in fused:   # each call against the emulation of ITS launch: the call alone once more, on what the step left in its inputs
            rtc.run(c.rfc)
            bk, ksl = fb.plan_of(rtc.last_launch())
            rtc.finish_and_sync()
            x, g = vals[c.args["in"]], vals[c.args["out_grad_loss"]]
            want_f = bc.filts_chain(x, g, c.fop.bck_conv_geom(), bk, ksl)
            want_b = fb.biases_chain(g, bk, ksl)
            for got in (fwd[c.args["filts_grad_loss"]], rtc.copy_var_to_nda(c.args["filts_grad_loss"])):
                assert same_bits(got, want_f), (c.tag, where_differs(got, want_f))
            for got in (fwd[c.args["biases_grad_loss"]], rtc.copy_var_to_nda(c.args["biases_grad_loss"])):
                assert same_bits(got.reshape(-1), want_b), (c.tag, where_differs(got.reshape(-1), want_b))
        check_against_f64(name, on, bp, fwd, "be=hip fused")
    finally:
        on.release()
