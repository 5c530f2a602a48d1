"""BckConv on the MI355X, held to its exact chains: every comparison in this file is np.array_equal on the fp32 bit patterns.

  * one K slice (KSL = 1), any K step: bodahip_bconv_filts equals be=cpu's hip_bconv_filts -- the reference template's loop
  * K slices: filts_grad_loss equals oracle/bck_chain.filts_sliced_chain(I, J, BK, KSL), the association written in kernels/bconv_filts_f32.hip (slab s = one
    chain over K steps [s * kt_per, (s + 1) * kt_per), the slabs added in slice order), with BK and KSL read from the launch and kt_per derived in the emulator
  * biases_grad_loss equals bck_chain.biases_chain, in_grad_loss equals bck_chain.in_grad_chain
on every recorded fixture shape with the planner's own plan, on forced slice plans at the edges (K < BK, K tails, empty slices, ragged tiles, strides, paddings),
with a reused slice workspace on different data, and replayed from a captured graph on new data.  The emulator itself is checked against be=cpu and float64 in
tests/test_bck_chain_cpu.py; the float64 bounds of the GPU gradients stay in tests/test_gpu_bck_conv.py."""
import numpy as np
import pytest

from boda_amd import rtc as rtc_mod
from boda_amd.cnn_op import NATIVE_ARGS, OpTune, add_bck_conv_annotations
from boda_amd.op import RtErr, read_ops
from boda_amd.ops_prof import OpsBackend, profile_rcg_call
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc

from oracle import bck_chain as bc

from test_bck_conv_cpu import GOLD, bck_op, rand_ins
from test_gpu_bck_conv import EDGE

pytestmark = pytest.mark.gpu


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
    """What a failing comparison prints: how many elements differ, the first of them, the largest difference."""
    d = np.argwhere(bits(got) != bits(want))
    if not len(d):
        return "equal"
    i = tuple(int(v) for v in d[0])
    return f"{len(d)} of {got.size} elements differ; first at {i}: got {got[i]!r} want {want[i]!r}; max|diff| {float(np.max(np.abs(got.astype(np.float64) - want))):.3g}"


def plan_of(launch):
    """(BK, KSL) of a bodahip_bconv_filts launch, from its configuration string BIxBJxBK_wWIxWJ[_sKSL]."""
    assert launch["kernel"] == "bodahip_bconv_filts", launch
    cfg = launch["cfg"]
    return int(cfg.split("_")[0].split("x")[2]), (int(cfg.split("_s")[1].split("_")[0]) if "_s" in cfg else 1)


def forced(tile):
    """(BK, KSL) a seven-field tile string BIxBJxBKxWIxWJxMINWxKSL asks for."""
    v = [int(x) for x in tile.split("x")]
    assert len(v) == 7
    return v[2], v[6]


def filts_func(op, ftile=""):
    _, _, ff = add_bck_conv_annotations(op, OpTune())
    if ftile:
        ff.str_vals["hip_tile"] = ftile
    return ff


def gpu_filts(be, op, ftile="", vi=0.0, runs=1):
    """hip_bconv_filts on device-generated mode-5 inputs -> ({in, out_grad_loss, filts_grad_loss}, (BK, KSL) as launched).  A forced tile must be what ran."""
    o, prc = profile_rcg_call(be, filts_func(op, ftile), 5, vi, runs, include_ins=True)
    plan = plan_of(prc.launch)
    if ftile:
        assert plan == forced(ftile), (ftile, prc.launch)
    return o, plan


def check_filts_chain(be, op, ftile="", vi=0.0, runs=1, operands=None):
    """One launch against its own emulation.  -> (filts_grad_loss, (BK, KSL), (I, J))."""
    o, (bk, ksl) = gpu_filts(be, op, ftile, vi, runs)
    I, J = operands or bc.filts_operands(o["in"], o["out_grad_loss"], op.bck_conv_geom())
    want = bc.filts_sliced_chain(I, J, bk, ksl, o["filts_grad_loss"].shape)
    assert same_bits(o["filts_grad_loss"], want), (ftile or "planner", (bk, ksl), op.to_str(), where_differs(o["filts_grad_loss"], want))
    return o["filts_grad_loss"], (bk, ksl), (I, J)


# ---- one slice: the GPU equals be=cpu's loop, for every K step
ONE_SLICE_TILES = ["64x64x8x2x2x1x1", "64x64x16x2x2x1x1", "128x128x32x2x2x1x1", "128x128x64x2x2x1x1"]


def check_one_slice_equals_cpu(hip, cpu, op):
    from test_bck_conv_cpu import run_func
    want = None
    for tile in ONE_SLICE_TILES:
        o, plan = gpu_filts(hip, op, tile)
        assert plan[1] == 1
        if want is None:   # (mode-5 inputs: the same for every tile)
            want = run_func(cpu, filts_func(op), o)
        assert same_bits(o["filts_grad_loss"], want), (tile, op.to_str(), where_differs(o["filts_grad_loss"], want))


@pytest.mark.parametrize("name", sorted(EDGE))
def test_one_slice_equals_cpu_bits_edge_geometries(hip, cpu, name):
    check_one_slice_equals_cpu(hip, cpu, bck_op(*EDGE[name]))


def test_one_slice_equals_cpu_bits_fixture_spread(hip, cpu):
    """Every tenth recorded op plus the longest K (5 x 57 x 57 = 16 245 terms per chain) and the shortest (K = 1)."""
    ops = read_ops(GOLD)
    ks = [o.bck_conv_geom()["B"] * o.bck_conv_geom()["OH"] * o.bck_conv_geom()["OW"] for o in ops]
    pick = sorted(set(range(0, len(ops), 10)) | {int(np.argmax(ks)), int(np.argmin(ks))})
    assert len(pick) >= 10
    for i in pick:
        check_one_slice_equals_cpu(hip, cpu, ops[i])


# ---- the planner's own plan, every recorded shape
def test_planner_default_every_fixture_shape_equals_chain(hip):
    ops = read_ops(GOLD)
    assert len(ops) >= 90
    bad, sliced = [], 0
    for op in ops:
        _, fb, ff = add_bck_conv_annotations(op, OpTune())
        o, prc = profile_rcg_call(hip, ff, 5, include_ins=True)
        bk, ksl = plan_of(prc.launch)
        assert f"ksl={ksl} " in rtc_mod.explain_plan(ff, num_cus=hip.rtc.get_device_info()["num_cus"]) + " ", (prc.launch, rtc_mod.explain_plan(ff))
        sliced += ksl > 1
        want = bc.filts_chain(o["in"], o["out_grad_loss"], op.bck_conv_geom(), bk, ksl)
        if not same_bits(o["filts_grad_loss"], want):
            bad.append(("filts", prc.launch["cfg"], op.to_str(), where_differs(o["filts_grad_loss"], want)))
        ob, prc = profile_rcg_call(hip, fb, 5, include_ins=True)
        assert prc.launch["kernel"] == "bodahip_bconv_biases" and np.array_equal(ob["out_grad_loss"], o["out_grad_loss"])
        want = bc.biases_chain(ob["out_grad_loss"])
        if not same_bits(ob["biases_grad_loss"], want):
            bad.append(("biases", op.to_str(), where_differs(ob["biases_grad_loss"], want)))
    assert not bad, (len(bad), bad[:6])
    assert sliced > len(ops) // 4   # the sweep is about the slices: most recorded shapes have few tiles and a long K


# ---- forced slice plans at the edges
def test_forced_k_smaller_than_bk_empty_slices(hip):
    """K = 9 < BK = 32: one K step, slice 0 holds it, slices 1..3 are empty (kt0 == kt1) and contribute +0."""
    op = bck_op(1, 3, 5, 5, 4, 3, 3, 1, 1, 0, 0)
    assert bc.filts_slices(9, 32, 4) == [(0, 9), (9, 9), (9, 9), (9, 9)]
    check_filts_chain(hip, op, "32x64x32x1x2x1x4")


def test_forced_k_tail_three_slices(hip):
    """K = 338 = 10 * 32 + 18, three slices of four K steps: the last slice ends in the K tail."""
    op = bck_op(2, 5, 13, 13, 7, 3, 3, 1, 1, 1, 1)
    assert bc.filts_slices(338, 32, 3)[-1] == (256, 338)
    check_filts_chain(hip, op, "32x64x32x1x2x1x3")


def test_forced_32_slices_of_33_k_steps_trailing_empty_slices(hip):
    """K = 2 * 21 * 25 = 1050: nkt = 33, KSL = 32 -> kt_per = 2: slice 16 holds the last (partial) K step, slices 17..31 are empty."""
    op = bck_op(2, 6, 21, 25, 20, 3, 3, 1, 1, 1, 1)
    sl = bc.filts_slices(1050, 32, 32)
    assert sl[16] == (1024, 1050) and sl[17] == sl[31] == (1050, 1050)
    check_filts_chain(hip, op, "32x64x32x1x2x1x32")


@pytest.mark.parametrize("oc", [33, 70, 130])
@pytest.mark.parametrize("tile", ["32x64x32x1x2x1x2", "64x64x16x2x2x1x3", "64x128x32x2x2x1x4"])
def test_forced_ragged_out_chans_and_columns_several_tile_rows_and_columns(hip, oc, tile):
    """OC = 33 / 70 / 130 against BI = 32 / 64 and C*KH*KW = 15 * 9 = 135 against BJ = 64 / 128: a ragged last tile row and column, and up to 5 x 3 tiles, so
    that a wrong tile_id -> (tile_i, tile_j) map, a wrong slab base or a tile's ticket taken by another tile shows."""
    check_filts_chain(hip, bck_op(2, 15, 9, 9, oc, 3, 3, 1, 1, 1, 1), tile)


@pytest.mark.parametrize("name", sorted(EDGE))
def test_forced_slices_edge_geometries(hip, name):
    """B = 1, strides 2 .. 4 (also larger than the kernel), pad >= stride, KH != KW, SY != SX: sliced, at both K steps."""
    op = bck_op(*EDGE[name])
    operands = None
    for tile in ("32x64x32x1x2x1x2", "64x64x16x2x2x1x3", "64x128x32x2x2x1x5"):
        _, _, operands = check_filts_chain(hip, op, tile, operands=operands)


def test_forced_same_slice_count_at_bk16_and_bk32(hip):
    """The same KSL at BK = 16 and BK = 32: each launch equals ITS OWN emulation.  The two agree only where kt_per * BK coincides: K = 338 -> three slices of 128
    either way, the same bits; K = 300 -> slices of 112 (BK = 16: nkt = 19, kt_per = 7) against 128 (BK = 32: nkt = 10, kt_per = 4), different bits."""
    same = bck_op(2, 5, 13, 13, 7, 3, 3, 1, 1, 1, 1)
    assert bc.filts_slices(338, 16, 3) == bc.filts_slices(338, 32, 3)
    a, _, ops_ = check_filts_chain(hip, same, "64x64x16x2x2x1x3")
    b, _, _ = check_filts_chain(hip, same, "64x64x32x2x2x1x3", operands=ops_)
    assert same_bits(a, b)
    other = bck_op(3, 5, 10, 10, 7, 3, 3, 1, 1, 1, 1)
    assert bc.filts_slices(300, 16, 3) != bc.filts_slices(300, 32, 3)
    a, _, ops_ = check_filts_chain(hip, other, "64x64x16x2x2x1x3")
    b, _, _ = check_filts_chain(hip, other, "64x64x32x2x2x1x3", operands=ops_)
    assert not same_bits(a, b)


# ---- the slice workspace, reused
def test_workspace_reuse_with_different_data_and_geometry(hip):
    """The same sliced call on other data (gen_data's `vi`; the vars are freed and re-created at the same addresses, so the call finds its workspace again), three
    launches in a row, then a DIFFERENT geometry with the same tensor sizes, tile count and tile (H and W exchanged: its workspace key can coincide): a stale slab,
    a ticket left non-zero or a slab read before it is complete would show, because no run's data equals the previous run's."""
    tile = "32x64x32x1x2x1x3"
    a, b = bck_op(2, 15, 13, 11, 70, 3, 3, 1, 1, 1, 1), bck_op(2, 15, 11, 13, 70, 3, 3, 1, 1, 1, 1)
    f0, _, _ = check_filts_chain(hip, a, tile, vi=0.0)
    f1, _, _ = check_filts_chain(hip, a, tile, vi=0.375, runs=3)
    assert not same_bits(f0, f1)
    f2, _, _ = check_filts_chain(hip, b, tile, vi=0.375)
    assert not same_bits(f1, f2)
    check_filts_chain(hip, a, tile, vi=0.0)


# ---- graph capture and replay
class BckCalls:
    """The three gradient functions of one op compiled on be=hip over vars of their own ('<arg>_<tag>'), for call sequences profile_rcg_call does not express."""
    ARGS = ("in", "filts", "out_grad_loss", "in_grad_loss", "filts_grad_loss", "biases_grad_loss")

    def __init__(self, be, op, ftile, tag):
        self.rtc, self.op, self.tag = be.rtc, op, tag
        self.funcs, self.vars, self.calls = [], [], []
        fi, fb, ff = add_bck_conv_annotations(op, OpTune())
        ff.str_vals["hip_tile"] = ftile
        for an in self.ARGS:
            self.rtc.create_var_with_dims(f"{an}_{tag}", op.get_dims(an)); self.vars.append(f"{an}_{tag}")
        for f in (fi, fb, ff):
            fn = f.get_func_name()
            name = f"{fn}__{tag}"
            self.rtc.compile([RtcFuncInfo(name, f"CUCL_GLOBAL_KERNEL void {name}( void ) {{ }}\n", [a for a, _ in NATIVE_ARGS[fn]], f)], be.compile_opts)
            self.funcs.append(name)
            am = {an: (RtcArg.ref(f.get_dims(an)) if io == "REF" else RtcArg.var(f"{an}_{tag}")) for an, io in NATIVE_ARGS[fn]}
            self.calls.append(RtcFuncCall(name, am))

    def set_ins(self, ins):
        for an in ("in", "filts", "out_grad_loss"):
            self.rtc.copy_nda_to_var(f"{an}_{self.tag}", ins[an])

    def zero_outs(self):
        for an in ("in_grad_loss", "filts_grad_loss", "biases_grad_loss"):
            self.rtc.set_var_to_zero(f"{an}_{self.tag}")

    def check_outs(self, ins, bk, ksl, what):
        self.rtc.finish_and_sync()
        geom = self.op.bck_conv_geom()
        want = {"filts_grad_loss": bc.filts_chain(ins["in"], ins["out_grad_loss"], geom, bk, ksl), "biases_grad_loss": bc.biases_chain(ins["out_grad_loss"]),
                "in_grad_loss": bc.in_grad_chain(ins["filts"], ins["out_grad_loss"], geom)}
        for an, w in want.items():
            got = self.rtc.copy_var_to_nda(f"{an}_{self.tag}")
            assert same_bits(got, w), (what, an, where_differs(got, w))

    def release(self):
        self.rtc.finish_and_sync()
        for v in self.vars:
            self.rtc.release_var(v)
        for f in self.funcs:
            self.rtc.release_func(f)
        self.rtc.release_per_call_id_data()


def test_graph_capture_before_first_run_is_refused_then_replay_on_new_data(hip):
    """A sliced hip_bconv_filts whose workspace does not exist yet cannot be captured: RtErr from the host, no launch.  After one plain run the three gradient
    calls are captured once and replayed three times, new inputs copied in and the outputs zeroed between the replays: every replay equals the emulation of ITS
    data (the tickets are left at zero by each launch, no slab of an earlier replay is read)."""
    rtc = hip.rtc
    op = bck_op(2, 15, 13, 11, 70, 3, 3, 2, 1, 1, 1)
    tile = "32x64x32x1x2x1x3"
    bk, ksl = forced(tile)
    warm = BckCalls(hip, op, tile, "warm")     # the same specialisation on other vars: the kernel is compiled and loaded, this call's workspace exists
    cold = BckCalls(hip, op, tile, "cold")     # never run: no workspace under its pointers
    try:
        ins = rand_ins(op, 11)
        warm.set_ins(ins); cold.set_ins(ins)
        for c in warm.calls:
            rtc.run(c)
        assert plan_of(rtc.last_launch()) == (bk, ksl)
        warm.check_outs(ins, bk, ksl, "plain run")
        rtc.graph_begin()
        with pytest.raises(RtErr, match="workspace"):
            rtc.run(cold.calls[2])
        with pytest.raises(RtErr):             # the refused call ended the capture
            rtc.graph_end()
        rtc.finish_and_sync()

        for c in cold.calls:                   # one plain run, then the capture
            rtc.run(c)
        cold.check_outs(ins, bk, ksl, "first plain run")
        rtc.graph_begin()
        for c in cold.calls:
            rtc.run(c)
        gid, n = rtc.graph_end()
        assert n == 3
        try:
            for r in range(3):
                ins = rand_ins(op, 100 + r)
                cold.set_ins(ins); cold.zero_outs()
                rtc.graph_launch(gid)
                cold.check_outs(ins, bk, ksl, f"replay {r}")
        finally:
            rtc.graph_destroy(gid)
    finally:
        warm.release(); cold.release()


# ---- several devices
def test_multi_device_data_gradient_equals_chain(hip):
    """hip_bconv_in over devices=0:0 (the images split between two backends on one GPU) on a strided shape: the bits of the single chain per output."""
    op = bck_op(4, 24, 11, 11, 40, 3, 3, 2, 2, 1, 1)
    r = make_rtc("(be=hip,devices=0:0)")
    r.init()
    try:
        fi, _, _ = add_bck_conv_annotations(op, OpTune())
        o, prc = profile_rcg_call(OpsBackend(r), fi, 5, include_ins=True)
        want = bc.in_grad_chain(o["filts"], o["out_grad_loss"], op.bck_conv_geom())
        assert same_bits(o["in_grad_loss"], want), where_differs(o["in_grad_loss"], want)
    finally:
        r.close()
    fi, _, _ = add_bck_conv_annotations(op, OpTune())
    o1, _ = profile_rcg_call(hip, fi, 5, include_ins=True)
    assert same_bits(o1["in_grad_loss"], want)
