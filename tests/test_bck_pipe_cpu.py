"""The full-net gradient pipe without a GPU: add_bck_ops' graph reversal (names, bots / tops and order, on three hand-built pipes and on the real nets), the four plumbing
functions on be=cpu bit for bit against tests/bck_pipe_ref.py, their refusals, and ConvPipeBck on be=cpu against a float64 backprop.

The float64 comparison uses max|got - want| / max|want| per node under the cap 5e-4, the reference's own bar for its gradient pipes (mrd_toler, src/test_compute.cc:45).
The measured values are printed (run with -s); they sit orders of magnitude below the cap.  Because such a cap would pass a flipped ReLU or pooling argmax, the float64
helper refuses data on which a flip is possible (bck_pipe_ref.net_f64); the seeds below are ones for which it does not."""
import numpy as np
import pytest

import bck_pipe_ref as ref
from boda_amd import rtc as rtc_mod
from boda_amd.bck_pipe import ConvPipeBck, add_bck_ops, grad_op_to_op
from boda_amd.cnn_op import NATIVE_ARGS, OpTune, PIPE_OP_FUNCS, add_pipe_op_annotations, pipe_func_args
from boda_amd.conv_pipe import ConvPipe, PipeOp, _conv, alexnet_ng_conv, googlenet_conv, nin_imagenet
from boda_amd.op import Dims, RtErr, UnsupErr, parse_op
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc

CAP = 5e-4
N_CLASS = 5


# ---- the three small pipes
def chain(B=2):
    """conv 3x3 / 2 + ReLU -> LRN(3) -> max pool 3 / 2 (a clipped last window) -> Dropout -> conv over the whole map -> loss"""
    p = ConvPipe("chain", "data", Dims.make("float", img=B, chan=3, y=13, x=13))
    _conv(p, "conv1", "data", 8, 3, 2)
    p.add(PipeOp("norm1", "LRN", "conv1", "norm1", lrn=(3, 0.05, 0.75, 1.0)))
    p.add(PipeOp("pool1", "Pooling", "norm1", "pool1", kern_sz=(3, 3), stride=(2, 2)))
    p.add(PipeOp("drop1", "Dropout", "pool1", "pool1"))
    p.add(PipeOp("fc", "Convolution", "pool1", "fc", out_chans=N_CLASS, kern_sz=(0, 0)))
    return p


def fan(B=2):
    """stem conv + ReLU = X; X -> 1x1 conv + ReLU | 3x3 pad-1 conv + ReLU | max pool 3 / 1 pad 1 -> 1x1 conv; Concat (4 + 4 + 3) -> global average -> 1x1 conv -> loss"""
    p = ConvPipe("fan", "data", Dims.make("float", img=B, chan=3, y=7, x=7))
    _conv(p, "stem", "data", 6, 3, 1, 1)
    _conv(p, "a", "stem", 4, 1); _conv(p, "b", "stem", 4, 3, 1, 1)
    p.add(PipeOp("cp", "Pooling", "stem", "cp", kern_sz=(3, 3), stride=(1, 1), in_pad=(1, 1)))
    p.add(PipeOp("c", "Convolution", "cp", "c", out_chans=3, kern_sz=(1, 1)))
    p.add(PipeOp("cat", "Concat", "a", "cat", bots=("a", "b", "c")))
    p.add(PipeOp("gap", "Pooling", "cat", "gap", kern_sz=None, avg_pool=1))
    p.add(PipeOp("fc", "Convolution", "gap", "fc", out_chans=N_CLASS, kern_sz=(1, 1)))
    return p


def heads(B=3):
    """conv + ReLU = X feeds the main path (conv -> max pool 2 / 2 -> conv over the map -> loss1) and an auxiliary head (conv over the map -> loss2); one label"""
    p = ConvPipe("heads", "data", Dims.make("float", img=B, chan=3, y=11, x=11))
    _conv(p, "conv1", "data", 8, 3, 2)
    p.add(PipeOp("mid", "Convolution", "conv1", "mid", out_chans=6, kern_sz=(2, 2)))
    p.add(PipeOp("pool1", "Pooling", "mid", "pool1", kern_sz=(2, 2), stride=(2, 2)))
    p.add(PipeOp("fc_main", "Convolution", "pool1", "fc_main", out_chans=N_CLASS, kern_sz=(0, 0)))
    p.add(PipeOp("fc_aux", "Convolution", "conv1", "fc_aux", out_chans=N_CLASS, kern_sz=(0, 0)))
    return p


HEADS_TOPS = ["fc_main", "fc_aux"]
PIPES = {"chain": (chain, None, 0), "fan": (fan, None, 0), "heads": (heads, HEADS_TOPS, 0)}   # name -> (builder, loss tops, data / param seed)
SEED_A, SEED_B = 1234, 99


def small_params(cp, seed):
    """He-scaled filters; biases lifted so that most (not all) ReLU inputs are positive: a max-pooling window of ReLU outputs then rarely holds two exact zeros on top."""
    rng = np.random.default_rng([seed, 7])
    out = {}
    for n, d in cp.params.items():
        if n.endswith("_filts"):
            out[n] = (rng.standard_normal(d.sizes) * np.sqrt(2.0 / (d.dsz("in_chan") * d.dsz("y") * d.dsz("x")))).astype(np.float32)
        else:
            out[n] = rng.uniform(0.6, 1.0, d.sizes).astype(np.float32)
    return out


def small_inputs(cp, seed):
    rng = np.random.default_rng([seed, 11])
    data = rng.uniform(-1, 1, cp.nodes["data"].sizes).astype(np.float32)
    label = rng.integers(0, N_CLASS, (data.shape[0], 1, 1)).astype(np.float32)
    return data, label


def drop_seeds(drv):
    return {t: int(am["det_drop_seed"].v[0]) for t, f, am in drv.calls() if f.get_func_name() == "hip_dropout" and not t.endswith("_bck")}


def grad_nodes(bp):
    return [n for n in bp.nodes if n.endswith("_grad_loss")]


def run_pipe(rtc, name, drop_seed=SEED_A):
    """One step of a small pipe on `rtc` -> (driver, BckPipe, params, data, label, {node: array} of every gradient node and loss)."""
    mk, tops, seed = PIPES[name]
    cp = mk(); bp = add_bck_ops(cp, loss_tops=tops)
    params = small_params(cp, seed); data, label = small_inputs(cp, seed)
    drv = ConvPipeBck(rtc); drv.init(bp, params)
    drv.set_det_drop_seed(drop_seed)
    fwd = {"data": data, "label": label}
    drv.run_bck(["data", "label"], fwd, grad_nodes(bp) + bp.loss_nodes)
    return drv, bp, params, data, label, fwd


_WANT = {}


def want_f64(name, drv):
    """The float64 backprop of a small pipe under SEED_A's masks, computed once."""
    if name not in _WANT:
        mk, tops, seed = PIPES[name]
        cp = mk(); data, label = small_inputs(cp, seed)
        _WANT[name] = ref.net_f64(cp, tops or [cp.out_node()], small_params(cp, seed), data, label, drop_seeds(drv))
    return _WANT[name]


def check_against_f64(name, drv, bp, fwd, where):
    want = want_f64(name, drv)
    checked = 0
    for n in grad_nodes(bp) + bp.loss_nodes:
        if "_split_" in n:   # a partial gradient: the float64 backprop accumulates, its sum is checked as <node>_grad_loss
            continue
        assert n in want, n
        got = fwd[n]
        assert got.shape == tuple(bp.nodes[n].sizes) and np.all(np.isfinite(got))
        if n in bp.loss_nodes:
            err = abs(got.item() - want[n]) / abs(want[n])
        else:
            err = ref.rel_err(got, want[n])
        print(f"{where} {name} {n}: {err:.3e}")
        assert err <= CAP, (n, err)
        checked += 1
    assert checked >= len(bp.cp.params) + 2


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


# ---- the graph reversal: names, bots / tops and order
def listing(bp):
    return [(o.tag, o.type, o.bots, o.tops) for o in bp.bck_ops()]


def test_reversal_chain():
    bp = add_bck_ops(chain())
    assert [(o.tag, o.type, o.bots, o.tops) for o in bp.fwd_ops()][-1] == ("loss", "SoftmaxWithLoss", ["fc", "label"], ["fc_grad_loss", "loss"])
    assert listing(bp) == [
        ("fc_bck", "BckConv", ["pool1", "fc_filts", "fc_biases", "fc_grad_loss"], ["pool1_grad_loss", "fc_filts_grad_loss", "fc_biases_grad_loss"]),
        ("drop1_bck", "BckDropout", ["pool1_grad_loss"], ["pool1_grad_loss"]),
        ("pool1_bck", "Spreading", ["pool1", "pool1_grad_loss", "norm1"], ["norm1_grad_loss"]),
        ("norm1_bck", "BckLRN", ["conv1", "norm1", "norm1_grad_loss"], ["conv1_grad_loss"]),
        ("relu_conv1_bck", "ZeroIfNonPos", ["conv1_grad_loss", "conv1"], ["conv1_grad_loss"]),
        ("conv1_bck", "BckConv", ["data", "conv1_filts", "conv1_biases", "conv1_grad_loss"], ["data_grad_loss", "conv1_filts_grad_loss", "conv1_biases_grad_loss"]),
    ]
    assert "label_grad_loss" not in bp.nodes and bp.nodes["data_grad_loss"] == bp.nodes["data"] and bp.loss_nodes == ["loss"]
    assert grad_op_to_op(bp, bp.fwd_ops()[3]).get_u32("emit_out_in_yx") == 1 and grad_op_to_op(bp, bp.fwd_ops()[2]).get_u32("emit_out_scale_base") == 1


def test_reversal_fan():
    bp = add_bck_ops(fan())
    sp = [f"stem_relu_stem_0_split_{i}_grad_loss" for i in range(3)]   # X_<last in-place op of X>_0_split_<index among X's readers>
    assert listing(bp) == [
        ("fc_bck", "BckConv", ["gap", "fc_filts", "fc_biases", "fc_grad_loss"], ["gap_grad_loss", "fc_filts_grad_loss", "fc_biases_grad_loss"]),
        ("gap_bck", "Spreading", ["gap", "gap_grad_loss", "cat"], ["cat_grad_loss"]),
        ("cat_bck", "Split", ["cat_grad_loss"], ["a_grad_loss", "b_grad_loss", "c_grad_loss"]),
        ("c_bck", "BckConv", ["cp", "c_filts", "c_biases", "c_grad_loss"], ["cp_grad_loss", "c_filts_grad_loss", "c_biases_grad_loss"]),
        ("cp_bck", "Spreading", ["cp", "cp_grad_loss", "stem"], [sp[2]]),
        ("relu_b_bck", "ZeroIfNonPos", ["b_grad_loss", "b"], ["b_grad_loss"]),
        ("b_bck", "BckConv", ["stem", "b_filts", "b_biases", "b_grad_loss"], [sp[1], "b_filts_grad_loss", "b_biases_grad_loss"]),
        ("relu_a_bck", "ZeroIfNonPos", ["a_grad_loss", "a"], ["a_grad_loss"]),
        ("a_bck", "BckConv", ["stem", "a_filts", "a_biases", "a_grad_loss"], [sp[0], "a_filts_grad_loss", "a_biases_grad_loss"]),
        ("reduce_stem_grad_loss", "Reduce", sp, ["stem_grad_loss"]),                       # after every partial gradient ...
        ("relu_stem_bck", "ZeroIfNonPos", ["stem_grad_loss", "stem"], ["stem_grad_loss"]),   # ... and before the in-place gradient op
        ("stem_bck", "BckConv", ["data", "stem_filts", "stem_biases", "stem_grad_loss"], ["data_grad_loss", "stem_filts_grad_loss", "stem_biases_grad_loss"]),
    ]
    assert sum(o.type == "Reduce" for o in bp.ops) == 1 and sum(o.type == "Split" for o in bp.ops) == 1
    assert grad_op_to_op(bp, [o for o in bp.ops if o.tag == "gap"][0]).get_u32("emit_out_in_yx") == 0   # an average has no argmax


def test_reversal_two_heads():
    bp = add_bck_ops(heads(), loss_tops=HEADS_TOPS)
    assert [(o.tag, o.bots, o.tops) for o in bp.fwd_ops()[-2:]] == [("loss1", ["fc_main", "label"], ["fc_main_grad_loss", "loss1"]), ("loss2", ["fc_aux", "label"], ["fc_aux_grad_loss", "loss2"])]
    sp = [f"conv1_relu_conv1_0_split_{i}_grad_loss" for i in range(2)]
    assert listing(bp) == [
        ("fc_main_bck", "BckConv", ["pool1", "fc_main_filts", "fc_main_biases", "fc_main_grad_loss"], ["pool1_grad_loss", "fc_main_filts_grad_loss", "fc_main_biases_grad_loss"]),
        ("pool1_bck", "Spreading", ["pool1", "pool1_grad_loss", "mid"], ["mid_grad_loss"]),
        ("mid_bck", "BckConv", ["conv1", "mid_filts", "mid_biases", "mid_grad_loss"], [sp[0], "mid_filts_grad_loss", "mid_biases_grad_loss"]),
        # (the walk starts from the sources in name order: fc_aux's params come before `label`, mid's after it, so fc_aux_bck is walked first and lands last)
        ("fc_aux_bck", "BckConv", ["conv1", "fc_aux_filts", "fc_aux_biases", "fc_aux_grad_loss"], [sp[1], "fc_aux_filts_grad_loss", "fc_aux_biases_grad_loss"]),
        ("reduce_conv1_grad_loss", "Reduce", sp, ["conv1_grad_loss"]),
        ("relu_conv1_bck", "ZeroIfNonPos", ["conv1_grad_loss", "conv1"], ["conv1_grad_loss"]),
        ("conv1_bck", "BckConv", ["data", "conv1_filts", "conv1_biases", "conv1_grad_loss"], ["data_grad_loss", "conv1_filts_grad_loss", "conv1_biases_grad_loss"]),
    ]
    assert not any("label" in t for o in bp.bck_ops() for t in o.tops) and "label_grad_loss" not in bp.nodes   # label's Reduce has no inputs: dropped
    assert bp.loss_nodes == ["loss1", "loss2"]


def test_reversal_refusals():
    p = chain()
    with pytest.raises(RtErr, match="no node"):
        add_bck_ops(p, loss_tops=["nope"])
    with pytest.raises(RtErr, match="not produced by SoftmaxWithLoss"):   # a second sink that no loss caps
        add_bck_ops(heads(), loss_tops=["fc_main"])
    with pytest.raises(RtErr, match="already has a node"):
        add_bck_ops(p, label_node="data")


GOOGLENET_TOPS = ["cls3_fc", "cls1_fc2", "cls2_fc2"]


@pytest.mark.parametrize("net", ["nin_imagenet", "alexnet_ng_conv", "googlenet_conv"])
def test_reversal_on_real_nets(net):
    cp = {"nin_imagenet": nin_imagenet, "alexnet_ng_conv": alexnet_ng_conv, "googlenet_conv": googlenet_conv}[net](2)
    tops = GOOGLENET_TOPS if net == "googlenet_conv" else None
    bp = add_bck_ops(cp, loss_tops=tops)
    n_of = lambda ops, t: sum(o.type == t for o in ops)
    for f, b in (("Convolution", "BckConv"), ("Pooling", "Spreading"), ("LRN", "BckLRN"), ("ReLU", "ZeroIfNonPos"), ("Dropout", "BckDropout"), ("Concat", "Split")):
        assert n_of(bp.bck_ops(), b) == n_of(cp.ops, f), (f, b)
    assert n_of(bp.fwd_ops(), "SoftmaxWithLoss") == len(tops or [1])
    readers = {}
    for o in bp.fwd_ops():
        if not o.in_place:
            for b in o.bots:
                readers[b] = readers.get(b, 0) + 1
    fan_outs = sorted(n for n, k in readers.items() if k > 1 and n != bp.label_node)
    assert sorted(o.tops[0][:-len("_grad_loss")] for o in bp.ops if o.type == "Reduce") == fan_outs
    assert bool(fan_outs) == (net == "googlenet_conv")
    for o in bp.ops:
        if o.type == "Reduce":
            assert len(o.bots) == readers[o.tops[0][:-len("_grad_loss")]] and 2 <= len(o.bots) <= 5   # (an inception output feeds four branches, and two of them an auxiliary head as well)
    written = {cp.in_node, bp.label_node} | set(cp.params)
    for o in bp.ops:   # every op's inputs are written earlier in the list
        for b in o.bots:
            assert b in written, (o.tag, b)
        written |= set(o.tops)
    for n, d in cp.params.items():
        assert bp.nodes[n + "_grad_loss"] == d
    assert bp.nodes["data_grad_loss"] == cp.nodes["data"]
    for o in bp.ops:   # every op has an op_base_t form that the op layer accepts
        assert parse_op(grad_op_to_op(bp, o).to_str()).to_str() == grad_op_to_op(bp, o).to_str()


# ---- the four functions on be=cpu
def _d(B, C, H, W):
    return f"(dims=(img={B},chan={C},y={H},x={W}))"


def reduce_op(n, dims="(dims=(v=1023))", ins_num=None):
    ins = ",".join(f"ins_{i}={dims}" for i in range(n))
    return parse_op(f"(str_vals=(type=Reduce),nda_vals=({ins},ins_num=(tn=uint32_t,v={n if ins_num is None else ins_num}),out={dims}))")


def dropout_op(ratio, dims="(dims=(img=2,chan=3,y=7,x=11))", typ="Dropout"):
    return parse_op(f"(str_vals=(type={typ}),nda_vals=(dropout_ratio=(tn=float,v={ratio!r}),in={dims},out={dims}))")


def concat_op(B, chans, H, W, typ="Concat", total=None):
    wide = _d(B, sum(chans) if total is None else total, H, W)
    if typ == "Concat":
        ins = ",".join(f"ins_{i}={_d(B, c, H, W)}" for i, c in enumerate(chans))
        return parse_op(f"(str_vals=(type=Concat),nda_vals=({ins},ins_num=(tn=uint32_t,v={len(chans)}),out={wide}))")
    outs = ",".join(f"outs_{i}={_d(B, c, H, W)}" for i, c in enumerate(chans))
    return parse_op(f"(str_vals=(type=Split),nda_vals=(in={wide},{outs},outs_num=(tn=uint32_t,v={len(chans)})))")


def ann(op):
    return add_pipe_op_annotations(op, OpTune())


def run_func(rtc, fop, ins, seed=None, alias=None, keep=None):
    """Run one annotated function with host inputs -> {OUT arg: array}.  `ins` also preloads OUT args (in-place functions; the untouched part of a concat output);
    alias: {arg: other arg} binds both to one var."""
    spec = pipe_func_args(fop)
    rtc.compile([RtcFuncInfo("f", "", [a for a, _ in spec], fop)])
    am, made = {}, []
    try:
        for an, io in spec:
            if io == "REF":
                am[an] = RtcArg.ref(fop.get_dims(an)); continue
            if io == "VAL":
                am[an] = RtcArg.scalar(seed, "uint32_t"); continue
            if alias and an in alias:
                am[an] = RtcArg.var(alias[an]); continue
            rtc.create_var_with_dims(an, fop.get_dims(an)); made.append(an); am[an] = RtcArg.var(an)
            if an in ins:
                rtc.copy_nda_to_var(an, np.ascontiguousarray(ins[an], dtype=np.float32))
        rtc.run(RtcFuncCall("f", am))
        rtc.finish_and_sync()
        if keep is not None:
            keep.append(rtc.last_launch()["kernel"] if rtc.be == "hip" else "")
        return {a: rtc.copy_var_to_nda(am[a].n) for a, io in spec if io == "OUT"}
    finally:
        for vn in made:
            rtc.release_var(vn)
        rtc.release_func("f"); rtc.release_per_call_id_data()


def bits_eq(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def reduce_inputs(n, size=1023, seed=0):
    rng = np.random.default_rng(seed)
    xs = [rng.uniform(-3, 3, size).astype(np.float32) for _ in range(n)]
    for x in xs:
        x[0] = -0.0                                   # -0 + -0 + ... from +0 is +0
    order = [2.0 ** 24, 1.0, -(2.0 ** 24)]            # ((0 + 2^24) + 1) - 2^24 = 0, any other order gives 1
    for i, x in enumerate(xs):
        x[1] = order[i] if i < 3 else 0.0
    if n == 2:
        xs[0][1], xs[1][1] = 2.0 ** 24, 1.0
    return xs


def test_tables():
    assert PIPE_OP_FUNCS == {"Reduce": ("hip_reduce",), "Dropout": ("hip_dropout",), "BckDropout": ("hip_dropout",), "Concat": ("hip_concat",), "Split": ("hip_split",)}
    assert NATIVE_ARGS["hip_dropout"] == (("inout", "OUT"), ("det_drop_seed", "VAL"))
    assert NATIVE_ARGS["hip_concat"] == (("in", "IN"), ("out", "OUT")) and NATIVE_ARGS["hip_split"] == (("in", "IN"), ("out", "OUT"))
    assert pipe_func_args(ann(reduce_op(3))[0]) == (("ins_0", "IN"), ("ins_1", "IN"), ("ins_2", "IN"), ("out", "OUT"))
    cat = ann(concat_op(2, (1, 2, 5), 3, 5))
    assert [f.get_func_name() for f in cat] == ["hip_concat"] * 3 and [f.get_u32("ocix") for f in cat] == [0, 1, 3]
    spl = ann(concat_op(2, (1, 2, 5), 3, 5, typ="Split"))
    assert [f.get_func_name() for f in spl] == ["hip_split"] * 3 and [f.get_u32("icix") for f in spl] == [0, 1, 3]
    assert ann(dropout_op(0.5, typ="BckDropout"))[0].get_func_name() == "hip_dropout"


def test_explain_plan_names_the_kernels():
    assert rtc_mod.explain_plan(ann(reduce_op(3))[0]).startswith("bodahip_reduce grid=4 ") and "-DNIN=3" in rtc_mod.explain_plan(reduce_op(3))
    assert rtc_mod.explain_plan(ann(dropout_op(0.5))[0]).startswith("bodahip_dropout grid=2 ")
    assert rtc_mod.explain_plan(dropout_op(0.5, typ="BckDropout")).startswith("bodahip_dropout ")
    assert rtc_mod.explain_plan(ann(concat_op(2, (1, 2, 5), 3, 5))[2]).startswith("bodahip_concat grid=1 ")
    assert rtc_mod.explain_plan(ann(concat_op(2, (1, 2, 5), 3, 5, typ="Split"))[1]).startswith("bodahip_split grid=1 ")
    with pytest.raises(UnsupErr, match="2 GiB"):
        rtc_mod.explain_plan(ann(reduce_op(2, "(dims=(v=536870912))"))[0])
    with pytest.raises(UnsupErr, match="2 GiB"):
        rtc_mod.explain_plan(ann(dropout_op(0.5, "(dims=(v=536870912))"))[0])
    with pytest.raises(UnsupErr, match="2 GiB"):
        rtc_mod.explain_plan(ann(concat_op(1, (1, 1 << 20), 23, 23))[0])


@pytest.mark.parametrize("n", [2, 3, 8])
def test_cpu_reduce(cpu, n):
    xs = reduce_inputs(n)
    got = run_func(cpu, ann(reduce_op(n))[0], {f"ins_{i}": x for i, x in enumerate(xs)})["out"]
    assert bits_eq(got, ref.reduce_f32(xs))
    assert bits_eq(got[:1], np.zeros(1, np.float32))                 # +0, not -0
    assert got[1] == (2.0 ** 24 if n == 2 else 0.0)                  # the chain runs in input order: 2^24 + 1 stays 2^24
    if n >= 3:
        assert ref.reduce_f32(xs[::-1])[1] == 1.0                    # ... and the reverse order would give 1


@pytest.mark.parametrize("ratio", [0.5, 0.1])
def test_cpu_dropout(cpu, ratio):
    x = np.random.default_rng(3).uniform(-2, 2, (2, 3, 7, 11)).astype(np.float32)
    f = ann(dropout_op(ratio))[0]
    a = run_func(cpu, f, {"inout": x}, seed=7)["inout"]
    b = run_func(cpu, f, {"inout": x}, seed=8)["inout"]
    assert bits_eq(a, ref.dropout_f32(x, ratio, 7)) and bits_eq(b, ref.dropout_f32(x, ratio, 8))
    assert np.any((a == 0) != (b == 0))                              # two seeds, two masks
    frac = np.mean(a == 0)
    assert abs(frac - ratio) < 0.08, frac                            # about `ratio` of the elements are dropped
    near = 2 ** 32 - 100                                             # index + seed wraps past 2^32 inside the tensor
    w = run_func(cpu, f, {"inout": x}, seed=near)["inout"]
    assert bits_eq(w, ref.dropout_f32(x, ratio, near))
    assert np.array_equal(ref.dropout_hash(x.size, near)[100:], ref.dropout_hash(x.size - 100, 0))
    hit = ref.dropout_seed_hitting(ratio, 5)                          # element 5 hashes to exactly the threshold: `>` drops it, `>=` would keep it
    assert ref.dropout_hash(x.size, hit)[5] == ref.dropout_thresh(ratio) and x.ravel()[5] != 0
    e = run_func(cpu, f, {"inout": x}, seed=hit)["inout"]
    assert e.ravel()[5] == 0 and bits_eq(e, ref.dropout_f32(x, ratio, hit))
    twice = run_func(cpu, f, {"inout": a}, seed=7)["inout"]          # the gradient of dropout is dropout: the same mask, the scale applied again
    s = ref.dropout_scale(ratio)
    assert bits_eq(twice, np.where(ref.dropout_keep(x.size, ratio, 7).reshape(x.shape), (x * s).astype(np.float32) * s, np.float32(0)))
    assert bits_eq(run_func(cpu, ann(dropout_op(ratio, typ="BckDropout"))[0], {"inout": x}, seed=7)["inout"], a)


def concat_inputs(B, chans, H, W, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-3, 3, (B, c, H, W)).astype(np.float32) for c in chans]


def concat_round_trip(rtc, B, chans, H, W, keep=None):
    xs = concat_inputs(B, chans, H, W)
    wide = np.full((B, sum(chans), H, W), 7.0, np.float32)   # every call must leave the other ranges alone
    for f, x in zip(ann(concat_op(B, chans, H, W)), xs):
        wide = run_func(rtc, f, {"in": x, "out": wide}, keep=keep)["out"]
    assert bits_eq(wide, ref.concat_f32(xs))
    back = [run_func(rtc, f, {"in": wide}, keep=keep)["out"] for f in ann(concat_op(B, chans, H, W, typ="Split"))]
    for b, x in zip(back, xs):
        assert bits_eq(b, x)
    return wide


def test_cpu_concat_split(cpu):
    concat_round_trip(cpu, 2, (1, 2, 5), 3, 5)


def test_cpu_refusals(cpu):
    for n in (1, 9):
        with pytest.raises(UnsupErr, match="2 to 8"):
            reduce_op(n)
    f = ann(reduce_op(2))[0]
    f.nda_vals["ins_num"] = reduce_op(3).get("ins_num"); f.nda_vals["ins_2"] = f.get("ins_0")
    f.nda_vals["ins_num"] = parse_op("(str_vals=(type=x),nda_vals=(n=(tn=uint32_t,v=9)))").get("n")
    with pytest.raises(UnsupErr, match="2 to 8"):   # the backend refuses a function op that grew past eight inputs as well
        cpu.compile([RtcFuncInfo("g", "", ["out"], f)])
    for r in (0.0, 1.0):
        with pytest.raises(RtErr, match="inside"):
            dropout_op(r)
    fd = ann(dropout_op(0.5))[0]; fd.nda_vals["dropout_ratio"] = parse_op("(str_vals=(type=x),nda_vals=(r=(tn=float,v=1.0)))").get("r")
    with pytest.raises(RtErr, match="inside"):
        run_func(cpu, fd, {"inout": np.zeros((2, 3, 7, 11), np.float32)}, seed=1)
    with pytest.raises(RtErr):   # mismatched dims
        parse_op(reduce_op(2).to_str().replace("ins_1=(dims=(v=1023))", "ins_1=(dims=(v=1022))"))
    with pytest.raises(RtErr):   # channels do not add up
        concat_op(2, (1, 2, 5), 3, 5, total=9)
    with pytest.raises(RtErr):   # planes differ
        parse_op(concat_op(2, (1, 2), 3, 5).to_str().replace("ins_1=(dims=(img=2,chan=2,y=3,x=5))", "ins_1=(dims=(img=2,chan=2,y=3,x=4))"))
    fc = ann(concat_op(2, (1, 2, 5), 3, 5))[2]; fc.nda_vals["ocix"] = parse_op("(str_vals=(type=x),nda_vals=(n=(tn=uint32_t,v=4)))").get("n")
    with pytest.raises(RtErr, match="do not fit"):   # the range must fit
        run_func(cpu, fc, {"in": np.zeros((2, 5, 3, 5), np.float32)})
    f2 = ann(reduce_op(2))[0]
    cpu.compile([RtcFuncInfo("g", "", ["ins_0", "ins_1", "out"], f2)])
    try:
        for an, n in (("ins_0", 1023), ("ins_1", 1022), ("out", 1023)):
            cpu.create_var_with_dims(an, Dims(("v",), (n,), "float"))
        with pytest.raises(RtErr, match="the op says"):
            cpu.run(RtcFuncCall("g", {an: RtcArg.var(an) for an in ("ins_0", "ins_1", "out")}))
    finally:
        for an in ("ins_0", "ins_1", "out"):
            cpu.release_var(an)
        cpu.release_func("g")
    with pytest.raises(RtErr):
        add_pipe_op_annotations(parse_op("(str_vals=(type=ZeroIfNonPos),nda_vals=(cond=(dims=(v=8)),in=(dims=(v=8)),out=(dims=(v=8))))"), OpTune())
    with pytest.raises(UnsupErr):
        add_pipe_op_annotations(reduce_op(2), OpTune(hip_dtype="bf16"))


# ---- ConvPipeBck on be=cpu
@pytest.mark.parametrize("name", sorted(PIPES))
def test_cpu_pipe_against_float64(cpu, name):
    drv, bp, params, data, label, fwd = run_pipe(cpu, name)
    try:
        check_against_f64(name, drv, bp, fwd, "be=cpu")
    finally:
        drv.release()


def test_cpu_calls_and_side_vars(cpu):
    drv, bp, *_ = run_pipe(cpu, "chain")
    try:
        funcs = [(t, f.get_func_name()) for t, f, _ in drv.calls()]
        assert funcs == [("conv1", "hip_conv"), ("norm1", "hip_lrn_sb"), ("pool1", "hip_pool_yx"), ("drop1", "hip_dropout"), ("fc", "hip_conv"),
                         ("loss", "hip_softmax"), ("loss", "hip_sm_grad_and_loss"), ("loss", "hip_sum_loss_over_imgs"),
                         ("fc_bck", "hip_bconv_in"), ("fc_bck", "hip_bconv_biases"), ("fc_bck", "hip_bconv_filts"), ("drop1_bck", "hip_dropout"), ("pool1_bck", "hip_spreading"),
                         ("norm1_bck", "hip_bck_lrn"), ("relu_conv1_bck", "hip_zero_if_non_pos"),
                         ("conv1_bck", "hip_bconv_in"), ("conv1_bck", "hip_bconv_biases"), ("conv1_bck", "hip_bconv_filts")]   # the fused ReLU emits no forward call
        assert drv.calls()[0][1].get_u32("conv_has_relu") == 1 and drv.calls()[4][1].get_u32("conv_has_relu") == 0
        for vn in ("pool1_in_yx", "norm1_scale_base", "loss_prob", "loss_per_pel"):   # the reference's names (src/rtc_fwd.cc:296-377)
            assert vn in drv.vars
        seeds = [int(am["det_drop_seed"].v[0]) for _, f, am in drv.calls() if f.get_func_name() == "hip_dropout"]
        assert seeds == [SEED_A, SEED_A]   # the forward and the backward call of one layer share the seed
        zi = [am for t, f, am in drv.calls() if f.get_func_name() == "hip_zero_if_non_pos"][0]
        assert zi["in"].n == zi["out"].n == "conv1_grad_loss" and zi["cond"].n == "conv1"   # in place
    finally:
        drv.release()


def test_cpu_seed_protocol(cpu):
    a1 = run_pipe(cpu, "chain", SEED_A); a1[0].release()
    b = run_pipe(cpu, "chain", SEED_B); b[0].release()
    a2 = run_pipe(cpu, "chain", SEED_A); a2[0].release()
    for n in grad_nodes(a1[1]) + ["loss"]:
        assert bits_eq(a1[5][n], a2[5][n]), n
    assert not bits_eq(a1[5]["conv1_filts_grad_loss"], b[5]["conv1_filts_grad_loss"]) and not bits_eq(a1[5]["pool1_grad_loss"], b[5]["pool1_grad_loss"])
