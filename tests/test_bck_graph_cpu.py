"""The gradient step as a graph, the parts that need no GPU: hip_dropout with its seed read from a var (seed_from_var=1) on be=cpu, ConvPipeBck(seed_in_var=True) on
be=cpu, the dependency lists a parallel capture hands to the backend (ConvPipeBck._call_deps), and the refusals.

Every comparison is np.array_equal on the uint32 views: no tolerance is involved.

_call_deps is checked twice.  Structure: what must and must not depend on what.  Sufficiency: the call list runs on be=cpu in two other orders that respect the
lists -- always the LATEST ready call, and a seeded random topological order -- with every var that a step writes poisoned first; a missing dependency lets a call read
the poison (or a stale value), and some var then differs from the list order's.  "Ordered" for a Dropout and its BckDropout twin means a path in the dependency graph:
the forward call rewrites X, the backward call X_grad_loss, and every call between them that touches X or X_grad_loss hangs on one of the two."""
import os

import numpy as np
import pytest

import bck_pipe_ref as ref
from boda_amd import rtc as rtc_mod
from boda_amd.bck_pipe import DROP_LAYER_STEP, SEED_VAR, ConvPipeBck, add_bck_ops
from boda_amd.cnn_op import NATIVE_ARGS, OpTune, pipe_func_args, seed_from_var
from boda_amd.conv_pipe import ConvPipe, PipeOp, _conv
from boda_amd.op import Dims, Nda, RtErr
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc

from test_bck_pipe_cpu import PIPES, SEED_A, SEED_B, ann, bits_eq, dropout_op, grad_nodes, reduce_op, run_func, run_pipe, small_inputs, small_params

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops", "bck-graph-ops.txt")
M32 = 1 << 32
LAYER_K = 3
SHAPES = {"462": ("(dims=(img=2,chan=3,y=7,x=11))", (2, 3, 7, 11)), "1023": ("(dims=(v=1023))", (1023,))}   # 115 quads and a tail of two | 255 quads and a tail of three
SEED_PAIRS = [(0, SEED_A), (SEED_A, 0), (0xFFFFFFF0, 0x20), (SEED_A, (LAYER_K * DROP_LAYER_STEP) % M32)]    # (word, by-value): the third wraps past 2^32


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


def drop_input(shape):
    return np.random.default_rng(3).uniform(-2, 2, shape).astype(np.float32)


def run_flagged(rtc, fop, x, word, byval, keep=None, seed_var=("uint32_t", 1), bind=None, fname="fsv"):
    """One call of a seed_from_var=1 hip_dropout: inout <- x, a var `seedw` of type / size seed_var holding `word`, the by-value det_drop_seed `byval` -> inout.
    bind: {arg: var name} overrides (None drops the arg)."""
    spec = pipe_func_args(fop)
    rtc.compile([RtcFuncInfo(fname, "", [a for a, _ in spec], fop)])
    made = []
    try:
        rtc.create_var_with_dims("inout", fop.get_dims("inout")); made.append("inout")
        rtc.copy_nda_to_var("inout", x)
        rtc.create_var_with_dims("seedw", Dims(("v",), (seed_var[1],), seed_var[0])); made.append("seedw")
        rtc.copy_nda_to_var("seedw", np.full(seed_var[1], word, {"uint32_t": np.uint32, "float": np.float32}[seed_var[0]]))
        am = {"inout": RtcArg.var("inout"), "det_drop_seed_var": RtcArg.var("seedw"), "det_drop_seed": RtcArg.scalar(byval, "uint32_t")}
        for an, vn in (bind or {}).items():
            if vn is None:
                am.pop(an)
            else:
                am[an] = RtcArg.var(vn)
        rtc.run(RtcFuncCall(fname, am)); rtc.finish_and_sync()
        if keep is not None:
            keep.append(rtc.last_launch()["kernel"] if rtc.be == "hip" else "")
        return rtc.copy_var_to_nda("inout")
    finally:
        for vn in made:
            rtc.release_var(vn)
        rtc.release_func(fname); rtc.release_per_call_id_data()


# ---- the seed var on be=cpu
@pytest.mark.parametrize("ratio", [0.5, 0.1])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_cpu_seed_from_var(cpu, shape, ratio):
    dims, shp = SHAPES[shape]
    x = drop_input(shp)
    plain = ann(dropout_op(ratio, dims))[0]
    flagged = seed_from_var(plain)
    masks = []
    for word, byval in SEED_PAIRS:
        summed = (word + byval) % M32
        got = run_flagged(cpu, flagged, x, word, byval)
        assert bits_eq(got, run_func(cpu, plain, {"inout": x}, seed=summed)["inout"]), (word, byval)
        assert bits_eq(got, ref.dropout_f32(x, ratio, summed)), (word, byval)
        masks.append(got == 0)
    assert bits_eq(run_flagged(cpu, flagged, x, *SEED_PAIRS[0]), run_flagged(cpu, flagged, x, *SEED_PAIRS[1]))   # only the sum counts
    assert np.any(masks[0] != masks[2]) and np.any(masks[0] != masks[3])                                         # other sums, other masks
    bck = seed_from_var(ann(dropout_op(ratio, dims, typ="BckDropout"))[0])                                       # a BckDropout's function takes the flag the same way
    assert bits_eq(run_flagged(cpu, bck, x, SEED_A, 7), ref.dropout_f32(x, ratio, SEED_A + 7))


def test_arg_lists_and_plan():
    plain = ann(dropout_op(0.5))[0]
    flagged = seed_from_var(plain)
    assert pipe_func_args(plain) == NATIVE_ARGS["hip_dropout"] == (("inout", "OUT"), ("det_drop_seed", "VAL"))
    assert pipe_func_args(flagged) == (("inout", "OUT"), ("det_drop_seed_var", "IN"), ("det_drop_seed", "VAL"))
    assert flagged.get_u32("seed_from_var") == 1 and not plain.has("seed_from_var") and not plain.has("det_drop_seed_var")
    d = flagged.get_dims("det_drop_seed_var")
    assert (d.tn, tuple(d.names), tuple(d.sizes)) == ("uint32_t", ("v",), (1,))
    off = flagged.copy(); off.nda_vals["seed_from_var"] = Nda(None, "uint32_t", (0,))   # 0 is the unflagged function
    assert pipe_func_args(off) == NATIVE_ARGS["hip_dropout"]
    p, f = rtc_mod.explain_plan(plain), rtc_mod.explain_plan(flagged)
    assert "SEEDVAR" not in p and f == p + " -DSEEDVAR=1", (p, f)
    assert rtc_mod.explain_plan(off) == p
    assert rtc_mod.prebuild(flagged) > 0   # the define compiles for gfx950
    with pytest.raises(RtErr, match="seed_from_var"):
        seed_from_var(ann(reduce_op(2))[0])


def test_cpu_refusals(cpu):
    x = drop_input(SHAPES["462"][1])
    flagged = seed_from_var(ann(dropout_op(0.5))[0])
    red = ann(reduce_op(2))[0]; red.set_u32("seed_from_var", 1)   # the flag on another function: at compile, at prebuild, in the plan
    with pytest.raises(RtErr, match="seed_from_var=1 on 'hip_reduce'"):
        cpu.compile([RtcFuncInfo("g", "", ["ins_0", "ins_1", "out"], red)])
    with pytest.raises(RtErr, match="seed_from_var=1 on 'hip_reduce'"):
        rtc_mod.prebuild(red)
    with pytest.raises(RtErr, match="seed_from_var=1 on 'hip_reduce'"):
        rtc_mod.explain_plan(red)
    with pytest.raises(RtErr, match="'det_drop_seed_var' is required"):
        run_flagged(cpu, flagged, x, 1, 2, bind={"det_drop_seed_var": None})
    with pytest.raises(RtErr, match="exactly one element"):
        run_flagged(cpu, flagged, x, 1, 2, seed_var=("float", 1))
    with pytest.raises(RtErr, match="exactly one element"):
        run_flagged(cpu, flagged, x, 1, 2, seed_var=("uint32_t", 2))
    with pytest.raises(RtErr, match="same var 'inout'"):
        run_flagged(cpu, flagged, x, 1, 2, bind={"det_drop_seed_var": "inout"})
    with pytest.raises(RtErr, match="by-value uint32_t scalar"):   # the by-value seed stays an argument of the flagged call
        run_flagged(cpu, flagged, x, 1, 2, bind={"det_drop_seed": "seedw"})


def fixture_ops():
    """The seed_from_var=1 function ops tests/test_gpu_bck_graph.py launches, in a fixed order: what tests/golden/ops/bck-graph-ops.txt holds, so that build()
    specialises bodahip_dropout -DSEEDVAR=1 ahead of the GPU run."""
    from boda_amd.conv_pipe import DryRtc, nin_imagenet
    ops = [seed_from_var(ann(dropout_op(ratio, SHAPES[shape][0]))[0]) for shape in sorted(SHAPES) for ratio in (0.5, 0.1)]
    for cp, tops in [(PIPES["chain"][0](), None), (nin_imagenet(2), None)]:
        drv = ConvPipeBck(DryRtc(), seed_in_var=True); drv.init(add_bck_ops(cp, loss_tops=tops), {n: np.zeros(d.sizes, np.float32) for n, d in cp.params.items()})
        ops += [f for _, f, _ in drv.calls() if f.has("seed_from_var")]
    seen, out = set(), []
    for f in ops:
        if f.to_str() not in seen:
            seen.add(f.to_str()); out.append(f)
    return out


def test_fixture_file_lists_these_ops():
    from boda_amd.op import read_ops
    have = [o.to_str() for o in read_ops(GOLD)]
    assert have == [f.to_str() for f in fixture_ops()] and len(have) >= 6
    for line in have:
        assert "seed_from_var=(tn=uint32_t,v=1)" in line and "func_name=hip_dropout" in line


# ---- ConvPipeBck(seed_in_var=True) on be=cpu
_DEFAULT = {}


def default_step(name, seed):
    """Every gradient node and loss of a default driver's step at `seed` on a be=cpu instance of its own (the var names are the pipe's), computed once."""
    if (name, seed) not in _DEFAULT:
        r = make_rtc("(be=cpu)"); r.init()
        try:
            drv, bp, params, data, label, fwd = run_pipe(r, name, seed)
            drv.release()
        finally:
            r.close()
        _DEFAULT[(name, seed)] = fwd
    return _DEFAULT[(name, seed)]


def make_driver(rtc, name, **kw):
    mk, tops, seed = PIPES[name]
    cp = mk(); bp = add_bck_ops(cp, loss_tops=tops)
    drv = ConvPipeBck(rtc, **kw); drv.init(bp, small_params(cp, seed))
    data, label = small_inputs(cp, seed)
    return drv, bp, data, label


def test_cpu_pipe_seed_in_var(cpu):
    drv, bp, data, label = make_driver(cpu, "chain", seed_in_var=True)
    try:
        assert SEED_VAR in drv.vars and cpu.get_var_dims(SEED_VAR) == Dims(("v",), (1,), "uint32_t")
        drops = [(t, f, am) for t, f, am in drv.calls() if f.get_func_name() == "hip_dropout"]
        assert [t for t, _, _ in drops] == ["drop1", "drop1_bck"]
        for _, f, am in drops:
            assert f.get_u32("seed_from_var") == 1 and am["det_drop_seed_var"].n == SEED_VAR and int(am["det_drop_seed"].v[0]) == 0   # layer 0: offset 0
        gets = grad_nodes(bp) + bp.loss_nodes
        forms = [c.rfc.__dict__.get("_c_form") for c in drv.bck_calls]
        for i, seed in enumerate((SEED_A, SEED_B)):
            before = rtc_mod.compile_stats()
            drv.set_det_drop_seed(seed)
            assert int(cpu.copy_var_to_nda(SEED_VAR)[0]) == seed
            fwd = {"data": data, "label": label}
            drv.run_bck(["data", "label"], fwd, gets)
            want = default_step("chain", seed)
            for n in gets:
                assert bits_eq(fwd[n], want[n]), (seed, n)
            after = rtc_mod.compile_stats()
            assert (after["compiled"], after["cache_hits"]) == (before["compiled"], before["cache_hits"])
            now = [c.rfc.__dict__.get("_c_form") for c in drv.bck_calls]
            if i:   # the marshalled form of every call survived the new seed: nothing was invalidated
                assert all(a is b and a is not None for a, b in zip(forms, now))
            forms = now
        assert not bits_eq(default_step("chain", SEED_A)["pool1_grad_loss"], default_step("chain", SEED_B)["pool1_grad_loss"])
    finally:
        drv.release()


def test_cpu_layer_offsets_and_default_unchanged(cpu):
    """Two Dropout layers: the by-value offsets are k * 0x9E3779B1 and the nodes equal the default driver's.  And the default driver is what it was."""
    def two_drops():
        p = ConvPipe("two_drops", "data", Dims.make("float", img=2, chan=3, y=9, x=9))
        _conv(p, "c1", "data", 6, 3, 2)
        p.add(PipeOp("d1", "Dropout", "c1", "c1"))
        _conv(p, "c2", "c1", 6, 1)
        p.add(PipeOp("d2", "Dropout", "c2", "c2"))
        p.add(PipeOp("fc", "Convolution", "c2", "fc", out_chans=5, kern_sz=(0, 0)))
        return p
    cp = two_drops(); bp = add_bck_ops(cp); params = small_params(cp, 0); data, label = small_inputs(cp, 0)
    gets = grad_nodes(bp) + bp.loss_nodes
    out = {}
    for sv in (False, True):
        drv = ConvPipeBck(cpu, seed_in_var=sv); drv.init(bp, params)
        try:
            drv.set_det_drop_seed(SEED_A)
            by_val = {t: int(am["det_drop_seed"].v[0]) for t, f, am in drv.calls() if f.get_func_name() == "hip_dropout"}
            base = 0 if sv else SEED_A
            assert by_val == {"d1": base, "d1_bck": base, "d2": (base + DROP_LAYER_STEP) % M32, "d2_bck": (base + DROP_LAYER_STEP) % M32}
            if not sv:
                assert SEED_VAR not in drv.vars
                for t, f, am in drv.calls():
                    assert not f.has("seed_from_var") and "det_drop_seed_var" not in am
                    if f.get_func_name() == "hip_dropout":
                        assert list(am) == ["inout", "det_drop_seed"]
            fwd = {"data": data, "label": label}
            drv.run_bck(["data", "label"], fwd, gets)
            out[sv] = fwd
        finally:
            drv.release()
    for n in gets:
        assert bits_eq(out[True][n], out[False][n]), n


def test_seed_var_name_clash(cpu):
    p = ConvPipe("clash", "data", Dims.make("float", img=2, chan=3, y=5, x=5))
    _conv(p, SEED_VAR, "data", 4, 3)
    p.add(PipeOp("fc", "Convolution", SEED_VAR, "fc", out_chans=5, kern_sz=(0, 0)))
    bp = add_bck_ops(p)
    drv = ConvPipeBck(cpu, seed_in_var=True)
    with pytest.raises(RtErr, match="is a node of the pipe"):
        drv.init(bp, small_params(p, 0))
    assert drv.vars == [] and drv.funcs == []   # refused before anything was created


# ---- the dependency lists
DEP_CASES = [("chain", {}), ("fan", {}), ("heads", {}), ("chain", {"fuse_relu_grad": True})]


def rd_wr(c):
    am = c.rfc.arg_map
    spec = pipe_func_args(c.fop)
    return ({am[a].n for a, io in spec if io == "IN" or a == "inout"}, {am[a].n for a, io in spec if io == "OUT"})


def closure(deps):
    reach = []
    for d in deps:
        r = set(d)
        for j in d:
            r |= reach[j]
        reach.append(r)
    return reach


@pytest.mark.parametrize("name,kw", DEP_CASES)
def test_call_deps_structure(cpu, name, kw):
    drv, bp, data, label = make_driver(cpu, name, seed_in_var=True, **kw)
    try:
        calls, deps = drv.bck_calls, drv._call_deps()
        assert len(deps) == len(calls)
        for i, d in enumerate(deps):
            assert all(0 <= j < i for j in d) and d == sorted(set(d)), (i, d)
        reach = closure(deps)
        by_tag = {}
        for i, c in enumerate(calls):
            by_tag.setdefault(c.tag, []).append(i)
        n_bconv = 0
        for o in bp.bck_ops():   # the three calls of one BckConv: independent of each other, directly and through others
            if o.type == "BckConv":
                ids = by_tag[o.tag]
                assert [calls[i].fop.get_func_name() for i in ids] == ["hip_bconv_in", "hip_bconv_biases", "hip_bconv_filts"]
                for i in ids:
                    assert not (reach[i] & set(ids)), (o.tag, i, reach[i])
                n_bconv += 1
        assert n_bconv == len(bp.cp.params) // 2
        n_red = 0
        for i, c in enumerate(calls):   # a Reduce hangs on the writer of each of its partial gradients
            if c.fop.get_func_name() == "hip_reduce":
                for an, io in pipe_func_args(c.fop):
                    if io == "IN":
                        w = max(j for j in range(i) if c.rfc.arg_map[an].n in rd_wr(calls[j])[1])
                        assert w in deps[i], (c.tag, an, w, deps[i])
                n_red += 1
        assert n_red == {"chain": 0, "fan": 1, "heads": 1}[name]
        drops = [i for i, c in enumerate(calls) if c.fop.get_func_name() == "hip_dropout"]
        if name == "chain":   # the forward dropout rewrites pool1, its twin pool1_grad_loss
            f, b = drops
            assert (calls[f].tag, calls[b].tag) == ("drop1", "drop1_bck") and f in reach[b]
            for i, c in enumerate(calls):
                rd, wr = rd_wr(c)
                if i > f and "pool1" in rd | wr:
                    assert f in reach[i], (c.tag, c.fop.get_func_name())      # everyone who touches pool1 later runs behind the forward dropout
                if i < f and "pool1" in rd | wr:
                    assert i in reach[f]                                      # ... which runs behind the pooling that wrote it
                if i > b and "pool1_grad_loss" in rd | wr:
                    assert b in reach[i], (c.tag, c.fop.get_func_name())
                if i < b and "pool1_grad_loss" in rd | wr:
                    assert i in reach[b]
            assert SEED_VAR in rd_wr(calls[f])[0] and all(SEED_VAR not in rd_wr(c)[1] for c in calls)   # read-only inside a step
        else:
            assert drops == []
        if kw:   # the fold's `in` is a read: the data gradient of fc_bck... none folds there; norm1_bck (BckLRN) takes relu_conv1_bck and reads conv1
            assert drv.fused_relu_grads["folded"] == ["relu_conv1_bck"]
            i = by_tag["norm1_bck"][0]
            assert "conv1" in rd_wr(calls[i])[0] and by_tag["conv1"][0] in reach[i]
        for p in bp.cp.params:
            assert all(p not in rd_wr(c)[1] for c in calls)
    finally:
        drv.release()


def poison(rtc, drv, keep):
    for vn in drv.vars:
        if vn not in keep:
            d = rtc.get_var_dims(vn)
            rtc.copy_nda_to_var(vn, np.full(d.sizes, 12345.0 if d.tn == "float" else 7, np.float32 if d.tn == "float" else np.uint32))


def run_in_order(rtc, drv, order, keep):
    poison(rtc, drv, keep)
    for i in order:
        rtc.run(drv.bck_calls[i].rfc)
    rtc.finish_and_sync(); rtc.release_per_call_id_data()
    return {vn: rtc.copy_var_to_nda(vn) for vn in drv.vars}


def topo_order(deps, pick):
    done, order = set(), []
    while len(order) < len(deps):
        ready = [i for i in range(len(deps)) if i not in done and all(j in done for j in deps[i])]
        i = pick(ready)
        done.add(i); order.append(i)
    return order


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name,kw", DEP_CASES)
def test_call_deps_are_sufficient(cpu, name, kw):
    drv, bp, data, label = make_driver(cpu, name, seed_in_var=True, **kw)
    try:
        drv.set_det_drop_seed(SEED_A)
        cpu.copy_nda_to_var("data", data); cpu.copy_nda_to_var("label", label)
        keep = set(bp.cp.params) | {"data", "label", SEED_VAR}
        deps = drv._call_deps()
        n = len(deps)
        want = run_in_order(cpu, drv, range(n), keep)
        for gn in grad_nodes(bp) + bp.loss_nodes:   # the poisoned list order is the step (seed_in_var or not)
            assert bits_eq(want[gn], default_step(name, SEED_A)[gn]), gn
        rng = np.random.default_rng(17)
        orders = {"latest ready first": topo_order(deps, max), "random topological": topo_order(deps, lambda r: r[int(rng.integers(len(r)))])}
        for what, order in orders.items():
            assert sorted(order) == list(range(n)) and order != list(range(n)), what   # another order, or the check shows nothing
            got = run_in_order(cpu, drv, order, keep)
            for vn in drv.vars:
                assert same_bits(got[vn], want[vn]), (what, vn)
        # and the check can fail: with the dependencies of one reader dropped, latest-first runs it ahead of its writer
        victim = max(i for i in range(n) if deps[i])
        loose = [([] if i == victim else d) for i, d in enumerate(deps)]
        got = run_in_order(cpu, drv, topo_order(loose, max), keep)
        assert any(not same_bits(got[vn], want[vn]) for vn in drv.vars)
    finally:
        drv.release()


# ---- refusals of the graph forms that need no GPU
class Spy:
    """The backend, with every graph_* call noted."""

    def __init__(self, rtc):
        self._rtc = rtc; self.graph_calls = []

    def __getattr__(self, n):
        if n.startswith("graph_"):
            self.graph_calls.append(n)
        return getattr(self._rtc, n)


def test_capture_refusals_reach_no_backend_call(cpu):
    spy = Spy(cpu)
    drv, bp, data, label = make_driver(spy, "chain")   # a Dropout, and the seed by value
    try:
        with pytest.raises(RtErr, match="seed_in_var=True"):
            drv.capture_graph()
        with pytest.raises(RtErr, match="seed_in_var=True"):
            drv.capture_graph(parallel=True)
        with pytest.raises(RtErr, match="no captured graph"):
            drv.run_bck(["data", "label"], {"data": data, "label": label}, [], graph=True)
        with pytest.raises(RtErr, match="no captured graph"):
            drv.run_graph()
        assert spy.graph_calls == []
    finally:
        drv.release()
    drv, bp, data, label = make_driver(spy, "chain", seed_in_var=True)
    try:
        def boom():
            raise RuntimeError("host-side error while building the deps")
        drv._call_deps = boom
        with pytest.raises(RuntimeError, match="host-side error"):
            drv.capture_graph(parallel=True)
        assert spy.graph_calls == []   # no capture was opened, so none is left open
    finally:
        drv.release()
    assert spy.graph_calls == []       # and release() destroys only a graph that exists
