"""The gradient pipe driver's call list, vars and backend traffic, pinned as digests: tests/golden/bck_calls/snapshot.json holds, per configuration of the small pipes,
one 12-hex digest per call of ConvPipeBck.calls() -- (tag, function op text, arg names, var names, by-value values) -- digests of vars, _call_deps(), sgd_params,
n_sgd_calls, frozen and fused_relu_grads, a digest of every backend call init() made (method, name, sha of the bytes where there are bytes), the same for an EvalPipe built on
the driver, and for both the backend calls of three eager passes and of the captures and two replays.  A driver refactor must leave every one of them as it is.  The refusals: type and message as recorded, and no var created before them.

The fixture is written by this module's own writer, which uses nothing but ConvPipeBck, EvalPipe, add_bck_ops and _call_deps:
    python tests/test_bck_calls_snapshot_cpu.py --write
(after `python -m boda_amd.build`; be=cpu, no device needed)."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (HERE, os.path.dirname(HERE)) if p not in sys.path]      # (the writer runs as a script)
import bn_ref as R
from boda_amd.bck_pipe import ConvPipeBck, Freeze, LrPolicy, SgdSolver, Solver, add_bck_ops
from boda_amd.cnn_op import OpTune
from boda_amd.conv_pipe import ConvPipe, DryRtc, PipeOp, _conv
from boda_amd.eval_pipe import EvalPipe
from boda_amd.input_pipe import InputTransform
from boda_amd.op import Dims, RtErr, UnsupErr
from boda_amd.rtc import make_rtc
from test_bck_pipe_cpu import HEADS_TOPS, chain, fan, heads, small_params

GOLD = os.path.join(HERE, "golden", "bck_calls", "snapshot.json")
NETS = {"chain": (chain, None, small_params), "fan": (fan, None, small_params), "heads": (heads, HEADS_TOPS, small_params),
        "residual": (R.residual, None, lambda cp, seed: R.res_params(cp, seed))}


def sha(x, n=12) -> str:
    return hashlib.sha256(x if isinstance(x, bytes) else repr(x).encode()).hexdigest()[:n]


def dims_txt(d) -> str:
    return "" if d is None else f"{d.tn} {tuple(d.names)} {tuple(d.sizes)}"


class MultiDry(DryRtc):      # the multi-device backend as tests/test_bck_shards_cpu.py builds it
    devices = [0, 0, 0]


class Recorder:
    """A backend that logs (method, name, what was passed) of every call and passes it on."""

    def __init__(self, inner):
        self._inner, self.log = inner, []

    def __getattr__(self, name):
        a = getattr(self._inner, name)
        if name.startswith("__") or not callable(a):
            return a

        def call(*args, **kw):
            self.log.append((name,) + tuple(self._txt(v) for v in args))
            return a(*args, **kw)
        return call

    @staticmethod
    def _txt(v):
        if isinstance(v, np.ndarray):
            return f"{v.dtype} {v.shape} {sha(np.ascontiguousarray(v).tobytes(), 16)}"
        if isinstance(v, Dims):
            return dims_txt(v)
        if isinstance(v, (list, tuple)):
            return [Recorder._txt(e) for e in v]
        if hasattr(v, "func_name") and hasattr(v, "op"):      # an RtcFuncInfo
            return (v.func_name, tuple(v.arg_names), sha(v.op.to_str(), 16))
        if hasattr(v, "rtc_func_name"):
            return v.rtc_func_name
        return v if isinstance(v, str) else repr(v)


def call_digests(calls):
    out = []
    for tag, fop, am in calls:
        args = [(an, a.n, dims_txt(a.dims), None if a.v is None else (str(a.v.dtype), a.v.tolist())) for an, a in am.items()]
        out.append(sha((tag, fop.to_str(), args)))
    return out


def _chain_xf():
    return InputTransform((16, 17), crop=13, mirror=True, scale=0.5, mean_value=[3.0, 2.0, 1.0], seed=5)


def _res_xf():
    return InputTransform((12, 12), crop=9, mirror=True, layout="chw", seed=5)


ADAM = lambda: Solver("adam", lr=0.01, clip_gradients=0.5, lr_policy=LrPolicy("step", gamma=0.5, stepsize=2))
# name -> (keyword arguments of ConvPipeBck, backend: "cpu" | "multi")
COMMON = {
    "default": ({}, "cpu"),
    "fuse_relu_grad": (dict(fuse_relu_grad=True), "cpu"),
    "seed_in_var": (dict(seed_in_var=True), "cpu"),
    "fuse_relu_grad+seed_in_var": (dict(fuse_relu_grad=True, seed_in_var=True), "cpu"),
    "fuse_filts_biases": (dict(fuse_filts_biases=True), "cpu"),
    "bf16": (dict(grad_operands="bf16"), "cpu"),
    "sgd_tpc2": (lambda: dict(solver=SgdSolver(lr=0.05, tensors_per_call=2, lr_mult={"biases": 2.0}, decay_mult={"biases": 0.0})), "cpu"),
    "solver_nesterov": (lambda: dict(solver=Solver("nesterov", lr=0.05, tensors_per_call=3)), "cpu"),
    "adam_clip_step_iter3": (lambda: dict(solver=ADAM(), iter_size=3), "cpu"),
    "freeze_biases": (lambda: dict(freeze=Freeze(params=("biases",)), solver=ADAM()), "cpu"),
    "freeze_keep_data": (lambda: dict(freeze=Freeze(keep_grads=("data",))), "cpu"),
    "freeze_empty": (lambda: dict(freeze=Freeze()), "cpu"),
    "img_chunks2": (dict(img_chunks=2), "cpu"),
}
CONFIGS = {
    "chain": dict(COMMON, input_transform=(lambda: dict(input_transform=_chain_xf(), solver=SgdSolver(lr=0.05)), "cpu"),
                  devices=(dict(seed_in_var=True, fuse_relu_grad=True), "multi"), devices_sgd=(lambda: dict(solver=SgdSolver(lr=0.05)), "multi")),
    "residual": dict(COMMON, input_transform=(lambda: dict(input_transform=_res_xf()), "cpu"),
                     freeze_bn_global_scale=(lambda: dict(freeze=Freeze(params=("scale", "bias"), bn_global_stats=True), solver=Solver("sgd", lr=0.05)), "cpu"),
                     freeze_bn_some=(lambda: dict(freeze=Freeze(params=("stem", "scale_a_2a_scale"), bn_global_stats=["bn_stem", "bn_a_2b"]), fuse_relu_grad=True), "cpu"),
                     freeze_all_but_fc=(lambda: dict(freeze=Freeze(params=("filts", "scale", "bias", "stem_biases"), bn_global_stats=True, keep_grads=("res_a",))), "cpu"),
                     devices_chunks3=(lambda: dict(img_chunks=3, solver=Solver("sgd", lr=0.05)), "multi")),
    "fan": {k: COMMON[k] for k in ("default", "fuse_relu_grad+seed_in_var", "sgd_tpc2", "freeze_biases", "freeze_keep_data")},
    "heads": {k: COMMON[k] for k in ("default", "fuse_relu_grad+seed_in_var", "adam_clip_step_iter3", "freeze_empty", "fuse_filts_biases")},
}
CONFIGS["fan"]["devices"] = ({}, "multi")


def step_logs(rec, obj, bp, xf, eager, capture, replay) -> dict:
    """The backend traffic of three eager passes (a whole update of iter_size=3) and -- where the call list can be captured -- of the captures and two replays, as digests;
    a refused capture as its type and message."""
    rng = np.random.default_rng(17)
    d = bp.nodes[bp.cp.in_node]
    feed = {"label": rng.integers(0, 5, (d.dsz("img"), 1, 1)).astype(np.float32)}
    if xf is not None:
        feed["data_raw"] = rng.integers(0, 256, xf.src_dims(d.dsz("img"), d.dsz("chan")).sizes).astype(np.uint8)
    else:
        feed[bp.cp.in_node] = rng.uniform(-1, 1, d.sizes).astype(np.float32)
    rec.log = []
    for _ in range(3):
        eager(feed)
    out = {"step_log": sha(rec.log), "n_step_log": len(rec.log), "per_call_ms": sha([c[:2] for c in obj.per_call_ms])}
    rec.log = []
    try:
        capture()
        for _ in range(2):
            replay(feed)
        out["graph_log"] = sha(rec.log)
    except (RtErr, UnsupErr) as e:
        out["graph_log"] = [type(e).__name__, str(e)[:80], sha(rec.log)]
    out["n_graph_log"] = len(rec.log)
    return out


def snapshot_of(net: str, cfg: str) -> dict:
    mk, tops, mkparams = NETS[net]
    kw, be = CONFIGS[net][cfg]
    kw = kw() if callable(kw) else dict(kw)
    cp = mk(3)
    bp = add_bck_ops(cp, loss_tops=tops)
    inner = make_rtc("(be=cpu)") if be == "cpu" else MultiDry()
    if be == "cpu":
        inner.init()
    rec = Recorder(inner)
    try:
        drv = ConvPipeBck(rec, **kw)
        drv.init(bp, mkparams(cp, 1))
        out = {"calls": call_digests(drv.calls()), "tags": sha([t for t, _, _ in drv.calls()]), "vars": sha(list(drv.vars)), "funcs": sha(list(drv.funcs)),
               "deps": sha(drv._call_deps()), "sgd_params": sha(list(drv.sgd_params)), "n_sgd_calls": drv.n_sgd_calls, "frozen": sha(sorted(drv.frozen.items())),
               "fused_relu_grads": sha(sorted(drv.fused_relu_grads.items())), "init_log": sha(rec.log), "n_init_log": len(rec.log)}
        rec.log = []
        try:
            ev = EvalPipe(drv, top_k=2)
            out["eval"] = {"calls": call_digests(ev.calls()), "vars": sha(list(ev.vars)), "funcs": sha(list(ev.funcs)), "log": sha(rec.log), "n_log": len(rec.log)}
            if be == "cpu":
                out["eval"].update(step_logs(rec, ev, bp, drv.input_transform, lambda feed: ev.run_batch(feed), ev.capture_graph, lambda feed: ev.run_batch(feed, graph=True)))
            ev.release()
        except (RtErr, UnsupErr) as e:
            out["eval"] = {"error": [type(e).__name__, str(e)], "n_log": len(rec.log)}
        if be == "cpu":
            step = lambda graph: lambda feed: drv.run_bck(list(feed), dict(feed), bp.loss_nodes, graph=graph)
            out.update(step_logs(rec, drv, bp, drv.input_transform, step(False), lambda: (drv.capture_graph(), drv.capture_graph(parallel=True)), step(True)))
        out["tag_list"] = [t for t, _, _ in drv.calls()]      # (for the message of a mismatch; not written to the fixture)
        drv.release()
    finally:
        if be == "cpu":
            inner.close()
    return out


# ---- the refusals
def _seed_clash():
    p = ConvPipe("clash", "data", Dims.make("float", img=2, chan=3, y=13, x=13))
    _conv(p, "det_drop_seed", "data", 8, 3, 2)
    p.add(PipeOp("fc", "Convolution", "det_drop_seed", "fc", out_chans=5, kern_sz=(0, 0)))
    return p


def _scale_bn():
    p = ConvPipe("scale_bn", "data", Dims.make("float", img=2, chan=3, y=5, x=5))
    p.add(PipeOp("c", "Convolution", "data", "c", out_chans=4, kern_sz=(3, 3)))
    p.add(PipeOp("sc", "Scale", "c", "c")); p.add(PipeOp("bn", "BatchNorm", "c", "c"))
    p.add(PipeOp("fc", "Convolution", "c", "fc", out_chans=5, kern_sz=(0, 0)))
    return p


REFUSALS = {      # name -> (pipe builder, keyword arguments)
    "seed_var_is_a_node": (_seed_clash, lambda: dict(seed_in_var=True)),
    "tensors_per_call_0": (lambda: chain(2), lambda: dict(solver=SgdSolver(lr=0.1, tensors_per_call=0))),
    "freeze_names_nothing": (lambda: chain(2), lambda: dict(freeze=Freeze(params=("conv9",)))),
    "freeze_everything": (lambda: chain(2), lambda: dict(freeze=Freeze(params=("filts", "biases")))),
    "input_transform_wrong_crop": (lambda: chain(2), lambda: dict(input_transform=InputTransform((16, 17), crop=12))),
    "scale_before_batchnorm": (_scale_bn, lambda: dict()),
    "annotation_unsup": (lambda: chain(2), lambda: dict(op_tune=OpTune(hip_algo="winograd"))),      # conv1 takes the tune; norm1, an LRN, has no such variant
}


def refusal_of(name: str):
    mk, kw = REFUSALS[name]
    inner = make_rtc("(be=cpu)"); inner.init()
    rec = Recorder(inner)
    try:
        drv = ConvPipeBck(rec, **kw())
        try:
            drv.init(add_bck_ops(mk()), None)
        except (RtErr, UnsupErr) as e:
            return {"type": type(e).__name__, "msg": str(e)}, [l[0] for l in rec.log]
        finally:
            for l in rec.log:      # (what a refusal behind a creation left)
                if l[0] == "create_var_with_dims":
                    inner.release_var(l[1])
        raise AssertionError(f"{name}: init raised nothing")
    finally:
        inner.close()


def write_fixture() -> None:
    snap = {"configs": {}, "refusals": {}}
    for net in CONFIGS:
        for cfg in CONFIGS[net]:
            s = snapshot_of(net, cfg); s.pop("tag_list")
            snap["configs"][f"{net}/{cfg}"] = s
    for name in REFUSALS:
        snap["refusals"][name] = refusal_of(name)[0]
    os.makedirs(os.path.dirname(GOLD), exist_ok=True)
    with open(GOLD, "w") as f:
        body = [json.dumps(sec) + ": {\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in sorted(snap[sec].items())) + "\n}" for sec in sorted(snap)]
        f.write("{\n" + ",\n".join(body) + "\n}\n")      # (one line per configuration)


@pytest.fixture(scope="module")
def gold():
    with open(GOLD) as f:
        return json.load(f)


def test_fixture_lists_these_configurations(gold):
    assert sorted(gold["configs"]) == sorted(f"{n}/{c}" for n in CONFIGS for c in CONFIGS[n]) and sorted(gold["refusals"]) == sorted(REFUSALS)
    assert len(gold["configs"]) >= 32 and os.path.getsize(GOLD) < 100 * 1024


@pytest.mark.parametrize("key", [f"{n}/{c}" for n in CONFIGS for c in CONFIGS[n]])
def test_snapshot(gold, key):
    net, cfg = key.split("/")
    got, want = snapshot_of(net, cfg), gold["configs"][key]
    tags = got.pop("tag_list")
    for i, (a, b) in enumerate(zip(got["calls"], want["calls"])):
        assert a == b, f"{key}: call {i} ({tags[i]}) differs from the recorded one"
    assert len(got["calls"]) == len(want["calls"]), f"{key}: {len(got['calls'])} calls, {len(want['calls'])} recorded"
    for k in want:
        if k == "eval":
            continue
        assert got[k] == want[k], f"{key}: {k} differs from the recorded one"
    ge, we = got["eval"], want["eval"]
    for i, (a, b) in enumerate(zip(ge.get("calls", []), we.get("calls", []))):
        assert a == b, f"{key}: EvalPipe call {i} differs from the recorded one"
    assert ge == we, f"{key}: EvalPipe: {[k for k in we if ge.get(k) != we[k]]} differ from the recorded ones"


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusal_comes_before_any_var(gold, name):
    got, log = refusal_of(name)
    assert got == gold["refusals"][name], name
    assert "create_var_with_dims" not in log and "compile" not in log, (name, log[:4])


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_bck_calls_snapshot_cpu.py --write")
    write_fixture()
    print(GOLD, os.path.getsize(GOLD), "bytes")
