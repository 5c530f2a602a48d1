"""The SGD update on the MI355X: bodahip_sgd_update (kernels/sgd_update_f32.hip) bit for bit against be=cpu and the numpy twin of the written formula
(tests/sgd_ref.py), and ConvPipeBck(solver=...) on be=hip -- eager, as one hipGraph replay, on three shards of device 0, and on NiN.

Every comparison is np.array_equal on the uint32 views.  The function has no pure output (w and h are rewritten in place, g is only read), so the check that nothing
else is written is a guard var behind every tensor var -- four floats holding a NaN with a payload -- that must come back unchanged; the var bound to an arg must have
exactly the op's dims, so the guard cannot live inside a wider var.  The descent bound is the one tests/test_sgd_cpu.py writes down (sgd_ref.DESCENT_BOUND)."""
import numpy as np
import pytest

import sgd_ref as S
from boda_amd import rtc as rtc_mod
from boda_amd.bck_pipe import SGD_HIST_SFX, ConvPipeBck, SgdSolver, add_bck_ops, host_params
from boda_amd.cnn_op import sgd_update_func_op
from boda_amd.conv_pipe import nin_imagenet
from boda_amd.op import Dims, RtErr
from boda_amd.rtc import make_rtc

from test_bck_pipe_cpu import PIPES, SEED_A, SEED_B, grad_nodes, small_inputs, small_params
from test_sgd_cpu import CASES, HYPER, mults

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    r = make_rtc("(be=hip)", 0)
    r.init()
    yield r
    r.close()


@pytest.fixture(scope="module")
def hip2():
    """The eager driver's backend: a second instance, with a stream, vars and kernels of its own."""
    r = make_rtc("(be=hip)", 0)
    r.init()
    yield r
    r.close()


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


# ---- the function
@pytest.mark.parametrize("sizes", CASES, ids=lambda s: f"n{len(s)}_{s[0]}")
def test_function_against_cpu_and_numpy(hip, cpu, sizes):
    guard = np.full(4, S.GUARD_BITS, np.uint32)
    for lr_mult, decay_mult in ((1, 1), (2, 0), (1, 0), (2, 1)):
        for momentum in (0.0, 0.9):
            lm, dm = mults(len(sizes), lr_mult, decay_mult)
            ins = S.make_inputs(sizes)
            hy = [(HYPER[0], momentum, HYPER[2])]
            keep = []
            got, guards = S.run_sgd(hip, sizes, lm, dm, hy, ins, guards=True, keep=keep)
            assert keep[0]["kernel"] == "bodahip_sgd_update" and keep[0]["kernels"] == 1 and keep[0]["grid"] == sum(-(-n // 4096) for n in sizes)
            assert keep[0]["algo_bytes"] == 20.0 * sum(sizes)
            on_cpu, _ = S.run_sgd(cpu, sizes, lm, dm, hy, ins)
            want = S.want_sgd(sizes, lm, dm, hy, ins)
            again, _ = S.run_sgd(hip, sizes, lm, dm, hy, ins)       # the inputs restored, launched once more
            for i in range(len(sizes)):
                what = (i, sizes[i], lr_mult, decay_mult, momentum)
                assert S.same_bits(got[i][1], ins[i][1]), (what, "g was written")
                for k, nm in ((0, "param"), (2, "history")):
                    assert S.same_bits(got[i][k], want[i][k]), (what, nm, "numpy")
                    assert S.same_bits(got[i][k], on_cpu[i][k]), (what, nm, "be=cpu")
                    assert S.same_bits(got[i][k], again[i][k]), (what, nm, "second launch")
            assert len(guards) == 3 * len(sizes) + 1
            for vn, a in guards.items():
                assert np.array_equal(a.view(np.uint32), guard), (vn, "an element outside the tensors changed")


def test_two_calls_new_hyper_no_compile_and_plan(hip, cpu):
    sizes = [9000, 5, 4096]
    lm, dm = [1.0, 2.0, 1.0], [1.0, 0.0, 1.0]
    ins = S.make_inputs(sizes, 3)
    S.run_sgd(hip, sizes, lm, dm, [HYPER], ins)                    # (the kernel is loaded)
    before = rtc_mod.compile_stats()
    steps = [HYPER, (0.5, 0.25, 0.125)]
    got, _ = S.run_sgd(hip, sizes, lm, dm, steps, ins)             # hyper rewritten between the two calls
    after = rtc_mod.compile_stats()
    assert (after["compiled"], after["cache_hits"]) == (before["compiled"], before["cache_hits"])
    want = S.want_sgd(sizes, lm, dm, steps, ins)
    on_cpu, _ = S.run_sgd(cpu, sizes, lm, dm, steps, ins)
    for i in range(len(sizes)):
        for k in (0, 2):
            assert S.same_bits(got[i][k], want[i][k]) and S.same_bits(got[i][k], on_cpu[i][k]), (i, k)
    f = sgd_update_func_op([S.tensor_dims(n, i) for i, n in enumerate(sizes)], lm, dm)
    assert rtc_mod.explain_plan(f, num_cus=hip.get_device_info()["num_cus"]).startswith("bodahip_sgd_update grid=5 ")


def test_same_var_is_refused_on_hip(hip):
    d = Dims.make("float", v=7)
    f = sgd_update_func_op([d])
    from boda_amd.cnn_op import pipe_func_args
    from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo
    hip.compile([RtcFuncInfo("sgd_same", "", [a for a, _ in pipe_func_args(f)], f)])
    made = []
    try:
        for an, _ in pipe_func_args(f):
            hip.create_var_with_dims("sv_" + an, f.get_dims(an)); made.append("sv_" + an)
            hip.copy_nda_to_var("sv_" + an, np.ones(f.get_dims(an).sizes, np.float32))
        with pytest.raises(RtErr, match="args 'w_0' and 'h_0' are the same var 'sv_w_0'"):
            hip.run(RtcFuncCall("sgd_same", {"w_0": RtcArg.var("sv_w_0"), "g_0": RtcArg.var("sv_g_0"), "h_0": RtcArg.var("sv_w_0"), "hyper": RtcArg.var("sv_hyper")}))
        hip.finish_and_sync()
        assert np.all(hip.copy_var_to_nda("sv_w_0") == 1.0)
    finally:
        for vn in made:
            hip.release_var(vn)
        hip.release_func("sgd_same"); hip.release_per_call_id_data()


# ---- the three small pipes
@pytest.mark.parametrize("name", sorted(PIPES))
def test_three_steps_are_numpy_updates(hip, name):
    packed = S.three_steps(hip, name, 32)
    single = S.three_steps(hip, name, 1)
    for vn in packed:
        assert S.same_bits(packed[vn], single[vn]), vn


def test_descent_on_chain(hip):
    l64 = S.descent_f64()
    got = S.descent_run(hip)
    dev = max(abs(a - b) for a, b in zip(got, l64))
    print("descent: float64", ["%.6f" % x for x in l64], "be=hip", ["%.6f" % x for x in got], "max deviation %.3e (bound %.3e)" % (dev, S.DESCENT_BOUND))
    assert got[-1] < got[0]
    assert dev <= S.DESCENT_BOUND, dev


# ---- the step with its update as one graph replay
@pytest.mark.parametrize("name", sorted(PIPES))
def test_graph_replay_with_solver(hip, hip2, name):
    mk_solver = lambda: SgdSolver(lr=0.05, momentum=0.9, weight_decay=5e-4, lr_mult={"biases": 2.0}, decay_mult={"biases": 0.0})
    G, bp = S.make_sgd_driver(hip, name, mk_solver(), seed_in_var=True)
    E, _ = S.make_sgd_driver(hip2, name, mk_solver())
    try:
        state = S.state_vars(bp)
        gets = grad_nodes(bp) + bp.loss_nodes + state
        cp = bp.cp
        rounds = [(SEED_A, 0, None), (SEED_B, 0, 0.02), (SEED_A, 1, None), (SEED_B, 2, 0.1), (SEED_A, 2, None), (SEED_B, 1, 0.01)]
        for parallel, some in ((False, rounds[:3]), (True, rounds[3:])):
            before = S.fetch(hip, state)
            n = G.capture_graph(parallel=parallel)     # (the first: no step has run on G, capture_graph runs one -- without the update calls)
            assert n == len(G.calls()) and G.n_sgd_calls == 1 and G.calls()[-1][0] == "sgd_update_0"
            after = S.fetch(hip, state)
            for vn in state:
                assert S.same_bits(before[vn], after[vn]), ("capture_graph changed", vn, parallel)
            for seed, inp, lr in some:
                if lr is not None:     # between replays: 16 bytes, no new capture
                    G.set_sgd_hyper(lr=lr); E.set_sgd_hyper(lr=lr)
                data, label = small_inputs(cp, inp)
                outs = []
                for d, graph in ((G, True), (E, False)):
                    d.set_det_drop_seed(seed)
                    fwd = {"data": data, "label": label}
                    d.run_bck(["data", "label"], fwd, gets, graph=graph)
                    outs.append(fwd)
                g, e = outs
                for vn in gets:
                    assert S.same_bits(g[vn], e[vn]), (parallel, seed, inp, vn)
                assert not S.same_bits(g[state[0]], before[state[0]])
    finally:
        G.release(); E.release()


# ---- several devices: the replicas stay equal
@pytest.mark.parametrize("B", [3, 5])
def test_three_shards_keep_their_replicas_equal(hip, B):
    """Two steps with the solver on devices=0:0:0, the params fetched (device 0's replica), one more step.  A one-device driver loaded with the fetched params gives that
    step's forward nodes and loss bit for bit -- on every image, so on every shard -- only if the other shards' replicas equal device 0's."""
    multi = make_rtc("(be=hip,devices=0:0:0)"); multi.init()
    try:
        mk, tops, pseed = PIPES["chain"]
        cp = mk(B); bp = add_bck_ops(cp, loss_tops=tops)
        M = ConvPipeBck(multi, solver=SgdSolver(lr=0.05, lr_mult={"biases": 2.0}, decay_mult={"biases": 0.0})); M.init(bp, small_params(cp, pseed))
        fwd_nodes = [n for n in cp.nodes if n != "data"] + bp.loss_nodes
        try:
            for k in range(2):
                data, label = small_inputs(cp, 30 + k)
                M.set_det_drop_seed(SEED_A + k)
                M.run_bck(["data", "label"], {"data": data, "label": label}, [])
            params = S.fetch(multi, list(cp.params))
            assert all(not S.same_bits(params[p], small_params(cp, pseed)[p]) for p in cp.params)
            data, label = small_inputs(cp, 32)
            M.set_det_drop_seed(SEED_B)
            many = {"data": data, "label": label}
            M.run_bck(["data", "label"], many, fwd_nodes)
        finally:
            M.release()
        One = ConvPipeBck(hip); One.init(add_bck_ops(cp, loss_tops=tops), params)
        try:
            One.set_det_drop_seed(SEED_B)
            one = {"data": data, "label": label}
            One.run_bck(["data", "label"], one, fwd_nodes)
        finally:
            One.release()
        for vn in fwd_nodes:
            assert S.same_bits(many[vn], one[vn]), vn
        with pytest.raises(RtErr, match="is sharded over the devices"):     # a tensor with a leading img dim is a sharded var there
            S.run_sgd(multi, [12], [1.0], [1.0], [HYPER], S.make_inputs([12]), dims=[Dims.make("float", img=3, v=4)])
    finally:
        multi.close()


# ---- one real net
def test_nin_two_images_one_step(hip):
    cp = nin_imagenet(2); bp = add_bck_ops(cp)
    solver = SgdSolver(lr=0.01, momentum=0.9, weight_decay=5e-4, lr_mult={"biases": 2.0}, decay_mult={"biases": 0.0})
    drv = ConvPipeBck(hip, solver=solver); drv.init(bp, host_params(bp, 5))
    try:
        assert len(cp.params) == 24 and drv.n_sgd_calls == 1
        for p, d in cp.params.items():     # a history that is not zero
            hip.copy_nda_to_var(p + SGD_HIST_SFX, np.random.default_rng([9, d.dims_prod()]).uniform(-1e-3, 1e-3, d.sizes).astype(np.float32))
        rng = np.random.default_rng(0)
        data = rng.uniform(-1, 1, cp.nodes["data"].sizes).astype(np.float32)
        label = np.array([3, 998], np.float32).reshape(2, 1, 1)
        before = S.fetch(hip, S.state_vars(bp))
        after, fwd = S.check_step_is_numpy_update(hip, drv, bp, before, [0.01, 0.9, 5e-4], data=data, label=label, seed=5)
        assert np.isfinite(fwd["loss"].item()) and all(np.all(np.isfinite(a)) for a in after.values())
        upd = [ms for t, fn, ms in drv.per_call_ms if fn == "hip_sgd_update"]
        print("NiN, 2 images: the update of 24 tensors as one call: %.1f us" % (1e3 * upd[0]))
    finally:
        drv.release()
