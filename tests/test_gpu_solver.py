"""The solver family on the MI355X: bodahip_solver_update_{sgd,nesterov,adam}, bodahip_grad_sumsq and bodahip_grad_norm (kernels/solver_update_f32.hip) bit for bit
against be=cpu and the numpy twins of their written chains (tests/solver_ref.py), and ConvPipeBck(solver=Solver(...)) on be=hip -- eager, as hipGraph replays, on three
shards of device 0, with a BatchNorm pipe, and the two descent runs.

Every comparison is on the uint32 views, except where the twin yields NaN (the backend must yield NaN, payloads are not compared).  The update has no pure output, so the
check that nothing else is written is a guard var behind every tensor var.  The descent bounds are the ones tests/solver_ref.py writes down."""
import numpy as np
import pytest

import sgd_ref as S
import solver_ref as V
from boda_amd.bck_pipe import SOLVER_HYPER_VAR, SOLVER_STATE_VAR, ConvPipeBck, LrPolicy, Solver, add_bck_ops
from boda_amd.rtc import make_rtc

from test_bck_pipe_cpu import PIPES, SEED_A, SEED_B, grad_nodes, small_inputs, small_params
from test_solver_cpu import BIG, CASES, HYPERS, STATE, mk_solver, mults, norm_case, test_cpu_batchnorm_pipe_with_adam as batchnorm_pipe_with_adam

pytestmark = pytest.mark.gpu
F = np.float32


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


# ---- 1. the update function
@pytest.mark.parametrize("form", V.FORMS, ids=V.form_id)
def test_update_against_cpu_and_numpy(hip, cpu, form):
    guard = np.full(4, V.GUARD_BITS, np.uint32)
    for sizes in CASES:
        lm, dm = mults(len(sizes))
        ins = V.make_inputs(sizes)
        keep = []
        got, guards = V.run_update(hip, sizes, form, lm, dm, HYPERS, ins, STATE, guards=True, keep=keep)
        assert keep[0]["kernel"] == "bodahip_solver_update_" + form[0] and keep[0]["kernels"] == 1 and keep[0]["grid"] == sum(-(-n // 4096) for n in sizes)
        assert keep[0]["algo_bytes"] == (28.0 if form[0] == "adam" else 20.0) * sum(sizes)
        on_cpu, _ = V.run_update(cpu, sizes, form, lm, dm, HYPERS, ins, STATE)
        want = V.want_update(form, lm, dm, HYPERS, ins, STATE)
        for i in range(len(sizes)):
            what = (form, i, sizes[i])
            assert V.same_bits(got[i][1], ins[i][1]) and np.array_equal(np.isnan(got[i][1]), np.isnan(ins[i][1])), (what, "g was written")
            for k, nm in ((2, "history"), (3, "second history"), (0, "param")):
                assert V.same_bits(got[i][k], want[i][k]), (what, nm, "numpy")
                assert V.same_bits(got[i][k], on_cpu[i][k]) and V.same_bits(on_cpu[i][k], got[i][k]), (what, nm, "be=cpu")
        assert len(guards) == (4 if form[0] == "adam" else 3) * len(sizes) + 2
        for vn, a in guards.items():
            assert np.array_equal(a.view(np.uint32), guard), (vn, "an element outside the tensors changed")


def test_sgd_form_leaves_hip_sgd_update_s_bits(hip):
    for sizes in CASES:
        lm, dm = mults(len(sizes))
        ins = V.make_inputs(sizes)
        got, _ = V.run_update(hip, sizes, ("sgd", False, False), lm, dm, HYPERS, ins, STATE)
        old, _ = S.run_sgd(hip, sizes, lm, dm, [tuple(h[:3]) for h in HYPERS], [t[:3] for t in ins])
        for i in range(len(sizes)):
            for k in (0, 2):
                assert V.same_bits(got[i][k], old[i][k]) and V.same_bits(old[i][k], got[i][k]), (sizes[i], k)


# ---- 2. the norm
@pytest.mark.parametrize("kind,clip", [("plain", 1e6), ("plain", 1.0), ("zero", 1.0), ("nan", 1.0), ("inf", 1.0)], ids=lambda x: str(x))
def test_norm_against_cpu_and_numpy(hip, cpu, kind, clip):
    keep = []
    (seen, state), (wseen, wstate), (ca, cb, total) = norm_case(hip, kind, clip, keep)
    (cseen, cstate), _, _ = norm_case(cpu, kind, clip)
    assert [k["kernel"] for k in keep] == ["bodahip_grad_sumsq"] * 2 and [k["grid"] for k in keep] == [cb, ca]
    for s, w, c in zip(seen, wseen, cseen):
        assert V.same_bits(s, w) and V.same_bits(s, c)
    assert np.all(seen[0][:2 + ca] == 0.5) and seen[0][-1] == 0.5 and np.all(seen[1][[0, 1, -1]] == 0.5)     # slots outside a call's range are untouched
    assert V.same_bits(state, wstate) and V.same_bits(state, cstate), (state, wstate, cstate)


def test_norm_three_four_five_and_big(hip):
    g = np.array([3.0, 4.0], F)
    (seen,), state = V.run_norm(hip, [(0, [g])], 1, np.zeros(1, F), 5.0)
    assert seen[0] == 25.0 and list(state) == [1.0, 5.0, 25.0, 0.0]     # norm == clip: coef is 1
    big = np.random.default_rng(3).uniform(-1, 1, BIG).astype(F)
    (seen,), state = V.run_norm(hip, [(0, [big])], 258, np.zeros(258, F), 10.0)
    (wseen,), wstate = V.want_norm([(0, [big])], np.zeros(258, F), 10.0)
    assert seen.size == 258 and V.same_bits(seen, wseen) and V.same_bits(state, wstate)


# ---- 4. the driver
@pytest.mark.parametrize("form", V.FORMS, ids=V.form_id)
@pytest.mark.parametrize("name", ["chain", "fan"])
def test_three_steps_are_the_twins(hip, name, form):
    packed = V.three_steps(hip, name, mk_solver(form, 32))
    three = V.three_steps(hip, name, mk_solver(form, 3))
    for vn in packed:
        assert V.same_bits(packed[vn], three[vn]), vn


def test_step_policy_boundary_inside_the_three_steps(hip):
    V.three_steps(hip, "chain", mk_solver(("adam", True, False), policy=LrPolicy(policy="step", gamma=0.5, stepsize=2)))


def test_batchnorm_pipe_with_adam(hip):
    batchnorm_pipe_with_adam(hip)


# ---- 5. graph and devices
@pytest.mark.parametrize("name", ["chain", "fan"])
def test_graph_replays_with_adam_and_clipping(hip, hip2, name):
    """Three replays per capture (serial, then parallel=True) leave the eager step's bits in every var; iter and corr advance between replays."""
    mk = lambda: Solver(type="adam", lr=0.01, clip_gradients=0.05, lr_policy=LrPolicy(policy="step", gamma=0.5, stepsize=4), lr_mult={"biases": 2.0}, decay_mult={"biases": 0.0})
    G, bp = V.make_driver(hip, name, mk(), seed_in_var=True)
    E, _ = V.make_driver(hip2, name, mk())
    try:
        state = V.state_vars(G) + [SOLVER_HYPER_VAR, SOLVER_STATE_VAR]
        gets = grad_nodes(bp) + bp.loss_nodes + state
        rounds = [(SEED_A, 0), (SEED_B, 0), (SEED_A, 1), (SEED_B, 2), (SEED_A, 2), (SEED_B, 1)]
        corrs = []
        for parallel, some in ((False, rounds[:3]), (True, rounds[3:])):
            before = V.fetch(hip, state)
            n = G.capture_graph(parallel=parallel)     # (the first: no step has run on G, capture_graph runs one -- without the solver's calls)
            assert n == len(G.calls()) and G.n_sgd_calls == 3 and [t for t, _, _ in G.calls()][-3:] == ["grad_sumsq_0", "grad_norm", "solver_update_0"]
            after = V.fetch(hip, state)
            for vn in state:
                assert V.same_bits(before[vn], after[vn]), ("capture_graph changed", vn, parallel)
            for seed, inp in some:
                data, label = small_inputs(bp.cp, inp)
                outs = []
                for d, graph in ((G, True), (E, False)):
                    d.set_det_drop_seed(seed)
                    fwd = {"data": data, "label": label}
                    d.run_bck(["data", "label"], fwd, gets, graph=graph)
                    outs.append(fwd)
                g, e = outs
                assert G.iter == E.iter == len(corrs) + 1
                for vn in gets:
                    assert V.same_bits(g[vn], e[vn]), (parallel, seed, inp, vn)
                assert V.same_bits(g[SOLVER_HYPER_VAR], V.want_hyper(G.solver, G.iter - 1))
                corrs.append(float(g[SOLVER_HYPER_VAR][5]))
                assert not V.same_bits(g[state[0]], before[state[0]])
        assert len(set(corrs)) == 6     # corr moves with t at every replay
    finally:
        G.release(); E.release()


@pytest.mark.parametrize("B", [3, 5])
def test_three_shards_keep_their_replicas_equal(hip, B):
    """Two adam steps with clipping on devices=0:0:0, the params fetched (device 0's replica), one more step.  A one-device driver loaded with the fetched params gives
    that step's forward nodes and loss bit for bit -- on every image, so on every shard -- only if the other shards' replicas equal device 0's."""
    multi = make_rtc("(be=hip,devices=0:0:0)"); multi.init()
    try:
        mk, tops, pseed = PIPES["chain"]
        cp = mk(B); bp = add_bck_ops(cp, loss_tops=tops)
        M = ConvPipeBck(multi, solver=Solver(type="adam", lr=0.01, clip_gradients=0.05, lr_mult={"biases": 2.0}, decay_mult={"biases": 0.0})); M.init(bp, small_params(cp, pseed))
        fwd_nodes = [n for n in cp.nodes if n != "data"] + bp.loss_nodes
        try:
            for k in range(2):
                data, label = small_inputs(cp, 30 + k)
                M.set_det_drop_seed(SEED_A + k)
                M.run_bck(["data", "label"], {"data": data, "label": label}, [])
            params = V.fetch(multi, list(cp.params))
            assert all(not V.same_bits(params[p], small_params(cp, pseed)[p]) for p in cp.params)
            st = multi.copy_var_to_nda(SOLVER_STATE_VAR)
            assert st[1] > 0.05 and 0 < st[0] < 1     # the clipping was at work
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
    finally:
        multi.close()


# ---- 6. descent
@pytest.mark.parametrize("which", sorted(V.DESCENT))
def test_descent_on_chain(hip, which):
    l64 = V.descent_f64(which)
    got = V.descent_run(hip, which)
    dev = max(abs(a - b) for a, b in zip(got, l64))
    print(which, "descent: float64", ["%.6f" % x for x in l64], "be=hip", ["%.6f" % x for x in got], "max deviation %.3e (bound %.3e)" % (dev, V.DESCENT_BOUND[which]))
    assert got[-1] < got[0]
    assert dev <= V.DESCENT_BOUND[which], dev
