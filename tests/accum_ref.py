"""What the gradient-accumulation tests share (tests/test_accum_cpu.py, tests/test_gpu_accum.py): the numpy twins of hip_grad_accum and hip_solver_update_acc (one numpy
operation per fp32 rounding; csrc/kernels/solver_update_f32.hip and DESIGN.md section 3.19 state the chains), built on tests/solver_ref.py's twins; a runner that rewrites
vars between the calls of one function; the op-level checks, which take the backend as an argument; and the passes of a ConvPipeBck(iter_size=n) held to the twins on the
backend's own recorded gradients.

Equality is solver_ref.same_bits: the uint32 views, except that where the twin yields NaN the backend must yield NaN."""
import numpy as np

import sgd_ref as S
import solver_ref as V
from boda_amd.bck_pipe import GRAD_ACC_SFX, SGD_HIST2_SFX, SGD_HIST_SFX, SOLVER_ACCUM_VAR, SOLVER_HYPER_VAR, SOLVER_PARTS_VAR, SOLVER_STATE_VAR, ConvPipeBck, Solver, add_bck_ops
from boda_amd.cnn_op import grad_accum_func_op, pipe_func_args, solver_update_acc_func_op
from boda_amd.op import Dims
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo

from test_bck_pipe_cpu import fan, small_inputs, small_params

F = np.float32
GUARD_BITS = S.GUARD_BITS
THIRD = F(1.0 / 3.0)


def words(first, apply, scale, micro=0):
    """solver_accum: [first, apply, scale, micro]."""
    return np.array([first, apply, scale, micro], F)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the twins
def accum_np(accum, g, a):
    """hip_grad_accum: accum[0] != 0: a' = g (a is not looked at); else a' = a + g, one fp32 add."""
    g = np.asarray(g, F)
    if accum[0] != 0:
        return g.copy()
    with np.errstate(all="ignore"):
        r = np.asarray(a, F) + g
    assert r.dtype == F
    return r


def update_acc_np(solver_type, w, g, h, h2, hyper, accum, lr_mult=1.0, decay_mult=1.0, clip=False, coef=1.0, decoupled_wd=False):
    """hip_solver_update_acc: accum[1] == 0: nothing changes.  Otherwise g0 = clip ? coef * g : g; gs = accum[2] * g0 (one rounding); solver_ref.solver_np's chain on gs."""
    if accum[1] == 0:
        return np.asarray(w, F), np.asarray(h, F), h2
    with np.errstate(all="ignore"):
        g0 = F(coef) * np.asarray(g, F) if clip else np.asarray(g, F)
        gs = F(accum[2]) * g0
    assert gs.dtype == F
    return V.solver_np(solver_type, w, gs, h, h2, hyper, lr_mult, decay_mult, False, 1.0, decoupled_wd)


# ---- a bare function, its vars rewritten between the calls
def run_steps(rtc, name, fop, vals, steps, guards=True, keep=None):
    """Compile `fop`, create one var per var arg (the op's dims) and, with guards, a 4-float guard var behind each; upload `vals` {arg: array}; then per entry of `steps`
    ({arg: array}) upload it and run the call once -> ([{arg: array fetched} after each call], {guard var: array} at the end)."""
    spec = [(an, io) for an, io in pipe_func_args(fop) if io in ("IN", "OUT", "INOUT")]
    rtc.compile([RtcFuncInfo(name, "", [a for a, _ in spec], fop)])
    made, am = [], {}
    guard = np.full(4, GUARD_BITS, np.uint32).view(F)
    up = lambda an, a: rtc.copy_nda_to_var(f"{name}_{an}", np.ascontiguousarray(a, F).reshape(fop.get_dims(an).sizes))
    try:
        for an, _ in spec:
            vn = f"{name}_{an}"
            rtc.create_var_with_dims(vn, fop.get_dims(an)); made.append(vn); am[an] = RtcArg.var(vn)
            if guards:
                rtc.create_var_with_dims(vn + "_guard", Dims.make("float", v=4)); made.append(vn + "_guard")
                rtc.copy_nda_to_var(vn + "_guard", guard)
        for an, a in vals.items():
            up(an, a)
        call = RtcFuncCall(name, am)
        seen = []
        for st in steps:
            for an, a in st.items():
                up(an, a)
            rtc.run(call); rtc.finish_and_sync()
            if keep is not None:
                keep.append(rtc.last_launch() if rtc.be == "hip" else {})
            seen.append({an: rtc.copy_var_to_nda(f"{name}_{an}").reshape(-1) for an, _ in spec})
        gv = {vn: rtc.copy_var_to_nda(vn) for vn in made if vn.endswith("_guard")}
        return seen, gv
    finally:
        for vn in made:
            rtc.release_var(vn)
        rtc.release_func(name); rtc.release_per_call_id_data()


def guards_intact(gv, n):
    assert len(gv) == n, (len(gv), n)
    for vn, a in gv.items():
        assert np.array_equal(a.view(np.uint32), np.full(4, GUARD_BITS, np.uint32)), (vn, "an element outside the tensors changed")


# ---- hip_grad_accum
ACCUM_CASES = [[n] for n in S.SIZES] + [S.MIXED_32]


def grads3(sizes, seed=0):
    """Three gradients per tensor, values of both signs with exact zeros of both signs (sgd_ref.make_inputs' w, g, h serve as the three)."""
    return S.make_inputs(sizes, seed)


def check_accum_three_calls(rtc, sizes):
    """first, add, add with the words and the gradients rewritten in between; the accumulators start as the payload NaN 0x7FC0BEEF, so `first` must not read them."""
    fop = grad_accum_func_op([S.tensor_dims(n, i) for i, n in enumerate(sizes)])
    gs = grads3(sizes)
    nan_fill = lambda n: np.full(n, GUARD_BITS, np.uint32).view(F)
    vals = {f"a_{i}": nan_fill(n) for i, n in enumerate(sizes)}
    accs = [words(1, 0, THIRD, 0), words(0, 0, THIRD, 1), words(0, 1, THIRD, 2)]
    steps = [dict({f"g_{i}": gs[i][k] for i in range(len(sizes))}, accum=accs[k]) for k in range(3)]
    keep = []
    seen, gv = run_steps(rtc, "gacc", fop, vals, steps, keep=keep)
    want = [nan_fill(n) for n in sizes]
    for k in range(3):
        for i, n in enumerate(sizes):
            want[i] = accum_np(accs[k], gs[i][k], want[i])
            assert bits_equal(seen[k][f"g_{i}"], gs[i][k].reshape(-1)), (k, i, n, "g was written")
            assert V.same_bits(seen[k][f"a_{i}"], want[i]), (k, i, n)
            if k == 0:
                assert bits_equal(seen[0][f"a_{i}"], gs[i][0].reshape(-1)), (i, n, "first: the bits of g")
        assert bits_equal(seen[k]["accum"], accs[k]), "accum was written"
    guards_intact(gv, 2 * len(sizes) + 1)
    return keep


def special_pairs():
    """(a, g) of 4097 + 5 elements in two tensors: special pairs in a chunk's quads, in the one-element second chunk of the first tensor and in the scalar tail of the second."""
    tiny = np.float32(1e-40)     # a denormal
    pairs = [(tiny, np.float32(2e-40)), (tiny, -tiny), (np.float32(1.2e-38), np.float32(-1.1e-38)),     # denormal sums; a normal pair whose sum is a denormal
             (F(0.0), F(-0.0)), (F(-0.0), F(-0.0)), (F(np.inf), F(-np.inf)), (F(np.inf), F(1.0)), (F(1.0), F(np.nan)), (F(3.0e38), F(3.0e38))]
    rng = np.random.default_rng(5)
    out = []
    for n, at in ((4097, list(range(len(pairs))) + [4096]), (5, [4, 0, 1, 2, 3])):
        a = rng.uniform(-1, 1, n).astype(F); g = rng.uniform(-1, 1, n).astype(F)
        for j, e in enumerate(at):
            a[e], g[e] = pairs[j % len(pairs)] if e != 4096 else pairs[0]
        out.append((a, g))
    return out


def check_accum_special_values(rtc):
    pr = special_pairs()
    fop = grad_accum_func_op([Dims.make("float", v=a.size) for a, _ in pr])
    vals = {}
    for i, (a, g) in enumerate(pr):
        vals.update({f"a_{i}": a, f"g_{i}": g})
    (seen,), gv = run_steps(rtc, "gacs", fop, vals, [{"accum": words(0, 1, 1, 1)}])
    for i, (a, g) in enumerate(pr):
        want = accum_np(words(0, 1, 1, 1), g, a)
        assert V.same_bits(seen[f"a_{i}"], want), i
    (a, g), want = pr[0], accum_np(words(0, 1, 1, 1), pr[0][1], pr[0][0])
    tiny = np.finfo(F).tiny
    assert 0 < want[0] < tiny and want[1] == 0 and 0 < want[2] < tiny and 0 < want[4096] < tiny     # denormal sums are kept
    assert want[3] == 0 and not np.signbit(want[3]) and want[4] == 0 and np.signbit(want[4])          # +0 + -0 = +0;  -0 + -0 = -0
    assert np.isnan(want[5]) and np.isinf(want[6]) and np.isnan(want[7]) and np.isinf(want[8])         # Inf + -Inf, NaN in g, overflow
    guards_intact(gv, 5)


# ---- hip_solver_update_acc
UPDATE_CASES = [[4097], [9000, 15], S.MIXED_32]
HYPER = V.hyper8(0.01, 0.9, 5e-4, 0.999, 1e-8, V.corr_f64(0.9, 0.999, 2))
STATE = np.array([0.37, 9.0, 81.0, 0.0], F)


def update_acc_fop(sizes, form, lm, dm):
    t, clip, dwd = form
    return solver_update_acc_func_op([S.tensor_dims(n, i) for i, n in enumerate(sizes)], t, lm, dm, clip=clip, decoupled_wd=dwd)


def check_update_acc(rtc, sizes, form):
    """apply = 0 leaves everything; apply = 1 with scale 1 leaves hip_solver_update's bits; scale 0.25 and fp32(1/3) leave the twin's.  Every run starts from the same inputs."""
    t, clip, dwd = form
    lm, dm = [float(1 + i % 2) for i in range(len(sizes))], [float((i + 1) % 2) for i in range(len(sizes))]
    ins = V.make_inputs(sizes)
    fop = update_acc_fop(sizes, form, lm, dm)
    vals = {"state": STATE, "hyper": HYPER}
    for i, (w, g, h, h2) in enumerate(ins):
        vals.update({f"w_{i}": w, f"g_{i}": g, f"h_{i}": h})
        if t == "adam":
            vals[f"h2_{i}"] = h2
    per = 4 if t == "adam" else 3
    plain, _ = V.run_update(rtc, sizes, form, lm, dm, [HYPER], ins, STATE)
    keeps = []
    for acc in (words(0, 0, 1, 1), words(0, 1, 1, 2), words(1, 1, 0.25, 0), words(0, 1, THIRD, 2), words(0, -1, 1, 0)):
        keep = []
        (seen,), gv = run_steps(rtc, "slva", fop, vals, [{"accum": acc}], keep=keep)
        keeps += keep
        for i, (w, g, h, h2) in enumerate(ins):
            w2, hn, vn = update_acc_np(t, w, g, h, h2, HYPER, acc, lm[i], dm[i], clip, STATE[0], dwd)
            what = (form, list(acc), i, sizes[i])
            assert V.same_bits(seen[f"g_{i}"], g) and np.array_equal(np.isnan(seen[f"g_{i}"]), np.isnan(g.reshape(-1))), (what, "g was written")
            if acc[1] == 0:     # nothing is written: the very bits that went in
                assert bits_equal(seen[f"w_{i}"], w.reshape(-1)) and bits_equal(seen[f"h_{i}"], h.reshape(-1)), what
                assert t != "adam" or bits_equal(seen[f"h2_{i}"], h2.reshape(-1)), what
                continue
            assert V.same_bits(seen[f"w_{i}"], w2) and V.same_bits(seen[f"h_{i}"], hn), what
            assert t != "adam" or V.same_bits(seen[f"h2_{i}"], vn), what
            if acc[2] == 1:     # hip_solver_update's bits on the same inputs
                assert V.same_bits(seen[f"w_{i}"], plain[i][0]) and V.same_bits(plain[i][0], seen[f"w_{i}"]) and V.same_bits(seen[f"h_{i}"], plain[i][2]), (what, "hip_solver_update")
                assert t != "adam" or (V.same_bits(seen[f"h2_{i}"], plain[i][3]) and V.same_bits(plain[i][3], seen[f"h2_{i}"])), (what, "hip_solver_update")
        for an, a in (("hyper", HYPER), ("state", STATE), ("accum", acc)):
            assert bits_equal(seen[an], a), (an, "was written")
        guards_intact(gv, per * len(sizes) + 3)
    return keeps


# ---- the driver
MULTS = dict(lr_mult={"biases": 2.0}, decay_mult={"biases": 0.0})


def mk_solver(form, per_call=32, policy=None, lr=0.05):
    t, clip, dwd = form
    return Solver(type=t, lr=lr, momentum=0.9, weight_decay=5e-4, decoupled_wd=dwd, clip_gradients=0.05 if clip else 0.0, lr_policy=policy, tensors_per_call=per_call, **MULTS)


def expected_tags(drv):
    per = drv.solver.tensors_per_call
    groups = -(-len(drv.sgd_params) // per)
    clip = drv.solver.clip_gradients > 0
    return [f"grad_accum_{k}" for k in range(groups)] + ([f"grad_sumsq_{k}" for k in range(groups)] + ["grad_norm"] if clip else []) + [f"solver_update_{k}" for k in range(groups)]


def passes(rtc, drv, bp, n_passes, graph=False, inputs=small_inputs, record=None):
    """n_passes micro-steps of a driver with iter_size > 1 (new inputs and a new dropout seed each), every one held to the twins on the backend's own recorded gradients:
    the uploaded words; the accumulators = the sequential fp32 sums of the recorded gradients in micro order; solver_state = the norm of the accumulators as they stand;
    params and histories untouched unless the pass applies, and then the twin's; iter counts updates.  record: a list that gets every var's bytes after each pass."""
    sv, n = drv.solver, drv.iter_size
    clip = sv.clip_gradients > 0
    names = list(drv.sgd_params) + [p + SGD_HIST_SFX for p in drv.sgd_params] + ([p + SGD_HIST2_SFX for p in drv.sgd_params] if sv.type == "adam" else [])
    state = V.fetch(rtc, names)
    sums = {}
    for k in range(n_passes):
        micro, it = drv.micro, drv.iter
        assert micro == k % n
        data, label = inputs(bp.cp, k)
        drv.set_det_drop_seed(1000 + k)
        fwd = {"data": data, "label": label}
        drv.run_bck(["data", "label"], fwd, [p + "_grad_loss" for p in drv.sgd_params] + bp.loss_nodes, graph=graph)
        acc = words(micro == 0, micro == n - 1, F(1.0 / n), micro)
        hyper = V.want_hyper(sv, it)
        assert bits_equal(rtc.copy_var_to_nda(SOLVER_ACCUM_VAR).reshape(-1), acc), (k, "the uploaded accum words")
        assert V.same_bits(rtc.copy_var_to_nda(SOLVER_HYPER_VAR), hyper), (k, "the uploaded hyper words")
        for p in drv.sgd_params:
            g = fwd[p + "_grad_loss"]
            sums[p] = accum_np(acc, g, sums.get(p))
            assert V.same_bits(rtc.copy_var_to_nda(p + GRAD_ACC_SFX), sums[p]), (k, p, "accumulator")
            assert bits_equal(rtc.copy_var_to_nda(p + "_grad_loss"), g)
        coef = 1.0
        if clip:     # (on a pass that does not apply: the norm of the partial sums, computed and not used)
            parts = V.partials_np([sums[p] for p in drv.sgd_params])
            want_state = V.norm_np(parts, hyper[6])
            assert V.same_bits(rtc.copy_var_to_nda(SOLVER_PARTS_VAR), parts), (k, "partials")
            assert V.same_bits(rtc.copy_var_to_nda(SOLVER_STATE_VAR), want_state), (k, "solver_state")
            coef = want_state[0]
        after = V.fetch(rtc, names)
        if micro != n - 1:
            assert drv.iter == it
            for vn in names:
                assert bits_equal(after[vn], state[vn]), (k, vn, "changed on a pass that does not apply")
        else:
            assert drv.iter == it + 1
            for p in drv.sgd_params:
                w2, hn, vn = update_acc_np(sv.type, state[p], sums[p], state[p + SGD_HIST_SFX], state.get(p + SGD_HIST2_SFX), hyper, acc, sv.mult_of(sv.lr_mult, p),
                                           sv.mult_of(sv.decay_mult, p), clip, coef, sv.decoupled_wd)
                assert V.same_bits(after[p + SGD_HIST_SFX], hn), (k, p, "history")
                assert sv.type != "adam" or V.same_bits(after[p + SGD_HIST2_SFX], vn), (k, p, "second history")
                assert V.same_bits(after[p], w2), (k, p, "param")
                assert not V.same_bits(after[p], state[p]), (k, p, "the update changed nothing")
        state = after
        if record is not None:
            record.append({vn: rtc.copy_var_to_nda(vn).tobytes() for vn in drv.vars})
    return state


def six_passes(rtc, name, solver, graph=None, record=None, **kw):
    """Six passes of a small pipe with iter_size=3: two updates.  graph: None eager | False one serial capture | True one parallel capture, replayed six times."""
    drv, bp = V.make_driver(rtc, name, solver, iter_size=3, **kw)
    try:
        assert [t for t, _, _ in drv.calls()][-drv.n_sgd_calls:] == expected_tags(drv)
        if graph is not None:
            assert drv.capture_graph(parallel=graph) == len(drv.calls())
            assert drv.micro == 0 and drv.iter == 0
        state = passes(rtc, drv, bp, 6, graph=graph is not None, record=record)
        assert drv.iter == 2 and drv.micro == 0
        return state
    finally:
        drv.release()


# ---- meaning: one sgd step at batch 2b against iter_size=2 at batch b fed the two halves, on `fan` (no BatchNorm, dropout or LRN: the images are independent).  The loss
# gradient is the per-image mean, so the whole batch's gradient is half the sum of the halves' and the two updates agree up to rounding.
# The figure: max over the params of max|w_whole - w_halves| / max|w_whole|.  be=cpu measures MEANING_DEV_CPU; be=hip is held to ten times it, the factor being for the GPU's
# K-slice order in the filter gradients (as the descent runs of DESIGN.md section 3.18).
MEANING_DEV_CPU = 4.799e-08     # be=cpu measures 4.798e-08 (fan at batch 4 against two halves of 2, data seed 77): held by tests/test_accum_cpu.py
MEANING_BOUND = 10 * MEANING_DEV_CPU
MEANING_B = 2


def meaning_dev(rtc):
    sv = lambda: Solver(type="sgd", lr=0.05, momentum=0.9, weight_decay=5e-4, **MULTS)
    cp2 = fan(2 * MEANING_B); data, label = small_inputs(cp2, 77)
    params = small_params(cp2, 0)
    whole = ConvPipeBck(rtc, solver=sv()); whole.init(add_bck_ops(cp2), params)
    try:
        whole.run_bck(["data", "label"], {"data": data, "label": label}, [])
        a = V.fetch(rtc, list(cp2.params))
    finally:
        whole.release()
    cp1 = fan(MEANING_B)
    halves = ConvPipeBck(rtc, solver=sv(), iter_size=2); halves.init(add_bck_ops(cp1), params)
    try:
        for k in range(2):
            sl = slice(k * MEANING_B, (k + 1) * MEANING_B)
            halves.run_bck(["data", "label"], {"data": np.ascontiguousarray(data[sl]), "label": np.ascontiguousarray(label[sl])}, [])
        assert halves.iter == 1
        b = V.fetch(rtc, list(cp1.params))
    finally:
        halves.release()
    assert all(not V.same_bits(a[p], params[p]) for p in a)
    return max(float(np.max(np.abs(a[p].astype(np.float64) - b[p])) / np.max(np.abs(a[p]))) for p in a)
