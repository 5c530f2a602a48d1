"""What the solver tests share (tests/test_solver_cpu.py, tests/test_gpu_solver.py): the numpy twins of hip_solver_update, hip_grad_sumsq and hip_grad_norm, one numpy
operation per fp32 rounding (csrc/kernels/solver_update_f32.hip states the chains and the tree), inputs with special values, runners for the bare functions, the per-step
check of a ConvPipeBck with a Solver, and the descent runs on `chain` with their float64 trajectories.

Equality is np.array_equal on the uint32 views -- except where the twin yields NaN: there the backend must yield NaN too, and payloads are not compared."""
import numpy as np

import bck_pipe_ref as ref
import sgd_ref as S
from boda_amd.bck_pipe import (SGD_HIST2_SFX, SGD_HIST_SFX, SOLVER_HYPER_VAR, SOLVER_PARTS_VAR, SOLVER_STATE_VAR, ConvPipeBck, LrPolicy, Solver, add_bck_ops)
from boda_amd.cnn_op import grad_norm_func_op, grad_sumsq_func_op, pipe_func_args, solver_update_func_op
from boda_amd.op import Dims
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo

from test_bck_pipe_cpu import PIPES, drop_seeds, small_inputs, small_params

F = np.float32
CHUNK = 4096
GUARD_BITS = S.GUARD_BITS
TYPES = ("sgd", "nesterov", "adam")
# (solver_type, clip, decoupled_wd): each type with clipping off and on, adam also with the decoupled decay
FORMS = [(t, c, False) for t in TYPES for c in (False, True)] + [("adam", c, True) for c in (False, True)]
form_id = lambda f: f"{f[0]}{'_clip' if f[1] else ''}{'_dwd' if f[2] else ''}"


def same_bits(a, b):
    """a: the backend's, b: the twin's.  Bit for bit, except that where the twin is NaN the backend must be NaN (any payload)."""
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    if not (a.dtype == b.dtype == F and a.shape == b.shape):
        return False
    nan = np.isnan(b)
    return bool(np.all(np.isnan(a[nan])) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32)))


def corr_f64(momentum, momentum2, t):
    """sqrt(1 - momentum2^t) / (1 - momentum^t) in float64 from the fp32 values of the two momenta; the device gets it rounded to fp32 once."""
    m1, m2 = float(F(momentum)), float(F(momentum2))
    return float(np.sqrt(1.0 - m2 ** t) / (1.0 - m1 ** t))


def hyper8(lr, momentum=0.9, weight_decay=5e-4, momentum2=0.999, delta=1e-8, corr=1.0, clip=0.0):
    return np.array([lr, momentum, weight_decay, momentum2, delta, corr, clip, 0.0], F)


# ---- the update
def solver_np(solver_type, w, g, h, h2, hyper, lr_mult=1.0, decay_mult=1.0, clip=False, coef=1.0, decoupled_wd=False):
    """-> (w', h', h2') float32 (h2' is h2 unless adam), every numpy operation one rounding.  hyper: the eight fp32 words."""
    with np.errstate(all="ignore"):
        w, g, h = (np.asarray(a, F) for a in (w, g, h))
        lr, mom, wd, mom2, delta, corr = (F(x) for x in hyper[:6])
        lr_i = lr * F(lr_mult)
        wd_i = wd * F(decay_mult)
        g0 = F(coef) * g if clip else g
        if solver_type == "adam":
            h2 = np.asarray(h2, F)
            if decoupled_wd:
                g1 = g0
            else:
                reg = wd_i * w
                g1 = g0 + reg
            o1 = F(1.0) - mom
            o2 = F(1.0) - mom2
            ma = mom * h
            mb = o1 * g1
            m = ma + mb
            q = g1 * g1
            va = mom2 * h2
            vb = o2 * q
            v = va + vb
            sq = np.sqrt(v)
            d = sq + delta
            r = m / d
            s = lr_i * corr
            u = s * r
            if decoupled_wd:
                lrwd = lr_i * wd_i
                dw = lrwd * w
                u = u + dw
            w2 = w - u
            assert all(x.dtype == F for x in (w2, m, v))
            return w2, m, v
        reg = wd_i * w
        g1 = g0 + reg
        a = mom * h
        b = lr_i * g1
        hn = a + b
        if solver_type == "nesterov":
            c = F(1.0) + mom
            u = c * hn
            u = u - a
            w2 = w - u
        else:
            assert solver_type == "sgd"
            w2 = w - hn
        assert w2.dtype == F and hn.dtype == F
        return w2, hn, h2


# ---- the sum of squares and the norm
def tree_np(a):
    """THE TREE over lane sums a[..., 256]: for h = 128 .. 1: a[t] = a[t] + a[t + h], t < h -> a[..., 0]."""
    a = np.array(a, F)
    h = 128
    while h:
        a[..., :h] = a[..., :h] + a[..., h:2 * h]
        h //= 2
    return a[..., 0]


def lanes_np(x, square):
    """x: one chain's terms, float32 (n,).  Lane t starts from +0 and adds term t, t + 256, ... in that order (square: x * x, the product rounded first) -> the tree's result."""
    n = x.size
    rows = -(-n // 256) or 1
    pad = np.zeros(rows * 256, F); pad[:n] = x
    valid = (np.arange(rows * 256) < n).reshape(rows, 256)
    pad = pad.reshape(rows, 256)
    acc = np.zeros(256, F)
    with np.errstate(all="ignore"):
        for j in range(rows):
            term = pad[j] * pad[j] if square else pad[j]
            acc = np.where(valid[j], acc + term, acc)
    return tree_np(acc)


def partials_np(gs):
    """One partial per chunk of 4096 floats of every tensor, chunks numbered over the tensors in order."""
    out = []
    for g in gs:
        g = np.asarray(g, F).reshape(-1)
        n = g.size
        nch = -(-n // CHUNK)
        pad = np.zeros(nch * CHUNK, F); pad[:n] = g
        valid = (np.arange(nch * CHUNK) < n).reshape(nch, 16, 256)
        pad = pad.reshape(nch, 16, 256)
        acc = np.zeros((nch, 256), F)
        with np.errstate(all="ignore"):
            for j in range(16):
                acc = np.where(valid[:, j], acc + pad[:, j] * pad[:, j], acc)
            out.append(tree_np(acc))
    return np.concatenate(out).astype(F)


def norm_np(partials, clip):
    """-> state = [coef, norm, sumsq, 0]."""
    with np.errstate(all="ignore"):
        sumsq = F(lanes_np(np.asarray(partials, F).reshape(-1), False))
        norm = np.sqrt(sumsq)
        clip = F(clip)
        coef = clip / norm if norm > clip else F(1.0)
    return np.array([coef, norm, sumsq, 0.0], F)


# ---- inputs
def make_inputs(sizes, seed=0, adam=True):
    """sgd_ref.make_inputs' (w, g, h) plus a non-negative second history, and in every tensor of 10 or more elements special gradients: |g| = 1e-22 and 1e-23 (q = g1 * g1
    underflows, into a denormal and to zero: w = 0 there so that g1 = g), 1e20 (q = inf, r = m' / inf = 0) -- and, in the tensor with index 1 (index 0 where there is one
    tensor), a NaN."""
    rng = np.random.default_rng([seed, 57])
    out = []
    nan_at = 1 if len(sizes) > 1 else 0
    for i, (w, g, h) in enumerate(S.make_inputs(sizes, seed)):
        n = w.size
        h2 = rng.uniform(0, 0.25, n).astype(F)
        h2[i % n] = 0.0
        if n >= 10:
            g[5] = F(1e-22) if i % 2 == 0 else F(-1e-22); w[5] = 0.0; h2[5] = F(1e-44)     # q = 1e-44: a denormal (the smallest is 1.4e-45)
            g[8] = F(1e-23); w[8] = 0.0                                                      # q = 1e-46 rounds to +0
            g[6] = F(1e20)
            if i == nan_at:
                g[7] = np.nan
        out.append((w, g, h, h2))
    return out


def run_fop(rtc, name, fop, vals, hypers=None, guards=False, keep=None):
    """Compile `fop`, create one var per var arg (the op's dims), upload `vals` {arg: array} (others zero), run the call once -- or once per entry of `hypers`, the var
    `hyper` rewritten in between -> ({arg: array fetched}, {guard var: array})."""
    spec = [(an, io) for an, io in pipe_func_args(fop) if io in ("IN", "OUT", "INOUT")]
    rtc.compile([RtcFuncInfo(name, "", [a for a, _ in spec], fop)])
    made, am = [], {}
    guard = np.full(4, GUARD_BITS, np.uint32).view(F)
    try:
        for an, _ in spec:
            vn = f"{name}_{an}"
            rtc.create_var_with_dims(vn, fop.get_dims(an)); made.append(vn); am[an] = RtcArg.var(vn)
            if guards:
                rtc.create_var_with_dims(vn + "_guard", Dims.make("float", v=4)); made.append(vn + "_guard")
                rtc.copy_nda_to_var(vn + "_guard", guard)
            if an in vals:
                rtc.copy_nda_to_var(vn, np.ascontiguousarray(vals[an], F).reshape(fop.get_dims(an).sizes))
        call = RtcFuncCall(name, am)
        for hy in (hypers if hypers is not None else [None]):
            if hy is not None:
                rtc.copy_nda_to_var(f"{name}_hyper", np.asarray(hy, F))
            rtc.run(call)
        rtc.finish_and_sync()
        if keep is not None:
            keep.append(rtc.last_launch() if rtc.be == "hip" else {})
        outs = {an: rtc.copy_var_to_nda(f"{name}_{an}").reshape(-1) for an, _ in spec}
        gv = {vn: rtc.copy_var_to_nda(vn) for vn in made if vn.endswith("_guard")}
        return outs, gv
    finally:
        for vn in made:
            rtc.release_var(vn)
        rtc.release_func(name); rtc.release_per_call_id_data()


def update_fop(sizes, form, lr_mults=None, decay_mults=None):
    t, clip, dwd = form
    return solver_update_func_op([S.tensor_dims(n, i) for i, n in enumerate(sizes)], t, lr_mults, decay_mults, clip=clip, decoupled_wd=dwd)


def run_update(rtc, sizes, form, lr_mults, decay_mults, hypers, inputs, state, guards=False, keep=None):
    """-> ([(w, g, h, h2)] after one call per entry of hypers, guards)."""
    fop = update_fop(sizes, form, lr_mults, decay_mults)
    vals = {"state": state}
    for i, (w, g, h, h2) in enumerate(inputs):
        vals.update({f"w_{i}": w, f"g_{i}": g, f"h_{i}": h})
        if form[0] == "adam":
            vals[f"h2_{i}"] = h2
    outs, gv = run_fop(rtc, "slv", fop, vals, hypers, guards, keep)
    return [(outs[f"w_{i}"], outs[f"g_{i}"], outs[f"h_{i}"], outs.get(f"h2_{i}", inputs[i][3])) for i in range(len(sizes))], gv


def want_update(form, lr_mults, decay_mults, hypers, inputs, state):
    t, clip, dwd = form
    out = []
    for i, (w, g, h, h2) in enumerate(inputs):
        for hy in hypers:
            w, h, h2 = solver_np(t, w, g, h, h2, hy, lr_mults[i], decay_mults[i], clip, state[0], dwd)
        out.append((w, g, h, h2))
    return out


def run_norm(rtc, calls, parts_total, prefill, clip, keep=None):
    """calls: [(part0, [gradient arrays])], each one hip_grad_sumsq call into ONE partials var prefilled with `prefill`; then hip_grad_norm.
    -> ([partials fetched after each sumsq call], state)."""
    fops = [grad_sumsq_func_op([Dims.make("float", v=g.size) for g in gs], p0, parts_total) for p0, gs in calls]
    fn = grad_norm_func_op(parts_total)
    infos = [RtcFuncInfo(f"ssq_{k}", "", [a for a, _ in pipe_func_args(f)], f) for k, f in enumerate(fops)] + [RtcFuncInfo("gnorm", "", [a for a, _ in pipe_func_args(fn)], fn)]
    rtc.compile(infos)
    made = []
    try:
        for vn, n in (("nv_partials", parts_total), ("nv_hyper", 8), ("nv_state", 4)):
            rtc.create_var_with_dims(vn, Dims.make("float", v=n)); made.append(vn)
        rtc.copy_nda_to_var("nv_partials", np.asarray(prefill, F)); rtc.copy_nda_to_var("nv_hyper", hyper8(0.1, clip=clip))
        rtc.copy_nda_to_var("nv_state", np.full(4, GUARD_BITS, np.uint32).view(F))
        seen = []
        for k, (p0, gs) in enumerate(calls):
            am = {"partials": RtcArg.var("nv_partials")}
            for i, g in enumerate(gs):
                vn = f"nv_g_{k}_{i}"
                rtc.create_var_with_dims(vn, Dims.make("float", v=g.size)); made.append(vn); rtc.copy_nda_to_var(vn, np.asarray(g, F)); am[f"g_{i}"] = RtcArg.var(vn)
            rtc.run(RtcFuncCall(f"ssq_{k}", am)); rtc.finish_and_sync()
            if keep is not None:
                keep.append(rtc.last_launch() if rtc.be == "hip" else {})
            seen.append(rtc.copy_var_to_nda("nv_partials").reshape(-1))
        rtc.run(RtcFuncCall("gnorm", {"partials": RtcArg.var("nv_partials"), "hyper": RtcArg.var("nv_hyper"), "state": RtcArg.var("nv_state")}))
        rtc.finish_and_sync()
        assert same_bits(rtc.copy_var_to_nda("nv_partials"), seen[-1]), "hip_grad_norm wrote the partials"
        return seen, rtc.copy_var_to_nda("nv_state").reshape(-1)
    finally:
        for vn in made:
            rtc.release_var(vn)
        for k in range(len(fops)):
            rtc.release_func(f"ssq_{k}")
        rtc.release_func("gnorm"); rtc.release_per_call_id_data()


def want_norm(calls, prefill, clip):
    p = np.asarray(prefill, F).copy()
    seen = []
    for p0, gs in calls:
        mine = partials_np(gs)
        p[p0:p0 + mine.size] = mine
        seen.append(p.copy())
    return seen, norm_np(p, clip)


# ---- the driver
def make_driver(rtc, name, solver, **kw):
    mk, tops, seed = PIPES[name]
    cp = mk(); bp = add_bck_ops(cp, loss_tops=tops)
    drv = ConvPipeBck(rtc, solver=solver, **kw); drv.init(bp, small_params(cp, seed))
    return drv, bp


def state_vars(drv):
    adam = drv.solver.type == "adam"
    return list(drv.bp.cp.params) + [p + SGD_HIST_SFX for p in drv.sgd_params] + ([p + SGD_HIST2_SFX for p in drv.sgd_params] if adam else [])


def fetch(rtc, names):
    return {n: rtc.copy_var_to_nda(n) for n in names}


def want_hyper(sv, it, lr=None):
    """The eight words the driver uploads for step `it`; lr: the rate where no policy gives it."""
    lr = sv.lr_policy.lr_at(sv.lr, it) if sv.lr_policy is not None else (sv.lr if lr is None else lr)
    return hyper8(lr, sv.momentum, sv.weight_decay, sv.momentum2, sv.delta, corr_f64(sv.momentum, sv.momentum2, it + 1) if sv.type == "adam" else 1.0, sv.clip_gradients)


def check_step(rtc, drv, before, grads, after, hyper, state_got):
    """Every updated param and history held to the twin applied to `before` (fetched ahead of the step) with the gradients the step left; solver_state to the twin too."""
    sv = drv.solver
    clip = sv.clip_gradients > 0
    coef = 1.0
    if clip:
        want_state = norm_np(partials_np([grads[p + "_grad_loss"] for p in drv.sgd_params]), hyper[6])
        assert same_bits(state_got, want_state), ("solver_state", state_got, want_state)
        assert same_bits(rtc.copy_var_to_nda(SOLVER_PARTS_VAR), partials_np([grads[p + "_grad_loss"] for p in drv.sgd_params])), "partials"
        coef = want_state[0]
    for p in drv.sgd_params:
        h2 = before.get(p + SGD_HIST2_SFX)
        w2, hn, vn = solver_np(sv.type, before[p], grads[p + "_grad_loss"], before[p + SGD_HIST_SFX], h2, hyper, sv.mult_of(sv.lr_mult, p), sv.mult_of(sv.decay_mult, p), clip, coef, sv.decoupled_wd)
        assert same_bits(after[p + SGD_HIST_SFX], hn), (p, "history")
        if sv.type == "adam":
            assert same_bits(after[p + SGD_HIST2_SFX], vn), (p, "second history")
        assert same_bits(after[p], w2), (p, "param")
        assert not same_bits(after[p], before[p]), (p, "the step changed nothing")


def three_steps(rtc, name, solver, graph=None, inputs=None, **kw):
    """Three steps of a small pipe with a Solver (a new dropout seed and new inputs each; without a policy the rate is changed once through set_sgd_hyper), each held to
    the twins on the backend's own values; the uploaded hyper words are checked at every step -> the state after the third."""
    drv, bp = make_driver(rtc, name, solver, **kw)
    try:
        per = solver.tensors_per_call
        groups = -(-len(drv.sgd_params) // per)
        clip = solver.clip_gradients > 0
        assert drv.n_sgd_calls == groups + ((groups + 1) if clip else 0)
        tags = [t for t, _, _ in drv.calls()][-drv.n_sgd_calls:]
        assert tags == ([f"grad_sumsq_{k}" for k in range(groups)] + ["grad_norm"] if clip else []) + [f"solver_update_{k}" for k in range(groups)]
        if graph is not None:
            drv.capture_graph(parallel=graph)
        names = state_vars(drv)
        state = fetch(rtc, names)
        assert drv.iter == 0 and all(not np.any(state[n]) for n in names if n.endswith(SGD_HIST_SFX) or n.endswith(SGD_HIST2_SFX))
        lr = None
        for k in range(3):
            if k == 1 and solver.lr_policy is None:
                lr = 0.4 * solver.lr; drv.set_sgd_hyper(lr=lr)
            data, label = inputs(bp.cp, k) if inputs else small_inputs(bp.cp, k)
            drv.set_det_drop_seed(1000 + k)
            fwd = {"data": data, "label": label}
            gets = [p + "_grad_loss" for p in drv.sgd_params] + bp.loss_nodes
            drv.run_bck(["data", "label"], fwd, gets, graph=graph is not None)
            assert drv.iter == k + 1
            hyper = want_hyper(solver, k, lr)
            assert same_bits(rtc.copy_var_to_nda(SOLVER_HYPER_VAR), hyper), (k, "the uploaded hyper words")
            after = fetch(rtc, names)
            check_step(rtc, drv, state, fwd, after, hyper, rtc.copy_var_to_nda(SOLVER_STATE_VAR))
            state = after
        return state
    finally:
        drv.release()


# ---- descent on `chain`: fixed data, label and dropout seed (sgd_ref.descent_*'s recipe)
# Two trajectories: adam, and nesterov with clipping.  lr and the step count were picked on be=cpu so that the float64 loss at least halves while bck_pipe_ref.net_f64's
# guards (no ReLU input near zero, no tie in a pooling window) hold at every step.
DESCENT_SEED = S.DESCENT_SEED
DESCENT = {
    "adam": dict(solver=dict(type="adam", lr=0.002, momentum=0.9, momentum2=0.999, delta=1e-8, weight_decay=5e-4), steps=8),
    "nesterov_clip": dict(solver=dict(type="nesterov", lr=0.005, momentum=0.9, weight_decay=5e-4, clip_gradients=0.5), steps=12),
}
# max over the steps of |loss(backend) - loss(float64)|: what be=cpu measures; the bound is that times 10, the margin being for the GPU's different K-slice
# summation order in the filter gradients.  Held by be=cpu (tests/test_solver_cpu.py) and by be=hip (tests/test_gpu_solver.py).
# adam: lr 0.002, 8 steps, the float64 loss falls 0.6126 -> 0.0184, be=cpu measures 2.433e-07.  nesterov_clip: lr 0.005, clip_gradients 0.5 (the norm starts above it),
# 12 steps, 0.6126 -> 0.0378, be=cpu measures 4.132e-07.
DESCENT_DEV_CPU = {"adam": 2.433e-07, "nesterov_clip": 4.132e-07}
DESCENT_BOUND = {k: 10 * v for k, v in DESCENT_DEV_CPU.items()}


def update_f64(sv, w, g, h, h2, t, coef):
    """The written formulas in float64 (the hyper-parameters as the fp32 values the device holds), t = iter + 1."""
    lr, mom, wd, mom2, delta = (float(F(x)) for x in (sv.lr, sv.momentum, sv.weight_decay, sv.momentum2, sv.delta))
    g0 = coef * g
    if sv.type == "adam":
        g1 = g0 if sv.decoupled_wd else g0 + wd * w
        m = mom * h + (1.0 - mom) * g1
        v = mom2 * h2 + (1.0 - mom2) * g1 * g1
        u = lr * float(F(corr_f64(sv.momentum, sv.momentum2, t))) * m / (np.sqrt(v) + delta)
        if sv.decoupled_wd:
            u = u + lr * wd * w
        return w - u, m, v
    g1 = g0 + wd * w
    a = mom * h
    hn = a + lr * g1
    if sv.type == "nesterov":
        return w - ((1.0 + mom) * hn - a), hn, h2
    return w - hn, hn, h2


def descent_f64(which):
    """The float64 trajectory -> the loss of every step (taken before that step's update)."""
    sv = Solver(**DESCENT[which]["solver"])
    mk, tops, seed = PIPES["chain"]
    cp = mk(); data, label = small_inputs(cp, seed)
    params = {n: np.asarray(a, np.float64) for n, a in small_params(cp, seed).items()}
    hist = {n: np.zeros_like(a) for n, a in params.items()}
    hist2 = {n: np.zeros_like(a) for n, a in params.items()}
    clip = float(F(sv.clip_gradients))
    losses = []
    for k in range(DESCENT[which]["steps"]):
        r = ref.net_f64(cp, [cp.out_node()], params, data, label, {"drop1": DESCENT_SEED})
        losses.append(r["loss"])
        coef = 1.0
        if clip > 0:
            norm = np.sqrt(sum(float(np.sum(r[n + "_grad_loss"] ** 2)) for n in params))
            coef = clip / norm if norm > clip else 1.0
        for n in params:
            params[n], hist[n], hist2[n] = update_f64(sv, params[n], r[n + "_grad_loss"], hist[n], hist2[n], k + 1, coef)
    return losses


def descent_run(rtc, which):
    """The same trajectory on a backend -> the loss of every step."""
    drv, bp = make_driver(rtc, "chain", Solver(**DESCENT[which]["solver"]))
    try:
        data, label = small_inputs(bp.cp, PIPES["chain"][2])
        drv.set_det_drop_seed(DESCENT_SEED)
        assert drop_seeds(drv) == {"drop1": DESCENT_SEED}
        losses = []
        for _ in range(DESCENT[which]["steps"]):
            fwd = {"data": data, "label": label}
            drv.run_bck(["data", "label"], fwd, ["loss"])
            losses.append(float(fwd["loss"].item()))
        return losses
    finally:
        drv.release()
