"""What the SGD-update tests share (tests/test_sgd_cpu.py, tests/test_gpu_sgd.py): the numpy twin of hip_sgd_update's formula, inputs with both signs and exact zeros,
a runner for the bare function, the per-step check of a ConvPipeBck with a solver, and the descent run on `chain` with its float64 trajectory.

The twin is the written formula on np.float32 arrays, one numpy operation per rounding:
    lr_i = lr * lr_mult_i;  wd_i = weight_decay * decay_mult_i;  g1 = g + wd_i * w;  h' = momentum * h + lr_i * g1;  w' = w - h'
Every equality is np.array_equal on the uint32 views."""
import numpy as np

import bck_pipe_ref as ref
from boda_amd.bck_pipe import SGD_HIST_SFX, ConvPipeBck, SgdSolver, add_bck_ops
from boda_amd.cnn_op import pipe_func_args, sgd_update_func_op
from boda_amd.op import Dims
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo

from test_bck_pipe_cpu import PIPES, drop_seeds, small_inputs, small_params

F = np.float32
SIZES = [1, 3, 4, 5, 1023, 4096, 4097, 9000]     # one chunk is 4096 floats: the last two span more than one, with a ragged end
MIXED_32 = [SIZES[i % len(SIZES)] for i in range(32)]   # tens_num = 32: a chunk boundary falls between tensors, most tensors are far smaller than a chunk
GUARD_BITS = 0x7FC0BEEF                          # a NaN with a payload: what the guard vars hold


def sgd_np(w, g, h, lr, momentum, weight_decay, lr_mult=1.0, decay_mult=1.0):
    """-> (w', h'), float32, every operation its own rounding."""
    w, g, h = (np.asarray(a, F) for a in (w, g, h))
    lr_i = F(lr) * F(lr_mult)
    wd_i = F(weight_decay) * F(decay_mult)
    reg = wd_i * w
    g1 = g + reg
    a = F(momentum) * h
    b = lr_i * g1
    h2 = a + b
    w2 = w - h2
    assert w2.dtype == F and h2.dtype == F
    return w2, h2


def sgd_f64(w, g, h, lr, momentum, weight_decay, lr_mult=1.0, decay_mult=1.0):
    """The same formula in float64 (the hyper-parameters as the float32 values the device holds)."""
    lr_i = float(F(lr)) * lr_mult; wd_i = float(F(weight_decay)) * decay_mult
    h2 = float(F(momentum)) * h + lr_i * (g + wd_i * w)
    return w - h2, h2


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == F and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def tensor_dims(n, i=0):
    """Any dims will do: every third tensor whose size allows it is two-dimensional."""
    if i % 3 == 1 and n % 3 == 0 and n > 3:
        return Dims.make("float", a=3, b=n // 3)
    return Dims.make("float", v=n)


def make_inputs(sizes, seed=0):
    """Per tensor (w, g, h): values of both signs, a non-zero history, and a few exact zeros of both signs in each of the three."""
    rng = np.random.default_rng([seed, 31])
    out = []
    for i, n in enumerate(sizes):
        w = rng.uniform(-2, 2, n).astype(F); g = rng.uniform(-1, 1, n).astype(F); h = rng.uniform(-0.5, 0.5, n).astype(F)
        for k, a in enumerate((w, g, h)):
            a[(k + i) % n] = 0.0
            a[(k + i + 3) % n] = -0.0
        if n >= 5:
            w[4] = g[4] = h[4] = 0.0      # 0 - (m * 0 + lr * (0 + wd * 0)): the signs of the zeros through the chain
            w[n - 1] = -0.0; g[n - 1] = -0.0; h[n - 1] = -0.0
        out.append((w, g, h))
    return out


def run_sgd(rtc, sizes, lr_mults, decay_mults, hypers, inputs, guards=False, keep=None, dims=None):
    """Compile hip_sgd_update over `sizes`, upload `inputs` [(w, g, h)], run one call per entry of `hypers` (each [lr, momentum, weight_decay]; the var is rewritten in
    between) -> ([(w, g, h)] fetched back, {guard var: array}).  guards: one 4-float var filled with GUARD_BITS is created behind every tensor var.  dims: the
    tensors' dims, where tensor_dims' choice will not do."""
    fop = sgd_update_func_op(dims or [tensor_dims(n, i) for i, n in enumerate(sizes)], lr_mults, decay_mults)
    spec = pipe_func_args(fop)
    rtc.compile([RtcFuncInfo("sgd_f", "", [a for a, _ in spec], fop)])
    made, am = [], {}
    guard = np.full(4, GUARD_BITS, np.uint32).view(F)
    try:
        for an, io in spec:
            vn = "sgdv_" + an
            rtc.create_var_with_dims(vn, fop.get_dims(an)); made.append(vn); am[an] = RtcArg.var(vn)
            if guards:
                rtc.create_var_with_dims(vn + "_guard", Dims.make("float", v=4)); made.append(vn + "_guard")
                rtc.copy_nda_to_var(vn + "_guard", guard)
        for i, (w, g, h) in enumerate(inputs):
            for b, a in (("w", w), ("g", g), ("h", h)):
                rtc.copy_nda_to_var(f"sgdv_{b}_{i}", a)
        call = RtcFuncCall("sgd_f", am)
        for hy in hypers:
            rtc.copy_nda_to_var("sgdv_hyper", np.array(list(hy) + [0.0], F))
            rtc.run(call)
        rtc.finish_and_sync()
        if keep is not None:
            keep.append(rtc.last_launch() if rtc.be == "hip" else {})
        outs = [tuple(rtc.copy_var_to_nda(f"sgdv_{b}_{i}").reshape(-1) for b in ("w", "g", "h")) for i in range(len(sizes))]
        gv = {vn: rtc.copy_var_to_nda(vn) for vn in made if vn.endswith("_guard")}
        return outs, gv
    finally:
        for vn in made:
            rtc.release_var(vn)
        rtc.release_func("sgd_f"); rtc.release_per_call_id_data()


def want_sgd(sizes, lr_mults, decay_mults, hypers, inputs):
    """The numpy twin of run_sgd's result."""
    out = []
    for i, (w, g, h) in enumerate(inputs):
        for lr, mom, wd in hypers:
            w, h = sgd_np(w, g, h, lr, mom, wd, lr_mults[i], decay_mults[i])
        out.append((w, g, h))
    return out


# ---- the driver
def make_sgd_driver(rtc, name, solver, **kw):
    mk, tops, seed = PIPES[name]
    cp = mk(); bp = add_bck_ops(cp, loss_tops=tops)
    drv = ConvPipeBck(rtc, solver=solver, **kw); drv.init(bp, small_params(cp, seed))
    return drv, bp


def state_vars(bp):
    return list(bp.cp.params) + [p + SGD_HIST_SFX for p in bp.cp.params]


def fetch(rtc, names):
    return {n: rtc.copy_var_to_nda(n) for n in names}


def check_step_is_numpy_update(rtc, drv, bp, before, hyper, graph=False, data=None, label=None, seed=0):
    """Run one step and hold every param and history var to the numpy update of `before` (fetched ahead of the step) with the gradients the step left.
    -> the fetched state after the step."""
    sv = drv.solver
    drv.set_det_drop_seed(seed)
    fwd = {"data": data, "label": label}
    gets = [p + "_grad_loss" for p in bp.cp.params] + bp.loss_nodes
    drv.run_bck(["data", "label"], fwd, gets, graph=graph)
    after = fetch(rtc, state_vars(bp))
    for p in bp.cp.params:
        w2, h2 = sgd_np(before[p], fwd[p + "_grad_loss"], before[p + SGD_HIST_SFX], hyper[0], hyper[1], hyper[2], sv.mult_of(sv.lr_mult, p), sv.mult_of(sv.decay_mult, p))
        assert same_bits(after[p + SGD_HIST_SFX], h2), (p, "history")
        assert same_bits(after[p], w2), (p, "param")
        assert not same_bits(after[p], before[p]), (p, "the step changed nothing")
    return after, fwd


def three_steps(rtc, name, tensors_per_call=32, **kw):
    """Three steps of a small pipe with a solver (a new dropout seed and new inputs each, the learning rate changed once through set_sgd_hyper), each held to the numpy
    update of the backend's own values -> the state after the third."""
    solver = SgdSolver(lr=0.05, momentum=0.9, weight_decay=5e-4, lr_mult={"biases": 2.0}, decay_mult={"biases": 0.0}, tensors_per_call=tensors_per_call)
    drv, bp = make_sgd_driver(rtc, name, solver, **kw)
    try:
        assert drv.n_sgd_calls == -(-len(bp.cp.params) // tensors_per_call)
        hyper = [0.05, 0.9, 5e-4]
        state = fetch(rtc, state_vars(bp))
        assert all(not np.any(state[p + SGD_HIST_SFX]) for p in bp.cp.params)
        for k in range(3):
            if k == 1:
                drv.set_sgd_hyper(lr=0.02); hyper[0] = 0.02
            data, label = small_inputs(bp.cp, k)
            state, _ = check_step_is_numpy_update(rtc, drv, bp, state, hyper, data=data, label=label, seed=1000 + k)
        return state
    finally:
        drv.release()


# ---- descent on `chain`: fixed data, label and dropout seed
# lr and the step count were picked on be=cpu so that the float64 loss falls from 0.6126 to 0.0005 (it has to halve at least) while bck_pipe_ref.net_f64's guards
# (no ReLU input near zero, no tie in a pooling window) hold at every step; larger rates memorise the two images in one step, which compares nothing.
DESCENT_LR, DESCENT_STEPS, DESCENT_SEED = 0.002, 12, 4321
DESCENT_MOM, DESCENT_WD = 0.9, 5e-4
# max over the steps of |loss(backend) - loss(float64)|: be=cpu measures 1.681e-07; the bound is that times 10, the margin being for the GPU's different K-slice
# summation order in the filter gradients.  Held by be=cpu (tests/test_sgd_cpu.py) and by be=hip (tests/test_gpu_sgd.py).
DESCENT_DEV_CPU = 1.681e-07
DESCENT_BOUND = 10 * DESCENT_DEV_CPU


def descent_f64():
    """The float64 trajectory: bck_pipe_ref.net_f64's gradients and the formula in float64 -> the loss of every step (taken before that step's update)."""
    mk, tops, seed = PIPES["chain"]
    cp = mk(); data, label = small_inputs(cp, seed)
    params = {n: np.asarray(a, np.float64) for n, a in small_params(cp, seed).items()}
    hist = {n: np.zeros_like(a) for n, a in params.items()}
    losses = []
    for _ in range(DESCENT_STEPS):
        r = ref.net_f64(cp, [cp.out_node()], params, data, label, {"drop1": DESCENT_SEED})
        losses.append(r["loss"])
        for n in params:
            params[n], hist[n] = sgd_f64(params[n], r[n + "_grad_loss"], hist[n], DESCENT_LR, DESCENT_MOM, DESCENT_WD)
    return losses


def descent_run(rtc):
    """The same trajectory on a backend -> the loss of every step."""
    solver = SgdSolver(lr=DESCENT_LR, momentum=DESCENT_MOM, weight_decay=DESCENT_WD)
    drv, bp = make_sgd_driver(rtc, "chain", solver)
    try:
        data, label = small_inputs(bp.cp, PIPES["chain"][2])
        drv.set_det_drop_seed(DESCENT_SEED)
        assert drop_seeds(drv) == {"drop1": DESCENT_SEED}
        losses = []
        for _ in range(DESCENT_STEPS):
            fwd = {"data": data, "label": label}
            drv.run_bck(["data", "label"], fwd, ["loss"])
            losses.append(float(fwd["loss"].item()))
        return losses
    finally:
        drv.release()
