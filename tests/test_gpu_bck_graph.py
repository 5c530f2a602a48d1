"""The gradient step as one hipGraph replay on the MI355X: the seed-var form of bodahip_dropout (kernels/bck_ops_f32.hip -DSEEDVAR=1) and ConvPipeBck's
capture_graph / run_graph / run_bck(graph=True), serial and with the calls' true dependencies (parallel=True).

Every comparison is np.array_equal on the uint32 views.  Driver G is ConvPipeBck(seed_in_var=True) with a captured graph on one backend instance; driver E is a default
eager driver on a second instance with the same params.  After every replay G must hold E's bits -- same seed, same inputs -- in every gradient node, every loss and the
side vars the backward pass reads (*_in_yx, *_scale_base, *_prob); a replay repeated on unchanged inputs must reproduce itself (the K-slice tickets of the filter
gradients are back at zero after every launch)."""
import numpy as np
import pytest

import bck_pipe_ref as ref
from boda_amd import rtc as rtc_mod
from boda_amd.bck_pipe import SEED_VAR, ConvPipeBck, add_bck_ops, host_params
from boda_amd.cnn_op import seed_from_var
from boda_amd.conv_pipe import nin_imagenet
from boda_amd.op import RtErr
from boda_amd.rtc import make_rtc

from test_bck_graph_cpu import M32, SEED_PAIRS, SHAPES, drop_input, make_driver, run_flagged
from test_bck_pipe_cpu import PIPES, SEED_A, SEED_B, ann, bits_eq, dropout_op, grad_nodes, run_func, small_inputs

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


# ---- the seed-var kernel
@pytest.mark.parametrize("ratio", [0.5, 0.1])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_seed_from_var_kernel(hip, cpu, shape, ratio):
    dims, shp = SHAPES[shape]
    x = drop_input(shp)
    plain = ann(dropout_op(ratio, dims))[0]
    flagged = seed_from_var(plain)
    for word, byval in SEED_PAIRS:
        keep = []
        got = run_flagged(hip, flagged, x, word, byval, keep=keep)
        assert keep == ["bodahip_dropout"], keep
        summed = (word + byval) % M32
        assert bits_eq(got, run_func(hip, plain, {"inout": x}, seed=summed)["inout"]), (word, byval)
        assert bits_eq(got, run_flagged(cpu, flagged, x, word, byval)), (word, byval)
        assert bits_eq(got, ref.dropout_f32(x, ratio, summed)), (word, byval)
    before = rtc_mod.compile_stats()
    got = run_flagged(hip, flagged, x, 424242, 77)   # a word and an offset never seen: no compile, not even a cache look-up
    after = rtc_mod.compile_stats()
    assert (after["compiled"], after["cache_hits"]) == (before["compiled"], before["cache_hits"])
    assert bits_eq(got, ref.dropout_f32(x, ratio, 424242 + 77))


# ---- the small pipes, captured
def side_vars(drv):
    return [v for v in drv.vars if v.endswith(("_in_yx", "_scale_base", "_prob"))]


def step(drv, seed, data, label, gets, graph):
    drv.set_det_drop_seed(seed)
    fwd = {"data": data, "label": label}
    drv.run_bck(["data", "label"], fwd, gets, graph=graph)
    return fwd


def check_rounds(hip, G, E, bp, parallel):
    n = G.capture_graph(parallel=parallel)   # (no step has run on G: capture_graph runs one first)
    assert n == len(G.calls()) and n > 0
    if parallel:
        assert len(G.call_deps) == n and any(len(d) > 1 for d in G.call_deps) and any(i and (i - 1) not in d for i, d in enumerate(G.call_deps))
    gets = grad_nodes(bp) + bp.loss_nodes + side_vars(G)
    assert set(side_vars(G)) == set(side_vars(E)) and any(v.endswith("_prob") for v in gets)
    cp = bp.cp
    d0, l0 = small_inputs(cp, 0)
    d1, l1 = small_inputs(cp, 1)
    assert not np.array_equal(d0, d1)
    for seed, data, label in ((SEED_A, d0, l0), (SEED_B, d0, l0), (SEED_A, d1, l1)):
        g = step(G, seed, data, label, gets, True)
        assert G.per_call_ms == [] and G.compute_dur_ms > 0
        e = step(E, seed, data, label, gets, False)
        for v in gets:
            assert bits_eq(g[v], e[v]), (seed, v)
        G.run_graph()   # the same replay once more, inputs unchanged
        for v in gets:
            assert bits_eq(hip.copy_var_to_nda(v), g[v]), ("replayed twice", seed, v)


@pytest.mark.parametrize("parallel", [False, True])
@pytest.mark.parametrize("name", sorted(PIPES))
def test_pipe_graph_replay(hip, hip2, name, parallel):
    G, bp, _, _ = make_driver(hip, name, seed_in_var=True)
    E, _, _, _ = make_driver(hip2, name)
    try:
        check_rounds(hip, G, E, bp, parallel)
    finally:
        G.release(); E.release()


@pytest.mark.parametrize("parallel", [False, True])
def test_chain_fused_relu_grad_graph_replay(hip, hip2, parallel):
    """The captured step with the ReLU gradient folded into the BckLRN, against the eager UNFUSED step."""
    G, bp, _, _ = make_driver(hip, "chain", seed_in_var=True, fuse_relu_grad=True)
    E, _, _, _ = make_driver(hip2, "chain")
    try:
        assert G.fused_relu_grads["folded"] == ["relu_conv1_bck"] and len(G.calls()) == len(E.calls()) - 1
        check_rounds(hip, G, E, bp, parallel)
    finally:
        G.release(); E.release()


def test_graph_refusals(hip, hip2):
    D, bp, data, label = make_driver(hip, "chain")   # a Dropout with its seed by value
    try:
        with pytest.raises(RtErr, match="seed_in_var=True"):
            D.capture_graph()
        with pytest.raises(RtErr, match="no captured graph"):
            D.run_bck(["data", "label"], {"data": data, "label": label}, [], graph=True)
        gets = grad_nodes(bp) + bp.loss_nodes
        step(D, SEED_A, data, label, gets, False)   # the refusals left the backend as it was
    finally:
        D.release()
    G, bp, data, label = make_driver(hip, "fan")    # no dropout: captures without the flag
    E, _, _, _ = make_driver(hip2, "fan")
    try:
        assert SEED_VAR not in G.vars
        with pytest.raises(RtErr, match="no captured graph"):
            G.run_bck(["data", "label"], {"data": data, "label": label}, [], graph=True)
        assert G.capture_graph() == len(G.calls())
        gets = grad_nodes(bp) + bp.loss_nodes
        g, e = step(G, 0, data, label, gets, True), step(E, 0, data, label, gets, False)
        for v in gets:
            assert bits_eq(g[v], e[v]), v
    finally:
        G.release(); E.release()


def test_second_capture_and_release(hip, hip2):
    """A second capture destroys the first; release() destroys the graph and leaves the backend usable: a fresh driver initialises and steps on it."""
    E, bp, data, label = make_driver(hip2, "chain")
    gets = grad_nodes(bp) + bp.loss_nodes
    try:
        e = step(E, SEED_B, data, label, gets, False)
    finally:
        E.release()
    G, _, _, _ = make_driver(hip, "chain", seed_in_var=True)
    try:
        G.capture_graph()
        first = G._graph
        G.capture_graph(parallel=True)
        assert G._graph != first
        with pytest.raises(RtErr, match="invalid graph id"):
            hip.graph_launch(first)
        last = G._graph
        g = step(G, SEED_B, data, label, gets, True)
    finally:
        G.release()
    assert G._graph is None
    with pytest.raises(RtErr, match="invalid graph id"):
        hip.graph_launch(last)
    for v in gets:
        assert bits_eq(g[v], e[v]), v
    F, _, _, _ = make_driver(hip, "chain", seed_in_var=True)   # the same var and function names again
    try:
        f = step(F, SEED_B, data, label, gets, False)
        for v in gets:
            assert bits_eq(f[v], e[v]), v
        F.capture_graph()
        f = step(F, SEED_B, data, label, gets, True)
        for v in gets:
            assert bits_eq(f[v], e[v]), v
    finally:
        F.release()


# ---- one real net
def test_nin_two_images_graph(hip, hip2):
    """NiN at two images, the shape of test_gpu_bck_pipe.test_nin_two_images: one serial and one parallel replay against the eager step.  The filter gradients of its
    first six convolutions run with more than one K slice there (conv1 .. cccp2: 23, conv2 .. cccp4: 5 at 256 CUs), each on the workspace of its own call."""
    cp = nin_imagenet(2); bp = add_bck_ops(cp)
    params = host_params(bp, 5)
    rng = np.random.default_rng(0)
    data = rng.uniform(-1, 1, cp.nodes["data"].sizes).astype(np.float32)
    label = np.array([3, 998], np.float32).reshape(2, 1, 1)
    gets = grad_nodes(bp) + ["loss"]
    E = ConvPipeBck(hip2); E.init(bp, params)
    try:
        e = step(E, 5, data, label, gets, False)
    finally:
        E.release()
    assert np.isfinite(e["loss"].item()) and np.any(e["conv1_filts_grad_loss"] != 0)
    G = ConvPipeBck(hip, seed_in_var=True); G.init(bp, params)
    try:
        cus = hip.get_device_info()["num_cus"]
        ksl = {c.tag: int(rtc_mod.explain_plan(c.fop, num_cus=cus).split("ksl=")[1].split()[0]) for c in G.bck_calls if c.fop.get_func_name() == "hip_bconv_filts"}
        print("K slices of the captured hip_bconv_filts calls:", ksl)
        assert len(ksl) == 12 and max(ksl.values()) > 1, ksl
        for parallel in (False, True):
            assert G.capture_graph(parallel=parallel) == len(G.calls())
            g = step(G, 5, data, label, gets, True)
            for v in gets:
                assert bits_eq(g[v], e[v]), (parallel, v)
    finally:
        G.release()
