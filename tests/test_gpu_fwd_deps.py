"""ConvPipeFwd's dependency lists, executed (-m gpu): the call list of a forward pass runs eagerly, ONE CALL AT A TIME with a device synchronisation behind each,
in orders other than the list's that respect ConvPipeFwd._call_deps -- always the highest-index ready call, and two seeded random topological orders.  Every var
that some call writes is zeroed first.  Such a run is deterministic: a missing dependency lets some order put a reader in front of its writer (it reads zeros) or a
writer in front of an earlier reader, and a var then differs from the list order's.  Every comparison is of the vars' raw bytes (bf16 vars included, their pad
channels too): no kernel's arithmetic is under test and there is no tolerance.

Per configuration also: in the list-order run every written var holds something other than zeros (else the poison is blind for it); each alternative order's
fraction of moved positions is printed, and is at least a quarter wherever the dependency lists leave that much freedom (a configuration whose list is a chain, or
close to one, is reported as NOT COVERED by the orders: fully fused channels-last lists are chains); and the rule that csrc/hip_compute.cc's graph_end_deps
orders by -- a call that works in the backend's one shared scratch launches at least two kernels -- holds for every call (last_launch()'s `kernels` and
`uses_scratch`).

One further case shows that the detector detects: with one true edge taken out of a copy of the lists, the latest-ready order reads zeros and a var differs.
Nothing here replays a graph to catch a race, and nothing reads the reference project."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fwd_deps_ref as fr
import resnet_ref as rr
from boda_amd.conv_pipe import DryRtc
from boda_amd.rtc import make_rtc

REPORT = {}     # configuration -> what was measured (printed by the last test)


@pytest.fixture(scope="module")
def hip():
    r = make_rtc("(be=hip)", 0)
    r.init()
    yield r
    r.finish_and_sync()
    r.close()


_DATA = {}


def net_data(net):
    """(pipe, params, input) of a small net, made once."""
    if net not in _DATA:
        cp = fr.SMALL_NETS[net]()
        x = np.random.default_rng(5).uniform(-1, 1, cp.nodes[cp.in_node].sizes).astype(np.float32)
        _DATA[net] = (cp, rr.he_params(cp, 4), x)
    return _DATA[net]


def run_in_order(rtc, f, x, order, written, stats=None):
    for vn in written:
        rtc.set_var_to_zero(vn)
    rtc.copy_nda_to_var(f.in_var, x)
    rtc.finish_and_sync()
    for i in order:
        rtc.run(f.fwd_calls[i].rfc); rtc.finish_and_sync()
        if stats is not None:
            ll = rtc.last_launch(); stats[i] = (ll["kernels"], ll["uses_scratch"])
    rtc.release_per_call_id_data()
    return {vn: np.ascontiguousarray(rtc.copy_var_to_nda(vn)).tobytes() for vn in written}


def start(hip, cfg):
    """The driver of a configuration after one ordinary pass and a serial capture, the vars its calls write, and its dependency lists."""
    net, layout, kw = cfg
    cp, P, x = net_data(net)
    dry = DryRtc(); twin = fr.make_driver(dry, net, layout, kw, cp)       # the same list on the recording backend: the declared directions come from its records
    rw = fr.all_rw(twin, dry)
    f = fr.make_driver(hip, net, layout, kw, cp, P)
    try:
        sig = lambda d: [(c.tag, c.func, sorted((a, v.n) for a, v in c.rfc.arg_map.items() if v.is_var())) for c in d.fwd_calls]
        assert sig(f) == sig(twin)
        if net == "chain":      # the switches of this net take effect: the pooling goes into its convolution, the first convolution reads a k-major copy of its filters
            assert bool(f.fused_pools) == bool(kw.get("fuse_f32_pools")) and bool(f.k1_chains) == (kw.get("fuse_k1_chains") is not False)
            assert [c.tag for c in f.fwd_calls if "filts_km" in c.rfc.arg_map] == (["c1"] if kw.get("filts_kmajor_once", True) else [])
        f.run_fwd([cp.in_node], {cp.in_node: x}, [])      # every lazily built kernel, table and workspace exists
        assert f.capture_graph() == len(f.fwd_calls)
        written = sorted(set().union(*[set(w) for _, w, _ in rw]))
        assert not (set(f._res_nodes) & set(written))     # (a flagged convolution's own node: no call writes it, nothing is read back for it; lazy nodes likewise, unless
        # a call of the pass writes them after all -- the pooling that ends a convolution's fused launch is also registered for materialisation)
        return f, x, rw, written, f._call_deps()
    except BaseException:
        f.release(); raise


@pytest.mark.parametrize("cfg", fr.GPU_CONFIGS, ids=fr.config_id)
def test_deps_are_sufficient_when_executed(hip, cfg):
    t0 = time.perf_counter()
    f, x, rw, written, deps = start(hip, cfg)
    try:
        n = len(deps)
        stats = {}
        want = run_in_order(hip, f, x, range(n), written, stats)
        blind = [vn for vn in written if not any(want[vn])]
        assert not blind, blind
        # the shared scratch's ordering rule: graph_end_deps keeps the calls that launch several kernels in launch order BECAUSE those are the ones in the scratch
        for i, (kernels, scratch) in stats.items():
            assert kernels >= 1, (f.fwd_calls[i].tag, kernels)
            assert not scratch or kernels >= 2, (f.fwd_calls[i].tag, f.fwd_calls[i].func, kernels, "works in the shared scratch with one kernel: graph_end_deps does not order it")
        orders = fr.alt_orders(deps)
        moved = {}
        for what, order in orders.items():
            assert sorted(order) == list(range(n)) and all(order.index(j) < order.index(i) for i in range(n) for j in deps[i])
            moved[what] = fr.moved_fraction(order)
            got = run_in_order(hip, f, x, order, written)
            bad = [vn for vn in written if got[vn] != want[vn]]
            assert not bad, (what, order, bad)
        coverable = fr.can_be_covered(deps)
        line = (f"{fr.config_id(cfg)}: {n} calls, {sum(map(len, deps))} edges, {len(fr.hazards(rw))} hazard pairs, {len(written)} vars compared; moved: "
                + ", ".join(f"{k} {v:.2f}" for k, v in moved.items()) + f"; {sum(s for _, s in stats.values())} calls in the shared scratch, "
                + f"{sum(1 for k, _ in stats.values() if k > 1)} with several kernels; " + ("covered" if coverable else f"NOT COVERED by the orders ({fr.free_positions(deps)} movable calls)"))
        if coverable:
            assert all(v >= fr.QUARTER for v in moved.values()), moved
    finally:
        f.release()
    REPORT[fr.config_id(cfg)] = line + f"; {time.perf_counter() - t0:.1f} s"
    print(REPORT[fr.config_id(cfg)])


def test_a_missing_edge_is_detected(hip):
    """incep, channels-last, default switches: the second module's first reader of the first module's Concat var loses its edge to a call that writes a channel slice
    of that var.  Latest-ready then runs the reader first: it reads zeros where the slice should be."""
    cfg = fr.GPU_CONFIGS[0]
    assert fr.config_id(cfg) == "incep-nhwc-default"
    f, x, rw, written, deps = start(hip, cfg)
    try:
        n = len(deps)
        cat = "a_out"
        reader = min(i for i in range(n) if cat in rw[i][0])
        slicers = [j for j in deps[reader] if any(r is not None for r in rw[j][1].get(cat, []))]
        assert slicers, (reader, deps[reader])
        victim = max(slicers)
        loose = [[j for j in d if not (i == reader and j == victim)] for i, d in enumerate(deps)]
        order = fr.topo_order(loose, max)
        assert order.index(reader) < order.index(victim), order      # the weakened lists do let the reader overtake the writer
        want = run_in_order(hip, f, x, range(n), written)
        got = run_in_order(hip, f, x, order, written)
        differs = [vn for vn in written if got[vn] != want[vn]]
        print(f"edge {f.fwd_calls[victim].tag} -> {f.fwd_calls[reader].tag} removed: {len(differs)} of {len(written)} vars differ ({', '.join(differs[:4])} ...)")
        assert differs
        again = run_in_order(hip, f, x, fr.topo_order(deps, max), written)      # and with the edge back, the same order rule gives the list order's bytes
        assert all(again[vn] == want[vn] for vn in written)
    finally:
        f.release()


def test_scratch_use_and_kernel_count_are_reported(hip):
    """What the scratch rule above is checked with, on two single ops whose plans are known: the bf16 input-patch convolution re-lays its filters into the shared scratch
    with one kernel and reads them with a second; the fp32 convolution of the same layer is one kernel and stays out of the scratch."""
    from boda_amd.cnn_op import OpTune, add_codegen_annotations
    from boda_amd.op import parse_op
    from boda_amd.ops_prof import OpsBackend, profile_rcg_call
    cv = parse_op("(str_vals=(type=Convolution),nda_vals=(biases=(dims=(out_chan=64)),filts=(dims=(out_chan=64,in_chan=32,y=5,x=5)),"
                  "in=(dims=(img=5,chan=32,y=14,x=14)),in_pad=(tn=none,dims=(y=2,x=2)),kern_sz=(tn=none,dims=(y=5,x=5)),"
                  "out=(dims=(img=5,chan=64,y=14,x=14)),out_chans=(tn=uint32_t,v=64),stride=(tn=none,dims=(y=1,x=1))))")
    be = OpsBackend(hip)
    _, p16 = profile_rcg_call(be, add_codegen_annotations(cv, OpTune(hip_dtype="bf16")), 5)
    assert p16.launch["kernel"] == "bodahip_conv_patch_bf16" and p16.launch["uses_scratch"] is True and p16.launch["kernels"] >= 2, p16.launch
    _, p32 = profile_rcg_call(be, add_codegen_annotations(cv, OpTune()), 5)
    assert p32.launch["kernel"] == "bodahip_conv_f32" and p32.launch["uses_scratch"] is False and p32.launch["kernels"] == 1, p32.launch


def test_zz_report():
    """What the cases above measured, in one place (printed)."""
    for line in REPORT.values():
        print(line)
    covered = [k for k, v in REPORT.items() if "NOT COVERED" not in v]
    print(f"{len(covered)} of {len(REPORT)} configurations covered by the orders: {', '.join(covered)}")
    if len(REPORT) == len(fr.GPU_CONFIGS):      # (the whole file ran) the lists that leave a quarter of their calls movable are these five, and each was run in three other orders
        assert covered == ["incep-nhwc-fuse_levels=False", "incep-nhwc-sets_take_groups=False", "incep-nhwc-fuse_pools=False", "incep-fp32-default", "res-fp32-default"], covered
