"""ConvPipeFwd._call_deps held against the ground truth, without a device: what every call reads and writes taken from the functions' declared argument directions
(tests/fwd_deps_ref.py), the hazards that follow from it, and the closure of the dependency lists.  Nets x layouts x every switch of the driver flipped alone, all on
the recording backend (DryRtc).  Every comparison is of sets and indices: no arithmetic, no tolerance.

  classification   the read and write sets _call_deps works from (ConvPipeFwd._call_rw) are the declared ones; every var argument is a read, a write, or a var that
                   no call of the pass writes
  sufficiency      every hazard pair (i, j) has i reachable from j through deps
  parallelism      deps[i] is sorted, unique and < i; an edge joins only calls that share a var; GoogLeNet's 3x3 / 5x5 / pool-projection branches and the Concat
                   copies into one var stay mutually unreachable
  level sets       the members of every level set, and of every sibling group, are pairwise unreachable in the ground-truth closure of the net built without them"""
import itertools

import pytest

import fwd_deps_ref as fr
from boda_amd import conv_pipe as cpm
from boda_amd import nhwc
from boda_amd.cnn_op import OpTune
from boda_amd.conv_pipe import ConvPipeFwd, DryRtc

NETS = {"nin": lambda: cpm.nin_imagenet(2), "alexnet": lambda: cpm.alexnet_ng_conv(2), "googlenet": lambda: cpm.googlenet_conv(2), "resnet50": lambda: cpm.resnet50(1),
        "incep": fr.incep_net, "chain": fr.chain_net, "res": fr.res_net, "catcopy": None,
        "nin128": lambda: cpm.nin_imagenet(128)}     # (fp32 only: the size at which plans read k-major filters and fuse_f32_pools finds its pairs; nothing runs here, so size is free)
FP32_ONLY = ("nin128",)
RESNETS = ("resnet50", "res")
NHWC_SWITCHES = [{"fuse_siblings": False}, {"fuse_levels": False}, {"sets_take_groups": False}, {"fuse_pools": False}, {"fuse_pool_lrn": True}, {"fuse_pool_lrn": False},
                 {"fuse_pool_lrn": "pool_first"}, {"fuse_post": False}, {"spec_fwd": False}, {"fuse_pool_lrn": True, "fuse_post": False},
                 {"fuse_levels": False, "fuse_siblings": False}]
FP32_SWITCHES = [{"fuse_k1_chains": False}, {"fuse_k1_chains": "all"}, {"fuse_f32_pools": True}, dict(fr.F32_POOLS), {"filts_kmajor_once": False}, {"spec_fwd": False}]


def catcopy_net():
    """A Concat with inputs that no convolution writes (a pooling's and an LRN's output): they reach the Concat's var through copies."""
    lines = ["input data 8 12 12", "conv c0 data c0 16 3 3 1 1 1 1", "relu c0_relu c0 c0", "pool pa c0 pa 3 3 1 1 1 1 0 0", "lrn na c0 na 5 0.0001 0.75 1.0",
             "conv cb c0 cb 8 1 1 1 1 0 0", "relu cb_relu cb cb", "concat cat cat_out pa,cb,na", "conv fc cat_out fc 16 1 1 1 1 0 0"]
    return cpm.pipe_from_spec("catcopy", lines, 2)


NETS["catcopy"] = catcopy_net
fr.HOST_NETS.update(NETS)


def matrix():
    out = []
    for net in NETS:
        for layout in ("fp32",) if net in FP32_ONLY else ("fp32", "nhwc"):
            sw = [{}] + (NHWC_SWITCHES if layout == "nhwc" else FP32_SWITCHES)
            if net in RESNETS and layout == "nhwc":
                sw = sw + [{"fuse_residual": False}]
            if net == "chain":
                sw = [dict(fr.CHAIN_BASE, **s) if "fuse_k1_chains" not in s else s for s in sw]
            for s in sw:
                if (net, layout, s) not in out:      # (the chain net's base switches make one of the flips its default)
                    out.append((net, layout, s))
    return out


MATRIX = matrix()
_BUILT = {}
COUNTS = {"classification": 0, "sufficiency": 0}


cid = fr.config_id


def built(net, layout, kw):
    """(driver, recording backend, [(reads, writes, directions)] per call, deps), built once per configuration."""
    key = cid((net, layout, kw))
    if key not in _BUILT:
        dry = DryRtc()
        f = fr.make_driver(dry, net, layout, kw, NETS[net]())
        _BUILT[key] = (f, dry, fr.all_rw(f, dry), f._call_deps())
    return _BUILT[key]


@pytest.mark.parametrize("cfg", MATRIX, ids=cid)
def test_classification(cfg):
    f, dry, rw, deps = built(*cfg)
    written = set().union(*[set(w) for _, w, _ in rw])
    n = 0
    for i, (c, (rd, wr, dirs)) in enumerate(zip(f.fwd_calls, rw)):
        got_rd, got_wr, part_of = f._call_rw(i)
        assert len(got_wr) == len(set(got_wr)) or c.func in (nhwc.GRP_FUNC, nhwc.SET_FUNC), (c.tag, got_wr)
        assert set(got_wr) == set(wr), (c.tag, c.func, sorted(got_wr), sorted(wr))
        assert set(part_of) == set(got_wr)
        # reads: equal on every var that some call of the pass writes; a read the driver does not list is of a var nothing writes (filters, biases, ...)
        assert set(got_rd) <= rd, (c.tag, c.func, sorted(set(got_rd) - rd))
        assert {v for v in rd if v in written} == {v for v in got_rd if v in written}, (c.tag, c.func, sorted(rd), sorted(got_rd))
        for a, v in c.rfc.arg_map.items():
            if v.is_var():
                assert dirs[a] in ("IN", "OUT", "INOUT"), (c.tag, a, dirs[a])     # no var argument is unclassified
                assert v.n in got_rd or v.n in got_wr or v.n not in written, (c.tag, a, v.n)
                n += 1
        # a write the driver exempts from ordering against the var's other writers is a proper channel range, clear of every other exempted writer's
        for v in got_wr:
            if part_of[v]:
                assert all(r is not None for r in wr[v]) or not any(v in rw[j][1] for j in range(len(rw)) if j != i), (c.tag, v, wr[v])
    COUNTS["classification"] += len(f.fwd_calls)
    print(f"{cid(cfg)}: {len(f.fwd_calls)} calls, {n} var arguments classified")


@pytest.mark.parametrize("cfg", MATRIX, ids=cid)
def test_sufficiency(cfg):
    f, dry, rw, deps = built(*cfg)
    haz = fr.hazards(rw)
    reach = fr.closure(deps)
    missing = [(i, j, f.fwd_calls[i].tag, f.fwd_calls[j].tag) for i, j in sorted(haz) if i not in reach[j]]
    assert not missing, missing
    COUNTS["sufficiency"] += len(f.fwd_calls)
    orders = fr.alt_orders(deps, tries=200 if cfg[0] in fr.SMALL_NETS else 4)      # (the small nets: the orders tests/test_gpu_fwd_deps.py runs)
    print(f"{cid(cfg)}: {len(deps)} calls, {sum(map(len, deps))} edges, {len(haz)} hazard pairs, {fr.free_positions(deps)} movable; moved: "
          + ", ".join(f"{k} {fr.moved_fraction(o):.2f}" for k, o in orders.items()))


@pytest.mark.parametrize("cfg", MATRIX, ids=cid)
def test_no_lost_parallelism(cfg):
    f, dry, rw, deps = built(*cfg)
    calls = f.fwd_calls
    assert len(deps) == len(calls)
    for i, d in enumerate(deps):
        assert all(0 <= j < i for j in d) and d == sorted(set(d)), (i, d)
        vi = rw[i][0] | set(rw[i][1])
        for j in d:
            assert vi & (rw[j][0] | set(rw[j][1])), (calls[j].tag, calls[i].tag, "an edge between calls that share no var")
    reach = fr.closure(deps)
    # no edge that the hazards do not ask for: a direct dependency is a hazard pair
    haz = fr.hazards(rw)
    for i, d in enumerate(deps):
        for j in d:
            assert (j, i) in haz, (calls[j].tag, calls[i].tag)
    # Concat copies into one var: mutually unreachable
    by_var = {}
    for i, c in enumerate(calls):
        if c.func in ("fwd_copy", "nhwc_copy"):
            by_var.setdefault(c.rfc.arg_map["out"].n, []).append(i)
    for v, ids in by_var.items():
        for a, b in itertools.combinations(ids, 2):
            assert a not in reach[b] and b not in reach[a], (v, calls[a].tag, calls[b].tag)
    if cfg[0] == "catcopy":
        assert sorted(map(len, by_var.values())) == [2], by_var      # (pa and na are copied, cb is written in place by its convolution)


def test_googlenet_branches_stay_parallel():
    f, dry, rw, deps = built("googlenet", "nhwc", {"fuse_levels": False, "fuse_siblings": False})
    reach = fr.closure(deps)
    idx = {}
    for i, c in enumerate(f.fwd_calls):
        for t in c.tag.split("+"):
            idx[t] = i
    cats = [o for o in f.cp.ops if o.type == "Concat"]
    assert len(cats) == 9
    for o in cats:
        producers = {p.top: p for p in f.cp.ops if p.type == "Convolution"}
        b1, b3, b5, bp = [producers[b] for b in o.bots]
        assert (tuple(b3.kern_sz), tuple(b5.kern_sz), tuple(bp.kern_sz)) == ((3, 3), (5, 5), (1, 1))
        branches = []
        for last in (b3, b5, bp):       # a branch: its last convolution and the op that feeds it (the reduce convolution; the pooling, where it still has a call)
            ids = {idx[last.tag]}
            if last.bot in idx or any(p.tag in idx and p.top == last.bot for p in f.cp.ops):
                feeder = next(p for p in f.cp.ops if p.top == last.bot and not p.in_place)
                if feeder.tag in idx:
                    ids.add(idx[feeder.tag])
            branches.append(ids)
        assert len(branches[0]) == 2 and len(branches[1]) == 2
        for x, y in itertools.combinations(branches, 2):
            assert not (x & y)
            for a in x:
                for b in y:
                    assert a not in reach[b] and b not in reach[a], (o.tag, f.fwd_calls[a].tag, f.fwd_calls[b].tag)


LEVEL_NETS = [n for n in NETS if n not in ("nin", "alexnet", "chain") + FP32_ONLY] + ["alexnet"]


@pytest.mark.parametrize("net", LEVEL_NETS)
def test_level_sets_and_groups_are_legal(net):
    f = built(net, "nhwc", {})[0]
    for kw, members_of in (({"fuse_levels": False}, f.level_sets), ({"fuse_levels": False, "fuse_siblings": False}, f.groups)):
        g, _, rw, _ = built(net, "nhwc", kw)
        truth = fr.closure(fr.hazard_deps(rw))
        idx = {c.tag: i for i, c in enumerate(g.fwd_calls)}
        for t, i in list(idx.items()):      # a convolution keeps its tag in front of whatever it took in (conv+pool+lrn, conv+eltwise+relu)
            idx.setdefault(t.split("+")[0], i)
        for members in members_of:
            ids = [idx[t] for t in members]
            assert len(set(ids)) == len(ids) >= 2, members
            for a, b in itertools.combinations(ids, 2):
                assert a not in truth[b] and b not in truth[a], (net, members, g.fwd_calls[a].tag, g.fwd_calls[b].tag)
    if net in ("googlenet", "incep"):
        assert f.level_sets and f.groups


def list_signature(cfg):
    """The call list of a configuration with everything a switch can change: tags, functions (a generated one by its source, a native one by its function op),
    the vars bound."""
    f, dry, rw, deps = built(*cfg)
    infos = {fi.func_name: fi for fi in dry.infos}
    def ident(fn):
        fi = infos.get(fn)
        return fn if fi is None else (fi.func_src or fi.op.to_str())
    return [(c.tag, c.func, ident(c.rfc.rtc_func_name), sorted((a, v.n) for a, v in c.rfc.arg_map.items() if v.is_var())) for c in f.fwd_calls]


def test_every_switch_changes_some_call_list():
    """A switch that changes no list of the matrix is checked in name only: every flip must differ from its net's default somewhere.  And the two whose effect
    depends on the layer sizes take effect where the tests say they do."""
    by_switch = {}
    for net, layout, kw in MATRIX:
        base = dict(fr.CHAIN_BASE) if net == "chain" else {}
        if kw == base:
            continue
        key = (layout, cid(("", "", {k: v for k, v in kw.items() if k not in base or kw[k] != base[k]})))
        by_switch.setdefault(key, []).append(list_signature((net, layout, kw)) != list_signature((net, layout, base)))
    idle = [k for k, v in by_switch.items() if not any(v)]
    assert idle == [("nhwc", cid(("", "", {"fuse_pool_lrn": "pool_first"})))], idle      # (the default value, listed for completeness: equal by construction)
    km = lambda cfg: [c.tag for c in built(*cfg)[0].fwd_calls if "filts_km" in c.rfc.arg_map and c.rfc.arg_map["filts_km"].is_var()]
    chain = dict(fr.CHAIN_BASE)
    assert km(("chain", "fp32", chain)) == ["c1"] and km(("chain", "fp32", dict(chain, filts_kmajor_once=False))) == []
    assert len(km(("nin128", "fp32", {}))) == 7 and km(("nin128", "fp32", {"filts_kmajor_once": False})) == []
    for cfg in (("chain", "fp32", chain), ("nin128", "fp32", {})):      # the k-major copy is a declared read of its convolution (fwd_deps_ref.OPTIONAL_NATIVE)
        f, dry, rw, deps = built(*cfg)
        for c, (rd, wr, dirs) in zip(f.fwd_calls, rw):
            if "filts_km" in c.rfc.arg_map:
                assert dirs["filts_km"] == "IN" and c.rfc.arg_map["filts_km"].n in rd
    assert built("chain", "fp32", dict(chain, **fr.F32_POOLS))[0].fused_pools == {"p1": "c4"}
    assert built("nin128", "fp32", {"fuse_f32_pools": True})[0].fused_pools == {"pool0": "conv2", "pool2": "conv3"}
    for cfg in (("chain", "fp32", dict(chain, **fr.F32_POOLS)), ("nin128", "fp32", {"fuse_f32_pools": True})):
        f, dry, rw, deps = built(*cfg)       # the convolution that took the pooling in reads the POOLING's input, and no call writes the pooled node
        for ptag, ctag in f.fused_pools.items():
            pool = next(o for o in f.cp.ops if o.tag == ptag); i = next(i for i, c in enumerate(f.fwd_calls) if c.tag.split("+")[-1] == ctag or c.tag == ctag)
            assert f.var_of(pool.bot) in rw[i][0] and all(f.var_of(pool.top) not in w for _, w, _ in rw) and pool.top in f._lazy


def test_fixture_file_lists_the_gpu_configurations_ops():
    """tests/golden/ops/fwd-deps-ops.txt holds the native function ops of tests/test_gpu_fwd_deps.py's configurations, so that build() specialises them ahead of the
    GPU run; and those configurations are the issue's sixteen."""
    import os
    from boda_amd.op import read_ops
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops", "fwd-deps-ops.txt")
    have = [o.to_str() for o in read_ops(gold)]
    assert have == [o.to_str() for o in fr.fixture_ops()] and len(have) >= 40
    funcs = {o.get_func_name() for o in read_ops(gold)}
    assert {"hip_conv", "hip_conv_nhwc", nhwc.GRP_FUNC, nhwc.SET_FUNC, cpm.K1_CHAIN_FUNC, "hip_chan_affine", "hip_reduce", "hip_zero_if_non_pos"} <= funcs, funcs
    ids = [fr.config_id(c) for c in fr.GPU_CONFIGS]
    assert len(ids) == len(set(ids)) == 16
    kinds = set()
    for net, layout, kw in fr.GPU_CONFIGS:      # the small nets produce every kind of call the matrix above classifies, but for the copies (catcopy) and what only large layers select
        dry = DryRtc(); f = fr.make_driver(dry, net, layout, kw)
        kinds |= {c.func for c in f.fwd_calls}
        if (net, layout, kw) == ("incep", "nhwc", {}):
            assert f.level_sets and f.groups and f.fused_pools and f.fused_post and any("+" in t for s in f.level_sets for t in s)     # (sets that take groups)
        if net == "chain":
            assert bool(f.k1_chains) == (kw.get("fuse_k1_chains", True) is not False)
            assert bool(f.fused_pools) == bool(kw.get("fuse_f32_pools")) and bool(f._km_params) == kw.get("filts_kmajor_once", True)
        if (net, layout) == ("res", "nhwc"):
            assert bool(f.fused_residuals["folded"]) == kw.get("fuse_residual", True) and ("nhwc_eltwise" in {c.func for c in f.fwd_calls}) == (not kw.get("fuse_residual", True))
    assert kinds >= {"nhwc_xpose_in", nhwc.FUNC, nhwc.GRP_FUNC, nhwc.SET_FUNC, "nhwc_pool", "nhwc_pool_lrn", "nhwc_eltwise", "hip_conv", cpm.K1_CHAIN_FUNC, "fwd_pool", "fwd_lrn",
                     "hip_chan_affine", "hip_reduce", "hip_zero_if_non_pos"}, kinds


def test_zz_counts():
    """The size of what was checked (printed; run after the parametrised tests of this file)."""
    n_cfg = len(MATRIX)
    print(f"{n_cfg} configurations; (configuration, call) pairs checked: classification {COUNTS['classification']}, sufficiency {COUNTS['sufficiency']}")
    assert n_cfg == len({cid(c) for c in MATRIX})
    if COUNTS["classification"]:       # (the whole file ran)
        assert COUNTS["classification"] == COUNTS["sufficiency"] == sum(len(b[0].fwd_calls) for k, b in _BUILT.items() if k in {cid(c) for c in MATRIX})
