"""What every call of a ConvPipeFwd call list reads and writes, from the functions' DECLARED argument directions -- an account that shares nothing with
ConvPipeFwd._call_rw / _call_deps, which go by how the arguments are spelled -- and, from it, the true hazards of the list.

Directions come from
  * native functions (an empty source, a func_name with an arg table): cnn_op.pipe_func_args(function op) / NATIVE_ARGS, nhwc.ARGS for the members of
    hip_conv_nhwc_grp / hip_conv_nhwc_set (whose own lists, nhwc.group_arg_names / multi_arg_names, give a member's args a suffix _<m>): IN is a read, OUT a write;
  * generated functions (CUCL source: conv_pipe.FWD_SRC, nhwc.FWD_SRC, nhwc.XPOSE_SRC and every source a recording backend was handed): the `// CUCL IN | OUT |
    INOUT | REF` annotation of a parameter where the template has one, else the pointee's const-ness in the kernel's signature (`GASQ T const *` read, `GASQ T *`
    written).  An INOUT parameter is a read and a write; so is the one parameter listed in RAW_INOUT, which a raw-source kernel loads before it stores.
REF arguments and scalars are neither.  Two tables keyed by FUNCTION fill what no declaration states: the optional var argument of hip_conv, and the in-place
parameters of the raw-source kernels.

A write carries the channel range [lo, hi) of the var it goes to, None for the whole var: out_chan_off (+ the function op's out_chans), a copy's off_out / chw_in
or off8 / C8_in.  Two writes conflict when their ranges overlap, a read conflicts with any write of the same var."""
import re

from boda_amd import conv_pipe as cpm
from boda_amd import nhwc
from boda_amd.cnn_op import NATIVE_ARGS, pipe_func_args

OPTIONAL_NATIVE = {"hip_conv": {"filts_km": "IN"}}     # native_kernels_t::conv( ..., float const *filts_km ): the caller's k-major copy of filts, or none
RAW_INOUT = {"fwd_relu": {"inout"}, "nhwc_relu": {"inout"}}     # `GASQ T * const inout`, compared before it is stored: a read as well as the write the signature declares
_NHWC_DIR = dict(nhwc.ARGS)


# ---- generated functions: directions from the source text
def _param_region(src, start):
    depth, i = 0, start
    while True:
        ch = src[i]
        if ch == "(":
            depth += 1
        elif ch == ")":
            depth -= 1
            if depth == 0:
                return src[start + 1:i]
        i += 1


def parse_kernels(src):
    """{kernel name: {pointer parameter: "IN" | "OUT" | "INOUT" | "REF"}} of every CUCL_GLOBAL_KERNEL in `src`."""
    out = {}
    for m in re.finditer(r"CUCL_GLOBAL_KERNEL\s+(?:__launch_bounds__\(\s*\d+\s*\)\s+)?void\s+(\w+)\s*\(", src):
        name = m.group(1)
        region = _param_region(src, m.end() - 1)
        anno = {}
        pieces = re.split(r"(//[^\n]*)", region)        # code, comment, code, comment ...: an annotation belongs to the parameter in front of it
        code = ""
        for p in pieces:
            if p.startswith("//"):
                a = re.match(r"//\s*CUCL\s+(INOUT|IN|OUT|REF)\b", p)
                if a:
                    last = re.findall(r"(\w+)\s*,?\s*$", code)
                    assert last, (name, p)
                    anno[last[0]] = a.group(1)
            else:
                code += p
        dirs = {}
        for prm in code.split(","):
            prm = " ".join(prm.split())
            if "*" not in prm:
                continue     # by value
            pm = re.match(r"^GASQ (.+?)\*\s*(?:const\s+)?(\w+)$", prm)
            assert pm, (name, prm)
            pointee, pn = pm.group(1), pm.group(2)
            dirs[pn] = anno.get(pn, "IN" if re.search(r"\bconst\b", pointee) else "OUT")
        out[name] = dirs
    return out


_STATIC = {}


def static_kernels():
    if not _STATIC:
        for src in (cpm.FWD_SRC, nhwc.FWD_SRC, nhwc.XPOSE_SRC):
            _STATIC.update(parse_kernels(src))
    return _STATIC


class Directions:
    """Per call of a ConvPipeFwd built on a recording backend: {arg name: "IN" | "OUT" | "INOUT" | "REF" | "VAL"} for every argument the call binds."""

    def __init__(self, drv, dry):
        self.drv, self.dry = drv, dry
        self.infos = {}
        for fi in dry.infos:
            self.infos[fi.func_name] = fi
        self.generated = dict(static_kernels())
        for fi in dry.infos:
            if fi.func_src:
                self.generated.update(parse_kernels(fi.func_src))

    def func_op(self, fname):
        return self.infos[fname].op

    def base_name(self, fname):
        fi = self.infos.get(fname)
        return fi.op.get_func_name() if (fi is not None and not fi.func_src and fi.op.has_func_name()) else fname

    def of_call(self, c):
        fname, am = c.rfc.rtc_func_name, c.rfc.arg_map
        fi = self.infos.get(fname)
        if fname in self.generated and (fi is None or fi.func_src or fname in static_kernels()):
            decl = self.generated[fname]
            dirs = {}
            for a, v in am.items():
                if v.is_var():
                    assert a in decl, (c.tag, fname, a, "a var argument that the kernel's signature does not declare as a pointer")
                    d = decl[a]
                    dirs[a] = "INOUT" if a in RAW_INOUT.get(fname, ()) else d
                else:
                    dirs[a] = "REF" if v.v is None else "VAL"
            names = self.infos[fname].arg_names if fi is not None else (cpm.FWD_FUNCS.get(fname) or nhwc.FWD_FUNCS.get(fname) or nhwc.XPOSE_FUNCS.get(fname))
            assert set(am) == set(names), (c.tag, fname, sorted(am), sorted(names))
            return dirs
        assert fi is not None and not fi.func_src, (c.tag, fname, "neither a generated function with a source nor a compiled native function")
        op = fi.op; base = op.get_func_name()
        if base == nhwc.SET_FUNC:
            return self._set_dirs(c, op)
        if base == nhwc.GRP_FUNC:
            n = sum(1 for k in op.nda_vals if re.fullmatch(r"out_\d+", k))
            assert fi.arg_names == nhwc.group_arg_names(n)
            return self._classify(c, self._grp_decl(n), am)
        decl = dict(pipe_func_args(op)); decl.update(OPTIONAL_NATIVE.get(base, {}))
        assert [a for a, _ in pipe_func_args(op)] == list(fi.arg_names), (c.tag, fi.arg_names)
        return self._classify(c, decl, am)

    @staticmethod
    def _grp_decl(n):
        decl = {a: _NHWC_DIR[a] for a in ("filts", "biases", "in", "stride", "in_pad")}
        decl["grp"] = "REF"
        for m in range(n):
            decl[f"out_{m}"] = _NHWC_DIR["out"]
        return decl

    @staticmethod
    def _classify(c, decl, am, sfx=""):
        dirs = {}
        for a, v in am.items():
            if v.is_var():
                assert a in decl and decl[a] in ("IN", "OUT"), (c.tag, a + sfx, "a var argument without a declared direction")
                dirs[a + sfx] = decl[a]
            else:
                dirs[a + sfx] = "REF" if v.v is None else "VAL"
        return dirs

    def _set_dirs(self, c, sop):
        """A set's call binds, for member m, the args of the member's own call with the suffix _<m> (ConvPipeFwd._fuse_level_sets); the member is a hip_conv_nhwc
        function (nhwc.ARGS) or a sibling group (the set's op then holds grp_<m>)."""
        am = c.rfc.arg_map
        n = sop.get_dims("multi").dsz("n")
        dirs = {"multi": "REF"}
        assert "multi" in am and not am["multi"].is_var()
        seen = {"multi"}
        for m in range(n):
            sfx = f"_{m}"
            mam = {a[:-len(sfx)]: v for a, v in am.items() if a.endswith(sfx) and a != "multi"}
            seen |= {a + sfx for a in mam}
            if sop.has(f"grp_{m}"):
                k = len(sop.get_dims(f"grp_{m}").sizes) - 1
                decl = self._grp_decl(k)
            else:
                decl = dict(_NHWC_DIR)
            dirs.update(self._classify(c, decl, mam, sfx))
        assert seen == set(am), (c.tag, sorted(set(am) - seen))
        return dirs

# ---- read / write sets with written ranges
def _scalar(am, a):
    return int(am[a].v[0])


def _out_chans(op, filts="filts"):
    return op.get_dims(filts).dsz("out_chan")


def call_rw(D, c):
    """-> (set of vars read, {var written: [(lo, hi) channel range | None for the whole var, ...]}, {arg: direction})."""
    drv, dry = D.drv, D.dry
    dirs = D.of_call(c)
    am = c.rfc.arg_map
    fname = c.rfc.rtc_func_name; base = D.base_name(fname)
    reads, writes = set(), {}
    for a, d in dirs.items():
        if d in ("IN", "INOUT"):
            reads.add(am[a].n)
    def chans(vn):
        return dry.get_var_dims(vn).dsz("chan")
    for a, d in dirs.items():
        if d not in ("OUT", "INOUT"):
            continue
        vn = am[a].n; rng = None
        if base in ("hip_conv", "hip_conv_nhwc", "hip_conv_winograd", "hip_conv_bf16", cpm.K1_CHAIN_FUNC) and "out_chan_off" in am:
            lo = _scalar(am, "out_chan_off"); rng = (lo, lo + _out_chans(D.func_op(fname), "filts2" if base == cpm.K1_CHAIN_FUNC else "filts"))
        elif base == nhwc.GRP_FUNC:
            m = a[len("out_"):]
            if f"out_chan_off_{m}" in am:
                lo = _scalar(am, f"out_chan_off_{m}"); rng = (lo, lo + D.func_op(fname).get_dims("grp").sizes[int(m)])
        elif base == nhwc.SET_FUNC:
            sop = D.func_op(fname)
            parts = a.split("_")       # out_<m> of a plain member, out_<k>_<m> of member m's k-th group member
            m = parts[-1]
            if len(parts) == 3:
                k = parts[1]
                if f"out_chan_off_{k}_{m}" in am:
                    lo = _scalar(am, f"out_chan_off_{k}_{m}"); rng = (lo, lo + sop.get_dims(f"grp_{m}").sizes[int(k)])
            elif f"out_chan_off_{m}" in am:
                lo = _scalar(am, f"out_chan_off_{m}"); rng = (lo, lo + _out_chans(sop, f"filts_{m}"))
        elif fname == "fwd_copy":
            hw = _scalar(am, "chw_out") // chans(vn)
            assert _scalar(am, "off_out") % hw == 0 and _scalar(am, "chw_in") % hw == 0
            rng = (_scalar(am, "off_out") // hw, (_scalar(am, "off_out") + _scalar(am, "chw_in")) // hw)
        elif fname == "nhwc_copy":
            assert 8 * _scalar(am, "C8_out") == chans(vn)
            rng = (8 * _scalar(am, "off8"), 8 * (_scalar(am, "off8") + _scalar(am, "C8_in")))
        if rng is not None:
            assert 0 <= rng[0] < rng[1] <= chans(vn), (c.tag, a, rng, chans(vn))
            if rng == (0, chans(vn)):
                rng = None
        writes.setdefault(vn, []).append(rng)
    return reads, writes, dirs


def overlap(r0, r1):
    return r0 is None or r1 is None or (r0[0] < r1[1] and r1[0] < r0[1])


def all_rw(drv, dry):
    D = Directions(drv, dry)
    return [call_rw(D, c) for c in drv.fwd_calls]


def hazards(rw):
    """The pairs i < j of calls that must stay in this order: j reads what i writes, j writes what i reads, or both write overlapping ranges of a var."""
    pairs = set()
    for j, (rj, wj, _) in enumerate(rw):
        for i in range(j):
            ri, wi, _ = rw[i]
            if (set(wi) & rj) or (ri & set(wj)) or any(overlap(a, b) for v in set(wi) & set(wj) for a in wi[v] for b in wj[v]):
                pairs.add((i, j))
    return pairs


def closure(deps):
    """reach[i] = every call that call i runs after, directly or through others (deps[i] holds only indices < i)."""
    reach = []
    for d in deps:
        r = set(d)
        for j in d:
            r |= reach[j]
        reach.append(r)
    return reach


def hazard_deps(rw):
    deps = [[] for _ in rw]
    for i, j in sorted(hazards(rw)):
        deps[j].append(i)
    return deps


# ---- the small nets of tests/test_gpu_fwd_deps.py (and of the host-only matrix): the smallest that still produce every kind of call
def _incep_module(lines, m, bot):
    def conv(tag, b, oc, k, pad=0):
        lines.append(f"conv {tag} {b} {tag} {oc} {k} {k} 1 1 {pad} {pad}"); lines.append(f"relu {tag}_relu {tag} {tag}")
        return tag
    conv(f"{m}_1x1", bot, 16, 1)
    conv(f"{m}_3x3", conv(f"{m}_3x3r", bot, 8, 1), 24, 3, 1)
    conv(f"{m}_5x5", conv(f"{m}_5x5r", bot, 8, 1), 8, 5, 2)
    lines.append(f"pool {m}_pool {bot} {m}_pool 3 3 1 1 1 1 0 0")
    conv(f"{m}_pp", f"{m}_pool", 8, 1)
    lines.append(f"concat {m}_cat {m}_out {m}_1x1,{m}_3x3,{m}_5x5,{m}_pp")
    return f"{m}_out"


def incep_net(batch=2, hw=45):
    """A 7x7/2 stem + ReLU + max pool 3x3/2 + LRN 5, two inception modules in a row (the second reads the first one's Concat), a global average pool and a 1x1 'fc'."""
    lines = [f"input data 3 {hw} {hw}", "conv conv1 data conv1 64 7 7 2 2 3 3", "relu conv1_relu conv1 conv1", "pool pool1 conv1 pool1 3 3 2 2 0 0 0 0",
             "lrn norm1 pool1 norm1 5 0.0001 0.75 1.0"]
    n = _incep_module(lines, "a", "norm1")
    n = _incep_module(lines, "b", n)
    lines += [f"pool gpool {n} gpool 0 0 1 1 0 0 1 1", "conv fc gpool fc 16 1 1 1 1 0 0"]
    return cpm.pipe_from_spec("incep", lines, batch)


def chain_net(batch=2, hw=45):
    """fp32: conv 3x3 -> 1x1 -> 1x1 (the k1 chain, its middle node lazy), max pool 3x3/2, conv 3x3 pad 1 (fuse_f32_pools), LRN, average pool, Dropout, 1x1.
    45 x 45 planes and 256 channels out of the first convolution: the smallest at which a plan reads its filters k-major (filts_km, filts_kmajor_once) -- at
    23 x 23 and 32 channels none does, and the switch would change nothing."""
    lines = [f"input data 3 {hw} {hw}", "conv c1 data c1 256 3 3 1 1 0 0", "relu c1_relu c1 c1", "conv c2 c1 c2 32 1 1 1 1 0 0", "relu c2_relu c2 c2",
             "conv c3 c2 c3 32 1 1 1 1 0 0", "relu c3_relu c3 c3", "pool p1 c3 p1 3 3 2 2 0 0 0 0", "conv c4 p1 c4 32 3 3 1 1 1 1", "relu c4_relu c4 c4",
             "lrn n1 c4 n1 5 0.0001 0.75 1.0", "pool p2 n1 p2 2 2 2 2 0 0 1 0", "drop d1 p2 p2", "conv c5 p2 c5 16 1 1 1 1 0 0"]
    return cpm.pipe_from_spec("chain", lines, batch)


def res_net(batch=2, hw=64):
    """ResNet-50 up to res2c: BatchNorm / Scale runs, a projection shortcut and two identity shortcuts."""
    import resnet_ref as rr
    return rr.truncated(cpm.resnet50(batch, hw), "res2c")


SMALL_NETS = {"incep": incep_net, "chain": chain_net, "res": res_net}
HOST_NETS = {}     # nets of the host-only matrix (tests/test_fwd_deps_cpu.py fills it)
CHAIN_BASE = {"fuse_k1_chains": "all"}     # the chain net is below the size from which 1x1 pairs are chained by default: "all" lifts that threshold, nothing else
# fuse_f32_pools by itself skips a convolution whose plan keeps several K tiles in flight -- every plan of a layer this small; the project's switch for "fuse those too"
# (tests/test_gpu_fullnet.py sets it for the same reason) makes the fusion happen here.  `env` is not a ConvPipeFwd switch: make_driver sets it around init()
F32_POOLS = {"fuse_f32_pools": True, "env": {"BODAHIP_F32_POOL_ALL": "1"}}
NHWC = "nhwc"
# (net, layout, switches): one GPU case each
GPU_CONFIGS = [("incep", NHWC, {}), ("incep", NHWC, {"fuse_levels": False}), ("incep", NHWC, {"fuse_siblings": False}), ("incep", NHWC, {"sets_take_groups": False}),
               ("incep", NHWC, {"fuse_pools": False}), ("incep", NHWC, {"fuse_post": False}), ("incep", NHWC, {"fuse_pool_lrn": True, "fuse_post": False}),
               ("incep", NHWC, {"spec_fwd": False}), ("incep", "fp32", {}),
               ("chain", "fp32", dict(CHAIN_BASE)), ("chain", "fp32", {"fuse_k1_chains": False}), ("chain", "fp32", dict(CHAIN_BASE, **F32_POOLS)),
               ("chain", "fp32", dict(CHAIN_BASE, filts_kmajor_once=False)),
               ("res", "fp32", {}), ("res", NHWC, {}), ("res", NHWC, {"fuse_residual": False})]


def config_id(cfg):
    net, layout, kw = cfg
    return "-".join([net, layout] + ([f"{k}={v}" for k, v in kw.items() if k != "env"] + [f"{k}={v}" for k, v in kw.get("env", {}).items()] or ["default"]))


def make_driver(rtc, net, layout, kw, cp=None, params=None):
    from boda_amd.cnn_op import OpTune
    import os
    full = {k: v for k, v in kw.items() if k != "env"}
    env = kw.get("env", {}); old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        f = cpm.ConvPipeFwd(rtc, OpTune(hip_dtype="bf16", hip_layout="nhwc") if layout == NHWC else None, **full)
        f.init(cp if cp is not None else (SMALL_NETS.get(net) or HOST_NETS[net])(), params)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return f


# ---- orders that respect a dependency list
def topo_order(deps, pick):
    done, order = set(), []
    while len(order) < len(deps):
        ready = [i for i in range(len(deps)) if i not in done and all(j in done for j in deps[i])]
        i = pick(ready)
        done.add(i); order.append(i)
    return order


QUARTER = 0.25     # an order shows something where it differs from the list order in at least this fraction of its positions


def alt_orders(deps, seeds=(17, 18), tries=200):
    """The orders the call list is executed in besides its own: always the highest-index ready call, and one seeded random topological order per seed -- the first
    of up to `tries` draws from that seed's stream that moves a quarter of the positions, else the draw that moved most."""
    import numpy as np
    orders = {"latest ready": topo_order(deps, max)}
    for s in seeds:
        rng = np.random.default_rng(s)
        best = None
        for _ in range(tries):
            o = topo_order(deps, lambda r: r[int(rng.integers(len(r)))])
            if best is None or moved_fraction(o) > moved_fraction(best):
                best = o
            if moved_fraction(best) >= QUARTER:
                break
        orders[f"random topological (seed {s})"] = best
    return orders


def moved_fraction(order):
    return sum(1 for p, i in enumerate(order) if p != i) / float(len(order))


def free_positions(deps):
    """How many calls some valid order can move at all: those that are not ordered against every other call (an upper bound on the positions in which an order
    can differ from the list's).  A pure chain has none."""
    reach = closure(deps); n = len(deps)
    after = [set() for _ in range(n)]
    for i, r in enumerate(reach):
        for j in r:
            after[j].add(i)
    return sum(1 for i in range(n) if len(reach[i]) + len(after[i]) < n - 1)


def can_be_covered(deps):
    """Can any valid order differ from the list order in a quarter of its positions?  (No: a chain, or close to one -- fewer movable calls than that.)"""
    return free_positions(deps) >= QUARTER * len(deps)


# ---- the native function ops of the GPU configurations (tests/golden/ops/fwd-deps-ops.txt: build() specialises them ahead of the GPU run)
def fixture_ops():
    seen, out = set(), []
    for net, layout, kw in GPU_CONFIGS:
        dry = cpm.DryRtc()
        make_driver(dry, net, layout, kw)
        for fi in dry.infos:
            if fi.func_src or fi.op is None or not fi.op.has_func_name():
                continue
            fn = fi.op.get_func_name()
            if not fn.startswith("hip_") or fn == cpm.FILTS_KMAJOR_FUNC or "_xpose_" in fn or not fi.op.nda_vals:
                continue
            if fi.op.to_str() not in seen:
                seen.add(fi.op.to_str()); out.append(fi.op)
    return out
