"""The ordered call list of a gradient-pipe object (ConvPipeBck's step, EvalPipe's batch) over one backend: `CallList` makes the calls' functions, compiles them, runs
the list eagerly with per-call times, captures it into a hipGraph -- serially or with the calls' true dependencies -- replays and destroys that graph, and releases the
functions it made.  What is uploaded before a pass and what advances behind it is its owner's business."""
from __future__ import annotations
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

from .cnn_op import IMG_SHARDS_FUNCS, on_img_shards, pipe_func_args
from .op import Op
from .rtc import RtcArg, RtcFuncCall, RtcFuncInfo


@dataclass
class BckCall:
    tag: str
    fop: Op                      # the annotated function op
    args: Dict[str, str]         # arg name -> var name (var args only; REF / by-value args follow from the function op)
    rfc: RtcFuncCall
    call_id: int = -1


class CallList:
    """calls: the BckCalls in run order.  funcs: the functions emit made, named <prefix>_<index of the call>_<native function> -- a call taken over with reuse() brings
    its owner's function and adds none.  graph: the captured hipGraph's id or None."""

    def __init__(self, rtc, prefix: str):
        self.rtc, self.prefix = rtc, prefix
        self.calls: List[BckCall] = []
        self.funcs: List[str] = []
        self.graph: Optional[int] = None
        self.alias: Dict[str, str] = {}          # a var that is a view of another var -> that var: deps() orders a call on the view as a call on the var
        self._infos: List[RtcFuncInfo] = []      # of the functions emitted since the last compile
        self._multi_dev = isinstance(getattr(rtc, "devices", None), list) and len(rtc.devices) > 1

    def emit(self, tag: str, fop: Op, args: Dict[str, str]) -> None:
        """Append one call of the annotated function op `fop` with its var args bound as `args` says; a REF arg carries its dims, a by-value arg a zero its owner
        rewrites.  Touches no backend: compile() makes the functions."""
        if self._multi_dev and fop.get_func_name() in IMG_SHARDS_FUNCS:   # (the only way these five run on img shards)
            fop = on_img_shards(fop)
        fname = f"{self.prefix}_{len(self.calls)}_{fop.get_func_name()}"
        spec = pipe_func_args(fop)
        am: Dict[str, RtcArg] = {}
        for an, io in spec:
            if io == "REF":
                am[an] = RtcArg.ref(fop.get_dims(an))
            elif io == "VAL":
                am[an] = RtcArg.scalar(0, "uint32_t")
            else:
                am[an] = RtcArg.var(args[an])
        self._infos.append(RtcFuncInfo(fname, "", [an for an, _ in spec], fop))
        self.calls.append(BckCall(tag, fop, dict(args), RtcFuncCall(fname, am)))
        self.funcs.append(fname)

    def reuse(self, c: BckCall) -> None:
        """Append another list's call as it is: its compiled function and arg bindings (the RtcFuncCall object itself)."""
        self.calls.append(BckCall(c.tag, c.fop, dict(c.args), c.rfc))

    def compile(self) -> None:
        self.rtc.compile(self._infos)
        self._infos = []

    def run(self, all_but_last: int = 0) -> Tuple[float, List[Tuple[str, str, float]]]:
        """Launch the calls in order -- all_but_last=n: without the last n -- and sync; -> (ms first-call-start to last-call-end, [(tag, function, ms)] per call)."""
        rtc = self.rtc
        todo = self.calls[:len(self.calls) - all_but_last] if all_but_last else self.calls
        for c in todo:
            c.call_id = rtc.run(c.rfc)
        rtc.finish_and_sync()
        ids = [c.call_id for c in todo]
        dur = rtc.get_dur(ids[0], ids[-1]) if ids else 0.0
        per_call = [(c.tag, c.fop.get_func_name(), rtc.get_dur(i, i)) for c, i in zip(todo, ids)]
        rtc.release_per_call_id_data()
        return dur, per_call

    def deps(self) -> List[List[int]]:
        """deps[i] = the earlier calls that call i must run after, from the IN / OUT kinds of each call's pipe_func_args on WHOLE vars: a call runs after the last
        writer of every var it reads or writes (read-after-write, write-after-write) and after every reader since of a var it writes (write-after-read).  The in-place
        arg `inout` is read and written; a var bound to an IN and an OUT arg of one call (an in-place hip_zero_if_non_pos) likewise.  The `in` of a zero_if_in_non_pos
        call is an IN like any other.  The params and det_drop_seed are only read inside a step and order nothing -- unless the
        driver has a solver: an arg of kind INOUT (w_i, h_i of hip_sgd_update) is read and written, so an update call follows every forward and backward reader of
        its params (write after read) and the writers of its gradients.  The hip_concat calls of one op fill disjoint
        channel ranges of one var; as whole-var writers they simply stay in list order among themselves, and a reader of the var follows the last of them."""
        writer: Dict[str, int] = {}
        readers: Dict[str, List[int]] = {}
        deps: List[List[int]] = []
        for i, c in enumerate(self.calls):
            am = c.rfc.arg_map
            rd, wr = set(), set()
            for an, io in pipe_func_args(c.fop):
                if io in ("IN", "INOUT") or an == "inout":
                    rd.add(self.alias.get(am[an].n, am[an].n))
                if io in ("OUT", "INOUT"):
                    wr.add(self.alias.get(am[an].n, am[an].n))
            d = {writer[v] for v in rd | wr if v in writer}
            for v in wr:
                d.update(readers.get(v, ()))
            d.discard(i)
            for v in rd:
                readers.setdefault(v, []).append(i)
            for v in wr:
                writer[v] = i; readers[v] = []
            deps.append(sorted(d))
        return deps

    def capture(self, deps: Optional[List[List[int]]] = None) -> int:
        """Capture the whole list into a hipGraph -- in launch order, or with `deps` as its edges; -> number of captured calls.  The owner has destroyed an earlier
        graph and run whatever step must come before a capture."""
        rtc = self.rtc
        rtc.finish_and_sync()
        rtc.graph_begin()
        for c in self.calls:   # (a call that raises inside a capture: the backend drops the capture before it rethrows)
            rtc.run(c.rfc)
        if deps is not None:
            self.graph = rtc.graph_end_deps(deps); n = len(self.calls)
        else:
            self.graph, n = rtc.graph_end()
        return n

    def replay(self) -> float:
        """One launch of the captured graph, synced; -> ms of the whole replay."""
        rtc = self.rtc
        cid = rtc.graph_launch(self.graph)
        rtc.finish_and_sync()
        dur = rtc.get_dur(cid, cid)
        rtc.release_per_call_id_data()
        return dur

    def destroy_graph(self) -> None:
        if self.graph is not None:
            self.rtc.graph_destroy(self.graph); self.graph = None

    def release(self) -> None:
        """Destroy the graph (before the funcs and vars its kernel nodes point into) and release the functions this list made."""
        self.destroy_graph()
        for f in self.funcs:
            self.rtc.release_func(f)
        self.funcs, self.calls = [], []
