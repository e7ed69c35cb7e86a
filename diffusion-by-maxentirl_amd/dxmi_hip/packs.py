"""The packed-weight cache of the nets: bf16 MFMA-fragment copies of the fp32 parameters, refreshed after every optimiser step at
the device addresses they were first given, because captured hipGraphs hold those addresses (dxmi_hip/graph.py)."""
import torch

from . import ops


class WeightPacks:
    """One packed-weight set of `module`: a dict, key -> PackedConvWeight | tensor | host value, filled by `build(module, packs)`
    inside one ops.pack_batch().  get() brings it up to date with the parameters:
      * key unchanged — the (data_ptr, _version) of ops.fast_parameters(module) — nothing runs;
      * parameters updated in place (same addresses, new versions): REPLAY.  The staged sources are refilled, the descriptor array
        of the build is launched again (ops.PackPlan), the derived packs are rewritten into their buffers and the entries a
        backward packed on demand are dropped.  No buffer is allocated and ops.PACK_GENERATION stays;
      * anything else — first use, moved parameters, ops.PACK_PLAN_REPLAY off, DXMI_PACK_BATCH=0 (no plan is recorded) — FULL BUILD:
        a fresh set in fresh buffers, ops.PACK_GENERATION bumped once (every StepGraph re-captures itself).
    A replay packs from the addresses the build packed from, so it needs every packed source to be a parameter's own storage
    or a staged buffer: a net with a packed parameter that is not fp32-contiguous (pack() had to copy it) takes a full build at
    every refresh, and its graphs re-capture every step.  No program of this repository creates such a net."""

    def __init__(self, module, build):
        self.module, self.build = module, build
        self.forget()

    def forget(self):
        """Drop the set: the next get() is a full build."""
        self.entries = self.key = self.plan = None

    @property
    def exists(self):
        return self.entries is not None

    # ---- for build()
    def pack(self, key, w, **kw):
        """entries[key] = ops.pack_conv_weight(w, **kw), w a parameter (or a view of one) or a staged buffer."""
        src = w.detach().contiguous().float()
        self.direct &= src.data_ptr() == w.data_ptr() and src.untyped_storage().data_ptr() in self.sources
        self.entries[key] = ops.pack_conv_weight(src, **kw)

    def stage(self, shape, fill, zero=False):
        """A persistent fp32 buffer for a source that is no parameter (concatenated weights, bias rows, the zero-padded conv_out):
        fill(out) runs now and before every replay."""
        out = (torch.zeros if zero else torch.empty)(shape, dtype=torch.float32, device=self.device)
        fill(out)
        self.fills.append((fill, out))
        self.sources.add(out.untyped_storage().data_ptr())
        return out

    def stage_cat(self, parts):
        """The staged concatenation (dim 0) of the parameters `parts`."""
        shape = (sum(t.shape[0] for t in parts),) + tuple(parts[0].shape[1:])
        return self.stage(shape, lambda out: torch.cat([t.detach() for t in parts], 0, out=out))

    def derived(self, key, make):
        """entries[key] = make(None), a pack that is a launch of its own; make(out) rewrites it at every replay."""
        self.entries[key] = make(None)
        self.fills_after.append((make, self.entries[key]))

    # ---- for the nets
    def get(self):
        key = param_key(self.module)
        if self.entries is not None and key == self.key:
            return self.entries
        in_place = self.entries is not None and len(key) == len(self.key) and all(a[0] == b[0] for a, b in zip(key, self.key))
        if in_place and self.plan is not None and self.direct and ops.PACK_PLAN_REPLAY:
            for fn, out in self.fills:
                fn(out)
            self.plan.replay()
            for fn, out in self.fills_after:
                fn(out)
            self.drop_on_demand()
        else:
            params = list(ops.fast_parameters(self.module))
            self.device = params[0].device
            self.sources = {p.untyped_storage().data_ptr() for p in params}
            self.entries, self.fills, self.fills_after, self.direct = {}, [], [], True
            try:
                with ops.pack_batch() as pb:      # every pack() of the build runs in a few multi-tensor launches
                    self.build(self.module, self)
            except BaseException:
                self.forget()
                raise
            self.plan, self.planned = pb.plan, frozenset(self.entries)
            ops.PACK_GENERATION += 1
        self.key = key
        return self.entries

    def on_demand(self, key, make):
        """entries[key], made by make() when a backward first needs it; dropped at every refresh."""
        if key not in self.entries:
            self.entries[key] = make()
        return self.entries[key]

    def drop_on_demand(self):
        for k in [k for k in self.entries if k not in self.planned]:
            del self.entries[k]


def param_key(module):
    # torch bumps _version on every in-place update (optimizer.step, load_state_dict, .to())
    return tuple((p.data_ptr(), p._version) for p in ops.fast_parameters(module))


class PackedWeights:
    """Mixin of a net with a forward set `_packs` (made in its __init__) and, once a backward has asked for one, a transposed set
    `_packs_t`.  dxmi_hip/graph.py finds such modules by refresh_packs / prepare_capture."""

    _packs_t = None

    def _param_key(self):
        return param_key(self)

    @property
    def _packed_key(self):
        """The parameter key the forward set was last brought up to date with (None: not built)."""
        return self._packs.key

    def packed(self):
        return self._packs.get()

    def refresh_packs(self):
        """Bring every packed-weight set of the net that exists up to date with the parameters (no-op when they are)."""
        self._packs.get()
        if self._packs_t is not None and self._packs_t.exists:
            self._packs_t.get()

    def prepare_capture(self):
        """Before a StepGraph capture: entries a backward packed on demand are dropped, so that the captured step packs them
        itself; the rest is refreshed eagerly."""
        if self._packs_t is not None and self._packs_t.exists:
            self._packs_t.drop_on_demand()
        self.refresh_packs()
