"""Flat parameter arena: every parameter of a model lives in ONE fp32 buffer (master) with a bf16
shadow (what the GEMMs read), and — for trainable models — one fp32 gradient buffer and the two
AdamW moment buffers of the same layout.

Why (MI355X-first): 288 GB of HBM make full replication trivial, a single fused AdamW
launch streams the whole optimizer state at HBM rate, the DDP gradient all-reduce works on
contiguous slices with no flatten/unflatten copies, and q/k/v projection weights sit next to each
other so one GEMM with N = 3d serves all three.  nn.Parameter objects keep the reference's names
(state_dict-compatible with MFULL); their .data are views into the arena.
"""
import torch

from . import kernels as K

ALIGN = 32          # elements: keeps every slot 64 B (bf16) / 128 B (fp32) aligned


def _round(n, a=ALIGN):
    return (n + a - 1) // a * a


class ParamArena:
    def __init__(self, model, device, trainable=True, pad_rows=None):
        """pad_rows: {id(param): padded_row_count} — e.g. the tied embedding padded to a multiple of 32 rows so the
        LM-head dgrad can run with K = V_pad (extra rows stay exactly zero)."""
        pad_rows = pad_rows or {}
        group_of = {}
        for m in model.modules():
            if hasattr(m, "arena_groups"):
                for g in m.arena_groups():
                    for p in g:
                        group_of.setdefault(id(p), g)
        groups, seen = [], set()
        for p in model.parameters():            # registration order; a fused group is placed where its first member appears
            if id(p) in seen:
                continue
            g = [q for q in group_of.get(id(p), [p]) if id(q) not in seen]
            groups.append(g)
            seen.update(id(q) for q in g)
        self.slots = {}
        off = 0
        for g in groups:
            off = _round(off)
            for p in g:
                n = p.numel()
                if id(p) in pad_rows:
                    n = pad_rows[id(p)] * p.shape[1]
                self.slots[id(p)] = (off, p.numel(), n)
                off += n
        self.n = _round(off, 1024)
        self.device = torch.device(device)
        self.trainable = trainable
        self.flat32 = torch.zeros(self.n, device=self.device, dtype=torch.float32)
        self.flat16 = torch.zeros(self.n, device=self.device, dtype=torch.bfloat16)
        self.grad = torch.zeros(self.n, device=self.device, dtype=torch.float32) if trainable else None
        self.exp_avg = self.exp_avg_sq = None
        self.ema = None
        self.refresh_hooks = []            # callables re-deriving packed copies of weights after refresh_shadow()
        self.params = []
        for p in model.parameters():
            if id(p) in {id(q) for q in self.params}:
                continue
            o, n, _ = self.slots[id(p)]
            self.flat32[o:o + n].copy_(p.data.reshape(-1).to(self.device, torch.float32))
            p.data = self.flat32[o:o + n].view(p.shape)
            p.w16 = self.flat16[o:o + n].view(p.shape)
            if trainable and p.requires_grad:
                p.grad = self.grad[o:o + n].view(p.shape)
            self.params.append(p)
        self.refresh_shadow()
        for m in model.modules():
            if hasattr(m, "bind_arena"):
                m.bind_arena(self)

    # ---- views ---------------------------------------------------------------------------------
    def offset(self, p):
        return self.slots[id(p)][0]

    def view16(self, p, rows=None):
        """bf16 shadow of p, optionally with padded row count."""
        o, n, cap = self.slots[id(p)]
        if rows is None:
            return self.flat16[o:o + n].view(p.shape)
        assert rows * p.shape[1] <= cap
        return self.flat16[o:o + rows * p.shape[1]].view(rows, p.shape[1])

    def fused(self, plist, which):
        """contiguous view over adjacent parameters (e.g. [k,v,q] weights -> [3d, d])."""
        o0 = self.offset(plist[0])
        tot, o = 0, o0
        for p in plist:
            assert self.offset(p) == o, "parameters are not adjacent in the arena"
            o += p.numel(); tot += p.numel()
        buf = {"w16": self.flat16, "f32": self.flat32, "grad": self.grad}[which]
        if buf is None:
            return None
        v = buf[o0:o0 + tot]
        if plist[0].dim() == 2:
            return v.view(-1, plist[0].shape[1])
        return v

    # ---- maintenance ---------------------------------------------------------------------------
    def refresh_shadow(self):
        if self.device.type == "cuda":
            K.cast_f32_bf16(self.flat32, self.flat16)
        else:
            # host-side arenas exist only for layout / reducer tests (gloo); no compute op accepts CPU tensors
            self.flat16.copy_(self.flat32)
        for hook in self.refresh_hooks:
            hook()

    def init_optimizer_state(self):
        self.exp_avg = torch.zeros(self.n, device=self.device, dtype=torch.float32)
        self.exp_avg_sq = torch.zeros(self.n, device=self.device, dtype=torch.float32)

    def init_ema(self):
        """fp32 moving average of the weights (FusedAdamW(ema_decay=...)), same layout as flat32; it starts as a copy of it."""
        self.ema = self.flat32.clone()

    def bucket_slices(self, bucket_bytes=256 << 20):
        """contiguous [start, end) element ranges of the gradient arena, in REVERSE layout order
        (the order backward finishes them), for the DDP reducer."""
        per = max(4, bucket_bytes // 16 * 4)          # whole 16-byte groups: a bucket is also a range of the vectorised AdamW kernel
        out, end = [], self.n
        while end > 0:
            start = max(0, end - per)
            out.append((start, end))
            end = start
        return out

    def group_table(self, named_params, spec, default_wd):
        """parameter-group table of this arena (see group_table below)."""
        return group_table(self, named_params, spec, default_wd)


# ---- parameter groups ------------------------------------------------------------------------------------------------------
# A spec is plain data (it travels in checkpoints):
#   [{"match": regex | [parameter names], "lr_scale": None | float, "weight_decay": None | float, "frozen": None | bool}, ...]
# matched with re.search against the names of named_parameters() (the reference's names).  Every field resolves on its own: a
# parameter takes each of lr_scale / weight_decay / frozen from the FIRST entry that matches it AND sets that field (not None);
# what no entry sets is the default {1.0, the optimizer's weight_decay, False}.  With entries that set all three fields this is
# "the first matching entry wins"; with entries that set one field each, a parameter can be both scaled and un-decayed.
# A parameter reachable under several names (the tied embedding / LM head, the attention weights tied by init_attn_weight) is known
# by its FIRST name in named_parameters() only; an entry that matches no parameter raises (a silent typo is worse).
_SPEC_FIELDS = ("lr_scale", "weight_decay", "frozen")
BLOCK = 1024        # elements per first_seg entry (arena sizes are multiples of it)


def normalize_spec(spec):
    """validated plain-data copy of a spec (None stays None)."""
    if spec is None:
        return None
    out = []
    for k, e in enumerate(spec):
        if not isinstance(e, dict) or "match" not in e or set(e) - {"match", *_SPEC_FIELDS}:
            raise ValueError(f"param_groups[{k}]: an entry is a dict with 'match' and any of {_SPEC_FIELDS}, got {e!r}")
        m = e["match"]
        if isinstance(m, str):
            import re
            try:
                re.compile(m)
            except re.error as err:
                raise ValueError(f"param_groups[{k}]: bad regex {m!r}: {err}") from None
        else:
            m = [str(x) for x in m]
            if not m:
                raise ValueError(f"param_groups[{k}]: empty name list")
        lr, wd, fr = e.get("lr_scale"), e.get("weight_decay"), e.get("frozen")
        if lr is not None and not (float(lr) >= 0.0 and float(lr) < float("inf")):
            raise ValueError(f"param_groups[{k}]: lr_scale={lr!r} must be a finite number >= 0")
        if wd is not None and not (float(wd) >= 0.0 and float(wd) < float("inf")):
            raise ValueError(f"param_groups[{k}]: weight_decay={wd!r} must be a finite number >= 0")
        if lr is None and wd is None and fr is None:
            raise ValueError(f"param_groups[{k}]: the entry sets none of {_SPEC_FIELDS}")
        out.append({"match": m, "lr_scale": None if lr is None else float(lr), "weight_decay": None if wd is None else float(wd),
                    "frozen": None if fr is None else bool(fr)})
    # two explicit name lists that set the same field for the same name: the second could never apply — almost surely a mistake
    for i, a in enumerate(out):
        for j in range(i + 1, len(out)):
            b = out[j]
            if isinstance(a["match"], list) and isinstance(b["match"], list):
                both = sorted(set(a["match"]) & set(b["match"]))
                same = [f for f in _SPEC_FIELDS if a[f] is not None and b[f] is not None]
                if both and same:
                    raise ValueError(f"param_groups[{i}] and [{j}] both list {both[:3]} and both set {same}")
    return out


def resolve_spec(names, spec, default_wd):
    """{name: (lr_scale, weight_decay, frozen)} for the given (first) parameter names; raises for an entry that matches none."""
    import re
    spec = normalize_spec(spec) or []
    names = list(names)
    known = set(names)
    hits = []
    for k, e in enumerate(spec):
        if isinstance(e["match"], list):
            unknown = [x for x in e["match"] if x not in known]
            if unknown:
                raise ValueError(f"param_groups[{k}]: {unknown[:3]} name no parameter of this optimizer (a tied parameter is known by "
                                 "its first name in named_parameters() only)")
            hit = set(e["match"])
        else:
            rx = re.compile(e["match"])
            hit = {x for x in names if rx.search(x)}
            if not hit:
                raise ValueError(f"param_groups[{k}]: {e['match']!r} matches no parameter of this optimizer")
        hits.append(hit)
    out = {}
    for x in names:
        val = {"lr_scale": 1.0, "weight_decay": float(default_wd), "frozen": False}
        for f in _SPEC_FIELDS:
            for e, hit in zip(spec, hits):
                if e[f] is not None and x in hit:
                    val[f] = e[f]
                    break
        out[x] = (val["lr_scale"], val["weight_decay"], val["frozen"])
    return out


class GroupTable:
    """the three tensors the grouped AdamW / clip-norm kernels read (include/vacnic_hip.h), on the host until .to(device)."""

    def __init__(self, seg_start, seg, first_seg):
        self.seg_start, self.seg, self.first_seg = seg_start, seg, first_seg
        self.nseg = seg.shape[0]

    def to(self, device):
        return GroupTable(self.seg_start.to(device), self.seg.to(device), self.first_seg.to(device))

    def segments(self):
        """[(start, end, lr_scale, weight_decay, frozen)]"""
        s, v = self.seg_start.tolist(), self.seg.cpu()
        fr = v.view(torch.int32)[:, 2].tolist()
        return [(s[i], s[i + 1], float(v[i, 0]), float(v[i, 1]), bool(fr[i])) for i in range(self.nseg)]


def table_from_segments(n, segments):
    """GroupTable over [0, n) from [(start, lr_scale, weight_decay, frozen)]: adjacent segments with equal values are merged, and
    the starts must ascend strictly from 0 and stay below n (so the segments tile [0, n) without overlap)."""
    if not segments or segments[0][0] != 0:
        raise ValueError("group table: the first segment must start at element 0")
    merged, prev = [], -1
    for start, lr, wd, fr in segments:
        if start <= prev:
            raise ValueError(f"group table: segment starts must ascend strictly ({prev} then {start})")
        prev = start
        if not 0 <= start < n:
            raise ValueError(f"group table: segment start {start} outside [0, {n})")
        val = (float(lr), float(wd), bool(fr))
        if merged and merged[-1][1] == val:
            continue
        merged.append((int(start), val))
    seg_start = torch.tensor([s for s, _ in merged] + [int(n)], dtype=torch.int64)
    seg = torch.zeros(len(merged), 4, dtype=torch.float32)
    seg[:, 0] = torch.tensor([v[0] for _, v in merged], dtype=torch.float32)
    seg[:, 1] = torch.tensor([v[1] for _, v in merged], dtype=torch.float32)
    seg.view(torch.int32)[:, 2] = torch.tensor([int(v[2]) for _, v in merged], dtype=torch.int32)
    assert bool((seg_start[1:] > seg_start[:-1]).all()) and int(seg_start[0]) == 0 and int(seg_start[-1]) == n
    blocks = torch.arange(0, (n + BLOCK - 1) // BLOCK, dtype=torch.int64) * BLOCK
    first_seg = (torch.searchsorted(seg_start, blocks, right=True) - 1).to(torch.int32)       # the segment holding element 1024 b
    return GroupTable(seg_start, seg, first_seg)


def first_names(arena, named_params):
    """[(first name, parameter)] of the arena's parameters in named_params order; parameters of other arenas are skipped."""
    out, seen = [], set()
    for name, p in named_params:
        if id(p) in arena.slots and id(p) not in seen:
            seen.add(id(p))
            out.append((name, p))
    missing = [i for i in arena.slots if i not in seen]
    if missing:
        raise ValueError(f"group table: {len(missing)} parameter(s) of the arena are not in named_params")
    return out


def name_at(arena, named_params, offset):
    """first name (first_names: a tied or shared parameter is known by the first of its names) of the parameter whose elements hold
    arena offset `offset`; None for alignment gaps, pad_rows padding and the arena's tail.  Pure host logic."""
    for name, p in first_names(arena, named_params):
        o, n, _ = arena.slots[id(p)]
        if o <= offset < o + n:
            return name
    return None


def group_table(arena, named_params, spec, default_wd):
    """Lay a spec over the arena's slots.  Alignment gaps, the pad_rows padding of a slot and the tail up to arena.n belong to the
    preceding parameter's segment (they hold p = g = m = v = 0 and stay 0 under any group: 0 * decay - lr * 0 / (0 + eps) = 0).
    Pure host logic: works on a "cpu" arena; the optimizer uploads the result once."""
    named = first_names(arena, named_params)
    vals = resolve_spec([nm for nm, _ in named], spec, default_wd)
    slots = sorted((arena.slots[id(p)][0], vals[nm]) for nm, p in named)
    if slots[0][0] != 0:
        raise ValueError("group table: the arena's first slot does not start at element 0")
    return table_from_segments(arena.n, [(o, *v) for o, v in slots])


# ---- per-parameter statistics ----------------------------------------------------------------------------------------------
STATS_UNIT = 4096   # elements per unit of the statistics kernel's first pass (include/vacnic_hip.h, vacnic_param_stats)


class StatsTable:
    """the tensors vacnic_param_stats reads (include/vacnic_hip.h), on the host until .to(device), and the slots they were cut
    from: slots[s] = (offset, numel) in rising offset order; slot s owns units [slot_unit[s], slot_unit[s + 1])."""

    def __init__(self, slots, unit_off, unit_len, slot_unit):
        self.slots = slots
        self.unit_off, self.unit_len, self.slot_unit = unit_off, unit_len, slot_unit
        self.nslot, self.nunit = len(slots), unit_off.numel()

    def to(self, device):
        return StatsTable(self.slots, self.unit_off.to(device), self.unit_len.to(device), self.slot_unit.to(device))


def stats_table_from_slots(slots, unit=STATS_UNIT):
    """StatsTable from [(offset, numel)]: sorted by offset, which must leave the slots disjoint; every slot is cut into units of at
    most `unit` (<= 4096) elements, none of which crosses a slot.  Gaps between slots lie in no unit."""
    if not 1 <= int(unit) <= STATS_UNIT:
        raise ValueError(f"stats table: unit={unit!r} must lie in [1, {STATS_UNIT}]")
    slots = sorted((int(o), int(n)) for o, n in slots)
    if not slots:
        raise ValueError("stats table: no slots")
    end = 0
    unit_off, unit_len, slot_unit = [], [], [0]
    for o, n in slots:
        if o < end or n < 0:
            raise ValueError(f"stats table: slot ({o}, {n}) overlaps its predecessor, which ends at {end}")
        end = o + n
        for u in range(o, end, unit):
            unit_off.append(u)
            unit_len.append(min(unit, end - u))
        slot_unit.append(len(unit_off))
    if not unit_off:
        raise ValueError("stats table: every slot is empty")
    return StatsTable(slots, torch.tensor(unit_off, dtype=torch.int64), torch.tensor(unit_len, dtype=torch.int32),
                      torch.tensor(slot_unit, dtype=torch.int64))


def stats_table(arena, unit=STATS_UNIT):
    """The statistics kernel's view of the arena: one slot (offset, numel) per parameter — a parameter reachable under several names
    has one —, without alignment gaps, pad_rows padding or the tail.  Names are not part of it: first_names() gives them when a
    report is read.  Pure host logic: works on a "cpu" arena; the optimizer uploads the result once."""
    return stats_table_from_slots([(o, n) for o, n, _ in arena.slots.values()], unit)


def no_decay_spec(model):
    """[{"match": [names], "weight_decay": 0.0}] for every `.bias` and every parameter of an nn.LayerNorm — chosen by module type
    and attribute, not by name pattern (BART's LayerNorms are `*_layer_norm` and `layernorm_embedding*`).  The frozen CLIP tower
    (`clip_model.*`) has its own arena and is left out."""
    first = {}
    for name, p in model.named_parameters():
        first.setdefault(id(p), name)
    names = []
    for mod in model.modules():
        for attr, p in mod._parameters.items():
            if p is None or not (attr == "bias" or isinstance(mod, torch.nn.LayerNorm)):
                continue
            nm = first[id(p)]
            if not nm.startswith("clip_model.") and nm not in names:
                names.append(nm)
    if not names:
        raise ValueError("no_decay_spec: the model has neither biases nor LayerNorms")
    return [{"match": names, "weight_decay": 0.0}]
