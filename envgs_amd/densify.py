"""Densify / prune support on the per-Gaussian SoA (include/envgs_densify.h).

`prune_rows` = every `tensor[mask]` of the reference's pruning (`_prune_optimizer` / `prune_stats`,
easyvolcap/utils/gaussian2d_utils.py:536-560,640-648) in one scan + one gather launch; `prune_optimizer` / `cat_tensors_to_optimizer`
keep the reference's contract (one parameter per group, fresh `nn.Parameter`, Adam moments carried over / zero-extended);
`knn3_mean_dist2` = `simple_knn.distCUDA2` (gaussian2d_utils.py:432-440).
"""
import torch
from torch import nn

from . import _lib


def _stream(dev):
    return _lib.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def prune_rows(tensors, keep, n_kept=None):
    """[t[keep] for t in tensors] for tensors sharing their first dimension; keep: (P,) bool (or uint8, non-zero = keep).  One host sync (the
    kept count) -- none when the caller knows the count and passes it as `n_kept`."""
    lib = _lib.load()
    if keep.device.type != "cuda":
        raise RuntimeError("prune_rows needs GPU tensors; there is no CPU path")
    dev = keep.device
    P = keep.shape[0]
    keep8 = keep.to(torch.uint8).contiguous()
    pos = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
    nk = torch.empty(1, dtype=torch.int32, device=dev)
    tb = lib.envgs_compact_temp_bytes(P)
    temp = torch.empty(max(tb, 1), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    _lib.check(lib.envgs_compact_scan(P, p(keep8), p(pos), p(nk), p(temp), tb, _stream(dev)), "envgs_compact_scan")
    n = int(nk.item()) & 0xFFFFFFFF if n_kept is None else int(n_kept)
    outs, srcs = [], []
    for t in tensors:
        if t.shape[0] != P or t.device != dev:
            raise RuntimeError("prune_rows: every tensor must have %d rows on %s" % (P, dev))
        if t.element_size() * (t[0].numel() if P else 1) % 4:
            raise RuntimeError("prune_rows: rows must be a multiple of 4 bytes")
        srcs.append(t.detach().contiguous())
        outs.append(torch.empty((n,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev))
    if n == 0:
        return outs
    for i in range(0, len(srcs), 32):
        chunk = list(zip(srcs[i:i + 32], outs[i:i + 32]))
        arr = (_lib.RowsTensor * len(chunk))()
        for j, (s, o) in enumerate(chunk):
            arr[j] = _lib.RowsTensor(s.data_ptr(), o.data_ptr(), s.element_size() * (s[0].numel() if P else 0))
        if n_kept is None:
            _lib.check(lib.envgs_compact_gather(len(chunk), arr, P, p(keep8), p(pos), _stream(dev)), "envgs_compact_gather")
        else:                                                         # the caller's count sized the outputs: no row beyond it is written
            _lib.check(lib.envgs_compact_gather_rows(len(chunk), arr, P, n, p(keep8), p(pos), _stream(dev)), "envgs_compact_gather_rows")
    return outs


def prune_optimizer(optimizer, keep):
    """`_prune_optimizer` of the reference for an optimizer whose groups hold ONE per-Gaussian parameter each: every parameter and its
    Adam moments are compacted together; returns {group name: new nn.Parameter} (state moved to the new parameter)."""
    items = []
    for group in optimizer.param_groups:
        assert len(group["params"]) == 1
        prm = group["params"][0]
        st = optimizer.state.get(prm, None)
        items.append((group, prm, st))
    flat = []
    for group, prm, st in items:
        flat.append(prm.data)
        if st is not None and "exp_avg" in st:
            flat += [st["exp_avg"], st["exp_avg_sq"]]
    outs = iter(prune_rows(flat, keep))
    result = {}
    for group, prm, st in items:
        new = nn.Parameter(next(outs).requires_grad_(True))
        if st is not None:
            if "exp_avg" in st:
                st["exp_avg"] = next(outs); st["exp_avg_sq"] = next(outs)
            del optimizer.state[prm]
            optimizer.state[new] = st
        group["params"][0] = new
        result[group.get("name", str(len(result)))] = new
    return result


def cat_tensors_to_optimizer(tensors_dict, optimizer):
    """`cat_tensors_to_optimizer` of the reference (gaussian2d_utils.py:562-588): append rows to each named group, zero moments."""
    result = {}
    for group in optimizer.param_groups:
        assert len(group["params"]) == 1
        ext = tensors_dict.get(group.get("name"))
        if ext is None:
            continue
        prm = group["params"][0]
        st = optimizer.state.get(prm, None)
        new = nn.Parameter(torch.cat((prm.data, ext), dim=0).requires_grad_(True))
        if st is not None:
            if "exp_avg" in st:
                st["exp_avg"] = torch.cat((st["exp_avg"], torch.zeros_like(ext)), dim=0)
                st["exp_avg_sq"] = torch.cat((st["exp_avg_sq"], torch.zeros_like(ext)), dim=0)
            del optimizer.state[prm]
            optimizer.state[new] = st
        group["params"][0] = new
        result[group["name"]] = new
    return result


def knn3_mean_dist2(xyz):
    """simple_knn.distCUDA2: mean squared distance to the 3 nearest neighbours, (P,) float32."""
    lib = _lib.load()
    if xyz.device.type != "cuda":
        raise RuntimeError("knn3_mean_dist2 needs a GPU tensor; there is no CPU path")
    x = xyz.detach().to(torch.float32).contiguous()
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    _lib.check(lib.envgs_knn3_mean_dist2(x.shape[0], _lib.ptr(x), _lib.ptr(out), _stream(x.device)), "envgs_knn3_mean_dist2")
    return out


def torch_rows(tensors, keep, n_kept=None):
    """`prune_rows` written with torch indexing.  NOT a product path: tests pass it as `row_ops` to exercise `SurfelSet`'s host logic on CPU."""
    return [t.detach()[keep] for t in tensors]


def weight_order_statistics(weight_accum, denom, ranks):
    """Exact order statistics of the average weight `weight_accum / denom` (NaN -> 0, -0 counted as +0; `get_xyz_weight_avg`,
    gaussian2d_utils.py:628-631) for one or two 0-based ranks: (values (len(ranks),) float32, below (len(ranks),) int32 = the number of keys
    strictly below each value), both on the device.  Three-pass radix select, no sort and no host synchronisation."""
    lib = _lib.load()
    if weight_accum.device.type != "cuda":
        raise RuntimeError("weight_order_statistics needs GPU tensors; there is no CPU path")
    dev, P = weight_accum.device, weight_accum.numel()
    ranks = [int(r) for r in ranks]
    if denom.numel() != P or denom.device != dev or len(ranks) not in (1, 2) or any(r < 0 or r >= P for r in ranks):
        raise RuntimeError("weight_order_statistics: two tensors of the same size on one GPU and one or two ranks in [0, %d)" % P)
    wa, dn = (t.detach().to(torch.float32).contiguous() for t in (weight_accum, denom))
    values = torch.empty(len(ranks), dtype=torch.float32, device=dev)
    below = torch.empty(len(ranks), dtype=torch.int32, device=dev)
    tb = lib.envgs_weight_select_temp_bytes()
    temp = torch.empty(tb, dtype=torch.uint8, device=dev)
    p = _lib.ptr
    _lib.check(lib.envgs_weight_select(P, p(wa), p(dn), len(ranks), ranks[0], ranks[-1], p(values), p(below), p(temp), tb, _stream(dev)),
               "envgs_weight_select")
    return values, below


def normal_offsets(stds, generator=None):
    """The values (and the generator advance) of `torch.normal(torch.zeros_like(stds), stds, generator=generator)`, the staged split's call, without
    that call's host check of `stds >= 0` -- a `.item()`, i.e. a second queue drain in a pass whose point is to have one.  torch evaluates the
    tensor-std form as a standard normal fill of the output followed by `mul_(std).add_(mean)`; these are the same three steps (the added zero
    turns a -0 offset into the +0 the staged call returns).  `stds` here are exp() of the raw scales, never negative.
    tests/test_densify_device.py holds the two forms to bit equality on the GPU."""
    return torch.empty_like(stds).normal_(0.0, 1.0, generator=generator).mul_(stds).add_(0.0)


class SurfelSet:
    """One Gaussian set's raw parameters, their optimizer groups and the densification statistics, with the densify / prune schedule of the
    reference's `GaussianModel` (easyvolcap/utils/gaussian2d_utils.py:622-909) rebuilt over the compaction kernels:

      * every removal is ONE `prune_rows` call over parameters + both Adam moments + the four statistics (the reference: `_prune_optimizer`
        :536-560 + `prune_stats` :640-648, 28 boolean-mask gathers);
      * every clone / split gathers all selected rows of all parameters in one call and appends them with one `torch.cat` per tensor;
      * selection masks are the reference's expressions (cited per method); random split offsets use the same `torch.normal(means, stds)` call.

    raw: {"_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity"[, "_specular", "_roughness"]} (ckpt.PT_PARAMS).
    optimizer: groups named `prefix + name`, one parameter each (the reference's layout, gaussian2d_utils.py:562-588); may be None.
    row_ops: the row gather; defaults to the HIP `prune_rows` (GPU tensors only).
    device_schedule: OPT-IN device-resident mode (GPU tensors only, no CPU path): `add_densification_stats` becomes one launch without a host
        round trip, and `densify_and_prune` runs its first three stages as `grow_and_prune` -- one plan, one read-back, one rewrite.  Survivors,
        clones, moments, statistics and `log` equal the staged path bit for bit; the split children's `_xyz` / `_scaling` are the same formulas
        evaluated in a HIP kernel, so they agree with the staged torch expressions to rounding, not to the bit: hence opt-in.  With True the
        tail (`prune_max_scene_and_screen`, `prune_visibility`: global order statistics) stays staged torch.
        device_schedule="all": the tail runs on the device as well.  The order statistics of the average weight come from a three-pass radix
        select (`weight_order_statistics`) instead of `torch.quantile`'s sort / `torch.topk`; `prune_visibility` builds its mask and compacts
        without any host synchronisation (the kept count is host arithmetic); `prune_max_scene_and_screen` builds both masks in one launch,
        reads its two counts back (its only synchronisation), compacts with the split flags riding along and splits with the staged torch
        expressions, so its result equals the staged path bit for bit.  One DEFINED difference, hence a value of its own: when several surfels
        have exactly the cut-off weight of `prune_visibility`, the tied surfels of LOWEST INDEX are pruned (`torch.topk` leaves the choice
        unspecified); exactly as many rows go as in the staged path.

    The schedule edits between densifications -- `reset_opacity`, `reset_specular`, `enlarge_opacity`, `enlarge_scaling`, `distort_color`
    (normal propagation and colour sabotage, gaussian2d_utils.py:482-515) and `set_learning_rate` (:916-919) -- are elementwise torch in every
    mode, on CPU or GPU tensors, without a host synchronisation."""

    STATS = ("xyz_gradient_accum", "denom", "max_radii2D", "xyz_weight_accum")

    def __init__(self, raw, optimizer=None, prefix="", spatial_scale=1.0, max_gs=None, max_gs_threshold=1.0, row_ops=None, generator=None,
                 device_schedule=False):
        self.names = [k for k in ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity", "_specular", "_roughness") if k in raw]
        self.optimizer, self.prefix, self.spatial_scale = optimizer, prefix, float(spatial_scale)
        self.max_gs, self.max_gs_threshold = max_gs, max_gs_threshold
        self.rows = row_ops or prune_rows
        if isinstance(device_schedule, str) and device_schedule != "all":
            raise ValueError("device_schedule is False, True or \"all\", not %r" % (device_schedule,))
        self.device_schedule = bool(device_schedule)
        self.device_tail = isinstance(device_schedule, str)          # "all": the pruning tail on the device as well
        # split offsets are random: with data parallelism every rank must draw the SAME ones, i.e. pass generators seeded
        # identically on all ranks (or seed the global generator identically before every densification)
        self.generator = generator
        self.p = {}
        groups = {g.get("name"): g for g in optimizer.param_groups} if optimizer is not None else {}
        for k in self.names:
            g = groups.get(prefix + k)
            self.p[k] = g["params"][0] if g is not None else nn.Parameter(raw[k].detach().clone().requires_grad_(True))
        if self.device_schedule and self.device.type != "cuda":
            raise RuntimeError("SurfelSet(device_schedule=%r) needs GPU tensors; there is no CPU path" % (device_schedule,))
        self.reset_stats()
        self.log = []                                # (event, count) pairs, the numbers the reference prints

    # ---- views -------------------------------------------------------------------------------------------------------------------------------
    @property
    def number(self):
        return self.p["_xyz"].shape[0]

    @property
    def device(self):
        return self.p["_xyz"].device

    def scaling(self):
        return torch.exp(self.p["_scaling"].detach())

    def opacity(self):
        return torch.sigmoid(self.p["_opacity"].detach())

    def raw(self):
        return {k: v.detach() for k, v in self.p.items()}

    # ---- statistics (gaussian2d_utils.py:622-637, 901-909) --------------------------------------------------------------------------------------
    def reset_stats(self):
        P, dev = self.number, self.device
        self.stats = {"xyz_gradient_accum": torch.zeros(P, 1, device=dev), "denom": torch.zeros(P, 1, device=dev),
                      "max_radii2D": torch.zeros(P, device=dev), "xyz_weight_accum": torch.zeros(P, 1, device=dev)}

    def add_densification_stats(self, viewspace_grad, update_filter, weight_accumulate=None, radii=None):
        """viewspace_grad: the `.grad` of the rasterizer's means2D (P,3); update_filter: (P,) bool; radii (optional): the max-radius update the
        sampler does next to it (gaussian2d_sampler.py:330-332)."""
        if self.device_schedule:
            return self._device_stats(viewspace_grad, update_filter, weight_accumulate, radii)
        s = self.stats
        s["denom"][update_filter] += 1
        s["xyz_gradient_accum"][update_filter] += torch.norm(viewspace_grad[update_filter], dim=-1, keepdim=True)
        if weight_accumulate is not None:
            s["xyz_weight_accum"][update_filter] += weight_accumulate[update_filter]
        if radii is not None:
            s["max_radii2D"][update_filter] = torch.max(s["max_radii2D"][update_filter], radii[update_filter].to(s["max_radii2D"].dtype))

    def _device_stats(self, viewspace_grad, update_filter, weight_accumulate, radii):
        """The same update as one launch of envgs_densify_stats: no boolean-mask indexing, hence no nonzero and no host read-back."""
        lib = _lib.load()
        s, P, dev = self.stats, self.number, self.device
        grad = viewspace_grad.detach()
        if grad.dim() != 2 or grad.shape[0] != P or grad.shape[1] not in (2, 3) or update_filter.shape != (P,):
            raise RuntimeError("add_densification_stats: viewspace_grad must be (%d, 2 or 3) and update_filter (%d,)" % (P, P))
        for t in (grad, update_filter, weight_accumulate, radii):
            if t is not None and t.device != dev:
                raise RuntimeError("add_densification_stats: device_schedule needs every tensor on %s; there is no CPU path" % dev)
        if grad.dtype != torch.float32 or not grad.is_contiguous():
            grad = grad.to(torch.float32).contiguous()
        flt = update_filter.contiguous()
        flt = flt.view(torch.uint8) if flt.dtype == torch.bool else (flt != 0).view(torch.uint8)
        w = weight_accumulate
        if w is not None:
            if w.numel() != P:
                raise RuntimeError("add_densification_stats: weight_accumulate must have %d elements" % P)
            w = w.detach()
            if w.dtype != torch.float32 or not w.is_contiguous():
                w = w.to(torch.float32).contiguous()
        r = radii
        if r is not None:
            if r.numel() != P:
                raise RuntimeError("add_densification_stats: radii must have %d elements" % P)
            if r.dtype != torch.int32 or not r.is_contiguous():
                r = r.to(torch.int32).contiguous()                   # (the rasterizer's radii are int32 already)
        p = _lib.ptr
        _lib.check(lib.envgs_densify_stats(P, grad.shape[1], p(grad), p(flt), p(w), p(r), p(s["xyz_gradient_accum"]), p(s["denom"]),
                                           p(s["max_radii2D"]), p(s["xyz_weight_accum"]), _stream(dev)), "envgs_densify_stats")

    def _avg(self, key):
        avg = self.stats[key] / self.stats["denom"]
        avg[avg.isnan()] = 0.0
        return avg

    def gradient_avg(self):
        return self._avg("xyz_gradient_accum")

    def weight_avg(self):
        return self._avg("xyz_weight_accum")

    # ---- row surgery ---------------------------------------------------------------------------------------------------------------------------
    def _groups(self):
        """[(name, group or None, parameter, adam state or None)] in parameter order."""
        out = []
        gs = {g.get("name"): g for g in self.optimizer.param_groups} if self.optimizer is not None else {}
        for k in self.names:
            g = gs.get(self.prefix + k)
            prm = self.p[k]
            st = self.optimizer.state.get(prm, None) if g is not None else None
            out.append((k, g, prm, st if st else None))
        return out

    def _install(self, k, g, old, st, new_data, m=None, v=None):
        new = nn.Parameter(new_data.requires_grad_(True))
        if g is not None:
            if st is not None:
                if m is not None:
                    st["exp_avg"], st["exp_avg_sq"] = m, v
                del self.optimizer.state[old]
                self.optimizer.state[new] = st
            g["params"][0] = new
        self.p[k] = new

    def remove(self, mask):
        """prune_points + prune_stats (:553-560, :640-648): drop the rows where `mask` is set -- parameters, Adam moments and statistics, one gather."""
        self._compact(~mask)

    def _compact(self, keep, n_kept=None, extra=()):
        """Keep the rows where `keep` is set.  n_kept: the kept count when the caller knows it (no read-back then); extra: further tensors of
        P rows that go through the same gather -- their kept rows are returned."""
        items = self._groups()
        flat = []
        for k, g, prm, st in items:
            flat.append(prm.data)
            if st is not None and "exp_avg" in st:
                flat += [st["exp_avg"], st["exp_avg_sq"]]
        flat += [self.stats[s] for s in self.STATS] + list(extra)
        outs = iter(self.rows(flat, keep) if n_kept is None else self.rows(flat, keep, n_kept=n_kept))
        for k, g, prm, st in items:
            data = next(outs)
            if st is not None and "exp_avg" in st:
                self._install(k, g, prm, st, data, next(outs), next(outs))
            else:
                self._install(k, g, prm, st, data)
        for s in self.STATS:
            self.stats[s] = next(outs)
        self._scene_changed()
        return list(outs)

    @staticmethod
    def _scene_changed():
        """Rows were removed / appended or the opacities reset: a tracer's stored topology no longer describes this set even when the count
        happens to be what it was -- its next request is a full build, not a refit (tracing.invalidate_all_structures)."""
        from . import tracing
        tracing.invalidate_all_structures()

    def _append(self, new, selected_stats, split, ratio):
        """densification_postfix + densify_stats (:590-621, :650-663): new rows get zero moments; their statistics are the parents' (gradient and
        radius scaled by `ratio`, weight multiplied by the current maximum -- the reference's expression, kept as is)."""
        for k, g, prm, st in self._groups():
            ext = new[k]
            if st is not None and "exp_avg" in st:
                m = torch.cat((st["exp_avg"], torch.zeros_like(ext)), dim=0)
                v = torch.cat((st["exp_avg_sq"], torch.zeros_like(ext)), dim=0)
                self._install(k, g, prm, st, torch.cat((prm.data, ext), dim=0), m, v)
            else:
                self._install(k, g, prm, st, torch.cat((prm.data, ext), dim=0))
        ga, dn, mr, wa = selected_stats
        s = self.stats
        wmax = s["xyz_weight_accum"].max()
        s["xyz_gradient_accum"] = torch.cat([s["xyz_gradient_accum"], ga.repeat(split, 1) * ratio], dim=0)
        s["denom"] = torch.cat([s["denom"], dn.repeat(split, 1)], dim=0)
        s["max_radii2D"] = torch.cat([s["max_radii2D"], mr.repeat(split) * ratio], dim=0)
        s["xyz_weight_accum"] = torch.cat([s["xyz_weight_accum"], wa.repeat(split, 1) * wmax], dim=0)
        self._scene_changed()

    def _selected(self, mask, n_selected=None):
        flat = [self.p[k].data for k in self.names] + [self.stats[s] for s in self.STATS]
        outs = self.rows(flat, mask) if n_selected is None else self.rows(flat, mask, n_kept=n_selected)
        return dict(zip(self.names, outs[:len(self.names)])), outs[len(self.names):]

    def clone(self, mask):
        """:665-677."""
        sel, st = self._selected(mask)
        self._append(sel, st, 1, 1.0)

    def split(self, mask, N=2, ratio=0.8, n_selected=None):
        """:679-706: N children per selected surfel, offsets ~ N(0, diag(sx, sy, 0)) in the surfel's frame, scales / (ratio N); parents removed.
        n_selected: the number of set rows of `mask` when the caller knows it -- the two read-backs of that count are skipped."""
        from .synth import build_rotation
        sel, st = self._selected(mask, n_selected)
        scal = torch.exp(sel["_scaling"])
        stds = scal.repeat(N, 1)
        stds = torch.cat([stds, torch.zeros_like(stds[:, :1])], dim=-1)
        if self.device_tail:
            samples = normal_offsets(stds, self.generator)               # the same draw without torch.normal's host check, a sync
        else:
            samples = torch.normal(torch.zeros_like(stds), stds, generator=self.generator)
        rots = build_rotation(sel["_rotation"]).repeat(N, 1, 1)
        new = {k: v.repeat(*([N] + [1] * (v.dim() - 1))) for k, v in sel.items()}
        new["_xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + sel["_xyz"].repeat(N, 1)
        new["_scaling"] = torch.log(scal.repeat(N, 1) / (ratio * N))
        self._append(new, st, N, 1.0 / (ratio * N))
        n_split = int(mask.sum().item()) if n_selected is None else int(n_selected)
        keep = ~torch.cat((mask, torch.zeros(n_split * N, device=mask.device, dtype=torch.bool)))
        self._compact(keep, None if n_selected is None else mask.shape[0] + n_split * (N - 1))

    def replace(self, name, tensor):
        """replace_tensor_to_optimizer (:517-534): new values, zeroed moments."""
        for k, g, prm, st in self._groups():
            if k == name:
                if st is not None and "exp_avg" in st:
                    self._install(k, g, prm, st, tensor.detach().clone(), torch.zeros_like(tensor), torch.zeros_like(tensor))
                else:
                    self._install(k, g, prm, st, tensor.detach().clone())

    def reset_opacity(self, value=0.01):
        """:512-515."""
        o = self.p["_opacity"].detach()
        self.replace("_opacity", torch.min(o, torch.logit(torch.ones_like(o) * value)))
        self._scene_changed()           # (leaf boxes are bounded by the alpha >= 1/255 disc: every box shrinks at once)

    def reset_specular(self, value=0.001, reset_all=False):
        """:505-510."""
        s = self.p["_specular"].detach()
        cap = torch.logit(torch.ones_like(s) * value)
        self.replace("_specular", cap if reset_all else torch.min(s, cap))

    def enlarge_opacity(self, value=0.9):
        """:499-503 (normal propagation): no opacity below `value`."""
        o = self.p["_opacity"].detach()
        self.replace("_opacity", torch.max(o, torch.logit(torch.ones_like(o) * value)))
        self._scene_changed()           # (every box bounded by a raised opacity grows)

    def _specular_peak(self):
        return torch.sigmoid(self.p["_specular"].detach()).max(dim=-1).values.flatten()

    def enlarge_scaling(self, ratio=1.5, threshold=0.02):
        """:491-497 (normal propagation): the surfels whose specular reaches `threshold` grow by `ratio`; the others keep their raw scale."""
        s = self.p["_scaling"].detach()
        dull = (self._specular_peak() < threshold).unsqueeze(-1)
        self.replace("_scaling", torch.where(dull, s, torch.log(torch.exp(s) * ratio)))
        self._scene_changed()

    def distort_color(self, range=0.4, threshold=0.05):
        """:482-489 (colour sabotage): uniform noise of +-`range` on the base colour of every surfel whose specular does not exceed `threshold`.
        The draw is `torch.rand_like` of the whole tensor, from the set's generator (the global one without)."""
        f = self.p["_features_dc"].detach()
        shiny = (self._specular_peak() > threshold).reshape([-1] + [1] * (f.dim() - 1))
        u = torch.empty_like(f).uniform_(0.0, 1.0, generator=self.generator)
        self.replace("_features_dc", torch.where(shiny, f, f + u * range * 2 - range))

    def set_learning_rate(self, name, lr):
        """update_learning_rate_by_name (:916-919): the group `prefix + name` trains at `lr` from now on; an unknown name changes nothing."""
        if self.optimizer is not None:
            for g in self.optimizer.param_groups:
                if g.get("name") == self.prefix + name:
                    g["lr"] = lr

    # ---- the schedule (gaussian2d_utils.py:718-899) ------------------------------------------------------------------------------------------------
    def densify_and_clone(self, grad_threshold, size_threshold):
        high = (self.gradient_avg() >= grad_threshold).squeeze(-1)
        mask = (torch.max(self.scaling(), dim=1).values <= size_threshold * self.spatial_scale) & high
        n = int(mask.sum().item())
        self.log.append(("clone", n))
        if n > 0:
            self.clone(mask)

    def densify_and_split(self, grad_threshold, size_threshold, split_screen_threshold=None, N=2):
        high = (self.gradient_avg() >= grad_threshold).squeeze(-1)
        mask = torch.max(self.scaling(), dim=1).values > size_threshold * self.spatial_scale
        if split_screen_threshold is not None:
            mask = mask | (self.stats["max_radii2D"] > split_screen_threshold)
        mask = mask & high
        n = int(mask.sum().item())
        self.log.append(("split", n))
        if n > 0:
            self.split(mask, N)

    def prune_min_opacity_and_gradients(self, min_opacity=None, min_gradient=None):
        P, dev = self.number, self.device
        occ = (self.opacity() < min_opacity).squeeze(-1) if min_opacity is not None else torch.zeros(P, dtype=torch.bool, device=dev)
        if min_gradient is not None:
            grd = ((self.gradient_avg() <= min_gradient) & (self.stats["denom"] != 0)).squeeze(-1)
        else:
            grd = torch.zeros(P, dtype=torch.bool, device=dev)
        mask = occ | grd
        n = int(mask.sum().item())
        self.log.append(("prune_occ_grad", n))
        if n > 0:
            self.remove(mask)

    _GROW_KINDS = {"_xyz": 2, "_scaling": 3}                  # ENVGS_GROW_XYZ / _SCALING; every other parameter is ENVGS_GROW_COPY
    _GROW_STATS = {"xyz_gradient_accum": 4, "denom": 5, "max_radii2D": 6, "xyz_weight_accum": 7}

    def grow_and_prune(self, min_opacity, min_gradient, grad_threshold, size_threshold, split_screen_threshold=None, N=2, ratio=0.8):
        """densify_and_clone -> densify_and_split -> prune_min_opacity_and_gradients as ONE pass (device_schedule only).  A clone child inherits
        the scale, opacity and statistics its parent is judged by, so what the later stages decide for it is known from the parent, and the
        three stages' result is a closed-form function of the set before the pass: one plan launch + scan decides and places every row, ONE
        read-back brings the counts (the pass's only host sync), the split offsets are the staged path's own `torch.normal` draw (`normal_offsets`),
        and one launch writes every parameter, both Adam moments and the four statistics at their final size.  Rows, moments, statistics and
        `log` equal the staged result; the split children's `_xyz` / `_scaling` agree with it to rounding (see the class docstring)."""
        if not self.device_schedule:
            raise RuntimeError("grow_and_prune is the device-resident pass: build the SurfelSet with device_schedule=True")
        lib = _lib.load()
        P, dev, p = self.number, self.device, _lib.ptr
        N = int(N)
        if P == 0:
            self.log += [("clone", 0), ("split", 0), ("prune_occ_grad", 0)]
            return
        scal = self.scaling().to(torch.float32).contiguous()
        opac = self.opacity().to(torch.float32).contiguous() if min_opacity is not None else None
        st = {k: self.stats[k].contiguous() for k in self.STATS}
        cls = torch.empty(P, dtype=torch.uint8, device=dev)
        scan = torch.empty(6 * P, dtype=torch.int32, device=dev)
        counters = torch.empty(16, dtype=torch.int32, device=dev)
        tb = lib.envgs_densify_plan_temp_bytes(P)
        temp = torch.empty(max(tb, 1), dtype=torch.uint8, device=dev)
        r = 1.0 / (ratio * N)
        flags = (1 if min_opacity is not None else 0) | (2 if min_gradient is not None else 0) | (4 if split_screen_threshold is not None else 0)
        plan = _lib.DensifyPlanArgs(P, N, flags, grad_threshold, size_threshold * self.spatial_scale, split_screen_threshold or 0.0, min_opacity or 0.0,
                                    min_gradient or 0.0, r, st["xyz_gradient_accum"].data_ptr(), st["denom"].data_ptr(), st["max_radii2D"].data_ptr(),
                                    st["xyz_weight_accum"].data_ptr(), scal.data_ptr(), opac.data_ptr() if opac is not None else None,
                                    cls.data_ptr(), scan.data_ptr(), counters.data_ptr(), temp.data_ptr(), tb)
        _lib.check(lib.envgs_densify_plan(plan, _stream(dev)), "envgs_densify_plan")
        nA, nB, nD, nE, nS1, nS2, n_clone = [int(v) & 0xFFFFFFFF for v in counters.cpu().tolist()[:7]]          # the one host sync
        nS = nS1 + nS2
        total = nA + nB + N * (nD + nE)
        self.log += [("clone", n_clone), ("split", nS), ("prune_occ_grad", P + n_clone + (N - 1) * nS - total)]
        if n_clone == 0 and nS == 0 and nA == P:
            return                                                   # nothing selected: nothing installed, nothing drawn
        samples = None
        if nS > 0:
            stds = torch.empty(N * nS, 3, dtype=torch.float32, device=dev)
            _lib.check(lib.envgs_densify_split_stds(P, N, p(cls), p(scan), p(counters), p(scal), p(stds), N * nS, _stream(dev)), "envgs_densify_split_stds")
            samples = normal_offsets(stds, self.generator)
        items, desc, keep = self._groups(), [], []

        def add(src, kind):
            src = src.detach().contiguous()
            if src.shape[0] != P or src.dtype != torch.float32:
                raise RuntimeError("grow_and_prune: every tensor must be float32 with %d rows" % P)
            dst = torch.empty((total,) + tuple(src.shape[1:]), dtype=src.dtype, device=dev)
            keep.append(src)
            desc.append(_lib.GrowTensor(src.data_ptr(), dst.data_ptr(), 4 * (src[0].numel()), kind, 0))
            return dst

        new = []
        for k, g, prm, ost in items:
            data = add(prm.data, self._GROW_KINDS.get(k, 0))
            if ost is not None and "exp_avg" in ost:
                new.append((data, add(ost["exp_avg"], 1), add(ost["exp_avg_sq"], 1)))
            else:
                new.append((data, None, None))
        new_stats = {k: add(st[k], self._GROW_STATS[k]) for k in self.STATS}
        rot = self.p["_rotation"].detach().to(torch.float32).contiguous()
        for i in range(0, len(desc), 32):
            chunk = desc[i:i + 32]
            arr = (_lib.GrowTensor * len(chunk))(*chunk)
            args = _lib.DensifyRewriteArgs(P, total, N * nS, N, len(chunk), float(ratio * N), r, 0, cls.data_ptr(), scan.data_ptr(), counters.data_ptr(),
                                           scal.data_ptr(), rot.data_ptr(), samples.data_ptr() if samples is not None else None, arr)
            _lib.check(lib.envgs_densify_rewrite(args, _stream(dev)), "envgs_densify_rewrite")
        for (k, g, prm, ost), (data, m, v) in zip(items, new):
            self._install(k, g, prm, ost, data, m, v)
        self.stats = new_stats
        self._scene_changed()

    def prune_max_scene_and_screen(self, max_scene_threshold=None, max_screen_threshold=None, min_weight_threshold=None):
        if self.device_tail:
            return self._device_prune_max(max_scene_threshold, max_screen_threshold, min_weight_threshold)
        P, dev = self.number, self.device
        none = torch.zeros(P, dtype=torch.bool, device=dev)
        screens = self.stats["max_radii2D"] > max_screen_threshold if max_screen_threshold is not None else none
        scenes = torch.max(self.scaling(), dim=-1).values > self.spatial_scale * max_scene_threshold if max_scene_threshold is not None else none
        if min_weight_threshold is not None:
            w = self.weight_avg()
            light = (w < torch.quantile(w, min_weight_threshold)).squeeze(-1)
        else:
            light = torch.ones(P, dtype=torch.bool, device=dev)
        big = screens | scenes
        prune = big & light
        split = (big & ~light)[~prune]
        n_prune, n_split = int(prune.sum().item()), int(split.sum().item())
        self.log.append(("prune_large", n_prune)); self.log.append(("split_large", n_split))
        if n_prune > 0:
            self.remove(prune)
        if n_split > 0:
            self.split(split, 5, 0.5)

    def _device_prune_max(self, max_scene_threshold, max_screen_threshold, min_weight_threshold):
        """The same stage with the masks from one launch (envgs_oversize_plan) and `torch.quantile`'s value from two selected order statistics:
        ranks floor / ceil of q (P - 1) in float32 and torch's own `lerp` between them, which is what `torch.quantile` does with its sorted
        copy.  One read-back (the two counts); the split flags are compacted with the rows; the split itself is the staged one."""
        lib = _lib.load()
        P, dev, p = self.number, self.device, _lib.ptr
        if P == 0:
            self.log += [("prune_large", 0), ("split_large", 0)]
            return
        st = {k: self.stats[k].contiguous() for k in ("max_radii2D", "xyz_weight_accum", "denom")}
        quant = None
        if min_weight_threshold is not None:
            rank = torch.tensor(min_weight_threshold, dtype=torch.float32) * (P - 1)                 # host tensors: torch.quantile's own arithmetic
            lo = rank.floor()
            values, _ = weight_order_statistics(st["xyz_weight_accum"], st["denom"], (int(lo), int(rank.ceil())))
            quant = torch.lerp(values[0:1], values[1:2], torch.full((1,), float(rank - lo), dtype=torch.float32, device=dev))
        scal = self.scaling().to(torch.float32).contiguous() if max_scene_threshold is not None else None
        keep = torch.empty(P, dtype=torch.uint8, device=dev)
        flags = torch.empty(P, dtype=torch.int32, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        which = (1 if max_screen_threshold is not None else 0) | (2 if max_scene_threshold is not None else 0) | (4 if quant is not None else 0)
        _lib.check(lib.envgs_oversize_plan(P, which, max_screen_threshold or 0.0, self.spatial_scale * (max_scene_threshold or 0.0), p(st["max_radii2D"]),
                                           p(scal), p(st["xyz_weight_accum"]), p(st["denom"]), p(quant), p(keep), p(flags), p(counts), _stream(dev)),
                   "envgs_oversize_plan")
        n_prune, n_split = [int(v) & 0xFFFFFFFF for v in counts.cpu().tolist()]                      # the one host sync
        self.log.append(("prune_large", n_prune)); self.log.append(("split_large", n_split))
        if n_prune > 0:
            flags, = self._compact(keep, P - n_prune, (flags,))
        if n_split > 0:
            self.split(flags != 0, 5, 0.5, n_selected=n_split)

    def _device_prune_visibility(self, n_prune):
        """The n_prune surfels of lowest average weight leave: one order statistic, the mask (ties by index order) and one compaction whose
        kept count is known on the host -- no synchronisation at all."""
        lib = _lib.load()
        P, dev, p = self.number, self.device, _lib.ptr
        if n_prune > P:
            raise RuntimeError("prune_visibility: %d surfels cannot lose %d" % (P, n_prune))
        wa, dn = (self.stats[k].to(torch.float32).contiguous() for k in ("xyz_weight_accum", "denom"))
        cut, below = weight_order_statistics(wa, dn, (n_prune - 1,))
        keep = torch.empty(P, dtype=torch.uint8, device=dev)
        tb = lib.envgs_visibility_mask_temp_bytes(P)
        temp = torch.empty(tb, dtype=torch.uint8, device=dev)
        _lib.check(lib.envgs_visibility_mask(P, p(wa), p(dn), n_prune, p(cut), p(below), p(keep), p(temp), tb, _stream(dev)), "envgs_visibility_mask")
        self._compact(keep, P - n_prune)

    def prune_visibility(self):
        n_prune = self.number - int(self.max_gs * self.max_gs_threshold)
        if n_prune > 0 and self.device_tail:
            self._device_prune_visibility(n_prune)
            self.log.append(("prune_visibility", n_prune))
        elif n_prune > 0:
            _, idx = torch.topk(self.weight_avg()[..., 0], n_prune, largest=False)
            mask = torch.zeros(self.number, dtype=torch.bool, device=self.device)
            mask[idx] = True
            self.remove(mask)
            self.log.append(("prune_visibility", n_prune))

    def densify_and_prune(self, min_opacity, min_gradient, densify_grad_threshold, densify_size_threshold, split_screen_threshold=None,
                          max_scene_threshold=None, max_screen_threshold=None, min_weight_threshold=None, prune_visibility=False, prune_large_gs=False):
        """:866-899, the same order: clone, split, prune by opacity / gradient, [prune or split the oversized], [prune the least visible], reset."""
        if self.device_schedule:
            self.grow_and_prune(min_opacity, min_gradient, densify_grad_threshold, densify_size_threshold, split_screen_threshold)
        else:
            self.densify_and_clone(densify_grad_threshold, densify_size_threshold)
            self.densify_and_split(densify_grad_threshold, densify_size_threshold, split_screen_threshold)
            self.prune_min_opacity_and_gradients(min_opacity, min_gradient)
        if prune_large_gs:
            self.prune_max_scene_and_screen(max_scene_threshold, max_screen_threshold, min_weight_threshold)
        if prune_visibility:
            self.prune_visibility()
        self.reset_stats()
