"""CPU: the trace oracle's forced hit lists, its audit kinds and ambiguous sets, and the validator of a GPU list (tests/trace_lists.py).
None of this needs a GPU: it is the machinery tests/test_trace_parity.py compares the fragile rays with."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import trace as otr
from oracle.raster import lib
from tests.test_oracle_trace import trace_scene, _ORACLE_CASES
from tests.trace_lists import validate_gpu_list, replay_rows, pad_lists, fragile_scene, ListRejected


@contextlib.contextmanager
def _one_thread():
    """The oracle sums per-surfel gradients over rays by atomics in thread order: bit-for-bit comparisons of two runs need one thread."""
    L = lib()
    old = L.omp_get_max_threads()
    L.omp_set_num_threads(1)
    try:
        yield
    finally:
        L.omp_set_num_threads(old)


def _args(g):
    return tuple(g[k].numpy() for k in ("means3D", "scales", "rotations", "opacities"))


def _case(use_sh, camera, deg, seed=3):
    g, ro, rd = trace_scene(seed=seed, camera=camera)
    ckw = dict(shs=g["shs"].numpy(), sh_degree=deg) if use_sh else dict(colors_precomp=g["colors_precomp"].numpy())
    akw = dict(shs=g["shs"].numpy(), sh_degree=deg) if use_sh else {}
    return g, ro.numpy(), rd.numpy(), ckw, akw


def _grads(R, seed=9):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(R, 3, generator=gen).numpy(), torch.randn(R, generator=gen).numpy(), torch.randn(R, generator=gen).numpy(),
            torch.randn(R, 3, generator=gen).numpy(), torch.randn(R, 2, generator=gen).numpy()]


FWD_KEYS = ("rgb", "dpt", "acc", "norm", "dist", "aux", "mid", "wet", "final_T", "nhits", "dist64", "dist_bound")


def _same(a, b, what):
    for k in a:
        if a[k] is None or isinstance(a[k], dict):
            continue
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), "%s: %s differs" % (what, k)


@pytest.mark.parametrize("use_sh,camera,deg", _ORACLE_CASES, ids=["-".join(str(x) for x in c) for c in _ORACLE_CASES])
@pytest.mark.parametrize("scale_modifier", [1.0, 1.7])
def test_forcing_the_natural_list_is_the_identity(use_sh, camera, deg, scale_modifier):
    """Every ray forced to the list it composites anyway: forward and backward bit for bit what they are without the override -- so the forced path
    evaluates a surfel with the same float code, sorts the same way and differs only in the decisions it does not take."""
    g, ro, rd, ckw, akw = _case(use_sh, camera, deg)
    R = ro.shape[0]
    kw = dict(others=g["others"].numpy(), bg=np.array([0.3, 0.1, 0.7], np.float32), start_from_first=camera, scale_modifier=scale_modifier, **ckw)
    a = otr.trace_audit(ro, rd, *_args(g), others=g["others"].numpy(), start_from_first=camera, scale_modifier=scale_modifier, detail=True, **akw)
    assert a["nhit"].max() > 5
    forced = (a["ids"], a["nhit"], np.ones(R, bool))
    with _one_thread():
        f0 = otr.trace_forward(ro, rd, *_args(g), **kw)
        f1 = otr.trace_forward(ro, rd, *_args(g), forced=forced, **kw)
        _same({k: f0[k] for k in FWD_KEYS}, f1, "forward")
        b0 = otr.trace_backward(f0, *_grads(R), want_cond=True)
        b1 = otr.trace_backward(f1, *_grads(R), want_cond=True)
        _same(b0, b1, "backward"); _same(b0["cond"], b1["cond"], "cond"); _same(b0["unc"], b1["unc"], "unc")
        # the override is cleared by the call that used it
        f2 = otr.trace_forward(ro, rd, *_args(g), **kw)
        _same({k: f0[k] for k in FWD_KEYS}, f2, "forward after a forced call")
    # ... and the audit's replay of the same lists composites the same entries and flags the same rays
    a1 = otr.trace_audit(ro, rd, *_args(g), others=g["others"].numpy(), start_from_first=camera, scale_modifier=scale_modifier, detail=True, forced=forced, **akw)
    for k in ("ids", "tbits", "nhit"):
        assert np.array_equal(a[k], a1[k]), k
    # a masked-out ray runs as before even when its row of the forced arrays holds nonsense
    junk = (np.zeros_like(a["ids"]), np.full(R, 3, np.int32), np.zeros(R, bool))
    _same({k: f0[k] for k in FWD_KEYS}, otr.trace_forward(ro, rd, *_args(g), forced=junk, **kw), "forward with nothing masked")


@pytest.mark.parametrize("use_sh,camera,deg", _ORACLE_CASES, ids=["-".join(str(x) for x in c) for c in _ORACLE_CASES])
def test_audit_kinds_are_the_fragile_flag(use_sh, camera, deg):
    """kind != 0 <=> fragile, and asking for the detail changes none of the fields the audit always returned -- on the oracle scenes, with the bounce
    decisions audited too (the deep scene, where the other kinds all occur: the `deep` fixture below)."""
    g, ro, rd, ckw, akw = _case(use_sh, camera, deg)
    for mod in (1.0, 1.7):
        kw = dict(others=g["others"].numpy(), start_from_first=camera, scale_modifier=mod, bounce_thr=0.1, **akw)
        a0 = otr.trace_audit(ro, rd, *_args(g), **kw)
        a1 = otr.trace_audit(ro, rd, *_args(g), detail=True, **kw)
        for k in ("fragile", "ids", "tbits", "nhit"):
            assert np.array_equal(a0[k], a1[k]), k
        assert np.array_equal(a1["kind"] != 0, a0["fragile"])
        assert not a1["amb_overflow"].any()
        for r in range(ro.shape[0]):
            assert (a1["cand"][r] is not None) == bool(a0["fragile"][r])


@pytest.fixture(scope="module")
def deep():
    g, ro, rd, bg, deg = fragile_scene()
    kw = dict(others=g["others"].numpy(), start_from_first=False, shs=g["shs"].numpy(), sh_degree=deg)
    a0 = otr.trace_audit(ro.numpy(), rd.numpy(), *_args(g), **kw)
    a = otr.trace_audit(ro.numpy(), rd.numpy(), *_args(g), detail=True, **kw)
    for k in ("fragile", "ids", "tbits", "nhit"):
        assert np.array_equal(a0[k], a[k]), k
    return dict(g=g, ro=ro.numpy(), rd=rd.numpy(), kw=kw, a=a)


def test_deep_scene_has_every_kind_and_no_overflowed_ambiguous_set(deep):
    a = deep["a"]
    assert np.array_equal(a["kind"] != 0, a["fragile"])
    n = {nm: int(((a["kind"] & b) != 0).sum()) for nm, b in (("geom", otr.KIND_GEOM), ("term", otr.KIND_TERM), ("clamp", otr.KIND_CLAMP))}
    assert int(a["fragile"].sum()) >= 8 and n["geom"] >= 1 and n["term"] >= 1 and n["clamp"] >= 1, n
    assert n["clamp"] <= 0.01 * a["fragile"].size            # the share whose colour gradient the GPU tests cannot replay
    assert not a["amb_overflow"].any() and a["namb"].max() <= otr.AMB_CAP
    assert all(a["cand"][r] is not None for r in np.nonzero(a["fragile"])[0])
    for r in np.nonzero(a["fragile"])[0]:                   # the composited list is the natural list up to the termination
        c = a["cand"][r]
        nat = c["ids"][(c["flags"] & otr.CAND_HIT) != 0]
        assert np.array_equal(nat[:a["nhit"][r]], a["ids"][r, :a["nhit"][r]])
        assert np.array_equal(c["tbits"][(c["flags"] & otr.CAND_HIT) != 0][:a["nhit"][r]], a["tbits"][r, :a["nhit"][r]])
        assert set(a["amb_ids"][r, :a["namb"][r]]) == set(c["ids"][(c["flags"] & otr.CAND_AMB) != 0])


def _pick(deep, want_kind):
    """A fragile ray of the deep scene of the given kind."""
    return int(np.nonzero((deep["a"]["kind"] & want_kind) != 0)[0][0])


def _validate(deep, r, G):
    rows, _ = replay_rows((deep["ro"][r:r + 1], deep["rd"][r:r + 1]), [G], _args(deep["g"]), **deep["kw"])
    return validate_gpu_list(rows[0], G, ray=r)


def _natural(deep, r):
    a = deep["a"]
    return [int(x) for x in a["ids"][r, :a["nhit"][r]]]


def test_validator_accepts_the_natural_list_of_every_fragile_ray(deep):
    a = deep["a"]
    fr = np.nonzero(a["fragile"])[0]
    lists = [_natural(deep, r) for r in fr]
    rows, _ = replay_rows((deep["ro"][fr], deep["rd"][fr]), lists, _args(deep["g"]), **deep["kw"])
    for r, row, G in zip(fr, rows, lists):
        assert validate_gpu_list(row, G, ray=r) == 0


def test_validator_accepts_a_toggled_ambiguous_hit(deep):
    """An ambiguous candidate the float code accepts may be missing, one it rejects may be there -- at its place in the (t, id) order.  The toggled hit
    changes T for everything behind it, so the list ends where the replay of the toggled candidates first terminates."""
    a = deep["a"]
    done = {True: 0, False: 0}
    for r in np.nonzero((a["kind"] & (otr.KIND_GEOM | otr.KIND_DISAGREE)) != 0)[0]:
        c = a["cand"][r]
        hit = (c["flags"] & otr.CAND_HIT) != 0; amb = (c["flags"] & otr.CAND_AMB) != 0
        last_t = a["tbits"][r, a["nhit"][r] - 1]
        for k in np.nonzero(amb & (c["tbits"] < last_t))[0]:          # (positive floats: their bits order like their values)
            take = hit.copy(); take[k] = not hit[k]
            full = [int(i) for i in c["ids"][take]]
            rows, _ = replay_rows((deep["ro"][r:r + 1], deep["rd"][r:r + 1]), [full], _args(deep["g"]), **deep["kw"])
            stop = np.nonzero((rows[0]["go"][:len(full)] & 1) == 0)[0]
            G = full[:int(stop[0])] if stop.size else full
            assert _validate(deep, int(r), G) == 1
            with pytest.raises(ListRejected):                         # ... but not anywhere else in the list
                moved = [i for i in G if i != int(c["ids"][k])]
                _validate(deep, int(r), [int(c["ids"][k])] + moved if not hit[k] else moved[:-1])
            done[bool(hit[k])] += 1
    assert done[True] >= 1 and done[False] >= 1, done


def test_validator_accepts_a_stop_moved_across_a_near_threshold_termination(deep):
    """A ray of termination kind: the hit whose T (1 - alpha) is within noise of 1e-4 may end the list or be composited."""
    a = deep["a"]
    moved = 0
    for r in np.nonzero((a["kind"] & otr.KIND_TERM) != 0)[0]:
        c = a["cand"][r]
        nat_all = [int(i) for i, f in zip(c["ids"], c["flags"]) if f & otr.CAND_HIT]
        n = int(a["nhit"][r])
        go = a["go"][r, :n]
        if n < len(nat_all) and not (go & 2).any():          # the near-threshold test is the terminating one: going one hit further is legitimate
            assert _validate(deep, r, nat_all[:n + 1]) == 0
            with pytest.raises(ListRejected, match="decisive termination"):
                _validate(deep, r, nat_all[:n + 2])
            moved += 1
        elif (go & 2).any():                                 # a composited hit was near the threshold: stopping in front of it is legitimate
            k = int(np.nonzero(go & 2)[0][0])
            assert _validate(deep, r, nat_all[:k]) == 0
            moved += 1
    assert moved >= 1


def test_validator_rejects_doctored_lists(deep):
    r = _pick(deep, otr.KIND_GEOM)
    a = deep["a"]
    c = a["cand"][r]
    nat = _natural(deep, r)
    amb = {int(i) for i, f in zip(c["ids"], c["flags"]) if f & otr.CAND_AMB}
    assert len(nat) > 20 and _validate(deep, r, nat) == 0
    un = [k for k, i in enumerate(nat) if i not in amb and (k + 1 < len(nat) and nat[k + 1] not in amb)]
    k = un[len(un) // 2]
    swapped = list(nat); swapped[k], swapped[k + 1] = swapped[k + 1], swapped[k]
    with pytest.raises(ListRejected, match="order"):
        _validate(deep, r, swapped)
    with pytest.raises(ListRejected, match="unambiguous hit"):
        _validate(deep, r, nat[:k] + nat[k + 1:])                         # an unambiguous hit dropped
    with pytest.raises(ListRejected, match="twice"):
        _validate(deep, r, nat[:k + 1] + [nat[k]] + nat[k + 1:])          # an id duplicated
    with pytest.raises(ListRejected, match="stops in front of the unambiguous hit"):
        _validate(deep, r, nat[:len(nat) // 2])                           # an early stop at a decisive T
    nat_all = [int(i) for i, f in zip(c["ids"], c["flags"]) if f & otr.CAND_HIT]
    assert len(nat_all) >= len(nat) + 3
    with pytest.raises(ListRejected, match="decisive termination"):
        _validate(deep, r, nat_all[:len(nat) + 3])                        # continuing past a decisive stop
    foreign = next(i for i in range(a["ids"].shape[1]) if i not in {int(x) for x in c["ids"]})
    with pytest.raises(ListRejected, match="neither a hit nor an ambiguous candidate"):
        _validate(deep, r, nat[:k] + [foreign] + nat[k:])                 # a foreign id
    with pytest.raises(ListRejected):
        _validate(deep, r, [])                                            # nothing composited at all


def test_forced_deletion_equals_the_scene_without_that_surfel():
    """R = 1: the natural list minus entry j, forced, against the unforced oracle on the scene with that surfel removed -- forward and the remaining
    surfels' gradients bit for bit (a ray that does not terminate, so that removing a hit changes no later decision)."""
    use_sh, camera, deg = _ORACLE_CASES[0]
    g, ro, rd, ckw, akw = _case(use_sh, camera, deg)
    P = g["means3D"].shape[0]
    a = otr.trace_audit(ro, rd, *_args(g), others=g["others"].numpy(), start_from_first=camera, detail=True, pool_cap=1 << 20, **akw)
    full = otr.trace_forward(ro, rd, *_args(g), others=g["others"].numpy(), start_from_first=camera, **ckw)
    r = int(np.nonzero((full["final_T"] > 1e-2) & (full["nhits"] >= 6))[0][0])          # far from terminating
    nat = [int(x) for x in a["ids"][r, :a["nhit"][r]]]
    o1, d1 = ro[r:r + 1], rd[r:r + 1]
    bg = np.array([0.3, 0.1, 0.7], np.float32)
    gr = _grads(1)
    for j in (0, len(nat) // 2, len(nat) - 1):
        sid = nat[j]
        ids, n = pad_lists([nat[:j] + nat[j + 1:]])
        keep = np.array([i for i in range(P) if i != sid])
        sub = lambda x: None if x is None else np.ascontiguousarray(x[keep])
        with _one_thread():
            f = otr.trace_forward(o1, d1, *_args(g), others=g["others"].numpy(), bg=bg, start_from_first=camera, forced=(ids, n, np.ones(1, bool)), **ckw)
            b = otr.trace_backward(f, *gr)
            ckw2 = {k: (sub(v) if isinstance(v, np.ndarray) else v) for k, v in ckw.items()}
            f2 = otr.trace_forward(o1, d1, *[sub(x) for x in _args(g)], others=sub(g["others"].numpy()), bg=bg, start_from_first=camera, **ckw2)
            b2 = otr.trace_backward(f2, *gr)
        assert f["nhits"][0] == len(nat) - 1 == f2["nhits"][0]
        for k in ("rgb", "dpt", "acc", "norm", "dist", "aux", "final_T", "dist64"):
            assert f[k].tobytes() == f2[k].tobytes(), (j, k)
        assert f["wet"][keep].tobytes() == f2["wet"].tobytes() and f["wet"][sid] == 0.0
        for k in b:
            if b[k] is None:
                continue
            if k in ("dray_o", "dray_d"):
                assert b[k].tobytes() == b2[k].tobytes(), (j, k)
            else:
                assert np.ascontiguousarray(b[k][keep]).tobytes() == b2[k].tobytes(), (j, k)
                assert not np.any(b[k][sid]), (j, k)


def test_forced_extension_composites_past_the_termination(deep):
    """A list that goes on past the natural termination point composites the extra hit: nhits grows by one and final_T is the running product of
    1 - alpha over the list, in float, in list order."""
    a, g = deep["a"], deep["g"]
    r = _pick(deep, otr.KIND_TERM)
    c = a["cand"][r]
    hit = (c["flags"] & otr.CAND_HIT) != 0
    nat_all = [int(i) for i in c["ids"][hit]]
    alpha = c["alpha"][hit]
    n = int(a["nhit"][r])
    assert n < len(nat_all)
    kw = dict(others=g["others"].numpy(), start_from_first=False, shs=g["shs"].numpy(), sh_degree=2)
    o1, d1 = deep["ro"][r:r + 1], deep["rd"][r:r + 1]
    f0 = otr.trace_forward(o1, d1, *_args(g), **kw)
    ids, cnt = pad_lists([nat_all[:n + 1]])
    f1 = otr.trace_forward(o1, d1, *_args(g), forced=(ids, cnt, np.ones(1, bool)), **kw)
    assert f0["nhits"][0] == n and f1["nhits"][0] == n + 1
    T = np.float32(1.0)
    for k in range(n + 1):
        if k == n:
            assert f0["final_T"][0] == T
        T = np.float32(T * np.float32(np.float32(1.0) - alpha[k]))
    assert f1["final_T"][0] == T and T < np.float32(1e-4)
    assert f1["wet"][nat_all[n]] > 0 and f0["wet"][nat_all[n]] == 0
