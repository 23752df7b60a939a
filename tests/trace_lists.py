"""What a traced ray's composited hit list may be, when some of its decisions lie within fp32 noise of their thresholds (pure numpy; no GPU).

The oracle's audit (oracle/surfel_trace_oracle.c: trc_audit, oracle/trace.py: trace_audit(detail=True)) gives per fragile ray
  N  the natural candidate list: every float-accepted hit in (t, id) order, termination not applied (candidate flag CAND_HIT),
  A  the ambiguous set: surfels whose |u|, |v| or alpha test is near its threshold or decided differently in float and double (CAND_AMB),
and, when the ray is REPLAYED under a given list G (forced=...), per entry of G whether going on was legitimate (`go`) and per candidate behind G's
last entry whether the walk may stop there (CAND_BEHIND, CAND_STOPS).  validate_gpu_list says whether G differs from brute force only in decisions
the audit itself marks ambiguous; anything else is a kernel bug."""
import numpy as np

from oracle import trace as otr


class ListRejected(AssertionError):
    pass


def validate_gpu_list(audit_row, gpu_ids, ray=None):
    """audit_row: one ray of a forced audit that replayed gpu_ids -- dict(cand=dict(ids, tbits, alpha, flags), ids, nhit, go).  Returns the number of
    ambiguous decisions the list takes differently from the natural list; raises ListRejected with the ray index and both lists otherwise."""
    G = [int(x) for x in gpu_ids]
    c = audit_row["cand"]
    assert c is not None, "ray %s: the audit kept no candidates for this ray" % ray
    cid = [int(x) for x in c["ids"]]
    fl = np.asarray(c["flags"]).astype(int)
    hit = (fl & otr.CAND_HIT) != 0
    amb = (fl & otr.CAND_AMB) != 0
    natural = [i for i, h in zip(cid, hit) if h]

    def reject(why):
        raise ListRejected("ray %s: %s\n  GPU list    (%d) %s\n  natural hits (%d) %s\n  ambiguous    %s" % (
            ray, why, len(G), G, len(natural), natural, [i for i, a in zip(cid, amb) if a]))

    if len(set(G)) != len(G):
        reject("surfel %d is composited twice" % next(i for i in G if G.count(i) > 1))
    pos = {i: k for k, i in enumerate(cid)}
    for i in G:
        if i not in pos:
            reject("surfel %d is neither a hit nor an ambiguous candidate of this ray" % i)
    p = [pos[i] for i in G]                 # the candidates are in the oracle's (t, id) order (t is bit-exact by construction): positions must increase
    for k in range(len(p) - 1):
        if p[k] >= p[k + 1]:
            reject("surfels %d and %d are not in (t, id) order" % (G[k], G[k + 1]))
    # no unambiguous hit skipped or reordered: G \ A is a prefix of N \ A, and nothing unambiguous is missing in front of G's last entry
    inG = set(G)
    n_unamb = [i for i, h, a in zip(cid, hit, amb) if h and not a]
    g_unamb = [i for i in G if not amb[pos[i]]]
    if g_unamb != n_unamb[:len(g_unamb)]:
        reject("the unambiguous hits %s are not a prefix of the natural ones %s" % (g_unamb, n_unamb[:len(g_unamb) + 1]))
    last = p[-1] if p else -1
    for k in range(last):
        if hit[k] and not amb[k] and cid[k] not in inG:
            reject("the unambiguous hit %d in front of the list's last entry is missing" % cid[k])
    # going on was legitimate at every entry: the forced replay composited G in the same order
    n = int(audit_row["nhit"])
    if n != len(G) or [int(x) for x in audit_row["ids"][:n]] != G:
        reject("the oracle replayed another list: %s" % [int(x) for x in audit_row["ids"][:n]])
    go = np.asarray(audit_row["go"][:n]).astype(int)
    for k in range(n):
        if go[k] == 0:
            reject("entry %d (surfel %d) is composited behind a decisive termination (T (1 - alpha) < 1e-4, not near the threshold)" % (k, G[k]))
    # stopping was legitimate: behind G's last entry only ambiguous candidates may be passed, up to the end or to one that terminates (or nearly does)
    for k in range(last + 1, len(cid)):
        assert fl[k] & otr.CAND_BEHIND, "ray %s: the audit row does not belong to this list" % ray
        if fl[k] & otr.CAND_STOPS:
            break
        if not amb[k]:
            reject("the list stops in front of the unambiguous hit %d, which does not terminate the ray" % cid[k])
    nat_in = set(natural)
    return sum(1 for i, a in zip(cid, amb) if a and pos[i] <= max(last, 0) and ((i in inG) != (i in nat_in)))


def pad_lists(lists, R=None, cap=None):
    """[(ray, ids)] or a list of id lists -> (ids (R, cap) int32 padded with -1, n (R,) int32)."""
    R = len(lists) if R is None else R
    cap = max([len(l) for l in lists] + [1]) if cap is None else cap
    ids = np.full((R, cap), -1, np.int32); n = np.zeros(R, np.int32)
    for r, l in enumerate(lists):
        ids[r, :len(l)] = l; n[r] = len(l)
    return ids, n


def replay_rows(rays, lists, scene_args, **audit_kw):
    """Forced audit of `rays` = (ray_o, ray_d) numpy (one row per list) under `lists`: the rows validate_gpu_list takes."""
    ids, n = pad_lists(lists)
    a = otr.trace_audit(rays[0], rays[1], *scene_args, detail=True, forced=(ids, n, np.ones(len(lists), bool)), lcap=ids.shape[1], **audit_kw)
    rows = [dict(cand=a["cand"][r], ids=a["ids"][r], nhit=a["nhit"][r], go=a["go"][r], kind=int(a["kind"][r])) for r in range(len(lists))]
    return rows, a


def fragile_scene():
    """The deep-list scene of test_fragile_rays_*: 1000 faint surfels packed into a tiny cluster plus a sparse far set, 4096 rays through the cluster
    (~200 composited hits per ray, up to ~440: within the 1024-entry list capacity).  Returns (g, ro, rd, bg, sh degree)."""
    import torch
    gen = torch.Generator().manual_seed(21)
    Pc, Pf = 1000, 200
    means = torch.cat([torch.tensor([0.0, 0.0, 5.0]) + 0.02 * torch.randn(Pc, 3, generator=gen), (torch.rand(Pf, 3, generator=gen) * 2 - 1) * 30])
    P = Pc + Pf
    scales = torch.cat([0.3 + 0.3 * torch.rand(Pc, 2, generator=gen), 2 + 2 * torch.rand(Pf, 2, generator=gen)])
    q = torch.randn(P, 4, generator=gen)
    g = dict(means3D=means, scales=scales, rotations=q / q.norm(dim=-1, keepdim=True), opacities=torch.sigmoid(torch.randn(P, 1, generator=gen) - 2.5),
             shs=torch.randn(P, 16, 3, generator=gen) * 0.3, others=torch.rand(P, 2, generator=gen))
    R = 4096
    ro = torch.randn(R, 3, generator=gen) * 0.2
    tgt = torch.tensor([0.0, 0.0, 5.0]) + 0.3 * torch.randn(R, 3, generator=gen)
    rd = tgt - ro; rd = rd / rd.norm(dim=-1, keepdim=True)
    return g, ro, rd, torch.tensor([0.2, 0.2, 0.2]), 2
