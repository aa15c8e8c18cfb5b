"""Independent numpy restatement of the global search (include/sps_hip.h, "NDT localiser, global search"):
the occupancy grid and its pooled levels, the per-yaw integer offsets of the scan slice, the branch and bound with its
frontier and certificate, and -- sharing nothing with it but the offsets -- an exhaustive scorer over all leaves.  It
shares no code with sps_amd/localiser.py.  Floating point is float64 with every operation rounded on its own (numpy
ufuncs never contract a multiply and an add); scores are integers, so nothing depends on an order of summation."""
import numpy as np

from tests import localiser_reference as LR

LIMIT = 1048576.0


# ---- grid ----------------------------------------------------------------------------------------------------------------
def grid(map_xyz, r, map_z):
    """-> (G0 uint8 [H, W], i0, j0): cell (floor(x / r) - i0, floor(y / r) - j0) of every map point with lo <= z <= hi"""
    xyz = np.asarray(map_xyz, dtype=np.float64)
    sel = xyz[(xyz[:, 2] >= map_z[0]) & (xyz[:, 2] <= map_z[1])]
    if len(sel) == 0:
        return np.zeros((1, 1), np.uint8), 0, 0
    c = np.floor(sel[:, :2] / np.float64(r)).astype(np.int64)
    i0, j0 = int(c[:, 0].min()), int(c[:, 1].min())
    G0 = np.zeros((int(c[:, 1].max()) - j0 + 1, int(c[:, 0].max()) - i0 + 1), np.uint8)
    G0[c[:, 1] - j0, c[:, 0] - i0] = 1
    return G0, i0, j0


def pooled(G0, l):
    """G_l by its definition, as an array [H + p, W + p], p = 2^l - 1, with G_l(x, y) at [y + p, x + p]"""
    H, W = G0.shape
    p = (1 << l) - 1
    big = np.zeros((H + 2 * p, W + 2 * p), np.uint8)
    big[p:p + H, p:p + W] = G0
    out = np.zeros((H + p, W + p), np.uint8)
    for dj in range(1 << l):
        for di in range(1 << l):
            np.maximum(out, big[dj:dj + H + p, di:di + W + p], out=out)
    return out


def stored(G0, L, l):
    """level l in the layout of the device: [H + pad, W + pad], pad = 2^L - 1, G_l(x, y) at [y + pad, x + pad]"""
    H, W = G0.shape
    pad, p = (1 << L) - 1, (1 << l) - 1
    out = np.zeros((H + pad, W + pad), np.uint8)
    out[pad - p:, pad - p:] = pooled(G0, l)
    return out


def lookup(Gl, l, x, y):
    """G_l(x, y) for integer arrays x, y; 0 outside [-(2^l - 1), W) x [-(2^l - 1), H)"""
    p = (1 << l) - 1
    xs, ys = x + p, y + p
    ok = (xs >= 0) & (xs < Gl.shape[1]) & (ys >= 0) & (ys < Gl.shape[0])
    out = np.zeros(np.broadcast(xs, ys).shape, np.int64)
    out[ok] = Gl[ys[ok], xs[ok]]
    return out


# ---- scan ----------------------------------------------------------------------------------------------------------------
def yaw_table(A):
    ang = 2.0 * np.pi * np.arange(A, dtype=np.float64) / np.float64(A)
    return np.stack([np.cos(ang), np.sin(ang)], axis=1)


def offsets(pts, T_up, scan_z, r, cs):
    """pts: the thinned points [n, 3] float64 -> (per yaw a pair (dx, dy) of int64 arrays over the points that count at
    that yaw, the number of points in the slice)"""
    q = LR.transform(np.asarray(pts, dtype=np.float64).reshape(-1, 3), np.asarray(T_up, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        keep = (q[:, 2] >= scan_z[0]) & (q[:, 2] <= scan_z[1])
    q = q[keep]
    out = []
    for c, s in cs:
        with np.errstate(invalid="ignore", over="ignore"):
            u = c * q[:, 0] - s * q[:, 1]
            v = s * q[:, 0] + c * q[:, 1]
            fu, fv = u / np.float64(r), v / np.float64(r)
            ok = (np.abs(fu) <= LIMIT) & (np.abs(fv) <= LIMIT)
        out.append((np.floor(fu[ok]).astype(np.int64), np.floor(fv[ok]).astype(np.int64)))
    return out, int(keep.sum())


def leaf_pose(a, j, i, cs, r, i0, j0, T_up):
    U = np.asarray(T_up, dtype=np.float64)
    c, s = cs[a]
    T = U.copy()
    T[0] = c * U[0] - s * U[1]
    T[1] = s * U[0] + c * U[1]
    T[0, 3] = T[0, 3] + np.float64(r) * np.float64(i0 + i)
    T[1, 3] = T[1, 3] + np.float64(r) * np.float64(j0 + j)
    return T


# ---- search --------------------------------------------------------------------------------------------------------------
def score_nodes(Gl, l, nodes, offs):
    """nodes int64 [m, 3] rows (a, j, i) -> their scores at level l"""
    out = np.zeros(len(nodes), np.int64)
    for a in np.unique(nodes[:, 0]):
        at = np.nonzero(nodes[:, 0] == a)[0]
        dx, dy = offs[a]
        for c0 in range(0, len(at), 4096):
            sel = at[c0:c0 + 4096]
            out[sel] = lookup(Gl, l, nodes[sel, 2][:, None] + dx[None, :], nodes[sel, 1][:, None] + dy[None, :]).sum(axis=1)
    return out


def search(G0, L, r, i0, j0, pts, A, keep=8, frontier=16384, min_score=1, scan_z=(-np.inf, np.inf), T_up=None):
    """-> dict(index, score, poses, n_found, certified, dropped_bound, n_dropped, candidates, kept, n_slice,
    candidate_lists, kept_lists, slot_lists, slot_scores), the lists as leaf / node ids per level.  slot_lists[l] is the
    candidate list of level l as the device lays it out -- at level L the root order, below it four slots per kept parent
    in the parents' order, -1 where the child is outside the grid -- and slot_scores[l] the score of every slot, -1 for a
    void"""
    H, W = G0.shape
    T_up = np.eye(4) if T_up is None else np.asarray(T_up, dtype=np.float64)
    if not 1 <= keep <= 64:
        raise ValueError("keep")
    if A * H * W >= 1 << 31:
        raise ValueError("id overflow")
    cs = yaw_table(A)
    step = 1 << L
    nodes = np.array([(a, j, i) for a in range(A) for j in range(0, H, step) for i in range(0, W, step)], np.int64).reshape(-1, 3)
    if len(nodes) > 4 * frontier:
        raise ValueError("too many candidates")
    offs, n_slice = offsets(pts, T_up, scan_z, r, cs)
    ids = lambda nd: (nd[:, 0] * H + nd[:, 1]) * W + nd[:, 2]
    bound, n_dropped = -1, 0
    n_cand, n_kept, cand_lists, kept_lists = np.zeros(L + 1, np.int64), np.zeros(L + 1, np.int64), [None] * (L + 1), [None] * (L + 1)
    slot_lists, slot_scores = [None] * (L + 1), [None] * (L + 1)
    filled = np.ones(len(nodes), bool)                                       # the slots of the level that hold a node
    for l in range(L, -1, -1):
        sc = score_nodes(pooled(G0, l), l, nodes, offs)
        alive = np.nonzero(sc >= min_score)[0]
        if len(alive) > frontier:
            order = sorted(alive.tolist(), key=lambda c: (-int(sc[c]), c))       # score descending, position ascending
            alive = np.array(sorted(order[:frontier]), np.int64)
        gone = np.ones(len(nodes), bool)
        gone[alive] = False
        if gone.any():
            bound = max(bound, int(sc[gone].max()))
        n_dropped += int(gone.sum())
        n_cand[l], n_kept[l], cand_lists[l], kept_lists[l] = len(nodes), len(alive), ids(nodes), ids(nodes[alive])
        slot_lists[l], slot_scores[l] = np.full(len(filled), -1, np.int64), np.full(len(filled), -1, np.int64)
        slot_lists[l][filled], slot_scores[l][filled] = ids(nodes), sc
        kept_nodes, kept_scores = nodes[alive], sc[alive]
        if l > 0:
            h = 1 << (l - 1)
            kids, inside = [], []
            for a, j, i in kept_nodes.tolist():
                for dj, di in ((0, 0), (0, 1), (1, 0), (1, 1)):
                    inside.append(i + di * h < W and j + dj * h < H)
                    if inside[-1]:
                        kids.append((a, j + dj * h, i + di * h))
            nodes, filled = np.array(kids, np.int64).reshape(-1, 3), np.array(inside, bool)
    leaf_ids = ids(kept_nodes)
    order = sorted(range(len(leaf_ids)), key=lambda c: (-int(kept_scores[c]), int(leaf_ids[c])))[:keep]
    index, score = np.full(keep, -1, np.int64), np.zeros(keep, np.int64)
    poses = np.tile(T_up, (keep, 1, 1))
    for k, c in enumerate(order):
        a, j, i = kept_nodes[c].tolist()
        index[k], score[k], poses[k] = leaf_ids[c], kept_scores[c], leaf_pose(a, j, i, cs, r, i0, j0, T_up)
    if order:
        poses[len(order):] = poses[0]
    certified = 0
    while certified < len(order) and score[certified] > bound:
        certified += 1
    return dict(index=index, score=score, poses=poses, n_found=len(order), certified=certified, dropped_bound=bound,
                n_dropped=n_dropped, candidates=n_cand, kept=n_kept, n_slice=n_slice, candidate_lists=cand_lists,
                kept_lists=kept_lists, slot_lists=slot_lists, slot_scores=slot_scores)


# ---- exhaustive scorer ---------------------------------------------------------------------------------------------------
def exhaustive(G0, r, pts, A, scan_z=(-np.inf, np.inf), T_up=None):
    """scores int64 [A, H, W] of every leaf, by adding shifted copies of G0: one per distinct offset of the yaw, weighted by
    the points that have it.  No pyramid, no node list."""
    H, W = G0.shape
    T_up = np.eye(4) if T_up is None else np.asarray(T_up, dtype=np.float64)
    offs, _ = offsets(pts, T_up, scan_z, r, yaw_table(A))
    G = G0.astype(np.int64)
    out = np.zeros((A, H, W), np.int64)
    for a, (dx, dy) in enumerate(offs):
        near = (np.abs(dx) < W) & (np.abs(dy) < H)                        # farther offsets reach no cell from any leaf
        if not near.any():
            continue
        uniq, cnt = np.unique(np.stack([dy[near], dx[near]], axis=1), axis=0, return_counts=True)
        for (oy, ox), c in zip(uniq.tolist(), cnt.tolist()):
            # leaf (j, i) reads G0[j + oy, i + ox]
            j_lo, j_hi, i_lo, i_hi = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
            out[a, j_lo:j_hi, i_lo:i_hi] += c * G[j_lo + oy:j_hi + oy, i_lo + ox:i_hi + ox]
    return out


def exhaustive_ranking(scores, keep, min_score=1):
    """-> (ids, scores) of the first ``keep`` leaves with score >= min_score by (score descending, id ascending)"""
    flat = scores.reshape(-1)
    ids = np.nonzero(flat >= min_score)[0]
    order = ids[np.lexsort((ids, -flat[ids]))][:keep]
    return order.astype(np.int64), flat[order]
