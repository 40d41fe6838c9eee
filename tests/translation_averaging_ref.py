"""Numpy restatement of the gtsfm_transavg_* entry points (include/gtsfm_hip.h): world-frame measurements and track
selection, the sequential greedy MFAS with the contract's operation order, and the recovery LM with two linear solvers,
"pcg" (the kernel's block-Jacobi conjugate gradients) and "exact" (a dense solve of the damped normal equations). MFAS
and the selection are exact restatements (same operations in the same order); the LM sums by np.bincount, so it agrees
with the kernels to rounding. MFAS also reports, per direction, the smallest decision margin it met."""
from typing import NamedTuple

import numpy as np

MIN_TRACK_MEASUREMENTS_FOR_AVERAGING = 3
TRACKS_MEASUREMENTS_PER_CAMERA = 12
OUTLIER_WEIGHT_THRESHOLD = 0.125
SOURCE_EPS = 1e-8
NEAR_TIE = 1e-9
HUBER_K = 1.345
ISIG = 100.0
PRIOR_W = 1.0e4
MIN_FIDELITY = 1e-3
LAMBDA_UPPER = 1e5
DBL_EPS = 2.220446049250313e-16
INNER_MAX = 64
_M64 = (1 << 64) - 1


def sm_mix(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def initial_value(seed: int, node: int) -> np.ndarray:
    base = sm_mix((seed & _M64) ^ sm_mix(node))
    return np.array([2.0 * ((sm_mix((base + k) & _M64) >> 11) * (1.0 / 9007199254740992.0)) - 1.0 for k in range(3)])


def unit3(p):
    """Unit3(p): every component divided by sqrt(x x + y y + z z); a zero vector stays zero."""
    p = np.asarray(p, np.float64)
    n2 = (p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]) + p[..., 2] * p[..., 2]
    n = np.sqrt(np.where(n2 > 0.0, n2, 1.0))
    return p / n[..., None]


def rotate(R, v):
    """Row-major 3 x 3 times vector, each row summed left to right."""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    v = np.asarray(v, np.float64).reshape(-1, 3)
    return (R[:, :, 0] * v[:, None, 0] + R[:, :, 1] * v[:, None, 1]) + R[:, :, 2] * v[:, None, 2]


def select_tracks(offsets, img, cam_valid, per_cam=TRACKS_MEASUREMENTS_PER_CAMERA):
    """_select_tracks_for_averaging on a CSR: the selected track ids in selection order."""
    offsets, img = np.asarray(offsets, np.int64), np.asarray(img, np.int64)
    T, n_img = len(offsets) - 1, len(cam_valid)
    ok = (img >= 0) & (img < n_img)
    ok[ok] = np.asarray(cam_valid).astype(bool)[img[ok]]
    cams = [[int(img[m]) for m in range(offsets[t], offsets[t + 1]) if ok[m]] for t in range(T)]
    improvement = np.array([len(c) if len(c) >= MIN_TRACK_MEASUREMENTS_FOR_AVERAGING else 0 for c in cams], np.int64)
    lookup = {}
    for t, c in enumerate(cams):
        if improvement[t] > 0:
            for i in c:
                lookup.setdefault(i, []).append(t)
    remaining = np.full(n_img, per_cam, np.int64)
    selected = []
    for _ in range(T):
        if T == 0:
            break
        best = int(np.argmax(improvement))
        if improvement[best] <= 0:
            break
        selected.append(best)
        improvement[best] = 0
        for i in cams[best]:
            if remaining[i] == 0:
                continue
            remaining[i] -= 1
            if remaining[i] == 0:
                for t in lookup[i]:
                    improvement[t] = improvement[t] - 1 if improvement[t] > 0 else 0
    return selected, cams


class Measurements(NamedTuple):
    key: np.ndarray  # (n_edges + n_meas, 2) int32
    dir: np.ndarray  # (n_edges + n_meas, 3)
    valid: np.ndarray  # uint8
    selected: list
    cam_valid: np.ndarray
    counts: np.ndarray  # the kernel's d_counts[4]


def measurements(edges, i2Ui1, edge_valid, wRi, rot_valid, offsets=None, img=None, uv=None, intr=None,
                 per_cam=TRACKS_MEASUREMENTS_PER_CAMERA) -> Measurements:
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    u = np.asarray(i2Ui1, np.float64).reshape(-1, 3)
    wRi = np.asarray(wRi, np.float64).reshape(-1, 3, 3)
    n_img, n_edges = len(wRi), len(edges)
    rv = np.ones(n_img, bool) if rot_valid is None else np.asarray(rot_valid).astype(bool)
    ev = np.ones(n_edges, bool) if edge_valid is None else np.asarray(edge_valid).astype(bool)
    n_meas = 0 if img is None else len(img)
    key = np.full((n_edges + n_meas, 2), -1, np.int32)
    d = np.zeros((n_edges + n_meas, 3))
    valid = np.zeros(n_edges + n_meas, np.uint8)
    cam_valid = np.zeros(n_img, np.uint8)
    i1, i2 = edges[:, 0], edges[:, 1]
    ok = ev & (i1 >= 0) & (i1 < n_img) & (i2 >= 0) & (i2 < n_img) & (i1 != i2)
    ok[ok] = rv[i2[ok]]
    e = np.nonzero(ok)[0]
    key[e, 0], key[e, 1] = i2[e], i1[e]
    d[e] = unit3(rotate(wRi[i2[e]], u[e]))
    valid[e] = 1
    cam_valid[i1[e]] = 1
    cam_valid[i2[e]] = 1
    selected, bad, slot = [], 0, n_edges
    if img is not None and len(offsets) > 1:
        offsets, img = np.asarray(offsets, np.int64), np.asarray(img, np.int64)
        uv = np.asarray(uv).reshape(-1, 2).astype(np.float64)
        K = np.asarray(intr, np.float64).reshape(-1, 3)
        selected, _ = select_tracks(offsets, img, cam_valid, per_cam)
        for s, t in enumerate(selected):
            for m in range(offsets[t], offsets[t + 1]):
                c = img[m]
                if not (0 <= c < n_img and cam_valid[c]):
                    continue
                if not rv[c]:
                    bad += 1
                    slot += 1
                    continue
                h = np.array([(uv[m, 0] - K[c, 1]) / K[c, 0], (uv[m, 1] - K[c, 2]) / K[c, 0], 1.0])
                d[slot] = unit3(rotate(wRi[c], unit3(h)[None])[0])
                key[slot] = (c, n_img + s)
                valid[slot] = 1
                slot += 1
    counts = np.array([len(e), slot - n_edges, len(selected), bad], np.int64)
    return Measurements(key, d, valid, selected, cam_valid, counts)


# ------------------------------------------------------------------ MFAS
def _weights(dirs, d):
    return (dirs[:, 0] * d[0] + dirs[:, 1] * d[1]) + dirs[:, 2] * d[2]


def mfas_use(key, valid, n_nodes):
    key = np.asarray(key, np.int64).reshape(-1, 2)
    v = np.ones(len(key), bool) if valid is None else np.asarray(valid).astype(bool)
    return v & (key[:, 0] >= 0) & (key[:, 0] < n_nodes) & (key[:, 1] >= 0) & (key[:, 1] < n_nodes) & \
        (key[:, 0] != key[:, 1])


def mfas_direction(key, dirs, use, n_nodes, d, incidence=None):
    """The sequential greedy ordering for one projection direction. Returns (violated mask over the measurements,
    |w|, removal position per node, the smallest decision margin met)."""
    key = np.asarray(key, np.int64).reshape(-1, 2)
    w = _weights(np.asarray(dirs, np.float64).reshape(-1, 3), np.asarray(d, np.float64))
    aw = np.abs(w)
    fwd = w >= 0.0
    src = np.where(fwd, key[:, 0], key[:, 1])
    dst = np.where(fwd, key[:, 1], key[:, 0])
    es = np.nonzero(use)[0]
    in_sum, out_sum = np.zeros(n_nodes), np.zeros(n_nodes)
    np.add.at(in_sum, dst[es], aw[es])  # unbuffered: ascending measurement index per node
    np.add.at(out_sum, src[es], aw[es])
    if incidence is None:
        incidence = [[] for _ in range(n_nodes)]
        for e in es:
            incidence[key[e, 0]].append(e)
            incidence[key[e, 1]].append(e)
    pos = np.full(n_nodes, -1, np.int64)
    margin = np.inf
    for step in range(n_nodes):
        rem = pos < 0
        margin = min(margin, float(np.min(np.abs(in_sum[rem] - SOURCE_EPS))))
        sources = np.nonzero(rem & (in_sum < SOURCE_EPS))[0]
        if len(sources):
            pick = int(sources[0])
        else:
            ratio = np.where(rem, (out_sum + 1.0) / (in_sum + 1.0), -np.inf)
            pick = int(np.argmax(ratio))  # first maximum: lowest index on ties
            if rem.sum() > 1:
                second = np.partition(ratio[rem], -2)[-2]
                margin = min(margin, float((ratio[pick] - second) / ratio[pick]))
        pos[pick] = step
        for e in incidence[pick]:
            other = key[e, 1] if key[e, 0] == pick else key[e, 0]
            if pos[other] >= 0:
                continue
            if src[e] == pick:
                in_sum[other] -= aw[e]
            else:
                out_sum[other] -= aw[e]
    violated = np.zeros(len(key), bool)
    violated[es] = pos[dst[es]] < pos[src[es]]
    return violated, aw, pos, margin


class MfasRef(NamedTuple):
    outlier_sum: np.ndarray
    inlier: np.ndarray
    violated: np.ndarray  # (n_dir, n_meas) bool
    margins: np.ndarray  # (n_dir,)


def mfas(key, dirs, valid, n_nodes, proj, threshold=OUTLIER_WEIGHT_THRESHOLD, only=None) -> MfasRef:
    """Every direction of proj (or the indices in `only`; outlier_sum and inlier are then over those alone)."""
    key = np.asarray(key, np.int64).reshape(-1, 2)
    proj = np.asarray(proj, np.float64).reshape(-1, 3)
    use = mfas_use(key, valid, n_nodes)
    incidence = [[] for _ in range(n_nodes)]
    for e in np.nonzero(use)[0]:
        incidence[key[e, 0]].append(e)
        incidence[key[e, 1]].append(e)
    idx = range(len(proj)) if only is None else only
    total = np.zeros(len(key))
    viol, margins = [], []
    for di in idx:
        v, aw, _, m = mfas_direction(key, dirs, use, n_nodes, proj[di], incidence)
        total = total + np.where(v, aw, 0.0)  # ascending direction index per edge
        viol.append(v)
        margins.append(m)
    inlier = (use & (total / len(idx) < threshold)).astype(np.uint8)
    return MfasRef(total, inlier, np.array(viol), np.array(margins))


def violated_bits_to_mask(bits, n_meas):
    """The kernel's d_violated words (n_dir, ceil(n_meas / 32)) uint32 as a (n_dir, n_meas) bool mask."""
    bits = np.asarray(bits).astype(np.uint32)
    e = np.arange(n_meas)
    return ((bits[:, e >> 5] >> (e & 31).astype(np.uint32)) & 1).astype(bool)


# ------------------------------------------------------------------ recovery
class RecoverRef(NamedTuple):
    wti: np.ndarray
    wti_valid: np.ndarray
    landmark: np.ndarray
    landmark_valid: np.ndarray
    stats: np.ndarray
    min_margin: float
    pcg_iters_per_solve: list


def _scatter(n, idx, vals):
    v = vals.reshape(len(idx), -1)
    out = np.stack([np.bincount(idx, v[:, j], minlength=n) for j in range(v.shape[1])], 1)
    return out.reshape((n,) + vals.shape[1:])


def recover(key, dirs, inlier, n_img, n_land, rot_valid=None, robust=True, scale=1.0, seed=0, max_iterations=0,
            pcg_rel_tol=1e-10, pcg_max_iter=2000, solver="pcg") -> RecoverRef:
    key = np.asarray(key, np.int64).reshape(-1, 2)
    dirs = np.asarray(dirs, np.float64).reshape(-1, 3)
    inl = np.asarray(inlier).astype(bool)
    n = n_img + n_land
    rv = np.ones(n_img, bool) if rot_valid is None else np.asarray(rot_valid).astype(bool)
    k1, k2 = key[:, 0], key[:, 1]
    ok = inl & (k1 >= 0) & (k1 < n_img) & (k2 >= 0) & (k2 < n) & (k1 != k2)
    cam_inl = np.zeros(n_img, bool)
    cc = ok & (k2 < n_img)
    cam_inl[k1[cc]] = True
    cam_inl[k2[cc]] = True
    kept = ok.copy()
    tr = ok & (k2 >= n_img)
    kept[tr] = cam_inl[k1[tr]]
    isvar = np.zeros(n, bool)
    isvar[k1[kept]] = True
    isvar[k2[kept]] = True
    rep = np.arange(n)
    zero = kept & (np.abs(dirs) <= 1e-9).all(1)
    changed = True
    while changed:
        changed = False
        for e in np.nonzero(zero)[0]:
            m = min(rep[k1[e]], rep[k2[e]])
            if rep[k1[e]] != m or rep[k2[e]] != m:
                rep[k1[e]] = rep[k2[e]] = m
                changed = True
    fe = np.nonzero(kept & (rep[k1] != rep[k2]))[0]
    stats = np.zeros(10)
    out_ok = isvar.copy()
    out_ok[:n_img] &= rv
    X = np.zeros((n, 3))

    def finish(status, margins, per_solve):
        stats[8] = out_ok[:n_img].sum()
        stats[9] = status
        P = np.where(out_ok[:, None], X[rep], 0.0)
        keys = ("fidelity", "stop", "relative", "absolute")
        mm = min([v for m in margins for k, v in m.items() if k in keys], default=np.inf)
        return RecoverRef(P[:n_img], out_ok[:n_img].astype(np.uint8), P[n_img:], out_ok[n_img:].astype(np.uint8), stats,
                          float(mm), per_solve)

    if not kept.any():
        return finish(1.0, [], [])
    if len(fe) == 0:
        return finish(0.0, [], [])
    fa, fb, fu = rep[k1[fe]], rep[k2[fe]], dirs[fe]
    # the scale factor is one more row, after the measurements
    ga, gb = np.append(fa, fa[0]), np.append(fb, fb[0])
    p0 = int(fa[0])
    active = np.zeros(n, bool)
    active[ga] = True
    active[gb] = True
    for v in np.nonzero(active)[0]:
        X[v] = initial_value(seed, int(v))
    stats[6], stats[7] = active.sum(), len(fe)
    eye = np.eye(3)

    def residual(X):
        v = X[gb] - X[ga]
        nrm = np.linalg.norm(v[:-1], axis=1)
        with np.errstate(all="ignore"):
            nh = v[:-1] / nrm[:, None]
        r = np.concatenate([nh - fu, (v[-1] - scale * fu[0])[None]])
        return r, nh, nrm

    def loss(r):
        d = np.linalg.norm(r, axis=1) * ISIG
        if not robust:
            return 0.5 * d * d
        return np.where(d <= HUBER_K, 0.5 * d * d, HUBER_K * d - 0.5 * HUBER_K * HUBER_K)

    def error(X):
        return np.sum(loss(residual(X)[0])) + 0.5 * np.dot(X[p0], X[p0]) * PRIOR_W

    err0 = err = error(X)
    lam = 1e-5
    max_iters = max_iterations if max_iterations > 0 else 100
    iters = trials = pcg_total = cap_hits = 0
    margins, per_solve = [], []
    if err > 0.0 and np.isfinite(err):
        while True:
            cur = err
            r, nh, nrm = residual(X)
            J = np.concatenate([(eye[None] - nh[:, :, None] * nh[:, None, :]) / nrm[:, None, None], eye[None]])
            ew = r * ISIG
            d = np.linalg.norm(ew, axis=1)
            sw = np.sqrt(np.where(d <= HUBER_K, 1.0, HUBER_K / np.where(d > 0, d, 1.0))) if robust else np.ones(len(d))
            A = J * (sw * ISIG)[:, None, None]
            b = -ew * sw[:, None]
            AtA = np.einsum("nkr,nkc->nrc", A, A)
            Atb = np.einsum("nkr,nk->nr", A, b)
            D = _scatter(n, ga, AtA) + _scatter(n, gb, AtA)
            g = _scatter(n, gb, Atb) - _scatter(n, ga, Atb)
            D[p0] += PRIOR_W * eye
            g[p0] += -X[p0] * PRIOR_W
            old_lin = 0.5 * (np.sum(b * b) + np.dot(X[p0], X[p0]) * PRIOR_W)

            def matvec(p, lam):
                p3 = p.reshape(n, 3)
                y = np.einsum("nrc,nc->nr", A, p3[gb] - p3[ga])
                Aty = np.einsum("nkr,nk->nr", A, y)
                q = _scatter(n, gb, Aty) - _scatter(n, ga, Aty) + lam * p3
                q[p0] += PRIOR_W * p3[p0]
                q[~active] = 0.0
                return q.reshape(-1)

            for _ in range(INNER_MAX):
                trials += 1
                m = {"trial": trials, "lambda": lam}
                Hd = D + lam * eye
                good = True
                Minv = np.zeros((n, 3, 3))
                try:
                    Minv[active] = np.linalg.inv(Hd[active])
                except np.linalg.LinAlgError:
                    good = False
                success = stop = False
                new_err = np.inf
                if good:
                    bvec = g.reshape(-1)
                    if solver == "exact":
                        H = np.zeros((3 * n, 3 * n))
                        ia = (3 * ga[:, None] + np.arange(3)[None]).astype(np.int64)
                        ib = (3 * gb[:, None] + np.arange(3)[None]).astype(np.int64)
                        for rows, cols, sg in ((ia, ia, 1.0), (ib, ib, 1.0), (ia, ib, -1.0), (ib, ia, -1.0)):
                            np.add.at(H, (rows[:, :, None], cols[:, None, :]), sg * AtA)
                        H[3 * p0:3 * p0 + 3, 3 * p0:3 * p0 + 3] += PRIOR_W * eye
                        av = np.repeat(active, 3)
                        x = np.zeros(3 * n)
                        x[av] = np.linalg.solve(H[np.ix_(av, av)] + lam * np.eye(int(av.sum())), bvec[av])
                    else:
                        def precond(rr_):
                            return np.einsum("vab,vb->va", Minv, rr_.reshape(n, 3)).reshape(-1)

                        x = np.zeros(3 * n)
                        rv_ = bvec.copy()
                        z = precond(rv_)
                        p = z.copy()
                        rz = np.dot(rv_, z)
                        rr = bb = np.dot(rv_, rv_)
                        k = 0
                        while np.isfinite(rr) and not np.sqrt(rr) <= pcg_rel_tol * np.sqrt(bb):
                            if k >= pcg_max_iter:
                                cap_hits += 1
                                break
                            q = matvec(p, lam)
                            with np.errstate(all="ignore"):
                                alpha = rz / np.dot(p, q)
                                x = x + alpha * p
                                rv_ = rv_ - alpha * q
                                z = precond(rv_)
                                rz_new = np.dot(rv_, z)
                                rr = np.dot(rv_, rv_)
                                p = z + (rz_new / rz) * p
                            rz = rz_new
                            k += 1
                        pcg_total += k
                        per_solve.append(k)
                    x3 = x.reshape(n, 3)
                    res = np.einsum("nrc,nc->nr", A, x3[gb] - x3[ga]) - b
                    new_lin = 0.5 * (np.sum(res * res) + np.sum((x3[p0] + X[p0]) ** 2) * PRIOR_W)
                    Xn = np.where(active[:, None], X + x3, X)
                    lin_change = old_lin - new_lin
                    m["lin_change"] = lin_change
                    if lin_change >= 0:
                        new_err = error(Xn)
                        cost_change = err - new_err
                        if lin_change > DBL_EPS * old_lin:
                            ratio = cost_change / lin_change
                            success = ratio > MIN_FIDELITY
                            m["fidelity"] = abs(ratio - MIN_FIDELITY)
                        else:
                            success = True
                        stop = abs(cost_change) < 1e-5 * err
                        m["stop"] = abs(abs(cost_change) / err - 1e-5)
                margins.append(m)
                if success:
                    X, err = Xn, new_err
                    lam /= 10.0
                    iters += 1
                    break
                if stop:
                    break
                lam *= 10.0
                if lam >= LAMBDA_UPPER:
                    break
            dec = cur - err
            margins[-1]["relative"] = abs(dec / cur - 1e-5)
            margins[-1]["absolute"] = abs(dec - 1e-5)
            if iters >= max_iters or dec / cur <= 1e-5 or dec <= 1e-5 or not np.isfinite(cur):
                break
    stats[:6] = err0, err, iters, trials, pcg_total, cap_hits
    return finish(0.0 if np.isfinite(err) else 2.0, margins, per_solve)


# ------------------------------------------------------------------ helpers shared by the tests
def sample_uniform_directions(n, seed):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def run_1dsfm(edges, i2Ui1, wRi, rot_valid=None, offsets=None, img=None, uv=None, intr=None, n_dir=2000, seed=0,
              robust=True, scale=1.0, solver="pcg", pcg_rel_tol=1e-10, reject_outliers=True):
    """The whole chain on the host; returns (Measurements, MfasRef or None, RecoverRef)."""
    ms = measurements(edges, i2Ui1, None, wRi, rot_valid, offsets, img, uv, intr)
    used = len(edges) + int(ms.counts[1])
    key, d, valid = ms.key[:used], ms.dir[:used], ms.valid[:used]
    n_img, n_land = len(np.asarray(wRi).reshape(-1, 3, 3)), len(ms.selected)
    mf = None
    inl = valid
    if reject_outliers:
        mf = mfas(key, d, valid, n_img + n_land, sample_uniform_directions(n_dir, seed))
        inl = mf.inlier
    rec = recover(key, d, inl, n_img, n_land, rot_valid, robust, scale, seed, solver=solver, pcg_rel_tol=pcg_rel_tol)
    return ms, mf, rec


def align_sim3(target, est):
    """est (N, 3) mapped onto target by the least-squares similarity (Umeyama); coincident points: translation only."""
    target, est = np.asarray(target, np.float64), np.asarray(est, np.float64)
    mt, me = target.mean(0), est.mean(0)
    a, b = target - mt, est - me
    var = np.sum(b * b)
    if var < 1e-24:
        return est + (mt - me)
    U, S, Vt = np.linalg.svd(a.T @ b)
    sgn = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        sgn[2] = -1.0
    R = U @ np.diag(sgn) @ Vt
    s = np.sum(S * sgn) / var
    return s * (b @ R.T) + mt


def seeded_scene(n_cam, seed, n_pts=0, edge_frac=0.5, outlier_frac=0.1, noise=0.002):
    """Cameras on a perturbed ring with identity-free random rotations, a random share of the pairs as edges with noisy
    directions and planted outliers, and optional tracks of n_pts points (float64 uv, f = 500). Dict of arrays."""
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(n_cam) / n_cam
    t = np.stack([5 * np.cos(ang), 5 * np.sin(ang), np.zeros(n_cam)], 1) + rng.normal(0, 0.5, (n_cam, 3))
    R = np.zeros((n_cam, 3, 3))
    for i in range(n_cam):
        z = -t[i] / np.linalg.norm(t[i]) + rng.normal(0, 0.05, 3)
        z /= np.linalg.norm(z)
        x = np.cross(np.array([0.0, 0.0, 1.0]), z)
        x /= np.linalg.norm(x)
        R[i] = np.stack([x, np.cross(z, x), z], 1)
    pairs = np.array([(i, j) for i in range(n_cam) for j in range(i + 1, n_cam) if rng.random() < edge_frac or j == i + 1],
                     np.int32)
    u = np.einsum("nji,nj->ni", R[pairs[:, 1]], t[pairs[:, 0]] - t[pairs[:, 1]])  # i2Ui1 = wRi2^T (t1 - t2)
    u = u / np.linalg.norm(u, axis=1, keepdims=True) + rng.normal(0, noise, u.shape)
    bad = rng.random(len(pairs)) < outlier_frac
    bad[:3] = False
    rnd = rng.normal(size=u.shape)
    u[bad] = rnd[bad]
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    out = dict(edges=pairs, i2Ui1=u, wRi=R, wti=t, outlier=bad)
    if n_pts:
        pts = rng.uniform(-1.0, 1.0, (n_pts, 3))
        lens = rng.integers(2, 7, n_pts)
        offsets = np.zeros(n_pts + 1, np.int32)
        np.cumsum(lens, out=offsets[1:])
        img = np.concatenate([np.sort(rng.choice(n_cam, k, replace=False)) for k in lens]).astype(np.int32)
        trk = np.repeat(np.arange(n_pts), lens)
        pc = np.einsum("nji,nj->ni", R[img], pts[trk] - t[img])
        K = np.tile(np.array([500.0, 320.0, 240.0]), (n_cam, 1))
        uv = K[img, 1:3] + K[img, :1] * pc[:, :2] / pc[:, 2:3] + rng.normal(0, 0.3, (len(img), 2))
        out.update(offsets=offsets, img=img, uv=uv, intr=K)
    return out
