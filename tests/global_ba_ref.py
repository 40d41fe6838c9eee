"""Vectorised numpy restatement of gtsfm_global_ba (include/gtsfm_hip.h): the same problem, factors, LM schedule and
point elimination, with two solvers of the reduced camera system: "pcg", block-Jacobi preconditioned conjugate gradients
with the kernel's stopping rule, and "exact", a dense Cholesky of the formed Schur complement. Sums are np.bincount /
einsum, so results agree with the kernel to rounding, not bit for bit. Also returns, per LM trial, the margins of its
decisions, so a test can tell a seed on which a count could legitimately differ."""
from typing import NamedTuple, Optional

import numpy as np

HUBER_K = 1.345
MIN_FIDELITY = 1e-3
LAMBDA_UPPER = 1e5
DBL_EPS = 2.220446049250313e-16
POINT_PRIOR_W = 100.0
INNER_MAX = 64


def skew(w):
    w = np.asarray(w, np.float64)
    S = np.zeros(w.shape[:-1] + (3, 3))
    S[..., 0, 1], S[..., 0, 2] = -w[..., 2], w[..., 1]
    S[..., 1, 0], S[..., 1, 2] = w[..., 2], -w[..., 0]
    S[..., 2, 0], S[..., 2, 1] = -w[..., 1], w[..., 0]
    return S


def pose_retract(R, t, xi):
    """Pose3 retraction (full exponential map, rotation first) of (N, 3, 3), (N, 3) by xi (N, 6)."""
    w, v = xi[..., :3], xi[..., 3:]
    th2 = np.sum(w * w, -1)
    small = th2 < 1e-16
    th = np.sqrt(np.where(small, 1.0, th2))
    a = np.where(small, 1.0 - th2 / 6.0, np.sin(th) / th)
    b = np.where(small, 0.5 - th2 / 24.0, (1.0 - np.cos(th)) / np.where(small, 1.0, th2))
    c = np.where(small, 1.0 / 6.0 - th2 / 120.0, (th - np.sin(th)) / np.where(small, 1.0, th2 * th))
    W = skew(w)
    W2 = W @ W
    dR = np.eye(3) + a[..., None, None] * W + b[..., None, None] * W2
    V = np.eye(3) + b[..., None, None] * W + c[..., None, None] * W2
    tv = np.einsum("...ij,...j->...i", V, v)
    return R @ dR, t + np.einsum("...ij,...j->...i", R, tv)


def so3_log(R):
    c = min(1.0, max(-1.0, 0.5 * (np.trace(R) - 1.0)))
    th = np.arccos(c)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if th < 1e-8:
        return 0.5 * v
    if np.pi - th < 1e-6:
        i = int(np.argmax(np.diag(R)))
        ax = np.zeros(3)
        ax[i] = np.sqrt(max(0.0, (R[i, i] + 1.0) * 0.5))
        for j in range(3):
            if j != i:
                ax[j] = (R[i, j] + R[j, i]) / (4.0 * ax[i])
        return th * ax / np.linalg.norm(ax)
    return th / (2.0 * np.sin(th)) * v


def pose_local(R0, t0, R, t):
    """Logmap(X0^-1 X), rotation first: the residual of the pose prior at X0."""
    Rr = R0.T @ R
    tr = R0.T @ (t - t0)
    w = so3_log(Rr)
    th = np.linalg.norm(w)
    if th < 1e-10:
        return np.concatenate([w, tr])
    W = skew(w / th)
    Wt = W @ tr
    WWt = W @ Wt
    return np.concatenate([w, tr - 0.5 * th * Wt + (1.0 - th / (2.0 * np.tan(0.5 * th))) * WWt])


def project(R, t, K, p):
    """Camera-frame points, pixel positions and the in-front mask of points p (N, 3) in cameras (N, ...)."""
    pc = np.einsum("nji,nj->ni", R, p - t)
    ok = pc[:, 2] > 0.0
    z = np.where(ok, pc[:, 2], 1.0)
    uv = K[:, 1:3] + K[:, :1] * (pc[:, :2] / z[:, None])
    return pc, uv, ok


def reproj_jacobians(R, t, K, pc):
    """d uv / d point (N, 2, 3) and d uv / d pose (N, 2, 6; body frame, rotation first) at camera-frame points pc."""
    iz = 1.0 / pc[:, 2]
    xn, yn, f = pc[:, 0] * iz, pc[:, 1] * iz, K[:, 0]
    D = np.zeros((len(pc), 2, 3))
    D[:, 0, 0] = f * iz
    D[:, 0, 2] = -f * xn * iz
    D[:, 1, 1] = f * iz
    D[:, 1, 2] = -f * yn * iz
    Jp = np.einsum("nrk,njk->nrj", D, R)
    Jx = np.concatenate([np.cross(D, pc[:, None, :]), -D], axis=2)
    return Jp, Jx


class GlobalBaRef(NamedTuple):
    wRc: np.ndarray
    wtc: np.ndarray
    point: np.ndarray
    track_keep: np.ndarray
    cam_keep: np.ndarray
    stats: np.ndarray  # the kernel's d_stats[10]
    margins: list  # per LM trial: dict of the decision margins
    min_margin: float
    pcg_iters_per_solve: list


def _scatter(n, idx, vals):
    """out[i] = sum of vals[k] over idx[k] == i, in ascending k (np.add.at's result, by one bincount per column)."""
    v = vals.reshape(len(idx), -1)
    out = np.stack([np.bincount(idx, v[:, j], minlength=n) for j in range(v.shape[1])], 1)
    return out.reshape((n,) + vals.shape[1:])


def _inv3(A):
    """The kernel's adjugate inverse; ok False where the determinant is zero or not finite."""
    c00 = A[:, 1, 1] * A[:, 2, 2] - A[:, 1, 2] * A[:, 2, 1]
    c01 = A[:, 1, 2] * A[:, 2, 0] - A[:, 1, 0] * A[:, 2, 2]
    c02 = A[:, 1, 0] * A[:, 2, 1] - A[:, 1, 1] * A[:, 2, 0]
    det = A[:, 0, 0] * c00 + A[:, 0, 1] * c01 + A[:, 0, 2] * c02
    ok = (np.abs(det) > 0.0) & np.isfinite(det)
    idet = 1.0 / np.where(ok, det, 1.0)
    inv = np.empty_like(A)
    inv[:, 0, 0] = c00
    inv[:, 0, 1] = A[:, 0, 2] * A[:, 2, 1] - A[:, 0, 1] * A[:, 2, 2]
    inv[:, 0, 2] = A[:, 0, 1] * A[:, 1, 2] - A[:, 0, 2] * A[:, 1, 1]
    inv[:, 1, 0] = c01
    inv[:, 1, 1] = A[:, 0, 0] * A[:, 2, 2] - A[:, 0, 2] * A[:, 2, 0]
    inv[:, 1, 2] = A[:, 0, 2] * A[:, 1, 0] - A[:, 0, 0] * A[:, 1, 2]
    inv[:, 2, 0] = c02
    inv[:, 2, 1] = A[:, 0, 1] * A[:, 2, 0] - A[:, 0, 0] * A[:, 2, 1]
    inv[:, 2, 2] = A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]
    return inv * idet[:, None, None], bool(ok.all())


def global_ba_ref(offsets, img, uv, point, track_valid, meas_valid, wRc, wtc, intr, cam_valid, robust=False,
                  measurement_sigma=1.0, cam_pose3_prior_sigma=0.1, max_iterations=0, pcg_rel_tol=1e-10,
                  pcg_max_iter=2000, reproj_error_thresh=np.inf, solver="pcg") -> GlobalBaRef:
    offsets = np.asarray(offsets, np.int64)
    img = np.asarray(img, np.int64)
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    P_in = np.asarray(point, np.float64).reshape(-1, 3)
    R_in = np.asarray(wRc, np.float64).reshape(-1, 3, 3)
    t_in = np.asarray(wtc, np.float64).reshape(-1, 3)
    K = np.asarray(intr, np.float64).reshape(-1, 3)
    T, M, C = len(offsets) - 1, len(img), len(K)
    tvalid = np.ones(T, bool) if track_valid is None else np.asarray(track_valid).astype(bool)[:T]
    mflag = np.ones(M, bool) if meas_valid is None else np.asarray(meas_valid).astype(bool)
    cvalid = np.ones(C, bool) if cam_valid is None else np.asarray(cam_valid).astype(bool)
    isig = 1.0 / measurement_sigma
    prior_w = 1.0 / (cam_pose3_prior_sigma * cam_pose3_prior_sigma)
    max_iters = max_iterations if max_iterations > 0 else 100

    mtrk = np.repeat(np.arange(T), np.diff(offsets))
    in_range = (img >= 0) & (img < C)
    camok = in_range & cvalid[np.clip(img, 0, max(C - 1, 0))] if C else np.zeros(M, bool)
    usable = mflag & camok
    cnt = np.bincount(mtrk[usable], minlength=T)
    part = tvalid & (cnt >= 2)
    fac = usable & part[mtrk] if T else np.zeros(M, bool)
    fm = np.nonzero(fac)[0]
    ft, fc = mtrk[fm], img[fm]
    modelled = np.zeros(C, bool)
    modelled[fc] = True
    if not part.any() or not modelled.any():
        stats = np.zeros(10)
        stats[9] = 1.0
        return GlobalBaRef(R_in.copy(), t_in.copy(), P_in.copy(), np.zeros(T, np.uint8), np.zeros(C, np.uint8), stats,
                           [], np.inf, [])
    c0, t0 = int(np.nonzero(modelled)[0][0]), int(np.nonzero(part)[0][0])
    fuv, fK = uv[fm], K[fc]

    def loss(d):
        if not robust:
            return 0.5 * d * d
        return np.where(d <= HUBER_K, 0.5 * d * d, HUBER_K * d - 0.5 * HUBER_K * HUBER_K)

    def error(R, t, P):
        _, pr, ok = project(R[fc], t[fc], fK, P[ft])
        d = np.linalg.norm(pr - fuv, axis=1) * isig
        e = np.sum(np.bincount(ft, np.where(ok, loss(d), 0.0), minlength=T))
        xi = pose_local(R_in[c0], t_in[c0], R[c0], t[c0])
        dp = P[t0] - P_in[t0]
        return e + 0.5 * np.dot(xi, xi) * prior_w + 0.5 * np.dot(dp, dp) * POINT_PRIOR_W

    def linearize(R, t, P):
        pc, pr, ok = project(R[fc], t[fc], fK, P[ft])
        pcs = np.where(ok[:, None], pc, np.array([0.0, 0.0, 1.0]))
        Jp, Jx = reproj_jacobians(R[fc], t[fc], fK, pcs)
        e = (pr - fuv) * isig
        d = np.linalg.norm(e, axis=1)
        sw = np.sqrt(np.where(d <= HUBER_K, 1.0, HUBER_K / np.where(d > 0, d, 1.0))) if robust else np.ones(len(d))
        s = np.where(ok, sw * isig, 0.0)
        return Jx * s[:, None, None], Jp * s[:, None, None], -e * np.where(ok, sw, 0.0)[:, None]

    R, t, P = R_in.copy(), t_in.copy(), P_in.copy()
    err0 = err = error(R, t, P)
    lam = 1e-5
    iters = trials = pcg_total = cap_hits = 0
    margins, per_solve = [], []
    eye6 = np.eye(6)
    if err > 0.0:
        while True:
            cur = err
            Jx, Jp, b = linearize(R, t, P)
            xi0 = pose_local(R_in[c0], t_in[c0], R[c0], t[c0])
            dp0 = P[t0] - P_in[t0]
            Hpp = _scatter(T, ft, np.einsum("nrk,nrl->nkl", Jp, Jp))
            rp = _scatter(T, ft, np.einsum("nrk,nr->nk", Jp, b))
            Hpp[t0] += POINT_PRIOR_W * np.eye(3)
            rp[t0] += -dp0 * POINT_PRIOR_W
            Hcc = _scatter(C, fc, np.einsum("nra,nrb->nab", Jx, Jx))
            gc = _scatter(C, fc, np.einsum("nra,nr->na", Jx, b))
            Hcc[c0] += prior_w * eye6
            gc[c0] += -xi0 * prior_w
            W = np.einsum("nra,nrk->nak", Jx, Jp)
            old_lin = 0.5 * (np.sum(b * b) + np.dot(dp0, dp0) * POINT_PRIOR_W + np.dot(xi0, xi0) * prior_w)
            for _ in range(INNER_MAX):
                trials += 1
                Hd = Hpp + lam * np.eye(3)
                Hd[~part] = np.eye(3)
                Minv, ok3 = _inv3(Hd)
                Minv[~part] = 0.0
                WM = np.einsum("nak,nkl->nal", W, Minv[ft])
                Scc = Hcc + lam * eye6 - _scatter(C, fc, np.einsum("nal,nbl->nab", WM, W))
                bred = gc - _scatter(C, fc, np.einsum("nal,nl->na", WM, rp[ft]))
                bred[~modelled] = 0.0
                good = ok3
                Pinv = np.zeros((C, 6, 6))
                if good:
                    try:
                        np.linalg.cholesky(Scc[modelled])
                        Pinv[modelled] = np.linalg.inv(Scc[modelled])
                    except np.linalg.LinAlgError:
                        good = False
                success = stop = False
                new_err = np.inf
                m = {"trial": trials, "lambda": lam}
                if good:
                    Hl = Hcc + lam * eye6

                    def matvec(p):
                        pc6 = p.reshape(C, 6)
                        u = np.einsum("nra,na->nr", Jx, pc6[fc])
                        s = _scatter(T, ft, np.einsum("nrk,nr->nk", Jp, u))
                        y = np.einsum("tij,tj->ti", Minv, s)
                        v = np.einsum("nrk,nk->nr", Jp, y[ft])
                        out = np.einsum("cab,cb->ca", Hl, pc6) - _scatter(C, fc, np.einsum("nra,nr->na", Jx, v))
                        out[~modelled] = 0.0
                        return out.reshape(-1)

                    bvec = bred.reshape(-1)
                    if solver == "exact":
                        E = np.zeros((3 * T, 6 * C))
                        rows = (3 * ft[:, None, None] + np.arange(3)[None, :, None])
                        cols = (6 * fc[:, None, None] + np.arange(6)[None, None, :])
                        E[rows, cols] = np.transpose(W, (0, 2, 1))
                        ME = np.einsum("tij,tjc->tic", Minv, E.reshape(T, 3, 6 * C)).reshape(3 * T, 6 * C)
                        S = -E.T @ ME
                        for c in range(C):
                            S[6 * c:6 * c + 6, 6 * c:6 * c + 6] += Hl[c]
                        try:
                            Lc = np.linalg.cholesky(S)
                            x = np.linalg.solve(Lc.T, np.linalg.solve(Lc, bvec))
                        except np.linalg.LinAlgError:
                            good = False
                        k = 0
                    else:
                        def precond(r):
                            return np.einsum("cab,cb->ca", Pinv, r.reshape(C, 6)).reshape(-1)

                        x = np.zeros(6 * C)
                        r = bvec.copy()
                        z = precond(r)
                        p = z.copy()
                        rz = np.dot(r, z)
                        rr = bb = np.dot(r, r)
                        k = 0
                        while np.isfinite(rr) and not np.sqrt(rr) <= pcg_rel_tol * np.sqrt(bb):
                            if k >= pcg_max_iter:
                                cap_hits += 1
                                break
                            q = matvec(p)
                            with np.errstate(all="ignore"):
                                alpha = rz / np.dot(p, q)
                                x = x + alpha * p
                                r = r - alpha * q
                                z = precond(r)
                                rz_new = np.dot(r, z)
                                rr = np.dot(r, r)
                                p = z + (rz_new / rz) * p
                            rz = rz_new
                            k += 1
                        pcg_total += k
                        per_solve.append(k)
                if good:
                    dc = x.reshape(C, 6)
                    u = np.einsum("nra,na->nr", Jx, dc[fc])
                    s = _scatter(T, ft, np.einsum("nrk,nr->nk", Jp, u))
                    dp = np.einsum("tij,tj->ti", Minv, rp - s)
                    res = u + np.einsum("nrk,nk->nr", Jp, dp[ft]) - b
                    new_lin = 0.5 * (np.sum(res * res) + np.sum((dp[t0] + dp0) ** 2) * POINT_PRIOR_W +
                                     np.sum((dc[c0] + xi0) ** 2) * prior_w)
                    Rn, tn = R.copy(), t.copy()
                    Rn[modelled], tn[modelled] = pose_retract(R[modelled], t[modelled], dc[modelled])
                    Pn = P.copy()
                    Pn[part] = P[part] + dp[part]
                    lin_change = old_lin - new_lin
                    m["lin_change"] = lin_change
                    if lin_change >= 0:
                        new_err = error(Rn, tn, Pn)
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
                    R, t, P, err = Rn, tn, Pn, new_err
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

    # filter_landmarks
    keep = part.copy()
    if np.isfinite(reproj_error_thresh):
        mi = np.nonzero(mflag & part[mtrk])[0]
        ci = np.clip(img[mi], 0, C - 1)
        pc, pr, ok = project(R[ci], t[ci], K[ci], P[mtrk[mi]])
        e = np.linalg.norm(pr - uv[mi], axis=1)
        bad = ~(camok[mi] & ok & (e < reproj_error_thresh))
        keep[np.unique(mtrk[mi][bad])] = False
    cam_keep = np.zeros(C, np.uint8)
    cam_keep[img[usable & keep[mtrk]]] = 1
    stats = np.array([err0, err, iters, trials, pcg_total, cap_hits, modelled.sum(), part.sum(), keep.sum(), 0.0])
    keys = ("fidelity", "stop", "relative", "absolute")
    min_margin = min([v for m in margins for k, v in m.items() if k in keys], default=np.inf)
    return GlobalBaRef(R, t, P, keep.astype(np.uint8), cam_keep, stats, margins, float(min_margin), per_solve)


# ------------------------------------------------------------------ seeded synthetic scenes shared by the tests
def ring_scene(n_cam, n_pts, min_len, max_len, seed, noise_px=0.5, outlier_frac=0.05, outlier_px=30.0,
               pose_noise=(0.01, 0.02), point_noise=0.02):
    """Cameras on a ring of radius 4 looking at a unit cube of points, f = 1000; each point is seen by min_len ..
    max_len cameras (ascending camera index, as the track CSR has them). Returns a dict of arrays: the CSR, noisy
    measurements (float64), perturbed initial cameras and points, and the ground truth."""
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(n_cam) / max(n_cam, 3) * (1.0 if n_cam > 3 else 0.25)
    ctr = np.stack([4 * np.cos(ang), 4 * np.sin(ang), 0.3 * np.sin(3 * ang)], 1)
    R = np.zeros((n_cam, 3, 3))
    for i in range(n_cam):
        zax = -ctr[i] / np.linalg.norm(ctr[i])
        xax = np.cross(np.array([0.0, 0.0, 1.0]), zax)
        xax /= np.linalg.norm(xax)
        R[i] = np.stack([xax, np.cross(zax, xax), zax], 1)
    K = np.tile(np.array([1000.0, 500.0, 400.0]), (n_cam, 1))
    pts = rng.uniform(-0.5, 0.5, (n_pts, 3))
    lens = rng.integers(min_len, max_len + 1, n_pts)
    offsets = np.zeros(n_pts + 1, np.int32)
    np.cumsum(lens, out=offsets[1:])
    img = np.concatenate([np.sort(rng.choice(n_cam, n, replace=False)) for n in lens]).astype(np.int32)
    trk = np.repeat(np.arange(n_pts), lens)
    _, uv, ok = project(R[img], ctr[img], K[img], pts[trk])
    assert ok.all()
    uv = uv + rng.normal(0, noise_px, uv.shape)
    out = rng.random(len(img)) < outlier_frac
    dirs = rng.normal(size=(len(img), 2))
    uv[out] += outlier_px * dirs[out] / np.linalg.norm(dirs[out], axis=1, keepdims=True)
    R0, t0 = pose_retract(R, ctr, np.concatenate([rng.normal(0, pose_noise[0], (n_cam, 3)),
                                                  rng.normal(0, pose_noise[1], (n_cam, 3))], 1))
    return dict(offsets=offsets, img=img, uv=uv, point=pts + rng.normal(0, point_noise, pts.shape), wRc=R0, wtc=t0,
                intr=K, gt_wRc=R, gt_wtc=ctr, gt_point=pts, track_valid=np.ones(n_pts, np.uint8),
                meas_valid=np.ones(len(img), np.uint8), cam_valid=np.ones(n_cam, np.uint8))


def call_args(s):
    """The positional arguments of global_ba_ref from a scene dict."""
    return (s["offsets"], s["img"], s["uv"], s["point"], s["track_valid"], s["meas_valid"], s["wRc"], s["wtc"],
            s["intr"], s["cam_valid"])


def scene_small(seed=1):
    return ring_scene(5, 40, 2, 5, seed)


def scene_medium(seed=2):
    """12 cameras x 300 points plus the edge entries: camera 12 invalid (seen by two tracks), camera 13 valid and
    unseen, track 7 invalid, one measurement switched off, and one landmark behind both of its cameras."""
    s = ring_scene(12, 300, 2, 7, seed)
    n_cam = 14
    for k, fill in (("wRc", np.eye(3)), ("wtc", np.array([9.0, 9.0, 9.0])), ("intr", np.array([1000.0, 500.0, 400.0]))):
        s[k] = np.concatenate([s[k], np.tile(fill, (2,) + (1,) * fill.ndim)])
        if "gt_" + k in s:
            s["gt_" + k] = np.concatenate([s["gt_" + k], np.tile(fill, (2,) + (1,) * fill.ndim)])
    s["cam_valid"] = np.ones(n_cam, np.uint8)
    s["cam_valid"][12] = 0
    # tracks 3 and 5 get one extra measurement each on the invalid camera 12 (appended last: ascending image order)
    off, img, uv, mv = s["offsets"].astype(np.int64), s["img"], s["uv"], s["meas_valid"]
    for t in (5, 3):
        e = off[t + 1]
        img = np.insert(img, e, 12)
        uv = np.insert(uv, e, np.array([500.0, 400.0]), axis=0)
        mv = np.insert(mv, e, 1)
        off[t + 1:] += 1
    s["offsets"], s["img"], s["uv"], s["meas_valid"] = off.astype(np.int32), img.astype(np.int32), uv, mv
    s["track_valid"][7] = 0
    long_t = int(np.nonzero(np.diff(off) >= 4)[0][0])
    s["meas_valid"][off[long_t] + 1] = 0
    # one two-view track whose landmark starts behind both of its cameras: its factors contribute nothing (z <= 0), so
    # it stays there and the filter must drop it for cheirality
    lens = np.diff(off)
    behind = next(j for j in range(8, len(lens)) if lens[j] == 2 and j != long_t and
                  np.dot(s["gt_wtc"][img[off[j]]], s["gt_wtc"][img[off[j] + 1]]) > -0.3 * 16)
    s["point"][behind] = 2.0 * (s["gt_wtc"][img[off[behind]]] + s["gt_wtc"][img[off[behind] + 1]])
    s["edge"] = dict(invalid_cam=12, unseen_cam=13, invalid_track=7, off_meas=int(off[long_t] + 1),
                     behind_track=int(behind), invalid_cam_tracks=(3, 5))
    return s


def scene_dense(seed=3):
    return ring_scene(3, 400, 3, 3, seed)


def rel_rot_deg(Ra, Rb):
    D = Ra.T @ Rb  # atan2 of the skew part: accurate near zero, where arccos of the trace resolves only 1e-6 degrees
    v = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.degrees(np.arctan2(np.linalg.norm(v), 0.5 * (np.trace(D) - 1.0))))


def pose_diff(R1, t1, R2, t2, cams):
    """Largest rotation difference (degrees) and relative translation difference over the listed cameras."""
    rot = max(rel_rot_deg(R1[c], R2[c]) for c in cams)
    scale = max(np.linalg.norm(t2[cams], axis=1).max(), 1e-300)
    return rot, float(np.abs(t1[cams] - t2[cams]).max() / scale)
