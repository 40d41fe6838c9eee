"""Vectorised numpy restatement of gtsfm_global_ba_calib (include/gtsfm_hip.h): global_ba_ref's problem, LM schedule,
point elimination and PCG, with GTSAM 4.2's Cal3Bundler calibration (f, k1, k2) refined, one variable per modelled camera
or one shared by all (gtsfm/bundle/bundle_adjustment.py:103-131, :180-208), each under an isotropic prior at its initial
value. GTSAM is not installed, so this restatement is the oracle, as global_ba_ref is for the fixed-calibration call.

The unknown of the reduced system is (C poses of 6, NK calibrations of 3), NK = C or 1; camera c uses calibration
kmap[c] = c or 0. Per track sums are np.bincount in CSR order, as in global_ba_ref. Per camera sums, and the sum of the
cameras' border slots, are taken in the kernel's fixed order (reduce.hpp: a lane's strided partial over the camera-major
index, a 64-lane butterfly, the waves in order; block_order_sum below). That matters here where it did not for the
fixed-calibration call: with k2 weakly observable the reduced system is ill-conditioned, a PCG solve of 21 unknowns takes
50 to 60 iterations, and how many it takes depends on the rounding error of the product; a sequential sum over a camera's
100 to 400 measurements carries more of it than the kernel's tree and needs 2 to 4 % more iterations (843 against 812 on
the dense / shared scene), while the solution is the same to 1e-10. reverse_cam_order=True feeds the same sums the
camera-major index backwards, so that every lane and every pair of the tree holds other terms, which is how the tests
measure what a different summation order may change."""
from typing import NamedTuple

import numpy as np

import global_ba_ref as base
from global_ba_ref import (DBL_EPS, HUBER_K, INNER_MAX, LAMBDA_UPPER, MIN_FIDELITY, POINT_PRIOR_W, _inv3, pose_local,
                           pose_retract)

TRUE_K1, TRUE_K2 = -0.3, 0.05
F_OFF = 1.03


def project_k(R, t, K, p):
    """Camera-frame points, Cal3Bundler pixel positions and the in-front mask; K (N, 5) = (f, k1, k2, u0, v0)."""
    pc = np.einsum("nji,nj->ni", R, p - t)
    ok = pc[:, 2] > 0.0
    z = np.where(ok, pc[:, 2], 1.0)
    xy = pc[:, :2] / z[:, None]
    r2 = np.sum(xy * xy, 1)
    g = 1.0 + (K[:, 1] + K[:, 2] * r2) * r2
    return pc, (K[:, 0] * g)[:, None] * xy + K[:, 3:5], ok


def reproj_jacobians_k(R, t, K, pc):
    """d uv / d point (N, 2, 3), d uv / d pose (N, 2, 6; body frame, rotation first) and d uv / d (f, k1, k2)
    (N, 2, 3) at camera-frame points pc in front of the camera."""
    iz = 1.0 / pc[:, 2]
    xy = pc[:, :2] * iz[:, None]
    f, k1, k2 = K[:, 0], K[:, 1], K[:, 2]
    r2 = np.sum(xy * xy, 1)
    g = 1.0 + (k1 + k2 * r2) * r2
    A = f[:, None, None] * (g[:, None, None] * np.eye(2) +
                            (2.0 * (k1 + 2.0 * k2 * r2))[:, None, None] * xy[:, :, None] * xy[:, None, :])
    Dn = np.zeros((len(pc), 2, 3))
    Dn[:, 0, 0] = iz
    Dn[:, 1, 1] = iz
    Dn[:, :, 2] = -xy * iz[:, None]
    D = A @ Dn
    Jp = np.einsum("nrk,njk->nrj", D, R)
    Jx = np.concatenate([np.cross(D, pc[:, None, :]), -D], axis=2)
    Jk = np.stack([xy * g[:, None], xy * (f * r2)[:, None], xy * (f * r2 * r2)[:, None]], 2)
    return Jp, Jx, Jk


CAM_LANES, VEC_LANES = 256, 1024  # lanes of a camera workgroup and of the single-workgroup vector kernels


def block_order_sum(n, idx, vals, lanes):
    """out[i] = sum of vals[k] over idx[k] == i in reduce.hpp's order for a workgroup of `lanes` lanes walking the
    entries of bin i in ascending k: lane l adds entries l, l + lanes, ... in turn; each wave of 64 lanes is summed by the
    xor butterfly 32, 16, ..., 1; the waves are added in order."""
    v = vals.reshape(len(idx), -1)
    order = np.argsort(idx, kind="stable")
    idx_s, v_s = idx[order], v[order]
    cnt = np.bincount(idx_s, minlength=n)
    pos = np.arange(len(idx_s)) - (np.cumsum(cnt) - cnt)[idx_s]
    rounds = max(1, -(-int(cnt.max(initial=0)) // lanes))
    buf = np.zeros((n, rounds, lanes, v.shape[1]))
    buf[idx_s, pos // lanes, pos % lanes] = v_s
    part = np.zeros((n, lanes, v.shape[1]))
    for k in range(rounds):
        part = part + buf[:, k]
    w = part.reshape(n, lanes // 64, 64, -1)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, :, lane ^ o]
    out = w[:, 0, 0]
    for k in range(1, lanes // 64):
        out = out + w[:, k, 0]
    return out.reshape((n,) + vals.shape[1:])


class GlobalBaCalibRef(NamedTuple):
    wRc: np.ndarray
    wtc: np.ndarray
    point: np.ndarray
    track_keep: np.ndarray
    cam_keep: np.ndarray
    stats: np.ndarray  # the kernel's d_stats[12]
    calib: np.ndarray  # (C, 5)
    margins: list  # per LM trial: dict of the decision margins
    min_margin: float
    pcg_iters_per_solve: list


def global_ba_calib_ref(offsets, img, uv, point, track_valid, meas_valid, wRc, wtc, calib, cam_valid, robust=False,
                        measurement_sigma=1.0, cam_pose3_prior_sigma=0.1, shared_calib=False,
                        calibration_prior_sigma=1e-5, max_iterations=0, pcg_rel_tol=1e-10, pcg_max_iter=2000,
                        reproj_error_thresh=np.inf, reverse_cam_order=False) -> GlobalBaCalibRef:
    offsets = np.asarray(offsets, np.int64)
    img = np.asarray(img, np.int64)
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    P_in = np.asarray(point, np.float64).reshape(-1, 3)
    R_in = np.asarray(wRc, np.float64).reshape(-1, 3, 3)
    t_in = np.asarray(wtc, np.float64).reshape(-1, 3)
    K_in = np.asarray(calib, np.float64).reshape(-1, 5)
    T, M, C = len(offsets) - 1, len(img), len(K_in)
    tvalid = np.ones(T, bool) if track_valid is None else np.asarray(track_valid).astype(bool)[:T]
    mflag = np.ones(M, bool) if meas_valid is None else np.asarray(meas_valid).astype(bool)
    cvalid = np.ones(C, bool) if cam_valid is None else np.asarray(cam_valid).astype(bool)
    isig = 1.0 / measurement_sigma
    prior_w = 1.0 / (cam_pose3_prior_sigma * cam_pose3_prior_sigma)
    kprior_w = 1.0 / (calibration_prior_sigma * calibration_prior_sigma)
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
        stats = np.zeros(12)
        stats[9] = 1.0
        return GlobalBaCalibRef(R_in.copy(), t_in.copy(), P_in.copy(), np.zeros(T, np.uint8), np.zeros(C, np.uint8),
                                stats, K_in.copy(), [], np.inf, [])
    c0, t0 = int(np.nonzero(modelled)[0][0]), int(np.nonzero(part)[0][0])
    fuv = uv[fm]
    mod_idx = np.nonzero(modelled)[0]
    # calibration variables: K0 (NK, 5) their initial values (and prior centres), kmap the variable of each camera
    if shared_calib:
        K0, kmap = K_in[c0:c0 + 1].copy(), np.zeros(C, np.int64)
    else:
        K0, kmap = K_in.copy(), np.arange(C)
    NK = len(K0)
    kvar = np.zeros(NK, bool)  # variables that exist: those of modelled cameras
    kvar[kmap[mod_idx]] = True

    def cam_scatter(vals):
        """Sum over the factor measurements of each camera, a camera workgroup's order over the camera-major index
        (measurement order within a camera) or over that index reversed."""
        if reverse_cam_order:
            return block_order_sum(C, fc[::-1], vals[::-1], CAM_LANES)
        return block_order_sum(C, fc, vals, CAM_LANES)

    def var_scatter(vals):
        """Sum over the modelled cameras of each calibration variable: per camera mode one term each; shared mode the
        single workgroup's order over the cameras' slots, or over the slots reversed."""
        v = np.where(modelled.reshape((C,) + (1,) * (vals.ndim - 1)), vals, 0.0)  # lane c holds camera c's slot
        if not shared_calib:
            return v
        if reverse_cam_order:
            v = v[::-1]
        return block_order_sum(1, np.zeros(C, np.int64), v, VEC_LANES)

    def loss(d):
        if not robust:
            return 0.5 * d * d
        return np.where(d <= HUBER_K, 0.5 * d * d, HUBER_K * d - 0.5 * HUBER_K * HUBER_K)

    def error(R, t, Kv, P):
        _, pr, ok = project_k(R[fc], t[fc], Kv[kmap[fc]], P[ft])
        d = np.linalg.norm(pr - fuv, axis=1) * isig
        e = np.sum(np.bincount(ft, np.where(ok, loss(d), 0.0), minlength=T))
        xi = pose_local(R_in[c0], t_in[c0], R[c0], t[c0])
        dp = P[t0] - P_in[t0]
        dk = (Kv - K0)[kvar, :3]
        return (e + 0.5 * np.dot(xi, xi) * prior_w + 0.5 * np.dot(dp, dp) * POINT_PRIOR_W +
                0.5 * np.sum(dk * dk) * kprior_w)

    def linearize(R, t, Kv, P):
        Kf = Kv[kmap[fc]]
        pc, pr, ok = project_k(R[fc], t[fc], Kf, P[ft])
        pcs = np.where(ok[:, None], pc, np.array([0.0, 0.0, 1.0]))
        Jp, Jx, Jk = reproj_jacobians_k(R[fc], t[fc], Kf, pcs)
        e = (pr - fuv) * isig
        d = np.linalg.norm(e, axis=1)
        sw = np.sqrt(np.where(d <= HUBER_K, 1.0, HUBER_K / np.where(d > 0, d, 1.0))) if robust else np.ones(len(d))
        s = np.where(ok, sw * isig, 0.0)[:, None, None]
        return np.concatenate([Jx, Jk], 2) * s, Jp * s, -e * np.where(ok, sw, 0.0)[:, None]

    def join(xc, xk):
        """(C, 9): each camera's pose entries and those of its calibration variable."""
        return np.concatenate([xc, xk[kmap]], 1)

    R, t, P, Kv = R_in.copy(), t_in.copy(), P_in.copy(), K0.copy()
    err0 = err = error(R, t, Kv, P)
    lam = 1e-5
    iters = trials = pcg_total = cap_hits = 0
    margins, per_solve = [], []
    eye6, eye3 = np.eye(6), np.eye(3)
    if err > 0.0:
        while True:
            cur = err
            J9, Jp, b = linearize(R, t, Kv, P)
            xi0 = pose_local(R_in[c0], t_in[c0], R[c0], t[c0])
            dp0 = P[t0] - P_in[t0]
            dk0 = np.where(kvar[:, None], (Kv - K0)[:, :3], 0.0)
            Hpp = base._scatter(T, ft, np.einsum("nrk,nrl->nkl", Jp, Jp))
            rp = base._scatter(T, ft, np.einsum("nrk,nr->nk", Jp, b))
            Hpp[t0] += POINT_PRIOR_W * np.eye(3)
            rp[t0] += -dp0 * POINT_PRIOR_W
            H9 = cam_scatter(np.einsum("nra,nrb->nab", J9, J9))
            g9 = cam_scatter(np.einsum("nra,nr->na", J9, b))
            H9[c0, :6, :6] += prior_w * eye6
            g9[c0, :6] += -xi0 * prior_w
            W = np.einsum("nra,nrk->nak", J9, Jp)
            old_lin = 0.5 * (np.sum(b * b) + np.dot(dp0, dp0) * POINT_PRIOR_W + np.dot(xi0, xi0) * prior_w +
                             np.sum(dk0 * dk0) * kprior_w)
            for _ in range(INNER_MAX):
                trials += 1
                Hd = Hpp + lam * np.eye(3)
                Hd[~part] = np.eye(3)
                Minv, ok3 = _inv3(Hd)
                Minv[~part] = 0.0
                WM = np.einsum("nak,nkl->nal", W, Minv[ft])
                S9 = H9 - cam_scatter(np.einsum("nal,nbl->nab", WM, W))
                b9 = g9 - cam_scatter(np.einsum("nal,nl->na", WM, rp[ft]))
                S9[~modelled] = 0.0
                b9[~modelled] = 0.0
                # the diagonal blocks of the damped Schur complement and the reduced right-hand side
                Skk = var_scatter(S9[:, 6:, 6:]) + (kprior_w + lam) * eye3
                bk = var_scatter(b9[:, 6:]) - dk0 * kprior_w
                bc = b9[:, :6]
                good = ok3
                Pc, Pk, P9 = np.zeros((C, 6, 6)), np.zeros((NK, 3, 3)), np.zeros((C, 9, 9))
                if good:
                    try:
                        if shared_calib:
                            Scc = S9[modelled][:, :6, :6] + lam * eye6
                            np.linalg.cholesky(Scc)
                            np.linalg.cholesky(Skk)
                            Pc[modelled] = np.linalg.inv(Scc)
                            Pk[:] = np.linalg.inv(Skk)
                        else:
                            D9 = S9[modelled].copy()
                            D9[:, 6:, 6:] = Skk[modelled] - lam * eye3
                            D9 += lam * np.eye(9)
                            np.linalg.cholesky(D9)
                            P9[modelled] = np.linalg.inv(D9)
                    except np.linalg.LinAlgError:
                        good = False
                success = stop = False
                new_err = np.inf
                m = {"trial": trials, "lambda": lam}
                if good:
                    def matvec(pc6, pk3):
                        p9 = join(pc6, pk3)
                        u = np.einsum("nra,na->nr", J9, p9[fc])
                        s = base._scatter(T, ft, np.einsum("nrk,nr->nk", Jp, u))
                        y = np.einsum("tij,tj->ti", Minv, s)
                        v = np.einsum("nrk,nk->nr", Jp, y[ft])
                        w = np.einsum("cab,cb->ca", H9, p9) - cam_scatter(np.einsum("nra,nr->na", J9, v))
                        w[~modelled] = 0.0
                        qc = w[:, :6] + lam * pc6
                        qc[~modelled] = 0.0
                        qk = var_scatter(w[:, 6:]) + (kprior_w + lam) * pk3
                        qk[~kvar] = 0.0
                        return qc, qk

                    def precond(rc, rk):
                        if shared_calib:
                            return np.einsum("cab,cb->ca", Pc, rc), np.einsum("cab,cb->ca", Pk, rk)
                        z = np.einsum("cab,cb->ca", P9, np.concatenate([rc, rk], 1))
                        return z[:, :6], z[:, 6:]

                    def dot(ac, ak, bc_, bk_):
                        return np.dot(ac.reshape(-1), bc_.reshape(-1)) + np.dot(ak.reshape(-1), bk_.reshape(-1))

                    bk = np.where(kvar[:, None], bk, 0.0)
                    xc, xk = np.zeros((C, 6)), np.zeros((NK, 3))
                    rc, rk = bc.copy(), bk.copy()
                    zc, zk = precond(rc, rk)
                    pc6, pk3 = zc.copy(), zk.copy()
                    rz = dot(rc, rk, zc, zk)
                    rr = bb = dot(rc, rk, rc, rk)
                    k = 0
                    while np.isfinite(rr) and not np.sqrt(rr) <= pcg_rel_tol * np.sqrt(bb):
                        if k >= pcg_max_iter:
                            cap_hits += 1
                            break
                        qc, qk = matvec(pc6, pk3)
                        with np.errstate(all="ignore"):
                            alpha = rz / dot(pc6, pk3, qc, qk)
                            xc, xk = xc + alpha * pc6, xk + alpha * pk3
                            rc, rk = rc - alpha * qc, rk - alpha * qk
                            zc, zk = precond(rc, rk)
                            rz_new = dot(rc, rk, zc, zk)
                            rr = dot(rc, rk, rc, rk)
                            pc6, pk3 = zc + (rz_new / rz) * pc6, zk + (rz_new / rz) * pk3
                        rz = rz_new
                        k += 1
                    pcg_total += k
                    per_solve.append(k)
                    x9 = join(xc, xk)
                    u = np.einsum("nra,na->nr", J9, x9[fc])
                    s = base._scatter(T, ft, np.einsum("nrk,nr->nk", Jp, u))
                    dp = np.einsum("tij,tj->ti", Minv, rp - s)
                    res = u + np.einsum("nrk,nk->nr", Jp, dp[ft]) - b
                    new_lin = 0.5 * (np.sum(res * res) + np.sum((dp[t0] + dp0) ** 2) * POINT_PRIOR_W +
                                     np.sum((xc[c0] + xi0) ** 2) * prior_w +
                                     np.sum((xk + dk0)[kvar] ** 2) * kprior_w)
                    Rn, tn = R.copy(), t.copy()
                    Rn[modelled], tn[modelled] = pose_retract(R[modelled], t[modelled], xc[modelled])
                    Kn = Kv.copy()
                    Kn[kvar, :3] = Kv[kvar, :3] + xk[kvar]
                    Pn = P.copy()
                    Pn[part] = P[part] + dp[part]
                    lin_change = old_lin - new_lin
                    m["lin_change"] = lin_change
                    if lin_change >= 0:
                        new_err = error(Rn, tn, Kn, Pn)
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
                    R, t, Kv, P, err = Rn, tn, Kn, Pn, new_err
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

    calib_out = K_in.copy()
    calib_out[modelled] = Kv[kmap[mod_idx]]
    # filter_landmarks, with the refined, distorted model
    keep = part.copy()
    if np.isfinite(reproj_error_thresh):
        mi = np.nonzero(mflag & part[mtrk])[0]
        ci = np.clip(img[mi], 0, C - 1)
        pc, pr, ok = project_k(R[ci], t[ci], calib_out[ci], P[mtrk[mi]])
        e = np.linalg.norm(pr - uv[mi], axis=1)
        bad = ~(camok[mi] & ok & (e < reproj_error_thresh))
        keep[np.unique(mtrk[mi][bad])] = False
    cam_keep = np.zeros(C, np.uint8)
    cam_keep[img[usable & keep[mtrk]]] = 1
    dff = np.abs(calib_out[modelled, 0] - K_in[modelled, 0]) / np.abs(K_in[modelled, 0])
    stats = np.array([err0, err, iters, trials, pcg_total, cap_hits, modelled.sum(), part.sum(), keep.sum(), 0.0,
                      kvar.sum(), dff.max()])
    keys = ("fidelity", "stop", "relative", "absolute")
    min_margin = min([v for m in margins for k, v in m.items() if k in keys], default=np.inf)
    return GlobalBaCalibRef(R, t, P, keep.astype(np.uint8), cam_keep, stats, calib_out, margins, float(min_margin),
                            per_solve)


# ------------------------------------------------------------------ scenes: global_ba_ref's, seen by a distorted camera
def distort_scene(s, k1=TRUE_K1, k2=TRUE_K2, f_off=F_OFF):
    """A global_ba_ref scene with its ground truth re-projected by a camera with radial distortion (k1, k2), the
    measurement noise and outliers kept as they are, and the initial calibration f off by f_off, k1 = k2 = 0.
    Adds `calib` (C, 5), `gt_calib` and drops nothing; measurements whose ground-truth projection does not exist (the
    edge entries on cameras without one) keep their pixel."""
    s = dict(s)
    C = len(s["intr"])
    img = np.clip(s["img"], 0, C - 1)
    trk = np.repeat(np.arange(len(s["offsets"]) - 1), np.diff(s["offsets"]))
    K3 = s["intr"]
    gt = np.concatenate([K3[:, :1], np.full((C, 1), k1), np.full((C, 1), k2), K3[:, 1:3]], 1)
    _, uv0, ok0 = base.project(s["gt_wRc"][img], s["gt_wtc"][img], K3[img], s["gt_point"][trk])
    _, uv1, ok1 = project_k(s["gt_wRc"][img], s["gt_wtc"][img], gt[img], s["gt_point"][trk])
    real = ok0 & ok1 & (np.abs(s["uv"] - uv0).max(1) < 100.0)  # the real measurements: noise and outliers stay < 100 px
    uv = s["uv"].copy()
    uv[real] = uv1[real] + (s["uv"][real] - uv0[real])
    s["uv"] = uv
    s["gt_calib"] = gt
    s["calib"] = np.concatenate([K3[:, :1] * f_off, np.zeros((C, 2)), K3[:, 1:3]], 1)
    s["distortion_px"] = float(np.abs(uv1[real] - uv0[real]).max())
    return s


def scene_small(seed=1):
    return distort_scene(base.scene_small(seed))


def scene_medium(seed=2):
    return distort_scene(base.scene_medium(seed))


def scene_medium_first_invalid(seed=2):
    """scene_medium with camera 0 invalid, so that the modelled camera of lowest index is camera 1, and with a principal
    point that differs from camera to camera by a fraction of a pixel: in shared mode camera 1's must reach every row."""
    s = scene_medium(seed)
    s["cam_valid"] = s["cam_valid"].copy()
    s["cam_valid"][0] = 0
    s["calib"] = s["calib"].copy()
    s["calib"][:, 3] += 0.125 * np.arange(len(s["calib"]))
    s["calib"][:, 4] -= 0.0625 * np.arange(len(s["calib"]))
    return s


def scene_dense(seed=3):
    return distort_scene(base.scene_dense(seed))


SCENES = {"small": scene_small, "medium": scene_medium, "medium0": scene_medium_first_invalid, "dense": scene_dense}


def call_args(s):
    """The positional arguments of global_ba_calib_ref from a scene dict."""
    return (s["offsets"], s["img"], s["uv"], s["point"], s["track_valid"], s["meas_valid"], s["wRc"], s["wtc"],
            s["calib"], s["cam_valid"])


def undistorted_args(s):
    """The positional arguments of global_ba_ref for the same scene with the distortion dropped from the model."""
    return (s["offsets"], s["img"], s["uv"], s["point"], s["track_valid"], s["meas_valid"], s["wRc"], s["wtc"],
            s["calib"][:, [0, 3, 4]], s["cam_valid"])


def calib_diff(Ka, Kb, cams):
    """Largest |df| / f and largest |dk1|, |dk2| (absolute) over the listed cameras."""
    d = np.abs(Ka[cams] - Kb[cams])
    return float((d[:, 0] / np.abs(Kb[cams, 0])).max()), float(d[:, 1:3].max())
