"""numpy restatement, in float64, of Shonan rotation averaging as include/gtsfm_hip.h states it for gtsfm_rotavg_shonan
(gtsfm/averaging/rotation/shonan.py on GTSAM's ShonanAveraging3): the edge filter and the largest component, the
Riemannian LM on St(p, 3)^n with its matrix-free PCG, the certificate, the lift along the minimum eigenvector and the
rounding. It shares no code with the kernels, and its certificate is a dense numpy.linalg.eigh of S, so it does not
depend on Lanczos. Also here: the alignment helper the comparisons use and the seeded scenes of the tests."""
import json
import os
from types import SimpleNamespace

import numpy as np

_M64 = (1 << 64) - 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rotation_averaging")

# the LM schedule (LevenbergMarquardtParams::CeresDefaults, as the header restates it)
LAMBDA_INITIAL = 1e-4
LAMBDA_FACTOR = 2.0
LAMBDA_UPPER = 1e32
LAMBDA_LOWER = 1e-16
MIN_MODEL_FIDELITY = 1e-3
ALPHA_MIN = 1e-2  # initializeWithDescent's smallest step

DEFAULTS = dict(p_min=5, p_max=30, optimality_threshold=-1e-4, grad_rel_tol=1e-10, max_iterations=100,
                pcg_rel_tol=1e-2, pcg_max_iter=200)


def sm_mix(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def hashed_uniform(seed: int, node: int, k: int) -> float:
    base = sm_mix((seed & _M64) ^ sm_mix(node))
    return 2.0 * ((sm_mix((base + k) & _M64) >> 11) * (1.0 / 9007199254740992.0)) - 1.0


# ---------------------------------------------------------------------------------------------- small helpers
def polar(A):
    """The polar factor A (A'A)^-1/2 of (..., p, 3) matrices: the retraction onto St(p, 3)."""
    w, V = np.linalg.eigh(np.swapaxes(A, -1, -2) @ A)
    return A @ (V * (1.0 / np.sqrt(w))[..., None, :]) @ np.swapaxes(V, -1, -2)


def closest_rotation(M):
    U, _, Vt = np.linalg.svd(M)
    d = np.sign(np.linalg.det(U @ Vt))
    D = np.zeros(M.shape)
    D[..., 0, 0] = D[..., 1, 1] = 1.0
    D[..., 2, 2] = d
    return U @ D @ Vt


def align(A, B, valid=None):
    """R* B_i, with R* the closest rotation to sum_i A_i B_i' over the valid cameras: B in A's frame."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    m = np.ones(len(A), bool) if valid is None else np.asarray(valid, bool)
    Rs = closest_rotation(np.einsum("nij,nkj->ik", A[m], B[m]))
    return Rs @ B


def angles_deg(A, B):
    """Angle of A_i' B_i from the chord |A_i - B_i|_F = 2 sqrt(2) sin(angle / 2): unlike arccos of the trace it
    resolves angles far below sqrt(eps)."""
    chord = np.linalg.norm(np.asarray(A, np.float64) - np.asarray(B, np.float64), axis=(1, 2))
    return np.degrees(2.0 * np.arcsin(np.clip(chord / (2.0 * np.sqrt(2.0)), 0.0, 1.0)))


def aligned_angles_deg(A, B, valid=None):
    m = np.ones(len(A), bool) if valid is None else np.asarray(valid, bool)
    return angles_deg(np.asarray(A)[m], align(A, B, m)[m])


def rot_xyz(x, y, z):
    """Rot3.RzRyRx(x, y, z) = Rz Ry Rx."""
    cx, sx, cy, sy, cz, sz = np.cos(x), np.sin(x), np.cos(y), np.sin(y), np.cos(z), np.sin(z)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def rodrigues(w):
    t = np.linalg.norm(w)
    if t < 1e-300:
        return np.eye(3)
    k = w / t
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


# ---------------------------------------------------------------------------------------------- section 1
def edges_from_two_view(pairs, i2Ri1, sigma=1.0):
    """(i1, i2) -> i2Ri1 gives the edge a = i2, b = i1, aRb = i2Ri1, kappa = 1 / sigma^2 (shonan.py:60-77)."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    return pairs[:, ::-1].copy(), np.asarray(i2Ri1, np.float64).reshape(-1, 3, 3), np.full(len(pairs), 1.0 / sigma ** 2)


def build_problem(edges, aRb, kappa, valid, n_img):
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    aRb = np.asarray(aRb, np.float64).reshape(-1, 3, 3)
    E = len(edges)
    kappa = np.ones(E) if kappa is None else np.asarray(kappa, np.float64)
    use = np.ones(E, bool) if valid is None else np.asarray(valid).astype(bool)
    a, b = edges[:, 0], edges[:, 1]
    use = use & (a >= 0) & (a < n_img) & (b >= 0) & (b < n_img) & (a != b) & np.isfinite(aRb).all((1, 2)) \
        & np.isfinite(kappa) & (kappa > 0)
    parent = list(range(n_img))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for e in np.nonzero(use)[0]:
        ra, rb = find(int(a[e])), find(int(b[e]))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    root = np.array([find(i) for i in range(n_img)])
    has_edge = np.zeros(n_img, bool)
    has_edge[a[use]] = True
    has_edge[b[use]] = True
    size = np.bincount(root[has_edge], minlength=n_img)
    best = int(np.argmax(size))  # first maximum: the component holding the lowest camera index
    keep = has_edge & (root == best) & (size[best] > 0)
    new = np.cumsum(keep) - 1
    use = use & keep[np.clip(a, 0, n_img - 1)]
    return SimpleNamespace(n=int(keep.sum()), a=new[a[use]], b=new[b[use]], R=aRb[use], k=kappa[use],
                           old=np.nonzero(keep)[0], keep=keep, n_img=n_img)


def apply_Q(P, Y):
    """Y Q for Y of shape (n, p, 3)."""
    out = np.zeros_like(Y)
    Ya, Yb = Y[P.a], Y[P.b]
    np.add.at(out, P.a, P.k[:, None, None] * (Ya - np.einsum("epk,eck->epc", Yb, P.R)))
    np.add.at(out, P.b, P.k[:, None, None] * (Yb - np.einsum("epk,ekc->epc", Ya, P.R)))
    return out


def degree(P):
    d = np.zeros(P.n)
    np.add.at(d, P.a, P.k)
    np.add.at(d, P.b, P.k)
    return d


def lambda_blocks(Y, G):
    L = np.einsum("npi,npj->nij", Y, G)
    return 0.5 * (L + np.swapaxes(L, 1, 2))


def dense_S(P, Lam):
    n = P.n
    S = np.zeros((3 * n, 3 * n))
    for e in range(len(P.a)):
        a, b, R, k = P.a[e], P.b[e], P.R[e], P.k[e]
        S[3 * a:3 * a + 3, 3 * a:3 * a + 3] += k * np.eye(3)
        S[3 * b:3 * b + 3, 3 * b:3 * b + 3] += k * np.eye(3)
        S[3 * b:3 * b + 3, 3 * a:3 * a + 3] -= k * R.T
        S[3 * a:3 * a + 3, 3 * b:3 * b + 3] -= k * R
    for i in range(n):
        S[3 * i:3 * i + 3, 3 * i:3 * i + 3] -= Lam[i]
    return S


# ---------------------------------------------------------------------------------------------- section 2
def _dot(a, b):
    return float(np.sum(a * b))


def optimise_level(P, Y, D, G0, o, counters):
    """Riemannian LM at one level. Returns Y, cost, status_not_finite."""
    G = apply_Q(P, Y)
    f = _dot(Y, G)
    lam, nu = LAMBDA_INITIAL, LAMBDA_FACTOR
    for _ in range(o["max_iterations"]):
        if not np.isfinite(f):
            return Y, f, True
        Lam = lambda_blocks(Y, G)
        g = 2.0 * (G - Y @ Lam)
        if np.sqrt(_dot(g, g)) <= o["grad_rel_tol"] * G0:
            break

        def A(V, lam, Lam=Lam, Y=Y):
            W = apply_Q(P, V) - V @ Lam
            sym = np.einsum("npi,npj->nij", Y, W)
            W = W - Y @ (0.5 * (sym + np.swapaxes(sym, 1, 2)))
            return 2.0 * W + lam * D[:, None, None] * V

        accepted = False
        while lam <= LAMBDA_UPPER:
            Minv = 1.0 / (D * (1.0 + lam))
            x = np.zeros_like(Y)
            r = -g
            z = r * Minv[:, None, None]
            p = z.copy()
            rz, bb = _dot(r, z), _dot(r, r)
            rr, k = bb, 0
            while not (np.sqrt(rr) <= o["pcg_rel_tol"] * np.sqrt(bb)):
                if k >= o["pcg_max_iter"]:
                    counters["cap_hits"] += 1
                    break
                q = A(p, lam)
                pq = _dot(p, q)
                k += 1
                if not (pq > 0.0):  # negative curvature: the preconditioned steepest descent step, or what there is
                    if k == 1:
                        x = p.copy()
                    break
                alpha = rz / pq
                x = x + alpha * p
                r = r - alpha * q
                z = r * Minv[:, None, None]
                rz_new = _dot(r, z)
                rr = _dot(r, r)
                p = z + (rz_new / rz) * p
                rz = rz_new
            counters["pcg"] += k
            q = A(x, lam)
            model = -_dot(g, x) - 0.5 * (_dot(x, q) - lam * _dot(x, D[:, None, None] * x))
            Yn = polar(Y + x)
            Gn = apply_Q(P, Yn)
            fn = _dot(Yn, Gn)
            if not np.isfinite(fn):
                return Y, fn, True
            rho = (f - fn) / model if model > 0.0 else -1.0
            if rho > MIN_MODEL_FIDELITY and fn < f:
                Y, G, f = Yn, Gn, fn
                lam = max(lam * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), LAMBDA_LOWER)
                nu = LAMBDA_FACTOR
                counters["outer"] += 1
                accepted = True
                break
            lam *= nu
            nu *= 2.0
        if not accepted:
            break
    return Y, f, False


def round_solution(Y):
    n, p, _ = Y.shape
    M = np.einsum("npi,nqi->pq", Y, Y)
    w, V = np.linalg.eigh(M)
    U = V[:, ::-1][:, :3]  # the three dominant left singular directions of the p x 3n matrix
    B = np.einsum("pi,npj->nij", U, Y)
    if np.sum(np.linalg.det(B) < 0) * 2 > n:
        B[:, 2, :] *= -1.0
    return closest_rotation(B)


def initial_rotation(seed, cam):
    A = np.array([hashed_uniform(seed, cam, k) for k in range(9)]).reshape(3, 3)
    R = polar(A)
    if np.linalg.det(R) < 0:
        R[:, 2] *= -1.0
    return R


def shonan(edges, aRb, kappa, valid, n_img, wRi_init=None, seed=0, lift_direction=None, **kw):
    """Returns wRi (n_img, 3, 3), rot_valid (n_img,) uint8, stats (12,) in the order of native.RA_STATS_FIELDS, and
    the last level's Y, Lambda and problem for the tests. lift_direction(theta, w, V) may pick another vector of a
    degenerate minimum eigenspace (default: eigh's first)."""
    o = dict(DEFAULTS)
    o.update(kw)
    P = build_problem(edges, aRb, kappa, valid, n_img)
    wRi = np.zeros((n_img, 3, 3))
    rot_valid = np.zeros(n_img, np.uint8)
    stats = np.zeros(12)
    if P.n == 0:
        stats[11] = 1
        return SimpleNamespace(wRi=wRi, rot_valid=rot_valid, stats=stats, P=P)
    p = o["p_min"]
    Y = np.zeros((P.n, p, 3))
    for j, i in enumerate(P.old):
        Y[j, :3] = initial_rotation(seed, int(i)) if wRi_init is None else np.asarray(wRi_init, np.float64)[i]
    Y = polar(Y)
    D = 2.0 * degree(P)
    G0 = np.sqrt(3.0 * np.sum(D * D))
    counters = dict(outer=0, pcg=0, cap_hits=0)
    f0 = _dot(Y, apply_Q(P, Y))
    status, theta = 2, 0.0
    while True:
        Y, f, bad = optimise_level(P, Y, D, G0, o, counters)
        if bad:
            status = 3
            break
        Lam = lambda_blocks(Y, apply_Q(P, Y))
        w, V = np.linalg.eigh(dense_S(P, Lam))
        theta = float(w[0])
        if theta > o["optimality_threshold"]:
            status = 0
            break
        if p >= o["p_max"]:
            break
        v = (V[:, 0] if lift_direction is None else lift_direction(theta, w, V)).reshape(P.n, 1, 3)
        Yl = np.concatenate([Y, np.zeros((P.n, 1, 3))], axis=1)
        step = np.concatenate([np.zeros((P.n, p, 3)), v], axis=1)
        alpha = max(1024 * ALPHA_MIN, 0.1 / abs(theta))
        while True:
            Yt = polar(Yl + alpha * step)
            if _dot(Yt, apply_Q(P, Yt)) < f or alpha / 2 < ALPHA_MIN:
                break
            alpha /= 2
        Y, p = Yt, p + 1
    Rn = round_solution(Y) if status != 3 else np.zeros((P.n, 3, 3))
    if status != 3:
        wRi[P.old] = Rn
        rot_valid[P.old] = 1
    ffin = _dot(Y, apply_Q(P, Y))
    stats[:] = [f0, ffin, p, theta, 0.0, counters["outer"], counters["pcg"], counters["cap_hits"], 0, P.n if status != 3
                else 0, len(P.a), status]
    return SimpleNamespace(wRi=wRi, rot_valid=rot_valid, stats=stats, P=P, Y=Y)


def cost_so3(P, wRi):
    Y = np.asarray(wRi)[P.old]
    return _dot(Y, apply_Q(P, Y))


# ---------------------------------------------------------------------------------------------- cases
def golden(name):
    g = json.load(open(os.path.join(GOLDEN, name + ".json")))
    n = g.get("num_images", len(g["wRi_expected"]))
    edges, aRb, kappa = edges_from_two_view(g["edges"], g["i2Ri1"])
    return dict(n_img=n, edges=edges, aRb=aRb, kappa=kappa, expected=np.array(g["wRi_expected"], np.float64),
                expected_valid=np.ones(n, bool), pairs=np.array(g["edges"], np.int64), wRi_init=None, p_min=5)


def _case(n, pairs, i2Ri1, expected, expected_valid=None):
    edges, aRb, kappa = edges_from_two_view(pairs, i2Ri1)
    return dict(n_img=n, edges=edges, aRb=aRb, kappa=kappa, expected=np.array(expected, np.float64),
                expected_valid=np.ones(n, bool) if expected_valid is None else np.asarray(expected_valid, bool),
                pairs=np.asarray(pairs, np.int64), wRi_init=None, p_min=5)


def simple():
    """test_shonan.py test_simple."""
    r10, r21 = rot_xyz(0, np.deg2rad(30), 0), rot_xyz(0, 0, np.deg2rad(20))
    return _case(3, [(1, 0), (2, 1)], [r10, r21], [np.eye(3), r10, r10 @ r21])


def simple_with_prior():
    """test_simple_with_prior: one measurement and the prior (0, 2) -> 0R2 with covariance 1e-5 I, i.e. the edge
    a = 0, b = 2, kappa = 1 / 1e-5 (shonan.py:85-97)."""
    expected = [np.eye(3), rot_xyz(0, np.deg2rad(30), 0), rot_xyz(np.deg2rad(30), 0, 0)]
    c = _case(3, [(1, 0)], [expected[1]], expected)
    sigma = np.sqrt(np.average(np.diag(np.eye(6) * 1e-5), axis=None))
    c["edges"] = np.concatenate([c["edges"], [[0, 2]]])
    c["aRb"] = np.concatenate([c["aRb"], [expected[0].T @ expected[2]]])
    c["kappa"] = np.concatenate([c["kappa"], [1.0 / sigma ** 2]])
    return c


def nonconsecutive():
    """test_nonconsecutive_indices: camera 0 is orphaned, all rotations identity."""
    I = np.eye(3)
    return _case(4, [(1, 2), (2, 3), (1, 3)], [I, I, I], [I, I, I, I], [False, True, True, True])


def ring6():
    """The saddle: six cameras on a ring with identity measurements, started at Rz(60 k): zero gradient, cost 12,
    lambda_min(S) = -1 twice."""
    pairs = [(k, (k + 1) % 6) for k in range(6)]
    c = _case(6, pairs, [np.eye(3)] * 6, [np.eye(3)] * 6)
    c["wRi_init"] = np.array([rot_xyz(0, 0, np.deg2rad(60.0 * k)) for k in range(6)])
    c["p_min"] = 3
    return c


def seeded_scene(n, seed, density=0.5, noise_deg=2.0, extra_component=0):
    """n cameras with random rotations, about density of the pairs as (i1, i2) edges with i2Ri1 = wRi2' wRi1 times a
    rotation of about noise_deg; extra_component more cameras form a second, smaller component (a chain)."""
    rng = np.random.default_rng(seed)
    wRi = np.array([rodrigues(rng.normal(size=3)) for _ in range(n + extra_component)])
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n) if rng.random() < density]
    for k in range(n - 1):  # a spanning chain keeps the main component connected
        if (k, k + 1) not in pairs:
            pairs.append((k, k + 1))
    pairs += [(n + k, n + k + 1) for k in range(extra_component - 1)]
    if extra_component:
        pairs.append((n, n + extra_component - 1))
    return _noisy_case(wRi, pairs, noise_deg, rng, n)


def _noisy_case(wRi, pairs, noise_deg, rng, n_main):
    rel = [wRi[j].T @ wRi[i] @ rodrigues(np.deg2rad(noise_deg) * rng.normal(size=3) / np.sqrt(3.0)) for i, j in pairs]
    valid = np.arange(len(wRi)) < n_main
    return _case(len(wRi), pairs, rel, wRi, valid)


def hub_scene(n=300, seed=3, noise_deg=2.0):
    """Camera 0 joined to all others, the rest a sparse ring: camera 0's row has n - 1 half-edges."""
    rng = np.random.default_rng(seed)
    wRi = np.array([rodrigues(rng.normal(size=3)) for _ in range(n)])
    pairs = [(0, k) for k in range(1, n)] + [(k, k + 1) for k in range(1, n - 1)] + [(1, n - 1)]
    return _noisy_case(wRi, pairs, noise_deg, rng, n)


def run_case(c, **kw):
    kw.setdefault("p_min", c["p_min"])
    return shonan(c["edges"], c["aRb"], c["kappa"], c.get("edge_valid"), c["n_img"], c["wRi_init"], **kw)
