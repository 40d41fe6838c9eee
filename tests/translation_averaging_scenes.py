"""Scenes shared by tests/test_translation_averaging.py and tests/test_translation_averaging_gpu.py."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
N_DIR = 2000
SEED = 0  # TranslationAveraging1DSFM's default


def golden(name):
    return json.load(open(os.path.join(GOLDEN, "translation_averaging", name + ".json")))


def sample_case(name):
    d = golden(name)
    out = dict(edges=np.array(d["edges"], np.int32), i2Ui1=np.array(d["i2Ui1"], np.float64),
               wRi=np.array(d["wRi"], np.float64))
    if "wti_expected" in d:
        out["wti"] = np.array(d["wti_expected"], np.float64)
    return out


def door(with_tracks):
    """Ground-truth rotations and the directions of all 66 pairs of the 12 door cameras, i2Ui1 = Unit3 of the
    translation of wTi2.between(wTi1); optionally the door's 2D tracks."""
    gt = json.load(open(os.path.join(GOLDEN, "lund_door", "gt.json")))
    R, t = np.array(gt["wRc"], np.float64), np.array(gt["wtc"], np.float64)
    n = len(R)
    edges = np.array([(i, j) for i in range(n) for j in range(i + 1, n)], np.int32)
    u = np.einsum("nji,nj->ni", R[edges[:, 1]], t[edges[:, 0]] - t[edges[:, 1]])
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    out = dict(edges=edges, i2Ui1=u, wRi=R, wti=t)
    if with_tracks:
        z = np.load(os.path.join(GOLDEN, "triangulation", "door_tracks2d.npz"))
        out.update(offsets=z["offsets"], img=z["image"], uv=z["uv"],
                   intr=np.tile(np.array(gt["fx_u0_v0"], np.float64), (n, 1)))
    return out


def mfas_graph(seed=7):
    """The seeded MFAS test graph: 300 nodes (260 cameras, 40 landmarks), 1,515 edges in shuffled order (not a
    multiple of 64, one of them switched off), directions from random node positions with 20 % replaced by random
    ones, 64 projection directions. Node 259 is isolated. Node 258 has in-edges only, for every direction: its five
    edges are stored as (other, 258) with direction +z, and every projection direction has d_z > 0."""
    rng = np.random.default_rng(seed)
    n_cam, n_land = 260, 40
    n = n_cam + n_land
    pos = rng.normal(size=(n, 3)) * 5
    keys = set()
    while len(keys) < 1390:
        a, b = rng.integers(0, 258, 2)
        if a != b and (b, a) not in keys:
            keys.add((int(a), int(b)))
    keys = sorted(keys)
    for s in range(n_land):
        for c in rng.choice(258, 3, replace=False):
            keys.append((int(c), n_cam + s))
    key = np.array(keys, np.int32)
    u = pos[key[:, 1]] - pos[key[:, 0]]
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    bad = rng.random(len(key)) < 0.2
    rnd = rng.normal(size=u.shape)
    u[bad] = rnd[bad] / np.linalg.norm(rnd[bad], axis=1, keepdims=True)
    extra = np.array([(int(c), 258) for c in rng.choice(258, 5, replace=False)], np.int32)
    key = np.concatenate([key, extra])
    u = np.concatenate([u, np.tile(np.array([0.0, 0.0, 1.0]), (5, 1))])
    order = rng.permutation(len(key))
    key, u = key[order], u[order]
    proj = rng.normal(size=(64, 3))
    proj[:, 2] = np.abs(proj[:, 2]) + 0.05
    proj /= np.linalg.norm(proj, axis=1, keepdims=True)
    valid = np.ones(len(key), np.uint8)
    valid[5] = 0
    return dict(key=np.ascontiguousarray(key), dir=np.ascontiguousarray(u), valid=valid, n_nodes=n, proj=proj,
                isolated=259, sink=258)
