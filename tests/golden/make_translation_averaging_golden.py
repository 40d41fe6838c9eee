"""Writes tests/golden/translation_averaging/*.json from the reference's own test data.

    python tests/golden/make_translation_averaging_golden.py /path/to/gtsfm

Read at generation time only, nothing of the reference is copied as code:
  tests/data/sample_poses.py is executed against the small numpy stand-in for gtsam below (Rot3.RzRyRx, Pose3.between,
  Unit3, and SFMdata.createPoses, the eight look-at poses on a circle of radius 40 at height 10 of GTSAM's Python
  examples), and convert_data_for_translation_averaging is applied to its CIRCLE_ALL_EDGES and PANORAMA cases: the
  numbers of wRi, i2Ui1 and the expected wti are stored.
  tests/averaging/translation/test_averaging_1dsfm.py is parsed, not run: the literals of Test1dsfmAllOutliers (five
  rotations, ten directions) and of test_select_tracks_for_averaging (track -> cameras table, expected camera lists).
"""
import ast
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


class Rot3:
    def __init__(self, R=None):
        self.R = np.eye(3) if R is None else np.asarray(R, np.float64)

    @staticmethod
    def RzRyRx(x, y, z):
        cx, sx, cy, sy, cz, sz = np.cos(x), np.sin(x), np.cos(y), np.sin(y), np.cos(z), np.sin(z)
        Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
        return Rot3(Rz @ Ry @ Rx)

    def matrix(self):
        return self.R


class Pose3:
    def __init__(self, R=None, t=None):
        self.R = R if R is not None else Rot3()
        self.t = np.zeros(3) if t is None else np.asarray(t, np.float64)

    def rotation(self):
        return self.R

    def translation(self):
        return self.t

    def between(self, other):  # self^-1 * other
        return Pose3(Rot3(self.R.R.T @ other.R.R), self.R.R.T @ (other.t - self.t))


class Unit3:
    def __init__(self, p):
        p = np.asarray(p, np.float64)
        n = np.linalg.norm(p)
        self.p = p / n if n > 0 else p

    def point3(self):
        return self.p


def _create_poses(K=None):
    poses = []
    for theta in np.linspace(0, 2 * np.pi, 8, endpoint=False):
        eye = np.array([40.0 * np.cos(theta), 40.0 * np.sin(theta), 10.0])
        z = -eye / np.linalg.norm(eye)
        x = np.cross(-np.array([0.0, 0.0, 1.0]), z)
        x /= np.linalg.norm(x)
        poses.append(Pose3(Rot3(np.stack([x, np.cross(z, x), z], 1)), eye))
    return poses


def _gtsam_stub():
    g = types.ModuleType("gtsam")
    g.Rot3, g.Pose3, g.Unit3 = Rot3, Pose3, Unit3
    g.Point3 = lambda x, y, z: np.array([x, y, z], np.float64)
    g.Cal3_S2 = lambda *a, **k: None
    ex = types.ModuleType("gtsam.examples")
    sfm = types.ModuleType("gtsam.examples.SFMdata")
    sfm.createPoses = _create_poses
    ex.SFMdata = sfm
    g.examples = ex
    return {"gtsam": g, "gtsam.examples": ex, "gtsam.examples.SFMdata": sfm}


def _sample_poses(root):
    saved = {k: sys.modules.get(k) for k in _gtsam_stub()}
    sys.modules.update(_gtsam_stub())
    try:
        ns = {"__name__": "sample_poses"}
        path = os.path.join(root, "tests", "data", "sample_poses.py")
        exec(compile(open(path).read(), path, "exec"), ns)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    out = {}
    for name, poses, rel in (("circle_all_edges", "CIRCLE_ALL_EDGES_GLOBAL_POSES", "CIRCLE_ALL_EDGES_RELATIVE_POSES"),
                             ("panorama", "PANORAMA_GLOBAL_POSES", "PANORAMA_RELATIVE_POSES")):
        wRi, i2Ui1, wti = ns["convert_data_for_translation_averaging"](ns[poses], ns[rel])
        out[name] = {"wRi": [r.matrix().tolist() for r in wRi], "edges": [list(k) for k in i2Ui1],
                     "i2Ui1": [u.point3().tolist() for u in i2Ui1.values()], "wti_expected": [list(t) for t in wti]}
    return out


def _literal(tree, func, name):
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name == func:
            for st in ast.walk(node):
                if isinstance(st, ast.Assign) and getattr(st.targets[0], "id", None) == name:
                    return eval(compile(ast.Expression(st.value), "<literal>", "eval"), {"np": np})
    raise KeyError((func, name))


def main(root: str) -> None:
    out_dir = os.path.join(HERE, "translation_averaging")
    os.makedirs(out_dir, exist_ok=True)
    for name, data in _sample_poses(root).items():
        json.dump(data, open(os.path.join(out_dir, name + ".json"), "w"), indent=1)
    path = os.path.join(root, "tests", "averaging", "translation", "test_averaging_1dsfm.py")
    tree = ast.parse(open(path).read())
    wRi = _literal(tree, "test_outlier_case_missing_value", "wRi_list")
    dirs = _literal(tree, "test_outlier_case_missing_value", "i2Ui1_input")
    json.dump({"wRi": [np.asarray(r).tolist() for r in wRi], "edges": [list(k) for k in dirs],
               "i2Ui1": [np.asarray(v).tolist() for v in dirs.values()]},
              open(os.path.join(out_dir, "all_outliers.json"), "w"), indent=1)
    table = _literal(tree, "test_select_tracks_for_averaging", "test_tracks_cameras")
    expected = _literal(tree, "test_select_tracks_for_averaging", "expected_track_cameras")
    json.dump({"valid_cameras": [0, 1, 2, 3], "measurements_per_camera": 3, "num_expected": 4,
               "track_cameras": [table[k] for k in sorted(table)], "expected_track_cameras": expected},
              open(os.path.join(out_dir, "select_tracks.json"), "w"), indent=1)
    print("wrote", sorted(os.listdir(out_dir)))


if __name__ == "__main__":
    main(sys.argv[1])
