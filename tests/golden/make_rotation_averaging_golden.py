"""Writes tests/golden/rotation_averaging/*.json from the reference's own test data.

    python tests/golden/make_rotation_averaging_golden.py /path/to/gtsfm

Read at generation time only, nothing of the reference is copied as code:
  tests/data/sample_poses.py is executed against the numpy stand-in for gtsam of make_translation_averaging_golden.py,
  and convert_data_for_rotation_averaging is applied to its CIRCLE_TWO_EDGES, CIRCLE_ALL_EDGES, LINE_LARGE_EDGES and
  PANORAMA cases: the (i1, i2) keys, the numbers of i2Ri1 and the expected wRi are stored.
  tests/data/reproducibility/inputs/relative_rotations_skydio32.pkl and global_rotations_post_shonan_skydio32.pkl hold
  gtsam.Rot3 objects whose pickled state is a boost text archive ending in nine numbers; a stand-in class parses them.
  The element order (row- or column-major) is decided on the pair of files by i2Ri1 ~ wRi2' wRi1: only one order fits.
"""
import json
import os
import pickle
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_translation_averaging_golden as ta  # noqa: E402

CASES = ("CIRCLE_TWO_EDGES", "CIRCLE_ALL_EDGES", "LINE_LARGE_EDGES", "PANORAMA")


def _sample_poses(root):
    stub = ta._gtsam_stub()
    saved = {k: sys.modules.get(k) for k in stub}
    sys.modules.update(stub)
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
    for case in CASES:
        i2Ri1, wRi = ns["convert_data_for_rotation_averaging"](ns[case + "_GLOBAL_POSES"], ns[case + "_RELATIVE_POSES"])
        out[case.lower()] = {"edges": [list(k) for k in i2Ri1], "i2Ri1": [r.matrix().tolist() for r in i2Ri1.values()],
                             "wRi_expected": [r.matrix().tolist() for r in wRi]}
    return out


class _ArchivedRot3:
    """gtsam.Rot3's pickle: state = (boost text archive,), whose last nine numbers are the matrix."""

    def __setstate__(self, state):
        text = state[0] if isinstance(state, tuple) else state
        self.nine = np.array([float(x) for x in text.split()[-9:]])


class _Unpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if module.startswith("gtsam") and name == "Rot3":
            return _ArchivedRot3
        return super().find_class(module, name)


def _skydio(root):
    d = os.path.join(root, "tests", "data", "reproducibility", "inputs")
    rel = _Unpickler(open(os.path.join(d, "relative_rotations_skydio32.pkl"), "rb")).load()
    glob = _Unpickler(open(os.path.join(d, "global_rotations_post_shonan_skydio32.pkl"), "rb")).load()
    # the global list has one entry per image (32, None where Shonan gave nothing); the relative rotations are keyed by
    # the consecutive indices 0..16 of the 17 cameras that have one, in ascending image order
    kept = [i for i, r in enumerate(glob) if r is not None]
    keys = [k for k, v in rel.items() if v is not None]
    assert sorted({i for k in keys for i in k}) == list(range(len(kept)))
    fits = {}
    for order in ("C", "F"):
        mat = lambda r: r.nine.reshape(3, 3, order=order)  # noqa: E731
        err = []
        for (i1, i2) in keys:
            d_ = mat(rel[(i1, i2)]).T @ (mat(glob[kept[i2]]).T @ mat(glob[kept[i1]]))
            err.append(np.degrees(np.arccos(np.clip((np.trace(d_) - 1) / 2, -1, 1))))
        fits[order] = float(np.median(err))
    order = min(fits, key=fits.get)
    print("skydio-32: median angle between i2Ri1 and wRi2' wRi1 in degrees, row-major %.3f, column-major %.3f -> %s" %
          (fits["C"], fits["F"], order))
    mat = lambda r: r.nine.reshape(3, 3, order=order)  # noqa: E731
    return {"num_images": len(kept), "image_indices": kept, "edges": [list(k) for k in keys],
            "i2Ri1": [mat(rel[k]).tolist() for k in keys], "wRi_expected": [mat(glob[i]).tolist() for i in kept],
            "element_order": order, "order_fit_median_deg": fits}


def main(root: str) -> None:
    out_dir = os.path.join(HERE, "rotation_averaging")
    os.makedirs(out_dir, exist_ok=True)
    for name, data in _sample_poses(root).items():
        json.dump(data, open(os.path.join(out_dir, name + ".json"), "w"), indent=1)
    json.dump(_skydio(root), open(os.path.join(out_dir, "skydio32.json"), "w"), indent=1)
    print("wrote", sorted(os.listdir(out_dir)))


if __name__ == "__main__":
    main(sys.argv[1])
