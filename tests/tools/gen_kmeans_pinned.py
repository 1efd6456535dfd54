"""Writes tests/golden/kmeans_pinned.npz: what the REFERENCE's RecMap.cluster(method='kmeans') (recognition/recmap.py:85-122, sklearn's
KMeans underneath) writes into its label file on the scenes of tests/kmeans_ref.py::SCENES, and what sklearn's KMeans(init=array)
gives on the inits of kmeans_ref.GIVEN, which leave 1 and 3 clusters empty at the first step.

Needs the reference tree beside the repository (see oracle/gen_golden.py, whose import shims are used as they are) and
scikit-learn; never runs in the test suite.  The RecMap object is built with __new__ and the points are SimpleNamespaces; the label
file is written into a temporary directory and read back.  The fixture holds results only: sklearn's version, ids, labels,
iteration counts and centres.  (RecMap.cluster keeps labels only; n_iter_ and the centres of its scenes come from the same
KMeans(n_clusters=k, random_state=0) on the same array, whose labels are asserted to equal the file's.)

Before anything is written the restatement has to agree: ids, iteration counts, centres within 1e-10 and the labels under the rule
of tests/test_kmeans_cpu.py.  If it does not, change the scene's seed in kmeans_ref.SCENES, not the rule.

    python tests/tools/gen_kmeans_pinned.py
"""
from __future__ import annotations

import contextlib
import io
import sys
import tempfile
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from oracle import gen_golden as G  # noqa: E402
from tests import kmeans_ref as KR  # noqa: E402

GAP = 2.0 ** -40      # a label may differ where the margin is at most GAP * R^2 ...
CAP = 1e-3            # ... for at most this share of the points


def compare(tag, xyz, mode, got, labels, n_iter, centers):
    margin, r2 = KR.margins(xyz, mode, got["centers"])
    differ = np.flatnonzero(got["labels"] != labels)
    excused = differ[margin[differ] <= GAP * r2]
    dc = float(np.abs(got["centers"] - centers).max())
    print(f"  {tag}: n_iter {n_iter} / {got['n_iter']}, {differ.size} labels differ ({excused.size} within the gap), centres within {dc:.2e}, "
          f"smallest margin {margin.min() / r2:.2e} R^2, relocations {got['relocations']}")
    assert got["n_iter"] == n_iter and differ.size == excused.size and differ.size <= CAP * labels.size and dc <= 1e-10, tag


def main():
    G.import_reference()
    G._stub_missing_modules()
    import sklearn
    import sklearn.cluster
    import recognition.recmap as ref
    assert ref.KMeans is sklearn.cluster.KMeans and isinstance(ref.KMeans, type) and ref.KMeans.__module__.startswith("sklearn.cluster"), \
        "the reference must run the real sklearn.cluster.KMeans, not a stand-in"
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for tag, (n, k, seed, mode) in KR.SCENES.items():
        xyz = KR.scene(n, k, seed, mode)
        if tag == "obs16":
            ids, track_len = KR.track_scene(n, seed)
        else:
            ids, track_len = np.arange(1, n + 1, dtype=np.int64), np.full(n, KR.MIN_OBS)
        rm = ref.RecMap.__new__(ref.RecMap)
        rm.points3D = {int(p): SimpleNamespace(id=int(p), xyz=xyz[i].copy(), point2D_idxs=np.zeros(int(track_len[i]), dtype=np.int64))
                       for i, p in enumerate(ids.tolist())}
        with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
            fn = str(Path(tmp) / "labels.npy")
            rm.cluster(k=k, mode=mode, min_obs=KR.MIN_OBS, save_fn=fn, method="kmeans")
            data = np.load(fn, allow_pickle=True)[()]
            rm.load_segmentation(fn)
        keep = track_len >= KR.MIN_OBS
        assert np.array_equal(data["id"], ids[keep]) and np.array_equal(data["xyz"], xyz[keep])
        assert list(rm.p3d_seg.items()) == list(zip(data["id"].tolist(), data["label"].tolist()))
        with contextlib.redirect_stdout(io.StringIO()):
            model = sklearn.cluster.KMeans(n_clusters=k, random_state=0).fit(KR.apply_mode(xyz[keep], mode))
        assert np.array_equal(model.labels_, data["label"])
        out[tag + "_id"], out[tag + "_label"] = data["id"].astype(np.int64), data["label"].astype(np.int32)
        out[tag + "_n_iter"], out[tag + "_centers"] = np.array(model.n_iter_), model.cluster_centers_.astype(np.float64)
        seg_keys = list(rm.seg_p3d.keys())
        out[tag + "_seg_keys"] = np.array(seg_keys, dtype=np.int32)
        out[tag + "_seg_off"] = np.concatenate([[0], np.cumsum([len(rm.seg_p3d[s]) for s in seg_keys])]).astype(np.int32)
        out[tag + "_seg_ids"] = np.concatenate([np.asarray(rm.seg_p3d[s], dtype=np.int64) for s in seg_keys])
        compare(tag, xyz[keep], mode, KR.cluster_points(xyz[keep], k, mode=mode), out[tag + "_label"], int(model.n_iter_), out[tag + "_centers"])
    for tag, (n, k, seed, n_far) in KR.GIVEN.items():
        xyz, init = KR.given_init(n, k, seed, n_far)
        model = sklearn.cluster.KMeans(n_clusters=k, init=init, n_init=1, random_state=0).fit(xyz)
        out[tag + "_label"], out[tag + "_n_iter"] = model.labels_.astype(np.int32), np.array(model.n_iter_)
        out[tag + "_centers"] = model.cluster_centers_.astype(np.float64)
        got = KR.cluster_points(xyz, k, init=init)
        assert got["relocations"] >= n_far, (tag, got["relocations"])
        compare(tag, xyz, "xyz", got, out[tag + "_label"], int(model.n_iter_), out[tag + "_centers"])
    G.save("kmeans_pinned", **out)


if __name__ == "__main__":
    main()
