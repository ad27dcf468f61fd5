"""CPU tier, no device and no emulator: the Steiner-point graph against a builder written in plain loops, the two properties that follow
from its construction, ``get_all_pairs_geodesic_distance`` and its cache rules, the libigl route through a stub module, and
``geodesic_label_errors`` against the reference's formula (geometry.py:754-896)."""
import inspect
import os
import sys
import types

import numpy as np
import pytest
import scipy.sparse.csgraph
import torch

import geodesic_cases as gc
import diffusion_net
from diffusion_net import geometry, utils

STRIP = (np.array([[0.0, 0.0, 0.0], [0.7, 0.1, 0.0], [0.1, 0.6, 0.2], [0.8, 0.7, -0.1]]), np.array([[0, 1, 2], [2, 1, 3]]))
TETRA = (np.array([[0.0, 0.0, 0.0], [0.9, 0.0, 0.1], [0.2, 0.8, 0.0], [0.3, 0.3, 0.7]]), np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]]))


def _planar_in_unit_ball():
    verts, faces = gc.planar_delaunay()
    return verts - np.array([0.5, 0.5, 0.0]), faces


def _slack(n_nodes):
    """Two correct builders differ by a few ulp per arc and a path has fewer arcs than nodes: n_nodes * 2^-50 for coordinates in the unit ball."""
    return n_nodes * 2.0 ** -50


def _symmetrised(d):
    d = np.nan_to_num(d, nan=np.nan, posinf=np.nan, neginf=np.nan)
    d = np.fmin(d, d.T)
    top = np.nanmax(d)
    return np.nan_to_num(d, nan=top, posinf=top, neginf=top)


def test_the_reference_names_exist_with_its_signatures():
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(geometry.geodesic_label_errors) == ["target_verts", "target_faces", "pred_labels", "gt_labels", "normalization", "geodesic_cache_dir"]
    assert sig(geometry.get_all_pairs_geodesic_distance)[:3] == ["verts_np", "faces_np", "geodesic_cache_dir"]
    p = inspect.signature(geometry.get_all_pairs_geodesic_distance).parameters
    assert p["method"].default == "steiner" and p["n_steiner"].default == 3 and p["method"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(geometry.geodesic_label_errors).parameters["normalization"].default == "diameter"
    assert sig(geometry.geodesic_distances) == ["verts", "faces", "sources", "n_steiner"]
    assert sig(geometry.mesh_distance_graph) == ["verts", "faces", "n_steiner"]
    for name in ("geodesic_label_errors", "get_all_pairs_geodesic_distance", "geodesic_distances"):
        assert getattr(diffusion_net, name) is getattr(geometry, name)
    from diffusion_net import _hip, ops
    assert "dn_minplus_sweeps_f64" in _hip.EXPORTED_SYMBOLS and callable(ops.minplus_distances)


@pytest.mark.parametrize("mesh", [STRIP, TETRA], ids=["strip", "tetrahedron"])
@pytest.mark.parametrize("m", [0, 1, 3])
def test_graph_against_the_loop_builder(mesh, m):
    verts, faces = mesh
    g = geometry.mesh_distance_graph(verts, faces, n_steiner=m)
    arcs, position = gc.loop_graph(verts, faces, m)
    V = len(verts)
    n_edges = 5 if mesh is STRIP else 6
    assert g.shape == (V + n_edges * m,) * 2 and g.dtype == np.float64 and g.nnz == 2 * len(arcs)
    assert (abs(g - g.T)).nnz == 0
    # match the Steiner nodes of the two builders by position (the numbering of the graph under test is its own)
    g2, pos = geometry._steiner_graph(verts, faces, m)
    assert (g2 != g).nnz == 0 and pos.shape == (g.shape[0], 3) and pos.dtype == np.float64 and np.array_equal(pos[:V], verts)
    nodes = set()
    for pair in arcs:
        nodes |= set(pair)
    steiner = [nd for nd in nodes if nd[0] == "s"]
    assert len(steiner) == n_edges * m
    ident = {i: ("v", i) for i in range(V)}
    for i in range(V, g.shape[0]):
        gap, nd = min((float(np.abs(position(nd) - pos[i]).max()), nd) for nd in steiner)
        assert gap <= 2.0 ** -52, (i, gap)
        ident[i] = nd
    assert len(set(ident.values())) == g.shape[0]
    coo = g.tocoo()
    got = {frozenset((ident[i], ident[j])): w for i, j, w in zip(coo.row, coo.col, coo.data)}
    assert set(got) == set(arcs)
    for pair, w in got.items():
        assert abs(w - arcs[pair]) <= 4 * np.spacing(arcs[pair]), pair


def test_graph_of_degenerate_input():
    """Duplicate vertices give arcs of length zero; an unreferenced vertex an empty row; a non-manifold edge is one edge."""
    verts = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 1, 0], [0, 0, 1], [5, 5, 5], [0, 0, -1]])
    faces = np.array([[0, 1, 2], [0, 1, 4], [1, 0, 6], [2, 3, 4]])          # edge (0, 1) in three faces; vertices 2 and 3 coincide
    g = geometry.mesh_distance_graph(verts, faces, n_steiner=1)
    assert g.indptr[6] - g.indptr[5] == 0 and g.nnz == 2 * len(gc.loop_graph(verts, faces, 1)[0])
    row2 = slice(g.indptr[2], g.indptr[3])
    assert 3 not in g.indices[row2]                        # vertices 2 and 3 are joined through the Steiner node of their edge,
    assert (g.data[row2] == 0.0).sum() == 1                # by arcs of length zero
    d = geometry.geodesic_distances(verts, faces, [2], n_steiner=1)
    assert d[0, 3] == 0.0 and np.isinf(d[0, 5]) and np.isfinite(d[0, [0, 1, 4, 6]]).all()


def test_distances_are_upper_bounds_and_fall_with_m():
    verts, faces = _planar_in_unit_ball()
    euclid = np.sqrt(((verts[:, None, :] - verts[None, :, :]) ** 2).sum(-1))
    d = {m: geometry.geodesic_distances(verts, faces, None, n_steiner=m) for m in (0, 1, 3)}
    slack = {m: _slack(geometry.mesh_distance_graph(verts, faces, m).shape[0]) for m in d}
    for m in d:
        assert d[m].shape == (64, 64) and (d[m] >= euclid - slack[m]).all()
    s = slack[3]
    assert (d[3] <= d[1] + s).all() and (d[1] + s <= d[0] + 2 * s).all()
    excess = {m: float(np.mean((d[m] - euclid)[euclid > 0] / euclid[euclid > 0])) for m in d}
    assert excess[3] < excess[1] < excess[0] and excess[3] < 0.03


def test_all_pairs_against_the_loop_builder(capsys):
    verts, faces = gc.icosphere(2)
    assert verts.shape[0] == 162
    ref = gc.loop_graph_csr(verts, faces, 3)
    assert ref.shape[0] == 1602
    want = _symmetrised(scipy.sparse.csgraph.dijkstra(ref, directed=True, indices=np.arange(162))[:, :162])
    got = geometry.get_all_pairs_geodesic_distance(verts, faces)
    out = capsys.readouterr().out
    assert "steiner" in out and "n_steiner=3" in out and len(out.strip().splitlines()) == 1
    assert got.dtype == np.float64 and got.shape == (162, 162)
    assert np.array_equal(got, got.T) and not got.diagonal().any() and np.isfinite(got).all()
    assert np.abs(got - want).max() <= _slack(1602)


def test_steiner_cache_round_trip_and_buckets(tmp_path, monkeypatch, capsys):
    verts, faces = gc.icosphere(0)
    first = geometry.get_all_pairs_geodesic_distance(verts, faces, str(tmp_path), n_steiner=2)
    key = str(utils.hash_arrays((verts, faces)))
    assert os.listdir(tmp_path) == [key + "_steiner2_0.npz"]            # nothing approximate under the reference's name
    npz = np.load(tmp_path / (key + "_steiner2_0.npz"))
    assert sorted(npz.files) == ["dist", "faces", "method", "n_steiner", "verts"]
    assert str(npz["method"]) == "steiner" and int(npz["n_steiner"]) == 2
    assert np.array_equal(npz["dist"], first) and np.array_equal(npz["verts"], verts) and np.array_equal(npz["faces"], faces)
    capsys.readouterr()
    monkeypatch.setattr(geometry, "geodesic_distances", lambda *a, **k: pytest.fail("the cache was not used"))
    assert np.array_equal(geometry.get_all_pairs_geodesic_distance(verts, faces, str(tmp_path), n_steiner=2), first)
    assert capsys.readouterr().out == ""
    monkeypatch.undo()
    # another n_steiner is another file; another mesh with the same hash lands in bucket 1
    geometry.get_all_pairs_geodesic_distance(verts, faces, str(tmp_path), n_steiner=1)
    assert sorted(os.listdir(tmp_path)) == [key + "_steiner1_0.npz", key + "_steiner2_0.npz"]
    monkeypatch.setattr(utils, "hash_arrays", lambda arrs: key)
    verts_b = verts * 2.0
    second = geometry.get_all_pairs_geodesic_distance(verts_b, faces, str(tmp_path), n_steiner=2)
    assert sorted(os.listdir(tmp_path)) == [key + "_steiner1_0.npz", key + "_steiner2_0.npz", key + "_steiner2_1.npz"]
    assert np.array_equal(np.load(tmp_path / (key + "_steiner2_1.npz"))["verts"], verts_b)
    assert np.array_equal(geometry.get_all_pairs_geodesic_distance(verts_b, faces, str(tmp_path), n_steiner=2), second)
    assert np.array_equal(geometry.get_all_pairs_geodesic_distance(verts, faces, str(tmp_path), n_steiner=2), first)
    assert len(os.listdir(tmp_path)) == 3


def test_reference_cache_file_is_returned_verbatim(tmp_path, monkeypatch):
    verts, faces = gc.icosphere(0)
    key = str(utils.hash_arrays((verts, faces)))
    sentinel = np.arange(144, dtype=np.float64).reshape(12, 12)         # not symmetric: returned as it is
    other = verts + 1.0
    np.savez(tmp_path / (key + "_0.npz"), verts=other, faces=faces, dist=-sentinel)      # a colliding entry of another mesh in bucket 0
    np.savez(tmp_path / (key + "_1.npz"), verts=verts, faces=faces, dist=sentinel)
    monkeypatch.setattr(geometry, "geodesic_distances", lambda *a, **k: pytest.fail("a distance was computed"))
    for method in ("steiner", "exact"):
        assert np.array_equal(geometry.get_all_pairs_geodesic_distance(verts, faces, str(tmp_path), method=method), sentinel)
    errs = geometry.geodesic_label_errors(torch.tensor(verts), torch.tensor(faces), torch.tensor([1, 2]), torch.tensor([3, 5]),
                                          geodesic_cache_dir=str(tmp_path))
    assert np.array_equal(errs, sentinel[[1, 2], [3, 5]] / 143.0)
    assert sorted(os.listdir(tmp_path)) == [key + "_0.npz", key + "_1.npz"]


def _stub_igl(calls):
    igl = types.ModuleType("igl")

    def exact_geodesic(v, f, vs, vt):
        calls.append(int(vs[0, 0]))
        d = np.sqrt(((v[vt[:, 0]] - v[vs[0, 0]]) ** 2).sum(-1))
        if vs[0, 0] == 1:
            d[4] = np.inf          # a failed value, as the reference expects now and then
        return d
    igl.exact_geodesic = exact_geodesic
    return igl


def test_exact_method_with_a_stub_igl(tmp_path, monkeypatch, capsys):
    verts, faces = gc.icosphere(0)
    calls = []
    monkeypatch.setitem(sys.modules, "igl", _stub_igl(calls))
    monkeypatch.setattr(geometry, "geodesic_distances", lambda *a, **k: pytest.fail("the Steiner route ran"))
    got = geometry.get_all_pairs_geodesic_distance(verts, faces, str(tmp_path), method="exact")
    assert "exact" in capsys.readouterr().out and calls == list(range(12))
    euclid = np.sqrt(((verts[:, None, :] - verts[None, :, :]) ** 2).sum(-1))
    assert got.shape == (12, 12) and np.array_equal(got, got.T) and np.allclose(got, euclid, rtol=0, atol=1e-15)   # fmin repaired (1, 4)
    key = str(utils.hash_arrays((verts, faces)))
    assert os.listdir(tmp_path) == [key + "_0.npz"]                      # the reference's format and name
    npz = np.load(tmp_path / (key + "_0.npz"))
    assert sorted(npz.files) == ["dist", "faces", "verts"] and np.array_equal(npz["dist"], got)
    assert np.array_equal(geometry.get_all_pairs_geodesic_distance(verts, faces, str(tmp_path)), got) and len(calls) == 12


def test_exact_method_without_igl(monkeypatch):
    monkeypatch.setitem(sys.modules, "igl", None)
    with pytest.raises(ImportError, match=r"method='steiner'"):
        geometry.get_all_pairs_geodesic_distance(*gc.icosphere(0), method="exact")
    with pytest.raises(ValueError):
        geometry.get_all_pairs_geodesic_distance(*gc.icosphere(0), method="heat")


def test_label_errors_follow_the_reference_formula():
    verts, faces = gc.icosphere(1)
    dists = geometry.get_all_pairs_geodesic_distance(verts, faces)
    rng = np.random.RandomState(3)
    pred, gt = rng.randint(0, 42, size=50), rng.randint(0, 42, size=50)
    v32, f = torch.tensor(verts).float(), torch.tensor(faces)                # fp32 torch, as the script passes them
    d32 = geometry.get_all_pairs_geodesic_distance(v32.numpy(), faces)
    got = geometry.geodesic_label_errors(v32, f, torch.from_numpy(pred), torch.from_numpy(gt))
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (50,)
    assert np.array_equal(got, d32[pred, gt] / d32.max())
    got = geometry.geodesic_label_errors(v32, f, torch.from_numpy(pred), torch.from_numpy(gt), normalization="area")
    c = v32[f]
    area = (0.5 * torch.linalg.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]).norm(dim=-1)).sum()
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and tuple(got.shape) == (50,)
    assert torch.equal(got, torch.from_numpy(d32[pred, gt]) / torch.sqrt(area))
    assert np.isfinite(torch.mean(got).item())
    with pytest.raises(ValueError, match="unrecognized normalization"):
        geometry.geodesic_label_errors(v32, f, torch.from_numpy(pred), torch.from_numpy(gt), normalization="radius")


def test_disconnected_mesh_takes_the_largest_finite_value():
    verts = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 0, 0], [6, 0, 0], [5, 2, 0]])
    faces = np.array([[0, 1, 2], [3, 4, 5]])
    raw = geometry.geodesic_distances(verts, faces)
    assert np.isinf(raw[:3, 3:]).all() and np.isinf(raw[3:, :3]).all() and np.isfinite(raw[:3, :3]).all()
    d = geometry.get_all_pairs_geodesic_distance(verts, faces)
    top = d[3:, 3:].max()                                  # the longest edge of the larger triangle
    assert abs(top - np.sqrt(5.0)) < 1e-15 and d.max() == top and (d[:3, 3:] == top).all() and (d[3:, :3] == top).all() and d[0, 1] == 1.0
