"""GPU tier: the (min, +) relaxation sweeps (dn_geodesic.hip) on the device -- the shared cases of geodesic_cases.py bit for bit against
scipy's Dijkstra on the same CSR arrays, one workload-shaped all-pairs run, and the evaluation lines of the functional-correspondence
experiment replayed on device tensors."""
import os

import numpy as np
import pytest
import torch

import geodesic_cases as gc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tier needs a ROCm device"
    from diffusion_net import _hip
    _hip._use_library_for_tests(None, False)
    if not os.path.exists(_hip.LIB_PATH):  # fresh checkout on the GPU box: compile the HIP sources
        import __graft_entry__
        __graft_entry__.build()
    lib = _hip.lib()                      # raises if libdiffnet_hip.so is missing: no fallback
    assert lib.dn_minplus_node_tile() >= 1
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", ["icosphere", "planar"])
@pytest.mark.parametrize("n_src", [1, 63, 64, 65, 130])
def test_mesh_graphs(dev, name, n_src):
    gc.run_graph(dev, name, n_src)


@pytest.mark.parametrize("sweeps_per_check", [8, 1, 7])
def test_path(dev, sweeps_per_check):
    gc.run_path(dev, sweeps_per_check)


def test_components_and_empty_rows(dev):
    gc.run_components(dev)


def test_zero_length_arcs(dev):
    gc.run_graph(dev, "zero_arcs", 5)


def test_hub_row(dev):
    gc.run_graph(dev, "star", 65)


def test_small_node_counts(dev):
    from diffusion_net import _hip
    tile = _hip.lib().dn_minplus_node_tile()
    for n in (1, 2, tile + 1):
        gc.run_small(dev, n)


@pytest.mark.parametrize("name", ["icosphere", "planar"])
def test_source_blocks_and_repeat(dev, name):
    gc.run_blocks(dev, name)


def test_error_returns(dev):
    gc.run_errors(dev)


def test_host_tensors_are_refused(dev):
    g = gc.graph("zero_arcs")
    from diffusion_net import ops
    with pytest.raises(RuntimeError):
        ops.minplus_distances(*gc.device_csr(g, "cpu"), torch.tensor([0]))


def test_all_pairs_at_workload_shape(dev, capsys):
    """Icosphere subdivided four times: 2 562 vertices, m = 3, 25 602 nodes, a 525 MB distance block.  All pairs through
    ``get_all_pairs_geodesic_distance``; the rows of 32 seeded sources, before symmetrisation, bit for bit against scipy on the same graph."""
    import scipy.sparse.csgraph
    from diffusion_net import geometry
    verts, faces = gc.icosphere(4)
    assert verts.shape[0] == 2562
    g = geometry.mesh_distance_graph(verts, faces, 3)
    assert g.shape[0] == 25602
    src = np.random.RandomState(31).choice(2562, size=32, replace=False)
    want = scipy.sparse.csgraph.dijkstra(g, directed=True, indices=src)[:, :2562]
    got = geometry.geodesic_distances(verts, faces, src, n_steiner=3)
    assert np.array_equal(got, want)
    full = geometry.get_all_pairs_geodesic_distance(verts, faces)
    assert "steiner" in capsys.readouterr().out
    assert full.shape == (2562, 2562) and np.isfinite(full).all() and np.array_equal(full, full.T) and not full.diagonal().any()
    assert np.array_equal(full[src], np.fmin(want, full[:, src].T)) and (full[src] <= want).all()
    assert 3.1 < full.max() < 3.2          # the diameter: a little above pi minus O(h^2)


def test_functional_correspondence_evaluation_lines(dev, tmp_path):
    """experiments/functional_correspondence/functional_correspondence.py:195-203 with synthetic shapes: device tensors in, a finite mean
    error out."""
    import diffusion_net
    from diffusion_net.utils import toNP
    verts1_np, faces1_np = gc.icosphere(2)              # shape 1: 162 vertices; shape 2: 140 vertices; 100 template vertices on each
    g = torch.Generator().manual_seed(41)
    verts1_orig = torch.tensor(verts1_np).float().to(dev)
    faces1 = torch.tensor(faces1_np).to(dev)
    V1, V2, n_fmap, T = verts1_orig.shape[0], 140, 30, 100
    evec1, evec2 = torch.randn(V1, 64, generator=g).to(dev), torch.randn(V2, 64, generator=g).to(dev)
    C_pred = torch.randn(1, n_fmap, n_fmap, generator=g).to(dev)
    vts1, vts2 = torch.randint(0, V1, (T,), generator=g).to(dev), torch.randint(0, V2, (T,), generator=g).to(dev)
    geodesic_cache_dir = str(tmp_path)

    evec1_on_2 = evec1[:, :n_fmap] @ C_pred.squeeze(0).transpose(0, 1)
    _, pred_labels2to1 = diffusion_net.geometry.find_knn(evec2[:, :n_fmap], evec1_on_2, k=1, method='cpu_kd')
    pred_labels2to1 = pred_labels2to1.squeeze(-1)
    vts2on1 = pred_labels2to1[vts2]
    errors = diffusion_net.geometry.geodesic_label_errors(verts1_orig, faces1, vts2on1, vts1, normalization='area',
                                                          geodesic_cache_dir=geodesic_cache_dir)
    geodesic_error = toNP(torch.mean(errors))

    assert isinstance(errors, torch.Tensor) and errors.dtype == torch.float64 and errors.shape == (T,)
    assert np.isfinite(geodesic_error) and 0.0 <= float(geodesic_error) < 1.0
    assert len(os.listdir(geodesic_cache_dir)) == 1 and "_steiner3_0.npz" in os.listdir(geodesic_cache_dir)[0]
