"""CPU tier (emulator build of the same kernel source, dn_geodesic.hip): the (min, +) relaxation sweeps through the C ABI and
``ops.minplus_distances`` on host buffers, bit for bit against scipy's Dijkstra on the same CSR arrays -- lane masks of ragged source
counts, node tiles, empty and hub rows, termination across host checks, source blocks, the error returns.  Bodies in geodesic_cases.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import geodesic_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "diffusion-net_amd", "csrc")
EMU_SO = os.path.join(ROOT, "tests", "emu", "_build", "libdiffnet_emu.so")
HOSTCXX = "/opt/rocm/lib/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not (os.path.exists(HOSTCXX) and shutil.which("make")), reason="host clang++/make not available")


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", CSRC, "-j8", "emu"], check=True, capture_output=True)
    from diffusion_net import _hip
    _hip._use_library_for_tests(EMU_SO, True)
    yield "cpu"
    _hip._use_library_for_tests(None, False)


@pytest.mark.parametrize("name", ["icosphere", "planar"])
@pytest.mark.parametrize("n_src", [1, 63, 64, 65, 130])
def test_mesh_graphs_on_emulator(emu, name, n_src):
    gc.run_graph(emu, name, n_src)


@pytest.mark.parametrize("sweeps_per_check", [8, 1, 7])
def test_path_on_emulator(emu, sweeps_per_check):
    gc.run_path(emu, sweeps_per_check)


def test_components_and_empty_rows_on_emulator(emu):
    gc.run_components(emu)


def test_zero_length_arcs_on_emulator(emu):
    gc.run_graph(emu, "zero_arcs", 5)


def test_hub_row_on_emulator(emu):
    gc.run_graph(emu, "star", 65)


def test_small_node_counts_on_emulator(emu):
    from diffusion_net import _hip
    tile = _hip.lib().dn_minplus_node_tile()
    assert tile >= 1
    for n in (1, 2, tile + 1):
        gc.run_small(emu, n)


@pytest.mark.parametrize("name", ["icosphere", "planar"])
def test_source_blocks_and_repeat_on_emulator(emu, name):
    gc.run_blocks(emu, name)


def test_error_returns_on_emulator(emu):
    gc.run_errors(emu)


def test_abi_on_emulator(emu):
    """The C entry itself: the changed word after sweeps that lower values and after one at the fixed point; the refused calls."""
    import torch
    from diffusion_net import _hip
    L = _hip.lib()
    g = gc.graph("path")
    rowptr, col, w = gc.device_csr(g, emu)
    dist = torch.full((300, 3), float("inf"), dtype=torch.float64)
    dist[0, 0] = dist[299, 1] = dist[7, 2] = 0.0
    changed = torch.full((1,), 5, dtype=torch.int32)
    args = (rowptr.data_ptr(), col.data_ptr(), w.data_ptr(), 300, dist.data_ptr(), 3)
    assert L.dn_minplus_sweeps_f64(*args, 0, changed.data_ptr(), None) == 0 and int(changed) == 0      # no sweep: the word is cleared
    assert L.dn_minplus_sweeps_f64(*args, 2, changed.data_ptr(), None) == 0 and int(changed) == 1
    assert L.dn_minplus_sweeps_f64(*args, 300, changed.data_ptr(), None) == 0 and int(changed) == 0
    assert np.array_equal(dist.t().numpy(), gc.oracle(g, np.array([0, 299, 7]), "path"))
    assert L.dn_minplus_sweeps_f64(*args, -1, changed.data_ptr(), None) != 0
    assert L.dn_minplus_sweeps_f64(*args, 1, None, None) != 0
    assert L.dn_minplus_sweeps_f64(rowptr.data_ptr(), col.data_ptr(), w.data_ptr(), -1, dist.data_ptr(), 3, 1, changed.data_ptr(), None) != 0
    assert L.dn_minplus_sweeps_f64(None, col.data_ptr(), w.data_ptr(), 300, dist.data_ptr(), 3, 1, changed.data_ptr(), None) != 0


def test_public_functions_take_the_kernel_route_on_emulator(emu, monkeypatch):
    """``geodesic_distances`` with the emulator bound goes through ``ops.minplus_distances`` and returns the bits of its scipy route."""
    import scipy.sparse.csgraph
    from diffusion_net import geometry, ops
    verts, faces = gc.planar_delaunay()
    src = np.array([3, 60, 3, 17])
    calls = []
    real = ops.minplus_distances
    monkeypatch.setattr(ops, "minplus_distances", lambda *a, **k: calls.append(1) or real(*a, **k))
    got = geometry.geodesic_distances(verts, faces, src, n_steiner=2)
    assert calls and got.dtype == np.float64 and got.shape == (4, 64)
    g = geometry.mesh_distance_graph(verts, faces, 2)
    assert np.array_equal(got, scipy.sparse.csgraph.dijkstra(g, directed=True, indices=src)[:, :64])
